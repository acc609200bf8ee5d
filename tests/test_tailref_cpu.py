"""CPU checks of tests/tailref.py: the float64 references of the boundary-weight, structure-loss and Adam kernels agree with the oracle and with torch's own
optimizers, and the seeded inputs of tests/test_gpu_train_tail_kernels.py have the properties those tests rely on."""
import numpy as np
import pytest
import torch

import tailref as R


def test_structure_loss_ref_equals_oracle_float64():
    from oracle.pranet_oracle import structure_loss
    for name in ("p4n3_20x27", "soft_mask", "saturated", "p8n2_33x65"):
        fg, bg, mask = (x.double() for x in R.loss_case(name))
        ref = R.structure_loss_ref(list(fg), list(bg), mask)
        m4 = mask[:, None]
        want = torch.stack([structure_loss(fg[p][:, None], bg[p][:, None], m4, 1 - m4) for p in range(fg.shape[0])])
        assert float((ref["losses"] - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), name
        assert abs(float(ref["total"]) - float(want.sum())) <= 1e-12 * max(1.0, float(want.sum().abs())), name


def test_structure_loss_ref_gradient_scales_per_pair():
    """upstream / gscale reach the gradient as the chain rule says: pair p's maps carry gscale * upstream[p] * d losses[p]."""
    fg, bg, mask = (x.double() for x in R.loss_case("p4n3_20x27"))
    plain = R.structure_loss_ref(list(fg), list(bg), mask, grad=True)
    scaled = R.structure_loss_ref(list(fg), list(bg), mask, upstream=R.UPSTREAM, gscale=R.UPSTREAM_SCALE, grad=True)
    for p, u in enumerate(R.UPSTREAM):
        for a, b in ((plain["gfg"][p], scaled["gfg"][p]), (plain["gbg"][p], scaled["gbg"][p])):
            assert float((a * u * R.UPSTREAM_SCALE - b).abs().max()) <= 1e-15 * float(a.abs().max())
    assert int(torch.count_nonzero(scaled["gfg"][1])) == 0 and int(torch.count_nonzero(scaled["gbg"][1])) == 0


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_adam_ref_equals_torch_optim(wd):
    """5 steps of torch.optim.Adam (wd = 0) / AdamW on float64 tensors; the clamp is applied to the gradient beforehand, as the issue of the fused kernel is
    clamp-then-Adam."""
    p0, grads = R.adam_case(1023)
    clip, gscale = R.ADAM_CLIPS["clip"]
    hp = R.ADAM_HP
    w = torch.nn.Parameter(p0.double().clone())
    cls = torch.optim.AdamW if wd else torch.optim.Adam
    opt = cls([w], lr=hp["lr"], betas=(hp["b1"], hp["b2"]), eps=hp["eps"], weight_decay=wd)
    p, m, v = p0.double(), torch.zeros(1023, dtype=torch.float64), torch.zeros(1023, dtype=torch.float64)
    for t in range(1, R.ADAM_T + 1):
        w.grad = (grads[t - 1].double() * gscale).clamp_(-clip, clip)
        opt.step()
        p, g, m, v = R.adam_ref(p, grads[t - 1], m, v, t, hp["lr"], hp["b1"], hp["b2"], hp["eps"], clip, gscale, wd)
        st = opt.state[w]
        assert torch.equal(g, w.grad)
        assert float((p - w.detach()).abs().max()) <= 1e-12
        assert float((m - st["exp_avg"]).abs().max()) <= 1e-12 and float((v - st["exp_avg_sq"]).abs().max()) <= 1e-12


@pytest.mark.parametrize("ks", [1, 3, 31, 63])
def test_weights_ref_on_binary_mask_is_quantised(ks):
    w = R.weights_ref(R.blob_masks(3, 33, 65).double(), ks)
    k = (w - 1) / 5 * ks * ks
    assert float((k - k.round()).abs().max()) < 1e-9 and float(k.min()) >= 0 and float(k.max()) <= ks * ks
    assert len(torch.unique(k.round())) > 1 or ks == 1


def test_weight_inputs():
    for H, W in R.WEIGHT_SHAPES:
        for kind in R.WEIGHT_KINDS:
            m = R.weight_masks(kind, H, W)
            assert m.shape == (3, H, W) and m.dtype == torch.float32 and float(m.min()) >= 0 and float(m.max()) <= 1
            w = R.weights_ref(m.double(), 31)
            assert bool(torch.isfinite(w).all()) and float(w.min()) >= 1 and float(w.max()) <= 6
            if kind == "blob":      # three different masks, none empty, none full
                assert set(torch.unique(m).tolist()) == {0.0, 1.0}
                assert not torch.equal(m[0], m[1]) and not torch.equal(m[1], m[2]) and not torch.equal(m[0], m[2])
            if kind == "zeros":
                assert torch.equal(w, torch.ones_like(w))
            if kind == "soft":
                assert len(torch.unique(m)) > H * W
    for ks in R.WEIGHT_KS:
        assert bool(torch.isfinite(R.weights_ref(R.weight_masks("soft", 33, 65).double(), ks)).all())
    assert torch.equal(R.weights_ref(R.weight_masks("soft", 33, 65).double(), 1), torch.ones(3, 33, 65, dtype=torch.float64))


@pytest.mark.parametrize("name", list(R.LOSS_CASES))
def test_loss_inputs(name):
    P, N, H, W, variant = R.LOSS_CASES[name]
    fg, bg, mask = R.loss_case(name)
    assert fg.shape == (P, N, H, W) and bg.shape == (P, N, H, W) and mask.shape == (N, H, W)
    for dt in (torch.float64, torch.float32):
        ref = R.structure_loss_ref(list(fg.to(dt)), list(bg.to(dt)), mask.to(dt), grad=True)
        for k in ("losses", "total", "sums", "wsum"):
            assert bool(torch.isfinite(ref[k]).all()), (k, dt)
        for x in ref["gfg"] + ref["gbg"]:
            assert bool(torch.isfinite(x).all()), dt
        assert float(ref["wsum"].min()) > 0
        assert float((ref["sums"][..., 3] - ref["sums"][..., 2] + 1).min()) > 0          # the Dice denominator U - I + 1
    if variant == "saturated":
        sat = fg.abs() >= 40
        assert abs(float(sat.float().mean()) - 0.25) < 0.01
        tgt = (2 * mask - 1)[None].expand_as(fg)
        for mag in (40.0, 100.0):
            for agree in (1.0, -1.0):
                assert int(((fg == mag * agree * tgt) & sat).sum()) > 0 and int(((bg == -mag * agree * tgt) & sat).sum()) > 0
    if variant == "const_masks":
        assert float(mask[1].max()) == 0.0 and float(mask[2].min()) == 1.0 and 0 < float(mask[0].mean()) < 1
    if variant == "soft_mask":
        assert len(torch.unique(mask)) > N * H * W // 2


def test_adam_inputs():
    for n in R.ADAM_N:
        p0, grads = R.adam_case(n)
        assert p0.shape == (n,) and grads.shape == (R.ADAM_T, n)
        if n == 0:
            continue
        for name, (clip, gscale) in R.ADAM_CLIPS.items():
            hit = (grads * gscale).abs() > clip
            if name == "clip":
                assert bool(hit.any()) and not bool(hit.all()), n
            else:
                assert not bool(hit.any())
            for wd in R.ADAM_WD:
                hp = {k: R.f32(x) for k, x in R.ADAM_HP.items()}
                p, m, v = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
                for t in range(1, R.ADAM_T + 1):
                    p, g, m, v = R.adam_ref(p, grads[t - 1], m, v, t, hp["lr"], hp["b1"], hp["b2"], hp["eps"], R.f32(clip), R.f32(gscale), R.f32(wd))
                    assert all(bool(torch.isfinite(x).all()) for x in (p, g, m, v))


def test_bias_corr_emulation_and_decay_factor():
    """What the Adam bound is built from.  The first tick is exact (1 - b is exact in fp32 for b in [0.5, 1]); later ones carry the rounding of b^t, magnified
    by 1 / (1 - b^t).  The decay factor 1 - lr * wd is the same fp32 number whether the product is rounded first or not (the kernel may contract it)."""
    for b in (R.ADAM_HP["b1"], R.ADAM_HP["b2"]):
        e = R.bias_corr_rel_err(b, R.ADAM_T)
        assert e[0] == 0.0 and max(e) > 0
        for t, x in enumerate(e, 1):          # at most t - 1 roundings of b^t (half an ulp of [0.5, 1) each) and one of the difference
            assert x <= (t - 1) * 2.0 ** -25 / (1.0 - float(np.float32(b)) ** t) + 2.0 ** -24, (b, t)
    lr, wd = np.float32(R.ADAM_HP["lr"]), np.float32(R.ADAM_WD[1])
    assert np.float32(np.float32(1) - np.float32(lr * wd)) == np.float32(1.0 - float(lr) * float(wd))
