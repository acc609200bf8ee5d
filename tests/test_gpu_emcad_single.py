"""GPU tests of the single-supervision EMCADNet (dual=False): the CE + Dice loss kernels (pn2_seg_loss_fwd / _bwd) against float64 for every built class
count and supervision mode, their agreement with the dual kernels' foreground half, the model against the vectors of the imported reference, the Trainer path
with hipGraph replay, and the pvt_v2_b0 encoder."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import seglossref as R

pytestmark = pytest.mark.gpu
os.environ.setdefault("PN2_NO_PRETRAINED", "1")
dev = "cuda"


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pn2
    pn2.load_library()
    yield
    pn2.set_compute_dtype("bf16")


def relmax(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def rell2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-12))


# ------------------------------------------------------------------------------------------------ loss kernels
def _loss_case(N, K, H, W, mode, weights=(0.3, 0.7), seed=3, label=None):
    """seg_loss + backward on random maps against tests/seglossref.py in float64: loss within 1e-5 relative, every map's gradient within 2e-5 relmax (the bounds of
    test_mutation_loss_kernels_vs_reference_formula: same arithmetic, same scale); a map outside every subset has a gradient of exact zeros."""
    from pn2.loss import seg_loss
    g = torch.Generator().manual_seed(seed * 100 + K)
    maps = [(torch.randn(N, K, H, W, generator=g) * 1.5).to(dev).requires_grad_(True) for _ in range(4)]
    if label is None:
        label = torch.randint(0, K, (N, H, W), generator=g)
    loss = seg_loss(maps, label.to(dev), mode, weights)
    loss.backward()
    m64 = [m.detach().double().cpu().requires_grad_(True) for m in maps]
    ref = R.seg_loss_ref(m64, label, mode, weights)
    ref.backward()
    used = {i for s in R.subsets(mode) for i in s}
    err = abs(float(loss) - float(ref)) / abs(float(ref))
    gerr = [relmax(a.grad, b.grad) if i in used else float(a.grad.abs().max()) for i, (a, b) in enumerate(zip(maps, m64))]
    print(f"\nseg_loss K={K} {mode} {N}x{H}x{W}: loss rel err {err:.2e}, gradient relmax / |unused|max {' '.join(f'{v:.2e}' for v in gerr)}")
    assert err < 1e-5
    for i, (a, b) in enumerate(zip(maps, m64)):
        if i in used:
            assert gerr[i] < 2e-5, i
        else:
            assert b.grad is None and int(torch.count_nonzero(a.grad)) == 0, i


# 3 x 20 x 27 = 1620 pixels: 6 full blocks of 256 + a block of 84 = 5 full 16-lane rows + a row of 4 (tail block, partial DPP row, partial wave)
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("K", [2, 3, 4, 9])
def test_seg_loss_kernels_vs_float64(K, mode):
    _loss_case(3, K, 20, 27, mode)


@pytest.mark.parametrize("K", [5, 6, 7, 8])
def test_seg_loss_kernels_vs_float64_other_class_counts(K):
    _loss_case(3, K, 20, 27, "mutation")


def test_seg_loss_empty_target_class():
    """K = 4 with labels that never take class 3: Dice with an empty target class (T = 0, the intersect sum exactly 0)."""
    label = torch.randint(0, 3, (3, 20, 27), generator=torch.Generator().manual_seed(11))
    assert int((label == 3).sum()) == 0
    _loss_case(3, 4, 20, 27, "mutation", label=label)


def test_seg_loss_single_partial_row():
    """N * H * W = 16: one block, one DPP row, 240 idle lanes."""
    _loss_case(1, 9, 4, 4, "mutation")


def test_seg_loss_matches_dual_kernels_foreground_half():
    """K = 9: seg_loss(maps, 'mutation', (0.5, 0.7)) against mutation_loss(maps + bg, (0.5, 0.7, 0.0)) - the dual kernels with the BCE weight at 0 compute the same
    sums (separate reductions: no bit identity asked)."""
    from pn2.loss import seg_loss, mutation_loss
    g = torch.Generator().manual_seed(21)
    N, K, H, W = 3, 9, 20, 27
    fg = [(torch.randn(N, K, H, W, generator=g) * 1.5).to(dev) for _ in range(4)]
    bg = [(torch.randn(N, K, H, W, generator=g) * 1.5).to(dev).requires_grad_(True) for _ in range(4)]
    label = torch.randint(0, K, (N, H, W), generator=g).to(dev)
    bgm = torch.stack([(label != k).float() for k in range(K)], 1)
    a = [f.clone().requires_grad_(True) for f in fg]
    b = [f.clone().requires_grad_(True) for f in fg]
    la = seg_loss(a, label, "mutation", (0.5, 0.7)); la.backward()
    lb = mutation_loss(b + bg, label, bgm, (0.5, 0.7, 0.0)); lb.backward()
    assert abs(float(la) - float(lb)) <= 1e-6 * abs(float(lb)), (float(la), float(lb))
    for x, y in zip(a, b):
        assert relmax(x.grad, y.grad) <= 2e-6


def test_seg_loss_bad_arguments():
    """K = 1, K = 10 raise with the supported range; subsets = 0 and a bit above 15 come back with status -2 from the entry points (checked before any launch)."""
    from pn2 import capi
    from pn2.loss import seg_loss
    lib = capi.load()
    for K in (1, 10):
        maps = [torch.zeros(1, K, 4, 4, device=dev) for _ in range(4)]
        with pytest.raises(RuntimeError, match="2 <= K <= 9"):
            seg_loss(maps, torch.zeros(1, 4, 4, dtype=torch.long, device=dev))
    assert lib.pn2_seg_loss_width(1) == -1 and lib.pn2_seg_loss_width(10) == -1 and lib.pn2_seg_loss_width(9) == 15 * 19 + 9
    with pytest.raises(ValueError):
        seg_loss([torch.zeros(1, 4, 4, 4, device=dev)] * 4, torch.zeros(1, 4, 4, dtype=torch.long, device=dev), "powerset")
    K = 4
    maps = [torch.zeros(1, 4, 4, K, device=dev) for _ in range(4)]
    grads = [torch.full_like(m, 7.0) for m in maps]
    lab = torch.zeros(1, 4, 4, dtype=torch.long, device=dev)
    wd = lib.pn2_seg_loss_width(K)
    partial = torch.zeros(lib.pn2_mutation_loss_blocks(16), wd, device=dev); sums = torch.zeros(wd, device=dev); loss = torch.full((1,), 7.0, device=dev)
    PA = C.c_void_p * 4
    pm, pg = PA(*[m.data_ptr() for m in maps]), PA(*[m.data_ptr() for m in grads])
    P = lambda t: C.c_void_p(t.data_ptr())
    for subsets, k in ((0, K), (0x8000, K), (0x7FFF, 1), (0x7FFF, 10)):
        assert lib.pn2_seg_loss_fwd(pm, subsets, P(lab), 1, 16, k, 0.3, 0.7, P(partial), P(sums), P(loss), None) == -2
        assert lib.pn2_seg_loss_bwd(pm, pg, subsets, P(lab), 1, 16, k, 0.3, 0.7, P(sums), 1.0, None) == -2
    torch.cuda.synchronize()
    assert float(loss) == 7.0 and all(float(g.min()) == 7.0 for g in grads)          # nothing ran


# ------------------------------------------------------------------------------------------------ model
def _model(fp32=True, dual=False):
    import pn2
    from lib.networks import EMCADNet
    from oracle import weights as W
    pn2.set_compute_dtype("fp32" if fp32 else "bf16")
    m = EMCADNet(num_classes=9, kernel_sizes=[1, 3, 5], expansion_factor=2, dw_parallel=True, add=True, lgag_ks=3, activation="relu6", encoder="pvt_v2_b2",
                 pretrain=False, dual=dual)
    m.load_state_dict(W.make_state_dict(W.manifest_emcadnet(9) if dual else R.single_manifest(9), seed=5), strict=True)
    m.backbone.reset_drop_path(0.0)
    return m.to(dev).train()


@pytest.mark.parametrize("fp32", [True, False])
def test_single_emcadnet_forward_backward_vs_reference(fp32):
    """EMCADNet.forward (dual=False) + seg_loss('mutation', 0.3 / 0.7) + backward against the reference's float64 run, with the rules of
    test_emcadnet_forward_backward_vs_reference (fp32: 3 x the reference's own fp32-to-float64 distance; bf16: sanity band)."""
    from pn2.loss import seg_loss
    z = R.load_fixture()
    model = _model(fp32)
    x = torch.from_numpy(z["x"]).to(dev); label = torch.from_numpy(z["label"]).to(dev)
    outs = model(x, mode="train")
    assert len(outs) == 4 and all(tuple(o.shape) == (2, 9, 64, 64) for o in outs)
    loss = seg_loss(outs, label)
    loss.backward()
    names = dict(model.named_parameters())
    o64, o32 = R.fixture_outs(z, "f64."), R.fixture_outs(z, "")
    if fp32:
        for i, o in enumerate(outs):
            own = float((o32[i].double() - o64[i]).abs().max())
            assert float((o.detach().double().cpu() - o64[i]).abs().max()) <= max(1e-4, 3 * own), i
        assert abs(float(loss) - float(z["f64.loss.mutation"])) < max(1e-4, 3 * abs(float(z["loss.mutation"]) - float(z["f64.loss.mutation"])))
        probes = [k[len("f64.grawnorm."):] for k in z.files if k.startswith("f64.grawnorm.")]
        assert {"out_head4.weight", "out_head4.bias", "out_head1.weight", "out_head1.bias"} <= set(probes) and len(probes) == 25
        for name in probes:
            g = names[name].grad
            r64, r32 = float(z["f64.grawnorm." + name]), float(z["grawnorm." + name])
            assert abs(float(g.norm()) - r64) <= max(1e-2 * r64, 3 * abs(r32 - r64)) + 2e-6, name
            h64 = torch.from_numpy(z["f64.graw." + name]).double(); h32 = torch.from_numpy(z["graw." + name]).double()
            ours = g.detach().reshape(-1)[:h64.numel()].double().cpu()
            assert float((ours - h64).norm()) <= max(6e-2 * float(h64.norm()), 3 * float((h32 - h64).norm())) + 2e-6, name
    else:
        rels = [rell2(o, o64[i]) for i, o in enumerate(outs)]
        print("\nEMCADNet single bf16 64x64, rel-L2 of the 4 maps against the reference's float64 run:", " ".join(f"{v:.3f}" for v in rels))
        for i, v in enumerate(rels):
            assert v < 0.35, i
        assert abs(float(loss) - float(z["loss.mutation"])) < 5e-2 * float(z["loss.mutation"])


def test_trainer_single_supervision_step_matches_module_surface_and_adamw():
    """Trainer(loss="mutation") on the single-supervision model against the nn.Module surface + pn2.loss.seg_loss + torch.optim.AdamW (fp32), under the tolerances of
    test_trainer_mutation_step_matches_module_surface_and_adamw; a (label, bg_mask) pair is accepted."""
    from pn2.loss import seg_loss
    from pn2.trainer import Trainer
    z = R.load_fixture()
    x = torch.from_numpy(z["x"]).to(dev); label = torch.from_numpy(z["label"]).to(dev)
    bg = torch.stack([(label != k).float() for k in range(9)], 1)
    lr, wd = 1e-3, 1e-2
    ma = _model(True)
    hot_a = ma.hot_parameters(True)
    opt = torch.optim.AdamW(hot_a, lr=lr, weight_decay=wd)
    losses_a = []
    for _ in range(2):
        loss = seg_loss(ma(x, mode="train"), label)
        opt.zero_grad(); loss.backward()
        if not losses_a:
            g_a = [p.grad.clone() for p in hot_a]
        opt.step(); losses_a.append(float(loss))
    mb = _model(True)
    hot_b = mb.hot_parameters(True)
    tr = Trainer(mb, lr=lr, clip=None, weight_decay=wd, loss="mutation", hot=hot_b)
    assert tr.loss_weights == (0.3, 0.7)
    l1 = tr.forward_backward(x, label)
    torch.cuda.synchronize()
    assert abs(float(l1[0]) - losses_a[0]) < 1e-6 * abs(losses_a[0])
    for (n, _), pa, pb in zip([(n, p) for n, p in mb.named_parameters() if any(p is q for q in hot_b)], g_a, hot_b):
        gb = tr._grad_view(pb)
        scale = float(pa.abs().max())
        assert float((gb - pa).abs().max()) <= 1e-5 * max(scale, 1e-3) + 1e-6, n
    tr.optimizer_step()
    l2 = tr.step(x, (label, bg))
    torch.cuda.synchronize()
    assert abs(float(l2[0]) - losses_a[1]) < 1e-5 * abs(losses_a[1])
    bad = tot = 0
    for pa, pb in zip(hot_a, hot_b):
        d = (pb.data - pa.data).abs()
        assert float(d.max()) <= 4.5 * lr
        bad += int((d > 0.05 * lr).sum()); tot += d.numel()
    assert bad <= 1e-2 * tot, (bad, tot)


def test_trainer_single_supervision_graph_replay_is_bit_identical():
    """capture() / replay(): three replays against the same three eager steps, loss and the flat gradient arena bit for bit (bf16, identical weights)."""
    from pn2.trainer import Trainer
    z = R.load_fixture()
    x = torch.from_numpy(z["x"]).to(dev); label = torch.from_numpy(z["label"]).to(dev)
    res = []
    for graph in (False, True):
        m = _model(False)
        tr = Trainer(m, lr=1e-3, clip=None, weight_decay=1e-2, loss="mutation", hot=m.hot_parameters(True))
        if graph:
            tr.capture(x, label, warmup=2)
        else:
            for _ in range(2):
                tr.step(x, label)
        seq = []
        for _ in range(3):
            out = tr.replay(x, label) if graph else tr.step(x, label)
            torch.cuda.synchronize()
            seq.append((out.clone(), tr.gflat.clone()))
        res.append((seq, tr.flat.clone()))
    for (la, ga), (lb, gb) in zip(res[0][0], res[1][0]):
        assert torch.isfinite(la).all() and torch.equal(la, lb) and torch.equal(ga, gb)
    assert torch.equal(res[0][1], res[1][1])


def test_trainer_deep_supervision_step_and_dual_refusal():
    from pn2.loss import seg_loss
    from pn2.trainer import Trainer
    z = R.load_fixture()
    x = torch.from_numpy(z["x"]).to(dev); label = torch.from_numpy(z["label"]).to(dev)
    want = float(seg_loss(_model(True)(x, mode="train"), label, "deep_supervision"))
    m = _model(True)
    tr = Trainer(m, lr=1e-3, clip=None, weight_decay=1e-2, loss="mutation", supervision="deep_supervision", hot=m.hot_parameters(True))
    got = tr.step(x, label)
    torch.cuda.synchronize()
    assert abs(float(got[0]) - want) <= 1e-6 * abs(want), (float(got[0]), want)
    # the reference's float64 value of the same loss, as in the model test
    assert abs(float(got[0]) - float(z["f64.loss.deep_supervision"])) < max(1e-4, 3 * abs(float(z["loss.deep_supervision"]) - float(z["f64.loss.deep_supervision"])))
    with pytest.raises(ValueError):
        Trainer(_model(True, dual=True), loss="mutation", supervision="deep_supervision")
    with pytest.raises(ValueError):
        Trainer(_model(True), loss="mutation", supervision="powerset")


def test_single_emcadnet_pvt_v2_b0_k4_bf16():
    """EMCADNet(encoder='pvt_v2_b0') (channels [256, 160, 64, 32]) at 2 x 64^2, K = 4, bf16: finite loss, finite gradients on every hot parameter, out_head1 trained."""
    import pn2
    from lib.networks import EMCADNet
    from pn2.loss import seg_loss
    pn2.set_compute_dtype("bf16")
    torch.manual_seed(5)
    m = EMCADNet(num_classes=4, kernel_sizes=[1, 3, 5], expansion_factor=2, activation="relu6", encoder="pvt_v2_b0", pretrain=False)
    m.backbone.reset_drop_path(0.0)
    m = m.to(dev).train()
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 1, 64, 64, generator=g).to(dev)
    label = torch.randint(0, 4, (2, 64, 64), generator=g).to(dev)
    outs = m(x, mode="train")
    assert len(outs) == 4 and all(tuple(o.shape) == (2, 4, 64, 64) for o in outs)
    loss = seg_loss(outs, label)
    loss.backward()
    assert bool(torch.isfinite(loss))
    for n, p in m.named_parameters():
        if any(p is q for q in m.hot_parameters(True)):
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    assert float(m.out_head1.weight.grad.abs().max()) > 0
