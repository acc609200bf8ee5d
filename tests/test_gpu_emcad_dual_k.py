"""GPU tests of the dual EMCADNet at a class count other than 9: EMCADNet(num_classes=4, encoder='pvt_v2_b0', dual=True) at 2 x 64^2 - a Trainer(loss="mutation")
step against the module surface + pn2.loss.mutation_loss + torch.optim.AdamW, hipGraph replay, bf16, and the three supervision modes of the loss against the
values the reference recorded (tests/golden/emcad_dual_k4_64.npz)."""
import os

import pytest
import torch

import duallossref as D

pytestmark = pytest.mark.gpu
os.environ.setdefault("PN2_NO_PRETRAINED", "1")
dev = "cuda"
K = 4


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pn2
    pn2.load_library()
    yield
    pn2.set_compute_dtype("bf16")


def _model(fp32=True):
    import pn2
    from lib.networks import EMCADNet
    from oracle import weights as W
    pn2.set_compute_dtype("fp32" if fp32 else "bf16")
    m = EMCADNet(num_classes=K, kernel_sizes=[1, 3, 5], expansion_factor=2, dw_parallel=True, add=True, lgag_ks=3, activation="relu6", encoder="pvt_v2_b0",
                 pretrain=False, dual=True)
    m.load_state_dict(W.make_state_dict(D.manifest_b0(K), seed=5), strict=True)
    m.backbone.reset_drop_path(0.0)
    return m.to(dev).train()


def _batch():
    z = D.load_fixture()
    label = torch.from_numpy(z["label"]).long()
    return z, torch.from_numpy(z["x"]).to(dev), label.to(dev), D.bg_mask_of(label, K).to(dev)


def test_trainer_dual_k4_step_matches_module_surface_and_adamw():
    """Trainer(loss="mutation") on the K = 4 dual model against the nn.Module surface + pn2.loss.mutation_loss + torch.optim.AdamW (fp32), under the tolerances
    of test_trainer_single_supervision_step_matches_module_surface_and_adamw."""
    from pn2.loss import mutation_loss
    from pn2.trainer import Trainer
    _, x, label, bg = _batch()
    lr, wd = 1e-3, 1e-2
    ma = _model(True)
    hot_a = ma.hot_parameters(True)
    opt = torch.optim.AdamW(hot_a, lr=lr, weight_decay=wd)
    losses_a = []
    for _ in range(2):
        outs = ma(x, mode="train")
        assert len(outs) == 8 and all(tuple(o.shape) == (2, K, 64, 64) for o in outs)
        loss = mutation_loss(outs, label, bg)
        opt.zero_grad(); loss.backward()
        if not losses_a:
            g_a = [p.grad.clone() for p in hot_a]
        opt.step(); losses_a.append(float(loss))
    mb = _model(True)
    hot_b = mb.hot_parameters(True)
    tr = Trainer(mb, lr=lr, clip=None, weight_decay=wd, loss="mutation", hot=hot_b)
    assert tr.loss_weights == (0.5, 0.7, 0.3) and not tr.single
    l1 = tr.forward_backward(x, (label, bg))
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


def test_trainer_dual_k4_graph_replay_is_bit_identical():
    """capture() / replay(): three replays against the same three eager steps, loss, the flat gradient arena and the parameters bit for bit (bf16, identical
    weights)."""
    from pn2.trainer import Trainer
    _, x, label, bg = _batch()
    res = []
    for graph in (False, True):
        m = _model(False)
        tr = Trainer(m, lr=1e-3, clip=None, weight_decay=1e-2, loss="mutation", hot=m.hot_parameters(True))
        if graph:
            tr.capture(x, (label, bg), warmup=2)
        else:
            for _ in range(2):
                tr.step(x, (label, bg))
        seq = []
        for _ in range(3):
            out = tr.replay(x, (label, bg)) if graph else tr.step(x, (label, bg))
            torch.cuda.synchronize()
            seq.append((out.clone(), tr.gflat.clone()))
        res.append((seq, tr.flat.clone()))
    for (la, ga), (lb, gb) in zip(res[0][0], res[1][0]):
        assert torch.isfinite(la).all() and torch.equal(la, lb) and torch.equal(ga, gb)
    assert torch.equal(res[0][1], res[1][1])


def test_dual_emcadnet_k4_bf16():
    """bf16: finite loss, a finite gradient on every hot parameter, the foreground and background heads trained."""
    from pn2.loss import mutation_loss
    _, x, label, bg = _batch()
    m = _model(False)
    outs = m(x, mode="train")
    loss = mutation_loss(outs, label, bg)
    loss.backward()
    assert bool(torch.isfinite(loss))
    hot = m.hot_parameters(True)
    for n, p in m.named_parameters():
        if any(p is q for q in hot):
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    names = dict(m.named_parameters())
    assert float(names["decoder.ConvBlock1_fg.conv.weight"].grad.abs().max()) > 0 and float(names["decoder.ConvBlock1_bg.conv.weight"].grad.abs().max()) > 0


def test_dual_emcadnet_k4_losses_vs_reference():
    """fp32 model + mutation_loss in each supervision mode against the reference's float64 loss: within max(1e-4, 3 x the reference's own fp32-to-float64
    distance), the rule of the single-model test."""
    from pn2.loss import mutation_loss
    z, x, label, bg = _batch()
    m = _model(True)
    outs = [o.detach() for o in m(x, mode="train")]
    o64, o32 = D.fixture_outs(z, "f64."), D.fixture_outs(z, "")
    for i, o in enumerate(outs):
        own = float((o32[i].double() - o64[i]).abs().max())
        err = float((o.double().cpu() - o64[i]).abs().max())
        print(f"\nmap {i}: max |ours - f64 ref| {err:.2e}, the reference's own fp32 distance {own:.2e}")          # (figures only: the losses are what is gated)
    for mode in D.MODES:
        got, r64, r32 = float(mutation_loss(outs, label, bg, supervision=mode)), float(z["f64.loss." + mode]), float(z["loss." + mode])
        print(f"{mode}: loss {got:.7f}, reference float64 {r64:.7f}, fp32 {r32:.7f}")
        assert abs(got - r64) <= max(1e-4, 3 * abs(r32 - r64)), mode
