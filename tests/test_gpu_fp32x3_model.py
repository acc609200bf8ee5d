"""fp32x3 at model level: the replayed bs = 32 step against the reference fixture (tests/golden/pranet_v2_bs32.npz) with the gates of the fp32fast tests,
the conv + BatchNorm + activation cases of tests/test_gpu_parity.py with fp32fast's 3e-5 relative-max gate, PVT_PraNet_V2 against
tests/golden/pvt_pranet_v2_96.npz, bit-identical replays, and mode switches fp32fast -> fp32x3 -> fp32fast on a live model and a Trainer."""
import os, sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
G = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, HERE); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "pranet-v2_amd"))
os.environ.setdefault("PN2_NO_PRETRAINED", "1")
import test_gpu_bs32 as B  # noqa: E402
from test_gpu_bs32 import z  # noqa: E402,F401  (the fixture)
import test_gpu_parity as PAR  # noqa: E402
import test_gpu_determinism as DET  # noqa: E402
import test_gpu_module_graph as MG  # noqa: E402
import test_gpu_pvt as PVT  # noqa: E402

dev = "cuda"


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pn2
    from pn2 import graph as GR
    pn2.load_library()
    yield
    pn2.set_compute_dtype("bf16")
    GR.set_module_graph(True)


def test_bs32_replayed_step_literal_tolerance(z):
    """Conditioned weights, the benchmarked batch, through the replayed hipGraph: |logit - reference fp32| <= 1e-4 and <= 1e-4 against float64, loss,
    BatchNorm buffers and gradient probes as test_bs32_replayed_step_fp32fast_literal_tolerance."""
    which = "cond"
    tr, model, maps, losses, bufs = B._replayed_step(z, which, "fp32x3")
    st, step = int(z["stride"]), int(z[f"{which}.image_step"])
    e32 = [float((maps[i][::step, ::st, ::st] - B.T(z[f"{which}.out{i}"])[:, 0]).abs().max()) for i in range(8)]
    e64 = [float((maps[i][::step, ::st, ::st] - B.T(z[f"{which}.f64.out{i}"])[:, 0]).abs().max()) for i in range(8)]
    print(f"[bs32 cond fp32x3, hipGraph replay] max |logit - ref fp32| {max(e32):.2e}   max |logit - ref f64| {max(e64):.2e}   (reference fp32 vs its f64: {float(z[which + '.own_abs'].max()):.2e})")
    assert max(e32) <= 1e-4, e32
    assert max(e64) <= 1e-4, e64
    assert np.abs(np.array(losses) - z[f"{which}.losses"]).max() < 2e-5, (losses, z[f"{which}.losses"])
    worst = max(float((bufs[k] - B.T(z[f"{which}.buf." + k])).abs().max()) for k in bufs)
    assert worst <= 1e-5, worst
    keys, ours, own = B._probes(z, which, tr, model)
    print(f"[bs32 cond fp32x3] gradient probes rel-L2 vs f64: median {np.median(ours):.2e} (reference fp32: {np.median(own):.2e}), worst {ours.max():.2e} at {keys[int(ours.argmax())]}")
    assert float(np.median(ours)) <= 1.5 * max(2e-6, float(np.median(own)))
    assert float(ours.max()) <= 2e-2, keys[int(ours.argmax())]


def test_bs32_replayed_step_random_init(z):
    """Random init: no further from float64 than max(1e-4, 1.5 x the reference's own fp32 run)."""
    which = "rand"
    tr, model, maps, losses, _ = B._replayed_step(z, which, "fp32x3")
    st, step = int(z["stride"]), int(z[f"{which}.image_step"])
    own = z[f"{which}.own_abs"]
    e64 = [float((maps[i][::step, ::st, ::st] - B.T(z[f"{which}.f64.out{i}"])[:, 0]).abs().max()) for i in range(8)]
    print(f"[bs32 rand fp32x3] max |logit - ref f64| per map {[f'{e:.1e}' for e in e64]}   reference fp32 vs its f64 {[f'{e:.1e}' for e in own]}")
    for e, o in zip(e64, own):
        assert e <= max(1e-4, 1.5 * float(o)), (e64, own)
    l64 = z[f"{which}.f64.losses"]
    assert np.abs(np.array(losses) - l64).max() <= max(1e-4, 1.5 * float(np.abs(z[f"{which}.losses"] - l64).max()))
    keys, ours, own_g = B._probes(z, which, tr, model)
    assert float(np.median(ours)) <= 1.5 * float(np.median(own_g)) or float(np.median(ours)) <= 2e-6


@pytest.mark.parametrize("cfg", PAR.CONVS)
def test_conv_bn_act_fwd_bwd(cfg):
    """test_gpu_parity.py's conv (+ BatchNorm) (+ ReLU) forward / backward cases in fp32x3, against float64 with fp32fast's 3e-5 relative-max gate"""
    from pn2.capi import F32X3
    from pn2.engine import Engine
    from pn2.graph import _seed_grad
    N, Cin, Cout, k, stride, pad, dil, H, Wd, bn, relu = cfg
    err, tol = PAR.relmax, 3e-5
    torch.manual_seed(1)
    conv = nn.Conv2d(Cin, Cout, k, stride, pad, dil, bias=False).to(dev)
    bnm = nn.BatchNorm2d(Cout).to(dev) if bn else None
    if bn:
        bnm.weight.data.uniform_(0.5, 1.5); bnm.bias.data.normal_(0, 0.2)
    x = torch.randn(N, Cin, H, Wd, device=dev)
    eng = Engine(F32X3, True, need_grad=True)
    a = eng.from_nchw(x, requires_grad=True)
    y = eng.conv_bn_act(a, conv, bnm, relu=relu)
    out = eng.to_nchw(y).clone()
    gy = torch.randn_like(out)
    _seed_grad(y, gy)
    eng.backward()
    gx = a.grad[..., :Cin].float().permute(0, 3, 1, 2)
    xc = x.double().cpu().requires_grad_(True)
    wc = conv.weight.detach().double().cpu().requires_grad_(True)
    r = F.conv2d(xc, wc, None, stride, pad, dil)
    if bn:
        g_ = bnm.weight.detach().double().cpu().requires_grad_(True); b_ = bnm.bias.detach().double().cpu().requires_grad_(True)
        r = F.batch_norm(r, None, None, g_, b_, True, 0.1, 1e-5)
    if relu:
        r = F.relu(r)
    r.backward(gy.double().cpu())
    assert err(out, r) < tol
    assert err(gx, xc.grad) < tol
    assert err(eng.pgrads.get(conv.weight), wc.grad) < tol
    if bn:
        assert err(eng.pgrads.get(bnm.weight), g_.grad) < tol
        assert err(eng.pgrads.get(bnm.bias), b_.grad) < tol


def test_pvt_pranet_v2_forward_backward_vs_reference():
    """PVT_PraNet_V2 (train mode, nn.Module + autograd) in fp32x3: outputs, loss and gradient probes within the fp32 gates of test_gpu_pvt.py"""
    import pn2
    from pn2.loss import structure_loss
    from oracle import weights as W
    zz = np.load(os.path.join(G, "pvt_pranet_v2_96.npz"))
    model = PVT._pvt_model(fp32=True)
    pn2.set_compute_dtype("fp32x3")
    x, mask = W.synthetic_batch(2, 96, seed=4321)
    xg, mg = x.to(dev), mask.to(dev)
    outs = model(xg)
    losses = [structure_loss(outs[i], outs[i + 4], mg, 1 - mg) for i in range(4)]
    loss = losses[3] + losses[2] + losses[1] + losses[0]
    loss.backward()
    names = dict(model.named_parameters())
    for i, o in enumerate(outs):
        ref64 = torch.from_numpy(zz[f"f64.out{i}"])
        own = float((torch.from_numpy(zz[f"out{i}"]).double() - ref64).abs().max())
        assert float((o.detach().double().cpu() - ref64).abs().max()) <= max(1e-4, 3 * own), i
    assert abs(float(loss) - float(zz["f64.losses"].sum())) < max(1e-4, 3 * abs(float(zz["loss"]) - float(zz["f64.losses"].sum())))
    n = 0
    for k in zz.files:
        if k.startswith("f64.grawnorm."):
            name = k[len("f64.grawnorm."):]
            g = names[name].grad
            r64, r32 = float(zz[k]), float(zz["grawnorm." + name])
            assert abs(float(g.norm()) - r64) <= max(2e-4 * r64, 3 * abs(r32 - r64)) + 1e-7, name
            n += 1
    assert n > 0


def test_captured_bs32_step_replays_bit_identically():
    """bench.py's Trainer capture / replay at 32 x 3 x 352 x 352 in fp32x3 with lr = 0: 20 replays, bit for bit."""
    DET._replays("fp32x3", 20)


def test_call_site_follows_fp32fast_fp32x3_fp32fast():
    """fp32fast -> fp32x3 -> fp32fast on one live model: each mode replays graphs captured in its own arithmetic, bit for bit what a model that only
    ever ran in that mode computes."""
    import pn2
    from pn2 import graph as GR
    from oracle import weights as W
    GR.set_module_graph(True)
    x, _ = W.synthetic_batch(2, 96, seed=7)
    x = x.to(dev)
    gs = [torch.randn(2, 1, 96, 96, device=dev, generator=torch.Generator(device=dev).manual_seed(i)) for i in range(8)]

    def calls(model, mode, n=5):
        pn2.set_compute_dtype(mode)
        for _ in range(n):
            model.zero_grad()
            outs = model(x)
            torch.autograd.backward(list(outs), gs)
        return [o.detach().clone() for o in outs], {n_: p.grad.detach().clone() for n_, p in model.named_parameters() if p.grad is not None}
    model = MG._model()
    rfast = calls(model, "fp32fast")
    rx3 = calls(model, "fp32x3")
    sites = next(iter(model.hot_parameters())).__dict__["_pn2_sites"]
    assert len(sites) == 2 and all(st.graph_f is not None for st in sites.values())
    assert MG._same(rx3, calls(MG._model(), "fp32x3"))
    assert not any(torch.equal(u, v) for u, v in zip(rx3[0], rfast[0]))          # the two modes are told apart
    assert MG._same(calls(model, "fp32fast", 2), rfast)


def test_trainer_keeps_fp32x3():
    """A Trainer built in fp32x3 keeps it when the process-wide mode changes afterwards (and one built in fp32fast keeps fp32fast)."""
    import pn2
    from pn2.trainer import Trainer
    from oracle import weights as W
    x, m = W.synthetic_batch(2, 96, seed=3)
    x, m = x.to(dev), m.to(dev)

    def run(mode, switch):
        pn2.set_compute_dtype(mode)
        tr = Trainer(MG._model(), lr=1e-4, clip=0.5)
        if switch:
            pn2.set_compute_dtype(switch)
        losses = [tr.step(x, m).clone() for _ in range(3)]
        torch.cuda.synchronize()
        return losses, tr.gflat.clone(), tr.last_outs.clone()
    for mode, other in (("fp32x3", "fp32fast"), ("fp32fast", "fp32x3")):
        ref, got = run(mode, None), run(mode, other)
        assert all(torch.equal(a, b) for a, b in zip(ref[0], got[0])), (mode, ref[0], got[0])
        assert torch.equal(ref[1], got[1]) and torch.equal(ref[2], got[2]), mode
    assert not torch.equal(run("fp32x3", None)[2], run("fp32fast", None)[2])
