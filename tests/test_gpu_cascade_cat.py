"""GPU tests of lib/cascade.py's CASCADE_Cat on tests/golden/cascade_cat_small.npz (make_golden_cascade_cat.py: N = 2, channels [64,40,24,16] at 2^2, 4^2, 8^2, 16^2),
by the rules of tests/test_gpu_cascade.py:
  outputs     train mode, fp32: within the project's literal 1e-4 absolute of the reference's fp32 AND float64 runs;
  gradients   of L = sum_i <out_i, R_i> with respect to the deepest input, the shallowest skip, three attention-gate weights and ConvBlock3.conv.0.weight (the first conv
              that reads a concatenated row), against the reference's float64 gradient: 1e-5 * max(scale, 1e-3) + 1e-6;
  replays     two forward + backward runs are bit-identical;
  eval        eval mode within 1e-4 of the reference's fp32 and float64 eval outputs;
  bf16        every train-mode output's relative L2 distance to float64 within 1.5 x the distance of the reference under torch.autocast(bfloat16) (the fixture's
              bf16.cat.rel), and a finite gradient on every parameter.
PVT_CASCADE(num_classes=4, encoder='pvt_v2_b0', dual=False, aggregation='concatenation', pretrain=False) at 2 x 64^2 under Trainer(loss="mutation", clip=None,
weight_decay=1e-4) in its single-supervision form: the eager steps equal the capture() / replay() steps bit for bit (the concatenating gate inside a captured graph), the
loss decreases over 5 steps, VolumePredictor's labels are the argmax of the module's own eval forward.
Each case prints its distances (run with -s, lines starting with CCAT)."""
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
SEED, CH, K = 9, [64, 40, 24, 16], 4
PROBES = ("AG1.psi.0.weight", "AG1.W_g.0.weight", "AG3.W_x.0.weight", "ConvBlock3.conv.0.weight")
TAG = "cat"


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pn2
    pn2.load_library()
    yield
    pn2.set_compute_dtype("bf16")


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(os.path.join(HERE, "golden", "cascade_cat_small.npz")))


def _model(fp32=True):
    import pn2
    from lib.cascade import CASCADE_Cat
    from oracle import weights as W
    pn2.set_compute_dtype("fp32" if fp32 else "bf16")
    m = CASCADE_Cat(channels=CH)
    m.load_state_dict(W.make_state_dict(OrderedDict((k, tuple(v.shape)) for k, v in m.state_dict().items()), seed=SEED), strict=True)
    return m.to(dev).train()


def _run(m, z):
    ins = [torch.from_numpy(z[k]).to(dev).requires_grad_(True) for k in ("x", "s0", "s1", "s2")]
    outs = m(ins[0], ins[1:])
    g = torch.Generator().manual_seed(SEED + 1)
    Rs = [torch.randn(*o.shape, generator=g).to(dev) for o in outs]
    m.zero_grad()
    sum((o * r).sum() for o, r in zip(outs, Rs)).backward()
    torch.cuda.synchronize()
    P = dict(m.named_parameters())
    return [o.detach() for o in outs], {"gx": ins[0].grad, "gs2": ins[3].grad, **{"g." + k: P[k].grad.clone() for k in PROBES}}


def test_cascade_cat_fp32_against_reference(fixture):
    z = fixture
    m = _model()
    outs, grads = _run(m, z)
    assert len(outs) == 4
    for i, o in enumerate(outs):
        r32, r64 = z[f"{TAG}.out{i}"].astype(np.float64), z[f"f64.{TAG}.out{i}"]
        got = o.double().cpu().numpy()
        e32, e64 = float(np.abs(got - r32).max()), float(np.abs(got - r64).max())
        print(f"CCAT out{i}: |ours - ref32| {e32:.2e}, |ours - ref64| {e64:.2e}, the reference's own {float(np.abs(r32 - r64).max()):.2e}")
        assert got.shape == r64.shape and e32 <= 1e-4 and e64 <= 1e-4, (i, e32, e64)
    for k, gt in grads.items():
        r32, r64 = z[f"{TAG}.{k}"].astype(np.float64), z[f"f64.{TAG}.{k}"]
        got = gt.double().cpu().numpy().reshape(r64.shape)
        err, own, scale = float(np.abs(got - r64).max()), float(np.abs(r32 - r64).max()), float(np.abs(r64).max())
        print(f"CCAT {k}: |ours - ref64| {err:.2e}, the reference's own {own:.2e}, scale {scale:.2e}")
        assert err <= 1e-5 * max(scale, 1e-3) + 1e-6, (k, err, own, scale)
    outs2, grads2 = _run(m, z)          # (running statistics moved: the train-mode outputs do not depend on them)
    assert all(torch.equal(a, b) for a, b in zip(outs, outs2)) and all(torch.equal(grads[k], grads2[k]) for k in grads)


def test_cascade_cat_eval_against_reference(fixture):
    z = fixture
    m = _model().eval()
    ins = [torch.from_numpy(z[k]).to(dev) for k in ("x", "s0", "s1", "s2")]
    with torch.no_grad():
        outs = m(ins[0], ins[1:])
    assert len(outs) == 4
    for i, o in enumerate(outs):
        got = o.double().cpu().numpy()
        e32, e64 = float(np.abs(got - z[f"eval.{TAG}.out{i}"]).max()), float(np.abs(got - z[f"f64.eval.{TAG}.out{i}"]).max())
        print(f"CCAT eval out{i}: |ours - ref32| {e32:.2e}, |ours - ref64| {e64:.2e}")
        assert e32 <= 1e-4 and e64 <= 1e-4, (i, e32, e64)


def test_cascade_cat_bf16_against_autocast(fixture):
    z = fixture
    m = _model(fp32=False)
    outs, _ = _run(m, z)
    tb = z[f"bf16.{TAG}.rel"]
    ours = []
    for i, o in enumerate(outs):
        r64 = z[f"f64.{TAG}.out{i}"]
        ours.append(float(np.linalg.norm(o.double().cpu().numpy().ravel() - r64.ravel()) / np.linalg.norm(r64.ravel())))
    print(f"CCAT bf16 rel-L2 per output: ours {[f'{e:.4f}' for e in ours]}   torch-autocast {[f'{e:.4f}' for e in tb]}")
    for n, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    for e, t in zip(ours, tb):
        assert e <= 1.5 * float(t), (ours, list(tb))


# ---------------------------------------------------------------------------------------------- PVT_CASCADE(aggregation='concatenation')
def _net(seed=5):
    import pn2
    from lib.cascade_net import PVT_CASCADE
    from oracle import weights as W
    pn2.set_compute_dtype("bf16")
    m = PVT_CASCADE(num_classes=K, encoder="pvt_v2_b0", dual=False, aggregation="concatenation", pretrain=False)
    m.load_state_dict(W.make_state_dict(OrderedDict((k, tuple(v.shape)) for k, v in m.state_dict().items()), seed=seed), strict=True)
    m.backbone.reset_drop_path(0.0)
    return m.to(dev).train()


def _batch():
    g = torch.Generator().manual_seed(77)
    x = torch.randn(2, 1, 64, 64, generator=g)
    label = torch.randint(0, K, (2, 8, 8), generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2)          # blocky labels
    return x.to(dev), label.long().to(dev)


def _trainer(m):
    from pn2.trainer import Trainer
    tr = Trainer(m, lr=1e-3, clip=None, weight_decay=1e-4, loss="mutation", hot=m.hot_parameters(True))
    assert tr.single
    return tr


def test_pvt_cascade_cat_graph_replay_is_bit_identical():
    x, label = _batch()
    res = []
    for graph in (False, True):
        tr = _trainer(_net())
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


def test_pvt_cascade_cat_loss_decreases():
    x, label = _batch()
    tr = _trainer(_net())
    losses = []
    for _ in range(5):
        losses.append(float(tr.step(x, label)[0]))
    print("CCAT PVT_CASCADE(concatenation) losses", [f"{v:.4f}" for v in losses])
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]


def test_pvt_cascade_cat_volume_predictor_labels():
    import volevalref as VR
    from oracle import weights as W
    from pn2.infer import VolumePredictor
    m = _net()
    m.load_state_dict(VR.nontrivial_bn_stats(W.make_state_dict(OrderedDict((k, tuple(v.shape)) for k, v in m.state_dict().items()), seed=5), seed=17), strict=True)
    m = m.eval()
    image = torch.randn(4, 64, 64, generator=torch.Generator().manual_seed(33)).to(dev)
    with torch.no_grad():
        want = torch.cat([m(image[i:i + 2, None].contiguous())[-1].argmax(1) for i in (0, 2)]).to(torch.uint8)
    got = VolumePredictor(m, patch_size=(64, 64), batch_size=2).predict(image, "last")
    assert got.dtype == torch.uint8 and tuple(got.shape) == (4, 64, 64)
    assert torch.equal(got, want) and len(torch.unique(want)) > 1
