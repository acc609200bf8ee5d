"""GPU tests of EMCADNet with the ResNet encoders (lib/resnet.py): the whole model against the imported reference's float64 run (tests/golden/emcad_resnet50_128.npz,
make_golden_emcad_resnet.py) under the gates of test_gpu_emcad_switches.py, the eval-mode forward behind the step, Trainer capture / replay, VolumePredictor, and the
geometry of resnet101 with the single-supervision heads."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
os.environ.setdefault("PN2_NO_PRETRAINED", "1")
import emcad_resnetref as R  # noqa: E402

dev = "cuda"


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pn2
    pn2.load_library()
    yield
    pn2.set_compute_dtype("bf16")


def _model(mode):
    import pn2
    pn2.set_compute_dtype(mode)
    m = R.build("resnet50")
    m.load_state_dict(R.state_dict(seed=5), strict=True)
    return m.to(dev).train()


def rell2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-12))


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_emcadnet_resnet50_forward_backward_vs_reference(mode):
    """The module surface (eager forward + mutation loss + backward) against the reference's float64 run with the gates and multipliers of
    test_gpu_emcad_switches.py::test_switch_models_forward_backward_vs_reference: fp32 within 3 x the reference's own fp32-to-float64 distance (floors 1e-4), bf16 in its
    sanity band; then the eval-mode forward on the running statistics that step left, under the same map gate."""
    from pn2.loss import mutation_loss
    z, x, label, bg = R.fixture()
    sub, sub_e = int(z["sub"]), int(z["sub_eval"])
    model = _model(mode)
    outs = model(x.to(dev), mode="train")
    assert len(outs) == 8
    loss = mutation_loss(outs, label.to(dev), bg.to(dev))
    loss.backward()
    names = dict(model.named_parameters())
    assert names["backbone.fc.weight"].grad is None and names["backbone.fc.bias"].grad is None
    band, rel = 3, 1e-4
    if mode != "bf16":
        for i, o in enumerate(outs):
            ref64 = torch.from_numpy(z[f"f64.out{i}"]).double()
            err, own = float((o.detach()[:, :, ::sub, ::sub].double().cpu() - ref64).abs().max()), float(z[f"own.out{i}"])
            print(f"\nresnet50 map {i}: |ours - f64| {err:.2e}, the reference's own {own:.2e}")
            assert err <= max(1e-4, 3 * own), i
        print(f"resnet50 loss: ours {float(loss.detach()):.8f}, float64 {float(z['f64.loss']):.8f}, the reference's fp32 {float(z['loss']):.8f}")
        assert abs(float(loss.detach()) - float(z["f64.loss"])) < max(1e-4, 3 * abs(float(z["loss"]) - float(z["f64.loss"])))
        probes = [k[len("f64.grawnorm."):] for k in z if k.startswith("f64.grawnorm.")]
        assert {"conv.0.weight", "backbone.conv1.weight", "backbone.layer1.0.conv1.weight", "backbone.layer1.0.conv2.weight", "backbone.layer1.0.conv3.weight",
                "backbone.layer1.0.downsample.0.weight", "backbone.layer2.0.downsample.0.weight", "backbone.layer4.0.conv2.weight", "backbone.layer4.2.bn3.weight",
                "decoder.mscb4.0.pconv1.0.weight", "decoder.mscb1.0.pconv2.0.weight"} <= set(probes)
        for pname in probes:
            g = names[pname].grad
            r64, r32 = float(z["f64.grawnorm." + pname]), float(z["grawnorm." + pname])
            h64 = torch.from_numpy(z["f64.graw." + pname]).double(); h32 = torch.from_numpy(z["graw." + pname]).double()
            ours = g.detach().reshape(-1)[:h64.numel()].double().cpu()
            print(f"resnet50 {pname}: norm off {abs(float(g.norm()) - r64):.2e} (own {abs(r32 - r64):.2e}, own.gerr {float(z['own.gerr.' + pname]):.2e}), "
                  f"head off {float((ours - h64).norm()):.2e} (own {float((h32 - h64).norm()):.2e})")
            assert abs(float(g.norm()) - r64) <= max(rel * r64, band * abs(r32 - r64), band * float(z["own.gerr." + pname])) + 2e-6, pname
            assert float((ours - h64).norm()) <= max(rel * float(h64.norm()), band * float((h32 - h64).norm())) + 2e-6, pname
    else:
        rels = [rell2(o.detach()[:, :, ::sub, ::sub], torch.from_numpy(z[f"f64.out{i}"])) for i, o in enumerate(outs)]
        print("\nresnet50 bf16, rel-L2 of the maps against the reference's float64 run:", " ".join(f"{v:.3f}" for v in rels))
        for i, v in enumerate(rels):
            assert v < 0.35, i
        assert abs(float(loss.detach()) - float(z["f64.loss"])) < 5e-2 * float(z["f64.loss"])
        for n_, p in names.items():
            if p.grad is not None:
                assert bool(torch.isfinite(p.grad).all()), n_
    # ---- eval mode: the BatchNorm running statistics are the ones the step above left (the weights are unchanged)
    model.eval()
    with torch.no_grad():
        ev = model(x.to(dev), mode="test")
    assert len(ev) == 8
    if mode != "bf16":
        for i, o in enumerate(ev):
            ref64 = torch.from_numpy(z[f"eval.f64.out{i}"]).double()
            err, own = float((o[:, :, ::sub_e, ::sub_e].double().cpu() - ref64).abs().max()), float(z[f"eval.own.out{i}"])
            print(f"resnet50 eval map {i}: |ours - f64| {err:.2e}, the reference's own {own:.2e}")
            assert err <= max(1e-4, 3 * own), i
    else:
        rels = [rell2(o[:, :, ::sub_e, ::sub_e], torch.from_numpy(z[f"eval.f64.out{i}"])) for i, o in enumerate(ev)]
        print("resnet50 bf16 eval, rel-L2 of the maps:", " ".join(f"{v:.3f}" for v in rels))
        for i, v in enumerate(rels):
            assert v < 0.35, i


def test_trainer_capture_replay_resnet50():
    """bf16 Trainer(mutation loss, AdamW): two trainers from equal state, each capture() + two replay()s - loss, flat gradient and parameters equal bit for bit, replay by
    replay.  Trainer(loss="mutation") keeps no maps (last_outs is None: the loss kernels read them in place), so the maps are compared on what the replays made of the two
    models: their forward on the same input, bit for bit."""
    from pn2.trainer import Trainer
    _, x, label, bg = R.fixture()
    x, tgt = x.to(dev), (label.to(dev), bg.to(dev))
    runs, maps = [], []
    for _ in range(2):
        m = _model("bf16")
        tr = Trainer(m, lr=1e-4, clip=None, weight_decay=1e-4, loss="mutation", hot=m.hot_parameters(True))
        tr.capture(x, tgt, warmup=2)
        got = []
        for _r in range(2):
            l = tr.replay(x, tgt).clone()
            torch.cuda.synchronize()
            got.append((l, tr.gflat.clone(), tr.flat.clone()))
        runs.append(got)
        with torch.no_grad():
            maps.append([o.clone() for o in m(x, mode="train")])
    for (l0, g0, w0), (l1, g1, w1) in zip(*runs):
        assert torch.isfinite(l0).all() and torch.isfinite(g0).all() and float(g0.abs().max()) > 0
        assert torch.equal(l0, l1) and torch.equal(g0, g1) and torch.equal(w0, w1)
    assert not torch.equal(runs[0][0][2], runs[0][1][2])          # (the second replay moved the parameters the first one left)
    assert len(maps[0]) == 8 and all(torch.equal(a, b) and bool(torch.isfinite(a).all()) for a, b in zip(*maps))


def test_volume_predictor_resnet101_single():
    """Eval mode, one 4-slice volume at the patch size: the labels are the argmax of the module surface's last map."""
    import pn2
    import volevalref as VR
    from oracle import weights as W
    from pn2.infer import VolumePredictor
    pn2.set_compute_dtype("bf16")
    m = R.build("resnet101", dual=False)          # (resnet50 with these heads stays refused: lib/networks.py)
    man = {k: list(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict(VR.nontrivial_bn_stats(W.make_state_dict(man, seed=5, bn3_gamma=R.BN3_GAMMA), seed=17), strict=True)
    m = m.to(dev).eval()
    image = torch.randn(4, 64, 64, generator=torch.Generator().manual_seed(33)).to(dev)
    with torch.no_grad():
        want = torch.cat([m(image[i:i + 2, None].contiguous())[-1].argmax(1) for i in (0, 2)]).to(torch.uint8)
    got = VolumePredictor(m, patch_size=(64, 64), batch_size=2).predict(image, "last")
    assert got.dtype == torch.uint8 and tuple(got.shape) == (4, 64, 64)
    assert torch.equal(got, want) and len(torch.unique(want)) > 1


def test_resnet101_single_supervision_geometry():
    """EMCADNet(resnet101, dual=False) at 1 x 1 x 64^2: the layer counts and the four out_head convs run forward and backward, every touched gradient finite."""
    import pn2
    from pn2.loss import seg_loss
    pn2.set_compute_dtype("bf16")
    torch.manual_seed(5)
    m = R.build("resnet101", dual=False).to(dev).train()
    assert [len(l) for l in (m.backbone.layer1, m.backbone.layer2, m.backbone.layer3, m.backbone.layer4)] == [3, 4, 23, 3]
    x = torch.randn(1, 1, 64, 64, device=dev)
    label = torch.randint(0, R.K, (1, 8, 8), device=dev).repeat_interleave(8, 1).repeat_interleave(8, 2)
    outs = m(x, mode="train")
    assert [tuple(o.shape) for o in outs] == [(1, R.K, 64, 64)] * 4
    seg_loss(outs, label).backward()
    hot = {id(p) for p in m.hot_parameters()}
    for n_, p in m.named_parameters():
        if id(p) in hot:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n_
        else:
            assert p.grad is None, n_
    assert float(m.backbone.layer3[22].conv2.weight.grad.abs().max()) > 0 and float(m.out_head1.weight.grad.abs().max()) > 0
