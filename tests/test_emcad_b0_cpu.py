"""EMCADNet(dual, K=9) with the PVTv2-B0 encoder on the CPU: the mirror builds with the reference's state_dict layout, and the oracle composed
with the b0 configuration reproduces the imported reference's float64 vectors (tests/golden/make_golden_emcad_b0.py)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pranet-v2_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ.setdefault("PN2_NO_PRETRAINED", "1")
import emcad_b0ref as R  # noqa: E402


def test_emcadnet_b0_state_dict_matches_reference_manifest():
    from lib.networks import EMCADNet
    m = EMCADNet(num_classes=9, kernel_sizes=[1, 3, 5], expansion_factor=2, activation="relu6", encoder="pvt_v2_b0", pretrain=False, dual=True)
    ref = R.reference_manifest()
    assert [(k, list(v.shape)) for k, v in m.state_dict().items()] == list(ref.items())
    assert [(k, list(v)) for k, v in R.manifest().items()] == list(ref.items())
    assert [m.backbone.block1[0].attn.num_heads, m.backbone.block4[0].attn.num_heads] == [1, 8]
    assert all(b[0].attn.dim // b[0].attn.num_heads == 32 for b in (m.backbone.block1, m.backbone.block2, m.backbone.block3, m.backbone.block4))


def test_emcadnet_other_encoders_still_refused():
    from lib.networks import EMCADNet
    for enc in ("resnet18", "resnet34"):
        try:
            EMCADNet(num_classes=9, encoder=enc, pretrain=False, dual=True)
        except NotImplementedError:
            continue
        raise AssertionError(enc)


def test_b0_oracle_matches_reference_float64():
    from oracle import emcad_oracle as E
    z, x, label, bg = R.fixture()
    P = {k: ((v.double().requires_grad_(True) if not k.endswith(("running_mean", "running_var")) else v.double()) if v.dtype.is_floating_point else v.clone())
         for k, v in R.state_dict().items()}
    sub = int(z["sub"])
    outs = R.forward(P, x.double(), True)
    for i, o in enumerate(outs):
        ref = torch.from_numpy(z[f"f64.out{i}"]).double()
        got = o.detach()[:, :, ::sub, ::sub]
        assert float((got - ref).abs().max()) <= 1e-6 * max(1.0, float(ref.abs().max())), i     # the fixture holds the float64 maps rounded to fp32
    loss = E.mutation_loss(outs, label, bg.double())
    assert abs(float(loss.detach()) - float(z["f64.loss"])) < 1e-9 * float(z["f64.loss"])
    loss.backward()
    for k in z.files:
        if k.startswith("f64.grawnorm."):
            name = k[len("f64.grawnorm."):]
            g = P[name].grad
            assert abs(float(g.norm()) - float(z[k])) <= 1e-8 * float(z[k]) + 1e-12, name
            raw = torch.from_numpy(z["f64.graw." + name])
            assert float((g.reshape(-1)[:raw.numel()] - raw).abs().max()) <= 1e-8 * float(raw.abs().max()) + 1e-12, name
