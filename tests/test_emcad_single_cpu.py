"""CPU checks of the single-supervision EMCADNet (dual=False): state_dict against the reference's manifest for the b2 and b0 encoders, the dual manifest
unchanged, the float64 restatement of its loss (tests/seglossref.py) against the losses the reference recorded, and the subset masks of the kernels."""
import json
import os

import pytest
import torch

import seglossref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
os.environ.setdefault("PN2_NO_PRETRAINED", "1")


def _keys(m):
    return [(k, list(v.shape)) for k, v in m.state_dict().items()]


def test_single_state_dict_matches_reference_manifest():
    from lib.networks import EMCADNet
    ref = json.load(open(os.path.join(G, "manifest_emcad_single.json")))
    m = EMCADNet(num_classes=9, activation="relu6", pretrain=False)
    assert m.dual is False
    assert _keys(m) == list(ref["emcadnet_single_k9"].items())
    assert sum(p.numel() for p in m.parameters()) == ref["n_params"]
    assert _keys(m) == [(k, list(v)) for k, v in R.single_manifest(9).items()]
    hot = {id(p) for p in m.hot_parameters()}
    assert all(id(p) in hot for n, p in m.named_parameters() if n.startswith("out_head"))


def _decoder_shapes(ch, K):
    """key -> shape of the EMCAD decoder (decoders.py:330-353: MSCB expansion 2, kernel sizes 1 / 3 / 5, LGAG with C/2 groups of two channels, CAB ratio 16) and
    the out_head convs (networks.py:94-97) for the stage widths ch = [c4, c3, c2, c1]."""
    d = {}

    def bn(p, c):
        for n in ("weight", "bias", "running_mean", "running_var"):
            d[f"{p}.{n}"] = [c]
        d[f"{p}.num_batches_tracked"] = []
    for i, lvl in enumerate((4, 3, 2, 1)):
        c = ch[i]
        p = f"decoder.mscb{lvl}.0."
        d[p + "pconv1.0.weight"] = [2 * c, c, 1, 1]; bn(p + "pconv1.1", 2 * c)
        for j, k in enumerate((1, 3, 5)):
            d[p + f"msdc.dwconvs.{j}.0.weight"] = [2 * c, 1, k, k]; bn(p + f"msdc.dwconvs.{j}.1", 2 * c)
        d[p + "pconv2.0.weight"] = [c, 2 * c, 1, 1]; bn(p + "pconv2.1", c)
        d[f"decoder.cab{lvl}.fc1.weight"] = [c // 16, c, 1, 1]; d[f"decoder.cab{lvl}.fc2.weight"] = [c, c // 16, 1, 1]
        d[f"out_head{lvl}.weight"] = [K, c, 1, 1]; d[f"out_head{lvl}.bias"] = [K]
        if i:
            cin, p = ch[i - 1], f"decoder.eucb{lvl}."
            d[p + "up_dwc.1.weight"] = [cin, 1, 3, 3]; bn(p + "up_dwc.2", cin)
            d[p + "pwc.0.weight"] = [c, cin, 1, 1]; d[p + "pwc.0.bias"] = [c]
            p = f"decoder.lgag{lvl}."
            for w in ("W_g", "W_x"):
                d[p + w + ".0.weight"] = [c // 2, 2, 3, 3]; d[p + w + ".0.bias"] = [c // 2]; bn(p + w + ".1", c // 2)
            d[p + "psi.0.weight"] = [1, c // 2, 1, 1]; d[p + "psi.0.bias"] = [1]; bn(p + "psi.1", 1)
    d["decoder.sab.conv.weight"] = [1, 2, 7, 7]
    return d


def test_single_state_dict_b0_channels():
    """pvt_v2_b0: channels [256, 160, 64, 32] (networks.py:25-28).  The shapes are derived from the channel list; the derivation is first checked against the
    reference's manifest for pvt_v2_b2, and the key order against the b2 model (whose order that manifest pins)."""
    from lib.networks import EMCADNet
    ref = json.load(open(os.path.join(G, "manifest_emcad_single.json")))["emcadnet_single_k9"]
    rest = lambda d: [k for k in d if k.startswith(("decoder.", "out_head"))]
    want2 = _decoder_shapes([512, 320, 128, 64], 9)
    assert {k: ref[k] for k in rest(ref)} == want2
    m = EMCADNet(num_classes=4, activation="relu6", encoder="pvt_v2_b0", pretrain=False)
    sd = {k: list(v.shape) for k, v in m.state_dict().items()}
    assert rest(sd) == rest(ref)
    assert {k: sd[k] for k in rest(sd)} == _decoder_shapes([256, 160, 64, 32], 4)
    assert tuple(m.backbone.patch_embed1.proj.weight.shape)[0] == 32


def test_dual_state_dict_still_matches_its_manifest():
    from lib.networks import EMCADNet
    ref = json.load(open(os.path.join(G, "manifest_emcad.json")))["emcadnet_dual_k9"]
    m = EMCADNet(num_classes=9, activation="relu6", pretrain=False, dual=True)
    assert _keys(m) == list(ref.items())
    assert not any(n.startswith("out_head") for n, p in m.named_parameters() if any(p is q for q in m.hot_parameters()))


def test_resnet_encoders_stay_unbuilt():
    from lib.networks import EMCADNet
    with pytest.raises(NotImplementedError):
        EMCADNet(num_classes=9, encoder="resnet50", pretrain=False)


@pytest.mark.parametrize("mode", R.MODES)
def test_float64_restatement_reproduces_reference_losses(mode):
    """tests/seglossref.py:seg_loss_ref on the reference's float64 outputs against the loss the reference's own trainer code computed from them."""
    z = R.load_fixture()
    outs = R.fixture_outs(z, "f64.")
    assert all(o.dtype == torch.float64 and tuple(o.shape) == (2, 9, 64, 64) for o in outs)
    got = float(R.seg_loss_ref(outs, torch.from_numpy(z["label"]), mode, (0.3, 0.7)))
    want = float(z["f64.loss." + mode])
    assert abs(got - want) <= 1e-10 * abs(want), (mode, got, want)


def test_subset_masks():
    from pn2.loss import SEG_SUBSETS
    assert R.subset_mask("mutation") == 0x7FFF and R.subset_mask("deep_supervision") == 0x8B and R.subset_mask("last") == 0x80
    assert {m: R.subset_mask(m) for m in R.MODES} == SEG_SUBSETS
    assert len(R.subsets("mutation")) == 15


def test_seg_loss_entry_points_refuse_bad_arguments_before_any_launch():
    """Status -2 for subsets == 0, a bit above 15 and K outside 2..9; -1 for a null pointer; the width helper's range.  Every case returns on a host-side check."""
    import ctypes as C
    from pn2 import capi
    lib = capi.load()
    assert [lib.pn2_seg_loss_width(k) for k in range(0, 12)] == [-1, -1] + [15 * (1 + 2 * k) + k for k in range(2, 10)] + [-1, -1]
    buf = (C.c_float * 16)()
    ptr = C.cast(buf, C.c_void_p)
    four = (C.c_void_p * 4)(*[ptr.value] * 4)
    fwd = lambda subsets, K, maps=four: lib.pn2_seg_loss_fwd(maps, subsets, ptr, 1, 16, K, 0.3, 0.7, ptr, ptr, ptr, None)
    bwd = lambda subsets, K, d=four: lib.pn2_seg_loss_bwd(four, d, subsets, ptr, 1, 16, K, 0.3, 0.7, ptr, 1.0, None)
    for subsets, K in ((0, 9), (0x8000, 9), (0xFFFF, 4), (0x7FFF, 1), (0x7FFF, 10), (0x80, 0)):
        assert fwd(subsets, K) == -2 and bwd(subsets, K) == -2, (subsets, K)
    hole = (C.c_void_p * 4)(ptr.value, ptr.value, None, ptr.value)
    assert fwd(0x7FFF, 9, None) == -1 and bwd(0x7FFF, 9, None) == -1
    assert fwd(0, 9, hole) == -2 and fwd(0x7FFF, 9, hole) == -1 and bwd(0x7FFF, 9, hole) == -1
