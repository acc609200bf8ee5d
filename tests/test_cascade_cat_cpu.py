"""CPU tests of the concatenating CASCADE decoder's host side: tests/cascadecatref.py (the float64 restatement the GPU kernel tests compare with) against the REFERENCE's
own float64 run of cat(Attention_block(g, x), g) stored in tests/golden/cascade_cat_small.npz ("gate.*", 1e-10 relative, output and every gradient); the state_dict keys,
order and shapes of lib/cascade.py's CASCADE_Cat against the manifest generated from the reference (tests/golden/manifest_cascade_cat.json, written by
tests/golden/make_golden_cascade_cat.py) at both widths; PVT_CASCADE's aggregation switch (the four plain heads, no dual heads, the two ValueErrors); the
NotImplementedError for a gate width that is not a multiple of 8."""
import json
import os
import types

import numpy as np
import pytest

import cascadecatref as RC

HERE = os.path.dirname(os.path.abspath(__file__))


def test_cascadecatref_gate_reproduces_reference_float64():
    z = np.load(os.path.join(HERE, "golden", "cascade_cat_small.npz"))
    C = z["gate.g"].shape[1]
    flat = lambda a: np.transpose(a, (0, 2, 3, 1)).reshape(-1, a.shape[1])
    p = lambda k: z["gate.p." + k]
    P = {"Wg": p("W_g.0.weight")[:, :, 0, 0], "bg": p("W_g.0.bias"), "gam_g": p("W_g.1.weight"), "bet_g": p("W_g.1.bias"),
         "Wx": p("W_x.0.weight")[:, :, 0, 0], "bx": p("W_x.0.bias"), "gam_x": p("W_x.1.weight"), "bet_x": p("W_x.1.bias"),
         "wpsi": p("psi.0.weight")[0, :, 0, 0], "bpsi": float(p("psi.0.bias")[0]), "gam_p": float(p("psi.1.weight")[0]), "bet_p": float(p("psi.1.bias")[0])}
    assert z["gate.out"].shape[1] == 2 * C and z["gate.R"].shape[1] == 2 * C
    o, cache = RC.gate_cat_forward(flat(z["gate.g"]), flat(z["gate.x"]), P)
    G = RC.gate_cat_backward(flat(z["gate.R"]), flat(z["gate.g"]), flat(z["gate.x"]), P, cache)
    rel = lambda a, b: float(np.abs(np.asarray(a) - np.asarray(b)).max() / float(np.abs(np.asarray(b)).max()))
    assert o.shape == (z["gate.g"].size // C, 2 * C) and rel(o, flat(z["gate.out"])) <= 1e-10
    assert np.array_equal(o[:, C:], flat(z["gate.g"]))
    assert rel(G["g"], flat(z["gate.dg"])) <= 1e-10 and rel(G["x"], flat(z["gate.dx"])) <= 1e-10
    for ours, theirs in (("Wg", "W_g.0.weight"), ("Wx", "W_x.0.weight"), ("gam_g", "W_g.1.weight"), ("bet_g", "W_g.1.bias"), ("gam_x", "W_x.1.weight"), ("bet_x", "W_x.1.bias"),
                         ("wpsi", "psi.0.weight"), ("gam_p", "psi.1.weight"), ("bet_p", "psi.1.bias")):
        assert rel(np.asarray(G[ours]).reshape(-1), z["gate.d." + theirs].reshape(-1)) <= 1e-10, ours


def test_cascadecatref_kernels_split_the_row():
    """bwd_gate_cat reads the left half for dx / dz and hands the right half to dg unchanged"""
    rng = np.random.default_rng(3)
    M, C = 7, 8
    x, dout, v = rng.standard_normal((M, C)), rng.standard_normal((M, 2 * C)), rng.standard_normal(M)
    dx, dg, dz, p1, p2 = RC.bwd_gate_cat(dout, x, v, 1.3, -0.2, 0.1, 0.9)
    psi = 1.0 / (1.0 + np.exp(-(1.3 * v - 0.2)))
    assert np.array_equal(dg, dout[:, C:]) and np.allclose(dx, dout[:, :C] * psi[:, None], rtol=1e-14, atol=0)
    assert np.allclose(dz, (dout[:, :C] * x).sum(1) * psi * (1 - psi), rtol=1e-13, atol=0) and np.isclose(p1, dz.sum()) and np.isclose(p2, (dz * (v - 0.1) * 0.9).sum())


@pytest.mark.parametrize("channels", [[768, 384, 192, 96], [512, 320, 128, 64]], ids=str)
def test_cascade_cat_state_dict_matches_reference_manifest(channels):
    from lib.cascade import CASCADE_Cat
    with open(os.path.join(HERE, "golden", "manifest_cascade_cat.json")) as f:
        man = json.load(f)
    want = man[f"CASCADE_Cat:{','.join(map(str, channels))}"]
    m = CASCADE_Cat(channels=channels)
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == want
    c = channels
    assert m.ConvBlock3.conv[0].in_channels == 2 * c[1] and m.ConvBlock1.conv[0].in_channels == 2 * c[3] and m.ConvBlock4.conv[0].in_channels == c[0]
    assert m.CA4.in_planes == c[0] and (m.CA3.in_planes, m.CA2.in_planes, m.CA1.in_planes) == (2 * c[1], 2 * c[2], 2 * c[3])


def test_pvt_cascade_aggregation_switch():
    from lib.cascade import CASCADE_Add, CASCADE_Add_dual, CASCADE_Cat
    from lib.cascade_net import PVT_CASCADE
    kw = dict(num_classes=4, encoder="pvt_v2_b0", pretrain=False)
    m = PVT_CASCADE(dual=False, aggregation="concatenation", **kw)
    assert type(m.decoder) is CASCADE_Cat and m.dual is False
    assert [getattr(m, f"out_head{i}").in_channels for i in (4, 3, 2, 1)] == [256, 160, 64, 32] and all(getattr(m, f"out_head{i}").out_channels == 4 for i in (1, 2, 3, 4))
    names = [n for n, _ in m.named_parameters()]
    assert not any("_fg" in n or "_bg" in n for n in names)
    hot = {id(p) for p in m.hot_parameters(True)}
    assert all(id(p) in hot for p in m.parameters())          # single supervision: the heads and the input conv are on the forward path
    # the default and the explicit additive form are today's modules, keys included
    a, b = PVT_CASCADE(dual=False, **kw), PVT_CASCADE(dual=False, aggregation="additive", **kw)
    assert type(a.decoder) is CASCADE_Add and list(a.state_dict()) == list(b.state_dict())
    assert type(PVT_CASCADE(**kw).decoder) is CASCADE_Add_dual
    with pytest.raises(ValueError):
        PVT_CASCADE(dual=True, aggregation="concatenation", **kw)
    with pytest.raises(ValueError):
        PVT_CASCADE(aggregation="concatenation", **kw)          # (dual defaults to True)
    with pytest.raises(ValueError):
        PVT_CASCADE(dual=False, aggregation="cat", **kw)


def test_concat_gate_refuses_a_width_that_is_no_multiple_of_8():
    """before any engine call: the stand-ins carry a width only"""
    from lib.cascade import Attention_block
    ag = Attention_block(12, 12, 6)
    act = types.SimpleNamespace(C=12)
    with pytest.raises(NotImplementedError):
        ag._build_concat(None, act, act)
