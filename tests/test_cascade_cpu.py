"""CPU tests of the CASCADE decoder's host side: tests/cascaderef.py (the float64 restatement the GPU kernel tests compare with) against the REFERENCE's own float64
Attention_block output and gradients stored in tests/golden/cascade_small.npz ("gate.*", 1e-10 relative), against torch autograd in float64 on the gate written with
torch's own conv / batch_norm at three more shapes, and the state_dict keys, order and shapes of lib/cascade.py's decoders against the manifest generated from the
reference (tests/golden/manifest_cascade.json, written by tests/golden/make_golden_cascade.py)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cascaderef as R

HERE = os.path.dirname(os.path.abspath(__file__))


def _gate_torch(g, x, P, eps=1e-5):
    conv = lambda t, W, b: F.conv2d(t, W[:, :, None, None], b)
    bn = lambda t, ga, be: F.batch_norm(t, None, None, ga, be, True, 0.1, eps)
    g1, x1 = bn(conv(g, P["Wg"], P["bg"]), P["gam_g"], P["bet_g"]), bn(conv(x, P["Wx"], P["bx"]), P["gam_x"], P["bet_x"])
    psi = torch.sigmoid(bn(conv(torch.relu(g1 + x1), P["wpsi"][None, :], P["bpsi"]), P["gam_p"], P["bet_p"]))
    return g + x * psi


@pytest.mark.parametrize("shape", [(2, 1, 1, 8, 4), (2, 3, 5, 12, 6), (2, 8, 8, 24, 12)], ids=str)
def test_cascaderef_gate_matches_torch_float64(shape):
    N, H, W, C, Fi = shape
    gen = torch.Generator().manual_seed(11 + C)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    P = {"Wg": rn(Fi, C) * 0.4, "bg": rn(Fi) * 0.1, "gam_g": rn(Fi) * 0.2 + 1, "bet_g": rn(Fi) * 0.1, "Wx": rn(Fi, C) * 0.4, "bx": rn(Fi) * 0.1, "gam_x": rn(Fi) * 0.2 + 1,
         "bet_x": rn(Fi) * 0.1, "wpsi": rn(Fi) * 0.5, "bpsi": rn(1) * 0.1, "gam_p": rn(1) * 0.2 + 1, "bet_p": rn(1) * 0.1}
    g, x, dout = rn(N, C, H, W), rn(N, C, H, W), rn(N, C, H, W)
    leaves = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    gt, xt = g.clone().requires_grad_(True), x.clone().requires_grad_(True)
    out = _gate_torch(gt, xt, leaves)
    out.backward(dout)
    flat = lambda t: t.permute(0, 2, 3, 1).reshape(-1, C).numpy()
    Pn = {k: (v.numpy() if v.numel() > 1 or k in ("wpsi",) else float(v)) for k, v in P.items()}
    o, cache = R.gate_forward(flat(g), flat(x), Pn)
    G = R.gate_backward(flat(dout), flat(g), flat(x), Pn, cache)
    rel = lambda a, b: float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(float(np.abs(np.asarray(b)).max()), 1e-30))
    assert rel(o, flat(out.detach())) <= 1e-10
    assert rel(G["g"], flat(gt.grad)) <= 1e-10 and rel(G["x"], flat(xt.grad)) <= 1e-10
    for k in ("Wg", "Wx", "gam_g", "bet_g", "gam_x", "bet_x", "wpsi", "gam_p", "bet_p"):
        assert rel(G[k], leaves[k].grad.numpy()) <= 1e-10, k
    # a bias in front of a train-mode BatchNorm has a zero gradient: both sides at rounding level
    for k in ("bg", "bx", "bpsi"):
        assert float(np.abs(G[k]).max()) <= 1e-10 and float(leaves[k].grad.abs().max()) <= 1e-10, k


def test_cascaderef_gate_reproduces_reference_float64():
    """cascaderef's gate, forward and backward, on the reference Attention_block's float64 run (g + AG(g, x), gradients of <out, R>): 1e-10 relative."""
    z = np.load(os.path.join(HERE, "golden", "cascade_small.npz"))
    C = z["gate.g"].shape[1]
    flat = lambda a: np.transpose(a, (0, 2, 3, 1)).reshape(-1, C)
    p = lambda k: z["gate.p." + k]
    P = {"Wg": p("W_g.0.weight")[:, :, 0, 0], "bg": p("W_g.0.bias"), "gam_g": p("W_g.1.weight"), "bet_g": p("W_g.1.bias"),
         "Wx": p("W_x.0.weight")[:, :, 0, 0], "bx": p("W_x.0.bias"), "gam_x": p("W_x.1.weight"), "bet_x": p("W_x.1.bias"),
         "wpsi": p("psi.0.weight")[0, :, 0, 0], "bpsi": float(p("psi.0.bias")[0]), "gam_p": float(p("psi.1.weight")[0]), "bet_p": float(p("psi.1.bias")[0])}
    o, cache = R.gate_forward(flat(z["gate.g"]), flat(z["gate.x"]), P)
    G = R.gate_backward(flat(z["gate.R"]), flat(z["gate.g"]), flat(z["gate.x"]), P, cache)
    rel = lambda a, b: float(np.abs(np.asarray(a) - np.asarray(b)).max() / float(np.abs(np.asarray(b)).max()))
    assert rel(o, flat(z["gate.out"])) <= 1e-10
    assert rel(G["g"], flat(z["gate.dg"])) <= 1e-10 and rel(G["x"], flat(z["gate.dx"])) <= 1e-10
    for ours, theirs in (("Wg", "W_g.0.weight"), ("Wx", "W_x.0.weight"), ("gam_g", "W_g.1.weight"), ("bet_g", "W_g.1.bias"), ("gam_x", "W_x.1.weight"), ("bet_x", "W_x.1.bias"),
                         ("wpsi", "psi.0.weight"), ("gam_p", "psi.1.weight"), ("bet_p", "psi.1.bias")):
        assert rel(np.asarray(G[ours]).reshape(-1), z["gate.d." + theirs].reshape(-1)) <= 1e-10, ours


@pytest.mark.parametrize("channels", [[768, 384, 192, 96], [512, 320, 128, 64]], ids=str)
def test_cascade_state_dict_matches_reference_manifest(channels):
    from lib.cascade import CASCADE_Add, CASCADE_Add_dual
    with open(os.path.join(HERE, "golden", "manifest_cascade.json")) as f:
        man = json.load(f)
    for name, m in (("CASCADE_Add", CASCADE_Add(channels=channels)), ("CASCADE_Add_dual", CASCADE_Add_dual(channels=channels, num_class=9, use_softmax=True))):
        want = man[f"{name}:{','.join(map(str, channels))}"]
        got = [[k, list(v.shape)] for k, v in m.state_dict().items()]
        assert got == want, name
