"""TEST INFRASTRUCTURE - float64 restatement (numpy) of the two kernels the concatenating CASCADE decoder adds to csrc/pn2_cascade.hip, on top of tests/cascaderef.py
(the psi branch and the ReLU-sum half of the backward pass do not depend on the aggregation and are cascaderef's), with the error bounds of the GPU tests.

  apply_cat       out[:, 0:C] = x * sigmoid(a * psi_raw + b)      out[:, C:2C] = g                        (MIST/lib/decoders.py:73-79 + the Concat line, :163)
  bwd_gate_cat    dx = dout[:, 0:C] * psi, dg = dout[:, C:2C], dz = psi (1 - psi) sum_{c < C} dout x      p1 = sum dz, p2 = sum dz xhat
tests/test_cascade_cat_cpu.py holds gate_cat_forward / gate_cat_backward (the pieces chained, with the convs) to the reference's float64 run in the fixture.

Bounds (cascaderef's rule; E = 2^-24, 2^-8 |ref| per bf16 store):
  out, left       |x| e_psi + E |x psi| (one fp32 rounding of the product)        right half: g bit for bit
  dx              cascaderef.bound_dx on the left half of dout                    dg without accumulation: the right half of dout bit for bit;
                                                                                  accumulating: E (|dout| + |old|) (one fp32 add)
  dz              cascaderef.bound_dz on the left half of dout"""
import numpy as np

import cascaderef as R

E, BF = R.E, R.BF


def apply_cat(g, x, v, a, b):
    return np.concatenate([x * R.sigmoid(a * v + b)[:, None], g], axis=1)


def bwd_gate_cat(dout, x, v, a, b, mean, invstd):
    """dout [M][2C] -> dx, dg, dz, p1, p2"""
    Cc = x.shape[1]
    dx, _, dz, p1, p2 = R.bwd_gate(dout[:, :Cc], x, v, a, b, mean, invstd)
    return dx, dout[:, Cc:].copy(), dz, p1, p2


def gate_cat_forward(g, x, P, eps=1e-5):
    """cascaderef.gate_forward with the Concat line in the place of the aggregate line -> out [M][2C], cache"""
    _, c = R.gate_forward(g, x, P, eps)
    return apply_cat(g, x, c["v"], c["a"], c["b"]), c


def gate_cat_backward(dout, g, x, P, c):
    """cascaderef.gate_backward with bwd_gate_cat in the place of bwd_gate -> dict of gradients: g, x and every parameter of P"""
    M = g.shape[0]
    dx, dg, dz, p1, p2 = bwd_gate_cat(dout, x, c["v"], c["a"], c["b"], c["mean"], c["invstd"])
    coef = (P["gam_p"] * c["invstd"], p1 / M, p2 / M)
    _, dsum, dw, db = R.bwd_sum(dz, c["v"], c["a"], c["mean"], c["invstd"], coef, c["s"], P["wpsi"])
    G = {"gam_p": p2, "bet_p": p1, "wpsi": dw, "bpsi": db}
    for t, raw, m_, i_, inp, acc in (("g", c["rg"], c["mg"], c["ig"], g, dg), ("x", c["rx"], c["mx"], c["ix"], x, dx)):
        draw, G["gam_" + t], G["bet_" + t] = R.bn_backward(dsum, raw, m_, i_, P["gam_" + t])
        G["W" + t], G["b" + t] = draw.T @ inp, draw.sum(0)
        G[t] = acc + draw @ P["W" + t]
    return G


# ---------------------------------------------------------------------------------------------- bounds
def bound_out_left(x, v, a, b, ref, bf16):
    return np.abs(x) * R.e_psi(v, a, b)[:, None] + E * np.abs(ref) + R.bound_store(ref, bf16)


def bound_dg(dright, old, acc, bf16):
    """acc = 0: exact"""
    return (E * (np.abs(dright) + np.abs(old)) + R.bound_store(dright + old, bf16)) * acc
