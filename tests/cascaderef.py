"""TEST INFRASTRUCTURE - float64 restatement (numpy) of the CASCADE decoders' additive attention gate, as csrc/pn2_cascade.hip splits it, with the error bounds the
GPU tests hold the kernels to.

  g1 = BN_g(W_g g)   x1 = BN_x(W_x x)   psi = sigmoid(BN_psi(w_psi . relu(g1 + x1) + b_psi))   out = g + x * psi      (MIST/lib/decoders.py:73-79 + the aggregate line)

The kernels start from the raw conv outputs rg, rx [M][F] and the BatchNorm rows (scale, shift), so the pieces are
  relu_sum      s = relu(rg * sg + hg + rx * sx + hx)                       psi_raw = s @ w
  bn1           train: batch mean / biased variance of psi_raw -> a = gamma * invstd, b = beta - mean * a ; eval: the running statistics
  apply         out = g + x * sigmoid(a * psi_raw + b)
  bwd_gate      dx = dout * psi, dg = dout, dz = psi (1 - psi) sum_c dout x     p1 = sum dz, p2 = sum dz xhat
  bwd_sum       dpsi_raw = c0 (dz - c1 - xhat c2)  (c0 = gamma invstd, c1 = mean dz, c2 = mean dz xhat; eval: a dz)
                dsum = dpsi_raw w [s > 0]     dw = sum_m dpsi_raw s     db = sum_m dpsi_raw
tests/test_cascade_cpu.py holds gate_forward / gate_backward (the pieces chained, with the convs) to torch autograd in float64.

Bounds (the rule of tests/test_gpu_vit_kernels.py: n * 2^-24 * sum|terms| per fp32 accumulation, + 2^-8 |ref| for a bf16 store; E = 2^-24):
  relu argument   4 E T, T = |rg sg| + |hg| + |rx sx| + |hx| (two fused multiply-adds and an add); where |argument| is below that the ReLU's side is not decided at fp32:
                  the mask-dependent outputs (dsum) are not compared there
  psi_raw         (F + 4) E sum_c |w_c| T_c
  sigmoid         z = a v + b: 2 E (|a v| + |b|); psi: z's error / 4 + 4 E (expf, the add, the division: each within an ulp of a value <= 1... 2 for expf)
  out, dx         |x| e_psi + 2 E (|g| + |x psi|)  /  |dout| e_psi + E |ref|
  dz              (Cp + 3) E sum_c |dout x| psi (1 - psi) + |t| e_psi    (|d psi (1 - psi) / d psi| <= 1)
  p1, p2          against float64 sums of the READ-BACK dz: M E sum |terms| (p2's terms carry xhat: + 3 E each)
  dpsi_raw        8 E (|c0 dz| + |c0 c1| + |c0 c2 xhat|)
  dsum            e_dp |w| + E |ref| ; dw: M E sum_m |dp s| + sum_m (e_dp |s| + |dp| e_s) ; db: M E sum |dp| + sum e_dp"""
import numpy as np

E = 2.0 ** -24
BF = 2.0 ** -8


def sigmoid(z):
    return 1.0 / (1.0 + np.exp(-z))


def relu_sum(rg, sg, hg, rx, sx, hx):
    """-> (s, T, arg): relu(BN_g + BN_x), the magnitude of the terms of its argument, the argument"""
    arg = rg * sg + hg + rx * sx + hx
    return np.maximum(arg, 0.0), np.abs(rg * sg) + np.abs(hg) + np.abs(rx * sx) + np.abs(hx), arg


def bn1(v, gamma, beta, eps, running=None):
    """one-channel BatchNorm rows -> (a, b, mean, invstd); running = (mean, var): eval mode (mean = invstd = None)"""
    if running is not None:
        a = gamma / np.sqrt(running[1] + eps)
        return a, beta - running[0] * a, None, None
    mean, var = v.mean(), v.var()
    invstd = 1.0 / np.sqrt(var + eps)
    a = gamma * invstd
    return a, beta - mean * a, mean, invstd


def apply(g, x, v, a, b):
    return g + x * sigmoid(a * v + b)[:, None]


def bwd_gate(dout, x, v, a, b, mean, invstd):
    """-> dx, dg, dz, p1, p2"""
    psi = sigmoid(a * v + b)
    dz = (dout * x).sum(1) * psi * (1.0 - psi)
    xh = (v - mean) * invstd if mean is not None else np.zeros_like(v)
    return dout * psi[:, None], dout.copy(), dz, dz.sum(), (dz * xh).sum()


def bwd_sum(dz, v, a, mean, invstd, coef, s, w):
    """coef = (c0, c1, c2) or None (eval) -> dpsi_raw, dsum, dw, db"""
    if coef is None:
        dp = a * dz
    else:
        dp = coef[0] * (dz - coef[1] - (v - mean) * invstd * coef[2])
    return dp, dp[:, None] * w[None, :] * (s > 0), (dp[:, None] * s).sum(0), dp.sum()


# ---------------------------------------------------------------------------------------------- the whole gate with its convs (module-level restatement)
def bn_train(t, gamma, beta, eps):
    mean, var = t.mean(0), t.var(0)
    invstd = 1.0 / np.sqrt(var + eps)
    return gamma * invstd, beta - mean * gamma * invstd, mean, invstd


def gate_forward(g, x, P, eps=1e-5):
    """g, x [M][C] float64; P: Wg [F][C], bg, gam_g, bet_g, Wx, bx, gam_x, bet_x, wpsi [F], bpsi, gam_p, bet_p (train-mode BatchNorm) -> out, cache"""
    rg, rx = g @ P["Wg"].T + P["bg"], x @ P["Wx"].T + P["bx"]
    sg, hg, mg, ig = bn_train(rg, P["gam_g"], P["bet_g"], eps)
    sx, hx, mx, ix = bn_train(rx, P["gam_x"], P["bet_x"], eps)
    s, _, _ = relu_sum(rg, sg, hg, rx, sx, hx)
    v = s @ P["wpsi"] + P["bpsi"]
    a, b, mean, invstd = bn1(v, P["gam_p"], P["bet_p"], eps)
    return apply(g, x, v, a, b), dict(rg=rg, rx=rx, mg=mg, ig=ig, mx=mx, ix=ix, s=s, v=v, a=a, b=b, mean=mean, invstd=invstd)


def bn_backward(dy, raw, mean, invstd, gamma):
    xh = (raw - mean) * invstd
    dbeta, dgamma = dy.sum(0), (dy * xh).sum(0)
    return gamma * invstd * (dy - dy.mean(0) - xh * (dy * xh).mean(0)), dgamma, dbeta


def gate_backward(dout, g, x, P, c):
    """-> dict of gradients: g, x and every parameter of P"""
    M = g.shape[0]
    dx, dg, dz, p1, p2 = bwd_gate(dout, x, c["v"], c["a"], c["b"], c["mean"], c["invstd"])
    coef = (P["gam_p"] * c["invstd"], p1 / M, p2 / M)
    dp, dsum, dw, db = bwd_sum(dz, c["v"], c["a"], c["mean"], c["invstd"], coef, c["s"], P["wpsi"])
    G = {"gam_p": p2, "bet_p": p1, "wpsi": dw, "bpsi": db}
    for t, raw, m_, i_, inp, acc in (("g", c["rg"], c["mg"], c["ig"], g, dg), ("x", c["rx"], c["mx"], c["ix"], x, dx)):
        draw, G["gam_" + t], G["bet_" + t] = bn_backward(dsum, raw, m_, i_, P["gam_" + t])
        G["W" + t], G["b" + t] = draw.T @ inp, draw.sum(0)
        G[t] = acc + draw @ P["W" + t]
    return G


# ---------------------------------------------------------------------------------------------- bounds
def e_psi(v, a, b):
    return 0.25 * 2 * E * (np.abs(a * v) + abs(b)) + 4 * E


def bound_psi_raw(T, w):
    return (T.shape[1] + 4) * E * (T * np.abs(w)[None, :]).sum(1)


def bound_store(ref, bf16):
    return BF * np.abs(ref) if bf16 else 0.0


def bound_out(g, x, v, a, b, ref, bf16):
    psi = sigmoid(a * v + b)
    return np.abs(x) * e_psi(v, a, b)[:, None] + 2 * E * (np.abs(g) + np.abs(x * psi[:, None])) + bound_store(ref, bf16)


def bound_dx(dout, v, a, b, ref, old, bf16):
    return np.abs(dout) * e_psi(v, a, b)[:, None] + E * (np.abs(ref) + np.abs(old)) + bound_store(ref, bf16)


def bound_dz(dout, x, v, a, b, Cp):
    psi = sigmoid(a * v + b)
    return (Cp + 3) * E * np.abs(dout * x).sum(1) * psi * (1 - psi) + np.abs((dout * x).sum(1)) * e_psi(v, a, b)


def bound_dp(dz, v, mean, invstd, coef, a):
    if coef is None:
        return 2 * E * np.abs(a * dz)
    xh = (v - mean) * invstd
    return 8 * E * (np.abs(coef[0] * dz) + abs(coef[0] * coef[1]) + np.abs(coef[0] * coef[2] * xh))
