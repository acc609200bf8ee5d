"""Plain float64 references of what pn2_vit.hip computes - LayerNorm forward / backward, column sums and their finalisation, the depth-wise 3x3 conv (flip,
bias, accumulate) with the exact-erf GELU and its derivative, the depth-wise weight / bias gradients and the DropPath scale - with the case tables, the seeded
inputs, the tolerance rules and a Python mirror of the launch geometry, for tests/test_gpu_vit_kernels.py.  Nothing here is shared with the product.

Everything is a torch tensor: float64 gives the yardstick, `dtype=torch.float32` gives "the same formula in fp32" (ref32), and the depth-wise functions are
nine shifted multiply-adds over a zero-padded NHWC tensor, so they also run on device tensors for the two large shapes.  Inputs are exactly representable in
the storage dtype of the case (bf16 cases draw bf16 numbers), so kernel and reference see the same numbers.

The mirror (ln_lpr, rows_for, colsum_plan, dw_row_geometry, dw_plan, dw_wgrad_plan) only labels cases: it says which kernel, vector width and segment plan a
case is meant to reach.  tests/test_vitref_cpu.py holds it to the library wherever the library exposes the plan, holds the references to torch in float64,
asserts that every route is reached by a case, and shows that the fp32 evaluation of each reference passes the bound the kernel gets.

Tolerance rules (bound functions below; no number is taken from a kernel):
  rows_bound    fp32 sums, per ROW: max(1e-5 * max|ref64 row|, 3 * max|ref32 - ref64| of that row).  `mean` is one number per row that may cancel to
                nothing, so its floor is 1e-5 * max|x row| (what it is the mean of); rstd's floor is 1e-5 * rstd.
  nterm_bound   an fp32 accumulation of n terms in any order: n * 2^-24 * sum|terms| per output.
  round_bound   a value accumulated in double and rounded once: 2^-24 * |ref|; accumulate adds 2^-24 * (|old| + |new|).
  bf16 stores   add the half ulp 2^-8 * |ref64| (a bf16 half ulp at the bottom of a binade: no room for a truncating convert), at least the 2^-134 of
                the subnormal range (bf_half).
  gelu_bound    K * (2^-23 * |z| + 2^-22 * |gelu(z)|), derivative K' * (2^-23 + 2^-22 * |gelu'(z)|): one ulp of erf at the top of its range carried through
                0.5 * z * (1 + erf).  K, K' = max(3, 3 * the largest share torch's own fp32 CPU GELU / its autograd derivative reach on GELU_GRID) - measured
                against the reference at run time (gelu_scales), never against the kernel."""
import math
import os
import zlib

import torch
import torch.nn.functional as F

F64, F32 = torch.float64, torch.float32
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16}
DT = {"fp32": 0, "bf16": 1}
VEC = {"fp32": 4, "bf16": 8}          # elements per 16-byte vector
U24, U23, U22, BF_HALF = 2.0 ** -24, 2.0 ** -23, 2.0 ** -22, 2.0 ** -8
LN_NV = 4
LN_MAXC = {dt: 64 * LN_NV * VEC[dt] for dt in VEC}          # the widest LayerNorm row: 1024 fp32, 2048 bf16
GRID_CAP = 16384
ENV_SWITCHES = ("PN2_DW_WIN", "PN2_DW_SEG")          # the mirror describes the plans with both unset


def f32(v):
    """The value a `float` argument of the C ABI carries."""
    return torch.tensor(v, dtype=F32).item()


def rt(t, dt):
    """Round to the storage dtype of the case, as float64."""
    return t.to(TDT[dt]).to(F64)


def representable(t, dt):
    return bool((rt(t, dt) == t).all())


def _gen(name, *key):
    return torch.Generator().manual_seed(zlib.crc32(repr((name,) + tuple(key)).encode()))


def values(name, shape, dt, scale=1.0):
    """Seeded Gaussian input named by case, representable in `dt`, float64 on the CPU."""
    return rt(torch.randn(tuple(shape), generator=_gen(name, *shape), dtype=F64) * scale, dt)


# ================================================================================================================ references
def ln_fwd_ref(x, gamma, beta, eps, dtype=F64):
    """-> y [M][C], mean [M], rstd [M] (two-pass variance, biased)."""
    x, gamma, beta = x.to(dtype), gamma.to(dtype), beta.to(dtype)
    C = x.shape[1]
    mean = x.sum(1) / C
    d = x - mean[:, None]
    rstd = torch.rsqrt((d * d).sum(1) / C + torch.tensor(eps, dtype=dtype))
    return d * rstd[:, None] * gamma + beta, mean, rstd


def ln_bwd_ref(dy, x, gamma, mean, rstd, dtype=F64):
    """-> dx [M][C], dgamma [C], dbeta [C] from the saved mean / rstd (dx = rstd * (g - mean(g) - xhat * mean(g * xhat)), g = dy * gamma)."""
    dy, x, gamma, mean, rstd = (t.to(dtype) for t in (dy, x, gamma, mean, rstd))
    C = x.shape[1]
    xh = (x - mean[:, None]) * rstd[:, None]
    g = dy * gamma
    c1, c2 = g.sum(1) / C, (g * xh).sum(1) / C
    return rstd[:, None] * (g - c1[:, None] - xh * c2[:, None]), (dy * xh).sum(0), dy.sum(0)


def colsum_ref(x, dtype=F64):
    return x.to(dtype).sum(0)


def dwconv_ref(x, w, b=None, flip=0, old=None, dtype=F64):
    """Depth-wise 3x3, stride 1, zero pad 1 over NHWC x [N][H][W][C]; w [C][9] with tap r * 3 + k on input pixel (oy + r - 1, ox + k - 1); flip correlates with
    the mirrored kernel (the data gradient); `old` is what an accumulating call adds to.  Nine shifted multiply-adds: runs on any device."""
    N, H, W, C = x.shape
    xp = F.pad(x.to(dtype), (0, 0, 1, 1, 1, 1))
    w = w.to(dtype)
    a = torch.zeros((N, H, W, C), dtype=dtype, device=x.device) if b is None else b.to(dtype).expand(N, H, W, C).clone()
    for t in range(9):
        r, k = divmod(t, 3)
        a += w[:, 8 - t if flip else t] * xp[:, r:r + H, k:k + W, :]
    return a if old is None else a + old.to(dtype)


def dw_wgrad_ref(dz, x, dtype=F64):
    """-> gw [C][9], gb [C]: gw[c][tap] = sum over pixels of dz[p][c] * x[p + tap][c]."""
    N, H, W, C = x.shape
    xp = F.pad(x.to(dtype), (0, 0, 1, 1, 1, 1))
    dz = dz.to(dtype)
    gw = torch.stack([(dz * xp[:, t // 3:t // 3 + H, t % 3:t % 3 + W, :]).sum((0, 1, 2)) for t in range(9)], 1)
    return gw, dz.sum((0, 1, 2))


def gelu_ref(z, dtype=F64):
    z = z.to(dtype)
    return 0.5 * z * (1 + torch.special.erf(z * math.sqrt(0.5)))


def gelu_grad_ref(z, dtype=F64):
    z = z.to(dtype)
    return 0.5 * (1 + torch.special.erf(z * math.sqrt(0.5))) + z * torch.exp(-0.5 * z * z) * (1 / math.sqrt(2 * math.pi))


def scale_ref(x, s, res=None, dtype=F64):
    """x [N][per_sample] * s[n] (+ res)."""
    y = x.to(dtype) * s.to(dtype)[:, None]
    return y if res is None else y + res.to(dtype)


# ================================================================================================================ bounds and the check
def rows_bound(ref64, ref32, dt=None, floor_of=None):
    """The fp32-sums rule, per row (see the module docstring); `floor_of` [M][...] replaces ref64 in the floor.  dt == "bf16" adds the store's half ulp."""
    M = ref64.shape[0]
    r64 = ref64.reshape(M, -1)
    d32 = (ref32.to(F64) - ref64).abs().reshape(M, -1).amax(1)
    fl = (r64 if floor_of is None else floor_of.reshape(M, -1)).abs().amax(1)
    b = torch.maximum(1e-5 * fl, 3 * d32)[:, None].expand_as(r64)
    if dt == "bf16":
        b = b + bf_half(r64)
    return b.reshape(ref64.shape)


def bf_half(ref):
    """Half a bf16 ulp at `ref`: 2^-8 * |ref| at the bottom of a binade, and never less than half the subnormal spacing 2^-133 (gelu of the smallest bf16
    subnormal is exactly 2^-134, a tie that rounds to zero)."""
    return (BF_HALF * ref.abs()).clamp_min(2.0 ** -134)


def nterm_bound(n, abs_terms):
    return n * U24 * abs_terms


def acc_bound(old, new):
    return U24 * (old.abs() + new.abs())


def gelu_shape(z):
    return U23 * z.abs() + U22 * gelu_ref(z).abs()


def gelu_grad_shape(z):
    return U23 + U22 * gelu_grad_ref(z).abs()


def share(got, ref64, bound):
    """-> (max distance, max distance / bound); a zero bound asks for equality."""
    d = (got.to(F64) - ref64).abs()
    s = torch.where(bound > 0, d / bound.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, math.inf), torch.zeros_like(d)))
    return (float(d.max()), float(s.max())) if d.numel() else (0.0, 0.0)


def check(tag, dt, got, ref64, bound, ref32=None, prefix="VITK"):
    """One line per case (distance, ref32's distance, share of the bound), then the assertion.  Works on device tensors: only scalars reach the host."""
    got = got.to(ref64.device)
    assert got.shape == ref64.shape, (tag, got.shape, ref64.shape)
    assert bool(torch.isfinite(got).all()), (tag, dt, "non-finite output")
    d, s = share(got, ref64, bound + torch.zeros_like(ref64))
    d32 = share(ref32, ref64, torch.ones_like(ref64))[0] if ref32 is not None else float("nan")
    print(f"\n{prefix} {tag} {dt}: ours {d:.2e} ref32 {d32:.2e} of-bound {s:.3f}")
    if not s <= 1.0:          # name the worst element
        b = (bound + torch.zeros_like(ref64)).reshape(-1)
        e = (got.to(F64) - ref64).abs().reshape(-1)
        i = int(torch.where(b > 0, e / b.clamp_min(1e-300), e * math.inf).nan_to_num(0.0, math.inf).argmax())
        where = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ref64.shape)) if ref64.dim() else ()
        raise AssertionError((tag, dt, f"share {s:.3f} at {where}: ours {float(got.reshape(-1)[i])!r} ref64 {float(ref64.reshape(-1)[i])!r} bound {float(b[i]):.3e}"))
    return s


# ---------------------------------------------------------------------------------------------------------------- GELU grids and the measured scale
SWITCH = 0.921875 * math.sqrt(2.0)          # |z| at which erf_nb2 changes its polynomial piece (|z / sqrt 2| = 0.921875)
CLAMP = 4.0 * math.sqrt(2.0)                # ... and at which it clamps


def _neighbours(v, k=3):
    """The fp32 numbers around v: k below .. k above."""
    c = torch.tensor([v], dtype=F32).view(torch.int32).item()
    return torch.tensor([c + i for i in range(-k, k + 1)], dtype=torch.int32).view(F32)


def gelu_grid(dt):
    """fp32: 204800 points - a uniform grid on [-9, 9], both switch points and both clamp points with their neighbouring floats, +-0, +-1e-20, +-30.
    bf16: every finite bf16 with |z| <= 16 (padded with zeros to a multiple of 8)."""
    if dt == "bf16":
        bits = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)
        z = bits.view(torch.bfloat16).to(F64)
        z = z[torch.isfinite(z) & (z.abs() <= 16)]
        return torch.cat([z, torch.zeros((-z.numel()) % 8, dtype=F64)])
    special = [_neighbours(s * v) for v in (SWITCH, CLAMP) for s in (1, -1)] + [torch.tensor([0.0, -0.0, 1e-20, -1e-20, 30.0, -30.0], dtype=F32)]
    special = torch.cat(special)
    n = 204800 - special.numel()
    return torch.cat([torch.linspace(-9, 9, n, dtype=F64).to(F32), special]).to(F64)


_SCALES = {}


def gelu_scales():
    """(K, K'): 3 x the largest share of the bound's shape that torch's fp32 CPU GELU and its autograd derivative reach on the fp32 grid, at least 3."""
    if not _SCALES:
        z = gelu_grid("fp32")
        z32 = z.to(F32).requires_grad_(True)
        y32 = F.gelu(z32)
        g32, = torch.autograd.grad(y32.sum(), z32)
        k = share(y32.detach(), gelu_ref(z), gelu_shape(z))[1]
        kg = share(g32, gelu_grad_ref(z), gelu_grad_shape(z))[1]
        _SCALES.update(torch_share=(k, kg), K=(max(3.0, 3 * k), max(3.0, 3 * kg)))
    return _SCALES["K"]


def gelu_bound(z, dt=None):
    b = gelu_scales()[0] * gelu_shape(z)
    return b + bf_half(gelu_ref(z)) if dt == "bf16" else b


def gelu_grad_bound(z, dt=None):
    b = gelu_scales()[1] * gelu_grad_shape(z)
    return b + bf_half(gelu_grad_ref(z)) if dt == "bf16" else b


# ================================================================================================================ mirror of the launch geometry
def pow2ceil(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def ln_lpr(dt, C):
    """Lanes per row of the LayerNorm kernels, -1 when the width is refused."""
    V = VEC[dt]
    if C % V:
        return -1
    lpr = min(64, max(8, pow2ceil(C // V)))
    return lpr if (C // V + lpr - 1) // lpr <= LN_NV else -1


def ln_slots(dt, C):
    lpr = ln_lpr(dt, C)
    return -1 if lpr < 0 else 4 * (64 // lpr)


def ln_nv(dt, C):
    """Instantiation of ln_bwd_k: 1 (one vector per lane) or LN_NV."""
    return 1 if C // VEC[dt] <= ln_lpr(dt, C) else LN_NV


def rows_for(M, unit):
    rows = (M + 511) // 512
    return max(unit, (rows + unit - 1) // unit * unit)


def rows_blocks(M, unit):
    return (M + rows_for(M, unit) - 1) // rows_for(M, unit)


def colsum_plan(dt, M, C, ld):
    """-> (cvp, rows, nblk) or None (refused)."""
    V = VEC[dt]
    if C % V or ld % V:
        return None
    cvp = min(256, pow2ceil(C // V))
    rows = rows_for(M, 256 // cvp)
    return cvp, rows, (M + rows - 1) // rows


def dw_row_geometry(dt, kind, N, H, W, C):
    """kind 0 = conv + GELU, 1 = plain conv / data gradient, 2 = weight gradient -> (VT, SEG, SPR)."""
    vmax = VEC[dt]

    def threads(vt, target):
        return N * H * ((W + target - 1) // target) * (C // vt)
    target = 16
    if kind == 2:
        VT = 2
    else:
        VT = vmax // 2 if kind == 0 else vmax
        while VT > 2 and (C % VT or (VT == vmax and kind == 1 and threads(VT, 16) < 2 * 256 * 8 * 64)):
            VT >>= 1
        if threads(VT, 16) < 200000:
            target = 8
    if dt == "bf16" and threads(4, 32) >= 2 * 256 * 4 * 64 * 4:
        target = 32
    SPR = (W + target - 1) // target
    return VT, (W + SPR - 1) // SPR, SPR


def dw_use_win(dt, N, H, W, C):
    return dt == "bf16" and N * H * W * C * 2 < 0x7fff0000


def dw_plan(dt, gelu, accumulate, N, H, W, C):
    VT, SEG, SPR = dw_row_geometry(dt, 0 if gelu else 1, N, H, W, C)
    win = (not accumulate) and dw_use_win(dt, N, H, W, C)
    if win:
        VT = 4 if C % 4 == 0 else 2
    CV, lanes = C // VT, (256 if dt == "fp32" else 512) // VT
    cvp = lanes if CV >= lanes else pow2ceil(CV)
    R, nseg = 256 // cvp, N * H * SPR
    return dict(win=win, VT=VT, SEG=SEG, SPR=SPR, cvp=cvp, R=R, nseg=nseg, gx=(nseg + R - 1) // R, gy=(CV + cvp - 1) // cvp, CV=CV,
                seg32=(W + 31) // 32 == SPR and dt == "bf16" and N * H * ((W + 31) // 32) * (C // 4) >= 524288)


def dw_colsum_blocks(dt, N, H, W, C):
    if dt != "bf16" or C % 2:
        return -1
    p = dw_plan(dt, False, False, N, H, W, C)
    return p["gx"] if p["win"] else -1


def dw_wgrad_plan(dt, N, H, W, C):
    VT, SEG, SPR = dw_row_geometry(dt, 2, N, H, W, C)
    win = dw_use_win(dt, N, H, W, C)
    if win:
        VT = 4 if C % 4 == 0 else 2
    CV, lanes = C // VT, (32 if dt == "fp32" else 64) // VT * 2
    cvp = lanes if CV >= lanes else pow2ceil(CV)
    R, nseg = 256 // cvp, N * H * SPR
    gy = (CV + cvp - 1) // cvp
    SPC = (nseg + max(1, 1536 // gy) - 1) // max(1, 1536 // gy)
    SPC = (SPC + R - 1) // R * R
    return dict(win=win, VT=VT, SEG=SEG, SPR=SPR, SPC=SPC, cvp=cvp, R=R, nseg=nseg, nchunk=(nseg + SPC - 1) // SPC, gy=gy, CV=CV)


def grid_for(total, cap=GRID_CAP):
    return min(cap, max(1, (total + 255) // 256))


# ================================================================================================================ case tables
# ---------------------------------------------------------------------------------------------------------------- LayerNorm
LN_WIDTHS = {"fp32": (4, 32, 64, 128, 160, 320, 512, 1024), "bf16": (8, 32, 64, 128, 160, 320, 512, 520, 1280, 2048)}
LN_REFUSED = {"fp32": (6, 1028), "bf16": (12, 2056)}          # no multiple of the vector; one vector above the widest
LN_FORMS = ("tight", "pad")
# backward row loops of 2 and 3 trips whose last workgroup / last iteration is partly live: (dt, C, M)
LN_LONG = (("bf16", 512, 2049), ("bf16", 1280, 2049), ("fp32", 320, 2049), ("fp32", 320, 5001), ("fp32", 64, 8193), ("fp32", 4, 16385), ("bf16", 8, 16385))
LN_CONTENT_WIDTHS = {"fp32": (4, 64, 320), "bf16": (8, 64, 520)}
LN_CONTENT_M = 13
EPS = (1e-5, 1e-6)


def ln_ld(dt, C, form):
    """(ld_x, ld_y, ld_dy, ld_dx): tight, or wider than C by one vector and by an odd number of vectors."""
    V = VEC[dt]
    return (C, C, C, C) if form == "tight" else (C + V, C + 3 * V, C + 3 * V, C + V)


def ln_cases():
    """(dt, C, M, form, eps, content): M = 1, one less / one more than a forward workgroup's rows on both forms, the long backward loops, the row-content cases."""
    out = []
    for dt in ("fp32", "bf16"):
        for i, C in enumerate(LN_WIDTHS[dt]):
            rpb = ln_slots(dt, C)
            for j, M in enumerate((1, rpb - 1, rpb + 1)):
                for k, form in enumerate(LN_FORMS):
                    out.append((dt, C, M, form, EPS[(i + j + k) % 2], False))
        for C in LN_CONTENT_WIDTHS[dt]:
            for eps in EPS:
                out.append((dt, C, LN_CONTENT_M, "pad", eps, True))
    for i, (dt, C, M) in enumerate(LN_LONG):
        out.append((dt, C, M, LN_FORMS[i % 2], EPS[i % 2], False))
    return out


def ln_id(c):
    return f"{c[0]}-C{c[1]}-M{c[2]}-{c[3]}-eps{c[4]:g}" + ("-content" if c[5] else "")


ROW_KINDS = ("gauss", "bigmean", "const", "outlier")
CONSTS = (3.0, -0.5, 0.0, 96.0)


def ln_row_kinds(M, content):
    return [ROW_KINDS[r % 4] if content else "gauss" for r in range(M)]


def ln_inputs(case):
    """x, dy, old [M][C] in the storage dtype; gamma (zeros and negative entries), beta fp32.  Content cases cycle Gaussian rows, rows with mean >> spread (fp32:
    1000 + 0.01 * randn, bf16: 256 + 2k - a one-pass variance goes negative on these), constant rows and rows with one outlier of 512."""
    dt, C, M, form, eps, content = case
    key = f"ln_{dt}_{C}_{M}"
    x = values(key + "_x", (M, C), dt)
    for r, kind in enumerate(ln_row_kinds(M, content)):
        if kind == "bigmean":
            g = _gen(key + "_big", r)
            x[r] = 256 + 2 * torch.randint(0, 128, (C,), generator=g).to(F64) if dt == "bf16" else rt(1000 + 0.01 * torch.randn(C, generator=g, dtype=F64), dt)
        elif kind == "const":
            x[r] = CONSTS[(r // 4) % len(CONSTS)]
        elif kind == "outlier":
            x[r, (7 * r) % C] = 512.0
    assert representable(x, dt)
    gamma = values(key + "_gamma", (C,), "fp32")
    gamma[::5] = 0.0
    return dict(x=x, dy=values(key + "_dy", (M, C), dt), old=values(key + "_old", (M, C), dt), gamma=gamma, beta=values(key + "_beta", (C,), "fp32"))


def ln_fwd_expect(case, inp):
    """name -> (ref64, ref32, bound) of pn2_layernorm_fwd."""
    dt, C, M, form, eps, content = case
    e = f32(eps)
    y64, m64, r64 = ln_fwd_ref(inp["x"], inp["gamma"], inp["beta"], e)
    y32, m32, r32 = ln_fwd_ref(inp["x"], inp["gamma"], inp["beta"], e, F32)
    return dict(y=(y64, y32, rows_bound(y64, y32, dt)), mean=(m64, m32, rows_bound(m64, m32, floor_of=inp["x"])), rstd=(r64, r32, rows_bound(r64, r32)))


def ln_saved(case, inp):
    """The mean / rstd the backward call is given: the float64 ones rounded to fp32 (kernel and reference read the same numbers)."""
    _, m, r = ln_fwd_ref(inp["x"], inp["gamma"], inp["beta"], f32(case[4]))
    return rt(m, "fp32"), rt(r, "fp32")


def ln_bwd_expect(case, inp, acc):
    """name -> (ref64, ref32, bound) of pn2_layernorm_bwd; dgamma / dbeta are the block partials summed in float64: M terms of up to three roundings each
    (x - mean, * rstd, * dy) for dgamma, M plain terms for dbeta."""
    dt, C, M = case[:3]
    mean, rstd = ln_saved(case, inp)
    dx64, dg64, db64 = ln_bwd_ref(inp["dy"], inp["x"], inp["gamma"], mean, rstd)
    dx32, dg32, db32 = ln_bwd_ref(inp["dy"], inp["x"], inp["gamma"], mean, rstd, F32)
    b = rows_bound(dx64, dx32)
    if acc:
        b = b + acc_bound(inp["old"], dx64)
        dx64, dx32 = inp["old"] + dx64, inp["old"].to(F32) + dx32
    if dt == "bf16":
        b = b + bf_half(dx64)
    xh = (inp["x"] - mean[:, None]) * rstd[:, None]
    return dict(dx=(dx64, dx32, b), dgamma=(dg64, dg32, nterm_bound(M + 2, (inp["dy"] * xh).abs().sum(0))), dbeta=(db64, db32, nterm_bound(M, inp["dy"].abs().sum(0))))


# ---------------------------------------------------------------------------------------------------------------- column sums
def colsum_cases():
    """(dt, C, M, ld): C = V (256 row lanes), 320, and a width whose channel loop takes a second pass with one live vector; M = 1, R - 1, and above 512 * R
    with a short last block; ld = C and C + V."""
    out = []
    for dt in ("fp32", "bf16"):
        V = VEC[dt]
        for C in (V, 320, 257 * V):
            R = 256 // min(256, pow2ceil(C // V))
            for M in sorted({1, max(1, R - 1), 512 * R + R + max(1, R // 2 - 1) + (R == 1)}):
                for ld in (C, C + V):
                    out.append((dt, C, M, ld))
    return out


FIN_NBLK = (1, 7, 8, 9, 31, 32, 33, 57)
FIN_C = (1, 31, 33, 320)


# ---------------------------------------------------------------------------------------------------------------- depth-wise 3x3
DW_SHAPES = ((2, 1, 1, 2), (2, 3, 2, 6), (3, 5, 9, 64), (1, 7, 40, 8), (2, 4, 17, 516), (2, 3, 3, 1280))
DW_LARGE = {"bf16": (4, 256, 33, 1024), "fp32": (2, 256, 17, 1024)}
DW_WALIGN_SHAPES = ((3, 5, 9, 64), (1, 7, 40, 8))
DW_COMBOS = tuple((flip, bias, gelu, acc) for flip in (0, 1) for bias in (0, 1) for gelu in (0, 1) for acc in (0, 1))


def dw_inputs(shape, dt, device="cpu"):
    """x, dy (dz of the weight gradient), zpre, old in the storage dtype; w [C][9], b [C] fp32.  zpre is spread over both pieces of the erf."""
    N, H, W, C = shape
    key = f"dw_{dt}"
    d = dict(x=values(key + "_x", shape, dt), dy=values(key + "_dy", shape, dt), zpre=values(key + "_z", shape, dt, 1.5), old=values(key + "_old", shape, dt),
             w=values(key + "_w", (C, 9), "fp32", 0.3), b=values(key + "_b", (C,), "fp32"))
    return {k: v.to(device) for k, v in d.items()}


def dw_expect(inp, dt, flip, bias, gelu, acc):
    """name -> (ref64, ref32, bound) of pn2_dwconv3x3: z has ten terms (nine products and the bias), the accumulating call one more; y = gelu(z) gets the GELU
    bound at ref z plus 1.13 x the conv's fp32 bound (max|gelu'| < 1.13)."""
    b, old = (inp["b"] if bias else None), (inp["old"] if acc else None)
    z64, z32 = dwconv_ref(inp["x"], inp["w"], b, flip, old), dwconv_ref(inp["x"], inp["w"], b, flip, old, F32)
    conv = nterm_bound(10, dwconv_ref(inp["x"].abs(), inp["w"].abs(), None if b is None else b.abs(), flip))
    if acc:
        conv = conv + acc_bound(old, z64 - old)
    out = dict(z=(z64, z32, conv + (bf_half(z64) if dt == "bf16" else 0)))
    if gelu:
        out["y"] = (gelu_ref(z64), gelu_ref(z32, F32), gelu_bound(z64, dt) + 1.13 * conv)
    return out


def dz_expect(inp, dt):
    """(ref64, ref32, bound) of dz_out = dy * gelu'(zpre): the derivative's bound times |dy|, the product's rounding, the bf16 store."""
    ref = inp["dy"] * gelu_grad_ref(inp["zpre"])
    b = inp["dy"].abs() * gelu_grad_bound(inp["zpre"]) + U24 * ref.abs() + (bf_half(ref) if dt == "bf16" else 0)
    return ref, inp["dy"].to(F32) * gelu_grad_ref(inp["zpre"], F32), b


def wgrad_expect(dz, x):
    """name -> (ref64, ref32, bound) of the chunk partials summed in float64: N * H * W terms per output (+ 1 for a product that is not fused)."""
    n = x.shape[0] * x.shape[1] * x.shape[2] + 1
    gw64, gb64 = dw_wgrad_ref(dz, x)
    gw32, gb32 = dw_wgrad_ref(dz, x, F32)
    aw, ab = dw_wgrad_ref(dz.abs(), x.abs())
    return dict(gw=(gw64, gw32, nterm_bound(n, aw)), gb=(gb64, gb32, nterm_bound(n, ab)))


# ---------------------------------------------------------------------------------------------------------------- DropPath scale, grid cap
SCALE_VECS = 256 + 37          # per_sample = SCALE_VECS * V: no multiple of 256 * V
SCALES = (0.0, 1.25, 1 / 0.9)
CAP_VECS = 3 * 1398103         # just above GRID_CAP * 256 vectors, three samples: the grid-stride loop takes a second trip


def scale_bound(x, s, res, dt):
    """fp32 without res is exact (one rounding of one product: compare with float32(x * s)); with res the product and the sum may or may not fuse."""
    y = scale_ref(x, s, res)
    b = U24 * y.abs() if res is None else U24 * (scale_ref(x, s).abs() + y.abs())
    return b + (bf_half(y) if dt == "bf16" else 0)


def env_clean():
    return not any(os.environ.get(k) for k in ENV_SWITCHES)
