"""Reference helpers of the fp32 / fp32fast conv kernel tests: the implicit-GEMM operands of a conv launch (pn2_conv_desc / pn2_wgrad_desc terms),
gathered for SAMPLED output rows, so that a float64 contraction of exactly the fp32 operands the kernel saw costs a small fraction of the launch, and the
precision gates of the two fp32 modes.

Column order of every gathered row is the packed-weight order of the C ABI: tap * Cin_p + ci (forward and weight gradient), tap * Cout_fwd + co (dgrad),
so that `gather(...) @ wp[:n_out, :K].T` is the conv's output rows and `dy[:, co].T @ gather(x, all rows)` the packed weight gradient row co.
Pinned against F.conv2d / F.conv_transpose2d / autograd by tests/test_fp32ref_cpu.py."""
import math

import torch

U32 = 2.0 ** -24          # unit roundoff of fp32 (round to nearest)
U64 = 2.0 ** -53


def rup(v, m):
    return (v + m - 1) // m * m


def sample_rows(M, seed, block=64, edge=128):
    """The first and last `edge` rows plus one seeded row in every `block`-row block: at least one checked row in every (row tile, column tile) pair for
    row tiles of 64 / 128, so a wrong tile remap cannot hide."""
    g = torch.Generator().manual_seed(seed)
    nb = (M + block - 1) // block
    pick = torch.arange(nb) * block + (torch.rand(nb, generator=g) * block).long()
    rows = torch.cat([torch.arange(min(edge, M)), torch.arange(max(0, M - edge), M), pick.clamp(max=M - 1)])
    return torch.unique(rows)


def _fwd_index(rows, N, H, W, OH, OW, KH, KW, s, ph, pw, dh, dw):
    """-> (pixel index [R, taps], valid [R, taps]) of the forward gather: output pixel m reads input (n, oy*s - ph + r*dh, ox*s - pw + c*dw)"""
    n, rem = rows // (OH * OW), rows % (OH * OW)
    oy, ox = rem // OW, rem % OW
    r = torch.arange(KH, device=rows.device).repeat_interleave(KW)
    c = torch.arange(KW, device=rows.device).repeat(KH)
    iy = oy[:, None] * s - ph + r[None, :] * dh
    ix = ox[:, None] * s - pw + c[None, :] * dw
    ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
    return (n[:, None] * H + iy.clamp(0, H - 1)) * W + ix.clamp(0, W - 1), ok


def _dgrad_index(rows, N, H, W, OH, OW, KH, KW, s, ph, pw, dh, dw):
    """Transposed gather in pn2_conv_desc terms (H, W: the gathered dy; OH, OW: the produced dx = the forward's input): dx pixel (n, iy, ix) reads
    dy (n, ty / s, tx / s) with ty = iy + ph - r*dh wherever s divides ty and the quotient lies inside dy."""
    n, rem = rows // (OH * OW), rows % (OH * OW)
    iy, ix = rem // OW, rem % OW
    r = torch.arange(KH, device=rows.device).repeat_interleave(KW)
    c = torch.arange(KW, device=rows.device).repeat(KH)
    ty = iy[:, None] + ph - r[None, :] * dh
    tx = ix[:, None] + pw - c[None, :] * dw
    ok = (ty >= 0) & (tx >= 0) & (ty % s == 0) & (tx % s == 0) & (ty // s < H) & (tx // s < W)
    oy, ox = (ty // s).clamp(0, H - 1), (tx // s).clamp(0, W - 1)
    return (n[:, None] * H + oy) * W + ox, ok


def gather(src, rows, geom, transposed):
    """src: [N*H*W, ld] rows of the gathered tensor (any dtype / device; channels [0, Cin_p) are read, the rest never), rows: output rows (int64, same
    device).  geom = (N, H, W, OH, OW, Cin_p, KH, KW, s, ph, pw, dh, dw) in pn2_conv_desc terms.  -> [R, KH*KW*Cin_p], zeros for taps outside the map."""
    N, H, W, OH, OW, Cin_p, KH, KW, s, ph, pw, dh, dw = geom
    idx, ok = (_dgrad_index if transposed else _fwd_index)(rows, N, H, W, OH, OW, KH, KW, s, ph, pw, dh, dw)
    v = src[idx.reshape(-1), :Cin_p].reshape(rows.numel(), KH * KW, Cin_p)
    v = torch.where(ok[:, :, None], v, torch.zeros((), dtype=v.dtype, device=v.device))
    return v.reshape(rows.numel(), KH * KW * Cin_p)


def wgrad_rows(dy, x, co, geom, dt=torch.float64, chunk=1 << 16):
    """Packed weight gradient rows co (all k columns) over ALL output pixels: sum_m dy[m, co] * gather(x, m)[k], accumulated in `dt` on dy's device
    chunk by chunk, plus the same contraction on |dy|, |x| (S of the gates).  geom as gather() (forward terms).  -> (g [len(co), K], S)"""
    N, H, W, OH, OW = geom[:5]
    M = N * OH * OW
    K = geom[6] * geom[7] * geom[5]
    g = torch.zeros(len(co), K, dtype=dt, device=dy.device)
    S = torch.zeros_like(g)
    cot = torch.as_tensor(co, device=dy.device)
    for m0 in range(0, M, chunk):
        rows = torch.arange(m0, min(M, m0 + chunk), device=dy.device)
        a = dy[rows][:, cot].to(dt)
        b = gather(x, rows, geom, False).to(dt)
        g += a.t() @ b
        S += a.abs().t() @ b.abs()
    return g, S


def spacing32(v):
    """ulp of the fp32 value(s) v (float64 tensor of fp32-representable values): distance to the next fp32 away from zero"""
    a = v.abs().float()
    return (torch.nextafter(a, torch.full_like(a, math.inf)) - a).double()


def gate_fp32(got, r, S, K, extra=None):
    """fp32 path: the contraction runs in double and is rounded ONCE to fp32.  |got - r| <= 1/2 ulp(got) (the rounding) + 2 K 2^-53 S (the double sums of
    the kernel and of the reference, each <= K u64 S in the worst case).  `extra`: bound of further roundings (accumulation, slabs) added to it."""
    tol = 0.5 * spacing32(got) + 2 * K * U64 * S
    if extra is not None:
        tol = tol + extra
    return tol


def gate_fp32fast(S, K, chain=16):
    """fp32fast worst case: fp32 products summed in MFMA chains of `chain` k-values from C = 0, chain results met by round-to-nearest adds.  An element
    of r passes through at most `chain` in-chain adds (charged 2 u each: the matrix core's internal adds need not round to nearest; an exact fmaf chain
    costs u per add and passes too), at most ceil(K / chain) round-to-nearest adds and one store rounding (+1 for slack):
    |got - r| <= (2 chain + ceil(K / chain) + 2) u32 S."""
    return (2 * chain + math.ceil(K / chain) + 2) * U32 * S


def rms(t):
    return float(t.double().pow(2).mean().sqrt())


def bf16_error(a, b):
    """rms error of the float64 contraction a @ b.T when its operands are rounded to bf16 first (a: [R, K], b: [C, K], float64 of fp32 values):
    the canary scale - any gate must be at least 10 x tighter than this, or it could not see an fp32 kernel that drops operand bits."""
    r = a @ b.t()
    rb = a.float().bfloat16().double() @ b.float().bfloat16().double().t()
    return rms(rb - r)


def table_codes(table):
    """{key: value} of the fp32fast ('f32f'-suffixed) entries of a tuning table ({repr(key): value} as shipped) with parsed keys"""
    import ast
    out = {}
    for k, v in table.items():
        kk = ast.literal_eval(k)
        if kk[-1] == "f32f":
            out[kk] = tuple(v) if isinstance(v, list) else v
    return out


def key_id(key):
    """readable test id of a table key: g_fwd / g_dgrad / g_ep / w, N x H x W -> OH x OW, channels, kernel, stride / pad / dilation, extras"""
    if key[0] == "g":
        _, N, H, W, OH, OW, Cin_p, ld_in, Cout, KH, KW, s, ph, pw, dh, dw, tr = key[:17]
        rest = key[17:]
        kind = ("dgrad" if tr else "fwd") + ("_ep%d-%d-%d-%d" % tuple(rest[1:5]) if "ep" in rest else "") + ("_pool" if "pool" in rest else "")
        ld = f"ld{ld_in}" if ld_in != Cin_p else ""
        return f"{kind}_n{N}_{H}x{W}to{OH}x{OW}_c{Cin_p}{ld}to{Cout}_k{KH}x{KW}_s{s}p{ph}{pw}d{dh}{dw}"
    _, N, H, W, OH, OW, Cin_p, ld_x, Cout_p, ld_dy, KH, KW, s, ph, pw, dh, dw, ns = key[:18]
    ld = (f"ldx{ld_x}" if ld_x != Cin_p else "") + (f"ldy{ld_dy}" if ld_dy != Cout_p else "")
    return f"wgrad_n{N}_{H}x{W}to{OH}x{OW}_c{Cin_p}to{Cout_p}{ld}_k{KH}x{KW}_s{s}p{ph}{pw}d{dh}{dw}_h{ns}"


def wgrad_tol(mode, got, slabs, ns, S, M):
    """Gate of a weight gradient reduced from `ns` fp32 slabs (got, S: float64 [rows, K]; slabs: float64 [ns, rows, K], the slab elements of those rows)
    over M pixels.  The reduce adds ns fp32 values (<= ns - 1 roundings of <= u times sum_i |slab_i|) and rounds once more at the store.
    fp32: every slab element is the correctly rounded sum of its pixels (1/2 ulp each, + 2 M 2^-53 S for the double sums).
    fp32fast: per split, 32-pixel chains (8 MFMAs of 4 pixels from C = 0: 32 in-chain adds at 2 u), one round-to-nearest add per 32-pixel stage
    (ceil(stages / ns) of them) and the slab store: (2*32 + ceil(stages / ns) + 2) u S."""
    tol = (ns - 1) * U32 * slabs.abs().sum(0) + 0.5 * spacing32(got)
    if mode == "F32":
        return tol + 0.5 * spacing32(slabs).sum(0) + 2 * M * U64 * S
    spb = -(-(-(-M // 32)) // ns)
    return tol + (2 * 32 + spb + 2) * U32 * S
