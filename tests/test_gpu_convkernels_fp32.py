"""The conv GEMM kernels of the two fp32 modes one by one at the C ABI, on plain fp32 operands (randn, never bf16-representable: products of bf16 values
are exact in fp32, so bf16 operands could not reveal a kernel that drops operand bits), against the float64 contraction of the same operands.

  PN2_F32  (fp32): contractions in double on v_mfma_f64_16x16x4_f64, one rounding per output.  Gate (tests/fp32ref.py gate_fp32):
           |got - r| <= 1/2 ulp(got) + 2 K 2^-53 S, S = sum |a b| - correct rounding with slack for the double sums of kernel and reference.  A double
           accumulator rounded to fp32 after a K-step adds up to 1/2 ulp(partial) per step and fails it (tests/test_fp32ref_cpu.py shows that on the CPU).
  PN2_F32F (fp32fast): fp32 products in chains of 16 k-values (4 x v_mfma_f32_16x16x4_f32 from C = 0) joined by round-to-nearest adds.  Gates:
           worst case |got - r| <= (2*16 + ceil(K/16) + 2) 2^-24 S (gate_fp32fast: in-chain adds at 2 u - the code does not rely on the matrix core
           rounding to nearest; an exact fmaf chain, MI355X_MICROARCH, passes too), and rms(got - r) <= 2 rms(ref32 - r) with ref32 = torch's CPU
           float32 conv of the same operands.  Measured ratios are printed (-s): 0.27 .. 1.14, median 0.55, on these geometries.
  Canary: every gate is asserted >= 10 x tighter than the error the same contraction has with bf16-rounded operands (_canary).

Tile codes: fp32fast takes BM / BN of a tuning code (kernel bits ignored, BN 128 clamped to 64) and every code must give the same bits - outputs and
PN2_CONV_STATS partials (of equal row-block height) - because the k order of an output does not depend on the tile.  fp32 ignores the code."""
import ctypes as C
import os, sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "pranet-v2_amd"))
import fp32ref as R  # noqa: E402
from fp32ref import rup  # noqa: E402

dev = "cuda"
MODES = ["F32", "F32F"]

# N, H, W, Cin, Cout, KH, KW, stride, pad_h, pad_w, dil  (tests/test_gpu_convkernels.py GEMMS and KS_GEOMS, plus the fp32 edges)
GEOMS = [
    (2, 11, 13, 72, 40, 1, 1, 1, 0, 0, 1),          # 3 K-steps of 32 floats
    (2, 11, 13, 104, 104, 3, 3, 1, 1, 1, 1),
    (3, 9, 10, 24, 56, 3, 3, 1, 1, 1, 1),
    (2, 12, 12, 32, 32, 3, 3, 1, 3, 3, 3),
    (1, 15, 9, 32, 32, 3, 3, 1, 7, 7, 7),
    (2, 10, 14, 32, 32, 1, 7, 1, 0, 3, 1),
    (2, 10, 14, 32, 32, 5, 1, 1, 2, 0, 1),
    (1, 9, 9, 40, 48, 5, 5, 1, 2, 2, 1),
    (2, 16, 18, 56, 56, 3, 3, 2, 1, 1, 1),
    (2, 17, 15, 8, 32, 3, 3, 2, 1, 1, 1),
    (1, 5, 7, 200, 136, 1, 1, 1, 0, 0, 1),
    (2, 40, 36, 32, 32, 3, 3, 1, 1, 1, 1),
    (3, 20, 18, 56, 56, 3, 3, 1, 1, 1, 1),
    (5, 30, 30, 16, 24, 5, 5, 1, 2, 2, 1),
    (2, 11, 11, 208, 208, 3, 3, 1, 1, 1, 1),        # 59 K-steps
    (1, 5, 7, 456, 136, 1, 1, 1, 0, 0, 1),
    (2, 7, 9, 8, 40, 1, 1, 1, 0, 0, 1),             # 1 K-step (8 of 32 columns live): the DEEP prefetch of fp32fast runs past the end
    (2, 7, 9, 32, 40, 1, 1, 1, 0, 0, 1),            # exactly 1 K-step
    (2, 7, 9, 40, 40, 1, 1, 1, 0, 0, 1),            # 2 K-steps, the second one 8 wide
    (1, 3, 5, 1024, 64, 1, 1, 1, 0, 0, 1),          # 32 K-steps, 15 rows: one ragged row tile
    (3, 13, 11, 16, 8, 3, 3, 1, 1, 1, 1),           # 8 output channels of a 32-wide tile
]
MIXED = {1, 8, 15, 19}          # geometries whose operands mix magnitudes over 2^-10 .. 2^10


def _ids(geoms):
    return [f"{N}x{H}x{W}_c{Ci}to{Co}_k{KH}x{KW}_s{s}p{ph}{pw}d{d}" for N, H, W, Ci, Co, KH, KW, s, ph, pw, d in geoms]


def _lib():
    from pn2 import capi
    return capi.load()


def _mode(name):
    from pn2.capi import F32, F32F
    return {"F32": F32, "F32F": F32F}[name]


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _randn(shape, g, mixed):
    t = torch.randn(*shape, generator=g)
    if mixed:
        t = t * torch.exp2(torch.randint(-10, 11, shape, generator=g).float())
    return t


def _canary(tol_rms, a, b):
    ebf = R.bf16_error(a, b)
    assert tol_rms * 10 <= ebf, f"gate ({tol_rms:.3g}) is not 10 x tighter than the error of bf16 operands ({ebf:.3g})"


def check(mode, got, r, S, K, ref32=None, extra=None, canary=None, what=""):
    """got, r, S: float64 [R, C] (CPU); mode 'F32' / 'F32F'.  Returns the rms ratio against the reference's own fp32 error (fp32fast) or None."""
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output (a tile was not written, or NaN reached it)"
    err = (got - r).abs()
    if mode == "F32":
        tol = R.gate_fp32(got, r, S, K, extra)
    else:
        tol = R.gate_fp32fast(S, K) + 0.5 * R.spacing32(got)
        if extra is not None:
            tol = tol + extra
    bad = err > tol
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the {mode} gate, worst excess {float((err - tol).max()):.3g}"
    ratio = None
    if mode == "F32F" and ref32 is not None:
        own = R.rms(ref32 - r)
        ratio = R.rms(got - r) / own
        print(f"{what}: rms(got - r) / rms(ref32 - r) = {ratio:.3f}")
        assert ratio <= 2.0, (what, ratio)
        if canary is not None:
            _canary(2 * own, *canary)
    elif canary is not None:
        _canary(R.rms(tol), *canary)
    return ratio


def _setup(geom, transposed, mode, slices, seed):
    """-> desc, src (device), wp (device), n_out, M, ld_out, float64 reference pieces (patches [M, K], weight rows [n_out, K]) and ref32"""
    from pn2 import capi
    N, H, W, Cin, Cout, KH, KW, s, ph, pw, dil = geom
    OH = (H + 2 * ph - dil * (KH - 1) - 1) // s + 1
    OW = (W + 2 * pw - dil * (KW - 1) - 1) // s + 1
    mixed = GEOMS.index(geom) in MIXED if geom in GEOMS else False
    g = torch.Generator().manual_seed(seed)
    taps = KH * KW
    d = capi.ConvDesc()
    d.KH, d.KW, d.stride, d.pad_h, d.pad_w, d.dil_h, d.dil_w = KH, KW, s, ph, pw, dil, dil
    if not transposed:
        d.N, d.H, d.W, d.OH, d.OW = N, H, W, OH, OW
        cin, n_out, M = Cin, Cout, N * OH * OW
    else:
        d.N, d.H, d.W, d.OH, d.OW = N, OH, OW, H, W
        cin, n_out, M = Cout, Cin, N * H * W
    ld_in = cin + (24 if slices else 0)
    ld_out = n_out + (12 if slices else 0)
    src = _randn((d.N * d.H * d.W, ld_in), g, mixed)
    src[:, cin:] = float("nan")              # channels of a wider buffer that belong to someone else: never read
    K = taps * cin
    d.Cin_p, d.ld_in, d.Cout, d.ld_out = cin, ld_in, n_out, ld_out
    d.transposed, d.Kp = transposed, rup(K, 128)
    wp = torch.zeros(rup(n_out, 128), d.Kp)
    wp[:n_out, :K] = _randn((n_out, K), g, mixed) * (2.0 / K) ** 0.5
    geo = (d.N, d.H, d.W, d.OH, d.OW, cin, KH, KW, s, ph, pw, dil, dil)
    a = R.gather(src.double(), torch.arange(M), geo, transposed)          # [M, K]
    b = wp[:n_out, :K].double()
    w4 = wp[:n_out, :K].reshape(n_out, KH, KW, cin)
    if not transposed:
        x4 = src[:, :cin].reshape(N, H, W, cin).permute(0, 3, 1, 2)
        ref32 = F.conv2d(x4, w4.permute(0, 3, 1, 2), None, s, (ph, pw), dil).permute(0, 2, 3, 1).reshape(M, n_out)
    else:
        dy4 = src[:, :cin].reshape(N, OH, OW, cin).permute(0, 3, 1, 2)
        op = (H - ((OH - 1) * s - 2 * ph + dil * (KH - 1) + 1), W - ((OW - 1) * s - 2 * pw + dil * (KW - 1) + 1))
        ref32 = F.conv_transpose2d(dy4, w4.permute(3, 0, 1, 2), None, s, (ph, pw), op, 1, dil).permute(0, 2, 3, 1).reshape(M, n_out)
    return d, src.to(dev), wp.to(dev), n_out, M, ld_out, a, b, ref32.double(), K


def _codes(mode, n_out):
    """every tuning code the dtype accepts, 0 (library heuristic) first; fp32fast ignores the kernel bits, so they vary too"""
    out = [0]
    for bm in (1, 2):
        for bn in (1, 2, 3):
            if (bn == 3 and n_out <= 64) or (bn == 2 and n_out <= 32):
                continue
            out.append((1 + (bm + bn) % 3) | (bm << 2) | (bn << 4))
    return out


def _tile_m(mode, code, M, n_out):
    from pn2.capi import call
    bm = (code >> 2) & 3 if mode == "F32F" else 0
    return (64 if bm == 1 else 128) if bm else call.pn2_conv_tile_m(M, n_out, _mode(mode))


def _chan_merge(ps, pq, tm, M):
    nblk = ps.shape[0]
    n_t = torch.full((nblk,), float(tm), dtype=torch.float64); n_t[-1] = M - (nblk - 1) * tm
    mean_t, m2_t = ps.double().cpu(), pq.double().cpu()
    mean = (mean_t * n_t[:, None]).sum(0) / M
    var = (m2_t.sum(0) + (n_t[:, None] * (mean_t - mean) ** 2).sum(0)) / M
    return mean, var


@pytest.mark.parametrize("slices", [0, 1], ids=["dense", "slices"])
@pytest.mark.parametrize("geom", GEOMS, ids=_ids(GEOMS))
@pytest.mark.parametrize("transposed", [0, 1], ids=["fwd", "dgrad"])
@pytest.mark.parametrize("mode", MODES)
def test_gather_gemm_every_tile_code_against_float64(mode, transposed, geom, slices):
    """pn2_conv_gemm, forward (with PN2_CONV_STATS) and dgrad gather, every tile code: bit-identical across codes, within the mode's gate of the float64
    contraction, NaN channels beyond Cin_p never read, guard columns beyond Cout (ld_out > Cout) untouched, the partials' Chan merge = the stored output's
    mean / variance."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    lib = _lib()
    from pn2 import capi
    dt = _mode(mode)
    d, src, wp, n_out, M, ld_out, a, b, ref32, K = _setup(geom, transposed, mode, slices, sum(geom) * 7 + transposed)
    outs, stats = {}, {}
    sentinel = -1.2345678e33
    for code in _codes(mode, n_out):
        tm = _tile_m(mode, code, M, n_out)
        d.flags = (code << 8) | (0 if transposed else capi.CONV_STATS)
        out = torch.full((M, ld_out), float("nan"), device=dev)
        out[:, n_out:] = sentinel
        nblk = (M + tm - 1) // tm
        ps = torch.full((nblk, n_out), float("nan"), device=dev) if not transposed else None
        pq = torch.full((nblk, n_out), float("nan"), device=dev) if not transposed else None
        assert lib.pn2_conv_gemm(dt, P(src), P(wp), P(out), P(ps), P(pq), C.byref(d), _stream()) == 0
        outs[code] = out
        if not transposed:          # the shifted sums start from row 0 of each WAVE tile: 4 x 1 waves (BN 32) and 2 x 2 waves (BN 64) shift differently
            bn = lib.pn2_conv_gemm_tile(dt, C.byref(d)) & 255
            stats.setdefault((tm, bn == 32), {})[code] = (ps, pq)
    torch.cuda.synchronize()
    first = outs[0]
    assert bool((first[:, n_out:] == sentinel).all()), "guard columns beyond Cout were written"
    for code, o in outs.items():
        assert torch.equal(o.view(torch.int32), first.view(torch.int32)), f"{mode}: tile code {code:#x} differs from the heuristic's bits"
    got = first[:, :n_out].double().cpu()
    r = a @ b.t()
    S = a.abs() @ b.abs().t()
    check(mode, got, r, S, K, ref32=ref32, canary=(a[:256], b), what=f"{mode} {'dgrad' if transposed else 'fwd'} {geom}")
    for (tm, _), per in stats.items():
        c0, (ps0, pq0) = next(iter(per.items()))
        for code, (ps, pq) in per.items():
            assert torch.equal(ps, ps0) and torch.equal(pq, pq0), f"{mode}: statistics of code {code:#x} differ from code {c0:#x}"
        mean, var = _chan_merge(ps0, pq0, tm, M)
        smean, svar = got.mean(0), got.var(0, unbiased=False)
        # fp32 shifted sums over <= 128 rows per block: a few 2^-24 of the column's scale
        assert float(((mean - smean).abs() / svar.sqrt()).max()) < 1e-5
        assert float(((var - svar).abs() / svar).max()) < 2e-5


WGEOMS = [
    (2, 11, 13, 272, 136, 1, 1, 1, 0, 0, 1),
    (2, 9, 10, 40, 200, 3, 3, 1, 1, 1, 1),
    (2, 11, 13, 72, 40, 1, 1, 1, 0, 0, 1),
    (2, 11, 13, 104, 104, 3, 3, 1, 1, 1, 1),
    (2, 12, 12, 32, 32, 3, 3, 1, 3, 3, 3),
    (2, 10, 14, 32, 32, 1, 7, 1, 0, 3, 1),
    (2, 16, 18, 56, 56, 3, 3, 2, 1, 1, 1),
    (3, 20, 20, 136, 200, 1, 1, 1, 0, 0, 1),
    (1, 5, 7, 16, 24, 3, 3, 1, 1, 1, 1),            # 35 pixels: 2 stages, the second 3 pixels deep
    (2, 9, 7, 8, 8, 1, 1, 1, 0, 0, 1),              # 126 pixels: a ragged last stage, 8 x 8 in a 32 x 128 tile
]


def _wsetup(geom, seed, slices):
    from pn2 import capi
    N, H, W, Cin, Cout, KH, KW, s, ph, pw, dil = geom
    OH = (H + 2 * ph - dil * (KH - 1) - 1) // s + 1
    OW = (W + 2 * pw - dil * (KW - 1) - 1) // s + 1
    g = torch.Generator().manual_seed(seed)
    ld_x, ld_dy = Cin + (16 if slices else 0), Cout + (8 if slices else 0)
    x = _randn((N * H * W, ld_x), g, slices)
    dy = _randn((N * OH * OW, ld_dy), g, slices)
    x[:, Cin:] = float("nan"); dy[:, Cout:] = float("nan")
    call = capi.call
    tco = call.pn2_wgrad_tile_co(Cout)
    wd = capi.WgradDesc()
    wd.N, wd.H, wd.W, wd.OH, wd.OW = N, H, W, OH, OW
    wd.Cin_p, wd.ld_x, wd.Cout_p, wd.ld_dy = Cin, ld_x, Cout, ld_dy
    wd.KH, wd.KW, wd.stride, wd.pad_h, wd.pad_w, wd.dil_h, wd.dil_w = KH, KW, s, ph, pw, dil, dil
    wd.Rp, wd.Kp = rup(Cout, tco), rup(KH * KW * Cin, 128)
    rd = capi.PackDesc()
    rd.Cout, rd.Cin, rd.KH, rd.KW = Cout, Cin, KH, KW
    rd.Cout_p, rd.gw_out, rd.gwp_out, rd.Cin_p, rd.gw_in, rd.gwp_in = Cout, Cout, Cout, Cin, Cin, Cin
    rd.Rp, rd.Kp, rd.transposed = wd.Rp, wd.Kp, 0
    geo = (N, H, W, OH, OW, Cin, KH, KW, s, ph, pw, dil, dil)
    return wd, rd, x, dy, geo


def _wgrad_check(mode, gw, slab, ns, ref, S, ref32, M, what, canary=None):
    """gw: OIHW fp32 result (device), slab: [ns, Rp, Kp] (device); gate: fp32ref.wgrad_tol"""
    Cout, Cin, KH, KW = gw.shape
    got = gw.double().cpu().permute(0, 2, 3, 1).reshape(Cout, KH * KW * Cin)
    sl = slab.double().cpu()[:, :Cout, :KH * KW * Cin]
    assert bool(torch.isfinite(got).all())
    err = (got - ref).abs()
    tol = R.wgrad_tol(mode, got, sl, ns, S, M)
    bad = err > tol
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} outside the {mode} gate, worst excess {float((err - tol).max()):.3g}"
    if mode == "F32F" and ref32 is not None:
        own = R.rms(ref32 - ref)
        ratio = R.rms(got - ref) / own
        print(f"{what}: rms(got - r) / rms(ref32 - r) = {ratio:.3f}")
        assert ratio <= 2.0, (what, ratio)
        if canary is not None:
            _canary(2 * own, *canary)
    elif canary is not None:
        _canary(R.rms(tol), *canary)


@pytest.mark.parametrize("geom", WGEOMS, ids=_ids(WGEOMS))
@pytest.mark.parametrize("mode", MODES)
def test_wgrad_splits_and_tunes_against_float64(mode, geom):
    """pn2_conv_wgrad + pn2_wgrad_reduce with 1, 3 and more pixel splits than 32-pixel stages (splits without work must still write zeros), tune 0 and 1
    (the same kernel for fp32: identical bits), NaN-poisoned slabs (every slab element of a live split is written) against the float64 weight gradient
    reduced over all pixels.  tune >= 2 (the bf16 LDS-DMA kernels) is rejected with -2."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    lib = _lib()
    dt = _mode(mode)
    wd, rd, x, dy, geo = _wsetup(geom, sum(geom) + 3, WGEOMS.index(geom) % 2 == 1)
    N, H, W, OH, OW, Cin, KH, KW = geo[:8]
    Cout = wd.Cout_p
    M = N * OH * OW
    stages = (M + 31) // 32
    xg, dyg = x.to(dev), dy.to(dev)
    co = list(range(Cout))
    ref, S = R.wgrad_rows(dy[:, :Cout].double(), x.double(), co, geo)
    # the reference's own fp32 weight gradient (torch CPU autograd in float32)
    w32 = torch.zeros(Cout, Cin, KH, KW, requires_grad=True)
    F.conv2d(x[:, :Cin].reshape(N, H, W, Cin).permute(0, 3, 1, 2), w32, None, geo[8], (geo[9], geo[10]), (geo[11], geo[12])).backward(
        dy[:, :Cout].reshape(N, OH, OW, Cout).permute(0, 3, 1, 2))
    ref32 = w32.grad.double().permute(0, 2, 3, 1).reshape(Cout, -1)
    res = {}
    for tune in (0, 1):
        for ns in sorted({1, 3, stages + 2}):
            wd.tune = tune
            slab = torch.full((ns, wd.Rp, wd.Kp), float("nan"), device=dev)
            gw = torch.full((Cout, Cin, KH, KW), float("nan"), device=dev)
            assert lib.pn2_conv_wgrad(dt, P(dyg), P(xg), P(slab), C.byref(wd), ns, _stream()) == 0
            assert lib.pn2_wgrad_reduce(P(slab), P(gw), C.byref(rd), ns, 0, _stream()) == 0
            torch.cuda.synchronize()
            assert bool(torch.isfinite(slab).all()), f"tune {tune}, {ns} splits: slab elements left unwritten"
            if ns > stages:
                assert bool((slab[stages:] == 0).all()), "splits without pixels must write zeros"
            _wgrad_check(mode, gw, slab, ns, ref, S, ref32, M, f"{mode} wgrad {geom} tune {tune} splits {ns}")
            res[(tune, ns)] = gw
    for ns in sorted({1, 3, stages + 2}):
        assert torch.equal(res[(0, ns)], res[(1, ns)]), f"tune 0 / 1 differ at {ns} splits (one kernel for fp32)"
    a = dy[:, :Cout].double()[:, :min(Cout, 64)].t()
    _canary(R.rms(R.gate_fp32(ref, ref, S, M)) if mode == "F32" else 2 * R.rms(ref32 - ref),
            a, R.gather(x.double(), torch.arange(M), geo, False).t()[:256])
    for tune in (2, 3):
        wd.tune = tune
        slab = torch.zeros((1, wd.Rp, wd.Kp), device=dev)
        assert lib.pn2_conv_wgrad(dt, P(dyg), P(xg), P(slab), C.byref(wd), 1, _stream()) == -2


# ---- epilogue entry points
EP_GEOM = (2, 12, 10, 40, 48, 3, 3, 1, 1, 1, 1)          # dgrad 48 -> 40 channels ... in forward terms: Cin 40, Cout 48


def _bn_operands(g, M, Cc):
    raw = torch.randn(M, Cc, generator=g)
    par = torch.empty(4, Cc)
    par[0] = torch.rand(Cc, generator=g) * 0.8 + 0.6
    par[1] = torch.randn(Cc, generator=g) * 0.3
    par[2] = torch.randn(Cc, generator=g) * 0.2
    par[3] = torch.rand(Cc, generator=g) * 0.8 + 0.6
    return raw, par


EP_FORMS = ["mask_y", "mask_raw", "no_mask", "dual", "accum", "pool"]


@pytest.mark.parametrize("form", EP_FORMS)
@pytest.mark.parametrize("mode", MODES)
def test_dgrad_batchnorm_backward_epilogue_against_float64(mode, form):
    """pn2_conv_gemm_ep in both fp32 modes: the stored gradient within the mode's gate (+ one rounding of the += for PN2_CONV_ACCUM / pool), the partial
    sums p1 = sum dz, p2 = invstd (sum dz raw - mean sum dz) over all rows against the float64 restatement (tests/test_gpu_baseline_shapes.py _expected_ep)
    of the STORED gradient.  The second BatchNorm (ep.c) is a bf16-only form: -2."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from test_gpu_baseline_shapes import _expected_ep
    from pn2 import capi
    lib = _lib()
    dt = _mode(mode)
    d, src, wp, n_out, M, ld_out, a, b, ref32, K = _setup(EP_GEOM, 1, mode, False, 11 + EP_FORMS.index(form))
    r = a @ b.t()
    S = a.abs() @ b.abs().t()
    g = torch.Generator().manual_seed(5 + EP_FORMS.index(form))
    amode = {"mask_y": 5, "mask_raw": 3, "no_mask": 1, "dual": 3, "accum": 5, "pool": 3}[form]
    accf = form in ("accum", "pool")
    d.flags = capi.CONV_ACCUM if accf else 0
    tm = _tile_m(mode, 0, M, n_out)
    nblk = (M + tm - 1) // tm
    ep = capi.ConvEp()
    keep = []

    def target(t, tmode):
        raw, par = _bn_operands(g, M, n_out)
        y = torch.randn(M, n_out, generator=g) if tmode & 4 else None
        p1 = torch.full((nblk, n_out), float("nan"), device=dev)
        p2 = torch.full((nblk, n_out), float("nan"), device=dev)
        rg, pg, yg = raw.to(dev), par.to(dev), (y.to(dev) if y is not None else None)
        t.mode, t.raw, t.ld_raw, t.par, t.ps = tmode, rg.data_ptr(), n_out, pg.data_ptr(), n_out
        if yg is not None:
            t.y, t.ld_y = yg.data_ptr(), n_out
        t.p1, t.p2, t.ldp = p1.data_ptr(), p2.data_ptr(), n_out
        keep.append((rg, pg, yg))
        return raw, par, y, p1, p2

    ta = target(ep.a, amode)
    prior, pool = None, None
    if form == "accum":
        prior = torch.randn(M, n_out, generator=g)
        out = prior.to(dev).clone()
        add = prior.double()
    elif form == "pool":
        N, OH, OW = d.N, d.OH, d.OW
        pool = torch.randn(N * (OH // 2) * (OW // 2), n_out + 4, generator=g)
        pool_g = pool.to(dev)
        ep.pool, ep.ld_pool = pool_g.data_ptr(), n_out + 4
        m = torch.arange(M)
        n_, rem = m // (OH * OW), m % (OH * OW)
        prow = (n_ * (OH // 2) + (rem // OW) // 2) * (OW // 2) + (rem % OW) // 2
        add = pool.double()[prow, :n_out] / 4
        out = torch.full((M, n_out), float("nan"), device=dev)
    else:
        out = torch.full((M, n_out), float("nan"), device=dev)
        add = None
    tb = None
    if form == "dual":
        tb = target(ep.b, 3)
        out_b = torch.full((M, n_out), float("nan"), device=dev)
        ep.b.out, ep.b.ld_out = out_b.data_ptr(), n_out
    assert lib.pn2_conv_gemm_ep(dt, P(src), P(wp), P(out), C.byref(d), C.byref(ep), _stream()) == 0
    torch.cuda.synchronize()
    got = out.double().cpu()
    if add is None:
        check(mode, got, r, S, K, ref32=ref32, what=f"{mode} ep {form}")
    else:          # got = fl(fl(conv) + prior): one more rounding of the conv result
        check(mode, got, r + add, S, K, extra=0.5 * R.spacing32(r), what=f"{mode} ep {form}")
    raw, par, y, p1, p2 = ta
    dz, e1, e2 = _expected_ep(got, raw, par, amode, y)
    s1, s2 = p1.double().cpu().sum(0), p2.double().cpu().sum(0)
    # fp32 sums over <= 128 rows per block and channel (fmaf chains), merged in float64 here
    assert float(((s1 - e1).abs() / (dz.abs().sum(0) + 1e-30)).max()) < 2e-5
    scale2 = par[3].double() * ((dz * raw.double()).abs().sum(0) + par[2].double().abs() * dz.abs().sum(0)) + 1e-30
    assert float(((s2 - e2).abs() / scale2).max()) < 2e-5
    if tb is not None:
        got_b = out_b.double().cpu()
        check(mode, got_b, r, S, K, what=f"{mode} ep dual, target b")
        assert torch.equal(out_b, out), "the second destination receives the plain result"
        raw, par, y, p1, p2 = tb
        dz, e1, e2 = _expected_ep(got_b, raw, par, 3, y)
        s1, s2 = p1.double().cpu().sum(0), p2.double().cpu().sum(0)
        assert float(((s1 - e1).abs() / (dz.abs().sum(0) + 1e-30)).max()) < 2e-5
        scale2 = par[3].double() * ((dz * raw.double()).abs().sum(0) + par[2].double().abs() * dz.abs().sum(0)) + 1e-30
        assert float(((s2 - e2).abs() / scale2).max()) < 2e-5
    if form == "no_mask":          # the bf16-only second BatchNorm (ep.c) is refused, not half-run
        ep.c.mode, ep.c.raw, ep.c.ld_raw, ep.c.par, ep.c.ps = 1, ep.a.raw, n_out, ep.a.par, n_out
        ep.c.p1, ep.c.p2, ep.c.ldp = ep.a.p1, ep.a.p2, n_out
        assert lib.pn2_conv_gemm_ep(dt, P(src), P(wp), P(out), C.byref(d), C.byref(ep), _stream()) == -2


@pytest.mark.parametrize("mode", MODES)
def test_gated_and_affine_epilogues_against_float64(mode):
    """pn2_conv_gemm_gated (out = (1 - sigmoid(gate[m])) conv(in)[m], statistics of the gated tile) and pn2_conv_gemm_affine (act(conv * scale + shift
    (+ residual)), ReLU / ReLU6) in both fp32 modes against float64.  The gate factor 1 - 1/(1 + exp(-gate)) is formed in fp32 with the hardware exp: 8 x 2^-24 of absolute slack on it."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from pn2 import capi
    lib = _lib()
    dt = _mode(mode)
    geom = (2, 13, 11, 72, 64, 1, 1, 1, 0, 0, 1)
    d, src, wp, n_out, M, ld_out, a, b, ref32, K = _setup(geom, 0, mode, False, 99)
    r = a @ b.t()
    S = a.abs() @ b.abs().t()
    g = torch.Generator().manual_seed(17)
    gate = torch.randn(M, generator=g) * 3
    gate_g = gate.to(dev)
    tm = _tile_m(mode, 0, M, n_out)
    nblk = (M + tm - 1) // tm
    ps = torch.full((nblk, n_out), float("nan"), device=dev); pq = torch.full((nblk, n_out), float("nan"), device=dev)
    out = torch.full((M, n_out), float("nan"), device=dev)
    d.flags = capi.CONV_STATS
    assert lib.pn2_conv_gemm_gated(dt, P(src), P(wp), P(out), P(ps), P(pq), C.byref(d), P(gate_g), _stream()) == 0
    torch.cuda.synchronize()
    fac = (1 - torch.sigmoid(gate.double()))[:, None]
    got = out.double().cpu()
    check(mode, got, fac * r, fac * S, K, extra=8 * R.U32 * r.abs(), what=f"{mode} gated")          # 1 - 1/(1 + e): absolute error of a few 2^-24
    mean, var = _chan_merge(ps, pq, tm, M)
    assert float(((mean - got.mean(0)).abs() / got.var(0, unbiased=False).sqrt()).max()) < 1e-5
    assert float(((var - got.var(0, unbiased=False)).abs() / got.var(0, unbiased=False)).max()) < 2e-5
    scale = torch.rand(n_out, generator=g) + 0.5
    shift = torch.randn(n_out, generator=g) * 0.5
    res = torch.randn(M, n_out, generator=g)
    sc_g, sh_g, res_g = scale.to(dev), shift.to(dev), res.to(dev)
    sc, sh = scale.double(), shift.double()
    for act in (0, capi.CONV_RELU, capi.CONV_RELU6):
        for with_res in (False, True):
            d.flags = capi.CONV_AFFINE | act
            out = torch.full((M, n_out), float("nan"), device=dev)
            assert lib.pn2_conv_gemm_affine(dt, P(src), P(wp), P(out), P(sc_g), P(sh_g), P(res_g) if with_res else P(None), n_out, C.byref(d), _stream()) == 0
            torch.cuda.synchronize()
            want = r * sc + sh + (res.double() if with_res else 0)
            if act:
                want = want.clamp(min=0)
            if act == capi.CONV_RELU6:
                want = want.clamp(max=6)
            # fp32: fl(conv) -> fmaf(., scale, shift) (-> + residual): the conv's gate scaled by |scale|, plus one ulp of the result per later rounding
            got = out.double().cpu()
            base = R.gate_fp32(r.float().double(), r, S, K) if mode == "F32" else R.gate_fp32fast(S, K) + 0.5 * R.spacing32(r)
            tol = base * sc.abs() + R.spacing32(r * sc + sh) + R.spacing32(got)
            assert bool(torch.isfinite(got).all())
            bad = (got - want).abs() > tol
            assert not bool(bad.any()), (mode, act, with_res, int(bad.sum()), float(((got - want).abs() - tol).max()))


# ---- table-driven launches
@pytest.mark.parametrize("mode", MODES)
def test_table_launches_match_single_launches_bitwise(mode):
    """pn2_conv_gemm_multi (ep = 0, 1, 2, 3: plain jobs, jobs with a BatchNorm-backward epilogue, the bf16 LDS hints ignored) and pn2_conv_wgrad_multi (every
    variant pn2_conv_wgrad_variant returns on WGEOMS) against one launch per job: bit for bit.  fp32fast refuses 128-wide tiles in a table (-2)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from pn2 import capi
    from pn2.engine import _job_table, _p
    lib = _lib()
    dt = _mode(mode)
    g = torch.Generator().manual_seed(77)
    # (N, H, W, Cin_p, Cout, KH, KW, ph, pw, dil, ld_in, off_in, ld_out, off_out, transposed)
    specs = [(2, 12, 12, 32, 32, 1, 3, 0, 1, 1, 224, 32, 32, 0, 0), (2, 12, 12, 32, 32, 3, 3, 3, 3, 3, 32, 0, 256, 64, 0),
             (2, 6, 6, 32, 64, 3, 3, 5, 5, 5, 32, 0, 256, 128, 0), (2, 3, 3, 32, 32, 1, 7, 0, 3, 1, 416, 96, 32, 0, 0),
             (2, 6, 6, 64, 64, 5, 1, 2, 0, 1, 64, 0, 64, 0, 1), (3, 24, 24, 64, 32, 1, 1, 0, 0, 1, 64, 0, 32, 0, 1), (1, 5, 7, 1024, 64, 1, 1, 0, 0, 1, 1024, 0, 64, 0, 0)]
    codes = [0] if mode == "F32" else [0, 1 | (1 << 2) | (1 << 4), 1 | (2 << 2) | (2 << 4), 2 | (1 << 2) | (3 << 4)]
    for code in codes:
        for epb in (0, 1, 2, 3):
            with_ep = epb & 1
            singles, structs, multis, keep = [], [], [], []
            for N, H, W, Cin_p, Cout, KH, KW, ph, pw, dil, ld_in, off_in, ld_out, off_out, tr in specs:
                d = capi.ConvDesc()
                d.N, d.H, d.W, d.OH, d.OW = N, H, W, H, W
                d.Cin_p, d.ld_in, d.Cout, d.ld_out = Cin_p, ld_in, Cout, ld_out
                d.KH, d.KW, d.stride, d.pad_h, d.pad_w, d.dil_h, d.dil_w = KH, KW, 1, ph, pw, dil, dil
                d.transposed, d.Kp = tr, rup(KH * KW * Cin_p, 128)
                d.flags = (code << 8) | (capi.CONV_STATS if not (with_ep or tr) else 0) | (capi.CONV_ACCUM if with_ep and tr else 0)
                M = N * H * W
                x = torch.randn(M, ld_in, generator=g).to(dev)[:, off_in:]
                wp = (torch.randn(rup(Cout, 128), d.Kp, generator=g) * 0.1).to(dev)
                tile = lib.pn2_conv_gemm_tile(dt, C.byref(d))
                assert tile > 0
                bm = tile >> 8
                nb = (M + bm - 1) // bm
                ep = capi.ConvEp()
                if with_ep:
                    raw, par = _bn_operands(g, M, Cout)
                    y = torch.randn(M, Cout, generator=g)
                    rg, pg, yg = raw.to(dev), par.to(dev), y.to(dev)
                    ep.a.mode, ep.a.raw, ep.a.ld_raw, ep.a.par, ep.a.ps, ep.a.y, ep.a.ld_y = 5, rg.data_ptr(), Cout, pg.data_ptr(), Cout, yg.data_ptr(), Cout
                    keep.append((rg, pg, yg))
                prior = torch.randn(M, ld_out, generator=g).to(dev)
                res = []
                for rep in range(2):
                    o = prior.clone()[:, off_out:]
                    ps = torch.zeros(nb, Cout, device=dev); pq = torch.zeros(nb, Cout, device=dev)
                    e = capi.ConvEp()
                    C.memmove(C.byref(e), C.byref(ep), C.sizeof(ep))
                    if with_ep:
                        e.a.p1, e.a.p2, e.a.ldp = ps.data_ptr(), pq.data_ptr(), Cout
                    res.append((o, ps, pq, e))
                o, ps, pq, e = res[0]
                if with_ep:
                    assert lib.pn2_conv_gemm_ep(dt, P(x), P(wp), P(o), C.byref(d), C.byref(e), _stream()) == 0
                else:
                    assert lib.pn2_conv_gemm(dt, P(x), P(wp), P(o), P(ps) if not tr else P(None), P(pq) if not tr else P(None), C.byref(d), _stream()) == 0
                singles.append(res[0][:3])
                o2, ps2, pq2, e2 = res[1]
                j = capi.ConvJob()
                j.in_, j.wp, j.out = x.data_ptr(), wp.data_ptr(), o2.data_ptr()
                j.psum, j.psq = (ps2.data_ptr(), pq2.data_ptr()) if not (with_ep or tr) else (None, None)
                C.memmove(C.byref(j.d), C.byref(d), C.sizeof(d))
                C.memmove(C.byref(j.ep), C.byref(e2), C.sizeof(e2))
                structs.append((tile, j, lib.pn2_conv_gemm_job_blocks(dt, C.byref(j), bm, tile & 255)))
                multis.append(res[1][:3])
                keep.append((x, wp, prior))
            for tile in sorted({t for t, _, _ in structs}):
                sel = [(j, nb) for t, j, nb in structs if t == tile]
                table, bstart, total = _job_table(capi.ConvJob, [j for j, _ in sel], [nb for _, nb in sel])
                assert lib.pn2_conv_gemm_multi(dt, tile >> 8, tile & 255, epb, _p(table), _p(bstart), len(sel), total, _stream()) == 0
                keep.append((table, bstart))
            torch.cuda.synchronize()
            for i, (a_, b_) in enumerate(zip(singles, multis)):
                assert torch.equal(a_[0], b_[0]), (mode, hex(code), epb, i, "output")
                assert torch.equal(a_[1], b_[1]) and torch.equal(a_[2], b_[2]), (mode, hex(code), epb, i, "statistics")
    # 128-wide tiles: never chosen for 4-byte types, refused by the table launch
    dummy = torch.zeros(64, dtype=torch.int32, device=dev)          # (never read: the tile is refused before any launch)
    assert lib.pn2_conv_gemm_multi(dt, 64, 128, 0, P(dummy), P(dummy), 1, 1, _stream()) == -2
    assert lib.pn2_conv_gemm_multi(dt, 128, 128, 1, P(dummy), P(dummy), 1, 1, _stream()) == -2
    # weight gradients: every variant of the geometry set, one table per variant, against single launches
    byv = {}
    for geom in WGEOMS:
        wd, rd, x, dy, geo = _wsetup(geom, sum(geom), True)
        ns = 3
        v = lib.pn2_conv_wgrad_variant(dt, C.byref(wd))
        assert v >= 0
        xg, dyg = x.to(dev), dy.to(dev)
        s1 = torch.full((ns, wd.Rp, wd.Kp), float("nan"), device=dev)
        s2 = torch.full_like(s1, float("nan"))
        assert lib.pn2_conv_wgrad(dt, P(dyg), P(xg), P(s1), C.byref(wd), ns, _stream()) == 0
        j = capi.WgradJob()
        j.dy, j.x, j.slab, j.nsplit, j.rot = dyg.data_ptr(), xg.data_ptr(), s2.data_ptr(), ns, len(byv.get(v, [])) % 8
        C.memmove(C.byref(j.d), C.byref(wd), C.sizeof(wd))
        byv.setdefault(v, []).append((j, lib.pn2_conv_wgrad_blocks(C.byref(wd), ns), s1, s2, xg, dyg))
    assert len(byv) >= 3, sorted(byv)
    keep = []
    for v, jobs in byv.items():
        table, bstart, total = _job_table(capi.WgradJob, [j for j, *_ in jobs], [nb for _, nb, *_ in jobs])
        assert lib.pn2_conv_wgrad_multi(dt, v, _p(table), _p(bstart), len(jobs), total, _stream()) == 0
        keep.append((table, bstart))
    torch.cuda.synchronize()
    for v, jobs in byv.items():
        for i, (_, _, s1, s2, _, _) in enumerate(jobs):
            assert torch.equal(s1, s2), (mode, "wgrad variant", v, i)
