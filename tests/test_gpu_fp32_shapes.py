"""Every fp32fast entry of the shipped tuning table (pn2/tuned_gfx950.json, keys ending in 'f32f') launched at the benchmark shape it was timed for, as the
engine launches it, against float64 - and the plain forward / dgrad / weight-gradient geometries of those entries in fp32 (no tuning code).

A table entry only applies at its benchmark shape (bs 32, 11^2 .. 352^2), so none of them is active in the small-geometry tests.  What only exists
there - grids of thousands of tiles, channel slices of wider buffers, statistics over 10^5 .. 10^6 rows, pixel splits from 3 to 640 - is verified here.
The parametrization is read from the table: a retune is covered without editing this file.

Per case: operands are fp32 randn generated on the device from a seeded generator; every destination is NaN-poisoned and must come back finite (every
tile written).  The float64 reference (tests/fp32ref.py) is computed for SAMPLED rows - the first and last 128 plus one seeded row in every 64-row block,
all columns - so that every (row tile, column tile) pair has a checked row; the weight gradient for one seeded co row in every co tile plus the first and
last, all k columns, reduced over ALL pixels.  Epilogue sums and BatchNorm partials are checked over all rows against the stored output.
Gates (tests/test_gpu_convkernels_fp32.py): fp32 correct rounding + double-sum slack; fp32fast the worst-case bound of its summation structure and
rms(got - r) <= 2 rms(ref32 - r), ref32 = a CPU float32 GEMM of the same gathered operands (torch's CPU conv arithmetic on the im2col operand)."""
import ctypes as C
import json
import os, sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "pranet-v2_amd"))
import fp32ref as R  # noqa: E402
from fp32ref import rup  # noqa: E402

dev = "cuda"
TABLE = R.table_codes(json.load(open(os.path.join(ROOT, "pranet-v2_amd", "pn2", "tuned_gfx950.json"))))
CASES = [(k, "F32F") for k in TABLE] + [(k[:-1], "F32") for k in TABLE if "ep" not in k]
RATIOS = {}


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _seed(key):
    return sum((i + 1) * (v if isinstance(v, int) else len(v)) for i, v in enumerate(key)) % 100003


def _ratio(mode, key, got, r, ref32):
    if mode != "F32F":
        return
    own = R.rms(ref32 - r)
    ratio = R.rms(got - r) / own
    RATIOS[key] = ratio
    print(f"{R.key_id(key)}: rms ratio {ratio:.3f}")
    assert ratio <= 2.0, ratio


def _gate(mode, got, r, S, K, extra=None):
    err = (got - r).abs()
    if mode == "F32":
        tol = R.gate_fp32(got, r, S, K, extra)
    else:
        tol = R.gate_fp32fast(S, K) + 0.5 * R.spacing32(got) + (extra if extra is not None else 0)
    bad = err > tol
    assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} elements outside the {mode} gate, worst excess {float((err - tol).max()):.3g}"
    return tol


def _canary(tol_rms, a, b):
    ebf = R.bf16_error(a, b)
    assert tol_rms * 10 <= ebf, (tol_rms, ebf)


def _bn_operands(g, M, Cc):
    raw = torch.randn(M, Cc, generator=g, device=dev)
    par = torch.empty(4, Cc, device=dev)
    par[0] = torch.rand(Cc, generator=g, device=dev) * 0.8 + 0.6
    par[1] = torch.randn(Cc, generator=g, device=dev) * 0.3
    par[2] = torch.randn(Cc, generator=g, device=dev) * 0.2
    par[3] = torch.rand(Cc, generator=g, device=dev) * 0.8 + 0.6
    return raw, par


@pytest.mark.parametrize("key,mode", CASES, ids=[f"{m}-{R.key_id(k)}" for k, m in CASES])
def test_shipped_entry_at_its_benchmark_shape(key, mode):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from pn2 import capi, engine
    from pn2.capi import F32, F32F
    lib = capi.load()
    dt = F32F if mode == "F32F" else F32
    if mode == "F32F":
        assert engine.TUNER.get(key) == TABLE[key], "the shipped table is not what the engine has loaded (PN2_TUNE_TABLE=0 / PN2_TUNE_CACHE set?)"
    g = torch.Generator(device=dev).manual_seed(_seed(key))
    if key[0] == "w":
        return _wgrad_case(key, mode, dt, lib, g)
    code = TABLE[key] if mode == "F32F" else 0
    _, N, H, W, OH, OW, Cin_p, ld_in, Cout, KH, KW, s, ph, pw, dh, dw, tr = key[:17]
    ep_key = key[18:22] if len(key) > 18 and key[17] == "ep" else None
    pool = "pool" in key
    taps, K, M = KH * KW, KH * KW * Cin_p, N * OH * OW
    src = torch.randn(N * H * W, ld_in, generator=g, device=dev)
    src[:, Cin_p:] = float("nan")
    d = capi.ConvDesc()
    d.N, d.H, d.W, d.OH, d.OW = N, H, W, OH, OW
    d.Cin_p, d.ld_in, d.Cout, d.ld_out = Cin_p, ld_in, Cout, Cout
    d.KH, d.KW, d.stride, d.pad_h, d.pad_w, d.dil_h, d.dil_w = KH, KW, s, ph, pw, dh, dw
    d.transposed, d.Kp = tr, rup(K, 128)
    wp = torch.zeros(rup(Cout, 128), d.Kp, device=dev)
    wp[:Cout, :K] = torch.randn(Cout, K, generator=g, device=dev) * (2.0 / K) ** 0.5
    bm = (code >> 2) & 3
    tm = (64 if bm == 1 else 128) if bm else lib.pn2_conv_tile_m(M, Cout, dt)
    nblk = (M + tm - 1) // tm
    out = torch.full((M, Cout), float("nan"), device=dev)
    add = None
    if ep_key is None:
        stats = not tr
        ps = torch.full((nblk, Cout), float("nan"), device=dev) if stats else None
        pq = torch.full((nblk, Cout), float("nan"), device=dev) if stats else None
        d.flags = (capi.CONV_STATS if stats else 0) | (code << 8)
        assert lib.pn2_conv_gemm(dt, P(src), P(wp), P(out), P(ps), P(pq), C.byref(d), _stream()) == 0
    else:
        amode, bmode, dual, accf = ep_key
        d.flags = (capi.CONV_ACCUM if accf else 0) | (code << 8)
        ep = capi.ConvEp()
        keep = []

        def target(t, tmode):
            raw, par = _bn_operands(g, M, Cout)
            y = torch.randn(M, Cout, generator=g, device=dev) if tmode & 4 else None
            p1 = torch.full((nblk, Cout), float("nan"), device=dev)
            p2 = torch.full((nblk, Cout), float("nan"), device=dev)
            t.mode, t.raw, t.ld_raw, t.par, t.ps = tmode, raw.data_ptr(), Cout, par.data_ptr(), Cout
            if y is not None:
                t.y, t.ld_y = y.data_ptr(), Cout
            t.p1, t.p2, t.ldp = p1.data_ptr(), p2.data_ptr(), Cout
            keep.append((raw, par, y))
            return raw, par, y, p1, p2

        ta = target(ep.a, amode)
        if pool:
            pl = torch.randn(N * (OH // 2) * (OW // 2), Cout, generator=g, device=dev)
            ep.pool, ep.ld_pool = pl.data_ptr(), Cout
            m = torch.arange(M, device=dev)
            n_, rem = m // (OH * OW), m % (OH * OW)
            add = pl[(n_ * (OH // 2) + (rem // OW) // 2) * (OW // 2) + (rem % OW) // 2] / 4
        elif accf:
            prior = torch.randn(M, Cout, generator=g, device=dev)
            out.copy_(prior)
            add = prior
        tb = None
        if dual:
            tb = target(ep.b, bmode)
            out_b = torch.full((M, Cout), float("nan"), device=dev)
            ep.b.out, ep.b.ld_out = out_b.data_ptr(), Cout
        assert lib.pn2_conv_gemm_ep(dt, P(src), P(wp), P(out), C.byref(d), C.byref(ep), _stream()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()), "output elements left unwritten (or NaN channels read)"
    # ---- sampled rows against float64
    rows = R.sample_rows(M, _seed(key)).to(dev)
    geo = (N, H, W, OH, OW, Cin_p, KH, KW, s, ph, pw, dh, dw)
    a = R.gather(src, rows, geo, tr).cpu()
    b = wp[:Cout, :K].cpu()
    a64, b64 = a.double(), b.double()
    r = a64 @ b64.t()
    S = a64.abs() @ b64.abs().t()
    ref32 = (a @ b.t()).double()
    got = out[rows].double().cpu()
    if add is None:
        tol = _gate(mode, got, r, S, K)
        _ratio(mode, key, got, r, ref32)
    else:
        tol = _gate(mode, got, r + add[rows].double().cpu(), S, K, extra=0.5 * R.spacing32(r))
        _ratio(mode, key, got - add[rows].double().cpu(), r, ref32)
    sub = slice(0, 256)
    _canary(R.rms(tol[sub]) if mode == "F32" else 2 * R.rms((ref32 - r)[sub]), a64[sub], b64)
    o64 = out.double()
    if ep_key is None and not tr:
        # BatchNorm partials (mean, M2 per row block): Chan merge over all rows == mean / biased variance of the stored output
        n_t = torch.full((nblk,), float(tm), dtype=torch.float64, device=dev); n_t[-1] = M - (nblk - 1) * tm
        mean_t, m2_t = ps.double(), pq.double()
        mean = (mean_t * n_t[:, None]).sum(0) / M
        var = (m2_t.sum(0) + (n_t[:, None] * (mean_t - mean) ** 2).sum(0)) / M
        smean, svar = o64.mean(0), o64.var(0, unbiased=False)
        assert float(((mean - smean).abs() / svar.sqrt()).max()) < 1e-5
        assert float(((var - svar).abs() / svar).max()) < 2e-5
    if ep_key is not None:
        from test_gpu_baseline_shapes import _expected_ep
        for t, tgt, mode_t in ((ta, o64, amode),) + (((tb, out_b.double(), bmode),) if tb is not None else ()):
            raw, par, y, p1, p2 = t
            dz, e1, e2 = _expected_ep(tgt, raw, par, mode_t, y)
            s1, s2 = p1.double().sum(0), p2.double().sum(0)
            assert float(((s1 - e1).abs() / (dz.abs().sum(0) + 1e-30)).max()) < 2e-5
            scale2 = par[3].double() * ((dz * raw.double()).abs().sum(0) + par[2].double().abs() * dz.abs().sum(0)) + 1e-30
            assert float(((s2 - e2).abs() / scale2).max()) < 2e-5
        if tb is not None:
            assert torch.equal(out_b, out) or accf, "the second destination receives the plain result"


def _wgrad_case(key, mode, dt, lib, g):
    from pn2 import capi
    from pn2.capi import call
    _, N, H, W, OH, OW, Cin_p, ld_x, Cout_p, ld_dy, KH, KW, s, ph, pw, dh, dw, heur = key[:18]
    kern, ns = TABLE[key] if mode == "F32F" else (0, heur)
    M, K = N * OH * OW, KH * KW * Cin_p
    x = torch.randn(N * H * W, ld_x, generator=g, device=dev)
    x[:, Cin_p:] = float("nan")
    dy = torch.randn(M, ld_dy, generator=g, device=dev)
    dy[:, Cout_p:] = float("nan")
    tco = call.pn2_wgrad_tile_co(Cout_p)
    wd = capi.WgradDesc()
    wd.N, wd.H, wd.W, wd.OH, wd.OW = N, H, W, OH, OW
    wd.Cin_p, wd.ld_x, wd.Cout_p, wd.ld_dy = Cin_p, ld_x, Cout_p, ld_dy
    wd.KH, wd.KW, wd.stride, wd.pad_h, wd.pad_w, wd.dil_h, wd.dil_w = KH, KW, s, ph, pw, dh, dw
    wd.Rp, wd.Kp, wd.tune = rup(Cout_p, tco), rup(K, 128), kern
    rd = capi.PackDesc()
    rd.Cout, rd.Cin, rd.KH, rd.KW = Cout_p, Cin_p, KH, KW
    rd.Cout_p, rd.gw_out, rd.gwp_out, rd.Cin_p, rd.gw_in, rd.gwp_in = Cout_p, Cout_p, Cout_p, Cin_p, Cin_p, Cin_p
    rd.Rp, rd.Kp, rd.transposed = wd.Rp, wd.Kp, 0
    slab = torch.full((ns, wd.Rp, wd.Kp), float("nan"), device=dev)
    gw = torch.full((Cout_p, Cin_p, KH, KW), float("nan"), device=dev)
    assert lib.pn2_conv_wgrad(dt, P(dy), P(x), P(slab), C.byref(wd), ns, _stream()) == 0
    assert lib.pn2_wgrad_reduce(P(slab), P(gw), C.byref(rd), ns, 0, _stream()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(slab).all()), "slab elements left unwritten"
    assert bool(torch.isfinite(gw).all())
    # one seeded co row in every co tile, plus the first and the last
    gen = torch.Generator().manual_seed(_seed(key))
    co = sorted({0, Cout_p - 1} | {min(Cout_p - 1, t0 + int(torch.randint(0, tco, (1,), generator=gen))) for t0 in range(0, Cout_p, tco)})
    geo = (N, H, W, OH, OW, Cin_p, KH, KW, s, ph, pw, dh, dw)
    ref, S = R.wgrad_rows(dy[:, :Cout_p], x, co, geo)
    # the reference's own arithmetic: CPU float32 sums over pixel chunks
    ref32 = torch.zeros(len(co), K)
    cot = torch.tensor(co, device=dev)
    for m0 in range(0, M, 1 << 16):
        rws = torch.arange(m0, min(M, m0 + (1 << 16)), device=dev)
        ref32 += dy[rws][:, cot].cpu().t() @ R.gather(x, rws, geo, False).cpu()
    ref, S, ref32 = ref.cpu(), S.cpu(), ref32.double()
    got = gw.permute(0, 2, 3, 1).reshape(Cout_p, K)[cot].double().cpu()
    sl = slab[:, cot, :K].double().cpu()
    err = (got - ref).abs()
    tol = R.wgrad_tol(mode, got, sl, ns, S, M)
    bad = err > tol
    assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} outside the {mode} gate, worst excess {float((err - tol).max()):.3g}"
    _ratio(mode, key, got, ref, ref32)
    if mode == "F32F":
        a = dy[:4096, :Cout_p][:, cot].double().cpu().t()
        _canary(2 * R.rms(ref32 - ref) * (4096 / M) ** 0.5, a, R.gather(x, torch.arange(min(M, 4096), device=dev), geo, False).double().cpu().t()[:256])
