"""Kernel / tile selection and refusal codes of the conv launch layer (pranet-v2_amd/csrc/pn2_conv.hip), pinned against a recorded fixture.

The selection helpers of the library are pure host code: they run without a device.  A fixed sweep of descriptors goes through them, and through
the launching entry points with argument sets that are refused BEFORE any launch (null pointers, misaligned descriptors, unknown dtype / variant /
tile, flag combinations an entry point does not take); every result must equal tests/golden/conv_select.json.  The fixture is recorded with the same
sweep from a library build that is known good (PN2_LIB selects the build):

    PN2_LIB=/path/to/libpn2_hip.so python tests/test_conv_select_cpu.py --record

A change of the launch / dispatch code that keeps behaviour leaves this test green without re-recording."""
import ctypes as C
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "conv_select.json")
if __name__ == "__main__":          # (under pytest, conftest.py has set the path)
    sys.path[:0] = [ROOT, os.path.join(ROOT, "pranet-v2_amd")]

M_LIST = (1, 64, 65, 128, 129, 1000, 4096, 8191, 8192, 12288, 20480, 24576, 40000, 65536, 1 << 18, 1 << 20)
COUTS = (8, 32, 56, 64, 96, 128, 208, 256, 2048)
DTYPES = (0, 1, 2, 3, 7)          # PN2_F32, PN2_BF16, PN2_F32F, PN2_F32X3 and a code the library does not know
PTR = C.c_void_p(4096)            # a non-null pointer for calls that are refused before anything reads it


def tune_codes():
    """Every tuning code pn2/ops_conv.py can put into flags bits 8..15 (kernel | BM << 2 | BN << 4, | 0x40 / 0x80 for the intra-workgroup split-K
    classes), the codes around them that the library has to fall through on, and 0 (library heuristic)."""
    plain = [k | (bm << 2) | (bn << 4) for k in (1, 2, 3) for bm in (1, 2) for bn in (1, 2, 3)]
    codes = [0] + plain
    codes += [c | 0x40 for c in plain] + [c | 0x80 for c in plain]
    codes += [3 | (1 << 2) | (2 << 4) | 0xC0, 2 | (2 << 2) | (3 << 4) | 0xC0, 0x40, 0x80, 2, 3, 3 << 2, 3 << 4]
    return codes


def conv_desc(capi, M, cout, tune=0, ksplit=0, flags=0, cin_p=64, ld_in=None, kp=None, stride=1, k=1):
    d = capi.ConvDesc()
    d.N, d.H, d.W, d.OH, d.OW = 1, M, 1, M, 1
    d.Cin_p, d.ld_in, d.Cout, d.ld_out = cin_p, cin_p if ld_in is None else ld_in, cout, cout
    d.KH = d.KW = k
    d.stride, d.pad_h, d.pad_w, d.dil_h, d.dil_w = stride, k // 2, k // 2, 1, 1
    d.Kp = -(-cout // 128) * 128 if kp is None else kp
    d.flags = flags | (tune << 8) | (ksplit << 16)
    return d


def wgrad_desc(capi, M, cout_p, k=1, tune=0, kp=128, ld=None, rp=None, cin_p=64, stride=1):
    d = capi.WgradDesc()
    d.N, d.H, d.W, d.OH, d.OW = 1, M, 1, M, 1
    d.Cin_p, d.ld_x, d.Cout_p, d.ld_dy = cin_p, cin_p if ld is None else ld, cout_p, cout_p if ld is None else ld
    d.KH = d.KW = k
    d.stride, d.pad_h, d.pad_w, d.dil_h, d.dil_w = stride, k // 2, k // 2, 1, 1
    bmc = 128 if cout_p > 64 else (64 if cout_p > 32 else 32)
    d.Rp, d.Kp, d.tune = (-(-cout_p // bmc) * bmc if rp is None else rp), kp, tune
    return d


def pack_desc(capi, cout, cin, k):
    p = capi.PackDesc()
    p.Cout, p.Cin, p.KH, p.KW = cout, cin, k, k
    p.Cout_p, p.Cin_p = -(-cout // 8) * 8, -(-cin // 8) * 8
    p.gw_out = p.gwp_out = p.Cout_p
    p.gw_in = p.gwp_in = p.Cin_p
    p.Rp, p.Kp, p.ld = -(-p.Cout_p // 32) * 32, -(-(k * k * p.Cin_p) // 128) * 128, -(-(k * k * p.Cin_p) // 128) * 128
    return p


def sweep(capi):
    """section name -> list of results, in a fixed order"""
    lib = capi.load()
    out = {}
    out["tile_n"] = [lib.pn2_conv_tile_n(c) for c in range(1, 300)] + [lib.pn2_conv_tile_n(c) for c in COUTS]
    out["tile_m"] = [lib.pn2_conv_tile_m(m, c, dt) for m in M_LIST for c in COUTS for dt in DTYPES]
    out["stat_blocks"] = [lib.pn2_conv_stat_blocks(m, c, dt) for m in M_LIST for c in COUTS for dt in DTYPES]

    # ---- pn2_conv_gemm_tile: the whole of gemm_select behind it
    codes = tune_codes()
    out["gemm_tile"] = [lib.pn2_conv_gemm_tile(dt, C.byref(conv_desc(capi, m, c, tune=t))) for m in M_LIST for c in COUTS for dt in DTYPES for t in codes]
    r = []
    for dt in DTYPES:
        r.append(lib.pn2_conv_gemm_tile(dt, None))
        for ks in range(2, 16):          # external split-K launches never join a table
            r.append(lib.pn2_conv_gemm_tile(dt, C.byref(conv_desc(capi, 121, 256, tune=2 | (1 << 2) | (3 << 4), ksplit=ks))))
        for kw in (dict(cin_p=12), dict(ld_in=68), dict(kp=64), dict(stride=3), dict(stride=8), dict(stride=16)):
            r.append(lib.pn2_conv_gemm_tile(dt, C.byref(conv_desc(capi, 4096, 64, **kw))))
        # operands around the 2 GB extent of the LDS-DMA kernels' buffer descriptor ((pixels - 1) * ld_in * 2 + Cin_p * 2 < 2^31)
        for m, ld, cin in ((1 << 19, 2048, 1024), (1 << 19, 2048, 2048), (1 << 20, 1024, 1024), (1 << 20, 2048, 64), (1 << 20, 4096, 64)):
            for t in (0, 2 | (2 << 2) | (3 << 4), 3 | (1 << 2) | (2 << 4) | 0x40, 1 | (1 << 2) | (1 << 4)):
                r.append(lib.pn2_conv_gemm_tile(dt, C.byref(conv_desc(capi, m, 256, tune=t, cin_p=cin, ld_in=ld))))
    out["gemm_tile_edges"] = r

    # ---- pn2_conv_gemm_job_blocks
    r = []
    for dt in DTYPES:
        for m in (1, 129, 8192, 1 << 20):
            for c in (8, 96, 256):
                for bm, bn in ((128, 128), (64, 32), (0x100 | 64, 128), (0x100 | 128, 64), (0, 64), (64, 0)):
                    j = capi.ConvJob()
                    j.in_, j.wp, j.out, j.d = PTR, PTR, PTR, conv_desc(capi, m, c)
                    r.append(lib.pn2_conv_gemm_job_blocks(dt, C.byref(j), bm, bn))
        for flags, psum, psq, mode_a, res, ld_y in ((capi.CONV_STATS, None, None, 0, None, 0), (capi.CONV_STATS, PTR, PTR, 0, None, 0), (capi.CONV_BIAS, None, None, 0, None, 0),
                                                    (capi.CONV_BIAS, PTR, None, 0, None, 0), (capi.CONV_AFFINE, None, None, 0, None, 0), (capi.CONV_AFFINE, PTR, PTR, 0, None, 0),
                                                    (capi.CONV_AFFINE | capi.CONV_ACCUM, PTR, PTR, 0, None, 0), (capi.CONV_AFFINE, PTR, PTR, 1, None, 0),
                                                    (capi.CONV_AFFINE, PTR, PTR, 0, PTR, 12), (capi.CONV_AFFINE, PTR, PTR, 0, PTR, 16), (0, None, None, 1, None, 0),
                                                    (capi.CONV_STATS, PTR, PTR, 1, None, 0)):
            for c in (64, 60):
                j = capi.ConvJob()
                j.in_, j.wp, j.out, j.psum, j.psq, j.d = PTR, PTR, PTR, psum, psq, conv_desc(capi, 4096, c, flags=flags)
                j.ep.a.mode, j.ep.a.y, j.ep.a.ld_y = mode_a, res, ld_y
                r.append(lib.pn2_conv_gemm_job_blocks(dt, C.byref(j), 64, 64))
        r.append(lib.pn2_conv_gemm_job_blocks(dt, None, 64, 64))
        j = capi.ConvJob()
        r.append(lib.pn2_conv_gemm_job_blocks(dt, C.byref(j), 64, 64))          # null operands
    out["gemm_job_blocks"] = r

    # ---- wgrad: variant and grid
    var, blk = [], []
    for m in (1, 4096, 8191, 8192, 65536, 1 << 20):
        for cp in COUTS:
            for k in (1, 3):
                for tune in (0, 1, 2, 3):
                    for kp in (128, 256, 384):
                        d = wgrad_desc(capi, m, cp, k=k, tune=tune, kp=kp)
                        var += [lib.pn2_conv_wgrad_variant(dt, C.byref(d)) for dt in DTYPES]
                        blk += [lib.pn2_conv_wgrad_blocks(C.byref(d), ns) for ns in (1, 7, 8, 9, 64)]
    for ld in (512, 1024, 2048):          # operand extents around 2 GB: the DMA kernels step aside
        for tune in (0, 2, 3):
            d = wgrad_desc(capi, 1 << 20, 256, tune=tune, kp=256, ld=ld)
            var += [lib.pn2_conv_wgrad_variant(dt, C.byref(d)) for dt in DTYPES]
            blk.append(lib.pn2_conv_wgrad_blocks(C.byref(d), 8))
    d = wgrad_desc(capi, 4096, 64, k=1, stride=2)          # 1 x 1 but strided: not pointwise
    var += [lib.pn2_conv_wgrad_variant(dt, C.byref(d)) for dt in DTYPES] + [lib.pn2_conv_wgrad_variant(dt, None) for dt in DTYPES]
    blk += [lib.pn2_conv_wgrad_blocks(None, 1), lib.pn2_conv_wgrad_blocks(C.byref(d), 0), lib.pn2_conv_wgrad_blocks(C.byref(wgrad_desc(capi, 4096, 96, rp=96)), 1),
            lib.pn2_conv_wgrad_blocks(C.byref(wgrad_desc(capi, 4096, 96, kp=192)), 1)]
    out["wgrad_variant"], out["wgrad_blocks"] = var, blk

    # ---- weight packing / split reduction grids
    pk, rd = [], []
    for cout in (1, 8, 33, 64, 256, 2048):
        for cin in (1, 3, 64, 100, 2048):
            for k in (1, 3, 5, 7, 15, 16):
                p = pack_desc(capi, cout, cin, k)
                pk.append(lib.pn2_pack_blocks(C.byref(p)))
                rd.append(lib.pn2_wgrad_reduce_blocks(C.byref(p)))
    out["pack_blocks"], out["reduce_blocks"] = pk + [lib.pn2_pack_blocks(None)], rd + [lib.pn2_wgrad_reduce_blocks(None)]

    out["refusals"] = refusals(capi, lib)
    return out


def refusals(capi, lib):
    """Launching entry points with arguments they refuse before a launch.  EVERY case here must return on a check of the host code: a case that got
    through would launch a kernel on pointers that are not memory."""
    r = []
    ok = lambda **kw: conv_desc(capi, 4096, 64, **kw)
    ks_ok = 2 | (1 << 2) | (2 << 4)
    for dt in DTYPES:
        vec = 8 if dt == capi.BF16 else 4
        # pn2_conv_gemm
        gemm = lambda d, in_=PTR, psum=None, psq=None: lib.pn2_conv_gemm(dt, in_, PTR, PTR, psum, psq, C.byref(d) if d is not None else None, None)
        r += [gemm(ok(), in_=None), gemm(None), gemm(ok(cin_p=12)), gemm(ok(ld_in=68)), gemm(ok(kp=64)), gemm(ok(stride=3)),
              gemm(ok(flags=capi.CONV_STATS)), gemm(ok(flags=capi.CONV_STATS), psum=PTR), gemm(ok(flags=capi.CONV_BIAS)),
              gemm(ok(flags=capi.CONV_BIAS | capi.CONV_STATS), psum=PTR, psq=PTR), gemm(ok(flags=capi.CONV_AFFINE)),
              gemm(ok(tune=ks_ok, ksplit=2)), gemm(ok(tune=1 | (1 << 2) | (2 << 4), ksplit=4), psum=PTR), gemm(ok(tune=ks_ok, ksplit=15, flags=capi.CONV_ACCUM), psum=PTR)]
        if dt != capi.BF16:
            r.append(gemm(ok(tune=ks_ok, ksplit=2), psum=PTR))          # external split-K: bf16 only
        if dt == capi.BF16:          # refusals of the split-K launchers themselves (-4), reached through the whole dispatch
            r += [gemm(conv_desc(capi, 1 << 16, 256, tune=2 | (2 << 2) | (3 << 4) | 0x40)),                    # two 3-stage rings of a 128 x 128 tile
                  gemm(ok(tune=3 | (1 << 2) | (2 << 4) | 0x40, ksplit=2), psum=PTR), gemm(ok(tune=2 | (1 << 2) | (2 << 4) | 0x80, ksplit=3), psum=PTR)]
        if dt == 7:
            r.append(gemm(ok()))
        # pn2_conv_gemm_affine
        aff = lambda d, in_=PTR, scale=PTR, res=None, ld_res=0: lib.pn2_conv_gemm_affine(dt, in_, PTR, PTR, scale, PTR, res, ld_res, C.byref(d) if d is not None else None, None)
        A = capi.CONV_AFFINE
        r += [aff(None), aff(ok(flags=A), scale=None), aff(ok()), aff(ok(flags=A | capi.CONV_STATS)), aff(ok(flags=A | capi.CONV_ACCUM)), aff(ok(flags=A, tune=ks_ok, ksplit=2)),
              aff(conv_desc(capi, 4096, 64 + vec // 2, flags=A), res=PTR, ld_res=64), aff(ok(flags=A), res=PTR, ld_res=vec + 1), aff(ok(flags=A | capi.CONV_RELU), in_=None),
              aff(ok(flags=A, cin_p=12)), aff(ok(flags=A, stride=16))]
        if dt == 7:
            r.append(aff(ok(flags=A)))
        # pn2_conv_gemm_ep
        def epc(d, in_=PTR, ep="new", **f):
            e = capi.ConvEp()
            for k, v in f.items():          # a_* / b_* / c_*: fields of that BatchNorm-backward target; anything else: a field of the struct itself
                if k[:2] in ("a_", "b_", "c_"):
                    setattr(getattr(e, k[0]), k[2:], v)
                else:
                    setattr(e, k, v)
            return lib.pn2_conv_gemm_ep(dt, in_, PTR, PTR, C.byref(d) if d is not None else None, None if ep is None else C.byref(e), None)
        full = dict(raw=PTR, par=PTR, p1=PTR, p2=PTR, ldp=64, ld_raw=64, ps=1)
        tgt = lambda t, **over: {f"{t}_{k}": v for k, v in {**full, **over}.items()}
        r += [epc(None), epc(ok(), ep=None), epc(ok(flags=capi.CONV_STATS)), epc(ok(flags=capi.CONV_BIAS)), epc(ok(tune=ks_ok, ksplit=2)),
              epc(conv_desc(capi, 4096, 64 + vec // 2)), epc(ok(), a_mode=1), epc(ok(), **tgt("a", mode=1, ld_raw=vec + 1)), epc(ok(), **tgt("a", mode=1, ps=0)),
              epc(ok(), **tgt("a", mode=1 | 4)), epc(ok(), **tgt("a", mode=1, split=vec + 1)), epc(ok(), b_mode=1), epc(ok(), b_out=PTR, b_ld_out=vec + 1),
              epc(ok(), **tgt("b", mode=1, out=PTR, ld_out=64, ldp=0)), epc(ok(), pool=PTR, **tgt("a", mode=1)), epc(ok(flags=capi.CONV_ACCUM), pool=PTR, ld_pool=32, **tgt("a", mode=1)),
              epc(ok(), c_mode=1), epc(ok(), c_mode=2, **tgt("a", mode=1)), epc(ok(), **tgt("a", mode=1), **tgt("c", mode=1, raw=None)),
              epc(conv_desc(capi, 1 << 16, 256), **tgt("a", mode=1), **tgt("c", mode=1)),          # second BatchNorm on a tile of more than 4096 elements
              epc(ok(), in_=None, **tgt("a", mode=1)), epc(ok(cin_p=12), **tgt("a", mode=1))]
        if dt == 7:
            r.append(epc(ok(), **tgt("a", mode=1)))
        # pn2_conv_gemm_multi
        multi = lambda bm, bn, ep=0, jobs=PTR, njobs=1, total=1: lib.pn2_conv_gemm_multi(dt, bm, bn, ep, jobs, PTR, njobs, total, None)
        r += [multi(64, 64, jobs=None), multi(64, 64, njobs=0), multi(64, 64, total=0), multi(96, 64), multi(64, 16, ep=1), multi(0x100 | 128, 128), multi(0x100 | 64, 32, ep=1),
              multi(0x200 | 64, 64), multi(32, 32)]
        if dt != capi.BF16:
            r += [multi(128, 128), multi(64, 128, ep=3), multi(0x100 | 64, 64)]          # fp32 storage: no 128-wide tiles, no split-K table kernel (or -3 first)
        # pn2_conv_wgrad
        wg = lambda d, dy=PTR, ns=1: lib.pn2_conv_wgrad(dt, dy, PTR, PTR, C.byref(d) if d is not None else None, ns, None)
        r += [wg(None), wg(wgrad_desc(capi, 4096, 64), dy=None), wg(wgrad_desc(capi, 4096, 64), ns=0), wg(wgrad_desc(capi, 4096, 64, cin_p=12)), wg(wgrad_desc(capi, 4096, 64, ld=68)),
              wg(wgrad_desc(capi, 4096, 60)), wg(wgrad_desc(capi, 4096, 96, rp=96)), wg(wgrad_desc(capi, 4096, 64, kp=192)), wg(wgrad_desc(capi, 4096, 64, rp=96, tune=2))]
        if dt != capi.BF16:
            r += [wg(wgrad_desc(capi, 4096, 64, tune=2)), wg(wgrad_desc(capi, 4096, 128, tune=3, kp=256))]
        if dt == 7:
            r.append(wg(wgrad_desc(capi, 4096, 64)))
        # pn2_conv_wgrad_multi
        wm = lambda v, jobs=PTR, njobs=1, total=1: lib.pn2_conv_wgrad_multi(dt, v, jobs, PTR, njobs, total, None)
        r += [wm(0, jobs=None), wm(0, njobs=0), wm(0, total=0), wm(-1), wm(15), wm(99)]
        if dt == 7:
            r.append(wm(3))
        if dt not in (capi.BF16, 7):
            r += [wm(v) for v in range(6, 15)]          # the LDS-DMA wgrad kernels are bf16 only
    return r


def _load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def results():
    from pn2 import capi
    return sweep(capi)


@pytest.mark.parametrize("section", ["tile_n", "tile_m", "stat_blocks", "gemm_tile", "gemm_tile_edges", "gemm_job_blocks", "wgrad_variant", "wgrad_blocks",
                                     "pack_blocks", "reduce_blocks", "refusals"])
def test_selection_matches_recorded(results, section):
    want, got = _load_fixture()[section], results[section]
    assert len(got) == len(want), (section, len(got), len(want))
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, f"{section}: {len(bad)} of {len(got)} results differ from the recorded ones; first (index, got, recorded): {bad[:8]}"


def test_refusals_never_launch(results):
    """a refusal is one of the library's own negative codes; 0 or a HIP error code would mean that a case reached a launch"""
    assert set(results["refusals"]) <= {-1, -2, -3, -4}, sorted(set(results["refusals"]))
    assert set(results["refusals"]) == {-1, -2, -3, -4}


def test_sweep_reaches_every_selection_branch(results):
    # pn2_conv_gemm_tile / gemm_select: every built tile, with and without the split-K table bit where that exists, and each refusal
    tiles = set(results["gemm_tile"]) | set(results["gemm_tile_edges"])
    plain = {(bm << 8) | bn for bm in (64, 128) for bn in (32, 64, 128)}
    ks2 = {((bm | 0x100) << 8) | bn for bm, bn in ((128, 64), (64, 128), (64, 64))}
    assert tiles == plain | ks2 | {-1, -2, -3}, sorted(tiles)
    assert set(results["tile_m"]) == {64, 128} and set(results["tile_n"]) == {32, 64, 128}
    # wgrad_variant: register-staged 0..5, LDS-DMA 6..11, the 128 x 256 tiles 12 / 13, and both refusals
    assert set(results["wgrad_variant"]) == set(range(14)) | {-1, -3}, sorted(set(results["wgrad_variant"]))
    assert {-1, -2} < set(results["wgrad_blocks"]) and {-1, -2} < set(results["gemm_job_blocks"])
    assert -1 in results["pack_blocks"] and -1 in results["reduce_blocks"]


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: [PN2_LIB=<library to record from>] python tests/test_conv_select_cpu.py --record")
    from pn2 import capi
    res = sweep(capi)
    with open(FIXTURE, "w") as f:
        json.dump(res, f, separators=(",", ":"))
        f.write("\n")
    print(f"recorded {sum(len(v) for v in res.values())} results from {capi.LIB_PATH}:")
    for k, v in res.items():
        print(f"  {k:16s} {len(v):6d} results, {len(set(v)):4d} distinct")
