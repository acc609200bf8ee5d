"""Launch plans and refusal codes of the non-conv launch layers (pn2_bn.hip, pn2_spatial.hip, pn2_emcad.hip and the layernorm / column-sum / depth-wise
half of pn2_vit.hip), pinned against a recorded fixture.

The geometry exports of these files (`pn2_*_blocks`, `pn2_*_job_blocks` and the fields they write into a job) are pure host code: they run without a
device.  A fixed sweep goes through them, and through every launching entry point with argument sets that are refused BEFORE any launch (a null
pointer, a misalignment or shape rule, an unknown dtype, and an unknown dtype together with a misalignment - which pins whether -2 or -3 wins); every
result must equal tests/golden/launch_select.json.  The fixture is recorded with the same sweep from a library build that is known good (PN2_LIB
selects the build):

    PN2_LIB=/path/to/libpn2_hip.so python tests/test_launch_select_cpu.py --record

A change of the launch / dispatch code that keeps behaviour leaves this test green without re-recording.  The depth-wise geometries read the
environment switches PN2_DW_WIN and PN2_DW_SEG: the sweep is recorded and compared with both unset, and the tests skip when either is set.

What a host-only export cannot show is the kernel a launch picks (for instance the register-lean BatchNorm backward apply): the sweep pins what the
geometry exports answer for the PN2_MULTI_LEAN / PN2_MULTI_F32DY / PN2_MULTI_F32OUT table codes, and the refusals of the `_multi` launchers for them."""
import ctypes as C
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "launch_select.json")
if __name__ == "__main__":          # (under pytest, conftest.py has set the path)
    sys.path[:0] = [ROOT, os.path.join(ROOT, "pranet-v2_amd")]

ENV_SWITCHES = ("PN2_DW_WIN", "PN2_DW_SEG")
DTYPES = (0, 1, 2, 3, 7)          # PN2_F32, PN2_BF16, two codes only the conv entry points take, and a code the library does not know
F32, BF16 = 0, 1
F32X, LEAN = 0x200, 0x100         # PN2_MULTI_F32OUT / PN2_MULTI_F32DY and PN2_MULTI_LEAN
M_LIST = (1, 7, 255, 256, 257, 4096, 123904, 1 << 20)
# channel counts: C / V = 1, 3, 32, 33, 256, 257 for V = 4 and V = 8, and counts that are no multiple of the vector
CHANNELS = (2, 4, 6, 8, 9, 12, 24, 100, 128, 132, 256, 264, 1024, 1028, 1030, 2048, 2056)
PTR = C.c_void_p(4096)            # a non-null pointer for calls that are refused before anything reads it
FILES = ("bn", "spatial", "emcad", "vit")


def vec(dt):
    return 4 if dt == F32 else 8


# ------------------------------------------------------------------------------------------------ host-only geometry
def bn_geometry(capi, lib, out):
    out["bn_bwd_blocks"] = [lib.pn2_bn_bwd_blocks(m, c, dt) for m in M_LIST for c in CHANNELS for dt in DTYPES]

    r = []
    for nblk in (0, 1, 7, 64, 512, 4096):
        for cp in (8, 100, 2048):
            j = capi.BnFinJob()
            for n in ("psum", "psq", "gamma", "beta", "scale", "shift", "mean", "invstd"):
                setattr(j, n, PTR)
            j.d.Cp, j.nblk = cp, nblk
            r.append([lib.pn2_bn_finalize_job_blocks(C.byref(j)), j.cpb])
    for n in ("psum", "psq", "gamma", "beta", "scale", "shift", "mean", "invstd"):
        j = capi.BnFinJob()
        for k in ("psum", "psq", "gamma", "beta", "scale", "shift", "mean", "invstd"):
            setattr(j, k, None if k == n else PTR)
        j.d.Cp, j.nblk = 64, 8
        r.append([lib.pn2_bn_finalize_job_blocks(C.byref(j)), j.cpb])
    r.append([lib.pn2_bn_finalize_job_blocks(None), 0])
    out["bn_finalize_job"] = r

    def affine(dt, m, c, **kw):
        j = capi.AffineJob()
        j.x, j.y, j.M, j.C = PTR, PTR, m, c
        j.ld_x = j.ld_y = j.ld_res = j.ld_add = j.ld_y2 = c
        for k, v in kw.items():
            setattr(j, k, v)
        return [lib.pn2_affine_job_blocks(dt, C.byref(j)), j.cvp, j.rows_per_blk]
    rows, elem = [], []
    for m in M_LIST:
        for c in CHANNELS:
            rows += [affine(dt, m, c) for dt in DTYPES]
            elem += [affine(dt | F32X, m, c) for dt in DTYPES]
    out["affine_job_rows"], out["affine_job_elementwise"] = rows, elem
    r = []
    for dt in DTYPES + (BF16 | F32X,):
        r += [affine(dt, 4096, 64, x=None), affine(dt, 4096, 64, y=None), affine(dt, 4096, 64, ld_x=68), affine(dt, 4096, 64, ld_y=66), affine(dt, 4096, 64, res=PTR),
              affine(dt, 4096, 64, res=PTR, ld_res=68), affine(dt, 4096, 64, ld_res=68), affine(dt, 4096, 64, y2=PTR), affine(dt, 4096, 64, y2=PTR, add=PTR),
              affine(dt, 4096, 64, y2=PTR, add=PTR, ld_add=68), affine(dt, 4096, 64, y2=PTR, add=PTR, ld_y2=68), affine(dt, 4096, 64, add=PTR), affine(dt, 0, 64),
              affine(dt, 4096, 0), [lib.pn2_affine_job_blocks(dt, None), 0, 0]]
    out["affine_job_edges"] = r

    def bfin(nseg, c0, nblk, cp=256, ldp=(256,) * 4, null=None):
        j = capi.BnBFinJob()
        for n in ("gamma", "invstd", "dgamma", "dbeta", "coef"):
            setattr(j, n, None if n == null else PTR)
        j.sg.nseg, j.d.Cp = nseg, cp
        for k in range(4):
            j.sg.c0[k], j.sg.nblk[k], j.sg.ldp[k] = c0[k], nblk[k], ldp[k]
            j.sg.p1[k] = None if null == f"p1{k}" else PTR
            j.sg.p2[k] = None if null == f"p2{k}" else PTR
        return [lib.pn2_bn_bwd_finalize_job_blocks(C.byref(j)), j.cpb]
    r = []
    for nseg in range(0, 6):
        for c0 in ((0, 64, 128, 192), (0, 0, 0, 0), (0, 128, 64, 192), (8, 64, 128, 192), (0, 64, 64, 192)):
            for nblk in ((1, 1, 1, 1), (512, 7, 64, 4096), (7, 4096, 1, 1), (8, 0, 8, 8), (64, 64, 64, 0)):
                r.append(bfin(nseg, c0, nblk))
    for cp in (8, 100, 2048):
        r += [bfin(1, (0,) * 4, (n,) * 4, cp=cp) for n in (1, 7, 64, 512, 4096)]
    r += [bfin(2, (0, 64, 0, 0), (8,) * 4, null=n) for n in ("gamma", "invstd", "dgamma", "dbeta", "coef", "p10", "p21", "p12", "p23")]
    r += [bfin(2, (0, 64, 0, 0), (8,) * 4, ldp=(256, 0, 256, 256)), bfin(2, (0, 64, 0, 0), (8,) * 4, ldp=(256, 256, 0, 256)), [lib.pn2_bn_bwd_finalize_job_blocks(None), 0]]
    out["bn_bwd_finalize_job"] = r

    def apply_(dt, m, cp, **kw):
        j = capi.BnApplyJob()
        j.dy, j.dx, j.M, j.Cp, j.pad_ = PTR, PTR, m, cp, 1
        j.ld_dy = j.ld_y = j.ld_x = j.ld_dx = j.ld_dres = cp
        for k, v in kw.items():
            setattr(j, k, v)
        return [lib.pn2_bn_bwd_apply_job_blocks(dt, C.byref(j)), j.cvp, j.rows_per_blk]
    rows, lean, elem = [], [], []
    for m in M_LIST:
        for c in CHANNELS:
            rows += [apply_(dt, m, c) for dt in DTYPES]
            lean += [apply_(dt | LEAN, m, c) for dt in DTYPES]
            elem += [apply_(dt | F32X, m, c) for dt in DTYPES]
    out["bn_apply_job_rows"], out["bn_apply_job_lean"], out["bn_apply_job_elementwise"] = rows, lean, elem
    full = dict(coef=PTR, x=PTR, mean=PTR, invstd=PTR)
    r = []
    for dt in DTYPES + (BF16 | F32X, BF16 | LEAN, F32 | LEAN, BF16 | LEAN | F32X):
        r += [apply_(dt, 4096, 64, dy=None), apply_(dt, 4096, 64, dx=None), apply_(dt, 4096, 64, coef=PTR), apply_(dt, 4096, 64, **{**full, "x": None}),
              apply_(dt, 4096, 64, **{**full, "mean": None}), apply_(dt, 4096, 64, **{**full, "invstd": None}), apply_(dt, 4096, 64, **full), apply_(dt, 4096, 64, **full, ld_x=68),
              apply_(dt, 4096, 64, ld_x=68), apply_(dt, 4096, 64, ld_dy=68), apply_(dt, 4096, 64, ld_dx=66), apply_(dt, 4096, 64, y=PTR), apply_(dt, 4096, 64, y=PTR, ld_y=68),
              apply_(dt, 4096, 64, ld_y=68), apply_(dt, 4096, 64, dres=PTR), apply_(dt, 4096, 64, dres=PTR, ld_dres=68), apply_(dt, 4096, 64, ld_dres=68), apply_(dt, 4096, 64, pad_=0),
              apply_(dt, 0, 64), apply_(dt, 4096, 0), [lib.pn2_bn_bwd_apply_job_blocks(dt, None), 0, 0]]
    out["bn_apply_job_edges"] = r

    def reduce_(dt, m, cp, nblk=512, **kw):
        j = capi.BnReduceJob()
        for n in ("dy", "x", "mean", "invstd", "p1", "p2"):
            setattr(j, n, PTR)
        j.M, j.Cp, j.nblk, j.pad_ = m, cp, nblk, 1
        j.ld_dy = j.ld_y = j.ld_x = cp
        for k, v in kw.items():
            setattr(j, k, v)
        return [lib.pn2_bn_bwd_reduce_job_blocks(dt, C.byref(j)), j.cvp, j.rows_per_blk]
    rows, scal = [], []
    for m in M_LIST:
        for c in CHANNELS:
            for nblk in (1, 512):
                rows += [reduce_(dt, m, c, nblk) for dt in DTYPES]
                scal += [reduce_(dt | F32X, m, c, nblk) for dt in DTYPES]
    out["bn_reduce_job_vector"], out["bn_reduce_job_scalar"] = rows, scal
    r = []
    for dt in DTYPES + (BF16 | F32X, BF16 | LEAN):
        r += [reduce_(dt, 4096, 64, **{n: None}) for n in ("dy", "x", "mean", "invstd", "p1", "p2")]
        r += [reduce_(dt, 4096, 64, nblk=0), reduce_(dt, 4096, 64, ld_dy=68), reduce_(dt, 4096, 64, ld_x=66), reduce_(dt, 4096, 64, ld_y=68), reduce_(dt, 4096, 64, y=PTR),
              reduce_(dt, 4096, 64, y=PTR, ld_y=68), reduce_(dt, 4096, 64, pad_=0), [lib.pn2_bn_bwd_reduce_job_blocks(dt, None), 0, 0]]
    out["bn_reduce_job_edges"] = r


def spatial_geometry(capi, lib, out):
    def copy(dt, m, c, **kw):
        j = capi.CopyJob()
        j.src, j.dst, j.M, j.C, j.ld_s, j.ld_d = PTR, PTR, m, c, c, c
        for k, v in kw.items():
            setattr(j, k, v)
        return lib.pn2_copy_job_blocks(dt, C.byref(j))
    r = [copy(dt, m, c) for m in M_LIST + (1 << 22,) for c in CHANNELS for dt in DTYPES]
    for dt in DTYPES:
        r += [copy(dt, 4096, 64, src=None), copy(dt, 4096, 64, dst=None), copy(dt, 0, 64), copy(dt, 4096, 0), copy(dt, 4096, 64, ld_s=68), copy(dt, 4096, 64, ld_d=66),
              lib.pn2_copy_job_blocks(dt, None)]
    out["copy_job"] = r


def vit_geometry(capi, lib, out):
    def colsum(dt, m, c, **kw):
        j = capi.ColsumInJob()
        j.dy, j.partial, j.M, j.C, j.ld = PTR, PTR, m, c, c
        for k, v in kw.items():
            setattr(j, k, v)
        return [lib.pn2_colsum_job_blocks(dt, C.byref(j)), j.rows, j.cvp]
    r = [colsum(dt, m, c) for m in M_LIST for c in CHANNELS for dt in DTYPES]
    for dt in DTYPES:
        r += [colsum(dt, 4096, 64, dy=None), colsum(dt, 4096, 64, partial=None), colsum(dt, 0, 64), colsum(dt, 4096, 64, ld=68), colsum(dt, 4096, 64, ld=66),
              [lib.pn2_colsum_job_blocks(dt, None), 0, 0]]
    out["colsum_job"] = r
    out["rows_blocks"] = [lib.pn2_rows_blocks(m, u) for m in (0,) + M_LIST for u in (0, 1, 2, 4, 8, 32, 64, 256)]
    out["ln_slots"] = [lib.pn2_ln_slots(dt, c) for dt in DTYPES for c in CHANNELS + (32, 64, 512, 4096, 8192, 16384, 16392)]
    out["colsum_unit"] = [lib.pn2_colsum_unit(dt, c) for dt in DTYPES for c in CHANNELS + (1, 16, 32, 64, 512, 4096)]
    out["colsum_finalize_blocks"] = [lib.pn2_colsum_finalize_blocks(c) for c in (-1, 0, 1, 31, 32, 33, 256, 2048, 2049)]
    # depth-wise 3x3 of the Mix-FFN: the window kernels' partial rows and the weight-gradient chunks; N * H * W around the 32-pixel-segment and
    # 200 000-thread switches, one tensor beyond the 2 GB extent that the window kernels address
    cb, wb = [], []
    shapes = [(n, w, w) for n in (1, 16) for w in (1, 11, 16, 88, 128)] + [(0, 16, 16), (1, 0, 16), (1, 16, 0), (64, 512, 512)]
    for dt in DTYPES:
        for n, h, w in shapes:
            for c in (2, 3, 4, 6, 8, 10, 12, 16, 32, 64, 66, 128, 256, 320, 512):
                cb.append(lib.pn2_dwconv3x3_colsum_blocks(dt, n, h, w, c))
                wb.append(lib.pn2_dwconv3x3_wgrad_blocks(dt, n, h, w, c))
    out["dwconv3x3_colsum_blocks"], out["dwconv3x3_wgrad_blocks"] = cb, wb


def emcad_geometry(capi, lib, out):
    # W = H; N = 1 and 16 put N * H * ceil(W / 16) * (C / VT) on both sides of the 200 000-thread switch of the segment length
    dw, pc = [], []
    for dt in DTYPES:
        for n in (1, 16):
            for w in (1, 11, 16, 88, 128):
                for k in (1, 3, 5, 7):
                    for c in (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 64, 66, 100, 256, 512, 1024):
                        dw += [lib.pn2_dwconv_blocks(dt, n, w, w, c, k, 0), lib.pn2_dwconv_blocks(dt, n, w, w, c, k, 1)]
                pc += [lib.pn2_pairconv_blocks(dt, n, w, w, f) for f in (1, 2, 3, 4, 6, 8, 30, 32, 34, 64, 128, 130, 512, 1024)]
        dw += [lib.pn2_dwconv_blocks(dt, 0, 16, 16, 64, 3, 0), lib.pn2_dwconv_blocks(dt, 1, 0, 16, 64, 3, 0), lib.pn2_dwconv_blocks(dt, 1, 16, 0, 64, 3, 1)]
        pc += [lib.pn2_pairconv_blocks(dt, 0, 16, 16, 64), lib.pn2_pairconv_blocks(dt, 1, 0, 16, 64), lib.pn2_pairconv_blocks(dt, 1, 16, 0, 64)]
    out["dwconv_blocks"], out["pairconv_blocks"] = dw, pc
    out["gate_blocks"] = [lib.pn2_gate_blocks(dt, hw, c) for dt in DTYPES for hw in (0,) + M_LIST for c in CHANNELS]
    out["mutation_loss_blocks"] = [lib.pn2_mutation_loss_blocks(n) for n in (-1, 0, 1, 255, 256, 257, 123904, 1 << 20, (1 << 20) + 1, 1 << 32)]
    out["mutation_loss_width"] = [lib.pn2_mutation_loss_width(k) for k in range(0, 13)]


# ------------------------------------------------------------------------------------------------ refusals of the launching entry points
class Case:
    """One launching entry point: `valid(dt)` gives an argument list that only an unknown dtype gets refused; `nulls` are the positions of the
    required pointers; `bad(dt)` gives (position -> value) edits that break one alignment or shape rule each (an edit may be None where the rule
    does not exist for that dtype).  dtype = False: the entry point takes no dtype."""

    def __init__(self, name, valid, nulls=(), bad=None, dtype=True):
        self.name, self.valid, self.nulls, self.bad, self.dtype = name, valid, nulls, bad or (lambda dt: []), dtype

    def run(self, lib):
        fn, r = getattr(lib, self.name), []
        for dt in (DTYPES if self.dtype else (None,)):
            base = self.valid(dt)
            for p in self.nulls:
                r.append(fn(*[None if i == p else a for i, a in enumerate(base)]))
            for edit in self.bad(dt):
                if edit is not None:
                    r.append(fn(*[edit.get(i, a) for i, a in enumerate(base)]))
            if self.dtype and dt not in (F32, BF16):
                r.append(fn(*base))          # valid shapes, unknown dtype
        return r


def multi_case(name, dtype=True, dts=DTYPES):
    """pn2_*_multi(dt?, jobs, block_start, njobs, total_blocks, stream)"""
    o = 1 if dtype else 0

    class Multi(Case):
        def run(self, lib):
            fn, r = getattr(lib, name), []
            for dt in (dts if dtype else (None,)):
                pre = [dt] if dtype else []
                r += [fn(*pre, None, PTR, 1, 1, None), fn(*pre, PTR, None, 1, 1, None), fn(*pre, PTR, PTR, 0, 1, None), fn(*pre, PTR, PTR, 1, 0, None)]
                if dtype and (dt & ~(LEAN | F32X)) not in (F32, BF16):
                    r.append(fn(*pre, PTR, PTR, 1, 1, None))
            return r
    return Multi(name, None)


def bn_desc(capi, cp=64):
    d = capi.BnDesc()
    d.M, d.Cp, d.C, d.gw, d.gwp = 4096, cp, cp, cp, cp
    return C.byref(d)


def bn_segs(capi, nseg=2, c0=(0, 32, 0, 0), nblk=(8, 8, 8, 8), ldp=(64,) * 4, null=None):
    s = capi.BnSegs()
    s.nseg = nseg
    for k in range(4):
        s.c0[k], s.nblk[k], s.ldp[k] = c0[k], nblk[k], ldp[k]
        s.p1[k] = None if null == f"p1{k}" else PTR
        s.p2[k] = None if null == f"p2{k}" else PTR
    return C.byref(s)


def bn_refusals(capi, lib):
    r = []
    D = bn_desc(capi)
    cases = [
        Case("pn2_bn_finalize", lambda dt: [PTR, PTR, 8, D, PTR, PTR, PTR, PTR, PTR, PTR, PTR, PTR, None], nulls=(0, 1, 3, 4, 5, 8, 9, 10, 11), dtype=False),
        Case("pn2_bn_eval_prepare", lambda dt: [D, PTR, PTR, PTR, PTR, PTR, PTR, None], nulls=range(7), dtype=False),
        multi_case("pn2_bn_eval_prepare_multi", dtype=False), multi_case("pn2_bn_finalize_multi", dtype=False), multi_case("pn2_bn_bwd_finalize_multi", dtype=False),
        multi_case("pn2_affine_multi", dts=DTYPES + (7 | F32X, 2 | F32X, BF16 | F32X)),
        multi_case("pn2_bn_bwd_apply_multi", dts=DTYPES + (7 | LEAN, 2 | LEAN, 7 | F32X, BF16 | LEAN, F32 | LEAN, BF16 | F32X, F32 | F32X, BF16 | LEAN | F32X)),
        multi_case("pn2_bn_bwd_reduce_multi", dts=DTYPES + (7 | F32X, BF16 | F32X, F32 | F32X, BF16 | LEAN)),
        Case("pn2_bn_bwd_finalize", lambda dt: [PTR, PTR, 8, D, PTR, PTR, PTR, PTR, 0, PTR, None], nulls=(0, 1, 3, 4, 5, 6, 7, 9), dtype=False),
        Case("pn2_bn_relu_maxpool_fwd", lambda dt: [dt, PTR, 64, PTR, PTR, PTR, 64, PTR, 2, 16, 16, 64, 8, 8, None], nulls=(1, 3, 4, 5, 7),
             bad=lambda dt: [{11: 64 + vec(dt) // 2}, {2: 68 if vec(dt) == 8 else 66}, {6: 66}, {12: 9}, {13: 7}, {8: 1 << 16, 9: 512, 10: 512, 12: 256, 13: 256}]),
        Case("pn2_pool_bn_bwd_reduce", lambda dt: [dt, PTR, 64, PTR, PTR, 64, 2, 16, 16, 64, 8, 8, PTR, PTR, PTR, PTR, PTR, PTR, 8, None], nulls=(1, 3, 4, 12, 13, 14, 15, 16, 17),
             bad=lambda dt: [{9: 64 + vec(dt) // 2}, {2: 66}, {5: 66}, {7: 15}, {8: 15}, {10: 7}, {11: 9}, {9: 3 * vec(dt), 2: 96, 5: 96}, {9: 4096}, {9: 0},
                             {6: 1 << 12, 7: 128, 8: 128, 10: 64, 11: 64}]),
        Case("pn2_pool_bn_bwd_apply", lambda dt: [dt, PTR, 64, PTR, PTR, 64, 2, 16, 16, 64, 8, 8, PTR, PTR, PTR, PTR, PTR, PTR, 64, None], nulls=(1, 3, 4, 12, 13, 14, 15, 16, 17),
             bad=lambda dt: [{9: 64 + vec(dt) // 2}, {2: 66}, {5: 66}, {18: 66}, {7: 15}, {8: 15}, {10: 7}, {11: 9}, {9: 4096}, {9: 0}, {6: 1 << 12, 7: 128, 8: 128, 10: 64, 11: 64}]),
        Case("pn2_affine_act_sum", lambda dt: [dt, PTR, 64, PTR, 64, 4096, 64, PTR, PTR, 1, PTR, 64, PTR, 64, None], nulls=(1, 3, 10, 12),
             bad=lambda dt: [{6: 64 + vec(dt) // 2}, {2: 66}, {4: 66}, {11: 66}, {13: 66}]),
        Case("pn2_affine_act_tee", lambda dt: [dt, PTR, 64, PTR, 64, 4096, 64, PTR, PTR, 1, PTR, 64, 32, None], nulls=(1, 3, 10),
             bad=lambda dt: [{6: 64 + vec(dt) // 2}, {2: 66}, {4: 66}, {11: 66}, {12: 34}, {12: -8}, {12: 64}]),
    ]
    for c in cases:
        r += c.run(lib)
    # the entry points with two or three dtype codes: every pair that is not one of bf16 -> bf16, bf16 -> fp32, fp32 -> fp32 is refused
    pairs_ok = {(BF16, BF16), (BF16, F32), (F32, F32)}
    for a in DTYPES:
        for b in DTYPES:
            act = lambda x=PTR, y=PTR: lib.pn2_affine_act(a, x, 64, b, y, 64, 4096, 64, PTR, PTR, None, 0, 1, None)
            red = lambda dt_y=a, y=None, **n: lib.pn2_bn_bwd_reduce(a, b, n.get("dy", PTR), 64, 64, y, 64, dt_y, n.get("x", PTR), 64, 4096, 64, n.get("mean", PTR), n.get("invstd", PTR),
                                                                    n.get("p1", PTR), n.get("p2", PTR), 8, None, None, 0, None)
            app = lambda dt_y=a, y=None, coef=None, x=None, mean=None, invstd=None, dy=PTR, dx=PTR: lib.pn2_bn_bwd_apply(
                a, b, dy, 64, 64, y, 64, dt_y, x, 64, 4096, 64, mean, invstd, coef, dx, 64, None, 0, 0, None, None, 0, None)
            r += [act(x=None), act(y=None)] + [red(**{n: None}) for n in ("dy", "x", "mean", "invstd", "p1", "p2")] + [red(dt_y=a ^ 1, y=PTR), red(dt_y=9, y=PTR)]
            r += [app(dy=None), app(dx=None), app(coef=PTR), app(coef=PTR, x=PTR, mean=PTR), app(coef=PTR, x=PTR, invstd=PTR), app(coef=PTR, mean=PTR, invstd=PTR),
                  app(dt_y=a ^ 1, y=PTR), app(dt_y=9, y=PTR)]
            if (a, b) not in pairs_ok:
                r += [act(), red(), red(y=PTR), app(), app(y=PTR), app(coef=PTR, x=PTR, mean=PTR, invstd=PTR)]
    # pn2_bn_bwd_finalize_seg: the segment rules (strictly increasing c0, unlike pn2_bn_bwd_finalize_job_blocks)
    seg = lambda s, **n: lib.pn2_bn_bwd_finalize_seg(s, n.get("d", D), n.get("gamma", PTR), n.get("invstd", PTR), n.get("dgamma", PTR), n.get("dbeta", PTR), 0, n.get("coef", PTR), None)
    r += [seg(None)] + [seg(bn_segs(capi), **{n: None}) for n in ("d", "gamma", "invstd", "dgamma", "dbeta", "coef")]
    r += [seg(bn_segs(capi, nseg=n)) for n in (0, 5, -1)]
    for nseg in (1, 2, 3, 4):
        r += [seg(bn_segs(capi, nseg=nseg, c0=c0)) for c0 in ((8, 16, 32, 48), (0, 0, 0, 0), (0, 32, 16, 48), (0, 16, 32, 32), (0, 16, 16, 48))
              if c0[0] != 0 or any(c0[k] <= c0[k - 1] for k in range(1, nseg))]          # (only the prefixes that break the rule within nseg segments)
        r += [seg(bn_segs(capi, nseg=nseg, c0=(0, 16, 32, 48), null=f"{p}{nseg - 1}")) for p in ("p1", "p2")]
        r += [seg(bn_segs(capi, nseg=nseg, c0=(0, 16, 32, 48), nblk=tuple(0 if k == nseg - 1 else 8 for k in range(4)))),
              seg(bn_segs(capi, nseg=nseg, c0=(0, 16, 32, 48), ldp=tuple(0 if k == nseg - 1 else 64 for k in range(4))))]
    return r


def spatial_refusals(capi, lib):
    big = 1 << 16          # N = 65536 at 256 x 256 pixels: more elements than the 32-bit loops of these kernels index
    pool = lambda name, nulls, tail: Case(name, lambda dt: [dt, PTR, 64, PTR, 64] + tail, nulls=nulls)
    cases = [
        Case("pn2_maxpool3x3s2_fwd", lambda dt: [dt, PTR, 64, PTR, 64, PTR, 2, 16, 16, 64, 8, 8, None], nulls=(1, 3, 5), bad=lambda dt: [{6: big, 10: 256, 11: 256}, {6: big, 10: 256, 11: 256, 2: 66}]),
        Case("pn2_maxpool3x3s2_bwd", lambda dt: [dt, PTR, 64, PTR, PTR, 64, 2, 16, 16, 64, 8, 8, None], nulls=(1, 3, 4), bad=lambda dt: [{6: big, 7: 256, 8: 256}, {6: big, 7: 256, 8: 256, 2: 66}]),
        Case("pn2_avgpool_fwd", lambda dt: [dt, PTR, 64, PTR, 64, 2, 16, 16, 64, 8, 8, 3, 2, 1, 1, None], nulls=(1, 3), bad=lambda dt: [{5: big, 9: 256, 10: 256}, {5: big, 9: 256, 10: 256, 4: 66}]),
        Case("pn2_avgpool_bwd", lambda dt: [dt, PTR, 64, PTR, 64, 2, 16, 16, 64, 8, 8, 3, 2, 1, 1, 0, None], nulls=(1, 3), bad=lambda dt: [{5: big, 6: 256, 7: 256}, {5: big, 6: 256, 7: 256, 2: 66}]),
        Case("pn2_bilinear_fwd", lambda dt: [dt, PTR, 64, PTR, 64, 2, 8, 8, 64, 16, 16, 0, 0.5, 0.5, None], nulls=(1, 3), bad=lambda dt: [{5: big, 9: 256, 10: 256}, {5: big, 9: 256, 10: 256, 8: 9}]),
        Case("pn2_bilinear_bwd", lambda dt: [dt, PTR, 64, PTR, 64, 2, 8, 8, 64, 16, 16, 0, 0.5, 0.5, 0, None], nulls=(1, 3), bad=lambda dt: [{5: big, 6: 256, 7: 256}, {5: big, 6: 256, 7: 256, 8: 9}]),
        Case("pn2_binary", lambda dt: [dt, 0, PTR, 64, PTR, 64, PTR, 64, 4096, 64, 0, None], nulls=(2, 4, 6), bad=lambda dt: [{8: 1 << 30, 9: 64}, {8: 1 << 30, 9: 66}]),
        Case("pn2_mul_bwd", lambda dt: [dt, PTR, 64, PTR, 64, PTR, 64, PTR, 64, 0, C.c_void_p(8192), 64, 0, 4096, 64, None], nulls=(1, 3, 5, 7, 10),
             bad=lambda dt: [{10: PTR}, {13: 1 << 30}, {13: 1 << 30, 14: 66}]),
        multi_case("pn2_copy_multi"),
        Case("pn2_nchw_to_nhwc", lambda dt: [dt, PTR, PTR, 64, 2, 3, 4096, 64, None], nulls=(1, 2), bad=lambda dt: [{4: 1 << 16, 6: 1 << 16}]),
        Case("pn2_bias_grad", lambda dt: [PTR, 4096, 9, PTR, 0, None], nulls=(0, 3), dtype=False),
    ]
    r = []
    for c in cases:
        r += c.run(lib)
    for a in DTYPES:          # pn2_copy: equal dtypes, or fp32 <-> bf16
        for b in DTYPES:
            cp = lambda src=PTR, dst=PTR, m=4096, c=64: lib.pn2_copy(a, src, 64, b, dst, 64, m, c, 0, None)
            r += [cp(src=None), cp(dst=None), cp(m=1 << 30), cp(m=1 << 30, c=66)]
            if not ({a, b} <= {F32, BF16}):
                r.append(cp())
    return r


def emcad_refusals(capi, lib):
    odd = lambda dt, pos, c=65: {pos: c} if dt != F32 else None          # fp32 depth-wise walks take odd channel counts
    four = (C.c_void_p * 4)(4096, 4096, 4096, 4096)
    hole = (C.c_void_p * 4)(4096, 4096, None, 4096)
    cases = [
        Case("pn2_dwconv", lambda dt: [dt, PTR, PTR, PTR, 2, 16, 16, 64, 3, 0, 0, None, None, None], nulls=(1, 2, 3),
             bad=lambda dt: [{11: PTR}, odd(dt, 7), {8: 7}, {8: 2}, {8: 0}, {8: 7, 7: 65}]),
        Case("pn2_dwconv_wgrad", lambda dt: [dt, PTR, PTR, PTR, 2, 16, 16, 64, 3, None], nulls=(1, 2, 3), bad=lambda dt: [odd(dt, 7), {8: 7}, {8: 4}, {8: 7, 7: 65}]),
        Case("pn2_pairconv3x3_fwd", lambda dt: [dt, PTR, PTR, PTR, 2, 16, 16, 64, PTR, PTR, None], nulls=(1, 2, 3, 8, 9), bad=lambda dt: [{7: 66 if dt != F32 else 65}, {4: 0}, {5: 0}, {6: 0}]),
        Case("pn2_pairconv3x3_dgrad", lambda dt: [dt, PTR, PTR, PTR, 2, 16, 16, 64, 0, None], nulls=(1, 2, 3), bad=lambda dt: [{7: 66 if dt != F32 else 65}, {4: 0}, {5: 0}, {6: 0}]),
        Case("pn2_pairconv3x3_wgrad", lambda dt: [dt, PTR, PTR, PTR, 2, 16, 16, 64, None], nulls=(1, 2, 3), bad=lambda dt: [{7: 66 if dt != F32 else 65}, {4: 0}, {5: 0}, {6: 0}]),
        Case("pn2_gate_mul", lambda dt: [dt, PTR, PTR, PTR, 2, 256, 64, 0, 0, None], nulls=(1, 2, 3), bad=lambda dt: [{6: 64 + vec(dt) // 2}]),
        Case("pn2_gate_bwd", lambda dt: [dt, PTR, PTR, PTR, 2, 256, 64, 0, None], nulls=(1, 2, 3), bad=lambda dt: [{6: 64 + vec(dt) // 2}, {6: 64 + vec(dt) // 2, 7: 1}]),
        Case("pn2_global_pool", lambda dt: [dt, PTR, PTR, PTR, PTR, 2, 256, 64, None], nulls=(1, 2, 3, 4), bad=lambda dt: [{7: 64 + vec(dt) // 2}]),
        Case("pn2_global_pool_bwd", lambda dt: [dt, PTR, PTR, PTR, PTR, 2, 256, 64, 0, None], nulls=(1, 2, 3, 4)),
        Case("pn2_chan_stats", lambda dt: [dt, PTR, PTR, PTR, 512, 64, None], nulls=(1, 2, 3)),
        Case("pn2_chan_stats_bwd", lambda dt: [dt, PTR, PTR, PTR, 512, 64, 0, None], nulls=(1, 2, 3)),
        Case("pn2_upsample_nearest2x", lambda dt: [dt, PTR, PTR, 2, 16, 16, 64, None], nulls=(1, 2), bad=lambda dt: [{6: 64 + vec(dt) // 2}]),
        Case("pn2_upsample_nearest2x_bwd", lambda dt: [dt, PTR, PTR, 2, 16, 16, 64, 0, None], nulls=(1, 2), bad=lambda dt: [{6: 64 + vec(dt) // 2}]),
        Case("pn2_gather_sum", lambda dt: [dt, PTR, PTR, PTR, PTR, PTR, 512, 64, None], nulls=(1, 4, 5)),
        Case("pn2_sigmoid", lambda dt: [dt, PTR, 8, 1, PTR, 512, None], nulls=(1, 4), bad=lambda dt: [{5: 0}, {5: -1}]),
        Case("pn2_sigmoid_bwd", lambda dt: [dt, PTR, PTR, PTR, 8, 1, 512, 0, None], nulls=(1, 2, 3), bad=lambda dt: [{6: 0}]),
        Case("pn2_mutation_loss_fwd", lambda dt: [four, four, PTR, PTR, 2, 256, 8, 1.0, 1.0, 1.0, PTR, PTR, PTR, None], nulls=(0, 1, 2, 3, 10, 11, 12),
             bad=lambda dt: [{6: 1}, {6: 9, 0: hole}, {6: 9, 1: hole}], dtype=False),
        Case("pn2_mutation_loss_bwd", lambda dt: [four, four, four, four, PTR, PTR, 2, 256, 8, 1.0, 1.0, 1.0, PTR, 1.0, None], nulls=(0, 1, 2, 3, 4, 5, 12),
             bad=lambda dt: [{8: 10}, {8: 9, 0: hole}, {8: 9, 1: hole}, {8: 9, 2: hole}, {8: 9, 3: hole}], dtype=False),
    ]
    r = []
    for c in cases:
        r += c.run(lib)
    return r


def vit_refusals(capi, lib):
    cases = [
        Case("pn2_layernorm_fwd", lambda dt: [dt, PTR, 64, PTR, 64, 4, 64, PTR, PTR, 1e-5, PTR, PTR, None], nulls=(1, 3, 7, 8, 10, 11),
             bad=lambda dt: [{5: 0}, {6: 64 + vec(dt) // 2}, {6: 1 << 15}]),
        Case("pn2_layernorm_bwd", lambda dt: [dt, PTR, 64, PTR, 64, 4, 64, PTR, PTR, PTR, PTR, 64, 0, PTR, PTR, 1, None], nulls=(1, 3, 7, 8, 9, 10, 13, 14),
             bad=lambda dt: [{5: 0}, {15: 0}, {6: 64 + vec(dt) // 2}, {6: 1 << 15}, {15: 2}, {5: 4096, 15: 1}]),
        Case("pn2_colsum_finalize", lambda dt: [PTR, 8, 64, 64, PTR, 0, None], nulls=(0, 4), bad=lambda dt: [{1: 0}, {2: 0}], dtype=False),
        multi_case("pn2_colsum_finalize_multi", dtype=False),
        Case("pn2_colsum", lambda dt: [dt, PTR, 64, 4, 64, PTR, 1, None], nulls=(1, 5), bad=lambda dt: [{3: 0}, {6: 0}, {4: 64 + vec(dt) // 2}, {2: 66}, {6: 2}, {3: 1 << 20}]),
        multi_case("pn2_colsum_multi"),
        Case("pn2_dwconv3x3", lambda dt: [dt, PTR, PTR, PTR, PTR, None, 1, 4, 4, 8, 0, 0, None], nulls=(1, 2, 4), bad=lambda dt: [{9: 9}, {6: 0}, {7: 0}, {8: 0}]),
        # the column sums ride on the bf16 window kernels only: any other dtype, known or not, answers -2 here
        Case("pn2_dwconv3x3_colsum", lambda dt: [dt, PTR, PTR, PTR, PTR, 1, 4, 4, 8, 0, PTR, 1, None], nulls=(1, 2, 4, 10),
             bad=lambda dt: [{11: 0}, {8: 9}, {5: 0}, {11: 2}, {} if dt != BF16 else None]),
        Case("pn2_gelu_bwd", lambda dt: [dt, PTR, PTR, PTR, 4096, None], nulls=(1, 2, 3), bad=lambda dt: [{4: 4096 + vec(dt) // 2}]),
        Case("pn2_dwconv3x3_wgrad", lambda dt: [dt, PTR, PTR, PTR, 1, 1, 4, 4, 8, None, None, None], nulls=(1, 2, 3), bad=lambda dt: [{4: 0}, {9: PTR}, {8: 9}, {4: 2}, {4: 2, 8: 9}]),
        Case("pn2_scale_samples", lambda dt: [dt, PTR, PTR, PTR, None, 2, 4096, None], nulls=(1, 2, 3), bad=lambda dt: [{5: 0}, {6: 4096 + vec(dt) // 2}]),
    ]
    r = []
    for c in cases:
        r += c.run(lib)
    return r


def sweep(capi):
    """section name -> list of results, in a fixed order"""
    lib = capi.load()
    out = {}
    bn_geometry(capi, lib, out)
    spatial_geometry(capi, lib, out)
    emcad_geometry(capi, lib, out)
    vit_geometry(capi, lib, out)
    for f, fn in zip(FILES, (bn_refusals, spatial_refusals, emcad_refusals, vit_refusals)):
        out[f"refusals_{f}"] = fn(capi, lib)
    return out


def _load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


pytestmark = pytest.mark.skipif(any(v in os.environ for v in ENV_SWITCHES), reason="the sweep is recorded with PN2_DW_WIN and PN2_DW_SEG unset")


@pytest.fixture(scope="module")
def results():
    from pn2 import capi
    return sweep(capi)


SECTIONS = ["bn_bwd_blocks", "bn_finalize_job", "affine_job_rows", "affine_job_elementwise", "affine_job_edges", "bn_bwd_finalize_job", "bn_apply_job_rows", "bn_apply_job_lean",
            "bn_apply_job_elementwise", "bn_apply_job_edges", "bn_reduce_job_vector", "bn_reduce_job_scalar", "bn_reduce_job_edges", "copy_job", "dwconv_blocks", "pairconv_blocks",
            "gate_blocks", "mutation_loss_blocks", "mutation_loss_width", "colsum_job", "rows_blocks", "ln_slots", "colsum_unit", "colsum_finalize_blocks",
            "dwconv3x3_colsum_blocks", "dwconv3x3_wgrad_blocks"] + [f"refusals_{f}" for f in FILES]


def test_sections_complete(results):
    assert sorted(results) == sorted(SECTIONS) == sorted(_load_fixture())


@pytest.mark.parametrize("section", SECTIONS)
def test_plan_matches_recorded(results, section):
    want, got = _load_fixture()[section], results[section]
    assert len(got) == len(want), (section, len(got), len(want))
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, f"{section}: {len(bad)} of {len(got)} results differ from the recorded ones; first (index, got, recorded): {bad[:8]}"


@pytest.mark.parametrize("f", FILES)
def test_refusals_never_launch(results, f):
    """a refusal is one of the library's own negative codes; 0 or a HIP error code would mean that a case reached a launch.  Every file refuses with
    each of -1 (null pointer), -2 (alignment / shape) and -3 (dtype)."""
    assert set(results[f"refusals_{f}"]) == {-1, -2, -3}, sorted(set(results[f"refusals_{f}"]))


def _accepted(rows):
    return [r for r in rows if r[0] > 0]


def test_sweep_reaches_every_plan(results):
    # vector (row-walk) and scalar / element-wise plans both appear, with distinct geometry: cvp counts 16-byte vectors in one and elements in the other
    for vec_s, sc_s in (("bn_reduce_job_vector", "bn_reduce_job_scalar"), ("affine_job_rows", "affine_job_elementwise"), ("bn_apply_job_rows", "bn_apply_job_elementwise")):
        v, s = _accepted(results[vec_s]), _accepted(results[sc_s])
        assert len({tuple(r) for r in v}) > 20 and len({tuple(r) for r in s}) > 5, (vec_s, len(v), len(s))
        assert -2 in {r[0] for r in results[vec_s]}          # a misaligned job is not batchable as vector rows
    assert {r[1] for r in _accepted(results["bn_reduce_job_vector"])} >= {1, 4, 32, 64, 256}          # cvp: pow2ceil of C / V = 1, 3, 32, 33, 256, 257, capped at 256
    assert {r[1] for r in _accepted(results["bn_reduce_job_scalar"])} >= {2, 4, 8, 16, 32, 128, 256}
    assert {r[1] for r in _accepted(results["affine_job_rows"])} >= {1, 4, 32, 64, 256}
    # the LEAN table code and the plain one both give row plans (the LEAN bit is not part of the storage dtype here: fp32 | LEAN counts 8-element vectors)
    lean, plain = _accepted(results["bn_apply_job_lean"]), _accepted(results["bn_apply_job_rows"])
    assert len({tuple(r) for r in lean}) > 20 and len({tuple(r) for r in plain}) > 20 and lean != plain
    # finalize: every channels-per-block value, refusals of both kinds
    assert len({r[1] for r in _accepted(results["bn_bwd_finalize_job"])}) >= 3 and {-1, -2} <= {r[0] for r in results["bn_bwd_finalize_job"]}
    assert len({r[1] for r in _accepted(results["bn_finalize_job"])}) >= 3 and -1 in {r[0] for r in results["bn_finalize_job"]}
    assert {-1, -2} < set(results["copy_job"]) and 4096 in results["copy_job"] and {-1, -2} < {r[0] for r in results["colsum_job"]}
    assert {r[2] for r in _accepted(results["colsum_job"])} >= {1, 4, 32, 64, 256}
    for s in ("dwconv_blocks", "pairconv_blocks", "gate_blocks", "dwconv3x3_colsum_blocks", "dwconv3x3_wgrad_blocks", "rows_blocks"):
        assert -1 in results[s] and len(set(results[s])) > 8, (s, sorted(set(results[s]))[:12])
    assert set(results["ln_slots"]) == {-1, 4, 8, 16, 32}          # 4 * (64 / lanes per row), lanes = 8 .. 64
    assert set(results["colsum_unit"]) == {1, 2, 4, 8, 16, 32, 64, 128, 256}
    assert set(results["mutation_loss_width"]) - {-1} and results["mutation_loss_width"].count(-1) == 12


def check_recordable(res):
    """the recorder's own condition: no launching entry point got past its checks"""
    for f in FILES:
        bad = [(i, v) for i, v in enumerate(res[f"refusals_{f}"]) if v >= 0]
        if bad:
            sys.exit(f"refusals_{f}: {len(bad)} cases were NOT refused (index, result): {bad[:8]} - a launch was reached with fake pointers; fix the sweep")


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: [PN2_LIB=<library to record from>] python tests/test_launch_select_cpu.py --record")
    if any(v in os.environ for v in ENV_SWITCHES):
        sys.exit("unset PN2_DW_WIN and PN2_DW_SEG: the fixture holds the default geometry")
    from pn2 import capi
    res = sweep(capi)
    check_recordable(res)
    with open(FIXTURE, "w") as f:
        json.dump(res, f, separators=(",", ":"))
        f.write("\n")
    print(f"recorded {sum(len(v) for v in res.values())} results from {capi.LIB_PATH}:")
    for k, v in res.items():
        print(f"  {k:26s} {len(v):6d} results, {len({json.dumps(x) for x in v}):5d} distinct")
