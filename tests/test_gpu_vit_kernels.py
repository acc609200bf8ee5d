"""GPU tests of pn2_vit.hip, entry point by entry point through the C ABI against tests/vitref.py in float64: LayerNorm forward / backward on every lanes-per-row
plan, both backward instantiations and row loops of one, two and three trips; the column sums and their finalisation; the depth-wise 3x3 conv on the bf16
window kernels and the row walks of both dtypes (flip, bias, GELU, accumulate, the column-sum variant, a misaligned weight pointer, the two full-size plans);
its weight gradient with and without the fused dz = dy * gelu'(z); the hand-written erf through pn2_gelu_bwd and a centre-tap identity conv on a dense grid;
the DropPath scale; the capped grids.  Case tables, inputs, references and bound functions are vitref's (tests/test_vitref_cpu.py holds them to torch in
float64 and to the library's own plans, and shows that every route named here is reached).

Buffers: rows are `ld` wide where the entry point takes an ld; every buffer has a guard region BEFORE and AFTER it; outputs that are not accumulated into are
pre-filled with NaN, their pads and guards with a sentinel that has to survive bit for bit; pads and guards of inputs hold NaN.  The depth-wise tensors are
contiguous by contract and their guards are at least two image rows long: the window kernels address through a buffer descriptor that is not clipped at the
tensor's end, so a lost halo mask reads NaN and a lost store mask breaks a sentinel.

Tolerance rule (per element or per row, never one number per tensor; the functions and their derivation are in vitref's docstring):
  exact by definition   refusals write nothing; scale_samples without res in fp32 is float32(x * s); the centre-tap identity conv returns its input (bit for
                        bit, except that -0 comes back as +0: the sum starts from a +0 bias); a constant LayerNorm row gives y = beta; table launches equal
                        single launches; the column-sum variant of the conv stores the z of the plain call;
  fp32 sums             LayerNorm y / mean / rstd / dx per row: max(1e-5 * max|ref64 row|, 3 * max|ref32 - ref64| of that row);
  fp32 accumulations    n * 2^-24 * sum|terms| per output (column sums, cpart, weight-gradient partials and dgamma / dbeta partials summed over their blocks in
                        float64, the conv's ten terms); finalize rounds a double once: 2^-24 * |ref|; accumulate adds 2^-24 * (|old| + |new|);
  bf16 stores           + the half ulp 2^-8 * |ref64|;
  GELU / derivative     K * (2^-23 |z| + 2^-22 |gelu z|), K' * (2^-23 + 2^-22 |gelu' z|) with K, K' = 3 x the share torch's own fp32 CPU GELU reaches on the
                        same grid (measured at run time, at least 3); y_gelu of the conv adds 1.13 x the conv's bound;
  fused weight gradient dz_out against dy * gelu'(z) with the bf16 rule, then the partial sums against float64 sums of the READ-BACK dz_out (the kernel's
                        contract: it accumulates what it stores); pn2_dwconv3x3_colsum's cpart against the column sums of the READ-BACK z.
Every case prints its distance, ref32's and the share of the bound it used (run with -s, lines starting with VITK).

MI355X, 2026-10-19, on top of commit d778469 (largest share of the bound per family; fp32 / bf16):
  LayerNorm forward     y 0.33 / 0.99, mean 0.009 / 0.002, rstd 0.34 / 0.02 (the fp32 maxima on the rows with mean >> spread)
  LayerNorm backward    dx 0.49 / 0.99, dgamma 0.83 / 0.85, dbeta 0.58 / 0.004
  column sums           0.002 / 0.000; finalize 0.997 (one rounding of a double); DropPath scale 0.999 / 0.996
  depth-wise 3x3        z 0.59 / 0.996, y 0.13 / 0.995 (small shapes); full-size plans z 0.75 / 0.996, y 0.17 / 0.995; misaligned weights z 0.32 / 0.99;
                        cpart 0.009; every bf16 figure is the final rounding
  weight gradient       dz_out 0.15 / 0.996, gw 0.32 / 0.14, gb 0.16 / 0.04 (full-size plans: below 0.001)
  GELU                  torch's fp32 CPU GELU reaches 2.68 (derivative 1.19) of the bound's shape -> K = 8.03, K' = 3.57; the kernel 0.043 of the bound through
                        the identity conv (0.35 of the shape), its derivative 0.125; bf16 0.99 (the final rounding)
  window vs row kernel  bit-identical on every shape, (4,256,33,1024) included.  Before the row walk wrote its fused multiply-adds out (bf16 instantiations),
                        the compiler left a few of its products unfused and the two differed in the last fp32 bit or two: 0 or 1 ulp on the small shapes, but
                        17 of 34 603 008 elements of the full-size shape were more than one ulp apart, the worst 29 ulps, where the ten terms cancel (both
                        kernels at 0.996 of their float64 bound)."""
import ctypes as C
import functools

import pytest
import torch

import vitref as R

pytestmark = pytest.mark.gpu
dev = "cuda"
F64, F32 = torch.float64, torch.float32
TDT, DT = R.TDT, R.DT
IDT = {"fp32": torch.int32, "bf16": torch.int16}
SENT = 7.0
NAN = float("nan")


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pn2
    pn2.load_library()
    yield


def _lib():
    from pn2 import capi
    return capi.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def sync():
    torch.cuda.synchronize()


class Buf:
    """[M][ld] device rows of which [:, :C] is the tensor, between two guard regions of at least `guard` elements.  Pads and guards hold `pad`; the body holds
    `body` (a float64 tensor that must be representable in the dtype) or NaN.  `shift` moves the start by that many elements (a misaligned pointer)."""

    def __init__(self, M, Cc, ld, dt, body=None, pad=SENT, guard=0, shift=0):
        assert ld >= Cc
        self.G = (max(guard, ld, 64) + 63) // 64 * 64 + shift
        self.M, self.C, self.ld, self.dt = M, Cc, ld, dt
        self.t = torch.full((2 * self.G + M * ld,), pad, dtype=TDT[dt], device=dev)
        if body is None:
            self.rows()[:, :Cc] = NAN
        else:
            b = body.to(dev).reshape(M, Cc)
            rb = b.to(TDT[dt])
            assert bool((rb.to(F64) == b).all()), "input not representable"
            self.rows()[:, :Cc] = rb
        self.before = self.t.clone()

    def rows(self, t=None):
        return (self.t if t is None else t)[self.G:self.G + self.M * self.ld].view(self.M, self.ld)

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr() + self.G * self.t.element_size())

    def body_dev(self, shape=None):
        a = self.rows()[:, :self.C].to(F64)
        return a if shape is None else a.reshape(shape)

    def body(self, shape=None):
        return self.body_dev(shape).cpu()

    def bits(self):
        return self.rows()[:, :self.C].contiguous().view(IDT[self.dt])

    def pads_untouched(self):
        a, b = self.t.clone(), self.before.clone()
        self.rows(a)[:, :self.C] = 0
        self.rows(b)[:, :self.C] = 0
        return torch.equal(a.view(IDT[self.dt]), b.view(IDT[self.dt]))

    def unchanged(self):
        return torch.equal(self.t.view(IDT[self.dt]), self.before.view(IDT[self.dt]))


def inp(M, Cc, ld, dt, body, **kw):
    return Buf(M, Cc, ld, dt, body, pad=NAN, **kw)


def vec(v, **kw):
    """An fp32 parameter / scalar-per-row array as an input buffer."""
    return inp(1, v.numel(), v.numel(), "fp32", v, **kw)


def out(n, dt="fp32", body=None, **kw):
    return Buf(1, n, n, dt, body, **kw)


def ok(*bufs_in, outs=()):
    return all(b.unchanged() for b in bufs_in) and all(b.pads_untouched() for b in outs)


# ================================================================================================================ LayerNorm
@pytest.mark.parametrize("case", R.ln_cases(), ids=R.ln_id)
def test_layernorm_fwd_vs_float64(case):
    dt, Cc, M, form, eps, content = case
    data = R.ln_inputs(case)
    ld_x, ld_y, _, _ = R.ln_ld(dt, Cc, form)
    xb, yb, g, b = inp(M, Cc, ld_x, dt, data["x"]), Buf(M, Cc, ld_y, dt), vec(data["gamma"]), vec(data["beta"])
    mean, rstd = out(M), out(M)
    assert _lib().pn2_layernorm_fwd(DT[dt], xb.ptr, ld_x, yb.ptr, ld_y, M, Cc, g.ptr, b.ptr, eps, mean.ptr, rstd.ptr, _stream()) == 0
    sync()
    exp = R.ln_fwd_expect(case, data)
    got = dict(y=yb.body(), mean=mean.body().reshape(M), rstd=rstd.body().reshape(M))
    for name, (r64, r32, bound) in exp.items():
        R.check(f"ln_fwd {R.ln_id(case)} {name}", dt, got[name], r64, bound, r32)
    for r, kind in enumerate(R.ln_row_kinds(M, content)):
        if kind == "const":          # x - mean is exactly zero: y = beta whatever rstd is
            assert torch.equal(got["y"][r], R.rt(data["beta"], dt)), (r, "constant row")
    assert ok(xb, g, b, outs=(yb, mean, rstd))


@pytest.mark.parametrize("case", R.ln_cases(), ids=R.ln_id)
def test_layernorm_bwd_vs_float64(case):
    """Fresh and accumulating dx; dgamma / dbeta are the block partials summed in float64.  The saved statistics are the float64 ones rounded to fp32."""
    dt, Cc, M, form, eps, content = case
    data = R.ln_inputs(case)
    ld_x, _, ld_dy, ld_dx = R.ln_ld(dt, Cc, form)
    m, r = R.ln_saved(case, data)
    nblk = _lib().pn2_rows_blocks(M, _lib().pn2_ln_slots(DT[dt], Cc))
    assert nblk == R.rows_blocks(M, R.ln_slots(dt, Cc))
    for acc in (0, 1):
        xb, dyb, g, mb, rb = inp(M, Cc, ld_x, dt, data["x"]), inp(M, Cc, ld_dy, dt, data["dy"]), vec(data["gamma"]), vec(m), vec(r)
        dxb, pg, pb = Buf(M, Cc, ld_dx, dt, data["old"] if acc else None), Buf(nblk, Cc, Cc, "fp32"), Buf(nblk, Cc, Cc, "fp32")
        assert _lib().pn2_layernorm_bwd(DT[dt], dyb.ptr, ld_dy, xb.ptr, ld_x, M, Cc, g.ptr, mb.ptr, rb.ptr, dxb.ptr, ld_dx, acc, pg.ptr, pb.ptr, nblk, _stream()) == 0
        sync()
        exp = R.ln_bwd_expect(case, data, acc)
        got = dict(dx=dxb.body(), dgamma=pg.body().sum(0), dbeta=pb.body().sum(0))
        for name, (r64, r32, bound) in exp.items():
            R.check(f"ln_bwd acc{acc} {R.ln_id(case)} {name}", dt, got[name], r64, bound, r32)
        assert ok(xb, dyb, g, mb, rb, outs=(dxb, pg, pb))


@pytest.mark.parametrize("dt", list(R.VEC))
def test_layernorm_refusals_write_nothing(dt):
    for Cc in R.LN_REFUSED[dt]:
        M, ld = 5, Cc + 16
        x = R.values("ln_refused", (M, Cc), dt)
        xb, yb, dxb, g = inp(M, Cc, ld, dt, x), Buf(M, Cc, ld, dt), Buf(M, Cc, ld, dt), vec(R.values("g", (Cc,), "fp32"))
        mean, rstd, pg, pb = out(M), out(M), out(Cc), out(Cc)
        assert _lib().pn2_layernorm_fwd(DT[dt], xb.ptr, ld, yb.ptr, ld, M, Cc, g.ptr, g.ptr, 1e-5, mean.ptr, rstd.ptr, _stream()) == -2
        assert _lib().pn2_layernorm_bwd(DT[dt], xb.ptr, ld, xb.ptr, ld, M, Cc, g.ptr, mean.ptr, rstd.ptr, dxb.ptr, ld, 0, pg.ptr, pb.ptr, 1, _stream()) == -2
        sync()
        assert all(b.unchanged() for b in (xb, yb, dxb, g, mean, rstd, pg, pb))


# ================================================================================================================ column sums
@pytest.mark.parametrize("case", R.colsum_cases(), ids=str)
def test_colsum_vs_float64(case):
    dt, Cc, M, ld = case
    x = R.values("colsum", (M, Cc), dt)
    cvp, rows, nblk = R.colsum_plan(dt, M, Cc, ld)
    assert nblk == _lib().pn2_rows_blocks(M, _lib().pn2_colsum_unit(DT[dt], Cc))
    xb, part = inp(M, Cc, ld, dt, x), Buf(nblk, Cc, Cc, "fp32")
    assert _lib().pn2_colsum(DT[dt], xb.ptr, ld, M, Cc, part.ptr, nblk, _stream()) == 0
    sync()
    R.check(f"colsum {case}", dt, part.body().sum(0), R.colsum_ref(x), R.nterm_bound(M, x.abs().sum(0)), R.colsum_ref(x, F32))
    assert ok(xb, outs=(part,))
    assert _lib().pn2_colsum(DT[dt], xb.ptr, ld, M, Cc, part.ptr, nblk + 1, _stream()) == -2          # a block count other than the plan's: refused


@pytest.mark.parametrize("Cc", R.FIN_C)
@pytest.mark.parametrize("nblk", R.FIN_NBLK)
def test_colsum_finalize_vs_float64(nblk, Cc):
    """Double accumulation, one rounding: 2^-24 * |ref| (+ 2^-24 * (|old| + |new|) when it accumulates)."""
    for ld in (Cc, Cc + 3):
        p, old = R.values("fin_p", (nblk, Cc), "fp32"), R.values("fin_old", (Cc,), "fp32")
        for acc in (0, 1):
            pbuf, ob = inp(nblk, Cc, ld, "fp32", p), out(Cc, body=old if acc else None)
            assert _lib().pn2_colsum_finalize(pbuf.ptr, nblk, Cc, ld, ob.ptr, acc, _stream()) == 0
            sync()
            new = p.sum(0)
            R.check(f"finalize nblk{nblk} C{Cc} ld{ld} acc{acc}", "fp32", ob.body().reshape(Cc), new + old if acc else new,
                    R.U24 * new.abs() + (R.acc_bound(old, new) if acc else 0), (p.to(F32).sum(0) + (old.to(F32) if acc else 0)))
            assert ok(pbuf, outs=(ob,))


def _table(jobs):
    arr = (type(jobs[0]) * len(jobs))(*jobs)
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)


@pytest.mark.parametrize("dt", list(R.VEC))
def test_colsum_tables_equal_single_launches(dt):
    """pn2_colsum_multi and pn2_colsum_finalize_multi against one launch per job: bit for bit."""
    from pn2 import capi
    lib, V = _lib(), R.VEC[dt]
    cases = [(V, 255, V), (320, 3, 320 + V), (257 * V, 2, 257 * V), (64, 1500, 64)]
    xs = [inp(M, Cc, ld, dt, R.values("tbl", (M, Cc), dt)) for Cc, M, ld in cases]
    single, multi, jobs, fjobs, start, fstart = [], [], [], [], [0], [0]
    for (Cc, M, ld), xb in zip(cases, xs):
        j = capi.ColsumInJob()
        j.dy, j.M, j.C, j.ld = xb.ptr.value, M, Cc, ld
        j.partial = 4096
        nblk = lib.pn2_colsum_job_blocks(DT[dt], C.byref(j))
        assert nblk == R.colsum_plan(dt, M, Cc, ld)[2]
        s, m = Buf(nblk, Cc, Cc, "fp32"), Buf(nblk, Cc, Cc, "fp32")
        j.partial = m.ptr.value
        assert lib.pn2_colsum(DT[dt], xb.ptr, ld, M, Cc, s.ptr, nblk, _stream()) == 0
        single.append(s), multi.append(m), jobs.append(j), start.append(start[-1] + nblk)
    bs = torch.tensor(start, dtype=torch.int32, device=dev)
    tbl = _table(jobs)
    assert lib.pn2_colsum_multi(DT[dt], C.c_void_p(tbl.data_ptr()), C.c_void_p(bs.data_ptr()), len(jobs), start[-1], _stream()) == 0
    sync()
    for s, m in zip(single, multi):
        assert torch.equal(s.t.view(torch.int32), m.t.view(torch.int32))
    fs, fm = [], []
    for i, ((Cc, M, ld), s) in enumerate(zip(cases, single)):
        old = R.values("tbl_old", (Cc,), "fp32")
        a, b = out(Cc, body=old if i % 2 else None), out(Cc, body=old if i % 2 else None)
        assert lib.pn2_colsum_finalize(s.ptr, s.M, Cc, Cc, a.ptr, i % 2, _stream()) == 0
        j = capi.ColsumJob()
        j.partial, j.out, j.nblk, j.C, j.ld, j.accumulate = s.ptr.value, b.ptr.value, s.M, Cc, Cc, i % 2
        fs.append(a), fm.append(b), fjobs.append(j), fstart.append(fstart[-1] + lib.pn2_colsum_finalize_blocks(Cc))
    bs, tbl = torch.tensor(fstart, dtype=torch.int32, device=dev), _table(fjobs)
    assert lib.pn2_colsum_finalize_multi(C.c_void_p(tbl.data_ptr()), C.c_void_p(bs.data_ptr()), len(fjobs), fstart[-1], _stream()) == 0
    sync()
    for a, b in zip(fs, fm):
        assert torch.equal(a.t.view(torch.int32), b.t.view(torch.int32)) and bool(torch.isfinite(a.body()).all())


# ================================================================================================================ depth-wise 3x3
@functools.lru_cache(maxsize=2)
def _dw_inputs(shape, dt, device):
    return R.dw_inputs(shape, dt, device)


def _dw_bufs(shape, dt, data, acc, gelu, shift=0):
    N, H, W, Cc = shape
    M, guard = N * H * W, 2 * W * Cc
    xb = inp(M, Cc, Cc, dt, data["x"], guard=guard)
    zb = Buf(M, Cc, Cc, dt, data["old"] if acc else None, guard=guard)
    yb = Buf(M, Cc, Cc, dt, guard=guard) if gelu else None
    return xb, zb, yb, vec(data["w"].reshape(-1), shift=shift), vec(data["b"])


def run_dw(shape, dt, data, flip, bias, gelu, acc, shift=0, tag=""):
    """One pn2_dwconv3x3 call against float64; -> the z buffer."""
    N, H, W, Cc = shape
    xb, zb, yb, wb, bb = _dw_bufs(shape, dt, data, acc, gelu, shift)
    assert (wb.ptr.value % 16 == 0) == (shift == 0)
    assert _lib().pn2_dwconv3x3(DT[dt], xb.ptr, wb.ptr, bb.ptr if bias else None, zb.ptr, yb.ptr if gelu else None, N, H, W, Cc, flip, acc, _stream()) == 0
    sync()
    exp = R.dw_expect(data, dt, flip, bias, gelu, acc)
    p = R.dw_plan(dt, gelu, acc, *shape)
    route = f"{'win' if p['win'] else 'row'}{p['VT']}seg{p['SEG']}"
    for name, b in (("z", zb), ("y", yb)):
        if b is not None:
            r64, r32, bound = exp[name]
            R.check(f"dw{tag} {shape} f{flip}b{bias}g{gelu}a{acc}[{route}] {name}", dt, b.body_dev(shape), r64, bound, r32)
    assert ok(xb, wb, bb, outs=[b for b in (zb, yb) if b is not None])
    return zb


def run_dw_colsum(shape, dt, data, flip, bias, zplain):
    """pn2_dwconv3x3_colsum: the z of the plain call, and cpart summed over its rows against the column sums of the stored z."""
    N, H, W, Cc = shape
    nblk = _lib().pn2_dwconv3x3_colsum_blocks(DT[dt], N, H, W, Cc)
    assert nblk == R.dw_colsum_blocks(dt, N, H, W, Cc)
    if nblk < 0:
        return
    xb, zb, _, wb, bb = _dw_bufs(shape, dt, data, 0, 0)
    cp = Buf(nblk, Cc, Cc, "fp32")
    assert _lib().pn2_dwconv3x3_colsum(DT[dt], xb.ptr, wb.ptr, bb.ptr if bias else None, zb.ptr, N, H, W, Cc, flip, cp.ptr, nblk, _stream()) == 0
    sync()
    assert torch.equal(zb.bits(), zplain.bits())
    z = zb.body_dev()
    R.check(f"dw_colsum {shape} f{flip}b{bias}", dt, cp.body_dev().sum(0), z.sum(0), R.nterm_bound(N * H * W, z.abs().sum(0)), z.to(F32).sum(0))
    assert ok(xb, wb, bb, outs=(zb, cp))


@pytest.mark.parametrize("dt", list(R.VEC))
@pytest.mark.parametrize("shape", R.DW_SHAPES, ids=str)
def test_dwconv3x3_vs_float64(shape, dt):
    """flip x bias x GELU x accumulate on every small shape; the column-sum variant wherever the library serves it."""
    data = R.dw_inputs(shape, dt)
    for flip, bias, gelu, acc in R.DW_COMBOS:
        zb = run_dw(shape, dt, data, flip, bias, gelu, acc)
        if not gelu and not acc:
            run_dw_colsum(shape, dt, data, flip, bias, zb)


@pytest.mark.parametrize("dt", list(R.VEC))
@pytest.mark.parametrize("shape", R.DW_WALIGN_SHAPES, ids=str)
def test_dwconv3x3_misaligned_weights(shape, dt):
    """The weight pointer one float off a 16-byte boundary (a slice of a flat parameter buffer): scalar weight loads, same results."""
    data = R.dw_inputs(shape, dt)
    for flip, gelu, acc in ((0, 1, 0), (1, 0, 0), (1, 0, 1), (0, 1, 1)):
        run_dw(shape, dt, data, flip, 1, gelu, acc, shift=1, tag="_walign0")


@pytest.mark.parametrize("flip,bias", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("dt", list(R.VEC))
def test_dwconv3x3_full_size_plans(dt, flip, bias):
    """bf16 (4,256,33,1024): the 32-pixel-segment plan of the window kernels (segments of 17 = 5 * 3 + 2 and 16) and, accumulating, the 8-channel row walk;
    fp32 (2,256,17,1024): the 4-channel row walk.  Reference and comparisons stay on the device; only scalars reach the host."""
    shape = R.DW_LARGE[dt]
    data = _dw_inputs(shape, dt, dev)
    for gelu in (0, 1):
        for acc in (0, 1):
            zb = run_dw(shape, dt, data, flip, bias, gelu, acc, tag="_full")
            if not gelu and not acc:
                run_dw_colsum(shape, dt, data, flip, bias, zb)


def _ordered(bits16):
    """bf16 bit patterns -> integers in the order of the values (one step = one ulp)."""
    b = bits16.to(torch.int32) & 0xffff
    return torch.where(b >= 0x8000, 0x8000 - b, b)


@pytest.mark.parametrize("shape", R.DW_SHAPES + (R.DW_LARGE["bf16"],), ids=str)
def test_dwconv3x3_window_and_row_kernels_agree(shape):
    """bf16: accumulate = 1 onto zeros takes the row kernel, accumulate = 0 the window kernel; each is within its bound of float64 (run_dw) and they differ by
    at most one bf16 ulp."""
    device = dev if shape == R.DW_LARGE["bf16"] else "cpu"
    data = dict(_dw_inputs(shape, "bf16", device))
    data["old"] = torch.zeros_like(data["x"])
    assert R.dw_plan("bf16", 0, 0, *shape)["win"] and not R.dw_plan("bf16", 0, 1, *shape)["win"]
    for flip in (0, 1):
        zw, zr = run_dw(shape, "bf16", data, flip, 1, 0, 0, tag="_agree"), run_dw(shape, "bf16", data, flip, 1, 0, 1, tag="_agree")
        ulps = (_ordered(zw.bits()) - _ordered(zr.bits())).abs()
        print(f"\nVITK dw_agree {shape} f{flip}: max {int(ulps.max())} bf16 ulps apart, {int((ulps > 1).sum())} of {ulps.numel()} elements more than one")
        assert int(ulps.max()) <= 1


# ---------------------------------------------------------------------------------------------------------------- weight gradient
def run_wgrad(shape, dt, data, zpre, tag=""):
    N, H, W, Cc = shape
    M, guard = N * H * W, 2 * W * Cc
    nchunk = _lib().pn2_dwconv3x3_wgrad_blocks(DT[dt], N, H, W, Cc)
    p = R.dw_wgrad_plan(dt, *shape)
    assert nchunk == p["nchunk"]
    dyb, xb, zpb = inp(M, Cc, Cc, dt, data["dy"], guard=guard), inp(M, Cc, Cc, dt, data["x"], guard=guard), inp(M, Cc, Cc, dt, data["zpre"], guard=guard)
    dzo, part = Buf(M, Cc, Cc, dt, guard=guard), Buf(nchunk, 10 * Cc, 10 * Cc, "fp32")
    assert _lib().pn2_dwconv3x3_wgrad(DT[dt], dyb.ptr, xb.ptr, part.ptr, nchunk, N, H, W, Cc, zpb.ptr if zpre else None, dzo.ptr if zpre else None, _stream()) == 0
    sync()
    route = f"{'win' if p['win'] else 'row'}{p['VT']}seg{p['SEG']}chunks{nchunk}"
    dz = data["dy"]
    if zpre:
        r64, r32, bound = R.dz_expect(data, dt)
        dz = dzo.body_dev(shape).to(data["x"].device)          # what the kernel stored: the sums below are formed from it
        R.check(f"wgrad_dz{tag} {shape}[{route}]", dt, dz, r64, bound, r32)
    else:
        assert dzo.unchanged()
    s = part.body_dev().sum(0)
    got = dict(gw=s[:9 * Cc].reshape(Cc, 9), gb=s[9 * Cc:])
    for name, (r64, r32, bound) in R.wgrad_expect(dz, data["x"]).items():
        R.check(f"wgrad{tag} {shape} zpre{int(zpre)}[{route}] {name}", dt, got[name], r64, bound, r32)
    assert ok(dyb, xb, zpb, outs=(dzo, part))


@pytest.mark.parametrize("zpre", [False, True])
@pytest.mark.parametrize("dt", list(R.VEC))
@pytest.mark.parametrize("shape", R.DW_SHAPES, ids=str)
def test_dwconv3x3_wgrad_vs_float64(shape, dt, zpre):
    run_wgrad(shape, dt, R.dw_inputs(shape, dt), zpre)


@pytest.mark.parametrize("zpre", [False, True])
@pytest.mark.parametrize("dt", list(R.VEC))
def test_dwconv3x3_wgrad_full_size_plans(dt, zpre):
    run_wgrad(R.DW_LARGE[dt], dt, _dw_inputs(R.DW_LARGE[dt], dt, dev), zpre, tag="_full")


# ================================================================================================================ GELU: the hand-written erf on a grid
@pytest.mark.parametrize("dt", list(R.VEC))
def test_gelu_derivative_on_grid(dt):
    """pn2_gelu_bwd with dy = 1 is gelu'(z): both polynomial pieces, the switch points and the clamp with their neighbouring floats."""
    z = R.gelu_grid(dt)
    n = z.numel()
    zb, dyb, dzb = inp(1, n, n, dt, z), inp(1, n, n, dt, torch.ones(n, dtype=F64)), out(n, dt)
    assert _lib().pn2_gelu_bwd(DT[dt], dyb.ptr, zb.ptr, dzb.ptr, n, _stream()) == 0
    sync()
    K = R.gelu_scales()
    print(f"\nVITK gelu scale: torch fp32 shares {R._SCALES['torch_share']} -> K {K}")
    R.check("gelu_grad grid", dt, dzb.body().reshape(n), R.gelu_grad_ref(z), R.gelu_grad_bound(z, dt), R.gelu_grad_ref(z, F32))
    assert ok(zb, dyb, outs=(dzb,))


@pytest.mark.parametrize("dt", list(R.VEC))
def test_gelu_through_identity_conv(dt):
    """A centre-tap weight of 1 and no bias: z = x exactly and y = gelu(x), the erf as gelu_f2 uses it."""
    z = R.gelu_grid(dt)
    n, Cc = z.numel(), 8
    shape = (1, 160, 160, Cc) if dt == "fp32" else (1, 1, n // Cc, Cc)
    assert shape[1] * shape[2] * Cc == n
    w = torch.zeros(Cc, 9, dtype=F64)
    w[:, 4] = 1.0
    data = dict(x=z.reshape(shape), w=w)
    for acc_route in ((0,) if dt == "fp32" else (0, 1)):          # bf16: the window kernel, and the row kernel accumulating onto zeros
        data["old"] = torch.zeros(shape, dtype=F64)
        xb, zb, yb, wb, _ = _dw_bufs(shape, dt, dict(data, b=torch.zeros(Cc, dtype=F64)), acc_route, 1)
        assert _lib().pn2_dwconv3x3(DT[dt], xb.ptr, wb.ptr, None, zb.ptr, yb.ptr, *shape, 0, acc_route, _stream()) == 0
        sync()
        got = zb.body(shape)
        assert torch.equal(got, data["x"])
        nz = (data["x"] != 0).reshape(-1, Cc)
        assert torch.equal(zb.bits().cpu()[nz], xb.bits().cpu()[nz])
        R.check(f"gelu grid via conv acc{acc_route}", dt, yb.body(shape), R.gelu_ref(data["x"]), R.gelu_bound(data["x"], dt), R.gelu_ref(data["x"], F32))
        assert ok(xb, wb, outs=(zb, yb))


# ================================================================================================================ DropPath scale, capped grids
@pytest.mark.parametrize("dt", list(R.VEC))
def test_scale_samples_vs_float64(dt):
    n = R.SCALE_VECS * R.VEC[dt]
    x, res, s = R.values("scale_x", (3, n), dt), R.values("scale_r", (3, n), dt), torch.tensor(R.SCALES, dtype=F32).to(F64)
    for r in (None, res):
        xb, rb, sb, yb = inp(3, n, n, dt, x), inp(3, n, n, dt, res), vec(s), Buf(3, n, n, dt)
        assert _lib().pn2_scale_samples(DT[dt], xb.ptr, yb.ptr, sb.ptr, rb.ptr if r is not None else None, 3, n, _stream()) == 0
        sync()
        ref = R.scale_ref(x, s, r)
        if dt == "fp32" and r is None:
            assert torch.equal(yb.body(), R.rt(ref, "fp32"))
        R.check(f"scale_samples res{int(r is not None)}", dt, yb.body(), ref, R.scale_bound(x, s, r, dt), R.scale_ref(x, s, r, F32))
        assert bool((yb.body()[0] == (0 if r is None else res[0])).all())
        assert ok(xb, rb, sb, outs=(yb,))


def test_scale_samples_capped_grid():
    """Just above 16384 * 256 vectors: the grid-stride loop takes a second trip (fp32, exact)."""
    n = R.CAP_VECS // 3 * 4
    x, s = R.values("cap_x", (3, n), "fp32").to(dev), torch.tensor(R.SCALES[::-1], dtype=F32).to(F64)
    xb, sb, yb = inp(3, n, n, "fp32", x), vec(s), Buf(3, n, n, "fp32")
    assert _lib().pn2_scale_samples(DT["fp32"], xb.ptr, yb.ptr, sb.ptr, None, 3, n, _stream()) == 0
    sync()
    assert torch.equal(yb.body_dev(), (x * s.to(dev)[:, None]).to(F32).to(F64))
    assert ok(xb, sb, outs=(yb,))


def test_gelu_bwd_capped_grid():
    """The same for pn2_gelu_bwd (bf16); reference and comparison on the device."""
    n = R.CAP_VECS * 8
    z, dy = R.values("cap_z", (n,), "bf16", 2.0).to(dev), R.values("cap_dy", (n,), "bf16").to(dev)
    zb, dyb, dzb = inp(1, n, n, "bf16", z), inp(1, n, n, "bf16", dy), out(n, "bf16")
    assert _lib().pn2_gelu_bwd(DT["bf16"], dyb.ptr, zb.ptr, dzb.ptr, n, _stream()) == 0
    sync()
    r64, r32, bound = R.dz_expect(dict(dy=dy, zpre=z), "bf16")
    R.check("gelu_bwd capped grid", "bf16", dzb.body_dev().reshape(n), r64, bound, r32)
    assert ok(zb, dyb, outs=(dzb,))
