"""GPU tests of pn2_spatial.hip, entry point by entry point through the C ABI against tests/spatialref.py in float64: max / average pooling, bilinear resizing and
its adjoint on every dispatch path, the element-wise ops, the table copy, the layout conversion and the bias gradient.  The case tables and inputs are spatialref's
(tests/test_spatialref_cpu.py holds them to torch in float64 and to the dispatch predicates).

Every output and accumulate buffer is `ld` wide with ld > C where the path allows it, followed by a guard row, both pre-filled with a sentinel that has to survive
bit for bit; the pad columns of the inputs hold NaN (a kernel that read them would show it), and so does the body of an output that is not accumulated into.

Tolerance rule (the project's own, no number taken from a kernel):
  exact by definition   max-pool y and idx, non-accumulating fp32 add / mul, non-accumulating same-dtype copies and bf16 -> fp32, layout and pad zeros, table
                        launch vs single launches;
  fp32 otherwise        |ours - ref64| <= max(1e-5 * max|ref64|, 3 * max|ref32 - ref64|) per case: ref32 is the same reference in fp32 on the CPU, the factor 3 allows
                        another summation order, the floor is the bound test_pool_and_bilinear_ops already holds these ops to;
  accumulating fp32 element-wise   2^-23 * (|old| + |new|) per element (one rounding of the product and one of the sum, whether or not they contract into an FMA);
  bf16                  inputs are bf16 numbers, sums run in fp32 and round once: per element 2^-8 * |ref64| + the fp32 bound of the same case;
                        the engine's separable route gets 2 * 2^-8.  2^-8 * |v| is a bf16 ulp only at the top of a binade; at the bottom (v just above a power
                        of two) the ulp is 2^-7 * |v| and 2^-8 * |v| is exactly the half ulp of round-to-nearest, which the measured shares of 0.99 - 1.00
                        reach: the rule has no room for an f2bf that truncates or rounds another way.
Every case prints its distance, ref32's and the share of the bound it used (run with -s, lines starting with SPATK)."""
import ctypes as C

import numpy as np
import pytest
import torch

import spatialref as R

pytestmark = pytest.mark.gpu
dev = "cuda"

TDT = {"fp32": torch.float32, "bf16": torch.bfloat16}
IDT = {"fp32": torch.int32, "bf16": torch.int16}
DT = {"fp32": 0, "bf16": 1}
SENT = 7.0
N = R.N_IMG
BF_ULP = 2.0 ** -8


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pn2
    pn2.load_library()
    yield
    pn2.set_compute_dtype("bf16")


def _lib():
    from pn2 import capi
    return capi.load()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Buf:
    """[M][ld] device rows of which [:, :C] is the tensor, plus one guard row.  Pads and guard hold `pad`; the body holds `body` (an array) or NaN."""

    def __init__(self, M, Cc, ld, dt, body=None, pad=SENT):
        assert ld >= Cc
        t = torch.full((M + 1, ld), pad, dtype=TDT[dt])
        t[:M, :Cc] = float("nan") if body is None else torch.from_numpy(np.asarray(body, dtype=np.float64).reshape(M, Cc)).to(TDT[dt])
        if body is not None:
            assert np.array_equal(t[:M, :Cc].double().numpy(), np.asarray(body, dtype=np.float64).reshape(M, Cc), equal_nan=True), "input not representable"
        self.M, self.C, self.ld, self.dt = M, Cc, ld, dt
        self.before = t.clone()
        self.t = t.to(dev)

    @property
    def ptr(self):
        return _p(self.t)

    def body(self, shape=None):
        a = self.t.cpu()[:self.M, :self.C].double().numpy()
        return a if shape is None else a.reshape(shape)

    def _bits(self, t):
        return t.contiguous().view(IDT[self.dt])

    def pads_untouched(self):
        out = self.t.cpu()
        return torch.equal(self._bits(out[:self.M, self.C:]), self._bits(self.before[:self.M, self.C:])) and torch.equal(self._bits(out[self.M]), self._bits(self.before[self.M]))

    def unchanged(self):
        return torch.equal(self._bits(self.t.cpu()), self._bits(self.before))


def inp(M, Cc, ld, dt, body):
    return Buf(M, Cc, ld, dt, body, pad=float("nan"))


def fp32_bound(ref64, ref32):
    d32 = float(np.abs(ref32.astype(np.float64) - ref64).max()) if ref64.size else 0.0
    return max(1e-5 * (float(np.abs(ref64).max()) if ref64.size else 0.0), 3 * d32), d32


def check(tag, ours, ref64, ref32, dt, bf=1.0):
    """The rule of the module docstring for everything that sums."""
    assert ours.shape == ref64.shape and np.isfinite(ours).all(), tag
    b32, d32 = fp32_bound(ref64, ref32)
    bound = b32 + (bf * BF_ULP * np.abs(ref64) if dt == "bf16" else 0.0) + np.zeros_like(ref64)
    d = np.abs(ours - ref64)
    ratio = float(np.where(bound > 0, d / np.where(bound > 0, bound, 1), np.where(d > 0, np.inf, 0)).max()) if d.size else 0.0
    print(f"\nSPATK {tag} {dt}: ours {float(d.max()):.2e} ref32 {d32:.2e} of-bound {ratio:.3f}")
    assert ratio <= 1.0, (tag, dt, float(d.max()), d32)


def check_ew(tag, ours, ref64, old, new, dt):
    """Element-wise results: exact in fp32 when nothing is accumulated, else 2^-23 * (|old| + |new|); bf16 adds its ulp."""
    assert np.isfinite(ours).all(), tag
    if dt == "fp32" and old is None:
        assert np.array_equal(ours, ref64.astype(np.float32).astype(np.float64)), tag
        return
    bound = 2.0 ** -23 * ((0 if old is None else np.abs(old)) + np.abs(new)) + (BF_ULP * np.abs(ref64) if dt == "bf16" else 0.0)
    d = np.abs(ours - ref64)
    ratio = float((d / np.maximum(bound, 1e-300)).max())
    print(f"\nSPATK {tag} {dt}: ours {float(d.max()):.2e} of-bound {ratio:.3f}")
    assert ratio <= 1.0, (tag, dt)


def forms(table):
    """(form, dtype) pairs of a {form: {dtype: ...}} table."""
    return [(f, dt) for f, per in table.items() for dt in per]


def _ids(v):
    return "x".join(str(a) for a in v) if isinstance(v, tuple) else str(v)


# ================================================================================================================ max pool
@pytest.mark.parametrize("kind", R.MAXPOOL_KINDS)
@pytest.mark.parametrize("shape", R.MAXPOOL_SHAPES, ids=_ids)
@pytest.mark.parametrize("form,dt", forms(R.POOL_FORMS))
def test_maxpool_vs_float64(form, dt, shape, kind):
    """y and the tap index equal the reference exactly (first maximum in row-major tap order, the last NaN wins, an all -inf window names its first in-image
    tap); dx meets the rule and is exact wherever at most one window names the element."""
    H, W = shape
    Cc, ld_x, ld_y = R.POOL_FORMS[form][dt]
    OH, OW = R.pool_out(H), R.pool_out(W)
    x = R.maxpool_input(kind, H, W, Cc)
    xb, yb = inp(N * H * W, Cc, ld_x, dt, x), Buf(N * OH * OW, Cc, ld_y, dt)
    idx = torch.full((N * OH * OW + 1, Cc), 255, dtype=torch.uint8, device=dev)
    assert _lib().pn2_maxpool3x3s2_fwd(DT[dt], xb.ptr, ld_x, yb.ptr, ld_y, _p(idx), N, H, W, Cc, OH, OW, _stream()) == 0
    torch.cuda.synchronize()
    y_ref, idx_ref = R.maxpool_ref(x)
    y = yb.body(y_ref.shape)
    num = ~np.isnan(y_ref)
    assert np.array_equal(y, y_ref, equal_nan=True) and np.array_equal(np.signbit(y[num]), np.signbit(y_ref[num]))
    got = idx.cpu().numpy()
    assert np.array_equal(got[:-1].reshape(idx_ref.shape), idx_ref) and (got[-1] == 255).all()
    assert yb.pads_untouched() and xb.unchanged()

    dy = R.values(f"maxpool_dy_{kind}", y_ref.shape)
    dyb, dxb = inp(N * OH * OW, Cc, ld_y, dt, dy), Buf(N * H * W, Cc, ld_y, dt)
    assert _lib().pn2_maxpool3x3s2_bwd(DT[dt], dyb.ptr, ld_y, _p(idx), dxb.ptr, ld_y, N, H, W, Cc, OH, OW, _stream()) == 0
    torch.cuda.synchronize()
    dx = dxb.body((N, H, W, Cc))
    ref64, ref32 = R.maxpool_bwd_ref(dy, idx_ref, H, W), R.maxpool_bwd_ref(dy, idx_ref, H, W, np.float32)
    check(f"maxpool_bwd {form} {H}x{W} {kind}", dx, ref64, ref32, dt)
    single = R.maxpool_contributions(idx_ref, H, W) <= 1
    assert np.array_equal(dx[single], ref64[single])
    assert dxb.pads_untouched() and dyb.unchanged()


# ================================================================================================================ average pool
@pytest.mark.parametrize("cfg", R.AVG_SETS, ids=_ids)
@pytest.mark.parametrize("shape", R.AVG_SHAPES, ids=_ids)
@pytest.mark.parametrize("form,dt", forms(R.POOL_FORMS))
def test_avgpool_vs_float64(form, dt, shape, cfg):
    H, W = shape
    k, s, p, ceil, inc = cfg
    Cc, ld_x, ld_y = R.POOL_FORMS[form][dt]
    OH, OW = R.avg_out(H, k, s, p, ceil), R.avg_out(W, k, s, p, ceil)
    x = R.values("avgpool_x", (N, H, W, Cc))
    xb, yb = inp(N * H * W, Cc, ld_x, dt, x), Buf(N * OH * OW, Cc, ld_y, dt)
    assert _lib().pn2_avgpool_fwd(DT[dt], xb.ptr, ld_x, yb.ptr, ld_y, N, H, W, Cc, OH, OW, k, s, p, int(inc), _stream()) == 0
    torch.cuda.synchronize()
    tag = f"{form} {H}x{W} k{k}s{s}p{p}{'c' if ceil else 'f'}{'i' if inc else 'e'}"
    check("avgpool_fwd " + tag, yb.body((N, OH, OW, Cc)), R.avgpool_ref(x, *cfg), R.avgpool_ref(x, *cfg, dtype=np.float32), dt)
    assert yb.pads_untouched() and xb.unchanged()
    dy, old = R.values("avgpool_dy", (N, OH, OW, Cc)), R.values("avgpool_old", (N, H, W, Cc))
    for acc in (0, 1):
        dyb, dxb = inp(N * OH * OW, Cc, ld_y, dt, dy), Buf(N * H * W, Cc, ld_y, dt, old if acc else None)
        assert _lib().pn2_avgpool_bwd(DT[dt], dyb.ptr, ld_y, dxb.ptr, ld_y, N, H, W, Cc, OH, OW, k, s, p, int(inc), acc, _stream()) == 0
        torch.cuda.synchronize()
        refs = [(old.astype(t) if acc else 0) + R.avgpool_bwd_ref(dy, H, W, *cfg, dtype=t) for t in (np.float64, np.float32)]
        check(f"avgpool_bwd acc{acc} " + tag, dxb.body((N, H, W, Cc)), refs[0], refs[1], dt)
        assert dxb.pads_untouched() and dyb.unchanged()


# ================================================================================================================ bilinear
def _bilinear_fwd(dt, x, ld_x, ld_y, OH, OW, ac, rh, rw):
    n, H, W, Cc = x.shape
    xb, yb = inp(n * H * W, Cc, ld_x, dt, x), Buf(n * OH * OW, Cc, ld_y, dt)
    assert _lib().pn2_bilinear_fwd(DT[dt], xb.ptr, ld_x, yb.ptr, ld_y, n, H, W, Cc, OH, OW, ac, rh, rw, _stream()) == 0
    torch.cuda.synchronize()
    assert yb.pads_untouched() and xb.unchanged()
    return yb.body((n, OH, OW, Cc))


@pytest.mark.parametrize("ac", [0, 1])
@pytest.mark.parametrize("geom", R.BL_FWD_GEOMS)
@pytest.mark.parametrize("form,dt", [(f, dt) for f, v in R.BL_FWD_FORMS.items() for dt in v[1]])
def test_bilinear_fwd_vs_float64(form, dt, geom, ac):
    """The reference's matrices are built from the fp32-rounded ratios the C call receives."""
    _, _, Cc, ld_x, ld_y = R.BL_FWD_FORMS[form]
    H, W, OH, OW, _ = R.GEOMS[geom]
    rh, rw = R.ratios(geom, ac)
    x = R.values("bilinear_x", (N, H, W, Cc))
    y = _bilinear_fwd(dt, x, ld_x, ld_y, OH, OW, ac, rh, rw)
    refs = [R.bilinear_ref(x, OH, OW, ac, R.f32(rh), R.f32(rw), t) for t in (np.float64, np.float32)]
    check(f"bilinear_fwd {form} {geom} ac{ac}", y, refs[0], refs[1], dt)


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("ac", [0, 1])
@pytest.mark.parametrize("case,dt", [(c, dt) for c, v in R.BL_BWD_CASES.items() for dt in v[1]])
def test_bilinear_bwd_vs_float64(case, dt, ac, acc):
    """One case per path of pn2_bilinear_bwd (the two sub-paths of the row kernel with R = 4 / 2 / 1 row lanes, the wave kernel, 12-byte, vector, scalar) and the
    r = 0 window of align_corners with a single output, fresh and accumulating onto a non-zero dx."""
    path, _, geom, Cc, ld_dy, ld_dx = R.BL_BWD_CASES[case]
    H, W, OH, OW, _ = R.GEOMS[geom]
    rh, rw = R.ratios(geom, ac)
    dy, old = R.values("bilinear_dy", (N, OH, OW, Cc)), R.values("bilinear_old", (N, H, W, Cc))
    dyb, dxb = inp(N * OH * OW, Cc, ld_dy, dt, dy), Buf(N * H * W, Cc, ld_dx, dt, old if acc else None)
    assert _lib().pn2_bilinear_bwd(DT[dt], dyb.ptr, ld_dy, dxb.ptr, ld_dx, N, H, W, Cc, OH, OW, ac, rh, rw, acc, _stream()) == 0
    torch.cuda.synchronize()
    refs = [(old.astype(t) if acc else 0) + R.bilinear_bwd_ref(dy, H, W, ac, R.f32(rh), R.f32(rw), t) for t in (np.float64, np.float32)]
    check(f"bilinear_bwd {case}[{path}] ac{ac} acc{acc}", dxb.body((N, H, W, Cc)), refs[0], refs[1], dt)
    assert dxb.pads_untouched() and dyb.unchanged()


@pytest.mark.parametrize("ac", [0, 1])
@pytest.mark.parametrize("name", list(R.ENGINE_ROUTES))
def test_engine_resize_backward_routes(name, ac):
    """SpatialOps._resize: the row kernel, the separable pair (whose first launch has the identity ratio 1.0 along y) and the single generic launch, forward and
    adjoint against the same matrices.  The bf16 pair keeps its intermediate in fp32 (a bf16 one, summed again over ~scale rows that cancel, was 3.9e-2 off
    at |ref64| = 0.10 on the x8 case here: 50x this bound)."""
    from pn2 import F32, BF16
    from pn2.engine import Engine
    from pn2.graph import _seed_grad
    route, dt, geom, Cc = R.ENGINE_ROUTES[name]
    H, W, OH, OW, scale = R.GEOMS[geom]
    rh, rw = R.ratios(geom, ac)
    x, g = R.values("engine_x", (N, H, W, Cc)), R.values("engine_g", (N, OH, OW, Cc))
    eng = Engine(F32 if dt == "fp32" else BF16, True, need_grad=True)
    a = eng.from_nchw(torch.from_numpy(x).float().permute(0, 3, 1, 2).to(dev), True)
    assert a.Cp == Cc
    y = eng.bilinear(a, scale, bool(ac))
    out = eng.to_nchw(y).permute(0, 2, 3, 1).double().cpu().numpy()
    _seed_grad(y, torch.from_numpy(g).float().permute(0, 3, 1, 2).to(dev))
    eng.backward()
    torch.cuda.synchronize()
    refs = [R.bilinear_ref(x, OH, OW, ac, R.f32(rh), R.f32(rw), t) for t in (np.float64, np.float32)]
    check(f"engine_resize_fwd {name} ac{ac}", out, refs[0], refs[1], dt)
    refs = [R.bilinear_bwd_ref(g, H, W, ac, R.f32(rh), R.f32(rw), t) for t in (np.float64, np.float32)]
    check(f"engine_resize_bwd {name}[{route}] ac{ac}", a.grad.double().cpu().numpy(), refs[0], refs[1], dt, bf=2.0 if route == "separable" else 1.0)


# ================================================================================================================ binary / mul_bwd / copy
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("op", [0, 1], ids=["add", "mul"])
@pytest.mark.parametrize("form,dt", [(f, dt) for f, v in R.EW_FORMS.items() for dt in v[1]])
def test_binary_vs_float64(form, dt, op, acc):
    Cc, ld_a, ld_b, ld_o = R.EW_FORMS[form][1][dt]
    M = R.EW_M
    a, b, old = (R.values(n, (M, Cc)) for n in ("ew_a", "ew_b", "ew_old"))
    ab, bb, ob = inp(M, Cc, ld_a, dt, a), inp(M, Cc, ld_b, dt, b), Buf(M, Cc, ld_o, dt, old if acc else None)
    assert _lib().pn2_binary(DT[dt], op, ab.ptr, ld_a, bb.ptr, ld_b, ob.ptr, ld_o, M, Cc, acc, _stream()) == 0
    torch.cuda.synchronize()
    check_ew(f"binary op{op} acc{acc} {form}", ob.body(), R.binary_ref(op, a, b, old if acc else None), old if acc else None, R.binary_ref(op, a, b), dt)
    assert ob.pads_untouched() and ab.unchanged() and bb.unchanged()


@pytest.mark.parametrize("acc_a,acc_b", [(0, 0), (1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("form,dt", [(f, dt) for f, v in R.EW_FORMS.items() for dt in v[1]])
def test_mul_bwd_vs_float64(form, dt, acc_a, acc_b):
    Cc, ld_a, ld_b, ld_o = R.EW_FORMS[form][1][dt]
    M = R.EW_M
    g, a, b, oa, ob_ = (R.values(n, (M, Cc)) for n in ("ew_g", "ew_a", "ew_b", "ew_old", "ew_old2"))
    gb_, ab, bb = inp(M, Cc, ld_o, dt, g), inp(M, Cc, ld_a, dt, a), inp(M, Cc, ld_b, dt, b)
    ga, gb = Buf(M, Cc, ld_o, dt, oa if acc_a else None), Buf(M, Cc, ld_o, dt, ob_ if acc_b else None)
    assert _lib().pn2_mul_bwd(DT[dt], gb_.ptr, ld_o, ab.ptr, ld_a, bb.ptr, ld_b, ga.ptr, ld_o, acc_a, gb.ptr, ld_o, acc_b, M, Cc, _stream()) == 0
    torch.cuda.synchronize()
    ra, rb = R.mul_bwd_ref(g, a, b, oa if acc_a else None, ob_ if acc_b else None)
    na, nb = R.mul_bwd_ref(g, a, b)
    check_ew(f"mul_bwd ga acc{acc_a} {form}", ga.body(), ra, oa if acc_a else None, na, dt)
    check_ew(f"mul_bwd gb acc{acc_b} {form}", gb.body(), rb, ob_ if acc_b else None, nb, dt)
    assert ga.pads_untouched() and gb.pads_untouched() and gb_.unchanged() and ab.unchanged() and bb.unchanged()


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_mul_bwd_rejects_aliased_gradients(dt):
    M, Cc = R.EW_M, 8
    g, a, b = (inp(M, Cc, 8, dt, R.values(n, (M, Cc))) for n in ("ew_g", "ew_a", "ew_b"))
    ga = Buf(M, Cc, 16, dt, R.values("ew_old", (M, Cc)))
    assert _lib().pn2_mul_bwd(DT[dt], g.ptr, 8, a.ptr, 8, b.ptr, 8, ga.ptr, 16, 0, ga.ptr, 16, 1, M, Cc, _stream()) == -1
    torch.cuda.synchronize()
    assert ga.unchanged()


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("dt_in,dt_out", [("fp32", "fp32"), ("bf16", "bf16"), ("fp32", "bf16"), ("bf16", "fp32")])
@pytest.mark.parametrize("form", list(R.EW_FORMS))
def test_copy_vs_float64(form, dt_in, dt_out, acc):
    """Same dtype: the bits when nothing is accumulated (both dtypes), else one rounding of the sum; fp32 -> bf16 rounds once (the source is a full fp32 number
    there); bf16 -> fp32 is exact."""
    Cc, ld_s, _, ld_d = R.EW_FORMS[form][1][dt_out if dt_in == dt_out else "fp32"]
    M = R.EW_M
    src = R.values("ew_a", (M, Cc))
    if dt_in == "fp32":          # not a bf16 number: the conversion has something to round
        src = (src * (1 + 2.0 ** -12)).astype(np.float32).astype(np.float64)
    old = R.values("ew_old", (M, Cc))
    sb, db = inp(M, Cc, ld_s, dt_in, src), Buf(M, Cc, ld_d, dt_out, old if acc else None)
    assert _lib().pn2_copy(DT[dt_in], sb.ptr, ld_s, DT[dt_out], db.ptr, ld_d, M, Cc, acc, _stream()) == 0
    torch.cuda.synchronize()
    ours = db.body()
    if not acc and (dt_in == dt_out or dt_out == "fp32"):          # bits moved, or a bf16 number widened: nothing may change
        assert np.array_equal(ours, src) and np.array_equal(np.signbit(ours), np.signbit(src))
    else:
        check_ew(f"copy {dt_in}->{dt_out} acc{acc} {form}", ours, R.copy_ref(src, old if acc else None), old if acc else None, src, dt_out)
    assert db.pads_untouched() and sb.unchanged()


def _copy_jobs(dt):
    """(M, C, ld_s, ld_d, accumulate): one partial block; more than 1024 vectors (two blocks); an accumulating one."""
    V = R.VEC[dt]
    return [(R.EW_M, 2 * V, 2 * V, 4 * V, 0), (700, 2 * V, 3 * V, 2 * V, 0), (R.EW_M, 4 * V, 4 * V, 5 * V, 1)]


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_copy_multi_equals_single_copies(dt):
    from pn2.capi import CopyJob
    lib = _lib()
    specs = _copy_jobs(dt)

    def buffers():
        return [(inp(M, Cc, ls, dt, R.values(f"cm_src{i}", (M, Cc))), Buf(M, Cc, ld, dt, R.values(f"cm_old{i}", (M, Cc)) if acc else None))
                for i, (M, Cc, ls, ld, acc) in enumerate(specs)]
    single, table = buffers(), buffers()
    for (s, d), (M, Cc, ls, ld, acc) in zip(single, specs):
        assert lib.pn2_copy(DT[dt], s.ptr, ls, DT[dt], d.ptr, ld, M, Cc, acc, _stream()) == 0
    jobs = (CopyJob * len(specs))()
    bstart = [0]
    for j, ((s, d), (M, Cc, ls, ld, acc)) in enumerate(zip(table, specs)):
        jobs[j] = CopyJob(s.t.data_ptr(), d.t.data_ptr(), ls, ld, M, Cc, acc, 0)
        nb = lib.pn2_copy_job_blocks(DT[dt], C.byref(jobs[j]))
        assert nb == (M * (Cc // R.VEC[dt]) + 1023) // 1024
        bstart.append(bstart[-1] + nb)
    assert bstart[1] == 1 and bstart[2] - bstart[1] == 2
    jd = torch.frombuffer(bytearray(bytes(jobs)), dtype=torch.uint8).to(dev)
    bd = torch.tensor(bstart, dtype=torch.int32, device=dev)
    assert lib.pn2_copy_multi(DT[dt], _p(jd), _p(bd), len(specs), bstart[-1], _stream()) == 0
    torch.cuda.synchronize()
    for i, ((s1, d1), (s2, d2), (M, Cc, ls, ld, acc)) in enumerate(zip(single, table, specs)):
        assert torch.equal(d1._bits(d1.t.cpu()), d2._bits(d2.t.cpu())), i
        assert d2.pads_untouched() and s2.unchanged()
        src = s2.body()
        if not acc:
            assert np.array_equal(d2.body(), src)
        else:
            old = R.values(f"cm_old{i}", (M, Cc))
            check_ew(f"copy_multi job{i}", d2.body(), R.copy_ref(src, old), old, src, dt)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_copy_job_blocks_rejects_unaligned(dt):
    from pn2.capi import CopyJob
    V = R.VEC[dt]
    buf = torch.zeros(64, device=dev)
    for (Cc, ls, ld) in ((V + 1, 2 * V, 2 * V), (V, V + 2, 2 * V), (V, 2 * V, V + 2)):
        job = CopyJob(buf.data_ptr(), buf.data_ptr(), ls, ld, 3, Cc, 0, 0)
        assert _lib().pn2_copy_job_blocks(DT[dt], C.byref(job)) == -2
    assert _lib().pn2_copy_job_blocks(DT[dt], C.byref(CopyJob(buf.data_ptr(), buf.data_ptr(), V, V, 3, V, 0, 0))) == 1


# ================================================================================================================ the grid stride's second trip
def test_binary_grid_stride_second_trip():
    """16384 * 256 + 1000 float4 vectors: the last 1000 are the second iteration of PIX_LOOP.  Whole output, exact."""
    M = R.STRIDE2_BINARY_M
    a, b = R.values("s2_a", (M, 4)).astype(np.float32), R.values("s2_b", (M, 4)).astype(np.float32)
    ad, bd = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    out = torch.full((M + 1, 4), SENT, device=dev)
    assert _lib().pn2_binary(0, 0, _p(ad), 4, _p(bd), 4, _p(out), 4, M, 4, 0, _stream()) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[:M], a + b) and (got[M] == SENT).all()


def test_bilinear_grid_stride_second_trip():
    """fp32 C = 4, 1025 x 1025 -> 2050 x 2050: 4 202 500 output vectors, 8196 more than one trip of the largest grid.  Whole output."""
    H, W, OH, OW = R.STRIDE2_BILINEAR
    x = R.values("s2_x", (1, H, W, 4))
    y = _bilinear_fwd("fp32", x, 4, 4, OH, OW, 0, 0.5, 0.5)
    refs = [R.bilinear_ref(x, OH, OW, 0, 0.5, 0.5, t) for t in (np.float64, np.float32)]
    check("bilinear_fwd second trip", y, refs[0], refs[1], "fp32")


# ================================================================================================================ NCHW -> NHWC
@pytest.mark.parametrize("name", list(R.NCHW_CASES))
def test_nchw_to_nhwc(name):
    path, dt, Cc, Cp, ld_y = R.NCHW_CASES[name]
    HW = R.NCHW_HW
    x = R.values("nchw_x", (N, Cc, HW))
    if dt == "bf16":          # full fp32 numbers: the conversion rounds once
        x = (x * (1 + 2.0 ** -12)).astype(np.float32).astype(np.float64)
    xd = torch.from_numpy(x).float().to(dev)
    yb = Buf(N * HW, Cp, ld_y, dt)
    assert _lib().pn2_nchw_to_nhwc(DT[dt], _p(xd), yb.ptr, ld_y, N, Cc, HW, Cp, _stream()) == 0
    torch.cuda.synchronize()
    y, ref = yb.body(), R.nchw_to_nhwc_ref(x, Cp)
    assert not y[:, Cc:].any() and not np.signbit(y[:, Cc:]).any()
    if dt == "fp32":
        assert np.array_equal(y, ref)
    else:
        assert bool((np.abs(y - ref) <= BF_ULP * np.abs(ref)).all()) and not np.array_equal(y, ref)
    assert yb.pads_untouched()


# ================================================================================================================ bias gradient
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("name", list(R.BIAS_CASES))
def test_bias_grad_vs_float64(name, acc):
    _, M, K = R.BIAS_CASES[name]
    # full fp32 numbers: sums of a few thousand bf16 numbers of one magnitude are exact in fp32 in any order, and would not show a summation error
    dy = (R.values("bias_" + name, (M, K), "pos") * (1 + 2.0 ** -12)).astype(np.float32).astype(np.float64)
    old = R.values("bias_old", (K,))
    dyd = torch.from_numpy(dy).float().to(dev)
    db = Buf(1, K, K + 3, "fp32", old if acc else None)
    assert _lib().pn2_bias_grad(_p(dyd), M, K, db.ptr, acc, _stream()) == 0
    torch.cuda.synchronize()
    refs = [R.bias_grad_ref(dy, old if acc else None, t) for t in (np.float64, np.float32)]
    check(f"bias_grad {name} acc{acc}", db.body().reshape(K), refs[0], refs[1], "fp32")
    assert db.pads_untouched()


# ================================================================================================================ status codes
ST_M, ST_C = 2 * 4 * 4, 8
# entry point -> (inputs, outputs, takes the idx map, call(lib, dt, p, stream)) on small valid shapes; p: its pointer arguments - inputs, outputs, then idx
STATUS_CALLS = {
    "maxpool_fwd": (1, 1, True, lambda lib, dt, p, st: lib.pn2_maxpool3x3s2_fwd(dt, p[0], 8, p[1], 8, p[2], 2, 4, 4, ST_C, 2, 2, st)),
    "maxpool_bwd": (1, 1, True, lambda lib, dt, p, st: lib.pn2_maxpool3x3s2_bwd(dt, p[0], 8, p[2], p[1], 8, 2, 4, 4, ST_C, 2, 2, st)),
    "avgpool_fwd": (1, 1, False, lambda lib, dt, p, st: lib.pn2_avgpool_fwd(dt, p[0], 8, p[1], 8, 2, 4, 4, ST_C, 2, 2, 2, 2, 0, 0, st)),
    "avgpool_bwd": (1, 1, False, lambda lib, dt, p, st: lib.pn2_avgpool_bwd(dt, p[0], 8, p[1], 8, 2, 4, 4, ST_C, 2, 2, 2, 2, 0, 0, 1, st)),
    "bilinear_fwd": (1, 1, False, lambda lib, dt, p, st: lib.pn2_bilinear_fwd(dt, p[0], 8, p[1], 8, 2, 2, 2, ST_C, 4, 4, 0, 0.5, 0.5, st)),
    "bilinear_bwd": (1, 1, False, lambda lib, dt, p, st: lib.pn2_bilinear_bwd(dt, p[0], 8, p[1], 8, 2, 2, 2, ST_C, 4, 4, 0, 0.5, 0.5, 1, st)),
    "binary": (2, 1, False, lambda lib, dt, p, st: lib.pn2_binary(dt, 0, p[0], 8, p[1], 8, p[2], 8, ST_M, ST_C, 0, st)),
    "mul_bwd": (3, 2, False, lambda lib, dt, p, st: lib.pn2_mul_bwd(dt, p[0], 8, p[1], 8, p[2], 8, p[3], 8, 0, p[4], 8, 0, ST_M, ST_C, st)),
    "copy": (1, 1, False, lambda lib, dt, p, st: lib.pn2_copy(dt, p[0], 8, dt, p[1], 8, ST_M, ST_C, 0, st)),
    "nchw_to_nhwc": (1, 1, False, lambda lib, dt, p, st: lib.pn2_nchw_to_nhwc(dt, p[0], p[1], 8, 2, 3, 16, 8, st)),
}


@pytest.mark.parametrize("entry", list(STATUS_CALLS))
def test_status_codes_leave_outputs_untouched(entry):
    """A NULL pointer in any position gives -1; the conv-only dtype codes PN2_F32F (2), PN2_F32X3 (3) and an unknown 7 give -3; nothing is written either way."""
    n_in, n_out, takes_idx, call = STATUS_CALLS[entry]
    idx = torch.full((ST_M, ST_C), 3, dtype=torch.uint8, device=dev)
    nptr = n_in + n_out + int(takes_idx)

    def run(dt, null):
        ins = [inp(ST_M, ST_C, 8, "fp32", R.values("st_in", (ST_M, ST_C))) for _ in range(n_in)]
        outs = [Buf(ST_M, ST_C, 8, "fp32", R.values("st_out", (ST_M, ST_C))) for _ in range(n_out)]
        p = [b.ptr for b in ins + outs] + ([_p(idx)] if takes_idx else [])
        if null is not None:
            p[null] = C.c_void_p(0)
        rc = call(_lib(), dt, p, _stream())
        torch.cuda.synchronize()
        return rc, outs
    for null in range(nptr):
        rc, outs = run(0, null)
        assert rc == -1 and all(o.unchanged() for o in outs), (entry, null)
    for dt in (2, 3, 7):
        rc, outs = run(dt, None)
        assert rc == -3 and all(o.unchanged() for o in outs), (entry, dt)
    rc, outs = run(0, None)          # the same call with nothing wrong goes through
    assert rc == 0 and all(o.pads_untouched() for o in outs) and not any(o.unchanged() for o in outs)


def test_status_codes_of_the_other_entry_points():
    from pn2.capi import CopyJob
    lib = _lib()
    src, dst = inp(4, 8, 8, "fp32", R.values("st_in", (4, 8))), Buf(4, 8, 8, "fp32", R.values("st_out", (4, 8)))
    assert lib.pn2_copy(0, src.ptr, 8, 2, dst.ptr, 8, 4, 8, 0, _stream()) == -3 and lib.pn2_copy(1, src.ptr, 8, 7, dst.ptr, 8, 4, 8, 0, _stream()) == -3
    job = (CopyJob * 1)(CopyJob(src.t.data_ptr(), dst.t.data_ptr(), 8, 8, 4, 8, 0, 0))
    jd = torch.frombuffer(bytearray(bytes(job)), dtype=torch.uint8).to(dev)
    bd = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    for dt in (2, 3, 7):
        assert lib.pn2_copy_multi(dt, _p(jd), _p(bd), 1, 1, _stream()) == -3
    assert lib.pn2_copy_multi(0, C.c_void_p(0), _p(bd), 1, 1, _stream()) == -1 and lib.pn2_copy_multi(0, _p(jd), C.c_void_p(0), 1, 1, _stream()) == -1
    assert lib.pn2_copy_job_blocks(0, None) == -1
    db = Buf(1, 4, 6, "fp32", R.values("bias_old", (4,)))
    dy = torch.ones(8, 4, device=dev)
    assert lib.pn2_bias_grad(C.c_void_p(0), 8, 4, db.ptr, 0, _stream()) == -1 and lib.pn2_bias_grad(_p(dy), 8, 4, C.c_void_p(0), 0, _stream()) == -1
    torch.cuda.synchronize()
    assert dst.unchanged() and db.unchanged()
