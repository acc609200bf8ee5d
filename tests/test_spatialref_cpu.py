"""CPU checks of tests/spatialref.py: every float64 reference agrees with torch's own op in float64 (1e-12 relative, forward and backward) on every case of the
tables that tests/test_gpu_spatial_kernels.py runs, the seeded inputs have the properties those tests rely on, and every case named after a dispatch path of
pn2_spatial.hip satisfies the predicate of that path as spatialref restates it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import spatialref as R

REL = 1e-12


def nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a)).permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return t.detach().permute(0, 2, 3, 1).contiguous().numpy()


def close(a, b, rel=REL):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max()) <= rel * max(float(np.abs(b).max()), 1e-300) if a.size else True


# ================================================================================================================ max pool
def _torch_maxpool(x):
    """torch max_pool2d on NHWC float64 x -> (the leaf, y, tap index): flat indices iy * W + ix converted to the tap (iy - (2 oy - 1)) * 3 + (ix - (2 ox - 1))."""
    t = nchw(x).requires_grad_(True)
    y, flat = F.max_pool2d(t, 3, 2, 1, return_indices=True)
    N, C, OH, OW = y.shape
    W = x.shape[2]
    oy = torch.arange(OH).view(1, 1, OH, 1)
    ox = torch.arange(OW).view(1, 1, 1, OW)
    tap = (flat // W - (2 * oy - 1)) * 3 + (flat % W - (2 * ox - 1))
    return t, y, tap


@pytest.mark.parametrize("kind", R.MAXPOOL_KINDS)
@pytest.mark.parametrize("shape", R.MAXPOOL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_maxpool_ref_equals_torch(shape, kind):
    """Values bit for bit (NaNs in the same places), tap indices equal, scatter equal to autograd's."""
    H, W = shape
    for C in (8, 5):
        x = R.maxpool_input(kind, H, W, C)
        y, idx = R.maxpool_ref(x)
        t, ty, tap = _torch_maxpool(x)
        assert np.array_equal(y, nhwc(ty), equal_nan=True)
        assert np.array_equal(idx, nhwc(tap).astype(np.uint8)) and int(tap.min()) >= 0 and int(tap.max()) <= 8
        dy = R.values(f"maxpool_dy_{kind}", y.shape)
        ty.backward(nchw(dy))
        assert close(R.maxpool_bwd_ref(dy, idx, H, W), nhwc(t.grad))


def _windows(H, W):
    for oy in range(R.pool_out(H)):
        for ox in range(R.pool_out(W)):
            ys, xs = range(max(2 * oy - 1, 0), min(2 * oy + 2, H)), range(max(2 * ox - 1, 0), min(2 * ox + 2, W))
            yield oy, ox, ys, xs


@pytest.mark.parametrize("shape", R.MAXPOOL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_maxpool_inputs(shape):
    H, W = shape
    C = 8
    many = H > 1 and W > 1          # a 1 x 1 map has one window of one tap and a 1 x 5 map windows of two or three: few ties are possible there
    for kind, least in (("ties", 0.30), ("relu", 0.10)):          # relu: windows that are zero in every tap, the tie the stem's pool meets behind its ReLU
        x = R.maxpool_input(kind, H, W, C)
        tied = total = 0
        for oy, ox, ys, xs in _windows(H, W):
            win = x[:, ys.start:ys.stop, xs.start:xs.stop, :].reshape(R.N_IMG, -1, C)
            tied += int(((win == win.max(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
            total += R.N_IMG * C
        if many:
            assert tied >= least * total, (kind, tied, total)
        if kind == "ties":
            assert np.array_equal(x * 4, np.round(x * 4)) and float(np.abs(x).max()) <= 1
        else:
            assert float((x == 0).mean()) >= 0.5 and float(x.min()) == 0 and not np.signbit(x).any()
    cont = R.maxpool_input("cont", H, W, C)
    assert len(np.unique(cont)) > 0.5 * cont.size          # bf16 rounding merges some; ties stay rare
    for kind in R.MAXPOOL_KINDS:          # bf16-representable: both dtypes and the reference see one set of numbers
        x = R.maxpool_input(kind, H, W, C)
        fin = np.isfinite(x)
        assert np.array_equal(R.bf16_round(np.where(fin, x, 0)), np.where(fin, x, 0))
    # NaN map: a border window and (where the map has one) an interior window hold a NaN; one window holds two
    x = R.maxpool_input("nan", H, W, C)
    nan = np.isnan(x[0, :, :, 0])
    assert nan[0, 0] and nan[H - 1, W - 1] and not np.isnan(x[1]).any() and not np.isnan(x[0, :, :, 1]).any()
    counts = {(oy, ox): int(nan[ys.start:ys.stop, xs.start:xs.stop].sum()) for oy, ox, ys, xs in _windows(H, W)}
    assert counts[(0, 0)] >= 1
    if H >= 7:
        OH, OW = R.pool_out(H), R.pool_out(W)
        assert any(v >= 1 for (oy, ox), v in counts.items() if 0 < oy < OH - 1 and 0 < ox < OW - 1)
        assert any(v >= 2 for v in counts.values())
    # -inf map: the named border windows are -inf in every in-image tap, and their tap 0 lies outside the image
    x = R.maxpool_input("neginf", H, W, C)
    for (oy, ox) in R.maxpool_neginf_windows(H, W):
        assert oy == 0 or ox == 0
        ys, xs = range(max(2 * oy - 1, 0), min(2 * oy + 2, H)), range(max(2 * ox - 1, 0), min(2 * ox + 2, W))
        assert np.isneginf(x[0, ys.start:ys.stop, xs.start:xs.stop, :3]).all()
    assert np.isneginf(x[1]).all()
    if many:
        assert np.isfinite(x[0, :, :, 3:]).all()
    _, idx = R.maxpool_ref(x)
    assert idx[1, 0, 0, 0] == 4 and (W == 1 or R.pool_out(W) == 1 or idx[1, 0, 1, 0] == 3)          # first in-image taps, not tap 0


def test_maxpool_neginf_is_torchs_documented_example():
    """A 4 x 4 all -inf map: torch's flat indices are [0, 1, 4, 5], the first in-image tap of each of the four windows (taps 4, 3, 1, 0)."""
    x = np.full((1, 4, 4, 1), -np.inf)
    _, idx = R.maxpool_ref(x)
    assert idx[0, :, :, 0].tolist() == [[4, 3], [1, 0]]
    _, flat = F.max_pool2d(nchw(x), 3, 2, 1, return_indices=True)
    assert flat.flatten().tolist() == [0, 1, 4, 5]


# ================================================================================================================ average pool
@pytest.mark.parametrize("cfg", R.AVG_SETS, ids=lambda c: "k%ds%dp%d_%s_%s" % (c[0], c[1], c[2], "ceil" if c[3] else "floor", "inc" if c[4] else "exc"))
@pytest.mark.parametrize("shape", R.AVG_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_avgpool_ref_equals_torch(shape, cfg):
    H, W = shape
    k, s, p, ceil, inc = cfg
    for C in (8, 5):
        x = R.values("avgpool_x", (R.N_IMG, H, W, C))
        t = nchw(x).requires_grad_(True)
        ty = F.avg_pool2d(t, k, s, p, ceil, inc)
        y = R.avgpool_ref(x, *cfg)
        assert y.shape[1:3] == (R.avg_out(H, k, s, p, ceil), R.avg_out(W, k, s, p, ceil))
        assert close(y, nhwc(ty))
        dy = R.values("avgpool_dy", y.shape)
        ty.backward(nchw(dy))
        assert close(R.avgpool_bwd_ref(dy, H, W, *cfg), nhwc(t.grad))


def test_avgpool_sets_discriminate():
    """The sets with a real padding give another result when count_include_pad is flipped, the ceil-mode set has an overhanging window on the odd shape."""
    x = R.values("avgpool_x", (R.N_IMG, 7, 9, 8))
    for cfg in R.AVG_SETS:
        k, s, p, ceil, inc = cfg
        if p:
            assert not close(R.avgpool_ref(x, k, s, p, ceil, inc), R.avgpool_ref(x, k, s, p, ceil, not inc), 1e-3)
        if ceil:
            assert R.avg_out(7, k, s, p, True) == R.avg_out(7, k, s, p, False) + 1


# ================================================================================================================ bilinear
def _torch_resize(x, geom, ac):
    H, W, OH, OW, scale = R.GEOMS[geom]
    t = nchw(x).requires_grad_(True)
    if scale is not None:
        y = F.interpolate(t, scale_factor=scale, mode="bilinear", align_corners=bool(ac))
    else:
        y = F.interpolate(t, size=(OH, OW), mode="bilinear", align_corners=bool(ac))
    assert tuple(y.shape[2:]) == (OH, OW)
    return t, y


@pytest.mark.parametrize("ac", [0, 1])
@pytest.mark.parametrize("geom", list(R.GEOMS))
def test_bilinear_ref_equals_torch(geom, ac):
    """With the ratio torch derives in float64 (spatialref.ideal_ratio) the two-matrix reference equals F.interpolate and its autograd adjoint to 1e-12.

    The GPU tests build the matrices from the fp32-ROUNDED ratio that the C call receives.  Where rounding changes nothing (x2, x8, x16, 0.25, 1.0, 0.0 and the
    other ratios that are fp32 numbers) that is the same comparison.  Where it does (13/9, 4/9, 31/256 ...), no torch call takes the rounded ratio, so the honest
    statement is made on the matrices instead: every entry of the rounded-ratio matrix lies within 3 * 2^-24 * max(source index) of the ideal-ratio matrix (the
    rounding moves a source index by at most 2^-24 of itself, and an interpolation weight moves by as much as its index does), and those matrices are the whole of
    the reference."""
    H, W, OH, OW, scale = R.GEOMS[geom]
    rh, rw = R.ratios(geom, ac)
    for C in (8, 5):
        x = R.values("bilinear_x", (R.N_IMG, H, W, C))
        t, ty = _torch_resize(x, geom, ac)
        assert close(R.bilinear_ref(x, OH, OW, ac, rh, rw), nhwc(ty))
        dy = R.values("bilinear_dy", (R.N_IMG, OH, OW, C))
        ty.backward(nchw(dy))
        assert close(R.bilinear_bwd_ref(dy, H, W, ac, rh, rw), nhwc(t.grad))
    for In, On, r in ((H, OH, rh), (W, OW, rw)):
        ideal, rounded = R.interp_matrix(In, On, ac, r), R.interp_matrix(In, On, ac, R.f32(r))
        assert np.allclose(rounded.sum(axis=1), 1.0, rtol=0, atol=1e-15)
        if R.f32(r) == r:
            assert np.array_equal(ideal, rounded)
        else:
            assert float(np.abs(ideal - rounded).max()) <= 3 * 2.0 ** -24 * max(In - 1, 1), (geom, ac)


def test_bilinear_geometries_cover_what_the_issue_names():
    exact = [g for g in R.GEOMS for ac in (0, 1) if all(R.f32(r) == r for r in R.ratios(g, ac))]
    inexact = [g for g in R.GEOMS for ac in (0, 1) if any(R.f32(r) != r for r in R.ratios(g, ac))]
    assert exact and inexact
    assert R.ratios("5x6_1x1", 1) == (0.0, 0.0) and R.ratios("1x1_4x4", 1) == (0.0, 0.0) and R.ratios("7x7_7x7", 0) == (1.0, 1.0)
    H, W, OH, OW, _ = R.GEOMS["13x11_9x17"]
    assert OH < H and OW > W
    for g in R.BL_FWD_GEOMS:
        assert g in R.GEOMS


# ================================================================================================================ element-wise, layout, bias gradient
def test_elementwise_refs_equal_torch():
    a, b, g, o = (R.values(n, (R.EW_M, 8)) for n in ("ew_a", "ew_b", "ew_g", "ew_old"))
    ta, tb, tg, to = (torch.from_numpy(v) for v in (a, b, g, o))
    assert np.array_equal(R.binary_ref(0, a, b), (ta + tb).numpy()) and np.array_equal(R.binary_ref(1, a, b), (ta * tb).numpy())
    assert np.array_equal(R.binary_ref(1, a, b, o), (to + ta * tb).numpy())
    ta.requires_grad_(True), tb.requires_grad_(True)
    (ta * tb).backward(tg)
    ga, gb = R.mul_bwd_ref(g, a, b)
    assert np.array_equal(ga, ta.grad.numpy()) and np.array_equal(gb, tb.grad.numpy())
    ga, gb = R.mul_bwd_ref(g, a, b, old_a=o)
    assert np.array_equal(ga, (to + tg * tb).detach().numpy()) and np.array_equal(gb, tb.grad.numpy())
    assert np.array_equal(R.copy_ref(a), a) and np.array_equal(R.copy_ref(a, o), (to + ta).detach().numpy())
    x = R.values("nchw_x", (2, 13, R.NCHW_HW))
    y = R.nchw_to_nhwc_ref(x, 16)
    assert np.array_equal(y[:, :13], torch.from_numpy(x).permute(0, 2, 1).reshape(-1, 13).numpy()) and not y[:, 13:].any()
    for name, (_, M, K) in R.BIAS_CASES.items():
        dy = R.values("bias_" + name, (M, K), "pos")
        assert close(R.bias_grad_ref(dy), torch.from_numpy(dy).sum(dim=0).numpy()), name
        assert float(dy.min()) >= 0.25          # no element is small against the floor of the sum: one dropped row shows


# ================================================================================================================ dispatch-path preconditions
def test_pool_and_elementwise_forms_select_their_path():
    for name, per_dt in R.POOL_FORMS.items():
        for dt, (C, ld_in, ld_out) in per_dt.items():
            assert R.elementwise_path(dt, C, ld_in, ld_out) == R.POOL_FORM_PATH[name], (name, dt)
            assert ld_in >= C and ld_out >= C
    assert R.POOL_FORMS["scalar_ld"]["fp32"][0] % 4 == 0 and R.POOL_FORMS["scalar_ld"]["bf16"][0] % 8 == 0          # the stride alone forces the scalar form
    assert R.POOL_FORMS["vec_ld12"]["fp32"][1:] == (12, 12)
    for name, (path, per_dt) in R.EW_FORMS.items():
        for dt, (C, *lds) in per_dt.items():
            assert R.elementwise_path(dt, C, *lds) == path, (name, dt)
            assert min(lds) >= C
    assert R.EW_M * 8 // 4 < 256          # one partial block: nothing here loops


def test_bilinear_forms_select_their_path():
    for name, (path, dts, C, ld_x, ld_y) in R.BL_FWD_FORMS.items():
        for dt in dts:
            assert R.bilinear_fwd_path(dt, C, ld_x, ld_y) == path, (name, dt)
    assert {p for p, *_ in R.BL_FWD_FORMS.values()} == {"vec", "x3", "scalar"}
    for name, (path, dts, geom, C, ld_dy, ld_dx) in R.BL_BWD_CASES.items():
        H, W, OH, OW, _ = R.GEOMS[geom]
        for dt in dts:
            assert R.bilinear_bwd_path(dt, C, ld_dy, ld_dx, H, W, OH, OW) == path, (name, dt)
            assert ld_dx > C          # an accumulate buffer wider than C in every case
    assert {p for p, *_ in R.BL_BWD_CASES.values()} == {"rows_f4_R4", "rows_f4_R2", "rows_f4_R1", "rows_scalar", "wave", "x3", "vec", "scalar"}
    H, W, OH, OW, _ = R.GEOMS["2x32_8x256"]
    assert OW * 4 == 1024
    H, W, OH, OW, _ = R.GEOMS["2x32_8x257"]
    assert OW * 4 > 1024 and (OW * 4) % 4 == 0
    H, W, OH, OW, _ = R.GEOMS["3x5_12x21"]
    assert (OW * 9) % 4 != 0
    for name, (route, dt, geom, C) in R.ENGINE_ROUTES.items():
        H, W, OH, OW, _ = R.GEOMS[geom]
        assert C % 8 == 0 and R.engine_resize_bwd_route(dt, C, H, W, OH, OW) == route, name
    assert {r for r, *_ in R.ENGINE_ROUTES.values()} == {"rows", "separable", "single"}


def test_layout_and_bias_cases_select_their_path():
    for name, (path, dt, C, Cp, ld_y) in R.NCHW_CASES.items():
        assert R.nchw_path(dt, Cp, ld_y) == path and ld_y > Cp >= C, name
    assert {(dt, C, Cp) for _, dt, C, Cp, _ in R.NCHW_CASES.values()} >= {("fp32", 3, 4), ("bf16", 3, 8), ("fp32", 1, 8), ("fp32", 13, 16)}
    want = {"k1_float4": ("float4", 1, 2, 1), "k1_general": ("general", 1, 2, 1), "k9": ("general", 1, 2, 1), "k1_m1": ("general", 0, 1, 0), "k9_m1": ("general", 0, 1, 0)}
    for name, (path, M, K) in R.BIAS_CASES.items():
        got = R.bias_grad_path(M, K)
        assert got[0] == path and got == want[name], (name, got)          # (path, unrolled trips, longest tail, shortest tail): a ragged end where they differ
    assert R.BIAS_CASES["k1_general"][1] % 4 == 1


def test_grid_stride_cases_make_exactly_one_more_trip():
    cap = R.GRID_CAP * 256
    assert cap < R.STRIDE2_BINARY_M <= cap + 256 * 8          # C = 4 fp32: one vector per row
    H, W, OH, OW = R.STRIDE2_BILINEAR
    assert (OH, OW) == (2 * H, 2 * W) and cap < OH * OW < 2 * cap
    # no other case gets there: the largest of the tables is far below one trip's worth of vectors
    biggest = max(R.N_IMG * max(g[0] * g[1], g[2] * g[3]) * 32 for g in R.GEOMS.values())
    assert biggest < cap and R.EW_M * 8 < cap and 2 * R.NCHW_HW < cap
