"""Plain numpy references (CPU) of what pn2_spatial.hip computes - 3x3 / stride-2 max pooling with its argmax tap, average pooling, bilinear resizing as two
dense 1-D interpolation matrices, the element-wise ops, the NCHW -> NHWC conversion and the bias gradient - with the case tables and the seeded inputs of
tests/test_gpu_spatial_kernels.py.  Nothing here is shared with the product.  Activations are NHWC arrays [N][H][W][C], as the kernels see them.  Every function
takes `dtype`: np.float64 gives the yardstick, np.float32 gives "the same formula in fp32" (ref32) whose distance to float64 sets the tolerance.
tests/test_spatialref_cpu.py holds the references to torch in float64 on every case below and checks the properties of the inputs that the GPU tests rely on."""
import numpy as np
import torch

F64, F32 = np.float64, np.float32
VEC = {"fp32": 4, "bf16": 8}          # elements per 16-byte vector


def f32(x):
    """The value a `float` argument of the C ABI carries: x rounded to fp32, as a Python float."""
    return float(np.float32(x))


def bf16_round(a):
    """fp32 / float64 array -> the nearest bf16 values, as float64 (the inputs of the bf16 cases: the reference then sees what the kernel sees)."""
    return torch.from_numpy(np.asarray(a, dtype=F32)).bfloat16().double().numpy()


# ---------------------------------------------------------------------------------------------------------------- max pool 3x3 / stride 2 / pad 1
def pool_out(n):
    return (n + 2 - 3) // 2 + 1


def maxpool_ref(x, dtype=F64):
    """-> (y [N][OH][OW][C], idx uint8 [N][OH][OW][C]).  idx is the tap r * 3 + s (row-major in the window) of the FIRST maximum; a NaN replaces whatever is held
    (so the last NaN of a window wins); a window whose in-image taps are all -inf names its first in-image tap - torch's max_pool2d rules."""
    x = np.asarray(x, dtype=dtype)
    N, H, W, C = x.shape
    OH, OW = pool_out(H), pool_out(W)
    y = np.full((N, OH, OW, C), -np.inf, dtype=dtype)
    idx = np.zeros((N, OH, OW, C), dtype=np.uint8)
    for oy in range(OH):
        for ox in range(OW):
            best = np.full((N, C), -np.inf, dtype=dtype)
            bi = np.full((N, C), -1, dtype=np.int64)
            for r in range(3):
                for s in range(3):
                    iy, ix = 2 * oy - 1 + r, 2 * ox - 1 + s
                    if not (0 <= iy < H and 0 <= ix < W):
                        continue
                    v = x[:, iy, ix, :]
                    take = (v > best) | np.isnan(v) | (bi < 0)          # bi < 0: the first in-image tap
                    best = np.where(take, v, best)
                    bi = np.where(take, r * 3 + s, bi)
            y[:, oy, ox, :], idx[:, oy, ox, :] = best, bi
    return y, idx


def maxpool_bwd_ref(dy, idx, H, W, dtype=F64):
    """Scatter of dy [N][OH][OW][C] by tap index into dx [N][H][W][C]."""
    dy = np.asarray(dy, dtype=dtype)
    N, OH, OW, C = dy.shape
    dx = np.zeros((N, H, W, C), dtype=dtype)
    for oy in range(OH):
        for ox in range(OW):
            for t in range(9):
                iy, ix = 2 * oy - 1 + t // 3, 2 * ox - 1 + t % 3
                if 0 <= iy < H and 0 <= ix < W:
                    dx[:, iy, ix, :] += np.where(idx[:, oy, ox, :] == t, dy[:, oy, ox, :], dtype(0))
    return dx


def maxpool_contributions(idx, H, W):
    """[N][H][W][C] int: how many windows name each input element (dx there is a sum of that many terms)."""
    return maxpool_bwd_ref(np.ones(idx.shape), idx, H, W).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------- average pool
def avg_out(i, k, stride, pad, ceil_mode):
    """The output-size rule of SpatialOps.avgpool (torch's pooling_output_shape)."""
    o = (i + 2 * pad - k + (stride - 1 if ceil_mode else 0)) // stride + 1
    if ceil_mode and (o - 1) * stride >= i + pad:
        o -= 1
    return o


def _avg_window(o, k, stride, pad, In, include_pad):
    """-> (lo, hi, divisor) of output index o along one axis: the window clipped to the padded extent counts in the divisor when include_pad, the window
    clipped to the image otherwise."""
    s = o * stride - pad
    e = min(s + k, In + pad)
    lo, hi = max(s, 0), min(e, In)
    return lo, hi, (e - s) if include_pad else (hi - lo)


def avgpool_ref(x, k, stride, pad, ceil_mode, include_pad, dtype=F64):
    x = np.asarray(x, dtype=dtype)
    N, H, W, C = x.shape
    OH, OW = avg_out(H, k, stride, pad, ceil_mode), avg_out(W, k, stride, pad, ceil_mode)
    y = np.zeros((N, OH, OW, C), dtype=dtype)
    for oy in range(OH):
        y0, y1, dh = _avg_window(oy, k, stride, pad, H, include_pad)
        for ox in range(OW):
            x0, x1, dw = _avg_window(ox, k, stride, pad, W, include_pad)
            y[:, oy, ox, :] = x[:, y0:y1, x0:x1, :].sum(axis=(1, 2), dtype=dtype) / dtype(dh * dw)
    return y


def avgpool_bwd_ref(dy, H, W, k, stride, pad, ceil_mode, include_pad, dtype=F64):
    dy = np.asarray(dy, dtype=dtype)
    N, OH, OW, C = dy.shape
    assert (OH, OW) == (avg_out(H, k, stride, pad, ceil_mode), avg_out(W, k, stride, pad, ceil_mode))
    dx = np.zeros((N, H, W, C), dtype=dtype)
    for oy in range(OH):
        y0, y1, dh = _avg_window(oy, k, stride, pad, H, include_pad)
        for ox in range(OW):
            x0, x1, dw = _avg_window(ox, k, stride, pad, W, include_pad)
            dx[:, y0:y1, x0:x1, :] += (dy[:, oy, ox, :] / dtype(dh * dw))[:, None, None, :]
    return dx


# ---------------------------------------------------------------------------------------------------------------- bilinear
def ideal_ratio(In, On, ac, scale=None):
    """The source-index ratio torch derives in float64: align_corners (In - 1) / (On - 1) (0 for one output); else 1 / scale_factor when a scale was given
    (recompute_scale_factor unset), In / On for size=.  SpatialOps.bilinear / resize_to compute the same and hand it to the C call as a `float`."""
    if ac:
        return (In - 1) / (On - 1) if On > 1 else 0.0
    return 1.0 / scale if scale is not None else In / On


def interp_matrix(In, On, ac, r, dtype=F64):
    """Dense [On][In] matrix of one axis.  torch's area_pixel_compute_source_index: src = r * o (align_corners) or max(r * (o + 0.5) - 0.5, 0);
    i0 = min(int(src), In - 1); i1 = i0 + (i0 < In - 1); l1 = clamp(src - i0, 0, 1); row o holds 1 - l1 at i0 and l1 at i1.  `r` is taken as an exact number
    and the index arithmetic runs in `dtype`."""
    R = np.zeros((On, In), dtype=dtype)
    r = dtype(r)
    for o in range(On):
        src = r * dtype(o) if ac else max(r * (dtype(o) + dtype(0.5)) - dtype(0.5), dtype(0))
        i0 = min(int(src), In - 1)
        i1 = i0 + (1 if i0 < In - 1 else 0)
        l1 = min(max(src - dtype(i0), dtype(0)), dtype(1))
        R[o, i0] += dtype(1) - l1
        R[o, i1] += l1
    return R


def bilinear_ref(x, OH, OW, ac, rh, rw, dtype=F64):
    """y = Ry . x . Rx^T per image and channel; rh / rw: the ratios as the C call receives them (see f32)."""
    x = np.asarray(x, dtype=dtype)
    N, H, W, C = x.shape
    Ry, Rx = interp_matrix(H, OH, ac, rh, dtype), interp_matrix(W, OW, ac, rw, dtype)
    t = np.tensordot(Ry, x, axes=(1, 1))                 # [OH][N][W][C]
    return np.ascontiguousarray(np.tensordot(Rx, t, axes=(1, 2)).transpose(2, 1, 0, 3))          # [OW][OH][N][C] -> NHWC


def bilinear_bwd_ref(dy, H, W, ac, rh, rw, dtype=F64):
    """The adjoint Ry^T . g . Rx."""
    dy = np.asarray(dy, dtype=dtype)
    N, OH, OW, C = dy.shape
    Ry, Rx = interp_matrix(H, OH, ac, rh, dtype), interp_matrix(W, OW, ac, rw, dtype)
    t = np.tensordot(Ry.T, dy, axes=(1, 1))              # [H][N][OW][C]
    return np.ascontiguousarray(np.tensordot(Rx.T, t, axes=(1, 2)).transpose(2, 1, 0, 3))


# ---------------------------------------------------------------------------------------------------------------- element-wise, layout, bias gradient
def binary_ref(op, a, b, old=None, dtype=F64):
    """op 0: a + b, op 1: a * b; `old`: the output's previous content when accumulating."""
    a, b = np.asarray(a, dtype=dtype), np.asarray(b, dtype=dtype)
    r = a + b if op == 0 else a * b
    return r if old is None else np.asarray(old, dtype=dtype) + r


def mul_bwd_ref(g, a, b, old_a=None, old_b=None, dtype=F64):
    """Backward of out = a * b: (ga, gb) = (g * b, g * a), each added to its old content when given."""
    return binary_ref(1, g, b, old_a, dtype), binary_ref(1, g, a, old_b, dtype)


def copy_ref(src, old=None, dtype=F64):
    s = np.asarray(src, dtype=dtype)
    return s.copy() if old is None else np.asarray(old, dtype=dtype) + s


def nchw_to_nhwc_ref(x, Cp, dtype=F64):
    """x [N][C][HW] -> [N * HW][Cp], pad channels zero."""
    x = np.asarray(x, dtype=dtype)
    N, C, HW = x.shape
    y = np.zeros((N * HW, Cp), dtype=dtype)
    y[:, :C] = x.transpose(0, 2, 1).reshape(N * HW, C)
    return y


def bias_grad_ref(dy, old=None, dtype=F64):
    """dy [M][K] -> column sums [K] (+ old).  Each column is summed as one contiguous row: numpy sums those pairwise, so the fp32 run is a careful fp32 sum
    (a row-by-row walk over [M][K] is a running sum whose fp32 error, 0.2 on the K = 9 case, would set no bound worth having)."""
    s = np.ascontiguousarray(np.asarray(dy, dtype=dtype).T).sum(axis=1, dtype=dtype)
    return s if old is None else np.asarray(old, dtype=dtype) + s


# ---------------------------------------------------------------------------------------------------------------- dispatch predicates, restated
# What the C entry points of pn2_spatial.hip decide from their arguments, restated here so that the case tables below can be checked against the path they are
# named after (test_spatialref_cpu.py): a change to the dispatch makes these visibly stale.
def vec_ok(dt, C, *lds):
    return all(v % VEC[dt] == 0 for v in (C,) + lds)


def elementwise_path(dt, C, *lds):
    """vec_or_scalar: max pool, average pool, binary, mul_bwd, same-dtype copy."""
    return "vec" if vec_ok(dt, C, *lds) else "scalar"


def bilinear_fwd_path(dt, C, ld_x, ld_y):
    if vec_ok(dt, C, ld_x, ld_y):
        return "vec"
    if dt == "fp32" and C % 3 == 0 and ld_x % 3 == 0 and ld_y % 3 == 0:
        return "x3"
    return "scalar"


def bilinear_bwd_path(dt, C, ld_dy, ld_dx, H, W, OH, OW):
    V = VEC[dt]
    mag = OH >= 4 * H and OW >= 4 * W
    if (C < V or (dt == "fp32" and C <= 16)) and mag and ld_dy == C and OW * C <= 8192:
        L = OW * C
        if dt == "fp32" and L % 4 == 0 and L <= 1024:
            lvp = 64
            while lvp < L // 4:
                lvp *= 2
            return f"rows_f4_R{256 // lvp}"
        return "rows_scalar"
    if C < V and mag:
        return "wave"
    return bilinear_fwd_path(dt, C, ld_dy, ld_dx)


def engine_resize_bwd_route(dt, Cp, H, W, OH, OW):
    """SpatialOps._resize's backward: the row kernel, the separable pair, or one generic launch.  Left out because the tests never vary them: the route also
    wants a contiguous output gradient (gy.stride(2) == Cp, which _seed_grad gives) and PN2_BL_ROWS unset or 1 (the default) for the row kernel."""
    mag = OH >= 4 * H and OW >= 4 * W
    rows_ok = dt == "fp32" and Cp <= 16 and OW * Cp <= 8192
    if mag and Cp >= VEC[dt] and not rows_ok:
        return "separable"
    return "rows" if bilinear_bwd_path(dt, Cp, Cp, Cp, H, W, OH, OW).startswith("rows") else "single"


# (nchw_to_nhwc_k's one-store path and bias_grad_k's float4 path also want a 16-byte-aligned base pointer; every buffer of the tests is a torch allocation,
# which is, so the two predicates below leave that condition out)
def nchw_path(dt, Cp, ld_y):
    return "fast" if Cp == VEC[dt] and ld_y % VEC[dt] == 0 else "general"


def bias_grad_path(M, K):
    """-> (path, iterations of the unrolled loop for thread 0, longest and shortest tail over the 1024 threads)."""
    path, n, u = ("float4", M // 4, 4) if K == 1 and M % 4 == 0 else ("general", M, 8)
    unrolled = 0
    m = 0
    while m + (u - 1) * 1024 < n:
        m += u * 1024
        unrolled += 1
    tails = [len(range(m + t, n, 1024)) if m + t < n else 0 for t in (0, 1023)]
    return path, unrolled, tails[0], tails[1]


GRID_CAP = 16384          # workgroups of 256 threads a grid-stride kernel gets at most: more than GRID_CAP * 256 vectors make PIX_LOOP iterate twice


# ---------------------------------------------------------------------------------------------------------------- seeded inputs
def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def _name_key(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name))


def values(name, shape, kind="cont"):
    """Seeded input named by case, bf16-representable (so fp32 and bf16 runs and the reference all see the same numbers), float64.
    cont: randn; ties: multiples of 1/4 in [-1, 1] (a clipped normal: the extremes are the likeliest values, so a window's maximum is often shared);
    relu: max(randn - 0.8, 0), four in five are zero, so whole windows are; pos: uniform in [0.25, 1.25)."""
    g = _rng(_name_key(name), *shape)
    if kind == "cont":
        v = g.standard_normal(shape)
    elif kind == "ties":
        v = np.round(np.clip(g.standard_normal(shape) * 1.25, -1, 1) * 4) / 4.0
    elif kind == "relu":
        v = np.maximum(g.standard_normal(shape) - 0.8, 0.0)
    else:
        assert kind == "pos"
        v = 0.25 + g.random(shape)
    return bf16_round(v)


# ---------------------------------------------------------------------------------------------------------------- case tables
N_IMG = 2
# name -> (C, ld_in, ld_out) per dtype.  The vector form keeps 16-byte rows and gets an output wider than C; the scalar form by C; the scalar form by stride alone
# (C = 8 in rows of 10).  A stride of 12 keeps fp32 rows 16-byte aligned - it is the vector form in a slice of a wider buffer, not a scalar one.
POOL_FORMS = {
    "vec_c8": {"fp32": (8, 8, 16), "bf16": (8, 8, 16)},
    "vec_ld12": {"fp32": (8, 12, 12)},
    "scalar_c5": {"fp32": (5, 5, 7), "bf16": (5, 5, 7)},
    "scalar_ld": {"fp32": (8, 10, 10), "bf16": (8, 10, 10)},
}
POOL_FORM_PATH = {"vec_c8": "vec", "vec_ld12": "vec", "scalar_c5": "scalar", "scalar_ld": "scalar"}
MAXPOOL_SHAPES = [(7, 9), (8, 8), (1, 1), (1, 5)]
MAXPOOL_KINDS = ["cont", "ties", "relu", "nan", "neginf"]


def maxpool_nan_sites(H, W):
    """(y, x) of the NaNs of the `nan` map (image 0, channels 0 and 3): the corners (border windows), two neighbours in the middle (one interior window holds
    both: the last one wins) and a lone one."""
    pts = [(0, 0), (H - 1, W - 1), (H // 2, W // 2), (H // 2, min(W // 2 + 1, W - 1)), (min(H // 2 + 2, H - 1), 1 if W > 1 else 0)]
    return sorted(set(pts))


def maxpool_neginf_windows(H, W):
    """(oy, ox) of the border windows of image 0 whose in-image taps are all -inf (channels 0..2): the top-left corner, the top-right corner, the bottom-left one.
    Image 1 is -inf everywhere."""
    OH, OW = pool_out(H), pool_out(W)
    return sorted({(0, 0), (0, OW - 1), (OH - 1, 0)})


def maxpool_input(kind, H, W, C):
    x = values(f"maxpool_{kind}", (N_IMG, H, W, C), kind if kind in ("cont", "ties", "relu") else "cont")
    if kind == "nan":
        for (iy, ix) in maxpool_nan_sites(H, W):
            x[0, iy, ix, 0] = np.nan
            x[0, iy, ix, min(3, C - 1)] = np.nan
    if kind == "neginf":
        for (oy, ox) in maxpool_neginf_windows(H, W):
            x[0, max(2 * oy - 1, 0):2 * oy + 2, max(2 * ox - 1, 0):2 * ox + 2, :3] = -np.inf
        x[1] = -np.inf
    return x


# (k, stride, pad, ceil_mode, count_include_pad): the sets of test_pool_and_bilinear_ops (the Res2Net 3x3 pools, the ceil-mode 2x2 downsample) and one that
# excludes a real padding from the divisor
AVG_SETS = [(3, 1, 1, False, True), (3, 2, 1, False, True), (2, 2, 0, True, False), (3, 2, 1, False, False)]
AVG_SHAPES = [(7, 9), (8, 8), (1, 1), (1, 6)]

# name -> (H, W, OH, OW, scale): scale is what F.interpolate gets as scale_factor (None: size=)
GEOMS = {
    "x2": (5, 7, 10, 14, 2),
    "x8_3x5": (3, 5, 24, 40, 8),
    "q_12x16": (12, 16, 3, 4, 0.25),
    "13x11_9x17": (13, 11, 9, 17, None),
    "9x17_13x11": (9, 17, 13, 11, None),
    "7x7_7x7": (7, 7, 7, 7, None),
    "1x1_4x4": (1, 1, 4, 4, None),
    "5x6_1x1": (5, 6, 1, 1, None),
    "x8_3x3": (3, 3, 24, 24, 8),
    "x16_3x5": (3, 5, 48, 80, 16),
    "2x32_8x256": (2, 32, 8, 256, None),
    "2x32_8x257": (2, 32, 8, 257, None),
    "3x5_12x21": (3, 5, 12, 21, None),
}
BL_FWD_GEOMS = ["x2", "x8_3x5", "q_12x16", "13x11_9x17", "7x7_7x7", "1x1_4x4", "5x6_1x1"]


def ratios(geom, ac):
    """-> (rh, rw) as Python floats in full precision (what the caller computes); the C call rounds them to fp32."""
    H, W, OH, OW, scale = GEOMS[geom]
    return ideal_ratio(H, OH, ac, scale), ideal_ratio(W, OW, ac, scale)


# name -> (path, dtypes, C, ld_x, ld_y)
BL_FWD_FORMS = {
    "vec_c8": ("vec", ("fp32", "bf16"), 8, 8, 16),
    "x3_c9": ("x3", ("fp32",), 9, 9, 9),
    "x3_c9_ld12": ("x3", ("fp32",), 9, 12, 12),
    "scalar_c5": ("scalar", ("fp32", "bf16"), 5, 5, 7),
    "scalar_c9_ld10": ("scalar", ("fp32", "bf16"), 9, 10, 10),
}

# name -> (path, dtypes, geometry, C, ld_dy, ld_dx); every case runs with accumulate 0 / 1 and align_corners 0 / 1
BL_BWD_CASES = {
    "rows_f4_R4": ("rows_f4_R4", ("fp32",), "x8_3x3", 1, 1, 3),
    "rows_f4_R2": ("rows_f4_R2", ("fp32",), "x16_3x5", 4, 4, 8),
    "rows_f4_R1": ("rows_f4_R1", ("fp32",), "2x32_8x256", 4, 4, 8),
    "rows_scalar_long": ("rows_scalar", ("fp32",), "2x32_8x257", 4, 4, 8),
    "rows_scalar_odd": ("rows_scalar", ("fp32",), "3x5_12x21", 9, 9, 12),
    "rows_scalar_bf16": ("rows_scalar", ("bf16",), "x8_3x5", 3, 3, 5),
    "wave_c3": ("wave", ("fp32", "bf16"), "x8_3x5", 3, 4, 5),
    "x3_c9_x2": ("x3", ("fp32",), "x2", 9, 9, 12),
    "x3_c9_x8_ld12": ("x3", ("fp32",), "x8_3x5", 9, 12, 12),
    "vec_x2": ("vec", ("fp32", "bf16"), "x2", 8, 16, 16),
    "vec_q": ("vec", ("fp32", "bf16"), "q_12x16", 8, 16, 16),
    "vec_13x11_9x17": ("vec", ("fp32", "bf16"), "13x11_9x17", 8, 16, 16),
    "vec_9x17_13x11": ("vec", ("fp32", "bf16"), "9x17_13x11", 8, 16, 16),
    "scalar_c5": ("scalar", ("fp32", "bf16"), "x2", 5, 5, 7),
    "r0_5x6_1x1": ("vec", ("fp32", "bf16"), "5x6_1x1", 8, 16, 16),
    "r0_scalar": ("scalar", ("fp32", "bf16"), "5x6_1x1", 5, 5, 7),
}

# name -> (route, dtype, geometry, C): the backward routes of SpatialOps._resize
ENGINE_ROUTES = {
    "rows": ("rows", "fp32", "x8_3x5", 8),
    "separable_fp32": ("separable", "fp32", "x8_3x5", 32),
    "separable_bf16": ("separable", "bf16", "x8_3x5", 8),
    "single": ("single", "fp32", "x2", 8),
    "single_bf16": ("single", "bf16", "x2", 8),
}

EW_M = 37
# name -> path, and per dtype (C, ld_a, ld_b, ld_out)
EW_FORMS = {
    "vec_c8": ("vec", {"fp32": (8, 16, 8, 24), "bf16": (8, 16, 8, 24)}),
    "scalar_c5": ("scalar", {"fp32": (5, 7, 5, 9), "bf16": (5, 7, 5, 9)}),
    "scalar_ld": ("scalar", {"fp32": (8, 8, 8, 10), "bf16": (8, 8, 8, 10)}),
}

# name -> (path, dtype, C, Cp, ld_y); HW = 35, N = 2
NCHW_HW = 35
NCHW_CASES = {
    "fast_f32": ("fast", "fp32", 3, 4, 8),
    "fast_bf16": ("fast", "bf16", 3, 8, 16),
    "general_c1": ("general", "fp32", 1, 8, 9),
    "general_c13_f32": ("general", "fp32", 13, 16, 17),
    "general_c13_bf16": ("general", "bf16", 13, 16, 17),
    "general_by_ld": ("general", "bf16", 3, 8, 9),
}

# name -> (path, M, K)
BIAS_CASES = {
    "k1_float4": ("float4", 4 * (4 * 1024 + 1024 + 37), 1),
    "k1_general": ("general", 8 * 1024 + 1024 + 5, 1),
    "k9": ("general", 8 * 1024 + 1024 + 5, 9),
    "k1_m1": ("general", 1, 1),
    "k9_m1": ("general", 1, 9),
}

# the two cases whose vector count just exceeds GRID_CAP * 256 (fp32, C = 4: one vector per pixel)
STRIDE2_BINARY_M = GRID_CAP * 256 + 1000
STRIDE2_BILINEAR = (1025, 1025, 2050, 2050)
