"""numpy float64 restatement of what the Synapse loader and test_single_volume do to a slice (multiclass_seg/EMCAD/utils/dataset_synapse.py:12-47,
utils/utils.py:179-181,197-198): scipy.ndimage.zoom(order=3) and (order=0) with scipy's defaults (mode='constant', cval=0, prefilter=True, grid_mode=False),
ndimage.rotate(order=0, reshape=False), and np.flip(np.rot90).  Every operation is written out in the order scipy's C code performs it, so the float32 cast of
the result equals scipy's output bit for bit (tests/test_zoomref_cpu.py pins that); pn2/volinput.py has to reproduce these arrays exactly."""
import numpy as np

POLE = -0.267949192431122706472553658494127633          # sqrt(3) - 2 rounded once, the literal of ni_splines.c:get_filter_poles; np.sqrt(3.0) - 2.0 is one ulp away
GAIN = (1.0 - POLE) * (1.0 - 1.0 / POLE)


def pole_pow(n):
    """z ** (n - 1) as the C library's pow gives it (ni_splines.c:_init_causal_mirror)."""
    return float(np.float64(POLE) ** (n - 1))


def _filter_axis0(c):
    """The cubic B-spline prefilter along axis 0 of a float64 array [n][...] in place: gain, mirror initialisation, causal and anticausal sweep."""
    n = c.shape[0]
    if n == 1:
        return c
    z = POLE
    c *= GAIN
    zn = pole_pow(n)
    c0 = c[0] + zn * c[n - 1]
    zi = z
    for i in range(1, n - 1):
        c0 = c0 + zi * (c[i] + zn * c[n - 1 - i])
        zi *= z
    c[0] = c0 / (1 - zn * zn)
    for i in range(1, n):
        c[i] = c[i] + z * c[i - 1]
    c[n - 1] = (z * c[n - 2] + c[n - 1]) * z / (z * z - 1)
    for i in range(n - 2, -1, -1):
        c[i] = z * (c[i + 1] - c[i])
    return c


def prefilter(a):
    """float64 spline coefficients of a 2-D array: axis 0, then axis 1 (the order decides bits)."""
    c = np.array(a, dtype=np.float64)
    _filter_axis0(c)
    c = np.ascontiguousarray(c.T)
    _filter_axis0(c)
    return np.ascontiguousarray(c.T)


def _coords(nin, nout):
    zr = (nin - 1) / (nout - 1) if nout > 1 else 1.0
    cc = np.arange(nout, dtype=np.float64) * zr
    return cc, ~(cc > nin - 1)


def tables3(nin, nout):
    """Per output index: 4 tap indices folded by mirror about 0 and nin - 1, 4 weights, validity (cc <= nin - 1)."""
    cc, valid = _coords(nin, nout)
    fl = np.floor(cc)
    idx = fl.astype(np.int64)[:, None] + np.arange(-1, 3)[None, :]
    if nin == 1:
        idx[:] = 0
    else:
        p = 2 * (nin - 1)
        idx = np.where(idx < 0, -idx, idx) % p          # ni_interpolation.c folds negative taps first, then the period
        idx = np.where(idx > nin - 1, p - idx, idx)
    y = cc - fl
    u = 1 - y
    w = np.empty((nout, 4), np.float64)
    w[:, 1] = (y * y * (y - 2) * 3 + 4) / 6
    w[:, 2] = (u * u * (u - 2) * 3 + 4) / 6
    w[:, 0] = u * u * u / 6
    w[:, 3] = 1 - w[:, 0] - w[:, 1] - w[:, 2]
    return idx, w, valid


def tables0(nin, nout):
    cc, valid = _coords(nin, nout)
    idx = np.floor(cc + 0.5).astype(np.int64)
    return np.where(valid, idx, 0), valid


def zoom3_f64(a, oh, ow):
    """scipy.ndimage.zoom(a, (oh / H, ow / W), order=3, output=float64): the sum before the cast, for the float64 pin of the CPU test."""
    a = np.asarray(a)
    H, W = a.shape
    c = prefilter(a)
    iy, wy, vy = tables3(H, oh)
    ix, wx, vx = tables3(W, ow)
    t = np.zeros((oh, ow), np.float64)
    for j in range(4):
        rows = c[iy[:, j]]                                # [oh][W]
        for k in range(4):
            t = t + (rows[:, ix[:, k]] * wy[:, j, None]) * wx[None, :, k]
    t[~vy, :] = 0.0
    t[:, ~vx] = 0.0
    return t


def zoom3(a, oh, ow):
    """scipy.ndimage.zoom(a, (oh / H, ow / W), order=3) of a 2-D float array -> float32 [oh][ow]."""
    return zoom3_f64(a, oh, ow).astype(np.float32)


def zoom0(a, oh, ow):
    """scipy.ndimage.zoom(a, (oh / H, ow / W), order=0): nearest sample, the dtype kept."""
    a = np.asarray(a)
    H, W = a.shape
    iy, vy = tables0(H, oh)
    ix, vx = tables0(W, ow)
    out = a[iy][:, ix].copy()
    out[~vy, :] = 0
    out[:, ~vx] = 0
    return out


def rotate_matrix(angle, H, W):
    """(m00, m01, m10, m11, off0, off1) of ndimage.rotate(angle, reshape=False)."""
    ang = np.deg2rad(angle)
    c, s = np.cos(ang), np.sin(ang)
    m = np.array([[c, s], [-s, c]])
    ctr = (np.array([H, W]) - 1) / 2
    off = ctr - m @ ctr
    return float(m[0, 0]), float(m[0, 1]), float(m[1, 0]), float(m[1, 1]), float(off[0]), float(off[1])


def rotate0(a, angle):
    """scipy.ndimage.rotate(a, angle, order=0, reshape=False) of a 2-D array, the dtype kept."""
    a = np.asarray(a)
    H, W = a.shape
    m00, m01, m10, m11, o0, o1 = rotate_matrix(angle, H, W)
    y = np.arange(H, dtype=np.float64)[:, None]
    x = np.arange(W, dtype=np.float64)[None, :]
    cy = (o0 + y * m00) + x * m01
    cx = (o1 + y * m10) + x * m11
    inside = ~((cy < 0) | (cy > H - 1) | (cx < 0) | (cx > W - 1))
    iy = np.where(inside, np.floor(cy + 0.5), 0).astype(np.int64)
    ix = np.where(inside, np.floor(cx + 0.5), 0).astype(np.int64)
    return np.where(inside, a[iy, ix], a.dtype.type(0))


def rot_flip(a, k, axis):
    return np.flip(np.rot90(a, k), axis).copy()


def random_generator(image, label, output_size, draws):
    """RandomGenerator.__call__ on a batch with the random decisions given: image float [N][H][W], label [N][H][W], draws[i] one of
    ('rot_flip', k, axis), ('rotate', angle), None -> {'image': float32 [N][1][oh][ow], 'label': int64 [N][oh][ow]}."""
    oh, ow = output_size
    imgs, labs = [], []
    for im, lb, d in zip(image, label, draws):
        if d is not None and d[0] == "rot_flip":
            im, lb = rot_flip(im, d[1], d[2]), rot_flip(lb, d[1], d[2])
        elif d is not None and d[0] == "rotate":
            im, lb = rotate0(im, d[1]), rotate0(lb, d[1])
        elif d is not None:
            raise ValueError(d)
        if im.shape != (oh, ow):
            im, lb = zoom3(im, oh, ow), zoom0(lb, oh, ow)
        imgs.append(im.astype(np.float32)[None])
        labs.append(lb.astype(np.float32).astype(np.int64))
    return {"image": np.stack(imgs), "label": np.stack(labs)}


# ------------------------------------------------------------------------------------------------ the cases the tests and tests/golden/synapse_zoom.npz share
SHAPES = [((7, 9), (12, 5)), ((2, 3), (7, 7)), ((5, 5), (5, 9)), ((33, 17), (16, 40)), ((64, 48), (28, 28)), ((28, 28), (64, 48)), ((100, 100), (37, 41)),
          ((3, 640), (5, 300)), ((512, 512), (224, 224)), ((224, 224), (512, 512))]
ZERO_LAST_ROW = {((64, 48), (28, 28)), ((512, 512), (224, 224))}
ZERO_LAST_COL = {((28, 28), (64, 48)), ((512, 512), (224, 224))}
ROTATE_SHAPES = [(37, 41), (64, 64)]
ANGLES = list(range(-20, 20))


def case_input(shape, seed=0):
    """(float32 image in [-0.3, 1.7], uint8 labels in 0..8) of one shape, from numpy's PCG64 so that every user sees the same arrays."""
    g = np.random.default_rng(1000 * shape[0] + shape[1] + 7919 * seed)
    return (g.random(shape) * 2.0 - 0.3).astype(np.float32), g.integers(0, 9, shape).astype(np.uint8)


def case_key(src, dst):
    return f"{src[0]}x{src[1]}_{dst[0]}x{dst[1]}"
