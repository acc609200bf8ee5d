"""numpy restatement of the augmented width pass (pn2_input_batch_width_aug, include/pn2.h) - TEST INFRASTRUCTURE ONLY; extends tests/inputbatchref.py.

RandomRotation(90) + RandomVerticalFlip + RandomHorizontalFlip of the polyp loaders are, on a PIL image, Image.rotate(angle, NEAREST, expand=False) and two
transposes.  Pillow's nearest-neighbour rotate is integer arithmetic: the matrix in Python doubles as Image.rotate forms it, six 16.16 fixed-point integers
(Geometry.c affine_fixed: FIX(v) = floor(v * 65536 + 0.5)), and per output pixel xin = (a2 + a0 x + a1 y) >> 16, yin = (a5 + a3 x + a4 y) >> 16, 0 outside.
Two routes to the same bytes are kept apart here: rotate_flip() uses the rotation's own integers and flips the result with numpy; rotate_coeffs() folds the
flips into the integers (x -> W-1-x, y -> H-1-y), which is what the device table holds, and gather() reads through them."""
import math

import numpy as np

import inputbatchref as R

I32 = (-(1 << 31), (1 << 31) - 1)


def fix(v):
    return int(math.floor(v * 65536.0 + 0.5))


def rotate_matrix(angle, H, W):
    """the six doubles Image.rotate hands to Image.transform(AFFINE) for an image of H rows and W columns"""
    r = -math.radians(float(angle) % 360.0)
    m = [round(math.cos(r), 15), round(math.sin(r), 15), 0.0, round(-math.sin(r), 15), round(math.cos(r), 15), 0.0]
    cx, cy = W / 2, H / 2
    x, y = -cx - 0, -cy - 0
    m[2], m[5] = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    m[2] += cx
    m[5] += cy
    return m


def rotate_ints(angle, H, W):
    m = rotate_matrix(angle, H, W)
    return [fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5)]


def rotate_coeffs(angle, flip_v, flip_h, H, W):
    """((a0 .. a5), mode): the row of the second table - the rotation's integers with the flips folded in; mode 0 for no rotation and no flip"""
    a0, a1, a2, a3, a4, a5 = rotate_ints(angle, H, W)
    if flip_v:
        a2, a5, a1, a4 = a2 + a1 * (H - 1), a5 + a4 * (H - 1), -a1, -a4
    if flip_h:
        a2, a5, a0, a3 = a2 + a0 * (W - 1), a5 + a3 * (W - 1), -a0, -a3
    return (a0, a1, a2, a3, a4, a5), int(float(angle) % 360.0 != 0.0 or bool(flip_v) or bool(flip_h))


def gather(img, a):
    """out[y][x] = img[yin][xin] or 0: a uint8 [H][W][C] image read through the six integers.  Every sum (and the one a running sum reaches one step past the
    last column) must fit int32, as the kernel's arithmetic is 32-bit: asserted."""
    H, W = img.shape[:2]
    a = [int(v) for v in a]
    for k in (0, 3):          # the sums are affine: their values at the corners bound them
        corners = [a[k + 2] + a[k] * x + a[k + 1] * y for x in (0, W) for y in (0, H - 1)]
        assert I32[0] <= min(corners) and max(corners) <= I32[1]
    x, y = np.arange(W, dtype=np.int64)[None, :], np.arange(H, dtype=np.int64)[:, None]
    xin, yin = (a[2] + a[0] * x + a[1] * y) >> 16, (a[5] + a[3] * x + a[4] * y) >> 16
    ok = (xin >= 0) & (xin < W) & (yin >= 0) & (yin < H)
    flat = np.where(ok, yin * W + xin, 0).reshape(-1)
    out = img.reshape(H * W, -1)[flat].reshape(img.shape)
    out[~ok] = 0
    return out


def rotate_flip(img, angle, flip_v, flip_h):
    """Image.rotate(angle, NEAREST) -> FLIP_TOP_BOTTOM -> FLIP_LEFT_RIGHT of a uint8 [H][W][C] image, the flips done on the rotated array"""
    out = gather(img, rotate_ints(angle, *img.shape[:2]))
    if flip_v:
        out = out[::-1]
    if flip_h:
        out = out[:, ::-1]
    return np.ascontiguousarray(out)


def aug_rows(shapes, draws):
    """the second table (pn2.input.AUG rows) of slots of these shapes: draws[i] = (angle, flip_v, flip_h) or None (mode 0)"""
    from pn2.input import AUG
    rows = np.zeros(len(shapes), dtype=AUG)
    for i, (s, d) in enumerate(zip(shapes, draws)):
        if s is not None and d is not None and s[0] > 0:
            rows[i]["a"], rows[i]["mode"] = rotate_coeffs(d[0], d[1], d[2], s[0], s[1])
    return rows


def width_pass(rows, aug, src, tmp, taps, S):
    """inputbatchref.width_pass with every mode-1 slot's source read through its map"""
    for r, g in zip(rows, aug):
        H, W, C = int(r["H"]), int(r["W"]), int(r["C"])
        if H == 0:
            continue
        img = src[int(r["src"]):int(r["src"]) + H * W * C].reshape(H, W, C)
        if int(g["mode"]) == 1:
            img = gather(img, g["a"])
        if W != S:
            img = R.one_pass(img, *R.tap_views(taps, r["tap_w"], S, int(r["kw"])), axis=1)
        tmp[int(r["tmp"]):int(r["tmp"]) + H * S * C] = img.reshape(-1)


def run(rows, aug, src, taps, S, tmp_bytes, n_rgb, n_mask, fill=np.float32(-7.0)):
    """inputbatchref.run for an augmented batch: (tmp, out_rgb, out_mask)"""
    tmp = np.full(int(tmp_bytes), 0xA5, np.uint8)
    out_rgb, out_mask = np.full((n_rgb, 3, S, S), fill, np.float32), np.full((n_mask, 1, S, S), fill, np.float32)
    width_pass(rows, aug, src, tmp, taps, S)
    R.height_pass(rows, tmp, taps, S, out_rgb, out_mask)
    return tmp, out_rgb, out_mask


def pil_pipeline(img, draw, S, norm):
    """What the reference loader computes for one decoded image: Pillow rotate, the two flips, resize((S, S), BILINEAR), then ToTensor (and Normalize) in float32.
    img: uint8 [H][W][3] or [H][W]; draw: (angle, flip_v, flip_h) or None (no augmentation)."""
    from PIL import Image
    pil = Image.fromarray(img)
    if draw is not None:
        pil = pil_rotate_flip(pil, *draw)
    res = np.asarray(pil.resize((S, S), Image.BILINEAR))
    return R.to_tensor(res.reshape(S, S, -1), norm)


def pil_rotate_flip(pil, angle, flip_v, flip_h):
    from PIL import Image
    pil = pil.rotate(angle, Image.NEAREST, expand=False)
    if flip_v:
        pil = pil.transpose(Image.FLIP_TOP_BOTTOM)
    if flip_h:
        pil = pil.transpose(Image.FLIP_LEFT_RIGHT)
    return pil
