"""numpy restatement of the ragged-batch input transform (pn2_input_batch_width / pn2_input_batch_height, include/pn2.h) - TEST INFRASTRUCTURE ONLY.

It reads the same table (pn2.input.SLOT rows) and the same three arenas as the kernels: a packed uint8 source arena, a uint8 scratch arena of [H][S][C] images and an
int32 tap arena of blocks xmin[S] | count[S] | kk[S][ksize].  Width pass, then height pass; a pass over an axis that already has length S is a copy; a byte is
(2^21 + sum src * kk) >> 22 clipped to 0..255 (int64 here: no overflow to think about); ToTensor / Normalize are numpy float32 divisions."""
import numpy as np

PREC = 22
MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)


def tap_views(taps, off, S, ksize):
    """(xmin[S], count[S], kk[S][ksize]) of the block at int32 offset `off`"""
    off = int(off)
    return taps[off:off + S], taps[off + S:off + 2 * S], taps[off + 2 * S:off + 2 * S + S * ksize].reshape(S, ksize)


def one_pass(img, xmin, cnt, kk, axis):
    """one separable pass over `axis` of a uint8 [H][W][C] image"""
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((len(xmin),) + src.shape[1:], np.int64)
    for o in range(len(xmin)):
        n = int(cnt[o])
        k = kk[o, :n].astype(np.int64).reshape((n,) + (1,) * (src.ndim - 1))
        out[o] = ((1 << (PREC - 1)) + (src[int(xmin[o]):int(xmin[o]) + n] * k).sum(axis=0)) >> PREC
    return np.moveaxis(np.clip(out, 0, 255).astype(np.uint8), 0, axis)


def to_tensor(img, norm, mean=MEAN, std=STD):
    """uint8 [S][S][C] -> fp32 [C][S][S]: / 255 and, with norm, (t - mean[c]) / std[c], every operation in float32"""
    t = img.astype(np.float32) / np.float32(255.0)
    if norm:
        t = (t - np.asarray(mean, np.float32)[:img.shape[2]]) / np.asarray(std, np.float32)[:img.shape[2]]
    return np.ascontiguousarray(t.transpose(2, 0, 1))


def width_pass(rows, src, tmp, taps, S):
    """fills the scratch arena `tmp` in place; bytes outside the live slots' [H][S][C] images are not touched"""
    for r in rows:
        H, W, C = int(r["H"]), int(r["W"]), int(r["C"])
        if H == 0:
            continue
        img = src[int(r["src"]):int(r["src"]) + H * W * C].reshape(H, W, C)
        if W != S:
            img = one_pass(img, *tap_views(taps, r["tap_w"], S, int(r["kw"])), axis=1)
        tmp[int(r["tmp"]):int(r["tmp"]) + H * S * C] = img.reshape(-1)


def height_bytes(rows, tmp, taps, S):
    """the uint8 [S][S][C] image of every slot (None for an empty one): the bytes the fused kernel forms and does not store"""
    out = []
    for r in rows:
        H, C = int(r["H"]), int(r["C"])
        if H == 0:
            out.append(None)
            continue
        img = tmp[int(r["tmp"]):int(r["tmp"]) + H * S * C].reshape(H, S, C)
        out.append(img.copy() if H == S else one_pass(img, *tap_views(taps, r["tap_h"], S, int(r["kh"])), axis=0))
    return out


def height_pass(rows, tmp, taps, S, out_rgb, out_mask, mean=MEAN, std=STD):
    """fills out_rgb [n][3][S][S] / out_mask [n][1][S][S] (fp32) in place; an empty slot's sample is not touched"""
    for r, b in zip(rows, height_bytes(rows, tmp, taps, S)):
        if b is not None:
            (out_rgb if int(r["C"]) == 3 else out_mask)[int(r["dst"])] = to_tensor(b, bool(r["norm"]), mean, std)


def run(rows, src, taps, S, tmp_bytes, n_rgb, n_mask, fill=np.float32(-7.0)):
    """(tmp, out_rgb, out_mask) of a whole batch; tmp starts as 0xA5 bytes and the outputs as `fill`, so untouched places show"""
    tmp = np.full(int(tmp_bytes), 0xA5, np.uint8)
    out_rgb, out_mask = np.full((n_rgb, 3, S, S), fill, np.float32), np.full((n_mask, 1, S, S), fill, np.float32)
    width_pass(rows, src, tmp, taps, S)
    height_pass(rows, tmp, taps, S, out_rgb, out_mask)
    return tmp, out_rgb, out_mask


def pack(arrays, rows, src_bytes, fill=0xA5):
    """the source arena of a batch: every array at its row's offset, `fill` elsewhere"""
    src = np.full(int(src_bytes), fill, np.uint8)
    for a, r in zip(arrays, rows):
        if a is not None and int(r["H"]) > 0:
            src[int(r["src"]):int(r["src"]) + a.size] = np.ascontiguousarray(a).reshape(-1)
    return src
