"""numpy restatement, in float32, of the fused label tail pn2_seg_labels_up (csrc/pn2_seg.hip): bl_src at align_corners = 0, the four-tap expression of
bilinear_fwd_k, the three combinations of seg_labels_k in their order, and its tie / NaN rule.  Maps are NHWC [N][h][w][ld] arrays whose channels K .. ld-1 are
padding.  Every operation is rounded to float32 on its own (no fused multiply-add); on the dyadic inputs of dyadic_maps every intermediate is exact, so this,
torch on the CPU and the kernels agree to the bit whatever their contraction.  Not a test module."""
import numpy as np

f32 = np.float32
MODES = {"last": 0, "sum_fg": 1, "sum_fg_minus_bg": 2}


def bl_src(On, r, In):
    """bl_src(o, r, 0, In, ...) of pn2_common.h for o = 0 .. On-1: (i0, i1, l0, l1).  r * (o + 0.5) - 0.5 is a fused multiply-add on the device; for the
    power-of-two scales used here the product is exact, so the two roundings coincide."""
    o = np.arange(On, dtype=f32)
    s = np.maximum(f32(r) * (o + f32(0.5)) - f32(0.5), f32(0))
    i0 = np.minimum(s.astype(np.int32), In - 1)
    i1 = i0 + (i0 < In - 1)
    l1 = (s - i0.astype(f32)).astype(f32)
    return i0, i1, (f32(1) - l1).astype(f32), l1


def upsample(m, s):
    """[N][h][w][C] -> [N][h*s][w*s][C]: ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * d), every operation in float32."""
    m = np.asarray(m, f32)
    N, h, w, C = m.shape
    r = f32(1.0 / s)
    y0, y1, ly0, ly1 = bl_src(h * s, r, h)
    x0, x1, lx0, lx1 = bl_src(w * s, r, w)
    ly0, ly1 = ly0[None, :, None, None], ly1[None, :, None, None]
    lx0, lx1 = lx0[None, None, :, None], lx1[None, None, :, None]
    a, b = m[:, y0][:, :, x0], m[:, y0][:, :, x1]
    c, d = m[:, y1][:, :, x0], m[:, y1][:, :, x1]
    with np.errstate(invalid="ignore"):
        return (ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * d)).astype(f32)


def combine(ups, mode):
    """The combined logits [N][H][W][C] of seg_labels_k: 'last', 0.0 + P0 + P1 + ..., 0.0 + (P0 - Pbg0) + (P1 - Pbg1) + ... in float32, in this order."""
    with np.errstate(invalid="ignore"):
        if mode == "last":
            return ups[-1]
        v = np.zeros_like(ups[0])
        if mode == "sum_fg":
            for p in ups:
                v = (v + p).astype(f32)
            return v
        h = len(ups) // 2
        for p, q in zip(ups[:h], ups[h:]):
            v = (v + (p - q).astype(f32)).astype(f32)
        return v


def argmax(v, K):
    """k == 0 || v > best || (v != v && best == best) over the channels 0 .. K-1: the first maximum, a NaN counting as the maximum."""
    best, bk = v[..., 0].copy(), np.zeros(v.shape[:-1], np.uint8)
    with np.errstate(invalid="ignore"):
        for k in range(1, K):
            x = v[..., k]
            upd = (x > best) | (np.isnan(x) & ~np.isnan(best))
            best, bk = np.where(upd, x, best), np.where(upd, np.uint8(k), bk)
    return bk


def labels(maps, scales, mode, K):
    """uint8 [N][H][W]: the fused tail on NHWC maps [N][h][w][ld >= K]."""
    return argmax(combine([upsample(np.asarray(m)[..., :K], s) for m, s in zip(maps, scales)], mode), K)


def tie_share(maps, scales, mode, K):
    """Share of the pixels whose maximal combined logit is attained by more than one channel."""
    v = combine([upsample(np.asarray(m)[..., :K], s) for m, s in zip(maps, scales)], mode)
    return float(((v == v.max(axis=-1, keepdims=True)).sum(axis=-1) > 1).mean())


LEVELS = np.array([-4, -2, -1, -33 / 64, -1 / 64, 0, 1 / 64, 31 / 64, 1, 2, 4], f32)          # multiples of 1/64 with |v| <= 4


def dyadic_maps(K, ld, sizes, N, seed):
    """One NHWC map [N][h][w][ld] for each (h, w) of sizes, values drawn from LEVELS: few levels, so neighbouring channels tie; in sample 0 channel K-1 is a
    copy of channel 0 besides, so those two tie wherever they lead.  The padding channels K .. ld-1 hold NaN: nothing may use them.
    With scales that are powers of two up to 32 the bilinear weights are multiples of 1/64, every product a multiple of 2^-18 below 2^2 and every sum of the
    eight-map combinations below 2^5: 23 bits hold all of it, so float32 is exact whatever the order, the rounding or the contraction."""
    g = np.random.default_rng(seed)
    out = []
    for h, w in sizes:
        m = np.full((N, h, w, ld), np.nan, f32)
        m[..., :K] = LEVELS[g.integers(0, len(LEVELS), (N, h, w, K))]
        m[0, :, :, K - 1] = m[0, :, :, 0]
        out.append(m)
    return out


def case(mode):
    """(number of maps, scales) of a mode as the volume functions use it: the last map, the four foreground maps, four foreground + four background maps."""
    return {"last": (1, [4]), "sum_fg": (4, [32, 16, 8, 4]), "sum_fg_minus_bg": (8, [32, 16, 8, 4] * 2)}[mode]
