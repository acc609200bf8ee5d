"""float64 restatement (torch, CPU) of flip test-time augmentation over the fused label tail (pn2_seg_labels_up_tta, csrc/pn2_seg.hip; the reference's tta_model,
multiclass_seg/EMCAD/utils/utils.py:303-325): every view's NHWC maps are up-sampled bilinearly with align_corners = False by the coordinate rule of bl_src
(pn2_common.h), flipped back, combined per mode in the order of seg_labels_k, and the views are added - their combined logits ("logit") or their softmax over the
K channels ("prob").  The sum is not divided by the number of views: the argmax does not see it.  The maps hold V * N samples, view v of sample n at v * N + n.
Shared by tests/test_ttaref_cpu.py (which holds it to torch's own interpolate / flip / softmax) and the GPU tests.  Not a test module."""
import numpy as np
import torch

F64 = torch.float64
MODES = {"last": 0, "sum_fg": 1, "sum_fg_minus_bg": 2}
VIEWS = {"id": 0, "h": 1, "v": 2, "hv": 3}          # bit 0: x mirrored, bit 1: y mirrored
AVERAGES = {"logit": 0, "prob": 1}
VIEW_SETS = [("id",), ("h",), ("id", "h", "v"), ("id", "h", "v", "hv"), ("hv", "id")]
MAX_EXCUSED = 0.005          # share of a case's pixels that may sit within the threshold of a tie
# The random maps are N(0, 1) * SCALE.  At SCALE = 4 the summed logits saturate the softmax, every view votes with probability 1 - 1e-7 and views that disagree
# tie: up to 14 % of a case's pixels lie within gap_cap of a tie in float64 ('prob').  At 1 the worst case holds 0.21 % (one pixel of 480; the smallest cases have
# 120 pixels, so the limit allows them none); tests/test_ttaref_cpu.py checks every case with the seeds of seed_of.
SCALE = 1.0


def bl_src(On, r, In):
    """bl_src(o, r, 0, In, ...) for o = 0 .. On-1 in float64: (i0, i1, l0, l1)."""
    o = torch.arange(On, dtype=F64)
    s = torch.clamp(r * (o + 0.5) - 0.5, min=0.0)
    i0 = torch.clamp(s.floor().long(), max=In - 1)
    i1 = i0 + (i0 < In - 1).long()
    l1 = s - i0.to(F64)
    return i0, i1, 1.0 - l1, l1


def upsample(m, s):
    """[N][h][w][K] -> float64 [N][h*s][w*s][K]."""
    m = torch.as_tensor(m).to(F64)
    N, h, w, K = m.shape
    y0, y1, ly0, ly1 = bl_src(h * s, 1.0 / s, h)
    x0, x1, lx0, lx1 = bl_src(w * s, 1.0 / s, w)
    ly0, ly1 = ly0[None, :, None, None], ly1[None, :, None, None]
    lx0, lx1 = lx0[None, None, :, None], lx1[None, None, :, None]
    top, bot = m[:, y0], m[:, y1]
    return ly0 * (lx0 * top[:, :, x0] + lx1 * top[:, :, x1]) + ly1 * (lx0 * bot[:, :, x0] + lx1 * bot[:, :, x1])


def flip_back(x, view):
    """x [N][H][W][...] of a view -> in the frame of the unflipped image (a flip is its own inverse)."""
    code = VIEWS[view]
    dims = [d for d, bit in ((2, 1), (1, 2)) if code & bit]
    return torch.flip(x, dims) if dims else x


def combine(ups, mode):
    if mode == "last":
        return ups[-1]
    v = torch.zeros_like(ups[0])
    if mode == "sum_fg":
        for p in ups:
            v = v + p
        return v
    h = len(ups) // 2
    for p, q in zip(ups[:h], ups[h:]):
        v = v + (p - q)
    return v


def scores(maps, scales, mode, views, average, K):
    """float64 [N][H][W][K]: the summed per-view logits or probabilities of maps [V * N][h][w][>= K]."""
    V = len(views)
    N = maps[0].shape[0] // V
    tot = None
    for v, view in enumerate(views):
        ups = [flip_back(upsample(torch.as_tensor(m)[v * N:(v + 1) * N, :, :, :K], s), view) for m, s in zip(maps, scales)]
        x = combine(ups, mode)
        if average == "prob":
            x = torch.softmax(x, dim=-1)
        tot = x if tot is None else tot + x
    return tot


def labels(sc):
    """uint8 [N][H][W]: the first maximum over the last axis."""
    return torch.argmax(sc, dim=-1).to(torch.uint8)


def gap(sc):
    """float64 [N][H][W]: the largest score minus the second largest."""
    top = torch.topk(sc, 2, dim=-1).values
    return top[..., 0] - top[..., 1]


def deficit(sc, got):
    """float64 [N][H][W]: how far the score of the class `got` picked lies below the largest score (0 where it picked a maximum)."""
    return sc.max(dim=-1).values - torch.gather(sc, -1, torch.as_tensor(got).long()[..., None])[..., 0]


def gap_cap(mode, average, nmaps, V, maxabs):
    """Upper estimate, from the number formats alone, of twice the fp32 error of a score - the largest float64 top-two gap at which an fp32 evaluation may pick
    another class.  One up-sampled value: three roundings of the four-tap expression, <= 4 * 2^-24 * maxabs.  A combined logit of n maps (n differences of
    two in mode 2, maxabs doubling): the n values' errors plus n adds of partial sums <= n * maxabs, together <= (4 n + n^2) * 2^-24 * maxabs <= 16 n * 2^-24
    * maxabs * (n / 8 + 1/4) - rounded up to e_l = 16 * nmaps * 2^-23 * maxabs, the margin tests/test_gpu_seg_labels_up.py derives for the same expression.
    'logit': V such logits and V adds -> e = V * e_l * (1 + 2^-23 * V).  'prob': a probability moves by at most sum_j |dp_i / dl_j| * e_l = 2 p (1 - p) * e_l <=
    e_l / 2, exp, the K-term sum and the division add <= 16 * 2^-24 (p <= 1) -> e = V * (e_l / 2 + 2^-20).  Returned: 2 * e (two scores move)."""
    e_l = 16 * nmaps * 2.0 ** -23 * maxabs
    e = V * e_l * (1 + 2.0 ** -20) if average == "logit" else V * (e_l / 2 + 2.0 ** -20)
    return 2 * e


# ---------------------------------------------------------------------------------------------------------------- the cases of the kernel tests
def map_set(name):
    """(low-resolution sizes (h, w), scales) of the map sets: (a) four maps to 32 x 32, (b) one 3 x 5 map to 12 x 20, (c) two 5 x 3 maps to 10 x 6, (d) the eight dual
    maps of (a)."""
    a = ([(1, 1), (2, 2), (4, 4), (8, 8)], [32, 16, 8, 4])
    return {"a": a, "b": ([(3, 5)], [4]), "c": ([(5, 3)] * 2, [2, 2]), "d": (a[0] * 2, a[1] * 2)}[name]


def cases():
    """(map set, mode) pairs: every mode on a set that fits it.  'last' takes the last map of a set."""
    return [("a", "last"), ("a", "sum_fg"), ("b", "last"), ("b", "sum_fg"), ("c", "last"), ("c", "sum_fg"), ("c", "sum_fg_minus_bg"), ("d", "sum_fg_minus_bg")]


def seed_of(name, mode, K, views):
    return 700000 + 1000 * K + 100 * "abcd".index(name) + 10 * MODES[mode] + VIEW_SETS.index(tuple(views))


def random_maps(name, K, ld, V, N, seed, scale=SCALE):
    """float32 NHWC maps [V * N][h][w][ld] of a map set, N(0, 1) * scale in the channels below K and NaN in the padding: nothing may use it."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for h, w in map_set(name)[0]:
        t = torch.full((V * N, h, w, ld), float("nan"))
        t[..., :K] = torch.randn(V * N, h, w, K, generator=g) * scale
        out.append(t)
    return out


LEVELS = np.array([-4, -2, -1, -33 / 64, -1 / 64, 0, 1 / 64, 31 / 64, 1, 2, 4], np.float32)          # multiples of 1/64 with |v| <= 4


def dyadic_maps(name, K, ld, V, N, seed):
    """As random_maps with values from LEVELS: with scales that are powers of two up to 32 the bilinear weights are multiples of 1/64, every product a multiple
    of 2^-18, an up-sampled value at most 4 and a sum of 4 maps over 4 views at most 64 = 2^24 * 2^-18: float32 holds every intermediate of the modes 'last'
    and 'sum_fg' exactly, whatever the order, the rounding or the contraction, and channels tie often."""
    g = np.random.default_rng(seed)
    out = []
    for h, w in map_set(name)[0]:
        m = np.full((V * N, h, w, ld), np.nan, np.float32)
        m[..., :K] = LEVELS[g.integers(0, len(LEVELS), (V * N, h, w, K))]
        out.append(torch.from_numpy(m))
    return out


# ---------------------------------------------------------------------------------------------------------------- the unfused fp32 composition (GPU)
def unfused_ups(dmaps, scales, views, K, N):
    """GPU: per view the list of its device maps [V * N][h][w][>= K] up-sampled by the project's bilinear op and flipped back: fp32 NCHW [N][K][OH][OW]."""
    from pn2.engine import Act, Engine, F32
    eng = Engine(F32, False, need_grad=False)
    out = []
    for v, view in enumerate(views):
        dims = [d for d, bit in ((3, 1), (2, 2)) if VIEWS[view] & bit]
        ups = []
        for t, s in zip(dmaps, scales):
            blk = t[v * N:(v + 1) * N, :, :, :K].contiguous()
            u = eng.to_nchw(eng.bilinear(Act(eng, blk, K, K, K, F32, requires_grad=False), s))
            ups.append(torch.flip(u, dims).contiguous() if dims else u.contiguous())
        out.append(ups)
    return out


def unfused_scores(per_view, mode, average):
    """The fp32 scores of the unfused composition, torch ops on the device: [N][OH][OW][K]."""
    tot = None
    for ups in per_view:
        if mode == "last":
            x = ups[-1]
        elif mode == "sum_fg":
            x = torch.zeros_like(ups[0])
            for p in ups:
                x = x + p
        else:
            x = torch.zeros_like(ups[0])
            for p, q in zip(ups[:len(ups) // 2], ups[len(ups) // 2:]):
                x = x + (p - q)
        if average == "prob":
            x = torch.softmax(x, dim=1)
        tot = x if tot is None else tot + x
    return tot.permute(0, 2, 3, 1)
