"""GPU tests, at the C ABI, of the two kernels of flip test-time augmentation (csrc/pn2_seg.hip): pn2_seg_labels_up_tta and pn2_flip_views.

Shapes: N = 2; K = 2, 4, 9 at ld = K (KV = 1 and 3; 16-byte reads at K = 4, scalar reads at 2 and 9) and K = 9 at ld = 16 with NaN padding (KV = 3, 16-byte reads);
the map sets of ttaref.map_set: (a) 1 x 1 .. 8 x 8 to 32 x 32, (b) 3 x 5 to 12 x 20 (not square, a row shorter than a wave, OH a multiple of 4), (c) two 5 x 3 to
10 x 6 (OH no multiple of 4), (d) the eight dual maps of (a); the view sets ("id",), ("h",), ("id","h","v"), ("id","h","v","hv"), ("hv","id"); the three modes; both averages.

Bit for bit:
  * views ("id",) with average "logit" returns the bytes of pn2_seg_labels_up, on Gaussian maps.
  * average "logit" in the modes 'last' and 'sum_fg' returns the labels of the unfused composition of the project's own ops - Engine.bilinear of every view's
    maps, torch.flip back, pn2_seg_labels over the list in view order (a torch fp32 sum in that order where the list is longer than its 8 maps) - and of ttaref
    in float64, on the dyadic maps of ttaref.dyadic_maps.  On those every intermediate is exact in float32, which the comparison needs: on other inputs the
    bilinear kernel rounds the four-tap expression differently from the fused tail (see seg_tap4 in csrc/pn2_seg.hip), and pn2_seg_labels adds the V * nmaps
    maps in one chain where the fused kernel adds per view first.  Gaussian inputs are covered by the float64 rule below.
  * pn2_flip_views against torch.flip at w = 5, 8, 20, every view code, and from a base that is not 16-byte aligned.
Against float64 (both averages in every mode, every view set), Gaussian maps N(0, 1) * ttaref.SCALE - the inexact inputs on which a wrong rounding, a
contracted add or a wrong view order of the "logit" average would show:
  * the threshold of a case is T = 2 * 3 * e32, e32 = the largest distance of the scores of the UNFUSED fp32 composition (Engine.bilinear, torch.flip, torch's
    fp32 sums and softmax on the device) from ttaref's float64 scores on the same inputs: margin 3, as the fp32-sum rule of tests/test_gpu_vit_kernels.py, and
    the factor 2 because two scores move.  Measured at run time; it has to stay below ttaref.gap_cap, the bound from the number formats, under which
    tests/test_ttaref_cpu.py holds the share of near ties of every case to 0.5 %.
  * the class the kernel picks may lie at most T below the largest float64 score, and at most 0.5 % of a case's pixels may have a float64 top-two gap below T.
Adversarial: two views whose own labels differ on most pixels (a kernel that drops a view or mirrors the wrong axis is wrong on most pixels, exactly); logits of
+-80 in one view under "prob".  Refusals: every -2 of the entry point leaves the output bytes as they were.
Each float64 case prints its figures (run with -s, lines starting with TTAK).

MI355X, 2026-10-21, the 323 float64 cases (160 of them "logit"): e32 between 4.6e-08 and 1.9e-06; T at most 0.15 of gap_cap (K = 4, set a, 'last', view id,
"logit": T 1.7e-06 against 1.1e-05); at most 4.9e-04 of a case's pixels within T of a tie (one pixel of 2048), none with a label other than float64's (largest
deficit 0); the three saturated cases: T 8.0e-07 .. 1.4e-06, the same."""
import ctypes as C
import os

import pytest
import torch

import ttaref as R

pytestmark = pytest.mark.gpu
os.environ.setdefault("PN2_NO_PRETRAINED", "1")
dev = "cuda"
N = 2
LAYOUTS = [(2, 2), (4, 4), (9, 9), (9, 16)]          # (K, ld)
IDS = ["K2", "K4", "K9", "K9-ld16"]


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pn2
    pn2.load_library()
    yield


def _table(dmaps):
    from pn2 import capi
    t = (capi.SegUpMap * len(dmaps))()
    for d, m in zip(t, dmaps):
        d.p, d.ld, d.H, d.W = m.data_ptr(), m.shape[3], m.shape[1], m.shape[2]
    return t


def _codes(views):
    return (C.c_int * len(views))(*[R.VIEWS[v] for v in views])


def _tta(dmaps, scales, mode, views, average, K, out=None):
    """pn2_seg_labels_up_tta on NHWC device maps [V * N][h][w][ld] -> (status, uint8 [N][OH][OW])"""
    from pn2 import capi
    from pn2.core import _stream
    OH, OW = dmaps[0].shape[1] * scales[0], dmaps[0].shape[2] * scales[0]
    if out is None:
        out = torch.full((N, OH, OW), 255, dtype=torch.uint8, device=dev)
    rc = capi.load().pn2_seg_labels_up_tta(_table(dmaps), len(dmaps), R.MODES[mode], _codes(views), len(views), R.AVERAGES[average], N, K, OH, OW,
                                           C.c_void_p(out.data_ptr()), _stream())
    return rc, out


def _used(maps, scales, mode):
    return (maps[-1:], scales[-1:]) if mode == "last" else (maps, scales)


# ------------------------------------------------------------------------------------------------ bit for bit
@pytest.mark.parametrize("K,ld", LAYOUTS, ids=IDS)
def test_identity_view_with_logit_average_is_the_plain_fused_tail(K, ld):
    from pn2 import voleval as V
    for name, mode in R.cases():
        _, scales = R.map_set(name)
        maps = [m.to(dev) for m in R.random_maps(name, K, ld, 1, N, R.seed_of(name, mode, K, ("id",)))]
        um, us = _used(maps, scales, mode)
        rc, got = _tta(um, us, mode, ("id",), "logit", K)
        assert rc == 0
        assert torch.equal(got, V.predict_labels_up([t[..., :K] for t in um], us, mode)), (name, mode)


@pytest.mark.parametrize("K,ld", LAYOUTS, ids=IDS)
def test_logit_average_equals_the_unfused_composition_on_dyadic_maps(K, ld):
    from pn2 import voleval as V
    seen = 0
    for name, mode in R.cases():
        if mode == "sum_fg_minus_bg":
            continue
        _, scales = R.map_set(name)
        for views in R.VIEW_SETS:
            maps = R.dyadic_maps(name, K, ld, len(views), N, R.seed_of(name, mode, K, views))
            um, us = _used(maps, scales, mode)
            dm = [m.to(dev) for m in um]
            rc, got = _tta(dm, us, mode, views, "logit", K)
            assert rc == 0
            sc = R.scores(um, us, mode, views, "logit", K)
            assert torch.equal(got.cpu(), R.labels(sc)), (name, mode, views)
            seen += int((R.gap(sc) == 0).sum())
            flat = [u for ups in R.unfused_ups(dm, us, views, K, N) for u in ups]          # view order, the maps of a view in their order
            if len(flat) <= 8:
                want = V.predict_labels(flat, "sum_fg")
            else:
                x = torch.zeros_like(flat[0])
                for u in flat:
                    x = x + u
                want = torch.argmax(x, dim=1).to(torch.uint8)
            assert torch.equal(got, want), (name, mode, views)
    assert seen > 0          # ties between channels occurred and were resolved alike


@pytest.mark.parametrize("w", [5, 8, 20])
def test_flip_views_is_torch_flip_bit_for_bit(w):
    from pn2 import capi
    from pn2.core import _stream
    lib = capi.load()
    h = 3
    g = torch.Generator().manual_seed(40 + w)
    bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (N, h, w), generator=g, dtype=torch.int64).to(torch.int32)          # every bit pattern, NaN payloads included
    x = bits.view(torch.float32).to(dev)
    for shift in (0, 1):          # 1: a base 4 bytes past a 16-byte boundary (the scalar rung even where w % 4 == 0)
        src = x
        if shift:
            buf = torch.zeros(x.numel() + 1, device=dev)
            buf[1:].view(torch.int32).copy_(x.reshape(-1).view(torch.int32))
            src = buf[1:].view(x.shape)
            assert src.data_ptr() % 16 == 4
        for views in [(v,) for v in R.VIEWS] + R.VIEW_SETS[2:]:
            out = torch.full((len(views) * N, h, w), 7.0, device=dev)
            assert lib.pn2_flip_views(C.c_void_p(src.data_ptr()), N, h, w, _codes(views), len(views), C.c_void_p(out.data_ptr()), _stream()) == 0
            want = torch.cat([torch.flip(x, [d for d, bit in ((2, 1), (1, 2)) if R.VIEWS[v] & bit]) if R.VIEWS[v] else x for v in views])
            assert torch.equal(out.view(torch.int32), want.view(torch.int32)), (w, shift, views)


# ------------------------------------------------------------------------------------------------ against float64
def _check64(um, us, mode, views, average, K, tag):
    """The float64 rule of the module docstring for one case; returns (T, share of near ties, pixels that differ from the float64 labels)."""
    dm = [m.to(dev) for m in um]
    rc, got = _tta(dm, us, mode, views, average, K)
    assert rc == 0, tag
    sc = R.scores(um, us, mode, views, average, K)
    e32 = float((R.unfused_scores(R.unfused_ups(dm, us, views, K, N), mode, average).cpu().double() - sc).abs().max())
    T = 2 * 3 * e32
    cap = R.gap_cap(mode, average, len(um), len(views), max(float(m[..., :K].abs().max()) for m in um))
    share = float((R.gap(sc) < T).double().mean())
    worst = float(R.deficit(sc, got.cpu()).max())
    differ = int((got.cpu() != R.labels(sc)).sum())
    print(f"TTAK {tag}: e32 {e32:.2e} T {T:.2e} cap {cap:.2e} near ties {share:.2e} largest deficit {worst:.2e} pixels that differ {differ}")
    assert T <= cap, tag
    assert share <= R.MAX_EXCUSED, tag
    assert worst <= T, tag
    return T, share, differ


@pytest.mark.parametrize("K,ld", LAYOUTS, ids=IDS)
def test_both_averages_in_every_mode_against_float64(K, ld):
    for name, mode in R.cases():
        _, scales = R.map_set(name)
        for views in R.VIEW_SETS:
            maps = R.random_maps(name, K, ld, len(views), N, R.seed_of(name, mode, K, views))
            um, us = _used(maps, scales, mode)
            for average in R.AVERAGES:
                _check64(um, us, mode, views, average, K, f"K{K} ld{ld} {name} {mode} {'+'.join(views)} {average}")


# ------------------------------------------------------------------------------------------------ adversarial
@pytest.mark.parametrize("views", [("id", "h"), ("id", "v"), ("h", "hv"), ("v", "id")], ids=lambda v: "+".join(v))
def test_views_that_disagree_on_most_pixels(views):
    """Dyadic 3 x 5 maps (12 x 20 output, K = 4), two views with independent maps: each view alone labels most pixels differently from the other and from the
    pair, and mirroring the second view about the other axis (or not at all) changes most labels too.  On these inputs float32 is exact, so the kernel has to
    return ttaref's labels for the pair byte for byte: nothing is excused."""
    K = 4
    maps = R.dyadic_maps("b", K, K, 2, N, seed=900 + sum(R.VIEWS[v] for v in views) * 7 + R.VIEWS[views[0]])
    dm = [m.to(dev) for m in maps]
    want = R.labels(R.scores(maps, [4], "last", views, "logit", K))
    alone = [R.labels(R.scores([maps[0][v * N:(v + 1) * N]], [4], "last", (views[v],), "logit", K)) for v in range(2)]
    assert float((alone[0] != alone[1]).double().mean()) > 0.5
    assert all(float((a != want).double().mean()) > 0.25 for a in alone)
    for other in R.VIEWS:          # the second view mirrored any other way
        if other != views[1]:
            wrong = R.labels(R.scores(maps, [4], "last", (views[0], other), "logit", K))
            assert float((wrong != want).double().mean()) > 0.25, other
    rc, got = _tta(dm, [4], "last", views, "logit", K)
    assert rc == 0 and torch.equal(got.cpu(), want)
    rc, got = _tta(dm, [4], "last", views[::-1], "logit", K)          # the views swapped WITHOUT their samples: another, equally definite answer
    assert rc == 0 and torch.equal(got.cpu(), R.labels(R.scores(maps, [4], "last", views[::-1], "logit", K)))


@pytest.mark.parametrize("mode,name", [("last", "b"), ("sum_fg", "a"), ("sum_fg_minus_bg", "c")])
def test_saturated_logits_in_one_view_under_prob(mode, name):
    """The second of three views holds logits of +-80 (sums of up to four of them in 'sum_fg'): exp(l - max) underflows to 0 for the losing channels and the
    view votes one-hot (or splits evenly between channels that tie at the top); nothing overflows, no NaN appears - a NaN score would send the pixel to label 0 -
    and the float64 rule holds."""
    K, views = 9, ("id", "h", "v")
    _, scales = R.map_set(name)
    maps = R.random_maps(name, K, K, 3, N, seed=7000 + R.MODES[mode])          # (in float64 no pixel of these three cases lies within gap_cap of a tie)
    g = torch.Generator().manual_seed(7)
    for m in maps:
        m[N:2 * N] = (torch.randint(0, 2, m[N:2 * N].shape, generator=g).float() * 2 - 1) * 80.0
    um, us = _used(maps, scales, mode)
    _check64(um, us, mode, views, "prob", K, f"saturated {mode}")
    rc, got = _tta([m.to(dev) for m in um], us, mode, views, "prob", K)
    assert rc == 0 and len(torch.unique(got)) > 2


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_output_untouched():
    from pn2 import capi
    from pn2.core import _stream
    lib = capi.load()
    K = 9
    _, scales = R.map_set("a")
    dm = [m.to(dev) for m in R.random_maps("a", K, K, 3, N, seed=1)]
    out = torch.full((N, 32, 32), 0xAB, dtype=torch.uint8, device=dev)
    o, st = C.c_void_p(out.data_ptr()), _stream()

    def call(nmaps=4, mode=1, views=(0, 1, 2), V=None, average=1, K_=K, OW=32, maps=None):
        codes = (C.c_int * max(len(views), 1))(*views)
        return lib.pn2_seg_labels_up_tta(_table(maps or dm), nmaps, mode, codes, len(views) if V is None else V, average, N, K_, 32, OW, o, st)
    assert call(V=0) == -2 and call(views=(0, 1, 2, 3, 0)) == -2                                  # V outside 1..4
    assert call(views=(0, 4)) == -2 and call(views=(-1,)) == -2                                  # an unknown view code
    assert call(views=(1, 1)) == -2 and call(views=(0, 3, 2, 3)) == -2                           # a view twice
    assert call(average=2) == -2 and call(average=-1) == -2
    assert call(K_=1) == -2 and call(K_=17) == -2                                                # K outside 2..16 (17 is also > ld)
    assert call(K_=10) == -2                                                                     # ld < K
    assert call(mode=3) == -2 and call(mode=2, nmaps=3) == -2 and call(nmaps=0) == -2 and call(nmaps=9) == -2
    assert call(OW=64) == -2                                                                     # two scales
    src = torch.zeros(N, 4, 8, device=dev)
    dst = torch.full((3 * N, 4, 8), 5.0, device=dev)
    for views in ((0, 4), (2, 2), ()):
        codes = (C.c_int * max(len(views), 1))(*views)
        assert lib.pn2_flip_views(C.c_void_p(src.data_ptr()), N, 4, 8, codes, len(views), C.c_void_p(dst.data_ptr()), st) == -2
    torch.cuda.synchronize()
    assert bool((out == 0xAB).all()) and bool((dst == 5.0).all())
    assert call() == 0          # the base call itself is taken
    torch.cuda.synchronize()
    assert not bool((out == 0xAB).all())
