"""CPU tests of flip test-time augmentation: tests/ttaref.py (the float64 restatement the GPU tests compare pn2_seg_labels_up_tta and the predictor with) against
torch's own interpolate / flip / softmax in float64; the share of near ties of every random case the GPU tests use; the parsing of the `tta` argument; and the
argument checks of the two entry points (the library loads without a GPU, the pointers are never dereferenced)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import ttaref as R

KS = [2, 4, 9]


def _used(maps, scales, mode):
    return (maps[-1:], scales[-1:]) if mode == "last" else (maps, scales)


@pytest.mark.parametrize("K", KS)
def test_reference_equals_torch_in_float64(K):
    """Per view F.interpolate(scale_factor=s, mode='bilinear', align_corners=False) of the float64 maps, torch.flip back, the combination of the mode, then the
    sum over the views of the logits or of torch.softmax: ttaref.scores agrees to 1e-12 (the two evaluate the same four-tap sums in float64 in another order)
    and picks the same labels wherever the top-two gap exceeds that.  N = 2, every map set, mode and view set of the GPU tests."""
    for name, mode in R.cases():
        _, scales = R.map_set(name)
        for views in R.VIEW_SETS:
            V = len(views)
            maps = R.random_maps(name, K, K, V, 2, R.seed_of(name, mode, K, views))
            um, us = _used(maps, scales, mode)
            for average in R.AVERAGES:
                tot = 0.0
                for v, view in enumerate(views):
                    ups = [F.interpolate(m[2 * v:2 * v + 2].double().permute(0, 3, 1, 2), scale_factor=s, mode="bilinear", align_corners=False) for m, s in zip(um, us)]
                    dims = [d for d, bit in ((3, 1), (2, 2)) if R.VIEWS[view] & bit]
                    ups = [torch.flip(u, dims) if dims else u for u in ups]
                    if mode == "last":
                        x = ups[-1]
                    elif mode == "sum_fg":
                        x = sum(ups[1:], ups[0])
                    else:
                        h = len(ups) // 2
                        x = sum((p - q for p, q in zip(ups[1:h], ups[h + 1:])), ups[0] - ups[h])
                    tot = tot + (torch.softmax(x, dim=1) if average == "prob" else x)
                want = tot.permute(0, 2, 3, 1)
                got = R.scores(um, us, mode, views, average, K)
                assert got.shape == want.shape and got.dtype == torch.float64
                assert float((got - want).abs().max()) <= 1e-12, (name, mode, views, average)
                clear = R.gap(want) > 1e-11
                assert torch.equal(R.labels(got)[clear], torch.argmax(want, dim=-1).to(torch.uint8)[clear])


def test_views_are_told_apart_and_the_sum_is_not_a_mean():
    """A map that is 1 in the top-left pixel: the 'h' view's contribution lands top-right, 'v' bottom-left, 'hv' bottom-right; 'prob' scores of V views sum to V."""
    m = torch.zeros(4, 2, 2, 2)
    m[:, 0, 0, 1] = 8.0
    sc = R.scores([m], [2], "last", ("id", "h", "v", "hv"), "logit", 2)
    assert sc.shape == (1, 4, 4, 2)
    assert float(sc[0, 0, 0, 1]) == float(sc[0, 0, 3, 1]) == float(sc[0, 3, 0, 1]) == float(sc[0, 3, 3, 1]) == 8.0
    for view, (y, x) in zip(("id", "h", "v", "hv"), ((0, 0), (0, 3), (3, 0), (3, 3))):
        one = R.scores([m[:1]], [2], "last", (view,), "logit", 2)
        assert float(one[0, y, x, 1]) == 8.0 and float(one[0, 3 - y, 3 - x, 1]) == 0.0, view
    pr = R.scores([m], [2], "last", ("id", "h", "v", "hv"), "prob", 2)
    assert float((pr.sum(-1) - 4.0).abs().max()) < 1e-12
    assert R.deficit(sc, R.labels(sc)).abs().max() == 0 and float(R.deficit(sc, torch.zeros(1, 4, 4))[0, 0, 0]) == 8.0


@pytest.mark.parametrize("K", KS)
def test_random_cases_stay_clear_of_ties_in_float64(K):
    """The condition of the GPU tests, on the CPU with their seeds: in every random case at most MAX_EXCUSED = 0.5 % of the pixels have a float64 top-two gap
    below ttaref.gap_cap (which bounds, from the number formats, the threshold the GPU tests measure).  See the note at ttaref.SCALE for how the scale was set."""
    worst = 0.0
    for name, mode in R.cases():
        _, scales = R.map_set(name)
        for views in R.VIEW_SETS:
            maps = R.random_maps(name, K, K, len(views), 2, R.seed_of(name, mode, K, views))
            um, us = _used(maps, scales, mode)
            maxabs = max(float(m.abs().max()) for m in um)
            for average in R.AVERAGES:
                sc = R.scores(um, us, mode, views, average, K)
                share = float((R.gap(sc) < R.gap_cap(mode, average, len(um), len(views), maxabs)).double().mean())
                worst = max(worst, share)
                assert share <= R.MAX_EXCUSED, (name, mode, views, average, share)
    print(f"\nK {K}: largest share of near ties {worst:.2e}")


def test_tta_argument_parsing():
    from pn2 import voleval as V
    assert V.VIEWS == R.VIEWS and V.AVERAGES == R.AVERAGES and V.MODES == R.MODES
    assert V.parse_tta(None) is None
    assert V.parse_tta("flips") == ("id", "h", "v")
    assert V.parse_tta(("hv", "id")) == ("hv", "id") and V.parse_tta(["v"]) == ("v",)
    assert V.parse_tta(("id", "h", "v", "hv")) == ("id", "h", "v", "hv")
    for bad in ("flip", "id", (), ("id", "x"), ("id", 1), 3, ("id", "h", "v", "hv", "id"), {"id"}):
        with pytest.raises(ValueError):
            V.parse_tta(bad)
    with pytest.raises(ValueError, match="twice"):
        V.parse_tta(("h", "id", "h"))


def test_volume_predictor_takes_and_refuses_tta_arguments():
    """The constructor parses before anything touches a device."""
    from pn2.infer import VolumePredictor

    class Net(torch.nn.Module):
        def _build_lowres(self, eng, x):
            raise AssertionError("not reached")
    assert VolumePredictor(Net(), (64, 64), 2).views is None
    vp = VolumePredictor(Net(), (64, 64), 2, tta="flips")
    assert vp.views == ("id", "h", "v") and vp.tta_average == "prob"
    assert VolumePredictor(Net(), (64, 64), 2, tta=("hv", "id"), tta_average="logit").views == ("hv", "id")
    with pytest.raises(ValueError):
        VolumePredictor(Net(), (64, 64), 2, tta="rot90")
    with pytest.raises(ValueError):
        VolumePredictor(Net(), (64, 64), 2, tta=("h", "h"))
    with pytest.raises(ValueError):
        VolumePredictor(Net(), (64, 64), 2, tta="flips", tta_average="mean")


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """-1 for a null pointer or an empty size, -2 outside the built range: every call fails its argument check, which comes before the first HIP call."""
    from pn2 import capi
    lib = capi.load()
    one = C.c_void_p(256)

    def maps(ld=16, p=256):
        arr = (capi.SegUpMap * 8)()
        for i, (h, w) in enumerate([(2, 2), (4, 4), (8, 8), (16, 16)] * 2):
            arr[i].p, arr[i].ld, arr[i].H, arr[i].W = p, ld, h, w
        return arr

    def codes(*v):
        return (C.c_int * max(len(v), 1))(*v)
    tta = lib.pn2_seg_labels_up_tta
    ok = codes(0, 1, 2)
    assert tta(None, 4, 1, ok, 3, 1, 2, 9, 64, 64, one, None) == -1
    assert tta(maps(), 4, 1, None, 3, 1, 2, 9, 64, 64, one, None) == -1
    assert tta(maps(), 4, 1, ok, 3, 1, 2, 9, 64, 64, None, None) == -1
    assert tta(maps(p=None), 4, 1, ok, 3, 1, 2, 9, 64, 64, one, None) == -1
    assert tta(maps(), 4, 1, ok, 3, 1, 0, 9, 64, 64, one, None) == -1
    assert tta(maps(), 4, 1, ok, 0, 1, 2, 9, 64, 64, one, None) == -2 and tta(maps(), 4, 1, codes(0, 1, 2, 3, 0), 5, 1, 2, 9, 64, 64, one, None) == -2          # V outside 1..4
    assert tta(maps(), 4, 1, codes(0, 4), 2, 1, 2, 9, 64, 64, one, None) == -2 and tta(maps(), 4, 1, codes(-1), 1, 1, 2, 9, 64, 64, one, None) == -2          # unknown code
    assert tta(maps(), 4, 1, codes(1, 0, 1), 3, 1, 2, 9, 64, 64, one, None) == -2          # a view twice
    assert tta(maps(), 4, 1, ok, 3, 2, 2, 9, 64, 64, one, None) == -2 and tta(maps(), 4, 1, ok, 3, -1, 2, 9, 64, 64, one, None) == -2          # unknown average
    assert tta(maps(), 4, 1, ok, 3, 1, 2, 1, 64, 64, one, None) == -2 and tta(maps(), 4, 1, ok, 3, 1, 2, 17, 64, 64, one, None) == -2          # K outside 2..16
    assert tta(maps(), 3, 2, ok, 3, 1, 2, 9, 64, 64, one, None) == -2 and tta(maps(), 4, 3, ok, 3, 1, 2, 9, 64, 64, one, None) == -2          # odd maps in mode 2, unknown mode
    assert tta(maps(ld=8), 4, 1, ok, 3, 1, 2, 9, 64, 64, one, None) == -2 and tta(maps(), 4, 1, ok, 3, 1, 2, 9, 64, 96, one, None) == -2          # ld < K, two scales
    assert tta(maps(), 4, 1, ok, 3, 1, 65536, 9, 64, 64, one, None) == -2          # the batch is a grid axis
    flip = lib.pn2_flip_views
    assert flip(None, 2, 8, 8, ok, 3, one, None) == -1 and flip(one, 2, 8, 8, None, 3, one, None) == -1 and flip(one, 2, 8, 8, ok, 3, None, None) == -1
    assert flip(one, 0, 8, 8, ok, 3, one, None) == -1 and flip(one, 2, 0, 8, ok, 3, one, None) == -1 and flip(one, 2, 8, 0, ok, 3, one, None) == -1
    assert flip(one, 2, 8, 8, ok, 0, one, None) == -2 and flip(one, 2, 8, 8, codes(0, 1, 2, 3, 0), 5, one, None) == -2
    assert flip(one, 2, 8, 8, codes(0, 5), 2, one, None) == -2 and flip(one, 2, 8, 8, codes(2, 2), 2, one, None) == -2
