"""The CPU restatement of the reference's volume metrics (tests/volevalref.py) on cases computable by hand, the host half of pn2.voleval (percentile and
means from d^2 histograms) against numpy on the distances themselves, and the argument checks of the pn2_seg_* entry points that need no GPU."""
import ctypes as C

import numpy as np
import torch

import volevalref as V


def _vol(shape, *voxels):
    m = np.zeros(shape, dtype=bool)
    for v in voxels:
        m[v] = True
    return m


def test_two_single_voxels_at_offset_1_2_2():
    """|(1, 2, 2)| = 3: every surface distance is 3 in both directions."""
    a, b = _vol((4, 5, 6), (1, 1, 1)), _vol((4, 5, 6), (2, 3, 3))
    assert V.surface_distances(a, b).tolist() == [3.0] and V.surface_distances(b, a).tolist() == [3.0]
    assert V.hd95(a, b) == 3.0 and V.assd(a, b) == 3.0
    assert V.calculate_metric_percase(a, b) == (0.0, 3.0, 0.0, 3.0)
    assert V.d2_histogram(a, b, 50).tolist() == [0] * 9 + [1] + [0] * 40


def test_two_identical_cubes():
    a = np.zeros((6, 7, 8), dtype=bool)
    a[1:5, 2:6, 2:6] = True
    assert V.calculate_metric_percase(a, a.copy()) == (1.0, 0.0, 1.0, 0.0)
    assert int(V.border(a).sum()) == 4 ** 3 - 2 ** 3          # a 4^3 cube's shell


def test_cube_against_its_centre_voxel():
    """A 3^3 cube (border: its 26 shell voxels) against its centre (border: itself).  cube -> centre: 6 faces at 1, 12 edges at sqrt 2, 8 corners at sqrt 3;
    centre -> cube: one distance of 1."""
    a = np.zeros((5, 5, 5), dtype=bool)
    a[1:4, 1:4, 1:4] = True
    b = _vol((5, 5, 5), (2, 2, 2))
    assert int(V.border(a).sum()) == 26 and not V.border(a)[2, 2, 2]
    assert V.d2_histogram(a, b, 4).tolist() == [0, 6, 12, 8] and V.d2_histogram(b, a, 4).tolist() == [0, 1, 0, 0]
    allv = np.sort(np.array([1.0] * 7 + [2 ** 0.5] * 12 + [3 ** 0.5] * 8))
    dice, hd, jac, asd = V.calculate_metric_percase(a, b)
    assert dice == 2 / 28 and jac == 1 / 27
    assert hd == np.percentile(allv, 95) == 3 ** 0.5          # index 0.95 * 26 = 24.7 lies among the eight corners
    assert abs(asd - ((6 + 12 * 2 ** 0.5 + 8 * 3 ** 0.5) / 26 + 1.0) / 2) < 1e-15


def test_special_case_returns():
    a, empty = _vol((3, 4, 5), (1, 1, 1)), np.zeros((3, 4, 5), dtype=bool)
    assert V.calculate_metric_percase(a, empty) == (1, 0, 1, 0) and V.calculate_dice_percase(a, empty) == 1
    assert V.calculate_metric_percase(empty, a) == (0, 0, 0, 0) and V.calculate_dice_percase(empty, a) == 0
    assert V.calculate_metric_percase(empty, empty) == (0, 0, 0, 0) and V.calculate_dice_percase(empty, empty) == 0
    lab = np.zeros((3, 4, 5), dtype=np.uint8)
    lab[1, 1, 1] = 2
    assert V.volume_metrics(lab, np.zeros_like(lab), 3) == [(0, 0, 0, 0), (1, 0, 1, 0)]
    assert V.volume_dice(lab, lab, 3) == [0, 1.0]


def test_two_dimensional_input_uses_the_four_neighbour_border():
    """A 3 x 3 square in 2-D: the centre has its four face neighbours inside, so the border is the ring of 8 (as a one-slice 3-D volume every voxel would be border)."""
    a = np.zeros((5, 6), dtype=bool)
    a[1:4, 1:4] = True
    assert int(V.border(a).sum()) == 8 and not V.border(a)[2, 2]
    assert int(V.border(a[None]).sum()) == 9
    b = _vol((5, 6), (2, 5))
    # ring -> (2, 5): columns 1, 2, 3 at dx = 4, 3, 2 and dy = -1, 0, 1 (the centre (2, 2) is not border)
    want = sorted([17, 16, 17, 10, 10, 5, 4, 5])
    assert sorted(np.rint(V.surface_distances(a, b) ** 2).astype(int).tolist()) == want
    assert V.surface_distances(b, a).tolist() == [2.0]


def test_label_combination_order_and_ties():
    g = np.random.default_rng(0)
    outs = [(g.integers(-80, 80, (2, 5, 4, 6)) / 8).astype(np.float32) for _ in range(8)]
    s = V.combine(outs[:4], "sum_fg")
    assert s.dtype == np.float32 and np.array_equal(s, ((outs[0] + outs[1]) + outs[2]) + outs[3])
    d = V.combine(outs, "sum_fg_minus_bg")
    assert np.array_equal(d, (((outs[0] - outs[4]) + (outs[1] - outs[5])) + (outs[2] - outs[6])) + (outs[3] - outs[7]))
    assert V.combine(outs, "last") is outs[-1]
    tie = np.zeros((1, 3, 1, 2), dtype=np.float32)
    tie[0, 1:, 0, 0] = 1.0
    assert V.labels([tie], "last").tolist() == [[[1, 0]]] and V.labels([tie], "last", softmax=False).tolist() == [[[1, 0]]]


def test_host_finish_from_histograms_matches_numpy_on_the_distances():
    """pn2.voleval._hd95_asd (percentile through cumulative counts, means through count x value) against numpy.percentile / mean on the expanded distances."""
    from pn2.voleval import _hd95_asd
    g = np.random.default_rng(5)
    for n1, n2, top in ((1, 1, 3), (7, 20, 40), (1000, 333, 5000), (20, 1, 2)):
        h1 = np.bincount(g.integers(0, top, n1), minlength=top).astype(np.int64)
        h2 = np.bincount(g.integers(0, top, n2), minlength=top).astype(np.int64)
        d1, d2 = np.sqrt(np.repeat(np.arange(top), h1).astype(np.float64)), np.sqrt(np.repeat(np.arange(top), h2).astype(np.float64))
        hd, asd = _hd95_asd(h1, h2)
        want_hd, want_asd = np.percentile(np.hstack((d1, d2)), 95), np.mean((d1.mean(), d2.mean()))
        assert abs(hd - want_hd) <= 1e-12 * max(want_hd, 1) and abs(asd - want_asd) <= 1e-12 * max(want_asd, 1)


def test_single_forward_restatement_reproduces_the_reference_fixture():
    """volevalref.emcadnet_single_forward in train mode against the recorded outputs of the reference model (tests/golden/emcad_single_64.npz, fp32 run)."""
    import seglossref as R
    from oracle import weights as W
    z = R.load_fixture()
    P = W.make_state_dict(R.single_manifest(9), seed=5)
    with torch.no_grad():
        outs = V.emcadnet_single_forward(P, torch.from_numpy(z["x"]), training=True)
    for o, r in zip(outs, R.fixture_outs(z, "")):
        assert tuple(o.shape) == tuple(r.shape)
        assert float((o - r).abs().max()) <= 1e-4 * max(1.0, float(r.abs().max()))


def test_seg_entry_points_refuse_bad_arguments_before_any_launch():
    """Status codes of the pn2_seg_* entries on bad arguments: they come back before the first HIP call, so this needs the library but no GPU."""
    from pn2 import capi
    lib = capi.load()
    one = C.c_void_p(8)          # never dereferenced: every call below fails its argument check
    maps = (C.c_void_p * 8)(*[8] * 8)
    assert lib.pn2_seg_labels(maps, 4, 1, 1, 1, 4, 4, one, None) == -2          # K < 2
    assert lib.pn2_seg_labels(maps, 4, 1, 1, 17, 4, 4, one, None) == -2         # K > 16
    assert lib.pn2_seg_labels(maps, 9, 1, 1, 9, 4, 4, one, None) == -2          # more than eight maps
    assert lib.pn2_seg_labels(maps, 3, 2, 1, 9, 4, 4, one, None) == -2          # odd number of maps for fg - bg
    assert lib.pn2_seg_labels(maps, 4, 3, 1, 9, 4, 4, one, None) == -2          # unknown mode
    assert lib.pn2_seg_labels(None, 4, 1, 1, 9, 4, 4, one, None) == -1
    assert lib.pn2_seg_counts(one, one, 16, 0, one, None) == -2 and lib.pn2_seg_counts(one, one, 16, 257, one, None) == -2
    assert lib.pn2_seg_counts(None, one, 16, 9, one, None) == -1
    nbytes = C.c_longlong(-7)
    assert lib.pn2_seg_surface_workspace(1, 1, 1025, 3, C.byref(nbytes)) == -2 and nbytes.value == -7
    assert lib.pn2_seg_surface_workspace(2, 8, 8, 2, C.byref(nbytes)) == -2          # ndim 2 means one slice
    assert lib.pn2_seg_surface_workspace(5, 37, 70, 3, C.byref(nbytes)) == 0 and nbytes.value == 64 + 2 * 4 * 5 * 37 * 70
    assert lib.pn2_seg_surface_hist_len(5, 37, 70) == 16 + 36 * 36 + 69 * 69 + 1 and lib.pn2_seg_surface_hist_len(1025, 1, 1) == -1
    assert lib.pn2_seg_surface_hist(one, one, 1, 1, 1025, 1, 3, one, one, one, None) == -2
    assert lib.pn2_seg_surface_hist(one, one, 1, 8, 8, 1, 4, one, one, one, None) == -2
    assert lib.pn2_seg_surface_hist(one, None, 1, 8, 8, 1, 2, one, one, one, None) == -1
