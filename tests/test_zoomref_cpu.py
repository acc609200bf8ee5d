"""tests/zoomref.py against live scipy.ndimage on the shapes the GPU tests use: every array bit for bit.  Also the committed fixture
tests/golden/synapse_zoom.npz against zoomref, so that the GPU tests (which never import scipy) compare with scipy's own outputs."""
import os

import numpy as np
import pytest

import zoomref as Z

HERE = os.path.dirname(os.path.abspath(__file__))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("src,dst", Z.SHAPES, ids=[Z.case_key(s, d) for s, d in Z.SHAPES])
def test_zoom_equals_scipy(src, dst):
    nd = pytest.importorskip("scipy.ndimage")
    img, lab = Z.case_input(src)
    fac = (dst[0] / src[0], dst[1] / src[1])
    want3, want0, want0f = nd.zoom(img, fac, order=3), nd.zoom(lab, fac, order=0), nd.zoom(img, fac, order=0)
    assert want3.shape == dst and want3.dtype == np.float32 and want0.dtype == np.uint8
    assert _same(Z.zoom3(img, *dst), want3)
    # the float32 cast hides a last-bit difference of the float64 arithmetic almost always, so the restatement is pinned before the cast as well
    assert np.array_equal(Z.prefilter(img), nd.spline_filter(img, 3, output=np.float64, mode="mirror"))
    assert np.array_equal(Z.zoom3_f64(img, *dst), nd.zoom(img, fac, order=3, output=np.float64))
    assert _same(Z.zoom0(lab, *dst), want0)
    assert _same(Z.zoom0(img, *dst), want0f)
    # the rows / columns scipy leaves at cval because (nout - 1) * ((nin - 1) / (nout - 1)) > nin - 1 in double
    assert (not want3[-1].any() and not want0[-1].any()) == ((src, dst) in Z.ZERO_LAST_ROW)
    assert (not want3[:, -1].any() and not want0[:, -1].any()) == ((src, dst) in Z.ZERO_LAST_COL)


@pytest.mark.parametrize("shape", Z.ROTATE_SHAPES + [(224, 224)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_rotate_equals_scipy(shape):
    nd = pytest.importorskip("scipy.ndimage")
    img, lab = Z.case_input(shape, seed=1)
    for angle in Z.ANGLES:
        assert _same(Z.rotate0(img, angle), nd.rotate(img, angle, order=0, reshape=False)), angle
        assert _same(Z.rotate0(lab, angle), nd.rotate(lab, angle, order=0, reshape=False)), angle
    assert _same(Z.rotate0(img, 0), img)


def test_rot_flip_and_random_generator_equal_the_loader():
    nd = pytest.importorskip("scipy.ndimage")
    draws = [("rot_flip", 1, 0), ("rotate", -13), None, ("rot_flip", 2, 1), ("rotate", 7), ("rot_flip", 3, 0)]
    imgs = np.stack([Z.case_input((40, 40), seed=i)[0] for i in range(6)])
    labs = np.stack([Z.case_input((40, 40), seed=i)[1] for i in range(6)])
    got = Z.random_generator(imgs, labs, (24, 24), draws)
    assert got["image"].shape == (6, 1, 24, 24) and got["image"].dtype == np.float32 and got["label"].shape == (6, 24, 24) and got["label"].dtype == np.int64
    for i, d in enumerate(draws):
        im, lb = imgs[i], labs[i]
        if d and d[0] == "rot_flip":          # dataset_synapse.py:12-19
            im, lb = np.flip(np.rot90(im, d[1]), axis=d[2]).copy(), np.flip(np.rot90(lb, d[1]), axis=d[2]).copy()
        elif d:          # :22-26
            im, lb = nd.rotate(im, d[1], order=0, reshape=False), nd.rotate(lb, d[1], order=0, reshape=False)
        im, lb = nd.zoom(im, (24 / 40, 24 / 40), order=3), nd.zoom(lb, (24 / 40, 24 / 40), order=0)
        assert _same(got["image"][i, 0], im.astype(np.float32)), i
        assert np.array_equal(got["label"][i], lb.astype(np.float32).astype(np.int64)), i


def test_fixture_holds_what_zoomref_computes():
    """The committed scipy outputs equal zoomref's on the same inputs (no scipy needed): the fixture and the restatement cannot drift apart unnoticed."""
    G = np.load(os.path.join(HERE, "golden", "synapse_zoom.npz"))
    for src, dst in Z.SHAPES:
        key = Z.case_key(src, dst)
        if key + "/out3" not in G:
            continue
        img, lab = Z.case_input(src)
        if key + "/img" in G:
            assert _same(G[key + "/img"], img) and _same(G[key + "/lab"], lab)
        assert _same(G[key + "/out3"], Z.zoom3(img, *dst)) and _same(G[key + "/out0"], Z.zoom0(lab, *dst)), key
    for shape in Z.ROTATE_SHAPES:
        img, lab = Z.case_input(shape, seed=1)
        key = f"rot{shape[0]}x{shape[1]}"
        assert _same(G[key + "/u8"], np.stack([Z.rotate0(lab, a) for a in Z.ANGLES]))
        if key + "/f32" in G:
            assert _same(G[key + "/f32"], np.stack([Z.rotate0(img, a) for a in Z.ANGLES]))
