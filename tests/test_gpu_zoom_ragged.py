"""GPU tests of the ragged entry points of pn2/volinput.py (the pn2_ragged_* half of csrc/pn2_zoom.hip) against tests/raggedref.py and numpy's / scipy's own outputs in
tests/golden/acdc_ragged.npz - never against live scipy.  Every comparison is array_equal on the raw bits."""
import os
import random

import numpy as np
import pytest
import torch

import raggedref as R
import zoomref as Z

pytestmark = pytest.mark.gpu
os.environ.setdefault("PN2_NO_PRETRAINED", "1")
dev = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = list(R.BATCHES) + ["one"]
_WANT = {}


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pn2
    pn2.load_library()
    yield


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "acdc_ragged.npz"))


def _case(name):
    """(images, labels, draws, size, what raggedref collates), computed once per case and left unchanged."""
    if name not in _WANT:
        images, labels, draws, size = R.batch_inputs(R.ONE if name == "one" else name)
        _WANT[name] = (images, labels, draws, size, R.random_generator(images, labels, size, draws))
    return _WANT[name]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _report(name, got, want):
    g = got.cpu().numpy()
    bad = np.nonzero((_bits(g) != _bits(want)).reshape(len(g), -1).any(1))[0]
    print(f"\n{name}: {len(bad)} of {len(g)} samples differ {bad.tolist()}, max |diff| {float(np.abs(g.astype(np.float64) - want).max()):.3e}")


# ------------------------------------------------------------------------------------------------ the training batch
@pytest.mark.parametrize("name", CASES)
def test_ragged_transform_equals_the_loader_bit_for_bit(name, golden):
    from pn2.volinput import RaggedSliceTransform
    images, labels, draws, size, want = _case(name)
    t = RaggedSliceTransform(size)
    got = t(images, labels, draws)          # host arrays in
    _report(name, got["image"], want["image"])
    assert tuple(got["image"].shape) == (len(images), 1) + size and got["image"].is_contiguous() and got["label"].dtype == torch.int64
    assert _same(got["image"], want["image"]) and _same(got["label"], want["label"])
    if name + "/image" in golden:          # scipy's own arrays
        assert _same(got["image"][:, 0], golden[name + "/image"]) and _same(got["label"].to(torch.uint8), golden[name + "/label"])
    ondev = t([_d(a) for a in images], [_d(a) for a in labels], draws)          # device tensors in, each an allocation of its own
    assert torch.equal(ondev["image"], got["image"]) and torch.equal(ondev["label"], got["label"])
    for i, (im, d) in enumerate(zip(images, draws)):          # a sample at the output size after its geometry is the geometry of its raw bits: no spline pass
        if d is None and im.shape == size:
            assert _same(got["image"][i, 0], im)


def test_the_edges_batch_holds_what_it_is_for():
    """The plan of the 'edges' batch: tiles of 63 / 64 / 65 columns and 31 / 32 / 33 / 65 rows on both prefilter axes, all eight rot_flip forms on non-square samples,
    the loader's extreme angles, axes of length 1 and 2, copies with and without a geometry, and a copy that only the odd-k swap makes one."""
    from pn2 import volinput as V
    images, _, draws, size, _ = _case("edges")
    plan = V.RaggedPlan(V.ragged_samples([im.shape for im in images], size, draws))
    ds = list(plan.descs)
    assert {63, 64, 65} <= {d.gw for d in ds} and {31, 32, 33, 65} <= {d.gh for d in ds} and {1, 2} <= {min(d.gh, d.gw) for d in ds}
    assert {(d.k, d.axis) for d in ds if d.geom == 1 and d.H != d.W and not d.copy} >= {(k, a) for k in range(4) for a in (0, 1)}
    assert {dr[1] for dr in draws if dr and dr[0] == "rotate"} >= {-20, -1, 0, 19}
    assert {d.geom for d in ds if d.copy} == {0, 1, 2} and any(d.copy and (d.H, d.W) != size for d in ds) and any((d.H, d.W) == size[::-1] and not d.copy for d in ds)
    assert plan.header.blocks0 > len(ds) - sum(d.copy for d in ds)          # more than one block per sample somewhere


def test_permuted_batch_gives_permuted_outputs_and_other_stream():
    from pn2.volinput import RaggedSliceTransform
    images, labels, draws, size, want = _case("edges")
    perm = np.random.default_rng(5).permutation(len(images)).tolist()
    t = RaggedSliceTransform(size)
    got = t([images[i] for i in perm], [labels[i] for i in perm], [draws[i] for i in perm])
    assert _same(got["image"], want["image"][perm]) and _same(got["label"], want["label"][perm])
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        other = t(images, labels, draws)
    s.synchronize()
    assert _same(other["image"], want["image"]) and _same(other["label"], want["label"])


def test_uniform_square_batch_equals_slice_transform():
    from pn2.volinput import RaggedSliceTransform, SliceTransform
    imgs = np.stack([Z.case_input((40, 40), seed=i)[0] for i in range(6)])
    labs = np.stack([Z.case_input((40, 40), seed=i)[1] for i in range(6)])
    random.seed(1); np.random.seed(1)
    draws = SliceTransform.draw(6)
    assert {None if d is None else d[0] for d in draws} == {None, "rot_flip", "rotate"}
    want = SliceTransform((24, 24))(_d(imgs), _d(labs), draws)
    got = RaggedSliceTransform((24, 24))(list(_d(imgs)), list(_d(labs)), draws)          # views of one allocation
    assert torch.equal(got["image"], want["image"]) and torch.equal(got["label"], want["label"])
    random.seed(1); np.random.seed(1)
    again = RaggedSliceTransform((24, 24))(list(imgs), list(labs))          # draws omitted: SliceTransform.draw's, from the seeded generators
    assert torch.equal(again["image"], want["image"]) and torch.equal(again["label"], want["label"])


# ------------------------------------------------------------------------------------------------ val(): zoom in, zoom back, Dice
def test_zoom_ragged_both_orders():
    from pn2 import volinput as V
    for name in ("zero_row", "zero_col"):
        images, labels, _, size, _ = _case(name)
        assert _same(V.zoom_ragged(images, size, 3), R.zoom_ragged(images, size, 3)) and _same(V.zoom_ragged(labels, size, 0), R.zoom_ragged(labels, size, 0))
        assert _same(V.zoom_ragged([_d(a) for a in images], size, 3), R.zoom_ragged(images, size, 3))
    images, labels, _, size, _ = _case("zero_row")
    for i, im in enumerate(images):          # the uniform entry point, sample by sample
        assert torch.equal(V.zoom_ragged([im], size, 3)[0], V.zoom(_d(im), size, 3))
        assert torch.equal(V.zoom_ragged([labels[i]], size, 0)[0], V.zoom(_d(labels[i]), size, 0))


def test_unzoom_labels_equals_zoom0_per_sample(golden):
    from pn2 import volinput as V
    maps, sizes = R.unzoom_inputs()
    views = V.unzoom_labels(_d(maps), sizes)
    assert [tuple(v.shape) for v in views] == sizes and all(v.dtype == torch.uint8 for v in views)
    assert views[0].untyped_storage().data_ptr() == views[-1].untyped_storage().data_ptr()          # one packed buffer
    for i, (v, m, s) in enumerate(zip(views, maps, sizes)):
        assert _same(v, m if m.shape == s else Z.zoom0(m, *s)) and _same(v, golden[f"unzoom/{i}"]), i
    one = V.unzoom_labels(_d(maps[:1]), sizes[:1])
    assert len(one) == 1 and torch.equal(one[0], views[0])


def test_dice_counts_equal_numpy():
    from pn2 import volinput as V
    g = np.random.default_rng(9)
    sizes = [(65, 63), (1, 37), (5, 7), (33, 65), (2, 5), (300, 257)]
    preds = [g.integers(0, 4, s).astype(np.uint8) for s in sizes]
    gts = [g.integers(0, 4, s).astype(np.uint8) for s in sizes]
    preds[2][:], gts[2][:] = 0, 0          # an empty prediction with an empty label
    preds[3][:] = 0                         # an empty prediction alone
    gts[4][:] = 3
    got = V.dice_counts(_d(np.concatenate([p.ravel() for p in preds])), _d(np.concatenate([q.ravel() for q in gts])), sizes)
    want = np.array([R.dice_counts(p, q) for p, q in zip(preds, gts)], np.int64)
    assert got.dtype == np.int64 and np.array_equal(got, want) and got[2].tolist() == [0, 0, 0] and got[3, 1] == 0 and got[4, 2] == 10


# ------------------------------------------------------------------------------------------------ errors
def test_errors():
    from pn2 import volinput as V
    f, u = np.zeros((8, 9), np.float32), np.zeros((8, 9), np.uint8)
    t = V.RaggedSliceTransform((4, 4))
    with pytest.raises((ValueError, RuntimeError)):
        t([f], [u, u], [None])
    with pytest.raises((ValueError, RuntimeError)):
        t([f], [np.zeros((9, 8), np.uint8)], [None])          # a label of another shape
    with pytest.raises((ValueError, RuntimeError)):
        t([f], [_d(u)], [None])          # one on the host, one on the device
    with pytest.raises((ValueError, RuntimeError)):
        t([u], [u], [None])          # images are fp32
    with pytest.raises((ValueError, RuntimeError), match="1024"):
        V.zoom_ragged([np.zeros((2, 1025), np.float32)], (4, 4), 3)
    with pytest.raises((ValueError, RuntimeError), match="1024"):
        V.zoom_ragged([f], (1025, 4), 3)
    with pytest.raises((ValueError, RuntimeError)):
        V.zoom_ragged([], (4, 4), 3)
    with pytest.raises((ValueError, RuntimeError)):
        V.unzoom_labels(_d(np.zeros((2, 4, 4), np.uint8)), [(8, 9)])
    with pytest.raises((ValueError, RuntimeError)):
        V.dice_counts(_d(np.zeros(10, np.uint8)), _d(np.zeros(10, np.uint8)), [(2, 2)])
