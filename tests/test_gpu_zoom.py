"""GPU tests of the Synapse slice transform (pn2/volinput.py on csrc/pn2_zoom.hip) against tests/zoomref.py and scipy's own outputs in
tests/golden/synapse_zoom.npz - never against live scipy.  Every comparison is array_equal on the raw bits."""
import os
import random
import sys

import numpy as np
import pytest
import torch

import zoomref as Z

pytestmark = pytest.mark.gpu
os.environ.setdefault("PN2_NO_PRETRAINED", "1")
dev = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pn2
    pn2.load_library()
    yield
    pn2.set_compute_dtype("bf16")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "synapse_zoom.npz"))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------------------------------------ zoom
@pytest.mark.parametrize("src,dst", Z.SHAPES, ids=[Z.case_key(s, d) for s, d in Z.SHAPES])
def test_zoom_equals_scipy_bit_for_bit(src, dst, golden):
    from pn2 import volinput as V
    img, lab = Z.case_input(src)
    got3, got0, got0f = V.zoom(_d(img), dst, 3), V.zoom(_d(lab), dst, 0), V.zoom(_d(img), dst, 0)
    got0l = V.zoom(_d(lab).long(), dst, 0)
    want3, want0 = Z.zoom3(img, *dst), Z.zoom0(lab, *dst)
    bad = int((_bits(got3.cpu().numpy()) != _bits(want3)).sum())
    print(f"\n{Z.case_key(src, dst)}: order 3 differs in {bad} of {want3.size} values, max |diff| {float(np.abs(got3.cpu().numpy().astype(np.float64) - want3).max()):.3e}")
    assert _same(got3, want3) and _same(got0, want0) and _same(got0f, Z.zoom0(img, *dst))
    assert got0l.dtype == torch.int64 and np.array_equal(got0l.cpu().numpy(), want0.astype(np.int64))
    key = Z.case_key(src, dst)
    if key + "/out3" in golden:          # scipy's own arrays
        assert _same(got3, golden[key + "/out3"]) and _same(got0, golden[key + "/out0"])
    for got in (got3, got0):
        g = got.cpu().numpy()
        assert (not g[-1].any()) == ((src, dst) in Z.ZERO_LAST_ROW) and (not g[:, -1].any()) == ((src, dst) in Z.ZERO_LAST_COL)
        assert g[:-1, :-1].any()


def test_batch_equals_single_calls_and_other_stream():
    from pn2 import volinput as V
    src, dst = (33, 17), (16, 40)
    imgs = np.stack([Z.case_input(src, seed=i)[0] for i in range(3)])
    labs = np.stack([Z.case_input(src, seed=i)[1] for i in range(3)])
    b3, b0 = V.zoom(_d(imgs), dst, 3), V.zoom(_d(labs), dst, 0)
    assert tuple(b3.shape) == (3,) + dst and tuple(b0.shape) == (3,) + dst
    for i in range(3):
        assert torch.equal(b3[i], V.zoom(_d(imgs[i]), dst, 3)) and torch.equal(b0[i], V.zoom(_d(labs[i]), dst, 0))
        assert _same(b3[i], Z.zoom3(imgs[i], *dst)) and _same(b0[i], Z.zoom0(labs[i], *dst))
    x, l = _d(imgs), _d(labs)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        s3, s0 = V.zoom(x, dst, 3), V.zoom(l, dst, 0)
    s.synchronize()
    assert torch.equal(s3, b3) and torch.equal(s0, b0)
    same = V.zoom(x, src, 3)
    assert same is x          # equal sizes: the reference skips the call


# ------------------------------------------------------------------------------------------------ rotate, rot90 + flip
@pytest.mark.parametrize("shape", Z.ROTATE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rotate_every_angle_of_the_loader(shape, golden):
    from pn2 import volinput as V
    img, lab = Z.case_input(shape, seed=1)
    n = len(Z.ANGLES)
    gotf = V.rotate(_d(np.broadcast_to(img, (n,) + shape)), Z.ANGLES)
    gotu = V.rotate(_d(np.broadcast_to(lab, (n,) + shape)), Z.ANGLES)
    assert _same(gotf, np.stack([Z.rotate0(img, a) for a in Z.ANGLES])) and _same(gotu, np.stack([Z.rotate0(lab, a) for a in Z.ANGLES]))
    key = f"rot{shape[0]}x{shape[1]}"
    assert _same(gotu, golden[key + "/u8"])
    if key + "/f32" in golden:
        assert _same(gotf, golden[key + "/f32"])
    assert _same(gotf[Z.ANGLES.index(0)], img)          # angle 0 is a plain copy
    assert _same(V.rotate(_d(lab), -7), Z.rotate0(lab, -7))


def test_rot_flip_all_eight():
    from pn2 import volinput as V
    img, lab = Z.case_input((16, 16), seed=2)
    ks, axes = [k for k in range(4) for _ in range(2)], [0, 1] * 4
    gotf, gotu = V.rot_flip(_d(np.broadcast_to(img, (8, 16, 16))), ks, axes), V.rot_flip(_d(np.broadcast_to(lab, (8, 16, 16))), ks, axes)
    assert _same(gotf, np.stack([Z.rot_flip(img, k, a) for k, a in zip(ks, axes)])) and _same(gotu, np.stack([Z.rot_flip(lab, k, a) for k, a in zip(ks, axes)]))
    # a flip after a quarter turn is one of the square's four reflections, and flip(1) after k turns is flip(0) after k + 2: four distinct arrays, each twice
    assert len({gotu[i].cpu().numpy().tobytes() for i in range(8)}) == 4 and not any(_same(gotu[i], lab) for i in range(8))
    assert _same(V.rot_flip(_d(img), 0, None), img)


# ------------------------------------------------------------------------------------------------ SliceTransform
def test_slice_transform_equals_random_generator():
    from pn2.volinput import SliceTransform
    imgs = np.stack([Z.case_input((40, 40), seed=i)[0] for i in range(6)])
    labs = np.stack([Z.case_input((40, 40), seed=i)[1] for i in range(6)])
    random.seed(1); np.random.seed(1)
    draws = SliceTransform.draw(6)
    random.seed(1); np.random.seed(1)
    want_draws = []
    for _ in range(6):          # the reference's calls in the reference's order (dataset_synapse.py:13,16,23,35-38)
        if random.random() > 0.5:
            k = np.random.randint(0, 4)
            want_draws.append(("rot_flip", k, np.random.randint(0, 2)))
        elif random.random() > 0.5:
            want_draws.append(("rotate", np.random.randint(-20, 20)))
        else:
            want_draws.append(None)
    assert draws == want_draws
    kinds = {None if d is None else d[0] for d in draws}
    assert kinds == {None, "rot_flip", "rotate"}, draws          # the seed covers all three branches
    t = SliceTransform((24, 24))
    got = t(_d(imgs), _d(labs), draws)
    want = Z.random_generator(imgs, labs, (24, 24), draws)
    assert tuple(got["image"].shape) == (6, 1, 24, 24) and got["label"].dtype == torch.int64
    assert _same(got["image"], want["image"]) and _same(got["label"], want["label"])
    random.seed(1); np.random.seed(1)
    again = t(_d(imgs), _d(labs))          # draws omitted: drawn on the host from the seeded generators
    assert torch.equal(again["image"], got["image"]) and torch.equal(again["label"], got["label"])
    with pytest.raises(ValueError):
        t(_d(imgs[:, :, :32]), _d(labs[:, :, :32]))


# ------------------------------------------------------------------------------------------------ volume evaluation
class _Spy:
    """The net with its inputs and outputs recorded."""

    def __init__(self, net):
        self.net, self.inputs, self.outs = net, [], []

    def eval(self):
        self.net.eval()
        return self

    def __call__(self, x):
        self.inputs.append(x.clone())
        self.outs.append(self.net(x))
        return self.outs[-1]


def _eval_model():
    """The single-supervision EMCADNet(K = 9, pvt_v2_b2) of tests/test_gpu_voleval.py: weights of the train-mode tests, non-trivial BatchNorm statistics, eval, fp32."""
    import pn2
    import seglossref as S
    import volevalref as R
    from lib.networks import EMCADNet
    from oracle import weights as W
    pn2.set_compute_dtype("fp32")
    m = EMCADNet(num_classes=9, kernel_sizes=[1, 3, 5], expansion_factor=2, dw_parallel=True, add=True, lgag_ks=3, activation="relu6", encoder="pvt_v2_b2",
                 pretrain=False, dual=False)
    m.load_state_dict(R.nontrivial_bn_stats(W.make_state_dict(S.single_manifest(9), seed=5), seed=17), strict=True)
    m.backbone.reset_drop_path(0.0)
    return m.to(dev).eval()


def test_volume_evaluation_resamples_on_the_device(monkeypatch):
    """3 x 96 x 80 volume, patch_size 64 x 64, scipy unimportable: the net sees zoomref.zoom3 of the slices bit for bit, the label volume is zoomref.zoom0 of
    the net's 64 x 64 labels byte for byte, and both volume functions return the metrics of exactly those labels."""
    from pn2 import voleval as V
    for name in ("scipy", "scipy.ndimage", "scipy.ndimage.interpolation"):
        monkeypatch.setitem(sys.modules, name, None)
    with pytest.raises(ImportError):
        import scipy.ndimage  # noqa: F401
    g = np.random.default_rng(11)
    vol = (g.random((3, 96, 80)) * 2.0 - 0.3).astype(np.float32)
    image, label = _d(vol)[None], _d(g.integers(0, 9, (1, 3, 96, 80)).astype(np.uint8))
    spy = _Spy(_eval_model())
    got_test = V.test_single_volume(image, label, spy, classes=9, patch_size=[64, 64], use_dual=False, batch_size=2)
    assert [tuple(x.shape) for x in spy.inputs] == [(2, 1, 64, 64), (1, 1, 64, 64)]          # the batches it already forms
    assert _same(torch.cat(spy.inputs)[:, 0], np.stack([Z.zoom3(s, 64, 64) for s in vol]))
    lab64 = torch.cat([V.predict_labels(o[-1:], "last") for o in spy.outs]).cpu().numpy()
    assert lab64.shape == (3, 64, 64) and len(np.unique(lab64)) > 1
    pred = _d(np.stack([Z.zoom0(s, 96, 80) for s in lab64]))
    seen = []
    inner = V.volume_metrics
    monkeypatch.setattr(V, "volume_metrics", lambda p, l, c: (seen.append(p.clone()), inner(p, l, c))[1])
    assert V.test_single_volume(image, label, spy, classes=9, patch_size=[64, 64], use_dual=False, batch_size=2) == got_test
    monkeypatch.setattr(V, "volume_metrics", inner)
    assert seen[0].dtype == torch.uint8 and torch.equal(seen[0], pred)
    assert got_test == V.volume_metrics(pred, label[0], 9) and len(got_test) == 8
    assert V.val_single_volume(image, label, spy, classes=9, patch_size=[64, 64], use_dual=False, batch_size=3) == V.volume_dice(pred, label[0], 9)


# ------------------------------------------------------------------------------------------------ errors
def test_errors():
    from pn2 import volinput as V
    f, u = torch.zeros(2, 8, 8), torch.zeros(2, 8, 8, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.zoom(f, (4, 4), 3)
    with pytest.raises((ValueError, RuntimeError)):
        V.zoom(u.to(dev), (4, 4), 3)          # order 3 takes fp32
    with pytest.raises((ValueError, RuntimeError)):
        V.zoom(f.to(dev).half(), (4, 4), 0)
    with pytest.raises((ValueError, RuntimeError)):
        V.rotate(f.to(dev).double(), [0, 0])
    with pytest.raises((ValueError, RuntimeError), match="1024"):
        V.zoom(torch.zeros(1, 2, 1025, device=dev), (4, 4), 3)
    with pytest.raises((ValueError, RuntimeError), match="1024"):
        V.zoom(f.to(dev), (1025, 4), 3)
    with pytest.raises((ValueError, RuntimeError)):
        V.rot_flip(torch.zeros(1, 8, 9, device=dev), [1], [0])
    with pytest.raises((ValueError, RuntimeError)):
        V.zoom(torch.full((1, 4, 4), 300, device=dev), (8, 8), 0)          # an int64 label outside uint8
