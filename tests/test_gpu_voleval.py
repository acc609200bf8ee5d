"""GPU tests of the multi-class volume evaluation (pn2/voleval.py on csrc/pn2_seg.hip) against tests/volevalref.py, the CPU restatement of the reference's
test_single_volume / val_single_volume with medpy's metrics: label maps byte for byte, voxel counts and d^2 histograms integer for integer, the four metrics,
the special cases, the size limit, determinism, and eval-mode EMCADNet (dual and single) against the oracle with the wiring of the two volume functions."""
import os

import numpy as np
import pytest
import torch

import volevalref as R

pytestmark = pytest.mark.gpu
os.environ.setdefault("PN2_NO_PRETRAINED", "1")
dev = "cuda"


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pn2
    pn2.load_library()
    yield
    pn2.set_compute_dtype("bf16")


# ------------------------------------------------------------------------------------------------ labels
def _logit_maps(K, seed, N=3, H=33, W=70):
    """Eight maps of multiples of 1/8 in [-10, 10); channel K-1 is a copy of channel 0 in every map, so the two tie in every combination."""
    g = np.random.default_rng(seed)
    maps = []
    for _ in range(8):
        m = (g.integers(-80, 80, (N, K, H, W)) / 8).astype(np.float32)
        m[:, K - 1] = m[:, 0]
        maps.append(m)
    return maps


@pytest.mark.parametrize("K", [2, 9])
def test_predict_labels_equals_the_reference_expression(K):
    """N = 3, 33 x 70 (W no multiple of 64, 6930 pixels: 27 blocks and a partial one), all three modes, byte for byte against argmax(softmax(outputs)).
    The inputs are checked first: >= 10 % of the pixels tie at the maximum and argmax(softmax) == argmax of the logits on them."""
    from pn2 import voleval as V
    maps = _logit_maps(K, 40 + K)
    dmaps = [torch.from_numpy(m).to(dev) for m in maps]
    for mode, sel in (("last", slice(0, 8)), ("sum_fg", slice(0, 4)), ("sum_fg_minus_bg", slice(0, 8))):
        x = R.combine(maps[sel], mode)
        top = x.max(axis=1, keepdims=True)
        ties = float(((x == top).sum(axis=1) > 1).mean())
        want = R.labels(maps[sel], mode)
        assert ties >= 0.10 and np.array_equal(want, R.labels(maps[sel], mode, softmax=False)), (mode, ties)
        got = V.predict_labels(dmaps[sel], mode)
        assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
        assert np.array_equal(got.cpu().numpy(), want), mode
    assert len(np.unique(want)) == K - 1          # every class but the copy's higher index is predicted somewhere
    with pytest.raises(ValueError):
        V.predict_labels(dmaps, "softmax")
    with pytest.raises(ValueError):
        V.predict_labels(dmaps[:3], "sum_fg_minus_bg")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.predict_labels([torch.from_numpy(maps[0])], "last")


# ------------------------------------------------------------------------------------------------ counts
def test_counts_dice_jaccard_with_absent_classes():
    """5 x 37 x 70, K = 9: classes 2 and 3 absent from pred, 4 absent from gt, 5 absent from both.  Counts equal numpy's, Dice / Jaccard the reference's float64
    values exactly (the same integer expressions)."""
    from pn2 import voleval as V
    g = np.random.default_rng(7)
    pred, gt = g.integers(0, 9, (5, 37, 70)).astype(np.uint8), g.integers(0, 9, (5, 37, 70)).astype(np.uint8)
    for c in (2, 3, 5):
        pred[pred == c] = 0
    for c in (4, 5):
        gt[gt == c] = 0
    p, t = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
    cnt = V.class_counts(p, t, 9)
    want = np.array([[(pred == c).sum(), (gt == c).sum(), ((pred == c) & (gt == c)).sum()] for c in range(9)])
    assert np.array_equal(cnt, want)
    assert V.volume_dice(p, t, 9) == R.volume_dice(pred, gt, 9)
    got, ref = V.volume_metrics(p, t, 9), R.volume_metrics(pred, gt, 9)
    for c, (a, b) in enumerate(zip(got, ref), start=1):
        assert a[0] == b[0] and a[2] == b[2], c
    assert ref[1] == (0, 0, 0, 0) and ref[3] == (1, 0, 1, 0) and ref[4] == (0, 0, 0, 0)


# ------------------------------------------------------------------------------------------------ surface distances
SHAPES = [(5, 37, 70), (67, 9, 130), (3, 64, 64), (37, 70)]
CONTENTS = ["ellipsoids", "voxels", "full_vs_voxel", "six_faces", "random4"]


def _pair(shape, content):
    """(pred, gt, classes) uint8 label volumes of `shape` (3-D or 2-D)."""
    full = (1,) * (3 - len(shape)) + tuple(shape)
    D, H, W = full
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    pred, gt, K = np.zeros(full, np.uint8), np.zeros(full, np.uint8), 2

    def ell(c, r):
        return ((z - c[0] * (D - 1)) / max(r[0] * D, 0.6)) ** 2 + ((y - c[1] * (H - 1)) / (r[1] * H)) ** 2 + ((x - c[2] * (W - 1)) / (r[2] * W)) ** 2 <= 1.0
    if content == "ellipsoids":          # class 1: two overlapping ellipsoids; class 2: disjoint ones far apart
        K = 3
        pred[ell((0.5, 0.45, 0.4), (0.35, 0.3, 0.25))] = 1
        gt[ell((0.5, 0.55, 0.5), (0.3, 0.25, 0.3))] = 1
        pred[ell((0.2, 0.15, 0.9), (0.2, 0.1, 0.06))] = 2
        gt[ell((0.8, 0.85, 0.08), (0.2, 0.1, 0.05))] = 2
    elif content == "voxels":
        pred[D // 3, H // 4, W // 5] = 1
        gt[D - 1, H - 1, W - 2] = 1
    elif content == "full_vs_voxel":          # the border of a full volume is its outer shell (ndim faces)
        pred[:] = 1
        gt[D // 2, H // 2, W // 3] = 1
    elif content == "six_faces":          # three bars through the centre reach all faces; gt: a box that touches none
        pred[:, H // 2 - 1:H // 2 + 2, W // 2 - 2:W // 2 + 2] = 1
        pred[D // 2, :, W // 2 - 2:W // 2 + 2] = 1
        pred[D // 2, H // 2 - 1:H // 2 + 2, :] = 1
        gt[(D > 2) * 1:D - (D > 2) * 1, H // 4:H // 2, W // 8:W // 2] = 1
    elif content == "random4":
        K = 4
        g = np.random.default_rng(sum(shape))
        pred, gt = g.integers(0, 4, full).astype(np.uint8), g.integers(0, 4, full).astype(np.uint8)
    return pred.reshape(shape), gt.reshape(shape), K


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_surface_histograms_and_metrics(shape, content):
    """Per class: the d^2 histogram of each direction equals rint(dt[border]^2) of the reference integer for integer, both border counts equal the reference's,
    hd95 and asd agree within 1e-9 relative (the n * 2^-53 bound of a float64 sum over at most 2^24 non-negative terms against numpy's pairwise sum; the
    percentile interpolates two exact square roots), Dice and Jaccard exactly."""
    from pn2 import voleval as V
    pred, gt, K = _pair(shape, content)
    p, t = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
    full = (1,) * (3 - len(shape)) + tuple(shape)
    L = sum((n - 1) ** 2 for n in full) + 1
    classes = list(range(1, K))
    assert all((pred == c).any() and (gt == c).any() for c in classes)
    hists = V.surface_histograms(p, t, classes)
    got = V.volume_metrics(p, t, K)
    ref = R.volume_metrics(pred, gt, K)
    for c in classes:
        a, b = pred == c, gt == c
        h_ab, h_ba, na, nb = hists[c]
        assert len(h_ab) == L and len(h_ba) == L
        assert na == int(R.border(a).sum()) and nb == int(R.border(b).sum()), c
        assert np.array_equal(h_ab, R.d2_histogram(a, b, L)), c
        assert np.array_equal(h_ba, R.d2_histogram(b, a, L)), c
        dice, hd95, jac, asd = got[c - 1]
        rd, rh, rj, ra = ref[c - 1]
        print(f"\n{shape} {content} class {c}: border {na}/{nb}, hd95 {hd95!r} (ref {rh!r}), asd {asd!r} (ref {ra!r})")
        assert dice == rd and jac == rj, c
        assert abs(hd95 - rh) <= 1e-9 * abs(rh) and abs(asd - ra) <= 1e-9 * abs(ra), c


def test_special_cases_launch_no_distance_pass(monkeypatch):
    """Class 1 in both, 2 only in pred -> (1, 0, 1, 0), 3 only in gt and 4 in neither -> (0, 0, 0, 0); the distance kernels are asked for class 1 alone."""
    from pn2 import voleval as V
    pred, gt = np.zeros((3, 20, 30), np.uint8), np.zeros((3, 20, 30), np.uint8)
    pred[1, 5:9, 5:9] = 1; gt[1, 6:10, 4:9] = 1
    pred[0, 1, 1] = 2
    gt[2, 18, 28] = 3
    asked = []
    inner = V.surface_histograms
    monkeypatch.setattr(V, "surface_histograms", lambda p, g, cl: (asked.append(list(cl)), inner(p, g, cl))[1])
    got = V.volume_metrics(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev), 5)
    ref = R.volume_metrics(pred, gt, 5)
    assert asked == [[1]]
    assert got[1] == ref[1] == (1, 0, 1, 0) and got[2] == ref[2] == (0, 0, 0, 0) and got[3] == ref[3] == (0, 0, 0, 0)
    assert all(type(v) is int for v in got[1] + got[2])
    assert got[0][0] == ref[0][0] and abs(got[0][1] - ref[0][1]) <= 1e-9 * ref[0][1]


def test_axis_limit_raises_before_any_launch(monkeypatch):
    from pn2 import voleval as V

    class NoLaunch:
        def __getattr__(self, name):
            raise AssertionError(f"{name} was called")
    monkeypatch.setattr(V, "call", NoLaunch())
    big = torch.ones((1, 1, 1025), dtype=torch.uint8, device=dev)
    for fn in (V.volume_metrics, V.volume_dice, V.class_counts):
        with pytest.raises(ValueError, match="1024"):
            fn(big, big, 2)
    with pytest.raises(ValueError, match="1024"):
        V.surface_histograms(big, big, [1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.volume_metrics(big.cpu(), big.cpu(), 2)


def test_two_calls_are_identical():
    from pn2 import voleval as V
    pred, gt, K = _pair((5, 37, 70), "random4")
    p, t = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
    h1, h2 = V.surface_histograms(p, t, [1, 2, 3]), V.surface_histograms(p, t, [1, 2, 3])
    for c in (1, 2, 3):
        assert np.array_equal(h1[c][0], h2[c][0]) and np.array_equal(h1[c][1], h2[c][1]) and h1[c][2:] == h2[c][2:]
    assert V.volume_metrics(p, t, K) == V.volume_metrics(p, t, K)


# ------------------------------------------------------------------------------------------------ model path
def _eval_model(dual):
    """EMCADNet(K = 9, pvt_v2_b2) with the weights of the train-mode tests and non-trivial BatchNorm running statistics, eval mode, fp32."""
    import pn2
    import seglossref as S
    from lib.networks import EMCADNet
    from oracle import weights as W
    pn2.set_compute_dtype("fp32")
    m = EMCADNet(num_classes=9, kernel_sizes=[1, 3, 5], expansion_factor=2, dw_parallel=True, add=True, lgag_ks=3, activation="relu6", encoder="pvt_v2_b2",
                 pretrain=False, dual=dual)
    sd = R.nontrivial_bn_stats(W.make_state_dict(W.manifest_emcadnet(9) if dual else S.single_manifest(9), seed=5), seed=17)
    m.load_state_dict(sd, strict=True)
    m.backbone.reset_drop_path(0.0)
    return m.to(dev).eval(), sd


@pytest.mark.parametrize("dual", [True, False])
def test_eval_mode_emcadnet_vs_oracle_and_volume_wiring(dual, monkeypatch):
    """Eval-mode forward under no_grad against the CPU oracle in float64 with the bound of the fp32 train-mode maps of tests/test_gpu_emcad.py
    (max(1e-4, 3 x the oracle's own fp32-to-float64 distance)); then val_single_volume / test_single_volume on a 4-slice volume: the labels are predict_labels
    of the net's own batched eval forward and the metrics volume_metrics / volume_dice of those labels."""
    from oracle import emcad_oracle as E
    from pn2 import voleval as V
    model, sd = _eval_model(dual)
    g = torch.Generator().manual_seed(23)
    x = torch.randn(2, 1, 64, 64, generator=g)
    with torch.no_grad():
        outs = model(x.to(dev))
        fwd = E.emcadnet_forward if dual else R.emcadnet_single_forward
        o32 = fwd({k: v.clone() for k, v in sd.items()}, x, training=False)
        o64 = fwd({k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}, x.double(), training=False)
    assert len(outs) == (8 if dual else 4) and all(tuple(o.shape) == (2, 9, 64, 64) and not o.requires_grad for o in outs)
    for i, (o, a, b) in enumerate(zip(outs, o32, o64)):
        own = float((a.double() - b).abs().max())
        err = float((o.double().cpu() - b).abs().max())
        print(f"\neval EMCADNet dual={dual} map {i}: max |ours - float64| {err:.2e}, the oracle's fp32 run {own:.2e}")
        assert err <= max(1e-4, 3 * own), i
    assert all(bool((v == sd[k].to(v.device)).all()) for k, v in model.state_dict().items() if k.endswith(("running_mean", "running_var")))
    # ---- wiring
    image = torch.randn(1, 4, 64, 64, generator=g).to(dev)
    label = torch.randint(0, 9, (1, 4, 64, 64), generator=g).to(dev)
    with torch.no_grad():
        o = model(image[0][:, None].contiguous())
    seen = {}
    inner = V.predict_labels
    monkeypatch.setattr(V, "predict_labels", lambda outs_, mode: seen.setdefault(mode, inner(outs_, mode)))
    got_test = V.test_single_volume(image, label, model, classes=9, patch_size=[64, 64], use_dual=dual)
    got_val = V.val_single_volume(image, label, model, classes=9, patch_size=[64, 64], use_dual=dual)
    monkeypatch.undo()
    lab_test = V.predict_labels(o[:4], "sum_fg") if dual else V.predict_labels(o[-1:], "last")
    lab_val = V.predict_labels(o[:4] + o[-4:], "sum_fg_minus_bg") if dual else lab_test
    assert set(seen) == ({"sum_fg", "sum_fg_minus_bg"} if dual else {"last"})
    assert torch.equal(seen["sum_fg" if dual else "last"], lab_test)
    assert got_test == V.volume_metrics(lab_test, label[0], 9) and len(got_test) == 8 and all(len(t) == 4 for t in got_test)
    assert got_val == V.volume_dice(lab_val, label[0], 9) and len(got_val) == 8
    assert model.training is False
