"""GPU tests of flip test-time augmentation in pn2.infer.VolumePredictor (tta=, tta_average=): eval-mode EMCADNet(num_classes=4, pvt_v2_b0, dual) and
PVT_CASCADE(dual=False) with seeded weights and non-trivial BatchNorm statistics, fp32 compute, patch 64 x 64, batch 2, a [3][48][40] volume (a short last
batch, resampled both ways).

The labels of every batch under tta="flips" are compared with tests/ttaref.py in float64 on the low-resolution maps that a PLAIN predictor (no tta) leaves for
each flipped batch - the path that shares nothing with the TTA graph but the forward itself.  Rule (that of tests/test_gpu_tta_kernels.py): T = 2 * 3 * e32 with
e32 the distance of the unfused fp32 composition (Engine.bilinear, torch.flip, torch's fp32 sums and softmax) from float64 on the same maps; the class picked may
lie at most T below the largest float64 score, and at most 0.5 % of a batch's pixels may have a float64 top-two gap below T.  Each case prints its figures
(run with -s, lines starting with TTAP).  Further: replays return the same bytes, tta=None is today's predictor byte for byte with today's graph keys, train mode is
refused, the volume functions return voleval's numbers for those labels, a single 2-D image takes its own B = 1 graph.

MI355X, 2026-10-21: e32 1.7e-07 .. 1.9e-06 (T 1.0e-06 .. 1.1e-05); in every batch no pixel within T of a tie and no label other than float64's; the maps the TTA
graph leaves for its V * B samples equal the plain graph's maps of the flipped batches bit for bit (largest distance 0)."""
import os
from collections import OrderedDict

import pytest
import torch

import ttaref as R

pytestmark = pytest.mark.gpu
os.environ.setdefault("PN2_NO_PRETRAINED", "1")
dev = "cuda"
PATCH, BATCH, K = (64, 64), 2, 4
FLIPS = ("id", "h", "v")


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pn2
    pn2.load_library()
    pn2.set_compute_dtype("fp32")
    yield
    pn2.set_compute_dtype("bf16")


def _model(kind):
    import volevalref as VR
    from oracle import weights as W
    if kind == "emcad":
        from lib.networks import EMCADNet
        m = EMCADNet(num_classes=K, encoder="pvt_v2_b0", dual=True, pretrain=False)
    else:
        from lib.cascade_net import PVT_CASCADE
        m = PVT_CASCADE(num_classes=K, encoder="pvt_v2_b0", dual=False, pretrain=False)
    manifest = OrderedDict((k, tuple(v.shape)) for k, v in m.state_dict().items())
    m.load_state_dict(VR.nontrivial_bn_stats(W.make_state_dict(manifest, seed=5), seed=17), strict=True)
    m.backbone.reset_drop_path(0.0)
    return m.to(dev).eval()


def _batches(image):
    """The batches VolumePredictor.predict forms: (zoomed [BATCH][ph][pw] filled with zero slices, number of real slices)."""
    from pn2.volinput import zoom
    out = []
    for i in range(0, image.shape[0], BATCH):
        xb = zoom(image[i:i + BATCH].float(), PATCH, 3)
        n = xb.shape[0]
        if n < BATCH:
            xb = torch.cat([xb, xb.new_zeros((BATCH - n,) + PATCH)])
        out.append((xb, n))
    return out


def _check_batch(plain, tta, xb, mode, views, average, tag, B=BATCH):
    """The float64 rule for one batch; returns the TTA labels [B][ph][pw]."""
    from pn2.infer import VolumePredictor
    lows = None
    for view in views:
        dims = [d for d, bit in ((2, 1), (1, 2)) if R.VIEWS[view] & bit]
        xv = torch.flip(xb, dims).contiguous() if dims else xb
        got = [lo.permute(0, 2, 3, 1).contiguous() for lo in plain.lowres(xv[:, None], mode)]          # NHWC [B][h][w][K]
        lows = [[g] for g in got] if lows is None else [a + [g] for a, g in zip(lows, got)]
    lows = [torch.cat(a) for a in lows]          # [V * B]...: view v of sample n at v * B + n
    scales = [PATCH[0] // lo.shape[1] for lo in lows]
    dm, sc_ = VolumePredictor._pick(lows, scales, mode)
    sc = R.scores([m.cpu() for m in dm], sc_, mode, views, average, K)
    e32 = float((R.unfused_scores(R.unfused_ups(dm, sc_, views, K, B), mode, average).cpu().double() - sc).abs().max())
    T = 2 * 3 * e32
    got = tta._labels(xb[:, None], mode)["labels"].clone()
    share = float((R.gap(sc) < T).double().mean())
    worst = float(R.deficit(sc, got.cpu()).max())
    own = tta.lowres(xb[:, None], mode)
    assert all(o.shape[0] == len(views) * B for o in own)
    fwd = max(float((o.permute(0, 2, 3, 1) - lo).abs().max()) for o, lo in zip(own, lows))
    print(f"TTAP {tag}: e32 {e32:.2e} T {T:.2e} near ties {share:.2e} largest deficit {worst:.2e} pixels that differ {int((got.cpu() != R.labels(sc)).sum())} "
          f"classes {len(torch.unique(got))} |TTA graph's maps - plain graph's maps| {fwd:.2e}")
    assert fwd == 0.0, tag          # fp32: pn2_flip_views + the forward over V * B samples ARE the per-view forwards of the flipped batches
    assert share <= R.MAX_EXCUSED, tag
    assert worst <= T, tag
    return got


def test_emcad_dual_under_flip_tta():
    from pn2 import voleval as V
    from pn2.infer import VolumePredictor
    from pn2.volinput import zoom
    model = _model("emcad")
    plain = VolumePredictor(model, patch_size=PATCH, batch_size=BATCH)
    tta = VolumePredictor(model, patch_size=PATCH, batch_size=BATCH, tta="flips")
    assert tta.views == FLIPS and tta.tta_average == "prob"
    g = torch.Generator().manual_seed(31)
    image = torch.randn(3, 48, 40, generator=g).to(dev)
    label = torch.randint(0, K, (3, 48, 40), generator=g).to(dev)
    want = {}
    for mode in ("last", "sum_fg", "sum_fg_minus_bg"):
        labs = [_check_batch(plain, tta, xb, mode, FLIPS, "prob", f"emcad {mode} batch {i}")[:n] for i, (xb, n) in enumerate(_batches(image))]
        want[mode] = torch.cat([zoom(lab, (48, 40), 0) for lab in labs])
        got = tta.predict(image, mode)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (3, 48, 40) and torch.equal(got, want[mode]), mode
        assert len(torch.unique(got)) > 1
    assert set(tta._states) == {(BATCH, *PATCH, mode, FLIPS, "prob") for mode in want}
    assert not torch.equal(want["sum_fg"], plain.predict(image, "sum_fg"))          # the augmentation changes labels
    # replays
    xb = _batches(image)[0][0]
    first = tta._labels(xb[:, None], "sum_fg")["labels"].clone()
    assert torch.equal(tta._labels(xb[:, None], "sum_fg")["labels"], first) and torch.equal(tta._labels(xb[:, None], "sum_fg")["labels"], first)
    # tta=None is the predictor without the keyword
    none = VolumePredictor(model, patch_size=PATCH, batch_size=BATCH, tta=None)
    for mode in ("last", "sum_fg_minus_bg"):
        assert torch.equal(none.predict(image, mode), plain.predict(image, mode))
    assert set(none._states) == {(BATCH, *PATCH, "last"), (BATCH, *PATCH, "sum_fg_minus_bg")}
    # the logit average through the predictor: one batch
    logit = VolumePredictor(model, patch_size=PATCH, batch_size=BATCH, tta=("hv", "id"), tta_average="logit")
    _check_batch(plain, logit, xb, "sum_fg_minus_bg", ("hv", "id"), "logit", "emcad sum_fg_minus_bg hv+id logit")
    # the volume functions, and a single 2-D image (its own B = 1 graph, the last map whatever use_dual says)
    assert tta.val_single_volume(image[None], label[None], K, use_dual=True) == V.volume_dice(want["sum_fg_minus_bg"], label, K)
    assert tta.test_single_volume(image[None], label[None], K, use_dual=True) == V.volume_metrics(want["sum_fg"], label, K)
    img2 = torch.randn(64, 64, generator=g).to(dev)
    lab2 = torch.randint(0, K, (64, 64), generator=g).to(dev)
    one = VolumePredictor(model, patch_size=PATCH, batch_size=1)
    one_tta = VolumePredictor(model, patch_size=PATCH, batch_size=1, tta="flips")
    lab = _check_batch(one, one_tta, img2[None], "last", FLIPS, "prob", "emcad single image", B=1)[0]
    assert torch.equal(one_tta.predict(img2, "last"), lab)
    assert one_tta.test_single_volume(img2[None], lab2[None], K, use_dual=True) == V.volume_metrics(lab, lab2, K)
    assert set(one_tta._states) == {(1, 64, 64, "last", FLIPS, "prob")}
    # train mode is refused, on a fresh predictor and on one that holds graphs
    model.train()
    with pytest.raises(RuntimeError, match="eval"):
        tta.predict(image, "sum_fg")
    with pytest.raises(RuntimeError, match="eval"):
        VolumePredictor(model, patch_size=PATCH, batch_size=BATCH, tta="flips").predict(image, "last")
    model.eval()


def test_val_slices_passes_tta_through():
    """voleval.val_slices builds its own predictor with the keyword, and takes a predictor built with it unchanged: the same numbers."""
    from pn2 import voleval as V
    from pn2.infer import VolumePredictor
    model = _model("emcad")
    g = torch.Generator().manual_seed(5)
    images = [torch.randn(48, 40, generator=g).to(dev), torch.randn(64, 64, generator=g).to(dev), torch.randn(30, 52, generator=g).to(dev)]
    labels = [torch.randint(0, K, tuple(im.shape), generator=g).to(torch.uint8).to(dev) for im in images]
    vp = VolumePredictor(model, patch_size=PATCH, batch_size=BATCH, tta="flips")
    d0, m0 = V.val_slices(images, labels, vp, 64, "sum_fg_minus_bg")
    d1, m1 = V.val_slices(images, labels, model, 64, "sum_fg_minus_bg", batch_size=BATCH, tta="flips")
    d2, _ = V.val_slices(images, labels, model, 64, "sum_fg_minus_bg", batch_size=BATCH)
    assert d0.tolist() == d1.tolist() and m0 == m1
    assert d0.tolist() != d2.tolist()
    with pytest.raises(ValueError):
        V.val_slices(images, labels, model, 64, "sum_fg_minus_bg", batch_size=BATCH, tta="rot")


def test_pvt_cascade_single_under_flip_tta():
    from pn2.infer import VolumePredictor
    model = _model("cascade")
    plain = VolumePredictor(model, patch_size=PATCH, batch_size=BATCH)
    tta = VolumePredictor(model, patch_size=PATCH, batch_size=BATCH, tta="flips")
    image = torch.randn(3, 48, 40, generator=torch.Generator().manual_seed(32)).to(dev)
    for i, (xb, n) in enumerate(_batches(image)):
        for mode in ("last", "sum_fg"):
            _check_batch(plain, tta, xb, mode, FLIPS, "prob", f"cascade {mode} batch {i}")
    got = tta.predict(image, "sum_fg")          # (with these weights the last map alone predicts one class everywhere; the sum of the four predicts three)
    assert tuple(got.shape) == (3, 48, 40) and len(torch.unique(got)) > 1
