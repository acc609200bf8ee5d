"""GPU test of pn2.voleval.val_slices - the val() loop of multiclass_seg/MIST/ACDC_train_test.py:48-93 on ragged batches - against the per-slice composition of the
public functions that were there before it: volinput.zoom (order 3), the labels of a VolumePredictor, volinput.zoom (order 0), medpy's dc restated in numpy.
A tiny EMCADNet(encoder='pvt_v2_b0', num_classes=4) at a 64 x 64 patch on three slices of differing sizes, one of them already 64 x 64."""
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

import raggedref as R

pytestmark = pytest.mark.gpu
os.environ.setdefault("PN2_NO_PRETRAINED", "1")
dev = "cuda"
S, BATCH, K = 64, 2, 4
SHAPES = [(80, 72), (64, 64), (50, 90)]


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pn2
    pn2.load_library()
    yield
    pn2.set_compute_dtype("bf16")


def _eval_model():
    """EMCADNet(dual, K = 4, pvt_v2_b0): the ACDC model, seeded weights of the oracle's distribution, non-trivial BatchNorm running statistics, eval mode."""
    import volevalref as VR
    from lib.networks import EMCADNet
    from oracle import weights as W
    m = EMCADNet(num_classes=K, kernel_sizes=[1, 3, 5], expansion_factor=2, dw_parallel=True, add=True, lgag_ks=3, activation="relu6", encoder="pvt_v2_b0",
                 pretrain=False, dual=True)
    manifest = OrderedDict((k, tuple(v.shape)) for k, v in m.state_dict().items())
    m.load_state_dict(VR.nontrivial_bn_stats(W.make_state_dict(manifest, seed=5), seed=17), strict=True)
    m.backbone.reset_drop_path(0.0)
    return m.to(dev).eval()


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def test_val_slices_equals_the_per_slice_composition(monkeypatch):
    from pn2 import voleval as E
    from pn2 import volinput as V
    from pn2.infer import VolumePredictor
    g = np.random.default_rng(21)
    images = [(g.random(s) * 2.0 - 0.3).astype(np.float32) for s in SHAPES]
    labels = [g.integers(0, K, s).astype(np.uint8) for s in SHAPES]
    labels[2][:] = 0          # an empty label: dc is 0.0 whatever the prediction holds
    vp = VolumePredictor(_eval_model(), patch_size=(S, S), batch_size=BATCH)
    seen = []
    inner = V._dice_counts_dev
    monkeypatch.setattr(V, "_dice_counts_dev", lambda p, q, sizes, plan=None: (seen.append((p.clone(), list(sizes))), inner(p, q, sizes, plan))[1])
    for mode in ("sum_fg_minus_bg", "last"):          # the dual combination of val() and a single-map mode
        seen.clear()
        dice, mean = E.val_slices(images, labels, vp, S, mode)
        assert dice.dtype == np.float64 and dice.shape == (3,) and [s for _, ss in seen for s in ss] == SHAPES          # batches of 2 and 1
        got = [p[o:o + s[0] * s[1]].view(s).cpu().numpy() for p, ss in seen for o, s in zip(np.cumsum([0] + [a * b for a, b in ss]), ss)]
        want_dice = []
        for i, (im, lb) in enumerate(zip(images, labels)):
            x = V.zoom(_d(im)[None], (S, S), 3)          # returns its input for the 64 x 64 slice: the reference skips the call
            xb = torch.cat([x, x.new_zeros((BATCH - 1, S, S))])
            lab = vp._labels(xb[:, None], mode)["labels"][:1].clone()
            back = V.zoom(lab, im.shape, 0)[0].cpu().numpy()
            assert back.dtype == np.uint8 and np.array_equal(got[i], back), (mode, i)
            assert np.array_equal(vp.predict(_d(im)[None], mode)[0].cpu().numpy(), back)
            want_dice.append(R.dc(back, lb))
            if i < 2:
                assert len(np.unique(back)) > 1
        print(f"\n{mode}: dice {dice.tolist()}")
        assert dice.tolist() == want_dice and dice[2] == 0.0 and 0.0 < dice[0] < 1.0
        assert mean == (0 + want_dice[0] + want_dice[1] + want_dice[2]) / 3
        again, mean2 = E.val_slices([_d(a) for a in images], [_d(a) for a in labels], vp, S, mode)          # GPU tensors in
        assert again.tolist() == want_dice and mean2 == mean
    assert set(vp._states) == {(BATCH, S, S, "sum_fg_minus_bg"), (BATCH, S, S, "last")}          # the predictor's existing graphs, nothing new
    # a non-square volume through the volume path that was there before (passes without the ragged entry points too: kept as a guard)
    vol = _d(np.stack([(g.random((80, 72)) * 2.0 - 0.3).astype(np.float32) for _ in range(3)]))
    lab = _d(g.integers(0, K, (3, 80, 72)).astype(np.uint8))
    pred = vp.predict(vol, "sum_fg_minus_bg")
    assert tuple(pred.shape) == (3, 80, 72) and torch.equal(pred, torch.cat([vp.predict(v[None], "sum_fg_minus_bg") for v in vol]))
    assert vp.val_single_volume(vol[None], lab[None], K, use_dual=True) == E.volume_dice(pred, lab, K)
    with pytest.raises(ValueError):
        E.val_slices(images, labels[:2], vp, S, "last")
    with pytest.raises(ValueError):
        E.val_slices(images, labels, vp, 32, "last")          # not the predictor's patch size
    with pytest.raises(ValueError):
        E.val_slices(images, labels, vp, S, "mean")
