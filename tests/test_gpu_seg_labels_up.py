"""GPU tests of the fused label tail pn2_seg_labels_up (csrc/pn2_seg.hip, through pn2.voleval.predict_labels_up) and of pn2.infer.VolumePredictor: the kernel
byte for byte against tests/seglabelupref.py and against the unfused device path (Engine.bilinear of every map, then predict_labels) on inputs where float32 is
exact, within a derived margin on Gaussian maps, and the predictor against the nn.Module surface and pn2.voleval on eval-mode EMCADNet (dual and single)."""
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

import seglabelupref as R

pytestmark = pytest.mark.gpu
os.environ.setdefault("PN2_NO_PRETRAINED", "1")
dev = "cuda"
SHAPES = [(64, 64), (64, 96)]


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pn2
    pn2.load_library()
    yield
    pn2.set_compute_dtype("bf16")


# ------------------------------------------------------------------------------------------------ kernel
def _unfused(dmaps, scales, mode, K):
    """The device path the fused kernel replaces: pn2_bilinear_fwd of every NHWC map (padding channels included), then predict_labels of the NCHW maps.
    -> (labels, the up-sampled NCHW maps)."""
    from pn2 import voleval as V
    from pn2.engine import Act, Engine, F32
    eng = Engine(F32, False, need_grad=False)
    ups = [eng.to_nchw(eng.bilinear(Act(eng, t, K, K, t.shape[3], F32, requires_grad=False), s)) for t, s in zip(dmaps, scales)]
    return V.predict_labels(ups, mode), ups


def _fused(dmaps, scales, mode, K):
    from pn2 import voleval as V
    return V.predict_labels_up([t[..., :K] for t in dmaps], scales, mode)


@pytest.mark.parametrize("wide", [False, True], ids=["ld=K", "ld=16"])
@pytest.mark.parametrize("K", [2, 4, 9, 16])
def test_fused_labels_exact_on_dyadic_maps(K, wide):
    """N = 3, outputs 64 x 64 and 64 x 96 (one and two 64-pixel waves per row, 16 row groups), maps at 1/32 .. 1/4 (s = 32 .. 4: the 2 x 2 / 2 x 3 source is
    mostly edge clamping), 'last' with 1 map, 'sum_fg' with 4, 'sum_fg_minus_bg' with 8.  ld = K reads scalars for K = 2 and 9 and 16-byte vectors for K = 4 and
    16; ld = 16 reads vectors, with NaN in the padding channels.  Dyadic inputs (seglabelupref.dyadic_maps): every intermediate is exact in float32, so the
    fused kernel, the restatement and the unfused device path must agree byte for byte; ties between channels occur in every case."""
    ld = 16 if wide else K
    for OH, OW in SHAPES:
        for mode in R.MODES:
            nmaps, scales = R.case(mode)
            maps = R.dyadic_maps(K, ld, [(OH // s, OW // s) for s in scales], 3, seed=100 * K + OW + nmaps)
            dmaps = [torch.from_numpy(m).to(dev) for m in maps]
            want = R.labels(maps, scales, mode, K)
            assert R.tie_share(maps, scales, mode, K) > 0
            got = _fused(dmaps, scales, mode, K)
            assert got.dtype == torch.uint8 and tuple(got.shape) == (3, OH, OW)
            assert np.array_equal(got.cpu().numpy(), want), (mode, OH, OW)
            assert torch.equal(got, _unfused(dmaps, scales, mode, K)[0]), (mode, OH, OW)


def test_fused_labels_with_a_nan_and_an_unaligned_base():
    """A NaN in one channel of one low-resolution pixel spreads over the pixels that tap it, in the fused and in the unfused path alike (the same weights, zero
    weights included), and wins the argmax there: byte for byte.  Then the same maps from a base that is not 16-byte aligned: the scalar reads at ld = 16."""
    K, OH, OW = 9, 64, 96
    nmaps, scales = R.case("sum_fg")
    maps = R.dyadic_maps(K, 16, [(OH // s, OW // s) for s in scales], 3, seed=77)
    maps[1][2, 1, 3, 5] = np.nan          # the 4 x 6 map (s = 16): sample 2, pixel (1, 3), channel 5
    want = R.labels(maps, scales, "sum_fg", K)
    dmaps = [torch.from_numpy(m).to(dev) for m in maps]
    got = _fused(dmaps, scales, "sum_fg", K)
    hit = want[2] == 5
    assert hit[16:32, 48:64].all() and not (want[:2] == 5).all()          # the pixel's own 16 x 16 block takes the NaN's channel
    assert np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(got, _unfused(dmaps, scales, "sum_fg", K)[0])
    shifted = []
    for t in dmaps:
        buf = torch.zeros(t.numel() + 1, device=dev)
        buf[1:].copy_(t.reshape(-1))
        shifted.append(buf[1:].view(t.shape))
        assert shifted[-1].data_ptr() % 16 == 4
    assert torch.equal(_fused(shifted, scales, "sum_fg", K), got)


@pytest.mark.parametrize("wide", [False, True], ids=["ld=9", "ld=16"])
def test_fused_labels_on_gaussian_maps_within_the_rounding_margin(wide):
    """Seeded N(0, 1) maps, K = 9, the shapes and modes of the exact test, against the unfused device path.  The two paths may round the four-tap expression
    differently (the instantiations of the bilinear kernel contract it differently) and nothing else: per map at most a few ulps of max|map|, so the combined
    logits differ by less than margin = 16 * nmaps * 2^-23 * max|map| (derived, not measured).  A pixel may differ only where the unfused path's two largest
    combined logits lie within that margin of each other, and such pixels must be at most 0.1 % of all (for Gaussian maps the expected share is of the order of
    the margin itself, ~1e-5)."""
    K, ld = 9, (16 if wide else 9)
    g = torch.Generator().manual_seed(2024 + ld)
    for OH, OW in SHAPES:
        for mode in R.MODES:
            nmaps, scales = R.case(mode)
            dmaps = []
            for s in scales:
                t = torch.full((3, OH // s, OW // s, ld), float("nan"))
                t[..., :K] = torch.randn(3, OH // s, OW // s, K, generator=g)
                dmaps.append(t.to(dev))
            got = _fused(dmaps, scales, mode, K)
            ref, ups = _unfused(dmaps, scales, mode, K)
            if mode == "last":
                x = ups[-1]
            elif mode == "sum_fg":
                x = torch.zeros_like(ups[0])
                for p in ups:
                    x = x + p
            else:
                x = torch.zeros_like(ups[0])
                for p, q in zip(ups[:nmaps // 2], ups[nmaps // 2:]):
                    x = x + (p - q)
            assert torch.equal(torch.argmax(x, dim=1).to(torch.uint8), ref)          # x is the unfused path's combined logit
            margin = 16 * nmaps * 2.0 ** -23 * max(float(t[..., :K].abs().max()) for t in dmaps)
            top = torch.topk(x, 2, dim=1).values
            near = (top[:, 0] - top[:, 1]) <= margin
            share, differ = float(near.float().mean()), got != ref
            print(f"\nld {ld} {OH}x{OW} {mode}: margin {margin:.2e}, pixels within it {share:.2e}, pixels that differ {int(differ.sum())}")
            assert share <= 1e-3
            assert not bool((differ & ~near).any()), (mode, OH, OW)


def test_predict_labels_up_refuses_what_the_kernel_does_not_take():
    from pn2 import voleval as V
    m = [torch.zeros(2, 64 // s, 64 // s, 16, device=dev) for s in (32, 16, 8, 4)]
    with pytest.raises(ValueError):
        V.predict_labels_up(m, [32, 16, 8, 4], "softmax")
    with pytest.raises(ValueError):
        V.predict_labels_up(m[:3], [32, 16, 8], "sum_fg_minus_bg")
    with pytest.raises(ValueError):
        V.predict_labels_up(m, [32, 16, 8, 8], "sum_fg")                       # two output sizes
    with pytest.raises(ValueError):
        V.predict_labels_up([t[..., ::2] for t in m], [32, 16, 8, 4], "sum_fg")          # channel stride 2
    with pytest.raises(ValueError):
        V.predict_labels_up([t[..., :1] for t in m], [32, 16, 8, 4], "sum_fg")           # K = 1
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.predict_labels_up([t.cpu() for t in m], [32, 16, 8, 4], "sum_fg")
    assert int(V.predict_labels_up([t[..., :9] for t in m], [32, 16, 8, 4], "sum_fg").max()) == 0          # all logits equal: class 0


# ------------------------------------------------------------------------------------------------ predictor
PATCH, BATCH = (64, 64), 4


def _eval_model(dual, mode):
    """EMCADNet(K = 9, pvt_v2_b0), seeded weights of the oracle's distribution and non-trivial BatchNorm running statistics, eval mode, compute mode `mode`."""
    import pn2
    import volevalref as VR
    from lib.networks import EMCADNet
    from oracle import weights as W
    pn2.set_compute_dtype(mode)
    m = EMCADNet(num_classes=9, kernel_sizes=[1, 3, 5], expansion_factor=2, dw_parallel=True, add=True, lgag_ks=3, activation="relu6", encoder="pvt_v2_b0",
                 pretrain=False, dual=dual)
    manifest = OrderedDict((k, tuple(v.shape)) for k, v in m.state_dict().items())
    m.load_state_dict(VR.nontrivial_bn_stats(W.make_state_dict(manifest, seed=5), seed=17), strict=True)
    m.backbone.reset_drop_path(0.0)
    return m.to(dev).eval()


def _pick(outs, mode):
    outs = list(outs)
    return {"last": outs[-1:], "sum_fg": outs[:4], "sum_fg_minus_bg": outs[:4] + outs[-4:]}[mode]


def _module_labels(model, image, mode):
    """voleval._predict_volume (the nn.Module surface, batch by batch) on the volume filled up with zero slices to whole batches: the batches the predictor runs."""
    from pn2 import voleval as V
    D = image.shape[0]
    pad = (-D) % BATCH
    full = torch.cat([image, image.new_zeros((pad,) + tuple(image.shape[1:]))]) if pad else image
    return V._predict_volume(full, model, PATCH, lambda outs, single: V.predict_labels(_pick(outs, mode), mode), BATCH)[:D]


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("dual", [True, False], ids=["dual", "single"])
def test_volume_predictor_against_the_module_surface(dual, mode):
    """(i) the low-resolution maps the graph leaves, up-sampled by the unfused device op in the layout the model hands it (K dense channels: the bilinear kernel's
    instantiations round the four-tap expression differently), are the maps of model(xb) bit for bit (the identity pn2.infer.Predictor has for the binary models); (ii) the labels of a [5][80][80] volume - two batches, the second filled with three zero slices, resampled 80 -> 64 -> 80 - equal
    voleval._predict_volume on the same batches byte for byte; (iii) the two volume functions return voleval's lists for those labels, a single 2-D image takes
    the last map and its own B = 1 graph; (iv) fifty replays give the same bytes; (v) a volume of another size reuses the graphs; (vi) train mode is refused."""
    from pn2 import voleval as V
    from pn2.engine import Act, Engine, F32
    from pn2.infer import VolumePredictor
    model = _eval_model(dual, mode)
    vp = VolumePredictor(model, patch_size=PATCH, batch_size=BATCH)
    g = torch.Generator().manual_seed(31)
    # (i)
    xb = torch.randn(BATCH, 1, *PATCH, generator=g).to(dev)
    with torch.no_grad():
        ref = model(xb)
    lows = vp.lowres(xb)
    scales = [32, 16, 8, 4] * (2 if dual else 1)
    assert len(lows) == len(ref) == len(scales)
    eng = Engine(F32, False, need_grad=False)
    for i, (lo, s, r) in enumerate(zip(lows, scales, ref)):
        assert tuple(lo.shape) == (BATCH, 9, PATCH[0] // s, PATCH[1] // s) and lo.dtype == torch.float32
        dense = Act(eng, lo.permute(0, 2, 3, 1).contiguous(), 9, 9, 9, F32, requires_grad=False)          # [B][h][w][9], ld = 9: the layout of the model's head maps
        assert torch.equal(eng.to_nchw(eng.bilinear(dense, s)), r), i
    assert torch.equal(vp._labels(xb, "last")["labels"], V.predict_labels(ref[-1:], "last"))
    # (ii)
    image = torch.randn(5, 80, 80, generator=g).to(dev)
    label = torch.randint(0, 9, (5, 80, 80), generator=g).to(dev)
    modes = ["sum_fg", "sum_fg_minus_bg"] if dual else ["last"]
    want = {}
    for md in modes:
        want[md] = _module_labels(model, image, md)
        got = vp.predict(image, md)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (5, 80, 80)
        assert torch.equal(got, want[md]), md
    assert len(torch.unique(want[modes[0]])) > 1
    # (iii)
    assert vp.test_single_volume(image[None], label[None], 9, use_dual=dual) == V.volume_metrics(want[modes[0]], label, 9)
    assert vp.val_single_volume(image[None], label[None], 9, use_dual=dual) == V.volume_dice(want[modes[-1]], label, 9)
    nstates = len(vp._states)
    assert set(vp._states) == {(BATCH, *PATCH, md) for md in modes + ["last"]}
    img2, lab2 = image[0, :64, :64].contiguous(), label[0, :64, :64].contiguous()
    assert vp.test_single_volume(img2[None], lab2[None], 9, use_dual=True) == V.test_single_volume(img2[None], lab2[None], model, 9, patch_size=list(PATCH), use_dual=True)
    assert set(vp._states) - {(BATCH, *PATCH, md) for md in modes + ["last"]} == {(1, 64, 64, "last")}
    # (iv)
    first = vp._labels(xb, modes[0])["labels"].clone()
    for _ in range(50):
        assert torch.equal(vp._labels(xb, modes[0])["labels"], first)
    # (v)
    other = torch.randn(3, 72, 90, generator=g).to(dev)
    assert torch.equal(vp.predict(other, modes[0]), _module_labels(model, other, modes[0]))
    assert len(vp._states) == nstates + 1
    # (vi)
    model.train()
    with pytest.raises(RuntimeError, match="eval"):
        vp.predict(image, modes[0])
    with pytest.raises(RuntimeError, match="eval"):
        VolumePredictor(model, patch_size=PATCH, batch_size=BATCH).predict(image, modes[0])
    model.eval()


def test_volume_predictor_recaptures_after_a_trainer_moved_the_weights():
    """(vii) A Trainer built over the same model re-points every parameter into its flat arena and frees the old storage; the packed-panel table and the captured
    graphs hold the old pointers.  The next call must start over (the _check_weights rule of Predictor) and, the values being unchanged, return the same labels."""
    from pn2.infer import VolumePredictor
    from pn2.trainer import Trainer
    model = _eval_model(True, "bf16")
    vp = VolumePredictor(model, patch_size=PATCH, batch_size=BATCH)
    image = torch.randn(5, 64, 64, generator=torch.Generator().manual_seed(32)).to(dev)
    before = vp.predict(image, "sum_fg")
    old_cache, old_state = vp.pack_cache, vp._states[(BATCH, *PATCH, "sum_fg")]
    ptr = next(model.parameters()).data_ptr()
    tr = Trainer(model.train(), lr=1e-4, clip=None, weight_decay=1e-4, loss="mutation", hot=model.hot_parameters(True))
    model.eval()
    assert next(model.parameters()).data_ptr() != ptr
    junk = [torch.full((1 << 12,), 0xFF, dtype=torch.uint8, device=dev) for _ in range(256)]      # lands in the blocks the old weights gave back
    after = vp.predict(image, "sum_fg")
    assert vp.pack_cache is not old_cache and vp._states[(BATCH, *PATCH, "sum_fg")] is not old_state
    assert torch.equal(after, before)
    del junk, tr
