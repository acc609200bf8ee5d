"""GPU tests of the batched test-set evaluation: pn2_eval_tail_batch / pn2_eval_counts_batch / pn2_eval_wfm_batch (csrc/pn2_eval.hip) through
pn2.evaltail.postprocess_batch / eval_batch and pn2.infer.Predictor.test_with_eval, against the per-image entries (bit for bit) and the reference's
eval_for_testAllInOne values of tests/golden/eval_full.npz."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
os.environ.setdefault("PN2_NO_PRETRAINED", "1")
NAMES = ["meanDic", "meanIoU", "wFm", "Sm", "meanEm", "mae"]
TAGS = ("blob", "zero_pred", "exact", "full", "two", "rand352")
# target sizes of one ragged batch: an odd offset after the first, enlarge, identity (for 24 x 24 maps), a single pixel, shrink one axis and grow the other, empty
SHAPES = [(17, 23), (40, 31), (24, 24), (1, 1), (7, 50), None]
CANARY = 0xA5


def _dev():
    return torch.device("cuda", 0)


def _maps(h, w, B=6, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return [(3 * torch.randn(B, 1, h, w, generator=g)).to(_dev()) for _ in range(4)]


@pytest.mark.parametrize("maps", ["sum4", "last"])
@pytest.mark.parametrize("hw", [(24, 24), (16, 24)])
def test_tail_batch_bit_for_bit(hw, maps):
    """Every image's bytes equal pn2_add x3 -> pn2_bilinear_fwd -> pn2_eval_tail of that image's maps (evaltail.test_postprocess); the bytes between the images,
    after the last one and the empty slot keep their canaries; a second run on another stream gives the same bytes."""
    from pn2 import evaltail
    outs = _maps(*hw)
    live = [s for s in SHAPES if s is not None]
    total = sum(H * W for H, W in live) + 3 * (len(live) + 1)
    buf = torch.full((total + 16,), CANARY, dtype=torch.uint8, device=_dev())
    packed, views = evaltail.postprocess_batch(outs, SHAPES, maps=maps, gap=3, out=buf)
    assert views.total == total and views[5] is None and len(views) == 6
    torch.cuda.synchronize()
    zero = torch.zeros_like(outs[0][:1])
    mask = torch.ones(total + 16, dtype=torch.bool, device=_dev())
    for b, s in enumerate(SHAPES):
        if s is None:
            continue
        ref = evaltail.test_postprocess([o[b:b + 1] for o in outs] if maps == "sum4" else [outs[-1][b:b + 1], zero, zero, zero], s)
        assert views[b].shape == s and torch.equal(views[b], ref), (b, s, int((views[b] != ref).sum()))
        off = int(views.rows["off"][b])
        mask[off:off + s[0] * s[1]] = False
    assert bool((buf[mask] == CANARY).all())
    assert int(views[3][0, 0]) == 0          # one pixel: max == min
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    buf2 = torch.full_like(buf, CANARY)
    with torch.cuda.stream(side):
        evaltail.postprocess_batch(outs, SHAPES, maps=maps, gap=3, out=buf2)
    side.synchronize()
    assert torch.equal(buf, buf2)


def test_tail_batch_constant_image_and_plain_packing():
    from pn2 import evaltail
    outs = _maps(16, 24, B=3, seed=5)
    for o in outs:
        o[1] = 0.75          # a constant image: max == min -> all zeros
    packed, views = evaltail.postprocess_batch(outs, [(9, 9), (33, 20), (5, 7)])
    assert packed.numel() == 81 + 660 + 35 and int(views[1].max()) == 0 and int(views[0].max()) > 0
    assert views[2].data_ptr() == packed.data_ptr() + 81 + 660
    for b, s in enumerate([(9, 9), (33, 20), (5, 7)]):
        assert torch.equal(views[b], evaltail.test_postprocess([o[b:b + 1] for o in outs], s))


def test_eval_batch_vs_reference_and_per_image():
    """The six cases of eval_full.npz (64 x 80 four times, 100 x 77, 352 x 352) and a seventh image without foreground in ONE ragged batch: the reference's values
    within 1e-9 * max(1, |ref|); the integers of the per-image entries exactly; wFm equal to threshold_metrics(full=True) - the batch kernels keep every image's
    own block decomposition and the host sums the same partial sums in the same order, so equality is asserted, not the 1e-11 a reordered sum would need."""
    from pn2 import evaltail
    from pn2.capi import call
    from oracle import pranet_oracle as O
    z = np.load(os.path.join(G, "eval_full.npz"))
    preds = [torch.from_numpy(z[t + "_pred"]).to(_dev()) for t in TAGS] + [torch.from_numpy(z["blob_pred"]).to(_dev())]
    gts = [torch.from_numpy(z[t + "_gt"]).to(_dev()) for t in TAGS] + [torch.zeros(z["blob_gt"].shape, dtype=torch.float32, device=_dev())]
    assert [tuple(p.shape) for p in preds] == [(64, 80)] * 4 + [(100, 77), (352, 352), (64, 80)]
    packed, views = evaltail.pack_batch(preds)
    counts = {}
    rows = evaltail.eval_batch({"metrics": NAMES}, packed, views, gts, counts=counts)
    assert rows.shape == (7, 6)
    for i, tag in enumerate(TAGS):
        for k, (got, ref) in enumerate(zip(rows[i], z[tag + "_vals"])):
            assert abs(got - float(ref)) <= 1e-9 * max(1.0, abs(float(ref))), (tag, NAMES[k], got, float(ref))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        o = O.full_metrics(z["blob_pred"], np.zeros_like(z["blob_gt"]))
    assert np.isnan(rows[6][2]) and abs(rows[6][3] - o["Sm"]) < 1e-12 and abs(rows[6][4] - o["meanEm"]) < 1e-12
    P = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for i, (p, g) in enumerate(zip(preds, gts)):
        g = g.float().contiguous()
        hist = torch.empty(512, dtype=torch.int32, device=_dev())
        q25 = torch.empty(25, dtype=torch.int64, device=_dev())
        call.pn2_eval_hist(P(p), P(g), p.numel(), P(hist), st)
        call.pn2_eval_region_sums(P(p), P(g), p.shape[0], p.shape[1], P(q25), st)
        assert np.array_equal(counts["hist"][i], hist.cpu().numpy()) and np.array_equal(counts["out25"][i], q25.cpu().numpy()), i
        r = evaltail.threshold_metrics(p, g, full=True)
        assert np.array_equal(rows[i], np.array([r[k] for k in NAMES]), equal_nan=True), (i, rows[i], [r[k] for k in NAMES])
    # a subset of the metrics: no wFm work, no region sums, the same values in the asked order
    sub = evaltail.eval_batch({"metrics": ["mae", "meanEm", "meanDic"]}, packed, views, gts, counts=counts)
    assert np.array_equal(sub, rows[:, [5, 4, 0]]) and counts["out25"] is None and counts["sums"] is None
    # the ground truths as one packed buffer
    again = evaltail.eval_batch({"metrics": NAMES}, packed, views, torch.cat([g.float().reshape(-1) for g in gts]))
    assert np.array_equal(again, rows, equal_nan=True)


def test_batch_entries_check_their_arguments():
    """-1 for a null pointer or an empty size, -2 outside the built range, and nothing launched: the device is still fine afterwards."""
    from pn2 import capi, evaltail
    lib = capi.load()
    dev = _dev()
    rows, total = evaltail.ragged_table([(5, 6), (4, 4)], 8, 8)
    tab = torch.from_numpy(rows.view(np.uint8).reshape(-1).copy()).to(dev)
    m = torch.zeros(2, 8, 8, device=dev)
    out = torch.zeros(total, dtype=torch.uint8, device=dev); gt = torch.zeros(total, device=dev)
    mm = torch.zeros(4, dtype=torch.int32, device=dev)
    hist = torch.zeros(2 * 512, dtype=torch.int32, device=dev); q = torch.zeros(50, dtype=torch.int64, device=dev)
    K = torch.zeros(49, dtype=torch.float64, device=dev); wi = torch.zeros(total, dtype=torch.int32, device=dev)
    wd = torch.zeros(2 * total, dtype=torch.float64, device=dev); part = torch.zeros(2 * 2048 * 2, dtype=torch.float64, device=dev)
    P = lambda t: C.c_void_p(t.data_ptr())
    ptrs = lambda n: (C.c_void_p * n)(*[m.data_ptr()] * n)
    big = 60 * 1024 // 4 + 1
    tail = lambda **k: lib.pn2_eval_tail_batch(*[k.get(n, d) for n, d in (("maps", ptrs(4)), ("nmaps", 4), ("B", 2), ("h", 8), ("w", 8), ("tab", P(tab)), ("maxH", 5), ("maxW", 6),
                                                                            ("total", total), ("out", P(out)), ("mm", P(mm)), ("st", None))])
    cnt = lambda **k: lib.pn2_eval_counts_batch(*[k.get(n, d) for n, d in (("pred", P(out)), ("gt", P(gt)), ("tab", P(tab)), ("B", 2), ("maxH", 5), ("maxW", 6), ("total", total),
                                                                             ("hist", P(hist)), ("q", P(q)), ("st", None))])
    wfm = lambda **k: lib.pn2_eval_wfm_batch(*[k.get(n, d) for n, d in (("pred", P(out)), ("gt", P(gt)), ("tab", P(tab)), ("B", 2), ("maxH", 5), ("maxW", 6), ("total", total),
                                                                          ("K", P(K)), ("c5", -0.1), ("wi", P(wi)), ("wd", P(wd)), ("part", P(part)), ("st", None))])
    assert tail(maps=None) == -1 and tail(tab=None) == -1 and tail(out=None) == -1 and tail(mm=None) == -1 and tail(maps=(C.c_void_p * 4)(m.data_ptr(), None, None, None)) == -1
    assert tail(B=0) == -1 and tail(h=0) == -1 and tail(maxH=0) == -1 and tail(total=0) == -1
    assert tail(nmaps=2) == -2 and tail(nmaps=0) == -2 and tail(maxW=big) == -2 and tail(B=65536) == -2
    assert cnt(pred=None) == -1 and cnt(gt=None) == -1 and cnt(tab=None) == -1 and cnt(hist=None) == -1 and cnt(B=0) == -1 and cnt(maxW=0) == -1
    assert cnt(maxW=big) == -2 and cnt(B=65536) == -2
    assert wfm(pred=None) == -1 and wfm(K=None) == -1 and wfm(wi=None) == -1 and wfm(wd=None) == -1 and wfm(part=None) == -1 and wfm(B=0) == -1
    assert wfm(maxW=big) == -2
    torch.cuda.synchronize()
    assert int(out.sum()) == 0 and int(hist.sum()) == 0 and int(mm.sum()) == 0          # nothing ran
    assert tail() == 0 and cnt() == 0 and wfm() == 0 and cnt(q=None) == 0
    torch.cuda.synchronize()
    # the Python wrappers have no CPU path
    cpu = [torch.zeros(1, 1, 8, 8)] * 4
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evaltail.postprocess_batch(cpu, [(5, 6)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evaltail.pack_batch([torch.zeros(4, 4, dtype=torch.uint8)])
    packed, views = evaltail.pack_batch([torch.zeros(4, 4, dtype=torch.uint8, device=dev)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evaltail.eval_batch({"metrics": ["mae"]}, packed, views, [torch.zeros(4, 4)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evaltail.eval_batch({"metrics": ["mae"]}, packed.cpu(), views, [torch.zeros(4, 4, device=dev)])


def _loader(n, S, shapes, seed):
    """(image [1][3][S][S], gt, name) as utils.dataloader.test_dataset.load_data yields them; gt: blobs with values in {0, 255} (scaled by test_with_eval)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    items = []
    for i in range(n):
        H, W = shapes[i]
        gt = np.zeros((H, W), dtype=np.float32)
        gt[H // 4:max(H // 4 + 1, 3 * H // 4), W // 3:max(W // 3 + 1, 2 * W // 3)] = 255.0
        items.append((torch.randn(1, 3, S, S, generator=g), gt, f"{i}.png"))
    return items


def test_predictor_test_with_eval_end_to_end():
    """Predictor.test_with_eval over 5 images at batch size 3 (the second batch has a filler slot) == image by image the per-image tail and eval_for_testAllInOne on
    slices of the SAME batched maps pred(images); a second pass returns the same arrays and captures no new graph."""
    import pn2
    from pn2 import evaltail
    from pn2.infer import Predictor
    from lib.pranet import PraNet_V2
    from oracle import weights as W
    dev = _dev()
    was = pn2.get_compute_dtype()
    pn2.set_compute_dtype("fp32")
    try:
        model = PraNet_V2(num_class=1)
        model.load_state_dict(W.make_state_dict(W.manifest_pranet_v2(1), seed=0, bn3_gamma=0.05), strict=True)
        model = model.to(dev).eval()
        pred = Predictor(model)
        shapes = [(34, 46), (80, 62), (64, 64), (2, 2), (14, 100)]          # the list of the tail test, scaled up
        items = _loader(5, 64, shapes, seed=11)
        opt = {"metrics": NAMES}
        res_i, mean = pred.test_with_eval(items, opt, batch_size=3)
        assert res_i.shape == (5, 6) and np.array_equal(mean, np.mean(res_i, axis=0), equal_nan=True)
        n_states = len(pred._states)
        assert n_states == 1
        for lo in (0, 3):
            chunk = items[lo:lo + 3]
            x = torch.cat([it[0] for it in chunk]).to(dev)
            if len(chunk) < 3:
                x = torch.cat([x, x.new_zeros((3 - len(chunk), 3, 64, 64))])
            outs = [o.clone() for o in pred(x)]
            packed, views = pred.postprocess_batch(x, [shapes[lo + b] for b in range(len(chunk))])
            assert len(views) == 3 and (len(chunk) == 3 or views[2] is None)
            for b, (_, gt, _) in enumerate(chunk):
                u8 = evaltail.test_postprocess([o[b:b + 1] for o in outs[:4]], gt.shape)
                assert torch.equal(views[b], u8), (lo, b)
                g = gt / (gt.max() + 1e-8)
                ref = evaltail.eval_for_testAllInOne(opt, u8, torch.from_numpy(g).to(dev))
                assert np.array_equal(res_i[lo + b], np.array(ref), equal_nan=True), (lo, b, res_i[lo + b], ref)
        res2, mean2 = pred.test_with_eval(items, opt, batch_size=3)
        assert np.array_equal(res2, res_i, equal_nan=True) and np.array_equal(mean2, mean, equal_nan=True) and len(pred._states) == n_states
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pred.evaluate(torch.zeros(3, 3, 64, 64, device=dev), [torch.zeros(5, 5)], opt)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pred.postprocess_batch(torch.zeros(3, 3, 64, 64), [(5, 5)])
        model.train()
        with pytest.raises(RuntimeError, match="eval"):
            Predictor(model).postprocess_batch(torch.zeros(3, 3, 64, 64, device=dev), [(5, 5)])
    finally:
        pn2.set_compute_dtype(was)


def test_predictor_last_map_of_the_v1_model():
    """maps="last" on lib.PraNet_Res2Net.PraNet (MyTest_med.py:98-102 takes res2, the last of its four maps, alone): one batch against the per-image chain."""
    import pn2
    from pn2 import evaltail
    from pn2.infer import Predictor
    from lib.PraNet_Res2Net import PraNet
    from oracle import weights as W
    dev = _dev()
    was = pn2.get_compute_dtype()
    pn2.set_compute_dtype("fp32")
    try:
        model = PraNet()
        model.load_state_dict(W.make_state_dict(W.manifest_pranet_v1(), seed=1), strict=True)
        pred = Predictor(model.to(dev).eval())
        x = torch.randn(2, 3, 96, 96, generator=torch.Generator(device="cpu").manual_seed(3)).to(dev)
        shapes = [(51, 69), (80, 31)]
        outs = [o.clone() for o in pred(x)]
        packed, views = pred.postprocess_batch(x, shapes, maps="last")
        zero = torch.zeros_like(outs[-1][:1])
        for b, s in enumerate(shapes):
            assert torch.equal(views[b], evaltail.test_postprocess([outs[-1][b:b + 1], zero, zero, zero], s)), b
        one = pred.postprocess(x[:1], shapes[0], maps="last")
        assert one.shape == shapes[0] and one.dtype == torch.uint8
    finally:
        pn2.set_compute_dtype(was)
