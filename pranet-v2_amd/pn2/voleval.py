"""Multi-class volume evaluation of the reference's test_synapse.py / trainer.py:inference on the GPU (multiclass_seg/EMCAD/utils/utils.py:140-301):
label maps from the K-channel logits, per-class voxel counts, and medpy's surface distances as exact histograms over the squared voxel distance
(csrc/pn2_seg.hip).  The four reported numbers - Dice, HD95, Jaccard, ASD - are finished on the host in float64 from those integers with the
expressions of medpy.metric.binary (dc, hd95, jc, assd).  GPU tensors only: there is no CPU fallback."""
import ctypes as C

import torch

from .capi import call, SegUpMap
from .core import _p, _stream
from .volinput import zoom

MODES = {"last": 0, "sum_fg": 1, "sum_fg_minus_bg": 2}
VIEWS = {"id": 0, "h": 1, "v": 2, "hv": 3}          # view codes of pn2_seg_labels_up_tta / pn2_flip_views: bit 0 = x mirrored, bit 1 = y mirrored
AVERAGES = {"logit": 0, "prob": 1}
MAX_AXIS = 1024


def _need_gpu(*ts):
    if not all(t.is_cuda for t in ts):
        raise RuntimeError("pn2.voleval needs GPU tensors (no CPU fallback)")


def predict_labels(outs, mode):
    """outs: 1..8 NCHW fp32 maps [N][K][H][W] as the model returns them, 2 <= K <= 16.  Returns uint8 [N][H][W]: the argmax over K of
      'last'             outs[-1]                                                   (utils.py:193,271)
      'sum_fg'           0.0 + outs[0] + outs[1] + ...                              (:188-190; pass the foreground maps)
      'sum_fg_minus_bg'  0.0 + (outs[0] - outs[h]) + (outs[1] - outs[h+1]) + ...    (:265-267; foreground maps, then as many background maps)
    in fp32 in this order; the lowest index wins a tie, as in torch.argmax.  The argmax is taken of the logits, not of their fp32 softmax."""
    if mode not in MODES:
        raise ValueError(f"mode {mode!r}: one of {sorted(MODES)}")
    outs = list(outs)
    _need_gpu(*outs)
    if not 1 <= len(outs) <= 8 or (mode == "sum_fg_minus_bg" and len(outs) % 2):
        raise ValueError("1..8 maps (an even number for sum_fg_minus_bg)")
    shape = tuple(outs[0].shape)
    if len(shape) != 4 or not 2 <= shape[1] <= 16 or any(tuple(o.shape) != shape or o.dtype != torch.float32 for o in outs):
        raise ValueError("maps must be fp32 [N][K][H][W] of one shape with 2 <= K <= 16")
    outs = [o.detach().contiguous() for o in outs]
    N, K, H, W = shape
    out = torch.empty((N, H, W), dtype=torch.uint8, device=outs[0].device)
    ptrs = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
    call.pn2_seg_labels(ptrs, len(outs), MODES[mode], N, K, H, W, _p(out), _stream())
    return out


def predict_labels_up(maps, scales, mode, out=None):
    """predict_labels of the maps up-sampled bilinearly (align_corners=False) by their integer `scales`, in one launch and without the full-resolution maps
    (pn2_seg_labels_up): maps are 1..8 NHWC fp32 tensors [N][h][w][K], 2 <= K <= 16, each of its own size with h * scale, w * scale the same for all.  The last
    axis may be a slice of a wider, channel-padded one (t[..., :K]): only its stride has to be 1.  Returns uint8 [N][h * scale][w * scale] (written into `out` if given)."""
    descs, N, K, OH, OW, dev = _up_descs(maps, scales, mode)
    out = _labels_out(out, (N, OH, OW), dev)
    call.pn2_seg_labels_up(descs, len(descs), MODES[mode], N, K, OH, OW, _p(out), _stream())
    return out


def _up_descs(maps, scales, mode):
    """The checked descriptor table of predict_labels_up / predict_labels_up_tta -> (table, samples in the maps, K, OH, OW, device)."""
    if mode not in MODES:
        raise ValueError(f"mode {mode!r}: one of {sorted(MODES)}")
    maps, scales = [m.detach() for m in maps], [int(s) for s in scales]
    _need_gpu(*maps)
    if not 1 <= len(maps) <= 8 or len(scales) != len(maps) or (mode == "sum_fg_minus_bg" and len(maps) % 2):
        raise ValueError("1..8 maps (an even number for sum_fg_minus_bg), one scale for each")
    N, _, _, K = maps[0].shape if maps[0].dim() == 4 else (0, 0, 0, 0)
    OH, OW = maps[0].shape[1] * scales[0], maps[0].shape[2] * scales[0]
    descs = (SegUpMap * len(maps))()
    for d, m, s in zip(descs, maps, scales):
        if m.dim() != 4 or m.dtype != torch.float32 or m.shape[0] != N or m.shape[3] != K or not 2 <= K <= 16 or s < 1 or (m.shape[1] * s, m.shape[2] * s) != (OH, OW):
            raise ValueError("maps must be fp32 [N][h][w][K] with 2 <= K <= 16 and one output size h * scale, w * scale")
        ld = m.stride(2)
        if m.stride(3) != 1 or ld < K or m.stride(1) != m.shape[2] * ld or m.stride(0) != m.shape[1] * m.shape[2] * ld:
            raise ValueError("maps must be dense NHWC up to a padded channel axis")
        d.p, d.ld, d.H, d.W = m.data_ptr(), ld, m.shape[1], m.shape[2]
    return descs, N, K, OH, OW, maps[0].device


def _labels_out(out, shape, device):
    if out is None:
        return torch.empty(shape, dtype=torch.uint8, device=device)
    if out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_contiguous() or not out.is_cuda:
        raise ValueError(f"out must be a contiguous uint8 GPU tensor {shape}")
    return out


def parse_tta(tta):
    """The `tta` argument of pn2.infer.VolumePredictor -> None or the tuple of view names: None; "flips" = ("id", "h", "v"), the three views of the reference's
    tta_model (utils.py:311-325); or a non-empty tuple / list of names from VIEWS without repeats.  Anything else raises ValueError."""
    if tta is None:
        return None
    if isinstance(tta, str):
        if tta != "flips":
            raise ValueError(f"tta {tta!r}: None, 'flips' or a tuple of views from {sorted(VIEWS)}")
        return ("id", "h", "v")
    if not isinstance(tta, (tuple, list)) or not 1 <= len(tta) <= len(VIEWS) or any(not isinstance(v, str) or v not in VIEWS for v in tta):
        raise ValueError(f"tta {tta!r}: None, 'flips' or a tuple of views from {sorted(VIEWS)}")
    if len(set(tta)) != len(tta):
        raise ValueError(f"tta {tta!r}: a view is listed twice")
    return tuple(tta)


def _view_codes(views):
    views = parse_tta(views)
    if views is None:
        raise ValueError("views: 'flips' or a tuple of views, not None")
    return views, (C.c_int * len(views))(*[VIEWS[v] for v in views])


def flip_views(x, views, out=None):
    """x: fp32 [N][h][w] (or [N][1][h][w]) on the GPU -> [V * N] samples of the same trailing shape: view v of sample n at v * N + n, mirrored as its name in
    VIEWS says (pn2_flip_views: one launch, raw bits)."""
    views, codes = _view_codes(views)
    _need_gpu(x)
    if x.dtype != torch.float32 or x.dim() not in (3, 4) or (x.dim() == 4 and x.shape[1] != 1) or not x.is_contiguous() or x.numel() == 0:
        raise ValueError("x must be a contiguous non-empty fp32 [N][h][w] or [N][1][h][w] tensor")
    shape = (len(views) * x.shape[0],) + tuple(x.shape[1:])
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous() or not out.is_cuda:
        raise ValueError(f"out must be a contiguous fp32 GPU tensor {shape}")
    call.pn2_flip_views(_p(x), x.shape[0], x.shape[-2], x.shape[-1], codes, len(views), _p(out), _stream())
    return out


def predict_labels_up_tta(maps, scales, mode, views, average="prob", out=None):
    """predict_labels_up under flip test-time augmentation, still one launch (pn2_seg_labels_up_tta).  The maps hold V * N samples, view v of sample n at v * N + n
    (the layout flip_views writes); `views` are names from VIEWS ("id", "h": x mirrored, "v": y mirrored, "hv": both), each at most once.  Every view's combined
    logits are read at the mirrored output pixel - the value that up-sampling the view's maps and flipping back gives - and the views are added in their order:
    average="logit" adds the combined logits, average="prob" their softmax over K (the reference's mean of predicted masks).  The sum is not divided by V: the
    argmax does not see it.  Returns uint8 [N][h * scale][w * scale]."""
    if average not in AVERAGES:
        raise ValueError(f"average {average!r}: one of {sorted(AVERAGES)}")
    views, codes = _view_codes(views)
    descs, VN, K, OH, OW, dev = _up_descs(maps, scales, mode)
    if VN % len(views):
        raise ValueError(f"{VN} samples in the maps are not a multiple of the {len(views)} views")
    N = VN // len(views)
    out = _labels_out(out, (N, OH, OW), dev)
    call.pn2_seg_labels_up_tta(descs, len(descs), MODES[mode], codes, len(views), AVERAGES[average], N, K, OH, OW, _p(out), _stream())
    return out


def _volumes(pred, label, classes):
    _need_gpu(pred, label)
    if pred.shape != label.shape or pred.dim() not in (2, 3):
        raise ValueError("pred and label must be [D][H][W] or [H][W] label volumes of one shape")
    if not 2 <= int(classes) <= 256:
        raise ValueError("2 <= classes <= 256")
    if max(pred.shape) > MAX_AXIS:
        raise ValueError(f"volume {tuple(pred.shape)}: every axis must be <= {MAX_AXIS}")
    return pred.to(torch.uint8).contiguous(), label.to(torch.uint8).contiguous()


def class_counts(pred, label, classes):
    """int64 ndarray [classes][3] = |pred = c|, |label = c|, |pred = c and label = c| (one kernel, one copy to the host)."""
    p, g = _volumes(pred, label, classes)
    cnt = torch.empty((int(classes), 3), dtype=torch.int64, device=p.device)
    call.pn2_seg_counts(_p(p), _p(g), p.numel(), int(classes), _p(cnt), _stream())
    return cnt.cpu().numpy()


def surface_histograms(pred, label, cls_list):
    """For every class c of cls_list both directions of medpy's __surface_distances as histograms over the squared distance:
    -> {c: (hist pred->label, hist label->pred, border voxels of pred, border voxels of label)} with int64 ndarrays.  All launches first, one copy to the host."""
    import numpy as np
    p, g = _volumes(pred, label, 256)
    ndim = p.dim()
    D, H, W = (1,) * (3 - ndim) + tuple(p.shape)
    cls_list = list(cls_list)
    if not cls_list:
        return {}
    L = int(call.pn2_seg_surface_hist_len(D, H, W))
    nbytes = C.c_longlong(0)
    call.pn2_seg_surface_workspace(D, H, W, ndim, C.byref(nbytes))
    work = torch.empty(int(nbytes.value), dtype=torch.uint8, device=p.device)
    hist = torch.empty((len(cls_list), 2, L), dtype=torch.int32, device=p.device)
    cnt = torch.empty((len(cls_list), 2, 2), dtype=torch.int32, device=p.device)
    st = _stream()
    for i, c in enumerate(cls_list):
        call.pn2_seg_surface_hist(_p(p), _p(g), D, H, W, int(c), ndim, _p(hist[i, 0]), _p(cnt[i, 0]), _p(work), st)
        call.pn2_seg_surface_hist(_p(g), _p(p), D, H, W, int(c), ndim, _p(hist[i, 1]), _p(cnt[i, 1]), _p(work), st)
    h, n = hist.cpu().numpy().astype(np.int64), cnt.cpu().numpy().astype(np.int64)
    out = {}
    for i, c in enumerate(cls_list):
        out[c] = (h[i, 0], h[i, 1], int(n[i, 0, 0]), int(n[i, 0, 1]))
    return out


def _hd95_asd(h_ab, h_ba):
    """medpy's hd95 = numpy.percentile(hstack(d(A->B), d(B->A)), 95) (linear interpolation) and assd = mean(mean d(A->B), mean d(B->A)) from the two
    d^2 histograms: the sorted distances are the bins of the merged histogram repeated by their counts, each value sqrt(float64(d^2)) as
    scipy's distance_transform_edt returns it."""
    import numpy as np
    merged = h_ab + h_ba
    bins = np.nonzero(merged)[0]
    cum = np.cumsum(merged[bins])
    n = int(cum[-1])
    vals = np.sqrt(bins.astype(np.float64))
    pos = np.float64(95) / 100 * (n - 1)                 # numpy's 'linear' method: virtual index q * (n - 1)
    lo = int(np.floor(pos))
    t = pos - lo
    a = vals[np.searchsorted(cum, lo, side="right")]
    b = vals[np.searchsorted(cum, min(lo + 1, n - 1), side="right")]
    hd95 = a + (b - a) * t if t < 0.5 else b - (b - a) * (1 - t)          # numpy's _lerp
    means = []
    for h in (h_ab, h_ba):
        k = np.nonzero(h)[0]
        means.append(float((h[k] * np.sqrt(k.astype(np.float64))).sum()) / int(h.sum()))
    return float(hd95), float(np.mean(means))


def volume_metrics(pred, label, classes):
    """calculate_metric_percase(pred == c, label == c) for c = 1 .. classes-1 (utils.py:140-152, :232-234): a list of (dice, hd95, jaccard, asd).
    pred has voxels and label none -> (1, 0, 1, 0); pred empty -> (0, 0, 0, 0); no distance pass runs for those classes."""
    cnt = class_counts(pred, label, classes)
    live = [c for c in range(1, int(classes)) if cnt[c, 0] > 0 and cnt[c, 1] > 0]
    hists = surface_histograms(pred, label, live)
    out = []
    for c in range(1, int(classes)):
        p, g, i = (int(v) for v in cnt[c])
        if p > 0 and g > 0:
            hd95, asd = _hd95_asd(hists[c][0], hists[c][1])
            out.append((2. * i / float(p + g), hd95, float(i) / float(p + g - i), asd))
        elif p > 0:
            out.append((1, 0, 1, 0))
        else:
            out.append((0, 0, 0, 0))
    return out


def volume_dice(pred, label, classes):
    """calculate_dice_percase(pred == c, label == c) for c = 1 .. classes-1 (utils.py:154-163, :298-300): needs the voxel counts only."""
    cnt = class_counts(pred, label, classes)
    out = []
    for c in range(1, int(classes)):
        p, g, i = (int(v) for v in cnt[c])
        out.append(2. * i / float(p + g) if p > 0 and g > 0 else (1 if p > 0 else 0))
    return out


def _predict_volume(image, net, patch_size, mode, batch_size):
    """The slices of image [D][H][W] (or one [H][W] image) through net.eval() under no_grad in batches -> uint8 label volume of the same shape.
    `mode(outs)` picks the maps and the combination for predict_labels.  Slices whose size differs from patch_size are resampled as the reference does
    (utils.py:179-181,197-198) - scipy's zoom of order 3 going in, of order 0 coming out - on the device, batch by batch (pn2/volinput.py)."""
    _need_gpu(image)
    net.eval()
    x = image.float()
    if x.dim() == 2:
        with torch.no_grad():
            return mode(net(x[None, None].contiguous()), True)[0]
    D, H, W = x.shape
    ph, pw = int(patch_size[0]), int(patch_size[1])
    preds = []
    with torch.no_grad():
        for i in range(0, D, batch_size):
            xb = zoom(x[i:i + batch_size], (ph, pw), 3)
            preds.append(zoom(mode(net(xb[:, None].contiguous()), False), (H, W), 0))
    return torch.cat(preds)


def test_single_volume(image, label, net, classes, patch_size=[256, 256], use_dual=None, batch_size=16):
    """utils.py:165-246 without the plotting / saving arguments: image, label [1][D][H][W] (or [1][H][W]) GPU tensors -> the list of
    (dice, hd95, jaccard, asd) for the classes 1 .. classes-1.  Dual models are combined as sum of the four foreground maps, others take the last map;
    a single 2-D image takes the last map whatever use_dual says, as the reference does (:224-231).  One net call per batch of slices."""
    image, label = image.squeeze(0), label.squeeze(0)

    def mode(outs, single_image):
        return predict_labels(outs[:4], "sum_fg") if use_dual and not single_image else predict_labels(outs[-1:], "last")
    pred = _predict_volume(image, net, patch_size, mode, batch_size)
    return volume_metrics(pred, label, classes)


def val_slices(images, labels, net_or_predictor, img_size, mode, batch_size=16, tta=None, tta_average="prob"):
    """The val() loop of multiclass_seg/MIST/ACDC_train_test.py:48-93 over single slices of differing sizes: images a list of fp32 [x_i][y_i] slices, labels a list
    of uint8 label maps of the same shapes (all host arrays or all GPU tensors).  Per batch of slices: the ragged spline zoom to img_size x img_size (a slice of that
    size is not resampled, :59), the captured eval forward and label launch of a pn2.infer.VolumePredictor in one of its MODES (the reference sums P - P_bg over the
    map pairs for a dual model, 'sum_fg_minus_bg', and its maps otherwise, 'sum_fg'), the order-0 zoom of the labels back to every slice's own size (:82-83) and the
    three counts of medpy's binary dc(prediction, label) (:87), which treats every non-zero label as foreground.
    Returns (per-slice Dice 2 I / (A + B) as float64 ndarray, 0.0 where A + B = 0; their mean, val()'s `performance`).  A net is wrapped in a VolumePredictor of its
    own (with flip test-time augmentation if `tta` is given: VolumePredictor's arguments); pass a VolumePredictor (patch_size (img_size, img_size)) to keep its
    graphs between calls - its own tta setting then holds."""
    import numpy as np
    from . import volinput as V
    from .infer import VolumePredictor
    if mode not in MODES:
        raise ValueError(f"mode {mode!r}: one of {sorted(MODES)}")
    if not torch.cuda.is_available():
        raise RuntimeError("pn2.voleval needs a GPU (no CPU fallback)")
    images, labels = list(images), list(labels)
    if not images or len(images) != len(labels):
        raise ValueError("one label map per slice, at least one slice")
    S = int(img_size)
    vp = net_or_predictor if isinstance(net_or_predictor, VolumePredictor) else VolumePredictor(net_or_predictor, (S, S), batch_size, tta=tta, tta_average=tta_average)
    if vp.patch_size != (S, S):
        raise ValueError(f"the predictor's patch size {vp.patch_size} is not {(S, S)}")
    B = vp.batch_size
    counts = []
    for i in range(0, len(images), B):
        ims, gts = images[i:i + B], labels[i:i + B]
        sizes = [tuple(int(a) for a in im.shape) for im in ims]
        if any(tuple(g.shape) != s for g, s in zip(gts, sizes)):
            raise ValueError("a label map whose shape differs from its slice's")
        xb = V.zoom_ragged(ims, (S, S), 3)
        n = xb.shape[0]
        if n < B:          # one graph serves every batch: zero slices fill the last one (eval-mode BatchNorm keeps the samples independent)
            xb = torch.cat([xb, xb.new_zeros((B - n, S, S))])
        lab = vp._labels(xb[:, None], mode)["labels"][:n]
        pred, _, plan = V._unzoom(lab, sizes)
        gt, _, off, _keep = V._gather_slices(gts, torch.uint8, "labels")
        if off is not None:          # GPU tensors of their own: packed in the order of the predictions
            gt = torch.cat([g.reshape(-1) for g in _keep])
        counts.append(V._dice_counts_dev(pred, gt, sizes, plan))
    cnt = torch.cat(counts).cpu().numpy()          # one copy, after the last batch is queued
    both = cnt[:, 1] + cnt[:, 2]
    dice = np.where(both > 0, 2.0 * cnt[:, 0] / np.maximum(both, 1).astype(np.float64), 0.0)
    dc_sum = 0
    for v in dice:          # :87-88: summed slice by slice, in the loader's order
        dc_sum += float(v)
    return dice, dc_sum / len(dice)


def val_single_volume(image, label, net, classes, patch_size=[256, 256], use_dual=False, batch_size=16):
    """utils.py:248-301: the in-training validation -> the list of Dice values for the classes 1 .. classes-1.  Dual models are combined as
    sum of (foreground - background) over the four map pairs, others take the last map."""
    image, label = image.squeeze(0), label.squeeze(0)

    def mode(outs, single_image):
        return predict_labels(list(outs[:4]) + list(outs[-4:]), "sum_fg_minus_bg") if use_dual else predict_labels(outs[-1:], "last")
    pred = _predict_volume(image, net, patch_size, mode, batch_size)
    return volume_dice(pred, label, classes)
