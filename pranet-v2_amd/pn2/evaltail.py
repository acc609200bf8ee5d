"""Inference tail of the reference's MyTest_med.py:104-111 on the GPU: res = p2+p3+p4+p5 -> bilinear resize to the
ground-truth size (align_corners=False) -> sigmoid -> min-max normalise -> uint8.

Two paths compute the same bytes and the same metrics: one image at a time (test_postprocess, threshold_metrics, eval_for_testAllInOne) and a ragged batch of
images whose ground truths all differ in size (postprocess_batch, eval_batch: csrc/pn2_eval.hip, second half).  Both finish in metrics_from_counts."""
import ctypes as C

import numpy as np
import torch

from .capi import call, F32
from .engine import Engine, Act, _p, _stream

WFM_MAX_BLOCKS = 2048          # PN2_EVAL_WFM_MAX_BLOCKS (include/pn2.h): rows of one image in the batch entry's `part`
# one row of the device table of the batch entries (pn2_eval_img, include/pn2.h)
ROW = np.dtype([("H", "<i4"), ("W", "<i4"), ("off", "<i8"), ("rh", "<f4"), ("rw", "<f4")])


def test_postprocess(outs, gt_shape):
    """outs: the model's 8-tuple (or its first four fg maps), each (1,1,h,w) fp32 on the GPU.  Returns a uint8 (H,W) GPU tensor."""
    eng = Engine(F32, training=False, need_grad=False)
    acts = []
    for o in outs[:4]:
        if not o.is_cuda:
            raise RuntimeError("pn2.evaltail needs GPU tensors (no CPU fallback)")
        n, k, h, w = o.shape
        assert n == 1 and k == 1
        acts.append(Act(eng, o.float().contiguous().reshape(1, h, w, 1), 1, 1, 1, F32, requires_grad=False))
    s = eng.add(eng.add(eng.add(acts[0], acts[1]), acts[2]), acts[3])
    r = eng.resize_to(s, int(gt_shape[0]), int(gt_shape[1]), align_corners=False)
    n = r.M
    out = torch.empty((int(gt_shape[0]), int(gt_shape[1])), dtype=torch.uint8, device=r.t.device)
    scratch = torch.empty(2 + 2 * 512, dtype=torch.float32, device=r.t.device)
    call.pn2_eval_tail(r.ptr, _p(out), _p(scratch), n, _stream())
    return out


def threshold_metrics(pred_u8, gt, full=False):
    """full=True: also meanEm, Sm and wFm - with meanDic / meanIoU / mae the complete opt["metrics"] set of the reference's eval_for_testAllInOne
    (eval.py:18-66); pred_u8 / gt are then 2-D maps (H, W).
    The reference's 256-threshold sweep (eval.py:22-50, Fmeasure_calu eval_functions.py:131-166) for one uint8 prediction map and its
    ground truth, both on the GPU.  One histogram kernel reads the maps; the 256x6 curves (precision, recall, specificity, Dice,
    F-measure, IoU) are then finished on the host in float64 with the reference's expressions, so they equal its numpy result exactly.
    Returns {"curves": ndarray[256, 6], "meanDic", "meanIoU", "meanSen", "meanSpe", "meanFm", "mae"}."""
    if not (pred_u8.is_cuda and gt.is_cuda):
        raise RuntimeError("pn2.evaltail needs GPU tensors (no CPU fallback)")
    if pred_u8.dtype != torch.uint8 or pred_u8.numel() != gt.numel():
        raise ValueError("pred must be uint8 with as many pixels as gt")
    p = pred_u8.contiguous()
    g = gt.float().contiguous()
    hist = torch.empty(512, dtype=torch.int32, device=p.device)
    call.pn2_eval_hist(_p(p), _p(g), p.numel(), _p(hist), _stream())
    h = hist.cpu().numpy().astype(np.int64)
    h_all, h_gt = h[:256], h[256:]
    if not full:
        return metrics_from_counts(h_all, h_gt, full=False)
    H, W = int(p.shape[-2]), int(p.shape[-1])
    N, num_obj = int(h_all.sum()), int(h_gt.sum())
    out25 = sums = None
    if 0 < num_obj < N:          # (StructureMeasure needs no regions for an empty or a full ground truth)
        q25 = torch.empty(25, dtype=torch.int64, device=p.device)
        call.pn2_eval_region_sums(_p(p), _p(g), H, W, _p(q25), _stream())
        out25 = [int(v) for v in q25.cpu()]
    if num_obj:
        Kd = torch.from_numpy(np.ascontiguousarray(gauss7())).to(p.device)
        nblk = int(call.pn2_eval_wfm_blocks(H, W))
        wi = torch.empty(H * W, dtype=torch.int32, device=p.device)
        wd = torch.empty(2 * H * W, dtype=torch.float64, device=p.device)
        part = torch.empty(nblk, 2, dtype=torch.float64, device=p.device)
        call.pn2_eval_wfm(_p(p), _p(g), H, W, _p(Kd), float(np.log(1 - 0.5) / 5), _p(wi), _p(wd), _p(part), _stream())
        pt = part.cpu().numpy()
        sums = (float(pt[:, 0].sum()), float(pt[:, 1].sum()))
    return metrics_from_counts(h_all, h_gt, out25, sums, H, W)


def eval_for_testAllInOne(opt, pred_u8, gt):
    """The reference's eval.py:18-66 with GPU tensors: the values of opt["metrics"] (any of meanDic, meanIoU, wFm, Sm, meanEm, mae) in that order."""
    r = threshold_metrics(pred_u8, gt, full=any(k in ("wFm", "Sm", "meanEm") for k in opt["metrics"]))
    return [r[k] for k in opt["metrics"]]


def gauss7():
    """fspecial_gauss(7, 5) of original_WFb (eval_functions.py:96-129), float64 [7][7]."""
    xk, yk = np.mgrid[-7 // 2 + 1:7 // 2 + 1, -7 // 2 + 1:7 // 2 + 1]
    K = np.exp(-((xk ** 2 + yk ** 2) / (2.0 * 5 ** 2)))
    return K / K.sum()


def metrics_from_counts(h_all, h_gt, out25=None, sums=None, H=None, W=None, full=True):
    """Host finish of every metric of eval_for_testAllInOne from what the kernels count - pure numpy, float64, the reference's expressions; the per-image path
    (threshold_metrics) and the batch path (eval_batch) both end here.
      h_all, h_gt  int64 [256]: pixels per prediction byte, all / where gt > 0.5 (pn2_eval_hist)
      out25        the 25 integers of pn2_eval_region_sums; used where 0 < foreground < all pixels.  None there: "Sm" is left out
      sums         (s_fg, s_bg): Ew summed over the foreground / background (pn2_eval_wfm).  None with a foreground: "wFm" is left out; without one wFm is NaN
      H, W         the map's size, when given checked against the pixel count
    full=False: the threshold sweep only (curves, meanDic, meanIoU, meanSen, meanSpe, meanFm, mae); full=True adds "E" (the 256 EnhancedMeasure scores),
    meanEm, Sm and wFm."""
    h_all, h_gt = np.asarray(h_all, dtype=np.int64), np.asarray(h_gt, dtype=np.int64)
    vals = np.arange(256).astype(np.float64) / 255                  # pred.astype(float64) / 255   (eval.py:28)
    thr = np.minimum(np.linspace(1, 0, 256), 1)                     # eval.py:19, eval_functions.py:132-133
    ge = (vals[None, :] >= thr[:, None]).astype(np.int64)           # Label3[pred >= threshold] = 1
    num_rec, num_and = ge @ h_all, ge @ h_gt
    total, num_obj = int(h_all.sum()), np.float64(h_gt.sum())
    if H is not None and W is not None and int(H) * int(W) != total:
        raise ValueError(f"{total} pixels counted for a {H} x {W} map")
    num_no_rec = total - num_rec
    fn = num_obj - num_and
    fp = num_rec - num_and
    tn = num_no_rec - fn
    cols = np.zeros((256, 6))
    ok = num_and != 0
    with np.errstate(divide="ignore", invalid="ignore"):
        pre = num_and / num_rec
        rec = num_and / num_obj
        cols[:, 0], cols[:, 1] = pre, rec
        cols[:, 2] = tn / (tn + fp)
        cols[:, 3] = 2 * num_and / (num_obj + num_rec.astype(np.float64))
        cols[:, 4] = (2.0 * pre * rec) / (pre + rec)
        cols[:, 5] = num_and / (fn + num_rec)
    cols[~ok] = 0
    h_bg = h_all - h_gt
    mae = float((h_gt * np.abs(1.0 - vals)).sum() + (h_bg * vals).sum()) / total
    m = cols.mean(axis=0)
    out = {"curves": cols, "meanDic": float(m[3]), "meanIoU": float(m[5]), "meanSen": float(m[1]), "meanSpe": float(m[2]), "meanFm": float(m[4]),
           "mae": mae}
    if full:
        out.update(_em_sm_wfm(h_all, h_gt, total, num_rec, num_and, out25, sums))
    return out


def _em_sm_wfm(h_all, h_gt, total, num_rec, num_and, q, sums):
    """meanEm / Sm / wFm of eval_for_testAllInOne (eval.py:31-33,46-47,59-60) from the two histograms, the integer quadrant moments of pn2_eval_region_sums and
    the weighted error sums of pn2_eval_wfm; float64 on the host with the expressions of utils/eval_functions.py (the sums over pixels the reference takes with
    numpy's pairwise summation become count x value / exact integer moments here: agreement to ~1e-15, not bit for bit)."""
    eps = np.finfo(np.float64).eps
    N, num_obj = int(total), int(h_gt.sum())
    vals = np.arange(256).astype(np.float64) / 255
    # ---- EnhancedMeasure per threshold (eval_functions.py:168-192): the alignment matrix of a binary map takes one value per (prediction bit, gt bit) class
    E = np.zeros(256)
    for i in range(256):
        nr, na = int(num_rec[i]), int(num_and[i])
        if num_obj == 0:
            s = N - nr
        elif num_obj == N:
            s = nr
        else:
            mp_, mg = np.float64(nr) / N, np.float64(num_obj) / N
            s = 0.0
            for b, gg, cnt in ((1, 1, na), (1, 0, nr - na), (0, 1, num_obj - na), (0, 0, N - nr - (num_obj - na))):
                if cnt:
                    ap, ag = b - mp_, gg - mg
                    al = 2 * (ag * ap) / (ag ** 2 + ap ** 2 + eps)
                    s += cnt * (((al + 1) ** 2) / 4)
        E[i] = s / (N - 1 + eps)
    out = {"E": E, "meanEm": float(E.mean())}
    # ---- StructureMeasure (eval_functions.py:5-94)
    h_bg = h_all - h_gt
    mean_pred = float((h_all * vals).sum()) / N
    y = np.float64(num_obj) / N
    sm = None
    if y == 0:
        sm = 1 - mean_pred
    elif y == 1:
        sm = mean_pred
    elif q is not None:
        def obj(h, v):              # Object(): mean and population std of the values v (histogram h)
            n = h.sum()
            x = float((h * v).sum()) / n
            sd = np.sqrt(float((h * (v - x) ** 2).sum()) / n)
            return 2.0 * x / (x ** 2 + 1 + sd + eps)
        s_obj = y * obj(h_gt, vals) + (1 - y) * obj(h_bg, 1 - vals)
        q = [int(v) for v in q]
        s_reg = 0.0
        for k in range(4):
            n, sk, skk, sg, skg = q[3 + 5 * k: 8 + 5 * k]
            if n == 0:
                s_reg = float("nan")            # numpy's mean of an empty quadrant is nan and the reference propagates it (eval_functions.py:50-70)
                continue
            x, yy = sk / 255 / n, sg / n
            den = n - 1 + eps
            sx = (n * skk - sk * sk) / (n * 65025) / den          # sum (p - x)^2 / (N - 1 + eps), exact integer numerators
            sy = (n * sg - sg * sg) / n / den
            sxy = (n * skg - sk * sg) / (n * 255) / den
            al, be = 4 * x * yy * sxy, (x ** 2 + yy ** 2) * (sx + sy)
            qq = al / (be + eps) if al != 0 else (1 if be == 0 else 0)
            s_reg = s_reg + qq * (n / N)
        sm = 0.5 * s_obj + 0.5 * s_reg
        if sm < 0:
            sm = 0
    if sm is not None:
        out["Sm"] = float(sm)
    # ---- original_WFb (eval_functions.py:96-129)
    if num_obj == 0:
        out["wFm"] = float("nan")           # scipy's feature transform has no site to return: the reference's value is undefined here
    elif sums is not None:
        s_fg, s_bg = float(sums[0]), float(sums[1])
        TPw, FPw = num_obj - s_fg, s_bg
        R = 1 - s_fg / num_obj
        Pq = TPw / (TPw + FPw + eps)
        out["wFm"] = float(2 * R * Pq / (R + Pq + eps))
    return out


# ------------------------------------------------------------------------------------------------ ragged batch
def ragged_table(gt_shapes, h, w, slots=None, gap=0):
    """The table of a ragged batch (pn2_eval_img rows, include/pn2.h) for ground truths of the sizes gt_shapes = [(H, W) or None, ...] and h x w model maps:
    images packed back to back (gap: bytes left free before every image and after the last - tests put canaries there), rh / rw = the double quotients h / H,
    w / W rounded once to fp32 (what Engine.resize_to hands to pn2_bilinear_fwd through ctypes).  None, (0, 0) and the slots up to `slots` are empty: H = 0.
    Returns (rows, total): a numpy array of dtype ROW and the pixel count of the packed buffers."""
    shapes = [None if s is None else (int(s[0]), int(s[1])) for s in gt_shapes]
    slots = len(shapes) if slots is None else int(slots)
    if slots < len(shapes):
        raise ValueError(f"{len(shapes)} images for {slots} slots")
    rows = np.zeros(slots, dtype=ROW)
    off = int(gap)
    for b, s in enumerate(shapes):
        if s is None or s[0] == 0 or s[1] == 0:
            continue
        H, W = s
        if H < 0 or W < 0:
            raise ValueError(f"ground-truth size {s}")
        rows[b] = (H, W, off, np.float32(h / H), np.float32(w / W))
        off += H * W + int(gap)
    return rows, off


class RaggedViews(list):
    """The per-image (H, W) uint8 views of a packed prediction buffer (None for an empty slot), with the table they were cut by: .rows (numpy, dtype ROW),
    .table (its device copy), .total (pixels of the packed buffers)."""
    rows = table = total = None


_SCRATCH = {}          # (device index, name) -> the largest buffer asked for so far: device scratch is reused across calls


def _scratch(dev, name, numel, dtype, pinned=False):
    key = (dev.index, name)
    t = _SCRATCH.get(key)
    if t is None or t.numel() < numel or t.dtype != dtype:
        t = _SCRATCH[key] = torch.empty(max(int(numel), 1), dtype=dtype, pin_memory=True) if pinned else torch.empty(max(int(numel), 1), dtype=dtype, device=dev)
    return t


def _upload_table(rows, dev):
    return torch.from_numpy(rows.view(np.uint8).reshape(-1).copy()).to(dev, non_blocking=True)


def _limits(rows):
    live = rows["H"] > 0
    if not live.any():
        raise ValueError("a batch without images")
    return int(rows["H"].max()), int(rows["W"][live].max())


def postprocess_batch(outs, gt_shapes, maps="sum4", gap=0, out=None):
    """MyTest_med.py:104-111 for a whole batch in two launches (pn2_eval_tail_batch).  outs: the model's output tuple for B images, K = 1 maps (B,1,h,w) fp32
    on the GPU; gt_shapes: up to B sizes (H, W), None = empty slot (a filler image: nothing is computed for it).  maps="sum4": res2 + res3 + res4 + res5, the first
    four maps (test_with_eval and the V2 branch); maps="last": the last map of the tuple alone (the V1 branch's res2).  Returns (packed, views): the uint8
    predictions of all images back to back and a RaggedViews list of (H, W) views into it, one per slot.  gap / out: see ragged_table (out: a prefilled buffer)."""
    if maps not in ("sum4", "last"):
        raise ValueError(f"maps {maps!r}: 'sum4' or 'last'")
    src = list(outs[:4]) if maps == "sum4" else [outs[-1]]
    if maps == "sum4" and len(src) != 4:
        raise ValueError("maps='sum4' needs four maps")
    for o in src:
        if not o.is_cuda:
            raise RuntimeError("pn2.evaltail needs GPU tensors (no CPU fallback)")
        if o.dim() != 4 or o.shape[1] != 1 or o.shape != src[0].shape:
            raise ValueError(f"K = 1 maps of one shape (B,1,h,w), got {tuple(o.shape)}")
    src = [o.float().contiguous() for o in src]
    B, _, h, w = src[0].shape
    dev = src[0].device
    rows, total = ragged_table(gt_shapes, h, w, slots=B, gap=gap)
    maxH, maxW = _limits(rows)
    if out is None:
        out = torch.empty(total, dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or out.numel() < total or not out.is_cuda or not out.is_contiguous():
        raise ValueError("out: a contiguous uint8 GPU buffer of at least the table's pixel count")
    table = _upload_table(rows, dev)
    mm = torch.empty(2 * B, dtype=torch.int32, device=dev)          # (from the caching allocator, per stream: calls on two streams never share it)
    ptrs = (C.c_void_p * len(src))(*[o.data_ptr() for o in src])
    call.pn2_eval_tail_batch(ptrs, len(src), B, h, w, _p(table), maxH, maxW, total, _p(out), _p(mm), _stream())
    views = RaggedViews(out[int(r["off"]):int(r["off"]) + int(r["H"]) * int(r["W"])].view(int(r["H"]), int(r["W"])) if r["H"] > 0 else None for r in rows)
    views.rows, views.table, views.total = rows, table, total
    return out, views


def pack_batch(preds):
    """(packed, views) as postprocess_batch returns them, for uint8 GPU prediction maps (H, W) that already exist (None = empty slot)."""
    for t in preds:
        if t is not None and not t.is_cuda:
            raise RuntimeError("pn2.evaltail needs GPU tensors (no CPU fallback)")
        if t is not None and (t.dtype != torch.uint8 or t.dim() != 2):
            raise ValueError("uint8 maps (H, W)")
    rows, total = ragged_table([None if t is None else tuple(t.shape) for t in preds], 1, 1)
    _limits(rows)
    packed = torch.cat([t.reshape(-1) for t in preds if t is not None and t.numel()])
    views = RaggedViews(packed[int(r["off"]):int(r["off"]) + int(r["H"]) * int(r["W"])].view(int(r["H"]), int(r["W"])) if r["H"] > 0 else None for r in rows)
    views.rows, views.table, views.total = rows, _upload_table(rows, packed.device), total
    return packed, views


def eval_batch(opt, packed_pred, views, gts, counts=None):
    """eval_for_testAllInOne (eval.py:18-66) of every image of a ragged batch: ndarray [n][len(opt["metrics"])], one row per non-empty slot in slot order, the
    values and order of the per-image eval_for_testAllInOne.  packed_pred, views: what postprocess_batch returned; gts: the ground truths - one GPU tensor (H, W)
    per slot (None for an empty slot), or one packed fp32 GPU buffer laid out like packed_pred.  Two launches for the histograms and region sums, three for wFm
    (skipped when opt["metrics"] has no wFm, the region sums likewise without Sm), then ONE device-to-host copy with every count and partial sum of the batch.
    counts: a dict to receive "hist" [n][512], "out25" [n][25] or None and "sums" [n][2] or None (tests)."""
    metrics = list(opt["metrics"])
    if not packed_pred.is_cuda:
        raise RuntimeError("pn2.evaltail needs GPU tensors (no CPU fallback)")
    if not isinstance(views, RaggedViews):
        raise TypeError("views: the RaggedViews that postprocess_batch returned")
    rows, total, dev = views.rows, int(views.total), packed_pred.device
    B = len(rows)
    live = [b for b in range(B) if rows["H"][b] > 0]
    if isinstance(gts, torch.Tensor):
        g = gts
        if not g.is_cuda:
            raise RuntimeError("pn2.evaltail needs GPU tensors (no CPU fallback)")
        g = g.float().contiguous().reshape(-1)
    else:
        gl = [gts[b] for b in live]
        for b, t in zip(live, gl):
            if not t.is_cuda:
                raise RuntimeError("pn2.evaltail needs GPU tensors (no CPU fallback)")
            if t.numel() != int(rows["H"][b]) * int(rows["W"][b]):
                raise ValueError(f"ground truth {b}: {tuple(t.shape)} for a {int(rows['H'][b])} x {int(rows['W'][b])} prediction")
        back_to_back = int(rows["off"][live[0]]) == 0 and all(int(rows["off"][b]) == int(rows["off"][a]) + int(rows["H"][a]) * int(rows["W"][a]) for a, b in zip(live, live[1:]))
        if back_to_back:
            g = torch.cat([t.reshape(-1).float() for t in gl])
        else:
            g = torch.zeros(total, dtype=torch.float32, device=dev)
            for b, t in zip(live, gl):
                g[int(rows["off"][b]):int(rows["off"][b]) + t.numel()] = t.reshape(-1)
    if g.numel() < total or packed_pred.numel() < total or packed_pred.dtype != torch.uint8:
        raise ValueError("packed buffers shorter than the table's pixel count")
    p = packed_pred.contiguous()
    maxH, maxW = _limits(rows)
    want_sm, want_wfm = "Sm" in metrics, "wFm" in metrics
    # one result buffer: part f64 [B][2048][2] | out25 u64 [B][25] | hist u32 [B][512]
    n_part, n_q = (B * WFM_MAX_BLOCKS * 2 if want_wfm else 0), (B * 25 if want_sm else 0)
    nbytes = 8 * (n_part + n_q) + 4 * B * 512
    res = _scratch(dev, "result", nbytes, torch.uint8)
    base = res.data_ptr()
    part_p, q_p, hist_p = C.c_void_p(base), C.c_void_p(base + 8 * n_part if want_sm else 0), C.c_void_p(base + 8 * (n_part + n_q))
    call.pn2_eval_counts_batch(_p(p), _p(g), _p(views.table), B, maxH, maxW, total, hist_p, q_p, _stream())
    if want_wfm:
        Kd = _SCRATCH.get((dev.index, "K49"))
        if Kd is None:
            Kd = _SCRATCH[(dev.index, "K49")] = torch.from_numpy(np.ascontiguousarray(gauss7())).to(dev)
        wi = _scratch(dev, "work_i", total, torch.int32)
        wd = _scratch(dev, "work_d", 2 * total, torch.float64)
        call.pn2_eval_wfm_batch(_p(p), _p(g), _p(views.table), B, maxH, maxW, total, _p(Kd), float(np.log(1 - 0.5) / 5), _p(wi), _p(wd), part_p, _stream())
    host = _scratch(dev, "result_host", nbytes, torch.uint8, pinned=True)
    host[:nbytes].copy_(res[:nbytes], non_blocking=True)
    torch.cuda.current_stream().synchronize()
    raw = host[:nbytes].numpy()
    part = raw[:8 * n_part].view(np.float64).reshape(B, WFM_MAX_BLOCKS, 2) if want_wfm else None
    q25 = raw[8 * n_part:8 * (n_part + n_q)].view(np.uint64).reshape(B, 25) if want_sm else None
    hist = raw[8 * (n_part + n_q):].view(np.uint32).reshape(B, 512).astype(np.int64)
    out = np.zeros((len(live), len(metrics)))
    full = any(k in ("wFm", "Sm", "meanEm") for k in metrics)
    sums_all = []
    for i, b in enumerate(live):
        H, W = int(rows["H"][b]), int(rows["W"][b])
        sums = None
        if want_wfm:
            nblk = int(call.pn2_eval_wfm_blocks(H, W))
            pt = np.ascontiguousarray(part[b, :nblk])          # the per-image entry's [nblk][2]: numpy sums it in the same order
            sums = (float(pt[:, 0].sum()), float(pt[:, 1].sum()))
        sums_all.append(sums)
        r = metrics_from_counts(hist[b, :256], hist[b, 256:], [int(v) for v in q25[b]] if want_sm else None, sums, H, W, full=full)
        out[i] = [r[k] for k in metrics]
    if counts is not None:
        counts["hist"] = hist[live].copy()
        counts["out25"] = q25[live].astype(np.int64) if want_sm else None
        counts["sums"] = np.array(sums_all) if want_wfm else None
    return out
