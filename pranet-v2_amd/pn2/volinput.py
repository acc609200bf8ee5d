"""Device-side slice transform of the multi-class (Synapse) side: what RandomGenerator applies to every training sample
(multiclass_seg/EMCAD/utils/dataset_synapse.py:12-47) and what test_single_volume / val_single_volume do to every slice (utils/utils.py:179-181,197-198):
scipy.ndimage.zoom with order 3 (image) and order 0 (label), ndimage.rotate(order=0, reshape=False), np.rot90 + np.flip.  File reading stays on the host;
everything after the arrays runs on the GPU (csrc/pn2_zoom.hip) and is bit-exact with scipy at the defaults the reference uses - including the rows and
columns scipy leaves at 0 because the last output coordinate exceeds the last input sample in double (512 -> 224 has a zero last row and column).
GPU tensors only: there is no CPU fallback."""
import ctypes as C
import random

import numpy as np
import torch

from .capi import call, RaggedDesc, RaggedHeader, RaggedSample, RAGGED_MAX_N

MAX_AXIS = 1024
_TABLES = {}
_ELEM = {torch.uint8: 1, torch.float32: 4}


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need_gpu(*ts):
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in ts):
        raise RuntimeError("pn2.volinput needs GPU tensors (no CPU fallback)")


def _batch(x):
    """[H][W] or [N][H][W] -> contiguous [N][H][W], and whether the batch axis was added."""
    if x.dim() not in (2, 3):
        raise ValueError(f"shape {tuple(x.shape)}: [H][W] or [N][H][W]")
    single = x.dim() == 2
    x = (x[None] if single else x).contiguous()
    if x.shape[0] < 1 or min(x.shape[1:]) < 1 or max(x.shape[1:]) > MAX_AXIS:
        raise ValueError(f"shape {tuple(x.shape)}: an empty batch, or an axis outside 1 .. {MAX_AXIS}")
    return x, single


def _tables(nin, nout, order, dev):
    """The per-axis tables of pn2_zoom_tables (host, double) as device tensors, cached per (axis lengths, order, device)."""
    key = (nin, nout, order, dev)
    hit = _TABLES.get(key)
    if hit is None:
        per = 4 if order == 3 else 1
        idx, w, valid = np.zeros(nout * per, np.int32), np.zeros(nout * per, np.float64), np.zeros(nout, np.int32)
        call.pn2_zoom_tables(nin, nout, order, C.c_void_p(idx.ctypes.data), C.c_void_p(w.ctypes.data), C.c_void_p(valid.ctypes.data))
        hit = _TABLES[key] = tuple(torch.from_numpy(a).to(dev) for a in (idx, w, valid))
    return hit


def zoom(x, size, order):
    """scipy.ndimage.zoom(s, (oh / H, ow / W), order=order) of every [H][W] slice of x ([H][W] or [N][H][W]) with size = (oh, ow).
    order 3: fp32 -> fp32.  order 0: uint8, int64 or fp32 -> the same dtype (int64 labels must lie in 0..255; they travel as uint8).
    Equal input and output size returns x itself: the reference skips the call then."""
    _need_gpu(x)
    if order not in (0, 3):
        raise ValueError("order 3 (image) or 0 (label)")
    oh, ow = int(size[0]), int(size[1])
    if not (1 <= oh <= MAX_AXIS and 1 <= ow <= MAX_AXIS):
        raise ValueError(f"size {(oh, ow)}: every axis must be in 1 .. {MAX_AXIS}")
    if x.dtype not in ((torch.float32,) if order == 3 else (torch.uint8, torch.int64, torch.float32)):
        raise ValueError(f"order {order} zoom of {x.dtype}: order 3 takes fp32, order 0 uint8, int64 or fp32")
    xb, single = _batch(x)
    N, H, W = xb.shape
    if (H, W) == (oh, ow):
        return x
    as_long = xb.dtype == torch.int64
    if as_long:
        if int(xb.min()) < 0 or int(xb.max()) > 255:
            raise ValueError("int64 labels must lie in 0 .. 255")
        xb = xb.to(torch.uint8)
    dev, st = xb.device, _stream()
    out = torch.empty((N, oh, ow), dtype=xb.dtype, device=dev)
    iy, wy, vy = _tables(H, oh, order, dev)
    ix, wx, vx = _tables(W, ow, order, dev)
    if order == 3:
        nbytes = C.c_longlong(0)
        call.pn2_zoom_workspace(N, H, W, C.byref(nbytes))
        work = torch.empty(int(nbytes.value), dtype=torch.uint8, device=dev)
        call.pn2_zoom_prefilter(_p(xb), N, H, W, _p(work), st)
        call.pn2_zoom3_gather(_p(work), N, H, W, oh, ow, _p(iy), _p(wy), _p(vy), _p(ix), _p(wx), _p(vx), _p(out), st)
    else:
        call.pn2_zoom0(_ELEM[xb.dtype], _p(xb), N, H, W, oh, ow, _p(iy), _p(vy), _p(ix), _p(vx), _p(out), st)
    if as_long:
        out = out.long()
    return out[0] if single else out


def _rotate_matrix(angle, H, W):
    """(m00, m01, m10, m11, off0, off1) of ndimage.rotate(angle, reshape=False): m = [[cos, sin], [-sin, cos]], off = ctr - m @ ctr, ctr = (shape - 1) / 2.
    The matrix product is numpy's, as in scipy's own Python code, so the six doubles are scipy's to the bit."""
    a = np.deg2rad(angle)
    c, s = np.cos(a), np.sin(a)
    m = np.array([[c, s], [-s, c]])
    ctr = (np.array([H, W]) - 1) / 2
    off = ctr - m @ ctr
    return float(m[0, 0]), float(m[0, 1]), float(m[1, 0]), float(m[1, 1]), float(off[0]), float(off[1])


def rotate(x, angles):
    """ndimage.rotate(s, angle, order=0, reshape=False) per sample: x uint8 or fp32 [N][H][W] (or [H][W] with one angle), angles in degrees.  Angle 0 copies."""
    _need_gpu(x)
    if x.dtype not in _ELEM:
        raise ValueError(f"rotate of {x.dtype}: uint8 or fp32")
    xb, single = _batch(x)
    angles = [angles] if np.isscalar(angles) else list(angles)
    N, H, W = xb.shape
    if len(angles) != N:
        raise ValueError(f"{len(angles)} angles for {N} samples")
    m6 = torch.tensor([_rotate_matrix(float(a), H, W) for a in angles], dtype=torch.float64).to(xb.device)
    out = torch.empty_like(xb)
    call.pn2_rotate0(_ELEM[xb.dtype], _p(xb), N, H, W, _p(m6), _p(out), _stream())
    return out[0] if single else out


def rot_flip(x, ks, axes):
    """np.flip(np.rot90(s, k), axis) per sample: x uint8 or fp32 [N][S][S] (or [S][S] with one k and axis), square.  axis None: no flip."""
    _need_gpu(x)
    if x.dtype not in _ELEM:
        raise ValueError(f"rot_flip of {x.dtype}: uint8 or fp32")
    xb, single = _batch(x)
    ks = [ks] if np.isscalar(ks) else list(ks)
    axes = [axes] if axes is None or np.isscalar(axes) else list(axes)
    N, H, W = xb.shape
    if H != W:
        raise ValueError(f"rot_flip needs square samples, got {H} x {W}")
    if len(ks) != N or len(axes) != N or any(a not in (None, 0, 1) for a in axes):
        raise ValueError("one k and one axis (0, 1 or None) per sample")
    ka = torch.tensor([[int(k) % 4, -1 if a is None else int(a)] for k, a in zip(ks, axes)], dtype=torch.int32).to(xb.device)
    out = torch.empty_like(xb)
    call.pn2_rot_flip(_ELEM[xb.dtype], _p(xb), N, H, _p(ka), _p(out), _stream())
    return out[0] if single else out


class SliceTransform:
    """t = SliceTransform((224, 224)); batch = t(images, labels) with images fp32 [N][H][H] and labels uint8 [N][H][H] on the device
    -> {'image': fp32 [N][1][oh][ow], 'label': int64 [N][oh][ow]}: the batch RandomGenerator + DataLoader would collate.
    draws: per sample ('rot_flip', k, axis), ('rotate', angle) or None; drawn by SliceTransform.draw(N) when omitted."""

    def __init__(self, output_size):
        self.output_size = (int(output_size[0]), int(output_size[1]))

    @staticmethod
    def draw(n):
        """The random decisions of n consecutive RandomGenerator calls, from the same generators in the same order (dataset_synapse.py:12-40): after
        random.seed / np.random.seed a run takes the decisions the reference's loader would take in one worker."""
        out = []
        for _ in range(n):
            if random.random() > 0.5:
                k = int(np.random.randint(0, 4))
                out.append(("rot_flip", k, int(np.random.randint(0, 2))))
            elif random.random() > 0.5:
                out.append(("rotate", int(np.random.randint(-20, 20))))
            else:
                out.append(None)
        return out

    def __call__(self, images, labels, draws=None):
        _need_gpu(images, labels)
        if images.dim() != 3 or images.shape != labels.shape or images.dtype != torch.float32 or labels.dtype != torch.uint8:
            raise ValueError("images fp32 [N][H][W] and labels uint8 [N][H][W] of one shape")
        N, H, W = images.shape
        if H != W:
            raise ValueError(f"SliceTransform needs square slices (np.rot90 changes the shape of others), got {H} x {W}")
        draws = self.draw(N) if draws is None else list(draws)
        if len(draws) != N or any(d is not None and d[0] not in ("rot_flip", "rotate") for d in draws):
            raise ValueError("one draw per sample: ('rot_flip', k, axis), ('rotate', angle) or None")
        if any(d is not None and d[0] == "rot_flip" for d in draws):
            ks = [d[1] if d is not None and d[0] == "rot_flip" else 0 for d in draws]
            axes = [d[2] if d is not None and d[0] == "rot_flip" else None for d in draws]
            images, labels = rot_flip(images, ks, axes), rot_flip(labels, ks, axes)
        if any(d is not None and d[0] == "rotate" for d in draws):
            angles = [d[1] if d is not None and d[0] == "rotate" else 0 for d in draws]
            images, labels = rotate(images, angles), rotate(labels, angles)
        images, labels = zoom(images, self.output_size, 3), zoom(labels, self.output_size, 0)
        return {"image": images[:, None].contiguous(), "label": labels.long()}


# ------------------------------------------------------------------------------------------------ ragged batches: the ACDC slices, every one its own [H][W]
# dataset_ACDC.py:13-48 (RandomGenerator on slices of any shape, np.rot90 swapping a non-square one) and MIST/ACDC_train_test.py:48-93 (val(): zoom in, net, order-0
# zoom back to the slice's own size, one binary Dice per slice).  One host-built plan (pn2_ragged_plan: descriptors, block tables, per-axis tables) goes to the device in
# one copy; the launches - 4 prefilter, 1 gather, 1 label - do not depend on N or on the shapes.  The uniform entry points above are untouched.
class RaggedPlan:
    """The blob of pn2_ragged_plan on the host (`host`, uint8 ndarray; `header`, `descs` are views of it) and, after to(dev), on the device (`dev`)."""

    def __init__(self, samples, packed=True):
        n = len(samples)
        if not 1 <= n <= RAGGED_MAX_N:
            raise ValueError(f"{n} samples: a ragged batch holds 1 .. {RAGGED_MAX_N}")
        arr = (RaggedSample * n)(*samples)
        nbytes = C.c_longlong(0)
        call.pn2_ragged_plan_bound(n, arr, C.byref(nbytes))
        buf = np.zeros(int(nbytes.value), np.uint8)
        call.pn2_ragged_plan(n, arr, 1 if packed else 0, C.c_void_p(buf.ctypes.data), buf.size)
        self.header = RaggedHeader.from_buffer(buf)
        self.host = buf[:int(self.header.bytes)]
        self.descs = (RaggedDesc * n).from_buffer(buf, self.header.desc_off)
        self.n, self.dev = n, None

    def block_starts(self):
        h = self.header
        return tuple(np.frombuffer(self.host, np.int32, self.n + 1, off).copy() for off in (h.bs0_off, h.bs1_off))

    def to(self, dev):
        self.dev = torch.from_numpy(self.host).to(dev)          # the one descriptor + table copy of the batch
        return self

    def hp(self):
        return C.c_void_p(self.host.ctypes.data)


def ragged_samples(shapes, sizes, draws=None, offsets=None):
    """One RaggedSample per slice: shapes [(H, W)], sizes [(oh, ow)] (or one size for all), draws as SliceTransform takes them, offsets [(fp32 elements, bytes)]
    relative to the launch's base pointers when the slices do not lie back to back.  Host code: no GPU needed."""
    shapes = [(int(h), int(w)) for h, w in shapes]
    n = len(shapes)
    sizes = list(sizes)
    if len(sizes) == 2 and np.isscalar(sizes[0]):
        sizes = [sizes] * n
    draws = [None] * n if draws is None else list(draws)
    if len(sizes) != n or len(draws) != n or (offsets is not None and len(offsets) != n):
        raise ValueError("one size, one draw and one offset pair per slice")
    out = []
    for i, ((H, W), (oh, ow), d) in enumerate(zip(shapes, sizes, draws)):
        if not all(1 <= int(a) <= MAX_AXIS for a in (H, W, oh, ow)):
            raise ValueError(f"slice {i}: {(H, W)} -> {(int(oh), int(ow))}: every axis must be in 1 .. {MAX_AXIS}")
        s = RaggedSample(H=H, W=W, oh=int(oh), ow=int(ow), axis=-1)
        if d is not None:
            if d[0] == "rot_flip" and len(d) == 3 and d[2] in (None, 0, 1):
                s.geom, s.k, s.axis = 1, int(d[1]) % 4, -1 if d[2] is None else int(d[2])
            elif d[0] == "rotate" and len(d) == 2:
                s.geom = 2
                s.m6[:] = _rotate_matrix(float(d[1]), H, W)
            else:
                raise ValueError("one draw per sample: ('rot_flip', k, axis), ('rotate', angle) or None")
        if offsets is not None:
            s.src_off, s.lab_off = int(offsets[i][0]), int(offsets[i][1])
        out.append(s)
    return out


def _gather_slices(items, dtype, what):
    """A list of [H][W] slices, all on the host (ndarrays / CPU tensors: packed into one buffer, ONE copy to the device) or all on the device (left where they are: the plan
    addresses them relative to the lowest one) -> (base tensor, shapes, element offsets or None when packed, whatever must stay alive until the launches are queued)."""
    items = list(items)
    if not items:
        raise ValueError("an empty batch")
    ts = [torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a for a in items]
    if any(not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype != dtype for t in ts):
        raise ValueError(f"{what}: a list of [H][W] {dtype} slices")
    shapes = [tuple(t.shape) for t in ts]
    if any(min(s) < 1 or max(s) > MAX_AXIS for s in shapes):
        raise ValueError(f"{what}: every axis must be in 1 .. {MAX_AXIS}")
    on_dev = [t.is_cuda for t in ts]
    if not any(on_dev):
        if not torch.cuda.is_available():
            raise RuntimeError("pn2.volinput needs a GPU (no CPU fallback)")
        flat = torch.cat([t.reshape(-1) for t in ts]) if len(ts) > 1 else ts[0].reshape(-1)
        return flat.to("cuda"), shapes, None, None
    if not all(on_dev):
        raise ValueError(f"{what}: all slices on the host or all on the device")
    ts = [t.contiguous() for t in ts]
    base = min(ts, key=lambda t: t.data_ptr())
    es = base.element_size()
    return base, shapes, [(t.data_ptr() - base.data_ptr()) // es for t in ts], ts


def _ragged_batch(images, labels, size, draws):
    """The launches of one ragged batch: images and / or labels (lists, either may be None) -> (fp32 [N][oh][ow] or None, uint8 [N][oh][ow] or None)."""
    oh, ow = int(size[0]), int(size[1])
    img = lab = None
    if images is not None:
        img, shapes, ioff, keep_i = _gather_slices(images, torch.float32, "images")
    if labels is not None:
        lab, lshapes, loff, keep_l = _gather_slices(labels, torch.uint8, "labels")
        if images is not None and (lshapes != shapes or (ioff is None) != (loff is None)):
            raise ValueError("images and labels: one shape per sample, both on the host or both on the device")
        shapes = lshapes
    offsets = None
    if (img is not None and ioff is not None) or (lab is not None and loff is not None):
        n = len(shapes)
        offsets = list(zip(ioff if img is not None else [0] * n, loff if lab is not None else [0] * n))
    dev = (img if img is not None else lab).device
    plan = RaggedPlan(ragged_samples(shapes, (oh, ow), draws, offsets), packed=offsets is None).to(dev)
    st, N = _stream(), plan.n
    out3 = out0 = None
    if img is not None:
        out3 = torch.empty((N, oh, ow), dtype=torch.float32, device=dev)
        work = torch.empty(max(1, 2 * int(plan.header.work_doubles)), dtype=torch.float64, device=dev)
        call.pn2_ragged_prefilter(_p(img), plan.hp(), _p(plan.dev), _p(work), st)
        call.pn2_ragged_zoom3(_p(img), plan.hp(), _p(plan.dev), _p(work), _p(out3), st)
    if lab is not None:
        out0 = torch.empty((N, oh, ow), dtype=torch.uint8, device=dev)
        call.pn2_ragged_zoom0(_p(lab), plan.hp(), _p(plan.dev), _p(out0), st)
    return out3, out0


def zoom_ragged(slices, size, order):
    """scipy.ndimage.zoom(s, (oh / H_i, ow / W_i), order=order) of every slice of a list of [H_i][W_i] tensors or host arrays -> [N][oh][ow] on the device; a slice
    already at (oh, ow) is copied, as the reference skips the call (ACDC_train_test.py:58-60).  order 3: fp32.  order 0: uint8."""
    if order not in (0, 3):
        raise ValueError("order 3 (image) or 0 (label)")
    out3, out0 = _ragged_batch(slices if order == 3 else None, slices if order == 0 else None, size, None)
    return out3 if order == 3 else out0


def _unzoom(labels, sizes):
    """uint8 [N][h][w] on the device -> (packed uint8 buffer, its [x_i][y_i] views, the plan whose out_off address the buffer)."""
    _need_gpu(labels)
    if labels.dim() != 3 or labels.dtype != torch.uint8:
        raise ValueError("labels: uint8 [N][h][w]")
    labels = labels.contiguous()
    N, h, w = labels.shape
    sizes = [(int(a), int(b)) for a, b in sizes]
    if len(sizes) != N:
        raise ValueError(f"{len(sizes)} sizes for {N} samples")
    plan = RaggedPlan(ragged_samples([(h, w)] * N, [(s[0], s[1]) for s in sizes])).to(labels.device)
    packed = torch.empty(int(plan.header.out_elems), dtype=torch.uint8, device=labels.device)
    call.pn2_ragged_zoom0(_p(labels), plan.hp(), _p(plan.dev), _p(packed), _stream())
    views = [packed[d.out_off:d.out_off + d.oh * d.ow].view(d.oh, d.ow) for d in plan.descs]
    return packed, views, plan


def unzoom_labels(labels, sizes):
    """The way back of val() (ACDC_train_test.py:82-83): scipy.ndimage.zoom(labels[i], (x_i / h, y_i / w), order=0) of uniform uint8 labels [N][h][w], every sample to
    its own size -> a list of [x_i][y_i] views of one packed buffer (one launch).  A sample already at its size is copied."""
    return _unzoom(labels, sizes)[1]


def dice_counts(pred, gt, sizes, plan=None):
    """int64 ndarray [N][3] = |pred != 0 and gt != 0|, |pred != 0|, |gt != 0| per sample of two packed uint8 buffers holding [x_i][y_i] samples back to back
    (one launch, one copy to the host): what medpy's dc(pred_i, gt_i) needs (ACDC_train_test.py:87)."""
    return _dice_counts_dev(pred, gt, sizes, plan).cpu().numpy()


def _dice_counts_dev(pred, gt, sizes, plan=None):
    _need_gpu(pred, gt)
    if plan is None:
        plan = RaggedPlan(ragged_samples(sizes, sizes)).to(pred.device)
    n = int(plan.header.out_elems)
    if pred.dtype != torch.uint8 or gt.dtype != torch.uint8 or pred.numel() != n or gt.numel() != n or not pred.is_contiguous() or not gt.is_contiguous():
        raise ValueError(f"pred and gt: contiguous uint8 buffers of {n} elements")
    cnt = torch.empty((plan.n, 3), dtype=torch.int64, device=pred.device)
    call.pn2_ragged_dice_counts(_p(pred), _p(gt), plan.hp(), _p(plan.dev), _p(cnt), _stream())
    return cnt


class RaggedSliceTransform:
    """t = RaggedSliceTransform((224, 224)); batch = t(images, labels) with lists of fp32 [H_i][W_i] images and uint8 labels of the same shapes, square or not, all on the
    host (one copy of the pixels, one of the labels) or all on the device -> {'image': fp32 [N][1][oh][ow], 'label': int64 [N][oh][ow]}: the batch the ACDC
    RandomGenerator + DataLoader would collate (dataset_ACDC.py:30-48).  draws as SliceTransform takes them, from SliceTransform.draw (the ACDC file consumes the
    generators in the Synapse file's order, :37-40 with :14,17,24).  np.rot90 with odd k swaps a sample's shape before the zoom; a sample at the output size after
    its geometry is not zoomed (:42)."""

    draw = staticmethod(SliceTransform.draw)

    def __init__(self, output_size):
        self.output_size = (int(output_size[0]), int(output_size[1]))
        if not all(1 <= a <= MAX_AXIS for a in self.output_size):
            raise ValueError(f"size {self.output_size}: every axis must be in 1 .. {MAX_AXIS}")

    def __call__(self, images, labels, draws=None):
        images, labels = list(images), list(labels)
        if len(images) != len(labels):
            raise ValueError("one label per image")
        draws = self.draw(len(images)) if draws is None else list(draws)
        image, label = _ragged_batch(images, labels, self.output_size, draws)
        return {"image": image[:, None], "label": label.long()}
