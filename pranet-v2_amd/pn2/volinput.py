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

from .capi import call

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
