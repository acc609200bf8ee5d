"""Device-side input transform: what PolypDataset / test_dataset apply to every decoded image
(binary_seg/utils/dataloader.py:104-111, 176-181): Resize((S, S)) -> ToTensor() -> Normalize(mean, std) for the image,
Resize((S, S)) -> ToTensor() for the mask.  File decoding stays on the host (PIL); everything after the uint8 pixels runs on the GPU and is
bit-exact with torchvision-on-PIL (the resize is Pillow's antialiased bilinear, two uint8 passes with 22-bit fixed-point taps).  The polyp loaders' augmentation
(multiclass_seg/EMCAD/utils/dataloader.py:24-39: RandomRotation(90), RandomVerticalFlip, RandomHorizontalFlip in front of the resize) runs inside the batched
transform: rotate_coeffs turns a draw into the integers of Pillow's nearest-neighbour rotate and the width pass reads through them."""
import ctypes as C
import math

import numpy as np
import torch

from . import capi
from .capi import call

_MEAN, _STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------ ragged batch: the host side, pure numpy
# one row of the device table of the batch entries (pn2_input_slot, include/pn2.h)
SLOT = np.dtype([("H", "<i4"), ("W", "<i4"), ("C", "<i4"), ("dst", "<i4"), ("norm", "<i4"), ("kw", "<i4"), ("kh", "<i4"), ("blk", "<i4"),
                 ("src", "<i8"), ("tmp", "<i8"), ("tap_w", "<i8"), ("tap_h", "<i8")])
PX = 4                 # PN2_INPUT_PX (include/pn2.h): adjacent output pixels per thread
ALIGN = 16             # every slot of the source and scratch arenas starts on a multiple of this


def _up(v, a):
    return -(-int(v) // a) * a


def slot_blocks(rows, S):
    """pn2_input_batch_blocks: 256-thread blocks of rows x S output pixels, PX pixels per thread."""
    return -(-(int(rows) * -(-int(S) // PX)) // 256)


def tap_block(in_size, S):
    """(block, ksize): the taps of one axis of length in_size resized to S, as the kernels read them - int32 xmin[S] | count[S] | kk[S][ksize], filled by
    pn2_resize_coeffs (host code of the library: Pillow's coefficient arithmetic exists once)."""
    ks = int(call.pn2_resize_ksize(int(in_size), int(S)))
    if ks < 0:
        raise ValueError(f"resize of an axis of {in_size} to {S}")
    blk = np.zeros(2 * S + S * ks, np.int32)
    call.pn2_resize_coeffs(int(in_size), int(S), C.c_void_p(blk.ctypes.data), C.c_void_p(blk[S:].ctypes.data), C.c_void_p(blk[2 * S:].ctypes.data))
    return blk, ks


class TapArena:
    """Host copy of the growing tap arena of one output size: .blocks[in_size] = (int32 offset, ksize), .data[:.ints] the blocks back to back in the order they
    were first asked for.  A size is computed once; get() of a known size changes nothing."""

    def __init__(self, size):
        self.size = int(size)
        self.blocks = {}
        self.data = np.zeros(0, np.int32)
        self.ints = 0

    def get(self, in_size):
        hit = self.blocks.get(int(in_size))
        if hit is None:
            blk, ks = tap_block(in_size, self.size)
            if self.ints + len(blk) > len(self.data):
                grown = np.zeros(max(2 * len(self.data), self.ints + len(blk)), np.int32)
                grown[:self.ints] = self.data[:self.ints]
                self.data = grown
            self.data[self.ints:self.ints + len(blk)] = blk
            hit = self.blocks[int(in_size)] = (self.ints, ks)
            self.ints += len(blk)
        return hit


def batch_table(shapes, S, taps, dst=None, norm=None, gap=0):
    """The table of a ragged batch (pn2_input_slot rows, include/pn2.h) for sources of the shapes [(H, W, C) or None, ...] (None, or H == 0: an empty slot, which
    takes no byte of either arena and no block).  Sources are packed in slot order, each on a multiple of ALIGN bytes, the [H][S][C] scratch images likewise;
    gap: bytes left free before every slot and after the last in both arenas (tests put canaries there).  taps: the TapArena of S - sizes it has not seen are
    added, slots of one size share a block; an axis that already has length S gets no block (that pass is a copy).  dst: the output sample of every slot
    (default: images and masks each count from 0 in slot order); norm: whether Normalize applies (default: where C == 3).
    Returns (rows, src_bytes, tmp_bytes): a numpy array of dtype SLOT and the sizes of the two arenas."""
    S = int(S)
    if taps.size != S:
        raise ValueError(f"a tap arena for size {taps.size}, asked for {S}")
    rows = np.zeros(len(shapes), dtype=SLOT)
    src = tmp = int(gap)
    blk = 0
    seen = {1: 0, 3: 0}
    for i, s in enumerate(shapes):
        rows[i]["blk"] = blk
        if s is None or int(s[0]) == 0:
            continue
        H, W, Cc = (int(v) for v in s)
        if H < 0 or W < 1 or Cc not in (1, 3):
            raise ValueError(f"slot {i}: a uint8 image [H][W][1 or 3], got {tuple(s)}")
        src, tmp = _up(src, ALIGN), _up(tmp, ALIGN)
        tw, kw = taps.get(W) if W != S else (0, 0)
        th, kh = taps.get(H) if H != S else (0, 0)
        rows[i] = (H, W, Cc, seen[Cc] if dst is None else int(dst[i]), int(Cc == 3) if norm is None else int(bool(norm[i])), kw, kh, blk, src, tmp, tw, th)
        seen[Cc] += 1
        src += H * W * Cc + int(gap)
        tmp += H * S * Cc + int(gap)
        blk += slot_blocks(H, S)
    return rows, src, tmp


# ------------------------------------------------------------------------------------------------ augmentation: rotation and flips as a map the width pass reads through
# one row of the second table of pn2_input_batch_width_aug (pn2_input_aug, include/pn2.h)
AUG = np.dtype([("a", "<i4", (6,)), ("mode", "<i4"), ("reserved", "<i4")])
AUG_MAX_AXIS = 16384          # PN2_INPUT_AUG_MAX_AXIS (include/pn2.h)
_NO_MAP = (0,) * 8            # a row in mode 0


def _fix(v):
    """Pillow's FIX (Geometry.c): floor(v * 65536 + 0.5), the int cast truncating only where the value is not negative"""
    v = v * 65536.0 + 0.5
    return int(v) if v >= 0.0 else int(math.floor(v))


def rotate_coeffs(angle, flip_v, flip_h, H, W):
    """((a0, a1, a2, a3, a4, a5), mode) for an [H][W][C] image: pixel (y, x) of
        Image.rotate(angle, NEAREST, expand=False) -> transpose(FLIP_TOP_BOTTOM) if flip_v -> transpose(FLIP_LEFT_RIGHT) if flip_h
    is src[(a5 + a3 * x + a4 * y) >> 16][(a2 + a0 * x + a1 * y) >> 16], or 0 when either index is outside the image - Pillow's bytes.
    The matrix is Image.rotate's, in Python doubles (angle % 360, -radians, cos / sin rounded to 15 decimals, centre (W/2, H/2)); the integers are Geometry.c's
    16.16 fixed point (affine_fixed); the flips are the substitutions x -> W-1-x, y -> H-1-y folded into them.  Pillow answers 0 with a copy, 180 and (on square
    images) 90 / 270 with a transpose, and a matrix without sine terms with its scaling loop: the same integers give those bytes too (tests/test_input_aug_cpu.py).
    mode 0 - read the source directly - for a multiple of 360 degrees without a flip, else 1."""
    H, W = int(H), int(W)
    a = float(angle) % 360.0
    mode = int(a != 0.0 or bool(flip_v) or bool(flip_h))
    r = -math.radians(a)
    c, s = round(math.cos(r), 15), round(math.sin(r), 15)
    m = [c, s, 0.0, -s, c, 0.0]          # (Pillow rounds -sin: round() is symmetric in sign, zeros included)
    cx, cy = W / 2, H / 2
    m[2], m[5] = m[0] * -cx + m[1] * -cy + m[2], m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    a0, a1, a3, a4 = _fix(m[0]), _fix(m[1]), _fix(m[3]), _fix(m[4])
    a2, a5 = _fix(m[2] + m[0] * 0.5 + m[1] * 0.5), _fix(m[5] + m[3] * 0.5 + m[4] * 0.5)
    if flip_h:          # the last transform applied: x -> W-1-x
        a2, a5, a0, a3 = a2 + a0 * (W - 1), a5 + a3 * (W - 1), -a0, -a3
    if flip_v:
        a2, a5, a1, a4 = a2 + a1 * (H - 1), a5 + a4 * (H - 1), -a1, -a4
    return (a0, a1, a2, a3, a4, a5), mode


def aug_table(shapes, draws):
    """The second table (dtype AUG) of a batch whose first table was built from `shapes`: draws[i] = (angle, flip_v, flip_h) or None for the slot of shapes[i]."""
    ints = [_NO_MAP] * len(shapes)
    done = {}          # a mask has its image's size and draw: the integers are formed once per pair
    for i, (s, d) in enumerate(zip(shapes, draws)):
        if s is None or d is None or int(s[0]) == 0:
            continue
        if max(int(s[0]), int(s[1])) > AUG_MAX_AXIS:
            raise ValueError(f"slot {i}: rotation is built for axes up to {AUG_MAX_AXIS}, got {tuple(s)}")
        key = (float(d[0]), bool(d[1]), bool(d[2]), int(s[0]), int(s[1]))
        hit = done.get(key)
        if hit is None:
            a, mode = rotate_coeffs(*key)
            hit = done[key] = a + (mode, 0)
        ints[i] = hit
    return np.array(ints, dtype=np.int32).reshape(-1).view(AUG)          # (one conversion: row-by-row stores into a structured array cost more than the arithmetic)


class DeviceTransform:
    """t = DeviceTransform(352); x, gt = t(images_u8, masks_u8) with lists of uint8 tensors [H][W][3] / [H][W] (any sizes)
    -> x fp32 [N][3][S][S] normalised, gt fp32 [N][1][S][S] in [0, 1]: the batch PolypDataset + DataLoader would collate.
    t.batch(images_u8, masks_u8) gives the same tensors for the whole list in two launches and one host-to-device copy; with draws=t.draw(n) every pair is
    rotated and flipped first, as the polyp loaders' augmentation switch does, in the same two launches."""

    def __init__(self, size, mean=_MEAN, std=_STD, device=None):
        if not torch.cuda.is_available():
            raise RuntimeError("pranet-v2_amd runs on MI355X only: no GPU visible and there is no CPU fallback")
        capi.load()
        self.size = int(size)
        self.dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.mean = torch.tensor(mean, dtype=torch.float32, device=self.dev)
        self.std = torch.tensor(std, dtype=torch.float32, device=self.dev)
        self._coeffs = {}
        # state of batch(): host tap arena and its device mirror, the reused buffers, and the event after which the pinned staging buffer may be rewritten
        self.taps = TapArena(self.size)
        self.tap_uploads = 0          # host-to-device copies of tap blocks so far (a batch without a new size makes none)
        self._taps_dev, self._taps_up = None, 0
        self._bufs = {}
        self._staged = None

    def _buf(self, name, nbytes, pinned=False):
        t = self._bufs.get(name)
        if t is None or t.numel() < nbytes:
            nbytes = max(int(nbytes), 2 * t.numel() if t is not None else 256)
            t = self._bufs[name] = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True) if pinned else torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        return t

    def _sync_taps(self):
        """the device mirror of self.taps: only the blocks added since the last call go up (all of them after the mirror had to grow)"""
        a = self.taps
        if self._taps_dev is None or self._taps_dev.numel() < a.ints:
            self._taps_dev, self._taps_up = torch.empty(max(len(a.data), 1), dtype=torch.int32, device=self.dev), 0
        if self._taps_up < a.ints:
            self._taps_dev[self._taps_up:a.ints].copy_(torch.from_numpy(a.data[self._taps_up:a.ints]))
            self._taps_up = a.ints
            self.tap_uploads += 1
        return self._taps_dev

    @staticmethod
    def draw(n):
        """[(angle, flip_v, flip_h)] * n: the random decisions of n consecutive PolypDataset.__getitem__ calls with augmentation on
        (multiclass_seg/EMCAD/utils/dataloader.py:59-68).  Per sample the loader draws seed = np.random.randint(2147483647) and seeds torch's global generator
        with it before the image's transforms and again before the mask's, so both get the same decisions; here the seed goes to a private torch.Generator and
        the global one (DropPath, every other consumer) is left alone.  The draws are those of torchvision 0.8 to 0.12, in the order of the Compose:
        RandomRotation.get_params: float(torch.empty(1).uniform_(-90., 90.).item()); RandomVerticalFlip, then RandomHorizontalFlip: torch.rand(1) < 0.5.
        torchvision is not installed where this was written: the calls and their order are taken from its source as remembered, not checked against it."""
        out = []
        g = torch.Generator()
        for _ in range(int(n)):
            g.manual_seed(int(np.random.randint(2147483647)))
            angle = float(torch.empty(1).uniform_(-90., 90., generator=g).item())
            flip_v = bool(torch.rand(1, generator=g) < 0.5)
            flip_h = bool(torch.rand(1, generator=g) < 0.5)
            out.append((angle, flip_v, flip_h))
        return out

    def batch(self, images, masks=None, out=None, draws=None):
        """__call__ for the whole list at once: the same x (and g), bit for bit, from two kernel launches (pn2_input_batch_width / _height) whatever the list's
        length.  images / masks: uint8 arrays [H][W][3] / [H][W] of any sizes - numpy arrays, CPU tensors or tensors on this device; None is an empty slot,
        whose output sample is left as it was (out=(x, g) or out=x: tensors to fill instead of new ones).  Host inputs are packed behind the table in one pinned
        staging buffer and go up in ONE copy; device inputs are gathered with device copies and only the table goes up.  Tap blocks are cached per input size
        (self.taps), scratch is reused between calls; calls of one DeviceTransform belong on one stream.
        draws: one (angle, flip_v, flip_h) or None per image (draw(n) makes them) - the image and the mask in the same position are rotated (nearest, same size,
        fill 0) and flipped as Pillow would before the resize.  The width pass reads through the map (pn2_input_batch_width_aug): still two launches, and the
        second table rides in the same copy as the first.  draws=None makes exactly the calls of a batch without the argument."""
        S, st = self.size, _stream()
        n_img = len(images)
        items = list(images) + (list(masks) if masks is not None else [])
        arrs, shapes = [], []
        for i, a in enumerate(items):
            if a is not None:
                if isinstance(a, torch.Tensor):
                    if a.dtype != torch.uint8 or (a.is_cuda and a.device != self.dev):
                        raise RuntimeError("DeviceTransform.batch needs uint8 arrays on the host or on its own device")
                    a = (a[:, :, None] if a.dim() == 2 else a).contiguous()
                    if not a.is_cuda:
                        a = a.numpy()
                else:
                    a = np.asarray(a)
                    if a.dtype != np.uint8:
                        raise RuntimeError("DeviceTransform.batch needs uint8 arrays on the host or on its own device")
                    a = np.ascontiguousarray(a[:, :, None] if a.ndim == 2 else a)
                if len(a.shape) != 3 or a.shape[2] != (3 if i < n_img else 1):
                    raise RuntimeError("images must be RGB (rgb_loader converts to 'RGB', dataloader.py:133-136)" if i < n_img else "masks must have one channel")
            arrs.append(a)
            shapes.append(None if a is None else tuple(a.shape))
        x, g = (out if isinstance(out, (tuple, list)) else (out, None)) if out is not None else (None, None)
        if x is None:
            x = torch.empty((n_img, 3, S, S), dtype=torch.float32, device=self.dev)
        if g is None and masks is not None:
            g = torch.empty((len(masks), 1, S, S), dtype=torch.float32, device=self.dev)
        for t, n, c in ((x, n_img, 3), (g, len(items) - n_img, 1)):
            if t is not None and (tuple(t.shape) != (n, c, S, S) or t.dtype != torch.float32 or t.device != self.dev or not t.is_contiguous()):
                raise ValueError(f"out: contiguous fp32 [{n}][{c}][{S}][{S}] on {self.dev}")
        n = len(items)
        if draws is not None and len(draws) != n_img:
            raise ValueError(f"draws: one (angle, flip_v, flip_h) or None per image, got {len(draws)} for {n_img} images")
        if n:
            rows, src_bytes, tmp_bytes = batch_table(shapes, S, self.taps, dst=[i if i < n_img else i - n_img for i in range(n)], norm=[i < n_img for i in range(n)])
            aug = None
            if draws is not None:          # a mask takes the draw of the image in its position
                aug = aug_table(shapes, [draws[j] if j < n_img else None for j in (i if i < n_img else i - n_img for i in range(n))])
            up = n * SLOT.itemsize + (n * AUG.itemsize if aug is not None else 0)
            tb = _up(up, 256)          # the table (and the second one behind it) leads the arena: host inputs and tables travel in one copy
            if self._staged is not None:
                self._staged.synchronize()            # the previous batch's copy has left the staging buffer
            stage = self._buf("stage", tb + src_bytes, pinned=True)
            host = stage.numpy()
            host[:n * SLOT.itemsize] = rows.view(np.uint8).reshape(-1)
            if aug is not None:
                host[n * SLOT.itemsize:up] = aug.view(np.uint8).reshape(-1)
            for r, a in zip(rows, arrs):
                if a is not None and r["H"] > 0 and not isinstance(a, torch.Tensor):
                    lo = tb + int(r["src"])
                    host[lo:lo + a.size] = a.reshape(-1)
                    up = tb + src_bytes
            arena, tmp = self._buf("arena", tb + src_bytes), self._buf("tmp", tmp_bytes)
            arena[:up].copy_(stage[:up], non_blocking=True)
            if self._staged is None:
                self._staged = torch.cuda.Event()
            self._staged.record()
            for r, a in zip(rows, arrs):
                if isinstance(a, torch.Tensor) and r["H"] > 0:
                    lo = tb + int(r["src"])
                    arena[lo:lo + a.numel()].copy_(a.reshape(-1))
            taps = self._sync_taps()
            th, td, src = C.c_void_p(rows.ctypes.data), C.c_void_p(arena.data_ptr()), C.c_void_p(arena.data_ptr() + tb)
            if aug is None:
                call.pn2_input_batch_width(th, td, n, S, src, src_bytes, _p(tmp), tmp_bytes, _p(taps), self.taps.ints, st)
            else:
                ah, ad = C.c_void_p(aug.ctypes.data), C.c_void_p(arena.data_ptr() + n * SLOT.itemsize)
                call.pn2_input_batch_width_aug(th, td, ah, ad, n, S, src, src_bytes, _p(tmp), tmp_bytes, _p(taps), self.taps.ints, st)
            call.pn2_input_batch_height(th, td, n, S, _p(tmp), tmp_bytes, _p(taps), self.taps.ints, _p(x), n_img, _p(g), n - n_img, _p(self.mean), _p(self.std), st)
        return x if masks is None else (x, g)

    def _taps(self, in_size):
        hit = self._coeffs.get(in_size)
        if hit is None:
            S = self.size
            ks = call.pn2_resize_ksize(in_size, S)
            xmin, cnt, kk = np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros((S, ks), np.int32)
            call.pn2_resize_coeffs(in_size, S, C.c_void_p(xmin.ctypes.data), C.c_void_p(cnt.ctypes.data), C.c_void_p(kk.ctypes.data))
            hit = self._coeffs[in_size] = tuple(torch.from_numpy(a).to(self.dev) for a in (xmin, cnt, kk)) + (ks,)
        return hit

    def resize(self, img):
        """uint8 [H][W][C] or [H][W] on the device -> uint8 [S][S][C]: PIL.Image.resize((S, S), BILINEAR)."""
        if not img.is_cuda or img.dtype != torch.uint8:
            raise RuntimeError("DeviceTransform needs uint8 GPU tensors (no CPU fallback)")
        if img.dim() == 2:
            img = img[:, :, None]
        img = img.contiguous()
        H, W, Cc = img.shape
        S, st = self.size, _stream()
        if W != S:                                           # Pillow's order: width pass, then height pass
            xmin, cnt, kk, ks = self._taps(W)
            tmp = torch.empty((H, S, Cc), dtype=torch.uint8, device=self.dev)
            call.pn2_resize_u8_pass(_p(img), _p(tmp), H, W, Cc, S, 1, _p(xmin), _p(cnt), _p(kk), ks, st)
            img, W = tmp, S
        if H != S:
            xmin, cnt, kk, ks = self._taps(H)
            out = torch.empty((S, S, Cc), dtype=torch.uint8, device=self.dev)
            call.pn2_resize_u8_pass(_p(img), _p(out), H, W, Cc, S, 0, _p(xmin), _p(cnt), _p(kk), ks, st)
            img = out
        return img

    def __call__(self, images, masks=None):
        S, st = self.size, _stream()
        x = torch.empty((len(images), 3, S, S), dtype=torch.float32, device=self.dev)
        for i, im in enumerate(images):
            r = self.resize(im)
            if r.shape[2] != 3:
                raise RuntimeError("images must be RGB (rgb_loader converts to 'RGB', dataloader.py:133-136)")
            call.pn2_u8_to_tensor(_p(r), _p(x[i]), S, S, 3, _p(self.mean), _p(self.std), st)
        if masks is None:
            return x
        g = torch.empty((len(masks), 1, S, S), dtype=torch.float32, device=self.dev)
        for i, m in enumerate(masks):
            r = self.resize(m)
            call.pn2_u8_to_tensor(_p(r), _p(g[i]), S, S, 1, C.c_void_p(0), C.c_void_p(0), st)
        return x, g
