"""Inference driver: the eval-mode forward of MyTest_med.py:98-104 (+ its post-processing :104-111) replayed from one hipGraph.

The nn.Module surface launches ~450 small kernels per image from Python; for a fixed input shape the whole pass - forward, sum of the four
foreground maps, bilinear resize to the ground-truth size, sigmoid, min-max, uint8 - is captured once and replayed."""
import ctypes as C

import torch

from . import evaltail
from .capi import call, F32
from .engine import Act, BnFoldCache, Engine, PackCache, StepArena, TUNER, _p, _stream
from .graph import get_compute_dtype
from .volinput import zoom
from .voleval import AVERAGES, MODES, flip_views, parse_tta, predict_labels_up, predict_labels_up_tta, volume_dice, volume_metrics


class Predictor:
    """p = Predictor(model.eval()); outs = p(images)            # the model's output tuple, fp32 NCHW GPU tensors (valid until the next call)
                                      u8 = p.postprocess(images, (H, W))   # MyTest_med.py:104-111 -> uint8 (H, W) map for one image
                                      res_i, mean = p.test_with_eval(loader, opt, batch_size=16)   # MyTest_med.py:26-45 for one data set, batched (ragged ground-truth sizes)"""

    def __init__(self, model, dtype=None):
        self.model = model
        self.dtype = get_compute_dtype() if dtype is None else dtype          # compute mode (BF16 / F32 / F32F / F32X3), kept for the object's life
        self.pack_cache = PackCache()
        self.bn_fold = BnFoldCache()    # folded BatchNorm rows of every layer: one table-driven launch per forward (inside the graph: the live statistics are used)
        self._states = {}               # input shape -> captured forward (insertion order = LRU order)
        self.max_shapes = 8

    def _forward(self, st, x, build=None):
        self.pack_cache.refresh()
        self.bn_fold.refresh()
        if st["arena"] is not None:
            st["arena"].begin_step(x.device)
        eng = Engine(self.dtype, False, need_grad=False, pack_cache=self.pack_cache, tuner=TUNER, arena=st["arena"], bn_fold=self.bn_fold)
        outs = (build or self.model._build)(eng, eng.from_nchw(x))
        eng.finish_forward()
        return eng, outs

    def _check_weights(self):
        """The packed-panel job table and the captured graphs bake raw weight pointers in: if anything re-allocated a parameter since (a Trainer built
        over the same model re-points p.data into its flat arena), start over instead of repacking from freed storage."""
        pc = self.pack_cache
        if (pc.keep and any(j.w != w.data_ptr() for j, w in zip(pc.jobs, pc.keep))) or self.bn_fold.stale():
            self.pack_cache = PackCache()
            self.bn_fold = BnFoldCache()
            self._states = {}

    def _state(self, x):
        """One captured forward per INPUT shape (test sets have one test size but a different ground-truth size for almost every image: the
        sum -> resize -> sigmoid -> min-max -> uint8 tail of MyTest_med.py:104-111 runs eagerly, 6 launches, on the replayed maps)."""
        def run(st):
            eng, outs = self._forward(st, st["x"])
            return tuple(eng.to_nchw(o) for o in outs)
        return self._captured(tuple(x.shape), x, run)

    def _captured(self, key, x, run, static=None):
        """The state of `key`, captured on first use: run(st) is the pass over the static input st["x"] (a clone of x); what it returns stays in st["out"].
        static(): further buffers of a new state that the pass writes."""
        self._check_weights()
        st = self._states.get(key)
        if st is None:
            if self.model.training:
                raise RuntimeError("Predictor runs eval-mode BatchNorm: call model.eval() first")
            if len(self._states) >= self.max_shapes:          # bounded: evict the least recently used input shape
                self._states.pop(next(iter(self._states)))
            st = self._states[key] = {"arena": StepArena(), "graph": None, "x": x.clone(), "out": None, **(static() if static else {})}
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(2):              # pass 1 sizes the arena and tunes, pass 2 runs on the addresses the graph will replay
                    run(st)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            st["graph"] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(st["graph"]):
                st["out"] = run(st)
        else:
            self._states[key] = self._states.pop(key)          # most recently used last
        return st

    def __call__(self, images):
        if not images.is_cuda:
            raise RuntimeError("pn2.infer needs GPU tensors (no CPU fallback)")
        st = self._state(images)
        st["x"].copy_(images, non_blocking=True)
        st["graph"].replay()
        return st["out"]

    def postprocess(self, images, gt_shape, maps="sum4"):
        """uint8 (H, W) prediction map of one image, as MyTest_med.py:104-111 writes it to disk.  maps="sum4": res2 + res3 + res4 + res5 (the V2 branch, :104-108);
        maps="last": the last map of the model's tuple alone (the V1 branch's res2, :98-102)."""
        assert images.shape[0] == 1
        if maps not in ("sum4", "last"):
            raise ValueError(f"maps {maps!r}: 'sum4' or 'last'")
        outs = self(images)
        H, W = int(gt_shape[0]), int(gt_shape[1])
        eng = Engine(F32, False, need_grad=False)
        src = outs[:4] if maps == "sum4" else outs[-1:]
        maps = [eng.from_nchw(o, dt=F32) if o.shape[1] != 1 else Act(eng, o.reshape(o.shape[0], o.shape[2], o.shape[3], 1), 1, 1, 1, F32, requires_grad=False) for o in src]
        s_ = eng.add(eng.add(eng.add(maps[0], maps[1]), maps[2]), maps[3]) if len(maps) == 4 else maps[0]              # res2 + res3 + res4 + res5 (MyTest_med.py:104)
        r = eng.resize_to(s_, H, W, align_corners=False)
        u8 = torch.empty((H, W), dtype=torch.uint8, device=images.device)
        scratch = torch.empty(2 + 2 * 512, dtype=torch.float32, device=images.device)
        call.pn2_eval_tail(r.ptr, _p(u8), _p(scratch), r.M, _stream())
        return u8

    def postprocess_batch(self, images, gt_shapes, maps="sum4"):
        """postprocess for a batch: images [B][3][S][S], gt_shapes up to B sizes (H, W), None = a filler slot.  One graph replay, then the two launches of
        pn2_eval_tail_batch.  Returns (packed uint8 predictions, RaggedViews of (H, W) views, one per slot): pn2.evaltail.postprocess_batch."""
        return evaltail.postprocess_batch(self(images), gt_shapes, maps)

    def evaluate(self, images, gts, opt, maps="sum4"):
        """The metric rows of one batch: images [B][3][S][S], gts up to B ground truths (H, W) on the GPU, already scaled to [0, 1] (None = a filler slot) ->
        ndarray [len(gts) without fillers][len(opt["metrics"])], eval_for_testAllInOne of every image (pn2.evaltail.eval_batch)."""
        gts = list(gts)
        for g in gts:
            if g is not None and not g.is_cuda:
                raise RuntimeError("pn2.infer needs GPU tensors (no CPU fallback)")
        packed, views = self.postprocess_batch(images, [None if g is None else tuple(g.shape[-2:]) for g in gts], maps)
        return evaltail.eval_batch(opt, packed, views, gts + [None] * (images.shape[0] - len(gts)))

    def test_with_eval(self, loader, opt, batch_size=16, maps="sum4"):
        """MyTest_med.py:26-45 for one data set: loader yields (image [1][3][S][S], gt, name) as utils.dataloader.test_dataset.load_data does (gt: a PIL image,
        an array or a tensor [H][W]); gt /= gt.max() + 1e-8 as :31-32.  Returns (res_i [n][len(opt["metrics"])], its column mean).  Images go through the graph of
        ONE batch shape: the last batch is filled with zero images whose table slots are empty (eval-mode BatchNorm keeps the samples independent), so a
        second pass over the set captures nothing.  A loader with load_batch(k) (test_dataset) is asked for whole batches instead: one input transform per batch."""
        import numpy as np
        B = int(batch_size)
        if B < 1:
            raise ValueError("batch_size >= 1")
        dev = next(self.model.parameters()).device
        rows, imgs, gts = [], [], []

        def flush():
            x = torch.cat(imgs)
            if x.shape[0] < B:
                x = torch.cat([x, x.new_zeros((B - x.shape[0],) + tuple(x.shape[1:]))])
            rows.append(self.evaluate(x, gts, opt, maps))
            imgs.clear()
            gts.clear()

        def scaled(gt):
            if isinstance(gt, torch.Tensor):
                g = gt.to(dev).float().reshape(gt.shape[-2], gt.shape[-1])
                return g / (g.max() + 1e-8)
            g = np.asarray(gt, np.float32).copy()
            g /= (g.max() + 1e-8)
            return torch.from_numpy(g).to(dev)
        if hasattr(loader, "load_batch"):          # utils.dataloader.test_dataset: the rest of the set, a batch per transform call
            while True:
                images, batch_gts, _names = loader.load_batch(B)
                if not batch_gts:
                    break
                imgs.append(images.to(dev).float())
                gts.extend(scaled(gt) for gt in batch_gts)
                flush()
            loader = ()
        for image, gt, _name in loader:
            imgs.append(image.to(dev).float())
            gts.append(scaled(gt))
            if len(imgs) == B:
                flush()
        if imgs:
            flush()
        res_i = np.concatenate(rows) if rows else np.zeros((0, len(opt["metrics"])))
        return res_i, np.mean(res_i, axis=0)


class VolumePredictor(Predictor):
    """The multi-class volume inference of test_single_volume / val_single_volume (multiclass_seg/EMCAD/utils/utils.py:165-301) from captured graphs:
           vp = VolumePredictor(model.eval(), patch_size=(224, 224), batch_size=16)
           labels = vp.predict(image, "sum_fg")                         # image [D][H][W] or [H][W] on the GPU -> uint8 labels of the same shape
           vp.test_single_volume(image, label, classes, use_dual=True)  # -> [(dice, hd95, jaccard, asd)] as pn2.voleval.test_single_volume
           vp.val_single_volume(image, label, classes, use_dual=True)   # -> [dice]                       as pn2.voleval.val_single_volume
    One graph per (batch, patch height, patch width, mode) holds the eval forward up to the low-resolution head maps (model._build_lowres) and ONE launch
    that turns them into the uint8 labels of the batch (pn2_seg_labels_up): the full-resolution K-class maps never exist.  The spline zoom going in, the order-0
    zoom coming out and the metric kernels stay outside (volume sizes vary; their tables are cached on the host, pn2/volinput.py).
    tta: flip test-time augmentation (the reference's tta_model, utils.py:303-325) - None, "flips" (= ("id", "h", "v"), the reference's three views) or a tuple of
    views from "id", "h" (x mirrored), "v" (y mirrored), "hv" without repeats.  tta_average "prob" adds the views' softmax probabilities (the reference's mean of
    predicted masks), "logit" their combined logits; the sum is not divided by the number of views (the argmax does not see it).  See _labels_tta."""

    def __init__(self, model, patch_size=(224, 224), batch_size=16, dtype=None, tta=None, tta_average="prob"):
        super().__init__(model, dtype)
        if not hasattr(model, "_build_lowres"):
            raise TypeError("VolumePredictor needs a model with K-class head maps (lib.networks.EMCADNet)")
        self.patch_size = (int(patch_size[0]), int(patch_size[1]))
        self.batch_size = int(batch_size)
        if self.batch_size < 1:
            raise ValueError("batch_size >= 1")
        self.views = parse_tta(tta)          # None: no test-time augmentation
        if tta_average not in AVERAGES:
            raise ValueError(f"tta_average {tta_average!r}: one of {sorted(AVERAGES)}")
        self.tta_average = tta_average

    @staticmethod
    def _pick(lows, scales, mode):
        """The maps of a mode, as voleval.test_single_volume / val_single_volume pick them from the model's output list."""
        sel = {"last": slice(-1, None), "sum_fg": slice(0, 4)}.get(mode)
        if sel is not None:
            return lows[sel], scales[sel]
        return lows[:4] + lows[-4:], scales[:4] + scales[-4:]

    def _labels(self, xb, mode):
        """xb [B][1][h][w] fp32 -> the state whose st["labels"] (uint8 [B][h][w]) holds the labels of xb until the next call with this shape and mode."""
        if mode not in MODES:
            raise ValueError(f"mode {mode!r}: one of {sorted(MODES)}")
        if not xb.is_cuda:
            raise RuntimeError("pn2.infer needs GPU tensors (no CPU fallback)")
        if self.model.training:          # on every call: a replay would go on serving the eval-mode graph
            raise RuntimeError("VolumePredictor runs eval-mode BatchNorm: call model.eval() first")
        B, _, h, w = xb.shape
        if self.views is not None:
            return self._labels_tta(xb, mode)

        def run(st):
            eng, (lows, scales) = self._forward(st, st["x"], self.model._build_lowres)
            st["lows"] = lows
            maps, sc = self._pick([a.t[..., :a.C] for a in lows], list(scales), mode)
            return predict_labels_up(maps, sc, mode, out=st["labels"])
        st = self._captured((B, h, w, mode), xb, run, lambda: {"labels": torch.empty((B, h, w), dtype=torch.uint8, device=xb.device), "lows": None})
        st["x"].copy_(xb, non_blocking=True)
        st["graph"].replay()
        return st

    def _labels_tta(self, xb, mode):
        """_labels under flip test-time augmentation (tta_model, utils.py:303-325): the graph of key (B, h, w, mode, views, average) holds pn2_flip_views (the
        V * B mirrored samples, view v of sample n at v * B + n), ONE eval forward over them (eval-mode BatchNorm keeps them independent) and one
        pn2_seg_labels_up_tta launch that reads every view at the mirrored pixel and adds the views: neither a flipped nor a full-resolution K-class map exists."""
        B, _, h, w = xb.shape
        V = len(self.views)

        def run(st):
            flip_views(st["x"], self.views, out=st["xv"])
            eng, (lows, scales) = self._forward(st, st["xv"], self.model._build_lowres)
            st["lows"] = lows
            maps, sc = self._pick([a.t[..., :a.C] for a in lows], list(scales), mode)
            return predict_labels_up_tta(maps, sc, mode, self.views, self.tta_average, out=st["labels"])
        st = self._captured((B, h, w, mode, self.views, self.tta_average), xb, run,
                            lambda: {"labels": torch.empty((B, h, w), dtype=torch.uint8, device=xb.device), "lows": None,
                                     "xv": torch.empty((V * B, 1, h, w), dtype=torch.float32, device=xb.device)})
        st["x"].copy_(xb, non_blocking=True)
        st["graph"].replay()
        return st

    def lowres(self, xb, mode="last"):
        """Debugging / tests: clones of the low-resolution head maps of one batch xb [B][1][h][w], NCHW fp32, as the graph of `mode` leaves them (with test-time
        augmentation: of the V * B mirrored samples)."""
        st = self._labels(xb.float(), mode)
        return [a.t[..., :a.C].permute(0, 3, 1, 2).clone() for a in st["lows"]]

    def predict(self, image, mode):
        """uint8 label volume of image [D][H][W] (or of one image [H][W], which is not resampled: utils.py:224-231).  Slices whose size differs from patch_size are
        resampled as the reference does; a last batch shorter than batch_size is filled with zero slices (eval-mode BatchNorm keeps the samples independent)."""
        x = image.float()
        if x.dim() == 2:
            return self._labels(x[None, None].contiguous(), mode)["labels"][0].clone()
        D, H, W = x.shape
        ph, pw = self.patch_size
        B = self.batch_size
        preds = []
        for i in range(0, D, B):
            xb = zoom(x[i:i + B], (ph, pw), 3)
            n = xb.shape[0]
            if n < B:
                xb = torch.cat([xb, xb.new_zeros((B - n, ph, pw))])
            lab = self._labels(xb[:, None], mode)["labels"][:n]
            preds.append(zoom(lab, (H, W), 0) if (H, W) != (ph, pw) else lab.clone())          # (the next replay rewrites the static buffer)
        return torch.cat(preds)

    def test_single_volume(self, image, label, classes, use_dual=None):
        image, label = image.squeeze(0), label.squeeze(0)
        pred = self.predict(image, "sum_fg" if use_dual and image.dim() == 3 else "last")
        return volume_metrics(pred, label, classes)

    def val_single_volume(self, image, label, classes, use_dual=False):
        image, label = image.squeeze(0), label.squeeze(0)
        return volume_dice(self.predict(image, "sum_fg_minus_bg" if use_dual else "last"), label, classes)
