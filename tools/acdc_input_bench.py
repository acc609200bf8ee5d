"""ACDC slice pipeline timings: the ragged-batch path of pn2/volinput.py (RaggedSliceTransform, val_slices) against what served such a batch before it.

    python tools/acdc_input_bench.py [--reps 5] [--host-reps 2] [--val-slices 100] [--no-val] [--trace N]

One JSON line per measurement.  Every device figure is the median of `reps` runs after one warm run, each between a pair of events on the current stream, and the wall
clock of the same runs around a device synchronise (the host work of a batch - planning, the copies - shows only there).
  train:    seeded ragged batches of 12 and 24 ACDC-like slices to 224^2 and 256^2 with SliceTransform.draw's decisions: host arrays in and device tensors in, against
            (a) numpy / scipy on the host with the copies to the device and (b) a per-sample loop over the uniform device functions (zoom, rotate, rot_flip) for the
            samples those can serve (rot_flip needs a square sample) - `served` says how many.
  uniform:  24 x 512^2 -> 224^2 through RaggedSliceTransform against SliceTransform, the same draws.
  val:      val_slices over `--val-slices` slices (EMCADNet pvt_v2_b0, K = 4, 224^2, batches of 16) against a per-slice loop over VolumePredictor.predict.
--trace N runs N training batches of 24 and nothing else: under a kernel trace every pn2 ragged kernel then shows N calls."""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pranet-v2_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ.setdefault("PN2_NO_PRETRAINED", "1")

import numpy as np
import torch

# in-plane sizes of the kind ACDC's patients have (each patient their own; non-square, some already at a patch size)
SIZES = [(154, 224), (216, 256), (184, 232), (208, 256), (256, 216), (224, 154), (174, 208), (224, 224), (256, 256), (232, 288), (192, 240), (200, 256)]


def make_batch(n, seed):
    g = np.random.default_rng(seed)
    pick = g.integers(0, len(SIZES), n)
    imgs = [(g.random(SIZES[k]) * 2.0 - 0.3).astype(np.float32) for k in pick]
    labs = [g.integers(0, 4, SIZES[k]).astype(np.uint8) for k in pick]
    random.seed(seed); np.random.seed(seed)
    from pn2.volinput import SliceTransform
    return imgs, labs, SliceTransform.draw(n)


def timed(f, reps):
    """(median device ms between two events, median wall ms around a synchronise, the last result) of `reps` runs after one warm run."""
    out = f()
    torch.cuda.synchronize()
    dev, wall = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        out = f()
        b.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(a.elapsed_time(b))
    return statistics.median(dev), statistics.median(wall), out


def host_path(imgs, labs, draws, size):
    from scipy import ndimage
    ims, lbs = [], []
    for im, lb, d in zip(imgs, labs, draws):
        if d is not None and d[0] == "rot_flip":
            im, lb = np.flip(np.rot90(im, d[1]), axis=d[2]).copy(), np.flip(np.rot90(lb, d[1]), axis=d[2]).copy()
        elif d is not None:
            im, lb = ndimage.rotate(im, d[1], order=0, reshape=False), ndimage.rotate(lb, d[1], order=0, reshape=False)
        x, y = im.shape
        if (x, y) != size:
            im, lb = ndimage.zoom(im, (size[0] / x, size[1] / y), order=3), ndimage.zoom(lb, (size[0] / x, size[1] / y), order=0)
        ims.append(im.astype(np.float32)[None])
        lbs.append(lb.astype(np.int64))
    return {"image": torch.from_numpy(np.stack(ims)).cuda(), "label": torch.from_numpy(np.stack(lbs)).cuda()}


def per_sample(imgs, labs, draws, size):
    """The uniform device functions, one sample at a time; a sample they cannot serve (rot_flip of a non-square one) is left out."""
    from pn2 import volinput as V
    out = []
    for im, lb, d in zip(imgs, labs, draws):
        if d is not None and d[0] == "rot_flip" and im.shape[0] != im.shape[1]:
            continue
        x, l = torch.from_numpy(im).cuda(), torch.from_numpy(lb).cuda()
        if d is not None and d[0] == "rot_flip":
            x, l = V.rot_flip(x, d[1], d[2]), V.rot_flip(l, d[1], d[2])
        elif d is not None:
            x, l = V.rotate(x, d[1]), V.rotate(l, d[1])
        out.append((V.zoom(x, size, 3), V.zoom(l, size, 0).long()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--val-slices", type=int, default=100)
    ap.add_argument("--no-val", action="store_true")
    ap.add_argument("--trace", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("acdc_input_bench needs a GPU: a CPU run measures nothing")
    from pn2 import volinput as V
    if a.trace:
        imgs, labs, draws = make_batch(24, 1)
        t = V.RaggedSliceTransform((224, 224))
        for _ in range(a.trace):
            t(imgs, labs, draws)
        torch.cuda.synchronize()
        return
    for size in ((224, 224), (256, 256)):
        for n in (12, 24):
            imgs, labs, draws = make_batch(n, n + size[0])
            t = V.RaggedSliceTransform(size)
            dimgs, dlabs = [torch.from_numpy(x).cuda() for x in imgs], [torch.from_numpy(x).cuda() for x in labs]
            hd, hw, got = timed(lambda: t(imgs, labs, draws), a.reps)
            dd, dw, got_d = timed(lambda: t(dimgs, dlabs, draws), a.reps)
            pd, pw, served = timed(lambda: per_sample(imgs, labs, draws, size), a.reps)
            line = {"train": True, "n": n, "size": size[0], "shapes": len({x.shape for x in imgs}), "ragged_host_in_ms": round(hd, 3), "ragged_host_in_wall_ms": round(hw, 3),
                    "ragged_device_in_ms": round(dd, 3), "ragged_device_in_wall_ms": round(dw, 3), "per_sample_ms": round(pd, 3), "per_sample_wall_ms": round(pw, 3),
                    "served": len(served), "equal_device_in": bool(torch.equal(got["image"], got_d["image"]) and torch.equal(got["label"], got_d["label"]))}
            try:
                _, sw, want = timed(lambda: host_path(imgs, labs, draws, size), a.host_reps)
                line["scipy_host_wall_ms"] = round(sw, 1)
                line["equal_scipy"] = bool(torch.equal(got["image"], want["image"]) and torch.equal(got["label"], want["label"]))
            except ImportError:
                line["scipy_host_wall_ms"] = None
            print(json.dumps(line), flush=True)
    # ---- a uniform batch through both transforms
    g = np.random.default_rng(0)
    x = torch.from_numpy((g.random((24, 512, 512)) * 2.0 - 0.3).astype(np.float32)).cuda()
    l = torch.from_numpy(g.integers(0, 9, (24, 512, 512)).astype(np.uint8)).cuda()
    random.seed(0); np.random.seed(0)
    draws = V.SliceTransform.draw(24)
    ut, rt = V.SliceTransform((224, 224)), V.RaggedSliceTransform((224, 224))
    xs, ls = list(x), list(l)
    ud, uw, want = timed(lambda: ut(x, l, draws), a.reps)
    rd, rw, got = timed(lambda: rt(xs, ls, draws), a.reps)
    nd, nw, _ = timed(lambda: rt(xs, ls, [None] * 24), a.reps)          # no geometry: what the first-pass read map costs shows against this
    un, unw, _ = timed(lambda: ut(x, l, [None] * 24), a.reps)
    print(json.dumps({"uniform": True, "n": 24, "src": 512, "size": 224, "slice_transform_ms": round(ud, 3), "slice_transform_wall_ms": round(uw, 3), "ragged_ms": round(rd, 3),
                      "ragged_wall_ms": round(rw, 3), "slice_transform_no_geometry_ms": round(un, 3), "ragged_no_geometry_ms": round(nd, 3), "ragged_no_geometry_wall_ms": round(nw, 3),
                      "equal": bool(torch.equal(got["image"], want["image"]) and torch.equal(got["label"], want["label"])),
                      "draws": {"rot_flip": sum(1 for d in draws if d and d[0] == "rot_flip"), "rotate": sum(1 for d in draws if d and d[0] == "rotate")}}), flush=True)
    if a.no_val:
        return
    # ---- val(): ragged batches against a per-slice loop
    from lib.networks import EMCADNet
    from pn2 import voleval as E
    from pn2.infer import VolumePredictor
    m = EMCADNet(num_classes=4, kernel_sizes=[1, 3, 5], expansion_factor=2, dw_parallel=True, add=True, lgag_ks=3, activation="relu6", encoder="pvt_v2_b0", pretrain=False, dual=True)
    m.backbone.reset_drop_path(0.0)
    m = m.cuda().eval()
    imgs, labs, _ = make_batch(a.val_slices, 7)
    vp, vp1 = VolumePredictor(m, (224, 224), 16), VolumePredictor(m, (224, 224), 1)

    def loop():
        out = []
        for im, lb in zip(imgs, labs):
            pred = vp1.predict(torch.from_numpy(im).cuda()[None], "sum_fg_minus_bg")[0]
            out.append(V.dice_counts(pred.reshape(-1), torch.from_numpy(lb).cuda().reshape(-1), [im.shape])[0])
        c = np.stack(out)
        return np.where(c[:, 1] + c[:, 2] > 0, 2.0 * c[:, 0] / np.maximum(c[:, 1] + c[:, 2], 1), 0.0)
    _, vw, (dice, mean) = timed(lambda: E.val_slices(imgs, labs, vp, 224, "sum_fg_minus_bg"), 3)
    _, lw, want = timed(loop, 3)
    print(json.dumps({"val": True, "slices": a.val_slices, "batch": 16, "val_slices_wall_ms": round(vw, 2), "per_slice_loop_wall_ms": round(lw, 2), "equal": bool(np.array_equal(dice, want)),
                      "mean_dice": mean}), flush=True)


if __name__ == "__main__":
    main()
