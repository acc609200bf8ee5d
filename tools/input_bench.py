"""Input-transform throughput: the per-image path (DeviceTransform.__call__ on arrays copied to the device one by one, what get_loader(batched=False) does)
against the ragged-batch path (DeviceTransform.batch on the host arrays) at S = 352, on a fixed, seeded mix of the source sizes recorded in the fixtures
tests/golden/input_pipeline.npz and eval_full.npz.  Inputs are host arrays, so the host-to-device copies count; file decoding is not part of either path.

    python tools/input_bench.py [--images 1024] [--loops 16] [--reps 7] [--batch-sizes 1,16,32] [--size 352] [--aug-batch-size 32] [--aug-loops 8]

Prints one JSON line per (batch size, with / without masks): images/s of both paths from the median and the fastest of `reps` timed passes, each `loops` times
over the set (a window of 0.1 s to 1 s) and ending in a device synchronise; the two paths alternate pass by pass after a warm pass of each (which fills the tap
caches and sizes the buffers).  Launches and host-to-device copies per batch are counted from the call sequence, and `equal` says whether the two
paths returned the same bits.  A last line ("augmented": true) times the loaders' augmentation on the same set with masks: PIL rotate and transposes on the host
followed by batch(), against batch(draws=...) (see augmented())."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pranet-v2_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

# (H, W) of every array in the two fixtures
SIZES = [(211, 257), (61, 47), (90, 150), (37, 53), (64, 64), (160, 120), (64, 80), (100, 77), (352, 352), (40, 53)]


def make_set(n, seed=0):
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, len(SIZES), n)
    imgs = [torch.from_numpy(rng.integers(0, 256, SIZES[k] + (3,), dtype=np.uint8)) for k in pick]
    gts = [torch.from_numpy((rng.random(SIZES[k]) > 0.6).astype(np.uint8) * 255) for k in pick]
    return imgs, gts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--loops", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--size", type=int, default=352)
    ap.add_argument("--batch-sizes", default="1,16,32", help="batch sizes of the per-image / batch lines ('' for none)")
    ap.add_argument("--aug-batch-size", type=int, default=32, help="batch size of the augmented line (0: no such line)")
    ap.add_argument("--aug-loops", type=int, default=8)
    a = ap.parse_args()
    from pn2.input import DeviceTransform
    if not torch.cuda.is_available():
        raise SystemExit("input_bench needs a GPU: a CPU run measures nothing")
    imgs, gts = make_set(a.images)
    n = len(imgs)
    for with_masks in (True, False):
        for bs in [int(v) for v in a.batch_sizes.split(",") if v]:
            t = DeviceTransform(a.size)
            chunks = [(imgs[i:i + bs], gts[i:i + bs] if with_masks else None) for i in range(0, n, bs)]

            def per_image():
                out = None
                for im, gt in chunks * loops[0]:
                    out = t([x.cuda(non_blocking=True) for x in im], None if gt is None else [x.cuda(non_blocking=True) for x in gt])
                return out

            def batched():
                out = None
                for im, gt in chunks * loops[0]:
                    out = t.batch(im, gt)
                return out
            ts = {"per_image": [], "batch": []}
            last = {}
            loops = [1]
            for rep in range(a.reps + 1):
                for name, fn in (("per_image", per_image), ("batch", batched)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    last[name] = fn()
                    torch.cuda.synchronize()
                    if rep:          # pass 0 (once over the set) warms both paths up
                        ts[name].append(time.perf_counter() - t0)
                loops[0] = a.loops
            pi, ba = last["per_image"], last["batch"]
            equal = all(torch.equal(u, v) for u, v in zip(pi, ba)) if with_masks else torch.equal(pi, ba)
            k = 2 if with_masks else 1
            n_timed = n * a.loops
            row = {"batch_size": bs, "masks": with_masks, "images": n_timed, "size": a.size, "equal": bool(equal),
                   # per image: up to 2 resize passes + to_tensor, and one copy, for the image and again for its mask; batch: 2 launches, 1 copy
                   "launches_per_batch": {"per_image": 3 * k * bs, "batch": 2}, "h2d_copies_per_batch": {"per_image": k * bs, "batch": 1}}
            for name in ("per_image", "batch"):
                med = statistics.median(ts[name])
                row[name] = {"images_per_s_median": n_timed / med, "images_per_s_best": n_timed / min(ts[name]), "spread": (max(ts[name]) - min(ts[name])) / med}
            row["ratio_median"] = row["batch"]["images_per_s_median"] / row["per_image"]["images_per_s_median"]
            print(json.dumps(row), flush=True)
    if a.aug_batch_size > 0:
        augmented(a, imgs, gts)


def augmented(a, imgs, gts):
    """The augmented line: pairs rotated and flipped by seeded draws.  `host_pil` is what a user of batch() without draws has to do - Image.rotate(NEAREST) and
    the two transposes on the host for every image and mask, then DeviceTransform.batch; `device` is batch(draws=...), the same two launches reading through the
    map.  Same set, same S, host arrays in; wrapping an array as a PIL image and reading the result back are part of the host path, as they are for that user."""
    from PIL import Image
    from pn2.input import DeviceTransform
    bs, n = a.aug_batch_size, len(imgs)
    np.random.seed(0)
    draws = DeviceTransform.draw(n)
    t = DeviceTransform(a.size)
    chunks = [(imgs[i:i + bs], gts[i:i + bs], draws[i:i + bs]) for i in range(0, n, bs)]

    def pil(arr, d):
        im = Image.fromarray(arr.numpy()).rotate(d[0], Image.NEAREST, expand=False)
        if d[1]:
            im = im.transpose(Image.FLIP_TOP_BOTTOM)
        if d[2]:
            im = im.transpose(Image.FLIP_LEFT_RIGHT)
        return np.asarray(im)

    def host_pil():
        out = None
        for im, gt, dr in chunks * loops[0]:
            out = t.batch([pil(x, d) for x, d in zip(im, dr)], [pil(x, d) for x, d in zip(gt, dr)])
        return out

    def device():
        out = None
        for im, gt, dr in chunks * loops[0]:
            out = t.batch(im, gt, draws=dr)
        return out
    ts = {"host_pil": [], "device": []}
    last = {}
    loops = [1]
    for rep in range(a.reps + 1):
        for name, fn in (("host_pil", host_pil), ("device", device)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[name] = fn()
            torch.cuda.synchronize()
            if rep:
                ts[name].append(time.perf_counter() - t0)
        loops[0] = a.aug_loops
    n_timed = n * a.aug_loops
    row = {"augmented": True, "batch_size": bs, "masks": True, "images": n_timed, "size": a.size,
           "equal": bool(all(torch.equal(u, v) for u, v in zip(last["host_pil"], last["device"]))), "launches_per_batch": {"host_pil": 2, "device": 2},
           "h2d_copies_per_batch": {"host_pil": 1, "device": 1}}
    for name in ("host_pil", "device"):
        med = statistics.median(ts[name])
        row[name] = {"images_per_s_median": n_timed / med, "images_per_s_best": n_timed / min(ts[name]), "spread": (max(ts[name]) - min(ts[name])) / med}
    row["ratio_median"] = row["device"]["images_per_s_median"] / row["host_pil"]["images_per_s_median"]
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
