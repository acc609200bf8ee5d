"""Test-set evaluation throughput: the per-image path (Predictor.postprocess + eval_for_testAllInOne, one image at a time) against the ragged-batch path
(Predictor.test_with_eval) on synthetic 352^2 inputs whose ground-truth sizes cycle over the typical ones of the five polyp test sets.

    python tools/eval_bench.py [--images 64] [--reps 5] [--batch-sizes 1,8,16,32] [--dtype bf16]

Prints one JSON line per configuration: images/s from the median and the fastest of `reps` passes after a warm pass (which captures the graphs and sizes the
scratch), launches and blocking host syncs per image (counted from the call sequence), and the largest difference between the two paths' metrics."""
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
os.environ.setdefault("PN2_NO_PRETRAINED", "1")

import numpy as np
import torch

GT_SIZES = [(288, 384), (500, 574), (531, 622), (966, 1225)]          # CVC-ClinicDB, CVC-ColonDB, Kvasir (typical), ETIS-LaribPolypDB
METRICS = ["meanDic", "meanIoU", "wFm", "Sm", "meanEm", "mae"]


def make_set(n, S, dev):
    g = torch.Generator(device="cpu").manual_seed(0)
    items = []
    for i in range(n):
        H, W = GT_SIZES[i % len(GT_SIZES)]
        yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        cy, cx = H * (0.35 + 0.3 * ((i * 7) % 10) / 10), W * (0.35 + 0.3 * ((i * 3) % 10) / 10)
        gt = ((((yy - cy) / (0.18 * H)) ** 2 + ((xx - cx) / (0.22 * W)) ** 2) < 1).float()
        items.append((torch.randn(1, 3, S, S, generator=g).to(dev), gt.to(dev), f"{i}.png"))
    return items


def timed(fn, reps):
    fn()          # warm pass
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return out, ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, default=352)
    ap.add_argument("--batch-sizes", default="1,8,16,32")
    ap.add_argument("--dtype", default="bf16")
    a = ap.parse_args()
    import pn2
    from pn2.evaltail import eval_for_testAllInOne
    from pn2.infer import Predictor
    from lib.pranet import PraNet_V2
    dev = torch.device("cuda", 0)
    pn2.set_compute_dtype(a.dtype)
    torch.manual_seed(0)
    model = PraNet_V2(num_class=1).to(dev).eval()
    items = make_set(a.images, a.size, dev)
    opt = {"metrics": METRICS}
    n = len(items)

    def per_image():
        pred = per_image.pred
        res = np.zeros((n, len(METRICS)))
        for j, (image, gt, _) in enumerate(items):
            gt = gt / (gt.max() + 1e-8)
            res[j] = eval_for_testAllInOne(opt, pred.postprocess(image, gt.shape), gt)
        return res
    per_image.pred = Predictor(model)
    ref, ts = timed(per_image, a.reps)
    # graph replay + 3 adds + resize + 3 tail + hist + 2 region + 3 wFm; blocking copies: hist, out25, part
    print(json.dumps({"path": "per_image", "images": n, "images_per_s_median": n / statistics.median(ts), "images_per_s_best": n / min(ts),
                      "spread": (max(ts) - min(ts)) / statistics.median(ts), "launches_per_image": 14, "host_syncs_per_image": 3}), flush=True)
    for bs in [int(v) for v in a.batch_sizes.split(",")]:
        pred = Predictor(model)
        (res, _), ts = timed(lambda: pred.test_with_eval(items, opt, batch_size=bs), a.reps)
        both = np.isfinite(ref) & np.isfinite(res)
        # per batch: graph replay + 2 tail + 2 counts + 3 wFm + the concatenations of the images and of the ground truths; one blocking copy
        print(json.dumps({"path": "test_with_eval", "batch_size": bs, "images": n, "images_per_s_median": n / statistics.median(ts), "images_per_s_best": n / min(ts),
                          "spread": (max(ts) - min(ts)) / statistics.median(ts), "launches_per_image": round(10 / bs, 3), "host_syncs_per_image": round(1 / bs, 3),
                          "graphs": len(pred._states), "max_abs_diff_vs_per_image": float(np.abs(ref - res)[both].max())}), flush=True)


if __name__ == "__main__":
    main()
