"""Flip test-time augmentation of pn2.infer.VolumePredictor, timed on one GPU: EMCADNet(dual, K = 9, pvt_v2_b2) with seeded weights, bf16, one batch of
B = 16 slices at config 5's 512 x 512, the reference's three views ("flips" = id, h, v).

    python tools/tta_bench.py [--batch 16] [--size 512] [--reps 20] [--warm 3] [--encoder pvt_v2_b2]

One JSON line per measurement, every figure the median (min - max) in ms of `reps` runs after `warm` warm runs, each between a pair of events on the current
stream; the two sides of a comparison alternate run by run inside one process.
  tail    per mode and average: ONE pn2_seg_labels_up_tta launch over the V * B low-resolution maps the TTA graph left, against the unfused composition of the
          ops the project had before it: Engine.bilinear of every map of every view (V * nmaps full-resolution K-class maps), torch.flip back, the fp32 sums,
          softmax for "prob", the sum over the views and argmax; its ops allocate their outputs inside the timed region, as they do wherever they are
          composed.  `agree` is the share of pixels on which the two return the same label.
  graph   one replay of the TTA graph (pn2_flip_views + the forward over V * B samples + the fused tail) against one replay of the plain graph of B samples."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pranet-v2_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ.setdefault("PN2_NO_PRETRAINED", "1")

import torch


def alternate(fs, reps, warm):
    """{name: [ms, ...]} of the callables in fs, run in turn `reps` times after `warm` turns, each run between two events."""
    for _ in range(warm):
        for f in fs.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fs}
    for _ in range(reps):
        for k, f in fs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b))
    return ms


def summary(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--encoder", default="pvt_v2_b2")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tta_bench needs a GPU: nothing is measured without one")
    import pn2
    from lib.networks import EMCADNet
    from pn2 import voleval as V
    from pn2.engine import Act, Engine, F32
    from pn2.infer import VolumePredictor
    pn2.set_compute_dtype("bf16")
    K, B, S, views = 9, a.batch, a.size, ("id", "h", "v")
    torch.manual_seed(0)
    model = EMCADNet(num_classes=K, encoder=a.encoder, dual=True, pretrain=False).cuda().eval()
    model.backbone.reset_drop_path(0.0)
    xb = torch.randn(B, 1, S, S, generator=torch.Generator().manual_seed(1)).cuda()
    plain = VolumePredictor(model, (S, S), B)
    eng = Engine(F32, False, need_grad=False)
    for average in ("prob", "logit"):
        tta = VolumePredictor(model, (S, S), B, tta=views, tta_average=average)
        for mode in ("sum_fg_minus_bg", "sum_fg", "last"):
            st = tta._labels(xb, mode)
            lows = [x.t[..., :x.C] for x in st["lows"]]
            maps, scales = VolumePredictor._pick(lows, [S // m.shape[1] for m in lows], mode)
            full, _ = VolumePredictor._pick([x.t for x in st["lows"]], scales, mode)          # the same maps with their padding channels
            out = torch.empty((B, S, S), dtype=torch.uint8, device="cuda")

            def fused():
                return V.predict_labels_up_tta(maps, scales, mode, views, average, out=out)

            def unfused():
                tot = None
                for v, view in enumerate(views):
                    dims = [d for d, bit in ((3, 1), (2, 2)) if V.VIEWS[view] & bit]
                    ups = []
                    for m, s in zip(full, scales):
                        blk = m[v * B:(v + 1) * B]
                        u = eng.to_nchw(eng.bilinear(Act(eng, blk, K, K, blk.shape[3], F32, requires_grad=False), s))
                        ups.append(torch.flip(u, dims) if dims else u)
                    if mode == "last":
                        x = ups[-1]
                    elif mode == "sum_fg":
                        x = sum(ups[1:], ups[0])
                    else:
                        h = len(ups) // 2
                        x = sum((p - q for p, q in zip(ups[1:h], ups[h + 1:])), ups[0] - ups[h])
                    if average == "prob":
                        x = torch.softmax(x, dim=1)
                    tot = x if tot is None else tot + x
                return torch.argmax(tot, dim=1).to(torch.uint8)
            agree = float((fused() == unfused()).float().mean())
            ms = alternate({"fused": fused, "unfused": unfused}, a.reps, a.warm)
            print(json.dumps({"what": "tail", "mode": mode, "average": average, "views": views, "B": B, "size": S, "K": K, "nmaps": len(maps), "agree": agree,
                              "fused": summary(ms["fused"]), "unfused": summary(ms["unfused"])}), flush=True)
        if average == "prob":
            for mode in ("sum_fg_minus_bg", "sum_fg", "last"):
                sp, stt = plain._labels(xb, mode), tta._labels(xb, mode)
                ms = alternate({"plain": sp["graph"].replay, "tta": stt["graph"].replay}, a.reps, a.warm)
                print(json.dumps({"what": "graph", "mode": mode, "average": average, "views": views, "B": B, "size": S, "K": K, "encoder": a.encoder,
                                  "plain": summary(ms["plain"]), "tta": summary(ms["tta"])}), flush=True)


if __name__ == "__main__":
    main()
