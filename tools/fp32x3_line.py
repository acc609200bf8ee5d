#!/usr/bin/env python3
"""fp32fast against fp32x3 on bench.py's workload (PraNet_V2, 32 x 3 x 352 x 352, Trainer capture / replay, lr = 1e-4, clip = 0.5 as bench.fp32_line), in ONE
process: both Trainers are built and captured first, then their timed windows alternate (--rounds of --steps replays each), so clocks, thermals and the
neighbours on the machine weigh on both modes alike.  Prints one line per window and a JSON summary (images/s and ms/step per mode: min / median / max).

    python tools/fp32x3_line.py [--rounds 5] [--steps 10]
    python tools/fp32x3_line.py --only fp32x3 --steps 10        # one mode, e.g. under rocprofv3 --kernel-trace --stats (per-family times: tools/stats_by_family.py)
fp32x3 has no shipped tuning entries: its first eager step times the tile candidates of every conv shape.  --save-tuner FILE writes the table after the
run; PN2_TUNE_CACHE=FILE loads it in a later process, so that a profiled run holds no tuning launches.
"""
import argparse, json, os, statistics, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "pranet-v2_amd"))
os.environ.setdefault("PN2_NO_PRETRAINED", "1")


def build(mode, x, m):
    import torch
    import pn2
    from pn2.trainer import Trainer
    from lib.pranet import PraNet_V2
    pn2.set_compute_dtype(mode)
    torch.manual_seed(0)
    tr = Trainer(PraNet_V2(num_class=1).cuda().train(), lr=1e-4, clip=0.5)
    tr.capture(x, m, warmup=2)
    tr.replay(); torch.cuda.synchronize()
    return tr


def window(tr, steps):
    import torch
    tr.replay(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.replay()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=352)
    ap.add_argument("--only", choices=["fp32fast", "fp32x3"], default=None)
    ap.add_argument("--save-tuner", default=None)
    a = ap.parse_args()
    import torch
    from oracle import weights as W
    x, m = W.synthetic_batch(a.batch, a.size, seed=1234)
    x, m = x.cuda(), m.cuda()
    modes = [a.only] if a.only else ["fp32fast", "fp32x3"]
    trs = {mode: build(mode, x, m) for mode in modes}
    per = {mode: [] for mode in modes}
    for r in range(a.rounds if not a.only else 1):
        for mode in (modes if r % 2 == 0 else modes[::-1]):
            el = window(trs[mode], a.steps)
            per[mode].append(el)
            print(f"round {r} {mode:9s} {1e3 * el:8.3f} ms/step  {a.batch / el:8.1f} images/s", flush=True)
    out = {}
    for mode, v in per.items():
        ips = sorted(a.batch / e for e in v)
        out[mode] = {"images_per_s": {"min": round(ips[0], 1), "median": round(statistics.median(ips), 1), "max": round(ips[-1], 1)},
                     "ms_per_step": {"min": round(1e3 * min(v), 3), "median": round(1e3 * statistics.median(v), 3), "max": round(1e3 * max(v), 3)},
                     "windows": len(v), "steps_per_window": a.steps, "loss": [round(float(t), 6) for t in trs[mode].replay()[:5]]}
    if len(modes) == 2:
        out["speedup_median"] = round(out["fp32x3"]["images_per_s"]["median"] / out["fp32fast"]["images_per_s"]["median"], 3)
    if a.save_tuner:
        from pn2 import core
        core.save_tuner(a.save_tuner)
    print(json.dumps({"workload": f"PraNet_V2 train step, {a.batch} x 3 x {a.size}^2, Trainer replay, lr 1e-4, clip 0.5", **out}))


if __name__ == "__main__":
    main()
