#!/usr/bin/env python3
"""The strided skip of the ResNet stage-opening blocks, measured.  Usage: resnet_micro.py [batch] [size]   (default 32 x 224^2, bf16)

1. pn2_subsample_fwd / pn2_subsample_bwd at the downsample shapes of layer2 and layer4 against pn2_copy on the SAME byte count: achieved bytes/s (algorithmic bytes:
   forward reads and writes the gathered rows; backward with accum = 0 reads them and writes the whole of dx).  Device events around REPS back-to-back launches, the
   median of ROUNDS rounds, the two kernels alternating round by round; `cold`: single launches behind a cache-evicting fill.
2. Engine.strided_pointwise against the generic stride-2 conv_bn_act (the implicit GEMM with the stride in its index math) at layer2.0's downsample shape, forward +
   backward in train mode: the sum of the event-bracketed kernel times of one pass (pn2.profile.Recorder) and the wall clock of PASSES passes, alternating."""
import ctypes as C
import os
import statistics
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "pranet-v2_amd"))
import torch
import torch.nn as nn
import pn2
from pn2 import capi, core, BF16
from pn2.engine import Engine
from pn2.graph import _seed_grad
from pn2.profile import Recorder

N = int(sys.argv[1]) if len(sys.argv) > 1 else 32
S = int(sys.argv[2]) if len(sys.argv) > 2 else 224
REPS, ROUNDS, COLD, PASSES = 50, 7, 10, 20
dev = "cuda"
lib = capi.load()
P_ = lambda t: C.c_void_p(t.data_ptr())
st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e-3


def compare(tag, a, b, nbytes):
    """a, b: (name, launch); prints GB/s of both (warm median, cold median) and the ratio a / b"""
    for _, f in (a, b):
        timed(f, 5)
    warm = {a[0]: [], b[0]: []}
    for _ in range(ROUNDS):
        for n_, f in (a, b):
            warm[n_].append(timed(f, REPS))
    cold = {a[0]: [], b[0]: []}
    for _ in range(COLD):
        for n_, f in (a, b):
            core._thrash(); torch.cuda.synchronize()
            cold[n_].append(timed(f, 1))
    w = {k: statistics.median(v) for k, v in warm.items()}
    c = {k: statistics.median(v) for k, v in cold.items()}
    print(f"{tag}: {nbytes / 1e6:.1f} MB | warm " + ", ".join(f"{k} {1e6 * w[k]:.1f} us = {nbytes / w[k] / 1e9:.0f} GB/s ({1e6 * min(warm[k]):.1f}-{1e6 * max(warm[k]):.1f})" for k in w)
          + f", ratio {w[b[0]] / w[a[0]]:.2f} | cold " + ", ".join(f"{k} {1e6 * c[k]:.1f} us = {nbytes / c[k] / 1e9:.0f} GB/s" for k in c) + f", ratio {c[b[0]] / c[a[0]]:.2f}")


def part1():
    for name, Cc, H in (("layer2.0", 256, S // 4), ("layer4.0", 1024, S // 16)):
        OH = (H - 1) // 2 + 1
        x = torch.randn(N, H, H, Cc, device=dev).bfloat16()
        y = torch.empty(N, OH, OH, Cc, device=dev, dtype=torch.bfloat16)
        dx = torch.empty_like(x)
        Mo, M = N * OH * OH, N * H * H
        src = torch.randn(M, Cc, device=dev).bfloat16(); dst = torch.empty_like(src)
        nb = 2 * Mo * Cc * 2
        compare(f"{name} fwd {N}x{H}x{H}x{Cc} -> {OH}x{OH}", ("subsample_fwd", lambda: lib.pn2_subsample_fwd(BF16, P_(x), Cc, P_(y), Cc, N, H, H, Cc, 2, st())),
                ("copy", lambda: lib.pn2_copy(BF16, P_(src), Cc, BF16, P_(dst), Cc, Mo, Cc, 0, st())), nb)
        rows = (Mo + M) // 2                                   # a copy that moves Mo + M rows in all
        nb = (Mo + M) * Cc * 2
        compare(f"{name} bwd (accum 0)", ("subsample_bwd", lambda: lib.pn2_subsample_bwd(BF16, P_(y), Cc, P_(dx), Cc, N, H, H, Cc, 2, 0, st())),
                ("copy", lambda: lib.pn2_copy(BF16, P_(src), Cc, BF16, P_(dst), Cc, rows, Cc, 0, st())), nb)
        nb = 3 * Mo * Cc * 2                                   # accum = 1: dy and the strided pixels of dx in, those pixels out
        rows = 3 * Mo // 2
        compare(f"{name} bwd (accum 1)", ("subsample_bwd", lambda: lib.pn2_subsample_bwd(BF16, P_(y), Cc, P_(dx), Cc, N, H, H, Cc, 2, 1, st())),
                ("copy", lambda: lib.pn2_copy(BF16, P_(src), Cc, BF16, P_(dst), Cc, rows, Cc, 0, st())), nb)


def part2():
    H, Cin, Cout = S // 4, 256, 512
    torch.manual_seed(0)
    conv = nn.Conv2d(Cin, Cout, 1, stride=2, bias=False).to(dev)
    bn = nn.BatchNorm2d(Cout).to(dev)
    x = torch.randn(N, Cin, H, H, device=dev)
    gy = torch.randn(N, Cout, H // 2, H // 2, device=dev)
    tuner = {}

    def one(path):
        eng = Engine(BF16, True, need_grad=True, tuner=tuner)
        a = eng.from_nchw(x, requires_grad=True)
        y = eng.conv_bn_act(a, conv, bn) if path == "generic" else eng.strided_pointwise(a, conv, bn)
        _seed_grad(y, gy)
        eng.backward()
    skip = ("pn2_nchw_to_nhwc",)          # the input conversion both paths share
    for p in ("generic", "split"):
        for _ in range(3):
            one(p)
    torch.cuda.synchronize()
    ktime = {"generic": [], "split": []}
    detail = {}
    for _ in range(ROUNDS):
        for p in ("generic", "split"):
            with Recorder() as rec:
                one(p)
            agg = rec.summary()
            ktime[p].append(sum(d["ms"] for k, d in agg.items() if k not in skip))
            detail[p] = {k: (round(d["ms"], 4), d["launches"]) for k, d in agg.items() if k not in skip}
    wall = {"generic": [], "split": []}
    for _ in range(ROUNDS):
        for p in ("generic", "split"):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _i in range(PASSES):
                one(p)
            torch.cuda.synchronize(); wall[p].append((time.perf_counter() - t0) / PASSES * 1e3)
    for p in ("generic", "split"):
        print(f"layer2.0 downsample {N}x{H}x{H}x{Cin} -> {Cout}, stride 2, bf16 train fwd+bwd, {p}: kernel time {statistics.median(ktime[p]):.3f} ms "
              f"({min(ktime[p]):.3f}-{max(ktime[p]):.3f}), {sum(v[1] for v in detail[p].values())} launches; wall {statistics.median(wall[p]):.3f} ms per pass")
        for k, v in sorted(detail[p].items(), key=lambda kv: -kv[1][0]):
            print(f"    {k:32s} {v[0]:8.4f} ms x{v[1]}")


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs a GPU"
    pn2.set_compute_dtype("bf16")
    part1()
    part2()
