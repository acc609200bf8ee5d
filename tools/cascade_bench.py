"""Times one CASCADE attention gate, forward + backward, fused (Engine.attention_gate, csrc/pn2_cascade.hip) against the same gate composed from the existing engine
ops (two conv_bn_act, the second with the first as residual + ReLU; the psi conv + BatchNorm as a one-channel head; sigmoid_gate; add), on the same weights and inputs.

Shapes: the stage-1 gate of MIST-small (C = 96, F_int = 48, 12 x 64^2) and of PVTv2-b2 at 224^2 (C = 64, F_int = 32, 16 x 56^2), bf16 and fp32.
Both variants run through the module surface (pn2.graph.run_module): after the warm-up calls each is a pair of captured graphs, so the figure is device time of the
launches plus the NCHW <-> NHWC conversions both share, not Python.  Per case: library launches of one eager forward + backward of each variant (counted at the C ABI),
then ROUNDS rounds that alternate the variants, ITERS forward + backward calls each between two device events; the median round and the spread are printed as one JSON
line per case.  Each case runs in a child process of its own under a time limit; the first failure ends the run.

    python tools/cascade_bench.py [--iters 200] [--rounds 7] [--timeout 240]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"mist_small": (12, 64, 64, 96, 48), "pvt_b2_224": (16, 56, 56, 64, 32)}


def one(case, dtype, iters, rounds):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "pranet-v2_amd")]
    import collections
    import numpy as np
    import torch
    import torch.nn as nn
    import pn2
    from pn2 import capi, F32
    from pn2.graph import run_module
    from lib.cascade import Attention_block
    real, counts = capi.load(), collections.Counter()

    class Counting:          # every launch entry point of the library, counted
        def __getattr__(self, n):
            f = getattr(real, n)
            if n in capi._VALUE_FUNCS:
                return f

            def w(*a):
                counts[n] += 1
                return f(*a)
            return w
    capi._lib = Counting()
    pn2.set_compute_dtype(dtype)
    N, H, W, C, Fi = CASES[case]

    class Fused(nn.Module):
        def __init__(self, ag):
            super().__init__(); self.ag = ag

        def forward(self, g, x):
            return run_module(lambda eng, a, b: [self.ag._build_aggregate(eng, a, b)], [g, x], list(self.parameters()), self.training)[0]

    class Composed(Fused):
        def _build(self, eng, g, x):
            ag = self.ag
            g1 = eng.conv_bn_act(g, ag.W_g[0], ag.W_g[1], bias=ag.W_g[0].bias)
            t = eng.conv_bn_act(x, ag.W_x[0], ag.W_x[1], bias=ag.W_x[0].bias, relu=True, residual=g1)
            pre = eng.conv_bn_act(t, ag.psi[0], ag.psi[1], bias=ag.psi[0].bias, out_map=(1, 8), y_dt=F32, y_C=1)
            return [eng.add(g, eng.sigmoid_gate(x, pre, 1))]

        def forward(self, g, x):
            return run_module(self._build, [g, x], list(self.parameters()), self.training)[0]
    torch.manual_seed(0)
    ag = Attention_block(C, C, Fi)
    mods = {"fused": Fused(ag).cuda().train(), "composed": Composed(ag).cuda().train()}
    g, x, R = (torch.randn(N, C, H, W, device="cuda") for _ in range(3))

    def step(m):
        m.zero_grad(set_to_none=True)
        m(g, x).backward(R)
    launches, outs = {}, {}
    for k, m in mods.items():
        counts.clear()
        step(m)
        torch.cuda.synchronize()
        launches[k] = sum(counts.values())
        outs[k] = (m(g, x).detach().float(), ag.psi[0].weight.grad.clone())
    dist = float((outs["fused"][0] - outs["composed"][0]).abs().max())
    for m in mods.values():          # warm-up: the call sites capture their graphs
        for _ in range(12):
            step(m)
    torch.cuda.synchronize()
    ms = {k: [] for k in mods}
    for _ in range(rounds):
        for k, m in mods.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                step(m)
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / iters)
    esz = 2 if dtype == "bf16" else 4
    M = N * H * W
    res = {"case": case, "dtype": dtype, "M": M, "C": C, "F_int": Fi, "launches_eager_fwd_bwd": launches, "max_abs_out_fused_vs_composed": dist,
           "ms_per_fwd_bwd": {k: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for k, v in ms.items()},
           "speedup_median": float(np.median(ms["composed"]) / np.median(ms["fused"])),
           "forward_bytes_not_written": M * (2 * rup8(Fi) + C) * esz}          # the normalised g1, relu(g1 + x1) and x * psi of the composed gate
    print(json.dumps(res), flush=True)


def rup8(v):
    return (v + 7) // 8 * 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--one", nargs=2, metavar=("CASE", "DTYPE"))
    a = ap.parse_args()
    if a.one:
        return one(a.one[0], a.one[1], a.iters, a.rounds)
    for case in CASES:
        for dtype in ("bf16", "fp32"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", case, dtype, "--iters", str(a.iters), "--rounds", str(a.rounds)], timeout=a.timeout)
            if r.returncode != 0:
                sys.exit(f"{case} {dtype}: exit status {r.returncode}; stopping")


if __name__ == "__main__":
    main()
