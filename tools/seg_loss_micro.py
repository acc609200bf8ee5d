#!/usr/bin/env python3
"""Loss kernels of config 5 on one GPU, event-bracketed: the dual pair (pn2_mutation_loss_fwd / _bwd, K = 9) next to the single-supervision pair
(pn2_seg_loss_fwd / _bwd) in its supervision modes and at K = 4, with the bytes-at-8-TB/s floor of the maps read and the gradients written.
Usage: seg_loss_micro.py [batch] [size] [reps]"""
import ctypes as C
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "pranet-v2_amd"))
import torch
from pn2.capi import call
from pn2.loss import SEG_SUBSETS

N = int(sys.argv[1]) if len(sys.argv) > 1 else 16
S = int(sys.argv[2]) if len(sys.argv) > 2 else 512
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 50
assert torch.cuda.is_available(), "needs a GPU"
dev, HW = "cuda", S * S
P = lambda t: C.c_void_p(t.data_ptr())
PA = C.c_void_p * 4
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
HBM = 8e12


def timed(fn):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / REPS * 1e3          # microseconds per call


def case(K, mode, dual):
    g = torch.Generator(device="cpu").manual_seed(K)
    nmap = 8 if dual else 4
    maps = [(torch.randn(N, S, S, K, generator=g) * 1.5).to(dev) for _ in range(nmap)]
    grads = [torch.empty_like(m) for m in maps]
    label = torch.randint(0, K, (N, S // 16, S // 16), generator=g)
    label = torch.nn.functional.interpolate(label[:, None].float(), size=(S, S), mode="nearest")[:, 0].long().to(dev)
    nb = call.pn2_mutation_loss_blocks(N * HW)
    wd = call.pn2_mutation_loss_width(K) if dual else call.pn2_seg_loss_width(K)
    partial, sums, loss = torch.empty(nb, wd, device=dev), torch.empty(wd, device=dev), torch.empty(1, device=dev)
    map_bytes = nmap * N * HW * K * 4
    if dual:
        bgm = torch.stack([(label != k).float() for k in range(K)], 1).contiguous()
        fg, bg, dfg, dbg = (PA(*[t.data_ptr() for t in ts]) for ts in (maps[:4], maps[4:], grads[:4], grads[4:]))
        fwd = lambda: call.pn2_mutation_loss_fwd(fg, bg, P(label), P(bgm), N, HW, K, 0.5, 0.7, 0.3, P(partial), P(sums), P(loss), st)
        bwd = lambda: call.pn2_mutation_loss_bwd(fg, bg, dfg, dbg, P(label), P(bgm), N, HW, K, 0.5, 0.7, 0.3, P(sums), 1.0, st)
        rd = map_bytes + N * HW * 8 + N * K * HW * 4
    else:
        sub = SEG_SUBSETS[mode]
        pm, pg = PA(*[t.data_ptr() for t in maps]), PA(*[t.data_ptr() for t in grads])
        fwd = lambda: call.pn2_seg_loss_fwd(pm, sub, P(label), N, HW, K, 0.3, 0.7, P(partial), P(sums), P(loss), st)
        bwd = lambda: call.pn2_seg_loss_bwd(pm, pg, sub, P(label), N, HW, K, 0.3, 0.7, P(sums), 1.0, st)
        rd = map_bytes + N * HW * 8
    tf, tb = timed(fwd), timed(bwd)
    name = f"dual mutation K={K}" if dual else f"single {mode} K={K}"
    print(f"{name:32s} fwd {tf:8.1f} us (floor {rd / HBM * 1e6:6.1f})   bwd {tb:8.1f} us (floor {(rd + map_bytes) / HBM * 1e6:6.1f})   loss {float(loss):.4f}")


print(f"loss kernels at {N} x {S}^2, fp32 [N][H][W][K] maps, {REPS} calls each (forward = main kernel + reduce + finalize)")
case(9, "mutation", True)
for K, mode in ((9, "mutation"), (9, "deep_supervision"), (9, "last"), (4, "mutation"), (4, "deep_supervision")):
    case(K, mode, False)
