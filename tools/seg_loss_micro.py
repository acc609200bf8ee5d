#!/usr/bin/env python3
"""Loss kernels of config 5 on one GPU, event-bracketed, each with the bytes-at-8-TB/s floor of the maps read and the gradients written.
Three pairs: the K = 9 dual pair (pn2_mutation_loss_fwd / _bwd), the K = 2..9 dual pair with a subset mask (pn2_dual_loss_fwd / _bwd) and the
single-supervision pair (pn2_seg_loss_fwd / _bwd), in their supervision modes, at K = 9 and K = 4.
At K = 9 / mutation the two dual pairs are timed alternately, three rounds each, so the spread of one shows next to the distance of the other.
Their forward kernels differ there; the mask entry's backward launches the K = 9 kernel for that one mask, so dloss_bwd_k<9> is timed with 14 of the
15 subsets (mask 0x7ffe), a lower bound of its time with all of them.
Usage: seg_loss_micro.py [batch] [size] [reps] [K:mode ...]   (extra dual cases; mode is a supervision name or a subset mask, e.g. 2:last 6:0x7f)"""
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


def case(K, mode, dual, rounds=1):
    """dual: False the single pair, "k9" the K = 9 entry points, "mask" the K = 2..9 ones, "both" the two alternately (same buffers)."""
    g = torch.Generator(device="cpu").manual_seed(K)
    nmap = 8 if dual else 4
    maps = [(torch.randn(N, S, S, K, generator=g) * 1.5).to(dev) for _ in range(nmap)]
    grads = [torch.empty_like(m) for m in maps]
    label = torch.randint(0, K, (N, S // 16, S // 16), generator=g)
    label = torch.nn.functional.interpolate(label[:, None].float(), size=(S, S), mode="nearest")[:, 0].long().to(dev)
    nb = call.pn2_mutation_loss_blocks(N * HW)
    wd = call.pn2_dual_loss_width(K) if dual else call.pn2_seg_loss_width(K)
    partial, sums, loss = torch.empty(nb, wd, device=dev), torch.empty(wd, device=dev), torch.empty(1, device=dev)
    map_bytes = nmap * N * HW * K * 4
    sub = SEG_SUBSETS[mode] if mode in SEG_SUBSETS else int(mode, 0)
    pairs = []
    if dual:
        bgm = torch.stack([(label != k).float() for k in range(K)], 1).contiguous()
        fg, bg, dfg, dbg = (PA(*[t.data_ptr() for t in ts]) for ts in (maps[:4], maps[4:], grads[:4], grads[4:]))
        if dual in ("k9", "both"):
            assert K == 9 and mode == "mutation"
            pairs.append((f"dual {mode} K={K} (K = 9 entry)",
                          lambda: call.pn2_mutation_loss_fwd(fg, bg, P(label), P(bgm), N, HW, K, 0.5, 0.7, 0.3, P(partial), P(sums), P(loss), st),
                          lambda: call.pn2_mutation_loss_bwd(fg, bg, dfg, dbg, P(label), P(bgm), N, HW, K, 0.5, 0.7, 0.3, P(sums), 1.0, st)))
        if dual in ("mask", "both"):
            pairs.append((f"dual {mode} K={K} (mask entry)",
                          lambda: call.pn2_dual_loss_fwd(fg, bg, sub, P(label), P(bgm), N, HW, K, 0.5, 0.7, 0.3, P(partial), P(sums), P(loss), st),
                          lambda: call.pn2_dual_loss_bwd(fg, bg, dfg, dbg, sub, P(label), P(bgm), N, HW, K, 0.5, 0.7, 0.3, P(sums), 1.0, st)))
        rd = map_bytes + N * HW * 8 + N * K * HW * 4
    else:
        pm, pg = PA(*[t.data_ptr() for t in maps]), PA(*[t.data_ptr() for t in grads])
        pairs.append((f"single {mode} K={K}",
                      lambda: call.pn2_seg_loss_fwd(pm, sub, P(label), N, HW, K, 0.3, 0.7, P(partial), P(sums), P(loss), st),
                      lambda: call.pn2_seg_loss_bwd(pm, pg, sub, P(label), N, HW, K, 0.3, 0.7, P(sums), 1.0, st)))
        rd = map_bytes + N * HW * 8
    for _ in range(rounds):
        for name, fwd, bwd in pairs:
            tf, tb = timed(fwd), timed(bwd)
            print(f"{name:40s} fwd {tf:8.1f} us (floor {rd / HBM * 1e6:6.1f})   bwd {tb:8.1f} us (floor {(rd + map_bytes) / HBM * 1e6:6.1f})   loss {float(loss):.4f}")


print(f"loss kernels at {N} x {S}^2, fp32 [N][H][W][K] maps, {REPS} calls each (forward = main kernel + reduce + finalize)")
case(9, "mutation", "both", rounds=3)
for K, mode in ((9, "0x7ffe"), (9, "deep_supervision"), (9, "last"), (4, "mutation"), (4, "deep_supervision"), (4, "last")):
    case(K, mode, "mask")
for a in sys.argv[4:]:
    case(int(a.split(":")[0]), a.split(":")[1], "mask")
for K, mode in ((9, "mutation"), (9, "deep_supervision"), (9, "last"), (4, "mutation"), (4, "deep_supervision")):
    case(K, mode, False)
