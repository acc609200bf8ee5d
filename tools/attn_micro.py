#!/usr/bin/env python3
"""Micro-benchmark of the spatial-reduction attention kernels, bf16.  Usage: attn_micro.py [head_dim] | attn_micro.py long [head_dim ...]
long: the streamed kernels (pn2_attn_long_*) at the shapes of 4 x 1024^2 and 4 x 640^2, each next to the on-chip kernels at 256 keys.
head_dim 64 (default): the PVTv2-B2 shapes of configs 4 (352^2) and 5 (512^2), bs=16.
head_dim 32: the PVTv2-B0 shapes (16 x 512^2, 16 x 352^2, 6 x 224^2), each also run at head_dim 64 on the same (B, Nq, Nkv, heads), with two floors:
the HBM bytes of q / kv / out / lse (forward) and q / kv / out / dO / lse / dq / dkv (backward) at 8 TB/s, and the exp count (B heads Nq Nkv, twice
in the backward, which recomputes P) at one v_exp_f32 per lane per 4 cycles: 256 CUs x 4 SIMDs x 16 lanes/clk x 2.4 GHz."""
import ctypes as C
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "pranet-v2_amd"))
import torch
from pn2.capi import call, BF16

P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def timeit(fn, reps=20):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


HBM, EXP = 8e12, 256 * 4 * 16 * 2.4e9


def bench(B, Nq, Nkv, heads, hd=64, floors=False):
    dev = "cuda"; st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    Cc = heads * hd
    q = torch.randn(B, Nq, Cc, device=dev).bfloat16(); kv = torch.randn(B, Nkv, 2 * Cc, device=dev).bfloat16()
    o = torch.empty_like(q); do = torch.randn_like(q); dq = torch.empty_like(q); dkv = torch.empty_like(kv)
    lse = torch.empty(B, heads, Nq, device=dev); delta = torch.empty(B, heads, Nq, device=dev)
    nb = call.pn2_attn_bwd_blocks(BF16, B, heads, Nq)
    part = torch.empty(B, heads, nb, 2, (Nkv + 63) // 64 * 64, hd, device=dev)
    sc = hd ** -0.5
    t_f = timeit(lambda: call.pn2_attn_fwd(BF16, P(q), Cc, P(kv), 2 * Cc, P(o), Cc, P(lse), B, Nq, Nkv, heads, hd, sc, st))
    t_b = timeit(lambda: call.pn2_attn_bwd(BF16, P(q), Cc, P(kv), 2 * Cc, P(o), Cc, P(do), Cc, P(lse), P(dq), Cc, P(dkv), 2 * Cc, P(part), P(delta), B, Nq, Nkv, heads, hd, sc, st))
    fl = 4.0 * B * heads * Nq * Nkv * hd
    # numerics against torch (fp32 math on the bf16-rounded inputs), first two samples
    nb_ = min(B, 2)
    qq = q[:nb_].float().reshape(nb_, Nq, heads, hd).permute(0, 2, 1, 3).requires_grad_(True)
    kk = kv[:nb_].float().reshape(nb_, Nkv, 2, heads, hd).permute(2, 0, 3, 1, 4).detach().requires_grad_(True)
    r = ((qq @ kk[0].transpose(-2, -1)) * sc).softmax(-1) @ kk[1]
    r.backward(do[:nb_].float().reshape(nb_, Nq, heads, hd).permute(0, 2, 1, 3))
    ro = r.permute(0, 2, 1, 3).reshape(nb_, Nq, Cc)
    rel = lambda a, b: float((a.float() - b).norm() / b.norm())
    e_o = rel(o[:nb_], ro)
    e_q = rel(dq[:nb_], qq.grad.permute(0, 2, 1, 3).reshape(nb_, Nq, Cc))
    e_kv = rel(dkv[:nb_], kk.grad.permute(1, 3, 0, 2, 4).reshape(nb_, Nkv, 2 * Cc))
    line = (f"B{B} Nq{Nq:6d} Nkv{Nkv:4d} h{heads}" + (f" hd{hd}" if floors else "") + f": fwd {t_f:7.1f} us {fl/t_f/1e6:6.1f} TF/s | bwd(slots {nb:3d}) {t_b:7.1f} us "
            f"{2.5*fl/t_b/1e6:6.1f} TF/s | rel err o {e_o:.1e} dq {e_q:.1e} dkv {e_kv:.1e}")
    if floors:
        lse_b = 4 * B * heads * Nq
        hf = (3 * q.numel() * 2 + kv.numel() * 2 + lse_b) / HBM * 1e6                       # q, kv, out, lse
        hb = (5 * q.numel() * 2 + 2 * kv.numel() * 2 + 2 * lse_b) / HBM * 1e6                # q, kv, out, dO, lse, delta, dq, dkv
        ex = B * heads * Nq * Nkv / EXP * 1e6
        line += f" | floors fwd HBM {hf:6.1f} exp {ex:6.1f} us, bwd HBM {hb:6.1f} exp {2 * ex:6.1f} us"
    print(line)
    return t_f, t_b


def bench_long(B, Nq, Nkv, heads, hd):
    """The streamed family (pn2_attn_long_*) at Nkv keys next to the on-chip family at 256 keys on the same (B, Nq, heads), same process: the figure of
    merit is time per query x key.  Floors as in bench(): the HBM bytes that have to move once, and the exp count."""
    dev = "cuda"; st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    Cc = heads * hd
    q = torch.randn(B, Nq, Cc, device=dev).bfloat16(); kv = torch.randn(B, Nkv, 2 * Cc, device=dev).bfloat16()
    o = torch.empty_like(q); do = torch.randn_like(q); dq = torch.empty_like(q); dkv = torch.empty_like(kv)
    lse = torch.empty(B, heads, Nq, device=dev)
    n = (C.c_longlong * 3)()
    call.pn2_attn_long_bwd_workspace(BF16, B, Nq, heads, hd, n)
    part, delta, dqacc = (torch.empty(int(v), device=dev) for v in n)
    sc = hd ** -0.5
    t_f = timeit(lambda: call.pn2_attn_long_fwd(BF16, P(q), Cc, P(kv), 2 * Cc, P(o), Cc, P(lse), B, Nq, Nkv, heads, hd, sc, st))
    t_b = timeit(lambda: call.pn2_attn_long_bwd(BF16, P(q), Cc, P(kv), 2 * Cc, P(o), Cc, P(do), Cc, P(lse), P(dq), Cc, P(dkv), 2 * Cc, P(part), P(delta), P(dqacc),
                                                B, Nq, Nkv, heads, hd, sc, st))
    lse_b = 4 * B * heads * Nq
    hf = (3 * q.numel() * 2 + kv.numel() * 2 + lse_b) / HBM * 1e6
    hb = (5 * q.numel() * 2 + 2 * kv.numel() * 2 + 2 * lse_b) / HBM * 1e6
    ex = B * heads * Nq * Nkv / EXP * 1e6
    print(f"long  B{B} Nq{Nq:6d} Nkv{Nkv:4d} h{heads} hd{hd}: fwd {t_f:8.1f} us | bwd {t_b:8.1f} us | floors fwd HBM {hf:6.1f} exp {ex:6.1f} us, bwd HBM {hb:6.1f} exp {2 * ex:6.1f} us"
          f" | workspaces partial {n[0] * 4 / 2**20:.1f} delta {n[1] * 4 / 2**20:.1f} dq {n[2] * 4 / 2**20:.1f} MiB")
    if Nkv > 256:
        s_f, s_b = bench(B, Nq, 256, heads, hd=hd, floors=True)
        qk_l, qk_s = B * heads * Nq * Nkv, B * heads * Nq * 256
        print(f"    per query x key, long / short(256 keys): fwd {(t_f / qk_l) / (s_f / qk_s):.2f}  bwd {(t_b / qk_l) / (s_b / qk_s):.2f}")
    return t_f, t_b


# (B, Nq, Nkv, heads): 4 x 1024^2 (1024 keys in every stage) and 4 x 640^2 (400 keys)
LONG_SHAPES = [(4, 65536, 1024, 1), (4, 16384, 1024, 2), (4, 4096, 1024, 5), (4, 1024, 1024, 8),
               (4, 25600, 400, 1), (4, 6400, 400, 2), (4, 1600, 400, 5), (4, 400, 400, 8)]

B0_SHAPES = [(16, 16384, 256, 1), (16, 4096, 256, 2), (16, 1024, 256, 5), (16, 256, 256, 8),       # 16 x 512^2
             (16, 7744, 121, 1), (16, 1936, 121, 2), (16, 484, 121, 5), (16, 121, 121, 8),         # 16 x 352^2
             (6, 3136, 49, 1), (6, 784, 49, 2), (6, 196, 49, 5), (6, 49, 49, 8)]                   # 6 x 224^2


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "long":          # attn_micro.py long [head_dim ...]: the streamed family, hd 32 and 64 by default
        for hd in ([int(a) for a in sys.argv[2:]] or [32, 64]):
            for shp in LONG_SHAPES:
                bench_long(*shp, hd)
        sys.exit(0)
    hd = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    if hd == 32:
        tot = [0.0] * 4
        for shp in B0_SHAPES:
            f32_, b32_ = bench(*shp, hd=32, floors=True)
            f64_, b64_ = bench(*shp, hd=64, floors=True)
            print(f"    hd32 / hd64: fwd {f32_ / f64_:.2f}  bwd {b32_ / b64_:.2f}")
            tot = [a + b for a, b in zip(tot, (f32_, b32_, f64_, b64_))]
        print(f"sum over the b0 shapes: hd32 fwd {tot[0]:.1f} bwd {tot[1]:.1f} us, hd64 fwd {tot[2]:.1f} bwd {tot[3]:.1f} us")
        sys.exit(0)
    for shp in [(16, 7744, 121, 1), (16, 1936, 121, 2), (16, 484, 121, 5), (16, 121, 121, 8),
                (16, 16384, 256, 1), (16, 4096, 256, 2), (16, 1024, 256, 5), (16, 256, 256, 8), (2, 256, 196, 2), (2, 256, 160, 2), (2, 200, 250, 1)]:
        bench(*shp)
