"""Precision model and gates of the fp32x3 conv kernels (PN2_F32X3): every fp32 operand x is split into bf16 terms h = bf16(x), m = bf16(x - h),
l = bf16(x - h - m) (x == h + m + l exactly for finite normal x), and six of the nine cross products - hh, hm, mh, hl, lh, mm - are summed by three
v_mfma_f32_16x16x32_bf16 per 16-deep sub-step, from C = 0, met by round-to-nearest adds (pn2_conv.hip, MMA<f32x3_t>).  Weight gradients chain the six
MFMAs of a 32-pixel stage.  The split, the six-product contraction and a two-term variant (hh + hm + mh: what a kernel that dropped the lo terms would
compute) are modelled here in float64, next to the gates of tests/test_gpu_convkernels_fp32x3.py."""
import math

import torch

from fp32ref import U32, spacing32

BF16_MAX = 3.3895313892515355e38          # largest finite bf16


def bf16(x):
    """round to nearest even bf16, returned in x's dtype (x: float32 / float64 of fp32 values)"""
    return x.float().bfloat16().to(x.dtype)


def split3(x):
    """x: float32 tensor -> (h, m, l) float32 tensors of bf16 values; each difference is exact in fp32 (Sterbenz-like: r has <= 16 significant bits)"""
    h = bf16(x)
    r = x - h
    m = bf16(r)
    l = bf16(r - m)
    return h, m, l


def x3_contract(a, b, terms=6):
    """float64 contraction a @ b.T (a: [R, K], b: [C, K], fp32 values) from the split operands: exact products of the kept terms, summed in float64.
    terms = 6: hh + hm + mh + hl + lh + mm (the kernel); 3: hh + hm + mh (a two-term split)."""
    ha, ma, la = (t.double() for t in split3(a.float()))
    hb, mb, lb = (t.double() for t in split3(b.float()))
    r = ha @ hb.t() + ha @ mb.t() + ma @ hb.t()
    if terms == 6:
        r = r + ha @ lb.t() + la @ hb.t() + ma @ mb.t()
    return r


def gate_fp32x3(S, K):
    """fp32x3 worst case for |got - r|, r the float64 contraction of the fp32 operands, S = sum_k |a_k b_k|:
      * dropped terms: |m| <= 2^-8 |x| (1 + 2^-8), |l| <= 2^-16 |x| (half a bf16 ulp of r each), so |ml| + |lm| + |ll| <= 2.02 u |a b|: 2.1 u S;
      * in-chain adds: a 16-deep sub-step is 16 k-values x 6 products = 96 terms summed inside three chained MFMAs from C = 0.  As in gate_fp32fast,
        every term's add is charged 2 u of the chain's sum of magnitudes (the matrix core's internal adds need not round to nearest; the kept
        products add up to at most (1 + 2^-7) S of the chunk): 2 * 96 * 1.01 u S <= 194 u S;
      * ceil(K / 16) round-to-nearest adds of the chain results into the accumulator, and one store rounding + slack: (ceil(K / 16) + 2) u S.
    -> (2.1 + 194 + ceil(K / 16) + 2) u S.  A two-term split errs by up to 3 * 2^-16 S = 768 u S, bf16 operands by ~2^-7 S: the worst case alone
    is no canary; the rms gate of the tests (<= 2 x the reference's own fp32 error) is: tests/test_fp32x3_cpu.py checks that it is >= 10 x tighter
    than the error of bf16 operands and >= 4 x tighter than that of a two-term split (which errs by only ~12-30 x the fp32 error)."""
    return (2.1 + 194 + math.ceil(K / 16) + 2) * U32 * S


def wgrad_tol_x3(got, slabs, ns, S, M):
    """fp32x3 gate of a weight gradient reduced from `ns` fp32 slabs over M pixels (arguments as fp32ref.wgrad_tol): per split, one chain per
    32-pixel stage (two 16-pixel sub-steps of three MFMAs: 192 terms, 2.02 u each) met by one round-to-nearest add per stage (ceil(stages / ns) of them)
    and the slab store, plus the dropped terms (2.1 u S); the reduce as fp32ref.wgrad_tol."""
    tol = (ns - 1) * U32 * slabs.abs().sum(0) + 0.5 * spacing32(got)
    spb = -(-(-(-M // 32)) // ns)
    return tol + (2.1 + 2 * 192 * 1.01 + spb + 2) * U32 * S
