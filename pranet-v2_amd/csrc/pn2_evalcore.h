// pn2_evalcore.h — the device arithmetic that the per-image test tail (pn2_add x3 -> pn2_bilinear_fwd -> pn2_eval_tail -> pn2_eval_hist) and the ragged-batch
// tail (pn2_eval_tail_batch / pn2_eval_counts_batch, pn2_eval.hip) must agree on bit for bit.  Each expression is written ONCE here and inlined into both
// paths; every file is built with the same -ffp-contract setting (the Makefile's one FLAGS line), and every product below has a single use, so the compiler's
// choice of which product of a sum it fuses is the same wherever the expression lands.
#pragma once
#include "pn2_common.h"

// four-tap bilinear value of bilinear_fwd_k (pn2_spatial.hip): weights ly0/ly1, lx0/lx1 of bl_src, taps a = (y0,x0), b = (y0,x1), c = (y1,x0), d = (y1,x1)
__device__ __forceinline__ float bl_tap4(float ly0, float ly1, float lx0, float lx1, float a, float b, float c, float d) {
    return ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * d);
}

// torch.sigmoid as the eval tail takes it (MyTest_med.py:109)
__device__ __forceinline__ float eval_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// (res - res.min()) / (res.max() - res.min() + 1e-8) * 255 -> uint8 by truncation (MyTest_med.py:110-113); den = max - min + 1e-8f
__device__ __forceinline__ unsigned char eval_byte(float s, float mn, float den) { return (unsigned char)(((s - mn) / den) * 255.f); }

// order-preserving map of a float onto unsigned integers (and back): min / max of floats by integer atomics, exact under any order
__device__ __forceinline__ unsigned f2ord(float f) { const unsigned u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ float ord2f(unsigned o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

// the two 256-bin histograms of pn2_eval_hist over the pixels i0, i0 + stride, ... < n of one image: h[0..255] all pixels, h[256..511] those with gt > 0.5.
// h is a zeroed LDS array of the block; integer LDS atomics, so the counts do not depend on the order.
__device__ __forceinline__ void eval_hist_accum(const unsigned char* __restrict__ pred, const float* __restrict__ gt, long long n, long long i0, long long stride,
                                                unsigned* h) {
    for (long long i = i0; i < n; i += stride) {
        const unsigned v = pred[i];
        atomicAdd(&h[v], 1u);
        if (gt[i] > 0.5f) atomicAdd(&h[256 + v], 1u);
    }
}
// ... and the block's non-zero bins added to the image's 512 global counts (256 threads)
__device__ __forceinline__ void eval_hist_flush(const unsigned* h, unsigned* __restrict__ hist) {
    if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
    if (h[threadIdx.x + 256]) atomicAdd(&hist[threadIdx.x + 256], h[threadIdx.x + 256]);
}
