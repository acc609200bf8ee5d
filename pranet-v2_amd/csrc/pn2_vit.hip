// pn2_vit.hip — the non-GEMM kernels of the PVTv2 encoder (reference: /root/reference/binary_seg/lib/pvtv2.py):
//   LayerNorm forward / backward            nn.LayerNorm at pvtv2.py:71,119,126,169,224-247 (eps 1e-5 / 1e-6)
//   column sums                             bias gradients of nn.Linear / biased nn.Conv2d (:19,22,62-65,70,167)
//   depth-wise 3x3 conv (+bias, +GELU)      DWConv :363-374 followed by nn.GELU in Mlp.forward :42-49
//   DropPath                                per-sample scale (+ residual) of Block.forward
// (the spatial-reduction attention of Attention.forward is pn2_attn.hip)
// Tokens [B, N, C] of the reference are NHWC pixels here (N = H*W), so no transposes are needed anywhere.
// The Linear layers themselves run on the implicit-GEMM conv kernels (1x1) of pn2_conv.hip.
// All kernels are deterministic (fixed-order reductions, no floating-point atomics).
#include <cstdint>
#include <cstdlib>
#include "pn2_common.h"
#include "pn2_dw.h"
#include "../../include/pn2.h"

namespace {

template <typename T> __device__ __forceinline__ void ldv(const T* p, float* f) { TT<T>::unpack(*reinterpret_cast<const uint4*>(p), f); }
template <typename T> __device__ __forceinline__ void stv(T* p, const float* f) { *reinterpret_cast<uint4*>(p) = TT<T>::pack(f); }

// ------------------------------------------------------------------------------------------ LayerNorm
// A row (token) is handled by LPR lanes of one wave (LPR = power of two >= C/VEC, <= 64); a lane owns up to NV channel vectors.
constexpr int LN_NV = 4;

template <typename T>
__global__ __launch_bounds__(256) void ln_fwd_k(const T* __restrict__ x, int ld_x, T* __restrict__ y, int ld_y, int M, int C, const float* __restrict__ gamma,
                                                const float* __restrict__ beta, float eps, float* __restrict__ mean, float* __restrict__ rstd, int LPR) {
    constexpr int V = TT<T>::VEC;
    const int CV = C / V, rpw = 64 / LPR, lane = threadIdx.x & 63, lr = lane % LPR, slot = lane / LPR;
    const int row = (blockIdx.x * 4 + (threadIdx.x >> 6)) * rpw + slot;
    const bool live = row < M;
    float v[LN_NV][V];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < LN_NV; ++k) {
        const int cv = lr + k * LPR;
        if (live && cv < CV) {
            ldv<T>(x + (size_t)row * ld_x + cv * V, v[k]);
#pragma unroll
            for (int e = 0; e < V; ++e) s += v[k][e];
        }
    }
    for (int o = 1; o < LPR; o <<= 1) s += __shfl_xor(s, o);
    const float mu = s / (float)C;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < LN_NV; ++k) {
        const int cv = lr + k * LPR;
        if (live && cv < CV) {
#pragma unroll
            for (int e = 0; e < V; ++e) { const float d = v[k][e] - mu; q += d * d; }
        }
    }
    for (int o = 1; o < LPR; o <<= 1) q += __shfl_xor(q, o);
    const float rs = rsqrtf(q / (float)C + eps);
    if (live && lr == 0) { mean[row] = mu; rstd[row] = rs; }
#pragma unroll
    for (int k = 0; k < LN_NV; ++k) {
        const int cv = lr + k * LPR;
        if (live && cv < CV) {
            float o[V];
#pragma unroll
            for (int e = 0; e < V; ++e) o[e] = (v[k][e] - mu) * rs * gamma[cv * V + e] + beta[cv * V + e];
            stv<T>(y + (size_t)row * ld_y + cv * V, o);
        }
    }
}

// dx = rstd * (g - mean(g) - xhat * mean(g * xhat)),  g = dy * gamma ;  partial dgamma / dbeta rows per block
template <typename T, int NV>
__global__ __launch_bounds__(256) void ln_bwd_k(const T* __restrict__ dy, int ld_dy, const T* __restrict__ x, int ld_x, int M, int C, const float* __restrict__ gamma,
                                                const float* __restrict__ mean, const float* __restrict__ rstd, T* __restrict__ dx, int ld_dx, int acc_dx,
                                                float* __restrict__ pg, float* __restrict__ pb, int rows_per_blk, int LPR) {
    constexpr int V = TT<T>::VEC;
    extern __shared__ float sh[];            // [2][slots][C] for the cross-slot reduction
    const int CV = C / V, rpw = 64 / LPR, lane = threadIdx.x & 63, wid = threadIdx.x >> 6, lr = lane % LPR, slot = wid * rpw + lane / LPR;
    const int nslot = 4 * rpw;
    const int r0 = blockIdx.x * rows_per_blk;
    int r1 = r0 + rows_per_blk; if (r1 > M) r1 = M;
    float ag[NV][V], ab[NV][V], gm[NV][V];
#pragma unroll
    for (int k = 0; k < NV; ++k)
#pragma unroll
        for (int e = 0; e < V; ++e) { ag[k][e] = 0.f; ab[k][e] = 0.f; const int c = (lr + k * LPR) * V + e; gm[k][e] = c < C ? gamma[c] : 0.f; }
    // the next row's vectors are fetched before the current row is reduced: the rows of a slot form a dependent chain (load -> two lane
    // reductions -> store), and without the prefetch every link pays the full memory latency
    uint4 nd[NV], nx[NV];
    float nmu = 0.f, nrs = 0.f;
    {
        const int row = r0 + slot;
        if (row < r1) {
            nmu = mean[row]; nrs = rstd[row];
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                const int cv = lr + k * LPR;
                if (cv < CV) { nd[k] = *reinterpret_cast<const uint4*>(dy + (size_t)row * ld_dy + cv * V); nx[k] = *reinterpret_cast<const uint4*>(x + (size_t)row * ld_x + cv * V); }
            }
        }
    }
    for (int rb = r0; rb < r1; rb += nslot) {           // uniform trip count: the shuffles below need every lane
        const int row = rb + slot;
        const bool live = row < r1;
        uint4 cd[NV], cx[NV];
#pragma unroll
        for (int k = 0; k < NV; ++k) { cd[k] = nd[k]; cx[k] = nx[k]; }
        const float mu = live ? nmu : 0.f, rs = live ? nrs : 0.f;
        {
            const int rown = row + nslot;
            if (rown < r1) {
                nmu = mean[rown]; nrs = rstd[rown];
#pragma unroll
                for (int k = 0; k < NV; ++k) {
                    const int cv = lr + k * LPR;
                    if (cv < CV) { nd[k] = *reinterpret_cast<const uint4*>(dy + (size_t)rown * ld_dy + cv * V); nx[k] = *reinterpret_cast<const uint4*>(x + (size_t)rown * ld_x + cv * V); }
                }
            }
        }
        float g[NV][V], xh[NV][V];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int cv = lr + k * LPR;
            if (live && cv < CV) {
                float d[V], xv[V];
                TT<T>::unpack(cd[k], d);
                TT<T>::unpack(cx[k], xv);
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    xh[k][e] = (xv[e] - mu) * rs; g[k][e] = d[e] * gm[k][e];
                    s1 += g[k][e]; s2 += g[k][e] * xh[k][e];
                    ag[k][e] += d[e] * xh[k][e]; ab[k][e] += d[e];
                }
            }
        }
        for (int o = 1; o < LPR; o <<= 1) { s1 += __shfl_xor(s1, o); s2 += __shfl_xor(s2, o); }
        const float c1 = s1 / (float)C, c2 = s2 / (float)C;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int cv = lr + k * LPR;
            if (live && cv < CV) {
                float o[V];
                T* d = dx + (size_t)row * ld_dx + cv * V;
                if (acc_dx) ldv<T>(d, o);
#pragma unroll
                for (int e = 0; e < V; ++e) { const float t = rs * (g[k][e] - c1 - xh[k][e] * c2); o[e] = acc_dx ? o[e] + t : t; }
                stv<T>(d, o);
            }
        }
    }
    // block partial of dgamma / dbeta: every slot owns the same channels -> sum the slots in a fixed order through LDS
    float* sg = sh; float* sb = sh + nslot * C;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int cv = lr + k * LPR;
        if (cv < CV) {
#pragma unroll
            for (int e = 0; e < V; ++e) { sg[slot * C + cv * V + e] = ag[k][e]; sb[slot * C + cv * V + e] = ab[k][e]; }
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        float a = 0.f, b = 0.f;
        for (int s_ = 0; s_ < nslot; ++s_) { a += sg[s_ * C + c]; b += sb[s_ * C + c]; }
        pg[(size_t)blockIdx.x * C + c] = a; pb[(size_t)blockIdx.x * C + c] = b;
    }
}

// out[c] (+)= sum_b p[b*ld + c]   (fixed order; double accumulation).  32 columns x 8 row lanes per block, 4 loads in flight per thread.
__device__ __forceinline__ void colsum_finalize_body(const float* __restrict__ p, int nblk, int C, int ld, float* __restrict__ out, int accumulate, int bloc) {
    __shared__ double sh[8][32];
    const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5, c = bloc * 32 + cl;
    double s = 0.0;
    if (c < C) {
        int r = rl;
        for (; r + 24 < nblk; r += 32) {
            const float a0 = p[(size_t)r * ld + c], a1 = p[(size_t)(r + 8) * ld + c], a2 = p[(size_t)(r + 16) * ld + c], a3 = p[(size_t)(r + 24) * ld + c];
            s += ((double)a0 + (double)a1) + ((double)a2 + (double)a3);
        }
        for (; r < nblk; r += 8) s += (double)p[(size_t)r * ld + c];
    }
    sh[rl][cl] = s;
    __syncthreads();
    if (rl == 0 && c < C) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) t += sh[k][cl];
        out[c] = accumulate ? out[c] + (float)t : (float)t;
    }
}
__global__ __launch_bounds__(256) void colsum_finalize_k(const float* __restrict__ p, int nblk, int C, int ld, float* __restrict__ out, int accumulate) {
    colsum_finalize_body(p, nblk, C, ld, out, accumulate, blockIdx.x);
}
// many finalisations in one launch, from a device job table (the parameter-gradient sums of a step only feed the optimizer, so the
// backward pass queues them): block b works on job j = find_job(bstart, b), local block b - bstart[j]
__global__ __launch_bounds__(256) void colsum_finalize_multi_k(const pn2_colsum_job* __restrict__ jobs, const int* __restrict__ bstart, int njobs) {
    const int jb = find_job(bstart, njobs, blockIdx.x);
    const pn2_colsum_job j = jobs[jb];
    colsum_finalize_body(j.partial, j.nblk, j.C, j.ld, j.out, j.accumulate, blockIdx.x - bstart[jb]);
}

// partial[blk][C] = sum over the block's rows of dy[row][c]
template <typename T>
__device__ __forceinline__ void colsum_body(const T* __restrict__ dy, int ld, int M, int C, float* __restrict__ partial, int rows_per_blk, int CVP, int bloc) {
    constexpr int V = TT<T>::VEC;
    extern __shared__ float sh[];            // [R][CVP*V]
    const int CV = C / V, R = 256 / CVP, cvl = threadIdx.x % CVP, rl = threadIdx.x / CVP;
    const int r0 = bloc * rows_per_blk;
    int r1 = r0 + rows_per_blk; if (r1 > M) r1 = M;
    for (int cvb = 0; cvb < CV; cvb += CVP) {
        const int cv = cvb + cvl;
        float a[V];
#pragma unroll
        for (int e = 0; e < V; ++e) a[e] = 0.f;
        if (cv < CV) {
            for (int m = r0 + rl; m < r1; m += R) {
                float d[V];
                ldv<T>(dy + (size_t)m * ld + cv * V, d);
#pragma unroll
                for (int e = 0; e < V; ++e) a[e] += d[e];
            }
        }
#pragma unroll
        for (int e = 0; e < V; ++e) sh[(rl * CVP + cvl) * V + e] = a[e];
        __syncthreads();
        if (rl == 0 && cv < CV) {
#pragma unroll
            for (int e = 0; e < V; ++e) {
                float s = 0.f;
                for (int r = 0; r < R; ++r) s += sh[(r * CVP + cvl) * V + e];
                partial[(size_t)bloc * C + cv * V + e] = s;
            }
        }
        __syncthreads();
    }
}
template <typename T>
__global__ __launch_bounds__(256) void colsum_k(const T* __restrict__ dy, int ld, int M, int C, float* __restrict__ partial, int rows_per_blk, int CVP) {
    colsum_body<T>(dy, ld, M, C, partial, rows_per_blk, CVP, blockIdx.x);
}
// the column sums of many tensors in one launch (device job table, as colsum_finalize_multi_k): the bias gradients of a step
template <typename T>
__global__ __launch_bounds__(256) void colsum_multi_k(const pn2_colsum_in_job* __restrict__ jobs, const int* __restrict__ bstart, int njobs) {
    const int jb = find_job(bstart, njobs, blockIdx.x);
    const pn2_colsum_in_job j = jobs[jb];
    colsum_body<T>((const T*)j.dy, j.ld, j.M, j.C, j.partial, j.rows, j.cvp, blockIdx.x - bstart[jb]);
}

// ------------------------------------------------------------------------------------------ depth-wise 3x3 (+bias, +GELU)
// erf without branches, on channel PAIRS (v_pk_fma_f32 / v_pk_mul_f32: one instruction per two channels).  The device library's erff is ~150 instructions
// with data-dependent branches; two of them per element made the depth-wise conv + GELU walks (and the weight-gradient walk that forms dz = dy * gelu'(z))
// instruction-bound.  Two polynomial pieces, both evaluated, one selected:
//   |a| <= 0.921875: erf(a) = a + a * p(a^2)                       (degree 5 in a^2)
//   |a| >  0.921875: erf(a) = sign(a) * (1 - exp(-(t + t * q(t)))), t = min(|a|, 4)   (degree 7: -log(erfc(t)) / t - 1 on [0.921875, 4])
// Chebyshev fits (coefficients rounded to fp32); max |error| 7.2e-8, max relative error 8.4e-8 against float64 erf over [-6, 6] - the last bit of fp32,
// as the library function.  NaN propagates through the first piece, +-inf saturates through the second.  Every operation is written out (no contraction
// left to the compiler), so the scalar wrappers below return the bits of the packed form.
typedef float dwf2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ dwf2 dw2(float v) { return dwf2{v, v}; }
__device__ __forceinline__ dwf2 dwfma(dwf2 a, dwf2 b, dwf2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ dwf2 dw_exp2(dwf2 v) { return dwf2{__builtin_amdgcn_exp2f(v.x), __builtin_amdgcn_exp2f(v.y)}; }
__device__ __forceinline__ dwf2 erf_nb2(dwf2 a) {
#pragma clang fp contract(off)
    const dwf2 t = dwf2{fabsf(a.x), fabsf(a.y)}, s = a * a;
    dwf2 p = dw2(-0x1.3b07e8p-11f);
    p = dwfma(p, s, dw2(0x1.477bf2p-8f)); p = dwfma(p, s, dw2(-0x1.b69768p-6f)); p = dwfma(p, s, dw2(0x1.ce1b58p-4f));
    p = dwfma(p, s, dw2(-0x1.8126ecp-2f)); p = dwfma(p, s, dw2(0x1.06eba6p-3f));
    const dwf2 ra = dwfma(p, a, a);
    const dwf2 tc = dwf2{fminf(t.x, 4.f), fminf(t.y, 4.f)};
    dwf2 q = dw2(-0x1.020fbcp-20f);
    q = dwfma(q, tc, dw2(0x1.142290p-15f)); q = dwfma(q, tc, dw2(-0x1.fff3bcp-12f)); q = dwfma(q, tc, dw2(0x1.176048p-8f)); q = dwfma(q, tc, dw2(-0x1.9a65fcp-6f));
    q = dwfma(q, tc, dw2(0x1.b94d44p-4f)); q = dwfma(q, tc, dw2(0x1.44b95ap-1f)); q = dwfma(q, tc, dw2(0x1.07f2d6p-3f));
    q = dwfma(q, tc, tc);
    const dwf2 e = dw2(1.f) - dw_exp2(q * dw2(-1.4426950408889634f));          // 1 - exp(-q)
    return dwf2{t.x > 0.921875f ? copysignf(e.x, a.x) : ra.x, t.y > 0.921875f ? copysignf(e.y, a.y) : ra.y};
}
__device__ __forceinline__ dwf2 gelu_f2(dwf2 x) {           // x * Phi(x)
#pragma clang fp contract(off)
    return (dw2(0.5f) * x) * (dw2(1.f) + erf_nb2(x * dw2(0.70710678118654752f)));
}
__device__ __forceinline__ dwf2 gelu_grad2(dwf2 x) {        // d/dx [x * Phi(x)] = Phi(x) + x * phi(x)
#pragma clang fp contract(off)
    const dwf2 ph = (x * dw2(0.3989422804014327f)) * dw_exp2(((dw2(-0.5f) * x) * x) * dw2(1.4426950408889634f));
    return dwfma(dw2(0.5f), dw2(1.f) + erf_nb2(x * dw2(0.70710678118654752f)), ph);
}
__device__ __forceinline__ float gelu_f(float x) { return gelu_f2(dw2(x)).x; }
__device__ __forceinline__ float gelu_grad(float x) { return gelu_grad2(dw2(x)).x; }

// z = sum_taps w[c][tap] * x[pixel + tap][c] (+ b[c]) ; y = gelu(z) (optional).  flip: correlate with the mirrored kernel (data gradient).
template <typename T>
__global__ __launch_bounds__(256) void gelu_bwd_k(const T* __restrict__ dy, const T* __restrict__ z, T* __restrict__ dz, size_t nvec) {
    constexpr int V = TT<T>::VEC;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (size_t)gridDim.x * 256) {
        float d[V], zz[V];
        ldv<T>(dy + i * V, d); ldv<T>(z + i * V, zz);
#pragma unroll
        for (int e = 0; e < V; ++e) d[e] *= gelu_grad(zz[e]);
        stv<T>(dz + i * V, d);
    }
}

// partial[blk][C*10]: [c*9 + tap] = sum_pixels dz[p][c] * x[p + tap][c] ; [C*9 + c] = sum_pixels dz[p][c]
// ---- sliding-window walk: a thread owns VT channels and walks a row segment of SEG output pixels, keeping the 3x3 input window packed in
// registers — 3 new loads per output pixel instead of 9 (a 9-load walk ran at ~1.5 TB/s, bound by the L1/TA requests in flight).
// VT = 8 / 4 / 2 channels per thread (16 / 8 / 4-byte loads for bf16): the narrow variants trade load width for 2-4x more waves, which is
// what the small late-stage tensors need (they are latency-bound, one short segment per thread).
template <typename T, int VT>
__device__ __forceinline__ void dw_load_col(const T* const (&rowp)[3], const bool (&vy)[3], int ix, int W, int C, DwVec<T, VT> (&col)[3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        col[r].zero();
        if (vy[r] && (unsigned)ix < (unsigned)W) col[r].load(rowp[r] + (size_t)ix * C);
    }
}

template <typename T, int VT>
__device__ __forceinline__ void dw_rows(const T* x, int row, int oy, int H, int W, int C, int cv, const T* (&rowp)[3], bool (&vy)[3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        vy[r] = (unsigned)(oy + r - 1) < (unsigned)H;
        rowp[r] = x + ((ptrdiff_t)(row + r - 1) * W) * C + cv * VT;
    }
}

template <typename T, int VT>
__global__ __launch_bounds__(256) void dwconv3x3_row_k(const T* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b, T* __restrict__ z, T* __restrict__ y,
                                                       int N, int H, int W, int C, int flip, int accumulate, int SEG, int SPR, int CVP, int walign) {
    typedef DwVec<T, VT> Vec;
    const int CV = C / VT, R = 256 / CVP, cvl = threadIdx.x % CVP, rl = threadIdx.x / CVP;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);          // consecutive segments (and their halo rows) share an XCD's L2
    const int s = bid * R + rl, cv = blockIdx.y * CVP + cvl;
    if (s >= N * H * SPR || cv >= CV) return;
    const int sx = s % SPR, row = s / SPR, oy = row % H;
    const int x0 = sx * SEG, x1 = min(W, x0 + SEG);
    float wr[9][VT], br[VT];
    {
        float wf[9 * VT];                                       // the 9*VT weights of this channel group are contiguous
        const float* wp = w + (size_t)cv * VT * 9;
        if constexpr (VT % 4 == 0) {
            if (walign) {
#pragma unroll
                for (int i = 0; i < 9 * VT / 4; ++i) {
                    const float4 q = reinterpret_cast<const float4*>(wp)[i];
                    wf[4 * i] = q.x; wf[4 * i + 1] = q.y; wf[4 * i + 2] = q.z; wf[4 * i + 3] = q.w;
                }
            } else {
#pragma unroll
                for (int i = 0; i < 9 * VT; ++i) wf[i] = wp[i];
            }
        } else {
#pragma unroll
            for (int i = 0; i < 9 * VT; ++i) wf[i] = wp[i];
        }
#pragma unroll
        for (int e = 0; e < VT; ++e) {
            br[e] = b ? b[cv * VT + e] : 0.f;
#pragma unroll
            for (int t = 0; t < 9; ++t) wr[t][e] = flip ? wf[e * 9 + 8 - t] : wf[e * 9 + t];
        }
    }
    const T* rowp[3]; bool vy[3];
    dw_rows<T, VT>(x, row, oy, H, W, C, cv, rowp, vy);
    Vec c0[3], c1[3], c2[3], n1[3], n2[3];
    dw_load_col<T, VT>(rowp, vy, x0 - 1, W, C, c0); dw_load_col<T, VT>(rowp, vy, x0, W, C, c1); dw_load_col<T, VT>(rowp, vy, x0 + 1, W, C, c2);
    dw_load_col<T, VT>(rowp, vy, x0 + 2 < x1 + 1 ? x0 + 2 : -1, W, C, n1);
    for (int ox = x0; ox < x1; ++ox) {
        dw_load_col<T, VT>(rowp, vy, ox + 3 < x1 + 1 ? ox + 3 : -1, W, C, n2);      // columns past the segment's halo are never needed
        float a[VT], xv[VT];
#pragma unroll
        for (int e = 0; e < VT; ++e) a[e] = br[e];
        // bf16: every product a written-out fused multiply-add, row-major taps on top of the bias - the fp32 sum of dwconv3x3_win_k bit for bit, so the two bf16
        // routes store the same values (left to the compiler, a few products stayed unfused, and where the ten terms cancel the last fp32 bit was up to 29
        // bf16 ulps of the result).  fp32 has no window twin and keeps the compiler's contraction.
        auto mac = [](float w_, float x_, float a_) {
            if constexpr (sizeof(T) == 2) return __builtin_fmaf(w_, x_, a_);
            else return a_ + w_ * x_;
        };
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            c0[r].unpack(xv);
#pragma unroll
            for (int e = 0; e < VT; ++e) a[e] = mac(wr[r * 3][e], xv[e], a[e]);
            c1[r].unpack(xv);
#pragma unroll
            for (int e = 0; e < VT; ++e) a[e] = mac(wr[r * 3 + 1][e], xv[e], a[e]);
            c2[r].unpack(xv);
#pragma unroll
            for (int e = 0; e < VT; ++e) a[e] = mac(wr[r * 3 + 2][e], xv[e], a[e]);
        }
        const size_t o = ((size_t)row * W + ox) * C + cv * VT;
        Vec ov;
        if (accumulate) {
            ov.load(z + o); ov.unpack(xv);
#pragma unroll
            for (int e = 0; e < VT; ++e) a[e] += xv[e];
        }
        ov.pack(a); ov.store(z + o);
        if (y) {
#pragma unroll
            for (int e = 0; e < VT; ++e) a[e] = gelu_f(a[e]);
            ov.pack(a); ov.store(y + o);
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) { c0[r] = c1[r]; c1[r] = c2[r]; c2[r] = n1[r]; n1[r] = n2[r]; }
    }
}

// ---- the 3x3 walks again, built for instruction count (round 5; bf16).  What the counters and three ablations said about dwconv3x3_row_k on the PVTv2 Mlp
// shapes (tools/dw_micro.py, tools/prof_dw_pmc.sh, tools/dw_dbg.py): it fetches 1.13x the algorithmic bytes (the halo rows hit the L2), keeping more loads
// in flight makes it slower, and with two of the three rows and all stores switched off it still takes 77 of 84 us - while a plain copy of the same tensors
// streams at 7 TB/s.  It is bound by vector instructions: every step re-unpacks the whole 3x3 window (72 shift / and per 8 channels), multiplies channel
// by channel, rotates the window through register moves (which also forces a vmcnt wait per step) and guards every load with a branch.  Here:
//   * the window lives UNPACKED in registers as channel pairs (3 columns x 3 rows x VT/2 float2): only the new column is unpacked per step;
//   * all arithmetic is packed (v_pk_fma_f32: two channels per instruction), GELU and its derivative too (erf_nb2);
//   * window slots and the ring of D = 3 prefetched (packed) columns are addressed by compile-time indices (the step loop is unrolled by 3 = a full
//     rotation of both), so nothing is moved and a column is fetched three steps before it is unpacked;
//   * halo rows, image border and segment end are buffer-descriptor range checks (offset with bit 31 set: loads return zeros, stores are dropped) - plain
//     integer arithmetic on byte offsets, no branches in the walk.  Tensors below 2 GB (host).
// Same order of the nine products per channel as dwconv3x3_row_k (row-major taps on top of the bias), every one a fused multiply-add; the row walk
// writes its fused multiply-adds out too (the compiler had left a few of its products unfused, v_pk_mul + v_pk_add), so the two form the same fp32 sum and
// store the same bf16 values (tests/test_gpu_vit_kernels.py: accumulate = 1 onto zeros against accumulate = 0; both sit at the bf16 rounding error against
// a float64 conv).
// Measured (tools/dw_micro.py, 16 x 88 x 88 x 512): conv + GELU 130 -> 108 us, data gradient 84 -> 62, weight gradient 100 -> 71, with dz = dy * gelu'(z) 155 -> 122;
// PVT_PraNet_V2 bs 16: 10.93 -> 10.69 ms per step.  The instruction count fell 2.5-3x, the time by a quarter: with loads and stores switched off the walk still
// takes 52 of 55 us (tools/dw_dbg.py) - what is left is issue-bound at roughly twice the ideal 4 cycles per wave instruction.
typedef unsigned dw_u4 __attribute__((ext_vector_type(4)));
typedef unsigned dw_u2 __attribute__((ext_vector_type(2)));
template <typename T, int VT>
__device__ __forceinline__ void dw_bload(DwVec<T, VT>& v, __amdgpu_buffer_rsrc_t rs, unsigned off) {
    constexpr int NW = DwVec<T, VT>::NW;
    if constexpr (NW == 4) { const dw_u4 q = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0); v.w[0] = q.x; v.w[1] = q.y; v.w[2] = q.z; v.w[3] = q.w; }
    else if constexpr (NW == 2) { const dw_u2 q = __builtin_amdgcn_raw_buffer_load_b64(rs, off, 0, 0); v.w[0] = q.x; v.w[1] = q.y; }
    else v.w[0] = __builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0);
}
template <typename T, int VT>
__device__ __forceinline__ void dw_bstore(const DwVec<T, VT>& v, __amdgpu_buffer_rsrc_t rs, unsigned off) {
    constexpr int NW = DwVec<T, VT>::NW;
    if constexpr (NW == 4) { dw_u4 q; q.x = v.w[0]; q.y = v.w[1]; q.z = v.w[2]; q.w = v.w[3]; __builtin_amdgcn_raw_buffer_store_b128(q, rs, off, 0, 0); }
    else if constexpr (NW == 2) { dw_u2 q; q.x = v.w[0]; q.y = v.w[1]; __builtin_amdgcn_raw_buffer_store_b64(q, rs, off, 0, 0); }
    else __builtin_amdgcn_raw_buffer_store_b32(v.w[0], rs, off, 0, 0);
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t dw_rsrc(const void* p) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)((unsigned long long)p >> 32)) << 32) |
                                                     (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned long long)p)), 0, (int)0x80000000u, 0x00020000);
}
constexpr unsigned DW_INV = 0x80000000u;
// -DPN2_DW_ABLATE (tools/dw_dbg.py): bit 1 of `flip` switches the two halo rows off, bit 2 the stores - what the walk costs without its memory traffic
#ifdef PN2_DW_ABLATE
#define DW_ABL_ROW(f, r) (((f) & 2) && (r) != 1)
#define DW_ABL_ST(f) ((f) & 4)
#else
#define DW_ABL_ROW(f, r) false
#define DW_ABL_ST(f) false
#endif
constexpr int DW_D = 3;          // packed columns in flight ahead of the window (= the unroll of the step loop)
__device__ __forceinline__ unsigned dw_mask(bool ok) { unsigned m = ok ? 0u : DW_INV; asm volatile("" : "+v"(m)); return m; }      // (opaque: see above)
// bf16 pair -> two floats / back
__device__ __forceinline__ dwf2 dw_unpk(unsigned w) { return dwf2{__uint_as_float(w << 16), __uint_as_float(w & 0xffff0000u)}; }
template <int VT>
__device__ __forceinline__ void dw_unpack_col(const DwVec<bf16_t, VT> (&c)[3], dwf2 (&o)[3][VT / 2]) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int i = 0; i < VT / 2; ++i) o[r][i] = dw_unpk(c[r].w[i]);
}
// the VT weights of tap t as channel pairs, from the [c][9] fp32 master
template <int VT>
__device__ __forceinline__ void dw_weights(const float* __restrict__ w, int cv, int flip, int walign, dwf2 (&wr)[9][VT / 2]) {
    float wf[9 * VT];
    const float* wp = w + (size_t)cv * VT * 9;
    if (VT % 4 == 0 && walign) {
#pragma unroll
        for (int i = 0; i < 9 * VT / 4; ++i) {
            const float4 q = reinterpret_cast<const float4*>(wp)[i];
            wf[4 * i] = q.x; wf[4 * i + 1] = q.y; wf[4 * i + 2] = q.z; wf[4 * i + 3] = q.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 9 * VT; ++i) wf[i] = wp[i];
    }
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int i = 0; i < VT / 2; ++i) wr[t][i] = flip ? dwf2{wf[(2 * i) * 9 + 8 - t], wf[(2 * i + 1) * 9 + 8 - t]} : dwf2{wf[(2 * i) * 9 + t], wf[(2 * i + 1) * 9 + t]};
}

// CS: the kernel also leaves the column sums of what it stores (as stored: the rounded values) per workgroup, cpart[gridDim.x][C] - the bias gradient of the
// nn.Linear in front (Mlp.fc1, whose dY this data gradient IS) without the second read of the largest gradient tensor of the block by the column-sum pass.
template <int VT, bool GELU, bool CS = false>
__global__ __launch_bounds__(256) void dwconv3x3_win_k(const bf16_t* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b, bf16_t* __restrict__ z,
                                                       bf16_t* __restrict__ y, int N, int H, int W, int C, int flip, int SEG, int SPR, int CVP, int walign,
                                                       float* __restrict__ cpart = nullptr) {
    typedef DwVec<bf16_t, VT> Vec;
    constexpr int NP = VT / 2;
    const int CV = C / VT, R = 256 / CVP, cvl = threadIdx.x % CVP, rl = threadIdx.x / CVP;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);          // consecutive segments (and their halo rows) share an XCD's L2
    int s = bid * R + rl;
    const int cv = blockIdx.y * CVP + cvl;
    bool live = true;
    if (s >= N * H * SPR || cv >= CV) {
        if constexpr (!CS) return;
        live = false; s = 0;          // (CS: every thread reaches the workgroup's column-sum exchange; a dead one walks no step)
    }
    const int cvx = live ? cv : 0;
    const int sx = s % SPR, row = s / SPR, oy = row % H;
    const int x0 = sx * SEG, x1 = live ? min(W, x0 + SEG) : x0, hi = min(x1, W - 1);          // columns x0 - 1 .. hi are read (the image's and the segment's halo)
    dwf2 wr[9][NP], br[NP];
    dw_weights<VT>(w, cvx, flip & 1, walign, wr);
#pragma unroll
    for (int i = 0; i < NP; ++i) br[i] = b ? dwf2{b[cvx * VT + 2 * i], b[cvx * VT + 2 * i + 1]} : dw2(0.f);
    const __amdgpu_buffer_rsrc_t rx = dw_rsrc(x), rz = dw_rsrc(z), ry = dw_rsrc(GELU ? y : z);
    const unsigned Cb = (unsigned)C * 2u, cvb = (unsigned)(cvx * VT) * 2u;
    unsigned rowb[3], rowm[3];          // byte offset of column 0 of the three input rows; bit 31 when the row lies outside the image
#pragma unroll
    for (int r = 0; r < 3; ++r) { rowb[r] = (unsigned)((row + r - 1) * W) * Cb + cvb; rowm[r] = dw_mask((unsigned)(oy + r - 1) < (unsigned)H && !DW_ABL_ROW(flip, r)); }
    const unsigned outb = (unsigned)(row * W) * Cb + cvb;
    Vec ring[DW_D][3];
    dwf2 win[3][3][NP];
    dwf2 csum[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) csum[i] = dw2(0.f);
    auto fetch = [&](Vec (&c)[3], int ix) {
        const unsigned co = (unsigned)ix * Cb, cm = dw_mask((unsigned)ix <= (unsigned)hi);
#pragma unroll
        for (int r = 0; r < 3; ++r) dw_bload<bf16_t, VT>(c[r], rx, (rowb[r] + co) | rowm[r] | cm);          // (the masks are OR-ed in: an add of two set bits 31 would carry out)
    };
    {
        Vec p0[3], p1[3];
        fetch(p0, x0 - 1); fetch(p1, x0);
#pragma unroll
        for (int k = 0; k < DW_D; ++k) fetch(ring[k], x0 + 1 + k);
        dw_unpack_col<VT>(p0, win[0]); dw_unpack_col<VT>(p1, win[1]);
    }
    for (int xb = x0; xb < x1; xb += 3) {
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const int ox = xb + u;
            dw_unpack_col<VT>(ring[u], win[(u + 2) % 3]);          // column ox + 1 takes the slot of column ox - 2
            fetch(ring[u], ox + 1 + DW_D);
            const unsigned o = (outb + (unsigned)ox * Cb) | dw_mask(ox < x1 && !DW_ABL_ST(flip));
            dwf2 a[NP];
#pragma unroll
            for (int i = 0; i < NP; ++i) a[i] = br[i];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int k = 0; k < 3; ++k)
#pragma unroll
                    for (int i = 0; i < NP; ++i) a[i] = dwfma(wr[r * 3 + k][i], win[(u + k) % 3][r][i], a[i]);
            Vec ov;
#pragma unroll
            for (int i = 0; i < NP; ++i) ov.w[i] = TT<bf16_t>::cvt2(a[i].x, a[i].y);
            dw_bstore<bf16_t, VT>(ov, rz, o);
            if constexpr (CS) {
                if (ox < x1) {
#pragma unroll
                    for (int i = 0; i < NP; ++i) csum[i] += dw_unpk(ov.w[i]);
                }
            }
            if constexpr (GELU) {
#pragma unroll
                for (int i = 0; i < NP; ++i) { const dwf2 g = gelu_f2(a[i]); ov.w[i] = TT<bf16_t>::cvt2(g.x, g.y); }
                dw_bstore<bf16_t, VT>(ov, ry, o);
            }
            __builtin_amdgcn_sched_barrier(0);          // one step at a time: the scheduler otherwise gathers the waits of all three steps at the top of the loop body
        }
    }
    if constexpr (CS) {          // the R segment lanes of a channel group meet in LDS (fixed order); one partial row per workgroup
        __shared__ float cs_sh[256 * VT];
#pragma unroll
        for (int i = 0; i < NP; ++i) { cs_sh[(rl * CVP + cvl) * VT + 2 * i] = csum[i].x; cs_sh[(rl * CVP + cvl) * VT + 2 * i + 1] = csum[i].y; }
        __syncthreads();
        if (rl == 0 && cv < CV) {
#pragma unroll
            for (int e = 0; e < VT; ++e) {
                float t = 0.f;
                for (int r = 0; r < R; ++r) t += cs_sh[(r * CVP + cvl) * VT + e];
                cpart[(size_t)blockIdx.x * C + cv * VT + e] = t;
            }
        }
    }
}

// weight gradient on the same window: partial[chunk][C*10] as dwconv3x3_wgrad_row_k leaves it (same segments per lane, same order of the sums).
template <int VT, bool ZP>
__global__ __launch_bounds__(256) void dwconv3x3_wgrad_win_k(const bf16_t* __restrict__ dz, const bf16_t* __restrict__ x, float* __restrict__ partial, int N, int H, int W, int C,
                                                             int SEG, int SPR, int SPC, int CVP, const bf16_t* __restrict__ zpre, bf16_t* __restrict__ dz_out) {
    typedef DwVec<bf16_t, VT> Vec;
    typedef DwVec<bf16_t, VT> Vec1;
    constexpr int NP = VT / 2;
    extern __shared__ float sh[];            // [R][CVP*VT] reused for each of the 10 sums
    const int CV = C / VT, R = 256 / CVP, cvl = threadIdx.x % CVP, rl = threadIdx.x / CVP;
    const int chunk = xcd_remap(blockIdx.x, gridDim.x), cv = blockIdx.y * CVP + cvl;
    const int nseg = N * H * SPR;
    dwf2 a[10][NP];
#pragma unroll
    for (int t = 0; t < 10; ++t)
#pragma unroll
        for (int i = 0; i < NP; ++i) a[t][i] = dw2(0.f);
    if (cv < CV) {
        const __amdgpu_buffer_rsrc_t rx = dw_rsrc(x), rd = dw_rsrc(dz), rzp = dw_rsrc(ZP ? zpre : dz), ro = dw_rsrc(ZP ? dz_out : (bf16_t*)nullptr);
        const unsigned Cb = (unsigned)C * 2u, cvb = (unsigned)(cv * VT) * 2u;
        const int s1 = min(nseg, (chunk + 1) * SPC);
        for (int s = chunk * SPC + rl; s < s1; s += R) {
            const int sx = s % SPR, row = s / SPR, oy = row % H;
            const int x0 = sx * SEG, x1 = min(W, x0 + SEG), hi = min(x1, W - 1);
            unsigned rowb[3], rowm[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) { rowb[r] = (unsigned)((row + r - 1) * W) * Cb + cvb; rowm[r] = dw_mask((unsigned)(oy + r - 1) < (unsigned)H); }
            const unsigned outb = (unsigned)(row * W) * Cb + cvb;
            Vec ring[DW_D][3];
            Vec1 dring[DW_D], zring[DW_D];
            dwf2 win[3][3][NP];
            auto fetch = [&](Vec (&c)[3], int ix) {
                const unsigned co = (unsigned)ix * Cb, cm = dw_mask((unsigned)ix <= (unsigned)hi);
#pragma unroll
                for (int r = 0; r < 3; ++r) dw_bload<bf16_t, VT>(c[r], rx, (rowb[r] + co) | rowm[r] | cm);
            };
            auto fetch_d = [&](int k, int ox) {          // dz (and the GELU input) of output column ox; zeros past the segment
                const unsigned o = (outb + (unsigned)ox * Cb) | dw_mask(ox < x1);
                dw_bload<bf16_t, VT>(dring[k], rd, o);
                if constexpr (ZP) dw_bload<bf16_t, VT>(zring[k], rzp, o);
            };
            {
                Vec p0[3], p1[3];
                fetch(p0, x0 - 1); fetch(p1, x0);
#pragma unroll
                for (int k = 0; k < DW_D; ++k) { fetch(ring[k], x0 + 1 + k); fetch_d(k, x0 + k); }
                dw_unpack_col<VT>(p0, win[0]); dw_unpack_col<VT>(p1, win[1]);
            }
            for (int xb = x0; xb < x1; xb += 3) {
#pragma unroll
                for (int u = 0; u < 3; ++u) {
                    const int ox = xb + u;
                    dw_unpack_col<VT>(ring[u], win[(u + 2) % 3]);
                    fetch(ring[u], ox + 1 + DW_D);
                    dwf2 d[NP];
#pragma unroll
                    for (int i = 0; i < NP; ++i) d[i] = dw_unpk(dring[u].w[i]);
                    if constexpr (ZP) {
                        Vec1 pk;
#pragma unroll
                        for (int i = 0; i < NP; ++i) {
                            const dwf2 g = d[i] * gelu_grad2(dw_unpk(zring[u].w[i]));
                            pk.w[i] = TT<bf16_t>::cvt2(g.x, g.y);
                            d[i] = dw_unpk(pk.w[i]);                  // accumulate what the data-gradient pass will read (the rounded value)
                        }
                        dw_bstore<bf16_t, VT>(pk, ro, (outb + (unsigned)ox * Cb) | dw_mask(ox < x1));
                    }
                    fetch_d(u, ox + DW_D);
#pragma unroll
                    for (int i = 0; i < NP; ++i) a[9][i] += d[i];
#pragma unroll
                    for (int r = 0; r < 3; ++r)
#pragma unroll
                        for (int k = 0; k < 3; ++k)
#pragma unroll
                            for (int i = 0; i < NP; ++i) a[r * 3 + k][i] = dwfma(d[i], win[(u + k) % 3][r][i], a[r * 3 + k][i]);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 10; ++t) {
#pragma unroll
        for (int i = 0; i < NP; ++i) { sh[(rl * CVP + cvl) * VT + 2 * i] = a[t][i].x; sh[(rl * CVP + cvl) * VT + 2 * i + 1] = a[t][i].y; }
        __syncthreads();
        if (rl == 0 && cv < CV) {
#pragma unroll
            for (int e = 0; e < VT; ++e) {
                float s_ = 0.f;
                for (int r = 0; r < R; ++r) s_ += sh[(r * CVP + cvl) * VT + e];
                const int c = cv * VT + e;
                partial[(size_t)chunk * C * 10 + (t < 9 ? c * 9 + t : C * 9 + c)] = s_;
            }
        }
        __syncthreads();
    }
}

// weight gradient, same walk: partial[chunk][C*10]; a block = CVP channel groups x R segment lanes, a chunk = SPC segments.
// zpre non-null: dz = dy * gelu'(zpre) is formed here (and written to dz_out) instead of by a separate pn2_gelu_bwd pass.
template <typename T, int VT>
__global__ __launch_bounds__(256) void dwconv3x3_wgrad_row_k(const T* __restrict__ dz, const T* __restrict__ x, float* __restrict__ partial, int N, int H, int W, int C,
                                                             int SEG, int SPR, int SPC, int CVP, const T* __restrict__ zpre, T* __restrict__ dz_out) {
    typedef DwVec<T, VT> Vec;
    extern __shared__ float sh[];            // [R][CVP*VT] reused for each of the 10 sums
    const int CV = C / VT, R = 256 / CVP, cvl = threadIdx.x % CVP, rl = threadIdx.x / CVP;
    const int chunk = xcd_remap(blockIdx.x, gridDim.x), cv = blockIdx.y * CVP + cvl;
    const int nseg = N * H * SPR;
    float a[10][VT];
#pragma unroll
    for (int t = 0; t < 10; ++t)
#pragma unroll
        for (int e = 0; e < VT; ++e) a[t][e] = 0.f;
    if (cv < CV) {
        const int s1 = min(nseg, (chunk + 1) * SPC);
        for (int s = chunk * SPC + rl; s < s1; s += R) {
            const int sx = s % SPR, row = s / SPR, oy = row % H;
            const int x0 = sx * SEG, x1 = min(W, x0 + SEG);
            const T* rowp[3]; bool vy[3];
            dw_rows<T, VT>(x, row, oy, H, W, C, cv, rowp, vy);
            const size_t o0 = ((size_t)row * W) * C + cv * VT;
            Vec c0[3], c1[3], c2[3], n1[3], dn, zn;
            zn.zero();
            dw_load_col<T, VT>(rowp, vy, x0 - 1, W, C, c0); dw_load_col<T, VT>(rowp, vy, x0, W, C, c1); dw_load_col<T, VT>(rowp, vy, x0 + 1, W, C, c2);
            dn.load(dz + o0 + (size_t)x0 * C);
            if (zpre) zn.load(zpre + o0 + (size_t)x0 * C);
            for (int ox = x0; ox < x1; ++ox) {
                const Vec dc = dn, zc = zn;
                dw_load_col<T, VT>(rowp, vy, ox + 2 < x1 + 1 ? ox + 2 : -1, W, C, n1);
                if (ox + 1 < x1) {
                    dn.load(dz + o0 + (size_t)(ox + 1) * C);
                    if (zpre) zn.load(zpre + o0 + (size_t)(ox + 1) * C);
                }
                float d[VT], xv[VT];
                dc.unpack(d);
                if (zpre) {
                    zc.unpack(xv);
#pragma unroll
                    for (int e = 0; e < VT; ++e) d[e] *= gelu_grad(xv[e]);
                    Vec pk; pk.pack(d); pk.store(dz_out + o0 + (size_t)ox * C);
                    pk.unpack(d);                              // accumulate what the data-gradient pass will read (the rounded value)
                }
#pragma unroll
                for (int e = 0; e < VT; ++e) a[9][e] += d[e];
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    c0[r].unpack(xv);
#pragma unroll
                    for (int e = 0; e < VT; ++e) a[r * 3][e] += d[e] * xv[e];
                    c1[r].unpack(xv);
#pragma unroll
                    for (int e = 0; e < VT; ++e) a[r * 3 + 1][e] += d[e] * xv[e];
                    c2[r].unpack(xv);
#pragma unroll
                    for (int e = 0; e < VT; ++e) a[r * 3 + 2][e] += d[e] * xv[e];
                }
#pragma unroll
                for (int r = 0; r < 3; ++r) { c0[r] = c1[r]; c1[r] = c2[r]; c2[r] = n1[r]; }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 10; ++t) {
#pragma unroll
        for (int e = 0; e < VT; ++e) sh[(rl * CVP + cvl) * VT + e] = a[t][e];
        __syncthreads();
        if (rl == 0 && cv < CV) {
#pragma unroll
            for (int e = 0; e < VT; ++e) {
                float s = 0.f;
                for (int r = 0; r < R; ++r) s += sh[(r * CVP + cvl) * VT + e];
                const int c = cv * VT + e;
                partial[(size_t)chunk * C * 10 + (t < 9 ? c * 9 + t : C * 9 + c)] = s;
            }
        }
        __syncthreads();
    }
}

// y[n][r][c] = x[n][r][c] * s[n]   (DropPath: per-sample keep mask / keep_prob, timm.models.layers.DropPath used at pvtv2.py:125,148-149)
template <typename T>
__global__ __launch_bounds__(256) void scale_samples_k(const T* __restrict__ x, T* __restrict__ y, const float* __restrict__ s, const T* __restrict__ res,
                                                       size_t vec_per_sample, size_t nvec) {
    constexpr int V = TT<T>::VEC;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (size_t)gridDim.x * 256) {
        float v[V], r[V];
        ldv<T>(x + i * V, v);
        const float f = s[i / vec_per_sample];
        if (res) {                    // x + drop_path(f(x)) of Block.forward in one pass
            ldv<T>(res + i * V, r);
#pragma unroll
            for (int e = 0; e < V; ++e) v[e] = v[e] * f + r[e];
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e) v[e] *= f;
        }
        stv<T>(y + i * V, v);
    }
}

using namespace pn2_host;
constexpr int GRID_CAP = 16384;

inline int ln_lpr(int dt, int C) {
    const int V = vec_of(dt);
    if (C % V) return -1;
    int lpr = pow2ceil(C / V);
    if (lpr < 8) lpr = 8;
    if (lpr > 64) lpr = 64;
    return ((C / V + lpr - 1) / lpr <= LN_NV) ? lpr : -1;
}

inline int rows_for(int M, int unit) {          /* rows per block of the column-sum style reductions: ~ROWS_TARGET blocks, a multiple of `unit` */
    constexpr int target = 512;   // 2 workgroups per CU measured best (256: -1.7 %, 1024: -1.1 % on config 4)
    int rows = (M + target - 1) / target;
    rows = ((rows + unit - 1) / unit) * unit;
    return rows < unit ? unit : rows;
}

// column sums of a [M][C] tensor: cvp channel vectors x 256 / cvp row lanes per block, `rows` rows per block.  pn2_colsum and pn2_colsum_job_blocks
struct ColsumPlan { int cvp, rows, nblk; };
inline int colsum_plan(int dt, int M, int C, int ld, ColsumPlan& p) {
    const int V = vec_of(dt);
    if (C % V || ld % V) return -2;
    p.cvp = pow2ceil(C / V); if (p.cvp > 256) p.cvp = 256;
    p.rows = rows_for(M, 256 / p.cvp);
    p.nblk = (M + p.rows - 1) / p.rows;
    return 0;
}

// channels per thread (VT) and segment length of the depth-wise walks, from a sweep on MI355X (tools/dw_micro.py):
// kind 0 = conv + GELU (ALU-heavier: 8-byte vectors, more waves), 1 = plain conv / data gradient (16-byte vectors while there are threads to
// spare), 2 = weight gradient (80 accumulators per 8 channels: 2 channels per thread keeps 8 waves per SIMD).  Short segments for small tensors.
// PN2_DW_WIN=0: the round-3 walks (dwconv3x3_row_k / dwconv3x3_wgrad_row_k) instead of the window kernels (A/B; bf16 only - fp32 always takes them)
inline int dw_win() { static const int v = [] { const char* e = getenv("PN2_DW_WIN"); return e ? atoi(e) : 1; }(); return v; }

inline void dw_row_geometry(int dt, int kind, int N, int H, int W, int C, int& VT, int& SEG, int& SPR) {
    const int vmax = vec_of(dt);
    auto threads = [&](int vt, int target) { return (long long)N * H * ((W + target - 1) / target) * (C / vt); };
    // window kernels: a segment costs ~150 instructions and two memory latencies before its first output (weights, the first five columns); 32-pixel segments
    // where the tensor still gives 4 resident waves per SIMD twice over (stage 1 of PVTv2-B2 at 352^2: 117 -> 108 us conv + GELU, 71 -> 62 us data gradient)
    static const int seg_env = [] { const char* e = getenv("PN2_DW_SEG"); return e ? atoi(e) : 32; }();
    int target = 16;
    if (kind == 2) VT = 2;
    else {
        VT = kind == 0 ? vmax / 2 : vmax;
        while (VT > 2 && ((C % VT) || (VT == vmax && kind == 1 && threads(VT, 16) < 2LL * 256 * 8 * 64))) VT >>= 1;
        if (threads(VT, 16) < 200000) target = 8;
    }
    if (seg_env > 0 && dt == PN2_BF16 && dw_win() && threads(4, seg_env) >= 2LL * 256 * 4 * 64 * 4) target = seg_env;
    SPR = (W + target - 1) / target; SEG = (W + SPR - 1) / SPR;
}

// the bf16 window kernels (dwconv3x3_win_k / dwconv3x3_wgrad_win_k) address the tensor with 32-bit byte offsets
inline bool dw_use_win(int dt, int N, int H, int W, int C) { return dt == PN2_BF16 && dw_win() && (long long)N * H * W * C * 2 < 0x7fff0000LL; }

// the built row walks dwconv3x3_row_k / dwconv3x3_wgrad_row_k: VT = 8 (bf16 only), 4, and 2 for everything else
template <typename T, typename F>
int with_dw_vt(int VT, F f) {
    if constexpr (sizeof(T) == 2) { if (VT == 8) return f(Int<8>{}); }
    return VT == 4 ? f(Int<4>{}) : f(Int<2>{});
}

// launch plan of pn2_dwconv3x3 / pn2_dwconv3x3_colsum: one lane per row segment; a block spans 1 KB of one pixel
struct DwPlan { bool win; int VT, SEG, SPR, cvp; dim3 grid; };
inline DwPlan dw_plan(int dt, bool gelu, bool accumulate, int N, int H, int W, int C) {
    DwPlan p;
    dw_row_geometry(dt, gelu ? 0 : 1, N, H, W, C, p.VT, p.SEG, p.SPR);
    p.win = !accumulate && dw_use_win(dt, N, H, W, C);
    if (p.win) p.VT = C % 4 == 0 ? 4 : 2;          // the window walk: 4 or 2 channels per thread
    const int CV = C / p.VT, lanes = (dt == PN2_F32 ? 256 : 512) / p.VT;
    p.cvp = CV >= lanes ? lanes : pow2ceil(CV);
    const int R = 256 / p.cvp, nseg = N * H * p.SPR;
    p.grid = dim3((nseg + R - 1) / R, (CV + p.cvp - 1) / p.cvp);
    return p;
}

int dwconv3x3_launch(int dt, const void* x, const float* w, const float* b, void* z, void* y_gelu, int N, int H, int W, int C, int flip, int accumulate, float* cpart, int cblk,
                     hipStream_t st) {
    if (!x || !w || !z) return -1;
    if (C % 2 || N < 1 || H < 1 || W < 1) return -2;
    const DwPlan p = dw_plan(dt, y_gelu != nullptr, accumulate != 0, N, H, W, C);
    const int walign = ((uintptr_t)w & 15) == 0;
    if (p.win) {
        if (cpart && (y_gelu || cblk != (int)p.grid.x)) return -2;
        auto win = [&](auto vt, auto gelu, auto cs) {
            return pn2_launch<dwconv3x3_win_k<decltype(vt)::value, decltype(gelu)::value, decltype(cs)::value>>(p.grid, dim3(256), 0, 0, st, (const bf16_t*)x, w, b, (bf16_t*)z, (bf16_t*)y_gelu,
                                                                                                                 N, H, W, C, flip, p.SEG, p.SPR, p.cvp, walign, cpart);
        };
        auto win_vt = [&](auto vt) { return cpart ? win(vt, Bool<false>{}, Bool<true>{}) : (y_gelu ? win(vt, Bool<true>{}, Bool<false>{}) : win(vt, Bool<false>{}, Bool<false>{})); };
        return p.VT == 4 ? win_vt(Int<4>{}) : win_vt(Int<2>{});
    }
    if (cpart) return -2;          // column sums only ride on the window kernels
    return with_storage_dtype(dt, [&](auto ty) {
        using T = type_of<decltype(ty)>;
        return with_dw_vt<T>(p.VT, [&](auto vt) {
            return pn2_launch<dwconv3x3_row_k<T, decltype(vt)::value>>(p.grid, dim3(256), 0, 0, st, (const T*)x, w, b, (T*)z, (T*)y_gelu, N, H, W, C, flip, accumulate, p.SEG, p.SPR, p.cvp, walign);
        });
    });
}

// launch plan of pn2_dwconv3x3_wgrad: a block spans 256 contiguous bytes of one pixel and takes SPC segments; ~1536 workgroups over (chunks x channel groups)
struct DwWgradPlan { bool win; int VT, SEG, SPR, SPC, cvp, nchunk, gy; };
inline DwWgradPlan dw_wgrad_plan(int dt, int N, int H, int W, int C) {
    DwWgradPlan p;
    dw_row_geometry(dt, 2, N, H, W, C, p.VT, p.SEG, p.SPR);
    p.win = dw_use_win(dt, N, H, W, C);
    if (p.win) p.VT = C % 4 == 0 ? 4 : 2;          // window kernel: 4 channels per thread (20 packed accumulators)
    const int CV = C / p.VT, lanes = (dt == PN2_F32 ? 32 : 64) / p.VT * 2;
    p.cvp = CV >= lanes ? lanes : pow2ceil(CV);
    const int R = 256 / p.cvp, nseg = N * H * p.SPR;
    p.gy = (CV + p.cvp - 1) / p.cvp;
    int want = 1536 / p.gy; if (want < 1) want = 1;
    p.SPC = (nseg + want - 1) / want;
    p.SPC = ((p.SPC + R - 1) / R) * R;
    p.nchunk = (nseg + p.SPC - 1) / p.SPC;
    return p;
}

}  // namespace

extern "C" {

int pn2_layernorm_fwd(int dt, const void* x, int ld_x, void* y, int ld_y, int M, int C, const float* gamma, const float* beta, float eps,
                      float* mean, float* rstd, void* stream) {
    if (!x || !y || !gamma || !beta || !mean || !rstd || M < 1) return -1;
    const int lpr = ln_lpr(dt, C);
    if (lpr < 0) return -2;
    const int rows_per_blk = 4 * (64 / lpr);
    return with_storage_dtype(dt, [&](auto ty) {
        using T = type_of<decltype(ty)>;
        return pn2_launch<ln_fwd_k<T>>(dim3((M + rows_per_blk - 1) / rows_per_blk), dim3(256), 0, 0, (hipStream_t)stream, (const T*)x, ld_x, (T*)y, ld_y, M, C, gamma, beta, eps, mean, rstd, lpr);
    });
}

int pn2_rows_blocks(int M, int unit) { if (M < 1 || unit < 1) return -1; const int rows = rows_for(M, unit); return (M + rows - 1) / rows; }

int pn2_layernorm_bwd(int dt, const void* dy, int ld_dy, const void* x, int ld_x, int M, int C, const float* gamma, const float* mean, const float* rstd,
                      void* dx, int ld_dx, int accumulate_dx, float* pg, float* pb, int nblk, void* stream) {
    if (!dy || !x || !gamma || !mean || !rstd || !dx || !pg || !pb || M < 1 || nblk < 1) return -1;
    const int lpr = ln_lpr(dt, C);
    if (lpr < 0) return -2;
    const int nslot = 4 * (64 / lpr);
    const int rows = rows_for(M, nslot);
    if ((M + rows - 1) / rows != nblk) return -2;          // nblk must be pn2_rows_blocks(M, pn2_ln_slots(dt, C))
    const size_t lds = (size_t)2 * nslot * C * 4;
    if (lds > 64 * 1024) return -2;
    const bool nv1 = C / vec_of(dt) <= lpr;          // one channel vector per lane (C <= 512 bf16 / 256 fp32): the lean instantiation
    return with_storage_dtype(dt, [&](auto ty) {
        using T = type_of<decltype(ty)>;
        auto launch = [&](auto nv) {
            return pn2_launch<ln_bwd_k<T, decltype(nv)::value>>(dim3(nblk), dim3(256), lds, 0, (hipStream_t)stream, (const T*)dy, ld_dy, (const T*)x, ld_x, M, C, gamma, mean, rstd,
                                                                (T*)dx, ld_dx, accumulate_dx, pg, pb, rows, lpr);
        };
        return nv1 ? launch(Int<1>{}) : launch(Int<LN_NV>{});
    });
}

int pn2_ln_slots(int dt, int C) { const int lpr = ln_lpr(dt, C); return lpr < 0 ? -1 : 4 * (64 / lpr); }

int pn2_colsum_finalize(const float* partial, int nblk, int C, int ld, float* out, int accumulate, void* stream) {
    if (!partial || !out || nblk < 1 || C < 1) return -1;
    return pn2_launch<colsum_finalize_k>(dim3((C + 31) / 32), dim3(256), 0, 0, (hipStream_t)stream, partial, nblk, C, ld, out, accumulate);
}

int pn2_colsum_finalize_blocks(int C) { return C < 1 ? -1 : (C + 31) / 32; }

int pn2_colsum_finalize_multi(const pn2_colsum_job* jobs_dev, const int* block_start_dev, int njobs, int total_blocks, void* stream) {
    if (!table_ok(jobs_dev, block_start_dev, njobs, total_blocks)) return -1;
    return pn2_launch<colsum_finalize_multi_k>(dim3(total_blocks), dim3(256), 0, 0, (hipStream_t)stream, jobs_dev, block_start_dev, njobs);
}

int pn2_colsum(int dt, const void* dy, int ld, int M, int C, float* partial, int nblk, void* stream) {
    if (!dy || !partial || M < 1 || nblk < 1) return -1;
    ColsumPlan p;
    if (int rc = colsum_plan(dt, M, C, ld, p)) return rc;
    if (p.nblk != nblk) return -2;          // nblk must be pn2_rows_blocks(M, pn2_colsum_unit(dt, C))
    return with_storage_dtype(dt, [&](auto ty) {
        using T = type_of<decltype(ty)>;
        return pn2_launch<colsum_k<T>>(dim3(nblk), dim3(256), 256 * TT<T>::VEC * 4, 0, (hipStream_t)stream, (const T*)dy, ld, M, C, partial, p.rows, p.cvp);
    });
}

/* fills rows / cvp of a job for pn2_colsum_multi and returns its workgroup count (= rows of its partial buffer, as pn2_rows_blocks gives) */
int pn2_colsum_job_blocks(int dt, pn2_colsum_in_job* j) {
    if (!j || !j->dy || !j->partial || j->M < 1) return -1;
    ColsumPlan p;
    if (int rc = colsum_plan(dt, j->M, j->C, j->ld, p)) return rc;
    j->cvp = p.cvp; j->rows = p.rows;
    return p.nblk;
}

int pn2_colsum_multi(int dt, const pn2_colsum_in_job* jobs_dev, const int* block_start_dev, int njobs, int total_blocks, void* stream) {
    if (!table_ok(jobs_dev, block_start_dev, njobs, total_blocks)) return -1;
    return with_storage_dtype(dt, [&](auto ty) {
        using T = type_of<decltype(ty)>;
        return pn2_launch<colsum_multi_k<T>>(dim3(total_blocks), dim3(256), 256 * TT<T>::VEC * 4, 0, (hipStream_t)stream, jobs_dev, block_start_dev, njobs);
    });
}

int pn2_colsum_unit(int dt, int C) { int cvp = pow2ceil(C / vec_of(dt)); if (cvp > 256) cvp = 256; return 256 / cvp; }

int pn2_dwconv3x3(int dt, const void* x, const float* w, const float* b, void* z, void* y_gelu, int N, int H, int W, int C, int flip, int accumulate, void* stream) {
    return dwconv3x3_launch(dt, x, w, b, z, y_gelu, N, H, W, C, flip, accumulate, nullptr, 0, (hipStream_t)stream);
}
/* rows of `cpart` for pn2_dwconv3x3_colsum at this geometry (< 0: that entry does not serve it - run pn2_dwconv3x3 and a column-sum pass) */
int pn2_dwconv3x3_colsum_blocks(int dt, int N, int H, int W, int C) {
    if (dt != PN2_BF16 || C % 2 || N < 1 || H < 1 || W < 1) return -1;
    const DwPlan p = dw_plan(dt, false, false, N, H, W, C);
    return p.win && p.grid.x > 0 ? (int)p.grid.x : -1;
}
/* pn2_dwconv3x3 (no GELU, no accumulate) that also leaves cpart[nblk][C]: per-workgroup column sums of the stored result */
int pn2_dwconv3x3_colsum(int dt, const void* x, const float* w, const float* b, void* z, int N, int H, int W, int C, int flip, float* cpart, int nblk, void* stream) {
    if (!cpart || nblk < 1) return -1;
    return dwconv3x3_launch(dt, x, w, b, z, nullptr, N, H, W, C, flip, 0, cpart, nblk, (hipStream_t)stream);
}

int pn2_gelu_bwd(int dt, const void* dy, const void* z, void* dz, long long n, void* stream) {
    if (!dy || !z || !dz) return -1;
    const int V = vec_of(dt);
    if (n % V) return -2;
    return with_storage_dtype(dt, [&](auto ty) {
        using T = type_of<decltype(ty)>;
        return pn2_launch<gelu_bwd_k<T>>(dim3(grid_for((size_t)n / V, GRID_CAP)), dim3(256), 0, 0, (hipStream_t)stream, (const T*)dy, (const T*)z, (T*)dz, (size_t)n / V);
    });
}

int pn2_dwconv3x3_wgrad_blocks(int dt, int N, int H, int W, int C) {
    if ((dt != PN2_F32 && dt != PN2_BF16) || C % 2 || N < 1 || H < 1 || W < 1) return -1;
    return dw_wgrad_plan(dt, N, H, W, C).nchunk;
}

int pn2_dwconv3x3_wgrad(int dt, const void* dz, const void* x, float* partial, int nblk, int N, int H, int W, int C, const void* zpre, void* dz_out, void* stream) {
    if (!dz || !x || !partial || nblk < 1 || (zpre && !dz_out)) return -1;
    if (C % 2) return -2;
    const DwWgradPlan p = dw_wgrad_plan(dt, N, H, W, C);
    if (p.nchunk != nblk) return -2;                           // nblk must be pn2_dwconv3x3_wgrad_blocks(dt, N, H, W, C)
    const dim3 grid(p.nchunk, p.gy);
    const size_t lds = (size_t)256 * p.VT * 4;
    hipStream_t st = (hipStream_t)stream;
    if (p.win) {
        auto win = [&](auto vt, auto z) {
            return pn2_launch<dwconv3x3_wgrad_win_k<decltype(vt)::value, decltype(z)::value>>(grid, dim3(256), lds, 0, st, (const bf16_t*)dz, (const bf16_t*)x, partial, N, H, W, C, p.SEG, p.SPR, p.SPC, p.cvp,
                                                                                               (const bf16_t*)zpre, (bf16_t*)dz_out);
        };
        auto win_vt = [&](auto vt) { return zpre ? win(vt, Bool<true>{}) : win(vt, Bool<false>{}); };
        return p.VT == 4 ? win_vt(Int<4>{}) : win_vt(Int<2>{});
    }
    return with_storage_dtype(dt, [&](auto ty) {
        using T = type_of<decltype(ty)>;
        return with_dw_vt<T>(p.VT, [&](auto vt) {
            return pn2_launch<dwconv3x3_wgrad_row_k<T, decltype(vt)::value>>(grid, dim3(256), lds, 0, st, (const T*)dz, (const T*)x, partial, N, H, W, C, p.SEG, p.SPR, p.SPC, p.cvp, (const T*)zpre, (T*)dz_out);
        });
    });
}

int pn2_scale_samples(int dt, const void* x, void* y, const float* scale, const void* res, int N, long long per_sample, void* stream) {
    if (!x || !y || !scale || N < 1) return -1;
    const int V = vec_of(dt);
    if (per_sample % V) return -2;
    return with_storage_dtype(dt, [&](auto ty) {
        using T = type_of<decltype(ty)>;
        return pn2_launch<scale_samples_k<T>>(dim3(grid_for((size_t)N * per_sample / V, GRID_CAP)), dim3(256), 0, 0, (hipStream_t)stream, (const T*)x, (T*)y, scale, (const T*)res,
                                              (size_t)per_sample / V, (size_t)N * per_sample / V);
    });
}

}  // extern "C"
