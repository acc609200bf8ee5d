// pn2_emcad.hip — kernels of the EMCAD decoder (reference: /root/reference/multiclass_seg/EMCAD/lib/decoders.py, BASELINE config 5):
//   depth-wise k x k convs (k = 1, 3, 5) feeding BatchNorm      MSDC :83-99, EUCB.up_dwc :170-175
//   grouped 3x3 conv with 2 input channels per group            LGAG.W_g / W_x :193-200 (groups = F_int)
//   channel / pixel gates x * g                                  CAB :233-241 and SAB :252-258 used at EMCAD_dual.forward :442-443 ; LGAG :214
//   global average + max pooling, channel mean + max             CAB :234-237, SAB :253-255
//   nearest x2 up-sampling                                       EUCB :171
//   sum of the three MSDC branches written through channel_shuffle   MSCB.forward :147-154 with channel_shuffle :69-77
//   sum / concatenation of up to four branches, shuffled through LDS  the same step for the other decoder switches (add = False, four kernel sizes)
//   sigmoid on small fp32 maps                                   CAB / SAB / LGAG.psi
// All element-wise / memory-bound; BatchNorm statistics come out of the producing kernel as per-block partial rows, like the conv
// epilogue of pn2_conv.hip, so pn2_bn_finalize / pn2_affine_act / pn2_bn_bwd_* are reused unchanged.  Deterministic (no atomics).
#include "pn2_common.h"
#include "pn2_dw.h"
#include "../../include/pn2.h"

namespace {

template <typename T> __device__ __forceinline__ void ldv(const T* p, float* f) { TT<T>::unpack(*reinterpret_cast<const uint4*>(p), f); }
template <typename T> __device__ __forceinline__ void stv(T* p, const float* f) { *reinterpret_cast<uint4*>(p) = TT<T>::pack(f); }
using namespace pn2_host;
constexpr int GRID_CAP = 16384;

// rows (pixels) per block of the "thread owns a channel vector and walks pixels" kernels: at least four rows per row lane, no upper bound
inline void walk_geometry(int M, int CV, int& cvp, int& pix, int& nblk) { rows_walk_geometry(M, CV, 4, 0, cvp, pix, nblk); }

// cross-row-lane sum of per-thread channel-vector accumulators a[V] -> dst[c] (block partial row), through LDS, fixed order
template <int V>
__device__ __forceinline__ void block_colsum(float* sh, const float* a, int CVP, int R, int cvl, int rl, bool active, float* dst) {
#pragma unroll
    for (int e = 0; e < V; ++e) sh[(rl * CVP + cvl) * V + e] = a[e];
    __syncthreads();
    if (rl == 0 && active) {
#pragma unroll
        for (int e = 0; e < V; ++e) {
            float s = 0.f;
            for (int r = 0; r < R; ++r) s += sh[(r * CVP + cvl) * V + e];
            dst[e] = s;
        }
    }
    __syncthreads();
}

// ------------------------------------------------------------------------------------------ depth-wise K x K
// z[p][c] = sum_taps w[c][tap] x[p + tap][c]; optional per-block partial sums of z and z^2 (BatchNorm batch statistics).
// flip: mirrored kernel = data gradient.  Sliding window (as the 3x3 + GELU kernels of pn2_vit.hip): a thread owns VT channels, keeps their
// K*K weights and the K x K input window (packed) in registers and walks row segments of SEG output pixels - K new loads per output pixel
// instead of K*K.  A block = CVP channel groups x R lanes; a lane walks the segments bid*SPB + rl, + R, ... of the block's range.
template <typename T, int K, int VT>
__device__ __forceinline__ void dwk_load_col(const T* base, const bool (&vy)[K], int ix, int W, int C, DwVec<T, VT> (&col)[K]) {
#pragma unroll
    for (int r = 0; r < K; ++r) {
        col[r].zero();
        if (vy[r] && (unsigned)ix < (unsigned)W) col[r].load(base + ((ptrdiff_t)(r - K / 2) * W + ix) * C);
    }
}

template <typename T, int K, int VT>
__global__ __launch_bounds__(256) void dwconv_row_k(const T* __restrict__ x, const float* __restrict__ w, T* __restrict__ z, int N, int H, int W, int C, int flip, int accumulate,
                                                    float* __restrict__ psum, float* __restrict__ psq, int SEG, int SPR, int SPB, int CVP) {
    typedef DwVec<T, VT> Vec;
    constexpr int KK = K * K, PD = K / 2;
    extern __shared__ float sh[];
    const int CV = C / VT, R = 256 / CVP, cvl = threadIdx.x % CVP, rl = threadIdx.x / CVP;
    const int bid = xcd_remap(blockIdx.x, gridDim.x), cv = blockIdx.y * CVP + cvl;
    const bool act = cv < CV;
    const int nseg = N * H * SPR;
    float wr[KK][VT], s1[VT], s2[VT];
#pragma unroll
    for (int e = 0; e < VT; ++e) {
        s1[e] = 0.f; s2[e] = 0.f;
#pragma unroll
        for (int t = 0; t < KK; ++t) wr[t][e] = act ? w[(size_t)(cv * VT + e) * KK + (flip ? KK - 1 - t : t)] : 0.f;
    }
    if (act) {
        const int send = min(nseg, (bid + 1) * SPB);
        for (int s = bid * SPB + rl; s < send; s += R) {
            const int sx = s % SPR, row = s / SPR, oy = row % H;
            const int x0 = sx * SEG, x1 = min(W, x0 + SEG);
            bool vy[K];
#pragma unroll
            for (int r = 0; r < K; ++r) vy[r] = (unsigned)(oy + r - PD) < (unsigned)H;
            const T* base = x + ((size_t)row * W) * C + cv * VT;           // pixel (row, 0) of this channel group
            Vec win[K][K], nx[K];                                         // win[j] = column x0 - PD + j
#pragma unroll
            for (int j = 0; j < K; ++j) dwk_load_col<T, K, VT>(base, vy, x0 - PD + j, W, C, win[j]);
            for (int ox = x0; ox < x1; ++ox) {
                dwk_load_col<T, K, VT>(base, vy, ox + 1 < x1 ? ox + PD + 1 : -1, W, C, nx);     // the column the next pixel adds
                float a[VT], xv[VT];
#pragma unroll
                for (int e = 0; e < VT; ++e) a[e] = 0.f;
#pragma unroll
                for (int r = 0; r < K; ++r)
#pragma unroll
                    for (int j = 0; j < K; ++j) {
                        win[j][r].unpack(xv);
#pragma unroll
                        for (int e = 0; e < VT; ++e) a[e] += wr[r * K + j][e] * xv[e];
                    }
                const size_t o = ((size_t)row * W + ox) * C + cv * VT;
                Vec ov;
                if (accumulate) {
                    ov.load(z + o); ov.unpack(xv);
#pragma unroll
                    for (int e = 0; e < VT; ++e) a[e] += xv[e];
                }
                ov.pack(a); ov.store(z + o);
                if (psum) {       // statistics of the values as stored (rounded to T), like the conv epilogue
                    ov.unpack(xv);
#pragma unroll
                    for (int e = 0; e < VT; ++e) { s1[e] += xv[e]; s2[e] += xv[e] * xv[e]; }
                }
#pragma unroll
                for (int j = 0; j + 1 < K; ++j)
#pragma unroll
                    for (int r = 0; r < K; ++r) win[j][r] = win[j + 1][r];
#pragma unroll
                for (int r = 0; r < K; ++r) win[K - 1][r] = nx[r];
            }
        }
    }
    if (psum) {
        block_colsum<VT>(sh, s1, CVP, R, cvl, rl, act, psum + (size_t)bid * C + cv * VT);
        block_colsum<VT>(sh, s2, CVP, R, cvl, rl, act, psq + (size_t)bid * C + cv * VT);
    }
}

// partial[blk][C*K*K]: [c*KK + tap] = sum_pixels dz[p][c] * x[p + tap][c], same walk
template <typename T, int K, int VT>
__global__ __launch_bounds__(256) void dwconv_wgrad_row_k(const T* __restrict__ dz, const T* __restrict__ x, float* __restrict__ partial, int N, int H, int W, int C,
                                                          int SEG, int SPR, int SPB, int CVP) {
    typedef DwVec<T, VT> Vec;
    constexpr int KK = K * K, PD = K / 2;
    extern __shared__ float sh[];
    const int CV = C / VT, R = 256 / CVP, cvl = threadIdx.x % CVP, rl = threadIdx.x / CVP;
    const int bid = xcd_remap(blockIdx.x, gridDim.x), cv = blockIdx.y * CVP + cvl;
    const bool act = cv < CV;
    const int nseg = N * H * SPR;
    float a[KK][VT];
#pragma unroll
    for (int t = 0; t < KK; ++t)
#pragma unroll
        for (int e = 0; e < VT; ++e) a[t][e] = 0.f;
    if (act) {
        const int send = min(nseg, (bid + 1) * SPB);
        for (int s = bid * SPB + rl; s < send; s += R) {
            const int sx = s % SPR, row = s / SPR, oy = row % H;
            const int x0 = sx * SEG, x1 = min(W, x0 + SEG);
            bool vy[K];
#pragma unroll
            for (int r = 0; r < K; ++r) vy[r] = (unsigned)(oy + r - PD) < (unsigned)H;
            const size_t o0 = ((size_t)row * W) * C + cv * VT;
            const T* base = x + o0;
            Vec win[K][K], nx[K], dn;
#pragma unroll
            for (int j = 0; j < K; ++j) dwk_load_col<T, K, VT>(base, vy, x0 - PD + j, W, C, win[j]);
            dn.load(dz + o0 + (size_t)x0 * C);
            for (int ox = x0; ox < x1; ++ox) {
                const Vec dc = dn;
                dwk_load_col<T, K, VT>(base, vy, ox + 1 < x1 ? ox + PD + 1 : -1, W, C, nx);
                if (ox + 1 < x1) dn.load(dz + o0 + (size_t)(ox + 1) * C);
                float d[VT], xv[VT];
                dc.unpack(d);
#pragma unroll
                for (int r = 0; r < K; ++r)
#pragma unroll
                    for (int j = 0; j < K; ++j) {
                        win[j][r].unpack(xv);
#pragma unroll
                        for (int e = 0; e < VT; ++e) a[r * K + j][e] += d[e] * xv[e];
                    }
#pragma unroll
                for (int j = 0; j + 1 < K; ++j)
#pragma unroll
                    for (int r = 0; r < K; ++r) win[j][r] = win[j + 1][r];
#pragma unroll
                for (int r = 0; r < K; ++r) win[K - 1][r] = nx[r];
            }
        }
    }
#pragma unroll
    for (int t = 0; t < KK; ++t) {
        float tmp[VT];
        block_colsum<VT>(sh, a[t], CVP, R, cvl, rl, act, tmp);
        if (rl == 0 && act) {
#pragma unroll
            for (int e = 0; e < VT; ++e) partial[(size_t)bid * C * KK + (size_t)(cv * VT + e) * KK + t] = tmp[e];
        }
    }
}

// ------------------------------------------------------------------------------------------ grouped 3x3, two input channels per group
// z[p][o] = sum_{j<2, taps} w[o][j][tap] x[p + tap][2o + j]   (LGAG.W_g / W_x, decoders.py:193-200; the bias is folded by the caller).
// Sliding-window walks as the depth-wise kernels: a thread owns VT outputs (= one 16-byte vector of 2*VT inputs), keeps their 18*VT weights and
// the packed 3x3 input window in registers and walks a row segment.
template <typename T, int VT>
__device__ __forceinline__ void pc_load_col(const T* base, const bool (&vy)[3], int ix, int W, int ld, DwVec<T, 2 * VT> (&col)[3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        col[r].zero();
        if (vy[r] && (unsigned)ix < (unsigned)W) col[r].load(base + ((ptrdiff_t)(r - 1) * W + ix) * ld);
    }
}
template <typename T, int VT>
__device__ __forceinline__ void pc_load_col1(const T* base, const bool (&vy)[3], int ix, int W, int ld, DwVec<T, VT> (&col)[3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        col[r].zero();
        if (vy[r] && (unsigned)ix < (unsigned)W) col[r].load(base + ((ptrdiff_t)(r - 1) * W + ix) * ld);
    }
}

template <typename T, int VT>
__global__ __launch_bounds__(256) void pairconv_fwd_k(const T* __restrict__ x, const float* __restrict__ w, T* __restrict__ z, int N, int H, int W, int F,
                                                      float* __restrict__ psum, float* __restrict__ psq, int SEG, int SPR, int SPB, int CVP) {
    typedef DwVec<T, 2 * VT> VI; typedef DwVec<T, VT> VO;
    extern __shared__ float sh[];
    const int FV = F / VT, R = 256 / CVP, cvl = threadIdx.x % CVP, rl = threadIdx.x / CVP;
    const int bid = xcd_remap(blockIdx.x, gridDim.x), fv = blockIdx.y * CVP + cvl;
    const bool act = fv < FV;
    const int nseg = N * H * SPR;
    float wr[VT][18], s1[VT], s2[VT];
#pragma unroll
    for (int e = 0; e < VT; ++e) {
        s1[e] = 0.f; s2[e] = 0.f;
#pragma unroll
        for (int t = 0; t < 18; ++t) wr[e][t] = act ? w[(size_t)(fv * VT + e) * 18 + t] : 0.f;
    }
    if (act) {
        const int send = min(nseg, (bid + 1) * SPB);
        for (int s = bid * SPB + rl; s < send; s += R) {
            const int sx = s % SPR, row = s / SPR, oy = row % H;
            const int x0 = sx * SEG, x1 = min(W, x0 + SEG);
            bool vy[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) vy[r] = (unsigned)(oy + r - 1) < (unsigned)H;
            const T* base = x + ((size_t)row * W) * (2 * F) + fv * 2 * VT;
            VI c0[3], c1[3], c2[3], nx[3];
            pc_load_col<T, VT>(base, vy, x0 - 1, W, 2 * F, c0); pc_load_col<T, VT>(base, vy, x0, W, 2 * F, c1); pc_load_col<T, VT>(base, vy, x0 + 1, W, 2 * F, c2);
            for (int ox = x0; ox < x1; ++ox) {
                pc_load_col<T, VT>(base, vy, ox + 1 < x1 ? ox + 2 : -1, W, 2 * F, nx);
                float a[VT], xv[2 * VT];
#pragma unroll
                for (int e = 0; e < VT; ++e) a[e] = 0.f;
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    c0[r].unpack(xv);
#pragma unroll
                    for (int e = 0; e < VT; ++e) a[e] += wr[e][r * 3] * xv[2 * e] + wr[e][9 + r * 3] * xv[2 * e + 1];
                    c1[r].unpack(xv);
#pragma unroll
                    for (int e = 0; e < VT; ++e) a[e] += wr[e][r * 3 + 1] * xv[2 * e] + wr[e][9 + r * 3 + 1] * xv[2 * e + 1];
                    c2[r].unpack(xv);
#pragma unroll
                    for (int e = 0; e < VT; ++e) a[e] += wr[e][r * 3 + 2] * xv[2 * e] + wr[e][9 + r * 3 + 2] * xv[2 * e + 1];
                }
                VO ov; ov.pack(a); ov.store(z + ((size_t)row * W + ox) * F + fv * VT);
                ov.unpack(a);                     // statistics of the stored (rounded) values, like the conv epilogue
#pragma unroll
                for (int e = 0; e < VT; ++e) { s1[e] += a[e]; s2[e] += a[e] * a[e]; }
#pragma unroll
                for (int r = 0; r < 3; ++r) { c0[r] = c1[r]; c1[r] = c2[r]; c2[r] = nx[r]; }
            }
        }
    }
    block_colsum<VT>(sh, s1, CVP, R, cvl, rl, act, psum + (size_t)bid * F + fv * VT);
    block_colsum<VT>(sh, s2, CVP, R, cvl, rl, act, psq + (size_t)bid * F + fv * VT);
}

// dx[p][2o + j] (+)= sum_taps w[o][j][8 - tap] dz[p + tap][o]
template <typename T, int VT>
__global__ __launch_bounds__(256) void pairconv_dgrad_k(const T* __restrict__ dz, const float* __restrict__ w, T* __restrict__ dx, int N, int H, int W, int F, int accumulate,
                                                        int SEG, int SPR, int CVP) {
    typedef DwVec<T, 2 * VT> VI; typedef DwVec<T, VT> VO;
    const int FV = F / VT, R = 256 / CVP, cvl = threadIdx.x % CVP, rl = threadIdx.x / CVP;
    const int bid = xcd_remap(blockIdx.x, gridDim.x), fv = blockIdx.y * CVP + cvl;
    const int s = bid * R + rl;
    if (s >= N * H * SPR || fv >= FV) return;
    float wr[VT][18];
#pragma unroll
    for (int e = 0; e < VT; ++e)
#pragma unroll
        for (int t = 0; t < 18; ++t) wr[e][t] = w[(size_t)(fv * VT + e) * 18 + t];
    const int sx = s % SPR, row = s / SPR, oy = row % H;
    const int x0 = sx * SEG, x1 = min(W, x0 + SEG);
    bool vy[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) vy[r] = (unsigned)(oy + r - 1) < (unsigned)H;
    const T* base = dz + ((size_t)row * W) * F + fv * VT;
    VO c0[3], c1[3], c2[3], nx[3];
    pc_load_col1<T, VT>(base, vy, x0 - 1, W, F, c0); pc_load_col1<T, VT>(base, vy, x0, W, F, c1); pc_load_col1<T, VT>(base, vy, x0 + 1, W, F, c2);
    for (int ox = x0; ox < x1; ++ox) {
        pc_load_col1<T, VT>(base, vy, ox + 1 < x1 ? ox + 2 : -1, W, F, nx);
        float a[2 * VT], d[VT];
#pragma unroll
        for (int e = 0; e < 2 * VT; ++e) a[e] = 0.f;
#pragma unroll
        for (int r = 0; r < 3; ++r) {          // tap t = r*3 + j uses the mirrored weight 8 - t
            c0[r].unpack(d);
#pragma unroll
            for (int e = 0; e < VT; ++e) { a[2 * e] += wr[e][8 - r * 3] * d[e]; a[2 * e + 1] += wr[e][17 - r * 3] * d[e]; }
            c1[r].unpack(d);
#pragma unroll
            for (int e = 0; e < VT; ++e) { a[2 * e] += wr[e][7 - r * 3] * d[e]; a[2 * e + 1] += wr[e][16 - r * 3] * d[e]; }
            c2[r].unpack(d);
#pragma unroll
            for (int e = 0; e < VT; ++e) { a[2 * e] += wr[e][6 - r * 3] * d[e]; a[2 * e + 1] += wr[e][15 - r * 3] * d[e]; }
        }
        T* dp = dx + ((size_t)row * W + ox) * (2 * F) + fv * 2 * VT;
        VI ov;
        if (accumulate) {
            float o[2 * VT];
            ov.load(dp); ov.unpack(o);
#pragma unroll
            for (int e = 0; e < 2 * VT; ++e) a[e] += o[e];
        }
        ov.pack(a); ov.store(dp);
#pragma unroll
        for (int r = 0; r < 3; ++r) { c0[r] = c1[r]; c1[r] = c2[r]; c2[r] = nx[r]; }
    }
}

// partial[blk][F*18]: [o*18 + j*9 + tap] = sum_pixels dz[p][o] * x[p + tap][2o + j]
template <typename T, int VT>
__global__ __launch_bounds__(256) void pairconv_wgrad_k(const T* __restrict__ dz, const T* __restrict__ x, float* __restrict__ partial, int N, int H, int W, int F,
                                                        int SEG, int SPR, int SPB, int CVP) {
    typedef DwVec<T, 2 * VT> VI; typedef DwVec<T, VT> VO;
    extern __shared__ float sh[];
    const int FV = F / VT, R = 256 / CVP, cvl = threadIdx.x % CVP, rl = threadIdx.x / CVP;
    const int bid = xcd_remap(blockIdx.x, gridDim.x), fv = blockIdx.y * CVP + cvl;
    const bool act = fv < FV;
    const int nseg = N * H * SPR;
    float a[18][VT];
#pragma unroll
    for (int t = 0; t < 18; ++t)
#pragma unroll
        for (int e = 0; e < VT; ++e) a[t][e] = 0.f;
    if (act) {
        const int send = min(nseg, (bid + 1) * SPB);
        for (int s = bid * SPB + rl; s < send; s += R) {
            const int sx = s % SPR, row = s / SPR, oy = row % H;
            const int x0 = sx * SEG, x1 = min(W, x0 + SEG);
            bool vy[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) vy[r] = (unsigned)(oy + r - 1) < (unsigned)H;
            const T* base = x + ((size_t)row * W) * (2 * F) + fv * 2 * VT;
            const T* dbase = dz + ((size_t)row * W) * F + fv * VT;
            VI c0[3], c1[3], c2[3], nx[3]; VO dn;
            pc_load_col<T, VT>(base, vy, x0 - 1, W, 2 * F, c0); pc_load_col<T, VT>(base, vy, x0, W, 2 * F, c1); pc_load_col<T, VT>(base, vy, x0 + 1, W, 2 * F, c2);
            dn.load(dbase + (size_t)x0 * F);
            for (int ox = x0; ox < x1; ++ox) {
                const VO dc = dn;
                pc_load_col<T, VT>(base, vy, ox + 1 < x1 ? ox + 2 : -1, W, 2 * F, nx);
                if (ox + 1 < x1) dn.load(dbase + (size_t)(ox + 1) * F);
                float d[VT], xv[2 * VT];
                dc.unpack(d);
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    c0[r].unpack(xv);
#pragma unroll
                    for (int e = 0; e < VT; ++e) { a[r * 3][e] += d[e] * xv[2 * e]; a[9 + r * 3][e] += d[e] * xv[2 * e + 1]; }
                    c1[r].unpack(xv);
#pragma unroll
                    for (int e = 0; e < VT; ++e) { a[r * 3 + 1][e] += d[e] * xv[2 * e]; a[9 + r * 3 + 1][e] += d[e] * xv[2 * e + 1]; }
                    c2[r].unpack(xv);
#pragma unroll
                    for (int e = 0; e < VT; ++e) { a[r * 3 + 2][e] += d[e] * xv[2 * e]; a[9 + r * 3 + 2][e] += d[e] * xv[2 * e + 1]; }
                }
#pragma unroll
                for (int r = 0; r < 3; ++r) { c0[r] = c1[r]; c1[r] = c2[r]; c2[r] = nx[r]; }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 18; ++t) {
        float tmp[VT];
        block_colsum<VT>(sh, a[t], CVP, R, cvl, rl, act, tmp);
        if (rl == 0 && act) {
#pragma unroll
            for (int e = 0; e < VT; ++e) partial[(size_t)bid * F * 18 + (size_t)(fv * VT + e) * 18 + t] = tmp[e];
        }
    }
}

// ------------------------------------------------------------------------------------------ gates
// mode 0: y[n][p][c] = x * g[n][c]   (channel gate, CAB) ; mode 1: y = x * g[n][p]   (pixel gate, SAB / LGAG.psi)
template <typename T>
__global__ __launch_bounds__(256) void gate_mul_k(const T* __restrict__ x, const float* __restrict__ g, T* __restrict__ y, int N, int HW, int C, int mode, int accumulate) {
    constexpr int V = TT<T>::VEC;
    const int CV = C / V;
    const size_t total = (size_t)N * HW * CV;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        int cv, pp_; const size_t p = divmod_idx(idx, CV, cv); const int n = (int)divmod_idx(p, HW, pp_);
        float v[V], o[V];
        ldv<T>(x + p * C + cv * V, v);
        if (accumulate) ldv<T>(y + p * C + cv * V, o);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const float t = v[e] * (mode ? g[p] : g[(size_t)n * C + cv * V + e]);
            o[e] = accumulate ? o[e] + t : t;
        }
        stv<T>(y + p * C + cv * V, o);
    }
}

// pixel gate gradient: dg[n][p] = sum_c dy * x   (one 8/16-lane group per pixel)
template <typename T>
__global__ __launch_bounds__(256) void gate_dpix_k(const T* __restrict__ dy, const T* __restrict__ x, float* __restrict__ dg, size_t NP, int C) {
    constexpr int V = TT<T>::VEC;
    const int CV = C / V;
    const int lane = threadIdx.x & 63;
    const size_t wave = ((size_t)blockIdx.x * 256 + threadIdx.x) >> 6, nw = ((size_t)gridDim.x * 256) >> 6;
    for (size_t p = wave; p < NP; p += nw) {
        float s = 0.f;
        for (int cv = lane; cv < CV; cv += 64) {
            float a[V], b[V];
            ldv<T>(dy + p * C + cv * V, a); ldv<T>(x + p * C + cv * V, b);
#pragma unroll
            for (int e = 0; e < V; ++e) s += a[e] * b[e];
        }
        s = wave_sum(s);
        if (lane == 0) dg[p] = s;
    }
}

// channel gate gradient partials: part[blk][n*C + c] = sum over the block's pixels of sample n of dy * x   (grid: blocks x N)
template <typename T>
__global__ __launch_bounds__(256) void gate_dchan_k(const T* __restrict__ dy, const T* __restrict__ x, float* __restrict__ part, int N, int HW, int C, int pix_per_blk, int CVP) {
    constexpr int V = TT<T>::VEC;
    extern __shared__ float sh[];
    const int CV = C / V, R = 256 / CVP, cvl = threadIdx.x % CVP, rl = threadIdx.x / CVP, n = blockIdx.y;
    const int p0 = blockIdx.x * pix_per_blk;
    int p1 = p0 + pix_per_blk; if (p1 > HW) p1 = HW;
    for (int cvb = 0; cvb < CV; cvb += CVP) {
        const int cv = cvb + cvl;
        const bool act = cv < CV;
        float a[V];
#pragma unroll
        for (int e = 0; e < V; ++e) a[e] = 0.f;
        if (act) {
            for (int m = p0 + rl; m < p1; m += R) {
                float d[V], xv[V];
                const size_t o = ((size_t)n * HW + m) * C + cv * V;
                ldv<T>(dy + o, d); ldv<T>(x + o, xv);
#pragma unroll
                for (int e = 0; e < V; ++e) a[e] += d[e] * xv[e];
            }
        }
        block_colsum<V>(sh, a, CVP, R, cvl, rl, act, part + (size_t)blockIdx.x * N * C + (size_t)n * C + cv * V);
    }
}

// ------------------------------------------------------------------------------------------ global avg + max pooling (CAB)
// one block per (n, channel-vector chunk): avg[n][c], mx[n][c] (compute dtype, rows of an [N][1][1][C] map) and the argmax pixel
template <typename T>
__global__ __launch_bounds__(256) void global_pool_k(const T* __restrict__ x, T* __restrict__ avg, T* __restrict__ mx, int* __restrict__ arg, int HW, int C) {
    constexpr int V = TT<T>::VEC;
    __shared__ float ssum[32][8]; __shared__ float smax[32][8]; __shared__ int sarg[32][8];
    const int CV = C / V, n = blockIdx.y;
    const int cvl = threadIdx.x % 8, rl = threadIdx.x / 8, cv = blockIdx.x * 8 + cvl;      // 8 channel vectors x 32 row lanes
    float s[V], m[V]; int am[V];
#pragma unroll
    for (int e = 0; e < V; ++e) { s[e] = 0.f; m[e] = -INFINITY; am[e] = 0; }
    if (cv < CV) {
        for (int p = rl; p < HW; p += 32) {
            float v[V];
            ldv<T>(x + ((size_t)n * HW + p) * C + cv * V, v);
#pragma unroll
            for (int e = 0; e < V; ++e) { s[e] += v[e]; if (v[e] > m[e]) { m[e] = v[e]; am[e] = p; } }
        }
    }
    // reduce the 32 row lanes per channel (sequential in lane order: first maximum wins, as torch's max pooling does)
#pragma unroll
    for (int e = 0; e < V; ++e) {
        ssum[rl][cvl] = s[e]; smax[rl][cvl] = m[e]; sarg[rl][cvl] = am[e];
        __syncthreads();
        if (rl == 0 && cv < CV) {
            float ts = 0.f, tm = -INFINITY; int ta = 0;
            for (int r = 0; r < 32; ++r) {
                ts += ssum[r][cvl];
                if (smax[r][cvl] > tm || (smax[r][cvl] == tm && sarg[r][cvl] < ta)) { tm = smax[r][cvl]; ta = sarg[r][cvl]; }
            }
            const int c = cv * V + e;
            TT<T>::st(avg + (size_t)n * C + c, ts / (float)HW);
            TT<T>::st(mx + (size_t)n * C + c, tm);
            arg[(size_t)n * C + c] = ta;
        }
        __syncthreads();
    }
}

// dx[n][p][c] (+)= davg[n][c] / HW + (p == arg[n][c]) * dmax[n][c]
template <typename T>
__global__ __launch_bounds__(256) void global_pool_bwd_k(const T* __restrict__ davg, const T* __restrict__ dmax, const int* __restrict__ arg, T* __restrict__ dx,
                                                         int N, int HW, int C, int accumulate) {
    const size_t total = (size_t)N * HW * C;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        int c, pp; const size_t p = divmod_idx(idx, C, c); const int n = (int)divmod_idx(p, HW, pp);
        float v = TT<T>::ld(davg + (size_t)n * C + c) / (float)HW;
        if (arg[(size_t)n * C + c] == pp) v += TT<T>::ld(dmax + (size_t)n * C + c);
        if (accumulate) v += TT<T>::ld(dx + idx);
        TT<T>::st(dx + idx, v);
    }
}

// ------------------------------------------------------------------------------------------ channel mean + max per pixel (SAB)
// out[p][0] = mean_c x, out[p][1] = max_c x, out[p][2..7] = 0 ; arg[p] = first channel attaining the max
template <typename T>
__global__ __launch_bounds__(256) void chan_stats_k(const T* __restrict__ x, T* __restrict__ out, int* __restrict__ arg, size_t NP, int C) {
    const int lane = threadIdx.x & 63;
    const size_t wave = ((size_t)blockIdx.x * 256 + threadIdx.x) >> 6, nw = ((size_t)gridDim.x * 256) >> 6;
    for (size_t p = wave; p < NP; p += nw) {
        float s = 0.f, m = -INFINITY; int am = 0x7fffffff;
        for (int c = lane; c < C; c += 64) {
            const float v = TT<T>::ld(x + p * C + c);
            s += v;
            if (v > m) { m = v; am = c; }
        }
        s = wave_sum(s);
        for (int o = 32; o > 0; o >>= 1) {
            const float om = __shfl_xor(m, o); const int oa = __shfl_xor(am, o);
            if (om > m || (om == m && oa < am)) { m = om; am = oa; }
        }
        if (lane < 8) TT<T>::st(out + p * 8 + lane, lane == 0 ? s / (float)C : (lane == 1 ? m : 0.f));
        if (lane == 0) arg[p] = am;
    }
}

// dx[p][c] (+)= dout[p][0] / C + (c == arg[p]) * dout[p][1]
template <typename T>
__global__ __launch_bounds__(256) void chan_stats_bwd_k(const T* __restrict__ dout, const int* __restrict__ arg, T* __restrict__ dx, size_t NP, int C, int accumulate) {
    const size_t total = NP * C;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        int c; const size_t p = divmod_idx(idx, C, c);
        float v = TT<T>::ld(dout + p * 8) / (float)C;
        if (arg[p] == c) v += TT<T>::ld(dout + p * 8 + 1);
        if (accumulate) v += TT<T>::ld(dx + idx);
        TT<T>::st(dx + idx, v);
    }
}

// ------------------------------------------------------------------------------------------ nearest x2
template <typename T>
__global__ __launch_bounds__(256) void up2_k(const T* __restrict__ x, T* __restrict__ y, int N, int H, int W, int C) {
    constexpr int V = TT<T>::VEC;
    const int CV = C / V, OH = 2 * H, OW = 2 * W;
    const size_t total = (size_t)N * OH * OW * CV;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        int cv, ox, oy; size_t p = divmod_idx(idx, CV, cv);
        p = divmod_idx(p, OW, ox); const int n = (int)divmod_idx(p, OH, oy);
        *reinterpret_cast<uint4*>(y + (((size_t)n * OH + oy) * OW + ox) * C + cv * V) =
            *reinterpret_cast<const uint4*>(x + (((size_t)n * H + (oy >> 1)) * W + (ox >> 1)) * C + cv * V);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void up2_bwd_k(const T* __restrict__ dy, T* __restrict__ dx, int N, int H, int W, int C, int accumulate) {
    constexpr int V = TT<T>::VEC;
    const int CV = C / V, OW = 2 * W;
    const size_t total = (size_t)N * H * W * CV;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        int cv, ix, iy; size_t p = divmod_idx(idx, CV, cv);
        p = divmod_idx(p, W, ix); const int n = (int)divmod_idx(p, H, iy);
        float a[V], b[V];
        const T* base = dy + (((size_t)n * 2 * H + 2 * iy) * OW + 2 * ix) * C + cv * V;
        ldv<T>(base, a);
        ldv<T>(base + C, b);
#pragma unroll
        for (int e = 0; e < V; ++e) a[e] += b[e];
        ldv<T>(base + (size_t)OW * C, b);
#pragma unroll
        for (int e = 0; e < V; ++e) a[e] += b[e];
        ldv<T>(base + (size_t)OW * C + C, b);
#pragma unroll
        for (int e = 0; e < V; ++e) a[e] += b[e];
        T* d = dx + (((size_t)n * H + iy) * W + ix) * C + cv * V;
        if (accumulate) { ldv<T>(d, b);
#pragma unroll
            for (int e = 0; e < V; ++e) a[e] += b[e]; }
        stv<T>(d, a);
    }
}

// ------------------------------------------------------------------------------------------ sum of up to 3 tensors through a channel permutation
// y[p][c] = a[p][perm[c]] (+ b[p][perm[c]] + c3[p][perm[c]])     (MSCB: dout = channel_shuffle(sum of the MSDC branches); backward: one gather)
template <typename T>
__global__ __launch_bounds__(256) void gather_sum_k(const T* __restrict__ a, const T* __restrict__ b, const T* __restrict__ c3, const int* __restrict__ perm,
                                                    T* __restrict__ y, size_t M, int C) {
    const size_t total = M * C;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        int c; const size_t p = divmod_idx(idx, C, c);
        const size_t s = p * C + perm[c];
        float v = TT<T>::ld(a + s);
        if (b) v += TT<T>::ld(b + s);
        if (c3) v += TT<T>::ld(c3 + s);
        TT<T>::st(y + idx, v);
    }
}

// ------------------------------------------------------------------------------------------ MSDC combine: sum / concatenation of up to 4 branches through channel_shuffle
// y[p][j] = in[p][src(j)], src(j) = (j % groups) * cpg + j / groups, cpg = Cw / groups: per pixel the [groups][cpg] matrix `in` is written as its transpose.
//   MC_SUM    in = ((p0 + p1) + p2) + p3 in fp32, rounded once (Cw = Cpart)          MC_CAT   in = cat(p0 .. p3) (Cw = n * Cpart), a move
//   MC_SPLIT  in = one tensor of width Cw, y = cat(out0 .. out3), each out (+)= its slice: the adjoint of MC_CAT when launched with groups' = cpg
// A block owns TP pixels x the whole row.  Phase 1: 16-byte global loads, the sum, and a scalar scatter into LDS IN OUTPUT ORDER; phase 2: ds_read_b128 of
// consecutive output channels and 16-byte global stores.  LDS row of a pixel = cpg transposed rows of `groups` elements; where that pitch is a multiple of
// 128 bytes (all 32 banks of a store) every transposed row starts on bank 0 and the lanes of a scatter store, which differ in their transposed row, pile up
// on one bank - each row is then padded by 16 bytes (4 banks; a multiple of the vector, so phase 2 stays aligned).  Other pitches are left linear.
enum { MC_SUM = 0, MC_CAT = 1, MC_SPLIT = 2 };
constexpr int MC_MAX_CW = 16384, MC_TILE_BYTES = 16384, MC_MAX_TP = 256;
struct McArgs { const void* in[4]; void* out[4]; int acc[4]; };
template <typename T> struct McRaw { typedef unsigned short type; };
template <> struct McRaw<float> { typedef unsigned type; };
__device__ __forceinline__ void mc_unpack(const uint4& q, unsigned short* r) {
    r[0] = (unsigned short)q.x; r[1] = (unsigned short)(q.x >> 16); r[2] = (unsigned short)q.y; r[3] = (unsigned short)(q.y >> 16);
    r[4] = (unsigned short)q.z; r[5] = (unsigned short)(q.z >> 16); r[6] = (unsigned short)q.w; r[7] = (unsigned short)(q.w >> 16);
}
__device__ __forceinline__ void mc_unpack(const uint4& q, unsigned* r) { r[0] = q.x; r[1] = q.y; r[2] = q.z; r[3] = q.w; }
template <typename P> __device__ __forceinline__ P mc_pick(P const (&a)[4], int i) { return i == 0 ? a[0] : i == 1 ? a[1] : i == 2 ? a[2] : a[3]; }

template <typename T, int MODE>
__global__ __launch_bounds__(256) void msdc_combine_k(McArgs A, int n, size_t M, int Cpart, int Cw, int groups, int padE, int TP) {
    typedef typename McRaw<T>::type R;
    constexpr int V = TT<T>::VEC;
    extern __shared__ uint4 mc_sh[];
    R* sh = reinterpret_cast<R*>(mc_sh);
    const int cpg = Cw / groups, CV = Cw / V, pitch = groups + padE, rowE = cpg * pitch;
    const size_t p0 = (size_t)blockIdx.x * TP;
    const int nvec = (int)min((size_t)TP, M - p0) * CV;
    for (int v = threadIdx.x; v < nvec; v += 256) {
        const int pl = v / CV, s = (v - pl * CV) * V;
        const size_t p = p0 + pl;
        uint4 q;
        if (MODE == MC_SUM && n > 1) {
            float a[V], b[V];
            ldv<T>((const T*)A.in[0] + p * Cw + s, a);
            ldv<T>((const T*)A.in[1] + p * Cw + s, b);
#pragma unroll
            for (int e = 0; e < V; ++e) a[e] += b[e];
            if (n > 2) { ldv<T>((const T*)A.in[2] + p * Cw + s, b);
#pragma unroll
                for (int e = 0; e < V; ++e) a[e] += b[e]; }
            if (n > 3) { ldv<T>((const T*)A.in[3] + p * Cw + s, b);
#pragma unroll
                for (int e = 0; e < V; ++e) a[e] += b[e]; }
            q = TT<T>::pack(a);
        } else if (MODE == MC_CAT) {
            const int i = s / Cpart;          // Cpart is a multiple of V: a vector lies in one part
            q = *reinterpret_cast<const uint4*>((const T*)mc_pick(A.in, i) + p * Cpart + (s - i * Cpart));
        } else {
            q = *reinterpret_cast<const uint4*>((const T*)A.in[0] + p * Cw + s);
        }
        R r[V];
        mc_unpack(q, r);
        R* row = sh + pl * rowE;
        int a = s % cpg, g = s / cpg;          // source channel s = g * cpg + a goes to output channel a * groups + g
#pragma unroll
        for (int e = 0; e < V; ++e) {
            row[a * pitch + g] = r[e];
            if (++a == cpg) { a = 0; ++g; }
        }
    }
    __syncthreads();
    for (int v = threadIdx.x; v < nvec; v += 256) {
        const int pl = v / CV, j = (v - pl * CV) * V;
        const size_t p = p0 + pl;
        const uint4 q = *reinterpret_cast<const uint4*>(sh + pl * rowE + (padE ? j + (j / groups) * padE : j));      // padE > 0 only where groups % V == 0
        if (MODE != MC_SPLIT) {
            *reinterpret_cast<uint4*>((T*)A.out[0] + p * Cw + j) = q;
        } else {
            const int i = j / Cpart;
            T* d = (T*)mc_pick(A.out, i) + p * Cpart + (j - i * Cpart);
            if (mc_pick(A.acc, i)) {
                float x[V], o[V];
                TT<T>::unpack(q, x);
                ldv<T>(d, o);
#pragma unroll
                for (int e = 0; e < V; ++e) o[e] += x[e];
                stv<T>(d, o);
            } else {
                *reinterpret_cast<uint4*>(d) = q;
            }
        }
    }
}

/* tile of msdc_combine_k for rows of Cw channels shuffled in `groups`: row padding (elements), pixels per block, LDS bytes; -2 = not built */
inline int mc_geometry(int dt, int Cw, int groups, int& padE, int& TP, size_t& lds) {
    const int V = vec_of(dt), sz = 16 / V;
    if (Cw < V || Cw % V || Cw > MC_MAX_CW || groups < 1 || Cw % groups) return -2;
    const int cpg = Cw / groups;
    padE = (cpg > 1 && ((size_t)groups * sz) % 128 == 0) ? V : 0;
    size_t row = (size_t)(Cw + cpg * padE) * sz;
    if (row > 64 * 1024) { padE = 0; row = (size_t)Cw * sz; }          // (fp32 rows of 16384 channels: exactly the default LDS, unpadded)
    const size_t tp = MC_TILE_BYTES / row;
    TP = tp < 1 ? 1 : (tp > (size_t)MC_MAX_TP ? MC_MAX_TP : (int)tp);
    lds = (size_t)TP * row;
    return 0;
}
template <int MODE>
inline int mc_launch(int dt, const McArgs& A, int n, long long M, int Cpart, int Cw, int groups, void* stream) {
    int padE, TP; size_t lds;
    if (mc_geometry(dt, Cw, groups, padE, TP, lds)) return -2;
    const long long nblk = (M + TP - 1) / TP;
    if (nblk > 0x7fffffffLL) return -2;
    return with_storage_dtype(dt, [&](auto ty) {
        using T = type_of<decltype(ty)>;
        return pn2_launch<msdc_combine_k<T, MODE>>(dim3((unsigned)nblk), dim3(256), lds, 0, (hipStream_t)stream, A, n, (size_t)M, Cpart, Cw, groups, padE, TP);
    });
}

// ------------------------------------------------------------------------------------------ sigmoid on small maps
template <typename Ti>
__global__ __launch_bounds__(256) void sigmoid_k(const Ti* __restrict__ x, float* __restrict__ y, size_t n, int ld, int C) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float v = TT<Ti>::ld(x + (i / C) * ld + i % C);
        y[i] = 1.f / (1.f + expf(-v));
    }
}
template <typename To>
__global__ __launch_bounds__(256) void sigmoid_bwd_k(const float* __restrict__ dy, const float* __restrict__ y, To* __restrict__ dx, size_t n, int ld, int C, int accumulate) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        To* d = dx + (i / C) * ld + i % C;
        const float g = dy[i] * y[i] * (1.f - y[i]);
        TT<To>::st(d, accumulate ? TT<To>::ld(d) + g : g);
    }
}

// ------------------------------------------------------------------------------------------ multi-class "mutation" loss (config 5)
// EMCAD/trainer.py:106-140 (dual, supervision='mutation') with utils/utils.py:102-138 (DiceLoss, softmax=True):
//   loss = sum over the 15 non-empty subsets s of the 4 scales of
//          lc1 * CE(sum_{i in s} fg_i, label) + lc2 * Dice(softmax(sum fg_i), onehot(label)) + lc3 * BCEWithLogits(sum_{i in s} bg_i, bg_mask)
// (hardware exp2 / log2 / rcp: the kernels are ALU-bound - ~300 transcendentals per pixel - and the sums are means over >= 10^6 terms)
// One pass over the 8 K-channel maps (NHWC fp32): a thread keeps its pixel's 8*K logits in registers and walks the 15 subsets; the per-subset
// sums (CE, BCE, per-class intersect and sum p^2) are reduced per wave and written as partial rows.  The backward recomputes the softmaxes.
constexpr int ML_NS = 15;
// row layouts of `partial` / `sums`: W values per subset, then the label histogram T[K]
template <int K> struct MLW { static constexpr int W = 2 + 2 * K, NV = ML_NS * W + K; };      // dual: CE, BCE, I[K], Z[K]
template <int K> struct SLW { static constexpr int W = 1 + 2 * K, NV = ML_NS * W + K; };      // single supervision: CE, I[K], Z[K]

// ---- the softmax CE + Dice core of one subset at one pixel, shared by the dual (mloss_*) and the single-supervision (sloss_*) kernels.  z: the subset's summed logits
// mx = max_k z[k], e[k] = exp(z[k] - mx); returns sum_k e[k]
template <int K>
__device__ __forceinline__ float exp_shifted(const float (&z)[K], float (&e)[K], float& mx) {
    mx = z[0];
#pragma unroll
    for (int k = 1; k < K; ++k) mx = fmaxf(mx, z[k]);
    float se = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) { e[k] = __expf(z[k] - mx); se += e[k]; }
    return se;
}

// forward: returns CE at the label; I[k] = p_k at the label (else 0), Z[k] = p_k^2
template <int K>
__device__ __forceinline__ float ce_dice_fwd(const float (&z)[K], int lab, float* I, float* Z) {
    float mx, e[K];
    const float se = exp_shifted<K>(z, e, mx);
    const float inv = __builtin_amdgcn_rcpf(se), lse = mx + __logf(se);
    float ce = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float pk = e[k] * inv;
        if (lab == k) ce = lse - z[k];
        I[k] = (lab == k) ? pk : 0.f;
        Z[k] = pk * pk;
    }
    return ce;
}

// the Dice coefficients of every (subset, class) - uniform over the pixels - once per block in LDS (as 270 global loads per thread the compiler hoisted them all
// to the top of a fully unrolled subset loop: 256 + 256 registers and scratch).  W: values per subset of `sums`, oI: column of I[0] (Z follows I); the caller syncs
template <int K>
__device__ __forceinline__ void dice_coef(const float* __restrict__ sums, int W, int oI, float wdice, float* tA, float* tB) {
    for (int j = threadIdx.x; j < ML_NS * K; j += 256) {
        const int s0 = j / K, k = j - s0 * K;
        const float* S = sums + s0 * W + oI;
        // d dice_k / d p_k = -(2 t / D - (2 I + eps) 2 p / D^2),  D = Z + T + eps
        const float D = S[K + k] + sums[ML_NS * W + k] + 1e-5f;
        tA[j] = wdice * 2.f / D; tB[j] = wdice * (2.f * S[k] + 1e-5f) * 2.f / (D * D);
    }
}

// backward, per class: d Dice / d p_k from the subset's Dice coefficients (a: tA at the label, else 0; b: tB), then dz_k = d(wce * CE + Dice) / d z_k through the
// softmax Jacobian (dot = sum_k g_k p_k).  The loop over the classes stays in the kernels: with its conditional LDS reads inside a helper the compiler contracts
// other multiply-adds and the kernels take 2 - 12 registers more
__device__ __forceinline__ float dice_dp(float a, float b, float p) { return -(a - b * p); }
__device__ __forceinline__ float ce_dice_dz(float p, bool hit, float g, float dot, float wce) { return wce * (p - (hit ? 1.f : 0.f)) + p * (g - dot); }

// group rows -> sh[NV] (double) and sums[NV], by the finalize kernels' one block; the caller syncs
__device__ __forceinline__ void group_sums(const double* __restrict__ grp, int ngrp, int NV, double* sh, float* __restrict__ sums) {
    for (int j = threadIdx.x; j < NV; j += blockDim.x) {
        double a = 0.0;
        for (int r = 0; r < ngrp; ++r) a += grp[(size_t)r * NV + j];
        sh[j] = a; sums[j] = (float)a;
    }
}
// sum over the classes of the Dice loss of one subset; oI, oZ: the subset's columns of sh, oT: the label histogram's
__device__ __forceinline__ double dice_sum(const double* sh, int K, int oI, int oZ, int oT) {
    double dice = 0.0;
    for (int k = 0; k < K; ++k) dice += 1.0 - (2.0 * sh[oI + k] + 1e-5) / (sh[oZ + k] + sh[oT + k] + 1e-5);
    return dice;
}

struct ml_maps { const float* fg[4]; const float* bg[4]; float* dfg[4]; float* dbg[4]; };

template <int K>
__global__ __launch_bounds__(256) void mloss_fwd_k(ml_maps m, const long long* __restrict__ label, const float* __restrict__ bgm, size_t NP, size_t HW,
                                                   float* __restrict__ partial) {
    constexpr int W = MLW<K>::W;
    // per-value sums stop at the 16-lane rows (DPP adds only); the 16 row partials of the block meet in LDS.  A full 64-lane butterfly per value
    // needs two LDS permutes each, and with ~300 values per pixel their latency was most of this kernel.
    __shared__ float red[16][ML_NS * W + K];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, rrow = wid * 4 + (lane >> 4);
    const bool rlead = (lane & 15) == 0;
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool ok = p < NP;
    // Round 6: foreground (softmax-coupled: CE, Dice sums) and background (BCE: every class on its own) parts apart, as in the backward - the background part runs
    // class by class with four logits and fifteen running sums live (205 -> ~110 registers, two -> four waves per SIMD); same sums, same order, bit for bit
    float f[4][K];
    int lab = -1;
    const size_t n = ok ? p / HW : 0, hw = ok ? p % HW : 0;
    if (ok) {
        lab = (int)label[p];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int k = 0; k < K; ++k) f[i][k] = m.fg[i][p * K + k];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {          // label histogram (sum of target^2 per class), once
        float t = (ok && lab == k) ? 1.f : 0.f;
        t = row16_sum(t);
        if (rlead) red[rrow][ML_NS * W + k] = t;
    }
#pragma unroll
    for (int s = 1; s <= ML_NS; ++s) {
        float z[K], v[W];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            z[k] = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) if (s >> i & 1) z[k] += f[i][k];
        }
        v[0] = ce_dice_fwd<K>(z, lab, v + 2, v + 2 + K); v[1] = 0.f;
#pragma unroll
        for (int j = 0; j < W; ++j) if (j != 1) v[j] = row16_sum(ok ? v[j] : 0.f);
        if (rlead) {
#pragma unroll
            for (int j = 0; j < W; ++j) if (j != 1) red[rrow][(s - 1) * W + j] = v[j];
        }
    }
    {
        float bce[ML_NS];
#pragma unroll
        for (int s = 0; s < ML_NS; ++s) bce[s] = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            float b[4] = {0.f, 0.f, 0.f, 0.f}, mk = 0.f;
            if (ok) {
#pragma unroll
                for (int i = 0; i < 4; ++i) b[i] = m.bg[i][p * K + k];
                mk = bgm[(n * K + k) * HW + hw];
            }
#pragma unroll
            for (int s = 1; s <= ML_NS; ++s) {
                float zb = 0.f;
#pragma unroll
                for (int i = 0; i < 4; ++i) if (s >> i & 1) zb += b[i];
                bce[s - 1] += fmaxf(zb, 0.f) - zb * mk + __logf(1.f + __expf(-fabsf(zb)));
            }
        }
#pragma unroll
        for (int s = 0; s < ML_NS; ++s) {
            const float t = row16_sum(ok ? bce[s] : 0.f);
            if (rlead) red[rrow][s * W + 1] = t;
        }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < ML_NS * W + K; j += 256) {
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) t += red[i][j];
        partial[(size_t)blockIdx.x * (ML_NS * W + K) + j] = t;
    }
}

// partial rows of either loss -> up to ML_RG group rows in double (every group sums a contiguous range of block rows, 4 independent chains per thread; the row
// width comes at run time: not hot)
constexpr int ML_RG = 128;
__global__ __launch_bounds__(256) void loss_reduce_k(const float* __restrict__ partial, int nblk, int NV, double* __restrict__ grp) {
    const int rb = (nblk + gridDim.x - 1) / gridDim.x, r0 = blockIdx.x * rb, r1 = min(nblk, r0 + rb);
    for (int j = threadIdx.x; j < NV; j += 256) {
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        int r = r0;
        for (; r + 3 < r1; r += 4) {
            a0 += (double)partial[(size_t)r * NV + j]; a1 += (double)partial[(size_t)(r + 1) * NV + j];
            a2 += (double)partial[(size_t)(r + 2) * NV + j]; a3 += (double)partial[(size_t)(r + 3) * NV + j];
        }
        for (; r < r1; ++r) a0 += (double)partial[(size_t)r * NV + j];
        grp[(size_t)blockIdx.x * NV + j] = (a0 + a1) + (a2 + a3);
    }
}

// sums[ML_NS*W + K] (double-accumulated over the group rows) and the scalar loss
template <int K>
__global__ void mloss_finalize_k(const double* __restrict__ grp, int ngrp, float* __restrict__ sums, float* __restrict__ loss, double npix, float lc1, float lc2, float lc3) {
    constexpr int W = MLW<K>::W, NV = MLW<K>::NV;
    __shared__ double sh[NV];
    group_sums(grp, ngrp, NV, sh, sums);
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int s = 0; s < ML_NS; ++s) {
            const double ce = sh[s * W] / npix, bce = sh[s * W + 1] / (npix * K);
            const double dice = dice_sum(sh, K, s * W + 2, s * W + 2 + K, ML_NS * W);
            tot += lc1 * ce + lc2 * dice / K + lc3 * bce;
        }
        loss[0] = (float)tot;
    }
}

// Round 6: the kernel was register-bound, not memory-bound (256 VGPRs + 256 AGPRs + 708 bytes of scratch, ONE wave per SIMD: nothing hid its transcendental chains;
// staging the 36-byte pixel rows through LDS as coalesced float4s made it slower still - profiles/r06_emcad_notes.txt).  The foreground part (softmax over the K classes
// couples them: CE + Dice) and the background part (BCE: every class on its own) share nothing but the subset loop, so they run one after the other, the background
// part class by class with four logits and four gradient sums live: ~130 registers, three to four waves per SIMD.
template <int K>
__global__ __launch_bounds__(256) void mloss_bwd_k(ml_maps m, const long long* __restrict__ label, const float* __restrict__ bgm, size_t NP, size_t HW,
                                                   const float* __restrict__ sums, float gscale, float lc1, float lc2, float lc3) {
    __shared__ float tA[ML_NS * K], tB[ML_NS * K];
    dice_coef<K>(sums, MLW<K>::W, 2, gscale * lc2 / K, tA, tB);
    __syncthreads();
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= NP) return;
    const int lab = (int)label[p];
    const size_t n = p / HW, hw = p % HW;
    const float wce = gscale * lc1 / (float)NP, wbce = gscale * lc3 / ((float)NP * K);
    {       // ---- foreground maps: d(CE + Dice) / d logits
        float f[4][K], gf[4][K];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int k = 0; k < K; ++k) { f[i][k] = m.fg[i][p * K + k]; gf[i][k] = 0.f; }
#pragma unroll 1
        for (int s = 1; s <= ML_NS; ++s) {
            const float w0 = s & 1 ? 1.f : 0.f, w1 = s & 2 ? 1.f : 0.f, w2 = s & 4 ? 1.f : 0.f, w3 = s & 8 ? 1.f : 0.f;          // (x * 1 and + 0 are exact: the subset sums keep their order)
            float z[K];
#pragma unroll
            for (int k = 0; k < K; ++k) z[k] = ((w0 * f[0][k] + w1 * f[1][k]) + w2 * f[2][k]) + w3 * f[3][k];
            float mx, pr[K], g[K], dot = 0.f;
            const float inv = __builtin_amdgcn_rcpf(exp_shifted<K>(z, pr, mx));
#pragma unroll
            for (int k = 0; k < K; ++k) {
                pr[k] *= inv;
                g[k] = dice_dp(lab == k ? tA[(s - 1) * K + k] : 0.f, tB[(s - 1) * K + k], pr[k]);
                dot += g[k] * pr[k];
            }
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const float dz = ce_dice_dz(pr[k], lab == k, g[k], dot, wce);
                gf[0][k] += w0 * dz; gf[1][k] += w1 * dz; gf[2][k] += w2 * dz; gf[3][k] += w3 * dz;
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int k = 0; k < K; ++k) m.dfg[i][p * K + k] = gf[i][k];
    }
    // ---- background maps: d BCE / d logits, class by class (same subset order, same sums per (map, class) as before)
#pragma unroll
    for (int k = 0; k < K; ++k) {
        float b[4], gb[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 4; ++i) b[i] = m.bg[i][p * K + k];
        const float mk = bgm[(n * K + k) * HW + hw];
#pragma unroll
        for (int s = 1; s <= ML_NS; ++s) {
            float zb = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) if (s >> i & 1) zb += b[i];
            const float sg = __builtin_amdgcn_rcpf(1.f + __expf(-zb)), dzb = wbce * (sg - mk);
#pragma unroll
            for (int i = 0; i < 4; ++i) if (s >> i & 1) gb[i] += dzb;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) m.dbg[i][p * K + k] = gb[i];
    }
}

// ------------------------------------------------------------------------------------------ single-supervision CE + Dice loss (EMCADNet, dual=False)
// EMCAD/trainer.py:141-153 with utils/utils.py:102-138 (DiceLoss, softmax=True):
//   loss = sum over the SELECTED non-empty subsets s of the 4 maps of  w_ce * CE(sum_{i in s} P_i, label) + w_dice * Dice(softmax(sum P_i), onehot(label))
// `subsets` is a 15-bit mask, bit s-1 selects subset s (bit i of s: map i is in the sum): 0x7FFF 'mutation', 0x008B 'deep_supervision', 0x0080 the last map.
// The foreground half of mloss_*_k (the same ce_dice_* core, reduce kernel and Dice term) around kernels of its own, K = 2..9 classes.  The subset loop is rolled:
// `s` and the mask live in scalar registers, an unselected subset is one scalar branch - no transcendentals, nothing added to any sum or gradient.
// A map's logits enter a subset sum through a select, not a multiply by 0: a map outside every selected subset cannot leak a NaN / inf into the loss.
struct sl_maps { const float* m[4]; float* d[4]; };

template <int K>
__global__ __launch_bounds__(256) void sloss_fwd_k(sl_maps m, unsigned subsets, const long long* __restrict__ label, size_t NP, float* __restrict__ partial) {
    constexpr int W = SLW<K>::W, NV = SLW<K>::NV;
    __shared__ float red[16][NV];          // the 16 DPP-row partials of the block (see mloss_fwd_k)
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, rrow = wid * 4 + (lane >> 4);
    const bool rlead = (lane & 15) == 0;
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool ok = p < NP;
    float f[4][K];
    int lab = -1;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < K; ++k) f[i][k] = 0.f;
    if (ok) {
        lab = (int)label[p];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int k = 0; k < K; ++k) f[i][k] = m.m[i][p * K + k];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {          // label histogram (sum of target^2 per class), once
        const float t = row16_sum((ok && lab == k) ? 1.f : 0.f);
        if (rlead) red[rrow][ML_NS * W + k] = t;
    }
#pragma unroll 1
    for (int s = 1; s <= ML_NS; ++s) {
        if (!(subsets >> (s - 1) & 1)) continue;
        const bool b0 = s & 1, b1 = s & 2, b2 = s & 4, b3 = s & 8;
        float z[K], v[W];
#pragma unroll
        for (int k = 0; k < K; ++k) z[k] = (((b0 ? f[0][k] : 0.f) + (b1 ? f[1][k] : 0.f)) + (b2 ? f[2][k] : 0.f)) + (b3 ? f[3][k] : 0.f);
        v[0] = ce_dice_fwd<K>(z, lab, v + 1, v + 1 + K);
#pragma unroll
        for (int j = 0; j < W; ++j) v[j] = row16_sum(ok ? v[j] : 0.f);
        if (rlead) {
#pragma unroll
            for (int j = 0; j < W; ++j) red[rrow][(s - 1) * W + j] = v[j];
        }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < NV; j += 256) {
        const int s0 = j / W;          // == ML_NS for the histogram columns
        float t = 0.f;
        if (s0 >= ML_NS || (subsets >> s0 & 1)) {          // an unselected subset's columns were never written: exact zeros
#pragma unroll
            for (int i = 0; i < 16; ++i) t += red[i][j];
        }
        partial[(size_t)blockIdx.x * NV + j] = t;
    }
}

// sums[15 * (1 + 2K) + K] (double-accumulated over the group rows) and the scalar loss over the selected subsets
__global__ void sloss_finalize_k(const double* __restrict__ grp, int ngrp, int K, unsigned subsets, float* __restrict__ sums, float* __restrict__ loss, double npix,
                                 float w_ce, float w_dice) {
    const int W = 1 + 2 * K, NV = ML_NS * W + K;
    __shared__ double sh[SLW<9>::NV];
    group_sums(grp, ngrp, NV, sh, sums);
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int s = 0; s < ML_NS; ++s) {
            if (!(subsets >> s & 1)) continue;
            const double dice = dice_sum(sh, K, s * W + 1, s * W + 1 + K, ML_NS * W);
            tot += w_ce * (sh[s * W] / npix) + w_dice * dice / K;
        }
        loss[0] = (float)tot;
    }
}

// gradients of the four maps (recomputed softmaxes, Dice coefficients once per block in LDS - see dice_coef); a map in no selected subset gets exact zeros, written
template <int K>
__global__ __launch_bounds__(256) void sloss_bwd_k(sl_maps m, unsigned subsets, const long long* __restrict__ label, size_t NP, const float* __restrict__ sums,
                                                   float gscale, float w_ce, float w_dice) {
    __shared__ float tA[ML_NS * K], tB[ML_NS * K];
    dice_coef<K>(sums, SLW<K>::W, 1, gscale * w_dice / K, tA, tB);
    __syncthreads();
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= NP) return;
    const int lab = (int)label[p];
    const float wce = gscale * w_ce / (float)NP;
    float f[4][K], gf[4][K];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < K; ++k) { f[i][k] = m.m[i][p * K + k]; gf[i][k] = 0.f; }
#pragma unroll 1
    for (int s = 1; s <= ML_NS; ++s) {
        if (!(subsets >> (s - 1) & 1)) continue;
        const bool b0 = s & 1, b1 = s & 2, b2 = s & 4, b3 = s & 8;
        float z[K];
#pragma unroll
        for (int k = 0; k < K; ++k) z[k] = (((b0 ? f[0][k] : 0.f) + (b1 ? f[1][k] : 0.f)) + (b2 ? f[2][k] : 0.f)) + (b3 ? f[3][k] : 0.f);
        float mx, pr[K], g[K], dot = 0.f;
        const float inv = __builtin_amdgcn_rcpf(exp_shifted<K>(z, pr, mx));
#pragma unroll
        for (int k = 0; k < K; ++k) {
            pr[k] *= inv;
            g[k] = dice_dp(lab == k ? tA[(s - 1) * K + k] : 0.f, tB[(s - 1) * K + k], pr[k]);
            dot += g[k] * pr[k];
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float dz = ce_dice_dz(pr[k], lab == k, g[k], dot, wce);
            gf[0][k] += b0 ? dz : 0.f; gf[1][k] += b1 ? dz : 0.f; gf[2][k] += b2 ? dz : 0.f; gf[3][k] += b3 ? dz : 0.f;
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < K; ++k) m.d[i][p * K + k] = gf[i][k];
}

// ------------------------------------------------------------------------------------------ dual-supervision loss, K = 2..9 classes, selected subsets
// EMCAD/trainer.py:109-140 (dual) in every supervision mode: mloss_*_k with the subsets that are scored as sloss_*_k's run-time 15-bit mask, on the same ce_dice_*
// core, MLW<K> rows, reduce kernel and Dice term.  The forward keeps mloss_fwd_k's unrolled subset loop, every subset under one scalar branch on its mask bit (which
// maps a subset sums is then fixed at compile time: a map outside every selected subset is loaded and never read, whatever it holds); the backward's foreground
// loop is rolled as in mloss_bwd_k, with sloss_bwd_k's selects instead of 0 / 1 multiplies.  Sums, their order and their values are those of mloss_*_k: with
// K = 9 and all 15 subsets the forward gives the bits of mloss_fwd_k<9>.  The backward does not (the compiler fuses other multiply-adds, one ulp here and there);
// pn2_dual_loss_bwd sends that one case to mloss_bwd_k<9> itself.
template <int K>
__global__ __launch_bounds__(256) void dloss_fwd_k(ml_maps m, unsigned subsets, const long long* __restrict__ label, const float* __restrict__ bgm, size_t NP, size_t HW,
                                                   float* __restrict__ partial) {
    constexpr int W = MLW<K>::W, NV = MLW<K>::NV;
    __shared__ float red[16][NV];          // the 16 DPP-row partials of the block (see mloss_fwd_k)
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, rrow = wid * 4 + (lane >> 4);
    const bool rlead = (lane & 15) == 0;
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool ok = p < NP;
    const size_t n = ok ? p / HW : 0, hw = ok ? p % HW : 0;
    int lab = -1;
    {       // ---- foreground maps: CE, intersect and sum p^2 per class
        float f[4][K];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int k = 0; k < K; ++k) f[i][k] = 0.f;
        if (ok) {
            lab = (int)label[p];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int k = 0; k < K; ++k) f[i][k] = m.fg[i][p * K + k];
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {          // label histogram (sum of target^2 per class), once
            const float t = row16_sum((ok && lab == k) ? 1.f : 0.f);
            if (rlead) red[rrow][ML_NS * W + k] = t;
        }
#pragma unroll
        for (int s = 1; s <= ML_NS; ++s) {
            if (!(subsets >> (s - 1) & 1)) continue;
            float z[K], v[W];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                z[k] = 0.f;
#pragma unroll
                for (int i = 0; i < 4; ++i) if (s >> i & 1) z[k] += f[i][k];
            }
            v[0] = ce_dice_fwd<K>(z, lab, v + 2, v + 2 + K); v[1] = 0.f;
#pragma unroll
            for (int j = 0; j < W; ++j) if (j != 1) v[j] = row16_sum(ok ? v[j] : 0.f);
            if (rlead) {
#pragma unroll
                for (int j = 0; j < W; ++j) if (j != 1) red[rrow][(s - 1) * W + j] = v[j];
            }
        }
    }
    {       // ---- background maps: BCE, class by class with four logits live
        float bce[ML_NS];
#pragma unroll
        for (int s = 0; s < ML_NS; ++s) bce[s] = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            float b[4] = {0.f, 0.f, 0.f, 0.f}, mk = 0.f;
            if (ok) {
#pragma unroll
                for (int i = 0; i < 4; ++i) b[i] = m.bg[i][p * K + k];
                mk = bgm[(n * K + k) * HW + hw];
            }
#pragma unroll
            for (int s = 1; s <= ML_NS; ++s) {
                if (!(subsets >> (s - 1) & 1)) continue;
                float zb = 0.f;
#pragma unroll
                for (int i = 0; i < 4; ++i) if (s >> i & 1) zb += b[i];
                bce[s - 1] += fmaxf(zb, 0.f) - zb * mk + __logf(1.f + __expf(-fabsf(zb)));
            }
        }
#pragma unroll
        for (int s = 0; s < ML_NS; ++s) {
            if (!(subsets >> s & 1)) continue;
            const float t = row16_sum(ok ? bce[s] : 0.f);
            if (rlead) red[rrow][s * W + 1] = t;
        }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < NV; j += 256) {
        const int s0 = j / W;          // == ML_NS for the histogram columns
        float t = 0.f;
        if (s0 >= ML_NS || (subsets >> s0 & 1)) {          // an unselected subset's columns were never written: exact zeros
#pragma unroll
            for (int i = 0; i < 16; ++i) t += red[i][j];
        }
        partial[(size_t)blockIdx.x * NV + j] = t;
    }
}

// sums[15 * (2 + 2K) + K] (double-accumulated over the group rows) and the scalar loss over the selected subsets
__global__ void dloss_finalize_k(const double* __restrict__ grp, int ngrp, int K, unsigned subsets, float* __restrict__ sums, float* __restrict__ loss, double npix,
                                 float lc1, float lc2, float lc3) {
    const int W = 2 + 2 * K, NV = ML_NS * W + K;
    __shared__ double sh[MLW<9>::NV];
    group_sums(grp, ngrp, NV, sh, sums);
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int s = 0; s < ML_NS; ++s) {
            if (!(subsets >> s & 1)) continue;
            const double ce = sh[s * W] / npix, bce = sh[s * W + 1] / (npix * K);
            const double dice = dice_sum(sh, K, s * W + 2, s * W + 2 + K, ML_NS * W);
            tot += lc1 * ce + lc2 * dice / K + lc3 * bce;
        }
        loss[0] = (float)tot;
    }
}

// gradients of the eight maps; a map in no selected subset gets exact zeros, written
template <int K>
__global__ __launch_bounds__(256) void dloss_bwd_k(ml_maps m, unsigned subsets, const long long* __restrict__ label, const float* __restrict__ bgm, size_t NP, size_t HW,
                                                   const float* __restrict__ sums, float gscale, float lc1, float lc2, float lc3) {
    __shared__ float tA[ML_NS * K], tB[ML_NS * K];
    dice_coef<K>(sums, MLW<K>::W, 2, gscale * lc2 / K, tA, tB);
    __syncthreads();
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= NP) return;
    const int lab = (int)label[p];
    const size_t n = p / HW, hw = p % HW;
    const float wce = gscale * lc1 / (float)NP, wbce = gscale * lc3 / ((float)NP * K);
    {       // ---- foreground maps: d(CE + Dice) / d logits
        float f[4][K], gf[4][K];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int k = 0; k < K; ++k) { f[i][k] = m.fg[i][p * K + k]; gf[i][k] = 0.f; }
#pragma unroll 1
        for (int s = 1; s <= ML_NS; ++s) {
            if (!(subsets >> (s - 1) & 1)) continue;
            const bool b0 = s & 1, b1 = s & 2, b2 = s & 4, b3 = s & 8;
            float z[K];
#pragma unroll
            for (int k = 0; k < K; ++k) z[k] = (((b0 ? f[0][k] : 0.f) + (b1 ? f[1][k] : 0.f)) + (b2 ? f[2][k] : 0.f)) + (b3 ? f[3][k] : 0.f);
            float mx, pr[K], g[K], dot = 0.f;
            const float inv = __builtin_amdgcn_rcpf(exp_shifted<K>(z, pr, mx));
#pragma unroll
            for (int k = 0; k < K; ++k) {
                pr[k] *= inv;
                g[k] = dice_dp(lab == k ? tA[(s - 1) * K + k] : 0.f, tB[(s - 1) * K + k], pr[k]);
                dot += g[k] * pr[k];
            }
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const float dz = ce_dice_dz(pr[k], lab == k, g[k], dot, wce);
                gf[0][k] += b0 ? dz : 0.f; gf[1][k] += b1 ? dz : 0.f; gf[2][k] += b2 ? dz : 0.f; gf[3][k] += b3 ? dz : 0.f;
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int k = 0; k < K; ++k) m.dfg[i][p * K + k] = gf[i][k];
    }
    // ---- background maps: d BCE / d logits, class by class (which maps a subset sums is fixed at compile time here)
#pragma unroll
    for (int k = 0; k < K; ++k) {
        float b[4], gb[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 4; ++i) b[i] = m.bg[i][p * K + k];
        const float mk = bgm[(n * K + k) * HW + hw];
#pragma unroll
        for (int s = 1; s <= ML_NS; ++s) {
            if (!(subsets >> (s - 1) & 1)) continue;
            float zb = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) if (s >> i & 1) zb += b[i];
            const float sg = __builtin_amdgcn_rcpf(1.f + __expf(-zb)), dzb = wbce * (sg - mk);
#pragma unroll
            for (int i = 0; i < 4; ++i) if (s >> i & 1) gb[i] += dzb;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) m.dbg[i][p * K + k] = gb[i];
    }
}

// the built class counts of the single-supervision and the dual-supervision loss: f(Int<K>) for 2 <= K <= 9, -2 for any other
template <typename F>
int with_seg_classes(int K, F f) {
    switch (K) {
        case 2: return f(Int<2>{}); case 3: return f(Int<3>{}); case 4: return f(Int<4>{}); case 5: return f(Int<5>{});
        case 6: return f(Int<6>{}); case 7: return f(Int<7>{}); case 8: return f(Int<8>{}); case 9: return f(Int<9>{});
    }
    return -2;
}

// the built depth-wise walks (K x K window, VT channels per thread): f(Int<K>, Int<VT>) for a built pair, -2 for any other.  bf16 packs two channels
// per register and has no VT = 1; fp32 has no VT = 8; wider windows take fewer channels per thread (registers)
template <typename T, typename F>
int with_dw_kernel(int K, int VT, F f) {
    constexpr bool bf = sizeof(T) == 2;
    if (K == 1 && VT == 8) { if constexpr (bf) return f(Int<1>{}, Int<8>{}); }
    if (K == 1 && VT == 4) return f(Int<1>{}, Int<4>{});
    if (K == 1 && VT == 2) return f(Int<1>{}, Int<2>{});
    if (K == 1 && VT == 1) { if constexpr (!bf) return f(Int<1>{}, Int<1>{}); }
    if (K == 3 && VT == 4) return f(Int<3>{}, Int<4>{});
    if (K == 3 && VT == 2) return f(Int<3>{}, Int<2>{});
    if (K == 3 && VT == 1) { if constexpr (!bf) return f(Int<3>{}, Int<1>{}); }
    if (K == 5 && VT == 2) return f(Int<5>{}, Int<2>{});
    if (K == 5 && VT == 1) { if constexpr (!bf) return f(Int<5>{}, Int<1>{}); }
    return -2;
}

// geometry of the segment walks (depth-wise K x K and pair conv): a thread owns VT channels (outputs) and walks row segments of SEG pixels, SPR per image
// row; a block = cvp channel groups x 256 / cvp lanes and takes SPB segments; grid (gx, gy).  gx is capped near 1024: it is also the number of partial rows
struct SegWalk { int VT, SEG, SPR, SPB, cvp, gx, gy; };
// CV: channel groups; lanes: the most of them that one block takes
inline void seg_walk(int N, int H, int W, int CV, int lanes, SegWalk& g) {
    int target = 16;
    if ((long long)N * H * ((W + 15) / 16) * CV < 200000) target = 8;
    g.SPR = (W + target - 1) / target; g.SEG = (W + g.SPR - 1) / g.SPR;
    g.cvp = CV >= lanes ? lanes : pow2ceil(CV);
    const int R = 256 / g.cvp, nseg = N * H * g.SPR;
    g.gy = (CV + g.cvp - 1) / g.cvp;
    int want = 2048 / g.gy; if (want < 1) want = 1; if (want > 1024) want = 1024;
    g.SPB = (nseg + want - 1) / want;
    g.SPB = ((g.SPB + R - 1) / R) * R;
    g.gx = (nseg + g.SPB - 1) / g.SPB;
}
// depth-wise K x K.  kind 0: forward / data gradient, 1: weight gradient.  Channels per thread shrink with the window (registers: K*K weights or
// accumulators per channel); a block spans 256 contiguous bytes of one pixel
inline int dwk_geometry(int dt, int kind, int N, int H, int W, int C, int K, SegWalk& g) {
    const int vmax = vec_of(dt);
    g.VT = K == 1 ? vmax : (K == 3 ? (kind ? 2 : 4) : 2);
    if (g.VT > vmax) g.VT = vmax;
    while (g.VT > 1 && C % g.VT) g.VT >>= 1;
    if (g.VT * (dt == PN2_F32 ? 4 : 2) < 4) return -2;          // at least one 32-bit word per thread (bf16: even channel counts)
    seg_walk(N, H, W, C / g.VT, (dt == PN2_F32 ? 64 : 128) / g.VT, g);
    return 0;
}
// pair conv: VT outputs per thread (one 16-byte vector of 2*VT inputs), 32 output groups per block
inline int pc_geometry(int dt, int N, int H, int W, int F, SegWalk& g) {
    g.VT = dt == PN2_F32 ? 2 : 4;
    if (F % g.VT || N < 1 || H < 1 || W < 1) return -2;
    seg_walk(N, H, W, F / g.VT, 32, g);
    return 0;
}

}  // namespace

extern "C" {

/* rows of the BatchNorm partial buffers of pn2_dwconv (wgrad = 0) / of the partial buffer of pn2_dwconv_wgrad (wgrad = 1) */
int pn2_dwconv_blocks(int dt, int N, int H, int W, int C, int K, int wgrad) {
    if (N < 1 || H < 1 || W < 1 || (K != 1 && K != 3 && K != 5)) return -1;
    SegWalk g;
    return dwk_geometry(dt, wgrad ? 1 : 0, N, H, W, C, K, g) ? -1 : g.gx;
}

/* depth-wise K x K conv (K = 1, 3, 5), pad K/2, stride 1, no bias; flip = data gradient; psum/psq: BatchNorm partial rows
 * [pn2_dwconv_blocks(dt, N, H, W, C, K, 0)][C] */
int pn2_dwconv(int dt, const void* x, const float* w, void* z, int N, int H, int W, int C, int K, int flip, int accumulate, float* psum, float* psq, void* stream) {
    if (!x || !w || !z || (psum && !psq)) return -1;
    SegWalk g;
    if (dwk_geometry(dt, 0, N, H, W, C, K, g)) return -2;
    return with_storage_dtype(dt, [&](auto ty) {
        using T = type_of<decltype(ty)>;
        return with_dw_kernel<T>(K, g.VT, [&](auto k, auto vt) {
            return pn2_launch<dwconv_row_k<T, decltype(k)::value, decltype(vt)::value>>(dim3(g.gx, g.gy), dim3(256), (size_t)256 * g.VT * 4, 0, (hipStream_t)stream, (const T*)x, w, (T*)z, N, H, W, C,
                                                                                        flip, accumulate, psum, psq, g.SEG, g.SPR, g.SPB, g.cvp);
        });
    });
}

/* partial[pn2_dwconv_blocks(dt, N, H, W, C, K, 1)][C*K*K] of the depth-wise weight gradient; finish with pn2_colsum_finalize(partial, nblk, C*K*K, C*K*K, dW, acc) */
int pn2_dwconv_wgrad(int dt, const void* dz, const void* x, float* partial, int N, int H, int W, int C, int K, void* stream) {
    if (!dz || !x || !partial) return -1;
    SegWalk g;
    if (dwk_geometry(dt, 1, N, H, W, C, K, g)) return -2;
    return with_storage_dtype(dt, [&](auto ty) {
        using T = type_of<decltype(ty)>;
        return with_dw_kernel<T>(K, g.VT, [&](auto k, auto vt) {
            return pn2_launch<dwconv_wgrad_row_k<T, decltype(k)::value, decltype(vt)::value>>(dim3(g.gx, g.gy), dim3(256), (size_t)256 * g.VT * 4, 0, (hipStream_t)stream, (const T*)dz, (const T*)x, partial,
                                                                                              N, H, W, C, g.SEG, g.SPR, g.SPB, g.cvp);
        });
    });
}

/* rows of the BatchNorm partial buffers of pn2_pairconv3x3_fwd and of the partial buffer of pn2_pairconv3x3_wgrad */
int pn2_pairconv_blocks(int dt, int N, int H, int W, int F) {
    SegWalk g;
    return pc_geometry(dt, N, H, W, F, g) ? -1 : g.gx;
}

/* grouped 3x3 conv, groups = F, 2 input channels per group (LGAG.W_g / W_x), pad 1, bias-free here (the bias is folded by the caller):
 * x [M][2F] -> z [M][F] + BN partial rows [pn2_pairconv_blocks(dt, N, H, W, F)][F] ; w [F][2][9] fp32 */
int pn2_pairconv3x3_fwd(int dt, const void* x, const float* w, void* z, int N, int H, int W, int F, float* psum, float* psq, void* stream) {
    if (!x || !w || !z || !psum || !psq) return -1;
    SegWalk g;
    if (pc_geometry(dt, N, H, W, F, g)) return -2;
    return with_storage_dtype(dt, [&](auto ty) {
        using T = type_of<decltype(ty)>;
        constexpr int VT = TT<T>::VEC / 2;
        return pn2_launch<pairconv_fwd_k<T, VT>>(dim3(g.gx, g.gy), dim3(256), 256 * VT * 4, 0, (hipStream_t)stream, (const T*)x, w, (T*)z, N, H, W, F, psum, psq, g.SEG, g.SPR, g.SPB, g.cvp);
    });
}

int pn2_pairconv3x3_dgrad(int dt, const void* dz, const float* w, void* dx, int N, int H, int W, int F, int accumulate, void* stream) {
    if (!dz || !w || !dx) return -1;
    SegWalk g;
    if (pc_geometry(dt, N, H, W, F, g)) return -2;
    const int R = 256 / g.cvp, nseg = N * H * g.SPR;          // one segment per lane: no partial rows to bound
    return with_storage_dtype(dt, [&](auto ty) {
        using T = type_of<decltype(ty)>;
        return pn2_launch<pairconv_dgrad_k<T, TT<T>::VEC / 2>>(dim3((nseg + R - 1) / R, g.gy), dim3(256), 0, 0, (hipStream_t)stream, (const T*)dz, w, (T*)dx, N, H, W, F, accumulate, g.SEG, g.SPR, g.cvp);
    });
}

/* partial[pn2_pairconv_blocks(dt, N, H, W, F)][F*18] ; finish with pn2_colsum_finalize */
int pn2_pairconv3x3_wgrad(int dt, const void* dz, const void* x, float* partial, int N, int H, int W, int F, void* stream) {
    if (!dz || !x || !partial) return -1;
    SegWalk g;
    if (pc_geometry(dt, N, H, W, F, g)) return -2;
    return with_storage_dtype(dt, [&](auto ty) {
        using T = type_of<decltype(ty)>;
        constexpr int VT = TT<T>::VEC / 2;
        return pn2_launch<pairconv_wgrad_k<T, VT>>(dim3(g.gx, g.gy), dim3(256), 256 * VT * 4, 0, (hipStream_t)stream, (const T*)dz, (const T*)x, partial, N, H, W, F, g.SEG, g.SPR, g.SPB, g.cvp);
    });
}

/* y (+)= x * gate ; mode 0: gate [N][C] (CAB), mode 1: gate [N][HW] (SAB, LGAG) ; gate fp32.  Also the data gradient (x := dy). */
int pn2_gate_mul(int dt, const void* x, const float* gate, void* y, int N, int HW, int C, int mode, int accumulate, void* stream) {
    if (!x || !gate || !y) return -1;
    const int V = vec_of(dt);
    if (C % V) return -2;
    return with_storage_dtype(dt, [&](auto ty) {
        using T = type_of<decltype(ty)>;
        return pn2_launch<gate_mul_k<T>>(dim3(grid_for((size_t)N * HW * (C / V), GRID_CAP)), dim3(256), 0, 0, (hipStream_t)stream, (const T*)x, gate, (T*)y, N, HW, C, mode, accumulate);
    });
}

/* gate gradient.  mode 1: dgate [N][HW] = sum_c dy*x, written directly.  mode 0: partial [pn2_gate_blocks(dt, HW, C)][N*C] rows, finish with
 * pn2_colsum_finalize(partial, nblk, N*C, N*C, dgate, acc) */
int pn2_gate_blocks(int dt, int HW, int C) {
    const int V = vec_of(dt);
    if (HW < 1 || C % V) return -1;
    int cvp, pix, nblk; walk_geometry(HW, C / V, cvp, pix, nblk);
    return nblk;
}

int pn2_gate_bwd(int dt, const void* dy, const void* x, float* dgate_or_partial, int N, int HW, int C, int mode, void* stream) {
    if (!dy || !x || !dgate_or_partial) return -1;
    const int V = vec_of(dt);
    if (C % V) return -2;
    hipStream_t st = (hipStream_t)stream;
    return with_storage_dtype(dt, [&](auto ty) {
        using T = type_of<decltype(ty)>;
        if (mode == 1) return pn2_launch<gate_dpix_k<T>>(dim3(grid_for((size_t)N * HW * 64, GRID_CAP)), dim3(256), 0, 0, st, (const T*)dy, (const T*)x, dgate_or_partial, (size_t)N * HW, C);
        int cvp, pix, nblk; walk_geometry(HW, C / V, cvp, pix, nblk);
        return pn2_launch<gate_dchan_k<T>>(dim3(nblk, N), dim3(256), 256 * TT<T>::VEC * 4, 0, st, (const T*)dy, (const T*)x, dgate_or_partial, N, HW, C, pix, cvp);
    });
}

/* nn.AdaptiveAvgPool2d(1) and nn.AdaptiveMaxPool2d(1) in one pass (CAB): avg, mx [N][C] in the compute dtype, arg [N][C] = argmax pixel */
int pn2_global_pool(int dt, const void* x, void* avg, void* mx, int* arg, int N, int HW, int C, void* stream) {
    if (!x || !avg || !mx || !arg) return -1;
    const int V = vec_of(dt);
    if (C % V) return -2;
    return with_storage_dtype(dt, [&](auto ty) {
        using T = type_of<decltype(ty)>;
        return pn2_launch<global_pool_k<T>>(dim3((C / V + 7) / 8, N), dim3(256), 0, 0, (hipStream_t)stream, (const T*)x, (T*)avg, (T*)mx, arg, HW, C);
    });
}

int pn2_global_pool_bwd(int dt, const void* davg, const void* dmax, const int* arg, void* dx, int N, int HW, int C, int accumulate, void* stream) {
    if (!davg || !dmax || !arg || !dx) return -1;
    return with_storage_dtype(dt, [&](auto ty) {
        using T = type_of<decltype(ty)>;
        return pn2_launch<global_pool_bwd_k<T>>(dim3(grid_for((size_t)N * HW * C, GRID_CAP)), dim3(256), 0, 0, (hipStream_t)stream, (const T*)davg, (const T*)dmax, arg, (T*)dx, N, HW, C, accumulate);
    });
}

/* SAB input: out [NP][8] = (mean over channels, max over channels, 0 x 6), arg [NP] = argmax channel */
int pn2_chan_stats(int dt, const void* x, void* out8, int* arg, long long NP, int C, void* stream) {
    if (!x || !out8 || !arg) return -1;
    return with_storage_dtype(dt, [&](auto ty) {
        using T = type_of<decltype(ty)>;
        return pn2_launch<chan_stats_k<T>>(dim3(grid_for((size_t)NP * 64, GRID_CAP)), dim3(256), 0, 0, (hipStream_t)stream, (const T*)x, (T*)out8, arg, (size_t)NP, C);
    });
}

int pn2_chan_stats_bwd(int dt, const void* dout8, const int* arg, void* dx, long long NP, int C, int accumulate, void* stream) {
    if (!dout8 || !arg || !dx) return -1;
    return with_storage_dtype(dt, [&](auto ty) {
        using T = type_of<decltype(ty)>;
        return pn2_launch<chan_stats_bwd_k<T>>(dim3(grid_for((size_t)NP * C, GRID_CAP)), dim3(256), 0, 0, (hipStream_t)stream, (const T*)dout8, arg, (T*)dx, (size_t)NP, C, accumulate);
    });
}

/* nn.Upsample(scale_factor=2) (nearest) and its adjoint */
int pn2_upsample_nearest2x(int dt, const void* x, void* y, int N, int H, int W, int C, void* stream) {
    if (!x || !y) return -1;
    const int V = vec_of(dt);
    if (C % V) return -2;
    return with_storage_dtype(dt, [&](auto ty) {
        using T = type_of<decltype(ty)>;
        return pn2_launch<up2_k<T>>(dim3(grid_for((size_t)N * 4 * H * W * (C / V), GRID_CAP)), dim3(256), 0, 0, (hipStream_t)stream, (const T*)x, (T*)y, N, H, W, C);
    });
}

int pn2_upsample_nearest2x_bwd(int dt, const void* dy, void* dx, int N, int H, int W, int C, int accumulate, void* stream) {
    if (!dy || !dx) return -1;
    const int V = vec_of(dt);
    if (C % V) return -2;
    return with_storage_dtype(dt, [&](auto ty) {
        using T = type_of<decltype(ty)>;
        return pn2_launch<up2_bwd_k<T>>(dim3(grid_for((size_t)N * H * W * (C / V), GRID_CAP)), dim3(256), 0, 0, (hipStream_t)stream, (const T*)dy, (T*)dx, N, H, W, C, accumulate);
    });
}

/* y[p][c] = a[p][perm[c]] + b[p][perm[c]] + c[p][perm[c]]   (b, c optional): the MSDC branch sum written through channel_shuffle, and (with the
 * inverse permutation, b = c = null) its adjoint */
int pn2_gather_sum(int dt, const void* a, const void* b, const void* c, const int* perm, void* y, long long M, int C, void* stream) {
    if (!a || !perm || !y) return -1;
    return with_storage_dtype(dt, [&](auto ty) {
        using T = type_of<decltype(ty)>;
        return pn2_launch<gather_sum_k<T>>(dim3(grid_for((size_t)M * C, GRID_CAP)), dim3(256), 0, 0, (hipStream_t)stream, (const T*)a, (const T*)b, (const T*)c, perm, (T*)y, (size_t)M, C);
    });
}

/* pixels per workgroup of pn2_msdc_combine / pn2_msdc_combine_bwd at an output width of Cw channels shuffled in `groups` (the kernel's own `groups`: Cw / groups
 * of the forward for the adjoint); -2 where the shape is not built */
int pn2_msdc_combine_tile(int dt, int Cw, int groups) {
    int padE, TP; size_t lds;
    return mc_geometry(dt, Cw, groups, padE, TP, lds) ? -2 : TP;
}

/* channel_shuffle(sum or cat of n MSDC branches, groups) in one pass: pn2.h */
int pn2_msdc_combine(int dt, int mode, int n, const void* p0, const void* p1, const void* p2, const void* p3, void* y, long long M, int Cpart, int groups, void* stream) {
    if (n < 1 || n > 4 || (mode != MC_SUM && mode != MC_CAT)) return -2;
    McArgs A = {{p0, p1, p2, p3}, {y, nullptr, nullptr, nullptr}, {0, 0, 0, 0}};
    for (int i = 0; i < n; ++i) if (!A.in[i]) return -1;
    if (!y) return -1;
    if (M < 1 || Cpart < 1 || Cpart % vec_of(dt) || Cpart > MC_MAX_CW) return -2;
    const int Cw = mode == MC_CAT ? n * Cpart : Cpart;
    return mode == MC_CAT ? mc_launch<MC_CAT>(dt, A, n, M, Cpart, Cw, groups, stream) : mc_launch<MC_SUM>(dt, A, n, M, Cpart, Cw, groups, stream);
}

/* adjoint of the cat mode: d_i[p][c] (+)= dy[p][dst(i * Cpart + c)], dst the inverse of the forward's src */
int pn2_msdc_combine_bwd(int dt, int n, const void* dy, void* d0, void* d1, void* d2, void* d3, int acc0, int acc1, int acc2, int acc3, long long M, int Cpart,
                         int groups, void* stream) {
    if (n < 1 || n > 4) return -2;
    McArgs A = {{dy, nullptr, nullptr, nullptr}, {d0, d1, d2, d3}, {acc0, acc1, acc2, acc3}};
    if (!dy) return -1;
    for (int i = 0; i < n; ++i) if (!A.out[i]) return -1;
    if (M < 1 || Cpart < 1 || Cpart % vec_of(dt) || Cpart > MC_MAX_CW || groups < 1) return -2;
    const int Cw = n * Cpart;
    if (Cw % groups) return -2;
    return mc_launch<MC_SPLIT>(dt, A, n, M, Cpart, Cw, Cw / groups, stream);
}

/* y = sigmoid(x) as fp32 [n] from a [rows][ld] map with C used channels; dx (+)= dy * y * (1 - y) */
int pn2_sigmoid(int dt_in, const void* x, int ld, int C, float* y, long long n, void* stream) {
    if (!x || !y || n < 1) return -1;
    return with_storage_dtype(dt_in, [&](auto ty) {
        using T = type_of<decltype(ty)>;
        return pn2_launch<sigmoid_k<T>>(dim3(grid_for((size_t)n, GRID_CAP)), dim3(256), 0, 0, (hipStream_t)stream, (const T*)x, y, (size_t)n, ld, C);
    });
}

int pn2_sigmoid_bwd(int dt_out, const float* dy, const float* y, void* dx, int ld, int C, long long n, int accumulate, void* stream) {
    if (!dy || !y || !dx || n < 1) return -1;
    return with_storage_dtype(dt_out, [&](auto ty) {
        using T = type_of<decltype(ty)>;
        return pn2_launch<sigmoid_bwd_k<T>>(dim3(grid_for((size_t)n, GRID_CAP)), dim3(256), 0, 0, (hipStream_t)stream, dy, y, (T*)dx, (size_t)n, ld, C, accumulate);
    });
}

static int ml_blocks(long long npix) { return (int)((npix + 255) / 256); }
/* rows of the `partial` scratch: one per 256 pixels + the double-precision group rows of the second reduction level */
int pn2_mutation_loss_blocks(long long npix) { return npix < 1 ? -1 : ml_blocks(npix) + 2 * ML_RG + 1; }
int pn2_mutation_loss_width(int K) { return K == 9 ? MLW<9>::NV : -1; }
int pn2_seg_loss_width(int K) { const int wd = with_seg_classes(K, [](auto k) { return SLW<decltype(k)::value>::NV; }); return wd > 0 ? wd : -1; }

/* second reduction level of both losses: the ml_blocks(NP) block rows of `partial` (NV floats each) -> ngrp group rows in double at grp, behind the block rows */
static int loss_reduce(float* partial, size_t NP, int NV, hipStream_t st, double*& grp, int& ngrp) {
    const int nblk = ml_blocks((long long)NP);
    ngrp = nblk < 8 * ML_RG ? (nblk + 7) / 8 : ML_RG;
    grp = reinterpret_cast<double*>(partial + (((size_t)nblk * NV + 1) & ~(size_t)1));          // 8-byte aligned
    return pn2_launch<loss_reduce_k>(dim3(ngrp), dim3(256), 0, 0, st, partial, nblk, NV, grp);
}

/* EMCAD/trainer.py:106-140: sum over the 15 non-empty subsets of the 4 scales of lc1*CE + lc2*Dice(softmax) + lc3*BCEWithLogits on the summed maps.
 * fg[4], bg[4]: [N][H][W][K] fp32 maps (K = 9); label [N][H][W] int64; bg_mask [N][K][H][W] fp32.  partial: [pn2_mutation_loss_blocks][pn2_mutation_loss_width]
 * scratch; sums [pn2_mutation_loss_width] is kept for the backward; loss[1]. */
int pn2_mutation_loss_fwd(const float* const* fg, const float* const* bg, const long long* label, const float* bg_mask, int N, long long HW, int K,
                          float lc1, float lc2, float lc3, float* partial, float* sums, float* loss, void* stream) {
    if (!fg || !bg || !label || !bg_mask || !partial || !sums || !loss) return -1;
    if (K != 9) return -2;
    ml_maps m;
    for (int i = 0; i < 4; ++i) { m.fg[i] = fg[i]; m.bg[i] = bg[i]; m.dfg[i] = nullptr; m.dbg[i] = nullptr; if (!fg[i] || !bg[i]) return -1; }
    const size_t NP = (size_t)N * HW;
    hipStream_t st = (hipStream_t)stream;
    double* grp; int ngrp;
    if (int rc = pn2_launch<mloss_fwd_k<9>>(dim3(ml_blocks((long long)NP)), dim3(256), 0, 0, st, m, label, bg_mask, NP, (size_t)HW, partial)) return rc;
    if (int rc = loss_reduce(partial, NP, MLW<9>::NV, st, grp, ngrp)) return rc;
    return pn2_launch<mloss_finalize_k<9>>(dim3(1), dim3(256), 0, 0, st, grp, ngrp, sums, loss, (double)NP, lc1, lc2, lc3);
}

int pn2_mutation_loss_bwd(const float* const* fg, const float* const* bg, float* const* dfg, float* const* dbg, const long long* label, const float* bg_mask,
                          int N, long long HW, int K, float lc1, float lc2, float lc3, const float* sums, float gscale, void* stream) {
    if (!fg || !bg || !dfg || !dbg || !label || !bg_mask || !sums) return -1;
    if (K != 9) return -2;
    ml_maps m;
    for (int i = 0; i < 4; ++i) { m.fg[i] = fg[i]; m.bg[i] = bg[i]; m.dfg[i] = dfg[i]; m.dbg[i] = dbg[i]; if (!fg[i] || !bg[i] || !dfg[i] || !dbg[i]) return -1; }
    const size_t NP = (size_t)N * HW;
    return pn2_launch<mloss_bwd_k<9>>(dim3((unsigned)((NP + 255) / 256)), dim3(256), 0, 0, (hipStream_t)stream, m, label, bg_mask, NP, (size_t)HW, sums, gscale, lc1, lc2, lc3);
}

static bool seg_loss_args_ok(unsigned subsets, int N, long long HW, int K) { return subsets != 0 && subsets <= 0x7FFFu && K >= 2 && K <= 9 && N >= 1 && HW >= 1; }

/* EMCAD/trainer.py:141-153 (single supervision): sum over the subsets selected by `subsets` of w_ce*CE + w_dice*Dice(softmax) on the summed maps.
 * maps[4]: [N][H][W][K] fp32 (2 <= K <= 9); label [N][H][W] int64.  partial: [pn2_mutation_loss_blocks][pn2_seg_loss_width] scratch; sums
 * [pn2_seg_loss_width] is kept for the backward; loss[1]. */
int pn2_seg_loss_fwd(const float* const* maps, unsigned subsets, const long long* label, int N, long long HW, int K, float w_ce, float w_dice,
                     float* partial, float* sums, float* loss, void* stream) {
    if (!maps || !label || !partial || !sums || !loss) return -1;
    if (!seg_loss_args_ok(subsets, N, HW, K)) return -2;
    sl_maps m;
    for (int i = 0; i < 4; ++i) { m.m[i] = maps[i]; m.d[i] = nullptr; if (!maps[i]) return -1; }
    const size_t NP = (size_t)N * HW;
    hipStream_t st = (hipStream_t)stream;
    double* grp; int ngrp;
    if (int rc = with_seg_classes(K, [&](auto k) {
            return pn2_launch<sloss_fwd_k<decltype(k)::value>>(dim3(ml_blocks((long long)NP)), dim3(256), 0, 0, st, m, subsets, label, NP, partial); })) return rc;
    if (int rc = loss_reduce(partial, NP, pn2_seg_loss_width(K), st, grp, ngrp)) return rc;
    return pn2_launch<sloss_finalize_k>(dim3(1), dim3(256), 0, 0, st, grp, ngrp, K, subsets, sums, loss, (double)NP, w_ce, w_dice);
}

int pn2_seg_loss_bwd(const float* const* maps, float* const* dmaps, unsigned subsets, const long long* label, int N, long long HW, int K, float w_ce, float w_dice,
                     const float* sums, float gscale, void* stream) {
    if (!maps || !dmaps || !label || !sums) return -1;
    if (!seg_loss_args_ok(subsets, N, HW, K)) return -2;
    sl_maps m;
    for (int i = 0; i < 4; ++i) { m.m[i] = maps[i]; m.d[i] = dmaps[i]; if (!maps[i] || !dmaps[i]) return -1; }
    const size_t NP = (size_t)N * HW;
    return with_seg_classes(K, [&](auto k) {
        return pn2_launch<sloss_bwd_k<decltype(k)::value>>(dim3((unsigned)((NP + 255) / 256)), dim3(256), 0, 0, (hipStream_t)stream, m, subsets, label, NP, sums,
                                                           gscale, w_ce, w_dice);
    });
}

/* EMCAD/trainer.py:109-140 (dual) in every supervision mode: pn2_mutation_loss_* for 2 <= K <= 9 over the subsets selected by `subsets` (the mask of pn2_seg_loss_*).
 * Buffers as there, rows of pn2_dual_loss_width(K) values; the columns of an unselected subset are zeros. */
int pn2_dual_loss_width(int K) { const int wd = with_seg_classes(K, [](auto k) { return MLW<decltype(k)::value>::NV; }); return wd > 0 ? wd : -1; }

int pn2_dual_loss_fwd(const float* const* fg, const float* const* bg, unsigned subsets, const long long* label, const float* bg_mask, int N, long long HW, int K,
                      float lc1, float lc2, float lc3, float* partial, float* sums, float* loss, void* stream) {
    if (!fg || !bg || !label || !bg_mask || !partial || !sums || !loss) return -1;
    if (!seg_loss_args_ok(subsets, N, HW, K)) return -2;
    ml_maps m;
    for (int i = 0; i < 4; ++i) { m.fg[i] = fg[i]; m.bg[i] = bg[i]; m.dfg[i] = nullptr; m.dbg[i] = nullptr; if (!fg[i] || !bg[i]) return -1; }
    const size_t NP = (size_t)N * HW;
    hipStream_t st = (hipStream_t)stream;
    double* grp; int ngrp;
    if (int rc = with_seg_classes(K, [&](auto k) {
            return pn2_launch<dloss_fwd_k<decltype(k)::value>>(dim3(ml_blocks((long long)NP)), dim3(256), 0, 0, st, m, subsets, label, bg_mask, NP, (size_t)HW, partial); }))
        return rc;
    if (int rc = loss_reduce(partial, NP, pn2_dual_loss_width(K), st, grp, ngrp)) return rc;
    return pn2_launch<dloss_finalize_k>(dim3(1), dim3(256), 0, 0, st, grp, ngrp, K, subsets, sums, loss, (double)NP, lc1, lc2, lc3);
}

int pn2_dual_loss_bwd(const float* const* fg, const float* const* bg, float* const* dfg, float* const* dbg, unsigned subsets, const long long* label,
                      const float* bg_mask, int N, long long HW, int K, float lc1, float lc2, float lc3, const float* sums, float gscale, void* stream) {
    if (!fg || !bg || !dfg || !dbg || !label || !bg_mask || !sums) return -1;
    if (!seg_loss_args_ok(subsets, N, HW, K)) return -2;
    ml_maps m;
    for (int i = 0; i < 4; ++i) { m.fg[i] = fg[i]; m.bg[i] = bg[i]; m.dfg[i] = dfg[i]; m.dbg[i] = dbg[i]; if (!fg[i] || !bg[i] || !dfg[i] || !dbg[i]) return -1; }
    const size_t NP = (size_t)N * HW;
    // K = 9 with all 15 subsets keeps the backward kernel it had: the faster one at 16 x 512^2, and the bits of pn2_mutation_loss_bwd, which
    // dloss_bwd_k<9> misses by one ulp in some elements (the compiler fuses other multiply-adds there)
    if (K == 9 && subsets == 0x7FFFu)
        return pn2_launch<mloss_bwd_k<9>>(dim3((unsigned)((NP + 255) / 256)), dim3(256), 0, 0, (hipStream_t)stream, m, label, bg_mask, NP, (size_t)HW, sums, gscale, lc1, lc2, lc3);
    return with_seg_classes(K, [&](auto k) {
        return pn2_launch<dloss_bwd_k<decltype(k)::value>>(dim3((unsigned)((NP + 255) / 256)), dim3(256), 0, 0, (hipStream_t)stream, m, subsets, label, bg_mask, NP,
                                                           (size_t)HW, sums, gscale, lc1, lc2, lc3);
    });
}

}  // extern "C"
