// pn2_resnet.hip — the strided skip of the ResNet stage-opening blocks (lib/resnet.py: downsample = Conv2d(1x1, stride 2, pad 0) + BatchNorm):
//   subsample_fwd_k   y[n][oh][ow][:] = x[n][oh*stride][ow*stride][:]          OH = (H-1)/stride + 1, OW likewise: the pixels a pad-0 1x1 conv of that stride reads
//   subsample_bwd_k   the adjoint over the WHOLE of dx in one pass: strided pixels take dy (accum: dx + dy), every other pixel takes zero (accum: is left alone, not read)
// The conv itself then runs on the stride-1 pointwise GEMM over the gathered rows (Engine.strided_pointwise): no strided path inside the conv kernels.
// Mapping: 256 threads = CVP channel vectors x R pixel lanes; a lane decodes its pixel ONCE and walks the row's 16-byte vectors, grid-stride over the pixels.  Pure data
// movement: one writer per element, no atomics, bit-identical replays.  ld_* may exceed C (channel slices of wider rows); the columns past C are never touched.
#include "pn2_common.h"
#include "../../include/pn2.h"

namespace {

using namespace pn2_host;
constexpr int GRID_CAP = 16384;

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <typename T>
__global__ __launch_bounds__(256) void subsample_fwd_k(const T* __restrict__ x, int ld_x, T* __restrict__ y, int ld_y, int H, int W, int OH, int OW, int CV, int stride,
                                                       int Mo, int CVP) {
    constexpr int V = TT<T>::VEC;
    const int R = 256 / CVP, cvl = threadIdx.x % CVP, rl = threadIdx.x / CVP;
    for (size_t m = (size_t)blockIdx.x * R + rl; m < (size_t)Mo; m += (size_t)gridDim.x * R) {
        const unsigned mm = (unsigned)m, t = mm / (unsigned)OW, ow = mm - t * (unsigned)OW, n = t / (unsigned)OH, oh = t - n * (unsigned)OH;
        const T* src = x + (((size_t)n * H + (size_t)oh * stride) * W + (size_t)ow * stride) * ld_x;
        T* dst = y + m * ld_y;
#pragma unroll 4
        for (int cv = cvl; cv < CV; cv += CVP) *reinterpret_cast<uint4*>(dst + cv * V) = *reinterpret_cast<const uint4*>(src + cv * V);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void subsample_bwd_k(const T* __restrict__ dy, int ld_dy, T* __restrict__ dx, int ld_dx, int H, int W, int OH, int OW, int CV, int stride,
                                                       int accum, int M, int CVP) {
    constexpr int V = TT<T>::VEC;
    const int R = 256 / CVP, cvl = threadIdx.x % CVP, rl = threadIdx.x / CVP;
    for (size_t m = (size_t)blockIdx.x * R + rl; m < (size_t)M; m += (size_t)gridDim.x * R) {
        const unsigned mm = (unsigned)m, t = mm / (unsigned)W, w = mm - t * (unsigned)W, n = t / (unsigned)H, h = t - n * (unsigned)H;
        const unsigned oh = h / (unsigned)stride, ow = w / (unsigned)stride;
        const bool on = oh * stride == h && ow * stride == w;          // (oh < OH, ow < OW: OH = (H-1)/stride + 1)
        T* dst = dx + m * ld_dx;
        if (on) {
            const T* src = dy + (((size_t)n * OH + oh) * OW + ow) * ld_dy;
            if (accum) {
                for (int cv = cvl; cv < CV; cv += CVP) {
                    float a[V], b[V];
                    TT<T>::unpack(*reinterpret_cast<const uint4*>(dst + cv * V), a); TT<T>::unpack(*reinterpret_cast<const uint4*>(src + cv * V), b);
#pragma unroll
                    for (int e = 0; e < V; ++e) a[e] += b[e];
                    *reinterpret_cast<uint4*>(dst + cv * V) = TT<T>::pack(a);
                }
            } else {
#pragma unroll 4
                for (int cv = cvl; cv < CV; cv += CVP) *reinterpret_cast<uint4*>(dst + cv * V) = *reinterpret_cast<const uint4*>(src + cv * V);
            }
        } else if (!accum) {
            const uint4 z = make_uint4(0u, 0u, 0u, 0u);
            for (int cv = cvl; cv < CV; cv += CVP) *reinterpret_cast<uint4*>(dst + cv * V) = z;
        }
    }
}

// -1 / -2 / 0 of the arguments both entry points share (N, H, W: the full-resolution side)
inline int subsample_check(int dt, const void* a, int ld_a, const void* b, int ld_b, int N, int H, int W, int C, int stride) {
    if (!a || !b) return -1;
    const int V = vec_of(dt);
    if (N < 1 || H < 1 || W < 1 || C < V || C % V || ld_a < C || ld_b < C || ld_a % V || ld_b % V || (stride != 1 && stride != 2) || !al16(a) || !al16(b)) return -2;
    if ((long long)N * H * W > 0x7fffffffLL) return -2;          // pixel indices are decoded in 32 bits
    return 0;
}
inline int pixel_lanes(int dt, int C, int& CVP) {
    CVP = pow2ceil(C / vec_of(dt)); if (CVP > 256) CVP = 256;
    return 256 / CVP;
}

}  // namespace

extern "C" {

int pn2_subsample_fwd(int dt, const void* x, int ld_x, void* y, int ld_y, int N, int H, int W, int C, int stride, void* stream) {
    if (const int rc = subsample_check(dt, x, ld_x, y, ld_y, N, H, W, C, stride)) return rc;
    if (dt != PN2_BF16 && dt != PN2_F32) return -3;
    if (stride == 1) return pn2_copy(dt, x, ld_x, dt, y, ld_y, N * H * W, C, 0, stream);
    const int OH = (H - 1) / stride + 1, OW = (W - 1) / stride + 1, Mo = N * OH * OW;
    int CVP; const int R = pixel_lanes(dt, C, CVP);
    const int grid = grid_for(((size_t)Mo + R - 1) / R * 256, GRID_CAP);
    return with_storage_dtype(dt, [&](auto t) {
        using T = type_of<decltype(t)>;
        return pn2_launch<subsample_fwd_k<T>>(dim3(grid), dim3(256), 0, 0, (hipStream_t)stream, (const T*)x, ld_x, (T*)y, ld_y, H, W, OH, OW, C / TT<T>::VEC, stride, Mo, CVP);
    });
}

int pn2_subsample_bwd(int dt, const void* dy, int ld_dy, void* dx, int ld_dx, int N, int H, int W, int C, int stride, int accum, void* stream) {
    if (const int rc = subsample_check(dt, dy, ld_dy, dx, ld_dx, N, H, W, C, stride)) return rc;
    if (accum != 0 && accum != 1) return -2;
    if (dt != PN2_BF16 && dt != PN2_F32) return -3;
    if (stride == 1) return pn2_copy(dt, dy, ld_dy, dt, dx, ld_dx, N * H * W, C, accum, stream);
    const int OH = (H - 1) / stride + 1, OW = (W - 1) / stride + 1, M = N * H * W;
    int CVP; const int R = pixel_lanes(dt, C, CVP);
    const int grid = grid_for(((size_t)M + R - 1) / R * 256, GRID_CAP);
    return with_storage_dtype(dt, [&](auto t) {
        using T = type_of<decltype(t)>;
        return pn2_launch<subsample_bwd_k<T>>(dim3(grid), dim3(256), 0, 0, (hipStream_t)stream, (const T*)dy, ld_dy, (T*)dx, ld_dx, H, W, OH, OW, C / TT<T>::VEC, stride, accum, M, CVP);
    });
}

}  // extern "C"
