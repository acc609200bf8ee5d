// pn2_zoom.hip - what the Synapse loader and test_single_volume do to a slice with scipy (multiclass_seg/EMCAD/utils/dataset_synapse.py:12-47,
// utils/utils.py:179-181,197-198), on the device and bit for bit:
//   scipy.ndimage.zoom(order=3)   = cubic B-spline prefilter (float64, axis 0 then axis 1, mirror boundaries) + 16-tap gather, cast to float32
//   scipy.ndimage.zoom(order=0)   = nearest sample, floor(cc + 0.5)
//   ndimage.rotate(order=0, reshape=False), np.flip(np.rot90(a, k), axis)
// with scipy's defaults mode='constant', cval=0, grid_mode=False: an output coordinate cc = o * ((nin-1)/(nout-1)) that exceeds nin-1 in double gives 0.
// Every float64 operation is the one ni_splines.c / ni_interpolation.c perform, in their order; scipy's build has no fused multiply-add, so contraction is off
// for this whole file (hipcc contracts a + b*c by default).  The coordinate tables and z^(n-1) are computed on the host in double (pn2_zoom_tables,
// pn2_zoom_pole_pow), so no device pow / floor of a product decides a bit.
#include <cmath>
#include <cstdint>
#include "pn2_common.h"
#include "../../include/pn2.h"

#pragma clang fp contract(off)

namespace {

constexpr int MAX_AXIS = 1024;
// the pole of the cubic B-spline: sqrt(3) - 2 rounded once (the literal of ni_splines.c:get_filter_poles); sqrt(3.0) - 2.0 evaluated in double is one ulp away
constexpr double ZP = -0.267949192431122706472553658494127633;
constexpr int TR = 32;          // rows per transposed tile of the anticausal sweep

inline double filter_gain() { return 1.0 * ((1.0 - ZP) * (1.0 - 1.0 / ZP)); }

// ---- prefilter, first half of one axis: gain, mirror initialisation (the whole line, serial), causal sweep.  One thread owns one line: src / dst are
// [N][R][Cn] with the line along R and the 64 lanes of a block on consecutive columns, so every load and store of the wave is one contiguous 256 / 512 bytes.
template <typename TS>
__global__ __launch_bounds__(64) void spline_causal_k(const TS* __restrict__ src, double* __restrict__ dst, int R, int Cn, int nb, double z, double gain, double zn) {
    const int n = blockIdx.x / nb, c = (blockIdx.x - n * nb) * 64 + threadIdx.x;
    if (c >= Cn) return;
    const TS* s = src + (size_t)n * R * Cn + c;
    double* d = dst + (size_t)n * R * Cn + c;
    if (R == 1) { d[0] = (double)s[0]; return; }          // scipy skips an axis of length 1 (no gain either)
    double c0 = (double)s[0] * gain + zn * ((double)s[(size_t)(R - 1) * Cn] * gain);
    double zi = z;
#pragma unroll 8
    for (int i = 1; i < R - 1; ++i) {          // zi turns denormal near i = 540 and zero near 566: the loop runs on as scipy's does
        const double a = (double)s[(size_t)i * Cn] * gain, b = (double)s[(size_t)(R - 1 - i) * Cn] * gain;
        c0 = c0 + zi * (a + zn * b);
        zi = zi * z;
    }
    c0 = c0 / (1.0 - zn * zn);
    d[0] = c0;
#pragma unroll 8
    for (int i = 1; i < R; ++i) {
        c0 = (double)s[(size_t)i * Cn] * gain + z * c0;
        d[(size_t)i * Cn] = c0;
    }
}

// ---- second half: anticausal initialisation and sweep, from the last row down, written TRANSPOSED: dst is [N][Cn][R].  The next axis then runs through the
// same two kernels with lanes on consecutive addresses again, and its own transposed store restores [N][H][W].  A block's 64 lines x 32 rows go through an
// LDS tile of 33 doubles per line: the column-wise ds_write_b64 of the sweep then falls on banks 2 * lane mod 32 (2 lanes per bank and half wave, the rate
// of an 8-byte store anyway; 32 doubles per line would put all 64 lanes on one bank), and the row-wise ds_read_b64 of the store takes 64 consecutive dwords
// per half wave.  Each half wave stores 256 contiguous bytes.
__global__ __launch_bounds__(64) void spline_anticausal_t_k(const double* __restrict__ src, double* __restrict__ dst, int R, int Cn, int nb, double z) {
    __shared__ double tile[64][TR + 1];
    const int tid = threadIdx.x, n = blockIdx.x / nb, cb = (blockIdx.x - n * nb) * 64, c = cb + tid;
    const bool live = c < Cn;
    const double* s = src + (size_t)n * R * Cn + (live ? c : 0);
    double* dn = dst + (size_t)n * R * Cn;
    double next = 0.0, last = 0.0;
    if (live) last = R > 1 ? (z * s[(size_t)(R - 2) * Cn] + s[(size_t)(R - 1) * Cn]) * z / (z * z - 1.0) : s[0];
    for (int k = (R - 1) / TR; k >= 0; --k) {
        const int r0 = k * TR;
        double v[TR];
#pragma unroll
        for (int rr = 0; rr < TR; ++rr) v[rr] = (live && r0 + rr < R) ? s[(size_t)(r0 + rr) * Cn] : 0.0;
#pragma unroll
        for (int rr = TR - 1; rr >= 0; --rr) {
            const int r = r0 + rr;
            if (r < R) {
                next = r == R - 1 ? last : z * (next - v[rr]);
                tile[tid][rr] = next;
            }
        }
        __syncthreads();
        const int rr = tid & 31;
        if (r0 + rr < R) {
            for (int i = tid >> 5; i < 64; i += 2)
                if (cb + i < Cn) dn[(size_t)(cb + i) * R + r0 + rr] = tile[i][rr];
        }
        __syncthreads();
    }
}

// ---- order 3: out[y][x] = sum_j sum_k (coef[iy_j][ix_k] * wy_j) * wx_k, j outer, k inner, from 0.0 (ni_interpolation.c:NI_ZoomShift), cast to float32
__global__ __launch_bounds__(256) void zoom3_gather_k(const double* __restrict__ coef, int H, int W, int OH, int OW, const int* __restrict__ iy, const double* __restrict__ wy,
                                                      const int* __restrict__ vy, const int* __restrict__ ix, const double* __restrict__ wx, const int* __restrict__ vx,
                                                      float* __restrict__ out, size_t total) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        int ox, oy;
        const size_t n = divmod_idx(divmod_idx(i, OW, ox), OH, oy);
        float r = 0.0f;
        if (vy[oy] && vx[ox]) {
            const double* p = coef + n * H * W;
            double t = 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double* row = p + (size_t)iy[oy * 4 + j] * W;
                const double wj = wy[oy * 4 + j];
#pragma unroll
                for (int k = 0; k < 4; ++k) t = t + (row[ix[ox * 4 + k]] * wj) * wx[ox * 4 + k];
            }
            r = (float)t;
        }
        out[i] = r;
    }
}

// ---- order 0 zoom: out[y][x] = src[iy[y]][ix[x]], 0 on the rows / columns whose coordinate lies past the last sample.  T: the element as raw bits
template <typename T>
__global__ __launch_bounds__(256) void zoom0_k(const T* __restrict__ src, int H, int W, int OH, int OW, const int* __restrict__ iy, const int* __restrict__ vy,
                                               const int* __restrict__ ix, const int* __restrict__ vx, T* __restrict__ out, size_t total) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        int ox, oy;
        const size_t n = divmod_idx(divmod_idx(i, OW, ox), OH, oy);
        out[i] = (vy[oy] && vx[ox]) ? src[(n * H + iy[oy]) * W + ix[ox]] : (T)0;
    }
}

// ---- order 0 rotate (ni_interpolation.c:NI_GeometricTransform with a matrix): m6[n] = { m00, m01, m10, m11, off0, off1 };
// cy = (off0 + y * m00) + x * m01, cx likewise; 0 outside [0, H-1] x [0, W-1] (a NaN counts as outside), else src[floor(cy + 0.5)][floor(cx + 0.5)]
template <typename T>
__global__ __launch_bounds__(256) void rotate0_k(const T* __restrict__ src, int H, int W, const double* __restrict__ m6, T* __restrict__ out, size_t total) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        int x, y;
        const size_t n = divmod_idx(divmod_idx(i, W, x), H, y);
        const double* m = m6 + n * 6;
        const double cy = (m[4] + (double)y * m[0]) + (double)x * m[1];
        const double cx = (m[5] + (double)y * m[2]) + (double)x * m[3];
        T v = (T)0;
        if (cy >= 0.0 && cy <= (double)(H - 1) && cx >= 0.0 && cx <= (double)(W - 1))
            v = src[(n * H + (size_t)floor(cy + 0.5)) * W + (size_t)floor(cx + 0.5)];
        out[i] = v;
    }
}

// ---- np.flip(np.rot90(a, k), axis) of square [S][S] samples as one indexed copy; ka[n] = { k, axis }, axis -1: no flip
template <typename T>
__global__ __launch_bounds__(256) void rot_flip_k(const T* __restrict__ src, int S, const int* __restrict__ ka, T* __restrict__ out, size_t total) {
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        int i, j;
        const size_t n = divmod_idx(divmod_idx(idx, S, j), S, i);
        const int k = ka[n * 2] & 3, axis = ka[n * 2 + 1];
        if (axis == 0) i = S - 1 - i; else if (axis == 1) j = S - 1 - j;
        int si = i, sj = j;                                      // rot90(a, 1)[i][j] = a[j][S-1-i]
        if (k == 1) { si = j; sj = S - 1 - i; }
        else if (k == 2) { si = S - 1 - i; sj = S - 1 - j; }
        else if (k == 3) { si = S - 1 - j; sj = i; }
        out[idx] = src[(n * S + si) * S + sj];
    }
}

inline bool axes_ok(int N, int H, int W) { return N >= 1 && H >= 1 && W >= 1 && H <= MAX_AXIS && W <= MAX_AXIS && (long long)N * H * W < (1ll << 40); }
inline unsigned grid_of(size_t total) { return (unsigned)pn2_host::grid_for(total, 16384); }

template <typename F>
int with_elem(int elem, F f) {
    if (elem == 1) return f(Ty<uint8_t>{});
    if (elem == 4) return f(Ty<uint32_t>{});
    return -3;
}

}  // namespace

extern "C" {

int pn2_zoom_pole_pow(int n, double* zn) {
    if (!zn) return -1;
    if (n < 1 || n > MAX_AXIS) return -2;
    *zn = std::pow(ZP, (double)(n - 1));
    return 0;
}

int pn2_zoom_tables(int nin, int nout, int order, int* idx, double* w, int* valid) {
    if (!idx || !valid || (order != 0 && order != 3) || (order == 3 && !w)) return -1;
    if (nin < 1 || nout < 1 || nin > MAX_AXIS || nout > MAX_AXIS) return -2;
    const double zr = nout > 1 ? (double)(nin - 1) / (double)(nout - 1) : 1.0;
    for (int o = 0; o < nout; ++o) {
        const double cc = (double)o * zr;
        const bool ok = !(cc > (double)(nin - 1));
        valid[o] = ok ? 1 : 0;
        if (order == 0) { idx[o] = ok ? (int)std::floor(cc + 0.5) : 0; continue; }
        for (int l = 0; l < 4; ++l) { idx[o * 4 + l] = 0; w[o * 4 + l] = 0.0; }
        if (!ok) continue;
        const double fl = std::floor(cc);
        const int start = (int)fl - 1, s2 = 2 * nin - 2;
        for (int l = 0; l < 4; ++l) {          // mirror about 0 and nin - 1, period 2 (nin - 1)
            int t = start + l;
            if (nin <= 1) t = 0;
            else {
                if (t < 0) t = -t;
                t %= s2;
                if (t >= nin) t = s2 - t;
            }
            idx[o * 4 + l] = t;
        }
        const double y = cc - fl, u = 1.0 - y;          // get_spline_interpolation_weights, order 3
        double* q = w + o * 4;
        q[1] = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0;
        q[2] = (u * u * (u - 2.0) * 3.0 + 4.0) / 6.0;
        q[0] = u * u * u / 6.0;
        q[3] = 1.0 - q[0] - q[1] - q[2];
    }
    return 0;
}

int pn2_zoom_workspace(int N, int H, int W, long long* bytes) {
    if (!bytes) return -1;
    if (!axes_ok(N, H, W)) return -2;
    *bytes = 2ll * N * H * W * (long long)sizeof(double);
    return 0;
}

int pn2_zoom_prefilter(const float* src, int N, int H, int W, void* work, void* stream) {
    if (!src || !work) return -1;
    if (!axes_ok(N, H, W)) return -2;
    hipStream_t st = (hipStream_t)stream;
    double* B = (double*)work;
    double* A = B + (size_t)N * H * W;
    const double gain = filter_gain();
    const long long b0 = (long long)N * ((W + 63) / 64), b1 = (long long)N * ((H + 63) / 64);
    if (b0 > 0x7fffffffll || b1 > 0x7fffffffll) return -2;
    // axis 0: lines along H, lanes on x; the result lands in B as [N][W][H]
    hipLaunchKernelGGL(spline_causal_k<float>, dim3((unsigned)b0), dim3(64), 0, st, src, A, H, W, (W + 63) / 64, ZP, gain, std::pow(ZP, (double)(H - 1)));
    PN2_CHECK_LAUNCH();
    hipLaunchKernelGGL(spline_anticausal_t_k, dim3((unsigned)b0), dim3(64), 0, st, (const double*)A, B, H, W, (W + 63) / 64, ZP);
    PN2_CHECK_LAUNCH();
    // axis 1: lines along W of the transposed planes, lanes on y; the transposed store gives [N][H][W] back
    hipLaunchKernelGGL(spline_causal_k<double>, dim3((unsigned)b1), dim3(64), 0, st, (const double*)B, A, W, H, (H + 63) / 64, ZP, gain, std::pow(ZP, (double)(W - 1)));
    PN2_CHECK_LAUNCH();
    hipLaunchKernelGGL(spline_anticausal_t_k, dim3((unsigned)b1), dim3(64), 0, st, (const double*)A, B, W, H, (H + 63) / 64, ZP);
    PN2_CHECK_LAUNCH();
    return 0;
}

int pn2_zoom3_gather(const double* coef, int N, int H, int W, int OH, int OW, const int* iy_dev, const double* wy_dev, const int* vy_dev, const int* ix_dev,
                     const double* wx_dev, const int* vx_dev, float* out, void* stream) {
    if (!coef || !iy_dev || !wy_dev || !vy_dev || !ix_dev || !wx_dev || !vx_dev || !out) return -1;
    if (!axes_ok(N, H, W) || !axes_ok(N, OH, OW)) return -2;
    const size_t total = (size_t)N * OH * OW;
    hipLaunchKernelGGL(zoom3_gather_k, dim3(grid_of(total)), dim3(256), 0, (hipStream_t)stream, coef, H, W, OH, OW, iy_dev, wy_dev, vy_dev, ix_dev, wx_dev, vx_dev, out, total);
    PN2_CHECK_LAUNCH();
    return 0;
}

int pn2_zoom0(int elem, const void* src, int N, int H, int W, int OH, int OW, const int* iy_dev, const int* vy_dev, const int* ix_dev, const int* vx_dev, void* out,
              void* stream) {
    if (!src || !iy_dev || !vy_dev || !ix_dev || !vx_dev || !out) return -1;
    if (!axes_ok(N, H, W) || !axes_ok(N, OH, OW)) return -2;
    const size_t total = (size_t)N * OH * OW;
    return with_elem(elem, [&](auto t) {
        using T = type_of<decltype(t)>;
        hipLaunchKernelGGL(zoom0_k<T>, dim3(grid_of(total)), dim3(256), 0, (hipStream_t)stream, (const T*)src, H, W, OH, OW, iy_dev, vy_dev, ix_dev, vx_dev, (T*)out, total);
        PN2_CHECK_LAUNCH();
        return 0;
    });
}

int pn2_rotate0(int elem, const void* src, int N, int H, int W, const double* m6_dev, void* out, void* stream) {
    if (!src || !m6_dev || !out) return -1;
    if (!axes_ok(N, H, W)) return -2;
    const size_t total = (size_t)N * H * W;
    return with_elem(elem, [&](auto t) {
        using T = type_of<decltype(t)>;
        hipLaunchKernelGGL(rotate0_k<T>, dim3(grid_of(total)), dim3(256), 0, (hipStream_t)stream, (const T*)src, H, W, m6_dev, (T*)out, total);
        PN2_CHECK_LAUNCH();
        return 0;
    });
}

int pn2_rot_flip(int elem, const void* src, int N, int S, const int* kaxis_dev, void* out, void* stream) {
    if (!src || !kaxis_dev || !out) return -1;
    if (!axes_ok(N, S, S)) return -2;
    const size_t total = (size_t)N * S * S;
    return with_elem(elem, [&](auto t) {
        using T = type_of<decltype(t)>;
        hipLaunchKernelGGL(rot_flip_k<T>, dim3(grid_of(total)), dim3(256), 0, (hipStream_t)stream, (const T*)src, S, kaxis_dev, (T*)out, total);
        PN2_CHECK_LAUNCH();
        return 0;
    });
}

}  // extern "C"
