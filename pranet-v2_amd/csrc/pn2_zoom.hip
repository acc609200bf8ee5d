// pn2_zoom.hip - what the Synapse loader and test_single_volume do to a slice with scipy (multiclass_seg/EMCAD/utils/dataset_synapse.py:12-47,
// utils/utils.py:179-181,197-198), on the device and bit for bit:
//   scipy.ndimage.zoom(order=3)   = cubic B-spline prefilter (float64, axis 0 then axis 1, mirror boundaries) + 16-tap gather, cast to float32
//   scipy.ndimage.zoom(order=0)   = nearest sample, floor(cc + 0.5)
//   ndimage.rotate(order=0, reshape=False), np.flip(np.rot90(a, k), axis)
// with scipy's defaults mode='constant', cval=0, grid_mode=False: an output coordinate cc = o * ((nin-1)/(nout-1)) that exceeds nin-1 in double gives 0.
// Every float64 operation is the one ni_splines.c / ni_interpolation.c perform, in their order; scipy's build has no fused multiply-add, so contraction is off
// for this whole file (hipcc contracts a + b*c by default).  The coordinate tables and z^(n-1) are computed on the host in double (pn2_zoom_tables,
// pn2_zoom_pole_pow), so no device pow / floor of a product decides a bit.
// The pn2_ragged_* half serves batches whose samples each have their own [H][W] (the ACDC slices: dataset_ACDC.py:13-48, MIST/ACDC_train_test.py:48-93) from one
// host-built descriptor table, with the same line bodies and the same host tables, so the same bits.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>
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
// The body of one line, shared by the uniform and the ragged kernels: at(i) is sample i of the line as a double, d its first output, Cn the output pitch.
template <typename L>
__device__ __forceinline__ void causal_line(L at, double* __restrict__ d, int R, int Cn, double z, double gain, double zn) {
    if (R == 1) { d[0] = at(0); return; }          // scipy skips an axis of length 1 (no gain either)
    double c0 = at(0) * gain + zn * (at(R - 1) * gain);
    double zi = z;
#pragma unroll 8
    for (int i = 1; i < R - 1; ++i) {          // zi turns denormal near i = 540 and zero near 566: the loop runs on as scipy's does
        const double a = at(i) * gain, b = at(R - 1 - i) * gain;
        c0 = c0 + zi * (a + zn * b);
        zi = zi * z;
    }
    c0 = c0 / (1.0 - zn * zn);
    d[0] = c0;
#pragma unroll 8
    for (int i = 1; i < R; ++i) {
        c0 = at(i) * gain + z * c0;
        d[(size_t)i * Cn] = c0;
    }
}

template <typename TS>
__global__ __launch_bounds__(64) void spline_causal_k(const TS* __restrict__ src, double* __restrict__ dst, int R, int Cn, int nb, double z, double gain, double zn) {
    const int n = blockIdx.x / nb, c = (blockIdx.x - n * nb) * 64 + threadIdx.x;
    if (c >= Cn) return;
    const TS* s = src + (size_t)n * R * Cn + c;
    causal_line([=](int i) { return (double)s[(size_t)i * Cn]; }, dst + (size_t)n * R * Cn + c, R, Cn, z, gain, zn);
}

// ---- second half: anticausal initialisation and sweep, from the last row down, written TRANSPOSED: dst is [N][Cn][R].  The next axis then runs through the
// same two kernels with lanes on consecutive addresses again, and its own transposed store restores [N][H][W].  A block's 64 lines x 32 rows go through an
// LDS tile of 33 doubles per line: the column-wise ds_write_b64 of the sweep then falls on banks 2 * lane mod 32 (2 lanes per bank and half wave, the rate
// of an 8-byte store anyway; 32 doubles per line would put all 64 lanes on one bank), and the row-wise ds_read_b64 of the store takes 64 consecutive dwords
// per half wave.  Each half wave stores 256 contiguous bytes.
// The body of one block, shared by the uniform and the ragged kernels: sp / dn are the [R][Cn] source and the [Cn][R] destination plane of the block's sample, cb its
// first column.
__device__ __forceinline__ void anticausal_t_lines(const double* __restrict__ sp, double* __restrict__ dn, int R, int Cn, int cb, double z, double (*tile)[TR + 1]) {
    const int tid = threadIdx.x, c = cb + tid;
    const bool live = c < Cn;
    const double* s = sp + (live ? c : 0);
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

__global__ __launch_bounds__(64) void spline_anticausal_t_k(const double* __restrict__ src, double* __restrict__ dst, int R, int Cn, int nb, double z) {
    __shared__ double tile[64][TR + 1];
    const int n = blockIdx.x / nb;
    anticausal_t_lines(src + (size_t)n * R * Cn, dst + (size_t)n * R * Cn, R, Cn, (blockIdx.x - n * nb) * 64, z, tile);
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

// ================================================================================================ ragged batches (pn2_ragged_*): every sample its own [H][W]
// Element (i, j) of sample d AFTER its geometry (shape gh x gw), read from the source: the index map of rot_flip_k for any H x W (odd k: gh = W, gw = H), the
// nearest-sample map of rotate0_k with 0 outside, or the element itself.  Raw bits either way, so this equals materialising the augmented plane first.
template <typename T>
__device__ __forceinline__ T geom_load(const T* __restrict__ s, const pn2_ragged_desc& d, int i, int j) {
    if (d.geom == 1) {
        if (d.axis == 0) i = d.gh - 1 - i; else if (d.axis == 1) j = d.gw - 1 - j;
        int si = i, sj = j;                                      // rot90(a, 1)[i][j] = a[j][W-1-i], rot90(a, 3)[i][j] = a[H-1-j][i]
        if (d.k == 1) { si = j; sj = d.W - 1 - i; }
        else if (d.k == 2) { si = d.H - 1 - i; sj = d.W - 1 - j; }
        else if (d.k == 3) { si = d.H - 1 - j; sj = i; }
        return s[(size_t)si * d.W + sj];
    }
    if (d.geom == 2) {
        const double cy = (d.m6[4] + (double)i * d.m6[0]) + (double)j * d.m6[1];
        const double cx = (d.m6[5] + (double)i * d.m6[2]) + (double)j * d.m6[3];
        if (cy >= 0.0 && cy <= (double)(d.H - 1) && cx >= 0.0 && cx <= (double)(d.W - 1))
            return s[(size_t)floor(cy + 0.5) * d.W + (size_t)floor(cx + 0.5)];
        return (T)0;
    }
    return s[(size_t)i * d.W + j];
}

// Block b of a prefilter pass -> (sample, 64-line tile) through the pass's prefix table (a sample that is a plain copy has no blocks).
// AXIS 0: lines along gh, lanes on the gw columns, the fp32 source read through the geometry map.  AXIS 1: lines along gw of the transposed plane [gw][gh].
template <int AXIS>
__global__ __launch_bounds__(64) void ragged_causal_k(const float* __restrict__ src, const double* __restrict__ plane, double* __restrict__ dst,
                                                      const pn2_ragged_desc* __restrict__ descs, const int* __restrict__ bstart, int N, double z, double gain) {
    const int n = find_job(bstart, N, (int)blockIdx.x);
    const pn2_ragged_desc d = descs[n];
    const int R = AXIS == 0 ? d.gh : d.gw, Cn = AXIS == 0 ? d.gw : d.gh;
    const int c = ((int)blockIdx.x - bstart[n]) * 64 + (int)threadIdx.x;
    if (c >= Cn) return;
    double* o = dst + d.work_off + c;
    if (AXIS == 0) {
        const float* s = src + d.src_off;
        causal_line([&](int i) { return (double)geom_load(s, d, i, c); }, o, R, Cn, z, gain, d.zn0);
    } else {
        const double* s = plane + d.work_off + c;
        causal_line([=](int i) { return s[(size_t)i * Cn]; }, o, R, Cn, z, gain, d.zn1);
    }
}

template <int AXIS>
__global__ __launch_bounds__(64) void ragged_anticausal_t_k(const double* __restrict__ src, double* __restrict__ dst, const pn2_ragged_desc* __restrict__ descs,
                                                            const int* __restrict__ bstart, int N, double z) {
    __shared__ double tile[64][TR + 1];
    const int n = find_job(bstart, N, (int)blockIdx.x);          // uniform over the block: every thread reaches the barriers of the body
    const pn2_ragged_desc* d = descs + n;
    const int R = AXIS == 0 ? d->gh : d->gw, Cn = AXIS == 0 ? d->gw : d->gh;
    anticausal_t_lines(src + d->work_off, dst + d->work_off, R, Cn, ((int)blockIdx.x - bstart[n]) * 64, z, tile);
}

// order 3 of sample blockIdx.y: the sum of zoom3_gather_k with the sample's own tables, or the geometry map alone where the sample is a copy
__global__ __launch_bounds__(256) void ragged_zoom3_k(const float* __restrict__ src, const double* __restrict__ work, const pn2_ragged_desc* __restrict__ descs,
                                                      const double* __restrict__ tab, float* __restrict__ out) {
    const pn2_ragged_desc d = descs[blockIdx.y];
    const int total = d.oh * d.ow;
    const float* s = src + d.src_off;
    float* o = out + d.out_off;
    const double* p = work + d.work_off;
    const double* wy = tab + d.ty3;
    const double* wx = tab + d.tx3;
    const int* iy = (const int*)(wy + 4 * d.oh);
    const int* ix = (const int*)(wx + 4 * d.ow);
    for (int i = (int)blockIdx.x * 256 + (int)threadIdx.x; i < total; i += (int)gridDim.x * 256) {
        const int oy = i / d.ow, ox = i - oy * d.ow;
        float r = 0.0f;
        if (d.copy) r = geom_load(s, d, oy, ox);
        else if (iy[oy * 4] >= 0 && ix[ox * 4] >= 0) {
            double t = 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double* row = p + (size_t)iy[oy * 4 + j] * d.gw;
                const double wj = wy[oy * 4 + j];
#pragma unroll
                for (int k = 0; k < 4; ++k) t = t + (row[ix[ox * 4 + k]] * wj) * wx[ox * 4 + k];
            }
            r = (float)t;
        }
        o[i] = r;
    }
}

// order 0 of sample blockIdx.y, u8: out[y][x] = geometry map at (iy[y], ix[x]), 0 where either coordinate lies past the last sample
__global__ __launch_bounds__(256) void ragged_zoom0_k(const uint8_t* __restrict__ src, const pn2_ragged_desc* __restrict__ descs, const double* __restrict__ tab,
                                                      uint8_t* __restrict__ out) {
    const pn2_ragged_desc d = descs[blockIdx.y];
    const int total = d.oh * d.ow;
    const uint8_t* s = src + d.lab_off;
    uint8_t* o = out + d.out_off;
    const int* iy = (const int*)(tab + d.ty0);
    const int* ix = (const int*)(tab + d.tx0);
    for (int i = (int)blockIdx.x * 256 + (int)threadIdx.x; i < total; i += (int)gridDim.x * 256) {
        int oy = i / d.ow, ox = i - oy * d.ow;
        bool ok = true;
        if (!d.copy) { oy = iy[oy]; ox = ix[ox]; ok = oy >= 0 && ox >= 0; }
        o[i] = ok ? geom_load(s, d, oy, ox) : (uint8_t)0;
    }
}

// one block per sample: |pred != 0 and gt != 0|, |pred != 0|, |gt != 0| of its oh * ow bytes (at most 2^20: the sums fit an int)
__global__ __launch_bounds__(256) void ragged_dice_k(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ gt, const pn2_ragged_desc* __restrict__ descs,
                                                     long long* __restrict__ counts) {
    __shared__ int part[4][3];
    const pn2_ragged_desc* d = descs + blockIdx.x;
    const int total = d->oh * d->ow;
    const uint8_t* p = pred + d->out_off;
    const uint8_t* g = gt + d->out_off;
    int v[3] = {0, 0, 0};
    for (int i = (int)threadIdx.x; i < total; i += 256) {
        const int a = p[i] != 0, b = g[i] != 0;
        v[0] += a & b; v[1] += a; v[2] += b;
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[q] += __shfl_xor(v[q], o);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][q] = v[q];
    }
    __syncthreads();
    if (threadIdx.x < 3) counts[(size_t)blockIdx.x * 3 + threadIdx.x] = (long long)part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
}

inline bool axes_ok(int N, int H, int W) { return N >= 1 && H >= 1 && W >= 1 && H <= MAX_AXIS && W <= MAX_AXIS && (long long)N * H * W < (1ll << 40); }

template <typename F>
int with_elem(int elem, F f) {
    if (elem == 1) return f(Ty<uint8_t>{});
    if (elem == 4) return f(Ty<uint32_t>{});
    return -3;
}

constexpr int RAGGED_MAGIC = 0x52474431;
// 8-byte units of one axis table in a plan: order 3 = 4 doubles + 4 ints per output index, order 0 = one int
inline int table_units(int nout, int order) { return order == 3 ? 6 * nout : (nout + 1) / 2; }
inline std::mutex& ragged_mutex() { static std::mutex m; return m; }

// The table of one (nin, nout, order) in the plan's layout, from pn2_zoom_tables; kept for the life of the process (the caller holds ragged_mutex)
const std::vector<double>& ragged_table(int nin, int nout, int order) {
    static std::map<std::tuple<int, int, int>, std::vector<double>> cache;
    const auto key = std::make_tuple(nin, nout, order);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    const int per = order == 3 ? 4 : 1;
    std::vector<int> idx((size_t)nout * per), valid((size_t)nout);
    std::vector<double> w((size_t)nout * 4);
    pn2_zoom_tables(nin, nout, order, idx.data(), w.data(), valid.data());
    std::vector<double> t((size_t)table_units(nout, order), 0.0);
    int* ti = (int*)(t.data() + (order == 3 ? 4 * nout : 0));
    if (order == 3) std::memcpy(t.data(), w.data(), sizeof(double) * 4 * (size_t)nout);
    for (int o = 0; o < nout; ++o) {
        for (int l = 0; l < per; ++l) ti[o * per + l] = idx[o * per + l];
        if (!valid[o]) ti[o * per] = -1;
    }
    return cache.emplace(key, std::move(t)).first->second;
}

inline bool header_ok(const pn2_ragged_header* h) {
    return h->magic == RAGGED_MAGIC && h->N >= 1 && h->N <= PN2_RAGGED_MAX_N && h->blocks0 >= 0 && h->blocks1 >= 0 && (h->blocks0 == 0) == (h->blocks1 == 0) &&
           h->max_out >= 1 && h->max_out <= MAX_AXIS * MAX_AXIS && h->desc_off == (int)sizeof(pn2_ragged_header);
}
inline unsigned ragged_grid_x(const pn2_ragged_header* h) { const int g = (h->max_out + 255) / 256; return (unsigned)(g > 1024 ? 1024 : g); }

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
    if (int rc = pn2_launch<spline_causal_k<float>>(dim3((unsigned)b0), dim3(64), 0, 0, st, src, A, H, W, (W + 63) / 64, ZP, gain, std::pow(ZP, (double)(H - 1)))) return rc;
    if (int rc = pn2_launch<spline_anticausal_t_k>(dim3((unsigned)b0), dim3(64), 0, 0, st, (const double*)A, B, H, W, (W + 63) / 64, ZP)) return rc;
    // axis 1: lines along W of the transposed planes, lanes on y; the transposed store gives [N][H][W] back
    if (int rc = pn2_launch<spline_causal_k<double>>(dim3((unsigned)b1), dim3(64), 0, 0, st, (const double*)B, A, W, H, (H + 63) / 64, ZP, gain, std::pow(ZP, (double)(W - 1)))) return rc;
    return pn2_launch<spline_anticausal_t_k>(dim3((unsigned)b1), dim3(64), 0, 0, st, (const double*)A, B, W, H, (H + 63) / 64, ZP);
}

int pn2_zoom3_gather(const double* coef, int N, int H, int W, int OH, int OW, const int* iy_dev, const double* wy_dev, const int* vy_dev, const int* ix_dev,
                     const double* wx_dev, const int* vx_dev, float* out, void* stream) {
    if (!coef || !iy_dev || !wy_dev || !vy_dev || !ix_dev || !wx_dev || !vx_dev || !out) return -1;
    if (!axes_ok(N, H, W) || !axes_ok(N, OH, OW)) return -2;
    const size_t total = (size_t)N * OH * OW;
    return pn2_launch<zoom3_gather_k>(dim3(pn2_host::grid_for(total, 16384)), dim3(256), 0, 0, (hipStream_t)stream, coef, H, W, OH, OW, iy_dev, wy_dev, vy_dev, ix_dev, wx_dev, vx_dev, out, total);
}

int pn2_zoom0(int elem, const void* src, int N, int H, int W, int OH, int OW, const int* iy_dev, const int* vy_dev, const int* ix_dev, const int* vx_dev, void* out,
              void* stream) {
    if (!src || !iy_dev || !vy_dev || !ix_dev || !vx_dev || !out) return -1;
    if (!axes_ok(N, H, W) || !axes_ok(N, OH, OW)) return -2;
    const size_t total = (size_t)N * OH * OW;
    return with_elem(elem, [&](auto t) {
        using T = type_of<decltype(t)>;
        return pn2_launch<zoom0_k<T>>(dim3(pn2_host::grid_for(total, 16384)), dim3(256), 0, 0, (hipStream_t)stream, (const T*)src, H, W, OH, OW, iy_dev, vy_dev, ix_dev, vx_dev, (T*)out, total);
    });
}

int pn2_rotate0(int elem, const void* src, int N, int H, int W, const double* m6_dev, void* out, void* stream) {
    if (!src || !m6_dev || !out) return -1;
    if (!axes_ok(N, H, W)) return -2;
    const size_t total = (size_t)N * H * W;
    return with_elem(elem, [&](auto t) {
        using T = type_of<decltype(t)>;
        return pn2_launch<rotate0_k<T>>(dim3(pn2_host::grid_for(total, 16384)), dim3(256), 0, 0, (hipStream_t)stream, (const T*)src, H, W, m6_dev, (T*)out, total);
    });
}

int pn2_rot_flip(int elem, const void* src, int N, int S, const int* kaxis_dev, void* out, void* stream) {
    if (!src || !kaxis_dev || !out) return -1;
    if (!axes_ok(N, S, S)) return -2;
    const size_t total = (size_t)N * S * S;
    return with_elem(elem, [&](auto t) {
        using T = type_of<decltype(t)>;
        return pn2_launch<rot_flip_k<T>>(dim3(pn2_host::grid_for(total, 16384)), dim3(256), 0, 0, (hipStream_t)stream, (const T*)src, S, kaxis_dev, (T*)out, total);
    });
}

// ---- ragged batches: the planner (host only) and the launchers
int pn2_ragged_plan_bound(int N, const pn2_ragged_sample* samples, long long* bytes) {
    if (!samples || !bytes) return -1;
    if (N < 1 || N > PN2_RAGGED_MAX_N) return -2;
    long long b = (long long)sizeof(pn2_ragged_header) + (long long)N * sizeof(pn2_ragged_desc) + 8ll * (N + 1);
    for (int n = 0; n < N; ++n) {
        const pn2_ragged_sample& s = samples[n];
        if (s.oh < 1 || s.ow < 1 || s.oh > MAX_AXIS || s.ow > MAX_AXIS) return -2;
        b += 8ll * (table_units(s.oh, 3) + table_units(s.ow, 3) + table_units(s.oh, 0) + table_units(s.ow, 0));
    }
    *bytes = b;
    return 0;
}

int pn2_ragged_plan(int N, const pn2_ragged_sample* samples, int packed, void* blob, long long blob_bytes) {
    if (!samples || !blob) return -1;
    if (N < 1 || N > PN2_RAGGED_MAX_N) return -2;
    for (int n = 0; n < N; ++n) {
        const pn2_ragged_sample& s = samples[n];
        if (s.H < 1 || s.W < 1 || s.oh < 1 || s.ow < 1 || s.H > MAX_AXIS || s.W > MAX_AXIS || s.oh > MAX_AXIS || s.ow > MAX_AXIS) return -2;
        if (s.geom < 0 || s.geom > 2 || (s.geom == 1 && (s.k < 0 || s.k > 3 || s.axis < -1 || s.axis > 1))) return -3;
    }
    pn2_ragged_header h = {};
    h.magic = RAGGED_MAGIC;
    h.N = N;
    h.desc_off = (int)sizeof(pn2_ragged_header);
    h.bs0_off = h.desc_off + N * (int)sizeof(pn2_ragged_desc);
    h.bs1_off = h.bs0_off + 4 * (N + 1);
    h.tab_off = h.bs1_off + 4 * (N + 1);          // 8 (N + 1) bytes of prefix tables: the table area stays 8-byte aligned
    h.uniform_out = 1;
    std::vector<pn2_ragged_desc> descs((size_t)N);
    std::vector<int> bs0((size_t)N + 1, 0), bs1((size_t)N + 1, 0);
    std::vector<double> tab;
    std::map<std::tuple<int, int, int>, int> placed;          // (nin, nout, order) -> offset in this blob: samples of equal axes share one table
    std::lock_guard<std::mutex> lock(ragged_mutex());
    auto place = [&](int nin, int nout, int order) {
        const auto key = std::make_tuple(nin, nout, order);
        auto it = placed.find(key);
        if (it != placed.end()) return it->second;
        const std::vector<double>& t = ragged_table(nin, nout, order);
        const int off = (int)tab.size();
        tab.insert(tab.end(), t.begin(), t.end());
        placed[key] = off;
        return off;
    };
    long long src = 0, work = 0, out = 0;
    for (int n = 0; n < N; ++n) {
        const pn2_ragged_sample& s = samples[n];
        pn2_ragged_desc& d = descs[n];
        d = pn2_ragged_desc{};
        const bool swap = s.geom == 1 && (s.k & 1);
        d.H = s.H; d.W = s.W; d.gh = swap ? s.W : s.H; d.gw = swap ? s.H : s.W; d.oh = s.oh; d.ow = s.ow;
        d.geom = s.geom; d.k = s.geom == 1 ? s.k : 0; d.axis = s.geom == 1 ? s.axis : -1;
        d.copy = d.gh == d.oh && d.gw == d.ow;
        d.src_off = packed ? src : s.src_off;
        d.lab_off = packed ? src : s.lab_off;
        d.out_off = out;
        d.work_off = work;
        d.zn0 = std::pow(ZP, (double)(d.gh - 1));
        d.zn1 = std::pow(ZP, (double)(d.gw - 1));
        if (s.geom == 2) for (int q = 0; q < 6; ++q) d.m6[q] = s.m6[q];
        bs0[n + 1] = bs0[n]; bs1[n + 1] = bs1[n];
        if (!d.copy) {
            d.ty3 = place(d.gh, d.oh, 3); d.tx3 = place(d.gw, d.ow, 3);
            d.ty0 = place(d.gh, d.oh, 0); d.tx0 = place(d.gw, d.ow, 0);
            bs0[n + 1] += (d.gw + 63) / 64; bs1[n + 1] += (d.gh + 63) / 64;
            work += (long long)d.gh * d.gw;
        }
        src += (long long)s.H * s.W;
        out += (long long)s.oh * s.ow;
        if (s.oh * s.ow > h.max_out) h.max_out = s.oh * s.ow;
        if (s.oh != samples[0].oh || s.ow != samples[0].ow) h.uniform_out = 0;
    }
    h.blocks0 = bs0[N]; h.blocks1 = bs1[N];
    h.ntables = (int)placed.size();
    h.work_doubles = work; h.src_elems = packed ? src : 0; h.out_elems = out;
    h.bytes = (long long)h.tab_off + 8ll * (long long)tab.size();
    if (h.bytes > blob_bytes) return -4;
    char* b = (char*)blob;
    std::memcpy(b, &h, sizeof h);
    std::memcpy(b + h.desc_off, descs.data(), (size_t)N * sizeof(pn2_ragged_desc));
    std::memcpy(b + h.bs0_off, bs0.data(), 4 * ((size_t)N + 1));
    std::memcpy(b + h.bs1_off, bs1.data(), 4 * ((size_t)N + 1));
    if (!tab.empty()) std::memcpy(b + h.tab_off, tab.data(), 8 * tab.size());
    return 0;
}

int pn2_ragged_prefilter(const float* src, const void* plan_host, const void* plan_dev, void* work, void* stream) {
    if (!src || !plan_host || !plan_dev) return -1;
    const pn2_ragged_header* h = (const pn2_ragged_header*)plan_host;
    if (!header_ok(h)) return -2;
    if (h->blocks0 == 0) return 0;          // every sample is already at its output size
    if (!work) return -1;
    const char* pd = (const char*)plan_dev;
    const pn2_ragged_desc* descs = (const pn2_ragged_desc*)(pd + h->desc_off);
    const int* bs0 = (const int*)(pd + h->bs0_off);
    const int* bs1 = (const int*)(pd + h->bs1_off);
    hipStream_t st = (hipStream_t)stream;
    double* B = (double*)work;
    double* A = B + h->work_doubles;
    const double gain = filter_gain();
    // the passes of pn2_zoom_prefilter, each sample on its own lines: axis 0 lands in B as [gw][gh], axis 1 restores [gh][gw]
    if (int rc = pn2_launch<ragged_causal_k<0>>(dim3((unsigned)h->blocks0), dim3(64), 0, 0, st, src, (const double*)nullptr, A, descs, bs0, h->N, ZP, gain)) return rc;
    if (int rc = pn2_launch<ragged_anticausal_t_k<0>>(dim3((unsigned)h->blocks0), dim3(64), 0, 0, st, (const double*)A, B, descs, bs0, h->N, ZP)) return rc;
    if (int rc = pn2_launch<ragged_causal_k<1>>(dim3((unsigned)h->blocks1), dim3(64), 0, 0, st, (const float*)nullptr, (const double*)B, A, descs, bs1, h->N, ZP, gain)) return rc;
    return pn2_launch<ragged_anticausal_t_k<1>>(dim3((unsigned)h->blocks1), dim3(64), 0, 0, st, (const double*)A, B, descs, bs1, h->N, ZP);
}

int pn2_ragged_zoom3(const float* src, const void* plan_host, const void* plan_dev, const void* work, float* out, void* stream) {
    if (!src || !plan_host || !plan_dev || !out) return -1;
    const pn2_ragged_header* h = (const pn2_ragged_header*)plan_host;
    if (!header_ok(h)) return -2;
    if (h->blocks0 != 0 && !work) return -1;
    const char* pd = (const char*)plan_dev;
    return pn2_launch<ragged_zoom3_k>(dim3(ragged_grid_x(h), (unsigned)h->N), dim3(256), 0, 0, (hipStream_t)stream, src, (const double*)work,
                                      (const pn2_ragged_desc*)(pd + h->desc_off), (const double*)(pd + h->tab_off), out);
}

int pn2_ragged_zoom0(const unsigned char* src, const void* plan_host, const void* plan_dev, unsigned char* out, void* stream) {
    if (!src || !plan_host || !plan_dev || !out) return -1;
    const pn2_ragged_header* h = (const pn2_ragged_header*)plan_host;
    if (!header_ok(h)) return -2;
    const char* pd = (const char*)plan_dev;
    return pn2_launch<ragged_zoom0_k>(dim3(ragged_grid_x(h), (unsigned)h->N), dim3(256), 0, 0, (hipStream_t)stream, src, (const pn2_ragged_desc*)(pd + h->desc_off),
                                      (const double*)(pd + h->tab_off), out);
}

int pn2_ragged_dice_counts(const unsigned char* pred, const unsigned char* gt, const void* plan_host, const void* plan_dev, long long* counts, void* stream) {
    if (!pred || !gt || !plan_host || !plan_dev || !counts) return -1;
    const pn2_ragged_header* h = (const pn2_ragged_header*)plan_host;
    if (!header_ok(h)) return -2;
    return pn2_launch<ragged_dice_k>(dim3((unsigned)h->N), dim3(256), 0, 0, (hipStream_t)stream, pred, gt, (const pn2_ragged_desc*)((const char*)plan_dev + h->desc_off), counts);
}

}  // extern "C"
