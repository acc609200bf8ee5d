// pn2_input.hip - the input transform of binary_seg/utils/dataloader.py:104-111 / :176-181 on the device:
//   transforms.Resize((S, S))  = PIL.Image.resize(BILINEAR): separable antialiased triangle filter, uint8 after each pass, 22-bit fixed-point taps
//   transforms.ToTensor()      = uint8 HWC -> float32 CHW / 255
//   transforms.Normalize(m, s) = (t - m) / s
// Bit-exact with Pillow (the taps are computed on the host in double exactly as Pillow's precompute_coeffs / normalize_coeffs_8bpc do).
#include <cmath>
#include <cstdint>
#include "pn2_common.h"
#include "pn2_inputcore.h"
#include "../../include/pn2.h"

namespace {

// one separable pass: dst[o][i][c] = clip8((2^21 + sum_x src[..][xmin[o] + x][..] * kk[o][x]) >> 22) along `axis` (1: width, 0: height)
__global__ __launch_bounds__(256) void resize_pass_k(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, int H, int W, int C, int out_size, int axis,
                                                     const int* __restrict__ xmin, const int* __restrict__ cnt, const int* __restrict__ kk, int ksize) {
    const int OH = axis == 0 ? out_size : H, OW = axis == 1 ? out_size : W;
    const size_t total = (size_t)OH * OW * C;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % C), ox = (int)((i / C) % OW), oy = (int)(i / ((size_t)C * OW));
        const int o = axis == 1 ? ox : oy;
        const int x0 = xmin[o];
        int acc[1];
        rs_tap_sum<1, false>(acc, axis == 1 ? src + ((size_t)oy * W + x0) * C + c : src + ((size_t)x0 * W + ox) * C + c, axis == 1 ? C : W * C, kk + (size_t)o * ksize, cnt[o]);
        dst[i] = rs_byte(acc[0]);
    }
}

// ToTensor (+ Normalize when mean/std are given): dst[c][y][x] = (src[y][x][c] / 255 - mean[c]) / std[c]   (true fp32 divisions, as torch)
__global__ __launch_bounds__(256) void to_tensor_k(const unsigned char* __restrict__ src, float* __restrict__ dst, int H, int W, int C, const float* __restrict__ mean,
                                                   const float* __restrict__ std) {
    const size_t total = (size_t)H * W * C;
    const bool norm = mean != nullptr;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int x = (int)(i % W), y = (int)((i / W) % H), c = (int)(i / ((size_t)W * H));
        dst[i] = u8_to_tensor(src[((size_t)y * W + x) * C + c], norm, norm ? mean[c] : 0.f, norm ? std[c] : 1.f);
    }
}

// ------------------------------------------------------------------------------------------------ ragged batch
// Both passes give a thread PN2_INPUT_PX adjacent output pixels of one row (4 or 12 bytes); the index arithmetic inside a slot is 32-bit (the entries refuse a
// slot of 2^31 bytes).  `wide`: out_size is a multiple of 4 and every base is aligned, so a thread's run of the [.][S][C] scratch image starts on a dword.
constexpr int PX = PN2_INPUT_PX;

// width pass of one slot: src [H][W][C] -> tmp [H][S][C]; a copy where W == S (Pillow skips that pass)
// AUG: the slot's row of the second table is given, and in its mode 1 every source pixel is read through the map (rs_map_px / rs_tap_sum_map)
template <int C, bool AUG>
__device__ __forceinline__ void width_slot(const pn2_input_slot& r, const pn2_input_aug& g, int local, int S, const unsigned char* __restrict__ src,
                                           unsigned char* __restrict__ tmp, const int* __restrict__ taps, bool wide) {
    const int G = (S + PX - 1) / PX;
    if (local >= r.H * G) return;
    const int y = local / G, px0 = (local - y * G) * PX;
    const unsigned char* srow = src + r.src + y * r.W * C;
    unsigned char b[PX * C];
    bool mapped = false;
    if constexpr (AUG) mapped = g.mode != 0;
    if (mapped) {
        if constexpr (AUG) {
            const unsigned char* img = src + r.src;
            const int a0 = g.a[0], a3 = g.a[3];
            const int xx0 = g.a[2] + g.a[1] * y, yy0 = g.a[5] + g.a[4] * y;          // the two sums at column 0 of this row
            if (r.W == S) {
#pragma unroll
                for (int p = 0; p < PX; ++p)
                    if (px0 + p < S) {
                        int px[C];
                        rs_map_px<C>(px, img, r.H, r.W, xx0 + a0 * (px0 + p), yy0 + a3 * (px0 + p));
#pragma unroll
                        for (int c = 0; c < C; ++c) b[p * C + c] = (unsigned char)px[c];
                    }
            } else {
                const int* xmin = taps + r.tap_w;
                const int* cnt = xmin + S;
                const int* kk = cnt + S;
#pragma unroll
                for (int p = 0; p < PX; ++p)
                    if (px0 + p < S) {
                        const int ox = px0 + p, x0 = xmin[ox];
                        int acc[C];
                        rs_tap_sum_map<C>(acc, img, r.H, r.W, xx0 + a0 * x0, yy0 + a3 * x0, a0, a3, kk + ox * r.kw, cnt[ox]);
#pragma unroll
                        for (int c = 0; c < C; ++c) b[p * C + c] = rs_byte(acc[c]);
                    }
            }
        }
    } else if (r.W == S) {
#pragma unroll
        for (int p = 0; p < PX; ++p)
            if (px0 + p < S) {
#pragma unroll
                for (int c = 0; c < C; ++c) b[p * C + c] = srow[(px0 + p) * C + c];
            }
    } else {
        const int* xmin = taps + r.tap_w;
        const int* cnt = xmin + S;
        const int* kk = cnt + S;
#pragma unroll
        for (int p = 0; p < PX; ++p)
            if (px0 + p < S) {
                const int ox = px0 + p;          // xmin / count: read once per output column
                int acc[C];
                rs_tap_sum<C, false>(acc, srow + xmin[ox] * C, C, kk + ox * r.kw, cnt[ox]);
#pragma unroll
                for (int c = 0; c < C; ++c) b[p * C + c] = rs_byte(acc[c]);
            }
    }
    unsigned char* d = tmp + r.tmp + (y * S + px0) * C;
    if (wide) {
#pragma unroll
        for (int w = 0; w < C; ++w)
            reinterpret_cast<unsigned*>(d)[w] = (unsigned)b[4 * w] | ((unsigned)b[4 * w + 1] << 8) | ((unsigned)b[4 * w + 2] << 16) | ((unsigned)b[4 * w + 3] << 24);
    } else {
#pragma unroll
        for (int p = 0; p < PX; ++p)
            if (px0 + p < S) {
#pragma unroll
                for (int c = 0; c < C; ++c) d[p * C + c] = b[p * C + c];
            }
    }
}

template <bool AUG>
__global__ __launch_bounds__(256) void input_batch_width_k(const pn2_input_slot* __restrict__ table, const pn2_input_aug* __restrict__ aug, int n, int S,
                                                           const unsigned char* __restrict__ src, unsigned char* __restrict__ tmp, const int* __restrict__ taps, int wide) {
    // the slot of this block: the last one whose first block is <= blockIdx.x (empty slots own no block and share the next slot's prefix)
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].blk <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const pn2_input_slot r = table[lo];
    if (r.H <= 0) return;
    const int local = ((int)blockIdx.x - r.blk) * 256 + (int)threadIdx.x;
    pn2_input_aug g = {};
    if constexpr (AUG) g = aug[lo];
    if (r.C == 3) width_slot<3, AUG>(r, g, local, S, src, tmp, taps, wide != 0);
    else width_slot<1, AUG>(r, g, local, S, src, tmp, taps, wide != 0);
}

// height pass of one slot fused with ToTensor / Normalize: tmp [H][S][C] -> out [C][S][S] fp32; the byte of resize_pass_k is formed and never stored
template <int C, bool WIDE>
__device__ __forceinline__ void height_slot(const pn2_input_slot& r, int local, int S, const unsigned char* __restrict__ tmp, const int* __restrict__ taps,
                                            float* __restrict__ out, const float* __restrict__ mean, const float* __restrict__ std) {
    const int G = (S + PX - 1) / PX;
    if (local >= S * G) return;
    const int oy = local / G, px0 = (local - oy * G) * PX;
    const int pitch = S * C;
    const unsigned char* t = tmp + r.tmp + px0 * C;
    unsigned char b[PX * C];
    if (r.H == S) {
        t += oy * pitch;
        if constexpr (WIDE) {
#pragma unroll
            for (int w = 0; w < C; ++w) {
                const unsigned v = reinterpret_cast<const unsigned*>(t)[w];
#pragma unroll
                for (int j = 0; j < 4; ++j) b[4 * w + j] = (unsigned char)((v >> (8 * j)) & 255u);
            }
        } else {
#pragma unroll
            for (int p = 0; p < PX; ++p)
                if (px0 + p < S) {
#pragma unroll
                    for (int c = 0; c < C; ++c) b[p * C + c] = t[p * C + c];
                }
        }
    } else {
        const int* xmin = taps + r.tap_h;
        const int* cnt = xmin + S;
        const int* k = cnt + S + oy * r.kh;
        const int n = cnt[oy];
        t += xmin[oy] * pitch;
        if constexpr (WIDE) {
            int acc[PX * C];
            rs_tap_sum<PX * C, true>(acc, t, pitch, k, n);
#pragma unroll
            for (int i = 0; i < PX * C; ++i) b[i] = rs_byte(acc[i]);
        } else {
#pragma unroll
            for (int p = 0; p < PX; ++p)
                if (px0 + p < S) {
                    int acc[C];
                    rs_tap_sum<C, false>(acc, t + p * C, pitch, k, n);
#pragma unroll
                    for (int c = 0; c < C; ++c) b[p * C + c] = rs_byte(acc[c]);
                }
        }
    }
    const bool norm = r.norm != 0;
    float* o = out + (size_t)r.dst * C * S * S + oy * S + px0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float m = norm ? mean[c] : 0.f, s = norm ? std[c] : 1.f;
        if constexpr (WIDE) {
            *reinterpret_cast<float4*>(o + c * S * S) = make_float4(u8_to_tensor(b[c], norm, m, s), u8_to_tensor(b[C + c], norm, m, s), u8_to_tensor(b[2 * C + c], norm, m, s),
                                                                   u8_to_tensor(b[3 * C + c], norm, m, s));
        } else {
#pragma unroll
            for (int p = 0; p < PX; ++p)
                if (px0 + p < S) o[c * S * S + p] = u8_to_tensor(b[p * C + c], norm, m, s);
        }
    }
}

template <bool WIDE>
__global__ __launch_bounds__(256) void input_batch_height_k(const pn2_input_slot* __restrict__ table, int S, int bps, const unsigned char* __restrict__ tmp,
                                                            const int* __restrict__ taps, float* __restrict__ out_rgb, float* __restrict__ out_mask,
                                                            const float* __restrict__ mean, const float* __restrict__ std) {
    const int slot = (int)blockIdx.x / bps;          // every slot has the same S x S outputs: bps blocks each
    const pn2_input_slot r = table[slot];
    if (r.H <= 0) return;
    const int local = ((int)blockIdx.x - slot * bps) * 256 + (int)threadIdx.x;
    if (r.C == 3) height_slot<3, WIDE>(r, local, S, tmp, taps, out_rgb, mean, std);
    else height_slot<1, WIDE>(r, local, S, tmp, taps, out_mask, mean, std);
}

inline long long slot_blocks(int rows, int S) { return ((long long)rows * ((S + PX - 1) / PX) + 255) / 256; }

// HOST check of a batch's table, before anything is launched.  Sizes < 0: that arena is not used by the calling pass and its offsets are not checked.
int check_table(const pn2_input_slot* t, int n, int S, long long src_bytes, long long tmp_bytes, long long tap_ints, int n_rgb, int n_mask, bool outputs,
                long long* width_blocks, bool* aligned4) {
    if ((long long)S * S * 3 > INT_MAX) return -2;
    long long blk = 0;
    *aligned4 = true;
    for (int i = 0; i < n; ++i) {
        const pn2_input_slot& r = t[i];
        if (r.H < 0 || (r.H > 0 && r.W < 1)) return -1;
        if (r.blk != blk) return -3;
        if (r.H == 0) continue;
        if (r.C != 1 && r.C != 3) return -2;
        const long long nsrc = (long long)r.H * r.W * r.C, ntmp = (long long)r.H * S * r.C;
        if (nsrc > INT_MAX || ntmp > INT_MAX) return -2;
        if (src_bytes >= 0 && (r.src < 0 || r.src > src_bytes - nsrc)) return -3;
        if (r.tmp < 0 || r.tmp > tmp_bytes - ntmp) return -3;
        if (r.tmp & 3) *aligned4 = false;
        const long long blkw = 2LL * S + (long long)S * r.kw, blkh = 2LL * S + (long long)S * r.kh;
        if (src_bytes >= 0 && r.W != S && (r.kw != pn2_resize_ksize(r.W, S) || r.tap_w < 0 || r.tap_w > tap_ints - blkw)) return -3;
        if (outputs && r.H != S && (r.kh != pn2_resize_ksize(r.H, S) || r.tap_h < 0 || r.tap_h > tap_ints - blkh)) return -3;
        if (outputs && (r.dst < 0 || r.dst >= (r.C == 3 ? n_rgb : n_mask))) return -3;
        blk += slot_blocks(r.H, S);
        if (blk > INT_MAX) return -2;
    }
    *width_blocks = blk;
    return 0;
}

// HOST check of the second table of pn2_input_batch_width_aug.
// Why PN2_INPUT_AUG_MAX_AXIS = 16384.  Image.rotate's matrix is m0 = m4 = c, m1 = -m3 = s with |c|, |s| <= 1 (cos and sin rounded to 15 decimals) and
// m2 = W/2 - c * W/2 - s * H/2, so the real sum at (x, y) is v = c * (x + 1/2 - W/2) + s * (y + 1/2 - H/2) + W/2 (the halves are the ones FIX folds into a2), and
// for 0 <= x <= W, 0 <= y <= H (the kernel's running sums stop one step past the last column):  |v| <= (W + 1)/2 + (H + 1)/2 + W/2 <= 1.5 B + 1  for axes <= B.
// The integers are a_i = 65536 * m_i + e_i with |e_i| <= 1/2 (FIX rounds; the doubles of m2 add < 1e-5), so |a2 + a0 x + a1 y| <= 65536 * (1.5 B + 1) + (1 + W + H)/2
// <= 65536 * (1.5 B + 2), and this is < 2^31 = 65536 * 32768 for B = 16384 (24578 < 32768).  The other sum is the same with W and H exchanged.  The flips are
// the exact integer substitutions x -> W-1-x, y -> H-1-y: the folded integers take the same values on the same set of pixels, the folded a2 / a5 are the sums at a
// corner pixel, and every partial sum the kernel forms (a2 + a1 y, then + a0 x) is the sum at a pixel of that set.  B = 32768 is not safe: at 45 degrees the sum at a
// corner is 65536 * (1/2 + 0.7071) * 32768 > 2^31.  Pillow itself leaves this arithmetic for a slower one where |v| >= 32768; below B = 16384 it never does.
// A table from elsewhere gets the direct test: the sums are affine in (x, y), so their values at the four corners bound them over the slot.
int check_aug(const pn2_input_slot* t, const pn2_input_aug* g, int n) {
    for (int i = 0; i < n; ++i) {
        if (g[i].mode != 0 && g[i].mode != 1) return -3;
        if (g[i].mode == 0 || t[i].H == 0) continue;
        if (t[i].H > PN2_INPUT_AUG_MAX_AXIS || t[i].W > PN2_INPUT_AUG_MAX_AXIS) return -2;
        for (int k = 0; k < 6; k += 3)
            for (int corner = 0; corner < 4; ++corner) {
                const long long dx = (long long)g[i].a[k] * ((corner & 1) ? t[i].W : 0), dy = (long long)g[i].a[k + 1] * ((corner & 2) ? t[i].H : 0);
                const long long v = (long long)g[i].a[k + 2] + dx + dy;
                if (dx != (int)dx || dy != (int)dy || v != (int)v) return -2;
            }
    }
    return 0;
}

// the width pass behind both entry points (their null checks are done); AUG: every slot reads its source through its row of the second table
template <bool AUG>
int input_batch_width(Bool<AUG>, const pn2_input_slot* table_host, const pn2_input_slot* table_dev, const pn2_input_aug* aug_host, const pn2_input_aug* aug_dev, int n,
                      int out_size, const unsigned char* src, long long src_bytes, unsigned char* tmp, long long tmp_bytes, const int* taps, long long tap_ints, void* stream) {
    if (n == 0) return 0;
    long long blocks = 0;
    bool aligned4 = false;
    if constexpr (AUG) if (int rc = check_aug(table_host, aug_host, n)) return rc;
    if (int rc = check_table(table_host, n, out_size, src_bytes, tmp_bytes, tap_ints, 0, 0, false, &blocks, &aligned4)) return rc;
    if (blocks == 0) return 0;          // every slot is empty
    const int wide = out_size % 4 == 0 && aligned4 && ((uintptr_t)tmp & 3) == 0;
    return pn2_launch<input_batch_width_k<AUG>>(dim3((unsigned)blocks), dim3(256), 0, 0, (hipStream_t)stream, table_dev, aug_dev, n, out_size, src, tmp, taps, wide);
}

}  // namespace

extern "C" {

int pn2_resize_ksize(int in_size, int out_size) {
    if (in_size < 1 || out_size < 1) return -1;
    double fs = (double)in_size / out_size; if (fs < 1.0) fs = 1.0;
    return (int)std::ceil(1.0 * fs) * 2 + 1;
}

/* HOST: the bilinear taps of one axis exactly as Pillow computes them (Resample.c precompute_coeffs + normalize_coeffs_8bpc):
 * xmin[out_size], count[out_size], kk[out_size][pn2_resize_ksize(in_size, out_size)] int32 fixed point (22 fractional bits) */
int pn2_resize_coeffs(int in_size, int out_size, int* xmin, int* count, int* kk) {
    if (!xmin || !count || !kk) return -1;
    const int ksize = pn2_resize_ksize(in_size, out_size);
    if (ksize < 0) return -1;
    const double scale = (double)in_size / out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale, support = 1.0 * filterscale, ss = 1.0 / filterscale;
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = (xx + 0.5) * scale;
        int lo = (int)(center - support + 0.5); if (lo < 0) lo = 0;
        int hi = (int)(center + support + 0.5); if (hi > in_size) hi = in_size;
        const int n = hi - lo;
        double w[64 * 1024 / 8]; double ww = 0.0;
        if (n > (int)(sizeof(w) / sizeof(w[0]))) return -2;
        for (int x = 0; x < n; ++x) {
            double a = (x + lo - center + 0.5) * ss; if (a < 0.0) a = -a;
            w[x] = a < 1.0 ? 1.0 - a : 0.0;
            ww += w[x];
        }
        int* k = kk + (size_t)xx * ksize;
        for (int x = 0; x < ksize; ++x) k[x] = 0;
        for (int x = 0; x < n; ++x) {
            const double v = (ww != 0.0 ? w[x] / ww : w[x]);
            k[x] = v < 0 ? (int)(-0.5 + v * (1 << RS_PREC)) : (int)(0.5 + v * (1 << RS_PREC));
        }
        xmin[xx] = lo; count[xx] = n;
    }
    return 0;
}

/* one pass of PIL.Image.resize(BILINEAR) on a device uint8 [H][W][C] image: axis 1 -> [H][out_size][C], axis 0 -> [out_size][W][C];
 * xmin / count / kk: DEVICE copies of pn2_resize_coeffs(axis length, out_size).  Pillow's order is width first, then height. */
int pn2_resize_u8_pass(const unsigned char* src, unsigned char* dst, int H, int W, int C, int out_size, int axis, const int* xmin_dev, const int* count_dev,
                       const int* kk_dev, int ksize, void* stream) {
    if (!src || !dst || !xmin_dev || !count_dev || !kk_dev || H < 1 || W < 1 || C < 1 || out_size < 1 || (axis != 0 && axis != 1)) return -1;
    const size_t total = (size_t)(axis == 0 ? out_size : H) * (axis == 1 ? out_size : W) * C;
    return pn2_launch<resize_pass_k>(dim3(pn2_host::grid_for(total, 8192)), dim3(256), 0, 0, (hipStream_t)stream, src, dst, H, W, C, out_size, axis, xmin_dev, count_dev, kk_dev, ksize);
}

/* transforms.ToTensor() [+ transforms.Normalize(mean, std) when mean != NULL]: uint8 [H][W][C] -> fp32 [C][H][W] (one sample of the NCHW batch) */
int pn2_u8_to_tensor(const unsigned char* src, float* dst, int H, int W, int C, const float* mean_dev, const float* std_dev, void* stream) {
    if (!src || !dst || H < 1 || W < 1 || C < 1 || ((mean_dev == nullptr) != (std_dev == nullptr))) return -1;
    return pn2_launch<to_tensor_k>(dim3(pn2_host::grid_for((size_t)H * W * C, 8192)), dim3(256), 0, 0, (hipStream_t)stream, src, dst, H, W, C, mean_dev, std_dev);
}

int pn2_input_batch_blocks(int rows, int out_size) {
    if (rows < 0 || out_size < 1) return -1;
    const long long b = slot_blocks(rows, out_size);
    return b > INT_MAX ? -1 : (int)b;
}

/* width pass of a ragged batch: ONE launch, src arena -> scratch arena [H][S][C] per slot */
int pn2_input_batch_width(const pn2_input_slot* table_host, const pn2_input_slot* table_dev, int n, int out_size, const unsigned char* src, long long src_bytes,
                          unsigned char* tmp, long long tmp_bytes, const int* taps, long long tap_ints, void* stream) {
    if (!table_host || !table_dev || !src || !tmp || !taps || n < 0 || out_size < 1 || src_bytes < 0 || tmp_bytes < 0 || tap_ints < 0) return -1;
    return input_batch_width(Bool<false>{}, table_host, table_dev, nullptr, nullptr, n, out_size, src, src_bytes, tmp, tmp_bytes, taps, tap_ints, stream);
}

/* the same launch with every source pixel of a mode-1 slot read through the slot's map: rotation and flips never materialise */
int pn2_input_batch_width_aug(const pn2_input_slot* table_host, const pn2_input_slot* table_dev, const pn2_input_aug* aug_host, const pn2_input_aug* aug_dev, int n,
                              int out_size, const unsigned char* src, long long src_bytes, unsigned char* tmp, long long tmp_bytes, const int* taps,
                              long long tap_ints, void* stream) {
    if (!table_host || !table_dev || !aug_host || !aug_dev || !src || !tmp || !taps || n < 0 || out_size < 1 || src_bytes < 0 || tmp_bytes < 0 || tap_ints < 0) return -1;
    return input_batch_width(Bool<true>{}, table_host, table_dev, aug_host, aug_dev, n, out_size, src, src_bytes, tmp, tmp_bytes, taps, tap_ints, stream);
}

/* height pass + ToTensor + Normalize of a ragged batch: ONE launch, scratch arena -> out_rgb [n_rgb][3][S][S] / out_mask [n_mask][1][S][S] fp32 */
int pn2_input_batch_height(const pn2_input_slot* table_host, const pn2_input_slot* table_dev, int n, int out_size, const unsigned char* tmp, long long tmp_bytes,
                           const int* taps, long long tap_ints, float* out_rgb, int n_rgb, float* out_mask, int n_mask, const float* mean_dev, const float* std_dev,
                           void* stream) {
    if (!table_host || !table_dev || !tmp || !taps || !mean_dev || !std_dev || n < 0 || out_size < 1 || tmp_bytes < 0 || tap_ints < 0 || n_rgb < 0 || n_mask < 0 ||
        (n_rgb > 0 && !out_rgb) || (n_mask > 0 && !out_mask))
        return -1;
    if (n == 0) return 0;
    long long blocks = 0;
    bool aligned4 = false;
    const int rc = check_table(table_host, n, out_size, -1, tmp_bytes, tap_ints, n_rgb, n_mask, true, &blocks, &aligned4);
    if (rc) return rc;
    if (blocks == 0) return 0;
    const long long bps = slot_blocks(out_size, out_size);
    if (bps * n > INT_MAX) return -2;
    const bool wide = out_size % 4 == 0 && aligned4 && ((uintptr_t)tmp & 3) == 0 && ((uintptr_t)out_rgb & 15) == 0 && ((uintptr_t)out_mask & 15) == 0;
    return with_int<1, 0>(wide, [&](auto wd) {
        return pn2_launch<input_batch_height_k<decltype(wd)::value != 0>>(dim3((unsigned)(bps * n)), dim3(256), 0, 0, (hipStream_t)stream, table_dev, out_size, (int)bps, tmp, taps, out_rgb,
                                                                          out_mask, mean_dev, std_dev);
    });
}

}  // extern "C"
