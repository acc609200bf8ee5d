// pn2_common.h — shared device helpers and the host launch layer of the PraNet-V2 gfx950 kernels.
// All activations are NHWC "views": base pointer (already offset to the first channel of the
// view), row = one pixel, `ld` = channel stride between consecutive pixels (elements).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "../../include/pn2.h"          // PN2_F32 / PN2_BF16 / PN2_F32F / PN2_F32X3

typedef unsigned short bf16_t;   // storage type; arithmetic always in f32
typedef __attribute__((ext_vector_type(8))) short bf16x8_t;
typedef __attribute__((ext_vector_type(4))) short s16x4_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(4))) double f64x4_t;

// storage type of PN2_F32F: a float under another name, so that the conv kernels (templated on the storage type) pick another MFMA form for it
struct f32f_t { float v; };
// storage type of PN2_F32X3: fp32 storage again; the conv kernels split the operands into bf16 terms (MMA<f32x3_t> in pn2_conv.hip)
struct f32x3_t { float v; };

__device__ __forceinline__ float bf2f(bf16_t h) { return __uint_as_float(((unsigned)h) << 16); }
__device__ __forceinline__ bf16_t f2bf(float f) {           // round-to-nearest-even, gfx950 hardware convert
    unsigned r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %1" : "=v"(r) : "v"(f));
    return (bf16_t)r;
}

template <typename T> struct TT;
template <> struct TT<float> {
    static constexpr int VEC = 4;                       // elements per 16-byte vector
    static constexpr int DT = PN2_F32;
    __device__ static __forceinline__ float ld(const float* p) { return *p; }
    __device__ static __forceinline__ void st(float* p, float v) { *p = v; }
    __device__ static __forceinline__ float round(float v) { return v; }          // the value as the storage type holds it
    __device__ static __forceinline__ void unpack(const uint4& v, float* f) {
        f[0] = __uint_as_float(v.x); f[1] = __uint_as_float(v.y); f[2] = __uint_as_float(v.z); f[3] = __uint_as_float(v.w);
    }
    __device__ static __forceinline__ uint4 pack(const float* f) {
        return make_uint4(__float_as_uint(f[0]), __float_as_uint(f[1]), __float_as_uint(f[2]), __float_as_uint(f[3]));
    }
};
template <> struct TT<f32f_t> : TT<float> {
    static constexpr int DT = PN2_F32F;
    __device__ static __forceinline__ float ld(const f32f_t* p) { return p->v; }
    __device__ static __forceinline__ void st(f32f_t* p, float v) { p->v = v; }
};
template <> struct TT<f32x3_t> : TT<float> {
    static constexpr int DT = PN2_F32X3;
    __device__ static __forceinline__ float ld(const f32x3_t* p) { return p->v; }
    __device__ static __forceinline__ void st(f32x3_t* p, float v) { p->v = v; }
};
template <> struct TT<bf16_t> {
    static constexpr int VEC = 8;
    static constexpr int DT = PN2_BF16;
    __device__ static __forceinline__ float ld(const bf16_t* p) { return bf2f(*p); }
    __device__ static __forceinline__ void st(bf16_t* p, float v) { *p = f2bf(v); }
    __device__ static __forceinline__ float round(float v) { return bf2f(f2bf(v)); }
    __device__ static __forceinline__ void unpack(const uint4& v, float* f) {
        f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xffff0000u);
        f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xffff0000u);
        f[4] = __uint_as_float(v.z << 16); f[5] = __uint_as_float(v.z & 0xffff0000u);
        f[6] = __uint_as_float(v.w << 16); f[7] = __uint_as_float(v.w & 0xffff0000u);
    }
    // gfx950 hardware convert: two f32 -> packed bf16x2, round-to-nearest-even (one VALU op per pair instead of ~12)
    __device__ static __forceinline__ unsigned cvt2(float lo, float hi) {
        unsigned r;
        asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
        return r;
    }
    __device__ static __forceinline__ uint4 pack(const float* f) {
        return make_uint4(cvt2(f[0], f[1]), cvt2(f[2], f[3]), cvt2(f[4], f[5]), cvt2(f[6], f[7]));
    }
};

// physical channel p of a group-padded layout (groups of `gw` logical channels stored in `gwp` slots)
// -> logical channel, or -1 for a pad slot.  Identity layout: gw == gwp.
__device__ __forceinline__ int phys2log(int p, int gw, int gwp, int C) {
    int g = p / gwp, o = p - g * gwp;
    int c = g * gw + o;
    return (o < gw && c < C) ? c : -1;
}

// bijective XCD-aware remap: hardware places block b on XCD b%8; give every XCD a contiguous range of logical tiles / pixel chunks so that
// neighbours (shared A rows and weight panels of the GEMMs, halo rows of the depth-wise convs) meet in one L2 instead of being fetched by several.
__device__ __forceinline__ int xcd_remap(int bid, int nblk) {
    const int q = nblk >> 3, r = nblk & 7, x = bid & 7;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (bid >> 3);
}

// flat 64-bit element index -> quotient / remainder by an int divisor, with 32-bit arithmetic whenever the index fits (a 64-bit division is ~100
// instructions on this part, and pixel decodes chain three or four of them)
__device__ __forceinline__ size_t divmod_idx(size_t idx, int d, int& rem) {
    if (idx >> 32) { const size_t q = idx / (size_t)d; rem = (int)(idx - q * (size_t)d); return q; }
    const unsigned i = (unsigned)idx, q = i / (unsigned)d;
    rem = (int)(i - q * (unsigned)d);
    return q;
}

// job lookup for the table-driven launches: largest j with bstart[j] <= b   (bstart has njobs + 1 entries)
__device__ __forceinline__ int find_job(const int* __restrict__ bstart, int njobs, int b) {
    int lo = 0, hi = njobs;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (bstart[mid] <= b) lo = mid; else hi = mid; }
    return lo;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <int CTRL> __device__ __forceinline__ float dpp_f(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
// sum over the 16 lanes of a DPP row by rotations (row_ror:8/4/2/1 fold into v_add_f32_dpp - no LDS permutes); every lane gets the total
__device__ __forceinline__ float row16_sum(float v) {
    v += dpp_f<0x128>(v); v += dpp_f<0x124>(v); v += dpp_f<0x122>(v); v += dpp_f<0x121>(v);
    return v;
}

// PyTorch upsample_bilinear2d index math (area_pixel_compute_source_index), shared by pn2_spatial.hip and the fused DSRA tail:
//   align_corners: src = r*dst ; else src = max(r*(dst+0.5)-0.5, 0) ; i0 = (int)src ; i1 = i0 + (i0 < In-1) ; l1 = src - i0.
__device__ __forceinline__ void bl_src(int o, float r, int ac, int In, int& i0, int& i1, float& l0, float& l1) {
    float s = ac ? r * (float)o : fmaxf(r * ((float)o + 0.5f) - 0.5f, 0.f);
    i0 = (int)s; if (i0 > In - 1) i0 = In - 1;
    i1 = i0 + (i0 < In - 1 ? 1 : 0);
    l1 = s - (float)i0; l0 = 1.f - l1;
}

// candidate output range whose 2-tap footprint can touch input index i (monotone src): conservative +-1, exact test in loop
__device__ __forceinline__ void bl_range(int i, float r, int ac, int On, int& lo, int& hi) {
    float a, b;
    if (ac) { if (r <= 0.f) { lo = 0; hi = On - 1; return; } a = ((float)i - 1.f) / r; b = ((float)i + 1.f) / r; }
    else { a = ((float)i - 0.5f) / r - 0.5f; b = ((float)i + 1.5f) / r - 0.5f; }
    lo = (int)floorf(a) - 1; hi = (int)ceilf(b) + 1;
    if (lo < 0) lo = 0; if (hi > On - 1) hi = On - 1;
}

#define PN2_CHECK_LAUNCH() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return (int)e_; } while (0)

// opt kernel K in to more than the default 64 KiB of dynamic LDS, once: the flag lives in a template keyed on the kernel, so every instantiation has exactly one
template <auto K>
inline void pn2_lds_opt_in(int lds_cap) {
    static bool done = false;
    if (!done) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize, lds_cap); done = true; }
}
// launch kernel K with `lds` bytes of dynamic LDS; lds_cap: the most this instantiation is ever launched with.  Returns 0 or the launch error.
template <auto K, typename... A>
inline int pn2_launch(dim3 grid, dim3 block, size_t lds, int lds_cap, hipStream_t st, const A&... args) {
    if (lds_cap > 64 * 1024) pn2_lds_opt_in<K>(lds_cap);
    hipLaunchKernelGGL(K, grid, block, lds, st, args...);
    PN2_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------------------------------------ host launch layer
// storage type handed to a with_*dtype visitor
template <typename T> struct Ty { using type = T; };
template <typename X> using type_of = typename X::type;
// compile-time int / bool handed to a generic lambda, so that one argument list serves every instantiation of a kernel
template <int N> using Int = std::integral_constant<int, N>;
template <bool B> using Bool = std::integral_constant<bool, B>;
// storage type of a PN2_* dtype code, the four codes of the conv contraction entry points: f(Ty<T>), -3 for an unknown code
template <typename F>
int with_dtype(int dtype, F f) {
    if (dtype == PN2_BF16) return f(Ty<bf16_t>{});
    if (dtype == PN2_F32) return f(Ty<float>{});
    if (dtype == PN2_F32F) return f(Ty<f32f_t>{});
    if (dtype == PN2_F32X3) return f(Ty<f32x3_t>{});
    return -3;
}
// ... of the storage-only kernels (everything but the conv contractions): bf16 and fp32, -3 for any other code
template <typename F>
int with_storage_dtype(int dtype, F f) {
    if (dtype == PN2_BF16) return f(Ty<bf16_t>{});
    if (dtype == PN2_F32) return f(Ty<float>{});
    return -3;
}
// (storage, gradient / output) pairs of the mixed-type entry points: bf16 -> bf16, bf16 -> fp32, fp32 -> fp32; f(Ty<T>, Ty<Tg>), -3 for any other pair
template <typename F>
int with_dtype_pair(int dt, int dt_g, F f) {
    if (dt == PN2_BF16 && dt_g == PN2_BF16) return f(Ty<bf16_t>{}, Ty<bf16_t>{});
    if (dt == PN2_BF16 && dt_g == PN2_F32) return f(Ty<bf16_t>{}, Ty<float>{});
    if (dt == PN2_F32 && dt_g == PN2_F32) return f(Ty<float>{}, Ty<float>{});
    return -3;
}
// run-time int that takes one of a few values -> f(Int<N>{}) for the first N that equals it, for the LAST one otherwise (the `default:` rung: the callers' range
// checks come first).  with_int<1, 2, 3, 4>(P, f) instantiates f for exactly the four listed values
template <int N0, int... Ns, typename F>
int with_int(int v, F f) {
    if constexpr (sizeof...(Ns) > 0) { if (v != N0) return with_int<Ns...>(v, f); }
    return f(Int<N0>{});
}
// elements per 16-byte vector of a dtype code.  An unknown code counts as bf16 (8) ON PURPOSE: the entry points test alignment (-2) before they
// dispatch on the dtype (-3), so this answer decides which of the two a call with a bad dtype and a misaligned shape gets
inline int vec_of(int dt) { return dt == PN2_F32 ? 4 : 8; }
inline int pow2ceil(int v) { int p = 1; while (p < v) p <<= 1; return p; }
// rows per block of the "256 threads = cvp channel vectors x R row lanes, a lane walks rows" kernels: ~1024 blocks (4 per CU), a multiple of R, between
// min_mult * R and (max_mult > 0) max_mult * R rows.  With scalar parameter loads every block paid a ~60-instruction prologue and 512 blocks was the
// optimum; with the 16-byte parameter loads the step time is flat from 768 up (15.59 / 15.57 / 15.51 / 15.51 / 15.49 ms at 384 / 512 / 768 / 1024 / 2048)
inline void rows_walk_geometry(int M, int CV, int min_mult, int max_mult, int& cvp, int& rows_per_blk, int& nblk) {
    cvp = pow2ceil(CV); if (cvp > 256) cvp = 256;
    const int R = 256 / cvp;
    constexpr int target = 1024;         // workgroups of a streaming pass (swept 256 .. 2048: flat up to 512 per pass kind)
    const int want = (M + target - 1) / target;
    rows_per_blk = ((want + R - 1) / R) * R;
    if (rows_per_blk < min_mult * R) rows_per_blk = min_mult * R;
    if (max_mult > 0 && rows_per_blk > max_mult * R) rows_per_blk = max_mult * R;
    nblk = (M + rows_per_blk - 1) / rows_per_blk;
}
// arguments of a table-driven launch (pn2_*_multi): device job table, njobs + 1 prefix sums, counts
inline bool table_ok(const void* jobs_dev, const int* block_start_dev, int njobs, int total_blocks) { return jobs_dev && block_start_dev && njobs >= 1 && total_blocks >= 1; }
namespace pn2_host {
// workgroups of a grid-stride kernel with 256 threads per element: ceil(total / 256) in [1, cap]
inline int grid_for(size_t total, int cap) { size_t g = (total + 255) / 256; return (int)(g > (size_t)cap ? cap : (g < 1 ? 1 : g)); }
}
