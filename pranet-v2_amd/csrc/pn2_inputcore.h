// pn2_inputcore.h - the device arithmetic that the per-image input transform (pn2_resize_u8_pass x2 -> pn2_u8_to_tensor) and the ragged-batch transform
// (pn2_input_batch_width / pn2_input_batch_height, pn2_input.hip) must agree on bit for bit.  Each expression is written ONCE here and inlined into both paths.
// The tap sum is integer arithmetic (exact in any order: bilinear taps are non-negative and sum to 2^22, so 255 * sum < 2^31); the two fp32 operations of
// ToTensor / Normalize are true divisions, which no contraction can change.  The augmented width pass (pn2_input_batch_width_aug) adds one variant of the tap sum
// that reads its pixels through a 16.16 fixed-point map (rs_tap_sum_map over rs_map_px); rounding, clipping and stores are the ones below.
#pragma once
#include "pn2_common.h"

constexpr int RS_PREC = 32 - 8 - 2;          // Pillow's PRECISION_BITS: 22 fractional bits per tap

// acc[b] = 2^21 + sum over x < n of s[x * stride + b] * k[x], for the NB adjacent bytes b of one tap position (the channels of a pixel, or a run of a row).
// WIDE: s + x * stride is 4-byte aligned for every x and NB is a multiple of 4 - the run is read as dwords.
template <int NB, bool WIDE>
__device__ __forceinline__ void rs_tap_sum(int (&acc)[NB], const unsigned char* __restrict__ s, int stride, const int* __restrict__ k, int n) {
    static_assert(!WIDE || NB % 4 == 0, "a wide run is whole dwords");
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = 1 << (RS_PREC - 1);
    for (int x = 0; x < n; ++x, s += stride) {
        const int kx = k[x];
        if constexpr (WIDE) {
#pragma unroll
            for (int w = 0; w < NB / 4; ++w) {
                const unsigned v = reinterpret_cast<const unsigned*>(s)[w];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[4 * w + j] += (int)((v >> (8 * j)) & 255u) * kx;
            }
        } else {
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[b] += (int)s[b] * kx;
        }
    }
}

// The pixel a 16.16 fixed-point map sends a read to (Pillow's Geometry.c affine_fixed, nearest): px[b] = img[yy >> 16][xx >> 16][b] of the [H][W][NB] image,
// or 0 when either index is outside it.  xx / yy: the two affine sums at the pixel that is asked for.
template <int NB>
__device__ __forceinline__ void rs_map_px(int (&px)[NB], const unsigned char* __restrict__ img, int H, int W, int xx, int yy) {
    const int xin = xx >> 16, yin = yy >> 16;
    const bool in = xin >= 0 && xin < W && yin >= 0 && yin < H;
    const unsigned char* s = img + (in ? (yin * W + xin) * NB : 0);
#pragma unroll
    for (int b = 0; b < NB; ++b) px[b] = in ? (int)s[b] : 0;
}

// rs_tap_sum along a row of an image that is read through such a map: tap x multiplies the pixel the sums (xx + x * dx, yy + x * dy) select
template <int NB>
__device__ __forceinline__ void rs_tap_sum_map(int (&acc)[NB], const unsigned char* __restrict__ img, int H, int W, int xx, int yy, int dx, int dy,
                                               const int* __restrict__ k, int n) {
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = 1 << (RS_PREC - 1);
    for (int x = 0; x < n; ++x, xx += dx, yy += dy) {
        const int kx = k[x];
        int px[NB];
        rs_map_px<NB>(px, img, H, W, xx, yy);
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[b] += px[b] * kx;
    }
}

// the byte of one pass: sum >> 22, clipped to 0..255 (Resample.c clip8)
__device__ __forceinline__ unsigned char rs_byte(int acc) {
    acc >>= RS_PREC;
    return (unsigned char)(acc < 0 ? 0 : (acc > 255 ? 255 : acc));
}

// transforms.ToTensor() [+ transforms.Normalize(mean, std)] of one byte: two true fp32 divisions, as torch
__device__ __forceinline__ float u8_to_tensor(unsigned char b, bool norm, float mean, float std) {
    float t = (float)b / 255.0f;
    if (norm) t = (t - mean) / std;
    return t;
}
