// pn2_inputcore.h - the device arithmetic that the per-image input transform (pn2_resize_u8_pass x2 -> pn2_u8_to_tensor) and the ragged-batch transform
// (pn2_input_batch_width / pn2_input_batch_height, pn2_input.hip) must agree on bit for bit.  Each expression is written ONCE here and inlined into both paths.
// The tap sum is integer arithmetic (exact in any order: bilinear taps are non-negative and sum to 2^22, so 255 * sum < 2^31); the two fp32 operations of
// ToTensor / Normalize are true divisions, which no contraction can change.
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
