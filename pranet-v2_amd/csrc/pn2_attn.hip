// pn2_attn.hip — spatial-reduction attention of the PVTv2 encoder (the reference's binary_seg/lib/pvtv2.py, Attention.forward :90-111).
// head_dim 32 or 64.  Two families of entry points:
//   pn2_attn_fwd / _bwd            <= 256 reduced key/value tokens, all of them on chip
//   pn2_attn_long_fwd / _bwd       1..4096 keys streamed through LDS in 128-key chunks (online softmax)
// Each family has a bf16 MFMA route (every ld a multiple of 8) and a scalar route (fp32 storage, bf16 views with another ld).  What the on-chip and
// the streamed kernels share is written once where that leaves every kernel's register allocation as it was: the LDS layouts (one struct per layout,
// used by the kernel's carving and by the launcher), the bf16 K / V staging, the pieces of the MFMA forward, the key/value reduce and the host
// dispatch.  All kernels are deterministic (fixed-order reductions, no floating-point atomics).
//
// q   [B][Nq][heads*HD]                      (Attention.q)
// kv  [B][Nkv][2*heads*HD]: k of head h at columns h*HD.., v at heads*HD + h*HD..   (Attention.kv reshaped (B,-1,2,heads,HD), :98-101)
// out [B][Nq][heads*HD]  = softmax(q k^T * scale) v   with heads concatenated (:107)
// Tokens [B, N, C] of the reference are NHWC pixels here (N = H*W), so no transposes are needed anywhere.
#include <cstdint>
#include "pn2_common.h"
#include "../../include/pn2.h"

namespace {

constexpr int AT_MAXK = 4;       // keys per lane of the on-chip kernels -> Nkv <= 256
constexpr int AT_QB = 4;         // queries a wave works on at once: every K / V value read from LDS is used AT_QB times
constexpr int AT_QCHUNK = 256;   // queries per block (on-chip) / per step of a block (streamed) of the scalar backward
constexpr int AL_CK = 128;       // keys per chunk of the streamed kernels
constexpr int AL_QPB = 64;       // queries per block of the streamed scalar forward

// ------------------------------------------------------------------------------------------ scalar kernels
// One block = 4 waves for one (b, head); K^T and V^T of NP = NK * 64 keys live in LDS as [HD dims][NP + 1].  Lane d < HD of a wave owns dimension d
// of q / out (at HD = 32 the upper half-wave idles in the dimension walks); lane l owns keys l, l + 64, ... for the score / softmax part.
// LDS layouts in floats: the kernels carve with these offsets, the launchers ask bytes().
template <int HD, int NP> struct ScalarFwdLds {
    static constexpr int RS = NP + 1, Kt = 0, Vt = HD * RS, kv_end = 2 * HD * RS;
    static constexpr size_t bytes() { return (size_t)kv_end * 4; }
};
template <int HD> struct ScalarLongFwdLds : ScalarFwdLds<HD, AL_CK> {          // + the running O [AL_QPB][HD], m and l [AL_QPB] of the block's queries
    static constexpr int Os = ScalarFwdLds<HD, AL_CK>::kv_end, Ms = Os + AL_QPB * HD, Ls = Ms + AL_QPB, end = Ls + AL_QPB;
    static constexpr size_t bytes() { return (size_t)end * 4; }
};
template <int HD, int NP, int QB> struct ScalarBwdLds : ScalarFwdLds<HD, NP> {          // + P, dS [GQ][NP] and q, dO [GQ][HD] of a group of GQ = 4 * QB queries
    static constexpr int GQ = 4 * QB, Pt = ScalarFwdLds<HD, NP>::kv_end, dSt = Pt + GQ * NP, qt = dSt + GQ * NP, dot = qt + GQ * HD, end = dot + GQ * HD;
    static constexpr size_t bytes() { return (size_t)end * 4; }
};

template <typename T, int HD>
__device__ __forceinline__ void attn_stage_kv(const T* __restrict__ kv, int ld_kv, int Nkv, int NP, int heads, int h, float* Kt, float* Vt) {
    // Kt/Vt: [HD dims][NP + 1]: the odd row stride makes both walks conflict-free — lanes over keys (row d, consecutive l) and lanes
    // over dims (column l, stride NP + 1); pad keys hold zeros
    const int RS = NP + 1;
    for (int i = threadIdx.x; i < NP * HD; i += 256) {
        const int l = i / HD, d = i % HD;
        float k = 0.f, v = 0.f;
        if (l < Nkv) { k = TT<T>::ld(kv + (size_t)l * ld_kv + h * HD + d); v = TT<T>::ld(kv + (size_t)l * ld_kv + heads * HD + h * HD + d); }
        Kt[d * RS + l] = k;
        Vt[d * RS + l] = v;
    }
}

__device__ __forceinline__ float rdlane(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }

// on-chip forward: 4 queries in flight per wave, full-row softmax
template <typename T, int NK, int HD>
__global__ __launch_bounds__(256) void attn_fwd_k(const T* __restrict__ q, int ld_q, const T* __restrict__ kv, int ld_kv, T* __restrict__ out, int ld_o,
                                                  float* __restrict__ lse, int Nq, int Nkv, int heads, float scale, int q_per_blk) {
    extern __shared__ float lds[];
    typedef ScalarFwdLds<HD, NK * 64> L;
    constexpr int NP = NK * 64, RS = L::RS;
    float* Kt = lds + L::Kt; float* Vt = lds + L::Vt;
    const int b = blockIdx.z, h = blockIdx.y, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int dl = lane & (HD - 1);                                      // dimension of this lane in the dimension walks (lane < HD stores)
    attn_stage_kv<T, HD>(kv + (size_t)b * Nkv * ld_kv, ld_kv, Nkv, NP, heads, h, Kt, Vt);
    __syncthreads();
    const int q0 = blockIdx.x * q_per_blk;
    int q1 = q0 + q_per_blk; if (q1 > Nq) q1 = Nq;
    for (int qb = q0 + wid * AT_QB; qb < q1; qb += 4 * AT_QB) {
        float qd[AT_QB], s[AT_QB][NK];
#pragma unroll
        for (int i = 0; i < AT_QB; ++i) {
            const int qi = qb + i < q1 ? qb + i : q1 - 1;
            qd[i] = TT<T>::ld(q + ((size_t)b * Nq + qi) * ld_q + h * HD + dl) * scale;
#pragma unroll
            for (int k = 0; k < NK; ++k) s[i][k] = 0.f;
        }
#pragma unroll
        for (int d = 0; d < HD; ++d) {
            float kk[NK];
#pragma unroll
            for (int k = 0; k < NK; ++k) kk[k] = Kt[d * RS + k * 64 + lane];
#pragma unroll
            for (int i = 0; i < AT_QB; ++i) {
                const float qq = rdlane(qd[i], d);
#pragma unroll
                for (int k = 0; k < NK; ++k) s[i][k] += qq * kk[k];
            }
        }
        float inv[AT_QB], o_[AT_QB];
#pragma unroll
        for (int i = 0; i < AT_QB; ++i) {
            float mx = -INFINITY;
#pragma unroll
            for (int k = 0; k < NK; ++k) if (k * 64 + lane < Nkv) mx = fmaxf(mx, s[i][k]);
            for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
            float sum = 0.f;
#pragma unroll
            for (int k = 0; k < NK; ++k) { s[i][k] = (k * 64 + lane < Nkv) ? expf(s[i][k] - mx) : 0.f; sum += s[i][k]; }
            sum = wave_sum(sum);
            inv[i] = 1.f / sum; o_[i] = 0.f;
            if (lane == 0 && qb + i < q1) lse[((size_t)b * heads + h) * Nq + qb + i] = mx + logf(sum);
        }
#pragma unroll
        for (int k = 0; k < NK; ++k) {
#pragma unroll
            for (int l = 0; l < 64; ++l) {
                const float vv = Vt[dl * RS + k * 64 + l];
#pragma unroll
                for (int i = 0; i < AT_QB; ++i) o_[i] += rdlane(s[i][k], l) * vv;
            }
        }
#pragma unroll
        for (int i = 0; i < AT_QB; ++i)
            if (qb + i < q1 && lane < HD) TT<T>::st(out + ((size_t)b * Nq + qb + i) * ld_o + h * HD + lane, o_[i] * inv[i]);
    }
}

// on-chip backward.  A block owns a chunk of queries of one (b, head).  Per group of 4 x QB queries (QB per wave): phase A recomputes
// p = exp(s - lse), dP = dO V^T, dS = p (dP - sum p dP) and dq = scale dS K exactly like the forward walks K / V; P, dS, q, dO of the
// group go to LDS tiles.  Phase B: every wave owns NP/4 keys and accumulates dK / dV in registers.  Block partials [2][NP][HD] are summed
// over the query chunks by attn_bwd_kv_reduce_k.
template <typename T, int NK, int QB, int HD>
__global__ __launch_bounds__(256) void attn_bwd_k(const T* __restrict__ q, int ld_q, const T* __restrict__ kv, int ld_kv, const T* __restrict__ dout, int ld_do,
                                                  const float* __restrict__ lse, T* __restrict__ dq, int ld_dq, float* __restrict__ part,
                                                  int Nq, int Nkv, int heads, float scale) {
    extern __shared__ float lds[];
    typedef ScalarBwdLds<HD, NK * 64, QB> L;
    constexpr int NP = NK * 64, RS = L::RS, KPW = NP / 4, GQ = L::GQ;
    float* Kt = lds + L::Kt; float* Vt = lds + L::Vt;
    float* Pt = lds + L::Pt; float* dSt = lds + L::dSt; float* qt = lds + L::qt; float* dot = lds + L::dot;
    const int b = blockIdx.z, h = blockIdx.y, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int dl = lane & (HD - 1);                                      // as in attn_fwd_k: lanes >= HD compute a copy of lane - HD and store nothing
    attn_stage_kv<T, HD>(kv + (size_t)b * Nkv * ld_kv, ld_kv, Nkv, NP, heads, h, Kt, Vt);
    __syncthreads();
    const int q0 = blockIdx.x * AT_QCHUNK;
    int q1 = q0 + AT_QCHUNK; if (q1 > Nq) q1 = Nq;
    float ak[KPW], av[KPW];
#pragma unroll
    for (int j = 0; j < KPW; ++j) { ak[j] = 0.f; av[j] = 0.f; }
    for (int g0 = q0; g0 < q1; g0 += GQ) {
        const int qb = g0 + wid * QB;
        float qd[QB], dod[QB], L_[QB], s[QB][NK], dp[QB][NK];
#pragma unroll
        for (int i = 0; i < QB; ++i) {
            const bool ok = qb + i < q1;
            const int qi = ok ? qb + i : q1 - 1;
            const size_t qo = (size_t)b * Nq + qi;
            qd[i] = ok && lane < HD ? TT<T>::ld(q + qo * ld_q + h * HD + lane) * scale : 0.f;
            dod[i] = ok && lane < HD ? TT<T>::ld(dout + qo * ld_do + h * HD + lane) : 0.f;
            L_[i] = lse[((size_t)b * heads + h) * Nq + qi];
#pragma unroll
            for (int k = 0; k < NK; ++k) { s[i][k] = 0.f; dp[i][k] = 0.f; }
        }
#pragma unroll
        for (int d = 0; d < HD; ++d) {
            float kk[NK], vv[NK];
#pragma unroll
            for (int k = 0; k < NK; ++k) { kk[k] = Kt[d * RS + k * 64 + lane]; vv[k] = Vt[d * RS + k * 64 + lane]; }
#pragma unroll
            for (int i = 0; i < QB; ++i) {
                const float qq = rdlane(qd[i], d), gg = rdlane(dod[i], d);
#pragma unroll
                for (int k = 0; k < NK; ++k) { s[i][k] += qq * kk[k]; dp[i][k] += gg * vv[k]; }
            }
        }
        float dqd[QB];
#pragma unroll
        for (int i = 0; i < QB; ++i) {
            const bool ok = qb + i < q1;
            float delta = 0.f;
#pragma unroll
            for (int k = 0; k < NK; ++k) { s[i][k] = (ok && k * 64 + lane < Nkv) ? expf(s[i][k] - L_[i]) : 0.f; delta += s[i][k] * dp[i][k]; }
            delta = wave_sum(delta);
            const int row = wid * QB + i;
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                dp[i][k] = s[i][k] * (dp[i][k] - delta);          // dS
                Pt[row * NP + k * 64 + lane] = s[i][k]; dSt[row * NP + k * 64 + lane] = dp[i][k];
            }
            if (lane < HD) { qt[row * HD + lane] = qd[i]; dot[row * HD + lane] = dod[i]; }
            dqd[i] = 0.f;
        }
#pragma unroll
        for (int k = 0; k < NK; ++k) {
#pragma unroll
            for (int l = 0; l < 64; ++l) {
                const float kk = Kt[dl * RS + k * 64 + l];
#pragma unroll
                for (int i = 0; i < QB; ++i) dqd[i] += rdlane(dp[i][k], l) * kk;
            }
        }
#pragma unroll
        for (int i = 0; i < QB; ++i)
            if (qb + i < q1 && lane < HD) TT<T>::st(dq + ((size_t)b * Nq + qb + i) * ld_dq + h * HD + lane, dqd[i] * scale);
        __syncthreads();
        // phase B: this wave's keys [wid*KPW, +KPW), all queries of the group
        for (int r = 0; r < GQ; ++r) {
            const float qv = qt[r * HD + dl], gv = dot[r * HD + dl];
            const float* pr = Pt + r * NP + wid * KPW; const float* dr = dSt + r * NP + wid * KPW;
#pragma unroll
            for (int j = 0; j < KPW; ++j) { ak[j] += dr[j] * qv; av[j] += pr[j] * gv; }
        }
        __syncthreads();
    }
    float* dst = part + ((((size_t)b * heads + h) * gridDim.x + blockIdx.x) * 2) * NP * HD;
    if (lane < HD) {
#pragma unroll
        for (int j = 0; j < KPW; ++j) {
            dst[(size_t)(wid * KPW + j) * HD + lane] = ak[j];             // qd carried the softmax scale already
            dst[(size_t)NP * HD + (size_t)(wid * KPW + j) * HD + lane] = av[j];
        }
    }
}

// one block of HD threads per (key, head, b): partial [B][heads][nqb][2][NP][HD], summed in slot order.  The streamed backward calls it per key
// range with NP = AL_CK and dkv advanced to the range's first key.
template <typename T, int HD>
__global__ __launch_bounds__(HD) void attn_bwd_kv_reduce_k(const float* __restrict__ part, T* __restrict__ dkv, int ld_dkv, int Nkv, int NP, int heads, int nqb) {
    const int l = blockIdx.x, h = blockIdx.y, b = blockIdx.z, d = threadIdx.x;
    const float* p = part + (((size_t)b * heads + h) * nqb * 2) * NP * HD + (size_t)l * HD + d;
    float sk = 0.f, sv = 0.f;
    for (int c = 0; c < nqb; ++c) { sk += p[(size_t)c * 2 * NP * HD]; sv += p[(size_t)c * 2 * NP * HD + (size_t)NP * HD]; }
    T* dst = dkv + ((size_t)b * Nkv + l) * ld_dkv;
    TT<T>::st(dst + h * HD + d, sk);
    TT<T>::st(dst + heads * HD + h * HD + d, sv);
}

// ------------------------------------------------------------------------------------------ bf16 MFMA kernels
// Same math on v_mfma_f32_16x16x32_bf16; every wave owns 16 queries.
// Fragment layouts (lane l): A[l&15][(l>>4)*8 + j], B[(l>>4)*8 + j][l&15], C: column l&15, rows (l>>4)*4 + r.
// LDS tiles keep 16-byte fragment rows with an 8-element pad so the 16 lanes of a quarter-wave hit distinct banks.
typedef __attribute__((ext_vector_type(4))) float f32x4v;
__device__ __forceinline__ f32x4v mfma16(const uint4& a, const uint4& b, f32x4v c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
}

// Fragment (A[i][k] or B[k][i], i = lane & 15) of a 16-wide column block of a ROW-MAJOR LDS tile [k][col] whose rows are the contraction index,
// through the transposing LDS read: k-slot (g, j) <-> tile row (j >> 2) * 16 + g * 4 + (j & 3).  The other operand of the MFMA has to walk the
// contraction in the same order (perm_frag).  Conflict-free when the row stride is an odd multiple of 32 bytes: ATR = 80 elements for 64-wide
// rows (head_dim 64, and the 64-query tiles of the backward), 48 for 32-wide rows (head_dim 32).
constexpr int ATR = 80;
template <int HD> constexpr int at_tr() { static_assert(HD == 32 || HD == 64, "head_dim 32 or 64"); return HD == 64 ? ATR : 48; }
template <int R = ATR>
__device__ __forceinline__ uint4 tr_frag(const bf16_t* tile, int col0, int lane) {
    const int g = lane >> 4, i = lane & 15;
    unsigned a = (unsigned)(size_t)(reinterpret_cast<const char*>(tile) + (g * 4 + (i >> 2)) * (R * 2) + (col0 + (i & 3) * 4) * 2);
    asm volatile("" : "+v"(a));            // keep the tile offset out of the instruction's immediate field
    const s16x4_t v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4_t __attribute__((address_space(3)))*)(a));
    const s16x4_t v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4_t __attribute__((address_space(3)))*)(a + 16 * R * 2));
    const uint2 lo = __builtin_bit_cast(uint2, v0), hi = __builtin_bit_cast(uint2, v1);
    return make_uint4(lo.x, lo.y, hi.x, hi.y);
}
// f2bf of a value that may come straight from v_exp_f32: gfx950 needs one wait state between a transcendental's result and a VALU that reads it,
// and the compiler's hazard recognizer does not look inside inline asm (f2bf's convert), so the pad is part of the asm
__device__ __forceinline__ bf16_t f2bf_trans(float f) {
    unsigned r;
    asm("s_nop 0\n\tv_cvt_pk_bf16_f32 %0, %1, %1" : "=v"(r) : "v"(f));
    return (bf16_t)r;
}
// the matching fragment of an operand stored with the contraction index contiguous: row[k0 + g*4 .. +3] and row[k0 + 16 + g*4 .. +3]
__device__ __forceinline__ uint4 perm_frag(const bf16_t* row, int k0, int g) {
    const uint2 lo = *reinterpret_cast<const uint2*>(row + k0 + g * 4), hi = *reinterpret_cast<const uint2*>(row + k0 + 16 + g * 4);
    return make_uint4(lo.x, lo.y, hi.x, hi.y);
}

// LDS layouts in bf16 elements of NP keys on chip (kernels carve with the offsets, launchers ask bytes()).
// forward: K rows are the B operand of S = Q K^T (lane = key, 16 bytes of d), V rows that of O = P V through tr_frag (contraction = keys), the
// probabilities the A operand of O = P V (perm_frag)
template <int HD, int NP> struct MfmaFwdLds {
    static constexpr int KR = HD + 8, VR = at_tr<HD>(), PR = NP + 8;
    static constexpr int Ks = 0, Vs = Ks + NP * KR, Ps = Vs + NP * VR, end = Ps + 8 * 16 * PR;          // [NP][KR], [NP][VR], [8 waves][16][PR]
    static constexpr size_t bytes() { return (size_t)end * 2; }
};
// backward: K, V, Q and dO tiles row-major; every product whose contraction runs over tile rows (keys for dQ, queries for dK / dV) reads its B
// operand with tr_frag, so nothing is transposed
template <int HD, int NP> struct MfmaBwdLds {
    static constexpr int DR = at_tr<HD>(), VR = HD + 8, TR = NP + 8, KR = 72;
    static constexpr int Ks = 0,                    // [NP][DR]  K rows: B of S = Q K^T (16-byte reads) and of dQ = dS K (tr_frag, contraction = keys)
                         Vs = Ks + NP * DR,         // [NP][VR]  V rows: B of dP = dO V^T
                         Qs = Vs + NP * VR,         // [64][DR]  Q tile  [q][d]: A of S, B of dK (tr_frag, contraction = queries)
                         Gs = Qs + 64 * DR,         // [64][DR]  dO tile [q][d]: A of dP, B of dV
                         Sa = Gs + 64 * DR,         // [4][16][TR] dS, A layout per wave (perm_frag over keys)
                         St = Sa + 64 * TR,         // [NP][KR]  dS transposed [key][q]  (perm_frag over queries)
                         Pt = St + NP * KR,         // [NP][KR]  P transposed  [key][q]
                         end = Pt + NP * KR;
    static constexpr size_t bytes() { return (size_t)end * 2; }
};

// K / V rows [key0, key0 + NP) of head h -> LDS rows of pitch KP / VP by 16-byte copies (no transposes), NTH threads; keys >= Nkv become zero rows
template <int HD, int NP, int KP, int VP, int NTH>
__device__ __forceinline__ void attn_stage_kv_bf16(const bf16_t* kvb, int ld_kv, int Nkv, int key0, int heads, int h, bf16_t* Ks, bf16_t* Vs) {
    constexpr int CH = HD / 8, CHS = HD == 64 ? 3 : 2;          // 16-byte chunks per row, and its log2
    for (int i = threadIdx.x; i < NP * CH; i += NTH) {
        const int kl = i >> CHS, ch = i & (CH - 1), key = key0 + kl;
        uint4 kk = make_uint4(0, 0, 0, 0), vv = kk;
        if (key < Nkv) { kk = *reinterpret_cast<const uint4*>(kvb + (size_t)key * ld_kv + h * HD + ch * 8);
                         vv = *reinterpret_cast<const uint4*>(kvb + (size_t)key * ld_kv + heads * HD + h * HD + ch * 8); }
        *reinterpret_cast<uint4*>(Ks + kl * KP + ch * 8) = kk;
        *reinterpret_cast<uint4*>(Vs + kl * VP + ch * 8) = vv;
    }
}

// ---- forward pieces.  HD = 32: S = Q K^T is one MFMA per 16 x 16 tile (the whole contraction is one A fragment) and O = P V has 2 column blocks instead of 4.
// S = Q K^T of this wave's 16 queries (A fragments aq) against the NT key tiles in Ks
template <int NT, int HD, int KR>
__device__ __forceinline__ void attn_mfma_scores(const bf16_t* Ks, const uint4 (&aq)[HD / 32], int l15, int g, f32x4v (&s)[NT]) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const bf16_t* kp = Ks + (nt * 16 + l15) * KR + g * 8;
        f32x4v c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kc = 0; kc < HD / 32; ++kc) c = mfma16(aq[kc], *reinterpret_cast<const uint4*>(kp + kc * 32), c);
        s[nt] = c;
    }
}
// the probabilities (fresh from v_exp_f32) into the wave's [16][PR] tile
template <int NT, int PR>
__device__ __forceinline__ void attn_mfma_store_p(bf16_t* pw, const f32x4v (&s)[NT], int l15, int g) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) pw[(g * 4 + r) * PR + nt * 16 + l15] = f2bf_trans(s[nt][r]);
}
// o += P V over the NP keys in Vs
template <int NP, int HD, int PR, int VR>
__device__ __forceinline__ void attn_mfma_pv(const bf16_t* pw, const bf16_t* Vs, int lane, int l15, int g, f32x4v (&o)[HD / 16]) {
#pragma unroll
    for (int ks = 0; ks < NP / 32; ++ks) {
        const uint4 ap = perm_frag(pw + l15 * PR, ks * 32, g);
#pragma unroll
        for (int nd = 0; nd < HD / 16; ++nd) o[nd] = mfma16(ap, tr_frag<VR>(Vs + ks * 32 * VR, nd * 16, lane), o[nd]);
    }
}
// out = o / sum, lse = mx + log(sum) for the wave's 16 queries from q0
template <int HD>
__device__ __forceinline__ void attn_mfma_fwd_store(bf16_t* out, int ld_o, float* lse, int b, int h, int heads, int Nq, int q0, int l15, int g,
                                                    const f32x4v (&o)[HD / 16], const float (&mx)[4], const float (&sum)[4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int qi = q0 + g * 4 + r;
        if (qi < Nq) {
            const float inv = 1.f / sum[r];
            bf16_t* op = out + ((size_t)b * Nq + qi) * ld_o + h * HD + l15;
#pragma unroll
            for (int nd = 0; nd < HD / 16; ++nd) op[nd * 16] = f2bf(o[nd][r] * inv);
            if (l15 == 0) lse[((size_t)b * heads + h) * Nq + qi] = mx[r] + __logf(sum[r]);
        }
    }
}

// on-chip forward.  A block = 8 waves = 128 queries per step; K and V rows of the (b, head) are staged once and the block walks query tiles
// blockIdx.x, blockIdx.x + gridDim.x, ...  (the K/V staging of the one-tile-per-block version cost more than its MFMAs).
template <int NK, int HD>
__global__ __launch_bounds__(512) void attn_fwd_mfma_k(const bf16_t* __restrict__ q, int ld_q, const bf16_t* __restrict__ kv, int ld_kv, bf16_t* __restrict__ out, int ld_o,
                                                       float* __restrict__ lse, int Nq, int Nkv, int heads, float scale) {
    typedef MfmaFwdLds<HD, NK * 64> L;
    constexpr int NP = NK * 64, NT = NP / 16, KR = L::KR, VR = L::VR, PR = L::PR, ND = HD / 16;
    extern __shared__ __attribute__((aligned(16))) bf16_t smem[];
    bf16_t* Ks = smem + L::Ks; bf16_t* Vs = smem + L::Vs; bf16_t* Ps = smem + L::Ps;
    const int b = blockIdx.z, h = blockIdx.y, lane = threadIdx.x & 63, wid = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
    attn_stage_kv_bf16<HD, NP, KR, VR, 512>(kv + (size_t)b * Nkv * ld_kv, ld_kv, Nkv, 0, heads, h, Ks, Vs);
    __syncthreads();
    bf16_t* pw = Ps + wid * 16 * PR;
    const int ntile = (Nq + 127) / 128;
    for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const int q0 = tile * 128 + wid * 16;
        const int qa = min(q0 + l15, Nq - 1);                             // A-operand row of this lane
        const bf16_t* qp = q + ((size_t)b * Nq + qa) * ld_q + h * HD + g * 8;
        uint4 aq[HD / 32];
#pragma unroll
        for (int kc = 0; kc < HD / 32; ++kc) aq[kc] = *reinterpret_cast<const uint4*>(qp + kc * 32);
        f32x4v s[NT];
        attn_mfma_scores<NT, HD, KR>(Ks, aq, l15, g, s);
        float mx[4], sum[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float m = -INFINITY;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) { const float v = (nt * 16 + l15 < Nkv) ? s[nt][r] * scale : -INFINITY; s[nt][r] = v; m = fmaxf(m, v); }
            m = fmaxf(m, __shfl_xor(m, 1)); m = fmaxf(m, __shfl_xor(m, 2)); m = fmaxf(m, __shfl_xor(m, 4)); m = fmaxf(m, __shfl_xor(m, 8));
            float t = 0.f;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) { const float p = __expf(s[nt][r] - m); s[nt][r] = p; t += p; }
            t += __shfl_xor(t, 1); t += __shfl_xor(t, 2); t += __shfl_xor(t, 4); t += __shfl_xor(t, 8);
            mx[r] = m; sum[r] = t;
        }
        attn_mfma_store_p<NT, PR>(pw, s, l15, g);
        __syncthreads();                                                  // (every wave walks the same number of tiles)
        f32x4v o[ND];
#pragma unroll
        for (int nd = 0; nd < ND; ++nd) o[nd] = f32x4v{0.f, 0.f, 0.f, 0.f};
        attn_mfma_pv<NP, HD, PR, VR>(pw, Vs, lane, l15, g, o);
        attn_mfma_fwd_store<HD>(out, ld_o, lse, b, h, heads, Nq, q0, l15, g, o, mx, sum);
        __syncthreads();                                                  // the next tile's probabilities overwrite Ps
    }
}

// delta[b][h][q] = sum_d dO[q][h*HD + d] * O[q][h*HD + d]   (= sum_keys P dP: lets the backward treat key ranges independently)
template <typename T, int HD>
__global__ __launch_bounds__(256) void attn_delta_k(const T* __restrict__ dout, int ld_do, const T* __restrict__ o, int ld_o, float* __restrict__ delta, int B, int Nq, int heads) {
    const int lane = threadIdx.x & 63;
    const size_t item = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6), total = (size_t)B * Nq * heads;
    if (item >= total) return;
    const int h = (int)(item % heads); const size_t bq = item / heads;          // bq = b * Nq + q
    float v = lane < HD ? TT<T>::ld(dout + bq * ld_do + h * HD + lane) * TT<T>::ld(o + bq * ld_o + h * HD + lane) : 0.f;
    v = wave_sum(v);
    if (lane == 0) { const size_t b = bq / Nq, qi = bq % Nq; delta[(b * heads + h) * Nq + qi] = v; }
}

// backward for the keys [key0, key0 + NKB*64) of one (b, head); the block walks 64-query tiles blockIdx.x, blockIdx.x + gridDim.x, ...:
//   S = Q K^T, dP = dO V^T (MFMA) -> P = exp(S scale - lse), dS = P (dP - delta) scale
//   dQ (+)= dS K ; dK += dS^T Q, dV += P^T dO accumulate in registers over the tiles of the block and leave as ONE fp32 partial [2][NPT][HD]
//   per block (summed by attn_bwd_kv_reduce_k).
//   HD = 32: S and dP are one MFMA per tile, dQ / dK / dV have 2 column blocks instead of 4.
template <int NKB, int HD>
__global__ __launch_bounds__(256) void attn_bwd_mfma_k(const bf16_t* __restrict__ q, int ld_q, const bf16_t* __restrict__ kv, int ld_kv, const bf16_t* __restrict__ dout, int ld_do,
                                                       const float* __restrict__ lse, const float* __restrict__ delta, bf16_t* __restrict__ dq, int ld_dq, float* __restrict__ part,
                                                       int Nq, int Nkv, int heads, float scale, int key0, int NPT, int dq_acc) {
    typedef MfmaBwdLds<HD, NKB * 64> L;
    constexpr int NP = NKB * 64, NT = NP / 16, KR = L::KR, TR = L::TR, NKT = NT / 4, DR = L::DR, VR = L::VR, ND = HD / 16, CH = HD / 8, CHS = HD == 64 ? 3 : 2, KC = HD / 32;
    extern __shared__ __attribute__((aligned(16))) bf16_t smem[];
    bf16_t* Ks = smem + L::Ks; bf16_t* Vs = smem + L::Vs; bf16_t* Qs = smem + L::Qs; bf16_t* Gs = smem + L::Gs;
    bf16_t* Sa = smem + L::Sa; bf16_t* St = smem + L::St; bf16_t* Pt = smem + L::Pt;
    const int b = blockIdx.z, h = blockIdx.y, lane = threadIdx.x & 63, wid = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
    attn_stage_kv_bf16<HD, NP, DR, VR, 256>(kv + (size_t)b * Nkv * ld_kv, ld_kv, Nkv, key0, heads, h, Ks, Vs);
    f32x4v ak[NKT][ND], av[NKT][ND];
#pragma unroll
    for (int i = 0; i < NKT; ++i)
#pragma unroll
        for (int nd = 0; nd < ND; ++nd) { ak[i][nd] = f32x4v{0.f, 0.f, 0.f, 0.f}; av[i][nd] = ak[i][nd]; }
    bf16_t* sa = Sa + wid * 16 * TR;
    const int ntile = (Nq + 63) / 64;
    for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const int qt0 = tile * 64;
        __syncthreads();                                                  // the previous tile's readers of Qs / Gs / St / Pt are done (and K / V are in)
        for (int i = threadIdx.x; i < 64 * CH; i += 256) {
            const int ql = i >> CHS, ch = i & (CH - 1), qi = qt0 + ql;
            uint4 qq = make_uint4(0, 0, 0, 0), gg = qq;
            if (qi < Nq) { qq = *reinterpret_cast<const uint4*>(q + ((size_t)b * Nq + qi) * ld_q + h * HD + ch * 8);
                           gg = *reinterpret_cast<const uint4*>(dout + ((size_t)b * Nq + qi) * ld_do + h * HD + ch * 8); }
            *reinterpret_cast<uint4*>(Qs + ql * DR + ch * 8) = qq;
            *reinterpret_cast<uint4*>(Gs + ql * DR + ch * 8) = gg;
        }
        const int q0 = qt0 + wid * 16;
        float Lr[4], D[4]; bool rok[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int qi = q0 + g * 4 + r;
            rok[r] = qi < Nq;
            const size_t li = ((size_t)b * heads + h) * Nq + (rok[r] ? qi : Nq - 1);
            Lr[r] = lse[li]; D[r] = delta[li];
        }
        __syncthreads();
        const bf16_t* qrow = Qs + (wid * 16 + l15) * DR + g * 8; const bf16_t* grow = Gs + (wid * 16 + l15) * DR + g * 8;
        uint4 aq[KC], ag[KC];
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) aq[kc] = *reinterpret_cast<const uint4*>(qrow + kc * 32);
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) ag[kc] = *reinterpret_cast<const uint4*>(grow + kc * 32);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const bf16_t* kp = Ks + (nt * 16 + l15) * DR + g * 8; const bf16_t* vp = Vs + (nt * 16 + l15) * VR + g * 8;
            f32x4v s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kc = 0; kc < KC; ++kc) s = mfma16(aq[kc], *reinterpret_cast<const uint4*>(kp + kc * 32), s);
#pragma unroll
            for (int kc = 0; kc < KC; ++kc) dp = mfma16(ag[kc], *reinterpret_cast<const uint4*>(vp + kc * 32), dp);
            const bool kok = key0 + nt * 16 + l15 < Nkv;
            bf16_t pb[4], sb[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = (kok && rok[r]) ? __expf(s[r] * scale - Lr[r]) : 0.f;
                const float ds = p * (dp[r] - D[r]) * scale;
                pb[r] = f2bf_trans(p); sb[r] = f2bf(ds);
                sa[(g * 4 + r) * TR + nt * 16 + l15] = sb[r];
            }
            // transposed tiles [key][query]: 4 consecutive queries of this lane -> one 8-byte store each
            const int key = nt * 16 + l15, qc = wid * 16 + g * 4;
            *reinterpret_cast<uint2*>(St + key * KR + qc) = make_uint2((unsigned)sb[0] | ((unsigned)sb[1] << 16), (unsigned)sb[2] | ((unsigned)sb[3] << 16));
            *reinterpret_cast<uint2*>(Pt + key * KR + qc) = make_uint2((unsigned)pb[0] | ((unsigned)pb[1] << 16), (unsigned)pb[2] | ((unsigned)pb[3] << 16));
        }
        __syncthreads();
        // dQ = dS K  (this wave's 16 queries x HD dims, contraction over the keys of this range)
        f32x4v dqa[ND];
#pragma unroll
        for (int nd = 0; nd < ND; ++nd) dqa[nd] = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < NP / 32; ++ks) {
            const uint4 a = perm_frag(sa + l15 * TR, ks * 32, g);
#pragma unroll
            for (int nd = 0; nd < ND; ++nd) dqa[nd] = mfma16(a, tr_frag<DR>(Ks + ks * 32 * DR, nd * 16, lane), dqa[nd]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (rok[r]) {
                bf16_t* dp_ = dq + ((size_t)b * Nq + q0 + g * 4 + r) * ld_dq + h * HD + l15;
#pragma unroll
                for (int nd = 0; nd < ND; ++nd) dp_[nd * 16] = f2bf(dq_acc ? bf2f(dp_[nd * 16]) + dqa[nd][r] : dqa[nd][r]);
            }
        }
        // dK += dS^T Q, dV += P^T dO : this wave's key tiles (kt = wid, wid + 4, ...), contraction over the 64 queries of the tile
#pragma unroll
        for (int i = 0; i < NKT; ++i) {
            const int kt = wid + 4 * i;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const uint4 as = perm_frag(St + (kt * 16 + l15) * KR, ks * 32, g);
                const uint4 ap = perm_frag(Pt + (kt * 16 + l15) * KR, ks * 32, g);
#pragma unroll
                for (int nd = 0; nd < ND; ++nd) {
                    ak[i][nd] = mfma16(as, tr_frag<DR>(Qs + ks * 32 * DR, nd * 16, lane), ak[i][nd]);
                    av[i][nd] = mfma16(ap, tr_frag<DR>(Gs + ks * 32 * DR, nd * 16, lane), av[i][nd]);
                }
            }
        }
    }
    float* dst = part + ((((size_t)b * heads + h) * gridDim.x + blockIdx.x) * 2) * (size_t)NPT * HD;
#pragma unroll
    for (int i = 0; i < NKT; ++i) {
        const int kt = wid + 4 * i;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const size_t row = (size_t)(key0 + kt * 16 + g * 4 + r) * HD + l15;
#pragma unroll
            for (int nd = 0; nd < ND; ++nd) { dst[row + nd * 16] = ak[i][nd][r]; dst[(size_t)NPT * HD + row + nd * 16] = av[i][nd][r]; }
        }
    }
}

// ------------------------------------------------------------------------------------------ streamed kernels (pn2_attn_long_*)
// The keys go through LDS in chunks of AL_CK; nothing on chip grows with Nkv.  Forward: online softmax.  Per chunk, with m / l / O the running
// maximum, sum and un-normalised output of a query row:  m' = max(m, max_j s_j), a = exp(m - m') (0 for the first chunk: m = -inf, m' finite
// because only chunks with a valid key are visited), l = l a + sum_j exp(s_j - m'), O = O a + exp(s - m') V.  out = O / l, lse = m + log l at the end.

// bf16 MFMA forward: a block = 8 waves = 128 queries of one (b, head), every wave 16 of them; the chunk in the layout of attn_fwd_mfma_k<2, HD>
template <int HD>
__global__ __launch_bounds__(512) void attn_long_fwd_mfma_k(const bf16_t* __restrict__ q, int ld_q, const bf16_t* __restrict__ kv, int ld_kv, bf16_t* __restrict__ out, int ld_o,
                                                            float* __restrict__ lse, int Nq, int Nkv, int heads, float scale) {
    typedef MfmaFwdLds<HD, AL_CK> L;
    constexpr int NP = AL_CK, NT = NP / 16, KR = L::KR, VR = L::VR, PR = L::PR, ND = HD / 16;
    extern __shared__ __attribute__((aligned(16))) bf16_t smem[];
    bf16_t* Ks = smem + L::Ks; bf16_t* Vs = smem + L::Vs; bf16_t* Ps = smem + L::Ps;
    const int b = blockIdx.z, h = blockIdx.y, lane = threadIdx.x & 63, wid = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
    const bf16_t* kvb = kv + (size_t)b * Nkv * ld_kv;
    bf16_t* pw = Ps + wid * 16 * PR;
    const int q0 = blockIdx.x * 128 + wid * 16;
    const int qa = min(q0 + l15, Nq - 1);                                 // A-operand row of this lane
    const bf16_t* qp = q + ((size_t)b * Nq + qa) * ld_q + h * HD + g * 8;
    uint4 aq[HD / 32];
#pragma unroll
    for (int kc = 0; kc < HD / 32; ++kc) aq[kc] = *reinterpret_cast<const uint4*>(qp + kc * 32);
    float mrun[4], lrun[4];
    f32x4v o[ND];
#pragma unroll
    for (int r = 0; r < 4; ++r) { mrun[r] = -INFINITY; lrun[r] = 0.f; }
#pragma unroll
    for (int nd = 0; nd < ND; ++nd) o[nd] = f32x4v{0.f, 0.f, 0.f, 0.f};
    for (int key0 = 0; key0 < Nkv; key0 += NP) {                          // every visited chunk holds key0 < Nkv: at least one valid key
        if (key0) __syncthreads();                                        // the previous chunk's readers of Ks / Vs are done
        attn_stage_kv_bf16<HD, NP, KR, VR, 512>(kvb, ld_kv, Nkv, key0, heads, h, Ks, Vs);
        __syncthreads();
        f32x4v s[NT];
        attn_mfma_scores<NT, HD, KR>(Ks, aq, l15, g, s);
        float al[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float m = -INFINITY;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) { const float v = (key0 + nt * 16 + l15 < Nkv) ? s[nt][r] * scale : -INFINITY; s[nt][r] = v; m = fmaxf(m, v); }
            m = fmaxf(m, __shfl_xor(m, 1)); m = fmaxf(m, __shfl_xor(m, 2)); m = fmaxf(m, __shfl_xor(m, 4)); m = fmaxf(m, __shfl_xor(m, 8));
            m = fmaxf(m, mrun[r]);                                        // finite
            al[r] = mrun[r] == -INFINITY ? 0.f : __expf(mrun[r] - m);
            float t = 0.f;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) { const float p = __expf(s[nt][r] - m); s[nt][r] = p; t += p; }
            t += __shfl_xor(t, 1); t += __shfl_xor(t, 2); t += __shfl_xor(t, 4); t += __shfl_xor(t, 8);
            mrun[r] = m; lrun[r] = lrun[r] * al[r] + t;
        }
        attn_mfma_store_p<NT, PR>(pw, s, l15, g);
        __syncthreads();
#pragma unroll
        for (int nd = 0; nd < ND; ++nd)
#pragma unroll
            for (int r = 0; r < 4; ++r) o[nd][r] *= al[r];
        attn_mfma_pv<NP, HD, PR, VR>(pw, Vs, lane, l15, g, o);
    }
    attn_mfma_fwd_store<HD>(out, ld_o, lse, b, h, heads, Nq, q0, l15, g, o, mrun, lrun);
}

// scalar forward: the walks of attn_fwd_k over one chunk at a time.  A block = 4 waves = AL_QPB queries, a wave 16 of them in 4 groups of AT_QB; the
// running m / l / O of the block's queries live in LDS between chunks (wave-private rows).
template <typename T, int HD>
__global__ __launch_bounds__(256) void attn_long_fwd_k(const T* __restrict__ q, int ld_q, const T* __restrict__ kv, int ld_kv, T* __restrict__ out, int ld_o,
                                                       float* __restrict__ lse, int Nq, int Nkv, int heads, float scale) {
    extern __shared__ float lds[];
    typedef ScalarLongFwdLds<HD> L;
    constexpr int NK = AL_CK / 64, NP = AL_CK, RS = L::RS;
    float* Kt = lds + L::Kt; float* Vt = lds + L::Vt;
    float* Os = lds + L::Os; float* Ms = lds + L::Ms; float* Ls = lds + L::Ls;
    const int b = blockIdx.z, h = blockIdx.y, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int dl = lane & (HD - 1);
    const int q0 = blockIdx.x * AL_QPB;
    int q1 = q0 + AL_QPB; if (q1 > Nq) q1 = Nq;
    for (int i = threadIdx.x; i < AL_QPB * HD; i += 256) Os[i] = 0.f;
    if (threadIdx.x < AL_QPB) { Ms[threadIdx.x] = -INFINITY; Ls[threadIdx.x] = 0.f; }
    for (int key0 = 0; key0 < Nkv; key0 += NP) {
        __syncthreads();                                                  // the previous chunk's walks are done, its m / l / O stores visible
        attn_stage_kv<T, HD>(kv + ((size_t)b * Nkv + key0) * ld_kv, ld_kv, Nkv - key0, NP, heads, h, Kt, Vt);
        __syncthreads();
#pragma unroll 1
        for (int grp = 0; grp < 16 / AT_QB; ++grp) {
            const int ql = wid * 16 + grp * AT_QB, qb = q0 + ql;
            if (qb >= q1) break;
            float qd[AT_QB], s[AT_QB][NK];
#pragma unroll
            for (int i = 0; i < AT_QB; ++i) {
                const int qi = qb + i < q1 ? qb + i : q1 - 1;
                qd[i] = TT<T>::ld(q + ((size_t)b * Nq + qi) * ld_q + h * HD + dl) * scale;
#pragma unroll
                for (int k = 0; k < NK; ++k) s[i][k] = 0.f;
            }
#pragma unroll
            for (int d = 0; d < HD; ++d) {
                float kk[NK];
#pragma unroll
                for (int k = 0; k < NK; ++k) kk[k] = Kt[d * RS + k * 64 + lane];
#pragma unroll
                for (int i = 0; i < AT_QB; ++i) {
                    const float qq = rdlane(qd[i], d);
#pragma unroll
                    for (int k = 0; k < NK; ++k) s[i][k] += qq * kk[k];
                }
            }
            float o_[AT_QB], mn[AT_QB], ln[AT_QB];
#pragma unroll
            for (int i = 0; i < AT_QB; ++i) {
                float mx = -INFINITY;
#pragma unroll
                for (int k = 0; k < NK; ++k) if (key0 + k * 64 + lane < Nkv) mx = fmaxf(mx, s[i][k]);
                for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
                const float mo = Ms[ql + i];
                mx = fmaxf(mx, mo);                                       // finite: the chunk has a valid key
                const float al = mo == -INFINITY ? 0.f : expf(mo - mx);
                float sum = 0.f;
#pragma unroll
                for (int k = 0; k < NK; ++k) { s[i][k] = (key0 + k * 64 + lane < Nkv) ? expf(s[i][k] - mx) : 0.f; sum += s[i][k]; }
                sum = wave_sum(sum);
                mn[i] = mx; ln[i] = Ls[ql + i] * al + sum;
                o_[i] = Os[(ql + i) * HD + dl] * al;
            }
#pragma unroll
            for (int k = 0; k < NK; ++k) {
#pragma unroll
                for (int l = 0; l < 64; ++l) {
                    const float vv = Vt[dl * RS + k * 64 + l];
#pragma unroll
                    for (int i = 0; i < AT_QB; ++i) o_[i] += rdlane(s[i][k], l) * vv;
                }
            }
#pragma unroll
            for (int i = 0; i < AT_QB; ++i) {
                if (lane < HD) Os[(ql + i) * HD + lane] = o_[i];
                if (lane == 0) { Ms[ql + i] = mn[i]; Ls[ql + i] = ln[i]; }
            }
        }
    }
    __syncthreads();
    for (int ql = wid * 16; ql < wid * 16 + 16 && q0 + ql < q1; ++ql) {
        const float l = Ls[ql];
        if (lane < HD) TT<T>::st(out + ((size_t)b * Nq + q0 + ql) * ld_o + h * HD + lane, Os[ql * HD + lane] / l);
        if (lane == 0) lse[((size_t)b * heads + h) * Nq + q0 + ql] = Ms[ql] + logf(l);
    }
}

// Backward, both routes: one launch per range of AL_CK keys from lse and delta.  dQ accumulates over the ranges in an fp32 workspace
// dqw [B][Nq][heads*HD] (written by the first range, added to by the later ones: every element belongs to one block per launch) and is converted
// once by attn_long_dq_store_k.  The dK / dV partial holds ONE range, [B][heads][slots][2][AL_CK][HD], rows local to the range, and is summed in
// slot order by attn_bwd_kv_reduce_k after each launch.
//
// attn_long_bwd_mfma_k<HD> has the text of attn_bwd_mfma_k<2, HD> (same LDS layout and staging helper) and differs in where results go: dQ is
// `float* dqw`, row pitch heads * HD, fp32 `old + dqa`; the partial has slot stride 2 * AL_CK * HD and rows local to the range.  One inlined body
// behind both kernels was built and measured: at head_dim 64 it moved the register allocation of all three instantiations (194 -> 198 VGPRs at 128
// keys, 119 -> 112 at 64 keys), whatever the body shared or left out, so the two stay separate kernels.  A change to one belongs in the other.
template <int HD>
__global__ __launch_bounds__(256) void attn_long_bwd_mfma_k(const bf16_t* __restrict__ q, int ld_q, const bf16_t* __restrict__ kv, int ld_kv, const bf16_t* __restrict__ dout, int ld_do,
                                                            const float* __restrict__ lse, const float* __restrict__ delta, float* __restrict__ dqw, float* __restrict__ part,
                                                            int Nq, int Nkv, int heads, float scale, int key0, int dq_acc) {
    typedef MfmaBwdLds<HD, AL_CK> L;
    constexpr int NP = AL_CK, NT = NP / 16, KR = L::KR, TR = L::TR, NKT = NT / 4, DR = L::DR, VR = L::VR, ND = HD / 16, CH = HD / 8, CHS = HD == 64 ? 3 : 2, KC = HD / 32;
    extern __shared__ __attribute__((aligned(16))) bf16_t smem[];
    bf16_t* Ks = smem + L::Ks; bf16_t* Vs = smem + L::Vs; bf16_t* Qs = smem + L::Qs; bf16_t* Gs = smem + L::Gs;
    bf16_t* Sa = smem + L::Sa; bf16_t* St = smem + L::St; bf16_t* Pt = smem + L::Pt;
    const int b = blockIdx.z, h = blockIdx.y, lane = threadIdx.x & 63, wid = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
    attn_stage_kv_bf16<HD, NP, DR, VR, 256>(kv + (size_t)b * Nkv * ld_kv, ld_kv, Nkv, key0, heads, h, Ks, Vs);
    f32x4v ak[NKT][ND], av[NKT][ND];
#pragma unroll
    for (int i = 0; i < NKT; ++i)
#pragma unroll
        for (int nd = 0; nd < ND; ++nd) { ak[i][nd] = f32x4v{0.f, 0.f, 0.f, 0.f}; av[i][nd] = ak[i][nd]; }
    bf16_t* sa = Sa + wid * 16 * TR;
    const int ntile = (Nq + 63) / 64;
    for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const int qt0 = tile * 64;
        __syncthreads();                                                  // the previous tile's readers of Qs / Gs / St / Pt are done (and K / V are in)
        for (int i = threadIdx.x; i < 64 * CH; i += 256) {
            const int ql = i >> CHS, ch = i & (CH - 1), qi = qt0 + ql;
            uint4 qq = make_uint4(0, 0, 0, 0), gg = qq;
            if (qi < Nq) { qq = *reinterpret_cast<const uint4*>(q + ((size_t)b * Nq + qi) * ld_q + h * HD + ch * 8);
                           gg = *reinterpret_cast<const uint4*>(dout + ((size_t)b * Nq + qi) * ld_do + h * HD + ch * 8); }
            *reinterpret_cast<uint4*>(Qs + ql * DR + ch * 8) = qq;
            *reinterpret_cast<uint4*>(Gs + ql * DR + ch * 8) = gg;
        }
        const int q0 = qt0 + wid * 16;
        float Lr[4], D[4]; bool rok[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int qi = q0 + g * 4 + r;
            rok[r] = qi < Nq;
            const size_t li = ((size_t)b * heads + h) * Nq + (rok[r] ? qi : Nq - 1);
            Lr[r] = lse[li]; D[r] = delta[li];
        }
        __syncthreads();
        const bf16_t* qrow = Qs + (wid * 16 + l15) * DR + g * 8; const bf16_t* grow = Gs + (wid * 16 + l15) * DR + g * 8;
        uint4 aq[KC], ag[KC];
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) aq[kc] = *reinterpret_cast<const uint4*>(qrow + kc * 32);
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) ag[kc] = *reinterpret_cast<const uint4*>(grow + kc * 32);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const bf16_t* kp = Ks + (nt * 16 + l15) * DR + g * 8; const bf16_t* vp = Vs + (nt * 16 + l15) * VR + g * 8;
            f32x4v s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kc = 0; kc < KC; ++kc) s = mfma16(aq[kc], *reinterpret_cast<const uint4*>(kp + kc * 32), s);
#pragma unroll
            for (int kc = 0; kc < KC; ++kc) dp = mfma16(ag[kc], *reinterpret_cast<const uint4*>(vp + kc * 32), dp);
            const bool kok = key0 + nt * 16 + l15 < Nkv;
            bf16_t pb[4], sb[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = (kok && rok[r]) ? __expf(s[r] * scale - Lr[r]) : 0.f;
                const float ds = p * (dp[r] - D[r]) * scale;
                pb[r] = f2bf_trans(p); sb[r] = f2bf(ds);
                sa[(g * 4 + r) * TR + nt * 16 + l15] = sb[r];
            }
            // transposed tiles [key][query]: 4 consecutive queries of this lane -> one 8-byte store each
            const int key = nt * 16 + l15, qc = wid * 16 + g * 4;
            *reinterpret_cast<uint2*>(St + key * KR + qc) = make_uint2((unsigned)sb[0] | ((unsigned)sb[1] << 16), (unsigned)sb[2] | ((unsigned)sb[3] << 16));
            *reinterpret_cast<uint2*>(Pt + key * KR + qc) = make_uint2((unsigned)pb[0] | ((unsigned)pb[1] << 16), (unsigned)pb[2] | ((unsigned)pb[3] << 16));
        }
        __syncthreads();
        // dQ (+)= dS K in fp32
        f32x4v dqa[ND];
#pragma unroll
        for (int nd = 0; nd < ND; ++nd) dqa[nd] = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < NP / 32; ++ks) {
            const uint4 a = perm_frag(sa + l15 * TR, ks * 32, g);
#pragma unroll
            for (int nd = 0; nd < ND; ++nd) dqa[nd] = mfma16(a, tr_frag<DR>(Ks + ks * 32 * DR, nd * 16, lane), dqa[nd]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (rok[r]) {
                float* dp_ = dqw + ((size_t)b * Nq + q0 + g * 4 + r) * (heads * HD) + h * HD + l15;
#pragma unroll
                for (int nd = 0; nd < ND; ++nd) dp_[nd * 16] = dq_acc ? dp_[nd * 16] + dqa[nd][r] : dqa[nd][r];
            }
        }
        // dK += dS^T Q, dV += P^T dO : this wave's key tiles (kt = wid, wid + 4, ...), contraction over the 64 queries of the tile
#pragma unroll
        for (int i = 0; i < NKT; ++i) {
            const int kt = wid + 4 * i;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const uint4 as = perm_frag(St + (kt * 16 + l15) * KR, ks * 32, g);
                const uint4 ap = perm_frag(Pt + (kt * 16 + l15) * KR, ks * 32, g);
#pragma unroll
                for (int nd = 0; nd < ND; ++nd) {
                    ak[i][nd] = mfma16(as, tr_frag<DR>(Qs + ks * 32 * DR, nd * 16, lane), ak[i][nd]);
                    av[i][nd] = mfma16(ap, tr_frag<DR>(Gs + ks * 32 * DR, nd * 16, lane), av[i][nd]);
                }
            }
        }
    }
    float* dst = part + ((((size_t)b * heads + h) * gridDim.x + blockIdx.x) * 2) * (size_t)NP * HD;
#pragma unroll
    for (int i = 0; i < NKT; ++i) {
        const int kt = wid + 4 * i;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const size_t row = (size_t)(kt * 16 + g * 4 + r) * HD + l15;
#pragma unroll
            for (int nd = 0; nd < ND; ++nd) { dst[row + nd * 16] = ak[i][nd][r]; dst[(size_t)NP * HD + row + nd * 16] = av[i][nd][r]; }
        }
    }
}

// scalar route: the phases of attn_bwd_k on one key range; delta = rowsum(dO * out) comes from attn_delta_k instead of the full-row sum p dP.
// The block walks the 256-query chunks blockIdx.x, blockIdx.x + gridDim.x, ... and leaves one partial.
template <typename T, int HD>
__global__ __launch_bounds__(256) void attn_long_bwd_k(const T* __restrict__ q, int ld_q, const T* __restrict__ kv, int ld_kv, const T* __restrict__ dout, int ld_do,
                                                       const float* __restrict__ lse, const float* __restrict__ delta, float* __restrict__ dqw, float* __restrict__ part,
                                                       int Nq, int Nkv, int heads, float scale, int key0, int dq_acc) {
    extern __shared__ float lds[];
    typedef ScalarBwdLds<HD, AL_CK, AT_QB> L;
    constexpr int NK = AL_CK / 64, NP = AL_CK, RS = L::RS, KPW = NP / 4, QB = AT_QB, GQ = L::GQ;
    float* Kt = lds + L::Kt; float* Vt = lds + L::Vt;
    float* Pt = lds + L::Pt; float* dSt = lds + L::dSt; float* qt = lds + L::qt; float* dot = lds + L::dot;
    const int b = blockIdx.z, h = blockIdx.y, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int dl = lane & (HD - 1);
    attn_stage_kv<T, HD>(kv + ((size_t)b * Nkv + key0) * ld_kv, ld_kv, Nkv - key0, NP, heads, h, Kt, Vt);
    __syncthreads();
    float ak[KPW], av[KPW];
#pragma unroll
    for (int j = 0; j < KPW; ++j) { ak[j] = 0.f; av[j] = 0.f; }
    const int nqc = (Nq + AT_QCHUNK - 1) / AT_QCHUNK;
    for (int qc = blockIdx.x; qc < nqc; qc += gridDim.x) {
        const int q0 = qc * AT_QCHUNK;
        int q1 = q0 + AT_QCHUNK; if (q1 > Nq) q1 = Nq;
        for (int g0 = q0; g0 < q1; g0 += GQ) {
            const int qb = g0 + wid * QB;
            float qd[QB], dod[QB], L_[QB], D[QB], s[QB][NK], dp[QB][NK];
#pragma unroll
            for (int i = 0; i < QB; ++i) {
                const bool ok = qb + i < q1;
                const int qi = ok ? qb + i : q1 - 1;
                const size_t qo = (size_t)b * Nq + qi;
                qd[i] = ok && lane < HD ? TT<T>::ld(q + qo * ld_q + h * HD + lane) * scale : 0.f;
                dod[i] = ok && lane < HD ? TT<T>::ld(dout + qo * ld_do + h * HD + lane) : 0.f;
                L_[i] = lse[((size_t)b * heads + h) * Nq + qi]; D[i] = delta[((size_t)b * heads + h) * Nq + qi];
#pragma unroll
                for (int k = 0; k < NK; ++k) { s[i][k] = 0.f; dp[i][k] = 0.f; }
            }
#pragma unroll
            for (int d = 0; d < HD; ++d) {
                float kk[NK], vv[NK];
#pragma unroll
                for (int k = 0; k < NK; ++k) { kk[k] = Kt[d * RS + k * 64 + lane]; vv[k] = Vt[d * RS + k * 64 + lane]; }
#pragma unroll
                for (int i = 0; i < QB; ++i) {
                    const float qq = rdlane(qd[i], d), gg = rdlane(dod[i], d);
#pragma unroll
                    for (int k = 0; k < NK; ++k) { s[i][k] += qq * kk[k]; dp[i][k] += gg * vv[k]; }
                }
            }
            float dqd[QB];
#pragma unroll
            for (int i = 0; i < QB; ++i) {
                const bool ok = qb + i < q1;
                const int row = wid * QB + i;
#pragma unroll
                for (int k = 0; k < NK; ++k) {
                    s[i][k] = (ok && key0 + k * 64 + lane < Nkv) ? expf(s[i][k] - L_[i]) : 0.f;
                    dp[i][k] = s[i][k] * (dp[i][k] - D[i]);           // dS
                    Pt[row * NP + k * 64 + lane] = s[i][k]; dSt[row * NP + k * 64 + lane] = dp[i][k];
                }
                if (lane < HD) { qt[row * HD + lane] = qd[i]; dot[row * HD + lane] = dod[i]; }
                dqd[i] = 0.f;
            }
#pragma unroll
            for (int k = 0; k < NK; ++k) {
#pragma unroll
                for (int l = 0; l < 64; ++l) {
                    const float kk = Kt[dl * RS + k * 64 + l];
#pragma unroll
                    for (int i = 0; i < QB; ++i) dqd[i] += rdlane(dp[i][k], l) * kk;
                }
            }
#pragma unroll
            for (int i = 0; i < QB; ++i)
                if (qb + i < q1 && lane < HD) {
                    float* dp_ = dqw + ((size_t)b * Nq + qb + i) * (heads * HD) + h * HD + lane;
                    *dp_ = dq_acc ? *dp_ + dqd[i] * scale : dqd[i] * scale;
                }
            __syncthreads();
            // phase B: this wave's keys [wid*KPW, +KPW), all queries of the group
            for (int r = 0; r < GQ; ++r) {
                const float qv = qt[r * HD + dl], gv = dot[r * HD + dl];
                const float* pr = Pt + r * NP + wid * KPW; const float* dr = dSt + r * NP + wid * KPW;
#pragma unroll
                for (int j = 0; j < KPW; ++j) { ak[j] += dr[j] * qv; av[j] += pr[j] * gv; }
            }
            __syncthreads();
        }
    }
    float* dst = part + ((((size_t)b * heads + h) * gridDim.x + blockIdx.x) * 2) * NP * HD;
    if (lane < HD) {
#pragma unroll
        for (int j = 0; j < KPW; ++j) {
            dst[(size_t)(wid * KPW + j) * HD + lane] = ak[j];
            dst[(size_t)NP * HD + (size_t)(wid * KPW + j) * HD + lane] = av[j];
        }
    }
}

// dq [rows][ld_dq] <- dqw [rows][Cc] fp32, one rounding
template <typename T>
__global__ __launch_bounds__(256) void attn_long_dq_store_k(const float* __restrict__ dqw, T* __restrict__ dq, int ld_dq, size_t rows, int Cc) {
    const size_t n = rows * Cc;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) TT<T>::st(dq + (i / Cc) * ld_dq + i % Cc, dqw[i]);
}

// ------------------------------------------------------------------------------------------ host
using namespace pn2_host;
constexpr int GRID_CAP = 16384;
constexpr int AL_MAXKV = 4096;

inline int attn_geom(int Nkv, int max_kv, int heads, int head_dim) { return ((head_dim == 32 || head_dim == 64) && Nkv >= 1 && Nkv <= max_kv && heads >= 1) ? 0 : -2; }
// the MFMA kernels take bf16 views whose every row pitch keeps 16-byte alignment
template <typename... L>
inline bool attn_use_mfma(int dt, L... ld) { return dt == PN2_BF16 && (((ld % 8) == 0) && ...); }

// head_dim (32 or 64: attn_geom) and the 64-key blocks of the on-chip kernels (1..4) as compile-time constants: f(Int<N>)
template <typename F>
int with_head_dim(int head_dim, F f) { return head_dim == 32 ? f(Int<32>{}) : f(Int<64>{}); }
template <typename F>
int with_attn_nk(int NK, F f) { return NK == 1 ? f(Int<1>{}) : NK == 2 ? f(Int<2>{}) : NK == 3 ? f(Int<3>{}) : f(Int<4>{}); }

// persistent attention blocks per launch: the blocks of one (b, head) share its K / V and walk the query tiles between them
inline int attn_target_blocks() { return 512; }
inline int attn_bwd_gx(int B, int heads, int Nq) {
    const int ntile = (Nq + 63) / 64;
    // backward: one block per CU measured best (the block state - K, V, two 64-query tiles, dS / P and their transposes - fills the LDS anyway)
    int gx = (attn_target_blocks() / 2 + B * heads - 1) / (B * heads);
    return gx > ntile ? ntile : (gx < 1 ? 1 : gx);
}
// partial slots per (b, head) of the streamed backward = blocks per (b, head) of one launch.  bf16: the one-block-per-CU rule of attn_bwd_gx on both
// routes (the scalar kernel walks its 256-query chunks the same way); fp32: one block per 256-query chunk
inline int attn_long_slots(int dt, int B, int heads, int Nq) { return dt == PN2_BF16 ? attn_bwd_gx(B, heads, Nq) : (Nq + AT_QCHUNK - 1) / AT_QCHUNK; }
inline unsigned attn_delta_blocks(int B, int Nq, int heads) { return (unsigned)(((size_t)B * Nq * heads + 3) / 4); }

}  // namespace

extern "C" {

int pn2_attn_fwd(int dt, const void* q, int ld_q, const void* kv, int ld_kv, void* out, int ld_o, float* lse, int B, int Nq, int Nkv, int heads, int head_dim,
                 float scale, void* stream) {
    if (!q || !kv || !out || !lse) return -1;
    if (int rc = attn_geom(Nkv, 64 * AT_MAXK, heads, head_dim)) return rc;
    const hipStream_t st = (hipStream_t)stream;
    const int NK = (Nkv + 63) / 64;
    return with_head_dim(head_dim, [&](auto hd) {
        constexpr int HD = decltype(hd)::value;
        if (attn_use_mfma(dt, ld_q, ld_kv, ld_o)) {
            const int ntile = (Nq + 127) / 128;
            int gx = (attn_target_blocks() + B * heads - 1) / (B * heads); if (gx > ntile) gx = ntile; if (gx < 1) gx = 1;
            return with_attn_nk(NK, [&](auto nk) {
                constexpr int NKM = decltype(nk)::value == 3 ? 4 : decltype(nk)::value;          // 129..192 keys run the 256-key instantiation (zero-padded keys are masked)
                constexpr size_t lds = MfmaFwdLds<HD, NKM * 64>::bytes();
                return pn2_launch<attn_fwd_mfma_k<NKM, HD>>(dim3(gx, heads, B), dim3(512), lds, (int)lds, st, (const bf16_t*)q, ld_q, (const bf16_t*)kv, ld_kv, (bf16_t*)out, ld_o, lse,
                                                            Nq, Nkv, heads, scale);
            });
        }
        const int qpb = 64;
        return with_storage_dtype(dt, [&](auto ty) {
            using T = type_of<decltype(ty)>;
            return with_attn_nk(NK, [&](auto nk) {
                constexpr int NKV = decltype(nk)::value;
                constexpr size_t lds = ScalarFwdLds<HD, NKV * 64>::bytes();
                return pn2_launch<attn_fwd_k<T, NKV, HD>>(dim3((Nq + qpb - 1) / qpb, heads, B), dim3(256), lds, (int)lds, st, (const T*)q, ld_q, (const T*)kv, ld_kv, (T*)out, ld_o, lse,
                                                          Nq, Nkv, heads, scale, qpb);
            });
        });
    });
}

int pn2_attn_bwd_blocks(int dt, int B, int heads, int Nq) {
    if (Nq < 1 || B < 1 || heads < 1) return -1;
    return dt == PN2_BF16 ? attn_bwd_gx(B, heads, Nq) : (Nq + AT_QCHUNK - 1) / AT_QCHUNK;
}

int pn2_attn_bwd(int dt, const void* q, int ld_q, const void* kv, int ld_kv, const void* out, int ld_o, const void* dout, int ld_do, const float* lse, void* dq, int ld_dq,
                 void* dkv, int ld_dkv, float* partial, float* delta, int B, int Nq, int Nkv, int heads, int head_dim, float scale, void* stream) {
    if (!q || !kv || !out || !dout || !lse || !dq || !dkv || !partial || !delta) return -1;
    if (int rc = attn_geom(Nkv, 64 * AT_MAXK, heads, head_dim)) return rc;
    const hipStream_t st = (hipStream_t)stream;
    const int NK = (Nkv + 63) / 64, NP = NK * 64;
    return with_head_dim(head_dim, [&](auto hd) {
        constexpr int HD = decltype(hd)::value;
        if (attn_use_mfma(dt, ld_q, ld_kv, ld_do, ld_dq)) {
            const int nqt = attn_bwd_gx(B, heads, Nq);                   // persistent blocks (= partial slots) per (b, head)
            if (int rc = pn2_launch<attn_delta_k<bf16_t, HD>>(dim3(attn_delta_blocks(B, Nq, heads)), dim3(256), 0, 0, st, (const bf16_t*)dout, ld_do, (const bf16_t*)out, ld_o, delta, B, Nq, heads))
                return rc;
            // 128 keys per launch at both head dims: at HD = 32 a 256-key block would need 161 KiB of LDS (its dS / P transposes are 64 queries wide
            // whatever HD is), one KiB over the CU's 160
            for (int key0 = 0; key0 < NP; key0 += 128) {
                auto range = [&](auto nkb) {
                    constexpr int NKB = decltype(nkb)::value;
                    constexpr size_t lds = MfmaBwdLds<HD, NKB * 64>::bytes();
                    return pn2_launch<attn_bwd_mfma_k<NKB, HD>>(dim3(nqt, heads, B), dim3(256), lds, (int)lds, st, (const bf16_t*)q, ld_q, (const bf16_t*)kv, ld_kv, (const bf16_t*)dout, ld_do,
                                                                lse, (const float*)delta, (bf16_t*)dq, ld_dq, partial, Nq, Nkv, heads, scale, key0, NP, key0 > 0 ? 1 : 0);
                };
                if (int rc = NP - key0 >= 128 ? range(Int<2>{}) : range(Int<1>{})) return rc;
            }
            return pn2_launch<attn_bwd_kv_reduce_k<bf16_t, HD>>(dim3(Nkv, heads, B), dim3(HD), 0, 0, st, (const float*)partial, (bf16_t*)dkv, ld_dkv, Nkv, NP, heads, nqt);
        }
        const int nqb = (Nq + AT_QCHUNK - 1) / AT_QCHUNK;
        // a bf16 view that the MFMA kernels cannot take: its partial has pn2_attn_bwd_blocks(bf16) = attn_bwd_gx slots, fewer than nqb for many (b, head)
        if (dt == PN2_BF16 && nqb > attn_bwd_gx(B, heads, Nq)) return -2;
        return with_storage_dtype(dt, [&](auto ty) {
            using T = type_of<decltype(ty)>;
            const int rc = with_attn_nk(NK, [&](auto nk) {
                constexpr int NKV = decltype(nk)::value, QB = NKV == 4 ? 2 : AT_QB;          // 256 keys: smaller query groups so that K, V and the tiles fit the 160 KiB of LDS
                constexpr size_t lds = ScalarBwdLds<HD, NKV * 64, QB>::bytes();
                return pn2_launch<attn_bwd_k<T, NKV, QB, HD>>(dim3(nqb, heads, B), dim3(256), lds, (int)lds, st, (const T*)q, ld_q, (const T*)kv, ld_kv, (const T*)dout, ld_do, lse, (T*)dq, ld_dq,
                                                              partial, Nq, Nkv, heads, scale);
            });
            if (rc) return rc;
            return pn2_launch<attn_bwd_kv_reduce_k<T, HD>>(dim3(Nkv, heads, B), dim3(HD), 0, 0, st, (const float*)partial, (T*)dkv, ld_dkv, Nkv, NP, heads, nqb);
        });
    });
}

// ---- 1..4096 keys streamed in chunks of AL_CK
int pn2_attn_long_fwd(int dt, const void* q, int ld_q, const void* kv, int ld_kv, void* out, int ld_o, float* lse, int B, int Nq, int Nkv, int heads, int head_dim,
                      float scale, void* stream) {
    if (!q || !kv || !out || !lse) return -1;
    if (int rc = attn_geom(Nkv, AL_MAXKV, heads, head_dim)) return rc;
    if (B < 1 || Nq < 1) return -2;
    const hipStream_t st = (hipStream_t)stream;
    return with_head_dim(head_dim, [&](auto hd) {
        constexpr int HD = decltype(hd)::value;
        if (attn_use_mfma(dt, ld_q, ld_kv, ld_o)) {
            constexpr size_t lds = MfmaFwdLds<HD, AL_CK>::bytes();
            return pn2_launch<attn_long_fwd_mfma_k<HD>>(dim3((Nq + 127) / 128, heads, B), dim3(512), lds, (int)lds, st, (const bf16_t*)q, ld_q, (const bf16_t*)kv, ld_kv, (bf16_t*)out, ld_o,
                                                        lse, Nq, Nkv, heads, scale);
        }
        return with_storage_dtype(dt, [&](auto ty) {
            using T = type_of<decltype(ty)>;
            constexpr size_t lds = ScalarLongFwdLds<HD>::bytes();
            return pn2_launch<attn_long_fwd_k<T, HD>>(dim3((Nq + AL_QPB - 1) / AL_QPB, heads, B), dim3(256), lds, (int)lds, st, (const T*)q, ld_q, (const T*)kv, ld_kv, (T*)out, ld_o,
                                                      lse, Nq, Nkv, heads, scale);
        });
    });
}

int pn2_attn_long_bwd_blocks(int dt, int B, int heads, int Nq) {
    if (Nq < 1 || B < 1 || heads < 1) return -1;
    return attn_long_slots(dt, B, heads, Nq);
}

int pn2_attn_long_bwd_workspace(int dt, int B, int Nq, int heads, int head_dim, long long* floats) {
    if (!floats) return -1;
    if (Nq < 1 || B < 1 || attn_geom(1, AL_MAXKV, heads, head_dim)) return -2;
    floats[0] = (long long)B * heads * attn_long_slots(dt, B, heads, Nq) * 2 * AL_CK * head_dim;
    floats[1] = (long long)B * heads * Nq;
    floats[2] = (long long)B * Nq * heads * head_dim;
    return 0;
}

int pn2_attn_long_bwd(int dt, const void* q, int ld_q, const void* kv, int ld_kv, const void* out, int ld_o, const void* dout, int ld_do, const float* lse, void* dq, int ld_dq,
                      void* dkv, int ld_dkv, float* partial, float* delta, float* dq_acc, int B, int Nq, int Nkv, int heads, int head_dim, float scale, void* stream) {
    if (!q || !kv || !out || !dout || !lse || !dq || !dkv || !partial || !delta || !dq_acc) return -1;
    if (int rc = attn_geom(Nkv, AL_MAXKV, heads, head_dim)) return rc;
    if (B < 1 || Nq < 1) return -2;
    const hipStream_t st = (hipStream_t)stream;
    const bool mfma = attn_use_mfma(dt, ld_q, ld_kv, ld_do);
    const int slots = attn_long_slots(dt, B, heads, Nq);
    const dim3 grid(slots, heads, B);
    return with_head_dim(head_dim, [&](auto hd) {
        constexpr int HD = decltype(hd)::value;
        return with_storage_dtype(dt, [&](auto ty) {
            using T = type_of<decltype(ty)>;
            if (int rc = pn2_launch<attn_delta_k<T, HD>>(dim3(attn_delta_blocks(B, Nq, heads)), dim3(256), 0, 0, st, (const T*)dout, ld_do, (const T*)out, ld_o, delta, B, Nq, heads)) return rc;
            for (int key0 = 0; key0 < Nkv; key0 += AL_CK) {              // plain launches in stream order: fixed summation order, no atomics
                constexpr size_t lm = MfmaBwdLds<HD, AL_CK>::bytes(), ls = ScalarBwdLds<HD, AL_CK, AT_QB>::bytes();
                int rc;
                if (mfma) rc = pn2_launch<attn_long_bwd_mfma_k<HD>>(grid, dim3(256), lm, (int)lm, st, (const bf16_t*)q, ld_q, (const bf16_t*)kv, ld_kv, (const bf16_t*)dout, ld_do, lse,
                                                                    (const float*)delta, dq_acc, partial, Nq, Nkv, heads, scale, key0, key0 > 0 ? 1 : 0);
                else rc = pn2_launch<attn_long_bwd_k<T, HD>>(grid, dim3(256), ls, (int)ls, st, (const T*)q, ld_q, (const T*)kv, ld_kv, (const T*)dout, ld_do, lse, (const float*)delta, dq_acc,
                                                             partial, Nq, Nkv, heads, scale, key0, key0 > 0 ? 1 : 0);
                if (rc) return rc;
                const int nk = Nkv - key0 < AL_CK ? Nkv - key0 : AL_CK;          // the range's partial [slots][2][AL_CK][HD] -> rows key0.. of dkv
                if ((rc = pn2_launch<attn_bwd_kv_reduce_k<T, HD>>(dim3(nk, heads, B), dim3(HD), 0, 0, st, (const float*)partial, (T*)dkv + (size_t)key0 * ld_dkv, ld_dkv, Nkv, AL_CK, heads, slots)))
                    return rc;
            }
            const size_t rows = (size_t)B * Nq;
            return pn2_launch<attn_long_dq_store_k<T>>(dim3(grid_for(rows * heads * HD, GRID_CAP)), dim3(256), 0, 0, st, (const float*)dq_acc, (T*)dq, ld_dq, rows, heads * HD);
        });
    });
}

}  // extern "C"
