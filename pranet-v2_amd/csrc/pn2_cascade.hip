// pn2_cascade.hip — the attention gate of the CASCADE decoders (Attention_block + the "aggregate" / "Concat" line behind it):
//   g1 = BN_g(W_g g)   x1 = BN_x(W_x x)   psi = sigmoid(BN_psi(w_psi . relu(g1 + x1) + b_psi))   out = g + x * psi (CASCADE_Add*)  or  cat(x * psi, g) (CASCADE_Cat)
// The two 1x1 convs and their BatchNorm statistics stay on the conv / pn2_bn_* kernels; what is here starts from the RAW conv outputs [M][Fp] and their
// (scale, shift) rows, so the F_int-wide relu(g1 + x1) only ever exists in registers:
//   ag_psi_fwd_k     psi_raw[m] = sum_c w_psi[c] * relu(fma(rg, sg, hg) + fma(rx, sx, hx)) + per-block (mean, M2) of psi_raw for pn2_bn_finalize (tile form)
//   ag_apply_fwd_k   out = g + x * sigmoid(a * psi_raw + b)
//   ag_bwd_gate_k    dx (+)= dout * psi, dg (+)= dout, dz[m] = psi (1 - psi) sum_c dout * x, per-block sums of dz and dz * xhat for pn2_bn_bwd_finalize
//   ag_apply_cat_fwd_k    out[m][0:C] = x * sigmoid(a * psi_raw + b), out[m][C:2C] = g: rows of 2C from one read of g and x (C % 8 == 0: no pad lanes, both halves 16-byte aligned)
//   ag_bwd_gate_cat_k     ag_bwd_gate_k on a dout row of 2C: dx (+)= dout[:, 0:C] * psi, dg (+)= dout[:, C:2C], dz and the block sums from the left half only
//   ag_bwd_sum_k     dpsi_raw from dz and the finalize's coefficients; dsum[m][c] = dpsi_raw * w_psi[c] * [relu' > 0] (ONE tensor: the gradient of both BatchNorm outputs),
//                    per-block rows of dw_psi = sum_m dpsi_raw * relu(...) and of db_psi = sum_m dpsi_raw for pn2_colsum_finalize
// Row walks: 256 threads = CVP channel vectors x R row lanes, 16-byte loads.  Every sum runs in a fixed order (butterflies, then LDS rows in index order): no atomics,
// bit-identical replays.  Pad lanes (c >= F_int, c >= C) contribute zero and are written as zero.
#include "pn2_common.h"
#include "../../include/pn2.h"

namespace {

using namespace pn2_host;
constexpr int GRID_CAP = 16384;
constexpr int AG_MAX_ROWS = 2048;          // rows per block of ag_psi_fwd_k: the block's psi_raw values stay in LDS for the two-pass (mean, M2)
constexpr int RU = 4;                      // rows in flight per thread

template <typename T> __device__ __forceinline__ void ldv(const T* p, float* f) { TT<T>::unpack(*reinterpret_cast<const uint4*>(p), f); }
template <typename T> __device__ __forceinline__ void stv(T* p, const float* f) { *reinterpret_cast<uint4*>(p) = TT<T>::pack(f); }
__device__ __forceinline__ float sigmoidf_(float z) { return 1.f / (1.f + expf(-z)); }

struct AgPlan { int cvp, rows, nblk; };
// cvp_cap 64: a row stays inside one wave (the channel reductions), and the F_int-wide kernels take at most 64 vectors
inline AgPlan ag_plan(int M, int CV, int cvp_cap, int max_rows) {
    AgPlan p;
    p.cvp = pow2ceil(CV); if (p.cvp > cvp_cap) p.cvp = cvp_cap;
    const int R = 256 / p.cvp, want = (M + 1023) / 1024;
    p.rows = (want + R - 1) / R * R;
    if (p.rows < 4 * R) p.rows = 4 * R;
    if (max_rows > 0 && p.rows > max_rows) p.rows = max_rows;          // (a power of two >= 256: a multiple of every R)
    p.nblk = (M + p.rows - 1) / p.rows;
    return p;
}
inline AgPlan ag_plan_kind(int dt, int M, int width_p, int kind) {
    const int CV = width_p / vec_of(dt);
    return ag_plan(M, CV, 64, kind == 0 ? AG_MAX_ROWS : 0);
}
inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// sum of v over the block in a fixed order (every thread gets it); red: 4 floats of LDS
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// relu(BN_g(rg) + BN_x(rx)) of one channel vector; null scale rows: the operand already is the BatchNorm output
template <int V>
__device__ __forceinline__ void relu_sum(const float* g, const float* x, const float* sg, const float* hg, const float* sx, const float* hx, float* s) {
#pragma unroll
    for (int e = 0; e < V; ++e) s[e] = fmaxf(fmaf(g[e], sg[e], hg[e]) + fmaf(x[e], sx[e], hx[e]), 0.f);
}
template <int V>
__device__ __forceinline__ void load_rows(const float* sc, const float* sh, int c, float* s, float* h) {
#pragma unroll
    for (int e = 0; e < V; ++e) { s[e] = sc ? sc[c + e] : 1.f; h[e] = sh ? sh[c + e] : 0.f; }
}

template <typename T>
__global__ __launch_bounds__(256) void ag_psi_fwd_k(const T* __restrict__ rg, int ld_g, const float* __restrict__ sc_g, const float* __restrict__ sh_g,
                                                    const T* __restrict__ rx, int ld_x, const float* __restrict__ sc_x, const float* __restrict__ sh_x,
                                                    const float* __restrict__ w, int F, int Fp, int M, float* __restrict__ psi, float* __restrict__ pmean,
                                                    float* __restrict__ pm2, int rows, int CVP) {
    constexpr int V = TT<T>::VEC;
    __shared__ float sv[AG_MAX_ROWS];
    __shared__ float red[4];
    const int CV = Fp / V, R = 256 / CVP, cvl = threadIdx.x % CVP, rl = threadIdx.x / CVP;
    const int r0 = blockIdx.x * rows;
    int r1 = r0 + rows; if (r1 > M) r1 = M;
    const bool act = cvl < CV;          // (host: CV <= CVP)
    const int c = cvl * V;
    float kw[V], sg[V], hg[V], sx[V], hx[V];
#pragma unroll
    for (int e = 0; e < V; ++e) { kw[e] = 0.f; sg[e] = 0.f; hg[e] = 0.f; sx[e] = 0.f; hx[e] = 0.f; }
    if (act) {
        load_rows<V>(sc_g, sh_g, c, sg, hg); load_rows<V>(sc_x, sh_x, c, sx, hx);
#pragma unroll
        for (int e = 0; e < V; ++e) kw[e] = (c + e < F) ? w[c + e] : 0.f;
    }
    for (int mb = r0; mb < r1; mb += R * RU) {          // (uniform trip count: the butterflies below run with every lane)
        uint4 vg[RU], vx[RU];
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            const int mm = mb + rl + u * R;
            if (act && mm < r1) {
                vg[u] = *reinterpret_cast<const uint4*>(rg + (size_t)mm * ld_g + c);
                vx[u] = *reinterpret_cast<const uint4*>(rx + (size_t)mm * ld_x + c);
            }
        }
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            const int mm = mb + rl + u * R;
            float d = 0.f;
            if (act && mm < r1) {
                float g[V], x[V], s[V];
                TT<T>::unpack(vg[u], g); TT<T>::unpack(vx[u], x);
                relu_sum<V>(g, x, sg, hg, sx, hx, s);
#pragma unroll
                for (int e = 0; e < V; ++e) d = fmaf(kw[e], s[e], d);
            }
            for (int off = CVP >> 1; off > 0; off >>= 1) d += __shfl_xor(d, off);
            if (cvl == 0 && mm < r1) { psi[mm] = d; sv[mm - r0] = d; }
        }
    }
    if (!pmean) return;
    __syncthreads();
    // the block's (mean, M2) in two passes over its values: the tile form of pn2_bn_finalize (bn desc tile_rows = rows)
    const int n = r1 - r0;
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += sv[i];
    const float mean = block_sum(s, red) / (float)n;
    float q = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) { const float dlt = sv[i] - mean; q = fmaf(dlt, dlt, q); }
    q = block_sum(q, red);
    if (threadIdx.x == 0) { pmean[blockIdx.x] = mean; pm2[blockIdx.x] = q; }
}

template <typename T>
__global__ __launch_bounds__(256) void ag_apply_fwd_k(const T* __restrict__ g, int ld_g, const T* __restrict__ x, int ld_x, const float* __restrict__ psi,
                                                      const float* __restrict__ a, const float* __restrict__ b, T* __restrict__ out, int ld_o, int M, int C, int Cp) {
    constexpr int V = TT<T>::VEC;
    const int CV = Cp / V;
    const size_t total = (size_t)M * CV;
    const float ka = a[0], kb = b[0];
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        int cv; const size_t m = divmod_idx(idx, CV, cv);
        const int c = cv * V;
        float gv[V], xv[V], o[V];
        ldv<T>(g + m * ld_g + c, gv); ldv<T>(x + m * ld_x + c, xv);
        const float s = sigmoidf_(fmaf(psi[m], ka, kb));
#pragma unroll
        for (int e = 0; e < V; ++e) o[e] = (c + e < C) ? fmaf(xv[e], s, gv[e]) : 0.f;
        stv<T>(out + m * ld_o + c, o);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void ag_bwd_gate_k(const T* __restrict__ dout, int ld_do, const T* __restrict__ x, int ld_x, const float* __restrict__ psi,
                                                     const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ mean, const float* __restrict__ invstd,
                                                     T* __restrict__ dx, int ld_dx, int dx_acc, T* __restrict__ dg, int ld_dg, int dg_acc,
                                                     float* __restrict__ dz, float* __restrict__ p1, float* __restrict__ p2, int M, int C, int Cp, int rows, int CVP) {
    constexpr int V = TT<T>::VEC;
    __shared__ float red[4];
    const int CV = Cp / V, R = 256 / CVP, cvl = threadIdx.x % CVP, rl = threadIdx.x / CVP;
    const int r0 = blockIdx.x * rows;
    int r1 = r0 + rows; if (r1 > M) r1 = M;
    const float ka = a[0], kb = b[0], mu = mean ? mean[0] : 0.f, is = mean ? invstd[0] : 0.f;
    float a1 = 0.f, a2 = 0.f;
    for (int mb = r0; mb < r1; mb += R) {          // (uniform trip count, as in ag_psi_fwd_k)
        const int m = mb + rl;
        const bool valid = m < r1;
        float pr = 0.f, s = 0.f, t = 0.f;
        if (valid) {
            pr = psi[m]; s = sigmoidf_(fmaf(pr, ka, kb));
            for (int cv = cvl; cv < CV; cv += CVP) {
                const int c = cv * V;
                float d[V], xv[V], o[V];
                ldv<T>(dout + (size_t)m * ld_do + c, d); ldv<T>(x + (size_t)m * ld_x + c, xv);
#pragma unroll
                for (int e = 0; e < V; ++e) { if (c + e >= C) d[e] = 0.f; t = fmaf(d[e], xv[e], t); }
                if (dx) {
                    if (dx_acc) ldv<T>(dx + (size_t)m * ld_dx + c, o);
#pragma unroll
                    for (int e = 0; e < V; ++e) o[e] = (c + e >= C) ? 0.f : (dx_acc ? fmaf(d[e], s, o[e]) : d[e] * s);
                    stv<T>(dx + (size_t)m * ld_dx + c, o);
                }
                if (dg) {
                    if (dg_acc) {
                        ldv<T>(dg + (size_t)m * ld_dg + c, o);
#pragma unroll
                        for (int e = 0; e < V; ++e) d[e] = (c + e >= C) ? 0.f : d[e] + o[e];
                    }
                    stv<T>(dg + (size_t)m * ld_dg + c, d);
                }
            }
        }
        for (int off = CVP >> 1; off > 0; off >>= 1) t += __shfl_xor(t, off);
        if (valid && cvl == 0) {
            const float z = t * s * (1.f - s);
            dz[m] = z;
            a1 += z; a2 = fmaf(z, (pr - mu) * is, a2);
        }
    }
    a1 = block_sum(a1, red);
    a2 = block_sum(a2, red);
    if (threadIdx.x == 0) { p1[blockIdx.x] = a1; p2[blockIdx.x] = a2; }
}

// cat(x * psi, g): one thread per channel vector of the C-wide operands, two stores (C % 8 == 0: Cp == C, the right half starts on a 16-byte boundary)
template <typename T>
__global__ __launch_bounds__(256) void ag_apply_cat_fwd_k(const T* __restrict__ g, int ld_g, const T* __restrict__ x, int ld_x, const float* __restrict__ psi,
                                                          const float* __restrict__ a, const float* __restrict__ b, T* __restrict__ out, int ld_o, int M, int C) {
    constexpr int V = TT<T>::VEC;
    const int CV = C / V;
    const size_t total = (size_t)M * CV;
    const float ka = a[0], kb = b[0];
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        int cv; const size_t m = divmod_idx(idx, CV, cv);
        const int c = cv * V;
        const uint4 gv = *reinterpret_cast<const uint4*>(g + m * ld_g + c);          // (copied as it is: the right half equals g bit for bit)
        float xv[V], o[V];
        ldv<T>(x + m * ld_x + c, xv);
        const float s = sigmoidf_(fmaf(psi[m], ka, kb));
#pragma unroll
        for (int e = 0; e < V; ++e) o[e] = xv[e] * s;
        stv<T>(out + m * ld_o + c, o);
        *reinterpret_cast<uint4*>(out + m * ld_o + C + c) = gv;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void ag_bwd_gate_cat_k(const T* __restrict__ dout, int ld_do, const T* __restrict__ x, int ld_x, const float* __restrict__ psi,
                                                         const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ mean, const float* __restrict__ invstd,
                                                         T* __restrict__ dx, int ld_dx, int dx_acc, T* __restrict__ dg, int ld_dg, int dg_acc,
                                                         float* __restrict__ dz, float* __restrict__ p1, float* __restrict__ p2, int M, int C, int rows, int CVP) {
    constexpr int V = TT<T>::VEC;
    __shared__ float red[4];
    const int CV = C / V, R = 256 / CVP, cvl = threadIdx.x % CVP, rl = threadIdx.x / CVP;
    const int r0 = blockIdx.x * rows;
    int r1 = r0 + rows; if (r1 > M) r1 = M;
    const float ka = a[0], kb = b[0], mu = mean ? mean[0] : 0.f, is = mean ? invstd[0] : 0.f;
    float a1 = 0.f, a2 = 0.f;
    for (int mb = r0; mb < r1; mb += R) {          // (uniform trip count, as in ag_psi_fwd_k)
        const int m = mb + rl;
        const bool valid = m < r1;
        float pr = 0.f, s = 0.f, t = 0.f;
        if (valid) {
            pr = psi[m]; s = sigmoidf_(fmaf(pr, ka, kb));
            for (int cv = cvl; cv < CV; cv += CVP) {
                const int c = cv * V;
                float d[V], xv[V], o[V];
                const uint4 dr = *reinterpret_cast<const uint4*>(dout + (size_t)m * ld_do + C + c);          // the right half: g's gradient as it is
                ldv<T>(dout + (size_t)m * ld_do + c, d); ldv<T>(x + (size_t)m * ld_x + c, xv);
#pragma unroll
                for (int e = 0; e < V; ++e) t = fmaf(d[e], xv[e], t);
                if (dx) {
                    if (dx_acc) ldv<T>(dx + (size_t)m * ld_dx + c, o);
#pragma unroll
                    for (int e = 0; e < V; ++e) o[e] = dx_acc ? fmaf(d[e], s, o[e]) : d[e] * s;
                    stv<T>(dx + (size_t)m * ld_dx + c, o);
                }
                if (dg) {
                    if (dg_acc) {
                        TT<T>::unpack(dr, d); ldv<T>(dg + (size_t)m * ld_dg + c, o);
#pragma unroll
                        for (int e = 0; e < V; ++e) d[e] += o[e];
                        stv<T>(dg + (size_t)m * ld_dg + c, d);
                    } else {
                        *reinterpret_cast<uint4*>(dg + (size_t)m * ld_dg + c) = dr;
                    }
                }
            }
        }
        for (int off = CVP >> 1; off > 0; off >>= 1) t += __shfl_xor(t, off);
        if (valid && cvl == 0) {
            const float z = t * s * (1.f - s);
            dz[m] = z;
            a1 += z; a2 = fmaf(z, (pr - mu) * is, a2);
        }
    }
    a1 = block_sum(a1, red);
    a2 = block_sum(a2, red);
    if (threadIdx.x == 0) { p1[blockIdx.x] = a1; p2[blockIdx.x] = a2; }
}

template <typename T>
__global__ __launch_bounds__(256) void ag_bwd_sum_k(const float* __restrict__ dz, const float* __restrict__ psi, const float* __restrict__ a, const float* __restrict__ mean,
                                                    const float* __restrict__ invstd, const float* __restrict__ coef,
                                                    const T* __restrict__ rg, int ld_g, const float* __restrict__ sc_g, const float* __restrict__ sh_g,
                                                    const T* __restrict__ rx, int ld_x, const float* __restrict__ sc_x, const float* __restrict__ sh_x,
                                                    const float* __restrict__ w, int F, int Fp, int M, T* __restrict__ ds, int ld_ds,
                                                    float* __restrict__ pw, float* __restrict__ pb, int rows, int CVP) {
    constexpr int V = TT<T>::VEC;
    __shared__ float sh[256 * V];
    __shared__ float shb[256];
    const int CV = Fp / V, R = 256 / CVP, cvl = threadIdx.x % CVP, rl = threadIdx.x / CVP;
    const int r0 = blockIdx.x * rows;
    int r1 = r0 + rows; if (r1 > M) r1 = M;
    const bool act = cvl < CV;          // (host: CV <= CVP)
    const int c = cvl * V;
    // dpsi_raw = k0 * dz + k1 * (psi_raw - mu) + k2: train mode from the finalize's rows (gamma * invstd, mean dz, mean dz * xhat), eval mode the folded scale alone
    float k0 = a[0], k1 = 0.f, k2 = 0.f, mu = 0.f;
    if (coef) { k0 = coef[0]; mu = mean[0]; k1 = -k0 * coef[2] * invstd[0]; k2 = -k0 * coef[1]; }
    float kw[V], sg[V], hg[V], sx[V], hx[V], aw[V], ab = 0.f;
#pragma unroll
    for (int e = 0; e < V; ++e) { kw[e] = 0.f; sg[e] = 0.f; hg[e] = 0.f; sx[e] = 0.f; hx[e] = 0.f; aw[e] = 0.f; }
    if (act) {
        load_rows<V>(sc_g, sh_g, c, sg, hg); load_rows<V>(sc_x, sh_x, c, sx, hx);
#pragma unroll
        for (int e = 0; e < V; ++e) kw[e] = (c + e < F) ? w[c + e] : 0.f;
        for (int m = r0 + rl; m < r1; m += R * RU) {
            uint4 vg[RU], vx[RU];
            float z[RU], pr[RU];
#pragma unroll
            for (int u = 0; u < RU; ++u) {
                const int mm = m + u * R;
                if (mm < r1) {
                    vg[u] = *reinterpret_cast<const uint4*>(rg + (size_t)mm * ld_g + c);
                    vx[u] = *reinterpret_cast<const uint4*>(rx + (size_t)mm * ld_x + c);
                    z[u] = dz[mm]; pr[u] = psi[mm];
                }
            }
#pragma unroll
            for (int u = 0; u < RU; ++u) {
                const int mm = m + u * R;
                if (mm < r1) {
                    float g[V], x[V], s[V], o[V];
                    TT<T>::unpack(vg[u], g); TT<T>::unpack(vx[u], x);
                    relu_sum<V>(g, x, sg, hg, sx, hx, s);
                    const float dp = fmaf(k0, z[u], fmaf(k1, pr[u] - mu, k2));
#pragma unroll
                    for (int e = 0; e < V; ++e) { o[e] = s[e] > 0.f ? dp * kw[e] : 0.f; aw[e] = fmaf(dp, s[e], aw[e]); }
                    stv<T>(ds + (size_t)mm * ld_ds + c, o);
                    if (cvl == 0) ab += dp;
                }
            }
        }
    }
    // the row lanes' sums, in lane order
#pragma unroll
    for (int e = 0; e < V; ++e) sh[(rl * CVP + cvl) * V + e] = aw[e];
    if (cvl == 0) shb[rl] = ab;
    __syncthreads();
    if (rl == 0 && act) {
#pragma unroll
        for (int e = 0; e < V; ++e) {
            float s = 0.f;
            for (int r = 0; r < R; ++r) s += sh[(r * CVP + cvl) * V + e];
            pw[(size_t)blockIdx.x * Fp + c + e] = (c + e < F) ? s : 0.f;
        }
    }
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int r = 0; r < R; ++r) s += shb[r];
        pb[blockIdx.x] = s;
    }
}

}  // namespace

extern "C" {

int pn2_ag_blocks(int dt, int M, int width_p, int kind) {
    if (M < 1 || width_p < 8 || width_p % 8 || kind < 0 || kind > 2 || (kind != 1 && width_p / vec_of(dt) > 64)) return -2;          // (the F_int-wide kernels take at most 64 vectors)
    return ag_plan_kind(dt, M, width_p, kind).nblk;
}

int pn2_ag_psi_rows(int dt, int M, int F_int_p) {
    if (M < 1 || F_int_p < 8 || F_int_p % 8 || F_int_p / vec_of(dt) > 64) return -2;
    return ag_plan_kind(dt, M, F_int_p, 0).rows;
}

int pn2_ag_psi_fwd(int dt, const void* raw_g, int ld_g, const float* scale_g, const float* shift_g, const void* raw_x, int ld_x, const float* scale_x, const float* shift_x,
                   const float* w_psi, int F_int, int F_int_p, int M, float* psi_raw, float* pmean, float* pm2, void* stream) {
    if (!raw_g || !raw_x || !w_psi || !psi_raw || (pmean == nullptr) != (pm2 == nullptr) || (scale_g == nullptr) != (shift_g == nullptr) || (scale_x == nullptr) != (shift_x == nullptr)) return -1;
    const int V = vec_of(dt);
    if (M < 1 || F_int < 1 || F_int > F_int_p || F_int_p % 8 || F_int_p / V > 64 || ld_g < F_int_p || ld_x < F_int_p || ld_g % V || ld_x % V || !al16(raw_g) || !al16(raw_x)) return -2;
    const AgPlan p = ag_plan_kind(dt, M, F_int_p, 0);
    return with_storage_dtype(dt, [&](auto t) {
        using T = type_of<decltype(t)>;
        return pn2_launch<ag_psi_fwd_k<T>>(dim3(p.nblk), dim3(256), 0, 0, (hipStream_t)stream, (const T*)raw_g, ld_g, scale_g, shift_g, (const T*)raw_x, ld_x, scale_x, shift_x,
                                           w_psi, F_int, F_int_p, M, psi_raw, pmean, pm2, p.rows, p.cvp);
    });
}

int pn2_ag_apply_fwd(int dt, const void* g, int ld_g, const void* x, int ld_x, const float* psi_raw, const float* a, const float* b, void* out, int ld_out,
                     int M, int C, int Cp, void* stream) {
    if (!g || !x || !psi_raw || !a || !b || !out) return -1;
    const int V = vec_of(dt);
    if (M < 1 || C < 1 || C > Cp || Cp % 8 || ld_g < Cp || ld_x < Cp || ld_out < Cp || ld_g % V || ld_x % V || ld_out % V || !al16(g) || !al16(x) || !al16(out)) return -2;
    return with_storage_dtype(dt, [&](auto t) {
        using T = type_of<decltype(t)>;
        return pn2_launch<ag_apply_fwd_k<T>>(dim3(grid_for((size_t)M * (Cp / V), GRID_CAP)), dim3(256), 0, 0, (hipStream_t)stream, (const T*)g, ld_g, (const T*)x, ld_x, psi_raw, a, b,
                                             (T*)out, ld_out, M, C, Cp);
    });
}

int pn2_ag_bwd_gate(int dt, const void* dout, int ld_dout, const void* x, int ld_x, const float* psi_raw, const float* a, const float* b, const float* mean, const float* invstd,
                    void* dx, int ld_dx, int dx_accum, void* dg, int ld_dg, int dg_accum, float* dz, float* p1, float* p2, int M, int C, int Cp, void* stream) {
    if (!dout || !x || !psi_raw || !a || !b || !dz || !p1 || !p2 || (mean == nullptr) != (invstd == nullptr)) return -1;
    const int V = vec_of(dt);
    if (M < 1 || C < 1 || C > Cp || Cp % 8 || ld_dout < Cp || ld_x < Cp || ld_dout % V || ld_x % V || !al16(dout) || !al16(x)) return -2;
    if ((dx && (ld_dx < Cp || ld_dx % V || !al16(dx))) || (dg && (ld_dg < Cp || ld_dg % V || !al16(dg)))) return -2;
    const AgPlan p = ag_plan_kind(dt, M, Cp, 1);
    return with_storage_dtype(dt, [&](auto t) {
        using T = type_of<decltype(t)>;
        return pn2_launch<ag_bwd_gate_k<T>>(dim3(p.nblk), dim3(256), 0, 0, (hipStream_t)stream, (const T*)dout, ld_dout, (const T*)x, ld_x, psi_raw, a, b, mean, invstd,
                                            (T*)dx, ld_dx, dx_accum, (T*)dg, ld_dg, dg_accum, dz, p1, p2, M, C, Cp, p.rows, p.cvp);
    });
}

int pn2_ag_apply_cat_fwd(int dt, const void* g, int ld_g, const void* x, int ld_x, const float* psi_raw, const float* a, const float* b, void* out, int ld_out,
                         int M, int C, int Cp, void* stream) {
    if (!g || !x || !psi_raw || !a || !b || !out) return -1;
    const int V = vec_of(dt);
    if (M < 1 || C < 8 || C % 8 || Cp != C || ld_g < C || ld_x < C || ld_out < 2 * C || ld_g % V || ld_x % V || ld_out % V || !al16(g) || !al16(x) || !al16(out)) return -2;
    return with_storage_dtype(dt, [&](auto t) {
        using T = type_of<decltype(t)>;
        return pn2_launch<ag_apply_cat_fwd_k<T>>(dim3(grid_for((size_t)M * (C / V), GRID_CAP)), dim3(256), 0, 0, (hipStream_t)stream, (const T*)g, ld_g, (const T*)x, ld_x, psi_raw, a, b,
                                                 (T*)out, ld_out, M, C);
    });
}

int pn2_ag_bwd_gate_cat(int dt, const void* dout, int ld_dout, const void* x, int ld_x, const float* psi_raw, const float* a, const float* b, const float* mean, const float* invstd,
                        void* dx, int ld_dx, int dx_accum, void* dg, int ld_dg, int dg_accum, float* dz, float* p1, float* p2, int M, int C, int Cp, void* stream) {
    if (!dout || !x || !psi_raw || !a || !b || !dz || !p1 || !p2 || (mean == nullptr) != (invstd == nullptr)) return -1;
    const int V = vec_of(dt);
    if (M < 1 || C < 8 || C % 8 || Cp != C || ld_dout < 2 * C || ld_x < C || ld_dout % V || ld_x % V || !al16(dout) || !al16(x)) return -2;
    if ((dx && (ld_dx < C || ld_dx % V || !al16(dx))) || (dg && (ld_dg < C || ld_dg % V || !al16(dg)))) return -2;
    const AgPlan p = ag_plan_kind(dt, M, C, 1);          // (the plan of pn2_ag_bwd_gate at this width: p1 / p2 hold pn2_ag_blocks(dt, M, C, 1) rows)
    return with_storage_dtype(dt, [&](auto t) {
        using T = type_of<decltype(t)>;
        return pn2_launch<ag_bwd_gate_cat_k<T>>(dim3(p.nblk), dim3(256), 0, 0, (hipStream_t)stream, (const T*)dout, ld_dout, (const T*)x, ld_x, psi_raw, a, b, mean, invstd,
                                                (T*)dx, ld_dx, dx_accum, (T*)dg, ld_dg, dg_accum, dz, p1, p2, M, C, p.rows, p.cvp);
    });
}

int pn2_ag_bwd_sum(int dt, const float* dz, const float* psi_raw, const float* a, const float* mean, const float* invstd, const float* coef,
                   const void* raw_g, int ld_g, const float* scale_g, const float* shift_g, const void* raw_x, int ld_x, const float* scale_x, const float* shift_x,
                   const float* w_psi, int F_int, int F_int_p, int M, void* dsum, int ld_dsum, float* pw, float* pb, void* stream) {
    if (!dz || !psi_raw || !a || !raw_g || !raw_x || !w_psi || !dsum || !pw || !pb || (coef && (!mean || !invstd))
        || (scale_g == nullptr) != (shift_g == nullptr) || (scale_x == nullptr) != (shift_x == nullptr)) return -1;
    const int V = vec_of(dt);
    if (M < 1 || F_int < 1 || F_int > F_int_p || F_int_p % 8 || F_int_p / V > 64 || ld_g < F_int_p || ld_x < F_int_p || ld_dsum < F_int_p || ld_g % V || ld_x % V || ld_dsum % V
        || !al16(raw_g) || !al16(raw_x) || !al16(dsum)) return -2;
    const AgPlan p = ag_plan_kind(dt, M, F_int_p, 2);
    return with_storage_dtype(dt, [&](auto t) {
        using T = type_of<decltype(t)>;
        return pn2_launch<ag_bwd_sum_k<T>>(dim3(p.nblk), dim3(256), 0, 0, (hipStream_t)stream, dz, psi_raw, a, mean, invstd, coef, (const T*)raw_g, ld_g, scale_g, shift_g,
                                           (const T*)raw_x, ld_x, scale_x, shift_x, w_psi, F_int, F_int_p, M, (T*)dsum, ld_dsum, pw, pb, p.rows, p.cvp);
    });
}

}  // extern "C"
