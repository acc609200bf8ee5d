// pn2_seg.hip — the multi-class volume evaluation of the reference's test_single_volume / val_single_volume (multiclass_seg/EMCAD/utils/utils.py:140-301) on the GPU:
//   label map        argmax over the K channels of the combined logits of 1..8 maps               -> pn2_seg_labels
//   dc / jc          |pred = c|, |gt = c|, |pred = c and gt = c| for every class                  -> pn2_seg_counts
//   hd95 / assd      medpy's __surface_distances: for every border voxel of A the exact squared Euclidean distance to the nearest border voxel of B,
//                    as a histogram over d^2                                                        -> pn2_seg_surface_hist
// pn2_seg_labels takes the argmax of the combined LOGITS; the reference takes argmax(softmax(logits)) (utils.py:195,273).  softmax is monotone, so the two differ
// only where fp32 softmax rounds two distinct logits to one probability (then the reference returns the lower index and this kernel the larger logit).
// Everything that decides a metric is an integer (labels, voxel counts, squared distances in voxels) accumulated with integer atomics: exact and independent of
// the order of execution.  The host finishes in float64 with medpy's expressions (pn2/voleval.py).
//
// Surface distances, for class c and label volumes A, B [D][H][W]:
//   border(V) = voxels with label c that have a face neighbour without it, outside the volume counting as "without" (mask ^ binary_erosion(mask) with
//               generate_binary_structure(ndim, 1), border value 0); ndim = 2 ignores the z neighbours.
//   seg_bbox_k   bounding boxes of the class-c voxels of A and of B (integer atomicMin / atomicMax): B's border lies inside B's box, A's inside A's
//   seg_rows_k   f1[z][y][x] = (x - x')^2 to the nearest border voxel x' of B in row (z, y); only rows inside B's box, only x inside A's box; counts B's border
//   seg_cols_k   f2[z][y][x] = min over y' in B's box of f1[z][y'][x] + (y - y')^2; only z inside B's box, only (y, x) inside A's box
//   seg_hist_k   at every border voxel of A: d^2 = min over z' in B's box of f2[z'][y][x] + (z - z')^2 -> hist[d^2] += 1; counts A's border
// int32 throughout: SEG_INF + 2 * 1023^2 < 2^31.  The boxes are read from device memory by every kernel: no host round trip.
#include "pn2_common.h"
#include "../../include/pn2.h"

namespace {

typedef unsigned long long u64;
typedef unsigned char u8;
constexpr int SEG_INF = 1 << 29;
constexpr int SEG_MAX_AXIS = 1024;

struct SegMaps { const float* p[8]; };

// one thread per pixel; channel k of map m at (n, k, p) is m[(n*K + k)*HW + p]: consecutive lanes read consecutive floats of one channel plane
template <int MODE>
__global__ __launch_bounds__(256) void seg_labels_k(SegMaps maps, int nmaps, int N, int K, long long HW, u8* __restrict__ out) {
    const long long total = (long long)N * HW;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long n = i / HW, p = i - n * HW;
        const size_t base = (size_t)n * K * HW + p;
        float best = 0.f; int bk = 0;
        for (int k = 0; k < K; ++k) {
            const size_t o = base + (size_t)k * HW;
            float v;
            if (MODE == 0) v = maps.p[nmaps - 1][o];
            else if (MODE == 1) { v = 0.0f; for (int m = 0; m < nmaps; ++m) v += maps.p[m][o]; }
            else { const int h = nmaps / 2; v = 0.0f; for (int m = 0; m < h; ++m) v += (maps.p[m][o] - maps.p[h + m][o]); }
            // torch.argmax: first maximum, a NaN counts as the maximum
            if (k == 0 || v > best || (v != v && best == best)) { best = v; bk = k; }
        }
        out[i] = (u8)bk;
    }
}

// ---- labels straight from the low-resolution head maps: bilinear up-sampling (align_corners = 0, scale s = OH / H per map), combination and argmax in one pass
struct SegUpMaps { const float* p[8]; int ld[8], H[8], W[8]; float r[8]; };          // r = 1 / s, as Engine.bilinear hands it to bilinear_fwd_k

// the four-tap value ly0*(lx0*a + lx1*b) + ly1*(lx0*c + lx1*d) of bilinear_fwd_k (pn2_spatial.hip).  There the compiler chooses which product of each sum is fused into
// a multiply-add, and chooses differently per instantiation and, after it has packed pairs of channels into v_pk_fma_f32, per channel (its 16-byte and 12-byte forms
// up-sample the same map to values one rounding apart; the scalar form leaves the outer sum as mul, mul, add) - so no way of writing the expression here reproduces
// its bits for every map layout.  This kernel pins ONE form for every channel, read path and K: x = fma(lx0, a, lx1*b), y = fma(lx0, c, lx1*d), value =
// fma(ly0, x, ly1*y).  Where every product and sum is exact all forms agree; elsewhere the value is within the three roundings of the expression of bilinear_fwd_k's.
__device__ __forceinline__ float seg_tap4(float ly0, float ly1, float lx0, float lx1, float a, float b, float c, float d) {
#pragma clang fp contract(off)
    const float x = __builtin_fmaf(lx0, a, lx1 * b), y = __builtin_fmaf(lx0, c, lx1 * d);
    return __builtin_fmaf(ly0, x, ly1 * y);
}

// v[0 .. 4*KV) = channels of map m at output pixel (n, oy, ox).  Tap offsets and weights once per map; VEC: the channels of a tap as 16-byte vectors (the
// pad channels up to 4*KV <= ld are read and never used), else scalars below K only
template <int KV, bool VEC>
__device__ __forceinline__ void seg_up_pixel(const SegUpMaps& maps, int m, int n, int oy, int ox, int K, float* v) {
    const int H = maps.H[m], W = maps.W[m], ld = maps.ld[m];
    const float r = maps.r[m];
    int y0, y1, x0, x1; float ly0, ly1, lx0, lx1;
    bl_src(oy, r, 0, H, y0, y1, ly0, ly1); bl_src(ox, r, 0, W, x0, x1, lx0, lx1);
    const float* b = maps.p[m] + (size_t)n * H * W * ld;
    const float* pa = b + (size_t)(y0 * W + x0) * ld; const float* pb = b + (size_t)(y0 * W + x1) * ld;
    const float* pc = b + (size_t)(y1 * W + x0) * ld; const float* pd = b + (size_t)(y1 * W + x1) * ld;
#pragma unroll
    for (int j = 0; j < KV; ++j) {
        float ta[4], tb[4], tc[4], td[4];
        if (VEC) {
            const f32x4_t va = ((const f32x4_t*)pa)[j], vb = ((const f32x4_t*)pb)[j], vc = ((const f32x4_t*)pc)[j], vd = ((const f32x4_t*)pd)[j];
#pragma unroll
            for (int e = 0; e < 4; ++e) { ta[e] = va[e]; tb[e] = vb[e]; tc[e] = vc[e]; td[e] = vd[e]; }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int k = 4 * j + e;
                const bool in = k < K;
                ta[e] = in ? pa[k] : 0.f; tb[e] = in ? pb[k] : 0.f; tc[e] = in ? pc[k] : 0.f; td[e] = in ? pd[k] : 0.f;
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * j + e] = seg_tap4(ly0, ly1, lx0, lx1, ta[e], tb[e], tc[e], td[e]);
    }
}

// one thread per output pixel, a wave = 64 consecutive x of one row, a block = 4 rows; 4*KV >= K running sums in registers, the maps as the outer loop so that every
// channel adds them in the order of seg_labels_k.  The sums and differences are plain fp32 adds of the rounded up-sampled values (what the unfused path stores and
// reads back): no contraction of an add into the four-tap expression
template <int MODE, int KV, bool VEC>
__global__ __launch_bounds__(256) void seg_labels_up_k(SegUpMaps maps, int nmaps, int K, int OH, int OW, u8* __restrict__ out) {
    const int ox = blockIdx.x * 64 + (threadIdx.x & 63), oy = blockIdx.y * 4 + (threadIdx.x >> 6), n = blockIdx.z;
    if (ox >= OW || oy >= OH) return;
    float acc[4 * KV];
    if (MODE == 0) seg_up_pixel<KV, VEC>(maps, nmaps - 1, n, oy, ox, K, acc);
    else {
#pragma unroll
        for (int k = 0; k < 4 * KV; ++k) acc[k] = 0.0f;
        const int h = nmaps / 2;
        for (int m = 0; m < (MODE == 1 ? nmaps : h); ++m) {
            float f[4 * KV], g[4 * KV];
            seg_up_pixel<KV, VEC>(maps, m, n, oy, ox, K, f);
            if (MODE == 2) seg_up_pixel<KV, VEC>(maps, h + m, n, oy, ox, K, g);
            {
#pragma clang fp contract(off)
#pragma unroll
                for (int k = 0; k < 4 * KV; ++k) { if (MODE == 1) acc[k] += f[k]; else acc[k] += (f[k] - g[k]); }
            }
        }
    }
    float best = 0.f; int bk = 0;
#pragma unroll
    for (int k = 0; k < 4 * KV; ++k) {
        const float v = acc[k];
        if (k < K && (k == 0 || v > best || (v != v && best == best))) { best = v; bk = k; }
    }
    out[((size_t)n * OH + oy) * OW + ox] = (u8)bk;
}

// ---- flip test-time augmentation (tta_model, utils.py:303-325): the maps hold V * N samples, view v of sample n at v * N + n; view code bit 0 = x mirrored,
// bit 1 = y mirrored.  Up-sampling a view's map and flipping the result back is reading the up-sampled map at the mirrored output pixel: the same seg_up_combined,
// the same bits.  The views are then added in their order, as combined logits (AVG 0) or as max-subtracted softmax probabilities (AVG 1), before the argmax.
// The reference divides the sum by V; the argmax does not see a positive factor, so the sum is left undivided.
// (seg_labels_up_k keeps its own copy of the combination: routed through seg_up_combined the compiler schedules it differently, and its device code is pinned.)
struct SegViews { int code[4]; };

// the combined logits of seg_labels_up_k at pixel (oy, ox) of sample n: the same expressions in the same order
template <int MODE, int KV, bool VEC>
__device__ __forceinline__ void seg_up_combined(const SegUpMaps& maps, int nmaps, int n, int oy, int ox, int K, float* acc) {
    if (MODE == 0) seg_up_pixel<KV, VEC>(maps, nmaps - 1, n, oy, ox, K, acc);
    else {
#pragma unroll
        for (int k = 0; k < 4 * KV; ++k) acc[k] = 0.0f;
        const int h = nmaps / 2;
        for (int m = 0; m < (MODE == 1 ? nmaps : h); ++m) {
            float f[4 * KV], g[4 * KV];
            seg_up_pixel<KV, VEC>(maps, m, n, oy, ox, K, f);
            if (MODE == 2) seg_up_pixel<KV, VEC>(maps, h + m, n, oy, ox, K, g);
            {
#pragma clang fp contract(off)
#pragma unroll
                for (int k = 0; k < 4 * KV; ++k) { if (MODE == 1) acc[k] += f[k]; else acc[k] += (f[k] - g[k]); }
            }
        }
    }
}

template <int MODE, int KV, bool VEC, int AVG>
__global__ __launch_bounds__(256) void seg_labels_up_tta_k(SegUpMaps maps, int nmaps, int K, int OH, int OW, int N, SegViews views, int V, u8* __restrict__ out) {
    const int ox = blockIdx.x * 64 + (threadIdx.x & 63), oy = blockIdx.y * 4 + (threadIdx.x >> 6), n = blockIdx.z;
    if (ox >= OW || oy >= OH) return;
    float tot[4 * KV];
    for (int v = 0; v < V; ++v) {
        const int code = views.code[v];
        float lg[4 * KV];
        seg_up_combined<MODE, KV, VEC>(maps, nmaps, v * N + n, (code & 2) ? OH - 1 - oy : oy, (code & 1) ? OW - 1 - ox : ox, K, lg);
        if (AVG == 1) {          // softmax over the channels below K; a NaN logit makes every probability of the view NaN, as torch.softmax does
#pragma clang fp contract(off)
            float mx = lg[0];
#pragma unroll
            for (int k = 1; k < 4 * KV; ++k) if (k < K) mx = fmaxf(mx, lg[k]);
            float s = 0.0f;
#pragma unroll
            for (int k = 0; k < 4 * KV; ++k) { lg[k] = k < K ? expf(lg[k] - mx) : 0.0f; s += lg[k]; }
            const float rs = 1.0f / s;          // s >= 1: the largest logit contributes exp(0)
#pragma unroll
            for (int k = 0; k < 4 * KV; ++k) lg[k] *= rs;
        }
        {
#pragma clang fp contract(off)
#pragma unroll
            for (int k = 0; k < 4 * KV; ++k) tot[k] = v == 0 ? lg[k] : tot[k] + lg[k];
        }
    }
    float best = 0.f; int bk = 0;
#pragma unroll
    for (int k = 0; k < 4 * KV; ++k) {
        const float t = tot[k];
        if (k < K && (k == 0 || t > best || (t != t && best == best))) { best = t; bk = k; }
    }
    out[((size_t)n * OH + oy) * OW + ox] = (u8)bk;
}

// out[v * N + n][y][x] = src[n][y'][x'] with (y', x') the pixel mirrored by view v's code: raw bits.  VEC: four x per thread, one 16-byte load (of the mirrored
// quad, reversed in registers) and one 16-byte store; W % 4 == 0 keeps both aligned
template <bool VEC>
__global__ __launch_bounds__(256) void flip_views_k(const float* __restrict__ src, int N, int H, int W, SegViews views, float* __restrict__ out, size_t total) {
    const int Wq = VEC ? W / 4 : W;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const int q = (int)(idx % Wq);
        size_t r = idx / Wq;
        const int y = (int)(r % H); r /= H;
        const int n = (int)(r % N), v = (int)(r / N);
        const int code = views.code[v];
        const float* row = src + ((size_t)n * H + ((code & 2) ? H - 1 - y : y)) * W;
        if (VEC) {
            f32x4_t t = ((const f32x4_t*)row)[(code & 1) ? Wq - 1 - q : q];
            if (code & 1) t = f32x4_t{t[3], t[2], t[1], t[0]};
            ((f32x4_t*)out)[idx] = t;
        } else out[idx] = row[(code & 1) ? W - 1 - q : q];
    }
}

// cnt[c][0..2] += |pred = c|, |gt = c|, |pred = c and gt = c|: LDS counters per block, then one atomic per non-zero counter
__global__ __launch_bounds__(256) void seg_counts_k(const u8* __restrict__ pred, const u8* __restrict__ gt, long long n, int K, u64* __restrict__ cnt) {
    __shared__ unsigned sh[256 * 3];
    for (int j = threadIdx.x; j < K * 3; j += 256) sh[j] = 0;
    __syncthreads();
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int a = pred[i], b = gt[i];
        if (a < K) atomicAdd(&sh[a * 3], 1u);
        if (b < K) atomicAdd(&sh[b * 3 + 1], 1u);
        if (a == b && a < K) atomicAdd(&sh[a * 3 + 2], 1u);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < K * 3; j += 256) if (sh[j]) atomicAdd(cnt + j, (u64)sh[j]);
}

// meta[0..5] = A's box {zmin, zmax, ymin, ymax, xmin, xmax}, meta[6..11] = B's; an empty box has min > max
__global__ void seg_meta_init_k(int* __restrict__ meta) {
    if (threadIdx.x < 12) meta[threadIdx.x] = ((threadIdx.x & 1) ? -1 : 0x7fffffff);
}

__device__ __forceinline__ void wave_box(int* meta, bool on, int z, int y, int x) {
    int v[6] = { on ? z : 0x7fffffff, on ? z : -1, on ? y : 0x7fffffff, on ? y : -1, on ? x : 0x7fffffff, on ? x : -1 };
    if (!__any(on)) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int j = 0; j < 6; ++j) { const int t = __shfl_xor(v[j], o); v[j] = (j & 1) ? max(v[j], t) : min(v[j], t); }
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int j = 0; j < 6; ++j) { if (j & 1) atomicMax(meta + j, v[j]); else atomicMin(meta + j, v[j]); }
}

__global__ __launch_bounds__(256) void seg_bbox_k(const u8* __restrict__ A, const u8* __restrict__ B, int D, int H, int W, int c, int* __restrict__ meta) {
    const long long n = (long long)D * H * W, HWl = (long long)H * W;
    const long long span = (long long)gridDim.x * 256;
    for (long long i0 = (long long)blockIdx.x * 256; i0 < n; i0 += span) {          // whole waves enter wave_box together
        const long long i = i0 + threadIdx.x;
        const bool in = i < n;
        const int z = in ? (int)(i / HWl) : 0;
        const long long r = in ? i - (long long)z * HWl : 0;
        const int y = (int)(r / W), x = (int)(r - (long long)y * W);
        wave_box(meta, in && A[i] == c, z, y, x);
        wave_box(meta + 6, in && B[i] == c, z, y, x);
    }
}

__device__ __forceinline__ bool seg_border(const u8* __restrict__ V, int D, int H, int W, int c, int ndim, int z, int y, int x) {
    const size_t HWs = (size_t)H * W, i = (size_t)z * HWs + (size_t)y * W + x;
    if (V[i] != c) return false;
    if (x == 0 || x == W - 1 || y == 0 || y == H - 1) return true;
    if (V[i - 1] != c || V[i + 1] != c || V[i - W] != c || V[i + W] != c) return true;
    if (ndim == 3) {
        if (z == 0 || z == D - 1) return true;
        if (V[i - HWs] != c || V[i + HWs] != c) return true;
    }
    return false;
}

// one block per row (z, y) of B's box: the row's border bits as sixteen 64-bit words in LDS (one ballot per wave and 256 columns), then per column the nearest
// set bit on either side
__global__ __launch_bounds__(256) void seg_rows_k(const u8* __restrict__ B, int D, int H, int W, int c, int ndim, const int* __restrict__ meta, int* __restrict__ f1,
                                                  unsigned* __restrict__ counts) {
    __shared__ u64 bits[SEG_MAX_AXIS / 64];
    const int y = blockIdx.x, z = blockIdx.y;
    if (z < meta[6] || z > meta[7] || y < meta[8] || y > meta[9]) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned nb = 0;
    for (int x0 = 0; x0 < W; x0 += 256) {
        const int x = x0 + threadIdx.x;
        const u64 m = __ballot(x < W && seg_border(B, D, H, W, c, ndim, z, y, x));
        if (lane == 0) { bits[(x0 >> 6) + wv] = m; nb += (unsigned)__popcll(m); }
    }
    if (lane == 0 && nb) atomicAdd(counts + 1, nb);
    __syncthreads();
    const int nw = (W + 63) >> 6, xa = meta[4], xb = meta[5];
    if (xa > xb) return;                                       // A has no voxel of the class: nothing will ask for a distance
    int* __restrict__ row = f1 + ((size_t)z * H + y) * W;
    for (int x = xa + (int)threadIdx.x; x <= xb; x += 256) {
        const int w0 = x >> 6, b = x & 63;
        int best = SEG_INF;
        u64 m = bits[w0] & (~0ULL >> (63 - b));                // bits at or below x
        for (int w = w0; ; ) {
            if (m) { const int d = x - ((w << 6) + 63 - __clzll((long long)m)); best = d * d; break; }
            if (--w < 0) break;
            m = bits[w];
        }
        m = bits[w0] & (~0ULL << b);                           // bits at or above x
        for (int w = w0; ; ) {
            if (m) { const int d = ((w << 6) + __ffsll((long long)m) - 1) - x; best = min(best, d * d); break; }
            if (++w >= nw) break;
            m = bits[w];
        }
        row[x] = best;
    }
}

// a block = 64 columns x 64 output rows of one slice z: thread (tx, ty) keeps the 16 outputs y0 + ty + 4k in registers and walks the candidate rows y' of B's box;
// the 64 lanes of a wave read 64 consecutive f1 values of one candidate row
__global__ __launch_bounds__(256) void seg_cols_k(int H, int W, const int* __restrict__ meta, const int* __restrict__ f1, int* __restrict__ f2) {
    const int z = blockIdx.z;
    const int ya = meta[2], yb = meta[3], xa = meta[4], xb = meta[5];
    if (z < meta[6] || z > meta[7] || xa > xb) return;
    const int x0 = blockIdx.x * 64, y0 = blockIdx.y * 64;
    if (x0 > xb || x0 + 63 < xa || y0 > yb || y0 + 63 < ya) return;
    const int x = x0 + (threadIdx.x & 63), ty = threadIdx.x >> 6;
    if (x < xa || x > xb) return;
    int best[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) best[k] = SEG_INF;
    const int* __restrict__ src = f1 + (size_t)z * H * W + x;
    const int cb = meta[9];
    for (int yc = meta[8]; yc <= cb; ++yc) {
        const int v = src[(size_t)yc * W];
        const int d0 = y0 + ty - yc;
#pragma unroll
        for (int k = 0; k < 16; ++k) { const int d = d0 + 4 * k; best[k] = min(best[k], v + d * d); }
    }
    int* __restrict__ dst = f2 + (size_t)z * H * W + x;
#pragma unroll
    for (int k = 0; k < 16; ++k) { const int y = y0 + ty + 4 * k; if (y >= ya && y <= yb) dst[(size_t)y * W] = best[k]; }
}

// every voxel of A's box: a border voxel takes the min-plus over the slices of B's box and adds one to its histogram bin
__global__ __launch_bounds__(256) void seg_hist_k(const u8* __restrict__ A, int D, int H, int W, int c, int ndim, const int* __restrict__ meta, const int* __restrict__ f2,
                                                  unsigned* __restrict__ hist, int nhist, unsigned* __restrict__ counts) {
    const int za = meta[0], zb = meta[1], ya = meta[2], yb = meta[3], xa = meta[4], xb = meta[5];
    if (za > zb) return;
    const long long bw = xb - xa + 1, bh = yb - ya + 1, n = bw * bh * (zb - za + 1);
    const int sa = meta[6], sb = meta[7];
    const size_t HWs = (size_t)H * W;
    unsigned na = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int z = za + (int)(i / (bw * bh));
        const long long r = i - (long long)(z - za) * bw * bh;
        const int y = ya + (int)(r / bw), x = xa + (int)(r - (long long)(y - ya) * bw);
        if (!seg_border(A, D, H, W, c, ndim, z, y, x)) continue;
        ++na;
        int best = SEG_INF;
        const int* __restrict__ col = f2 + (size_t)y * W + x;
        for (int zc = sa; zc <= sb; ++zc) { const int d = z - zc; best = min(best, col[(size_t)zc * HWs] + d * d); }
        if (best < nhist) atomicAdd(hist + best, 1u);          // (B without a border: nothing to measure, the bins stay empty)
    }
    for (int o = 32; o > 0; o >>= 1) na += __shfl_xor(na, o);
    if ((threadIdx.x & 63) == 0 && na) atomicAdd(counts, na);
}

bool seg_dims_ok(int D, int H, int W, int ndim) {
    return D >= 1 && H >= 1 && W >= 1 && D <= SEG_MAX_AXIS && H <= SEG_MAX_AXIS && W <= SEG_MAX_AXIS && (ndim == 3 || (ndim == 2 && D == 1));
}

// the map table of pn2_seg_labels_up / _tta: every row checked, r = 1 / s, vec = all rows readable as 16-byte vectors
int seg_up_table(const pn2_seg_up_map* maps, int nmaps, int K, int OH, int OW, SegUpMaps& m, bool& vec) {
    vec = true;
    for (int i = 0; i < nmaps; ++i) {
        const pn2_seg_up_map& s = maps[i];
        if (!s.p) return -1;
        if (s.ld < K || s.H < 1 || s.W < 1 || OH % s.H || OW % s.W || OH / s.H != OW / s.W) return -2;
        m.p[i] = s.p; m.ld[i] = s.ld; m.H[i] = s.H; m.W[i] = s.W;
        m.r[i] = (float)(1.0 / (double)(OH / s.H));
        vec = vec && s.ld % 4 == 0 && ((uintptr_t)s.p & 15) == 0;
    }
    return 0;
}

// 1..4 view codes 0..3, none twice
bool seg_views_ok(const int* views, int V, SegViews& sv) {
    if (V < 1 || V > 4) return false;
    unsigned seen = 0;
    for (int v = 0; v < V; ++v) {
        if (views[v] < 0 || views[v] > 3 || (seen >> views[v] & 1)) return false;
        seen |= 1u << views[v];
        sv.code[v] = views[v];
    }
    return true;
}

}  // namespace

extern "C" {

int pn2_seg_labels(const float* const* maps, int nmaps, int mode, int N, int K, int H, int W, unsigned char* out, void* stream) {
    if (!maps || !out || N < 1 || H < 1 || W < 1) return -1;
    if (K < 2 || K > 16 || nmaps < 1 || nmaps > 8 || mode < 0 || mode > 2 || (mode == 2 && (nmaps & 1))) return -2;
    SegMaps m;
    for (int i = 0; i < 8; ++i) { m.p[i] = i < nmaps ? maps[i] : nullptr; if (i < nmaps && !maps[i]) return -1; }
    const long long HW = (long long)H * W;
    const dim3 g(pn2_host::grid_for((size_t)N * HW, 65536));
    hipStream_t st = (hipStream_t)stream;
    return with_int<0, 1, 2>(mode, [&](auto mo) { return pn2_launch<seg_labels_k<decltype(mo)::value>>(g, dim3(256), 0, 0, st, m, nmaps, N, K, HW, out); });
}

// the map table of pn2_seg_labels_up / _tta: every row checked, r = 1 / s, vec = all rows readable as 16-byte vectors
static int seg_up_table(const pn2_seg_up_map* maps, int nmaps, int K, int OH, int OW, SegUpMaps& m, bool& vec) {
    vec = true;
    for (int i = 0; i < nmaps; ++i) {
        const pn2_seg_up_map& s = maps[i];
        if (!s.p) return -1;
        if (s.ld < K || s.H < 1 || s.W < 1 || OH % s.H || OW % s.W || OH / s.H != OW / s.W) return -2;
        m.p[i] = s.p; m.ld[i] = s.ld; m.H[i] = s.H; m.W[i] = s.W;
        m.r[i] = (float)(1.0 / (double)(OH / s.H));
        vec = vec && s.ld % 4 == 0 && ((uintptr_t)s.p & 15) == 0;
    }
    return 0;
}

// 1..4 view codes 0..3, none twice
static bool seg_views_ok(const int* views, int V, SegViews& sv) {
    if (V < 1 || V > 4) return false;
    unsigned seen = 0;
    for (int v = 0; v < V; ++v) {
        if (views[v] < 0 || views[v] > 3 || (seen >> views[v] & 1)) return false;
        seen |= 1u << views[v];
        sv.code[v] = views[v];
    }
    return true;
}

int pn2_seg_labels_up(const pn2_seg_up_map* maps, int nmaps, int mode, int N, int K, int OH, int OW, unsigned char* out, void* stream) {
    if (!maps || !out || N < 1 || OH < 1 || OW < 1) return -1;
    if (K < 2 || K > 16 || nmaps < 1 || nmaps > 8 || mode < 0 || mode > 2 || (mode == 2 && (nmaps & 1)) || N > 65535 || (OH + 3) / 4 > 65535) return -2;
    SegUpMaps m = {};
    bool vec;
    if (int rc = ::seg_up_table(maps, nmaps, K, OH, OW, m, vec)) return rc;
    const dim3 g((OW + 63) / 64, (OH + 3) / 4, N);
    hipStream_t st = (hipStream_t)stream;
    return with_int<0, 1, 2>(mode, [&](auto mo) { return with_int<1, 2, 3, 4>((K + 3) / 4, [&](auto kv) { return with_int<1, 0>(vec, [&](auto ve) {
        return pn2_launch<seg_labels_up_k<decltype(mo)::value, decltype(kv)::value, decltype(ve)::value != 0>>(g, dim3(256), 0, 0, st, m, nmaps, K, OH, OW, out);
    }); }); });
}

int pn2_seg_labels_up_tta(const pn2_seg_up_map* maps, int nmaps, int mode, const int* views, int V, int average, int N, int K, int OH, int OW, unsigned char* out,
                          void* stream) {
    if (!maps || !views || !out || N < 1 || OH < 1 || OW < 1) return -1;
    if (K < 2 || K > 16 || nmaps < 1 || nmaps > 8 || mode < 0 || mode > 2 || (mode == 2 && (nmaps & 1)) || N > 65535 || (OH + 3) / 4 > 65535) return -2;
    SegViews sv = {};
    // the kernel forms the sample index v * N + n as an int: already implied by N <= 65535 and V <= 4 above, stated here (with room to spare) for the day N's limit moves
    if (average < 0 || average > 1 || !::seg_views_ok(views, V, sv) || (long long)V * N > 0x7fffffffLL / 4) return -2;
    SegUpMaps m = {};
    bool vec;
    if (int rc = ::seg_up_table(maps, nmaps, K, OH, OW, m, vec)) return rc;
    const dim3 g((OW + 63) / 64, (OH + 3) / 4, N);
    hipStream_t st = (hipStream_t)stream;
    return with_int<0, 1, 2>(mode, [&](auto mo) { return with_int<1, 2, 3, 4>((K + 3) / 4, [&](auto kv) { return with_int<1, 0>(vec, [&](auto ve) {
        return with_int<0, 1>(average, [&](auto av) {
            return pn2_launch<seg_labels_up_tta_k<decltype(mo)::value, decltype(kv)::value, decltype(ve)::value != 0, decltype(av)::value>>(
                g, dim3(256), 0, 0, st, m, nmaps, K, OH, OW, N, sv, V, out);
        });
    }); }); });
}

int pn2_flip_views(const float* src, int N, int H, int W, const int* views, int V, float* out, void* stream) {
    if (!src || !views || !out || N < 1 || H < 1 || W < 1) return -1;
    SegViews sv = {};
    // flip_views_k splits a size_t index into int (v, n, y, q): the number of output samples has to fit an int (N has no other limit here)
    if (!::seg_views_ok(views, V, sv) || (long long)V * N > 0x7fffffffLL) return -2;
    const bool vec = W % 4 == 0 && (((uintptr_t)src | (uintptr_t)out) & 15) == 0;
    const size_t total = (size_t)V * N * H * (vec ? W / 4 : W);
    const dim3 g(pn2_host::grid_for(total, 16384));
    return with_int<1, 0>(vec, [&](auto ve) {
        return pn2_launch<flip_views_k<decltype(ve)::value != 0>>(g, dim3(256), 0, 0, (hipStream_t)stream, src, N, H, W, sv, out, total);
    });
}

int pn2_seg_counts(const unsigned char* pred, const unsigned char* gt, long long n, int K, unsigned long long* counts, void* stream) {
    if (!pred || !gt || !counts || n < 1) return -1;
    if (K < 1 || K > 256) return -2;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, (size_t)K * 3 * sizeof(unsigned long long), st) != hipSuccess) return -4;
    return pn2_launch<seg_counts_k>(dim3(pn2_host::grid_for((size_t)((n + 15) / 16), 2048)), dim3(256), 0, 0, st, pred, gt, n, K, counts);
}

int pn2_seg_surface_workspace(int D, int H, int W, int ndim, long long* bytes) {
    if (!bytes) return -1;
    if (!seg_dims_ok(D, H, W, ndim)) return -2;
    *bytes = 64 + 2LL * D * H * W * (long long)sizeof(int);
    return 0;
}

int pn2_seg_surface_hist_len(int D, int H, int W) {
    if (!seg_dims_ok(D, H, W, 3)) return -1;
    return (D - 1) * (D - 1) + (H - 1) * (H - 1) + (W - 1) * (W - 1) + 1;
}

int pn2_seg_surface_hist(const unsigned char* A, const unsigned char* B, int D, int H, int W, int cls, int ndim, unsigned* hist, unsigned* counts2, void* work, void* stream) {
    if (!A || !B || !hist || !counts2 || !work) return -1;
    if (!seg_dims_ok(D, H, W, ndim) || cls < 0 || cls > 255) return -2;
    hipStream_t st = (hipStream_t)stream;
    const int nhist = pn2_seg_surface_hist_len(D, H, W);
    const size_t n = (size_t)D * H * W;
    int* meta = (int*)work;
    int* f1 = meta + 16;
    int* f2 = f1 + n;
    if (hipMemsetAsync(hist, 0, (size_t)nhist * sizeof(unsigned), st) != hipSuccess || hipMemsetAsync(counts2, 0, 2 * sizeof(unsigned), st) != hipSuccess) return -4;
    if (int rc = pn2_launch<seg_meta_init_k>(dim3(1), dim3(64), 0, 0, st, meta)) return rc;
    if (int rc = pn2_launch<seg_bbox_k>(dim3(pn2_host::grid_for((n + 15) / 16, 2048)), dim3(256), 0, 0, st, A, B, D, H, W, cls, meta)) return rc;
    if (int rc = pn2_launch<seg_rows_k>(dim3(H, D), dim3(256), 0, 0, st, B, D, H, W, cls, ndim, (const int*)meta, f1, counts2)) return rc;
    if (int rc = pn2_launch<seg_cols_k>(dim3((W + 63) / 64, (H + 63) / 64, D), dim3(256), 0, 0, st, H, W, (const int*)meta, (const int*)f1, f2)) return rc;
    return pn2_launch<seg_hist_k>(dim3(pn2_host::grid_for((n + 3) / 4, 8192)), dim3(256), 0, 0, st, A, D, H, W, cls, ndim, (const int*)meta, (const int*)f2, hist, nhist, counts2);
}

}  // extern "C"
