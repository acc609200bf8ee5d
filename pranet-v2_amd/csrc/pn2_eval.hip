// pn2_eval.hip — the remaining metrics of the reference's eval_for_testAllInOne on the GPU (binary_seg/eval.py:18-66):
//   Sm   StructureMeasure   utils/eval_functions.py:5-94     -> pn2_eval_region_sums (integer moments of the four centroid quadrants; S_Object comes from the
//                                                                histograms of pn2_eval_hist)
//   wFm  original_WFb       utils/eval_functions.py:96-129   -> pn2_eval_wfm (exact Euclidean feature transform with scipy's tie-breaking, 7x7 Gaussian of the
//                                                                propagated error, weighted TP / FP sums)
//   meanEm EnhancedMeasure  utils/eval_functions.py:168-192  -> needs no kernel: for a binarised map the alignment matrix takes four values, so every
//                                                                threshold's score is a function of the two histograms (pn2/evaltail.py)
// All sums that decide a metric are integers (atomics on integers are order-independent) or fixed-order double reductions: deterministic.  The host finishes
// in float64 with the reference's expressions (pn2/evaltail.py), as it does for the threshold sweep.
//
// Every kernel body is a __device__ function of ONE image (its pointers, its size, the block's position in the image's own grid); the per-image entries run it
// over a 1-D grid, the ragged-batch entries (pn2_eval_tail_batch / pn2_eval_counts_batch / pn2_eval_wfm_batch, second half of this file) over blockIdx.y = image
// with the image's row of the device table.  The batch grid is sized for the largest image; a block past an image's own grid returns at once.
#include "pn2_common.h"
#include "pn2_evalcore.h"
#include "../../include/pn2.h"

namespace {

typedef unsigned long long u64;

__device__ __forceinline__ void block_add3(u64 a, u64 b, u64 c, u64* dst) {
    __shared__ u64 sh[3][4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); c += __shfl_xor(c, o); }
    if (lane == 0) { sh[0][wv] = a; sh[1][wv] = b; sh[2][wv] = c; }
    __syncthreads();
    if (threadIdx.x < 3) { const u64 s = sh[threadIdx.x][0] + sh[threadIdx.x][1] + sh[threadIdx.x][2] + sh[threadIdx.x][3]; if (s) atomicAdd(dst + threadIdx.x, s); }
    __syncthreads();
}

// blocks of the region-sum kernels / of wfm_sums_k for an image of n pixels (host and device: the batch kernels recompute an image's own grid from its row)
__host__ __device__ inline int region_blocks(long long n) { const long long g = (n + 256 * 8 - 1) / (256 * 8); return (int)(g < 1024 ? g : 1024); }
__host__ __device__ inline int wfm_blocks(long long n) { const long long g = (n + 255) / 256; return (int)(g < PN2_EVAL_WFM_MAX_BLOCKS ? g : PN2_EVAL_WFM_MAX_BLOCKS); }
__host__ __device__ inline int hist_blocks(long long n) { const long long g = (n + 256 * 16 - 1) / (256 * 16); return (int)(g < 1024 ? g : 1024); }

// out[0..2] = sum of row indices, sum of column indices, count of the pixels with gt > 0.5   (centroid of S_Region, eval_functions.py:28-35)
__device__ __forceinline__ void centroid_body(const float* __restrict__ gt, int H, int W, int blk, int nblk, u64* __restrict__ out) {
    u64 sr = 0, sc = 0, cnt = 0;
    const long long n = (long long)H * W;
    for (long long i = (long long)blk * 256 + threadIdx.x; i < n; i += (long long)nblk * 256)
        if (gt[i] > 0.5f) { const int r = (int)(i / W); sr += r; sc += (int)(i - (long long)r * W); ++cnt; }
    block_add3(sr, sc, cnt, out);
}
__global__ __launch_bounds__(256) void eval_centroid_k(const float* __restrict__ gt, int H, int W, u64* __restrict__ out) {
    centroid_body(gt, H, W, blockIdx.x, gridDim.x, out);
}

// out[3 + q*5 + {0..4}] = {pixels, sum k, sum k^2, sum g, sum k*g} of quadrant q = (row >= X) + 2*(col >= Y): LT, RT, LB, RB of divide() (eval_functions.py:37-48),
// k = prediction byte, g = gt > 0.5; X, Y = int(mean.round()) of the foreground rows / columns (numpy rounds half to even: rint), (H//2, W//2) without foreground
__device__ __forceinline__ void quadrants_body(const unsigned char* __restrict__ pred, const float* __restrict__ gt, int H, int W, int blk, int nblk, u64* __restrict__ out) {
    const u64 cnt = out[2];
    const int X = cnt ? (int)rint((double)out[0] / (double)cnt) : H / 2, Y = cnt ? (int)rint((double)out[1] / (double)cnt) : W / 2;
    u64 a[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { a[q][0] = 0; a[q][1] = 0; a[q][2] = 0; a[q][3] = 0; }
    const long long n = (long long)H * W;
    for (long long i = (long long)blk * 256 + threadIdx.x; i < n; i += (long long)nblk * 256) {
        const int r = (int)(i / W), c = (int)(i - (long long)r * W), q = (r >= X ? 1 : 0) + (c >= Y ? 2 : 0);
        const u64 k = pred[i], g = gt[i] > 0.5f ? 1 : 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) if (t == q) { a[t][0] += k; a[t][1] += k * k; a[t][2] += g; a[t][3] += k * g; }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        block_add3(a[q][0], a[q][1], a[q][2], out + 3 + q * 5 + 1);
        block_add3(a[q][3], 0, 0, out + 3 + q * 5 + 4);
    }
    if (blk == 0 && threadIdx.x < 4) {
        const int q = threadIdx.x;
        const long long rows = (q & 1) ? H - X : X, cols = (q & 2) ? W - Y : Y;
        out[3 + q * 5] = (u64)(rows * cols);
        if (q == 0) { out[23] = (u64)X; out[24] = (u64)Y; }
    }
}
__global__ __launch_bounds__(256) void eval_quadrants_k(const unsigned char* __restrict__ pred, const float* __restrict__ gt, int H, int W, u64* __restrict__ out) {
    quadrants_body(pred, gt, H, W, blockIdx.x, gridDim.x, out);
}

// ---- exact Euclidean feature transform with scipy's order of preference (ndimage.distance_transform_edt(return_indices=True): Maurer's sweep along axis 0,
// then along axis 1, keeping the earlier site unless the next one is STRICTLY closer):
// (1) per column j the nearest foreground row of every pixel, the smaller row on a tie (-1: no foreground in the column)
__device__ __forceinline__ void edt_col_body(const float* __restrict__ gt, int H, int W, int j, int* __restrict__ rcol) {
    int last = -1;
    for (int i = 0; i < H; ++i) { if (gt[(size_t)i * W + j] > 0.5f) last = i; rcol[(size_t)i * W + j] = last; }
    int nxt = -1;
    for (int i = H - 1; i >= 0; --i) {
        if (gt[(size_t)i * W + j] > 0.5f) nxt = i;
        const int a = rcol[(size_t)i * W + j];
        rcol[(size_t)i * W + j] = a < 0 ? nxt : (nxt < 0 || i - a <= nxt - i ? a : nxt);
    }
}
__global__ __launch_bounds__(256) void edt_cols_k(const float* __restrict__ gt, int H, int W, int* __restrict__ rcol) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < W) edt_col_body(gt, H, W, j, rcol);
}
// (2) over the columns' candidates (rcol[i][j'], j') the smallest squared distance, the smaller column on a tie; one block per row i, the row's candidates in LDS.
// et[i][j] = E at the nearest foreground pixel (E = |pred/255 - g|, eval_functions.py:97,102-103), dst[i][j] = the distance (foreground pixels: themselves, 0)
__device__ __forceinline__ void edt_row_body(const unsigned char* __restrict__ pred, const float* __restrict__ gt, int H, int W, int i, const int* __restrict__ rcol,
                                             double* __restrict__ et, double* __restrict__ dst, int* cand) {
    for (int j = threadIdx.x; j < W; j += 256) cand[j] = rcol[(size_t)i * W + j];
    __syncthreads();
    for (int j = threadIdx.x; j < W; j += 256) {
        long long best = 0x7fffffffffffffffLL; int bj = j;
        for (int c = 0; c < W; ++c) {
            const int r = cand[c];
            if (r >= 0) { const long long dr = r - i, dc = c - j, dd = dr * dr + dc * dc; if (dd < best) { best = dd; bj = c; } }
        }
        const int br = cand[bj];
        const size_t src = (size_t)(br < 0 ? i : br) * W + bj;          // (no foreground at all: the host never uses the result)
        et[(size_t)i * W + j] = fabs((double)pred[src] / 255.0 - (gt[src] > 0.5f ? 1.0 : 0.0));
        dst[(size_t)i * W + j] = sqrt((double)best);
    }
}
__global__ __launch_bounds__(256) void edt_rows_k(const unsigned char* __restrict__ pred, const float* __restrict__ gt, int H, int W, const int* __restrict__ rcol,
                                                  double* __restrict__ et, double* __restrict__ dst) {
    extern __shared__ int cand[];
    edt_row_body(pred, gt, H, W, blockIdx.x, rcol, et, dst, cand);
}
// (3) EA = convolve(Et, K, mode='nearest') with the 7x7 Gaussian (accumulated in scipy's order: the flipped kernel row-major), MIN_E_EA, B, Ew and the block's
// sums {Ew over foreground, Ew over background} in a fixed order -> part[block][2]
__device__ __forceinline__ void wfm_sums_body(const unsigned char* __restrict__ pred, const float* __restrict__ gt, int H, int W, const double* __restrict__ et,
                                              const double* __restrict__ dst, const double* __restrict__ K, double c5, int blk, int nblk, double* __restrict__ part) {
    __shared__ double sh[2][256];
    double sf = 0.0, sb = 0.0;
    const long long n = (long long)H * W;
    for (long long p = (long long)blk * 256 + threadIdx.x; p < n; p += (long long)nblk * 256) {
        const int i = (int)(p / W), j = (int)(p - (long long)i * W);
        const bool fg = gt[p] > 0.5f;
        const double E = fabs((double)pred[p] / 255.0 - (fg ? 1.0 : 0.0));
        double ew;
        if (fg) {
            double ea = 0.0;
            for (int a = 0; a < 7; ++a) {
                const int ii = min(max(i + a - 3, 0), H - 1);
                for (int b = 0; b < 7; ++b) { const int jj = min(max(j + b - 3, 0), W - 1); ea += K[(6 - a) * 7 + (6 - b)] * et[(size_t)ii * W + jj]; }
            }
            ew = ea < E ? ea : E;          // B = 1 on the foreground
            sf += ew;
        } else {
            ew = E * (2.0 - exp(c5 * dst[p]));
            sb += ew;
        }
    }
    sh[0][threadIdx.x] = sf; sh[1][threadIdx.x] = sb;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { sh[0][threadIdx.x] += sh[0][threadIdx.x + o]; sh[1][threadIdx.x] += sh[1][threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { part[blk * 2] = sh[0][0]; part[blk * 2 + 1] = sh[1][0]; }
}
__global__ __launch_bounds__(256) void wfm_sums_k(const unsigned char* __restrict__ pred, const float* __restrict__ gt, int H, int W, const double* __restrict__ et,
                                                  const double* __restrict__ dst, const double* __restrict__ K, double c5, double* __restrict__ part) {
    wfm_sums_body(pred, gt, H, W, et, dst, K, c5, blockIdx.x, gridDim.x, part);
}

// ------------------------------------------------------------------------------------------------ ragged batch
// Image b = blockIdx.y of a batch: its row of the device table, or false for an empty slot (H == 0) and for a row that does not fit what the host sized the
// launch and the buffers for (H, W above the grid's maxima, pixels outside [0, total)): such a row is skipped, nothing of it is read or written.
__device__ __forceinline__ bool batch_row(const pn2_eval_img* __restrict__ tab, int maxH, int maxW, long long total, pn2_eval_img& r) {
    r = tab[blockIdx.y];
    return r.H >= 1 && r.W >= 1 && r.H <= maxH && r.W <= maxW && r.off >= 0 && r.off + (long long)r.H * r.W <= total;
}

struct EvalMaps { const float* p[4]; };

// sigmoid of the bilinear sample (align_corners = 0) of m0 or of ((m0 + m1) + m2) + m3 at output pixel (oy, ox): pn2_add x3 -> bilinear_fwd_k<float, 1> -> the
// sigmoid of pn2_eval_tail, through the same inlined expressions (pn2_evalcore.h, bl_src)
template <int NM>
__device__ __forceinline__ float tail_sample(const EvalMaps& M, size_t base, int h, int w, int oy, int ox, float rh, float rw) {
    int y0, y1, x0, x1; float ly0, ly1, lx0, lx1;
    bl_src(oy, rh, 0, h, y0, y1, ly0, ly1); bl_src(ox, rw, 0, w, x0, x1, lx0, lx1);
    const auto at = [&](int y, int x) {
        const size_t i = base + (size_t)(y * w + x);
        float s = M.p[0][i];
        if (NM == 4) s = ((s + M.p[1][i]) + M.p[2][i]) + M.p[3][i];
        return s;
    };
    return eval_sigmoid(bl_tap4(ly0, ly1, lx0, lx1, at(y0, x0), at(y0, x1), at(y1, x0), at(y1, x1)));
}

// pass 1: min and max of the sigmoid over every image, by integer atomics on the order-preserving code of a float (exact under any order, so the bytes of
// pass 2 do not depend on the grid).  mm[b] = { ~code(min), code(max) }: both grow, so one memset to zero starts every image.
template <int NM>
__global__ __launch_bounds__(256) void tail_minmax_batch_k(EvalMaps M, int h, int w, const pn2_eval_img* __restrict__ tab, int maxH, int maxW, long long total,
                                                           unsigned* __restrict__ mm) {
    pn2_eval_img r;
    if (!batch_row(tab, maxH, maxW, total, r)) return;
    const long long n = (long long)r.H * r.W;
    if ((long long)blockIdx.x * 256 >= n) return;
    const size_t base = (size_t)blockIdx.y * h * w;
    float mn = INFINITY, mx = -INFINITY;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        int ox; const int oy = (int)divmod_idx((size_t)i, r.W, ox);
        const float s = tail_sample<NM>(M, base, h, w, oy, ox, r.rh, r.rw);
        mn = fminf(mn, s); mx = fmaxf(mx, s);
    }
    for (int o = 32; o > 0; o >>= 1) { mn = fminf(mn, __shfl_xor(mn, o)); mx = fmaxf(mx, __shfl_xor(mx, o)); }
    if ((threadIdx.x & 63) == 0) { atomicMax(mm + 2 * blockIdx.y, ~f2ord(mn)); atomicMax(mm + 2 * blockIdx.y + 1, f2ord(mx)); }
}
// pass 2: every value again, normalised and truncated to the byte at the image's offset of the packed buffer
template <int NM>
__global__ __launch_bounds__(256) void tail_bytes_batch_k(EvalMaps M, int h, int w, const pn2_eval_img* __restrict__ tab, int maxH, int maxW, long long total,
                                                          const unsigned* __restrict__ mm, unsigned char* __restrict__ out) {
    pn2_eval_img r;
    if (!batch_row(tab, maxH, maxW, total, r)) return;
    const long long n = (long long)r.H * r.W;
    const size_t base = (size_t)blockIdx.y * h * w;
    const float mn = ord2f(~mm[2 * blockIdx.y]), den = ord2f(mm[2 * blockIdx.y + 1]) - mn + 1e-8f;
    unsigned char* o = out + r.off;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        int ox; const int oy = (int)divmod_idx((size_t)i, r.W, ox);
        o[i] = eval_byte(tail_sample<NM>(M, base, h, w, oy, ox, r.rh, r.rw), mn, den);
    }
}

// the 512 histogram counts and (region != 0) the three centroid sums of every image; the blocks of an image are those of the per-image entries
__global__ __launch_bounds__(256) void counts_batch_k(const unsigned char* __restrict__ pred, const float* __restrict__ gt, const pn2_eval_img* __restrict__ tab,
                                                      int maxH, int maxW, long long total, unsigned* __restrict__ hist, u64* __restrict__ out25) {
    __shared__ unsigned hl[512];
    pn2_eval_img r;
    if (!batch_row(tab, maxH, maxW, total, r)) return;
    const long long n = (long long)r.H * r.W;
    const int blk = blockIdx.x, nh = hist_blocks(n), nr = region_blocks(n);
    if (blk < nh) {
        hl[threadIdx.x] = 0; hl[threadIdx.x + 256] = 0;
        __syncthreads();
        eval_hist_accum(pred + r.off, gt + r.off, n, (long long)blk * 256 + threadIdx.x, (long long)nh * 256, hl);
        __syncthreads();
        eval_hist_flush(hl, hist + (size_t)blockIdx.y * 512);
    }
    if (out25 && blk < nr) centroid_body(gt + r.off, r.H, r.W, blk, nr, out25 + (size_t)blockIdx.y * 25);
}
__global__ __launch_bounds__(256) void quadrants_batch_k(const unsigned char* __restrict__ pred, const float* __restrict__ gt, const pn2_eval_img* __restrict__ tab,
                                                         int maxH, int maxW, long long total, u64* __restrict__ out25) {
    pn2_eval_img r;
    if (!batch_row(tab, maxH, maxW, total, r)) return;
    const int nr = region_blocks((long long)r.H * r.W);
    if ((int)blockIdx.x < nr) quadrants_body(pred + r.off, gt + r.off, r.H, r.W, blockIdx.x, nr, out25 + (size_t)blockIdx.y * 25);
}

// the three wFm passes of every image: 64 columns per block (a batch has few columns per image and many images), one block per row, the per-image blocks of
// the sums.  Work buffers at the image's pixel offset: rcol[total], et[total], dst[total].
__global__ __launch_bounds__(64) void edt_cols_batch_k(const float* __restrict__ gt, const pn2_eval_img* __restrict__ tab, int maxH, int maxW, long long total,
                                                       int* __restrict__ rcol) {
    pn2_eval_img r;
    if (!batch_row(tab, maxH, maxW, total, r)) return;
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j < r.W) edt_col_body(gt + r.off, r.H, r.W, j, rcol + r.off);
}
__global__ __launch_bounds__(256) void edt_rows_batch_k(const unsigned char* __restrict__ pred, const float* __restrict__ gt, const pn2_eval_img* __restrict__ tab,
                                                        int maxH, int maxW, long long total, const int* __restrict__ rcol, double* __restrict__ work_d) {
    extern __shared__ int cand[];
    pn2_eval_img r;
    if (!batch_row(tab, maxH, maxW, total, r)) return;
    if ((int)blockIdx.x < r.H) edt_row_body(pred + r.off, gt + r.off, r.H, r.W, blockIdx.x, rcol + r.off, work_d + r.off, work_d + total + r.off, cand);
}
__global__ __launch_bounds__(256) void wfm_sums_batch_k(const unsigned char* __restrict__ pred, const float* __restrict__ gt, const pn2_eval_img* __restrict__ tab,
                                                        int maxH, int maxW, long long total, const double* __restrict__ work_d, const double* __restrict__ K, double c5,
                                                        double* __restrict__ part) {
    pn2_eval_img r;
    if (!batch_row(tab, maxH, maxW, total, r)) return;
    const int nb = wfm_blocks((long long)r.H * r.W);
    if ((int)blockIdx.x < nb)
        wfm_sums_body(pred + r.off, gt + r.off, r.H, r.W, work_d + r.off, work_d + total + r.off, K, c5, blockIdx.x, nb, part + (size_t)blockIdx.y * PN2_EVAL_WFM_MAX_BLOCKS * 2);
}

constexpr size_t EDT_LDS_CAP = 60 * 1024;          // a row of W ints in the LDS of the edt_rows kernels
// -1: null pointer / empty size, -2: outside the built range (blockIdx.y carries the image; edt_rows keeps a row of W ints in LDS)
int batch_check(const void* a, const void* b, const void* tab, int B, int maxH, int maxW, long long total) {
    if (!a || !b || !tab || B < 1 || maxH < 1 || maxW < 1 || total < 1) return -1;
    if (B > 65535 || (size_t)maxW * sizeof(int) > EDT_LDS_CAP) return -2;
    return 0;
}

}  // namespace

extern "C" {

int pn2_eval_region_sums(const unsigned char* pred_u8, const float* gt, int H, int W, unsigned long long* out25, void* stream) {
    if (!pred_u8 || !gt || !out25 || H < 1 || W < 1) return -1;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(out25, 0, 25 * sizeof(unsigned long long), st) != hipSuccess) return -4;
    const int g = region_blocks((long long)H * W);
    if (int rc = pn2_launch<eval_centroid_k>(dim3(g), dim3(256), 0, 0, st, gt, H, W, out25)) return rc;
    return pn2_launch<eval_quadrants_k>(dim3(g), dim3(256), 0, 0, st, pred_u8, gt, H, W, out25);
}

int pn2_eval_wfm_blocks(int H, int W) { return wfm_blocks((long long)H * W); }

int pn2_eval_wfm(const unsigned char* pred_u8, const float* gt, int H, int W, const double* K49, double c5, int* work_i, double* work_d, double* part, void* stream) {
    if (!pred_u8 || !gt || !K49 || !work_i || !work_d || !part || H < 1 || W < 1) return -1;
    if ((size_t)W * sizeof(int) > EDT_LDS_CAP) return -2;
    hipStream_t st = (hipStream_t)stream;
    double* et = work_d; double* dst = work_d + (size_t)H * W;
    if (int rc = pn2_launch<edt_cols_k>(dim3((W + 255) / 256), dim3(256), 0, 0, st, gt, H, W, work_i)) return rc;
    if (int rc = pn2_launch<edt_rows_k>(dim3(H), dim3(256), (size_t)W * sizeof(int), (int)EDT_LDS_CAP, st, pred_u8, gt, H, W, (const int*)work_i, et, dst)) return rc;
    return pn2_launch<wfm_sums_k>(dim3(pn2_eval_wfm_blocks(H, W)), dim3(256), 0, 0, st, pred_u8, gt, H, W, (const double*)et, (const double*)dst, K49, c5, part);
}

int pn2_eval_tail_batch(const float* const* maps, int nmaps, int B, int h, int w, const pn2_eval_img* table_dev, int maxH, int maxW, long long total,
                        unsigned char* out, unsigned* minmax, void* stream) {
    if (!maps || h < 1 || w < 1) return -1;
    if (int rc = batch_check(out, minmax, table_dev, B, maxH, maxW, total)) return rc;
    if (nmaps != 1 && nmaps != 4) return -2;
    if ((long long)h * w > 0x3fffffffLL) return -2;
    EvalMaps M;
    for (int j = 0; j < 4; ++j) { M.p[j] = maps[j < nmaps ? j : 0]; if (!M.p[j]) return -1; }
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(minmax, 0, (size_t)B * 2 * sizeof(unsigned), st) != hipSuccess) return -4;
    const long long n = (long long)maxH * maxW;
    const dim3 grid((unsigned)std::min<long long>((n + 1023) / 1024, 512), B);
    return with_int<4, 1>(nmaps, [&](auto nm) {
        constexpr int NM = decltype(nm)::value;
        if (int rc = pn2_launch<tail_minmax_batch_k<NM>>(grid, dim3(256), 0, 0, st, M, h, w, table_dev, maxH, maxW, total, minmax)) return rc;
        return pn2_launch<tail_bytes_batch_k<NM>>(grid, dim3(256), 0, 0, st, M, h, w, table_dev, maxH, maxW, total, (const unsigned*)minmax, out);
    });
}

int pn2_eval_counts_batch(const unsigned char* pred_u8, const float* gt, const pn2_eval_img* table_dev, int B, int maxH, int maxW, long long total,
                          unsigned* hist, unsigned long long* out25, void* stream) {
    if (!hist) return -1;
    if (int rc = batch_check(pred_u8, gt, table_dev, B, maxH, maxW, total)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(hist, 0, (size_t)B * 512 * sizeof(unsigned), st) != hipSuccess) return -4;
    if (out25 && hipMemsetAsync(out25, 0, (size_t)B * 25 * sizeof(unsigned long long), st) != hipSuccess) return -4;
    const long long n = (long long)maxH * maxW;
    const int nr = region_blocks(n);
    const int rc = pn2_launch<counts_batch_k>(dim3(std::max(hist_blocks(n), out25 ? nr : 1), B), dim3(256), 0, 0, st, pred_u8, gt, table_dev, maxH, maxW, total, hist, out25);
    if (rc || !out25) return rc;
    return pn2_launch<quadrants_batch_k>(dim3(nr, B), dim3(256), 0, 0, st, pred_u8, gt, table_dev, maxH, maxW, total, out25);
}

int pn2_eval_wfm_batch(const unsigned char* pred_u8, const float* gt, const pn2_eval_img* table_dev, int B, int maxH, int maxW, long long total,
                       const double* K49, double c5, int* work_i, double* work_d, double* part, void* stream) {
    if (!K49 || !work_i || !work_d || !part) return -1;
    if (int rc = batch_check(pred_u8, gt, table_dev, B, maxH, maxW, total)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = pn2_launch<edt_cols_batch_k>(dim3((maxW + 63) / 64, B), dim3(64), 0, 0, st, gt, table_dev, maxH, maxW, total, work_i)) return rc;
    if (int rc = pn2_launch<edt_rows_batch_k>(dim3(maxH, B), dim3(256), (size_t)maxW * sizeof(int), (int)EDT_LDS_CAP, st, pred_u8, gt, table_dev, maxH, maxW, total, (const int*)work_i, work_d))
        return rc;
    return pn2_launch<wfm_sums_batch_k>(dim3(wfm_blocks((long long)maxH * maxW), B), dim3(256), 0, 0, st, pred_u8, gt, table_dev, maxH, maxW, total, (const double*)work_d, K49, c5, part);
}

}  // extern "C"
