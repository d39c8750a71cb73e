// Boundary-quality primitives on int8 class maps for gfx950: the squared Euclidean distance of every pixel to the nearest
// pixel of ANOTHER class, and the integer count tables behind Boundary IoU and trimap accuracy.  Not in the reference.  Everything is
// integer arithmetic; every result is unique (independent of scheduling).
//   boundary_dist2_kernel   one workgroup per BT_W x BT_H tile of one image: the tile and a halo of rmax pixels are staged as int8 in LDS
//                           (out-of-image positions as fill, so the image border is no boundary and needs no test in the search), then a
//                           thread searches the window of each of its pixels outward: rows y -+ ady in the order ady = 0, 1, ... while
//                           ady^2 < best, and inside a row pair columns x -+ adx for adx = 0, 1, ... while ady^2 + adx^2 < best.  The first
//                           hit of a row pair is its minimum, so the scan of the pair ends there; best starts at rmax^2 + 1, which keeps
//                           ady, adx <= rmax: every LDS index stays inside the staged halo.  A staged tile that holds at most one class has
//                           no source at all: its pixels are FAR without a search.
//   boundary_count_kernel   per valid pixel the first threshold index k0 with d2 <= t_k0 (thresholds ascend: the pixel counts for every
//                           k >= k0); LDS histograms over k0 (u32 adds), folded to running sums over k when the workgroup flushes: one
//                           64-bit global add per non-empty (k, cell) and workgroup
//   boundary_count_direct_kernel   the same counts as 64-bit global adds per pixel and k, for tables beyond the LDS budget
// LDS: dist2 (BT_H + 64) x LDS_W = 80 x 128 B = 10 KiB static (a wave reads 64 consecutive bytes of a row: 16 banks, four lanes per
// word, no conflict); counts K * ncls * (ncls + 3) u32 cells, at most MAX_CELLS = 8192 (32 KiB).
#include "common.h"

namespace {

constexpr int BT_W = 64, BT_H = 16, BTPB = 256, MAX_R = 32;
constexpr int LDS_W = BT_W + 2 * MAX_R, LDS_H = BT_H + 2 * MAX_R;  // 128 x 80
constexpr int FAR = 0x7fffffff;
constexpr int MAX_IMAGES = 65535;  // grid.y
constexpr int MAX_K = 8, MAX_T = 1024, MAX_NCLS = 127, MAX_CELLS = 8192, MAX_WG = 1024, CTPB = 256;

// grid.x = tiles of one image (row-major), grid.y = image
__global__ __launch_bounds__(BTPB) void boundary_dist2_kernel(const signed char* __restrict__ cls, int* __restrict__ dist2, int H, int W,
                                                              int tiles_x, int rmax, int fill) {
    __shared__ signed char tile[LDS_H * LDS_W];
    __shared__ int cmin, cmax;
    const long base = (long)blockIdx.y * H * W;
    const int ty0 = ((int)blockIdx.x / tiles_x) * BT_H, tx0 = ((int)blockIdx.x % tiles_x) * BT_W;
    const int sh = BT_H + 2 * rmax, sw = BT_W + 2 * rmax;  // staged rows and columns: <= LDS_H, LDS_W
    if (threadIdx.x == 0) cmin = 128, cmax = -129;
    __syncthreads();
    {
        const int sc = threadIdx.x % LDS_W, gx = tx0 - rmax + sc;
        int lo = 128, hi = -129;
        if (sc < sw) {
            for (int sr = threadIdx.x / LDS_W; sr < sh; sr += BTPB / LDS_W) {
                const int gy = ty0 - rmax + sr;
                int v = fill;
                if (gx >= 0 && gx < W && gy >= 0 && gy < H) v = cls[base + (long)gy * W + gx];
                tile[sr * LDS_W + sc] = (signed char)v;
                if (v != fill) lo = v < lo ? v : lo, hi = v > hi ? v : hi;
            }
        }
        if (lo <= hi) atomicMin(&cmin, lo), atomicMax(&cmax, hi);
    }
    __syncthreads();
    const bool one_class = cmin >= cmax;  // no class or a single one among the staged pixels: nothing can be a source
    const int lx = threadIdx.x % BT_W, ly0 = threadIdx.x / BT_W, gx = tx0 + lx;
    constexpr int PER = BT_W * BT_H / BTPB, STEP = BTPB / BT_W;
    const int lim = rmax * rmax + 1;
#pragma unroll 1
    for (int k = 0; k < PER; ++k) {
        const int ly = ly0 + k * STEP, gy = ty0 + ly;
        if (gx >= W || gy >= H) continue;
        const signed char* ctr = tile + (ly + rmax) * LDS_W + lx + rmax;
        const int c = *ctr;
        int out = -1;
        if (c != fill) {
            int best = lim;
            if (!one_class) {
                for (int ady = 0; ady * ady < best; ++ady) {  // ady <= rmax since best <= rmax^2 + 1
                    const signed char* up = ctr - ady * LDS_W;
                    const signed char* dn = ctr + ady * LDS_W;
                    const int d0 = ady * ady;
                    for (int adx = 0; d0 + adx * adx < best; ++adx) {  // adx <= rmax likewise
                        const int a = up[-adx], b = up[adx], e = dn[-adx], f = dn[adx];
                        if ((a != fill && a != c) || (b != fill && b != c) || (e != fill && e != c) || (f != fill && f != c)) {
                            best = d0 + adx * adx;
                            break;
                        }
                    }
                }
            }
            out = best < lim ? best : FAR;
        }
        dist2[base + (long)gy * W + gx] = out;
    }
}

struct Thresholds {
    int t[MAX_K];  // entries K.. repeat the last one
};

// first k with d2 <= t[k], K when there is none
__device__ __forceinline__ int first_k(const Thresholds& th, int K, int d2) {
    int k0 = 0;
#pragma unroll
    for (int k = 0; k < MAX_K; ++k) k0 += (k < K && d2 > th.t[k]) ? 1 : 0;
    return k0;
}

__device__ __forceinline__ bool count_pixel(const signed char* gt, const signed char* pred, long m, int ncls, int fill, int& g, int& p) {
    g = gt[m], p = pred[m];
    return g != fill && p != fill && g >= 0 && g < ncls && p >= 0 && p < ncls;
}

// LDS: [K][cols] u32, cols = 3 * ncls (band, [c][3]) + ncls * ncls (trimap, [gt][pred]), a pixel is entered at its first k only.
// A workgroup sees at most 2^40 / MAX_WG = 2^30 pixels (checked by the entry point): the u32 cells cannot wrap.
__global__ __launch_bounds__(CTPB) void boundary_count_kernel(const signed char* __restrict__ gt, const signed char* __restrict__ pred,
                                                              const int* __restrict__ gt_d2, const int* __restrict__ pred_d2, Thresholds th,
                                                              int K, unsigned long long* __restrict__ band,
                                                              unsigned long long* __restrict__ trimap, long M, int ncls, int fill) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned* s = reinterpret_cast<unsigned*>(smem);
    const int nb = 3 * ncls, cols = nb + ncls * ncls;
    for (int i = threadIdx.x; i < K * cols; i += CTPB) s[i] = 0u;
    __syncthreads();
    for (long m = blockIdx.x * (long)CTPB + threadIdx.x; m < M; m += (long)gridDim.x * CTPB) {
        int g, p;
        if (!count_pixel(gt, pred, m, ncls, fill, g, p)) continue;
        const int kg = first_k(th, K, gt_d2[m]), kp = first_k(th, K, pred_d2[m]);
        if (kg < K) {
            atomicAdd(s + kg * cols + g * 3, 1u);
            atomicAdd(s + kg * cols + nb + g * ncls + p, 1u);
        }
        if (kp < K) atomicAdd(s + kp * cols + p * 3 + 1, 1u);
        const int kb = kg > kp ? kg : kp;
        if (g == p && kb < K) atomicAdd(s + kb * cols + g * 3 + 2, 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < cols; i += CTPB) {
        unsigned long long* dst = i < nb ? band + i : trimap + (i - nb);
        const long pitch = i < nb ? nb : (long)ncls * ncls;
        unsigned long long run = 0;
        for (int k = 0; k < K; ++k) {
            run += s[k * cols + i];
            if (run) atomicAdd(dst + k * pitch, run);
        }
    }
}

__global__ __launch_bounds__(CTPB) void boundary_count_direct_kernel(const signed char* __restrict__ gt, const signed char* __restrict__ pred,
                                                                     const int* __restrict__ gt_d2, const int* __restrict__ pred_d2,
                                                                     Thresholds th, int K, unsigned long long* __restrict__ band,
                                                                     unsigned long long* __restrict__ trimap, long M, int ncls, int fill) {
    const long nb = 3 * ncls, nt = (long)ncls * ncls;
    for (long m = blockIdx.x * (long)CTPB + threadIdx.x; m < M; m += (long)gridDim.x * CTPB) {
        int g, p;
        if (!count_pixel(gt, pred, m, ncls, fill, g, p)) continue;
        const int kg = first_k(th, K, gt_d2[m]), kp = first_k(th, K, pred_d2[m]);
        const int kb = kg > kp ? kg : kp;
        for (int k = kg; k < K; ++k) {
            atomicAdd(band + k * nb + g * 3, 1ull);
            atomicAdd(trimap + k * nt + g * ncls + p, 1ull);
        }
        for (int k = kp; k < K; ++k) atomicAdd(band + k * nb + p * 3 + 1, 1ull);
        if (g == p)
            for (int k = kb; k < K; ++k) atomicAdd(band + k * nb + g * 3 + 2, 1ull);
    }
}

}  // namespace

#define ST(s) ((hipStream_t)(s))

extern "C" {

int ig_boundary_dist2(const signed char* cls, int* dist2, int n, int H, int W, int rmax, int fill, void* stream) {
    IG_REQUIRE(rmax >= 1 && rmax <= MAX_R, "ig_boundary_dist2: 1 <= rmax <= %d (got %d)", MAX_R, rmax);
    IG_REQUIRE(fill >= -128 && fill <= 127, "ig_boundary_dist2: fill must fit int8 (got %d)", fill);
    IG_REQUIRE(n >= 0 && H >= 1 && W >= 1, "ig_boundary_dist2: need n >= 0, H >= 1, W >= 1 (n %d, H %d, W %d)", n, H, W);
    IG_REQUIRE((long)H * W <= 0x7fffffffL, "ig_boundary_dist2: H * W = %ld exceeds 2^31 - 1", (long)H * W);
    if (n == 0) return IG_OK;
    IG_REQUIRE(cls && dist2, "ig_boundary_dist2: null pointer");
    const long HW = (long)H * W;
    const int tiles_x = ig_cdiv(W, BT_W), tiles_y = ig_cdiv(H, BT_H);
    for (int i0 = 0; i0 < n; i0 += MAX_IMAGES) {
        const unsigned ni = (unsigned)(n - i0 < MAX_IMAGES ? n - i0 : MAX_IMAGES);
        const int rc = ig_launch<boundary_dist2_kernel>("ig_boundary_dist2", dim3((unsigned)tiles_x * (unsigned)tiles_y, ni), dim3(BTPB), 0,
                                                        ST(stream), cls + (long)i0 * HW, dist2 + (long)i0 * HW, H, W, tiles_x, rmax, fill);
        if (rc != IG_OK) return rc;
    }
    return IG_OK;
}

int ig_boundary_update(const signed char* gt, const signed char* pred, const int* gt_d2, const int* pred_d2, const int* thresholds, int K,
                       unsigned long long* band, unsigned long long* trimap, int n, long HW, int ncls, int fill, void* stream) {
    IG_REQUIRE(K >= 1 && K <= MAX_K, "ig_boundary_update: 1 <= K <= %d (got %d)", MAX_K, K);
    IG_REQUIRE(thresholds, "ig_boundary_update: null pointer (thresholds)");
    for (int k = 0; k < K; ++k) {
        IG_REQUIRE(thresholds[k] >= 1 && thresholds[k] <= MAX_T, "ig_boundary_update: thresholds[%d] = %d is not in [1, %d]", k, thresholds[k],
                   MAX_T);
        IG_REQUIRE(k == 0 || thresholds[k] > thresholds[k - 1], "ig_boundary_update: thresholds must ascend strictly (thresholds[%d] = %d after %d)",
                   k, thresholds[k], k ? thresholds[k - 1] : 0);
    }
    IG_REQUIRE(ncls >= 2 && ncls <= MAX_NCLS, "ig_boundary_update: 2 <= ncls <= %d (got %d)", MAX_NCLS, ncls);
    IG_REQUIRE(fill >= -128 && fill <= 127, "ig_boundary_update: fill must fit int8 (got %d)", fill);
    IG_REQUIRE(n >= 0 && HW >= 1 && HW <= 0x7fffffffL, "ig_boundary_update: need n >= 0 and 1 <= HW <= 2^31 - 1 (n %d, HW %ld)", n, HW);
    if (n == 0) return IG_OK;
    const long M = (long)n * HW;
    IG_REQUIRE(M <= (1L << 40), "ig_boundary_update: n * HW = %ld exceeds 2^40 pixels per call (32-bit LDS counts)", M);
    IG_REQUIRE(gt && pred && gt_d2 && pred_d2 && band && trimap, "ig_boundary_update: null pointer");
    Thresholds th;
    for (int k = 0; k < MAX_K; ++k) th.t[k] = thresholds[k < K ? k : K - 1];
    const long nblk = (M + CTPB - 1) / CTPB;
    const dim3 grid((unsigned)(nblk < MAX_WG ? nblk : MAX_WG));
    const int cells = K * ncls * (ncls + 3);
    if (cells <= MAX_CELLS)
        return ig_launch<boundary_count_kernel>("ig_boundary_update", grid, dim3(CTPB), cells * 4, ST(stream), gt, pred, gt_d2, pred_d2, th, K,
                                                band, trimap, M, ncls, fill);
    return ig_launch<boundary_count_direct_kernel>("ig_boundary_update", grid, dim3(CTPB), 0, ST(stream), gt, pred, gt_d2, pred_d2, th, K, band,
                                                   trimap, M, ncls, fill);
}

}  // extern "C"
