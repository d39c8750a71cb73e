// Probability-blended tile inference for gfx950: overlapping sliding windows are averaged on a tile canvas with a separable
// window weight instead of the nearest-centre hand-off of infer_utils.stitch_windows.
//   accumulate  acc[c] += w * softmax(logits)[c], wsum += w  over the windows of one batch   segmentation.py:202-213
//   finalize    p_c = acc_c / wsum, argmax -> int8 class map, NaN / fill where uncovered or NODATA
// Window grid: the row-major product of sorted tops x lefts (process_test's rule, dataloader.py:655-664, optionally with a last
// origin at size - crop on each axis).
//
// Gather form, no atomics: one thread owns one canvas pixel and visits the windows that cover it in row-major window order,
// skipping those outside the batch.  A batch is a contiguous range of that order, so every pixel receives the same sequence of
// fp32 additions whatever the batch size: the canvas is bit-identical for any batching ("Blended tile inference").
// HBM-bound: per covered pixel and batch (ncls + 1) x 8 bytes of canvas traffic plus ncls x 4 bytes of logits per window.
//
// Test-time augmentation over the dihedral group D4 (the eight transforms G_k are defined once, in include/instageo_hip.h):
//   d4_apply         windows -> their K transforms before the forward pass, logits -> back to the canvas frame after it (bit copies)
//   accumulate_tta   the same gather with K logit sets per window: a window's K terms are summed in order j = 0..K-1 in an fp64 register
//                    and reach the fp32 canvas as one addition, acc[c] += w * sum_j softmax(logits[j])[c], wsum += K * w (one rounding
//                    each), so a pixel's canvas values round once per window as in the one-set kernel, not K times
//   uncertainty      normalised entropy and top-two margin of the finished canvas, finalize's validity rule
#include "common.h"

namespace {

constexpr int BTPB = 256;
constexpr int BCHUNK = 8;  // classes held in registers per pass (ncls > 8 takes ceil(ncls / 8) passes; each acc[c] is read and written once)

// first index i in [0, n) with a[i] > v (a ascending); n when there is none
__device__ __forceinline__ int upper_bound(const int* __restrict__ a, int n, int v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] > v) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// Windows [w0, w0 + n) of the n_rows x n_cols grid; logits (n, K, ncls, crop, crop); acc (ncls, Hb, W) and wsum (Hb, W) hold canvas rows
// [y0, y0 + Hb); the grid walks canvas rows [ya, yb) (inside the band).  blockIdx.y -> row (wave-uniform row search), x -> lane.
// TTA = false is the one-logit-set kernel (K == 1, the loop over j folds away); TTA = true sums a window's K sets in order j = 0..K-1
// in fp64 and adds the sum to the canvas once.
template <bool TTA>
__global__ __launch_bounds__(BTPB) void window_blend_accumulate_kernel(const float* __restrict__ logits, const int* __restrict__ tops,
                                                                       const int* __restrict__ lefts, int n_rows, int n_cols, long w0,
                                                                       int n, int K_, const float* __restrict__ wvec,
                                                                       float* __restrict__ acc, float* __restrict__ wsum, int ncls, int crop,
                                                                       int W, int y0, int Hb, int ya, int yb) {
    const int K = TTA ? K_ : 1;
    const int x = blockIdx.x * BTPB + threadIdx.x;
    if (x >= W) return;
    const long wend = w0 + n;
    const int r_first = (int)(w0 / n_cols), r_last = (int)((wend - 1) / n_cols);
    const long cc = (long)crop * crop, plane = (long)Hb * W;
    // covering columns: lefts[c] in (x - crop, x]
    const int chi = upper_bound(lefts, n_cols, x) - 1;
    const int clo = upper_bound(lefts, n_cols, x - crop);
    if (clo > chi) return;
    for (int y = ya + (int)blockIdx.y; y < yb; y += (int)gridDim.y) {
        const int rlo = max(upper_bound(tops, n_rows, y - crop), r_first);
        const int rhi = min(upper_bound(tops, n_rows, y) - 1, r_last);
        if (rlo > rhi) continue;
        // does any covering window lie in the batch?  (only the first and last grid row of a batch are partial)
        const long wa = (long)rlo * n_cols + clo, wb = (long)rhi * n_cols + chi;
        if (wb < w0 || wa >= wend) continue;
        const long pix = (long)(y - y0) * W + x;
        for (int c0 = 0; c0 < ncls; c0 += BCHUNK) {
            float a[BCHUNK];
#pragma unroll
            for (int j = 0; j < BCHUNK; ++j) a[j] = (c0 + j < ncls) ? acc[(long)(c0 + j) * plane + pix] : 0.f;
            float ws = c0 == 0 ? wsum[pix] : 0.f;
            bool any = false;
            for (int r = rlo; r <= rhi; ++r) {
                const int dy = y - tops[r];
                if ((unsigned)dy >= (unsigned)crop) continue;  // only if tops is not ascending (a caller's error): never read outside a window
                const float wy = wvec[dy];
                for (int c = clo; c <= chi; ++c) {
                    const long w = (long)r * n_cols + c;
                    if (w < w0 || w >= wend) continue;
                    const int dx = x - lefts[c];
                    if ((unsigned)dx >= (unsigned)crop) continue;
                    const float wt = wy * wvec[dx];
                    double sp[BCHUNK];  // TTA: the sum over a window's K sets of the fp32 terms, in order j = 0..K-1, held in fp64
#pragma unroll
                    for (int j = 0; j < BCHUNK; ++j) sp[j] = 0.0;
                    for (int t = 0; t < K; ++t) {
                        const float* lp = logits + ((w - w0) * K + t) * ncls * cc + (long)dy * crop + dx;
                        if (ncls == 1) {  // regression head: the raw value
                            if (TTA) sp[0] += (double)lp[0];
                            else a[0] = fmaf(wt, lp[0], a[0]);
                        } else {  // max-subtracted softmax (ig_softmax_prob)
                            float mx = -INFINITY;
                            for (int k = 0; k < ncls; ++k) mx = fmaxf(mx, lp[k * cc]);
                            float se = 0.f;
                            for (int k = 0; k < ncls; ++k) se += expf(lp[k * cc] - mx);
#pragma unroll
                            for (int j = 0; j < BCHUNK; ++j)
                                if (c0 + j < ncls) {
                                    const float p = expf(lp[(c0 + j) * cc] - mx) / se;
                                    if (TTA) sp[j] += (double)p;
                                    else a[j] = fmaf(wt, p, a[j]);
                                }
                        }
                    }
                    if (TTA) {  // one rounding per window and canvas value: acc += wt * sum_j p_j, wsum += K * wt
#pragma unroll
                        for (int j = 0; j < BCHUNK; ++j)
                            if (c0 + j < ncls) a[j] = (float)fma((double)wt, sp[j], (double)a[j]);
                        if (c0 == 0) ws = fmaf((float)K, wt, ws);
                    } else if (c0 == 0) {
                        ws += wt;
                    }
                    any = true;
                }
            }
            if (!any) break;
#pragma unroll
            for (int j = 0; j < BCHUNK; ++j)
                if (c0 + j < ncls) acc[(long)(c0 + j) * plane + pix] = a[j];
            if (c0 == 0) wsum[pix] = ws;
        }
    }
}

// Per pixel of the (ncls, HW) canvas: fill / NaN where wsum == 0 or any band of the tile is NODATA, else p = acc / wsum and the
// first maximum (ig_argmax_i8's tie rule).
template <typename T>
__global__ __launch_bounds__(BTPB) void window_blend_finalize_kernel(const float* __restrict__ acc, const float* __restrict__ wsum,
                                                                     const T* __restrict__ tile, int TC, double nd,
                                                                     signed char* __restrict__ classmap, float* __restrict__ prob,
                                                                     int ncls, long HW, int fill) {
    const long m = blockIdx.x * (long)BTPB + threadIdx.x;
    if (m >= HW) return;
    const float ws = wsum[m];
    bool bad = !(ws > 0.f);
    if (tile)
        for (int b = 0; b < TC && !bad; ++b) bad = (double)tile[(long)b * HW + m] == nd;
    if (bad) {
        if (classmap) classmap[m] = (signed char)fill;
        if (prob)
            for (int c = 0; c < ncls; ++c) prob[(long)c * HW + m] = __builtin_nanf("");
        return;
    }
    float best = -INFINITY;
    int am = 0;
    for (int c = 0; c < ncls; ++c) {
        const float p = acc[(long)c * HW + m] / ws;
        if (prob) prob[(long)c * HW + m] = p;
        if (p > best) best = p, am = c;
    }
    if (classmap) classmap[m] = (signed char)am;
}

// Normalised entropy and top-two margin of p = acc / wsum per pixel of the (ncls, HW) canvas; NaN where finalize writes fill / NaN.
// p ln p is taken as 0 at p == 0, and ln 1 == 0 exactly, so a one-hot pixel has entropy 0 and margin 1.
template <typename T>
__global__ __launch_bounds__(BTPB) void window_blend_uncertainty_kernel(const float* __restrict__ acc, const float* __restrict__ wsum,
                                                                        const T* __restrict__ tile, int TC, double nd,
                                                                        float* __restrict__ entropy, float* __restrict__ margin, int ncls,
                                                                        long HW, float ln_ncls) {
    const long m = blockIdx.x * (long)BTPB + threadIdx.x;
    if (m >= HW) return;
    const float ws = wsum[m];
    bool bad = !(ws > 0.f);
    if (tile)
        for (int b = 0; b < TC && !bad; ++b) bad = (double)tile[(long)b * HW + m] == nd;
    if (bad) {
        if (entropy) entropy[m] = __builtin_nanf("");
        if (margin) margin[m] = __builtin_nanf("");
        return;
    }
    float p1 = -INFINITY, p2 = -INFINITY, e = 0.f;
    for (int c = 0; c < ncls; ++c) {
        const float p = acc[(long)c * HW + m] / ws;
        if (p > p1) p2 = p1, p1 = p;
        else if (p > p2) p2 = p;
        if (p > 0.f) e -= p * logf(p);
    }
    if (entropy) entropy[m] = e / ln_ncls;
    if (margin) margin[m] = p1 - p2;
}

// ---- D4 transforms of S x S f32 planes (bit copies) -------------------------------------------------------------------------------
// One block moves one DT x DT tile of one destination plane; block b -> plane b / tiles, tile b % tiles (no per-image launch).  The code
// of a plane is block-uniform.  t = 0 (flips): wave w copies destination rows w, w + 4, ... of the tile; a lane's source column is x or
// S-1-x, so a wave reads one reversed-or-not contiguous row and writes one contiguous row.  t = 1 (transposing codes) goes through LDS:
//   load   for j = w, w + 4, ...: lane l reads src[sy(X0 + j)][sx(Y0 + l)] (one contiguous source row per wave, ascending or descending
//          in l) and writes lds[j * 65 + l];
//   store  for r = w, w + 4, ...: lane l reads lds[l * 65 + r] and writes dst[Y0 + r][X0 + l] (one contiguous destination row).
// LDS layout: 64 rows x 65 dwords, row = destination column offset, column = destination row offset.  Banks are (a / 4) % 32 per 32-lane
// half for ds_write_b32 / ds_read_b32: the write's dword index j * 65 + l has bank (j + l) % 32, the read's l * 65 + r has (l + r) % 32;
// both run over 32 distinct banks across the 32 lanes of a half, so neither conflicts.
constexpr int DT = 64, DLD = DT + 1, DTPB = 256;
struct D4Codes {
    int k[8];
};

__global__ __launch_bounds__(DTPB) void d4_apply_kernel(const unsigned* __restrict__ src, unsigned* __restrict__ dst, D4Codes codes, int K,
                                                        int P, int S, int expand, int tiles_x, int tiles) {
    __shared__ unsigned lds[DT * DLD];
    const long q = blockIdx.x / (unsigned)tiles;  // destination plane: (image i * K + j, p)
    const int tile = (int)(blockIdx.x % (unsigned)tiles);
    const int Y0 = (tile / tiles_x) * DT, X0 = (tile % tiles_x) * DT;
    const long img = q / P;
    const int p = (int)(q % P), j = (int)(img % K);
    const int code = codes.k[j];
    const bool h = code & 1, v = code & 2, t = code & 4;
    const long plane = (long)S * S;
    const unsigned* sp = src + (expand ? (img / K) * P + p : q) * plane;
    unsigned* dp = dst + q * plane;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (!t) {
        const int x = X0 + lane;
        if (x >= S) return;
        const int sx = h ? S - 1 - x : x;
        for (int r = w; r < DT; r += DTPB / 64) {
            const int y = Y0 + r;
            if (y >= S) break;
            dp[(long)y * S + x] = sp[(long)(v ? S - 1 - y : y) * S + sx];
        }
        return;
    }
    // transposing codes: source row from the destination column, source column from the destination row
    const int yl = Y0 + lane;  // this lane's destination row in the load phase
    if (yl < S) {
        const int sx = h ? S - 1 - yl : yl;
        for (int c = w; c < DT; c += DTPB / 64) {
            const int x = X0 + c;
            if (x >= S) break;
            lds[c * DLD + lane] = sp[(long)(v ? S - 1 - x : x) * S + sx];
        }
    }
    __syncthreads();
    const int x = X0 + lane;
    if (x >= S) return;
    for (int r = w; r < DT; r += DTPB / 64) {
        const int y = Y0 + r;
        if (y >= S) break;
        dp[(long)y * S + x] = lds[lane * DLD + r];
    }
}

}  // namespace

#define ST(s) ((hipStream_t)(s))

extern "C" {

int ig_window_blend_accumulate(const float* logits, const int* tops, const int* lefts, int n_rows, int n_cols, long w0, int n,
                               const float* wvec, float* acc, float* wsum, int ncls, int crop, int H, int W, int y0, int Hb, int ylo,
                               int yhi, void* stream) {
    IG_REQUIRE(logits && tops && lefts && wvec && acc && wsum, "ig_window_blend_accumulate: null pointer");
    IG_REQUIRE(ncls >= 1 && ncls <= 127, "ig_window_blend_accumulate: 1 <= ncls <= 127 (got %d)", ncls);
    IG_REQUIRE(crop >= 1 && crop <= H && crop <= W, "ig_window_blend_accumulate: need 1 <= crop <= H, W (crop %d, H %d, W %d)", crop, H, W);
    IG_REQUIRE(n_rows >= 1 && n_cols >= 1 && w0 >= 0 && n >= 0 && w0 + n <= (long)n_rows * n_cols,
               "ig_window_blend_accumulate: need 0 <= w0 and w0 + n <= n_rows * n_cols (w0 %ld, n %d, grid %d x %d)", w0, n, n_rows, n_cols);
    IG_REQUIRE(y0 >= 0 && Hb >= 0 && y0 + Hb <= H, "ig_window_blend_accumulate: band rows [y0, y0 + Hb) must lie in [0, H)");
    IG_REQUIRE(ylo >= 0 && ylo <= yhi && yhi <= H, "ig_window_blend_accumulate: need 0 <= ylo <= yhi <= H");
    const int ya = ylo > y0 ? ylo : y0, yb = yhi < y0 + Hb ? yhi : y0 + Hb;
    if (n == 0 || ya >= yb) return IG_OK;
    const int rows = yb - ya;
    hipLaunchKernelGGL(window_blend_accumulate_kernel<false>, dim3((unsigned)ig_cdiv(W, BTPB), (unsigned)(rows < 65535 ? rows : 65535)),
                       dim3(BTPB), 0, ST(stream), logits, tops, lefts, n_rows, n_cols, w0, n, 1, wvec, acc, wsum, ncls, crop, W, y0, Hb, ya, yb);
    return ig_check_launch("ig_window_blend_accumulate");
}

int ig_window_blend_accumulate_tta(const float* logits, const int* tops, const int* lefts, int n_rows, int n_cols, long w0, int n, int K,
                                   const float* wvec, float* acc, float* wsum, int ncls, int crop, int H, int W, int y0, int Hb, int ylo,
                                   int yhi, void* stream) {
    IG_REQUIRE(logits && tops && lefts && wvec && acc && wsum, "ig_window_blend_accumulate_tta: null pointer");
    IG_REQUIRE(K >= 1 && K <= 8, "ig_window_blend_accumulate_tta: 1 <= K <= 8 (got %d)", K);
    IG_REQUIRE(ncls >= 1 && ncls <= 127, "ig_window_blend_accumulate_tta: 1 <= ncls <= 127 (got %d)", ncls);
    IG_REQUIRE(crop >= 1 && crop <= H && crop <= W, "ig_window_blend_accumulate_tta: need 1 <= crop <= H, W (crop %d, H %d, W %d)", crop, H, W);
    IG_REQUIRE(n_rows >= 1 && n_cols >= 1 && w0 >= 0 && n >= 0 && w0 + n <= (long)n_rows * n_cols,
               "ig_window_blend_accumulate_tta: need 0 <= w0 and w0 + n <= n_rows * n_cols (w0 %ld, n %d, grid %d x %d)", w0, n, n_rows, n_cols);
    IG_REQUIRE(y0 >= 0 && Hb >= 0 && y0 + Hb <= H, "ig_window_blend_accumulate_tta: band rows [y0, y0 + Hb) must lie in [0, H)");
    IG_REQUIRE(ylo >= 0 && ylo <= yhi && yhi <= H, "ig_window_blend_accumulate_tta: need 0 <= ylo <= yhi <= H");
    const int ya = ylo > y0 ? ylo : y0, yb = yhi < y0 + Hb ? yhi : y0 + Hb;
    if (n == 0 || ya >= yb) return IG_OK;
    const int rows = yb - ya;
    const dim3 grid((unsigned)ig_cdiv(W, BTPB), (unsigned)(rows < 65535 ? rows : 65535));
    if (K == 1)  // the kernel of ig_window_blend_accumulate itself
        hipLaunchKernelGGL(window_blend_accumulate_kernel<false>, grid, dim3(BTPB), 0, ST(stream), logits, tops, lefts, n_rows, n_cols, w0, n, 1,
                           wvec, acc, wsum, ncls, crop, W, y0, Hb, ya, yb);
    else
        hipLaunchKernelGGL(window_blend_accumulate_kernel<true>, grid, dim3(BTPB), 0, ST(stream), logits, tops, lefts, n_rows, n_cols, w0, n, K,
                           wvec, acc, wsum, ncls, crop, W, y0, Hb, ya, yb);
    return ig_check_launch("ig_window_blend_accumulate_tta");
}

int ig_window_blend_finalize(const float* acc, const float* wsum, const void* tile, int tile_dtype, int TC, double no_data_value,
                             int nodata_enabled, signed char* classmap, float* prob, int ncls, long HW, int fill, void* stream) {
    IG_REQUIRE(acc && wsum, "ig_window_blend_finalize: null pointer");
    IG_REQUIRE(ncls >= 1 && ncls <= 127, "ig_window_blend_finalize: 1 <= ncls <= 127 (got %d)", ncls);
    IG_REQUIRE(ncls > 1 ? classmap != nullptr : (prob != nullptr && classmap == nullptr),
               "ig_window_blend_finalize: ncls > 1 needs a class map, ncls == 1 (regression) a value map and no class map");
    IG_REQUIRE(!nodata_enabled || (tile && TC >= 1), "ig_window_blend_finalize: NODATA test needs the tile (null pointer)");
    IG_REQUIRE(fill >= -128 && fill <= 127, "ig_window_blend_finalize: fill must fit int8 (got %d)", fill);
    IG_REQUIRE(HW >= 0, "ig_window_blend_finalize: HW < 0");
    if (HW == 0) return IG_OK;
    const dim3 grid((unsigned)((HW + BTPB - 1) / BTPB));
    if (!nodata_enabled)
        hipLaunchKernelGGL(window_blend_finalize_kernel<float>, grid, dim3(BTPB), 0, ST(stream), acc, wsum, (const float*)nullptr, 0,
                           no_data_value, classmap, prob, ncls, HW, fill);
    else if (tile_dtype == 0)
        hipLaunchKernelGGL(window_blend_finalize_kernel<int16_t>, grid, dim3(BTPB), 0, ST(stream), acc, wsum, (const int16_t*)tile, TC,
                           no_data_value, classmap, prob, ncls, HW, fill);
    else if (tile_dtype == 1)
        hipLaunchKernelGGL(window_blend_finalize_kernel<float>, grid, dim3(BTPB), 0, ST(stream), acc, wsum, (const float*)tile, TC,
                           no_data_value, classmap, prob, ncls, HW, fill);
    else {
        ig_set_error("ig_window_blend_finalize: unsupported tile_dtype %d", tile_dtype);
        return IG_ERR_UNSUPPORTED;
    }
    return ig_check_launch("ig_window_blend_finalize");
}

int ig_window_blend_uncertainty(const float* acc, const float* wsum, const void* tile, int tile_dtype, int TC, double no_data_value,
                                int nodata_enabled, float* entropy, float* margin, int ncls, long HW, void* stream) {
    IG_REQUIRE(acc && wsum, "ig_window_blend_uncertainty: null pointer (acc, wsum)");
    IG_REQUIRE(entropy || margin, "ig_window_blend_uncertainty: null pointer (entropy and margin: at least one output)");
    IG_REQUIRE(ncls >= 2 && ncls <= 127, "ig_window_blend_uncertainty: 2 <= ncls <= 127 (got %d)", ncls);
    IG_REQUIRE(!nodata_enabled || (tile && TC >= 1), "ig_window_blend_uncertainty: NODATA test needs the tile (null pointer)");
    IG_REQUIRE(HW >= 0, "ig_window_blend_uncertainty: HW < 0");
    if (HW == 0) return IG_OK;
    const dim3 grid((unsigned)((HW + BTPB - 1) / BTPB));
    const float ln_ncls = (float)log((double)ncls);
    if (!nodata_enabled)
        hipLaunchKernelGGL(window_blend_uncertainty_kernel<float>, grid, dim3(BTPB), 0, ST(stream), acc, wsum, (const float*)nullptr, 0,
                           no_data_value, entropy, margin, ncls, HW, ln_ncls);
    else if (tile_dtype == 0)
        hipLaunchKernelGGL(window_blend_uncertainty_kernel<int16_t>, grid, dim3(BTPB), 0, ST(stream), acc, wsum, (const int16_t*)tile, TC,
                           no_data_value, entropy, margin, ncls, HW, ln_ncls);
    else if (tile_dtype == 1)
        hipLaunchKernelGGL(window_blend_uncertainty_kernel<float>, grid, dim3(BTPB), 0, ST(stream), acc, wsum, (const float*)tile, TC,
                           no_data_value, entropy, margin, ncls, HW, ln_ncls);
    else {
        ig_set_error("ig_window_blend_uncertainty: unsupported tile_dtype %d", tile_dtype);
        return IG_ERR_UNSUPPORTED;
    }
    return ig_check_launch("ig_window_blend_uncertainty");
}

int ig_d4_apply(const float* src, float* dst, const int* codes, int K, int m, int P, int S, int expand, void* stream) {
    IG_REQUIRE(K >= 1 && K <= 8, "ig_d4_apply: 1 <= K <= 8 (got %d)", K);
    IG_REQUIRE(codes, "ig_d4_apply: null pointer (codes)");
    D4Codes ck{};
    for (int j = 0; j < K; ++j) {
        IG_REQUIRE(codes[j] >= 0 && codes[j] <= 7, "ig_d4_apply: codes[%d] = %d is not a D4 code (0..7)", j, codes[j]);
        ck.k[j] = codes[j];
    }
    IG_REQUIRE(m >= 0 && P >= 1 && S >= 1, "ig_d4_apply: need m >= 0, P >= 1, S >= 1 (m %d, P %d, S %d)", m, P, S);
    if (m == 0) return IG_OK;  // no images: src / dst are null
    IG_REQUIRE(src && dst, "ig_d4_apply: null pointer (src, dst)");
    IG_REQUIRE(src != dst, "ig_d4_apply: src == dst (the transforms are not done in place)");
    const int tiles_x = ig_cdiv(S, DT);
    const long tiles = (long)tiles_x * tiles_x, blocks = tiles * m * K * P;
    IG_REQUIRE(blocks <= 0x7fffffffL, "ig_d4_apply: m * K * P planes of S = %d need %ld blocks (> 2^31 - 1)", S, blocks);
    hipLaunchKernelGGL(d4_apply_kernel, dim3((unsigned)blocks), dim3(DTPB), 0, ST(stream), (const unsigned*)src, (unsigned*)dst, ck, K, P, S,
                       expand ? 1 : 0, tiles_x, (int)tiles);
    return ig_check_launch("ig_d4_apply");
}

}  // extern "C"
