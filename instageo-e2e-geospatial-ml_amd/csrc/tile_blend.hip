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

// Windows [w0, w0 + n) of the n_rows x n_cols grid; logits (n, ncls, crop, crop); acc (ncls, Hb, W) and wsum (Hb, W) hold canvas rows
// [y0, y0 + Hb); the grid walks canvas rows [ya, yb) (inside the band).  blockIdx.y -> row (wave-uniform row search), x -> lane.
__global__ __launch_bounds__(BTPB) void window_blend_accumulate_kernel(const float* __restrict__ logits, const int* __restrict__ tops,
                                                                       const int* __restrict__ lefts, int n_rows, int n_cols, long w0,
                                                                       int n, const float* __restrict__ wvec, float* __restrict__ acc,
                                                                       float* __restrict__ wsum, int ncls, int crop, int W, int y0,
                                                                       int Hb, int ya, int yb) {
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
                    const float* lp = logits + (w - w0) * ncls * cc + (long)dy * crop + dx;
                    if (ncls == 1) {  // regression head: the raw value
                        a[0] = fmaf(wt, lp[0], a[0]);
                    } else {  // max-subtracted softmax (ig_softmax_prob)
                        float mx = -INFINITY;
                        for (int k = 0; k < ncls; ++k) mx = fmaxf(mx, lp[k * cc]);
                        float se = 0.f;
                        for (int k = 0; k < ncls; ++k) se += expf(lp[k * cc] - mx);
#pragma unroll
                        for (int j = 0; j < BCHUNK; ++j)
                            if (c0 + j < ncls) a[j] = fmaf(wt, expf(lp[(c0 + j) * cc] - mx) / se, a[j]);
                    }
                    if (c0 == 0) ws += wt;
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
    hipLaunchKernelGGL(window_blend_accumulate_kernel, dim3((unsigned)ig_cdiv(W, BTPB), (unsigned)(rows < 65535 ? rows : 65535)), dim3(BTPB),
                       0, ST(stream), logits, tops, lefts, n_rows, n_cols, w0, n, wvec, acc, wsum, ncls, crop, W, y0, Hb, ya, yb);
    return ig_check_launch("ig_window_blend_accumulate");
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

}  // extern "C"
