// Overview pyramids and tile layout for Cloud Optimized GeoTIFF output on gfx950.  Not in the reference, which calls
// gdal_translate -of COG.  The two resampling rules (mode with a fill value for int8 class maps, NaN-aware mean for float32 rasters) are
// stated in include/instageo_hip.h.  Every result is unique (independent of scheduling): the class histogram is integer sums, everything
// else is written exactly once.
//
//   1  overview_mode_kernel   one workgroup per 64 x 64 block of the source (origin at multiples of 64, so every 2 x 2 group of every
//                             level nests in one block): the block goes to LDS once, levels 1..6 come out of LDS with a barrier between
//                             levels, so HBM is read once for up to six levels.  Optionally the class histogram of the source: runs of
//                             equal classes are merged per thread and per wave (segreduce.h), counted into an LDS table and flushed as one
//                             64-bit add per non-empty cell and workgroup.
//   2  overview_mean_kernel   the same plan on float32, one band per blockIdx.z
//   3  cog_tiles_kernel<T>    (bands, H, W) -> (bands, ny, nx, tile, tile) with padding and optional horizontal differencing; a gather:
//                             a thread builds 16 bytes of the output and stores them once
//
// More than six levels: the entry point launches again on level 6 (64 x 64 blocks of it).  No workgroup waits for another.  Out-of-range
// accesses are impossible: every load is guarded by row < H and column < W (the 16-byte path runs only where W is a multiple of the vector,
// so a vector that starts inside a row ends inside it), every store by the level's own size.
#include "segreduce.h"

namespace {

constexpr int CB = 64, CTPB = 256, CMAXL = 6;  // block side, threads, levels per launch
constexpr int CLDS = 4096 + 1024 + 256 + 64 + 16 + 4 + 1;  // the block's levels 0..6 back to back
constexpr int MAX_NCLS = 127;

__device__ __forceinline__ int lvl_off(int k) {  // sum over j < k of (64 >> j)^2 = (4^6 - 4^(6-k)) * 4 / 3
    return ((4096 - (4096 >> (2 * k))) * 4) / 3;
}

struct ModeOp {
    int fill;
    // the value with the most children among those that are not fill; ties to the smallest value; fill when none is left
    __device__ __forceinline__ signed char operator()(signed char a, signed char b, signed char c, signed char d) const {
        const int v[4] = {a, b, c, d};
        int best = fill, bestn = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = (v[0] == v[i]) + (v[1] == v[i]) + (v[2] == v[i]) + (v[3] == v[i]);
            if (v[i] != fill && (n > bestn || (n == bestn && v[i] < best))) best = v[i], bestn = n;
        }
        return (signed char)best;
    }
};

struct MeanOp {
    // the float32 sum of the children that are not NaN in row-major order, divided (correctly rounded) by their number; NaN when none
    __device__ __forceinline__ float operator()(float a, float b, float c, float d) const {
        const float v[4] = {a, b, c, d};
        float s = 0.f;
        int n = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (v[i] == v[i]) {
                s = n ? s + v[i] : v[i];
                ++n;
            }
        return n ? __fdiv_rn(s, (float)n) : __uint_as_float(0x7fc00000u);
    }
};

// levels 1..nlev of the block in lds[0 .. 4096) -> LDS and dst.  dst: level-major, then (bands, H_k, W_k).
template <typename T, typename Op>
__device__ __forceinline__ void emit_levels(T* lds, const Op op, int nlev, int H, int W, int bands, int band, T* __restrict__ dst) {
    long base = 0;
    int Hk = H, Wk = W;
    for (int k = 1; k <= nlev; ++k) {
        const int sh = 6 - k, n = CB >> k, pn = n * 2;  // side of level k inside the block, pitch of level k - 1
        const T* in = lds + lvl_off(k - 1);
        T* out = lds + lvl_off(k);
        Hk = (Hk + 1) >> 1, Wk = (Wk + 1) >> 1;
        for (int i = threadIdx.x; i < n * n; i += CTPB) {
            const int r = i >> sh, c = i & (n - 1);
            const T* p = in + (2 * r) * pn + 2 * c;
            const T v = op(p[0], p[1], p[pn], p[pn + 1]);
            out[i] = v;
            const int gr = blockIdx.y * n + r, gc = blockIdx.x * n + c;
            if (gr < Hk && gc < Wk) dst[base + ((long)band * Hk + gr) * Wk + gc] = v;
        }
        base += (long)bands * Hk * Wk;
        __syncthreads();
    }
}

__global__ __launch_bounds__(CTPB) void overview_mode_kernel(const signed char* __restrict__ src, int H, int W, int fill, int ncls, int nlev,
                                                             int vec, signed char* __restrict__ dst, unsigned long long* __restrict__ counts) {
    __shared__ __attribute__((aligned(16))) signed char lds[CLDS + 11];
    __shared__ unsigned hist[MAX_NCLS + 1];
    if (counts) {
        if (threadIdx.x <= MAX_NCLS) hist[threadIdx.x] = 0u;
        __syncthreads();
    }
    // thread t: 16 pixels of block row t / 4 from column (t % 4) * 16; outside the raster = fill (ignored by the rule, like a missing child)
    const int lr = threadIdx.x >> 2, lc = (threadIdx.x & 3) * 16;
    const int gr = blockIdx.y * CB + lr, gc = blockIdx.x * CB + lc;
    signed char px[16];
    if (vec && gr < H && gc < W) {
        const uint4 u = *reinterpret_cast<const uint4*>(src + (long)gr * W + gc);
        __builtin_memcpy(px, &u, 16);
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) px[j] = (gr < H && gc + j < W) ? src[(long)gr * W + gc + j] : (signed char)fill;
    }
    uint4 u;
    __builtin_memcpy(&u, px, 16);
    *reinterpret_cast<uint4*>(lds + lr * CB + lc) = u;
    if (counts) {  // uniform over the grid
        int key = -1, cnt = 0;  // -1: outside the raster, counted nowhere
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int v = px[j];
            const int k = (gr < H && gc + j < W) ? ((v != fill && v >= 0 && v < ncls) ? v : ncls) : -1;
            if (k != key) {
                if (key >= 0) atomicAdd(&hist[key], (unsigned)cnt);
                key = k;
                cnt = 0;
            }
            ++cnt;
        }
        const Seg s = seg_of(key);  // the thread's last run joins those of its neighbours: one add per run of lanes
        const int tot = seg_reduce<OpAdd>(cnt, s);
        if (s.head && key >= 0) atomicAdd(&hist[key], (unsigned)tot);
    }
    __syncthreads();
    emit_levels<signed char, ModeOp>(lds, ModeOp{fill}, nlev, H, W, 1, 0, dst);
    if (counts && threadIdx.x <= ncls && hist[threadIdx.x]) atomicAdd(counts + threadIdx.x, (unsigned long long)hist[threadIdx.x]);
}

__global__ __launch_bounds__(CTPB) void overview_mean_kernel(const float* __restrict__ src, int bands, int H, int W, int nlev, int vec,
                                                             float* __restrict__ dst) {
    __shared__ __attribute__((aligned(16))) float lds[CLDS + 3];
    const int band = blockIdx.z;
    const float* plane = src + (long)band * H * W;
    const float nan = __uint_as_float(0x7fc00000u);
#pragma unroll
    for (int i = 0; i < 4; ++i) {  // 4 x (256 threads x 4 floats): 16 rows of the block per step
        const int idx = i * CTPB + threadIdx.x;
        const int lr = idx >> 4, lc = (idx & 15) * 4;
        const int gr = blockIdx.y * CB + lr, gc = blockIdx.x * CB + lc;
        float4 v;
        if (vec && gr < H && gc < W) {
            v = *reinterpret_cast<const float4*>(plane + (long)gr * W + gc);
        } else {
            const bool row = gr < H;
            v.x = row && gc < W ? plane[(long)gr * W + gc] : nan;
            v.y = row && gc + 1 < W ? plane[(long)gr * W + gc + 1] : nan;
            v.z = row && gc + 2 < W ? plane[(long)gr * W + gc + 2] : nan;
            v.w = row && gc + 3 < W ? plane[(long)gr * W + gc + 3] : nan;
        }
        *reinterpret_cast<float4*>(lds + lr * CB + lc) = v;
    }
    __syncthreads();
    emit_levels<float, MeanOp>(lds, MeanOp{}, nlev, H, W, bands, band, dst);
}

// One thread = 16 bytes of the output: N = 16 / sizeof(T) consecutive elements of one tile row.  q counts those chunks in output order.
template <typename T>
__global__ __launch_bounds__(CTPB) void cog_tiles_kernel(const T* __restrict__ src, int H, int W, int tile, int nx, int ny, T pad, int predictor,
                                                         long chunks, uint4* __restrict__ dst) {
    constexpr int N = 16 / (int)sizeof(T);
    const long q = blockIdx.x * (long)CTPB + threadIdx.x;
    if (q >= chunks) return;
    const int per_row = tile / N;
    const int cx = (int)(q % per_row);
    const long rowid = q / per_row;  // (band, ty, tx, row)
    const int row = (int)(rowid % tile);
    const long t = rowid / tile;
    const int tx = (int)(t % nx), ty = (int)((t / nx) % ny);
    const long band = t / ((long)nx * ny);
    const int y = ty * tile + row, x0 = tx * tile + cx * N;
    const T* line = src + (band * H + y) * (long)W;
    const bool in_row = y < H;
    T prev = 0;  // the element left of the chunk inside the tile row; none at the tile's first column
    if (predictor == 2 && cx > 0) prev = (in_row && x0 - 1 < W) ? line[x0 - 1] : pad;
    T out[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const T v = (in_row && x0 + j < W) ? line[x0 + j] : pad;
        out[j] = predictor == 2 ? (T)(v - prev) : v;  // wrap-around arithmetic in the element's width
        prev = v;
    }
    uint4 u;
    __builtin_memcpy(&u, out, 16);
    dst[q] = u;
}

}  // namespace

#define ST(s) ((hipStream_t)(s))
#define IG_REQUIRE_PYRAMID(name)                                                                    \
    IG_REQUIRE(H >= 0 && W >= 0, name ": need H >= 0 and W >= 0 (H %d, W %d)", H, W);               \
    IG_REQUIRE((long)H * W <= 0x7fffffffL, name ": H * W = %ld exceeds 2^31 - 1", (long)H * W);     \
    IG_REQUIRE(levels >= 1 && levels <= 12, name ": need 1 <= levels <= 12 (got %d)", levels)

// Walks the launches of a pyramid: up to CMAXL levels each, the next one on the last level written.  launch(src, H, W, nlev, dst, first)
template <typename T, typename F>
static int pyramid_launches(const T* src, int bands, int H, int W, int levels, T* dst, F launch) {
    bool first = true;
    while (levels > 0) {
        const int n = levels < CMAXL ? levels : CMAXL;
        const int rc = launch(src, H, W, n, dst, first);
        if (rc != IG_OK) return rc;
        long off = 0, last = 0;
        for (int k = 0; k < n; ++k) {
            H = (H + 1) / 2, W = (W + 1) / 2;
            last = off;
            off += (long)bands * H * W;
        }
        src = dst + last;
        dst += off;
        levels -= n;
        first = false;
    }
    return IG_OK;
}

static inline dim3 block_grid(int H, int W, int bands) { return dim3((unsigned)ig_cdiv(W, CB), (unsigned)ig_cdiv(H, CB), (unsigned)bands); }

extern "C" {

int ig_overview_mode(const signed char* src, int H, int W, int fill, int ncls, int levels, signed char* dst, unsigned long long* counts,
                     void* stream) {
    IG_REQUIRE_PYRAMID("ig_overview_mode");
    IG_REQUIRE(fill >= -128 && fill <= 127, "ig_overview_mode: fill must fit int8 (got %d)", fill);
    IG_REQUIRE(ncls >= 1 && ncls <= MAX_NCLS, "ig_overview_mode: 1 <= ncls <= %d (got %d)", MAX_NCLS, ncls);
    if ((long)H * W == 0) return IG_OK;
    IG_REQUIRE(src && dst, "ig_overview_mode: null pointer");
    IG_REQUIRE(((uintptr_t)counts & 7) == 0, "ig_overview_mode: counts must be 8-byte aligned");
    IG_REQUIRE(ig_cdiv(H, CB) <= 65535, "ig_overview_mode: H = %d exceeds 65535 blocks of 64 rows", H);
    return pyramid_launches<signed char>(src, 1, H, W, levels, dst, [&](const signed char* s, int h, int w, int n, signed char* d, bool first) {
        const int vec = (w % 16 == 0) && ((uintptr_t)s & 15) == 0;
        return ig_launch<overview_mode_kernel>("ig_overview_mode", block_grid(h, w, 1), dim3(CTPB), 0, ST(stream), s, h, w, fill, ncls, n, vec, d,
                                               first ? counts : (unsigned long long*)nullptr);
    });
}

int ig_overview_mean(const float* src, int bands, int H, int W, int levels, float* dst, void* stream) {
    IG_REQUIRE_PYRAMID("ig_overview_mean");
    IG_REQUIRE(bands >= 0 && bands <= 65535, "ig_overview_mean: need 0 <= bands <= 65535 (got %d)", bands);
    IG_REQUIRE((long)bands * H * W <= (1L << 40), "ig_overview_mean: bands * H * W = %ld exceeds 2^40", (long)bands * H * W);
    if ((long)bands * H * W == 0) return IG_OK;
    IG_REQUIRE(src && dst, "ig_overview_mean: null pointer");
    IG_REQUIRE(((uintptr_t)src & 3) == 0 && ((uintptr_t)dst & 3) == 0, "ig_overview_mean: src and dst must be 4-byte aligned");
    IG_REQUIRE(ig_cdiv(H, CB) <= 65535, "ig_overview_mean: H = %d exceeds 65535 blocks of 64 rows", H);
    return pyramid_launches<float>(src, bands, H, W, levels, dst, [&](const float* s, int h, int w, int n, float* d, bool) {
        const int vec = (w % 4 == 0) && ((uintptr_t)s & 15) == 0;
        return ig_launch<overview_mean_kernel>("ig_overview_mean", block_grid(h, w, bands), dim3(CTPB), 0, ST(stream), s, bands, h, w, n, vec, d);
    });
}

int ig_cog_tiles(const void* src, int bands, int H, int W, int elem_size, int is_float, int tile, unsigned pad, int predictor, void* dst,
                 void* stream) {
    IG_REQUIRE(H >= 0 && W >= 0, "ig_cog_tiles: need H >= 0 and W >= 0 (H %d, W %d)", H, W);
    IG_REQUIRE(bands >= 0 && bands <= 65535, "ig_cog_tiles: need 0 <= bands <= 65535 (got %d)", bands);
    IG_REQUIRE((long)H * W <= 0x7fffffffL, "ig_cog_tiles: H * W = %ld exceeds 2^31 - 1", (long)H * W);
    IG_REQUIRE(elem_size == 1 || elem_size == 2 || elem_size == 4, "ig_cog_tiles: elem_size must be 1, 2 or 4 (got %d)", elem_size);
    IG_REQUIRE(tile >= 16 && tile <= 4096 && tile % 16 == 0, "ig_cog_tiles: tile must be a multiple of 16 in 16..4096 (got %d)", tile);
    IG_REQUIRE(predictor == 1 || predictor == 2, "ig_cog_tiles: predictor must be 1 or 2 (got %d)", predictor);
    IG_REQUIRE(!(predictor == 2 && is_float), "ig_cog_tiles: predictor 2 is for integers only (floating point samples given)");
    IG_REQUIRE(!is_float || elem_size == 4, "ig_cog_tiles: floating point samples have elem_size 4 (got %d)", elem_size);
    const int nx = ig_cdiv(W, tile), ny = ig_cdiv(H, tile);
    // (ny * tile) * (nx * tile) < (H + 4096) * (W + 4096) <= 2^44 with H * W < 2^31, times 4 bytes and 65535 bands: below 2^62
    const long bytes = (long)bands * ny * nx * tile * tile * elem_size;
    IG_REQUIRE(bytes <= (1L << 40), "ig_cog_tiles: the tiled raster has %ld bytes, more than 2^40", bytes);
    if (bytes == 0) return IG_OK;
    IG_REQUIRE(src && dst, "ig_cog_tiles: null pointer");
    IG_REQUIRE(((uintptr_t)src & (elem_size - 1)) == 0, "ig_cog_tiles: src must be aligned to its elements");
    IG_REQUIRE(((uintptr_t)dst & 15) == 0, "ig_cog_tiles: dst must be 16-byte aligned");
    const long chunks = bytes / 16;
    const dim3 grid((unsigned)((chunks + CTPB - 1) / CTPB));
    if (elem_size == 1)
        return ig_launch<cog_tiles_kernel<uint8_t>>("ig_cog_tiles", grid, dim3(CTPB), 0, ST(stream), (const uint8_t*)src, H, W, tile, nx, ny,
                                                    (uint8_t)pad, predictor, chunks, (uint4*)dst);
    if (elem_size == 2)
        return ig_launch<cog_tiles_kernel<uint16_t>>("ig_cog_tiles", grid, dim3(CTPB), 0, ST(stream), (const uint16_t*)src, H, W, tile, nx, ny,
                                                     (uint16_t)pad, predictor, chunks, (uint4*)dst);
    return ig_launch<cog_tiles_kernel<uint32_t>>("ig_cog_tiles", grid, dim3(CTPB), 0, ST(stream), (const uint32_t*)src, H, W, tile, nx, ny,
                                                 (uint32_t)pad, predictor, chunks, (uint4*)dst);
}

}  // extern "C"
