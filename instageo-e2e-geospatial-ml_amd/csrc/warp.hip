// Reprojection and resampling of north-up rasters between grids for gfx950.  The reference's viewer reprojects with
// rasterio before display (apps/viz.py); here the warp is what brings the mosaics of several UTM zones onto one canvas.  The rule is stated
// in include/instageo_hip.h.  A GATHER: every destination pixel is computed by the one thread that stores it.  No atomics, no waiting
// between workgroups, every result unique (independent of scheduling).
//
//   coords_kernel     one thread per destination pixel: (u, v) in one source grid, as float64 planes.
//   warp_kernel<T, BILINEAR>   one workgroup of 256 threads per 64 x 64 block of the destination (origin at multiples of 64: the blocking of
//                     mosaic.hip and cog.hip).  The descriptions of the (at most 8) sources are checked and staged in LDS once; the block's
//                     source list (CSR, built by the host) is walked backwards (last) or forwards (first) until a source contributes.  A
//                     wave owns 64 consecutive pixels of a row and stores them with one instruction; a thread takes 16 rows in turn.
//                     The longitude and latitude of a pixel are computed once, when the first source of another coordinate system asks
//                     for them; sources of one coordinate system share the forward projection.
//
// Out-of-range accesses are impossible as long as starts[i] + h * w lies inside the packed buffer (the caller's promise, checked by
// ops.warp): a source index outside [0, nsrc) or a description outside the stated bounds is staged as an empty source, every source load
// is guarded by 0 <= row < h and 0 <= column < w, tested on the float64 coordinates before they become integers (NaN fails), every store
// by row < H and column < W.
#include "common.h"
#include "warp_proj.h"

namespace {

constexpr int WB = 64, WTPB = 256, WMAX = 8;  // block side, threads, sources per launch
constexpr int WLIM = 1 << 30;                 // h, w at most this
constexpr int R_LAST = 0, R_FIRST = 1;

__global__ __launch_bounds__(WTPB) void coords_kernel(const double* __restrict__ dst_crs, const double* __restrict__ dst_grid, int H, int W,
                                                      const double* __restrict__ src_crs, const double* __restrict__ src_grid,
                                                      double* __restrict__ uv) {
    const int c = blockIdx.x * WB + (threadIdx.x & 63), r = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (r >= H || c >= W) return;
    const Crs dc = load_crs(dst_crs), sc = load_crs(src_crs);
    const Grid dg = load_grid(dst_grid), sg = load_grid(src_grid);
    double x = dg.x0 + (c + 0.5) * dg.sx, y = dg.y0 - (r + 0.5) * dg.sy;
    bool ok = grid_ok(sg);
    if (ok && !same_crs(dc, sc)) {
        double lon, lat;
        ok = to_lonlat(dc, x, y, lon, lat) && from_lonlat(sc, lon, lat, x, y);
    }
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const long at = (long)r * W + c;
    uv[at] = ok ? (x - sg.x0) / sg.sx : nan;
    uv[(long)H * W + at] = ok ? (sg.y0 - y) / sg.sy : nan;
}

struct Sources {
    Crs crs[WMAX];
    Grid grid[WMAX];
    long long start[WMAX];
    int h[WMAX], w[WMAX];  // h = 0: contributes nothing
    int same[WMAX];        // the destination's coordinate system: affine
    int rep[WMAX];         // the smallest index with this coordinate system
};

__device__ __forceinline__ bool clear_px(signed char v, int fill) { return v == (signed char)fill; }
__device__ __forceinline__ bool clear_px(float v, int) { return v != v; }

// the value source e gives at (u, v); false: no contribution
template <typename T, bool BILINEAR>
__device__ __forceinline__ bool sample(const T* __restrict__ src, const Sources& s, int e, double u, double v, int fill, T& out) {
    const int h = s.h[e], w = s.w[e];
    const T* p = src + s.start[e];
    if constexpr (!BILINEAR) {
        const double fc = floor(u), fr = floor(v);
        if (!(fc >= 0.0 && fc < (double)w && fr >= 0.0 && fr < (double)h)) return false;
        const T x = p[(long)fr * w + (long)fc];
        if (clear_px(x, fill)) return false;
        out = x;
        return true;
    } else {
        const double a = u - 0.5, b = v - 0.5;
        const double fc = floor(a), fr = floor(b);
        if (!(fc >= -1.0 && fc < (double)w && fr >= -1.0 && fr < (double)h)) return false;  // no neighbour inside (NaN included)
        const int c0 = (int)fc, r0 = (int)fr;
        const double wx = a - fc, wy = b - fr;
        const double wt[4] = {(1.0 - wx) * (1.0 - wy), wx * (1.0 - wy), (1.0 - wx) * wy, wx * wy};
        double acc = 0.0, tot = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int rr = r0 + (q >> 1), cc = c0 + (q & 1);
            if ((unsigned)rr < (unsigned)h && (unsigned)cc < (unsigned)w && wt[q] > 0.0) {
                const float x = p[(long)rr * w + cc];
                if (x == x) acc += wt[q] * (double)x, tot += wt[q];
            }
        }
        if (!(tot > 0.0)) return false;
        out = (float)(acc / tot);
        return true;
    }
}

template <typename T, bool BILINEAR>
__global__ __launch_bounds__(WTPB) void warp_kernel(const T* __restrict__ src, const long long* __restrict__ starts,
                                                    const double* __restrict__ src_crs, const double* __restrict__ src_grid,
                                                    const int* __restrict__ src_size, int nsrc, const int* __restrict__ bin_ptr,
                                                    const int* __restrict__ bin_idx, const double* __restrict__ dst_crs,
                                                    const double* __restrict__ dst_grid, int H, int W, int rule, int fill, T* __restrict__ dst,
                                                    unsigned char* __restrict__ src_id) {
    __shared__ Sources s;
    const Crs dc = load_crs(dst_crs);
    const Grid dg = load_grid(dst_grid);
    if ((int)threadIdx.x < WMAX) {
        const int i = threadIdx.x;
        Crs c{0.0, 0.0, 0.0, 0.0, 0.0};
        Grid g{0.0, 0.0, 1.0, 1.0};
        long long st = 0;
        int h = 0, w = 0, rep = i;
        if (i < nsrc) {
            c = load_crs(src_crs + 5 * i);
            g = load_grid(src_grid + 4 * i);
            st = starts[i];
            const int hh = src_size[2 * i], ww = src_size[2 * i + 1];
            if (hh >= 1 && ww >= 1 && hh <= WLIM && ww <= WLIM && st >= 0 && grid_ok(g)) h = hh, w = ww;
            for (int j = i - 1; j >= 0; --j)
                if (same_crs(load_crs(src_crs + 5 * j), c)) rep = j;
        }
        s.crs[i] = c, s.grid[i] = g, s.start[i] = st, s.h[i] = h, s.w[i] = w, s.same[i] = same_crs(c, dc), s.rep[i] = rep;
    }
    __syncthreads();
    const int b = blockIdx.y * gridDim.x + blockIdx.x;
    const int first = bin_ptr ? bin_ptr[b] : 0;
    const int n = bin_ptr ? max(bin_ptr[b + 1] - first, 0) : 0;
    const int* list = bin_idx + first;
    const int c = blockIdx.x * WB + (threadIdx.x & 63);
    if (c >= W) return;
    const double x = dg.x0 + (c + 0.5) * dg.sx;
    for (int k = 0; k < WB / 4; ++k) {
        const int r = blockIdx.y * WB + 4 * k + (threadIdx.x >> 6);  // wave-uniform
        if (r >= H) break;
        const double y = dg.y0 - (r + 0.5) * dg.sy;
        T out;
        if constexpr (sizeof(T) == 1) out = (T)fill;
        else out = __uint_as_float(0x7fc00000u);
        int who = 255;
        int ll = 0;  // 0: longitude / latitude not asked for yet, 1: inside the domain, -1: outside
        double lon = 0.0, lat = 0.0, px = 0.0, py = 0.0;
        int cur = -1;  // the coordinate system (px, py) belongs to
        bool pok = false;
        for (int i = 0; i < n; ++i) {
            const int e = list[rule == R_LAST ? n - 1 - i : i];
            if ((unsigned)e >= (unsigned)nsrc || s.h[e] == 0) continue;
            double sxp, syp;
            if (s.same[e]) {
                sxp = x, syp = y;
            } else {
                if (ll == 0) ll = to_lonlat(dc, x, y, lon, lat) ? 1 : -1;
                if (ll < 0) continue;  // outside the destination's domain: only a source of its own system can contribute
                if (s.rep[e] != cur) cur = s.rep[e], pok = from_lonlat(s.crs[e], lon, lat, px, py);
                if (!pok) continue;
                sxp = px, syp = py;
            }
            const Grid& g = s.grid[e];
            if (sample<T, BILINEAR>(src, s, e, (sxp - g.x0) / g.sx, (g.y0 - syp) / g.sy, fill, out)) {
                who = e;
                break;
            }
        }
        const long at = (long)r * W + c;
        dst[at] = out;
        if (src_id) src_id[at] = (unsigned char)who;
    }
}

template <typename T, bool BILINEAR>
int launch(const void* src, const long long* starts, const double* src_crs, const double* src_grid, const int* src_size, int nsrc,
           const int* bin_ptr, const int* bin_idx, const double* dst_crs, const double* dst_grid, int H, int W, int rule, int fill, void* dst,
           unsigned char* src_id, void* stream) {
    return ig_launch<warp_kernel<T, BILINEAR>>("ig_warp", dim3((unsigned)ig_cdiv(W, WB), (unsigned)ig_cdiv(H, WB)), dim3(WTPB), 0,
                                               (hipStream_t)stream, (const T*)src, starts, src_crs, src_grid, src_size, nsrc, bin_ptr, bin_idx,
                                               dst_crs, dst_grid, H, W, rule, fill, (T*)dst, src_id);
}

}  // namespace

extern "C" int ig_warp_coords(const double* dst_crs, const double* dst_grid, int H, int W, const double* src_crs, const double* src_grid,
                              double* uv, void* stream) {
    IG_REQUIRE(H >= 0 && W >= 0, "ig_warp_coords: need H >= 0 and W >= 0 (H %d, W %d)", H, W);
    IG_REQUIRE((long)H * W <= 0x7fffffffL, "ig_warp_coords: H * W = %ld exceeds 2^31 - 1", (long)H * W);
    if ((long)H * W == 0) return IG_OK;
    IG_REQUIRE(ig_cdiv(H, 4) <= 65535, "ig_warp_coords: H = %d exceeds 65535 workgroups of 4 rows", H);
    IG_REQUIRE(dst_crs && dst_grid && src_crs && src_grid && uv, "ig_warp_coords: null pointer");
    IG_REQUIRE((((uintptr_t)dst_crs | (uintptr_t)dst_grid | (uintptr_t)src_crs | (uintptr_t)src_grid | (uintptr_t)uv) & 7) == 0,
               "ig_warp_coords: the float64 arrays must be 8-byte aligned");
    return ig_launch<coords_kernel>("ig_warp_coords", dim3((unsigned)ig_cdiv(W, WB), (unsigned)ig_cdiv(H, 4)), dim3(WTPB), 0, (hipStream_t)stream,
                                    dst_crs, dst_grid, H, W, src_crs, src_grid, uv);
}

extern "C" int ig_warp(const void* src, const long long* starts, const double* src_crs, const double* src_grid, const int* src_size, int nsrc,
                       const int* bin_ptr, const int* bin_idx, const double* dst_crs, const double* dst_grid, int H, int W, int elem_size,
                       int resampling, int rule, int fill, void* dst, unsigned char* src_id, void* stream) {
    IG_REQUIRE(elem_size == 1 || elem_size == 4, "ig_warp: elem_size must be 1 (int8) or 4 (float32) (got %d)", elem_size);
    IG_REQUIRE(resampling == 0 || resampling == 1, "ig_warp: resampling must be 0 nearest or 1 bilinear (got %d)", resampling);
    IG_REQUIRE(resampling == 0 || elem_size == 4, "ig_warp: bilinear resampling needs float32 rasters (elem_size %d)", elem_size);
    IG_REQUIRE(rule == R_LAST || rule == R_FIRST, "ig_warp: rule must be 0 last or 1 first (got %d)", rule);
    IG_REQUIRE(fill >= -128 && fill <= 127, "ig_warp: fill must fit int8 (got %d)", fill);
    IG_REQUIRE(H >= 0 && W >= 0, "ig_warp: need H >= 0 and W >= 0 (H %d, W %d)", H, W);
    IG_REQUIRE((long)H * W <= 0x7fffffffL, "ig_warp: H * W = %ld exceeds 2^31 - 1", (long)H * W);
    IG_REQUIRE(nsrc >= 0 && nsrc <= WMAX, "ig_warp: need 0 <= nsrc <= %d (got %d)", WMAX, nsrc);
    if ((long)H * W == 0) return IG_OK;
    IG_REQUIRE(ig_cdiv(H, WB) <= 65535, "ig_warp: H = %d exceeds 65535 blocks of 64 rows", H);
    IG_REQUIRE(dst && dst_crs && dst_grid, "ig_warp: null pointer (dst, dst_crs or dst_grid)");
    IG_REQUIRE(((uintptr_t)dst & (elem_size - 1)) == 0, "ig_warp: dst must be aligned to its elements");
    IG_REQUIRE((((uintptr_t)dst_crs | (uintptr_t)dst_grid) & 7) == 0, "ig_warp: the float64 arrays must be 8-byte aligned");
    if (nsrc > 0) {
        IG_REQUIRE(src && starts && src_crs && src_grid && src_size && bin_ptr && bin_idx, "ig_warp: null pointer");
        IG_REQUIRE(((uintptr_t)src & (elem_size - 1)) == 0, "ig_warp: src must be aligned to its elements");
        IG_REQUIRE((((uintptr_t)src_crs | (uintptr_t)src_grid | (uintptr_t)starts) & 7) == 0 &&
                       (((uintptr_t)src_size | (uintptr_t)bin_ptr | (uintptr_t)bin_idx) & 3) == 0,
                   "ig_warp: the float64 arrays and starts must be 8-byte, src_size, bin_ptr and bin_idx 4-byte aligned");
    } else {
        bin_ptr = nullptr;  // every block's list is empty: the destination becomes fill
    }
#define WARP(T, B) \
    return launch<T, B>(src, starts, src_crs, src_grid, src_size, nsrc, bin_ptr, bin_idx, dst_crs, dst_grid, H, W, rule, fill, dst, src_id, stream)
    if (elem_size == 1) WARP(signed char, false);
    if (resampling == 0) WARP(float, false);
    WARP(float, true);
#undef WARP
}
