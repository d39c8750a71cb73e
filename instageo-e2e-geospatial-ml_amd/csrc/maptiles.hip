// Web Mercator map tiles rendered from an overview pyramid for gfx950.  The reference's backend answers every
// tiles/WebMercatorQuad/{z}/{x}/{y} request through TiTiler (new_apps/backend/app/tiler_service.py): a warp into EPSG:3857, an overview
// level, nearest sampling and a colormap or a rescale per request, on the host.  Here the rule, stated in include/instageo_hip.h, is one
// kernel for a batch of tiles.  A GATHER: every output pixel is computed and stored once by one thread; the only atomics are integer adds
// of the opaque counts, one per workgroup; results are unique (independent of scheduling).
//
//   tile_render_kernel<STYLE>   one workgroup of 256 threads per 64 x 64 block of one tile (the blocking of ig_chip_warp).  A wave owns 64
//                               consecutive pixels of a row and stores their 256 bytes with one instruction, a thread takes 16 rows in
//                               turn.  Per pixel: the float64 chain of warp_proj.h once, the scale to the tile's level, one gather per
//                               band, the colour, one 32-bit store.  The float64 chain is what the time goes to (a transverse Mercator
//                               pixel costs a few hundred float64 operations against 4 bytes stored); the row loop is kept rolled, which
//                               keeps the code to one copy of the chain.
//
// Out-of-range accesses are impossible as long as levels[k] holds bands * H_k * W_k elements (the caller's promise, checked by
// ops.tile_render): a source offset is formed only after 0 <= floor(v) < H_k and 0 <= floor(u) < W_k held on the float64 values (NaN
// fails), H * W <= 2^31 - 1 is checked by the entry point, a level outside [0, nlevels) or a grid that is not finite and positive reads
// nothing, a lut index is < 256 by construction, and tile is a multiple of 64, so every thread of every workgroup owns 16 pixels of rgba.
#include "common.h"
#include "pixel_seg.h"
#include "warp_proj.h"

namespace {

constexpr int MB = 64, MTPB = 256, MROWS = MB / 4;  // block side, threads, rows per thread
constexpr int MMAX_LEVELS = 13;                     // level 0 + the 12 of cog.hip
constexpr int S_PALETTE = 0, S_RAMP = 1, S_RGB = 2;

struct RenderArgs {
    int nlevels, H, W, tile, nb, ncolors, fill, o0, o1, o2;
    double lo, span;
};

// (int)rint(clamp((v - lo) / span, 0, 1) * 255): every operation rounded on its own
__device__ __forceinline__ unsigned ramp_index(float v, double lo, double span) {
#pragma clang fp contract(off)
    double t = ((double)v - lo) / span;
    t = t < 0.0 ? 0.0 : t > 1.0 ? 1.0 : t;
    return (unsigned)(int)rint(t * 255.0);
}

template <int STYLE>
__device__ __forceinline__ unsigned shade(const void* __restrict__ level, long off, long plane, const RenderArgs& a,
                                          const unsigned* __restrict__ lut) {
    if constexpr (STYLE == S_PALETTE) {
        const int v = static_cast<const signed char*>(level)[off];
        return (v >= 0 && v < a.ncolors && v != a.fill) ? lut[v] : 0u;
    } else if constexpr (STYLE == S_RAMP) {
        const float v = static_cast<const float*>(level)[off];
        return v != v ? 0u : lut[ramp_index(v, a.lo, a.span)];
    } else {
        const float* p = static_cast<const float*>(level) + off;
        const float r = p[a.o0 * plane], g = p[a.o1 * plane], b = p[a.o2 * plane];
        if (r != r || g != g || b != b) return 0u;
        return ramp_index(r, a.lo, a.span) | ramp_index(g, a.lo, a.span) << 8 | ramp_index(b, a.lo, a.span) << 16 | 0xff000000u;
    }
}

template <int STYLE>
__global__ __launch_bounds__(MTPB) void tile_render_kernel(const void* const* __restrict__ levels, const double* __restrict__ src_crs,
                                                           const double* __restrict__ src_grid, const double* __restrict__ tile_grids,
                                                           const int* __restrict__ tile_level, RenderArgs a, const unsigned* __restrict__ lut,
                                                           unsigned* __restrict__ rgba, int* __restrict__ opaque) {
    __shared__ int part[4];
    const int per = a.nb * a.nb;
    const int t = blockIdx.x / per, blk = blockIdx.x - t * per;
    const int br = (blk / a.nb) * MB, c = (blk % a.nb) * MB + (threadIdx.x & 63);
    const int wave = threadIdx.x >> 6;
    unsigned* q = rgba + ((long)t * a.tile + br + wave) * a.tile + c;  // pixel k lies 4 k rows further down
    const int lvl = tile_level[t];
    const Grid dg = load_grid(tile_grids + 4 * (long)t), sg = load_grid(src_grid);
    if (lvl < 0 || lvl >= a.nlevels || !grid_ok(dg) || !grid_ok(sg)) {  // uniform over the workgroup: a transparent tile, nothing read
#pragma unroll
        for (int k = 0; k < MROWS; ++k) q[(long)(4 * k) * a.tile] = 0u;
        return;
    }
    const Crs dc{2.0, 0.0, 0.0, 0.0, 0.0}, sc = load_crs(src_crs);
    const bool affine = same_crs(dc, sc);
    const long round_up = (1L << lvl) - 1;
    const int Hk = (int)((a.H + round_up) >> lvl), Wk = (int)((a.W + round_up) >> lvl);
    const long plane = (long)Hk * Wk;
    const double inv = 1.0 / (double)(1 << lvl);  // a power of two: the product is the exact quotient
    const void* level = levels[lvl];
    const double x = dg.x0 + (c + 0.5) * dg.sx;
    int count = 0;
#pragma unroll 1
    for (int k = 0; k < MROWS; ++k) {
        const int r = br + 4 * k + wave;  // wave-uniform
        double sx = x, sy = dg.y0 - (r + 0.5) * dg.sy;
        bool ok = true;
        if (!affine) {
            double lon, lat;
            ok = to_lonlat(dc, sx, sy, lon, lat) && from_lonlat(sc, lon, lat, sx, sy);
        }
        unsigned px = 0u;
        if (ok) {
            const double fc = floor((sx - sg.x0) / sg.sx * inv), fr = floor((sg.y0 - sy) / sg.sy * inv);
            if (fc >= 0.0 && fc < (double)Wk && fr >= 0.0 && fr < (double)Hk) px = shade<STYLE>(level, (long)fr * Wk + (long)fc, plane, a, lut);
        }
        q[(long)(4 * k) * a.tile] = px;
        count += (px >> 24) != 0u;
    }
    const int total = block_sum_int(count, part);
    if (threadIdx.x == 0 && total) atomicAdd(opaque + t, total);
}

}  // namespace

extern "C" int ig_tile_render(const void* const* levels, int nlevels, int elem_size, int bands, int H, int W, const double* src_crs,
                              const double* src_grid, const double* tile_grids, const int* tile_level, int n, int tile, int style,
                              const unsigned char* lut, int ncolors, int fill, double lo, double span, int order0, int order1, int order2,
                              unsigned char* rgba, int* opaque, void* stream) {
    IG_REQUIRE(n >= 0, "ig_tile_render: need n >= 0 (got %d)", n);
    IG_REQUIRE(style >= S_PALETTE && style <= S_RGB, "ig_tile_render: style must be 0 palette, 1 ramp or 2 rgb (got %d)", style);
    IG_REQUIRE(elem_size == (style == S_PALETTE ? 1 : 4) && bands == (style == S_RGB ? 3 : 1),
               "ig_tile_render: style %d needs %s (got elem_size %d, bands %d)", style,
               style == S_PALETTE ? "int8 with 1 band" : style == S_RAMP ? "float32 with 1 band" : "float32 with 3 bands", elem_size, bands);
    IG_REQUIRE(nlevels >= 1 && nlevels <= MMAX_LEVELS, "ig_tile_render: need 1 <= nlevels <= %d (got %d)", MMAX_LEVELS, nlevels);
    IG_REQUIRE(H >= 1 && W >= 1, "ig_tile_render: need H >= 1 and W >= 1 (H %d, W %d)", H, W);
    IG_REQUIRE((long)H * W <= 0x7fffffffL, "ig_tile_render: H * W = %ld exceeds 2^31 - 1", (long)H * W);
    IG_REQUIRE(tile >= 64 && tile <= 1024 && tile % 64 == 0, "ig_tile_render: tile must be a multiple of 64 in 64..1024 (got %d)", tile);
    IG_REQUIRE(ncolors >= 0 && ncolors <= 256, "ig_tile_render: need 0 <= ncolors <= 256 (got %d)", ncolors);
    IG_REQUIRE(fill >= -128 && fill <= 127, "ig_tile_render: fill must fit int8 (got %d)", fill);
    if (style != S_PALETTE) {
        // x - x is NaN for NaN and the infinities
        IG_REQUIRE(lo - lo == 0.0 && span - span == 0.0 && span > 0.0, "ig_tile_render: need a finite lo and a finite span = hi - lo > 0 (got %g, %g)", lo,
                   span);
    }
    if (style == S_RGB) {
        IG_REQUIRE((unsigned)order0 < 3u && (unsigned)order1 < 3u && (unsigned)order2 < 3u, "ig_tile_render: order must name planes 0..2 (got %d, %d, %d)",
                   order0, order1, order2);
    }
    if (n == 0) return IG_OK;
    IG_REQUIRE((long)n * tile * tile < 0x80000000L, "ig_tile_render: n * tile * tile = %ld reaches 2^31 (n %d, tile %d)", (long)n * tile * tile, n, tile);
    IG_REQUIRE(levels && src_crs && src_grid && tile_grids && tile_level && rgba && opaque, "ig_tile_render: null pointer");
    IG_REQUIRE(style == S_RGB || lut, "ig_tile_render: null pointer (lut)");
    IG_REQUIRE((((uintptr_t)levels | (uintptr_t)src_crs | (uintptr_t)src_grid | (uintptr_t)tile_grids) & 7) == 0,
               "ig_tile_render: the level table and the float64 arrays must be 8-byte aligned");
    IG_REQUIRE((((uintptr_t)tile_level | (uintptr_t)lut | (uintptr_t)rgba | (uintptr_t)opaque) & 3) == 0,
               "ig_tile_render: tile_level, lut, rgba and opaque must be 4-byte aligned");
    const int nb = tile / MB;
    const RenderArgs a{nlevels, H, W, tile, nb, ncolors, fill, order0, order1, order2, lo, span};
    const dim3 grid((unsigned)((long)nb * nb * n));  // < 2^31 / 4096
#define TILE_RENDER(S)                                                                                                                 \
    return ig_launch<tile_render_kernel<S>>("ig_tile_render", grid, dim3(MTPB), 0, (hipStream_t)stream, levels, src_crs, src_grid,     \
                                            tile_grids, tile_level, a, (const unsigned*)lut, (unsigned*)rgba, opaque)
    if (style == S_PALETTE) TILE_RENDER(S_PALETTE);
    if (style == S_RAMP) TILE_RENDER(S_RAMP);
    TILE_RENDER(S_RGB);
#undef TILE_RENDER
}
