// Sentinel-2 chips warped onto label grids for gfx950.  The reference's label-raster chip creator for Sentinel-2
// (instageo/data/raster_chip_creator.py, S2RasterPipeline.process_row) lets stackstac resample the 10 m, 20 m and 60 m bands and the scene
// classification onto the label's coordinate system and resolution on the host and cuts, masks and quality-checks with xarray; here the
// rule, stated in include/instageo_hip.h, is one kernel for all chips of a granule that reads every plane on its own grid.  A GATHER: every
// output element is written once by the thread that computed it; the tallies are integer atomics, one set per workgroup; results are
// unique (independent of scheduling).
//
//   s2_chip_warp_kernel<L>   the blocking of chip_warp_kernel (raster_chips.hip): one workgroup of 256 threads per 64 x 64 block of one
//                            chip, a wave owns 64 consecutive pixels of a row, a thread 16 rows of one column.  Phase 1: the float64 chain
//                            of warp_proj.h once per pixel -> the pixel's SOURCE MAP coordinates (x, y) in registers (NaN: none).  Phase 2,
//                            class by class: the class's 16 source offsets rs * W + cs from (x, y) by the class's grid (two divisions per
//                            pixel), then the SCL bytes of the class's SCL planes -> one 32-bit date mask per pixel.  Phase 3, class by
//                            class: the offsets again, then the class's bands stream through: gather, offset, mask, range, count, one
//                            store.  Phase 4: the validity byte and the label pixel (chip_epilogue.h).
//                            The offsets of one class at a time, recomputed in phase 3, instead of 16 x G offsets held: 32 float64
//                            coordinates (64 registers) + 16 offsets + 16 date masks stay below 128 registers for any G.
//
// Out-of-range accesses are impossible: a source offset is formed only after 0 <= floor(v) < H_g and 0 <= floor(u) < W_g held on the
// float64 values (NaN fails) for a class with 1 <= H_g, W_g and H_g * W_g <= 2^31 - 1; a plane whose class index lies outside [0, G) or
// whose start is negative is never addressed; a grid (the chip's or any class's) that is not finite and positive yields no coordinates at
// all; every store and every label load is guarded by row < S and column < S of a chip index below n.
#include "chip_kernels.h"
#include "common.h"
#include "warp_proj.h"

namespace {

constexpr int QB = 64, QTPB = 256, QROWS = QB / 4;  // block side, threads, rows per thread
constexpr int QMAX_G = 8;

struct S2WarpArgs {
    int T, C, S, G, any, no_data, boa, range, lo, hi, nb, valid_bit, K;
    unsigned class_bits;
};

// the source offsets of the thread's pixels in class g (-1: outside the plane, no coordinates, or a class that reads nothing) -> the
// class's plane size in pixels (0: nothing to read)
__device__ __forceinline__ long class_offsets(const double* __restrict__ class_grid, const int* __restrict__ class_size, int g,
                                              const double (&px)[QROWS], const double (&py)[QROWS], int (&off)[QROWS]) {
    const Grid sg = load_grid(class_grid + 4 * g);
    int H = class_size[2 * g];
    const int W = class_size[2 * g + 1];
    if (H < 1 || W < 1 || (long)H * W > 0x7fffffffL) H = 0;
#pragma unroll
    for (int k = 0; k < QROWS; ++k) {
        const double fc = floor((px[k] - sg.x0) / sg.sx), fr = floor((sg.y0 - py[k]) / sg.sy);
        int o = -1;
        if (fc >= 0.0 && fc < (double)W && fr >= 0.0 && fr < (double)H) o = (int)fr * W + (int)fc;
        off[k] = o;
    }
    return (long)H * W;
}

template <typename L>  // signed char, float, or void (no labels)
__global__ __launch_bounds__(QTPB, 2) void s2_chip_warp_kernel(const unsigned short* __restrict__ bands, const long long* __restrict__ starts,
                                                            const unsigned char* __restrict__ scl, const long long* __restrict__ scl_starts,
                                                            const int* __restrict__ plane_class, const double* __restrict__ class_grid,
                                                            const int* __restrict__ class_size, const double* __restrict__ src_crs,
                                                            const double* __restrict__ dst_crs, const double* __restrict__ dst_grids,
                                                            S2WarpArgs a, const void* __restrict__ labels_v,
                                                            unsigned short* __restrict__ chips, int* __restrict__ valid_values,
                                                            unsigned char* __restrict__ validity, void* __restrict__ maps_v,
                                                            int* __restrict__ valid_labels, int* __restrict__ hist) {
    __shared__ int part[4];
    __shared__ int cells[EPI_MAX_K];
    constexpr bool LABELS = !__is_same(L, void);
    const int per = a.nb * a.nb;
    const int chip = blockIdx.x / per, blk = blockIdx.x - chip * per;
    const int br = (blk / a.nb) * QB, c = (blk % a.nb) * QB + (threadIdx.x & 63);
    const int wave = threadIdx.x >> 6;
    if constexpr (LABELS) {
        for (int i = threadIdx.x; i < EPI_MAX_K; i += QTPB) cells[i] = 0;
        __syncthreads();
    }
    const bool col_live = c < a.S;
    const long cplane = (long)a.S * a.S;
    const int TC = a.T * a.C;
    const double nan = __builtin_nan("");

    // phase 1: source map coordinates
    double px[QROWS], py[QROWS];
    {
        const Crs dc = load_crs(dst_crs), sc = load_crs(src_crs);
        const Grid dg = load_grid(dst_grids + 4 * (long)chip);
        bool grids = grid_ok(dg);
        for (int g = 0; g < a.G; ++g) grids = grids && grid_ok(load_grid(class_grid + 4 * g));
        const bool affine = same_crs(dc, sc);
#pragma unroll
        for (int k = 0; k < QROWS; ++k) {
            const int r = br + 4 * k + wave;
            double x = nan, y = nan;
            if (grids && col_live && r < a.S) {
                x = dg.x0 + (c + 0.5) * dg.sx, y = dg.y0 - (r + 0.5) * dg.sy;
                bool ok = true;
                if (!affine) {
                    double lon, lat;
                    ok = to_lonlat(dc, x, y, lon, lat) && from_lonlat(sc, lon, lat, x, y);
                }
                if (!ok) x = nan, y = nan;
            }
            px[k] = x, py[k] = y;
        }
    }

    // phase 2: the date masks (bit t: date t is masked at pixel k).  A pixel outside the plane, and every pixel of a plane whose table
    // entry is unusable, has SCL class 0.
    int off[QROWS];
    unsigned dm[QROWS];
#pragma unroll
    for (int k = 0; k < QROWS; ++k) dm[k] = 0u;
    if (scl && a.class_bits) {
        for (int g = -1; g < a.G; ++g) {  // -1: the planes that read nothing
            bool any_plane = false;
            for (int t = 0; t < a.T; ++t) {
                const int pc = plane_class[TC + t];
                const int mine = (pc < 0 || pc >= a.G || scl_starts[t] < 0) ? -1 : pc;
                any_plane = any_plane || mine == g;
            }
            if (!any_plane) continue;
            long size = 0;
            if (g >= 0) size = class_offsets(class_grid, class_size, g, px, py, off);
            for (int t = 0; t < a.T; ++t) {
                const int pc = plane_class[TC + t];
                const long long at = scl_starts[t];
                const int mine = (pc < 0 || pc >= a.G || at < 0) ? -1 : pc;
                if (mine != g) continue;
                const unsigned char* p = scl + at;
#pragma unroll
                for (int k = 0; k < QROWS; ++k) {
                    unsigned f = 0u;
                    if (size > 0 && off[k] >= 0) f = p[off[k]];
                    dm[k] |= (f < 32u && (a.class_bits >> f & 1u)) ? 1u << t : 0u;
                }
            }
        }
        if (a.any) {
#pragma unroll
            for (int k = 0; k < QROWS; ++k) dm[k] = dm[k] ? 0xffffffffu : 0u;
        }
    }

    // phase 3: the bands, class by class
    unsigned live = 0u;  // bit k: pixel k exists
#pragma unroll
    for (int k = 0; k < QROWS; ++k) live |= (col_live && br + 4 * k + wave < a.S) ? 1u << k : 0u;
    unsigned all = live, some = 0u;
    int count = 0;
    const long at0 = (long)(br + wave) * a.S + c;  // pixel k lies 4 k rows further down
    unsigned short* const q0 = chips + (long)chip * TC * cplane + at0;
    for (int g = -1; g < a.G; ++g) {  // -1: the planes that read nothing
        bool any_plane = false;
        for (int b = 0; b < TC; ++b) {
            const int pc = plane_class[b];
            const int mine = (pc < 0 || pc >= a.G || starts[b] < 0) ? -1 : pc;
            any_plane = any_plane || mine == g;
        }
        if (!any_plane) continue;
        long size = 0;
        if (g >= 0) size = class_offsets(class_grid, class_size, g, px, py, off);
        for (int b = 0; b < TC; ++b) {
            const int pc = plane_class[b];
            const long long at = starts[b];
            const int mine = (pc < 0 || pc >= a.G || at < 0) ? -1 : pc;
            if (mine != g) continue;
            const unsigned short* p = bands + at;
            unsigned short* q = q0 + b * cplane;
            const int t = b / a.C;
            unsigned ok = 0u;
#pragma unroll
            for (int k = 0; k < QROWS; ++k) {
                if (!(live >> k & 1u)) continue;
                int x = a.no_data;
                if (size > 0 && off[k] >= 0) {
                    x = p[off[k]];
                    if (a.boa > 0 && x != 0) x = max(x - a.boa, 0);
                    if (dm[k] >> t & 1u) x = a.no_data;
                    if (a.range && (x < a.lo || x > a.hi)) x = a.no_data;
                }
                ok |= x != a.no_data ? 1u << k : 0u;
                q[(long)(4 * k) * a.S] = (unsigned short)x;
            }
            all &= ok, some |= ok;
            count += __popc(ok);
        }
    }

    // phase 4: validity and labels
    chip_epilogue<L, QROWS, QTPB>(live, all, some, count, chip, cplane, at0, a.S, a.valid_bit, a.K, labels_v, valid_values, validity, maps_v,
                                  valid_labels, hist, part, cells);
}

}  // namespace

extern "C" int ig_s2_chip_warp(const unsigned short* bands, const long long* starts, const unsigned char* scl, const long long* scl_starts,
                               const int* plane_class, const double* class_grid, const int* class_size, int G, const double* src_crs,
                               const double* dst_crs, const double* dst_grids, int n, int T, int C, int S, unsigned class_bits, int strategy,
                               int no_data, int boa_offset, int range, int range_lo, int range_hi, const void* labels, int elem_size,
                               int valid_bit, int K, unsigned short* chips, int* valid_values, unsigned char* validity, void* maps,
                               int* valid_labels, int* hist, void* stream) {
    CHIP_CHECK(chip_check_stack("ig_s2_chip_warp", n, T, C));
    CHIP_CHECK(chip_check_side("ig_s2_chip_warp", S));
    IG_REQUIRE(G >= 1 && G <= QMAX_G, "ig_s2_chip_warp: 1 <= G <= %d geometry classes (got %d)", QMAX_G, G);
    CHIP_CHECK(chip_check_s2_rule("ig_s2_chip_warp", strategy, no_data, boa_offset, range, range_lo, range_hi));
    CHIP_CHECK(chip_check_labels("ig_s2_chip_warp", elem_size, valid_bit, K));
    const long TC = (long)T * C;
    IG_REQUIRE(TC <= 0x7fffffffL - CHIP_MAX_T, "ig_s2_chip_warp: T * C = %ld planes are too many for the int32 class table", TC);
    CHIP_CHECK(chip_check_values("ig_s2_chip_warp", TC, S));
    if (n == 0) return IG_OK;
    const int nb = ig_cdiv(S, QB);
    CHIP_CHECK(chip_check_launch("ig_s2_chip_warp", n, TC, S, (long)nb * nb));
    IG_REQUIRE(bands && starts && plane_class && class_grid && class_size && src_crs && dst_crs && dst_grids && chips && valid_values,
               "ig_s2_chip_warp: null pointer");
    IG_REQUIRE(!scl || scl_starts, "ig_s2_chip_warp: null pointer (scl_starts goes with scl)");
    IG_REQUIRE(!labels || (maps && valid_labels), "ig_s2_chip_warp: null pointer (maps, valid_labels)");
    IG_REQUIRE(K == 0 || (labels && hist), "ig_s2_chip_warp: null pointer (labels, hist): a class histogram needs both");
    IG_REQUIRE((((uintptr_t)class_grid | (uintptr_t)src_crs | (uintptr_t)dst_crs | (uintptr_t)dst_grids | (uintptr_t)starts | (uintptr_t)scl_starts) & 7) == 0,
               "ig_s2_chip_warp: the float64 arrays, starts and scl_starts must be 8-byte aligned");
    IG_REQUIRE((((uintptr_t)bands | (uintptr_t)chips) & 1) == 0 &&
                   (((uintptr_t)plane_class | (uintptr_t)class_size | (uintptr_t)valid_values | (uintptr_t)valid_labels | (uintptr_t)hist) & 3) == 0 &&
                   (((uintptr_t)labels | (uintptr_t)maps) & (elem_size - 1)) == 0,
               "ig_s2_chip_warp: bands and chips must be 2-byte, plane_class, class_size, valid_values, valid_labels and hist 4-byte aligned, "
               "labels and maps to their elements");
    const S2WarpArgs a{T, C, S, G, strategy, no_data, boa_offset, range, range_lo, range_hi, nb, labels ? valid_bit : 0, K, scl ? class_bits : 0u};
    const dim3 grid((unsigned)((long)nb * nb * n));
#define S2_CHIP_WARP(L)                                                                                                                       \
    return ig_launch<s2_chip_warp_kernel<L>>("ig_s2_chip_warp", grid, dim3(QTPB), 0, (hipStream_t)stream, bands, starts, scl, scl_starts,     \
                                             plane_class, class_grid, class_size, src_crs, dst_crs, dst_grids, a, labels, chips,              \
                                             valid_values, validity, maps, valid_labels, K ? hist : nullptr)
    if (!labels) S2_CHIP_WARP(void);
    if (elem_size == 1) S2_CHIP_WARP(signed char);
    S2_CHIP_WARP(float);
#undef S2_CHIP_WARP
}
