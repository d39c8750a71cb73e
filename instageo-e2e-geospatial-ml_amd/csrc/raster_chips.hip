// Chips warped onto label grids for gfx950.  The reference's label-raster chip creator (instageo/data/
// raster_chip_creator.py, HLSRasterPipeline.process_row) lets stackstac resample the granule stack onto the label's coordinate system and
// resolution and cuts, masks and quality-checks every label's chip on the host with xarray; here the rule, stated in
// include/instageo_hip.h, is one kernel for all chips of a granule.  A GATHER: every output element is written once by the thread that
// computed it; the tallies are integer atomics, one set per workgroup; results are unique (independent of scheduling).
//
//   chip_warp_kernel<L>   one workgroup of 256 threads per 64 x 64 block of one chip.  A wave owns 64 consecutive pixels of a row, a thread
//                         16 rows of one column.  Phase 1: the float64 chain of warp_proj.h once per pixel -> the source offset
//                         rs * W + cs (int32, -1: outside the tile or the domain) in registers.  Phase 2: the T Fmask bytes of each pixel
//                         -> one 32-bit date mask per pixel.  Phase 3: the T * C bands stream through: gather, mask, clip, one store; the
//                         all / some bits of the validity plane and the count of valid values accumulate.  Phase 4: the validity byte and
//                         the label pixel (L = signed char | float; void: no labels) from the same registers (chip_epilogue.h, shared
//                         with s2_raster_chips.hip).
//
// Out-of-range accesses are impossible: a source offset is formed only after 0 <= floor(v) < H and 0 <= floor(u) < W held on the float64
// values (NaN fails), H * W <= 2^31 - 1 is checked by the entry point, a grid that is not finite and positive yields no offset at all, and
// every store and every label load is guarded by row < S and column < S of a chip index below n.
#include "chip_kernels.h"
#include "common.h"
#include "warp_proj.h"

namespace {

constexpr int RB = 64, RTPB = 256, RROWS = RB / 4;  // block side, threads, rows per thread
constexpr int RMAX_K = EPI_MAX_K;

struct WarpCutArgs {
    int T, C, H, W, S, mask_bits, any, no_data, clip, lo, hi, nb, valid_bit, K;
};

template <typename L>  // signed char, float, or void (no labels)
__global__ __launch_bounds__(RTPB) void chip_warp_kernel(const short* __restrict__ tile, const unsigned char* __restrict__ fmask,
                                                         const double* __restrict__ src_crs, const double* __restrict__ src_grid,
                                                         const double* __restrict__ dst_crs, const double* __restrict__ dst_grids,
                                                         WarpCutArgs a, const void* __restrict__ labels_v, short* __restrict__ chips,
                                                         int* __restrict__ valid_values, unsigned char* __restrict__ validity,
                                                         void* __restrict__ maps_v, int* __restrict__ valid_labels, int* __restrict__ hist) {
    __shared__ int part[4];
    __shared__ int cells[RMAX_K];
    constexpr bool LABELS = !__is_same(L, void);
    const int per = a.nb * a.nb;
    const int chip = blockIdx.x / per, blk = blockIdx.x - chip * per;
    const int br = (blk / a.nb) * RB, c = (blk % a.nb) * RB + (threadIdx.x & 63);
    const int wave = threadIdx.x >> 6;
    if constexpr (LABELS) {
        for (int i = threadIdx.x; i < RMAX_K; i += RTPB) cells[i] = 0;
        __syncthreads();
    }
    const bool col_live = c < a.S;
    const long cplane = (long)a.S * a.S, plane = (long)a.H * a.W;

    // phase 1: source offsets
    int off[RROWS];
    {
        const Crs dc = load_crs(dst_crs), sc = load_crs(src_crs);
        const Grid dg = load_grid(dst_grids + 4 * (long)chip), sg = load_grid(src_grid);
        const bool grids = grid_ok(dg) && grid_ok(sg);
        const bool affine = same_crs(dc, sc);
#pragma unroll
        for (int k = 0; k < RROWS; ++k) {
            const int r = br + 4 * k + wave;
            int o = -1;
            if (grids && col_live && r < a.S) {
                double x = dg.x0 + (c + 0.5) * dg.sx, y = dg.y0 - (r + 0.5) * dg.sy;
                bool ok = true;
                if (!affine) {
                    double lon, lat;
                    ok = to_lonlat(dc, x, y, lon, lat) && from_lonlat(sc, lon, lat, x, y);
                }
                if (ok) {
                    const double fc = floor((x - sg.x0) / sg.sx), fr = floor((sg.y0 - y) / sg.sy);
                    if (fc >= 0.0 && fc < (double)a.W && fr >= 0.0 && fr < (double)a.H) o = (int)fr * a.W + (int)fc;
                }
            }
            off[k] = o;
        }
    }

    // phase 2: the date masks (bit t: date t is masked at pixel k)
    unsigned dm[RROWS];
#pragma unroll
    for (int k = 0; k < RROWS; ++k) dm[k] = 0u;
    if (fmask && a.mask_bits) {
        for (int t = 0; t < a.T; ++t) {
            const unsigned char* p = fmask + t * plane;
#pragma unroll
            for (int k = 0; k < RROWS; ++k)
                if (off[k] >= 0) dm[k] |= (p[off[k]] & a.mask_bits) ? 1u << t : 0u;
        }
        if (a.any) {
#pragma unroll
            for (int k = 0; k < RROWS; ++k) dm[k] = dm[k] ? 0xffffffffu : 0u;
        }
    }

    // phase 3: the bands
    unsigned live = 0u;  // bit k: pixel k exists
#pragma unroll
    for (int k = 0; k < RROWS; ++k) live |= (col_live && br + 4 * k + wave < a.S) ? 1u << k : 0u;
    unsigned all = live, some = 0u;
    int count = 0;
    const short nd = (short)a.no_data, lo = (short)a.lo, hi = (short)a.hi;
    const long at0 = (long)(br + wave) * a.S + c;  // pixel k lies 4 k rows further down
    {
        short* q = chips + (long)chip * a.T * a.C * cplane + at0;
        const short* p = tile;
        int t = 0, cc = 0;
        for (int b = 0; b < a.T * a.C; ++b) {
            unsigned ok = 0u;
#pragma unroll
            for (int k = 0; k < RROWS; ++k) {
                if (!(live >> k & 1u)) continue;
                short x = off[k] >= 0 ? p[off[k]] : nd;
                if (dm[k] >> t & 1u) x = nd;
                if (a.clip) x = x < lo ? lo : x > hi ? hi : x;
                ok |= x != nd ? 1u << k : 0u;
                q[(long)(4 * k) * a.S] = x;
            }
            all &= ok, some |= ok;
            count += __popc(ok);
            p += plane, q += cplane;
            if (++cc == a.C) cc = 0, ++t;
        }
    }

    // phase 4: validity and labels
    chip_epilogue<L, RROWS, RTPB>(live, all, some, count, chip, cplane, at0, a.S, a.valid_bit, a.K, labels_v, valid_values, validity, maps_v,
                                  valid_labels, hist, part, cells);
}

}  // namespace

extern "C" int ig_chip_warp(const short* tile, const unsigned char* fmask, const double* src_crs, const double* src_grid,
                            const double* dst_crs, const double* dst_grids, int n, int T, int C, int H, int W, int S, int mask_bits,
                            int strategy, int no_data, int clip, int clip_lo, int clip_hi, const void* labels, int elem_size, int valid_bit,
                            int K, short* chips, int* valid_values, unsigned char* validity, void* maps, int* valid_labels, int* hist,
                            void* stream) {
    CHIP_CHECK(chip_check_stack("ig_chip_warp", n, T, C));
    IG_REQUIRE(H >= 1 && W >= 1, "ig_chip_warp: need H >= 1 and W >= 1 (H %d, W %d)", H, W);
    IG_REQUIRE((long)H * W <= 0x7fffffffL, "ig_chip_warp: H * W = %ld exceeds 2^31 - 1 (source offsets are int32)", (long)H * W);
    CHIP_CHECK(chip_check_side("ig_chip_warp", S));
    CHIP_CHECK(chip_check_hls_rule("ig_chip_warp", mask_bits, strategy, no_data, clip, clip_lo, clip_hi));
    CHIP_CHECK(chip_check_labels("ig_chip_warp", elem_size, valid_bit, K));
    const long TC = (long)T * C;
    CHIP_CHECK(chip_check_values("ig_chip_warp", TC, S));
    if (n == 0) return IG_OK;
    const int nb = ig_cdiv(S, RB);
    CHIP_CHECK(chip_check_launch("ig_chip_warp", n, TC, S, (long)nb * nb));
    IG_REQUIRE(tile && src_crs && src_grid && dst_crs && dst_grids && chips && valid_values, "ig_chip_warp: null pointer");
    IG_REQUIRE(!labels || (maps && valid_labels), "ig_chip_warp: null pointer (maps, valid_labels)");
    IG_REQUIRE(K == 0 || (labels && hist), "ig_chip_warp: null pointer (labels, hist): a class histogram needs both");
    IG_REQUIRE((((uintptr_t)src_crs | (uintptr_t)src_grid | (uintptr_t)dst_crs | (uintptr_t)dst_grids) & 7) == 0,
               "ig_chip_warp: the float64 arrays must be 8-byte aligned");
    IG_REQUIRE((((uintptr_t)tile | (uintptr_t)chips) & 1) == 0 && (((uintptr_t)valid_values | (uintptr_t)valid_labels | (uintptr_t)hist) & 3) == 0 &&
                   (((uintptr_t)labels | (uintptr_t)maps) & (elem_size - 1)) == 0,
               "ig_chip_warp: tile and chips must be 2-byte, valid_values, valid_labels and hist 4-byte aligned, labels and maps to their elements");
    const WarpCutArgs a{T, C, H, W, S, fmask ? mask_bits : 0, strategy, no_data, clip, clip_lo, clip_hi, nb, labels ? valid_bit : 0, K};
    const dim3 grid((unsigned)((long)nb * nb * n));
#define CHIP_WARP(L)                                                                                                                    \
    return ig_launch<chip_warp_kernel<L>>("ig_chip_warp", grid, dim3(RTPB), 0, (hipStream_t)stream, tile, fmask, src_crs, src_grid,     \
                                          dst_crs, dst_grids, a, labels, chips, valid_values, validity, maps, valid_labels,             \
                                          K ? hist : nullptr)
    if (!labels) CHIP_WARP(void);
    if (elem_size == 1) CHIP_WARP(signed char);
    CHIP_WARP(float);
#undef CHIP_WARP
}
