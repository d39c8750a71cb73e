// Sentinel-1 chips warped onto label grids, for gfx950.  The reference has no label-raster pipeline for Sentinel-1; the
// rule, stated in include/instageo_hip.h, joins the sources and the value rule of ig_s1_chip_cut (s1_chips.hip: float32 RTC scenes
// stacked per date, each on its own grid in its own coordinate system, first present slice) with the destination and the label maps of
// ig_chip_warp (raster_chips.hip: one grid per chip in one coordinate system, label pixels masked by the chip's validity).  A GATHER:
// every output element is written once by the thread that computed it; the tallies are integer atomics, one set per workgroup; results
// are unique (independent of scheduling).
//
//   s1_chip_warp_kernel<L>   the blocking of chip_warp_kernel: one workgroup of 256 threads per 64 x 64 block of one chip, a wave owns 64
//                            consecutive float32 of a row (256 B per store instruction), a thread 16 rows of one column, which it takes
//                            WG = 4 at a time, as s1_chip_cut_kernel does and for its reason (the inlined projection alone takes about
//                            240 registers; the kernel is capped to two waves per SIMD).  For each group of rows.  Phase 1, only when
//                            some scene lives in another coordinate system than the chips (the common case here: label grids in
//                            EPSG:4326 or 3857): the inverse projection of dst_crs once per pixel -> (lon, lat) in registers (NaN: none).
//                            Phase 2, date by date and slice by slice in list order: the slice's source offsets rs * W_s + cs (-1:
//                            none), then the C bands stream through: gather, presence test, clip, count, one store, under the 32-bit
//                            PENDING mask per pixel of s1_chip_cut_kernel (a present value is stored at once, the date's last slice
//                            stores what is still pending, a slice is neither projected nor read for a pixel with nothing pending).
//                            After the groups, phase 3: the validity byte, the label pixel (L = signed char | float; void: no labels)
//                            and the tallies (chip_epilogue.h); the histogram cells are in LDS, zeroed before the first barrier.
//
// Out-of-range accesses are impossible: a source offset is formed only after 0 <= floor(v) < H_s and 0 <= floor(u) < W_s held on the
// float64 values (NaN fails) for a scene with 1 <= H_s, W_s and H_s * W_s <= 2^31 - 1; a plane whose start is negative is never addressed;
// a grid (the chip's or the scene's) that is not finite and positive yields no offsets at all; every store and every label load is
// guarded by row < S and column < S of a chip index below n.  The caller guarantees that starts[k] + H_s * W_s lies inside the buffer.
#include "chip_kernels.h"
#include "common.h"
#include "warp_proj.h"

namespace {

constexpr int WB = 64, WTPB = 256, WROWS = WB / 4, WG = 4;  // block side, threads, rows per thread, rows in flight at a time
constexpr int WMAX_N = 32;

struct S1WarpArgs {
    int T, C, N, S, nb, has_nodata, clip, valid_bit, K;
    unsigned first_bits;
    float no_data, src_nodata, lo, hi;
};

// values travel as their 32 bits (copied, never re-encoded); the float view is for the comparisons only
template <typename L>  // signed char, float, or void (no labels)
__global__ __launch_bounds__(WTPB, 2) void s1_chip_warp_kernel(const unsigned* __restrict__ planes, const long long* __restrict__ starts,
                                                            const double* __restrict__ scene_crs, const double* __restrict__ scene_grid,
                                                            const int* __restrict__ scene_size, const double* __restrict__ dst_crs,
                                                            const double* __restrict__ dst_grids, S1WarpArgs a,
                                                            const void* __restrict__ labels_v, unsigned* __restrict__ chips,
                                                            int* __restrict__ valid_values, unsigned char* __restrict__ validity,
                                                            void* __restrict__ maps_v, int* __restrict__ valid_labels,
                                                            int* __restrict__ hist) {
    __shared__ int part[4];
    __shared__ int cells[EPI_MAX_K];
    constexpr bool LABELS = !__is_same(L, void);
    const int per = a.nb * a.nb;
    const int chip = blockIdx.x / per, blk = blockIdx.x - chip * per;
    const int br = (blk / a.nb) * WB, c = (blk % a.nb) * WB + (threadIdx.x & 63);
    const int wave = threadIdx.x >> 6;
    if constexpr (LABELS) {
        for (int i = threadIdx.x; i < EPI_MAX_K; i += WTPB) cells[i] = 0;
        __syncthreads();
    }
    const bool col_live = c < a.S;
    const long cplane = (long)a.S * a.S;
    const double nan = __builtin_nan("");
    const Crs dc = load_crs(dst_crs);
    const Grid dg = load_grid(dst_grids + 4 * (long)chip);
    const bool dgrid = grid_ok(dg);
    const double x = dg.x0 + (c + 0.5) * dg.sx;  // the pixel centres of the thread's column and of row r, on the chip's map
#define S1W_Y(r) (dg.y0 - ((r) + 0.5) * dg.sy)
    unsigned live = 0u;  // bit k: pixel k exists
#pragma unroll
    for (int k = 0; k < WROWS; ++k) live |= (col_live && br + 4 * k + wave < a.S) ? 1u << k : 0u;
    bool other = false;  // some scene lives in another system than the chips
    for (int s = 0; s < a.N; ++s) other = other || !same_crs(dc, load_crs(scene_crs + 5 * s));

    unsigned all = live, some = 0u;
    int count = 0;
    const unsigned nd_bits = __float_as_uint(a.no_data), lo_bits = __float_as_uint(a.lo), hi_bits = __float_as_uint(a.hi);
    const long at0 = (long)(br + wave) * a.S + c;  // pixel k lies 4 k rows further down
    unsigned* const q0 = chips + (long)chip * a.T * a.C * cplane + at0;
#pragma unroll 1
    for (int g = 0; g < WROWS; g += WG) {  // the thread's pixels g .. g + WG - 1
        if (!(live >> g & ((1u << WG) - 1u))) continue;
        // phase 1: longitude and latitude, once per pixel, when a scene needs them
        double lon[WG], lat[WG];
#pragma unroll
        for (int i = 0; i < WG; ++i) {
            double lo = nan, la = nan;
            if (other && dgrid && (live >> (g + i) & 1u)) {
                if (!to_lonlat(dc, x, S1W_Y(br + 4 * (g + i) + wave), lo, la)) lo = nan, la = nan;
            }
            lon[i] = lo, lat[i] = la;
        }
        // phase 2: the dates, slice by slice
        int s = 0;
        for (int t = 0; t < a.T; ++t) {
            int e = s + 1;  // the scenes of date t: s .. e - 1
            while (e < a.N && !(a.first_bits >> e & 1u)) ++e;
            for (int cb = 0; cb < a.C; cb += 32) {
                const int cn = min(32, a.C - cb);
                unsigned pend[WG];  // bit b: band cb + b of the pixel has no value yet
#pragma unroll
                for (int i = 0; i < WG; ++i) pend[i] = (live >> (g + i) & 1u) ? 0xffffffffu >> (32 - cn) : 0u;
                for (int j = s; j < e; ++j) {
                    const bool last = j == e - 1;
                    unsigned need = 0u;
#pragma unroll
                    for (int i = 0; i < WG; ++i) need |= pend[i];
                    if (!need) break;
                    // the slice's source offsets of the pixels that still need it
                    const Crs sc = load_crs(scene_crs + 5 * j);
                    const Grid sg = load_grid(scene_grid + 4 * j);
                    const int H = scene_size[2 * j], W = scene_size[2 * j + 1];
                    const bool usable = dgrid && grid_ok(sg) && H >= 1 && W >= 1 && (long)H * W <= 0x7fffffffL;
                    const bool affine = same_crs(dc, sc);
                    int off[WG];
#pragma unroll
                    for (int i = 0; i < WG; ++i) {
                        int o = -1;
                        if (usable && pend[i]) {
                            double xs = x, ys = S1W_Y(br + 4 * (g + i) + wave);
                            bool ok = true;
                            if (!affine) ok = lon[i] == lon[i] && from_lonlat(sc, lon[i], lat[i], xs, ys);
                            if (ok) {
                                const double fc = floor((xs - sg.x0) / sg.sx), fr = floor((sg.y0 - ys) / sg.sy);
                                if (fc >= 0.0 && fc < (double)W && fr >= 0.0 && fr < (double)H) o = (int)fr * W + (int)fc;
                            }
                        }
                        off[i] = o;
                    }
                    for (int b = 0; b < cn; ++b) {
                        const long long at = starts[(long)j * a.C + cb + b];
                        const bool readable = usable && at >= 0;
                        const unsigned* p = planes + (readable ? at : 0);
                        unsigned* q = q0 + ((long)t * a.C + cb + b) * cplane + (long)(4 * g) * a.S;
#pragma unroll
                        for (int i = 0; i < WG; ++i) {
                            if (!(pend[i] >> b & 1u)) continue;
                            unsigned bits = nd_bits;
                            bool present = false;
                            if (readable && off[i] >= 0) {
                                bits = p[off[i]];
                                const float v = __uint_as_float(bits);
                                present = v == v && !(a.has_nodata && v == a.src_nodata);
                            }
                            if (!present && !last) continue;  // a later slice may have it
                            float v = __uint_as_float(bits);
                            if (!present) {
                                bits = nd_bits, v = a.no_data;
                            } else if (a.clip) {
                                if (v < a.lo) bits = lo_bits, v = a.lo;
                                if (v > a.hi) bits = hi_bits, v = a.hi;
                            }
                            q[(long)(4 * i) * a.S] = bits;
                            pend[i] &= ~(1u << b);
                            if (v != a.no_data) {
                                some |= 1u << (g + i);
                                ++count;
                            } else {
                                all &= ~(1u << (g + i));
                            }
                        }
                    }
                }
            }
            s = e;
        }
    }
#undef S1W_Y

    // phase 3: validity, labels and the tallies
    chip_epilogue<L, WROWS, WTPB>(live, all, some, count, chip, cplane, at0, a.S, a.valid_bit, a.K, labels_v, valid_values, validity, maps_v,
                                  valid_labels, hist, part, cells);
}

}  // namespace

extern "C" int ig_s1_chip_warp(const float* planes, const long long* starts, const double* scene_crs, const double* scene_grid,
                               const int* scene_size, int N, unsigned first_bits, const double* dst_crs, const double* dst_grids, int n, int T,
                               int C, int S, float no_data, int has_src_nodata, float src_nodata, int clip, float clip_lo, float clip_hi,
                               const void* labels, int elem_size, int valid_bit, int K, float* chips, int* valid_values,
                               unsigned char* validity, void* maps, int* valid_labels, int* hist, void* stream) {
    CHIP_CHECK(chip_check_stack("ig_s1_chip_warp", n, T, C));
    IG_REQUIRE(N >= 1 && N <= WMAX_N, "ig_s1_chip_warp: 1 <= N <= %d scenes in all (got %d)", WMAX_N, N);
    IG_REQUIRE((first_bits & 1u) && __builtin_popcount(first_bits) == T && (N == 32 || (first_bits >> N) == 0u),
               "ig_s1_chip_warp: every date needs at least one scene: first_bits 0x%x must mark the first scene of each of the %d dates among "
               "%d scenes (bit 0, T bits in all, none at or above N)",
               first_bits, T, N);
    CHIP_CHECK(chip_check_side("ig_s1_chip_warp", S));
    IG_REQUIRE(no_data == no_data, "ig_s1_chip_warp: no_data must not be NaN (a NaN equals nothing, itself included)");
    IG_REQUIRE(has_src_nodata == 0 || has_src_nodata == 1, "ig_s1_chip_warp: has_src_nodata must be 0 or 1 (got %d)", has_src_nodata);
    IG_REQUIRE(!has_src_nodata || src_nodata == src_nodata, "ig_s1_chip_warp: src_nodata must not be NaN (a NaN is absent anyway)");
    IG_REQUIRE(clip == 0 || clip == 1, "ig_s1_chip_warp: clip must be 0 or 1 (got %d)", clip);
    IG_REQUIRE(!clip || clip_lo <= clip_hi, "ig_s1_chip_warp: the clip range needs clip_lo <= clip_hi, neither NaN (got %g, %g)",
               (double)clip_lo, (double)clip_hi);
    CHIP_CHECK(chip_check_labels("ig_s1_chip_warp", elem_size, valid_bit, K));
    const long TC = (long)T * C;
    CHIP_CHECK(chip_check_values("ig_s1_chip_warp", TC, S));
    if (n == 0) return IG_OK;
    const int nb = ig_cdiv(S, WB);
    CHIP_CHECK(chip_check_launch("ig_s1_chip_warp", n, TC, S, (long)nb * nb));
    IG_REQUIRE(planes && starts && scene_crs && scene_grid && scene_size && dst_crs && dst_grids && chips && valid_values,
               "ig_s1_chip_warp: null pointer");
    IG_REQUIRE(!labels || (maps && valid_labels), "ig_s1_chip_warp: null pointer (maps, valid_labels)");
    IG_REQUIRE(K == 0 || (labels && hist), "ig_s1_chip_warp: null pointer (labels, hist): a class histogram needs both");
    IG_REQUIRE((((uintptr_t)starts | (uintptr_t)scene_crs | (uintptr_t)scene_grid | (uintptr_t)dst_crs | (uintptr_t)dst_grids) & 7) == 0,
               "ig_s1_chip_warp: starts and the float64 arrays must be 8-byte aligned");
    IG_REQUIRE((((uintptr_t)planes | (uintptr_t)chips | (uintptr_t)scene_size | (uintptr_t)valid_values | (uintptr_t)valid_labels |
                 (uintptr_t)hist) & 3) == 0 && (((uintptr_t)labels | (uintptr_t)maps) & (elem_size - 1)) == 0,
               "ig_s1_chip_warp: planes, chips, scene_size, valid_values, valid_labels and hist must be 4-byte aligned, labels and maps to "
               "their elements");
    const S1WarpArgs a{T, C, N, S, nb, has_src_nodata, clip, labels ? valid_bit : 0, K, first_bits, no_data, src_nodata, clip_lo, clip_hi};
    const dim3 grid((unsigned)((long)nb * nb * n));
#define S1_CHIP_WARP(L)                                                                                                                   \
    return ig_launch<s1_chip_warp_kernel<L>>("ig_s1_chip_warp", grid, dim3(WTPB), 0, (hipStream_t)stream,                                 \
                                             reinterpret_cast<const unsigned*>(planes), starts, scene_crs, scene_grid, scene_size, dst_crs, \
                                             dst_grids, a, labels, reinterpret_cast<unsigned*>(chips), valid_values, validity, maps,      \
                                             valid_labels, K ? hist : nullptr)
    if (!labels) S1_CHIP_WARP(void);
    if (elem_size == 1) S1_CHIP_WARP(signed char);
    S1_CHIP_WARP(float);
#undef S1_CHIP_WARP
}
