// Sentinel-1 chips cut from float32 RTC scenes stacked per date, for gfx950.  The reference's Sentinel-1 point pipeline
// (instageo/data/s1_utils.py, S1PointsPipeline) lets stackstac resample every scene of every date (nearest, fill_value -1) onto one lattice
// that spans the union of their bounds, on the host, and cuts and quality-checks with xarray; here the rule, stated in
// include/instageo_hip.h, is one kernel for all chips of a stack that reads every scene on its own grid, in its own coordinate system.
// A GATHER: every output element is written once by the thread that computed it; the tallies are integer atomics, one set per workgroup;
// results are unique (independent of scheduling).
//
//   s1_chip_cut_kernel   the blocking of chip_warp_kernel (raster_chips.hip): one workgroup of 256 threads per 64 x 64 block of one chip, a
//                        wave owns 64 consecutive float32 of a row (256 B per store instruction), a thread 16 rows of one column, which
//                        it takes VG = 4 at a time.  For each group of rows.  Phase 1, only when some scene lives in another coordinate
//                        system than the stack: the inverse projection of dst_crs once per pixel -> (lon, lat) in registers (NaN:
//                        none).  Phase 2, date by date and, within a date, slice by slice in list order: the slice's source offsets
//                        rs * W_s + cs (-1: none; the affine arithmetic alone, or the forward projection of the slice's system from
//                        (lon, lat)), then the C bands stream through: gather, presence test, clip, count, one store.  A 32-bit mask per
//                        pixel (one bit per band; C > 32 goes in groups of 32 bands) marks the values still PENDING: a value found
//                        present is stored and its bit cleared, the date's last slice stores every value still pending (the fill where
//                        it is not present either), and a slice is not even projected for a pixel with nothing pending.  With one slice
//                        per date, the common case, every store is a whole row segment of the wave.  The offsets of one slice at a
//                        time, and four rows at a time: the inlined projection alone takes about 240 registers, so the kernel is capped
//                        to two waves per SIMD (256 VGPRs, 22 spilled; 16 rows at a time spilled 80).  After the groups, phase 3: the
//                        validity byte from the two per-pixel flags kept across the dates, and the tally (chip_epilogue.h without
//                        labels).
//
// Out-of-range accesses are impossible: a source offset is formed only after 0 <= floor(v) < H_s and 0 <= floor(u) < W_s held on the
// float64 values (NaN fails) for a scene with 1 <= H_s, W_s and H_s * W_s <= 2^31 - 1; a plane whose start is negative is never addressed;
// a grid (the stack's or the scene's) that is not finite and positive yields no offsets at all; every store is guarded by row < S and
// column < S of a chip index below n.  The caller guarantees that starts[k] + H_s * W_s lies inside the buffer.
#include "chip_kernels.h"
#include "common.h"
#include "warp_proj.h"

namespace {

constexpr int VB = 64, VTPB = 256, VROWS = VB / 4, VG = 4;  // block side, threads, rows per thread, rows in flight at a time
constexpr int VMAX_N = 32;

struct S1CutArgs {
    int T, C, N, S, nb, has_nodata, clip;
    unsigned first_bits;
    float no_data, src_nodata, lo, hi;
};

// values travel as their 32 bits (copied, never re-encoded); the float view is for the comparisons only
__global__ __launch_bounds__(VTPB, 2) void s1_chip_cut_kernel(const unsigned* __restrict__ planes, const long long* __restrict__ starts,
                                                           const double* __restrict__ scene_crs, const double* __restrict__ scene_grid,
                                                           const int* __restrict__ scene_size, const double* __restrict__ dst_crs,
                                                           const double* __restrict__ dst_grid, const int* __restrict__ origins, S1CutArgs a,
                                                           unsigned* __restrict__ chips, int* __restrict__ valid_values,
                                                           unsigned char* __restrict__ validity) {
    __shared__ int part[4];
    const int per = a.nb * a.nb;
    const int chip = blockIdx.x / per, blk = blockIdx.x - chip * per;
    const int br = (blk / a.nb) * VB, c = (blk % a.nb) * VB + (threadIdx.x & 63);
    const int wave = threadIdx.x >> 6;
    const bool col_live = c < a.S;
    const long cplane = (long)a.S * a.S;
    const double nan = __builtin_nan("");
    const Crs dc = load_crs(dst_crs);
    const Grid dg = load_grid(dst_grid);
    const bool dgrid = grid_ok(dg);
    const double row0 = (double)origins[2 * chip], col0 = (double)origins[2 * chip + 1];
    const double x = dg.x0 + (col0 + c + 0.5) * dg.sx;  // the pixel centres of the thread's column and of row r, on the stack's map
#define S1_Y(r) (dg.y0 - (row0 + (r) + 0.5) * dg.sy)
    unsigned live = 0u;  // bit k: pixel k exists
#pragma unroll
    for (int k = 0; k < VROWS; ++k) live |= (col_live && br + 4 * k + wave < a.S) ? 1u << k : 0u;
    bool other = false;  // some scene lives in another system than the stack
    for (int s = 0; s < a.N; ++s) other = other || !same_crs(dc, load_crs(scene_crs + 5 * s));

    unsigned all = live, some = 0u;
    int count = 0;
    const unsigned nd_bits = __float_as_uint(a.no_data), lo_bits = __float_as_uint(a.lo), hi_bits = __float_as_uint(a.hi);
    const long at0 = (long)(br + wave) * a.S + c;  // pixel k lies 4 k rows further down
    unsigned* const q0 = chips + (long)chip * a.T * a.C * cplane + at0;
#pragma unroll 1
    for (int g = 0; g < VROWS; g += VG) {  // the thread's pixels g .. g + VG - 1
        if (!(live >> g & ((1u << VG) - 1u))) continue;
        // phase 1: longitude and latitude, once per pixel, when a scene needs them
        double lon[VG], lat[VG];
#pragma unroll
        for (int i = 0; i < VG; ++i) {
            double lo = nan, la = nan;
            if (other && dgrid && (live >> (g + i) & 1u)) {
                if (!to_lonlat(dc, x, S1_Y(br + 4 * (g + i) + wave), lo, la)) lo = nan, la = nan;
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
                unsigned pend[VG];  // bit b: band cb + b of the pixel has no value yet
#pragma unroll
                for (int i = 0; i < VG; ++i) pend[i] = (live >> (g + i) & 1u) ? 0xffffffffu >> (32 - cn) : 0u;
                for (int j = s; j < e; ++j) {
                    const bool last = j == e - 1;
                    unsigned need = 0u;
#pragma unroll
                    for (int i = 0; i < VG; ++i) need |= pend[i];
                    if (!need) break;
                    // the slice's source offsets of the pixels that still need it
                    const Crs sc = load_crs(scene_crs + 5 * j);
                    const Grid sg = load_grid(scene_grid + 4 * j);
                    const int H = scene_size[2 * j], W = scene_size[2 * j + 1];
                    const bool usable = dgrid && grid_ok(sg) && H >= 1 && W >= 1 && (long)H * W <= 0x7fffffffL;
                    const bool affine = same_crs(dc, sc);
                    int off[VG];
#pragma unroll
                    for (int i = 0; i < VG; ++i) {
                        int o = -1;
                        if (usable && pend[i]) {
                            double xs = x, ys = S1_Y(br + 4 * (g + i) + wave);
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
                        for (int i = 0; i < VG; ++i) {
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
#undef S1_Y

    // phase 3: validity and the tally
    chip_epilogue<void, VROWS, VTPB>(live, all, some, count, chip, cplane, at0, a.S, 0, 0, nullptr, valid_values, validity, nullptr, nullptr,
                                     nullptr, part, nullptr);
}

}  // namespace

extern "C" int ig_s1_chip_cut(const float* planes, const long long* starts, const double* scene_crs, const double* scene_grid,
                              const int* scene_size, int N, unsigned first_bits, const double* dst_crs, const double* dst_grid,
                              const int* origins, int n, int T, int C, int S, float no_data, int has_src_nodata, float src_nodata, int clip,
                              float clip_lo, float clip_hi, float* chips, int* valid_values, unsigned char* validity, void* stream) {
    CHIP_CHECK(chip_check_stack("ig_s1_chip_cut", n, T, C));
    IG_REQUIRE(N >= 1 && N <= VMAX_N, "ig_s1_chip_cut: 1 <= N <= %d scenes in all (got %d)", VMAX_N, N);
    IG_REQUIRE((first_bits & 1u) && __builtin_popcount(first_bits) == T && (N == 32 || (first_bits >> N) == 0u),
               "ig_s1_chip_cut: every date needs at least one scene: first_bits 0x%x must mark the first scene of each of the %d dates among "
               "%d scenes (bit 0, T bits in all, none at or above N)",
               first_bits, T, N);
    CHIP_CHECK(chip_check_side("ig_s1_chip_cut", S));
    IG_REQUIRE(no_data == no_data, "ig_s1_chip_cut: no_data must not be NaN (a NaN equals nothing, itself included)");
    IG_REQUIRE(has_src_nodata == 0 || has_src_nodata == 1, "ig_s1_chip_cut: has_src_nodata must be 0 or 1 (got %d)", has_src_nodata);
    IG_REQUIRE(!has_src_nodata || src_nodata == src_nodata, "ig_s1_chip_cut: src_nodata must not be NaN (a NaN is absent anyway)");
    IG_REQUIRE(clip == 0 || clip == 1, "ig_s1_chip_cut: clip must be 0 or 1 (got %d)", clip);
    IG_REQUIRE(!clip || clip_lo <= clip_hi, "ig_s1_chip_cut: the clip range needs clip_lo <= clip_hi, neither NaN (got %g, %g)", (double)clip_lo,
               (double)clip_hi);
    const long TC = (long)T * C;
    CHIP_CHECK(chip_check_values("ig_s1_chip_cut", TC, S));
    if (n == 0) return IG_OK;
    const int nb = ig_cdiv(S, VB);
    CHIP_CHECK(chip_check_launch("ig_s1_chip_cut", n, TC, S, (long)nb * nb));
    IG_REQUIRE(planes && starts && scene_crs && scene_grid && scene_size && dst_crs && dst_grid && origins && chips && valid_values,
               "ig_s1_chip_cut: null pointer");
    IG_REQUIRE((((uintptr_t)starts | (uintptr_t)scene_crs | (uintptr_t)scene_grid | (uintptr_t)dst_crs | (uintptr_t)dst_grid) & 7) == 0,
               "ig_s1_chip_cut: starts and the float64 arrays must be 8-byte aligned");
    IG_REQUIRE((((uintptr_t)planes | (uintptr_t)chips | (uintptr_t)scene_size | (uintptr_t)origins | (uintptr_t)valid_values) & 3) == 0,
               "ig_s1_chip_cut: planes, chips, scene_size, origins and valid_values must be 4-byte aligned");
    const S1CutArgs a{T, C, N, S, nb, has_src_nodata, clip, first_bits, no_data, src_nodata, clip_lo, clip_hi};
    const dim3 grid((unsigned)((long)nb * nb * n));
    return ig_launch<s1_chip_cut_kernel>("ig_s1_chip_cut", grid, dim3(VTPB), 0, (hipStream_t)stream,
                                         reinterpret_cast<const unsigned*>(planes), starts, scene_crs, scene_grid, scene_size, dst_crs, dst_grid,
                                         origins, a, reinterpret_cast<unsigned*>(chips), valid_values, validity);
}
