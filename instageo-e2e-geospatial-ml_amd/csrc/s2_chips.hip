// Chips cut from Sentinel-2 L2A planes of several resolutions under the scene classification, for gfx950.  The reference
// lets stackstac resample the 10 m and 20 m bands onto one resolution on the host and then cuts with xarray (instageo/data/s2_utils.py:
// S2PointsPipeline, create_mask_from_scl, apply_mask); here the rule, stated in include/instageo_hip.h, is one kernel that reads every plane
// on its own grid and whose results are integers or copies and unique (independent of scheduling).
//
//   s2_chip_cut_kernel   the blocking of chip_cut_kernel (chips.hip): one workgroup of 256 threads per block of 16 rows x 128 columns of one
//                        chip, a thread owns 8 consecutive output pixels of one row.  It gathers its T SCL classes per pixel once into a
//                        per-pixel date mask, streams the T * C bands through (gather, offset, mask, range, count, one 16-byte store) and
//                        writes the validity byte from the same pass.  The read side of a plane is chosen from its pixel size, uniformly
//                        for the workgroup:
//                          p_k = p_o     the 8 pixels in the widest units their address allows (16 / 8 / 4 / 2 bytes);
//                          p_k = 2 p_o   the 4 (even first column) or 5 (odd) source pixels the 8 outputs come from, 8 / 4 / 2 bytes at a
//                                        time, expanded in registers.  The two output rows of a pair lie in one wave and read the same
//                                        addresses in the same instruction, so the pair costs one trip to the cache; staging the source
//                                        block in LDS instead would put a barrier between every two bands of a kernel that is otherwise
//                                        a free-running stream of independent loads and stores;
//                          otherwise     element by element: one 64-bit division for the thread's first pixel, then quotient-and-
//                                        remainder steps (60 m planes, downsampling), also every segment that crosses the chip's or the
//                                        plane's edge.
//                        valid_values: wave shuffle, LDS across the 4 waves, one integer atomic per workgroup.
//
// Out-of-range accesses are impossible: a chip whose origin does not leave it wholly inside the output grid is skipped by its workgroups
// (the host checks origins before they are uploaded, this is the second fence); a plane whose table entry breaks the bounds of the header
// reads nothing; every source index is compared with the plane's size before it is used and a vector read is taken only when its last
// element lies inside the row; every store is guarded by row < S and column < S.
#include "chip_kernels.h"
#include "common.h"

namespace {

constexpr int CB_H = 16, CB_W = 128, CSEG = 8, CTPB = 256;  // block rows, block columns, pixels per thread, threads
constexpr int MAX_P = 1 << 15;                              // pixel sizes

struct S2Args {
    int T, C, Ho, Wo, po, S, any, no_data, boa, range, lo, hi, bx, by;
    unsigned class_bits;
};

// The CSEG values of plane `base` (H x W pixels of size p; H = 0: a plane that reads nothing) under the output pixels (R, Cc .. Cc + 7) of
// size po, the first npx of them; 0 where the source pixel lies outside the plane and for j >= npx.
template <typename E>
__device__ __forceinline__ void gather_seg(const E* __restrict__ base, int H, int W, int p, int po, int R, int Cc, int npx, E* v) {
#pragma unroll
    for (int j = 0; j < CSEG; ++j) v[j] = (E)0;
    if (H <= 0) return;
    if (p == po) {  // ratio 1
        if (R >= H) return;
        const E* src = base + (long)R * W + Cc;
        if (npx == CSEG && Cc + CSEG <= W) {
            load_seg<CSEG * (int)sizeof(E)>(src, v);
        } else {
#pragma unroll
            for (int j = 0; j < CSEG; ++j)
                if (j < npx && Cc + j < W) v[j] = src[j];
        }
        return;
    }
    if (p == 2 * po) {  // each source pixel fans out into 2 x 2
        const int rs = R >> 1, cs = Cc >> 1, odd = Cc & 1;
        if (rs >= H) return;
        const E* src = base + (long)rs * W + cs;
        if (npx == CSEG && cs + 4 + odd <= W) {
            E e[5];
            load_seg<4 * (int)sizeof(E)>(src, e);
            e[4] = odd ? src[4] : (E)0;
#pragma unroll
            for (int j = 0; j < CSEG; ++j) v[j] = odd ? e[(j + 1) >> 1] : e[j >> 1];
        } else {
#pragma unroll
            for (int j = 0; j < CSEG; ++j) {
                const int c = (Cc + j) >> 1;
                if (j < npx && c < W) v[j] = base[(long)rs * W + c];
            }
        }
        return;
    }
    // any other ratio: floor(((2 x + 1) po) / (2 p)) by one division for the first pixel, then steps of (quotient, remainder) of 2 po / 2 p
    const long d = 2L * p;
    const long rs = ((2L * R + 1) * po) / d;
    if (rs >= H) return;
    const long num = (2L * Cc + 1) * po;
    long cs = num / d;
    int rem = (int)(num - cs * d);
    const int dq = (2 * po) / (2 * p), dm = 2 * po - dq * 2 * p;
    const E* row = base + rs * W;
#pragma unroll
    for (int j = 0; j < CSEG; ++j) {
        if (j < npx && cs < W) v[j] = row[cs];
        cs += dq, rem += dm;
        if (rem >= (int)d) rem -= (int)d, ++cs;
    }
}

__global__ __launch_bounds__(CTPB) void s2_chip_cut_kernel(const unsigned short* __restrict__ bands, const long long* __restrict__ starts,
                                                           const unsigned char* __restrict__ scl, const long long* __restrict__ scl_starts,
                                                           const int* __restrict__ geom, const int* __restrict__ origins, S2Args a,
                                                           unsigned short* __restrict__ chips, int* __restrict__ valid_values,
                                                           unsigned char* __restrict__ validity) {
    __shared__ int part[4];
    const int per = a.bx * a.by;
    const int chip = blockIdx.x / per, blk = blockIdx.x - chip * per;
    const int r0 = origins[2 * chip], c0 = origins[2 * chip + 1];
    if (r0 < 0 || c0 < 0 || r0 > a.Ho - a.S || c0 > a.Wo - a.S) return;  // the whole workgroup: nothing is read for a chip outside the grid
    const int r = (blk / a.bx) * CB_H + (threadIdx.x >> 4), c = (blk % a.bx) * CB_W + (threadIdx.x & 15) * CSEG;
    const bool live = r < a.S && c < a.S;
    const bool whole = live && c + CSEG <= a.S;  // the segment lies inside the chip row
    const int npx = live ? min(CSEG, a.S - c) : 0;
    const int TC = a.T * a.C;
    const long cplane = (long)a.S * a.S;
    const long dst = (long)chip * TC * cplane + (long)r * a.S + c;
    const int R = r0 + r, Cc = c0 + c;  // on the output grid
    int count = 0;
    if (live) {
        unsigned dm[CSEG];  // bit t: date t is masked at pixel j
#pragma unroll
        for (int j = 0; j < CSEG; ++j) dm[j] = 0u;
        if (scl && a.class_bits) {
            for (int t = 0; t < a.T; ++t) {
                const int* g = geom + 3 * (TC + t);
                int H = g[0], W = g[1];
                const int p = g[2];
                const long long at = scl_starts[t];
                if (H < 1 || W < 1 || p < 1 || p > MAX_P || (long)H * W > 0x7fffffffL || at < 0) H = 0;
                unsigned char f[CSEG];
                gather_seg<unsigned char>(scl + at, H, W, p, a.po, R, Cc, npx, f);
#pragma unroll
                for (int j = 0; j < CSEG; ++j) dm[j] |= (f[j] < 32 && (a.class_bits >> f[j] & 1u)) ? 1u << t : 0u;
            }
            if (a.any) any_date(dm);
        }
        unsigned all = 0xffu, some = 0u;  // bit j: all / at least one of the pixel's values differ from no_data
        int t = 0, cc = 0;
        for (int b = 0; b < TC; ++b) {
            const int* g = geom + 3 * b;
            int H = g[0], W = g[1];
            const int p = g[2];
            const long long at = starts[b];
            if (H < 1 || W < 1 || p < 1 || p > MAX_P || (long)H * W > 0x7fffffffL || at < 0) H = 0;
            unsigned short v[CSEG];
            gather_seg<unsigned short>(bands + at, H, W, p, a.po, R, Cc, npx, v);
            unsigned short* q = chips + dst + b * cplane;
            unsigned ok = 0u;
#pragma unroll
            for (int j = 0; j < CSEG; ++j) {
                int x = v[j];
                if (a.boa > 0 && x != 0) x = max(x - a.boa, 0);
                if (dm[j] >> t & 1u) x = a.no_data;
                if (a.range && (x < a.lo || x > a.hi)) x = a.no_data;
                v[j] = (unsigned short)x;
                ok |= (x != a.no_data && j < npx) ? 1u << j : 0u;
            }
            all &= ok, some |= ok;
            count += __popc(ok);
            store_run<CSEG>(q, whole, npx, v);
            if (++cc == a.C) cc = 0, ++t;
        }
        if (validity) {
            unsigned char m[CSEG];
#pragma unroll
            for (int j = 0; j < CSEG; ++j) m[j] = (unsigned char)((all >> j & 1u) | (some >> j & 1u) << 1);
            unsigned char* q = validity + (long)chip * cplane + (long)r * a.S + c;
            store_run<CSEG>(q, whole, npx, m);
        }
    }
    const int total = block_sum_int(count, part);
    if (threadIdx.x == 0 && total) atomicAdd(valid_values + chip, total);
}

}  // namespace

extern "C" int ig_s2_chip_cut(const unsigned short* bands, const long long* starts, const unsigned char* scl, const long long* scl_starts,
                              const int* geom, const int* origins, int n, int T, int C, int Ho, int Wo, int po, int S, unsigned class_bits,
                              int strategy, int no_data, int boa_offset, int range, int range_lo, int range_hi, unsigned short* chips,
                              int* valid_values, unsigned char* validity, void* stream) {
    CHIP_CHECK(chip_check_stack("ig_s2_chip_cut", n, T, C));
    IG_REQUIRE(Ho >= 1 && Wo >= 1, "ig_s2_chip_cut: need an output grid of Ho >= 1 and Wo >= 1 pixels (Ho %d, Wo %d)", Ho, Wo);
    IG_REQUIRE((long)Ho * Wo <= 0x7fffffffL, "ig_s2_chip_cut: an output grid of Ho * Wo = %ld pixels exceeds 2^31 - 1", (long)Ho * Wo);
    IG_REQUIRE(po >= 1 && po <= MAX_P, "ig_s2_chip_cut: the output pixel size must lie in [1, 2^15] (got %d)", po);
    IG_REQUIRE(S >= 1, "ig_s2_chip_cut: need a chip side S >= 1 (got %d)", S);
    IG_REQUIRE(S <= Ho && S <= Wo, "ig_s2_chip_cut: a chip of side S = %d does not fit an output grid of %d x %d pixels", S, Ho, Wo);
    CHIP_CHECK(chip_check_s2_rule("ig_s2_chip_cut", strategy, no_data, boa_offset, range, range_lo, range_hi));
    const long TC = (long)T * C;
    IG_REQUIRE(TC <= 0x7fffffffL / 3 - CHIP_MAX_T, "ig_s2_chip_cut: T * C = %ld planes are too many for the int32 plane table", TC);
    CHIP_CHECK(chip_check_values("ig_s2_chip_cut", TC, S));
    if (n == 0) return IG_OK;
    const int bx = ig_cdiv(S, CB_W), by = ig_cdiv(S, CB_H);
    CHIP_CHECK(chip_check_launch("ig_s2_chip_cut", n, TC, S, (long)bx * by));
    IG_REQUIRE(bands && starts && geom && origins && chips && valid_values, "ig_s2_chip_cut: null pointer");
    IG_REQUIRE(!scl || scl_starts, "ig_s2_chip_cut: null pointer (scl_starts goes with scl)");
    IG_REQUIRE((((uintptr_t)bands | (uintptr_t)chips) & 1) == 0 && (((uintptr_t)geom | (uintptr_t)origins | (uintptr_t)valid_values) & 3) == 0 &&
                   (((uintptr_t)starts | (uintptr_t)scl_starts) & 7) == 0,
               "ig_s2_chip_cut: bands and chips must be 2-byte, geom, origins and valid_values 4-byte, starts and scl_starts 8-byte aligned");
    const S2Args a{T, C, Ho, Wo, po, S, strategy, no_data, boa_offset, range, range_lo, range_hi, bx, by, scl ? class_bits : 0u};
    return ig_launch<s2_chip_cut_kernel>("ig_s2_chip_cut", dim3((unsigned)((long)bx * by * n)), dim3(CTPB), 0, (hipStream_t)stream, bands, starts,
                                         scl, scl_starts, geom, origins, a, chips, valid_values, validity);
}
