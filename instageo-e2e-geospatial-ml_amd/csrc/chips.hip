// Chips and label maps cut from a satellite tile for gfx950.  The reference cuts them with xarray on the host
// (instageo/data/data_pipeline.py: apply_mask, create_segmentation_map, mask_segmentation_map and the loop of
// create_and_save_chips_with_seg_maps); here the rule, stated in include/instageo_hip.h, runs as two kernels whose results are integers or
// copies and unique (independent of scheduling).
//
//   chip_cut_kernel      one workgroup of 256 threads per block of 16 rows x 128 columns of one chip; a thread owns 8 consecutive pixels of
//                        one row.  It reads its T fmask bytes per pixel once into a per-pixel date mask, streams the T * C bands through
//                        (load, mask, clip, count, store) and writes the validity byte from the same pass.  The access width of every
//                        8-pixel segment is chosen from its address (16 / 8 / 4 / 2 bytes): with a row pitch that is 8 mod 16 alignment
//                        alternates from row to row.  valid_values: wave shuffle, LDS across the 4 waves, one integer atomic per workgroup.
//   chip_labels_kernel   one workgroup per 64 x 64 block of one chip's label map, an int32 winner plane in LDS (-1); a thread takes every
//                        256th point of the chip, clips its window to the chip and the block and applies an LDS atomic max of the original
//                        index; after the barrier a thread resolves 16 pixels (winner -> label, validity bit), stores them and tallies
//                        valid_labels and the class histogram in LDS; integer atomics add them.
//
// Out-of-range accesses are impossible: a chip whose origin does not leave it wholly inside the tile is skipped by its workgroups (the
// host checks origins before they are uploaded, this is the second fence), every pixel access is guarded by row < S and column < S, a
// point outside its chip or with an index outside [0, P) paints nothing, and a label outside [0, K) is not counted.
#include "chip_kernels.h"
#include "common.h"

namespace {

constexpr int CB_H = 16, CB_W = 128, CSEG = 8, CTPB = 256;  // block rows, block columns, pixels per thread, threads
constexpr int LB = 64, LTPB = 256, MAX_K = 256;             // label block side, threads, histogram cells
constexpr int MAX_W = 1 << 20;

struct CutArgs {
    int T, C, H, W, S, mask_bits, any, no_data, clip, lo, hi, bx, by;  // bx, by: blocks across and down one chip
};

__global__ __launch_bounds__(CTPB) void chip_cut_kernel(const short* __restrict__ tile, const unsigned char* __restrict__ fmask,
                                                        const int* __restrict__ origins, CutArgs a, short* __restrict__ chips,
                                                        int* __restrict__ valid_values, unsigned char* __restrict__ validity) {
    __shared__ int part[4];
    const int per = a.bx * a.by;
    const int chip = blockIdx.x / per, blk = blockIdx.x - chip * per;
    const int r0 = origins[2 * chip], c0 = origins[2 * chip + 1];
    if (r0 < 0 || c0 < 0 || r0 > a.H - a.S || c0 > a.W - a.S) return;  // the whole workgroup: nothing is read for a chip outside the tile
    const int r = (blk / a.bx) * CB_H + (threadIdx.x >> 4), c = (blk % a.bx) * CB_W + (threadIdx.x & 15) * CSEG;
    const bool live = r < a.S && c < a.S;
    const bool whole = live && c + CSEG <= a.S;  // the segment lies inside the chip row
    const int npx = live ? min(CSEG, a.S - c) : 0;
    const long plane = (long)a.H * a.W, cplane = (long)a.S * a.S;
    const long src = (long)(r0 + r) * a.W + c0 + c, dst = (long)chip * a.T * a.C * cplane + (long)r * a.S + c;
    int count = 0;
    if (live) {
        unsigned dm[CSEG];  // bit t: date t is masked at pixel j
#pragma unroll
        for (int j = 0; j < CSEG; ++j) dm[j] = 0u;
        if (fmask) {
            for (int t = 0; t < a.T; ++t) {
                unsigned char f[CSEG];
                const unsigned char* p = fmask + t * plane + src;
                if (whole) {
                    load_seg<CSEG>(p, f);
                } else {
#pragma unroll
                    for (int j = 0; j < CSEG; ++j) f[j] = j < npx ? p[j] : 0;
                }
#pragma unroll
                for (int j = 0; j < CSEG; ++j) dm[j] |= (f[j] & a.mask_bits) ? 1u << t : 0u;
            }
            if (a.any) any_date(dm);
        }
        unsigned all = 0xffu, some = 0u;  // bit j: all / at least one of the pixel's values differ from no_data
        const short nd = (short)a.no_data, lo = (short)a.lo, hi = (short)a.hi;
        int t = 0, cc = 0;
        for (int b = 0; b < a.T * a.C; ++b) {
            short v[CSEG];
            const short* p = tile + b * plane + src;
            short* q = chips + dst + b * cplane;
            if (whole) {
                load_seg<2 * CSEG>(p, v);
            } else {
#pragma unroll
                for (int j = 0; j < CSEG; ++j) v[j] = j < npx ? p[j] : nd;
            }
            unsigned ok = 0u;
#pragma unroll
            for (int j = 0; j < CSEG; ++j) {
                short x = (dm[j] >> t & 1u) ? nd : v[j];
                if (a.clip) x = x < lo ? lo : x > hi ? hi : x;
                v[j] = x;
                ok |= (x != nd && j < npx) ? 1u << j : 0u;
            }
            all &= ok, some |= ok;
            count += __popc(ok);
            if (whole) {
                store_seg<2 * CSEG>(q, v);
            } else {
#pragma unroll
                for (int j = 0; j < CSEG; ++j)
                    if (j < npx) q[j] = v[j];
            }
            if (++cc == a.C) cc = 0, ++t;
        }
        if (validity) {
            unsigned char m[CSEG];
#pragma unroll
            for (int j = 0; j < CSEG; ++j) m[j] = (unsigned char)((all >> j & 1u) | (some >> j & 1u) << 1);
            unsigned char* q = validity + (long)chip * cplane + (long)r * a.S + c;
            if (whole) {
                store_seg<CSEG>(q, m);
            } else {
#pragma unroll
                for (int j = 0; j < CSEG; ++j)
                    if (j < npx) q[j] = m[j];
            }
        }
    }
    const int total = block_sum_int(count, part);
    if (threadIdx.x == 0 && total) atomicAdd(valid_values + chip, total);
}

template <typename L>
__device__ __forceinline__ L minus_one();
template <>
__device__ __forceinline__ short minus_one<short>() { return (short)-1; }
template <>
__device__ __forceinline__ float minus_one<float>() { return -1.0f; }

template <typename L>
__global__ __launch_bounds__(LTPB) void chip_labels_kernel(const int* __restrict__ origins, int S, int nb, const int* __restrict__ ptr,
                                                           const int* __restrict__ pts, const L* __restrict__ labels, long P, int w,
                                                           const unsigned char* __restrict__ validity, int valid_bit, int K,
                                                           L* __restrict__ maps, int* __restrict__ valid_labels, int* __restrict__ hist) {
    __shared__ int win[LB * LB];
    __shared__ int cells[MAX_K];
    __shared__ int part[4];
    const int per = nb * nb;
    const int chip = blockIdx.x / per, blk = blockIdx.x - chip * per;
    const int br = (blk / nb) * LB, bc = (blk % nb) * LB;  // the block's first row and column in the chip
    const int r0 = origins[2 * chip], c0 = origins[2 * chip + 1];
    for (int i = threadIdx.x; i < LB * LB; i += LTPB) win[i] = -1;
    for (int i = threadIdx.x; i < MAX_K; i += LTPB) cells[i] = 0;
    __syncthreads();
    const int first = ptr[chip], last = ptr[chip + 1];
    for (int j = first + (int)threadIdx.x; j < last; j += LTPB) {
        const int pr = pts[3 * (long)j] - r0, pc = pts[3 * (long)j + 1] - c0, idx = pts[3 * (long)j + 2];
        if ((unsigned)pr >= (unsigned)S || (unsigned)pc >= (unsigned)S || idx < 0 || idx >= P) continue;
        // the window, clipped to the chip and to the block (w <= 2^20, S < 2^31 - 2^20: no overflow)
        const int ra = max(max(pr - w, 0), br), rb = min(min(pr + w, S - 1), br + LB - 1);
        const int ca = max(max(pc - w, 0), bc), cb = min(min(pc + w, S - 1), bc + LB - 1);
        for (int r = ra; r <= rb; ++r)
            for (int c = ca; c <= cb; ++c) atomicMax(&win[(r - br) * LB + (c - bc)], idx);
    }
    __syncthreads();
    int count = 0;
    for (int i = threadIdx.x; i < LB * LB; i += LTPB) {
        const int r = br + i / LB, c = bc + i % LB;
        if (r >= S || c >= S) continue;
        const long at = (long)chip * S * S + (long)r * S + c;
        const int wi = win[i];
        L v = minus_one<L>();
        if (wi >= 0 && (!validity || (validity[at] & valid_bit))) v = labels[wi];
        maps[at] = v;
        if (v != minus_one<L>()) {
            ++count;
            if constexpr (sizeof(L) == 2) {
                if (hist && (unsigned)v < (unsigned)K) atomicAdd(&cells[(int)v], 1);
            }
        }
    }
    const int total = block_sum_int(count, part);  // its barrier also orders the histogram cells
    if (threadIdx.x == 0 && total) atomicAdd(valid_labels + chip, total);
    if constexpr (sizeof(L) == 2) {
        if (hist)
            for (int k = threadIdx.x; k < K; k += LTPB)
                if (cells[k]) atomicAdd(hist + (long)chip * K + k, cells[k]);
    }
}

}  // namespace

extern "C" int ig_chip_cut(const short* tile, const unsigned char* fmask, const int* origins, int n, int T, int C, int H, int W, int S,
                           int mask_bits, int strategy, int no_data, int clip, int clip_lo, int clip_hi, short* chips, int* valid_values,
                           unsigned char* validity, void* stream) {
    CHIP_CHECK(chip_check_stack("ig_chip_cut", n, T, C));
    IG_REQUIRE(H >= 1 && W >= 1, "ig_chip_cut: need H >= 1 and W >= 1 (H %d, W %d)", H, W);
    IG_REQUIRE(S >= 1, "ig_chip_cut: need a chip side S >= 1 (got %d)", S);
    IG_REQUIRE(S <= H && S <= W, "ig_chip_cut: a chip of side S = %d does not fit a tile of %d x %d pixels", S, H, W);
    CHIP_CHECK(chip_check_hls_rule("ig_chip_cut", mask_bits, strategy, no_data, clip, clip_lo, clip_hi));
    const long TC = (long)T * C;
    IG_REQUIRE(TC * H * W < CHIP_LIM40, "ig_chip_cut: T * C * H * W = %ld values exceeds 2^40", TC * H * W);
    CHIP_CHECK(chip_check_values("ig_chip_cut", TC, S));
    if (n == 0) return IG_OK;
    const int bx = ig_cdiv(S, CB_W), by = ig_cdiv(S, CB_H);
    CHIP_CHECK(chip_check_launch("ig_chip_cut", n, TC, S, (long)bx * by));
    IG_REQUIRE(tile && origins && chips && valid_values, "ig_chip_cut: null pointer");
    IG_REQUIRE((((uintptr_t)tile | (uintptr_t)chips) & 1) == 0 && (((uintptr_t)origins | (uintptr_t)valid_values) & 3) == 0,
               "ig_chip_cut: tile and chips must be 2-byte, origins and valid_values 4-byte aligned");
    const CutArgs a{T, C, H, W, S, fmask ? mask_bits : 0, strategy, no_data, clip, clip_lo, clip_hi, bx, by};
    return ig_launch<chip_cut_kernel>("ig_chip_cut", dim3((unsigned)((long)bx * by * n)), dim3(CTPB), 0, (hipStream_t)stream, tile, fmask,
                                      origins, a, chips, valid_values, validity);
}

extern "C" int ig_chip_labels(const int* origins, int n, int S, const int* ptr, const int* pts, const void* labels, long P, int elem_size,
                              int w, const unsigned char* validity, int valid_bit, int K, void* maps, int* valid_labels, int* hist,
                              void* stream) {
    IG_REQUIRE(n >= 0, "ig_chip_labels: need n >= 0 (got %d)", n);
    IG_REQUIRE(S >= 1 && S <= (1 << 30), "ig_chip_labels: need a chip side 1 <= S <= 2^30 (got %d)", S);
    IG_REQUIRE(elem_size == 2 || elem_size == 4, "ig_chip_labels: elem_size must be 2 (int16) or 4 (float32) (got %d)", elem_size);
    IG_REQUIRE(w >= 0 && w <= MAX_W, "ig_chip_labels: need a window 0 <= w <= 2^20 (got %d)", w);
    IG_REQUIRE(K >= 0 && K <= MAX_K, "ig_chip_labels: need 0 <= K <= %d histogram cells (got %d)", MAX_K, K);
    IG_REQUIRE(K == 0 || elem_size == 2, "ig_chip_labels: a class histogram (K = %d) needs int16 labels", K);
    IG_REQUIRE(P >= 0 && P <= 0x7fffffffL, "ig_chip_labels: need 0 <= P <= 2^31 - 1 points (got %ld)", P);
    IG_REQUIRE(valid_bit >= 0 && valid_bit <= 2, "ig_chip_labels: valid_bit must be 0 none, 1 any or 2 each (got %d)", valid_bit);
    IG_REQUIRE((valid_bit != 0) == (validity != nullptr), "ig_chip_labels: valid_bit %d does not go with %s validity plane", valid_bit,
               validity ? "a" : "no");
    if (n == 0) return IG_OK;
    const int nb = ig_cdiv(S, LB);
    IG_REQUIRE((long)nb * nb * n <= 0x7fffffffL, "ig_chip_labels: %ld workgroups exceed 2^31 - 1 (n %d, S %d)", (long)nb * nb * n, n, S);
    IG_REQUIRE((long)S * S < CHIP_LIM40 / n, "ig_chip_labels: n * S * S exceeds 2^40 pixels (n %d, S %d)", n, S);
    IG_REQUIRE(origins && ptr && maps && valid_labels, "ig_chip_labels: null pointer");
    IG_REQUIRE(P == 0 || (pts && labels), "ig_chip_labels: null pointer (pts, labels)");
    IG_REQUIRE(K == 0 || hist, "ig_chip_labels: null pointer (hist)");
    IG_REQUIRE((((uintptr_t)origins | (uintptr_t)ptr | (uintptr_t)pts | (uintptr_t)valid_labels | (uintptr_t)hist) & 3) == 0 &&
                   (((uintptr_t)labels | (uintptr_t)maps) & (elem_size - 1)) == 0,
               "ig_chip_labels: origins, ptr, pts, valid_labels and hist must be 4-byte aligned, labels and maps to their elements");
    const dim3 grid((unsigned)((long)nb * nb * n));
    if (elem_size == 2)
        return ig_launch<chip_labels_kernel<short>>("ig_chip_labels", grid, dim3(LTPB), 0, (hipStream_t)stream, origins, S, nb, ptr, pts,
                                                    (const short*)labels, P, w, validity, valid_bit, K, (short*)maps, valid_labels,
                                                    K ? hist : nullptr);
    return ig_launch<chip_labels_kernel<float>>("ig_chip_labels", grid, dim3(LTPB), 0, (hipStream_t)stream, origins, S, nb, ptr, pts,
                                                (const float*)labels, P, w, validity, valid_bit, 0, (float*)maps, valid_labels, nullptr);
}
