// The last phase shared by the column kernels (raster_chips.hip, s2_raster_chips.hip, and s1_chips.hip without labels; they include it
// through chip_kernels.h): the validity byte and the label pixel of a thread's ROWS pixels, then the tallies, as the rule of
// include/instageo_hip.h states them.  All three files include this text, so all evaluate the same epilogue.
#pragma once
#include "common.h"
#include "pixel_seg.h"

namespace {

constexpr int EPI_MAX_K = 128;  // cells of the class histogram

template <typename L>
__device__ __forceinline__ bool label_nan(L) { return false; }
template <>
__device__ __forceinline__ bool label_nan<float>(float v) { return v != v; }

// A thread owns the pixels at0 + 4 k rows (k < ROWS) of chip `chip` (cplane = S * S); bit k of live / all / some: the pixel exists / all /
// at least one of its values differ from no_data; count: the thread's values that differ from no_data.  L: signed char, float, or void
// (no labels).  part (4 ints) and cells (EPI_MAX_K ints, zeroed before the first barrier of the kernel when L is not void) are LDS.
template <typename L, int ROWS, int TPB>
__device__ __forceinline__ void chip_epilogue(unsigned live, unsigned all, unsigned some, int count, int chip, long cplane, long at0, int S,
                                              int valid_bit, int K, const void* __restrict__ labels_v, int* __restrict__ valid_values,
                                              unsigned char* __restrict__ validity, void* __restrict__ maps_v, int* __restrict__ valid_labels,
                                              int* __restrict__ hist, int* part, int* cells) {
    constexpr bool LABELS = !__is_same(L, void);
    int lcount = 0;
#pragma unroll
    for (int k = 0; k < ROWS; ++k) {
        if (!(live >> k & 1u)) continue;
        const long at = (long)chip * cplane + at0 + (long)(4 * k) * S;
        const unsigned m = (all >> k & 1u) | (some >> k & 1u) << 1;
        if (validity) validity[at] = (unsigned char)m;
        if constexpr (LABELS) {
            L v = static_cast<const L*>(labels_v)[at];
            if ((valid_bit && !(m & (unsigned)valid_bit)) || label_nan<L>(v)) v = (L)-1;
            static_cast<L*>(maps_v)[at] = v;
            if (v != (L)-1) {
                ++lcount;
                if constexpr (sizeof(L) == 1) {
                    if (hist && (unsigned)(int)v < (unsigned)K) atomicAdd(&cells[(int)v], 1);
                }
            }
        }
    }
    const int total = block_sum_int(count, part);
    if (threadIdx.x == 0 && total) atomicAdd(valid_values + chip, total);
    if constexpr (LABELS) {
        __syncthreads();  // part is read by every thread before it is written again; also orders the histogram cells
        const int ltotal = block_sum_int(lcount, part);
        if (threadIdx.x == 0 && ltotal) atomicAdd(valid_labels + chip, ltotal);
        if constexpr (sizeof(L) == 1) {
            if (hist)
                for (int k = threadIdx.x; k < K; k += TPB)
                    if (cells[k]) atomicAdd(hist + (long)chip * K + k, cells[k]);
        }
    }
}

}  // namespace
