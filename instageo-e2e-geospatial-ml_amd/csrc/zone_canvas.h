// The toggle canvas of zonal.hip and burn.hip, once: the geometry of a workgroup on a canvas row, the loader of a
// thread's toggles and the scan that turns them into inside masks.
#pragma once
#include "common.h"

constexpr int ZTPB = 256, ZWAVES = ZTPB / 64;
constexpr int ZVPT = 4, ZCHUNK = ZTPB * ZVPT;  // columns a workgroup scans in one step
constexpr int ZBITS = 64, MAX_WG = 1024;       // zones (features) of a pass; workgroups of a launch that walks rows

// v[j] = the toggles of columns c .. c + ZVPT - 1 of a canvas row of W columns, 0 past the row's end.
__device__ __forceinline__ void zone_load_toggles(unsigned long long (&v)[ZVPT], const unsigned long long* row, long c, long W) {
#pragma unroll
    for (int j = 0; j < ZVPT; ++j) v[j] = c + j < W ? row[c + j] : 0ull;
}

// The scan, once for every kernel that turns toggles into inside masks: the inclusive prefix XOR of one chunk of ZCHUNK columns of a
// canvas row, continued from the row's earlier chunks.  v[j] = the toggles of this thread's columns c .. c + ZVPT - 1 (0 past the row's
// end) become the inside masks of those columns (dead columns hold the mask of the last live one: the caller drops them).  Thread run,
// wave scan, workgroup scan through wtot (the wave totals of this chunk: the caller alternates two of them, so one barrier per chunk is
// enough), and carry = the prefix XOR of the row's earlier chunks, the same in every thread, updated for the next chunk.  Every thread of
// the workgroup calls it (it holds a barrier).
__device__ __forceinline__ void zone_scan_chunk(unsigned long long (&v)[ZVPT], unsigned long long& carry, unsigned long long* wtot) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 1; j < ZVPT; ++j) v[j] ^= v[j - 1];
    unsigned long long t = v[ZVPT - 1];  // inclusive scan of the thread totals over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long u = __shfl_up(t, o, 64);
        if (lane >= o) t ^= u;
    }
    if (lane == 63) wtot[wave] = t;
    __syncthreads();
    unsigned long long pre = carry ^ t ^ v[ZVPT - 1];  // XOR undoes itself: inclusive ^ own = exclusive
#pragma unroll
    for (int w = 0; w < ZWAVES; ++w) {
        const unsigned long long u = wtot[w];
        if (w < wave) pre ^= u;
        carry ^= u;
    }
#pragma unroll
    for (int j = 0; j < ZVPT; ++j) v[j] ^= pre;
}
