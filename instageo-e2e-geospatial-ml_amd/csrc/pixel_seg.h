// Pixel-segment access and integer workgroup sums shared by the integer raster kernels (chips.hip, s2_chips.hip, clean.hip, and the chip
// layer of chip_kernels.h): a thread owns a short run of consecutive pixels whose alignment depends on the row or plane it lies in, so the
// access width is chosen from the address.
#pragma once
#include "common.h"

namespace {

// BYTES bytes (2, 4, 8, 16 or 32) from / to p in the widest units the address allows; an arm is taken only when BYTES holds its unit
template <int BYTES>
__device__ __forceinline__ void load_seg(const void* p, void* v) {
    const unsigned a = (unsigned)reinterpret_cast<uintptr_t>(p);
    const char* s = static_cast<const char*>(p);
    char* d = static_cast<char*>(v);
    if (BYTES >= 16 && (a & 15) == 0) {
#pragma unroll
        for (int q = 0; q < BYTES / 16; ++q) {
            const uint4 u = *reinterpret_cast<const uint4*>(s + 16 * q);
            __builtin_memcpy(d + 16 * q, &u, 16);
        }
    } else if (BYTES >= 8 && (a & 7) == 0) {
#pragma unroll
        for (int q = 0; q < BYTES / 8; ++q) {
            const uint2 u = *reinterpret_cast<const uint2*>(s + 8 * q);
            __builtin_memcpy(d + 8 * q, &u, 8);
        }
    } else if (BYTES >= 4 && (a & 3) == 0) {
#pragma unroll
        for (int q = 0; q < BYTES / 4; ++q) {
            const unsigned u = *reinterpret_cast<const unsigned*>(s + 4 * q);
            __builtin_memcpy(d + 4 * q, &u, 4);
        }
    } else if (BYTES >= 2 && (a & 1) == 0) {
#pragma unroll
        for (int q = 0; q < BYTES / 2; ++q) {
            const unsigned short u = *reinterpret_cast<const unsigned short*>(s + 2 * q);
            __builtin_memcpy(d + 2 * q, &u, 2);
        }
    } else {
#pragma unroll
        for (int q = 0; q < BYTES; ++q) d[q] = s[q];
    }
}

template <int BYTES>
__device__ __forceinline__ void store_seg(void* p, const void* v) {
    const unsigned a = (unsigned)reinterpret_cast<uintptr_t>(p);
    char* d = static_cast<char*>(p);
    const char* s = static_cast<const char*>(v);
    if (BYTES >= 16 && (a & 15) == 0) {
#pragma unroll
        for (int q = 0; q < BYTES / 16; ++q) {
            uint4 u;
            __builtin_memcpy(&u, s + 16 * q, 16);
            *reinterpret_cast<uint4*>(d + 16 * q) = u;
        }
    } else if (BYTES >= 8 && (a & 7) == 0) {
#pragma unroll
        for (int q = 0; q < BYTES / 8; ++q) {
            uint2 u;
            __builtin_memcpy(&u, s + 8 * q, 8);
            *reinterpret_cast<uint2*>(d + 8 * q) = u;
        }
    } else if (BYTES >= 4 && (a & 3) == 0) {
#pragma unroll
        for (int q = 0; q < BYTES / 4; ++q) {
            unsigned u;
            __builtin_memcpy(&u, s + 4 * q, 4);
            *reinterpret_cast<unsigned*>(d + 4 * q) = u;
        }
    } else if (BYTES >= 2 && (a & 1) == 0) {
#pragma unroll
        for (int q = 0; q < BYTES / 2; ++q) {
            unsigned short u;
            __builtin_memcpy(&u, s + 2 * q, 2);
            *reinterpret_cast<unsigned short*>(d + 2 * q) = u;
        }
    } else {
#pragma unroll
        for (int q = 0; q < BYTES; ++q) d[q] = s[q];
    }
}

// A run of N elements of which the first npx exist (whole: npx == N, one segment access): q <- v
template <int N, typename E>
__device__ __forceinline__ void store_run(E* q, bool whole, int npx, const E* v) {
    if (whole) {
        store_seg<N * (int)sizeof(E)>(q, v);
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j)
            if (j < npx) q[j] = v[j];
    }
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the workgroup's sum of v (4 waves) -> thread 0
__device__ __forceinline__ int block_sum_int(int v, int* part) {
    v = wave_sum_int(v);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    return part[0] + part[1] + part[2] + part[3];
}

}  // namespace
