// Segmented wave reductions (wave = 64 lanes), shared by regions.hip and vectorize.hip.
#pragma once
#include "common.h"

// Lanes hold (key, value); runs of equal keys in ADJACENT lanes are reduced to the first lane of the run, which then issues ONE atomic.
// Equal keys that are not adjacent reach memory as separate atomics (same result).  All 64 lanes must call.
struct Seg {
    bool head;
    int end;  // last lane of this lane's run
};
__device__ __forceinline__ Seg seg_of(int key) {
    const int lane = threadIdx.x & 63;
    const int prev = __shfl_up(key, 1, 64);
    Seg s;
    s.head = lane == 0 || prev != key;
    const unsigned long long heads = __ballot(s.head);
    const unsigned long long above = lane == 63 ? 0ull : heads & ~((2ull << lane) - 1ull);
    s.end = above ? __ffsll((long long)above) - 2 : 63;
    return s;
}
struct OpAdd {
    template <typename T>
    __device__ static T f(T a, T b) { return a + b; }
};
struct OpMin {
    template <typename T>
    __device__ static T f(T a, T b) { return a < b ? a : b; }
};
struct OpMax {
    template <typename T>
    __device__ static T f(T a, T b) { return a > b ? a : b; }
};
// after the call the head lane of a run holds the reduction over the run
template <typename Op, typename T>
__device__ __forceinline__ T seg_reduce(T v, const Seg& s) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T other = __shfl_down(v, o, 64);
        if (lane + o <= s.end) v = Op::f(v, other);
    }
    return v;
}
