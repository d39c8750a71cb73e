// The shared layer of the kernels that walk (B, ncls, HW) fp32 planar logits one pixel (or VEC consecutive pixels) per thread: the loss,
// metric and inference kernels of head.hip and the calibration kernels of calibrate.hip.  It owns the pixel split, the rule that says which
// labels carry loss and gradient, the plane-coalesced load / store of a thread's logits, the workgroup and grid totals in a fixed order,
// the capped grid and the label-dtype dispatch.  A new per-pixel kernel starts from these; it does not copy them.
#pragma once
#include <type_traits>

#include "common.h"

namespace {

constexpr int PX_TPB = 256, PX_NWAVE = PX_TPB / 64;  // every kernel of the family: 256 threads, 4 waves
constexpr int PX_MAX_WG = 1024;                       // grid-stride above it: one round of global adds / one partial row per workgroup

// ---- device ---------------------------------------------------------------------------------------------------------------------
// m = b * HW + pix.  A 64-bit integer division is ~150 instructions on this hardware and sat in per-pixel loops; the 32-bit form
// (pixel counts below 2^31: every real batch) is ~30.
__device__ __forceinline__ void split_pixel(long m, long HW, long& b, long& pix) {
    if ((unsigned long)(m | HW) < (1ul << 31)) {
        const unsigned bu = (unsigned)m / (unsigned)HW;
        b = bu, pix = (long)((unsigned)m - bu * (unsigned)HW);
    } else {
        b = m / HW, pix = m - b * HW;
    }
}

// THE validity rule: a pixel carries loss and gradient iff its label is not ignore_index and names a class, 0 <= label < ncls.
// (auc_update_kernel alone deviates, see there.)  valid_class: the class of a label already loaded and widened, -1 where the pixel is not
// valid.  valid_label: the same as a predicate, and the form that loads the label of pixel m (y = the class where valid).
__device__ __forceinline__ long valid_class(long l, long ignore_index, int ncls) {
    if (l == ignore_index || l < 0 || l >= ncls) l = -1;
    return l;
}
__device__ __forceinline__ bool valid_label(long l, long ignore_index, int ncls) { return valid_class(l, ignore_index, ncls) >= 0; }
template <typename LABEL>
__device__ __forceinline__ bool valid_label(const LABEL* labels, long m, long ignore_index, int ncls, int& y) {
    const long l = (long)labels[m];
    y = (int)l;
    return valid_label(l, ignore_index, ncls);
}

// z[n][.] = the logits of class n < ncls at VEC consecutive pixels of image b starting at pix: one 16-byte load per class plane when
// VEC == 4 (the caller guarantees HW % 4 == 0 and 16-byte aligned bases), one scalar load when VEC == 1.  Consecutive lanes read
// consecutive addresses of one plane.  store_logits / add_logits write them back the same way (add: read-modify-write).
template <int NCB, int VEC>
__device__ __forceinline__ void load_logits(const float* logits, long b, long pix, long HW, int ncls, float (&z)[NCB][VEC]) {
    static_assert(VEC == 1 || VEC == 4, "scalar or float4");
#pragma unroll
    for (int n = 0; n < NCB; ++n) {
        if (n < ncls) {
            const float* src = logits + (b * ncls + n) * HW + pix;
            if constexpr (VEC == 4) {
                const float4 v = *reinterpret_cast<const float4*>(src);
                z[n][0] = v.x, z[n][1] = v.y, z[n][2] = v.z, z[n][3] = v.w;
            } else {
                z[n][0] = *src;
            }
        }
    }
}
template <int NCB, int VEC, bool ADD>
__device__ __forceinline__ void store_logits_impl(float* out, long b, long pix, long HW, int ncls, const float (&z)[NCB][VEC]) {
    static_assert(VEC == 1 || VEC == 4, "scalar or float4");
#pragma unroll
    for (int n = 0; n < NCB; ++n) {
        if (n < ncls) {
            float* dst = out + (b * ncls + n) * HW + pix;
            if constexpr (VEC == 4) {
                float4 v = make_float4(z[n][0], z[n][1], z[n][2], z[n][3]);
                if constexpr (ADD) {
                    v = *reinterpret_cast<const float4*>(dst);
                    v.x += z[n][0], v.y += z[n][1], v.z += z[n][2], v.w += z[n][3];
                }
                *reinterpret_cast<float4*>(dst) = v;
            } else {
                if constexpr (ADD) *dst += z[n][0];
                else *dst = z[n][0];
            }
        }
    }
}
template <int NCB, int VEC>
__device__ __forceinline__ void store_logits(float* out, long b, long pix, long HW, int ncls, const float (&z)[NCB][VEC]) {
    store_logits_impl<NCB, VEC, false>(out, b, pix, HW, ncls, z);
}
template <int NCB, int VEC>
__device__ __forceinline__ void add_logits(float* out, long b, long pix, long HW, int ncls, const float (&z)[NCB][VEC]) {
    store_logits_impl<NCB, VEC, true>(out, b, pix, HW, ncls, z);
}

// Workgroup totals of NV doubles per thread in a FIXED order: each value goes through the xor butterfly of its wave (offsets 32, 16, ..,
// 1), lane 0 of every wave writes its row, and after the barrier thread i < NV adds the rows of value i in wave order 0, 1, 2, 3.
// Returns that total in thread i < NV and 0 elsewhere.  Contains one __syncthreads: every thread of the workgroup calls it (LDS writes a
// caller made before the call are visible after it).  blockDim.x == PX_TPB.
template <int NV>
__device__ __forceinline__ double block_totals(const double* v) {
    __shared__ double red[PX_NWAVE][NV];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        double a = v[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
        if (lane == 0) red[wave][i] = a;
    }
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x < NV) {
#pragma unroll
        for (int w = 0; w < PX_NWAVE; ++w) t += red[w][threadIdx.x];
    }
    return t;
}

// Grid-wide sums in a FIXED order (the reported loss statistics are bit-identical from run to run): thread i < NV of every workgroup
// hands in its workgroup's partial t; partials go to scratch[workgroup][i]; the workgroup that takes the last ticket adds them up in
// workgroup order (16 strided subsets per value, folded in subset order) and gets the totals back in t of its threads i < NV.
// Returns true in that workgroup only.  NV <= 16, blockDim.x == 256.  Launches that share the scratch are ordered on one stream.
template <int NV>
__device__ __forceinline__ bool ordered_grid_totals(double& t, double* __restrict__ scratch, unsigned* __restrict__ ticket) {
    static_assert(NV <= 16, "at most 16 values");
    __shared__ int s_last;
    __shared__ double s_sub[16][16];
    if (threadIdx.x < NV) scratch[(size_t)blockIdx.x * NV + threadIdx.x] = t;
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) s_last = atomicAdd(ticket, 1u) == gridDim.x - 1;
    __syncthreads();
    if (!s_last) return false;
    __threadfence();
    const int i = threadIdx.x & 15, g = threadIdx.x >> 4;
    double a = 0.0;
    if (i < NV)
        for (unsigned b = g; b < gridDim.x; b += 16) a += *reinterpret_cast<volatile double*>(scratch + (size_t)b * NV + i);
    s_sub[g][i] = a;
    __syncthreads();
    if (threadIdx.x < NV) {
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < 16; ++q) s += s_sub[q][threadIdx.x];
        t = s;
    }
    if (threadIdx.x == 0) atomicExch(ticket, 0u);
    return true;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
// Workgroups of a grid-stride launch over M pixels, vec pixels per thread: one workgroup per 256 * vec pixels, at most PX_MAX_WG.
inline int pixel_grid(long M, int vec = 1) {
    const long nblk = (M + (long)PX_TPB * vec - 1) / ((long)PX_TPB * vec);
    return (int)(nblk < PX_MAX_WG ? nblk : PX_MAX_WG);
}

// label_dtype of the C ABI: 0 = int64, 1 = int32, 2 = float32 (reference labels are float tensors cast with .long()).
// ig_label_dispatch calls f(LabelTag<T>{}) for the type the code names and returns what f returns; the entry points reject any other
// code first, each with its own error text (ig_label_dtype_ok).
template <typename T>
struct LabelTag {
    using type = T;
};
template <int V>
using IntTag = std::integral_constant<int, V>;  // a compile-time choice (VEC, NCB, KT ..) handed to a generic lambda: decltype(tag)::value
inline bool ig_label_dtype_ok(int label_dtype) { return label_dtype >= 0 && label_dtype <= 2; }
template <class F>
inline int ig_label_dispatch(int label_dtype, F&& f) {
    if (label_dtype == 0) return f(LabelTag<long long>{});
    if (label_dtype == 1) return f(LabelTag<int>{});
    return f(LabelTag<float>{});
}

}  // namespace
