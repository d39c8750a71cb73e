// Cloud-free temporal composites of HLS scenes for gfx950.  The reference takes one scene per temporal step
// (instageo/data/hls_utils.py: add_hls_stac_items picks the least cloudy granule near the step's date) and masks what Fmask flags in it;
// here the m <= 16 scenes near a step's date become one scene by the rule stated in include/instageo_hip.h (NEAREST, MEDIAN or MEDOID of
// the clear observations), all T steps in one launch.  Results are integers or copies and unique (independent of scheduling).
//
//   composite_kernel<MAXM, CT, METHOD>   a streaming read.  Every plane of every scene is one whole H x W grid, contiguous in its buffer,
//                        so the pixels are taken in plane order and the row pitch never enters: one workgroup of 256 threads per 512
//                        consecutive pixels of one step, a thread owns TWO of them, which travel together as the two 16-bit halves of one
//                        register (a wave reads 256 contiguous bytes of a plane per instruction).  The access width is chosen per plane from
//                        its address: 4 bytes where the pair is 4-byte aligned, else 2 + 2 (a plane may start at any element); the last
//                        workgroup of a plane, where it is short of pixels, goes element by element.  MAXM in {4, 8, 16} is the size of the register arrays and of the
//                        sorting network (the caller's max_m rounded up), CT the number of bands when the values stay in registers.
//                        Phase 1: the m Fmask pairs and (CT > 0) all m * CT value pairs are loaded, every load issued before the first
//                        is used; a candidate is clear where its Fmask passes and none of its values is no_data: two 16-bit masks.
//                        Phase 2, band by band: the keys of the band (a candidate that is not clear becomes 32767: it sorts behind every
//                        clear value, and where it ties with a real 32767 either gives the same value) go through Batcher's odd-even
//                        merge network on packed 16-bit minima / maxima, both pixels per instruction (63 comparators at 16 keys); the
//                        lower median is element (count - 1) >> 1 of the sorted keys.  MEDOID adds |v - median| in 32 bits to the two
//                        distances of every candidate while the band is in registers, takes the earliest smallest clear candidate after
//                        the last band and copies its values out of the registers.  NEAREST copies the first clear candidate's.
//                        CT == 0 (any other number of bands): the register file cannot hold m * C pairs, so phase 1 reads the values for
//                        the no_data test alone and phase 2 reads a band's values again; the winner's values are read a third time.
//                        hist: one LDS cell per count value, LDS atomics, then at most 17 integer atomics per workgroup.
//
// Out-of-range accesses are impossible: a thread touches pixels p < H * W only; a step whose list bounds break 0 <= step_ptr[t] <=
// step_ptr[t + 1] <= N has no candidates, one longer than MAXM is cut to MAXM; every output index is below T * C * H * W.  The caller
// guarantees that starts[k] + H * W and fmask_starts[n] + H * W lie inside the buffers (ops.composite checks it before the upload).
#include "common.h"

namespace {

constexpr int KTPB = 256, KPIX = 2 * KTPB;  // threads, pixels per workgroup
constexpr int KMAX_T = 32, KMAX_M = 16, KCELLS = KMAX_M + 1;
constexpr long KLIM40 = 1L << 40;
enum { NEAREST = 0, MEDIAN = 1, MEDOID = 2 };

struct CompArgs {
    int T, N, C, per, min_clear;
    unsigned bits2, nd2;  // mask_bits in both bytes of a pair of Fmask values; no_data in both halves of a pair of values
    long HW;
};

typedef short s16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned pk_min(unsigned a, unsigned b) {
    return __builtin_bit_cast(unsigned, __builtin_elementwise_min(__builtin_bit_cast(s16x2, a), __builtin_bit_cast(s16x2, b)));
}
__device__ __forceinline__ unsigned pk_max(unsigned a, unsigned b) {
    return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(s16x2, a), __builtin_bit_cast(s16x2, b)));
}

// the pixels p, p + 1 of a plane as one word (low half: p).  fast: wave-uniform, the pair is 4-byte aligned and every thread of the
// workgroup has both pixels; otherwise element by element, and with npx == 1 the high half repeats the low one and is never stored
__device__ __forceinline__ unsigned load_pair(const short* p, int npx, bool fast) {
    if (fast) return *reinterpret_cast<const unsigned*>(p);
    const unsigned lo = (unsigned short)p[0];
    return lo | (npx == 2 ? (unsigned)(unsigned short)p[1] : lo) << 16;
}
__device__ __forceinline__ void store_pair(short* p, unsigned v, int npx, bool fast) {
    if (fast) {
        *reinterpret_cast<unsigned*>(p) = v;
    } else {
        p[0] = (short)(v & 0xffffu);
        if (npx == 2) p[1] = (short)(v >> 16);
    }
}
// two bytes in the low 16 bits (low byte: p); with npx == 1 the second byte is 0
__device__ __forceinline__ unsigned load_bytes(const unsigned char* p, int npx, bool fast) {
    if (fast) return *reinterpret_cast<const unsigned short*>(p);
    return (unsigned)p[0] | (npx == 2 ? (unsigned)p[1] << 8 : 0u);
}
__device__ __forceinline__ void store_bytes(unsigned char* p, unsigned b0, unsigned b1, int npx, bool fast) {
    if (fast) {
        *reinterpret_cast<unsigned short*>(p) = (unsigned short)(b0 | b1 << 8);
    } else {
        p[0] = (unsigned char)b0;
        if (npx == 2) p[1] = (unsigned char)b1;
    }
}
// bit 0: the low half of x differs from no_data, bit 16: the high half does
__device__ __forceinline__ unsigned differs(unsigned x, unsigned nd2) {
    const unsigned y = x ^ nd2;
    return ((y & 0xffffu) ? 1u : 0u) | ((y >> 16) ? 0x10000u : 0u);
}
// whether pixel pairs of the plane that starts `elems` elements after base are aligned to their two elements (wave-uniform)
__device__ __forceinline__ bool pair_aligned(const void* base, long elems, int elem_size) {
    return ((reinterpret_cast<uintptr_t>(base) + (uintptr_t)elems * elem_size) & (2 * elem_size - 1)) == 0;
}

// Batcher's odd-even merge sort of N = 2^k words, ascending in each signed 16-bit half on its own
template <int N>
__device__ __forceinline__ void sort_pairs(unsigned* a) {
#pragma unroll
    for (int p = 1; p < N; p <<= 1) {
#pragma unroll
        for (int k = p; k >= 1; k >>= 1) {
#pragma unroll
            for (int j = k % p; j + k < N; j += 2 * k) {
#pragma unroll
                for (int i = 0; i < k; ++i) {
                    if (i + j + k < N && (i + j) / (2 * p) == (i + j + k) / (2 * p)) {
                        const unsigned lo = pk_min(a[i + j], a[i + j + k]), hi = pk_max(a[i + j], a[i + j + k]);
                        a[i + j] = lo, a[i + j + k] = hi;
                    }
                }
            }
        }
    }
}

template <int MAXM, int CT, int METHOD>
__global__ __launch_bounds__(KTPB, 3) void composite_kernel(const short* __restrict__ bands, const long long* __restrict__ starts,
                                                         const unsigned char* __restrict__ fmasks, const long long* __restrict__ fstarts,
                                                         const int* __restrict__ step_ptr, CompArgs a, short* __restrict__ comp,
                                                         unsigned char* __restrict__ count, unsigned char* __restrict__ source,
                                                         int* __restrict__ hist) {
    __shared__ int cells[KCELLS];
    const int t = blockIdx.x / a.per, blk = blockIdx.x - t * a.per;
    if (threadIdx.x < KCELLS) cells[threadIdx.x] = 0;
    __syncthreads();
    const int n0 = step_ptr[t], n1 = step_ptr[t + 1];
    const int m = (n0 < 0 || n1 < n0 || n1 > a.N) ? 0 : min(n1 - n0, MAXM);
    const int C = CT ? CT : a.C;
    const long pix = 2 * ((long)blk * KTPB + threadIdx.x);
    const int npx = pix + 1 < a.HW ? 2 : pix < a.HW ? 1 : 0;
    const bool full = ((long)blk + 1) * KPIX <= a.HW;  // no thread of the workgroup is short of a pixel
    if (npx) {
        // phase 1: which candidates are clear (bit n: at the first pixel, bit 16 + n: at the second)
        unsigned v[MAXM][CT ? CT : 1], fm[MAXM];
#pragma unroll
        for (int n = 0; n < MAXM; ++n) {
            fm[n] = 0u;
#pragma unroll
            for (int c = 0; c < (CT ? CT : 1); ++c) v[n][c] = a.nd2;  // a candidate the step does not have is never clear
            if (n < m) {
                if (fmasks) {
                    const long long at = fstarts[n0 + n];
                    fm[n] = load_bytes(fmasks + at + pix, npx, full && pair_aligned(fmasks, at, 1));
                }
                if constexpr (CT > 0) {
#pragma unroll
                    for (int c = 0; c < CT; ++c) {
                        const long long at = starts[(long)(n0 + n) * CT + c];
                        v[n][c] = load_pair(bands + at + pix, npx, full && pair_aligned(bands, at, 2));
                    }
                }
            }
        }
        unsigned clr = 0u;
#pragma unroll
        for (int n = 0; n < MAXM; ++n) {
            const unsigned f = fm[n] & a.bits2;
            unsigned ok = ((f & 0xffu) ? 0u : 1u) | ((f >> 8) ? 0u : 0x10000u);
            if constexpr (CT > 0) {
#pragma unroll
                for (int c = 0; c < CT; ++c) ok &= differs(v[n][c], a.nd2);
            } else {
                if (n < m) {
                    for (int c = 0; c < C; ++c) {
                        const long long at = starts[(long)(n0 + n) * C + c];
                        ok &= differs(load_pair(bands + at + pix, npx, full && pair_aligned(bands, at, 2)), a.nd2);
                    }
                } else {
                    ok = 0u;
                }
            }
            clr |= ok << n;
        }
        if (npx == 1) clr &= 0xffffu;
        const int cnt0 = __popc(clr & 0xffffu), cnt1 = __popc(clr >> 16);
        const bool live0 = cnt0 >= a.min_clear, live1 = npx == 2 && cnt1 >= a.min_clear;
        int win0 = 255, win1 = 255;  // the candidate that gives the values (NEAREST, MEDOID)
        if (METHOD == NEAREST) {
            if (live0) win0 = __ffs(clr & 0xffffu) - 1;
            if (live1) win1 = __ffs(clr >> 16) - 1;
        }
        // a word that keeps the halves of the clear pixels: for the keys of a candidate that is not clear
        unsigned keep[MAXM];
#pragma unroll
        for (int n = 0; n < MAXM; ++n) keep[n] = ((clr >> n & 1u) ? 0xffffu : 0u) | ((clr >> (16 + n) & 1u) ? 0xffff0000u : 0u);
        const int k0 = live0 ? (cnt0 - 1) >> 1 : -1, k1 = live1 ? (cnt1 - 1) >> 1 : -1;
        int d0[MAXM], d1[MAXM];
#pragma unroll
        for (int n = 0; n < MAXM; ++n) d0[n] = d1[n] = 0;
        auto put = [&](int c, unsigned pair) {  // band c of the step's composite
            const long at = ((long)t * C + c) * a.HW;
            store_pair(comp + at + pix, pair, npx, full && pair_aligned(comp, at, 2));
        };

        // phase 2: band by band
        if (METHOD != NEAREST) {
            auto band = [&](int c, const unsigned* x) {  // x: the MAXM pairs of band c
                unsigned key[MAXM];
#pragma unroll
                for (int n = 0; n < MAXM; ++n) key[n] = (x[n] & keep[n]) | (0x7fff7fffu & ~keep[n]);
                sort_pairs<MAXM>(key);
                unsigned med = a.nd2;
#pragma unroll
                for (int i = 0; i < (MAXM + 1) / 2; ++i) {
                    if (k0 == i) med = (med & 0xffff0000u) | (key[i] & 0xffffu);
                    if (k1 == i) med = (med & 0xffffu) | (key[i] & 0xffff0000u);
                }
                if (METHOD == MEDIAN) {
                    put(c, med);
                } else {
                    const int m0 = (int)(short)(med & 0xffffu), m1 = (int)med >> 16;
#pragma unroll
                    for (int n = 0; n < MAXM; ++n) {
                        const int e0 = (int)(short)(x[n] & 0xffffu) - m0, e1 = ((int)x[n] >> 16) - m1;
                        d0[n] += e0 < 0 ? -e0 : e0;
                        d1[n] += e1 < 0 ? -e1 : e1;
                    }
                }
            };
            if constexpr (CT > 0) {
#pragma unroll
                for (int c = 0; c < CT; ++c) {
                    unsigned x[MAXM];
#pragma unroll
                    for (int n = 0; n < MAXM; ++n) x[n] = v[n][c];
                    band(c, x);
                }
            } else {
                for (int c = 0; c < C; ++c) {
                    unsigned x[MAXM];
#pragma unroll
                    for (int n = 0; n < MAXM; ++n) {
                        x[n] = a.nd2;
                        if (n < m) {
                            const long long at = starts[(long)(n0 + n) * C + c];
                            x[n] = load_pair(bands + at + pix, npx, full && pair_aligned(bands, at, 2));
                        }
                    }
                    band(c, x);
                }
            }
        }
        if (METHOD == MEDOID) {
            int b0 = 0x7fffffff, b1 = 0x7fffffff;
#pragma unroll
            for (int n = 0; n < MAXM; ++n) {  // ascending: the earliest of the smallest
                if (live0 && (clr >> n & 1u) && d0[n] < b0) b0 = d0[n], win0 = n;
                if (live1 && (clr >> (16 + n) & 1u) && d1[n] < b1) b1 = d1[n], win1 = n;
            }
        }
        if (METHOD != MEDIAN) {  // the winner's values
            if constexpr (CT > 0) {
#pragma unroll
                for (int c = 0; c < CT; ++c) {
                    unsigned out = a.nd2;
#pragma unroll
                    for (int n = 0; n < MAXM; ++n) {
                        if (win0 == n) out = (out & 0xffff0000u) | (v[n][c] & 0xffffu);
                        if (win1 == n) out = (out & 0xffffu) | (v[n][c] & 0xffff0000u);
                    }
                    put(c, out);
                }
            } else {
                for (int c = 0; c < C; ++c) {
                    unsigned out = a.nd2;
                    if (win0 != 255) out = (out & 0xffff0000u) | (unsigned short)bands[starts[(long)(n0 + win0) * C + c] + pix];
                    if (win1 != 255) out = (out & 0xffffu) | (unsigned)(unsigned short)bands[starts[(long)(n0 + win1) * C + c] + pix + 1] << 16;
                    put(c, out);
                }
            }
        }
        store_bytes(count + (long)t * a.HW + pix, (unsigned)cnt0, (unsigned)cnt1, npx, full && pair_aligned(count, (long)t * a.HW, 1));
        store_bytes(source + (long)t * a.HW + pix, (unsigned)win0, (unsigned)win1, npx, full && pair_aligned(source, (long)t * a.HW, 1));
        atomicAdd(&cells[cnt0], 1);
        if (npx == 2) atomicAdd(&cells[cnt1], 1);
    }
    __syncthreads();
    if (threadIdx.x < KCELLS && cells[threadIdx.x]) atomicAdd(hist + t * KCELLS + threadIdx.x, cells[threadIdx.x]);
}

template <int MAXM, int CT>
int launch_method(int method, dim3 grid, hipStream_t st, const short* bands, const long long* starts, const unsigned char* fmasks,
                  const long long* fstarts, const int* step_ptr, const CompArgs& a, short* comp, unsigned char* count, unsigned char* source,
                  int* hist) {
    if (method == NEAREST)
        return ig_launch<composite_kernel<MAXM, CT, NEAREST>>("ig_composite", grid, dim3(KTPB), 0, st, bands, starts, fmasks, fstarts, step_ptr, a,
                                                              comp, count, source, hist);
    if (method == MEDIAN)
        return ig_launch<composite_kernel<MAXM, CT, MEDIAN>>("ig_composite", grid, dim3(KTPB), 0, st, bands, starts, fmasks, fstarts, step_ptr, a,
                                                             comp, count, source, hist);
    return ig_launch<composite_kernel<MAXM, CT, MEDOID>>("ig_composite", grid, dim3(KTPB), 0, st, bands, starts, fmasks, fstarts, step_ptr, a, comp,
                                                         count, source, hist);
}

template <int CT>
int launch_size(int max_m, int method, dim3 grid, hipStream_t st, const short* bands, const long long* starts, const unsigned char* fmasks,
                const long long* fstarts, const int* step_ptr, const CompArgs& a, short* comp, unsigned char* count, unsigned char* source,
                int* hist) {
    if (max_m <= 4) return launch_method<4, CT>(method, grid, st, bands, starts, fmasks, fstarts, step_ptr, a, comp, count, source, hist);
    if (max_m <= 8) return launch_method<8, CT>(method, grid, st, bands, starts, fmasks, fstarts, step_ptr, a, comp, count, source, hist);
    return launch_method<16, CT>(method, grid, st, bands, starts, fmasks, fstarts, step_ptr, a, comp, count, source, hist);
}

}  // namespace

extern "C" int ig_composite(const short* bands, const long long* starts, const unsigned char* fmasks, const long long* fmask_starts,
                            const int* step_ptr, int T, int N, int max_m, int C, int H, int W, int mask_bits, int no_data, int min_clear,
                            int method, short* composite, unsigned char* count, unsigned char* source, int* hist, void* stream) {
    IG_REQUIRE(T >= 0 && T <= KMAX_T, "ig_composite: 0 <= T <= %d steps (got %d)", KMAX_T, T);
    IG_REQUIRE(max_m >= 0 && max_m <= KMAX_M, "ig_composite: a step has 0 <= m <= %d candidates (got max_m = %d)", KMAX_M, max_m);
    IG_REQUIRE(N >= 0 && N <= T * max_m, "ig_composite: N = %d candidates in all do not go with %d steps of at most %d", N, T, max_m);
    IG_REQUIRE(C >= 1 && C <= 32767, "ig_composite: need 1 <= C <= 32767 bands (got %d)", C);
    IG_REQUIRE(H >= 0 && W >= 0, "ig_composite: need H >= 0 and W >= 0 (H %d, W %d)", H, W);
    const long HW = (long)H * W;
    IG_REQUIRE(HW <= 0x7fffffffL, "ig_composite: H * W = %ld pixels exceeds 2^31 - 1", HW);
    IG_REQUIRE(mask_bits >= 0 && mask_bits <= 255, "ig_composite: mask_bits must be a byte (got %d)", mask_bits);
    IG_REQUIRE(no_data >= -32768 && no_data <= 32767, "ig_composite: no_data must fit int16 (got %d)", no_data);
    IG_REQUIRE(min_clear >= 1 && min_clear <= KMAX_M, "ig_composite: need 1 <= min_clear <= %d (got %d)", KMAX_M, min_clear);
    IG_REQUIRE(method >= NEAREST && method <= MEDOID, "ig_composite: method must be 0 nearest, 1 median or 2 medoid (got %d)", method);
    if (HW == 0 || T == 0) return IG_OK;
    IG_REQUIRE((long)T * C * HW < KLIM40, "ig_composite: T * C * H * W = %ld values exceeds 2^40", (long)T * C * HW);
    IG_REQUIRE(step_ptr && composite && count && source && hist, "ig_composite: null pointer");
    IG_REQUIRE(N == 0 || (bands && starts), "ig_composite: null pointer (bands, starts)");
    IG_REQUIRE((fmasks == nullptr) == (fmask_starts == nullptr) || N == 0, "ig_composite: fmasks and fmask_starts go together");
    IG_REQUIRE((((uintptr_t)bands | (uintptr_t)composite) & 1) == 0 && (((uintptr_t)step_ptr | (uintptr_t)hist) & 3) == 0 &&
                   (((uintptr_t)starts | (uintptr_t)fmask_starts) & 7) == 0,
               "ig_composite: bands and composite must be 2-byte, step_ptr and hist 4-byte, starts and fmask_starts 8-byte aligned");
    const int per = ig_cdiv(HW, KPIX);
    const unsigned nd = (unsigned short)(short)no_data;
    const CompArgs a{T, N, C, per, min_clear, (unsigned)mask_bits * 0x0101u, nd | nd << 16, HW};
    const dim3 grid((unsigned)((long)per * T));
    hipStream_t st = (hipStream_t)stream;
    if (N == 0) fmasks = nullptr;
#define IG_COMPOSITE_BANDS(CT) \
    if (C == CT) return launch_size<CT>(max_m, method, grid, st, bands, starts, fmasks, fmask_starts, step_ptr, a, composite, count, source, hist)
    IG_COMPOSITE_BANDS(1);
    IG_COMPOSITE_BANDS(2);
    IG_COMPOSITE_BANDS(3);
    IG_COMPOSITE_BANDS(4);
    IG_COMPOSITE_BANDS(6);
#undef IG_COMPOSITE_BANDS
    return launch_size<0>(max_m, method, grid, st, bands, starts, fmasks, fmask_starts, step_ptr, a, composite, count, source, hist);
}
