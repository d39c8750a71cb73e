// Mosaic of per-chip rasters on one canvas for gfx950.  The reference runs gdal_merge.py over the prediction folder
// (new_apps/backend/app/cog_converter.py); this is the paste with its overlap rule, stated in include/instageo_hip.h, as a GATHER: every
// canvas pixel is computed by the one thread that stores it, from the chips that cover it in chip order.  No atomics, no waiting between
// workgroups, every result unique (independent of scheduling).
//
//   mosaic_kernel<T, RULE>   one workgroup of 256 threads per 64 x 64 block of the canvas (origin at multiples of 64: the blocking of
//                            cog.hip).  The block's chip list (CSR: bin_ptr / bin_idx, ascending chip indices, built by the host) is
//                            staged through LDS in chunks of 256 entries; a list that fits one chunk is staged once.  A thread owns 16
//                            consecutive pixels of one row and stores them once.  last walks the list backwards and first forwards, both
//                            until all 16 pixels are set (the workgroup leaves a chunked list when all its threads are done); mean walks
//                            forwards once; mode re-walks the list once per distinct value in ascending order, so ties go to the smallest.
//
// Out-of-range accesses are impossible as long as starts[i] + h * w lies inside the packed buffer (the caller's promise, checked by
// ops.mosaic_paste): a chip index outside [0, nchips) or a rectangle outside the stated bounds is staged as an empty rectangle, every chip
// load is guarded by row < h and column < w (the 16-byte path runs only where the whole segment lies inside the chip row and its address
// is 16-byte aligned), every store by row < H and column < W.
#include "common.h"

namespace {

constexpr int MB = 64, MTPB = 256, MSEG = 16, MCH = 256;  // block side, threads, pixels per thread, list entries per LDS chunk
constexpr int MLIM = 1 << 30;  // |row0|, |col0|, h, w at most this: differences of coordinates stay inside int32
constexpr int R_LAST = 0, R_FIRST = 1, R_MODE = 2, R_MEAN = 3;

struct Chunk {
    long long start[MCH];
    int r0[MCH], c0[MCH], h[MCH], w[MCH];
};

struct Src {
    const long long* starts;
    const int* rects;
    const int* idx;  // the block's list
    int nchips, n, vec;
};

__device__ __forceinline__ bool clear_px(signed char v, int fill) { return v == (signed char)fill; }
__device__ __forceinline__ bool clear_px(float v, int) { return v != v; }

__device__ __forceinline__ void stage(Chunk& s, int slot, int ci, const Src& src) {
    int r0 = 0, c0 = 0, h = 0, w = 0;  // h = 0: covers nothing
    long long st = 0;
    if ((unsigned)ci < (unsigned)src.nchips) {
        const int4 r = *reinterpret_cast<const int4*>(src.rects + 4 * (long)ci);
        st = src.starts[ci];
        if (r.z >= 1 && r.w >= 1 && r.z <= MLIM && r.w <= MLIM && r.x >= -MLIM && r.x <= MLIM && r.y >= -MLIM && r.y <= MLIM && st >= 0)
            r0 = r.x, c0 = r.y, h = r.z, w = r.w;
    }
    s.start[slot] = st, s.r0[slot] = r0, s.c0[slot] = c0, s.h[slot] = h, s.w[slot] = w;
}

// The contributors of the thread's 16 pixels (row gr, columns gc .. gc + 15) in list order (BACK: reversed): visit(j, value) for every
// pixel j a chip covers with a value that is not transparent.  done() ends the thread's walk early; a chunked list is left by the whole
// workgroup once done() holds for all its threads.  Barriers are reached by every thread: callers pass done() = true for idle threads.
template <typename T, bool BACK, typename V, typename D>
__device__ __forceinline__ void walk(Chunk& s, const T* __restrict__ chips, const Src& src, int gr, int gc, int fill, V visit, D done) {
    const bool resident = src.n <= MCH;  // staged once by the kernel
    for (int pos = 0; pos < src.n; pos += MCH) {
        const int len = min(MCH, src.n - pos), lo = BACK ? src.n - pos - len : pos;
        if (!resident) {
            if (__syncthreads_and(done())) break;  // and: everyone has finished with the previous chunk
            if ((int)threadIdx.x < len) stage(s, threadIdx.x, src.idx[lo + threadIdx.x], src);
            __syncthreads();
        }
        for (int i = 0; i < len && !done(); ++i) {
            const int e = BACK ? len - 1 - i : i;
            const int rr = gr - s.r0[e], w = s.w[e], cc = gc - s.c0[e];  // the chip's row, and its column under pixel 0
            if ((unsigned)rr >= (unsigned)s.h[e] || cc >= w || cc + MSEG <= 0) continue;
            const long off = s.start[e] + (long)rr * w + cc;
            T v[MSEG];
            if (src.vec && cc >= 0 && cc + MSEG <= w && (reinterpret_cast<uintptr_t>(chips + off) & 15) == 0) {
#pragma unroll
                for (int q = 0; q < MSEG * (int)sizeof(T) / 16; ++q) {
                    const uint4 u = *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(chips + off) + 16 * q);
                    __builtin_memcpy(reinterpret_cast<char*>(v) + 16 * q, &u, 16);
                }
#pragma unroll
                for (int j = 0; j < MSEG; ++j)
                    if (!clear_px(v[j], fill)) visit(j, v[j]);
            } else {
#pragma unroll
                for (int j = 0; j < MSEG; ++j)
                    if ((unsigned)(cc + j) < (unsigned)w) {
                        const T x = chips[off + j];
                        if (!clear_px(x, fill)) visit(j, x);
                    }
            }
        }
    }
}

template <typename T, int RULE>
__global__ __launch_bounds__(MTPB) void mosaic_kernel(const T* __restrict__ chips, const long long* __restrict__ starts,
                                                      const int* __restrict__ rects, int nchips, const int* __restrict__ bin_ptr,
                                                      const int* __restrict__ bin_idx, int H, int W, int fill, int vec_load, int vec_store,
                                                      int vec_cover, T* __restrict__ dst, unsigned char* __restrict__ cover) {
    __shared__ Chunk s;
    const int b = blockIdx.y * gridDim.x + blockIdx.x;
    const int first = bin_ptr ? bin_ptr[b] : 0;
    Src src{starts, rects, bin_idx + first, nchips, bin_ptr ? max(bin_ptr[b + 1] - first, 0) : 0, vec_load};
    if (src.n <= MCH) {
        if ((int)threadIdx.x < src.n) stage(s, threadIdx.x, src.idx[threadIdx.x], src);
        __syncthreads();
    }
    const int gr = blockIdx.y * MB + (threadIdx.x >> 2), gc = blockIdx.x * MB + (threadIdx.x & 3) * MSEG;
    const bool idle = gr >= H || gc >= W;
    const bool count = cover != nullptr;
    T out[MSEG];
    int tot[MSEG];
#pragma unroll
    for (int j = 0; j < MSEG; ++j) tot[j] = 0;

    if constexpr (RULE == R_LAST || RULE == R_FIRST) {
        unsigned open = idle ? 0u : (gc + MSEG <= W ? 0xffffu : (1u << (W - gc)) - 1u);  // the pixels inside the canvas still without a value
#pragma unroll
        for (int j = 0; j < MSEG; ++j) {
            if constexpr (sizeof(T) == 1) out[j] = (T)fill;
            else out[j] = __uint_as_float(0x7fc00000u);
        }
        auto visit = [&](int j, T v) {
            if (open >> j & 1u) out[j] = v, open &= ~(1u << j);
            tot[j] += 1;
        };
        auto done = [&]() { return idle || (!count && open == 0u); };
        walk<T, RULE == R_LAST>(s, chips, src, gr, gc, fill, visit, done);
    } else if constexpr (RULE == R_MEAN) {
        float sum[MSEG];
#pragma unroll
        for (int j = 0; j < MSEG; ++j) sum[j] = 0.f;
        auto visit = [&](int j, float v) {
            sum[j] = tot[j] ? sum[j] + v : v;
            tot[j] += 1;
        };
        walk<T, false>(s, chips, src, gr, gc, fill, visit, [&]() { return idle; });
#pragma unroll
        for (int j = 0; j < MSEG; ++j) out[j] = tot[j] ? __fdiv_rn(sum[j], (float)tot[j]) : __uint_as_float(0x7fc00000u);
    } else {  // R_MODE: one walk per candidate value, ascending; the first walk (no candidate yet) finds the smallest value and counts
        int cand[MSEG], best[MSEG], bestn[MSEG];
#pragma unroll
        for (int j = 0; j < MSEG; ++j) cand[j] = -129, best[j] = fill, bestn[j] = 0;
        bool live = !idle;
        for (int pass = 0;; ++pass) {
            int nxt[MSEG], cnt[MSEG];
#pragma unroll
            for (int j = 0; j < MSEG; ++j) nxt[j] = 128, cnt[j] = 0;
            const int one = pass == 0;
            auto visit = [&](int j, signed char v) {
                const int x = v;
                cnt[j] += x == cand[j];
                if (x > cand[j] && x < nxt[j]) nxt[j] = x;
                tot[j] += one;
            };
            walk<T, false>(s, chips, src, gr, gc, fill, visit, [&]() { return !live; });
            bool more = false;
#pragma unroll
            for (int j = 0; j < MSEG; ++j) {
                if (cnt[j] > bestn[j]) best[j] = cand[j], bestn[j] = cnt[j];  // strictly more: a tie stays with the smaller value
                cand[j] = nxt[j];
                more |= nxt[j] != 128;
            }
            live = live && more;
            if (!__syncthreads_or(live)) break;
        }
#pragma unroll
        for (int j = 0; j < MSEG; ++j) out[j] = (T)best[j];
    }
    if (idle) return;
    const long at = (long)gr * W + gc;
    const bool whole = gc + MSEG <= W;
    if (vec_store && whole) {
#pragma unroll
        for (int q = 0; q < MSEG * (int)sizeof(T) / 16; ++q) {
            uint4 u;
            __builtin_memcpy(&u, reinterpret_cast<const char*>(out) + 16 * q, 16);
            *reinterpret_cast<uint4*>(reinterpret_cast<char*>(dst + at) + 16 * q) = u;
        }
    } else {
#pragma unroll
        for (int j = 0; j < MSEG; ++j)
            if (gc + j < W) dst[at + j] = out[j];
    }
    if (count) {
        unsigned char cv[MSEG];
#pragma unroll
        for (int j = 0; j < MSEG; ++j) cv[j] = (unsigned char)min(tot[j], 255);
        if (vec_cover && whole) {
            uint4 u;
            __builtin_memcpy(&u, cv, 16);
            *reinterpret_cast<uint4*>(cover + at) = u;
        } else {
#pragma unroll
            for (int j = 0; j < MSEG; ++j)
                if (gc + j < W) cover[at + j] = cv[j];
        }
    }
}

template <typename T, int RULE>
int launch(const void* chips, const long long* starts, const int* rects, int nchips, const int* bin_ptr, const int* bin_idx, int H, int W, int fill,
           void* dst, unsigned char* cover, void* stream) {
    constexpr int per16 = 16 / (int)sizeof(T);  // elements in 16 bytes: dst is 16-byte aligned, so every row is iff W is a multiple
    const int vec_load = ig_env_int("IG_MOSAIC_VEC", 1) != 0;
    const int vec_store = W % per16 == 0, vec_cover = W % 16 == 0 && ((uintptr_t)cover & 15) == 0;
    return ig_launch<mosaic_kernel<T, RULE>>("ig_mosaic_paste", dim3((unsigned)ig_cdiv(W, MB), (unsigned)ig_cdiv(H, MB)), dim3(MTPB), 0,
                                             (hipStream_t)stream, (const T*)chips, starts, rects, nchips, bin_ptr, bin_idx, H, W, fill, vec_load,
                                             vec_store, vec_cover, (T*)dst, cover);
}

}  // namespace

extern "C" int ig_mosaic_paste(const void* chips, const long long* starts, const int* rects, int nchips, const int* bin_ptr, const int* bin_idx,
                               int H, int W, int elem_size, int rule, int fill, void* dst, unsigned char* cover, void* stream) {
    IG_REQUIRE(elem_size == 1 || elem_size == 4, "ig_mosaic_paste: elem_size must be 1 (int8) or 4 (float32) (got %d)", elem_size);
    IG_REQUIRE(rule >= R_LAST && rule <= R_MEAN, "ig_mosaic_paste: rule must be 0 last, 1 first, 2 mode or 3 mean (got %d)", rule);
    IG_REQUIRE(rule != R_MODE || elem_size == 1, "ig_mosaic_paste: rule mode needs int8 class maps (elem_size %d)", elem_size);
    IG_REQUIRE(rule != R_MEAN || elem_size == 4, "ig_mosaic_paste: rule mean needs float32 rasters (elem_size %d)", elem_size);
    IG_REQUIRE(fill >= -128 && fill <= 127, "ig_mosaic_paste: fill must fit int8 (got %d)", fill);
    IG_REQUIRE(H >= 0 && W >= 0, "ig_mosaic_paste: need H >= 0 and W >= 0 (H %d, W %d)", H, W);
    IG_REQUIRE((long)H * W <= 0x7fffffffL, "ig_mosaic_paste: H * W = %ld exceeds 2^31 - 1", (long)H * W);
    IG_REQUIRE(nchips >= 0, "ig_mosaic_paste: need nchips >= 0 (got %d)", nchips);
    if ((long)H * W == 0) return IG_OK;
    IG_REQUIRE(ig_cdiv(H, MB) <= 65535, "ig_mosaic_paste: H = %d exceeds 65535 blocks of 64 rows", H);
    IG_REQUIRE(dst, "ig_mosaic_paste: null pointer (dst)");
    IG_REQUIRE(((uintptr_t)dst & 15) == 0, "ig_mosaic_paste: dst must be 16-byte aligned");
    if (nchips > 0) {
        IG_REQUIRE(chips && starts && rects && bin_ptr && bin_idx, "ig_mosaic_paste: null pointer");
        IG_REQUIRE(((uintptr_t)chips & (elem_size - 1)) == 0, "ig_mosaic_paste: chips must be aligned to its elements");
        IG_REQUIRE(((uintptr_t)rects & 15) == 0 && ((uintptr_t)starts & 7) == 0 && (((uintptr_t)bin_ptr | (uintptr_t)bin_idx) & 3) == 0,
                   "ig_mosaic_paste: rects must be 16-byte, starts 8-byte, bin_ptr and bin_idx 4-byte aligned");
    } else {
        bin_ptr = nullptr;  // every block's list is empty: the canvas becomes fill
    }
#define MOSAIC(T, R) return launch<T, R>(chips, starts, rects, nchips, bin_ptr, bin_idx, H, W, fill, dst, cover, stream)
    if (elem_size == 1) {
        if (rule == R_LAST) MOSAIC(signed char, R_LAST);
        if (rule == R_FIRST) MOSAIC(signed char, R_FIRST);
        MOSAIC(signed char, R_MODE);
    }
    if (rule == R_LAST) MOSAIC(float, R_LAST);
    if (rule == R_FIRST) MOSAIC(float, R_FIRST);
    MOSAIC(float, R_MEAN);
#undef MOSAIC
}
