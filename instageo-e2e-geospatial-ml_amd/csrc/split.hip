// Spatially blocked dataset splitting for gfx950.  The reference clusters chip locations with sklearn's k-means on the
// host (instageo/data/data_splitter.py) and never looks at what it produced; here the rule, stated in include/instageo_hip.h, works on
// unit vectors quantised to int32 and runs as two integer kernels whose results are unique (independent of scheduling).
//
//   split_assign_kernel    one Lloyd round.  One workgroup of 256 threads per 2048 consecutive points; the K centres sit in LDS as int4.
//                          A thread owns 8 points (i = block base + k * 256 + lane, so a wave reads 768 contiguous bytes per step), walks
//                          the centres for each (3 subtractions, 3 multiply-adds into a 64-bit sum, strict <: the smallest centre index
//                          wins a tie), and keeps the coordinate sums of a run of points with one centre in registers; a run is added to
//                          the centre's four 64-bit cells in LDS with integer atomics when the centre changes.  After the barrier the
//                          non-zero cells go to HBM with 64-bit integer atomics, and the changed count with one 32-bit atomic.
//   split_nearest_kernel   one workgroup per (block of 256 * RA rows of a, contiguous range of b).  A thread holds RA rows of a in
//                          registers; the range of b is staged through LDS in tiles of 1024 points (int4, 16 KB) and every thread reads the
//                          same point at the same time (a broadcast: no bank conflict).  b is walked in ascending index and the comparison
//                          is strict, so the first minimum is the smallest index.  With one range the results are final; with more they go
//                          to a scratch buffer (range-major) and
//   split_merge_kernel     takes, per row of a, the candidates of the ranges in ascending order with the same strict comparison.
//
// Out-of-range accesses are impossible: a point index is guarded by i < N (or < Na, < the end of the range <= Nb) before every global
// access, the LDS tile is read below the number of points staged, a centre index is < K <= 256, and coordinate differences are taken
// modulo 2^32, so even coordinates outside +-2^29 only give a meaningless distance.  Nothing here is floating point.
#include <algorithm>

#include "common.h"
#include "pixel_seg.h"

namespace {

constexpr int TPB = 256, PPT = 8, MAX_K = 256;  // threads, points per thread of the assign kernel, centres
constexpr int TB = 1024;                        // points of b per LDS tile
constexpr int LIMN = 1 << 30;
typedef unsigned long long u64;

__device__ __forceinline__ u64 dist2(int ax, int ay, int az, int bx, int by, int bz) {
    const int dx = (int)((unsigned)ax - (unsigned)bx), dy = (int)((unsigned)ay - (unsigned)by), dz = (int)((unsigned)az - (unsigned)bz);
    return (u64)((long long)dx * dx) + (u64)((long long)dy * dy) + (u64)((long long)dz * dz);
}

__global__ __launch_bounds__(TPB) void split_assign_kernel(const int* __restrict__ pts, int N, const int* __restrict__ centres, int K,
                                                           int* __restrict__ assign, u64* __restrict__ sums, int* __restrict__ changed) {
    __shared__ int4 cen[MAX_K];
    __shared__ u64 cell[MAX_K * 4];
    __shared__ int part[4];
    for (int k = threadIdx.x; k < K; k += TPB) cen[k] = make_int4(centres[3 * k], centres[3 * k + 1], centres[3 * k + 2], 0);
    for (int k = threadIdx.x; k < 4 * K; k += TPB) cell[k] = 0ull;
    __syncthreads();
    const long base = (long)blockIdx.x * (TPB * PPT) + threadIdx.x;
    int run = -1, moved = 0;  // the centre of the run of points held in registers
    long long sx = 0, sy = 0, sz = 0, cnt = 0;
    auto flush = [&]() {
        if (run >= 0) {
            atomicAdd(&cell[4 * run], (u64)sx), atomicAdd(&cell[4 * run + 1], (u64)sy);
            atomicAdd(&cell[4 * run + 2], (u64)sz), atomicAdd(&cell[4 * run + 3], (u64)cnt);
        }
    };
    for (int k = 0; k < PPT; ++k) {
        const long i = base + (long)k * TPB;
        if (i >= N) break;
        const int px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];
        u64 best = dist2(px, py, pz, cen[0].x, cen[0].y, cen[0].z);
        int bi = 0;
        for (int c = 1; c < K; ++c) {
            const int4 q = cen[c];
            const u64 d = dist2(px, py, pz, q.x, q.y, q.z);
            if (d < best) best = d, bi = c;
        }
        moved += assign[i] != bi;
        assign[i] = bi;
        if (bi != run) {
            flush();
            run = bi, sx = sy = sz = cnt = 0;
        }
        sx += px, sy += py, sz += pz, ++cnt;
    }
    flush();
    const int total = block_sum_int(moved, part);  // its barrier also orders the cells
    if (threadIdx.x == 0 && total) atomicAdd(changed, total);
    for (int k = threadIdx.x; k < 4 * K; k += TPB)
        if (cell[k]) atomicAdd(sums + k, cell[k]);
}

// grid: blockIdx.x = range of b * nblocks_a + block of a.  out_d2 / out_idx: (ranges, Na), range-major (the final arrays with one range).
template <int RA>
__global__ __launch_bounds__(TPB) void split_nearest_kernel(const int* __restrict__ a, int Na, const int* __restrict__ b, int Nb, int nblocks_a,
                                                            int per_range, u64* __restrict__ out_d2, int* __restrict__ out_idx) {
    __shared__ int4 tile[TB];
    const int range = blockIdx.x / nblocks_a, blk = blockIdx.x - range * nblocks_a;
    const long first = (long)range * per_range, last = min(first + (long)per_range, (long)Nb);  // this workgroup's points of b
    const long row0 = (long)blk * (TPB * RA) + threadIdx.x;
    int ax[RA], ay[RA], az[RA], bi[RA];
    u64 best[RA];
#pragma unroll
    for (int r = 0; r < RA; ++r) {
        const long i = row0 + (long)r * TPB;
        const bool live = i < Na;
        ax[r] = live ? a[3 * i] : 0, ay[r] = live ? a[3 * i + 1] : 0, az[r] = live ? a[3 * i + 2] : 0;
        best[r] = ~0ull, bi[r] = 0;  // every range holds at least one point and d2 <= 3 * 2^60 < 2^64 - 1: always replaced
    }
    for (long j0 = first; j0 < last; j0 += TB) {
        const int n = (int)min((long)TB, last - j0);
        __syncthreads();  // the previous tile has been read by every thread
        for (int t = threadIdx.x; t < n; t += TPB) {
            const long j = j0 + t;
            tile[t] = make_int4(b[3 * j], b[3 * j + 1], b[3 * j + 2], 0);
        }
        __syncthreads();
#pragma unroll 4
        for (int t = 0; t < n; ++t) {
            const int4 q = tile[t];
#pragma unroll
            for (int r = 0; r < RA; ++r) {
                const u64 d = dist2(ax[r], ay[r], az[r], q.x, q.y, q.z);
                if (d < best[r]) best[r] = d, bi[r] = (int)j0 + t;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < RA; ++r) {
        const long i = row0 + (long)r * TPB;
        if (i < Na) out_d2[(long)range * Na + i] = best[r], out_idx[(long)range * Na + i] = bi[r];
    }
}

__global__ __launch_bounds__(TPB) void split_merge_kernel(const u64* __restrict__ part_d2, const int* __restrict__ part_idx, int Na, int ranges,
                                                          u64* __restrict__ d2, int* __restrict__ idx) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= Na) return;
    u64 best = part_d2[i];
    int bi = part_idx[i];
    for (int s = 1; s < ranges; ++s) {  // ascending ranges hold ascending indices: strict < keeps the smallest index
        const u64 d = part_d2[(long)s * Na + i];
        if (d < best) best = d, bi = part_idx[(long)s * Na + i];
    }
    d2[i] = best, idx[i] = bi;
}

}  // namespace

extern "C" int ig_split_assign(const int* pts, int N, const int* centres, int K, int* assign, long long* sums, int* changed, void* stream) {
    IG_REQUIRE(N >= 0 && N < LIMN, "ig_split_assign: need 0 <= N < 2^30 points (got %d)", N);
    IG_REQUIRE(K >= 1 && K <= MAX_K, "ig_split_assign: need 1 <= K <= %d centres (got %d)", MAX_K, K);
    if (N == 0) return IG_OK;
    IG_REQUIRE(pts && centres && assign && sums && changed, "ig_split_assign: null pointer");
    IG_REQUIRE((((uintptr_t)pts | (uintptr_t)centres | (uintptr_t)assign | (uintptr_t)changed) & 3) == 0 && ((uintptr_t)sums & 7) == 0,
               "ig_split_assign: pts, centres, assign and changed must be 4-byte, sums 8-byte aligned");
    return ig_launch<split_assign_kernel>("ig_split_assign", dim3((unsigned)ig_cdiv(N, TPB * PPT)), dim3(TPB), 0, (hipStream_t)stream, pts, N,
                                          centres, K, assign, (u64*)sums, changed);
}

extern "C" int ig_split_nearest(const int* a, int Na, const int* b, int Nb, unsigned long long* d2, int* idx, void* stream) {
    IG_REQUIRE(Na >= 0 && Na < LIMN, "ig_split_nearest: need 0 <= Na < 2^30 rows (got %d)", Na);
    IG_REQUIRE(Nb >= 1 && Nb < LIMN, "ig_split_nearest: need 1 <= Nb < 2^30 rows to search (got %d)", Nb);
    if (Na == 0) return IG_OK;
    IG_REQUIRE(a && b && d2 && idx, "ig_split_nearest: null pointer");
    IG_REQUIRE((((uintptr_t)a | (uintptr_t)b | (uintptr_t)idx) & 3) == 0 && ((uintptr_t)d2 & 7) == 0,
               "ig_split_nearest: a, b and idx must be 4-byte, d2 8-byte aligned");
    const hipStream_t st = (hipStream_t)stream;
    const int RA = Na >= 4 * TPB ? 4 : 1;
    const int nblocks_a = ig_cdiv(Na, TPB * RA), tiles = ig_cdiv(Nb, TB);
    // enough workgroups for four per compute unit: b is cut when the blocks of a alone are fewer; a range is a whole number of tiles
    const int want = std::max(1, std::min(tiles, 4 * ig_cu_count() / nblocks_a));
    const int per_range = ig_cdiv(tiles, want) * TB;
    const int ranges = ig_cdiv(Nb, per_range);
    u64* out_d2 = d2;
    int* out_idx = idx;
    if (ranges > 1) {
        const size_t cells = (size_t)ranges * Na;
        char* buf = (char*)ig_scratch(IG_SLOT_SPLIT_NEAREST, cells * 12, st);
        if (!buf) {
            ig_set_error("ig_split_nearest: cannot allocate %zu bytes of scratch for %d ranges of b", cells * 12, ranges);
            return IG_ERR_HIP;
        }
        out_d2 = (u64*)buf, out_idx = (int*)(buf + cells * 8);
    }
    const dim3 grid((unsigned)((long)nblocks_a * ranges));
    ig_note_kernel(ranges > 1 ? "split_nearest_kernel<%d>+split_merge_kernel" : "split_nearest_kernel<%d>", RA);
    ig_note_grid((int)grid.x);
    const int rc = RA == 4 ? ig_launch<split_nearest_kernel<4>>("ig_split_nearest", grid, dim3(TPB), 0, st, a, Na, b, Nb, nblocks_a, per_range,
                                                                 out_d2, out_idx)
                           : ig_launch<split_nearest_kernel<1>>("ig_split_nearest", grid, dim3(TPB), 0, st, a, Na, b, Nb, nblocks_a, per_range,
                                                                 out_d2, out_idx);
    if (rc != IG_OK || ranges == 1) return rc;
    return ig_launch<split_merge_kernel>("ig_split_nearest", dim3((unsigned)ig_cdiv(Na, TPB)), dim3(TPB), 0, st, (const u64*)out_d2,
                                         (const int*)out_idx, Na, ranges, d2, idx);
}
