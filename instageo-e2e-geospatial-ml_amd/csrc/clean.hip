// Dataset cleaning for gfx950.  The reference cleans a chip dataset file by file with numpy on the host
// (instageo/data/data_cleaner.py: should_drop_chip, buffer_observation_pixels, limit_seg_map_to_observation_pixels); here the rule, stated
// in include/instageo_hip.h, runs as three batched kernels whose results are integers or bit copies and unique (independent of scheduling).
//
//   chip_nodata_kernel    one workgroup of 256 threads per 2048 consecutive pixels of one chip's plane; a thread owns 8 of them and walks
//                         the B bands (load, compare with the 16-bit pattern, OR into any, AND into all), then writes its 8 plane bytes once.
//                         The access width of every segment is chosen from its address (16 / 8 / 4 / 2 bytes): with H * W odd every second
//                         band starts 2-byte aligned.  The segment that crosses the end of the plane goes element by element.  counts: wave
//                         shuffle, LDS across the 4 waves, one integer atomic pair per workgroup.
//   label_buffer_kernel   one workgroup per 64 x 64 block of one map.  Source flags of the block plus a halo of w as bytes in LDS (outside
//                         the map: 0); row pass: for every staged row and block column the right-most flagged staged column within +-w, or
//                         -1; column pass per output pixel: the bottom-most staged row within +-w with a hit.  A thread resolves 16 pixels:
//                         the winner's value from global memory, the plane's bit 1, one store; valid_labels and the class histogram are
//                         tallied in LDS and added with integer atomics.
//   label_limit_kernel    the same block ownership with a 4096-bit mask in LDS; a thread takes every 256th point of the map's list and sets
//                         the bit of a point inside the block with an LDS atomic OR.
//
// Out-of-range accesses are impossible: every pixel access is guarded by row < H and column < W (or pixel < H * W), a staged pixel outside
// the map is never read, a winner is a staged pixel that was read, the list bounds of a map are clamped to [0, P], a point outside the map
// or the block sets no bit, and a value outside [0, K) is not counted.
#include "common.h"
#include "pixel_seg.h"

namespace {

constexpr int NSEG = 8, NTPB = 256, NPIX = NSEG * NTPB;  // pixels per thread, threads, pixels per workgroup
constexpr int LB = 64, LTPB = 256, MAX_K = 256;          // label block side, threads, histogram cells
constexpr int MAX_W = 32, STG = LB + 2 * MAX_W;          // window half-width, staged side at the largest window
constexpr long LIM40 = 1L << 40;

__global__ __launch_bounds__(NTPB) void chip_nodata_kernel(const unsigned short* __restrict__ chips, int B, int HW, int per,
                                                           unsigned short nd, unsigned char* __restrict__ plane, int* __restrict__ counts) {
    __shared__ int part_any[4], part_all[4];
    const int chip = blockIdx.x / per, blk = blockIdx.x - chip * per;
    const long p0 = (long)blk * NPIX + (long)threadIdx.x * NSEG;  // the first of the thread's pixels in the plane
    const bool live = p0 < HW;
    const bool whole = live && p0 + NSEG <= HW;
    const int npx = live ? (int)min((long)NSEG, HW - p0) : 0;
    unsigned any = 0u, all = 0u;  // bit j: pixel j
    if (live) {
        all = (1u << npx) - 1u;
        const unsigned short* p = chips + (long)chip * B * HW + p0;
        for (int b = 0; b < B; ++b, p += HW) {
            unsigned short v[NSEG];
            if (whole) {
                load_seg<2 * NSEG>(p, v);
            } else {
#pragma unroll
                for (int j = 0; j < NSEG; ++j) v[j] = j < npx ? p[j] : (unsigned short)~nd;
            }
            unsigned eq = 0u;
#pragma unroll
            for (int j = 0; j < NSEG; ++j) eq |= v[j] == nd ? 1u << j : 0u;
            any |= eq, all &= eq;
        }
        unsigned char m[NSEG];
#pragma unroll
        for (int j = 0; j < NSEG; ++j) m[j] = (unsigned char)((any >> j & 1u) | (all >> j & 1u) << 1);
        store_run<NSEG>(plane + (long)chip * HW + p0, whole, npx, m);
    }
    const int n_any = block_sum_int(__popc(any), part_any), n_all = block_sum_int(__popc(all), part_all);
    if (threadIdx.x == 0) {
        if (n_any) atomicAdd(counts + 2 * chip, n_any);
        if (n_all) atomicAdd(counts + 2 * chip + 1, n_all);
    }
}

// the pixels of one 64 x 64 block resolved: value(i, r, c, at) gives the output value of pixel (r, c) at element offset `at`
template <typename L, typename F>
__device__ __forceinline__ void resolve_block(int map, int br, int bc, int H, int W, L ign, int K, L* __restrict__ out,
                                              int* __restrict__ valid_labels, int* __restrict__ hist, int* cells, int* part, F value) {
    int count = 0;
    for (int i = threadIdx.x; i < LB * LB; i += LTPB) {
        const int r = br + i / LB, c = bc + i % LB;
        if (r >= H || c >= W) continue;
        const long at = (long)map * H * W + (long)r * W + c;
        const L v = value(i, r, c, at);
        out[at] = v;
        if (v != ign) {
            ++count;
            if constexpr (sizeof(L) == 2) {
                if (hist && (unsigned)v < (unsigned)K) atomicAdd(&cells[(int)v], 1);
            }
        }
    }
    const int total = block_sum_int(count, part);  // its barrier also orders the histogram cells
    if (threadIdx.x == 0 && total) atomicAdd(valid_labels + map, total);
    if constexpr (sizeof(L) == 2) {
        if (hist)
            for (int k = threadIdx.x; k < K; k += LTPB)
                if (cells[k]) atomicAdd(hist + (long)map * K + k, cells[k]);
    }
}

template <typename L>
__global__ __launch_bounds__(LTPB) void label_buffer_kernel(const L* __restrict__ labels, int H, int W, int nbx, int nby, int w, L ign,
                                                            const unsigned char* __restrict__ plane, int K, L* __restrict__ out,
                                                            int* __restrict__ valid_labels, int* __restrict__ hist) {
    __shared__ unsigned char flag[STG * STG];  // staged (sr, sc) <-> map (br - w + sr, bc - w + sc); row pitch `side`
    __shared__ short hit[STG * LB];            // (sr, c): the right-most flagged staged column in [c, c + 2 w], or -1
    __shared__ int cells[MAX_K];
    __shared__ int part[4];
    const int per = nbx * nby;
    const int map = blockIdx.x / per, blk = blockIdx.x - map * per;
    const int br = (blk / nbx) * LB, bc = (blk % nbx) * LB;
    const int side = LB + 2 * w;
    const L* in = labels + (long)map * H * W;
    for (int i = threadIdx.x; i < MAX_K; i += LTPB) cells[i] = 0;
    for (int i = threadIdx.x; i < side * side; i += LTPB) {
        const int sr = i / side, sc = i - sr * side;
        const int r = br - w + sr, c = bc - w + sc;
        unsigned char f = 0;
        if (r >= 0 && r < H && c >= 0 && c < W) f = in[(long)r * W + c] != ign ? 1 : 0;
        flag[i] = f;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < side * LB; i += LTPB) {
        const int sr = i / LB, c = i % LB;
        const unsigned char* row = flag + sr * side;
        int h = -1;
        for (int sc = c + 2 * w; sc >= c; --sc)
            if (row[sc]) {
                h = sc;
                break;
            }
        hit[i] = (short)h;
    }
    __syncthreads();
    resolve_block<L>(map, br, bc, H, W, ign, K, out, valid_labels, hist, cells, part, [&](int i, int r, int c, long at) -> L {
        if (plane && (plane[at] & 2)) return ign;
        const int lr = i / LB, lc = i % LB;
        for (int sr = lr + 2 * w; sr >= lr; --sr) {
            const int h = hit[sr * LB + lc];
            if (h >= 0) return in[(long)(br - w + sr) * W + (bc - w + h)];
        }
        return in[(long)r * W + c];
    });
}

template <typename L>
__global__ __launch_bounds__(LTPB) void label_limit_kernel(const L* __restrict__ labels, int H, int W, int nbx, int nby,
                                                           const int* __restrict__ ptr, const int* __restrict__ pts, long P, L ign, int K,
                                                           L* __restrict__ out, int* __restrict__ valid_labels, int* __restrict__ hist) {
    __shared__ unsigned mask[LB * LB / 32];
    __shared__ int cells[MAX_K];
    __shared__ int part[4];
    const int per = nbx * nby;
    const int map = blockIdx.x / per, blk = blockIdx.x - map * per;
    const int br = (blk / nbx) * LB, bc = (blk % nbx) * LB;
    for (int i = threadIdx.x; i < LB * LB / 32; i += LTPB) mask[i] = 0u;
    for (int i = threadIdx.x; i < MAX_K; i += LTPB) cells[i] = 0;
    __syncthreads();
    const long first = max((long)ptr[map], 0L), last = min((long)ptr[map + 1], P);
    for (long j = first + threadIdx.x; j < last; j += LTPB) {
        const int pr = pts[2 * j], pc = pts[2 * j + 1];
        if ((unsigned)pr >= (unsigned)H || (unsigned)pc >= (unsigned)W) continue;
        const int lr = pr - br, lc = pc - bc;
        if ((unsigned)lr >= (unsigned)LB || (unsigned)lc >= (unsigned)LB) continue;
        const int bit = lr * LB + lc;
        atomicOr(&mask[bit >> 5], 1u << (bit & 31));
    }
    __syncthreads();
    resolve_block<L>(map, br, bc, H, W, ign, K, out, valid_labels, hist, cells, part,
                     [&](int i, int r, int c, long at) -> L { return (mask[i >> 5] >> (i & 31) & 1u) ? labels[at] : ign; });
}

// the checks the two label entry points share -> IG_OK, or IG_ERR_ARG with the error text set
int check_label_args(const char* what, const void* labels, int n, int H, int W, int elem_size, int ignore_index, int K, const void* out,
                     const int* valid_labels, const int* hist) {
    IG_REQUIRE(n >= 0, "%s: need n >= 0 (got %d)", what, n);
    IG_REQUIRE(H >= 1 && W >= 1 && H <= (1 << 30) && W <= (1 << 30), "%s: need 1 <= H, W <= 2^30 (H %d, W %d)", what, H, W);
    IG_REQUIRE(elem_size == 2 || elem_size == 4, "%s: elem_size must be 2 (int16) or 4 (float32) (got %d)", what, elem_size);
    IG_REQUIRE(elem_size == 2 ? (ignore_index >= -32768 && ignore_index <= 32767) : (ignore_index >= -(1 << 24) && ignore_index <= (1 << 24)),
               "%s: ignore_index %d is not representable in the map's type (elem_size %d)", what, ignore_index, elem_size);
    IG_REQUIRE(K >= 0 && K <= MAX_K, "%s: need 0 <= K <= %d histogram cells (got %d)", what, MAX_K, K);
    IG_REQUIRE(K == 0 || elem_size == 2, "%s: a class histogram (K = %d) needs int16 labels", what, K);
    if (n == 0) return IG_OK;
    IG_REQUIRE((long)H * W < LIM40 / n, "%s: n * H * W exceeds 2^40 pixels (n %d, H %d, W %d)", what, n, H, W);
    const long groups = (long)ig_cdiv(H, LB) * ig_cdiv(W, LB) * n;
    IG_REQUIRE(groups <= 0x7fffffffL, "%s: %ld workgroups exceed 2^31 - 1 (n %d, H %d, W %d)", what, groups, n, H, W);
    IG_REQUIRE(labels && out && valid_labels, "%s: null pointer", what);
    IG_REQUIRE(labels != out, "%s: out must be distinct from labels", what);
    IG_REQUIRE(K == 0 || hist, "%s: null pointer (hist)", what);
    IG_REQUIRE((((uintptr_t)valid_labels | (uintptr_t)hist) & 3) == 0 && (((uintptr_t)labels | (uintptr_t)out) & (elem_size - 1)) == 0,
               "%s: valid_labels and hist must be 4-byte aligned, labels and out to their elements", what);
    return IG_OK;
}

}  // namespace

extern "C" int ig_chip_nodata(const void* chips, int n, int B, int H, int W, int no_data, unsigned char* plane, int* counts, void* stream) {
    IG_REQUIRE(n >= 0, "ig_chip_nodata: need n >= 0 (got %d)", n);
    IG_REQUIRE(B >= 1, "ig_chip_nodata: need B >= 1 bands (got %d)", B);
    IG_REQUIRE(H >= 1 && W >= 1, "ig_chip_nodata: need H >= 1 and W >= 1 (H %d, W %d)", H, W);
    IG_REQUIRE((long)H * W <= 0x7fffffffL, "ig_chip_nodata: H * W = %ld pixels exceeds 2^31 - 1 (counts is int32)", (long)H * W);
    IG_REQUIRE(no_data >= -32768 && no_data <= 65535, "ig_chip_nodata: no_data must be a 16-bit value (got %d)", no_data);
    if (n == 0) return IG_OK;
    const long HW = (long)H * W;
    IG_REQUIRE(HW < LIM40 / n / B, "ig_chip_nodata: n * B * H * W exceeds 2^40 values (n %d, B %d, H %d, W %d)", n, B, H, W);
    const int per = ig_cdiv(HW, NPIX);
    IG_REQUIRE((long)per * n <= 0x7fffffffL, "ig_chip_nodata: %ld workgroups exceed 2^31 - 1 (n %d, H %d, W %d)", (long)per * n, n, H, W);
    IG_REQUIRE(chips && plane && counts, "ig_chip_nodata: null pointer");
    IG_REQUIRE(((uintptr_t)chips & 1) == 0 && ((uintptr_t)counts & 3) == 0, "ig_chip_nodata: chips must be 2-byte, counts 4-byte aligned");
    return ig_launch<chip_nodata_kernel>("ig_chip_nodata", dim3((unsigned)((long)per * n)), dim3(NTPB), 0, (hipStream_t)stream,
                                         (const unsigned short*)chips, B, (int)HW, per, (unsigned short)(no_data & 0xffff), plane, counts);
}

extern "C" int ig_label_buffer(const void* labels, int n, int H, int W, int elem_size, int w, int ignore_index, const unsigned char* plane,
                               int K, void* out, int* valid_labels, int* hist, void* stream) {
    IG_REQUIRE(w >= 0 && w <= MAX_W, "ig_label_buffer: need a window 0 <= w <= %d (got %d)", MAX_W, w);
    const int rc = check_label_args("ig_label_buffer", labels, n, H, W, elem_size, ignore_index, K, out, valid_labels, hist);
    if (rc != IG_OK || n == 0) return rc;
    const int nbx = ig_cdiv(W, LB), nby = ig_cdiv(H, LB);
    const dim3 grid((unsigned)((long)nbx * nby * n));
    if (elem_size == 2)
        return ig_launch<label_buffer_kernel<short>>("ig_label_buffer", grid, dim3(LTPB), 0, (hipStream_t)stream, (const short*)labels, H, W,
                                                     nbx, nby, w, (short)ignore_index, plane, K, (short*)out, valid_labels,
                                                     K ? hist : nullptr);
    return ig_launch<label_buffer_kernel<float>>("ig_label_buffer", grid, dim3(LTPB), 0, (hipStream_t)stream, (const float*)labels, H, W,
                                                 nbx, nby, w, (float)ignore_index, plane, 0, (float*)out, valid_labels, nullptr);
}

extern "C" int ig_label_limit(const void* labels, int n, int H, int W, int elem_size, const int* ptr, const int* pts, long P,
                              int ignore_index, int K, void* out, int* valid_labels, int* hist, void* stream) {
    IG_REQUIRE(P >= 0 && P <= 0x3fffffffL, "ig_label_limit: need 0 <= P <= 2^30 - 1 points (got %ld)", P);
    const int rc = check_label_args("ig_label_limit", labels, n, H, W, elem_size, ignore_index, K, out, valid_labels, hist);
    if (rc != IG_OK || n == 0) return rc;
    IG_REQUIRE(ptr && (P == 0 || pts), "ig_label_limit: null pointer (ptr, pts)");
    IG_REQUIRE((((uintptr_t)ptr | (uintptr_t)pts) & 3) == 0, "ig_label_limit: ptr and pts must be 4-byte aligned");
    const int nbx = ig_cdiv(W, LB), nby = ig_cdiv(H, LB);
    const dim3 grid((unsigned)((long)nbx * nby * n));
    if (elem_size == 2)
        return ig_launch<label_limit_kernel<short>>("ig_label_limit", grid, dim3(LTPB), 0, (hipStream_t)stream, (const short*)labels, H, W,
                                                    nbx, nby, ptr, pts, P, (short)ignore_index, K, (short*)out, valid_labels,
                                                    K ? hist : nullptr);
    return ig_launch<label_limit_kernel<float>>("ig_label_limit", grid, dim3(LTPB), 0, (hipStream_t)stream, (const float*)labels, H, W, nbx,
                                                nby, ptr, pts, P, (float)ignore_index, 0, (float*)out, valid_labels, nullptr);
}
