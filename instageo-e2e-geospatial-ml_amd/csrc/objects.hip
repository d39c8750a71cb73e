// Object-level comparison of two labelled class maps for gfx950: the overlap of every ground-truth region with every
// predicted region as a sparse table, the matches above an IoU threshold and the region counts behind object F1 and panoptic quality.
// Not in the reference.  Everything is integer arithmetic; every result is unique (independent of scheduling and of the table's size).
//   object_pairs_kernel   per pixel the key (image * HW + gt label, pred label); a wave first merges the lanes that hold the same key
//                         (up to OP_MERGE distinct keys, one ballot each: neighbouring pixels share their regions, most waves hold one
//                         or two), then the leader of each group inserts (key, lanes) into the open-addressed table: a relaxed load of
//                         the slot, a 64-bit compare-and-swap only where it is empty, a 32-bit add on the slot's count.  Keys are never
//                         removed, so a slot seen with another key stays another key: linear probing goes on to the next slot.  A lane
//                         gives up after `capacity` probes, or earlier once it sees *status set (the table is invalid by then): it
//                         sets bit 0 of *status.  Nothing waits: every loop is bounded by `capacity`.
//   object_match_kernel   one thread per slot, the rule of include/instageo_objects.h; tp and iou_q cells as 64-bit LDS adds, then one
//                         64-bit global add per non-empty cell and workgroup.  A slot whose key points outside the maps is skipped.
//   object_count_kernel   root positions per class in a 32-bit LDS histogram (a call holds fewer than 2^31 pixels: no wrap), one 64-bit
//                         global add per non-empty class and workgroup
// LDS: match 2 * K * ncls u64 cells, at most 2 * 10 * 127 * 8 B = 20320 B dynamic; count 128 u32 static.
#include "common.h"

namespace {

constexpr int OTPB = 256, MAX_WG = 2048, OP_MERGE = 4, MAX_K = 10, MAX_NCLS = 127;
constexpr long MIN_CAP = 1024, MAX_CAP = 1L << 30;
constexpr unsigned long long EMPTY = ~0ull;
#define RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// the murmur3 64-bit finaliser
__device__ __forceinline__ unsigned long long mix64(unsigned long long k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}

__device__ __forceinline__ void table_add(unsigned long long* __restrict__ keys, unsigned* __restrict__ counts, long capacity,
                                          unsigned long long key, unsigned cnt, int* __restrict__ status) {
    const unsigned long long mask = (unsigned long long)capacity - 1ull;
    unsigned long long slot = mix64(key) & mask;  // < capacity: every index below stays inside both arrays
    for (long probe = 0; probe < capacity; ++probe) {
        unsigned long long cur = __hip_atomic_load(&keys[slot], RLX_AGENT);
        if (cur == EMPTY) {
            cur = atomicCAS(&keys[slot], EMPTY, key);
            if (cur == EMPTY) cur = key;
        }
        if (cur == key) {
            atomicAdd(&counts[slot], cnt);
            return;
        }
        if ((probe & 63) == 63 && __hip_atomic_load(status, RLX_AGENT) & 1) break;  // already invalid: do not walk a full table again
        slot = (slot + 1ull) & mask;
    }
    atomicOr(status, 1);
}

__global__ __launch_bounds__(OTPB) void object_pairs_kernel(const int* __restrict__ gt_labels, const int* __restrict__ pred_labels,
                                                            unsigned long long* __restrict__ keys, unsigned* __restrict__ counts,
                                                            long capacity, int* __restrict__ status, unsigned M, unsigned HW) {
    const int lane = threadIdx.x & 63;
    // the trip count is the same in every lane of the workgroup: the ballots below see whole waves
    for (unsigned long base = blockIdx.x * (unsigned long)OTPB; base < M; base += (unsigned long)gridDim.x * OTPB) {
        const unsigned long q = base + threadIdx.x;
        int g = -1, p = -1;
        if (q < M) g = gt_labels[q], p = pred_labels[q];
        bool act = g >= 0 && p >= 0;
        const unsigned img0 = act ? ((unsigned)q / HW) * HW : 0u;  // M <= 2^31 - 1: 32-bit division
        const unsigned khi = img0 + (unsigned)g, klo = (unsigned)p;
        bool lead = false;
        unsigned mine = 0;
        for (int it = 0; it < OP_MERGE; ++it) {
            const unsigned long long todo = __ballot(act);
            if (!todo) break;
            const int src = __ffsll((long long)todo) - 1;
            const unsigned shi = __shfl(khi, src, 64), slo = __shfl(klo, src, 64);
            const bool hit = act && khi == shi && klo == slo;
            const unsigned c = (unsigned)__popcll(__ballot(hit));
            if (lane == src) lead = true, mine = c;
            act = act && !hit;
        }
        if (act) lead = true, mine = 1u;  // more than OP_MERGE keys in the wave: the rest insert one by one
        if (lead) table_add(keys, counts, capacity, ((unsigned long long)khi << 32) | klo, mine, status);
    }
}

struct Ratios {
    unsigned num[MAX_K], den[MAX_K];
};

// LDS: tp[K][ncls] then iou_q[K][ncls], u64
__global__ __launch_bounds__(OTPB) void object_match_kernel(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ counts,
                                                            long capacity, const signed char* __restrict__ gt,
                                                            const signed char* __restrict__ pred, const int* __restrict__ gt_area,
                                                            const int* __restrict__ pred_area, Ratios th, int K,
                                                            unsigned long long* __restrict__ tp, unsigned long long* __restrict__ iou_q,
                                                            unsigned M, unsigned HW, int ncls, int min_area) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long* s = reinterpret_cast<unsigned long long*>(smem);
    const int cells = K * ncls;
    for (int i = threadIdx.x; i < 2 * cells; i += OTPB) s[i] = 0ull;
    __syncthreads();
    for (long slot = blockIdx.x * (long)OTPB + threadIdx.x; slot < capacity; slot += (long)gridDim.x * OTPB) {
        const unsigned long long key = keys[slot];
        if (key == EMPTY) continue;
        const unsigned long long hi = key >> 32;
        const unsigned p = (unsigned)key;
        if (hi >= M || p >= HW) continue;  // not a key of these maps
        const unsigned img0 = ((unsigned)hi / HW) * HW;
        const unsigned long gi = hi, pi = (unsigned long)img0 + p;  // pi < M: img0 + HW <= M because hi < M lies in a whole image
        const int cg = gt[gi], cp = pred[pi];
        if (cg != cp || cg < 0 || cg >= ncls) continue;
        const long ag = gt_area[gi], ap = pred_area[pi];
        const long cnt = counts[slot], u = ag + ap - cnt;
        if (ag < min_area || ap < min_area || cnt <= 0 || u <= 0) continue;
        const unsigned long long q = (((unsigned long long)cnt << 25) + (unsigned long long)u) / (2ull * (unsigned long long)u);
        for (int k = 0; k < K; ++k) {
            if ((unsigned long long)cnt * th.den[k] > (unsigned long long)th.num[k] * (unsigned long long)u) {
                atomicAdd(s + k * ncls + cg, 1ull);
                atomicAdd(s + cells + k * ncls + cg, q);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * cells; i += OTPB) {
        const unsigned long long v = s[i];
        if (v) atomicAdd(i < cells ? tp + i : iou_q + (i - cells), v);
    }
}

__global__ __launch_bounds__(OTPB) void object_count_kernel(const signed char* __restrict__ cls, const int* __restrict__ labels,
                                                            const int* __restrict__ area, unsigned long long* __restrict__ n_regions,
                                                            unsigned M, unsigned HW, int ncls, int min_area) {
    __shared__ unsigned s[MAX_NCLS + 1];
    if (threadIdx.x <= MAX_NCLS) s[threadIdx.x] = 0u;
    __syncthreads();
    for (unsigned long q = blockIdx.x * (unsigned long)OTPB + threadIdx.x; q < M; q += (unsigned long)gridDim.x * OTPB) {
        const int l = labels[q];
        if (l < 0 || (unsigned)l != (unsigned)q % HW) continue;
        const int c = cls[q];
        if (c >= 0 && c < ncls && area[q] >= min_area) atomicAdd(s + c, 1u);
    }
    __syncthreads();
    if ((int)threadIdx.x < ncls && s[threadIdx.x]) atomicAdd(n_regions + threadIdx.x, (unsigned long long)s[threadIdx.x]);
}

inline unsigned grid_for(long items) {
    const long nblk = (items + OTPB - 1) / OTPB;
    return (unsigned)(nblk < MAX_WG ? nblk : MAX_WG);
}

}  // namespace

#define ST(s) ((hipStream_t)(s))
#define IG_REQUIRE_PIXELS(what)                                                                                                   \
    IG_REQUIRE(n >= 0 && HW >= 1 && HW <= 0x7fffffffL, what ": need n >= 0 and 1 <= HW <= 2^31 - 1 (n %d, HW %ld)", n, HW);      \
    IG_REQUIRE((long)n * HW <= 0x7fffffffL, what ": n * HW = %ld exceeds 2^31 - 1 pixels per call", (long)n * HW)
#define IG_REQUIRE_CAPACITY(what)                                                                                       \
    IG_REQUIRE(capacity >= MIN_CAP && capacity <= MAX_CAP && (capacity & (capacity - 1)) == 0,                          \
               what ": capacity must be a power of two in [1024, 2^30] (got %ld)", capacity)

extern "C" {

int ig_objects_header_stamp(void) { return (int)(IG_OBJECTS_STAMP); }

int ig_object_pairs(const int* gt_labels, const int* pred_labels, unsigned long long* keys, unsigned* counts, long capacity, int* status,
                    int n, long HW, void* stream) {
    IG_REQUIRE_CAPACITY("ig_object_pairs");
    IG_REQUIRE_PIXELS("ig_object_pairs");
    if (n == 0) return IG_OK;
    IG_REQUIRE(gt_labels && pred_labels && keys && counts && status, "ig_object_pairs: null pointer");
    IG_REQUIRE(((uintptr_t)keys & 7) == 0 && ((uintptr_t)counts & 3) == 0, "ig_object_pairs: keys must be 8-byte aligned, counts 4-byte");
    if (hipMemsetAsync(keys, 0xff, (size_t)capacity * sizeof(unsigned long long), ST(stream)) != hipSuccess ||
        hipMemsetAsync(counts, 0, (size_t)capacity * sizeof(unsigned), ST(stream)) != hipSuccess) {
        ig_set_error("ig_object_pairs: hipMemsetAsync failed");
        return IG_ERR_HIP;
    }
    const long M = (long)n * HW;
    return ig_launch<object_pairs_kernel>("ig_object_pairs", dim3(grid_for(M)), dim3(OTPB), 0, ST(stream), gt_labels, pred_labels, keys,
                                          counts, capacity, status, (unsigned)M, (unsigned)HW);
}

int ig_object_match(const unsigned long long* keys, const unsigned* counts, long capacity, const signed char* gt, const signed char* pred,
                    const int* gt_area, const int* pred_area, const int* num, const int* den, int K, unsigned long long* tp,
                    unsigned long long* iou_q, int n, long HW, int ncls, int min_area, void* stream) {
    IG_REQUIRE_CAPACITY("ig_object_match");
    IG_REQUIRE(K >= 1 && K <= MAX_K, "ig_object_match: 1 <= K <= %d (got %d)", MAX_K, K);
    IG_REQUIRE(num && den, "ig_object_match: null pointer (num, den)");
    Ratios th = {};
    for (int k = 0; k < K; ++k) {
        IG_REQUIRE(den[k] >= 1, "ig_object_match: den[%d] = %d is not positive", k, den[k]);
        IG_REQUIRE(2L * num[k] >= den[k] && num[k] < den[k], "ig_object_match: threshold %d = %d / %d is outside [1/2, 1)", k, num[k], den[k]);
        th.num[k] = (unsigned)num[k], th.den[k] = (unsigned)den[k];
    }
    IG_REQUIRE(ncls >= 2 && ncls <= MAX_NCLS, "ig_object_match: 2 <= ncls <= %d (got %d)", MAX_NCLS, ncls);
    IG_REQUIRE(min_area >= 1, "ig_object_match: min_area must be at least 1 (got %d)", min_area);
    IG_REQUIRE_PIXELS("ig_object_match");
    if (n == 0) return IG_OK;
    IG_REQUIRE(keys && counts && gt && pred && gt_area && pred_area && tp && iou_q, "ig_object_match: null pointer");
    return ig_launch<object_match_kernel>("ig_object_match", dim3(grid_for(capacity)), dim3(OTPB), 2 * K * ncls * 8, ST(stream), keys, counts,
                                          capacity, gt, pred, gt_area, pred_area, th, K, tp, iou_q, (unsigned)((long)n * HW), (unsigned)HW,
                                          ncls, min_area);
}

int ig_object_count(const signed char* cls, const int* labels, const int* area, unsigned long long* n_regions, int n, long HW, int ncls,
                    int min_area, void* stream) {
    IG_REQUIRE(ncls >= 2 && ncls <= MAX_NCLS, "ig_object_count: 2 <= ncls <= %d (got %d)", MAX_NCLS, ncls);
    IG_REQUIRE(min_area >= 1, "ig_object_count: min_area must be at least 1 (got %d)", min_area);
    IG_REQUIRE_PIXELS("ig_object_count");
    if (n == 0) return IG_OK;
    IG_REQUIRE(cls && labels && area && n_regions, "ig_object_count: null pointer");
    const long M = (long)n * HW;
    return ig_launch<object_count_kernel>("ig_object_count", dim3(grid_for(M)), dim3(OTPB), 0, ST(stream), cls, labels, area, n_regions,
                                          (unsigned)M, (unsigned)HW, ncls, min_area);
}

}  // extern "C"
