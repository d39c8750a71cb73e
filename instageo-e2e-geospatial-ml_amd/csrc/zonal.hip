// Zonal statistics for gfx950: polygon zones scan-converted onto the raster of a class map and tallied per zone and
// class.  Not in the reference.  The rule (Q = 256 fixed point, half-open crossing, even-odd on pixel centres) is stated in
// include/instageo_hip.h.  Everything is integer arithmetic and every result is unique (independent of scheduling).
//
//   1  zone_edge_rows_kernel   per edge: the number of raster rows whose centre line it crosses
//   2  zone_toggle_kernel      per (edge, crossed row) pair, found by binary search in the caller's exclusive scan of (1): the first column
//                              whose centre lies at or right of the crossing, and one 64-bit atomic XOR of the zone's bit there
//   3  zone_tally_kernel       per row: inclusive prefix XOR of the toggles (thread run of ZVPT, wave scan, workgroup scan, carry over the
//                              chunks of ZCHUNK columns), which is the inside mask of 64 zones; every set bit is counted into an LDS table
//                              [64][ncls + 1] and the table reaches memory as one 64-bit add per non-empty cell and workgroup
//
// Up to 64 zones share a pass: one bit of a uint64 canvas each.  A pass costs one sweep of the 8-byte canvas (read, optionally written)
// and of the 1-byte class map, whatever the number of edges; the toggles are one atomic per crossing.
// The tally merges runs of adjacent lanes that hold the same (mask, class) before it touches LDS: inside a large zone a wave adds once
// per zone, not 64 times to one address.
// Every launch does a fixed amount of work; no workgroup waits for another (a workgroup owns whole rows, so the carry between the chunks
// of a long row stays in a register).  Out-of-range writes are impossible: a row or column outside the raster, an item past its edge's
// rows (a scan that does not belong to the edges) and a bit outside 0..63 are dropped.
#include "common.h"

namespace {

constexpr int ZTPB = 256, ZWAVES = ZTPB / 64;
constexpr int ZVPT = 4, ZCHUNK = ZTPB * ZVPT;  // columns a workgroup scans in one step
constexpr int ZQ = 256, ZHALF = 128;           // fixed-point units per pixel; the centre's offset
constexpr int ZLIMIT = 1 << 29;                // |X|, |Y| <= 2^29
constexpr int ZBITS = 64, MAX_NCLS = 127, MAX_WG = 1024;

struct RowSpan {
    int lo, n;  // first crossed row in [0, H) and their number
};

// rows r with (y0 <= Yc) != (y1 <= Yc), Yc = 256 r + 128: min(y0, y1) <= Yc < max(y0, y1).  An edge with a coordinate beyond the limit
// crosses nothing (the host refuses such zones; this keeps every difference below 2^31 whatever arrives).
__device__ __forceinline__ RowSpan rows_of(const int4 e, int H) {
    const int lim = ZLIMIT;
    if (e.x < -lim || e.x > lim || e.y < -lim || e.y > lim || e.z < -lim || e.z > lim || e.w < -lim || e.w > lim) return RowSpan{0, 0};
    const int ylo = e.y < e.w ? e.y : e.w, yhi = e.y < e.w ? e.w : e.y;
    int lo = (ylo - ZHALF + ZQ - 1) >> 8;  // ceil((ylo - 128) / 256): arithmetic shift = floor
    int hi = (yhi - ZHALF - 1) >> 8;       // floor((yhi - 129) / 256)
    lo = lo < 0 ? 0 : lo;
    hi = hi > H - 1 ? H - 1 : hi;
    return RowSpan{lo, hi >= lo ? hi - lo + 1 : 0};
}

__global__ __launch_bounds__(ZTPB) void zone_edge_rows_kernel(const int4* __restrict__ edges, int* __restrict__ rows, long E, int H) {
    const long e = blockIdx.x * (long)ZTPB + threadIdx.x;
    if (e < E) rows[e] = rows_of(edges[e], H).n;
}

__global__ __launch_bounds__(ZTPB) void zone_toggle_kernel(const int4* __restrict__ edges, const unsigned char* __restrict__ bit,
                                                           const long long* __restrict__ first, unsigned long long* __restrict__ canvas,
                                                           long E, long T, int H, int W) {
    const long t = blockIdx.x * (long)ZTPB + threadIdx.x;
    if (t >= T) return;
    long lo = 0, hi = E;  // the last e with first[e] <= t: its rows are first[e] .. first[e + 1] - 1
    while (hi - lo > 1) {
        const long mid = (lo + hi) >> 1;
        if (first[mid] <= t) lo = mid;
        else hi = mid;
    }
    const long long k = t - first[lo];
    const int4 e = edges[lo];
    const RowSpan span = rows_of(e, H);
    const unsigned b = bit[lo];
    if (k < 0 || k >= span.n || b >= (unsigned)ZBITS) return;
    const int r = span.lo + (int)k;
    // xc = x0 + (x1 - x0)(Yc - y0)/(y1 - y0);  c* = max(0, ceil((xc - 128)/256)) = max(0, ceil(N / D)) with
    // N = (x0 - 128)(y1 - y0) + (x1 - x0)(Yc - y0), D = 256 (y1 - y0), both negated when y1 < y0.  |N| < 2^61.
    const long long yc = (long long)ZQ * r + ZHALF;
    long long den = (long long)e.w - e.y;
    long long num = ((long long)e.x - ZHALF) * den + ((long long)e.z - e.x) * (yc - e.y);
    if (den < 0) den = -den, num = -num;
    den *= ZQ;
    long long q = num / den;  // truncates towards zero: one more when a positive remainder is left
    if (num % den > 0) ++q;
    const long long c = q < 0 ? 0 : q;
    if (c < W) atomicXor(canvas + (long)r * W + c, 1ull << b);
}

// cls = NULL: the masks only, nothing is counted.  grid.x workgroups take rows blockIdx.x, blockIdx.x + gridDim.x, ...  LDS: tab[64][ncls + 1]
// u32 (dynamic; a cell counts at most the H * W <= 2^31 - 1 pixels of the raster, so it cannot wrap) and the wave totals of two
// consecutive chunks (one barrier per chunk).
__global__ __launch_bounds__(ZTPB) void zone_tally_kernel(unsigned long long* __restrict__ canvas, const signed char* __restrict__ cls,
                                                          unsigned long long* __restrict__ counts, int H, int W, int ncls, int fill,
                                                          int write_mask) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned* tab = reinterpret_cast<unsigned*>(smem);
    __shared__ unsigned long long wtot[2][ZWAVES];
    const int cols = ncls + 1, cells = ZBITS * cols;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < cells; i += ZTPB) tab[i] = 0u;
    __syncthreads();
    int par = 0;
    for (int r = blockIdx.x; r < H; r += gridDim.x) {
        unsigned long long* row = canvas + (long)r * W;
        const signed char* crow = cls ? cls + (long)r * W : nullptr;
        unsigned long long carry = 0;  // the prefix XOR of the row's earlier chunks: the same in every thread
        for (long c0 = 0; c0 < W; c0 += ZCHUNK, par ^= 1) {  // long: W may be close to 2^31
            const long c = c0 + (long)threadIdx.x * ZVPT;
            unsigned long long v[ZVPT];
            int k[ZVPT];
#pragma unroll
            for (int j = 0; j < ZVPT; ++j) {
                v[j] = 0;
                k[j] = ncls;
                if (c + j < W) {
                    v[j] = row[c + j];
                    const int s = cls ? crow[c + j] : fill;
                    if (s != fill && s >= 0 && s < ncls) k[j] = s;
                }
                if (j) v[j] ^= v[j - 1];
            }
            unsigned long long t = v[ZVPT - 1];  // inclusive scan of the thread totals over the wave
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned long long u = __shfl_up(t, o, 64);
                if (lane >= o) t ^= u;
            }
            if (lane == 63) wtot[par][wave] = t;
            __syncthreads();
            unsigned long long pre = carry ^ t ^ v[ZVPT - 1];  // XOR undoes itself: inclusive ^ own = exclusive
#pragma unroll
            for (int w = 0; w < ZWAVES; ++w) {
                const unsigned long long u = wtot[par][w];
                if (w < wave) pre ^= u;
                carry ^= u;
            }
#pragma unroll
            for (int j = 0; j < ZVPT; ++j) {
                const bool live = c + j < W;
                const unsigned long long m = live ? v[j] ^ pre : 0ull;
                if (live && write_mask) row[c + j] = m;
                if (!cls) continue;  // masks only (uniform over the grid)
                // runs of adjacent lanes with the same (mask, class) add once, at their first lane
                const unsigned long long pm = __shfl_up(m, 1, 64);
                const int pk = __shfl_up(k[j], 1, 64);
                const bool head = lane == 0 || pm != m || pk != k[j];
                const unsigned long long above = (__ballot(head) >> lane) >> 1;  // the heads of the lanes after this one
                if (head && m) {
                    const unsigned len = above ? (unsigned)__ffsll((long long)above) : (unsigned)(64 - lane);
                    unsigned long long rest = m;
                    while (rest) {
                        const int b = __ffsll((long long)rest) - 1;
                        rest &= rest - 1;
                        atomicAdd(tab + b * cols + k[j], len);
                    }
                }
            }
        }
    }
    __syncthreads();
    if (!cls) return;
    for (int i = threadIdx.x; i < cells; i += ZTPB)
        if (tab[i]) atomicAdd(counts + i, (unsigned long long)tab[i]);
}

}  // namespace

#define ST(s) ((hipStream_t)(s))
#define IG_REQUIRE_RASTER(name)                                                                     \
    IG_REQUIRE(H >= 0 && W >= 0, name ": need H >= 0 and W >= 0 (H %d, W %d)", H, W);               \
    IG_REQUIRE((long)H * W <= 0x7fffffffL, name ": H * W = %ld exceeds 2^31 - 1", (long)H * W)

static inline dim3 blocks_for(long items) { return dim3((unsigned)((items + ZTPB - 1) / ZTPB)); }

extern "C" {

int ig_zone_edge_rows(const int* edges, int* rows, long E, int H, void* stream) {
    IG_REQUIRE(E >= 0 && E <= 0x7fffffffL, "ig_zone_edge_rows: need 0 <= E <= 2^31 - 1 (got %ld)", E);
    IG_REQUIRE(H >= 0, "ig_zone_edge_rows: need H >= 0 (got %d)", H);
    if (E == 0) return IG_OK;
    IG_REQUIRE(edges && rows, "ig_zone_edge_rows: null pointer");
    IG_REQUIRE(((uintptr_t)edges & 15) == 0, "ig_zone_edge_rows: edges must be 16-byte aligned");
    return ig_launch<zone_edge_rows_kernel>("ig_zone_edge_rows", blocks_for(E), dim3(ZTPB), 0, ST(stream), (const int4*)edges, rows, E, H);
}

int ig_zone_toggle(const int* edges, const unsigned char* bit, const long long* first, unsigned long long* canvas, long E, long T, int H,
                   int W, void* stream) {
    IG_REQUIRE(E >= 0 && E <= 0x7fffffffL, "ig_zone_toggle: need 0 <= E <= 2^31 - 1 (got %ld)", E);
    IG_REQUIRE(T >= 0 && T <= (1L << 38), "ig_zone_toggle: need 0 <= T <= 2^38 crossings per call (got %ld)", T);
    IG_REQUIRE_RASTER("ig_zone_toggle");
    if (E == 0 || T == 0 || (long)H * W == 0) return IG_OK;
    IG_REQUIRE(edges && bit && first && canvas, "ig_zone_toggle: null pointer");
    IG_REQUIRE(((uintptr_t)edges & 15) == 0, "ig_zone_toggle: edges must be 16-byte aligned");
    IG_REQUIRE(((uintptr_t)first & 7) == 0 && ((uintptr_t)canvas & 7) == 0, "ig_zone_toggle: first and canvas must be 8-byte aligned");
    return ig_launch<zone_toggle_kernel>("ig_zone_toggle", blocks_for(T), dim3(ZTPB), 0, ST(stream), (const int4*)edges, bit, first, canvas, E,
                                         T, H, W);
}

int ig_zone_tally(unsigned long long* canvas, const signed char* cls, unsigned long long* counts, int H, int W, int ncls, int fill,
                  int write_mask, void* stream) {
    IG_REQUIRE(ncls >= 2 && ncls <= MAX_NCLS, "ig_zone_tally: 2 <= ncls <= %d (got %d)", MAX_NCLS, ncls);
    IG_REQUIRE(fill >= -128 && fill <= 127, "ig_zone_tally: fill must fit int8 (got %d)", fill);
    IG_REQUIRE_RASTER("ig_zone_tally");
    if ((long)H * W == 0) return IG_OK;
    IG_REQUIRE(canvas && (cls ? counts != nullptr : write_mask != 0), "ig_zone_tally: null pointer (cls = NULL needs write_mask, else counts)");
    IG_REQUIRE(((uintptr_t)canvas & 7) == 0 && ((uintptr_t)counts & 7) == 0, "ig_zone_tally: canvas and counts must be 8-byte aligned");
    return ig_launch<zone_tally_kernel>("ig_zone_tally", dim3((unsigned)(H < MAX_WG ? H : MAX_WG)), dim3(ZTPB), ZBITS * (ncls + 1) * 4,
                                        ST(stream), canvas, cls, counts, H, W, ncls, fill, write_mask);
}

}  // extern "C"
