// Zonal statistics for gfx950: polygon zones scan-converted onto the raster of a class map and tallied per zone and
// class.  Not in the reference.  The rule (Q = 256 fixed point, half-open crossing, even-odd on pixel centres) is stated in
// include/instageo_hip.h.  Everything is integer arithmetic and every result is unique (independent of scheduling).
//
//   1  zone_rows_kernel<rows_of>  per edge: the number of raster rows whose centre line it crosses
//   2  zone_toggle_kernel      per (edge, crossed row) pair, found by binary search in the caller's exclusive scan of (1) (edge_of_item): the
//                              first column whose centre lies at or right of the crossing, and one 64-bit atomic XOR of the zone's bit there
//   3  zone_tally_kernel       per row: inclusive prefix XOR of the toggles (zone_scan_chunk of zone_canvas.h, shared with burn.hip: thread run
//                              of ZVPT, wave scan, workgroup scan, carry over the chunks of ZCHUNK columns), which is the inside mask of 64
//                              zones; every set bit is counted into an LDS table
//                              [64][ncls + 1] and the table reaches memory as one 64-bit add per non-empty cell and workgroup
//   4  zone_value_tally_kernel the same rows and the same scan over a float32 raster of up to 8 bands: per zone bit and band the valid
//                              values' (n, sum, M2, min, max), merged as triples (Chan, Golub, LeVeque) through the wave, the wave's LDS
//                              accumulators and the workgroup into one partial per workgroup; the canvas is only read
//   5  zone_value_reduce_kernel  the partials merged in workgroup order -> valid, mean, M2, min, max and the inside pixels
//   (4) and (5) are float64 in a fixed order, without atomics: unique results too.
//   6  zone_quantile_hist_kernel  one round of a radix selection of order statistics (median, percentiles): the rows and scan of (4);
//                              per valid value, zone bit, band and rank slot whose key prefix it continues, one count in the histogram of
//                              the round's 8-bit digit: unsigned integer atomics, equal targets merged across the wave first
//   7  zone_quantile_pick_kernel  per (band, zone bit, slot): the digit that holds the wanted rank; after the last round the values
//   (6) and (7) count with integer atomics only and select members of the data: unique results as well.
//   8  zone_rows_kernel<touch_rows_of>  all_touched (the rule: include/instageo_hip.h): per edge the number of raster rows whose open strip
//                              it meets; (1) over the other span
//   9  zone_touch_kernel       per (edge, touched row) pair: the columns whose open square the edge meets in that row, exact rationals in
//                              int64, and a 64-bit atomic OR of the zone's bit into each of them on a second canvas.  A lane writes a span of
//                              up to ZT_SHORT columns itself; longer ones are taken by the whole wave, one after the other, 64 columns a step
//   10 zone_touch_merge_kernel per row: m = (prefix XOR of the toggles, the scan of (3)) | touch, written back as toggles m[c] ^ m[c - 1]:
//                              the canvas is a toggle canvas again and (3), (4), (6) and ig_burn_resolve work on it as they are
//
// Up to 64 zones share a pass: one bit of a uint64 canvas each.  A pass costs one sweep of the 8-byte canvas (read, optionally written)
// and of the 1-byte class map, whatever the number of edges; the toggles are one atomic per crossing.
// The tally merges runs of adjacent lanes that hold the same (mask, class) before it touches LDS: inside a large zone a wave adds once
// per zone, not 64 times to one address.
// Every launch does a fixed amount of work; no workgroup waits for another (a workgroup owns whole rows, so the carry between the chunks
// of a long row stays in a register).  Out-of-range writes are impossible: a row or column outside the raster, an item past its edge's
// rows (a scan that does not belong to the edges) and a bit outside 0..63 are dropped.
#include "zone_canvas.h"

namespace {

constexpr int ZQ = 256, ZHALF = 128;  // fixed-point units per pixel; the centre's offset
constexpr int ZLIMIT = 1 << 29;       // |X|, |Y| <= 2^29
constexpr int MAX_NCLS = 127;

struct RowSpan {
    int lo, n;  // first row in [0, H) and their number
};

// The rows floor((ymin + below) / 256) .. floor((ymax + above) / 256) of an edge (arithmetic shift = floor), clamped to [0, H).  An edge
// with a coordinate beyond the limit has none (the host refuses such zones; this keeps every difference below 2^31 whatever arrives).
__device__ __forceinline__ RowSpan row_span(const int4 e, int H, int below, int above) {
    const int lim = ZLIMIT;
    if (e.x < -lim || e.x > lim || e.y < -lim || e.y > lim || e.z < -lim || e.z > lim || e.w < -lim || e.w > lim) return RowSpan{0, 0};
    const int ylo = e.y < e.w ? e.y : e.w, yhi = e.y < e.w ? e.w : e.y;
    int lo = (ylo + below) >> 8, hi = (yhi + above) >> 8;
    lo = lo < 0 ? 0 : lo;
    hi = hi > H - 1 ? H - 1 : hi;
    return RowSpan{lo, hi >= lo ? hi - lo + 1 : 0};
}

// rows r with (y0 <= Yc) != (y1 <= Yc), Yc = 256 r + 128: min(y0, y1) <= Yc < max(y0, y1), i.e. ceil((ymin - 128) / 256) <= r <=
// floor((ymax - 129) / 256)
__device__ __forceinline__ RowSpan rows_of(const int4 e, int H) { return row_span(e, H, ZQ - 1 - ZHALF, -ZHALF - 1); }

// all_touched: rows r whose open strip (256 r, 256 r + 256) the edge's y range meets: floor(ymin / 256) <= r <= ceil(ymax / 256) - 1.  Empty
// for a horizontal edge on a row border.
__device__ __forceinline__ RowSpan touch_rows_of(const int4 e, int H) { return row_span(e, H, 0, -1); }

template <RowSpan (*Rows)(const int4, int)>
__global__ __launch_bounds__(ZTPB) void zone_rows_kernel(const int4* __restrict__ edges, int* __restrict__ rows, long E, int H) {
    const long e = blockIdx.x * (long)ZTPB + threadIdx.x;
    if (e < E) rows[e] = Rows(edges[e], H).n;
}

// Item t of a launch over (edge, row) pairs belongs to the last edge e with first[e] <= t (first = the caller's exclusive scan of the
// edges' row counts): its rows are items first[e] .. first[e + 1] - 1.
__device__ __forceinline__ long edge_of_item(const long long* __restrict__ first, long E, long t) {
    long lo = 0, hi = E;
    while (hi - lo > 1) {
        const long mid = (lo + hi) >> 1;
        if (first[mid] <= t) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(ZTPB) void zone_toggle_kernel(const int4* __restrict__ edges, const unsigned char* __restrict__ bit,
                                                           const long long* __restrict__ first, unsigned long long* __restrict__ canvas,
                                                           long E, long T, int H, int W) {
    const long t = blockIdx.x * (long)ZTPB + threadIdx.x;
    if (t >= T) return;
    const long lo = edge_of_item(first, E, t);
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

// ---- all_touched: the pixels whose open square an edge meets --------------------------------------------------------------------------------
constexpr int ZT_SHORT = 4;  // columns a lane writes on its own; a longer span is written by its wave

__device__ __forceinline__ long long floor_div(long long n, long long d) {  // d > 0
    const long long q = n / d;
    return n % d < 0 ? q - 1 : q;
}
__device__ __forceinline__ long long ceil_div(long long n, long long d) {  // d > 0
    const long long q = n / d;
    return n % d > 0 ? q + 1 : q;
}

struct ColSpan {
    int lo, n;  // first touched column in [0, W) and their number
};

// The columns of row r (one of touch_rows_of) whose open square the edge meets.  The part of the edge inside the closed strip runs from
// ya = max(ymin, 256 r) to yb = min(ymax, 256 r + 256), ya < yb for a non-horizontal edge; its abscissae there are N / D with
// N = x0 (y1 - y0) + (x1 - x0)(y - y0), D = y1 - y0, both negated when y1 < y0: |N| < 2^61.  A horizontal edge has its own two ends.
// With lo / hi the smaller / larger: floor(lo / 256) <= c <= ceil(hi / 256) - 1, clamped to [0, W) (nothing is moved onto column 0).
__device__ __forceinline__ ColSpan touch_cols_of(const int4 e, int r, int W) {
    long long den = (long long)e.w - e.y, a, b;
    if (den == 0) {
        den = 1;
        a = e.x, b = e.z;
    } else {
        const long long ylo = e.y < e.w ? e.y : e.w, yhi = e.y < e.w ? e.w : e.y;
        const long long top = (long long)ZQ * r, ya = ylo > top ? ylo : top, yb = yhi < top + ZQ ? yhi : top + ZQ;
        a = (long long)e.x * den + ((long long)e.z - e.x) * (ya - e.y);
        b = (long long)e.x * den + ((long long)e.z - e.x) * (yb - e.y);
        if (den < 0) den = -den, a = -a, b = -b;
    }
    den *= ZQ;
    long long lo = floor_div(a < b ? a : b, den), hi = ceil_div(a < b ? b : a, den) - 1;
    lo = lo < 0 ? 0 : lo;
    hi = hi > W - 1 ? W - 1 : hi;
    return ColSpan{(int)lo, hi >= lo ? (int)(hi - lo + 1) : 0};
}

// No lane leaves before the end: the long spans are written by all 64 lanes of the wave.  Every address is row r < H, column < W of the
// (H, W) canvas: r and the span come clamped from touch_rows_of / touch_cols_of, and a lane without an item holds an empty span.
__global__ __launch_bounds__(ZTPB) void zone_touch_kernel(const int4* __restrict__ edges, const unsigned char* __restrict__ bit,
                                                          const long long* __restrict__ first, unsigned long long* __restrict__ touch,
                                                          long E, long T, int H, int W) {
    const long t = blockIdx.x * (long)ZTPB + threadIdx.x;
    const int lane = threadIdx.x & 63;
    long at = 0;  // canvas index of the span's first pixel
    int n = 0;    // its columns
    unsigned long long mask = 0;
    if (t < T) {
        const long lo = edge_of_item(first, E, t);
        const long long k = t - first[lo];
        const int4 e = edges[lo];
        const RowSpan rows = touch_rows_of(e, H);
        const unsigned b = bit[lo];
        if (k >= 0 && k < rows.n && b < (unsigned)ZBITS) {
            const int r = rows.lo + (int)k;
            const ColSpan cols = touch_cols_of(e, r, W);
            at = (long)r * W + cols.lo;
            n = cols.n;
            mask = 1ull << b;
        }
    }
    if (n <= ZT_SHORT)
        for (int i = 0; i < n; ++i) atomicOr(touch + at + i, mask);
    for (unsigned long long todo = __ballot(n > ZT_SHORT); todo; todo &= todo - 1) {  // the same in every lane
        const int src = __ffsll((long long)todo) - 1;
        const long s_at = __shfl(at, src, 64);
        const int s_n = __shfl(n, src, 64);
        const unsigned long long s_mask = __shfl(mask, src, 64);
        for (int i = lane; i < s_n; i += 64) atomicOr(touch + s_at + i, s_mask);
    }
}

// grid.x workgroups take rows blockIdx.x, blockIdx.x + gridDim.x, ...; a chunk is read (canvas and touch) before the scan's barrier and
// written after it, each thread its own columns.  The mask left of a thread's run is the exclusive prefix XOR the scan gives it, OR the
// touch bits of that column, which it reads itself: no further exchange between lanes.
__global__ __launch_bounds__(ZTPB) void zone_touch_merge_kernel(unsigned long long* __restrict__ canvas,
                                                                const unsigned long long* __restrict__ touch, int H, int W) {
    __shared__ unsigned long long wtot[2][ZWAVES];
    int par = 0;
    for (int r = blockIdx.x; r < H; r += gridDim.x) {
        unsigned long long* row = canvas + (long)r * W;
        const unsigned long long* trow = touch + (long)r * W;
        unsigned long long carry = 0;
        for (long c0 = 0; c0 < W; c0 += ZCHUNK, par ^= 1) {
            const long c = c0 + (long)threadIdx.x * ZVPT;
            unsigned long long v[ZVPT], tb[ZVPT];
            zone_load_toggles(v, row, c, W);
            zone_load_toggles(tb, trow, c, W);
            const unsigned long long left_touch = c > 0 && c < W ? trow[c - 1] : 0ull;
            const unsigned long long own = v[0];
            zone_scan_chunk(v, carry, wtot[par]);
            unsigned long long prev = c > 0 ? ((v[0] ^ own) | left_touch) : 0ull;  // m[c - 1]; XOR undoes itself: inclusive ^ own = exclusive
#pragma unroll
            for (int j = 0; j < ZVPT; ++j) {
                const unsigned long long m = v[j] | tb[j];
                if (c + j < W) row[c + j] = m ^ prev;
                prev = m;
            }
        }
    }
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
    const int lane = threadIdx.x & 63;
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
            zone_load_toggles(v, row, c, W);
#pragma unroll
            for (int j = 0; j < ZVPT; ++j) {
                k[j] = ncls;
                if (c + j < W) {
                    const int s = cls ? crow[c + j] : fill;
                    if (s != fill && s >= 0 && s < ncls) k[j] = s;
                }
            }
            zone_scan_chunk(v, carry, wtot[par]);
#pragma unroll
            for (int j = 0; j < ZVPT; ++j) {
                const bool live = c + j < W;
                const unsigned long long m = live ? v[j] : 0ull;
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

// ---- values: per zone and band (n, T, M2, min, max) of a float32 raster -----------------------------------------------------------------
// A partial result of the valid values of one zone and band: their number, their sum, the sum of their squared deviations from their own
// mean t / n, and their extremes.  32 bytes; the partials in memory are arrays of it.
struct __attribute__((aligned(16))) ZAcc {
    double n, t, m2;
    float lo, hi;
};
constexpr int ZV_MAX_BANDS = 8, ZV_MAX_WG = 512;
static_assert(sizeof(ZAcc) == 32, "the partials are (.., 4) float64 records");

__device__ __forceinline__ ZAcc zacc_empty() { return ZAcc{0.0, 0.0, 0.0, __builtin_huge_valf(), -__builtin_huge_valf()}; }

// Chan, Golub and LeVeque's pairwise update, a before b.  An empty side leaves the other's bits as they are.
__device__ __forceinline__ ZAcc zacc_merge(const ZAcc& a, const ZAcc& b) {
    ZAcc r;
    r.n = a.n + b.n;
    r.t = a.t + b.t;
    double w = 0.0;
    if (a.n > 0.0 && b.n > 0.0) {
        const double d = b.t / b.n - a.t / a.n;
        w = d * d * (a.n * b.n / r.n);
    }
    r.m2 = a.m2 + b.m2 + w;
    r.lo = fminf(a.lo, b.lo);
    r.hi = fmaxf(a.hi, b.hi);
    return r;
}

__device__ __forceinline__ ZAcc zacc_shfl_xor(const ZAcc& a, int o) {
    return ZAcc{__shfl_xor(a.n, o, 64), __shfl_xor(a.t, o, 64), __shfl_xor(a.m2, o, 64), __shfl_xor(a.lo, o, 64), __shfl_xor(a.hi, o, 64)};
}

// The rows, chunks and scan of zone_tally_kernel; the canvas is only read.  Per chunk a wave loops over the zone bits that any of its
// lanes is inside of (the OR of the lanes' masks: wave-uniform), band by band: every lane forms the triple of its own run (two passes
// over at most ZVPT values), a 6-step butterfly merges the 64 of them (the lower lane is the left operand, so both lanes of a pair
// compute the same bits), lane z keeps the result of bit z, and the lanes of the bits present then merge into the wave's own LDS
// accumulators acc[wave][band][64], which nobody else writes.  Lane z also counts the inside pixels of bit z in a register.  At the end
// waves 0..3 are merged in order into the workgroup's partials.  LDS (dynamic): acc, then pixw[ZWAVES][64] u32.
__global__ __launch_bounds__(ZTPB) void zone_value_tally_kernel(const unsigned long long* __restrict__ canvas, const float* __restrict__ raster,
                                                                ZAcc* __restrict__ partials, unsigned long long* __restrict__ pix_partials,
                                                                int H, int W, int B, int has_nodata, float nodata) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    ZAcc* acc = reinterpret_cast<ZAcc*>(smem);
    unsigned* pixw = reinterpret_cast<unsigned*>(acc + ZWAVES * B * ZBITS);
    __shared__ unsigned long long wtot[2][ZWAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < ZWAVES * B * ZBITS; i += ZTPB) acc[i] = zacc_empty();
    __syncthreads();
    ZAcc* mine_acc = acc + (long)wave * B * ZBITS;
    const long plane = (long)H * W;
    unsigned inside = 0;  // the inside pixels of bit `lane` this wave has met: at most H * W <= 2^31 - 1
    int par = 0;
    for (int r = blockIdx.x; r < H; r += gridDim.x) {
        const unsigned long long* row = canvas + (long)r * W;
        const float* vrow = raster + (long)r * W;
        unsigned long long carry = 0;
        for (long c0 = 0; c0 < W; c0 += ZCHUNK, par ^= 1) {
            const long c = c0 + (long)threadIdx.x * ZVPT;
            unsigned long long m[ZVPT];
            zone_load_toggles(m, row, c, W);
            zone_scan_chunk(m, carry, wtot[par]);  // the workgroup's only barrier in this loop: what follows is per wave
            unsigned long long present = 0;
#pragma unroll
            for (int j = 0; j < ZVPT; ++j) {
                if (c + j >= W) m[j] = 0ull;
                present |= m[j];
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) present |= __shfl_xor(present, o, 64);
            if (!present) continue;  // the same in every lane of the wave
            for (unsigned long long rest = present; rest; rest &= rest - 1) {
                const int z = __ffsll((long long)rest) - 1;
                unsigned cnt = 0;
#pragma unroll
                for (int j = 0; j < ZVPT; ++j) cnt += (unsigned)__popcll(__ballot((m[j] >> z) & 1ull));
                if (lane == z) inside += cnt;
            }
            for (int b = 0; b < B; ++b) {
                float x[ZVPT];
                bool ok[ZVPT];
#pragma unroll
                for (int j = 0; j < ZVPT; ++j) {
                    x[j] = c + j < W ? vrow[b * plane + c + j] : 0.f;
                    // finite (the exponent is not all ones) and not the no-data value
                    ok[j] = c + j < W && (__float_as_uint(x[j]) & 0x7f800000u) != 0x7f800000u && !(has_nodata && x[j] == nodata);
                }
                ZAcc keep = zacc_empty();  // lane z: the wave's result of bit z
                for (unsigned long long rest = present; rest; rest &= rest - 1) {
                    const int z = __ffsll((long long)rest) - 1;
                    ZAcc a = zacc_empty();
                    bool in[ZVPT];
#pragma unroll
                    for (int j = 0; j < ZVPT; ++j) {
                        in[j] = ok[j] && ((m[j] >> z) & 1ull);
                        if (in[j]) {
                            a.n += 1.0;
                            a.t += (double)x[j];
                            a.lo = fminf(a.lo, x[j]);
                            a.hi = fmaxf(a.hi, x[j]);
                        }
                    }
                    if (__ballot(a.n > 0.0) == 0ull) continue;  // no valid value of this bit in the wave: keep stays empty
                    if (a.n > 0.0) {
                        const double mean = a.t / a.n;
#pragma unroll
                        for (int j = 0; j < ZVPT; ++j) {
                            const double d = (double)x[j] - mean;
                            if (in[j]) a.m2 += d * d;
                        }
                    }
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) {
                        const ZAcc other = zacc_shfl_xor(a, o);
                        const bool upper = (lane & o) != 0;
                        a = zacc_merge(upper ? other : a, upper ? a : other);
                    }
                    if (lane == z) keep = a;
                }
                if ((present >> lane) & 1ull) {
                    ZAcc* slot = mine_acc + b * ZBITS + lane;
                    *slot = zacc_merge(*slot, keep);
                }
            }
        }
    }
    pixw[wave * ZBITS + lane] = inside;
    __syncthreads();
    for (int i = threadIdx.x; i < B * ZBITS; i += ZTPB) {  // i = band * 64 + bit
        ZAcc a = acc[i];
#pragma unroll
        for (int w = 1; w < ZWAVES; ++w) a = zacc_merge(a, acc[w * B * ZBITS + i]);
        partials[(long)blockIdx.x * B * ZBITS + i] = a;
    }
    if (threadIdx.x < ZBITS) {
        unsigned long long total = 0;
#pragma unroll
        for (int w = 0; w < ZWAVES; ++w) total += pixw[w * ZBITS + threadIdx.x];
        pix_partials[(long)blockIdx.x * ZBITS + threadIdx.x] = total;
    }
}

// One workgroup per band, one thread per zone bit: the G partials merged in workgroup order.
__global__ __launch_bounds__(ZBITS) void zone_value_reduce_kernel(const ZAcc* __restrict__ partials,
                                                                  const unsigned long long* __restrict__ pix_partials,
                                                                  long long* __restrict__ valid, double* __restrict__ stats,
                                                                  long long* __restrict__ pixels, int G, int B) {
    const int z = threadIdx.x, b = blockIdx.x;
    ZAcc a = zacc_empty();
    for (int g = 0; g < G; ++g) a = zacc_merge(a, partials[((long)g * B + b) * ZBITS + z]);
    valid[z * B + b] = (long long)a.n;
    double* out = stats + ((long)z * B + b) * 4;
    out[0] = a.n > 0.0 ? a.t / a.n : 0.0;
    out[1] = a.m2;
    out[2] = (double)a.lo;
    out[3] = (double)a.hi;
    if (b == 0 && pixels) {
        unsigned long long total = 0;
        for (int g = 0; g < G; ++g) total += pix_partials[(long)g * ZBITS + z];
        pixels[z] = (long long)total;
    }
}

// ---- order statistics: per zone and band the values of given ranks (the median, percentiles) ------------------------------------------------
// Radix selection, most significant digit first, on order-preserving keys (the rule: include/instageo_hip.h).  ZQ_ROUNDS rounds of
// ZQ_DIGIT bits; a round is one histogram launch and one pick launch.
constexpr int ZQ_ROUNDS = 4, ZQ_DIGIT = 8, ZQ_BINS = 1 << ZQ_DIGIT;
constexpr int ZQ_MAX_Q = 8, ZQ_MAX_SLOTS = 2 * ZQ_MAX_Q;
constexpr int ZQ_MERGE = 8;               // digits a wave merges before the lanes left over add on their own
constexpr unsigned ZQ_DEAD = 0xFFFFFFFFu;  // the rank of a slot whose zone has no valid value
static_assert(ZQ_ROUNDS * ZQ_DIGIT == 32, "the rounds cover the key");

struct ZFractions {
    double f[ZQ_MAX_Q];
};

// ascending floats <-> ascending unsigned keys; zeros are canonical (-0.0 + 0.0 = +0.0)
__device__ __forceinline__ unsigned zq_key(float v) {
    const unsigned u = __float_as_uint(v + 0.0f);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float zq_unkey(unsigned k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }

// bins[d[j]] += 1 for every j with act[j], over the wave: up to ZQ_MERGE times the digit of the first lane that still has one is taken,
// every (lane, j) that holds it is counted by ballots and that lane adds the count once; what is left adds one by one.  Integer adds: the
// sums do not depend on any of this.  `bins` is the same in every lane; every lane of the wave calls it.
__device__ __forceinline__ void zq_wave_add(unsigned* bins, bool (&act)[ZVPT], const unsigned (&d)[ZVPT], int lane) {
    for (int it = 0; it < ZQ_MERGE; ++it) {
        bool any = false;
        unsigned mine = 0;
#pragma unroll
        for (int j = ZVPT - 1; j >= 0; --j)
            if (act[j]) any = true, mine = d[j];
        const unsigned long long todo = __ballot(any);
        if (!todo) return;
        const int src = __ffsll((long long)todo) - 1;
        const unsigned digit = __shfl(mine, src, 64);
        unsigned cnt = 0;
#pragma unroll
        for (int j = 0; j < ZVPT; ++j) {
            const bool hit = act[j] && d[j] == digit;
            cnt += (unsigned)__popcll(__ballot(hit));
            act[j] = act[j] && !hit;
        }
        if (lane == src) atomicAdd(bins + digit, cnt);
    }
#pragma unroll
    for (int j = 0; j < ZVPT; ++j)
        if (act[j]) atomicAdd(bins + d[j], 1u);
}

// Round `round` of a selection: the rows, chunks, scan and validity test of zone_value_tally_kernel.  Per chunk and band a wave walks
// the zone bits any of its lanes is inside of and, per bit, the leader slots of (band, bit): the lanes whose key continues the slot's
// prefix add their digit to hist[band][bit][slot][.].  Round 0 has no prefix: slot 0 counts every valid value and state is not read.
// state: (B, 64, S) x {prefix, rank, leader, -}.  Every index into hist is below B * 64 * S * 256 (band < B, bit < 64, slot < S, digit < 256).
__global__ __launch_bounds__(ZTPB) void zone_quantile_hist_kernel(const unsigned long long* __restrict__ canvas, const float* __restrict__ raster,
                                                                  const uint4* __restrict__ state, unsigned* __restrict__ hist, int H, int W,
                                                                  int B, int S, int round, int has_nodata, float nodata) {
    __shared__ unsigned long long wtot[2][ZWAVES];
    const int lane = threadIdx.x & 63;
    const long plane = (long)H * W;
    const int shift = 32 - ZQ_DIGIT * round;  // the key bits from here up are the prefix (round >= 1: 24, 16, 8)
    int par = 0;
    for (int r = blockIdx.x; r < H; r += gridDim.x) {
        const unsigned long long* row = canvas + (long)r * W;
        const float* vrow = raster + (long)r * W;
        unsigned long long carry = 0;
        for (long c0 = 0; c0 < W; c0 += ZCHUNK, par ^= 1) {
            const long c = c0 + (long)threadIdx.x * ZVPT;
            unsigned long long m[ZVPT];
            zone_load_toggles(m, row, c, W);
            zone_scan_chunk(m, carry, wtot[par]);  // the workgroup's only barrier in this loop: what follows is per wave
            unsigned long long present = 0;
#pragma unroll
            for (int j = 0; j < ZVPT; ++j) {
                if (c + j >= W) m[j] = 0ull;
                present |= m[j];
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) present |= __shfl_xor(present, o, 64);
            if (!present) continue;  // the same in every lane of the wave
            for (int b = 0; b < B; ++b) {
                unsigned key[ZVPT], dig[ZVPT];
                bool ok[ZVPT];
#pragma unroll
                for (int j = 0; j < ZVPT; ++j) {
                    const float x = c + j < W ? vrow[b * plane + c + j] : 0.f;
                    ok[j] = c + j < W && (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u && !(has_nodata && x == nodata);
                    key[j] = zq_key(x);
                    dig[j] = (key[j] >> (shift - ZQ_DIGIT)) & (unsigned)(ZQ_BINS - 1);
                }
                for (unsigned long long rest = present; rest; rest &= rest - 1) {
                    const int z = __ffsll((long long)rest) - 1;
                    const long cell = ((long)b * ZBITS + z) * S;
                    bool in[ZVPT];
                    bool some = false;
#pragma unroll
                    for (int j = 0; j < ZVPT; ++j) {
                        in[j] = ok[j] && ((m[j] >> z) & 1ull);
                        some = some || in[j];
                    }
                    if (__ballot(some) == 0ull) continue;
                    if (round == 0) {
                        zq_wave_add(hist + cell * ZQ_BINS, in, dig, lane);
                        continue;
                    }
                    for (int s = 0; s < S; ++s) {
                        const uint4 st = state[cell + s];  // the same address in every lane
                        if (st.z != (unsigned)s) continue;  // another slot with this prefix counts for it
                        bool act[ZVPT];
#pragma unroll
                        for (int j = 0; j < ZVPT; ++j) act[j] = in[j] && (key[j] >> shift) == (st.x >> shift);
                        zq_wave_add(hist + (cell + s) * ZQ_BINS, act, dig, lane);
                    }
                }
            }
        }
    }
}

// One workgroup per (band, zone bit), one thread per slot.  See include/instageo_hip.h.
__global__ __launch_bounds__(ZQ_MAX_SLOTS) void zone_quantile_pick_kernel(unsigned* __restrict__ hist, uint4* __restrict__ state,
                                                                          const ZFractions fr, long long* __restrict__ valid,
                                                                          float* __restrict__ order, int B, int S, int round) {
#pragma clang fp contract(off)
    __shared__ unsigned pre[ZQ_MAX_SLOTS], dead[ZQ_MAX_SLOTS];
    const int s = threadIdx.x, b = blockIdx.x / ZBITS, z = blockIdx.x % ZBITS;
    const long cell = (long)blockIdx.x * S;
    const bool live = s < S;
    uint4 st = make_uint4(0u, 0u, 0u, 0u);  // round 0: empty prefix, slot 0 leads
    if (live && round > 0) st = state[cell + s];
    const uint4* bins = reinterpret_cast<const uint4*>(hist + (cell + (live ? st.z : 0u)) * ZQ_BINS);
    if (live && round == 0) {
        unsigned n = 0;
        for (int i = 0; i < ZQ_BINS / 4; ++i) {
            const uint4 q = bins[i];
            n += q.x + q.y + q.z + q.w;
        }
        if (s == 0) valid[(long)z * B + b] = (long long)n;
        if (n == 0) {
            st.y = ZQ_DEAD;
        } else {
            const double h = (double)(n - 1u) * fr.f[s >> 1];
            const unsigned lo = (unsigned)floor(h);
            const unsigned hi = lo + 1u < n - 1u ? lo + 1u : n - 1u;
            st.y = (s & 1) ? hi : lo;
        }
    }
    const bool sel = live && st.y != ZQ_DEAD;
    if (sel) {
        unsigned cum = 0, digit = 0, below = 0;
        bool found = false;
        for (int i = 0; i < ZQ_BINS / 4; ++i) {  // no early exit: the loads do not wait for one another
            const uint4 q = bins[i];
            const unsigned cnt[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!found && cum + cnt[k] > st.y) found = true, digit = (unsigned)(4 * i + k), below = cum;
                cum += cnt[k];
            }
        }
        st.y -= below;
        st.x |= digit << (32 - ZQ_DIGIT * (round + 1));
    }
    pre[s] = st.x;
    dead[s] = sel ? 0u : 1u;
    __syncthreads();  // every slot has read its leader's bins
    if (live && st.z == (unsigned)s && round + 1 < ZQ_ROUNDS) {
        uint4* mine = reinterpret_cast<uint4*>(hist + (cell + s) * ZQ_BINS);
        for (int i = 0; i < ZQ_BINS / 4; ++i) mine[i] = make_uint4(0u, 0u, 0u, 0u);
    }
    if (!live) return;
    unsigned lead = (unsigned)s;
    for (int t = s - 1; t >= 0; --t)
        if (sel && !dead[t] && pre[t] == st.x) lead = (unsigned)t;
    st.z = lead;
    state[cell + s] = st;
    if (round + 1 == ZQ_ROUNDS) order[((long)z * B + b) * S + s] = sel ? zq_unkey(st.x) : __builtin_nanf("");
}

}  // namespace

#define ST(s) ((hipStream_t)(s))
#define IG_REQUIRE_RASTER(name)                                                                     \
    IG_REQUIRE(H >= 0 && W >= 0, name ": need H >= 0 and W >= 0 (H %d, W %d)", H, W);               \
    IG_REQUIRE((long)H * W <= 0x7fffffffL, name ": H * W = %ld exceeds 2^31 - 1", (long)H * W)

// the checks of the two launches over edges (rows of `edges`, E, H) and of the two over (edge, row) items, whose T counts `items` and
// which write the canvas `out`; an empty call returns before a pointer is looked at
#define IG_REQUIRE_EDGE_ROWS(name)                                                           \
    IG_REQUIRE(E >= 0 && E <= 0x7fffffffL, name ": need 0 <= E <= 2^31 - 1 (got %ld)", E);   \
    IG_REQUIRE(H >= 0, name ": need H >= 0 (got %d)", H);                                    \
    if (E == 0) return IG_OK;                                                                \
    IG_REQUIRE(edges && rows, name ": null pointer");                                        \
    IG_REQUIRE(((uintptr_t)edges & 15) == 0, name ": edges must be 16-byte aligned")
#define IG_REQUIRE_EDGE_ITEMS(name, out, items)                                                              \
    IG_REQUIRE(E >= 0 && E <= 0x7fffffffL, name ": need 0 <= E <= 2^31 - 1 (got %ld)", E);                   \
    IG_REQUIRE(T >= 0 && T <= (1L << 38), name ": need 0 <= T <= 2^38 " items " per call (got %ld)", T);     \
    IG_REQUIRE_RASTER(name);                                                                                 \
    if (E == 0 || T == 0 || (long)H * W == 0) return IG_OK;                                                  \
    IG_REQUIRE(edges && bit && first && out, name ": null pointer");                                         \
    IG_REQUIRE(((uintptr_t)edges & 15) == 0, name ": edges must be 16-byte aligned");                        \
    IG_REQUIRE(((uintptr_t)first & 7) == 0 && ((uintptr_t)out & 7) == 0, name ": first and " #out " must be 8-byte aligned")

static inline dim3 blocks_for(long items) { return dim3((unsigned)((items + ZTPB - 1) / ZTPB)); }

extern "C" {

int ig_zone_edge_rows(const int* edges, int* rows, long E, int H, void* stream) {
    IG_REQUIRE_EDGE_ROWS("ig_zone_edge_rows");
    return ig_launch<zone_rows_kernel<rows_of>>("ig_zone_edge_rows", blocks_for(E), dim3(ZTPB), 0, ST(stream), (const int4*)edges, rows, E, H);
}

int ig_zone_toggle(const int* edges, const unsigned char* bit, const long long* first, unsigned long long* canvas, long E, long T, int H,
                   int W, void* stream) {
    IG_REQUIRE_EDGE_ITEMS("ig_zone_toggle", canvas, "crossings");
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

int ig_zone_touch_rows(const int* edges, int* rows, long E, int H, void* stream) {
    IG_REQUIRE_EDGE_ROWS("ig_zone_touch_rows");
    return ig_launch<zone_rows_kernel<touch_rows_of>>("ig_zone_touch_rows", blocks_for(E), dim3(ZTPB), 0, ST(stream), (const int4*)edges, rows, E,
                                                      H);
}

int ig_zone_touch(const int* edges, const unsigned char* bit, const long long* first, unsigned long long* touch, long E, long T, int H, int W,
                  void* stream) {
    IG_REQUIRE_EDGE_ITEMS("ig_zone_touch", touch, "touched rows");
    return ig_launch<zone_touch_kernel>("ig_zone_touch", blocks_for(T), dim3(ZTPB), 0, ST(stream), (const int4*)edges, bit, first, touch, E, T,
                                        H, W);
}

int ig_zone_touch_merge(unsigned long long* canvas, const unsigned long long* touch, int H, int W, void* stream) {
    IG_REQUIRE_RASTER("ig_zone_touch_merge");
    if ((long)H * W == 0) return IG_OK;
    IG_REQUIRE(canvas && touch, "ig_zone_touch_merge: null pointer");
    IG_REQUIRE(((uintptr_t)canvas & 7) == 0 && ((uintptr_t)touch & 7) == 0, "ig_zone_touch_merge: canvas and touch must be 8-byte aligned");
    IG_REQUIRE(canvas != touch, "ig_zone_touch_merge: canvas and touch must be two canvases");
    return ig_launch<zone_touch_merge_kernel>("ig_zone_touch_merge", dim3((unsigned)(H < MAX_WG ? H : MAX_WG)), dim3(ZTPB), 0, ST(stream), canvas,
                                              touch, H, W);
}

int ig_zone_value_grid(int H) { return H < 0 ? 0 : H < ZV_MAX_WG ? H : ZV_MAX_WG; }

int ig_zone_value_tally(const unsigned long long* canvas, const float* raster, double* partials, unsigned long long* pix_partials, int H,
                        int W, int B, int has_nodata, float nodata, void* stream) {
    IG_REQUIRE(B >= 0 && B <= ZV_MAX_BANDS, "ig_zone_value_tally: 0 <= B <= %d bands per call (got %d)", ZV_MAX_BANDS, B);
    IG_REQUIRE_RASTER("ig_zone_value_tally");
    if ((long)H * W == 0 || B == 0) return IG_OK;
    IG_REQUIRE(canvas && raster && partials && pix_partials, "ig_zone_value_tally: null pointer");
    IG_REQUIRE(((uintptr_t)canvas & 7) == 0 && ((uintptr_t)partials & 15) == 0 && ((uintptr_t)pix_partials & 7) == 0,
               "ig_zone_value_tally: canvas and pix_partials must be 8-byte aligned, partials 16-byte");
    IG_REQUIRE(((uintptr_t)raster & 3) == 0, "ig_zone_value_tally: raster must be 4-byte aligned");
    return ig_launch<zone_value_tally_kernel>("ig_zone_value_tally", dim3((unsigned)ig_zone_value_grid(H)), dim3(ZTPB),
                                              ZWAVES * ZBITS * (B * (int)sizeof(ZAcc) + 4), ST(stream), canvas, raster,
                                              reinterpret_cast<ZAcc*>(partials), pix_partials, H, W, B, has_nodata, nodata);
}

int ig_zone_value_reduce(const double* partials, const unsigned long long* pix_partials, long long* valid, double* stats,
                         long long* pixels, int G, int B, void* stream) {
    IG_REQUIRE(B >= 0 && B <= ZV_MAX_BANDS, "ig_zone_value_reduce: 0 <= B <= %d bands per call (got %d)", ZV_MAX_BANDS, B);
    IG_REQUIRE(G >= 0 && G <= ZV_MAX_WG, "ig_zone_value_reduce: 0 <= G <= %d workgroups (got %d)", ZV_MAX_WG, G);
    if (G == 0 || B == 0) return IG_OK;
    IG_REQUIRE(partials && pix_partials && valid && stats, "ig_zone_value_reduce: null pointer");
    IG_REQUIRE((((uintptr_t)pix_partials | (uintptr_t)valid | (uintptr_t)stats | (uintptr_t)pixels) & 7) == 0 && ((uintptr_t)partials & 15) == 0,
               "ig_zone_value_reduce: every pointer must be 8-byte aligned, partials 16-byte");
    return ig_launch<zone_value_reduce_kernel>("ig_zone_value_reduce", dim3((unsigned)B), dim3(ZBITS), 0, ST(stream),
                                               reinterpret_cast<const ZAcc*>(partials), pix_partials, valid, stats, pixels, G, B);
}

#define IG_REQUIRE_SELECTION(name)                                                                                            \
    IG_REQUIRE(B >= 0 && B <= ZV_MAX_BANDS, name ": 0 <= B <= %d bands per selection (got %d)", ZV_MAX_BANDS, B);             \
    IG_REQUIRE(Q >= 0 && Q <= ZQ_MAX_Q, name ": 0 <= Q <= %d fractions per selection (got %d)", ZQ_MAX_Q, Q);                 \
    IG_REQUIRE(round >= 0 && round < ZQ_ROUNDS, name ": round must be 0..%d (got %d)", ZQ_ROUNDS - 1, round)

int ig_zone_quantile_hist(const unsigned long long* canvas, const float* raster, const unsigned* state, unsigned* hist, int H, int W,
                          int B, int Q, int round, int has_nodata, float nodata, void* stream) {
    IG_REQUIRE_SELECTION("ig_zone_quantile_hist");
    IG_REQUIRE_RASTER("ig_zone_quantile_hist");
    if ((long)H * W == 0 || B == 0 || Q == 0) return IG_OK;
    IG_REQUIRE(canvas && raster && state && hist, "ig_zone_quantile_hist: null pointer");
    IG_REQUIRE(((uintptr_t)canvas & 7) == 0 && (((uintptr_t)state | (uintptr_t)hist) & 15) == 0 && ((uintptr_t)raster & 3) == 0,
               "ig_zone_quantile_hist: canvas must be 8-byte aligned, state and hist 16-byte, raster 4-byte");
    return ig_launch<zone_quantile_hist_kernel>("ig_zone_quantile_hist", dim3((unsigned)ig_zone_value_grid(H)), dim3(ZTPB), 0, ST(stream),
                                                canvas, raster, reinterpret_cast<const uint4*>(state), hist, H, W, B, 2 * Q, round, has_nodata,
                                                nodata);
}

int ig_zone_quantile_pick(unsigned* hist, unsigned* state, const double* fractions, long long* valid, float* order, int B, int Q,
                          int round, void* stream) {
    IG_REQUIRE_SELECTION("ig_zone_quantile_pick");
    if (B == 0 || Q == 0) return IG_OK;
    IG_REQUIRE(hist && state && fractions && valid && order, "ig_zone_quantile_pick: null pointer");
    IG_REQUIRE((((uintptr_t)state | (uintptr_t)hist) & 15) == 0 && ((uintptr_t)valid & 7) == 0 && ((uintptr_t)order & 3) == 0,
               "ig_zone_quantile_pick: state and hist must be 16-byte aligned, valid 8-byte, order 4-byte");
    ZFractions fr = {};
    for (int q = 0; q < Q; ++q) {
        IG_REQUIRE(fractions[q] >= 0.0 && fractions[q] <= 1.0, "ig_zone_quantile_pick: fraction %d = %g is outside [0, 1]", q, fractions[q]);
        fr.f[q] = fractions[q];
    }
    return ig_launch<zone_quantile_pick_kernel>("ig_zone_quantile_pick", dim3((unsigned)(B * ZBITS)), dim3(ZQ_MAX_SLOTS), 0, ST(stream), hist,
                                                reinterpret_cast<uint4*>(state), fr, valid, order, B, 2 * Q, round);
}

}  // extern "C"
