// Region post-processing of int8 class maps for gfx950: connected-component labelling, region areas, the minimum-mapping-unit sieve
// and per-region statistics.  Everything is integer arithmetic; every result is unique (independent of scheduling).
//
// Labelling: a pixel's label is the smallest row-major index y * W + x of its component (same class, 4- or 8-connected); fill = -1.
//   1  ccl_tile_kernel     one workgroup per CT_W x CT_H tile: union-find in LDS over tile-local indices (row-major inside a tile agrees
//                          with the global order), then labels[p] = global index of p's tile-local root
//   2  ccl_merge_kernel    every same-class pixel pair that crosses a tile border is united in global memory (labels is the parent array)
//   3  ccl_flatten_kernel  labels[p] = find(p)
// Invariant: parent[p] <= p and parent[p] lies in p's component, at every moment.  The only writes to a parent are integer atomic mins
// with a member of the same set (a link hangs the LARGER root under the smaller, path compression lowers a parent to an ancestor), so
// the root of a set is its minimum index whatever the order of the atomics: the result is bit-identical from run to run.
// Parents are read with relaxed agent-scope atomic loads (a plain load may be served stale by another XCD's L2); a stale parent is
// still an ancestor, it only costs a step or a retry.
// Redundant pairs are skipped: a vertical pair whose left neighbours form the same pair, a diagonal pair that an edge pair already
// joins.  Each skipped pair is implied by performed ones (induction towards the start of the run / the tile edge; pairs at a tile
// corner are never skipped, which keeps the induction free of cycles), so a one-class map costs one union per tile border.
//
// Every data-dependent loop is capped.  Tile-local chains strictly decrease inside [0, CT_PIX), so CT_PIX steps always suffice there.
// In global memory a chain passes through tile-local roots only (at most one per tile: <= 2^21 tiles for H, W >= 16); FIND_CAP = 2^22
// steps and UNION_CAP retries are far beyond what compression leaves, and a lane that reaches a cap stops, sets *status and every other
// lane leaves its loop at its next look at *status (once per 256 steps): a bug cannot spin.  The host raises on a nonzero status.
#include "common.h"
#include "segreduce.h"

namespace {

constexpr int CT_W = 64, CT_H = 16, CT_PIX = CT_W * CT_H, CTPB = 256;
constexpr int FIND_CAP = 1 << 22, UNION_CAP = 1 << 20;
constexpr int RTPB = 256, RUN = 4;  // region reductions: RUN consecutive pixels per thread
constexpr int NOCLS = -1000;        // LDS class of a fill pixel or a pixel outside the image (no int8 value)
enum { ST_FIND_CAP = 1, ST_UNION_CAP = 2, ST_TILE_CAP = 4 };

#define RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
#define RLX_WG __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP

// ---- tile-local union-find in LDS ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int lds_find(int* par, int x) {
    for (int it = 0; it < CT_PIX; ++it) {  // parents strictly decrease inside [0, CT_PIX)
        const int p = __hip_atomic_load(&par[x], RLX_WG);
        if (p == x) return x;
        x = p;
    }
    return -1;
}

// the larger of the two roots strictly decreases with every failed attempt: at most CT_PIX attempts
__device__ __forceinline__ bool lds_union(int* par, int a, int b) {
    for (int it = 0; it < CT_PIX; ++it) {
        a = lds_find(par, a);
        b = lds_find(par, b);
        if (a < 0 || b < 0) return false;
        if (a == b) return true;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = __hip_atomic_fetch_min(&par[a], b, RLX_WG);
        if (old == a) return true;
        a = old;  // a was no root any more: its former parent and b still have to meet
    }
    return false;
}

// grid.x = tiles of one image (row-major), grid.y = image
__global__ __launch_bounds__(CTPB) void ccl_tile_kernel(const signed char* __restrict__ cls, int* __restrict__ labels, int H, int W,
                                                        int tiles_x, int conn8, int fill, int* __restrict__ status) {
    __shared__ int par[CT_PIX];
    __shared__ short cl[CT_PIX];
    const long base = (long)blockIdx.y * H * W;
    const int ty0 = ((int)blockIdx.x / tiles_x) * CT_H, tx0 = ((int)blockIdx.x % tiles_x) * CT_W;
    const int lx = threadIdx.x % CT_W, ly0 = threadIdx.x / CT_W;  // this thread: column lx, rows ly0, ly0 + 4, ...
    const int gx = tx0 + lx;
    constexpr int PER = CT_PIX / CTPB, STEP = CTPB / CT_W;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int ly = ly0 + k * STEP, gy = ty0 + ly;
        int c = NOCLS;
        if (gx < W && gy < H) {
            const int v = cls[base + (long)gy * W + gx];
            if (v != fill) c = v;
        }
        cl[ly * CT_W + lx] = (short)c;
    }
    __syncthreads();
    // rows: link to the left neighbour, then flatten every run to its first pixel (chains of at most CT_W - 1 steps)
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int i = (ly0 + k * STEP) * CT_W + lx;
        par[i] = (lx > 0 && cl[i] != NOCLS && cl[i] == cl[i - 1]) ? i - 1 : i;
    }
    __syncthreads();
    int run[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        int r = (ly0 + k * STEP) * CT_W + lx;
        for (int it = 0; it < CT_W; ++it) {
            const int p = par[r];
            if (p == r) break;
            r = p;
        }
        run[k] = r;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PER; ++k) par[(ly0 + k * STEP) * CT_W + lx] = run[k];
    __syncthreads();
    // columns and diagonals
    bool ok = true;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int ly = ly0 + k * STEP, i = ly * CT_W + lx;
        const int c = cl[i];
        if (c == NOCLS || ly == 0) continue;
        const bool up = cl[i - CT_W] == c;
        const bool left = lx > 0 && cl[i - 1] == c, right = lx < CT_W - 1 && cl[i + 1] == c;
        const bool ul = lx > 0 && cl[i - CT_W - 1] == c, ur = lx < CT_W - 1 && cl[i - CT_W + 1] == c;
        if (up && !(left && ul)) ok &= lds_union(par, i, i - CT_W);
        if (conn8) {
            if (ul && !up && !left) ok &= lds_union(par, i, i - CT_W - 1);
            if (ur && !up && !right) ok &= lds_union(par, i, i - CT_W + 1);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int ly = ly0 + k * STEP, gy = ty0 + ly, i = ly * CT_W + lx;
        if (gx >= W || gy >= H) continue;
        int out = -1;
        if (cl[i] != NOCLS) {
            const int r = lds_find(par, i);
            if (r < 0) ok = false;
            else out = (ty0 + r / CT_W) * W + tx0 + r % CT_W;  // < H * W <= 2^31 - 1
        }
        labels[base + (long)gy * W + gx] = out;
    }
    if (!ok) atomicOr(status, ST_TILE_CAP);
}

// ---- union-find in global memory (par = the labels of one image) -------------------------------------------------------------------
// root of x, or -1 at the cap / once another lane has set *status; lowers the parents on the path to the root found
__device__ __forceinline__ int g_find(int* par, int x, int* status) {
    int r = x, depth = 0;
    for (;; ++depth) {
        if (depth >= FIND_CAP) {
            atomicOr(status, ST_FIND_CAP);
            return -1;
        }
        if ((depth & 255) == 255 && __hip_atomic_load(status, RLX_AGENT) != 0) return -1;
        const int p = __hip_atomic_load(&par[r], RLX_AGENT);
        if (p == r) break;
        r = p;
    }
    if (depth >= 2) {  // path compression: r is an ancestor of every node on the path (and still is if r has since been linked)
        for (int it = 0; it < depth && x > r; ++it) {
            const int p = __hip_atomic_load(&par[x], RLX_AGENT);
            if (p > r) __hip_atomic_fetch_min(&par[x], r, RLX_AGENT);
            x = p;
        }
    }
    return r;
}

__device__ __forceinline__ void g_union(int* par, int a, int b, int* status) {
    for (int it = 0; it < UNION_CAP; ++it) {
        a = g_find(par, a, status);
        b = g_find(par, b, status);
        if (a < 0 || b < 0 || a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = __hip_atomic_fetch_min(&par[a], b, RLX_AGENT);  // the larger root under the smaller
        if (old == a) return;
        a = old;  // a had been linked meanwhile: its former parent and b still have to meet
    }
    atomicOr(status, ST_UNION_CAP);
}

// one thread per pixel (grid.y = image); only pixels with a backward neighbour (left, up, up-left, up-right) in another tile work
__global__ __launch_bounds__(CTPB) void ccl_merge_kernel(const signed char* __restrict__ cls, int* __restrict__ labels, int H, int W,
                                                         int conn8, int fill, int* __restrict__ status) {
    const long HW = (long)H * W;
    const long p = blockIdx.x * (long)CTPB + threadIdx.x;
    if (p >= HW) return;
    const int y = (int)(p / W), x = (int)(p - (long)y * W);
    const bool edge_l = x % CT_W == 0 && x > 0, edge_u = y % CT_H == 0 && y > 0, edge_r = x % CT_W == CT_W - 1 && x < W - 1;
    if (!(edge_l || edge_u || (conn8 && edge_r && y > 0))) return;
    const signed char* c = cls + (long)blockIdx.y * HW;
    int* par = labels + (long)blockIdx.y * HW;
    const int v = c[p];
    if (v == fill) return;
    const bool up = y > 0 && c[p - W] == v, left = x > 0 && c[p - 1] == v;
    const bool ul = y > 0 && x > 0 && c[p - W - 1] == v;
    if (edge_l && left && !(y % CT_H != 0 && up && ul)) g_union(par, (int)p, (int)p - 1, status);
    if (edge_u && up && !(x % CT_W != 0 && left && ul)) g_union(par, (int)p, (int)p - W, status);
    if (conn8 && y > 0) {
        if ((edge_l || edge_u) && ul && !up && !left) g_union(par, (int)p, (int)p - W - 1, status);
        if (x < W - 1 && (edge_u || edge_r) && c[p - W + 1] == v && !up && c[p + 1] != v) g_union(par, (int)p, (int)p - W + 1, status);
    }
}

__global__ __launch_bounds__(CTPB) void ccl_flatten_kernel(int* __restrict__ labels, long HW, int* __restrict__ status) {
    const long p = blockIdx.x * (long)CTPB + threadIdx.x;
    if (p >= HW) return;
    int* par = labels + (long)blockIdx.y * HW;
    const int l = __hip_atomic_load(&par[p], RLX_AGENT);
    if (l < 0) return;
    const int r = g_find(par, l, status);
    if (r >= 0 && r != l) __hip_atomic_store(&par[p], r, RLX_AGENT);  // an ancestor replaces an ancestor: concurrent finds stay valid
}

// area[root] = pixels of the region, 0 elsewhere (area zeroed by the entry point); grid.y = image
__global__ __launch_bounds__(RTPB) void region_area_kernel(const int* __restrict__ labels, int* __restrict__ area, long HW) {
    const int* lab = labels + (long)blockIdx.y * HW;
    int* ar = area + (long)blockIdx.y * HW;
    const long p0 = (blockIdx.x * (long)RTPB + threadIdx.x) * RUN;
    int key = -1, cnt = 0;  // the run of equal roots this thread is in
#pragma unroll
    for (int k = 0; k < RUN; ++k) {
        const int r = p0 + k < HW ? lab[p0 + k] : -1;
        if (r != key) {
            if (key >= 0) atomicAdd(&ar[key], cnt);
            key = r;
            cnt = 0;
        }
        ++cnt;
    }
    const Seg s = seg_of(key);
    const int tot = seg_reduce<OpAdd>(cnt, s);
    if (s.head && key >= 0) atomicAdd(&ar[key], tot);
}

// ---- sieve ------------------------------------------------------------------------------------------------------------------------
// select: every pixel of a small region offers its kept 4-neighbours to best[root of the small region]
__global__ __launch_bounds__(RTPB) void sieve_select_kernel(const int* __restrict__ labels, const int* __restrict__ area, int min_region,
                                                            int H, int W, unsigned long long* __restrict__ best) {
    const long HW = (long)H * W;
    const long p = blockIdx.x * (long)RTPB + threadIdx.x;
    if (p >= HW) return;
    const long base = (long)blockIdx.y * HW;
    const int* lab = labels + base;
    const int* ar = area + base;
    const int R = lab[p];
    if (R < 0 || ar[R] >= min_region) return;
    const int y = (int)(p / W), x = (int)(p - (long)y * W);
    unsigned long long key = 0;
    auto offer = [&](long q) {
        const int S = lab[q];
        if (S < 0 || S == R) return;
        const int a = ar[S];
        if (a < min_region) return;
        const unsigned long long k = ((unsigned long long)(unsigned)a << 32) | (0xFFFFFFFFull - (unsigned)S);
        if (k > key) key = k;
    };
    if (y > 0) offer(p - W);
    if (x > 0) offer(p - 1);
    if (x < W - 1) offer(p + 1);
    if (y < H - 1) offer(p + W);
    if (key) atomicMax(&best[base + R], key);
}

// apply: the pixels of a small region with a winner take the class of the winner's root pixel (a kept region: unchanged in this pass)
__global__ __launch_bounds__(RTPB) void sieve_apply_kernel(signed char* __restrict__ cls, const int* __restrict__ labels,
                                                           const int* __restrict__ area, int min_region, long HW,
                                                           const unsigned long long* __restrict__ best, int* __restrict__ changed) {
    const long p = blockIdx.x * (long)RTPB + threadIdx.x;
    const long base = (long)blockIdx.y * HW;
    bool root_changed = false;
    if (p < HW) {
        const int R = labels[base + p];
        if (R >= 0 && area[base + R] < min_region) {
            const unsigned long long b = best[base + R];
            if (b) {
                const long S = (long)(0xFFFFFFFFull - (b & 0xFFFFFFFFull));
                cls[base + p] = cls[base + S];
                root_changed = p == R;
            }
        }
    }
    const unsigned long long m = __ballot(root_changed);  // one atomic per wave
    if (m && (threadIdx.x & 63) == 0) atomicAdd(changed, __popcll(m));
}

// ---- per-region statistics --------------------------------------------------------------------------------------------------------
constexpr int NSTAT = 7;  // area, row_min, row_max, col_min, col_max, row_sum, col_sum
__global__ __launch_bounds__(RTPB) void region_stats_init_kernel(long long* __restrict__ stats, long R) {
    const long i = blockIdx.x * (long)RTPB + threadIdx.x;
    if (i >= R) return;
    long long* s = stats + i * NSTAT;
    s[0] = 0;
    s[1] = 0x7fffffffLL;
    s[2] = -1;
    s[3] = 0x7fffffffLL;
    s[4] = -1;
    s[5] = 0;
    s[6] = 0;
}

struct RAcc {
    long long n, y0, y1, x0, x1, ys, xs;
    __device__ void clear() { n = 0, y0 = 0x7fffffffLL, y1 = -1, x0 = 0x7fffffffLL, x1 = -1, ys = 0, xs = 0; }
    __device__ void add(int y, int x) {
        ++n;
        y0 = y < y0 ? y : y0, y1 = y > y1 ? y : y1, x0 = x < x0 ? x : x0, x1 = x > x1 ? x : x1;
        ys += y, xs += x;
    }
    __device__ void flush(long long* s) const {
        atomicAdd((unsigned long long*)&s[0], (unsigned long long)n);
        __hip_atomic_fetch_min(&s[1], y0, RLX_AGENT);
        __hip_atomic_fetch_max(&s[2], y1, RLX_AGENT);
        __hip_atomic_fetch_min(&s[3], x0, RLX_AGENT);
        __hip_atomic_fetch_max(&s[4], x1, RLX_AGENT);
        atomicAdd((unsigned long long*)&s[5], (unsigned long long)ys);
        atomicAdd((unsigned long long*)&s[6], (unsigned long long)xs);
    }
};

// rid[image * HW + root] = dense region id (only read at roots); grid.y = image
__global__ __launch_bounds__(RTPB) void region_stats_kernel(const int* __restrict__ labels, const int* __restrict__ rid,
                                                            long long* __restrict__ stats, int W, long HW) {
    const long base = (long)blockIdx.y * HW;
    const int* lab = labels + base;
    const long p0 = (blockIdx.x * (long)RTPB + threadIdx.x) * RUN;
    int y = (int)(p0 / W), x = (int)(p0 - (long)y * W);
    int key = -1;
    RAcc a;
    a.clear();
#pragma unroll
    for (int k = 0; k < RUN; ++k) {
        const int r = p0 + k < HW ? lab[p0 + k] : -1;
        if (r != key) {
            if (key >= 0) a.flush(stats + (long)rid[base + key] * NSTAT);
            key = r;
            a.clear();
        }
        a.add(y, x);
        if (++x == W) x = 0, ++y;
    }
    const Seg s = seg_of(key);
    a.n = seg_reduce<OpAdd>(a.n, s);
    a.y0 = seg_reduce<OpMin>(a.y0, s);
    a.y1 = seg_reduce<OpMax>(a.y1, s);
    a.x0 = seg_reduce<OpMin>(a.x0, s);
    a.x1 = seg_reduce<OpMax>(a.x1, s);
    a.ys = seg_reduce<OpAdd>(a.ys, s);
    a.xs = seg_reduce<OpAdd>(a.xs, s);
    if (s.head && key >= 0) a.flush(stats + (long)rid[base + key] * NSTAT);
}

constexpr int MAX_IMAGES = 65535;  // grid.y

}  // namespace

#define ST(s) ((hipStream_t)(s))
#define IG_REQUIRE_MAP(name)                                                                                              \
    IG_REQUIRE(n >= 0 && H >= 1 && W >= 1, name ": need n >= 0, H >= 1, W >= 1 (n %d, H %d, W %d)", n, H, W);            \
    IG_REQUIRE((long)H * W <= 0x7fffffffL, name ": H * W = %ld exceeds 2^31 - 1 (labels are int32 pixel indices)", (long)H * W)

extern "C" {

int ig_ccl_label(const signed char* cls, int* labels, int n, int H, int W, int connectivity, int fill, int* status, void* stream) {
    IG_REQUIRE(connectivity == 4 || connectivity == 8, "ig_ccl_label: connectivity must be 4 or 8 (got %d)", connectivity);
    IG_REQUIRE(fill >= -128 && fill <= 127, "ig_ccl_label: fill must fit int8 (got %d)", fill);
    IG_REQUIRE_MAP("ig_ccl_label");
    if (n == 0) return IG_OK;
    IG_REQUIRE(cls && labels && status, "ig_ccl_label: null pointer");
    const long HW = (long)H * W;
    const int tiles_x = ig_cdiv(W, CT_W), tiles_y = ig_cdiv(H, CT_H), conn8 = connectivity == 8;
    const unsigned pix_blocks = (unsigned)((HW + CTPB - 1) / CTPB);
    for (int i0 = 0; i0 < n; i0 += MAX_IMAGES) {
        const unsigned ni = (unsigned)(n - i0 < MAX_IMAGES ? n - i0 : MAX_IMAGES);
        const signed char* c = cls + (long)i0 * HW;
        int* l = labels + (long)i0 * HW;
        hipLaunchKernelGGL(ccl_tile_kernel, dim3((unsigned)tiles_x * (unsigned)tiles_y, ni), dim3(CTPB), 0, ST(stream), c, l, H, W, tiles_x,
                           conn8, fill, status);
        if (tiles_x > 1 || tiles_y > 1) {
            hipLaunchKernelGGL(ccl_merge_kernel, dim3(pix_blocks, ni), dim3(CTPB), 0, ST(stream), c, l, H, W, conn8, fill, status);
            hipLaunchKernelGGL(ccl_flatten_kernel, dim3(pix_blocks, ni), dim3(CTPB), 0, ST(stream), l, HW, status);
        }
    }
    return ig_check_launch("ig_ccl_label");
}

int ig_region_area(const int* labels, int* area, int n, long HW, void* stream) {
    IG_REQUIRE(n >= 0 && HW >= 1 && HW <= 0x7fffffffL, "ig_region_area: need n >= 0 and 1 <= HW <= 2^31 - 1 (n %d, HW %ld)", n, HW);
    if (n == 0) return IG_OK;
    IG_REQUIRE(labels && area, "ig_region_area: null pointer");
    if (hipMemsetAsync(area, 0, (size_t)n * HW * sizeof(int), ST(stream)) != hipSuccess) {
        ig_set_error("ig_region_area: hipMemsetAsync failed");
        return IG_ERR_HIP;
    }
    const unsigned blocks = (unsigned)((HW + (long)RTPB * RUN - 1) / ((long)RTPB * RUN));
    for (int i0 = 0; i0 < n; i0 += MAX_IMAGES) {
        const unsigned ni = (unsigned)(n - i0 < MAX_IMAGES ? n - i0 : MAX_IMAGES);
        hipLaunchKernelGGL(region_area_kernel, dim3(blocks, ni), dim3(RTPB), 0, ST(stream), labels + (long)i0 * HW, area + (long)i0 * HW, HW);
    }
    return ig_check_launch("ig_region_area");
}

int ig_sieve_pass(signed char* cls, const int* labels, const int* area, int min_region, int n, int H, int W, int fill,
                  unsigned long long* best, int* changed, void* stream) {
    IG_REQUIRE(min_region >= 0, "ig_sieve_pass: min_region must not be negative (got %d)", min_region);
    IG_REQUIRE(fill >= -128 && fill <= 127, "ig_sieve_pass: fill must fit int8 (got %d)", fill);
    IG_REQUIRE_MAP("ig_sieve_pass");
    if (n == 0) return IG_OK;
    IG_REQUIRE(cls && labels && area && best && changed, "ig_sieve_pass: null pointer");
    const long HW = (long)H * W;
    if (hipMemsetAsync(best, 0, (size_t)n * HW * sizeof(unsigned long long), ST(stream)) != hipSuccess) {
        ig_set_error("ig_sieve_pass: hipMemsetAsync failed");
        return IG_ERR_HIP;
    }
    const unsigned blocks = (unsigned)((HW + RTPB - 1) / RTPB);
    for (int i0 = 0; i0 < n; i0 += MAX_IMAGES) {
        const unsigned ni = (unsigned)(n - i0 < MAX_IMAGES ? n - i0 : MAX_IMAGES);
        const long off = (long)i0 * HW;
        hipLaunchKernelGGL(sieve_select_kernel, dim3(blocks, ni), dim3(RTPB), 0, ST(stream), labels + off, area + off, min_region, H, W,
                           best + off);
        hipLaunchKernelGGL(sieve_apply_kernel, dim3(blocks, ni), dim3(RTPB), 0, ST(stream), cls + off, labels + off, area + off, min_region,
                           HW, best + off, changed);
    }
    return ig_check_launch("ig_sieve_pass");
}

int ig_region_stats(const int* labels, const int* rid, long long* stats, long n_regions, int n, int H, int W, void* stream) {
    IG_REQUIRE(n_regions >= 0 && n_regions <= 0x7fffffffL, "ig_region_stats: need 0 <= n_regions <= 2^31 - 1 (got %ld)", n_regions);
    IG_REQUIRE_MAP("ig_region_stats");
    if (n == 0 || n_regions == 0) return IG_OK;
    IG_REQUIRE(labels && rid && stats, "ig_region_stats: null pointer");
    const long HW = (long)H * W;
    hipLaunchKernelGGL(region_stats_init_kernel, dim3((unsigned)((n_regions + RTPB - 1) / RTPB)), dim3(RTPB), 0, ST(stream), stats, n_regions);
    const unsigned blocks = (unsigned)((HW + (long)RTPB * RUN - 1) / ((long)RTPB * RUN));
    for (int i0 = 0; i0 < n; i0 += MAX_IMAGES) {
        const unsigned ni = (unsigned)(n - i0 < MAX_IMAGES ? n - i0 : MAX_IMAGES);
        hipLaunchKernelGGL(region_stats_kernel, dim3(blocks, ni), dim3(RTPB), 0, ST(stream), labels + (long)i0 * HW, rid + (long)i0 * HW, stats,
                           W, HW);
    }
    return ig_check_launch("ig_region_stats");
}

}  // extern "C"
