// Vectorisation of labelled class maps into polygon rings for gfx950: live boundary edges, local linking, ring roots and
// vertex ranks by pointer jumping, ring sums and the vertex scatter.  The rule (sides, live edges, successor, rings) is stated in
// include/instageo_hip.h.  Everything is integer arithmetic and every result is unique (independent of scheduling).
//
//   1  edge_mask_kernel   per pixel: which of its four sides face another label (4 bits) and how many (3 bits), + the total
//   2  edge_link_kernel   per live edge e (compact id from the caller's scan): succ[e], tail vertex, and the flag byte of the SUCCESSOR
//   3  ring_jump_kernel   one round of pointer jumping, out of place: <0> min-propagation (ring root), <1> ranking of the turn edges
//   4  ring_sums_kernel   per ring: vertices and twice the signed area, integer atomics after a segmented wave reduction
//   5  ring_emit_kernel   every turn edge stores its tail at first[ring] + position
//
// Memory traffic.  The mask kernel reads each label once from HBM: a thread takes VRUN consecutive pixels, lanes take consecutive runs, so
// a wave reads 1 KiB of a row contiguously and the rows above and below are re-reads that L2 serves (plain coalesced reads; a halo tile in
// LDS would save no HBM byte here).  The jump rounds gather through a pointer: rings of a few edges stay inside a cache line, long rings
// scatter, and nothing can be done about that short of renumbering.
// Every launch does a fixed amount of work: no loop depends on data, no workgroup waits for another, the caller decides on the rounds.
// Out-of-range writes are impossible for consistent inputs and are guarded (status) for inconsistent ones.
#include "common.h"
#include "segreduce.h"

namespace {

constexpr int VTPB = 256, VRUN = 4;  // mask kernel: VRUN consecutive pixels per thread, one 32-bit store of their four mask bytes
enum { ST_DEAD_SUCC = 1, ST_EDGE_RANGE = 2, ST_VERTEX_RANGE = 4 };

__device__ __forceinline__ int label_at(const int* __restrict__ lab, int r, int c, int H, int W) {
    return (r >= 0 && r < H && c >= 0 && c < W) ? lab[(long)r * W + c] : -1;
}

// NP = n * H * W pixels of all images, numbered image * HW + pixel
__global__ __launch_bounds__(VTPB) void edge_mask_kernel(const int* __restrict__ labels, unsigned char* __restrict__ mask,
                                                         unsigned long long* __restrict__ total, long NP, int H, int W) {
    const long HW = (long)H * W;
    const long g0 = (blockIdx.x * (long)VTPB + threadIdx.x) * VRUN;
    int cnt = 0;
    if (g0 < NP) {
        const long img = g0 / HW, p0 = g0 - img * HW;
        int r = (int)(p0 / W), c = (int)(p0 - (long)r * W);
        const int* lab = labels + img * HW;
        unsigned packed = 0;
#pragma unroll
        for (int k = 0; k < VRUN; ++k) {
            if (g0 + k >= NP) break;
            const int me = lab[(long)r * W + c];
            unsigned m = 0;
            if (me >= 0) {  // the pixel across side s is p + d[(s + 3) % 4]: N, E, S, W
                m = (unsigned)(label_at(lab, r - 1, c, H, W) != me) | (unsigned)(label_at(lab, r, c + 1, H, W) != me) << 1 |
                    (unsigned)(label_at(lab, r + 1, c, H, W) != me) << 2 | (unsigned)(label_at(lab, r, c - 1, H, W) != me) << 3;
                m |= (unsigned)__popc(m) << 4;
            }
            packed |= m << (8 * k);
            cnt += (int)(m >> 4);
            if (++c == W) {
                c = 0;
                if (++r == H) r = 0, lab += HW;
            }
        }
        if (g0 + VRUN <= NP) {
            *reinterpret_cast<unsigned*>(mask + g0) = packed;  // g0 is a multiple of 4 and the entry point checks the base
        } else {
            for (int k = 0; g0 + k < NP; ++k) mask[g0 + k] = (unsigned char)(packed >> (8 * k));
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(total, (unsigned long long)cnt);  // one atomic per wave
}

// one thread per pixel; a pixel writes succ / tail of its own live edges and the flag byte of their successors
__global__ __launch_bounds__(VTPB) void edge_link_kernel(const int* __restrict__ labels, const unsigned char* __restrict__ mask,
                                                         const int* __restrict__ off, int* __restrict__ succ, int2* __restrict__ tail,
                                                         unsigned char* __restrict__ flag, long NP, int H, int W, long E,
                                                         int* __restrict__ status) {
    const long g = blockIdx.x * (long)VTPB + threadIdx.x;
    if (g >= NP) return;
    const unsigned m = mask[g] & 15u;
    if (!m) return;
    const long HW = (long)H * W;
    const long img = g / HW, p = g - img * HW;
    const int r = (int)(p / W), c = (int)(p - (long)r * W);
    const int* lab = labels + img * HW;
    const unsigned char* mk = mask + img * HW;
    const int* of = off + img * HW;
    const int me = lab[p];
    long e = of[p];
    constexpr int DR[4] = {0, 1, 0, -1}, DC[4] = {1, 0, -1, 0};  // E, S, W, N
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        if (!(m >> s & 1u)) continue;
        const int l = (s + 3) & 3;
        const int ar = r + DR[s], ac = c + DC[s], br = ar + DR[l], bc = ac + DC[l];
        int qr = r, qc = c, t = (s + 1) & 3;  // right turn, unless ...
        if (label_at(lab, br, bc, H, W) == me) qr = br, qc = bc, t = l;       // ... left turn
        else if (label_at(lab, ar, ac, H, W) == me) qr = ar, qc = ac, t = s;  // ... straight
        const long q = (long)qr * W + qc;
        const unsigned mq = mk[q];
        const long f = (long)of[q] + __popc(mq & ((1u << t) - 1u));
        if (!(mq >> t & 1u)) {
            atomicOr(status, ST_DEAD_SUCC);
        } else if ((unsigned long)e >= (unsigned long)E || (unsigned long)f >= (unsigned long)E) {
            atomicOr(status, ST_EDGE_RANGE);
        } else {
            succ[e] = (int)f;
            tail[e] = make_int2(c + (s == 1 || s == 2), r + (s >= 2));
            flag[f] = (unsigned char)(t | (t != s) << 2);
        }
        ++e;
    }
}

// PHASE 0: val = the smallest id seen along the ring so far; PHASE 1: val = turn edges from e up to (not including) ptr, ptr = -1 past the
// root.  FIRST: the round that reads succ (and, in phase 1, root and flag) in place of a buffer pair.
template <int PHASE, bool FIRST>
__global__ __launch_bounds__(VTPB) void ring_jump_kernel(const int* __restrict__ val_in, const int* __restrict__ ptr_in, int* __restrict__ val_out,
                                                         int* __restrict__ ptr_out, const int* __restrict__ root,
                                                         const unsigned char* __restrict__ flag, long E, int* __restrict__ changed) {
    const long e = blockIdx.x * (long)VTPB + threadIdx.x;
    bool more = false;
    if (e < E) {
        if constexpr (PHASE == 0) {
            const int j = ptr_in[e];
            const int v = FIRST ? (int)e : val_in[e], vj = FIRST ? j : val_in[j];
            val_out[e] = vj < v ? vj : v;
            ptr_out[e] = ptr_in[j];
            more = vj < v;
        } else {
            auto val = [&](long i) { return FIRST ? (int)(flag[i] >> 2 & 1) : val_in[i]; };
            auto ptr = [&](long i) {
                const int j = ptr_in[i];
                return FIRST && j == root[i] ? -1 : j;
            };
            int v = val(e), j = ptr(e);
            if (j >= 0) {
                v += val(j);
                j = ptr(j);
            }
            val_out[e] = v;
            ptr_out[e] = j;
            more = j >= 0;
        }
    }
    if (__ballot(more) && (threadIdx.x & 63) == 0) atomicOr(changed, 1);  // one atomic per wave
}

// twice the signed area: an edge (x, y) -> (x + dx, y + dy) adds x (y + dy) - (x + dx) y = -y, x, y, -x for E, S, W, N
__global__ __launch_bounds__(VTPB) void ring_sums_kernel(const int* __restrict__ root, const int* __restrict__ ring_id,
                                                         const int2* __restrict__ tail, const unsigned char* __restrict__ flag,
                                                         long long* __restrict__ sums, long E, long n_rings) {
    const long e = blockIdx.x * (long)VTPB + threadIdx.x;
    int key = -1;
    long long a = 0, v = 0;
    if (e < E) {
        const int id = ring_id[root[e]];
        if (id >= 0 && id < n_rings) {
            key = id;
            const unsigned fl = flag[e];
            const int2 t = tail[e];
            const int h = (int)(fl & 3u);
            a = h == 0 ? -(long long)t.y : h == 1 ? (long long)t.x : h == 2 ? (long long)t.y : -(long long)t.x;
            v = fl >> 2 & 1u;
        }
    }
    const Seg s = seg_of(key);  // edges of a pixel, and of neighbouring pixels, mostly share a ring: one atomic per run
    a = seg_reduce<OpAdd>(a, s);
    v = seg_reduce<OpAdd>(v, s);
    if (s.head && key >= 0) {
        atomicAdd((unsigned long long*)&sums[2 * (long)key], (unsigned long long)v);
        atomicAdd((unsigned long long*)&sums[2 * (long)key + 1], (unsigned long long)a);
    }
}

__global__ __launch_bounds__(VTPB) void ring_emit_kernel(const int* __restrict__ root, const int* __restrict__ ring_id,
                                                         const int* __restrict__ rank, const int2* __restrict__ tail,
                                                         const unsigned char* __restrict__ flag, const long long* __restrict__ first,
                                                         int2* __restrict__ vertices, long E, long n_rings, long n_vertices,
                                                         int* __restrict__ status) {
    const long e = blockIdx.x * (long)VTPB + threadIdx.x;
    if (e >= E || !(flag[e] & 4u)) return;
    const int r = root[e];
    const int id = ring_id[r];
    if (id < 0 || id >= n_rings) {
        atomicOr(status, ST_VERTEX_RANGE);
        return;
    }
    const long long dst = first[id] + (rank[r] - rank[e]);
    if ((unsigned long long)dst >= (unsigned long long)n_vertices) {
        atomicOr(status, ST_VERTEX_RANGE);
        return;
    }
    vertices[dst] = tail[e];
}

}  // namespace

#define ST(s) ((hipStream_t)(s))
#define IG_REQUIRE_EDGES(name) \
    IG_REQUIRE(E >= 0 && E <= 0x7fffffffL, name ": need 0 <= E <= 2^31 - 1 (compact edge ids are int32; got %ld)", E)
#define IG_REQUIRE_LABELS(name)                                                                                          \
    IG_REQUIRE(n >= 0 && H >= 1 && W >= 1, name ": need n >= 0, H >= 1, W >= 1 (n %d, H %d, W %d)", n, H, W);            \
    IG_REQUIRE((long)H * W <= 0x7fffffffL, name ": H * W = %ld exceeds 2^31 - 1 (labels are int32 pixel indices)", (long)H * W); \
    IG_REQUIRE((long)n * H * W <= (1L << 38), name ": n * H * W = %ld exceeds 2^38 pixels per call", (long)n * H * W)

static inline dim3 blocks_for(long items) { return dim3((unsigned)((items + VTPB - 1) / VTPB)); }

extern "C" {

int ig_edge_mask(const int* labels, unsigned char* mask, unsigned long long* total, int n, int H, int W, void* stream) {
    IG_REQUIRE_LABELS("ig_edge_mask");
    if (n == 0) return IG_OK;
    IG_REQUIRE(labels && mask && total, "ig_edge_mask: null pointer");
    IG_REQUIRE(((uintptr_t)mask & 3) == 0, "ig_edge_mask: mask must be 4-byte aligned");
    const long NP = (long)n * H * W;
    return ig_launch<edge_mask_kernel>("ig_edge_mask", blocks_for((NP + VRUN - 1) / VRUN), dim3(VTPB), 0, ST(stream), labels, mask, total,
                                       NP, H, W);
}

int ig_edge_link(const int* labels, const unsigned char* mask, const int* off, int* succ, int* tail, unsigned char* flag, int n, int H,
                 int W, long E, int* status, void* stream) {
    IG_REQUIRE_LABELS("ig_edge_link");
    IG_REQUIRE_EDGES("ig_edge_link");
    if (n == 0 || E == 0) return IG_OK;
    IG_REQUIRE(labels && mask && off && succ && tail && flag && status, "ig_edge_link: null pointer");
    IG_REQUIRE(((uintptr_t)tail & 7) == 0, "ig_edge_link: tail must be 8-byte aligned");
    const long NP = (long)n * H * W;
    return ig_launch<edge_link_kernel>("ig_edge_link", blocks_for(NP), dim3(VTPB), 0, ST(stream), labels, mask, off, succ, (int2*)tail, flag,
                                       NP, H, W, E, status);
}

int ig_ring_jump(int phase, const int* val_in, const int* ptr_in, int* val_out, int* ptr_out, const int* root, const unsigned char* flag,
                 long E, int* changed, void* stream) {
    IG_REQUIRE(phase == 0 || phase == 1, "ig_ring_jump: phase must be 0 (root) or 1 (rank) (got %d)", phase);
    IG_REQUIRE_EDGES("ig_ring_jump");
    if (E == 0) return IG_OK;
    IG_REQUIRE(ptr_in && val_out && ptr_out && changed, "ig_ring_jump: null pointer");
    IG_REQUIRE(val_in != val_out && ptr_in != ptr_out && val_in != ptr_out && ptr_in != val_out,
               "ig_ring_jump: a round must not write the buffers it reads (in-place jumping races)");
    const bool first = val_in == nullptr;
    IG_REQUIRE(!(phase == 1 && first) || (root && flag), "ig_ring_jump: the first ranking round needs root and flag");
    const dim3 grid = blocks_for(E), block(VTPB);
#define JUMP(P, F) \
    ig_launch<ring_jump_kernel<P, F>>("ig_ring_jump", grid, block, 0, ST(stream), val_in, ptr_in, val_out, ptr_out, root, flag, E, changed)
    if (phase == 0) return first ? JUMP(0, true) : JUMP(0, false);
    return first ? JUMP(1, true) : JUMP(1, false);
#undef JUMP
}

int ig_ring_sums(const int* root, const int* ring_id, const int* tail, const unsigned char* flag, long long* sums, long E, long n_rings,
                 void* stream) {
    IG_REQUIRE_EDGES("ig_ring_sums");
    IG_REQUIRE(n_rings >= 0 && n_rings <= E, "ig_ring_sums: need 0 <= n_rings <= E (n_rings %ld, E %ld)", n_rings, E);
    if (E == 0) return IG_OK;
    IG_REQUIRE(root && ring_id && tail && flag && sums, "ig_ring_sums: null pointer");
    IG_REQUIRE(((uintptr_t)tail & 7) == 0, "ig_ring_sums: tail must be 8-byte aligned");
    return ig_launch<ring_sums_kernel>("ig_ring_sums", blocks_for(E), dim3(VTPB), 0, ST(stream), root, ring_id, (const int2*)tail, flag, sums,
                                       E, n_rings);
}

int ig_ring_emit(const int* root, const int* ring_id, const int* rank, const int* tail, const unsigned char* flag, const long long* first,
                 int* vertices, long E, long n_rings, long n_vertices, int* status, void* stream) {
    IG_REQUIRE_EDGES("ig_ring_emit");
    IG_REQUIRE(n_rings >= 0 && n_rings <= E, "ig_ring_emit: need 0 <= n_rings <= E (n_rings %ld, E %ld)", n_rings, E);
    IG_REQUIRE(n_vertices >= 0 && n_vertices <= E, "ig_ring_emit: need 0 <= n_vertices <= E (n_vertices %ld, E %ld)", n_vertices, E);
    if (E == 0) return IG_OK;
    IG_REQUIRE(root && ring_id && rank && tail && flag && first && vertices && status, "ig_ring_emit: null pointer");
    IG_REQUIRE(((uintptr_t)tail & 7) == 0 && ((uintptr_t)vertices & 7) == 0, "ig_ring_emit: tail and vertices must be 8-byte aligned");
    return ig_launch<ring_emit_kernel>("ig_ring_emit", blocks_for(E), dim3(VTPB), 0, ST(stream), root, ring_id, rank, (const int2*)tail, flag,
                                       first, (int2*)vertices, E, n_rings, n_vertices, status);
}

}  // extern "C"
