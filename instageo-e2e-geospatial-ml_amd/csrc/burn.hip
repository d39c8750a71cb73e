// Polygon labels burned into label rasters for gfx950.  Not in the reference, which expects rasters made with
// gdal_rasterize.  The rule (the zonal block's grid and inside test, the last containing feature wins, untouched pixels keep what the
// raster held) is stated in include/instageo_hip.h.  Everything is integer work or a copy of a caller-supplied value.
//
//   1  burn_resolve_kernel   per canvas row: inclusive prefix XOR of the toggles that ig_zone_toggle left on the pass canvas (zone_scan_chunk
//                            of zone_canvas.h, the scan of zonal.hip, with its geometry: chunks of ZCHUNK columns, ZVPT per thread) =
//                            the inside mask of the pass's 64 features; the highest set bit is the last feature in file order; its value
//                            comes from a 64-entry table in LDS and goes to the raster at (r0 + r, c0 + c).  Pixels with an empty mask
//                            are not written.  The pixels written are counted per thread, wave and workgroup: one atomic per workgroup.
//   2  label_cells_kernel    per S x S cell of the finished raster: the valid pixels and, for int8, the class histogram; lanes of a wave
//                            with the same value add once to an LDS table, the table reaches memory as one atomic per non-empty cell.
//
// The byte store.  A thread owns four consecutive pixels of a row.  int8 pixels go out as single bytes; only when all four are written
// and their address is 4-byte aligned do they go out as one word, which no other thread touches.  No lane ever read-modify-writes a word
// it shares, so any pitch and any c0 are safe.
// Out-of-range writes are impossible: the entry point checks that the pass rectangle lies inside the raster, and the kernel writes only
// columns c < Wp of rows r < Hp of that rectangle.
#include "zone_canvas.h"

namespace {

constexpr int CELL_ROWS = 64, MAX_SIDE = 1 << 15, MAX_K = 128;

// The workgroup's sum of `mine`, in thread 0 (the others get 0): wave sums, wcount[ZWAVES], one barrier.  Every thread calls it.
__device__ __forceinline__ unsigned long long block_total(unsigned mine, unsigned* wcount) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if ((threadIdx.x & 63) == 0) wcount[threadIdx.x >> 6] = mine;
    __syncthreads();
    unsigned long long total = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < ZWAVES; ++w) total += wcount[w];
    return total;
}

// T = signed char (int8 rasters) or unsigned (the bits of float32 rasters)
template <typename T>
__global__ __launch_bounds__(ZTPB) void burn_resolve_kernel(const unsigned long long* __restrict__ canvas, const T* __restrict__ table,
                                                            T* __restrict__ out, unsigned long long* __restrict__ written, int Hp, int Wp,
                                                            long pitch, int r0, int c0) {
    __shared__ T tab[ZBITS];
    __shared__ unsigned long long wtot[2][ZWAVES];  // the wave totals of two consecutive chunks (one barrier per chunk)
    __shared__ unsigned wcount[ZWAVES];
    if (threadIdx.x < ZBITS) tab[threadIdx.x] = table[threadIdx.x];
    __syncthreads();
    unsigned mine = 0;  // pixels this thread stored: at most Hp * Wp <= 2^31 - 1
    int par = 0;
    for (int r = blockIdx.x; r < Hp; r += gridDim.x) {
        const unsigned long long* row = canvas + (long)r * Wp;
        T* orow = out + ((long)r0 + r) * pitch + c0;
        unsigned long long carry = 0;  // the prefix XOR of the row's earlier chunks: the same in every thread
        for (long cc = 0; cc < Wp; cc += ZCHUNK, par ^= 1) {
            const long c = cc + (long)threadIdx.x * ZVPT;
            unsigned long long v[ZVPT];
            zone_load_toggles(v, row, c, Wp);
            zone_scan_chunk(v, carry, wtot[par]);  // every thread of the workgroup, whatever its columns
            T val[ZVPT];
            bool hit[ZVPT];
            int hits = 0;
#pragma unroll
            for (int j = 0; j < ZVPT; ++j) {
                const unsigned long long m = c + j < Wp ? v[j] : 0ull;  // a dead column's mask is dropped
                hit[j] = m != 0;
                val[j] = tab[hit[j] ? 63 - __clzll((long long)m) : 0];
                hits += hit[j];
            }
            mine += (unsigned)hits;
            bool packed = false;
            if constexpr (sizeof(T) == 1) {
                if (hits == ZVPT && ((uintptr_t)(orow + c) & 3) == 0) {
                    // all four pixels of this thread, word aligned: the word is private to the thread
                    const unsigned word = (unsigned)(unsigned char)val[0] | (unsigned)(unsigned char)val[1] << 8 |
                                          (unsigned)(unsigned char)val[2] << 16 | (unsigned)(unsigned char)val[3] << 24;
                    *reinterpret_cast<unsigned*>(orow + c) = word;
                    packed = true;
                }
            }
            if (!packed) {
#pragma unroll
                for (int j = 0; j < ZVPT; ++j)
                    if (hit[j]) orow[c + j] = val[j];
            }
        }
    }
    if (!written) return;  // uniform over the grid
    const unsigned long long total = block_total(mine, wcount);
    if (total) atomicAdd(written, total);
}

// grid (cells, ceil(S / CELL_ROWS)).  LDS: tab[max(K, 1)] u32 (dynamic; a cell counts at most CELL_ROWS * S <= 2^21 pixels).
template <bool F32>
__global__ __launch_bounds__(ZTPB) void label_cells_kernel(const void* __restrict__ raster, unsigned long long* __restrict__ valid,
                                                           unsigned long long* __restrict__ hist, int nx, int S, int ignore, int K,
                                                           FDiv by_s) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned* tab = reinterpret_cast<unsigned*>(smem);
    __shared__ unsigned wcount[ZWAVES];
    const int lane = threadIdx.x & 63;
    for (int i = threadIdx.x; i < K; i += ZTPB) tab[i] = 0u;
    __syncthreads();
    const long cell = blockIdx.x;
    const long cy = cell / nx, cx = cell - cy * nx;
    const int row0 = blockIdx.y * CELL_ROWS;
    const int rows = S - row0 < CELL_ROWS ? S - row0 : CELL_ROWS;
    const long W = (long)nx * S;
    const long base = (cy * S + row0) * W + cx * S;
    const int n = rows * S;  // <= 2^21
    unsigned mine = 0;
    for (int first = 0; first < n; first += ZTPB) {  // uniform trip count: every lane takes part in the ballots below
        const int idx = first + (int)threadIdx.x;
        int k = -1;  // the histogram cell, or none
        if (idx < n) {
            const int r = by_s.div(idx), c = idx - r * S;
            const long at = base + (long)r * W + c;
            if (F32) {
                const float f = reinterpret_cast<const float*>(raster)[at];
                mine += f == f;
            } else {
                const int s = reinterpret_cast<const signed char*>(raster)[at];
                mine += s != ignore;
                if (s != ignore && s >= 0 && s < K) k = s;
            }
        }
        if (F32) continue;
        unsigned long long todo = __ballot(k >= 0);
        while (todo) {  // lanes with the same value add once, at the first of them
            const int lead = __ffsll((long long)todo) - 1;
            const int kk = __shfl(k, lead, 64);
            const unsigned long long same = __ballot(k == kk);
            if (lane == lead) atomicAdd(tab + kk, (unsigned)__popcll(same));
            todo &= ~same;
        }
    }
    const unsigned long long total = block_total(mine, wcount);  // its barrier also ends the adds to tab
    if (total) atomicAdd(valid + cell, total);
    for (int i = threadIdx.x; i < K; i += ZTPB)
        if (tab[i]) atomicAdd(hist + cell * K + i, (unsigned long long)tab[i]);
}

}  // namespace

#define ST(s) ((hipStream_t)(s))

extern "C" {

int ig_burn_resolve(const unsigned long long* canvas, int Hp, int Wp, const void* table, int elem_size, void* out, int H, int W, long pitch,
                    int r0, int c0, unsigned long long* written, void* stream) {
    IG_REQUIRE(elem_size == 1 || elem_size == 4, "ig_burn_resolve: elem_size must be 1 (int8) or 4 (float32) (got %d)", elem_size);
    IG_REQUIRE(Hp >= 0 && Wp >= 0, "ig_burn_resolve: need Hp >= 0 and Wp >= 0 (Hp %d, Wp %d)", Hp, Wp);
    IG_REQUIRE((long)Hp * Wp <= 0x7fffffffL, "ig_burn_resolve: Hp * Wp = %ld exceeds 2^31 - 1", (long)Hp * Wp);
    IG_REQUIRE(H >= 0 && W >= 0 && pitch >= W, "ig_burn_resolve: need H >= 0, W >= 0 and pitch >= W (H %d, W %d, pitch %ld)", H, W, pitch);
    IG_REQUIRE(pitch <= 0x7fffffffL && (long)H * pitch < (1L << 40), "ig_burn_resolve: H * pitch = %ld must stay below 2^40", (long)H * pitch);
    IG_REQUIRE(r0 >= 0 && c0 >= 0 && (long)r0 + Hp <= H && (long)c0 + Wp <= W,
               "ig_burn_resolve: the pass rectangle (r0 %d, c0 %d, Hp %d, Wp %d) must lie inside the raster (H %d, W %d)", r0, c0, Hp, Wp, H, W);
    if ((long)Hp * Wp == 0) return IG_OK;
    IG_REQUIRE(canvas && table && out, "ig_burn_resolve: null pointer");
    IG_REQUIRE(((uintptr_t)canvas & 7) == 0 && ((uintptr_t)written & 7) == 0, "ig_burn_resolve: canvas and written must be 8-byte aligned");
    IG_REQUIRE(elem_size == 1 || (((uintptr_t)table & 3) == 0 && ((uintptr_t)out & 3) == 0),
               "ig_burn_resolve: a float32 table and raster must be 4-byte aligned");
    const dim3 grid((unsigned)(Hp < MAX_WG ? Hp : MAX_WG));
    if (elem_size == 1)
        return ig_launch<burn_resolve_kernel<signed char>>("ig_burn_resolve", grid, dim3(ZTPB), 0, ST(stream), canvas, (const signed char*)table,
                                                          (signed char*)out, written, Hp, Wp, pitch, r0, c0);
    return ig_launch<burn_resolve_kernel<unsigned>>("ig_burn_resolve", grid, dim3(ZTPB), 0, ST(stream), canvas, (const unsigned*)table,
                                                   (unsigned*)out, written, Hp, Wp, pitch, r0, c0);
}

int ig_label_cells(const void* raster, int ny, int nx, int S, int elem_size, int ignore, int K, unsigned long long* valid,
                   unsigned long long* hist, void* stream) {
    IG_REQUIRE(elem_size == 1 || elem_size == 4, "ig_label_cells: elem_size must be 1 (int8) or 4 (float32) (got %d)", elem_size);
    IG_REQUIRE(ny >= 0 && nx >= 0 && (long)ny * nx <= 0x7fffffffL, "ig_label_cells: need ny >= 0, nx >= 0 and ny * nx <= 2^31 - 1 (ny %d, nx %d)",
               ny, nx);
    IG_REQUIRE(S >= 1 && S <= MAX_SIDE, "ig_label_cells: cell side in [1, 2^15] (got %d)", S);
    IG_REQUIRE((long)ny * S * ((long)nx * S) < (1L << 40), "ig_label_cells: a raster of %ld x %ld pixels is beyond 2^40", (long)ny * S,
               (long)nx * S);
    IG_REQUIRE(K >= 0 && K <= MAX_K, "ig_label_cells: a class histogram has 0 <= K <= %d cells (got %d)", MAX_K, K);
    IG_REQUIRE(K == 0 || elem_size == 1, "ig_label_cells: a class histogram (K = %d) needs an int8 raster", K);
    IG_REQUIRE(ignore >= -128 && ignore <= 127, "ig_label_cells: ignore must fit int8 (got %d)", ignore);
    if ((long)ny * nx == 0) return IG_OK;
    IG_REQUIRE(raster && valid && (K == 0 || hist), "ig_label_cells: null pointer");
    IG_REQUIRE(((uintptr_t)valid & 7) == 0 && ((uintptr_t)hist & 7) == 0, "ig_label_cells: valid and hist must be 8-byte aligned");
    IG_REQUIRE(elem_size == 1 || ((uintptr_t)raster & 3) == 0, "ig_label_cells: a float32 raster must be 4-byte aligned");
    const dim3 grid((unsigned)((long)ny * nx), (unsigned)((S + CELL_ROWS - 1) / CELL_ROWS));
    const int smem = (K > 0 ? K : 1) * 4;
    if (elem_size == 4)
        return ig_launch<label_cells_kernel<true>>("ig_label_cells", grid, dim3(ZTPB), smem, ST(stream), raster, valid, hist, nx, S, ignore, K,
                                                   make_fdiv(S));
    return ig_launch<label_cells_kernel<false>>("ig_label_cells", grid, dim3(ZTPB), smem, ST(stream), raster, valid, hist, nx, S, ignore, K,
                                                make_fdiv(S));
}

}  // extern "C"
