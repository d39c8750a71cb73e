// Multi-temporal (Quegan and Yu) speckle filtering of Sentinel-1 RTC planes for gfx950.  N float32 planes packed as
// ig_s1_speckle takes them, each placed at an integer offset on the lattice of its group (one band on one pixel lattice) and carrying a
// date, are filtered in one launch by the rule stated in include/instageo_hip.h: per plane the local mean m of ig_s1_speckle's window
// (first moment and count of the PRESENT values, float64, fixed order), per lattice pixel the sum R of x / m over the dates that have a
// present value there and their number c, and per plane y = m (R / c).  Every output depends on its pixel's windows and the member order
// alone, so the bits are the same for any launch geometry; the counts are integer atomics, per workgroup and touched plane.
//
//   s1_temporal_kernel   one workgroup of 256 threads per tile of 64 columns x 32 rows of one GROUP's lattice; the workgroup finds its
//                        group by a binary search in the caller's prefix table of tiles (tile_ptr, G + 1 entries).  A thread owns one
//                        column of the tile and the 8 rows wave, wave + 4, ...  Sweep 1 walks the group's members in order; a member
//                        whose extent misses the tile is passed over.  Its part of the tile and a halo of h pixels go to LDS as float32
//                        (absent values and what lies outside the PLANE as NaN, bounds tests at the load, no padding read), then the row
//                        moments (A float64, K int32) of the staged rows, then each thread sums the 2h + 1 row moments of its pixels
//                        top to bottom: exactly the three phases of s1_speckle_kernel without the second moment.  R, c and the last
//                        date taken stay in registers (4 dwords x 8 pixels).  Sweep 2 stages every member again (its values were read
//                        a moment ago by this workgroup: a cache hit), forms m again and stores y: a wave writes 64 consecutive float32
//                        of a row, 4 bytes per lane, which any W and any 4-byte-aligned start allow.  LDS at h = 7: 14 352 + 35 328
//                        bytes, three workgroups per CU.
//
// Out-of-range accesses are impossible: a workgroup whose lattice has H < 1, W < 1 or H * W > 2^31 - 1, whose tile number is not below the
// lattice's own number of tiles or whose member range breaks 0 <= begin <= end <= M returns at once; a member entry outside [0, N) and a
// plane with H < 1, W < 1, H * W > 2^31 - 1, a negative start, an end beyond `total`, a negative offset or date, or an extent that leaves
// the lattice is skipped in both sweeps (all of these tests are uniform over the workgroup, so the barriers stay matched); every load and
// store is guarded by row < H and column < W of that plane.  The caller guarantees that `planes` and `out` hold `total` elements.
#include "common.h"
#include "pixel_seg.h"

namespace {

constexpr int TW = 64, TH = 32, TTPB = 256, TMAX_H = 7, TPX = TH / 4;  // tile width and height, threads, the largest half window, pixels per thread
constexpr long TLIM40 = 1L << 40;
constexpr unsigned TQNAN = 0x7fc00000u;

struct TemporalArgs {
    int N, G, M, has_nodata, to_db;
    float src_nodata;
    long total;
};

struct Member {  // a plane as one tile sees it
    const float* src;
    long long start;
    int H, W, pr, pc, date;  // pr, pc: the plane's row and column of the tile's first pixel (may be negative)
};

// member entry i of the tables checked -> whether the tile has anything to do with it
__device__ __forceinline__ bool load_member(const long long* __restrict__ starts, const int* __restrict__ sizes, const int* __restrict__ place,
                                            const int* __restrict__ members, const float* __restrict__ planes, const TemporalArgs& a, int i, int Hg,
                                            int Wg, int r0, int c0, Member& m, int& p) {
    p = members[i];
    if (p < 0 || p >= a.N) return false;
    m.H = sizes[2 * p];
    m.W = sizes[2 * p + 1];
    m.start = starts[p];
    const int row0 = place[3 * p], col0 = place[3 * p + 1];
    m.date = place[3 * p + 2];
    if (m.H < 1 || m.W < 1 || (long)m.H * m.W > 0x7fffffffL || m.start < 0 || m.start + (long)m.H * m.W > a.total) return false;
    if (row0 < 0 || col0 < 0 || (long)row0 + m.H > Hg || (long)col0 + m.W > Wg || m.date < 0) return false;
    m.pr = r0 - row0;
    m.pc = c0 - col0;
    m.src = planes + m.start;
    return m.pr < m.H && m.pr + TH > 0 && m.pc < m.W && m.pc + TW > 0;  // the tile and the plane share a pixel
}

// phases 1 and 2 of s1_speckle_kernel for one member: the tile and its halo to LDS (absent values NaN), then the row moments A and K
template <int HALF>
__device__ __forceinline__ void stage_member(const Member& m, const TemporalArgs& a, float* tile, double* mA, int* mK, int lane, int wave) {
    constexpr int h = HALF, w = 2 * h + 1, SH = TH + 2 * h, SP = TW + 2 * h;
    const float nanf_ = __uint_as_float(TQNAN);
    __syncthreads();  // the previous member's sums have been read
    for (int r = wave; r < SH; r += 4) {
        const int gr = m.pr - h + r;
        const bool row_in = gr >= 0 && gr < m.H;
#pragma unroll
        for (int c = lane; c < SP; c += 64) {
            const int gc = m.pc - h + c;
            float f = nanf_;
            if (row_in && gc >= 0 && gc < m.W) {
                f = m.src[(long)gr * m.W + gc];
                if (!(fabsf(f) <= 3.402823466e+38f) || (a.has_nodata && f == a.src_nodata)) f = nanf_;
            }
            tile[r * SP + c] = f;
        }
    }
    __syncthreads();
    {
#pragma clang fp contract(off)
        for (int r = wave; r < SH; r += 8) {  // rows r and r + 4 together: two independent float64 chains
            const int r1 = min(r + 4, SH - 1);  // read inside the tile; stored only when it is a row of its own
            const float* row0 = tile + r * SP + lane;
            const float* row1 = tile + r1 * SP + lane;
            double A0 = 0.0, A1 = 0.0;
            int K0 = 0, K1 = 0;
#pragma unroll
            for (int j = 0; j < w; ++j) {
                const float f0 = row0[j], f1 = row1[j];
                const bool p0 = f0 == f0, p1 = f1 == f1;
                A0 = A0 + (p0 ? (double)f0 : 0.0);  // an absent value adds +0.0: a sum that began at +0.0 keeps its bits
                A1 = A1 + (p1 ? (double)f1 : 0.0);
                K0 += p0 ? 1 : 0;
                K1 += p1 ? 1 : 0;
            }
            mA[r * TW + lane] = A0;
            mK[r * TW + lane] = K0;
            if (r + 4 < SH) {
                mA[(r + 4) * TW + lane] = A1;
                mK[(r + 4) * TW + lane] = K1;
            }
        }
    }
    __syncthreads();
}

// phase 3 for the thread's pixel u (tile row wave + 4 u): the window's A and n down the column, and the centre
template <int HALF>
__device__ __forceinline__ float window_sum(const float* tile, const double* mA, const int* mK, int lane, int i, double& A, int& n) {
#pragma clang fp contract(off)
    constexpr int h = HALF, w = 2 * h + 1, SP = TW + 2 * h;
    A = 0.0;
    n = 0;
#pragma unroll
    for (int j = 0; j < w; ++j) {
        A = A + mA[(i + j) * TW + lane];
        n += mK[(i + j) * TW + lane];
    }
    return tile[(i + h) * SP + lane + h];
}

template <int HALF>
__global__ __launch_bounds__(TTPB, 3) void s1_temporal_kernel(const float* __restrict__ planes, const long long* __restrict__ starts,
                                                           const int* __restrict__ sizes, const int* __restrict__ place,
                                                           const int* __restrict__ lattice, const int* __restrict__ member_ptr,
                                                           const int* __restrict__ members, const long long* __restrict__ tile_ptr,
                                                           TemporalArgs a, unsigned* __restrict__ out, int* __restrict__ counts) {
    extern __shared__ double lds[];
    __shared__ int part[8];
    constexpr int h = HALF, SH = TH + 2 * h, SP = TW + 2 * h;
    double* const mA = lds;                                      // [SH][TW]
    int* const mK = reinterpret_cast<int*>(mA + SH * TW);        // [SH][TW]
    float* const tile = reinterpret_cast<float*>(mK + SH * TW);  // [SH][SP]

    // the group: the last g with tile_ptr[g] <= blockIdx.x
    const long long b = blockIdx.x;
    int lo = 0, hi = a.G;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tile_ptr[mid] <= b) lo = mid;
        else hi = mid;
    }
    const int g = lo;
    const int Hg = lattice[2 * g], Wg = lattice[2 * g + 1];
    if (Hg < 1 || Wg < 1 || (long)Hg * Wg > 0x7fffffffL) return;  // the second fence
    const int nbx = (Wg + TW - 1) / TW, nby = (Hg + TH - 1) / TH;
    const long long k = b - tile_ptr[g];
    if (k < 0 || k >= (long long)nbx * nby) return;
    const int mb = member_ptr[g], me = member_ptr[g + 1];
    if (mb < 0 || me < mb || me > a.M) return;
    const int r0 = (int)(k / nbx) * TH, c0 = (int)(k % nbx) * TW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

    // sweep 1: the ratio sum R and the number c of contributing dates of the thread's 8 pixels, in member order
    double R[TPX];
    int c[TPX], last[TPX];
#pragma unroll
    for (int u = 0; u < TPX; ++u) {
        R[u] = 0.0;
        c[u] = 0;
        last[u] = -1;
    }
    int touched = 0;
    for (int i = mb; i < me; ++i) {
        Member m;
        int p;
        if (!load_member(starts, sizes, place, members, planes, a, i, Hg, Wg, r0, c0, m, p)) continue;
        ++touched;
        stage_member<HALF>(m, a, tile, mA, mK, lane, wave);
#pragma unroll
        for (int u = 0; u < TPX; ++u) {
#pragma clang fp contract(off)
            double A;
            int n;
            const float xf = window_sum<HALF>(tile, mA, mK, lane, wave + 4 * u, A, n);
            if (xf == xf && m.date != last[u]) {  // the first present member of its date decides for the date
                last[u] = m.date;
                const double mean = A / (double)n;  // n >= 1: the centre is present
                if (mean > 0.0) {
                    const double r = (double)xf / mean;
                    R[u] = R[u] + r;
                    c[u] += 1;
                }
            }
        }
    }
    if (!touched) return;

    // sweep 2: every member again; y = m (R / c), the scale, one store per element of the plane inside the tile
    for (int i = mb; i < me; ++i) {
        Member m;
        int p;
        if (!load_member(starts, sizes, place, members, planes, a, i, Hg, Wg, r0, c0, m, p)) continue;
        stage_member<HALF>(m, a, tile, mA, mK, lane, wave);
        int present = 0, dropped = 0, passed = 0, single = 0;
        const int pc = m.pc + lane;
#pragma unroll
        for (int u = 0; u < TPX; ++u) {
#pragma clang fp contract(off)
            double A;
            int n;
            const float xf = window_sum<HALF>(tile, mA, mK, lane, wave + 4 * u, A, n);
            const int pr = m.pr + wave + 4 * u;
            if (pr < 0 || pr >= m.H || pc < 0 || pc >= m.W) continue;
            unsigned bits = TQNAN;
            if (xf == xf) {
                const double mean = A / (double)n;
                double y = (double)xf;
                if (mean > 0.0 && c[u] >= 1) {
                    const double q = R[u] / (double)c[u];
                    y = mean * q;
                } else {
                    ++passed;
                }
                if (!a.to_db) {
                    bits = __float_as_uint((float)y);
                    ++present;
                    single += c[u] == 1;
                } else if (y > 0.0) {
                    const double db = 10.0 * log10(y);
                    bits = __float_as_uint((float)db);
                    ++present;
                    single += c[u] == 1;
                } else {
                    ++dropped;
                }
            }
            out[m.start + (long)pr * m.W + pc] = bits;
        }
        // a thread counts at most 8 pixels, a workgroup 2048: two counts share an int
        const int pd = wave_sum_int(present | (dropped << 16)), ps = wave_sum_int(passed | (single << 16));
        if (lane == 0) {
            part[wave] = pd;
            part[4 + wave] = ps;
        }
        __syncthreads();  // the next write of part lies behind the barriers of the next member's staging
        if (threadIdx.x == 0) {
            const int tpd = part[0] + part[1] + part[2] + part[3], tps = part[4] + part[5] + part[6] + part[7];
            if (tpd & 0xffff) atomicAdd(counts + 4 * p, tpd & 0xffff);
            if (tpd >> 16) atomicAdd(counts + 4 * p + 1, tpd >> 16);
            if (tps & 0xffff) atomicAdd(counts + 4 * p + 2, tps & 0xffff);
            if (tps >> 16) atomicAdd(counts + 4 * p + 3, tps >> 16);
        }
    }
}

}  // namespace

extern "C" int ig_s1_temporal(const float* planes, const long long* starts, const int* sizes, const int* place, const int* lattice,
                              const int* member_ptr, const int* members, const long long* tile_ptr, int N, int G, int M, long total, long tiles,
                              int h, int has_src_nodata, float src_nodata, int to_db, float* out, int* counts, void* stream) {
    IG_REQUIRE(h >= 1 && h <= TMAX_H, "ig_s1_temporal: the half window h must be in 1..%d (got %d)", TMAX_H, h);
    IG_REQUIRE(has_src_nodata == 0 || has_src_nodata == 1, "ig_s1_temporal: has_src_nodata must be 0 or 1 (got %d)", has_src_nodata);
    IG_REQUIRE(!has_src_nodata || src_nodata == src_nodata, "ig_s1_temporal: src_nodata must not be NaN (a NaN is absent anyway)");
    IG_REQUIRE(to_db == 0 || to_db == 1, "ig_s1_temporal: to_db must be 0 or 1 (got %d)", to_db);
    IG_REQUIRE(N >= 0, "ig_s1_temporal: need N >= 0 planes (got %d)", N);
    if (N == 0) return IG_OK;
    IG_REQUIRE(G >= 1 && G <= N, "ig_s1_temporal: %d planes form 1 <= G <= N groups (got %d)", N, G);
    IG_REQUIRE(M >= 0 && M <= N, "ig_s1_temporal: the member lists hold 0 <= M <= N entries (got %d)", M);
    IG_REQUIRE(total >= 0 && total < TLIM40, "ig_s1_temporal: the buffers hold 0 <= total < 2^40 elements (got %ld)", total);
    IG_REQUIRE(tiles >= 0 && tiles <= 0x7fffffffL, "ig_s1_temporal: 0 <= tiles <= 2^31 - 1 workgroups (got %ld)", tiles);
    IG_REQUIRE(planes && starts && sizes && place && lattice && member_ptr && members && tile_ptr && out && counts, "ig_s1_temporal: null pointer");
    IG_REQUIRE((((uintptr_t)planes | (uintptr_t)out | (uintptr_t)sizes | (uintptr_t)place | (uintptr_t)lattice | (uintptr_t)member_ptr |
                 (uintptr_t)members | (uintptr_t)counts) & 3) == 0 && (((uintptr_t)starts | (uintptr_t)tile_ptr) & 7) == 0,
               "ig_s1_temporal: planes, out, sizes, place, lattice, member_ptr, members and counts must be 4-byte, starts and tile_ptr 8-byte aligned");
    IG_REQUIRE(out + total <= planes || planes + total <= out, "ig_s1_temporal: out must not overlap planes");
    if (tiles == 0) return IG_OK;
    const TemporalArgs a{N, G, M, has_src_nodata, to_db, src_nodata, total};
    const int SH = TH + 2 * h;
    const int smem = SH * TW * ((int)sizeof(double) + (int)sizeof(int)) + SH * (TW + 2 * h) * (int)sizeof(float);
    const dim3 grid((unsigned)tiles);
    hipStream_t st = (hipStream_t)stream;
    unsigned* const o = reinterpret_cast<unsigned*>(out);
#define IG_TEMPORAL_HALF(HALF) \
    if (h == HALF)             \
    return ig_launch<s1_temporal_kernel<HALF>>("ig_s1_temporal", grid, dim3(TTPB), smem, st, planes, starts, sizes, place, lattice, member_ptr, members, tile_ptr, a, o, counts)
    IG_TEMPORAL_HALF(1);
    IG_TEMPORAL_HALF(2);
    IG_TEMPORAL_HALF(3);
    IG_TEMPORAL_HALF(4);
    IG_TEMPORAL_HALF(5);
    IG_TEMPORAL_HALF(6);
#undef IG_TEMPORAL_HALF
    return ig_launch<s1_temporal_kernel<TMAX_H>>("ig_s1_temporal", grid, dim3(TTPB), smem, st, planes, starts, sizes, place, lattice, member_ptr,
                                                  members, tile_ptr, a, o, counts);
}
