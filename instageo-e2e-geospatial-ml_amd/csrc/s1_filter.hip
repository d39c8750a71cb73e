// Speckle filtering and dB scaling of Sentinel-1 RTC planes for gfx950.  The reference copies linear gamma0 into its
// chips as it comes (instageo/data/s1_utils.py); here N float32 planes of any sizes, packed in one buffer as ig_s1_chip_cut packs them,
// are filtered in one launch by the rule stated in include/instageo_hip.h: windowed first and second moments of the PRESENT values in
// float64, in a fixed order, then BOXCAR, LEE or GAMMA_MAP, then linear or dB.  Every output depends on its window alone, so the bits
// are the same for any launch geometry; the counts are integer atomics, one pair per workgroup.
//
//   s1_speckle_kernel    one workgroup of 256 threads per tile of 64 columns x 32 rows of one plane; the workgroup finds its plane by a
//                        binary search in the caller's prefix table of tiles (tile_ptr, N + 1 entries) and its tile from the plane's own
//                        size.  Phase 1: the tile and its halo of h pixels, (32 + 2h) x (64 + 2h) float32, go to LDS, a wave per staged
//                        row, 64 (+ 2h) consecutive floats per load instruction; a value that is not finite, equals src_nodata or lies
//                        outside the plane becomes NaN there, so presence is one test afterwards.  Phase 2: the row moments (A_i, Q_i, K_i)
//                        of the 32 + 2h staged rows for the 64 columns of the tile, left to right over the window's columns, to LDS
//                        (float64, float64, int32): lane c reads the staged floats c .. c + 2h of a row, consecutive lanes consecutive
//                        banks.  Phase 3: a wave owns the output rows wave, wave + 4, ...; a thread sums the 2h + 1 row moments of its
//                        column top to bottom, applies the filter and the scale and stores one float32: 256 contiguous bytes per wave
//                        and store instruction wherever the plane starts (4-byte stores: rows of any W at any element offset have no
//                        wider common alignment).  A row outside the plane has moments +0.0, 0: adding it changes no bit (a sum that
//                        starts from +0.0 is never -0.0), which is how the window is clipped.  LDS at h = 7: 14 352 + 58 880 bytes, two
//                        workgroups per CU.
//   s1_refined_lee_kernel  the refined Lee filter (the rule is in the header): the same tile, plane lookup, staging, row
//                        moments, column sums, stores and counts at h = 3.  Before the column sums the workgroup also writes the means
//                        of the 3 x 3 sub-windows around the (32 + 4) x (64 + 4) centres its pixels can ask for, float64, NaN where a
//                        sub-window is empty; a pixel then reads nine of them, takes the direction, and sums its half window in one
//                        unrolled 7 x 7 loop over the staged tile under the direction's 49-bit mask (a value outside the mask adds
//                        +0.0), so the lanes of a wave stay together whatever their directions.  LDS 78 864 bytes, two workgroups per
//                        CU.
//
// Out-of-range accesses are impossible: a workgroup whose plane has H < 1, W < 1, H * W > 2^31 - 1, a negative start or an end beyond
// `total` returns at once, as does one whose tile number is not below the plane's own number of tiles; every load and store is guarded by
// row < H and column < W of that plane.  The caller guarantees that `planes` and `out` hold `total` elements.
#include "common.h"
#include "pixel_seg.h"

namespace {

constexpr int FW = 64, FH = 32, FTPB = 256, FMAX_H = 7;  // tile width and height, threads, the largest half window
constexpr long FLIM40 = 1L << 40;
constexpr unsigned FQNAN = 0x7fc00000u;
enum { BOXCAR = 0, LEE = 1, GAMMA_MAP = 2 };

struct SpeckleArgs {
    int N, method, has_nodata, to_db;
    float src_nodata;
    double looks, s;  // s = 1 / looks
    long total;
};

// the filtered value of a present centre x from the window sums (n >= 1); every operation rounded on its own
__device__ __forceinline__ double speckle_value(double A, double Q, int n, double x, const SpeckleArgs& a) {
#pragma clang fp contract(off)
    const double dn = (double)n;
    const double m = A / dn;
    const double q = Q / dn;
    const double mm = m * m;
    double v = q - mm;
    if (v < 0.0) v = 0.0;
    if (a.method == BOXCAR) return m;
    if (a.method == LEE) {
        const double t = mm * a.s;
        const double vx = (v - t) / (1.0 + a.s);
        const double b = (v > 0.0 && vx > 0.0) ? vx / v : 0.0;
        const double d = x - m;
        const double bd = b * d;
        return m + bd;
    }
    if (m <= 0.0) return m;
    const double ci2 = v / mm;
    if (ci2 <= a.s) return m;
    if (ci2 >= 2.0 * a.s) return x;
    const double al = (1.0 + a.s) / (ci2 - a.s);
    const double B = al - a.looks - 1.0;
    const double bb = B * B;
    const double d1 = mm * bb;
    const double mx = m * x;
    const double d2 = ((4.0 * al) * a.looks) * mx;
    const double D = d1 + d2;
    if (!(D >= 0.0)) return m;
    const double bm = B * m;
    const double num = bm + sqrt(D);
    return num / (2.0 * al);
}

// HALF = h: the window loops unroll, so the LDS reads of a sum are issued together; two rows per thread are in flight at a time (four
// independent float64 chains), and an absent value adds +0.0 instead of branching (a sum that began at +0.0 keeps its bits)
template <int HALF>
__global__ __launch_bounds__(FTPB, 2) void s1_speckle_kernel(const float* __restrict__ planes, const long long* __restrict__ starts,
                                                          const int* __restrict__ sizes, const long long* __restrict__ tile_ptr,
                                                          SpeckleArgs a, unsigned* __restrict__ out, int* __restrict__ counts) {
    extern __shared__ double lds[];
    __shared__ int part[4];
    constexpr int h = HALF, w = 2 * h + 1, SH = FH + 2 * h, SP = FW + 2 * h;  // window, staged rows, staged pitch
    double* const mA = lds;                                      // [SH][FW]
    double* const mQ = mA + SH * FW;                             // [SH][FW]
    int* const mK = reinterpret_cast<int*>(mQ + SH * FW);        // [SH][FW]
    float* const tile = reinterpret_cast<float*>(mK + SH * FW);  // [SH][SP]

    // the plane: the last p with tile_ptr[p] <= blockIdx.x
    const long long b = blockIdx.x;
    int lo = 0, hi = a.N;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tile_ptr[mid] <= b) lo = mid;
        else hi = mid;
    }
    const int p = lo;
    const int H = sizes[2 * p], W = sizes[2 * p + 1];
    const long long start = starts[p];
    if (H < 1 || W < 1 || (long)H * W > 0x7fffffffL || start < 0 || start + (long)H * W > a.total) return;  // the second fence
    const int nbx = (W + FW - 1) / FW, nby = (H + FH - 1) / FH;
    const long long k = b - tile_ptr[p];
    if (k < 0 || k >= (long long)nbx * nby) return;
    const int r0 = (int)(k / nbx) * FH, c0 = (int)(k % nbx) * FW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* const src = planes + start;
    const float nanf_ = __uint_as_float(FQNAN);

    // phase 1: the tile and its halo, absent values as NaN
    for (int r = wave; r < SH; r += 4) {
        const int gr = r0 - h + r;
        const bool row_in = gr >= 0 && gr < H;
#pragma unroll
        for (int c = lane; c < SP; c += 64) {
            const int gc = c0 - h + c;
            float f = nanf_;
            if (row_in && gc >= 0 && gc < W) {
                f = src[(long)gr * W + gc];
                if (!(fabsf(f) <= 3.402823466e+38f) || (a.has_nodata && f == a.src_nodata)) f = nanf_;
            }
            tile[r * SP + c] = f;
        }
    }
    __syncthreads();

    // phase 2: the row moments of every staged row for the tile's columns, left to right; rows r and r + 4 together
    {
#pragma clang fp contract(off)
        for (int r = wave; r < SH; r += 8) {
            const int r1 = min(r + 4, SH - 1);  // read inside the tile; stored only when it is a row of its own
            const float* row0 = tile + r * SP + lane;
            const float* row1 = tile + r1 * SP + lane;
            double A0 = 0.0, Q0 = 0.0, A1 = 0.0, Q1 = 0.0;
            int K0 = 0, K1 = 0;
#pragma unroll
            for (int j = 0; j < w; ++j) {
                const float f0 = row0[j], f1 = row1[j];
                const bool p0 = f0 == f0, p1 = f1 == f1;
                const double x0 = p0 ? (double)f0 : 0.0, x1 = p1 ? (double)f1 : 0.0;
                const double s0 = x0 * x0, s1 = x1 * x1;
                A0 = A0 + x0;
                A1 = A1 + x1;
                Q0 = Q0 + s0;
                Q1 = Q1 + s1;
                K0 += p0 ? 1 : 0;
                K1 += p1 ? 1 : 0;
            }
            mA[r * FW + lane] = A0;
            mQ[r * FW + lane] = Q0;
            mK[r * FW + lane] = K0;
            if (r + 4 < SH) {
                mA[(r + 4) * FW + lane] = A1;
                mQ[(r + 4) * FW + lane] = Q1;
                mK[(r + 4) * FW + lane] = K1;
            }
        }
    }
    __syncthreads();

    // phase 3: down the columns, the filter, the scale, one store; the output rows i and i + 4 together (FH is a multiple of 8)
    int present = 0, dropped = 0;
    const int gc = c0 + lane;
    {
#pragma clang fp contract(off)
        for (int i = wave; i < FH; i += 8) {
            double A[2] = {0.0, 0.0}, Q[2] = {0.0, 0.0};
            int n[2] = {0, 0};
#pragma unroll
            for (int j = 0; j < w; ++j) {
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int at = (i + 4 * u + j) * FW + lane;
                    A[u] = A[u] + mA[at];
                    Q[u] = Q[u] + mQ[at];
                    n[u] += mK[at];
                }
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int gr = r0 + i + 4 * u;
                if (gr >= H || gc >= W) continue;
                unsigned bits = FQNAN;
                const float xf = tile[(i + 4 * u + h) * SP + lane + h];
                if (xf == xf) {
                    const double y = speckle_value(A[u], Q[u], n[u], (double)xf, a);
                    if (!a.to_db) {
                        bits = __float_as_uint((float)y);
                        ++present;
                    } else if (y > 0.0) {
                        const double db = 10.0 * log10(y);
                        bits = __float_as_uint((float)db);
                        ++present;
                    } else {
                        ++dropped;
                    }
                }
                out[start + (long)gr * W + gc] = bits;
            }
        }
    }
    const int tp = block_sum_int(present, part);
    __syncthreads();  // part is read by every thread before it is written again
    const int td = block_sum_int(dropped, part);
    if (threadIdx.x == 0) {
        if (tp) atomicAdd(counts + 2 * p, tp);
        if (td) atomicAdd(counts + 2 * p + 1, td);
    }
}

// ---- the refined Lee filter -------------------------------------------------------------------------------------------
constexpr int RH = 3, RSH = FH + 2 * RH, RSP = FW + 2 * RH;  // the half window, staged rows, staged pitch
constexpr int RMH = FH + 4, RMW = FW + 4;                    // the plane of sub-window means: centres up to 2 pixels outside the tile
constexpr int RLDS = RSH * FW * (2 * (int)sizeof(double) + (int)sizeof(int)) + RMH * RMW * (int)sizeof(double) + RSH * RSP * (int)sizeof(float);
enum { DIR_SE = 0, DIR_NW, DIR_NE, DIR_SW, DIR_E, DIR_W, DIR_S, DIR_N };

// the half window of a direction as 49 bits: bit 7 (dy + 3) + (dx + 3) is set where the mask holds the offset (dy, dx)
constexpr unsigned long long half_mask(int dir) {
    unsigned long long m = 0;
    for (int dy = -3; dy <= 3; ++dy)
        for (int dx = -3; dx <= 3; ++dx) {
            const bool in = dir == DIR_SE ? dx + dy >= 0 : dir == DIR_NW ? dx + dy <= 0 : dir == DIR_NE ? dx - dy >= 0 : dir == DIR_SW ? dx - dy <= 0
                          : dir == DIR_E ? dx >= 0 : dir == DIR_W ? dx <= 0 : dir == DIR_S ? dy >= 0 : dy <= 0;
            if (in) m |= 1ull << (7 * (dy + 3) + (dx + 3));
        }
    return m;
}

struct LeeTerms {
    double m, v, vx;
};
// m, v and vx of LEE from the sums of a window (n >= 1), in the order of speckle_value
__device__ __forceinline__ LeeTerms lee_terms(double A, double Q, int n, double s) {
#pragma clang fp contract(off)
    const double dn = (double)n;
    const double m = A / dn;
    const double q = Q / dn;
    const double mm = m * m;
    double v = q - mm;
    if (v < 0.0) v = 0.0;
    const double t = mm * s;
    const double vx = (v - t) / (1.0 + s);
    return {m, v, vx};
}
__device__ __forceinline__ double lee_apply(const LeeTerms& k, double x) {
#pragma clang fp contract(off)
    const double b = (k.v > 0.0 && k.vx > 0.0) ? k.vx / k.v : 0.0;
    const double d = x - k.m;
    const double bd = b * d;
    return k.m + bd;
}

// Steps 1 to 4 of the rule for a present centre x.  (A, Q, n): the sums of the full window; win: the staged float of the window's top
// left corner; sub: the mean of the sub-window i = j = 0 (the others lie 2 i rows and 2 j columns on, NaN where a sub-window is empty).
__device__ __forceinline__ double refined_lee_value(double A, double Q, int n, double x, const float* win, const double* sub, double s) {
#pragma clang fp contract(off)
    const LeeTerms full = lee_terms(A, Q, n, s);
    if (!(full.v > 0.0 && full.vx > 0.0)) return full.m;  // homogeneous
    double M[3][3];
    bool all = true;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            M[i][j] = sub[2 * i * RMW + 2 * j];
            all = all && M[i][j] == M[i][j];
        }
    if (!all) return lee_apply(full, x);  // the fallback
    const double c0 = M[1][1];
    const double gd1 = fabs(((M[1][2] + M[2][1]) + M[2][2]) - ((M[0][0] + M[0][1]) + M[1][0]));
    const double gd2 = fabs(((M[0][1] + M[0][2]) + M[1][2]) - ((M[1][0] + M[2][0]) + M[2][1]));
    const double gh = fabs(((M[0][2] + M[1][2]) + M[2][2]) - ((M[0][0] + M[1][0]) + M[2][0]));
    const double gv = fabs(((M[2][0] + M[2][1]) + M[2][2]) - ((M[0][0] + M[0][1]) + M[0][2]));
    // the first-named half of each pair wins when its sub-window is at least as close to the centre mean
    const bool se = fabs(M[2][2] - c0) <= fabs(M[0][0] - c0), ne = fabs(M[0][2] - c0) <= fabs(M[2][0] - c0);
    const bool e = fabs(M[1][2] - c0) <= fabs(M[1][0] - c0), so = fabs(M[2][1] - c0) <= fabs(M[0][1] - c0);
    double best = gd1;
    unsigned long long mask = se ? half_mask(DIR_SE) : half_mask(DIR_NW);
    if (gd2 > best) {
        best = gd2;
        mask = ne ? half_mask(DIR_NE) : half_mask(DIR_SW);
    }
    if (gh > best) {
        best = gh;
        mask = e ? half_mask(DIR_E) : half_mask(DIR_W);
    }
    if (gv > best) mask = so ? half_mask(DIR_S) : half_mask(DIR_N);
    // one uniform 7 x 7 loop: a value outside the mask, absent or outside the plane adds +0.0 and counts 0
    const unsigned mlo = (unsigned)mask, mhi = (unsigned)(mask >> 32);
    double As = 0.0, Qs = 0.0;
    int ns = 0;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        double Ar = 0.0, Qr = 0.0;
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const int k = 7 * i + j;
            const float f = win[i * RSP + j];
            const bool in = ((k < 32 ? mlo >> k : mhi >> (k - 32)) & 1u) != 0 && f == f;
            const double xv = in ? (double)f : 0.0;
            const double sq = xv * xv;
            Ar = Ar + xv;
            Qr = Qr + sq;
            ns += in ? 1 : 0;
        }
        As = As + Ar;
        Qs = Qs + Qr;
    }
    return lee_apply(lee_terms(As, Qs, ns, s), x);
}

// The tile, the plane lookup, the staging, the row moments, the column sums, the stores and the counts of s1_speckle_kernel at h = 3;
// between the row moments and the column sums the sub-window means of the tile go to LDS
__global__ __launch_bounds__(FTPB, 2) void s1_refined_lee_kernel(const float* __restrict__ planes, const long long* __restrict__ starts,
                                                              const int* __restrict__ sizes, const long long* __restrict__ tile_ptr,
                                                              SpeckleArgs a, unsigned* __restrict__ out, int* __restrict__ counts) {
    extern __shared__ double lds[];
    __shared__ int part[4];
    constexpr int h = RH, w = 2 * RH + 1, SH = RSH, SP = RSP;
    double* const mA = lds;                                      // [SH][FW]
    double* const mQ = mA + SH * FW;                             // [SH][FW]
    double* const sM = mQ + SH * FW;                             // [RMH][RMW]
    int* const mK = reinterpret_cast<int*>(sM + RMH * RMW);      // [SH][FW]
    float* const tile = reinterpret_cast<float*>(mK + SH * FW);  // [SH][SP]

    // the plane: the last p with tile_ptr[p] <= blockIdx.x
    const long long b = blockIdx.x;
    int lo = 0, hi = a.N;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tile_ptr[mid] <= b) lo = mid;
        else hi = mid;
    }
    const int p = lo;
    const int H = sizes[2 * p], W = sizes[2 * p + 1];
    const long long start = starts[p];
    if (H < 1 || W < 1 || (long)H * W > 0x7fffffffL || start < 0 || start + (long)H * W > a.total) return;  // the second fence
    const int nbx = (W + FW - 1) / FW, nby = (H + FH - 1) / FH;
    const long long k = b - tile_ptr[p];
    if (k < 0 || k >= (long long)nbx * nby) return;
    const int r0 = (int)(k / nbx) * FH, c0 = (int)(k % nbx) * FW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* const src = planes + start;
    const float nanf_ = __uint_as_float(FQNAN);

    // phase 1: the tile and its halo, absent values as NaN
    for (int r = wave; r < SH; r += 4) {
        const int gr = r0 - h + r;
        const bool row_in = gr >= 0 && gr < H;
#pragma unroll
        for (int c = lane; c < SP; c += 64) {
            const int gc = c0 - h + c;
            float f = nanf_;
            if (row_in && gc >= 0 && gc < W) {
                f = src[(long)gr * W + gc];
                if (!(fabsf(f) <= 3.402823466e+38f) || (a.has_nodata && f == a.src_nodata)) f = nanf_;
            }
            tile[r * SP + c] = f;
        }
    }
    __syncthreads();

    // phase 2: the row moments of every staged row for the tile's columns, left to right; rows r and r + 4 together
    {
#pragma clang fp contract(off)
        for (int r = wave; r < SH; r += 8) {
            const int r1 = min(r + 4, SH - 1);  // read inside the tile; stored only when it is a row of its own
            const float* row0 = tile + r * SP + lane;
            const float* row1 = tile + r1 * SP + lane;
            double A0 = 0.0, Q0 = 0.0, A1 = 0.0, Q1 = 0.0;
            int K0 = 0, K1 = 0;
#pragma unroll
            for (int j = 0; j < w; ++j) {
                const float f0 = row0[j], f1 = row1[j];
                const bool p0 = f0 == f0, p1 = f1 == f1;
                const double x0 = p0 ? (double)f0 : 0.0, x1 = p1 ? (double)f1 : 0.0;
                const double s0 = x0 * x0, s1 = x1 * x1;
                A0 = A0 + x0;
                A1 = A1 + x1;
                Q0 = Q0 + s0;
                Q1 = Q1 + s1;
                K0 += p0 ? 1 : 0;
                K1 += p1 ? 1 : 0;
            }
            mA[r * FW + lane] = A0;
            mQ[r * FW + lane] = Q0;
            mK[r * FW + lane] = K0;
            if (r + 4 < SH) {
                mA[(r + 4) * FW + lane] = A1;
                mQ[(r + 4) * FW + lane] = Q1;
                mK[(r + 4) * FW + lane] = K1;
            }
        }
        // the mean of the 3 x 3 sub-window around every centre a pixel of the tile can ask for: entry (i, j) is centred on the staged
        // float (i + 1, j + 1), which is the pixel (r0 - 2 + i, c0 - 2 + j); NaN where nothing is present
        for (int e = threadIdx.x; e < RMH * RMW; e += FTPB) {
            const int i = e / RMW, j = e - i * RMW;
            const float* const t = tile + i * SP + j;
            double A3 = 0.0;
            int n3 = 0;
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                double Ar = 0.0;
#pragma unroll
                for (int v = 0; v < 3; ++v) {
                    const float f = t[u * SP + v];
                    const bool pr = f == f;
                    Ar = Ar + (pr ? (double)f : 0.0);
                    n3 += pr ? 1 : 0;
                }
                A3 = A3 + Ar;
            }
            sM[e] = n3 ? A3 / (double)n3 : (double)nanf_;
        }
    }
    __syncthreads();

    // phase 3: down the columns, the filter, the scale, one store
    int present = 0, dropped = 0;
    const int gc = c0 + lane;
    {
#pragma clang fp contract(off)
        for (int i = wave; i < FH; i += 4) {
            double A = 0.0, Q = 0.0;
            int n = 0;
#pragma unroll
            for (int j = 0; j < w; ++j) {
                const int at = (i + j) * FW + lane;
                A = A + mA[at];
                Q = Q + mQ[at];
                n += mK[at];
            }
            const int gr = r0 + i;
            if (gr >= H || gc >= W) continue;
            unsigned bits = FQNAN;
            const float xf = tile[(i + h) * SP + lane + h];
            if (xf == xf) {
                const double y = refined_lee_value(A, Q, n, (double)xf, tile + i * SP + lane, sM + i * RMW + lane, a.s);
                if (!a.to_db) {
                    bits = __float_as_uint((float)y);
                    ++present;
                } else if (y > 0.0) {
                    const double db = 10.0 * log10(y);
                    bits = __float_as_uint((float)db);
                    ++present;
                } else {
                    ++dropped;
                }
            }
            out[start + (long)gr * W + gc] = bits;
        }
    }
    const int tp = block_sum_int(present, part);
    __syncthreads();  // part is read by every thread before it is written again
    const int td = block_sum_int(dropped, part);
    if (threadIdx.x == 0) {
        if (tp) atomicAdd(counts + 2 * p, tp);
        if (td) atomicAdd(counts + 2 * p + 1, td);
    }
}

}  // namespace

extern "C" int ig_s1_refined_lee(const float* planes, const long long* starts, const int* sizes, const long long* tile_ptr, int N, long total,
                                 long tiles, float looks, int has_src_nodata, float src_nodata, int to_db, float* out, int* counts,
                                 void* stream) {
    IG_REQUIRE(looks > 0.f && looks <= 3.402823466e+38f, "ig_s1_refined_lee: looks must be finite and > 0 (got %g)", (double)looks);
    IG_REQUIRE(has_src_nodata == 0 || has_src_nodata == 1, "ig_s1_refined_lee: has_src_nodata must be 0 or 1 (got %d)", has_src_nodata);
    IG_REQUIRE(!has_src_nodata || src_nodata == src_nodata, "ig_s1_refined_lee: src_nodata must not be NaN (a NaN is absent anyway)");
    IG_REQUIRE(to_db == 0 || to_db == 1, "ig_s1_refined_lee: to_db must be 0 or 1 (got %d)", to_db);
    IG_REQUIRE(N >= 0, "ig_s1_refined_lee: need N >= 0 planes (got %d)", N);
    if (N == 0) return IG_OK;
    IG_REQUIRE(total >= 0 && total < FLIM40, "ig_s1_refined_lee: the buffers hold 0 <= total < 2^40 elements (got %ld)", total);
    IG_REQUIRE(tiles >= 0 && tiles <= 0x7fffffffL, "ig_s1_refined_lee: 0 <= tiles <= 2^31 - 1 workgroups (got %ld)", tiles);
    IG_REQUIRE(planes && starts && sizes && tile_ptr && out && counts, "ig_s1_refined_lee: null pointer");
    IG_REQUIRE((((uintptr_t)planes | (uintptr_t)out | (uintptr_t)sizes | (uintptr_t)counts) & 3) == 0 &&
                   (((uintptr_t)starts | (uintptr_t)tile_ptr) & 7) == 0,
               "ig_s1_refined_lee: planes, out, sizes and counts must be 4-byte, starts and tile_ptr 8-byte aligned");
    IG_REQUIRE(out + total <= planes || planes + total <= out, "ig_s1_refined_lee: out must not overlap planes");
    if (tiles == 0) return IG_OK;
    const SpeckleArgs a{N, LEE, has_src_nodata, to_db, src_nodata, (double)looks, 1.0 / (double)looks, total};
    return ig_launch<s1_refined_lee_kernel>("ig_s1_refined_lee", dim3((unsigned)tiles), dim3(FTPB), RLDS, (hipStream_t)stream, planes, starts,
                                            sizes, tile_ptr, a, reinterpret_cast<unsigned*>(out), counts);
}

extern "C" int ig_s1_speckle(const float* planes, const long long* starts, const int* sizes, const long long* tile_ptr, int N, long total,
                             long tiles, int h, int method, float looks, int has_src_nodata, float src_nodata, int to_db, float* out,
                             int* counts, void* stream) {
    IG_REQUIRE(h >= 1 && h <= FMAX_H, "ig_s1_speckle: the half window h must be in 1..%d (got %d)", FMAX_H, h);
    IG_REQUIRE(method >= BOXCAR && method <= GAMMA_MAP, "ig_s1_speckle: method must be 0 boxcar, 1 lee or 2 gamma_map (got %d)", method);
    IG_REQUIRE(looks > 0.f && looks <= 3.402823466e+38f, "ig_s1_speckle: looks must be finite and > 0 (got %g)", (double)looks);
    IG_REQUIRE(has_src_nodata == 0 || has_src_nodata == 1, "ig_s1_speckle: has_src_nodata must be 0 or 1 (got %d)", has_src_nodata);
    IG_REQUIRE(!has_src_nodata || src_nodata == src_nodata, "ig_s1_speckle: src_nodata must not be NaN (a NaN is absent anyway)");
    IG_REQUIRE(to_db == 0 || to_db == 1, "ig_s1_speckle: to_db must be 0 or 1 (got %d)", to_db);
    IG_REQUIRE(N >= 0, "ig_s1_speckle: need N >= 0 planes (got %d)", N);
    if (N == 0) return IG_OK;
    IG_REQUIRE(total >= 0 && total < FLIM40, "ig_s1_speckle: the buffers hold 0 <= total < 2^40 elements (got %ld)", total);
    IG_REQUIRE(tiles >= 0 && tiles <= 0x7fffffffL, "ig_s1_speckle: 0 <= tiles <= 2^31 - 1 workgroups (got %ld)", tiles);
    IG_REQUIRE(planes && starts && sizes && tile_ptr && out && counts, "ig_s1_speckle: null pointer");
    IG_REQUIRE((((uintptr_t)planes | (uintptr_t)out | (uintptr_t)sizes | (uintptr_t)counts) & 3) == 0 &&
                   (((uintptr_t)starts | (uintptr_t)tile_ptr) & 7) == 0,
               "ig_s1_speckle: planes, out, sizes and counts must be 4-byte, starts and tile_ptr 8-byte aligned");
    IG_REQUIRE(out + total <= planes || planes + total <= out, "ig_s1_speckle: out must not overlap planes");
    if (tiles == 0) return IG_OK;
    const SpeckleArgs a{N, method, has_src_nodata, to_db, src_nodata, (double)looks, 1.0 / (double)looks, total};
    const int SH = FH + 2 * h;
    const int smem = SH * FW * (2 * (int)sizeof(double) + (int)sizeof(int)) + SH * (FW + 2 * h) * (int)sizeof(float);
    const dim3 grid((unsigned)tiles);
    hipStream_t st = (hipStream_t)stream;
    unsigned* const o = reinterpret_cast<unsigned*>(out);
#define IG_SPECKLE_HALF(HALF) \
    if (h == HALF) return ig_launch<s1_speckle_kernel<HALF>>("ig_s1_speckle", grid, dim3(FTPB), smem, st, planes, starts, sizes, tile_ptr, a, o, counts)
    IG_SPECKLE_HALF(1);
    IG_SPECKLE_HALF(2);
    IG_SPECKLE_HALF(3);
    IG_SPECKLE_HALF(4);
    IG_SPECKLE_HALF(5);
    IG_SPECKLE_HALF(6);
#undef IG_SPECKLE_HALF
    return ig_launch<s1_speckle_kernel<FMAX_H>>("ig_s1_speckle", grid, dim3(FTPB), smem, st, planes, starts, sizes, tile_ptr, a, o, counts);
}
