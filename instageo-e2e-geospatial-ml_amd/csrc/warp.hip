// Reprojection and resampling of north-up rasters between grids for gfx950.  The reference's viewer reprojects with
// rasterio before display (apps/viz.py); here the warp is what brings the mosaics of several UTM zones onto one canvas.  The rule is stated
// in include/instageo_hip.h.  A GATHER: every destination pixel is computed by the one thread that stores it.  No atomics, no waiting
// between workgroups, every result unique (independent of scheduling).
//
//   coords_kernel     one thread per destination pixel: (u, v) in one source grid, as float64 planes.
//   warp_kernel<T, BILINEAR>   one workgroup of 256 threads per 64 x 64 block of the destination (origin at multiples of 64: the blocking of
//                     mosaic.hip and cog.hip).  The descriptions of the (at most 8) sources are checked and staged in LDS once; the block's
//                     source list (CSR, built by the host) is walked backwards (last) or forwards (first) until a source contributes.  A
//                     wave owns 64 consecutive pixels of a row and stores them with one instruction; a thread takes 16 rows in turn.
//                     The longitude and latitude of a pixel are computed once, when the first source of another coordinate system asks
//                     for them; sources of one coordinate system share the forward projection.
//
// Out-of-range accesses are impossible as long as starts[i] + h * w lies inside the packed buffer (the caller's promise, checked by
// ops.warp): a source index outside [0, nsrc) or a description outside the stated bounds is staged as an empty source, every source load
// is guarded by 0 <= row < h and 0 <= column < w, tested on the float64 coordinates before they become integers (NaN fails), every store
// by row < H and column < W.
#include "common.h"

namespace {

constexpr int WB = 64, WTPB = 256, WMAX = 8;  // block side, threads, sources per launch
constexpr int WLIM = 1 << 30;                 // h, w at most this
constexpr int R_LAST = 0, R_FIRST = 1;

// WGS84
constexpr double WA = 6378137.0, WF = 1.0 / 298.257223563;
constexpr double WE2 = WF * (2.0 - WF), WE = 0.081819190842621494335;  // e^2, e
constexpr double WN = WF / (2.0 - WF);                                 // third flattening n
constexpr double N2 = WN * WN, N3 = N2 * WN, N4 = N3 * WN, N5 = N4 * WN, N6 = N5 * WN;
constexpr double WRECT = WA / (1.0 + WN) * (1.0 + N2 / 4.0 + N4 / 64.0 + N6 / 256.0);  // rectifying radius A
constexpr double D2R = 0.017453292519943295769, R2D = 57.295779513082320877, HALF_PI = 1.5707963267948966192;
constexpr double LAT_MAX = 89.9, DLON_MAX = 80.0;
// Krueger's series to n^6 (Karney 2011, eqs. 35 and 36): forward alpha_j, inverse beta_j
constexpr double AL1 = WN / 2 - 2 * N2 / 3 + 5 * N3 / 16 + 41 * N4 / 180 - 127 * N5 / 288 + 7891 * N6 / 37800;
constexpr double AL2 = 13 * N2 / 48 - 3 * N3 / 5 + 557 * N4 / 1440 + 281 * N5 / 630 - 1983433 * N6 / 1935360;
constexpr double AL3 = 61 * N3 / 240 - 103 * N4 / 140 + 15061 * N5 / 26880 + 167603 * N6 / 181440;
constexpr double AL4 = 49561 * N4 / 161280 - 179 * N5 / 168 + 6601661 * N6 / 7257600;
constexpr double AL5 = 34729 * N5 / 80640 - 3418889 * N6 / 1995840;
constexpr double AL6 = 212378941 * N6 / 319334400;
constexpr double BE1 = WN / 2 - 2 * N2 / 3 + 37 * N3 / 96 - N4 / 360 - 81 * N5 / 512 + 96199 * N6 / 604800;
constexpr double BE2 = N2 / 48 + N3 / 15 - 437 * N4 / 1440 + 46 * N5 / 105 - 1118711 * N6 / 3870720;
constexpr double BE3 = 17 * N3 / 480 - 37 * N4 / 840 - 209 * N5 / 4480 + 5569 * N6 / 90720;
constexpr double BE4 = 4397 * N4 / 161280 - 11 * N5 / 504 - 830251 * N6 / 7257600;
constexpr double BE5 = 4583 * N5 / 161280 - 108847 * N6 / 3991680;
constexpr double BE6 = 20648693 * N6 / 638668800;

struct Crs {
    double kind, lon0, k0, fe, fn;
};
struct Grid {
    double x0, y0, sx, sy;
};

__device__ __forceinline__ bool same_crs(const Crs& a, const Crs& b) {
    return a.kind == b.kind && a.lon0 == b.lon0 && a.k0 == b.k0 && a.fe == b.fe && a.fn == b.fn;
}

// (xi, eta) + sign * sum_j c_j sin(2j (xi + i eta)): sin / cos of 2j xi and sinh / cosh of 2j eta by angle addition from the first pair
__device__ __forceinline__ void kruger(double xi, double eta, double sign, double c1, double c2, double c3, double c4, double c5, double c6,
                                       double& oxi, double& oeta) {
    double s1, k1;
    sincos(2.0 * xi, &s1, &k1);
    const double sh1 = sinh(2.0 * eta), ch1 = cosh(2.0 * eta);
    const double c[6] = {c1, c2, c3, c4, c5, c6};
    double s = s1, k = k1, sh = sh1, ch = ch1, ax = 0.0, ae = 0.0;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        ax += c[j] * (s * ch);
        ae += c[j] * (k * sh);
        const double sn = s * k1 + k * s1, kn = k * k1 - s * s1;
        const double shn = sh * ch1 + ch * sh1, chn = ch * ch1 + sh * sh1;
        s = sn, k = kn, sh = shn, ch = chn;
    }
    oxi = xi + sign * ax, oeta = eta + sign * ae;
}

// tan of the conformal latitude from tan of the geographic one
__device__ __forceinline__ double taup_of(double tau) {
    const double t1 = sqrt(1.0 + tau * tau);
    const double sig = sinh(WE * atanh(WE * tau / t1));
    return tau * sqrt(1.0 + sig * sig) - sig * t1;
}

// (x, y) of `c` -> longitude, latitude in degrees; false outside the domain
__device__ __forceinline__ bool to_lonlat(const Crs& c, double x, double y, double& lon, double& lat) {
    if (c.kind == 0.0) {
        lon = x, lat = y;
    } else if (c.kind == 2.0) {
        lon = x / WA * R2D;
        lat = atan(sinh(y / WA)) * R2D;
    } else {
        const double ka = c.k0 * WRECT;
        double xip, etap;
        kruger((y - c.fn) / ka, (x - c.fe) / ka, -1.0, BE1, BE2, BE3, BE4, BE5, BE6, xip, etap);
        if (!(fabs(xip) <= HALF_PI)) return false;
        double sx, cx;
        sincos(xip, &sx, &cx);
        const double sh = sinh(etap);
        const double tp = sx / sqrt(sh * sh + cx * cx);
        double tau = tp / (1.0 - WE2);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double tpi = taup_of(tau);
            tau += (tp - tpi) / sqrt(1.0 + tpi * tpi) * (1.0 + (1.0 - WE2) * tau * tau) / ((1.0 - WE2) * sqrt(1.0 + tau * tau));
        }
        lon = c.lon0 + atan2(sh, cx) * R2D;
        lat = atan(tau) * R2D;
    }
    return isfinite(lon) && isfinite(lat) && fabs(lat) <= LAT_MAX;
}

// longitude, latitude (degrees, inside the domain of to_lonlat) -> (x, y) of `c`; false outside the domain
__device__ __forceinline__ bool from_lonlat(const Crs& c, double lon, double lat, double& x, double& y) {
    if (c.kind == 0.0) {
        x = lon, y = lat;
    } else if (c.kind == 2.0) {
        x = WA * (lon * D2R);
        y = WA * asinh(tan(lat * D2R));
    } else {
        const double dl = remainder(lon - c.lon0, 360.0);
        if (!(fabs(dl) < DLON_MAX)) return false;
        const double tp = taup_of(tan(lat * D2R));
        double sl, cl;
        sincos(dl * D2R, &sl, &cl);
        double xi, eta;
        kruger(atan2(tp, cl), asinh(sl / sqrt(tp * tp + cl * cl)), 1.0, AL1, AL2, AL3, AL4, AL5, AL6, xi, eta);
        const double ka = c.k0 * WRECT;
        x = c.fe + ka * eta, y = c.fn + ka * xi;
    }
    return true;
}

__device__ __forceinline__ Crs load_crs(const double* p) { return Crs{p[0], p[1], p[2], p[3], p[4]}; }
__device__ __forceinline__ Grid load_grid(const double* p) { return Grid{p[0], p[1], p[2], p[3]}; }
__device__ __forceinline__ bool grid_ok(const Grid& g) { return isfinite(g.x0) && isfinite(g.y0) && g.sx > 0.0 && g.sy > 0.0 && isfinite(g.sx) && isfinite(g.sy); }

__global__ __launch_bounds__(WTPB) void coords_kernel(const double* __restrict__ dst_crs, const double* __restrict__ dst_grid, int H, int W,
                                                      const double* __restrict__ src_crs, const double* __restrict__ src_grid,
                                                      double* __restrict__ uv) {
    const int c = blockIdx.x * WB + (threadIdx.x & 63), r = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (r >= H || c >= W) return;
    const Crs dc = load_crs(dst_crs), sc = load_crs(src_crs);
    const Grid dg = load_grid(dst_grid), sg = load_grid(src_grid);
    double x = dg.x0 + (c + 0.5) * dg.sx, y = dg.y0 - (r + 0.5) * dg.sy;
    bool ok = grid_ok(sg);
    if (ok && !same_crs(dc, sc)) {
        double lon, lat;
        ok = to_lonlat(dc, x, y, lon, lat) && from_lonlat(sc, lon, lat, x, y);
    }
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const long at = (long)r * W + c;
    uv[at] = ok ? (x - sg.x0) / sg.sx : nan;
    uv[(long)H * W + at] = ok ? (sg.y0 - y) / sg.sy : nan;
}

struct Sources {
    Crs crs[WMAX];
    Grid grid[WMAX];
    long long start[WMAX];
    int h[WMAX], w[WMAX];  // h = 0: contributes nothing
    int same[WMAX];        // the destination's coordinate system: affine
    int rep[WMAX];         // the smallest index with this coordinate system
};

__device__ __forceinline__ bool clear_px(signed char v, int fill) { return v == (signed char)fill; }
__device__ __forceinline__ bool clear_px(float v, int) { return v != v; }

// the value source e gives at (u, v); false: no contribution
template <typename T, bool BILINEAR>
__device__ __forceinline__ bool sample(const T* __restrict__ src, const Sources& s, int e, double u, double v, int fill, T& out) {
    const int h = s.h[e], w = s.w[e];
    const T* p = src + s.start[e];
    if constexpr (!BILINEAR) {
        const double fc = floor(u), fr = floor(v);
        if (!(fc >= 0.0 && fc < (double)w && fr >= 0.0 && fr < (double)h)) return false;
        const T x = p[(long)fr * w + (long)fc];
        if (clear_px(x, fill)) return false;
        out = x;
        return true;
    } else {
        const double a = u - 0.5, b = v - 0.5;
        const double fc = floor(a), fr = floor(b);
        if (!(fc >= -1.0 && fc < (double)w && fr >= -1.0 && fr < (double)h)) return false;  // no neighbour inside (NaN included)
        const int c0 = (int)fc, r0 = (int)fr;
        const double wx = a - fc, wy = b - fr;
        const double wt[4] = {(1.0 - wx) * (1.0 - wy), wx * (1.0 - wy), (1.0 - wx) * wy, wx * wy};
        double acc = 0.0, tot = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int rr = r0 + (q >> 1), cc = c0 + (q & 1);
            if ((unsigned)rr < (unsigned)h && (unsigned)cc < (unsigned)w && wt[q] > 0.0) {
                const float x = p[(long)rr * w + cc];
                if (x == x) acc += wt[q] * (double)x, tot += wt[q];
            }
        }
        if (!(tot > 0.0)) return false;
        out = (float)(acc / tot);
        return true;
    }
}

template <typename T, bool BILINEAR>
__global__ __launch_bounds__(WTPB) void warp_kernel(const T* __restrict__ src, const long long* __restrict__ starts,
                                                    const double* __restrict__ src_crs, const double* __restrict__ src_grid,
                                                    const int* __restrict__ src_size, int nsrc, const int* __restrict__ bin_ptr,
                                                    const int* __restrict__ bin_idx, const double* __restrict__ dst_crs,
                                                    const double* __restrict__ dst_grid, int H, int W, int rule, int fill, T* __restrict__ dst,
                                                    unsigned char* __restrict__ src_id) {
    __shared__ Sources s;
    const Crs dc = load_crs(dst_crs);
    const Grid dg = load_grid(dst_grid);
    if ((int)threadIdx.x < WMAX) {
        const int i = threadIdx.x;
        Crs c{0.0, 0.0, 0.0, 0.0, 0.0};
        Grid g{0.0, 0.0, 1.0, 1.0};
        long long st = 0;
        int h = 0, w = 0, rep = i;
        if (i < nsrc) {
            c = load_crs(src_crs + 5 * i);
            g = load_grid(src_grid + 4 * i);
            st = starts[i];
            const int hh = src_size[2 * i], ww = src_size[2 * i + 1];
            if (hh >= 1 && ww >= 1 && hh <= WLIM && ww <= WLIM && st >= 0 && grid_ok(g)) h = hh, w = ww;
            for (int j = i - 1; j >= 0; --j)
                if (same_crs(load_crs(src_crs + 5 * j), c)) rep = j;
        }
        s.crs[i] = c, s.grid[i] = g, s.start[i] = st, s.h[i] = h, s.w[i] = w, s.same[i] = same_crs(c, dc), s.rep[i] = rep;
    }
    __syncthreads();
    const int b = blockIdx.y * gridDim.x + blockIdx.x;
    const int first = bin_ptr ? bin_ptr[b] : 0;
    const int n = bin_ptr ? max(bin_ptr[b + 1] - first, 0) : 0;
    const int* list = bin_idx + first;
    const int c = blockIdx.x * WB + (threadIdx.x & 63);
    if (c >= W) return;
    const double x = dg.x0 + (c + 0.5) * dg.sx;
    for (int k = 0; k < WB / 4; ++k) {
        const int r = blockIdx.y * WB + 4 * k + (threadIdx.x >> 6);  // wave-uniform
        if (r >= H) break;
        const double y = dg.y0 - (r + 0.5) * dg.sy;
        T out;
        if constexpr (sizeof(T) == 1) out = (T)fill;
        else out = __uint_as_float(0x7fc00000u);
        int who = 255;
        int ll = 0;  // 0: longitude / latitude not asked for yet, 1: inside the domain, -1: outside
        double lon = 0.0, lat = 0.0, px = 0.0, py = 0.0;
        int cur = -1;  // the coordinate system (px, py) belongs to
        bool pok = false;
        for (int i = 0; i < n; ++i) {
            const int e = list[rule == R_LAST ? n - 1 - i : i];
            if ((unsigned)e >= (unsigned)nsrc || s.h[e] == 0) continue;
            double sxp, syp;
            if (s.same[e]) {
                sxp = x, syp = y;
            } else {
                if (ll == 0) ll = to_lonlat(dc, x, y, lon, lat) ? 1 : -1;
                if (ll < 0) continue;  // outside the destination's domain: only a source of its own system can contribute
                if (s.rep[e] != cur) cur = s.rep[e], pok = from_lonlat(s.crs[e], lon, lat, px, py);
                if (!pok) continue;
                sxp = px, syp = py;
            }
            const Grid& g = s.grid[e];
            if (sample<T, BILINEAR>(src, s, e, (sxp - g.x0) / g.sx, (g.y0 - syp) / g.sy, fill, out)) {
                who = e;
                break;
            }
        }
        const long at = (long)r * W + c;
        dst[at] = out;
        if (src_id) src_id[at] = (unsigned char)who;
    }
}

template <typename T, bool BILINEAR>
int launch(const void* src, const long long* starts, const double* src_crs, const double* src_grid, const int* src_size, int nsrc,
           const int* bin_ptr, const int* bin_idx, const double* dst_crs, const double* dst_grid, int H, int W, int rule, int fill, void* dst,
           unsigned char* src_id, void* stream) {
    return ig_launch<warp_kernel<T, BILINEAR>>("ig_warp", dim3((unsigned)ig_cdiv(W, WB), (unsigned)ig_cdiv(H, WB)), dim3(WTPB), 0,
                                               (hipStream_t)stream, (const T*)src, starts, src_crs, src_grid, src_size, nsrc, bin_ptr, bin_idx,
                                               dst_crs, dst_grid, H, W, rule, fill, (T*)dst, src_id);
}

}  // namespace

extern "C" int ig_warp_coords(const double* dst_crs, const double* dst_grid, int H, int W, const double* src_crs, const double* src_grid,
                              double* uv, void* stream) {
    IG_REQUIRE(H >= 0 && W >= 0, "ig_warp_coords: need H >= 0 and W >= 0 (H %d, W %d)", H, W);
    IG_REQUIRE((long)H * W <= 0x7fffffffL, "ig_warp_coords: H * W = %ld exceeds 2^31 - 1", (long)H * W);
    if ((long)H * W == 0) return IG_OK;
    IG_REQUIRE(ig_cdiv(H, 4) <= 65535, "ig_warp_coords: H = %d exceeds 65535 workgroups of 4 rows", H);
    IG_REQUIRE(dst_crs && dst_grid && src_crs && src_grid && uv, "ig_warp_coords: null pointer");
    IG_REQUIRE((((uintptr_t)dst_crs | (uintptr_t)dst_grid | (uintptr_t)src_crs | (uintptr_t)src_grid | (uintptr_t)uv) & 7) == 0,
               "ig_warp_coords: the float64 arrays must be 8-byte aligned");
    return ig_launch<coords_kernel>("ig_warp_coords", dim3((unsigned)ig_cdiv(W, WB), (unsigned)ig_cdiv(H, 4)), dim3(WTPB), 0, (hipStream_t)stream,
                                    dst_crs, dst_grid, H, W, src_crs, src_grid, uv);
}

extern "C" int ig_warp(const void* src, const long long* starts, const double* src_crs, const double* src_grid, const int* src_size, int nsrc,
                       const int* bin_ptr, const int* bin_idx, const double* dst_crs, const double* dst_grid, int H, int W, int elem_size,
                       int resampling, int rule, int fill, void* dst, unsigned char* src_id, void* stream) {
    IG_REQUIRE(elem_size == 1 || elem_size == 4, "ig_warp: elem_size must be 1 (int8) or 4 (float32) (got %d)", elem_size);
    IG_REQUIRE(resampling == 0 || resampling == 1, "ig_warp: resampling must be 0 nearest or 1 bilinear (got %d)", resampling);
    IG_REQUIRE(resampling == 0 || elem_size == 4, "ig_warp: bilinear resampling needs float32 rasters (elem_size %d)", elem_size);
    IG_REQUIRE(rule == R_LAST || rule == R_FIRST, "ig_warp: rule must be 0 last or 1 first (got %d)", rule);
    IG_REQUIRE(fill >= -128 && fill <= 127, "ig_warp: fill must fit int8 (got %d)", fill);
    IG_REQUIRE(H >= 0 && W >= 0, "ig_warp: need H >= 0 and W >= 0 (H %d, W %d)", H, W);
    IG_REQUIRE((long)H * W <= 0x7fffffffL, "ig_warp: H * W = %ld exceeds 2^31 - 1", (long)H * W);
    IG_REQUIRE(nsrc >= 0 && nsrc <= WMAX, "ig_warp: need 0 <= nsrc <= %d (got %d)", WMAX, nsrc);
    if ((long)H * W == 0) return IG_OK;
    IG_REQUIRE(ig_cdiv(H, WB) <= 65535, "ig_warp: H = %d exceeds 65535 blocks of 64 rows", H);
    IG_REQUIRE(dst && dst_crs && dst_grid, "ig_warp: null pointer (dst, dst_crs or dst_grid)");
    IG_REQUIRE(((uintptr_t)dst & (elem_size - 1)) == 0, "ig_warp: dst must be aligned to its elements");
    IG_REQUIRE((((uintptr_t)dst_crs | (uintptr_t)dst_grid) & 7) == 0, "ig_warp: the float64 arrays must be 8-byte aligned");
    if (nsrc > 0) {
        IG_REQUIRE(src && starts && src_crs && src_grid && src_size && bin_ptr && bin_idx, "ig_warp: null pointer");
        IG_REQUIRE(((uintptr_t)src & (elem_size - 1)) == 0, "ig_warp: src must be aligned to its elements");
        IG_REQUIRE((((uintptr_t)src_crs | (uintptr_t)src_grid | (uintptr_t)starts) & 7) == 0 &&
                       (((uintptr_t)src_size | (uintptr_t)bin_ptr | (uintptr_t)bin_idx) & 3) == 0,
                   "ig_warp: the float64 arrays and starts must be 8-byte, src_size, bin_ptr and bin_idx 4-byte aligned");
    } else {
        bin_ptr = nullptr;  // every block's list is empty: the destination becomes fill
    }
#define WARP(T, B) \
    return launch<T, B>(src, starts, src_crs, src_grid, src_size, nsrc, bin_ptr, bin_idx, dst_crs, dst_grid, H, W, rule, fill, dst, src_id, stream)
    if (elem_size == 1) WARP(signed char, false);
    if (resampling == 0) WARP(float, false);
    WARP(float, true);
#undef WARP
}
