// The float64 projection code shared by the kernels that map a destination pixel into a source grid (warp.hip, maptiles.hip,
// raster_chips.hip, s2_raster_chips.hip, s1_chips.hip): WGS84 constants, Krueger's series for transverse Mercator, the coordinate-system
// and grid descriptions and their chain, as the rule of include/instageo_hip.h states them.  All of them include this text, so all
// evaluate the same arithmetic.
#pragma once
#include "common.h"

namespace {

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

}  // namespace
