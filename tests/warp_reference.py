"""An independent twin of the warp (include/instageo_hip.h) for the tests.  It does not import the product.

Transverse Mercator here is Krueger's series written as complex arithmetic, term by term: zeta = zeta' + sum_j alpha_j sin(2j zeta') with
zeta' = xi' + i eta' from the conformal latitude, which comes from the isometric latitude psi = asinh(tan phi) - e atanh(e sin phi); the
way back finds phi from psi by the fixed-point iteration phi <- atan(sinh(psi + e atanh(e sin phi))) (contraction ratio e^2 = 0.0067, 12
steps).  Web Mercator uses the logarithmic forms.  The coefficients are exact fractions (Karney 2011, "Transverse Mercator with an accuracy
of a few nanometers", eqs. 35, 36).  The resampling is written pixel by pixel.
"""
from fractions import Fraction as Fr

import numpy as np

A = 6378137.0
F = 1 / 298.257223563
E = (F * (2 - F)) ** 0.5
N = F / (2 - F)
RECT = A / (1 + N) * (1 + N**2 / 4 + N**4 / 64 + N**6 / 256)
ALPHA_Q = [
    [Fr(1, 2), Fr(-2, 3), Fr(5, 16), Fr(41, 180), Fr(-127, 288), Fr(7891, 37800)],
    [Fr(13, 48), Fr(-3, 5), Fr(557, 1440), Fr(281, 630), Fr(-1983433, 1935360)],
    [Fr(61, 240), Fr(-103, 140), Fr(15061, 26880), Fr(167603, 181440)],
    [Fr(49561, 161280), Fr(-179, 168), Fr(6601661, 7257600)],
    [Fr(34729, 80640), Fr(-3418889, 1995840)],
    [Fr(212378941, 319334400)],
]
BETA_Q = [
    [Fr(1, 2), Fr(-2, 3), Fr(37, 96), Fr(-1, 360), Fr(-81, 512), Fr(96199, 604800)],
    [Fr(1, 48), Fr(1, 15), Fr(-437, 1440), Fr(46, 105), Fr(-1118711, 3870720)],
    [Fr(17, 480), Fr(-37, 840), Fr(-209, 4480), Fr(5569, 90720)],
    [Fr(4397, 161280), Fr(-11, 504), Fr(-830251, 7257600)],
    [Fr(4583, 161280), Fr(-108847, 3991680)],
    [Fr(20648693, 638668800)],
]
ALPHA = [sum(float(q) * N ** (j + 1 + k) for k, q in enumerate(row)) for j, row in enumerate(ALPHA_Q)]
BETA = [sum(float(q) * N ** (j + 1 + k) for k, q in enumerate(row)) for j, row in enumerate(BETA_Q)]
NAN32 = np.uint32(0x7FC00000).view(np.float32)


def utm(zone, south=False):
    return (1.0, 6.0 * zone - 183.0, 0.9996, 500000.0, 1e7 if south else 0.0)


GEOGRAPHIC = (0.0, 0.0, 0.0, 0.0, 0.0)
WEB_MERCATOR = (2.0, 0.0, 0.0, 0.0, 0.0)


def isometric(lat_deg):
    """psi of a geographic latitude in degrees."""
    phi = np.radians(np.asarray(lat_deg, dtype=np.float64))
    return np.arcsinh(np.tan(phi)) - E * np.arctanh(E * np.sin(phi))


def latitude_of_isometric(psi):
    phi = np.arctan(np.sinh(psi))
    for _ in range(12):
        phi = np.arctan(np.sinh(psi + E * np.arctanh(E * np.sin(phi))))
    return np.degrees(phi)


def tm_forward(lon0, k0, fe, fn, dlon_deg, lat_deg):
    psi, lam = isometric(lat_deg), np.radians(np.asarray(dlon_deg, dtype=np.float64))
    zp = np.arctan2(np.sinh(psi), np.cos(lam)) + 1j * np.arctanh(np.sin(lam) / np.cosh(psi))
    z = zp.copy()
    for j, a in enumerate(ALPHA, start=1):
        z = z + a * np.sin(2 * j * zp)
    return fe + k0 * RECT * z.imag, fn + k0 * RECT * z.real


def tm_inverse(lon0, k0, fe, fn, x, y):
    z = (np.asarray(y, dtype=np.float64) - fn) / (k0 * RECT) + 1j * (np.asarray(x, dtype=np.float64) - fe) / (k0 * RECT)
    zp = z.copy()
    for j, b in enumerate(BETA, start=1):
        zp = zp - b * np.sin(2 * j * z)
    xip, etap = zp.real, zp.imag
    lam = np.arctan2(np.sinh(etap), np.cos(xip))
    psi = np.arctanh(np.sin(xip) / np.cosh(etap))
    return lon0 + np.degrees(lam), latitude_of_isometric(psi), xip


def to_lonlat(crs, x, y):
    """-> (lon, lat) in degrees, NaN outside the domain of the header."""
    kind, lon0, k0, fe, fn = crs
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    with np.errstate(all="ignore"):
        if kind == 0:
            lon, lat = x + 0.0, y + 0.0
        elif kind == 2:
            lon, lat = np.degrees(x / A), np.degrees(2 * np.arctan(np.exp(y / A)) - np.pi / 2)
        else:
            lon, lat, xip = tm_inverse(lon0, k0, fe, fn, x, y)
            lat = np.where(np.abs(xip) <= np.pi / 2, lat, np.nan)
        bad = ~(np.isfinite(lon) & np.isfinite(lat) & (np.abs(lat) <= 89.9))
    return np.where(bad, np.nan, lon), np.where(bad, np.nan, lat)


def from_lonlat(crs, lon, lat):
    kind, lon0, k0, fe, fn = crs
    lon, lat = np.asarray(lon, dtype=np.float64), np.asarray(lat, dtype=np.float64)
    with np.errstate(all="ignore"):
        bad = ~(np.isfinite(lon) & np.isfinite(lat) & (np.abs(lat) <= 89.9))
        if kind == 0:
            x, y = lon + 0.0, lat + 0.0
        elif kind == 2:
            x, y = A * np.radians(lon), A * np.log(np.tan(np.pi / 4 + np.radians(lat) / 2))
        else:
            dl = np.fmod(lon - lon0, 360.0)
            dl = np.where(dl > 180, dl - 360, np.where(dl < -180, dl + 360, dl))
            bad |= ~(np.abs(dl) < 80.0)
            x, y = tm_forward(lon0, k0, fe, fn, np.where(bad, 0.0, dl), np.where(bad, 0.0, lat))
    return np.where(bad, np.nan, x), np.where(bad, np.nan, y)


def coords(dst_crs, dst_grid, shape, src_crs, src_grid):
    """(u, v) of the destination's pixel centres in the source grid."""
    H, W = shape
    X0, Y0, sx, sy = dst_grid
    x, y = np.meshgrid(X0 + (np.arange(W) + 0.5) * sx, Y0 - (np.arange(H) + 0.5) * sy)
    if tuple(dst_crs) != tuple(src_crs):
        x, y = from_lonlat(src_crs, *to_lonlat(dst_crs, x, y))
    u, v = (x - src_grid[0]) / src_grid[2], (src_grid[1] - y) / src_grid[3]
    bad = np.isnan(u) | np.isnan(v)
    return np.where(bad, np.nan, u), np.where(bad, np.nan, v)


def sample(a, u, v, resampling, fill):
    """One source at one point -> (value, contributes, the largest |neighbour| that counted), in plain Python."""
    h, w = a.shape
    if u != u or v != v:
        return None, False, 0.0
    if resampling == "nearest":
        c, r = int(np.floor(u)), int(np.floor(v))
        if not (0 <= r < h and 0 <= c < w):
            return None, False, 0.0
        x = a[r, c]
        clear = (x != x) if a.dtype == np.float32 else (x == fill)
        return x, not clear, 0.0
    fu, fv = u - 0.5, v - 0.5
    c0, r0 = int(np.floor(fu)), int(np.floor(fv))
    wx, wy = fu - c0, fv - r0
    acc = tot = big = 0.0
    for (dr, dc), wt in zip(((0, 0), (0, 1), (1, 0), (1, 1)), ((1 - wx) * (1 - wy), wx * (1 - wy), (1 - wx) * wy, wx * wy)):
        r, c = r0 + dr, c0 + dc
        if 0 <= r < h and 0 <= c < w and wt > 0 and a[r, c] == a[r, c]:
            acc, tot, big = acc + wt * float(a[r, c]), tot + wt, max(big, abs(float(a[r, c])))
    if not tot > 0:
        return None, False, 0.0
    return np.float32(acc / tot), True, big


def warp(arrays, systems, grids, dst_crs, dst_grid, shape, resampling="nearest", rule="last", fill=-1):
    """-> (raster, src_id uint8, ties bool, scale float64): ``ties`` marks the pixels where some source's u or v lies within 1e-6 of an
    integer (nearest) or of a half-integer (bilinear) -- there a rounding error of the coordinates may pick another pixel; ``scale`` is
    the largest |neighbour| behind a bilinear value."""
    H, W = shape
    dtype = arrays[0].dtype
    out = np.full((H, W), NAN32 if dtype == np.float32 else fill, dtype=dtype)
    sid = np.full((H, W), 255, dtype=np.uint8)
    ties = np.zeros((H, W), dtype=bool)
    scale = np.zeros((H, W))
    uvs = [coords(dst_crs, dst_grid, shape, s, g) for s, g in zip(systems, grids)]
    shift = 0.0 if resampling == "nearest" else 0.5
    for u, v in uvs:
        with np.errstate(invalid="ignore"):
            ties |= (np.abs(u - shift - np.round(u - shift)) < 1e-6) | (np.abs(v - shift - np.round(v - shift)) < 1e-6)
    order = list(range(len(arrays)))
    if rule == "last":
        order.reverse()
    for r in range(H):
        for c in range(W):
            for i in order:
                h, w = arrays[i].shape
                u, v = uvs[i][0][r, c], uvs[i][1][r, c]
                if not (-2 < u < w + 2 and -2 < v < h + 2):
                    continue
                x, ok, big = sample(arrays[i], u, v, resampling, fill)
                if ok:
                    out[r, c], sid[r, c], scale[r, c] = x, i, big
                    break
    return out, sid, ties, scale
