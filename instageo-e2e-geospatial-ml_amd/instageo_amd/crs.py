"""Coordinate systems of the warp: the GeoKeys of a GeoTIFF profile -> the five doubles of ``include/instageo_hip.h``, and
the projections themselves in numpy float64: the host path of :mod:`instageo_amd.warp` and its extent computation.

A coordinate system is ``(kind, lon0, k0, FE, FN)``: kind 0 geographic WGS84 in degrees (EPSG:4326), 1 transverse Mercator on WGS84 (the
UTM zones EPSG:32601-32660 north and 32701-32760 south), 2 spherical web Mercator (EPSG:3857).  Transverse Mercator is Krueger's series to
n^6 (Karney 2011), summed by Clenshaw's recurrence; the latitude comes back from the conformal one by three Newton steps.

Not done: other datums, polar stereographic, anything that needs the GeoKey parameter tags 34736 / 34737.
"""
from __future__ import annotations

from typing import Any, Dict, NamedTuple, Tuple

import numpy as np

GEOGRAPHIC, TRANSVERSE_MERCATOR, WEB_MERCATOR = 0, 1, 2
A = 6378137.0
F = 1.0 / 298.257223563
E2 = F * (2.0 - F)
E = float(np.sqrt(E2))
N = F / (2.0 - F)
RECT = A / (1.0 + N) * (1.0 + N**2 / 4.0 + N**4 / 64.0 + N**6 / 256.0)  # the rectifying radius
LAT_MAX = 89.9  # degrees: beyond, a point is outside the domain
DLON_MAX = 80.0  # degrees from the central meridian of a transverse Mercator system, likewise


def _poly(*rows):
    """rows[j] = the coefficients of n^(j+1), n^(j+2), ... of the j-th series coefficient."""
    return np.array([sum(c * N ** (j + 1 + k) for k, c in enumerate(row)) for j, row in enumerate(rows)])


ALPHA = _poly((1 / 2, -2 / 3, 5 / 16, 41 / 180, -127 / 288, 7891 / 37800),
              (13 / 48, -3 / 5, 557 / 1440, 281 / 630, -1983433 / 1935360),
              (61 / 240, -103 / 140, 15061 / 26880, 167603 / 181440),
              (49561 / 161280, -179 / 168, 6601661 / 7257600),
              (34729 / 80640, -3418889 / 1995840),
              (212378941 / 319334400,))  # fmt: skip
BETA = _poly((1 / 2, -2 / 3, 37 / 96, -1 / 360, -81 / 512, 96199 / 604800),
             (1 / 48, 1 / 15, -437 / 1440, 46 / 105, -1118711 / 3870720),
             (17 / 480, -37 / 840, -209 / 4480, 5569 / 90720),
             (4397 / 161280, -11 / 504, -830251 / 7257600),
             (4583 / 161280, -108847 / 3991680),
             (20648693 / 638668800,))  # fmt: skip


class Crs(NamedTuple):
    """The five doubles of a coordinate system and its EPSG code."""
    kind: float
    lon0: float
    k0: float
    fe: float
    fn: float
    epsg: int

    @property
    def params(self) -> Tuple[float, float, float, float, float]:
        return tuple(float(x) for x in self[:5])

    @property
    def unit(self) -> str:
        return "degree" if self.kind == GEOGRAPHIC else "metre"


def from_epsg(epsg: int) -> Crs:
    """EPSG 32601-32660, 32701-32760, 3857 or 4326 -> :class:`Crs`; anything else raises a ValueError that names the code."""
    if isinstance(epsg, bool) or not isinstance(epsg, (int, np.integer)):
        raise ValueError(f"an EPSG code is an int (got {epsg!r})")
    epsg = int(epsg)
    if epsg == 4326:
        return Crs(GEOGRAPHIC, 0.0, 0.0, 0.0, 0.0, epsg)
    if epsg == 3857:
        return Crs(WEB_MERCATOR, 0.0, 0.0, 0.0, 0.0, epsg)
    if 32601 <= epsg <= 32660 or 32701 <= epsg <= 32760:
        zone = epsg % 100
        return Crs(TRANSVERSE_MERCATOR, 6.0 * zone - 183.0, 0.9996, 500000.0, 1e7 if epsg >= 32700 else 0.0, epsg)
    raise ValueError(f"EPSG:{epsg} is not a coordinate system the warp knows (EPSG:32601-32660, 32701-32760, 3857, 4326)")


def parse(text: str) -> Crs:
    """``"EPSG:32636"`` -> :class:`Crs`."""
    s = str(text).strip()
    if not s.upper().startswith("EPSG:") or not s[5:].isdigit():
        raise ValueError(f"a coordinate system is written EPSG:<code> (got {text!r})")
    return from_epsg(int(s[5:]))


def from_profile(profile: Dict[str, Any]) -> Crs:
    """The coordinate system of a GeoTIFF profile (:func:`tiff.read`) from its GeoKey directory, tag 34735: GTModelTypeGeoKey 1024
    (1 projected, 2 geographic), GeographicTypeGeoKey 2048 and ProjectedCSTypeGeoKey 3072."""
    entry = ((profile or {}).get("tags") or {}).get(34735)
    if entry is None:
        raise ValueError("no GeoKey directory (tag 34735): the raster has no coordinate system")
    keys = [int(x) for x in entry[1]]
    if len(keys) < 4 or len(keys) < 4 * (keys[3] + 1):
        raise ValueError("a GeoKey directory shorter than its header says")
    found = {}
    for k in range(1, keys[3] + 1):
        key, loc, _, value = keys[4 * k : 4 * k + 4]
        if key in (1024, 2048, 3072):
            if loc != 0:
                raise ValueError(f"GeoKey {key} is stored in another tag: the coordinate system is not an EPSG code")
            found[key] = value
    model = found.get(1024)
    if model == 1 or (model is None and 3072 in found):
        if 3072 not in found:
            raise ValueError("a projected raster without a ProjectedCSTypeGeoKey (3072)")
        return from_epsg(found[3072])
    if model == 2 or (model is None and 2048 in found):
        if 2048 not in found:
            raise ValueError("a geographic raster without a GeographicTypeGeoKey (2048)")
        return from_epsg(found[2048])
    raise ValueError(f"GTModelTypeGeoKey {model!r}: neither a projected nor a geographic coordinate system")


def geokeys(epsg: int) -> Dict[int, Tuple[int, Tuple[int, ...]]]:
    """The tags to write for ``epsg``: {34735: (SHORT, the GeoKey directory)}.  Tags 34736 / 34737 of a source do not apply to it and are
    dropped by the caller."""
    crs = from_epsg(epsg)
    if crs.kind == GEOGRAPHIC:
        keys = (1, 1, 0, 3, 1024, 0, 1, 2, 1025, 0, 1, 1, 2048, 0, 1, crs.epsg)
    else:
        keys = (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, crs.epsg)
    return {34735: (3, keys)}


# ---- the projections ---------------------------------------------------------------------------------------------------------------------
def _clenshaw(coef: np.ndarray, xi: np.ndarray, eta: np.ndarray):
    """sum_j coef[j-1] sin(2j (xi + i eta)) -> (real, imaginary) by Clenshaw's recurrence on the complex argument."""
    z = 2.0 * (xi + 1j * eta)
    two_cos = 2.0 * np.cos(z)
    b1 = np.zeros_like(z)
    b2 = np.zeros_like(z)
    for c in coef[::-1]:
        b1, b2 = c + two_cos * b1 - b2, b1
    s = b1 * np.sin(z)
    return s.real, s.imag


def _taup(tau):
    t1 = np.sqrt(1.0 + tau * tau)
    sig = np.sinh(E * np.arctanh(E * tau / t1))
    return tau * np.sqrt(1.0 + sig * sig) - sig * t1


def inverse(crs, x, y):
    """(x, y) of ``crs`` -> (longitude, latitude) in degrees, float64 arrays; NaN outside the domain (not finite, |latitude| > 89.9, a
    transverse Mercator point beyond the pole)."""
    kind, lon0, k0, fe, fn = (float(v) for v in tuple(crs)[:5])
    x, y = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
    with np.errstate(all="ignore"):
        if kind == GEOGRAPHIC:
            lon, lat = x.copy(), y.copy()
        elif kind == WEB_MERCATOR:
            lon, lat = np.degrees(x / A), np.degrees(np.arctan(np.sinh(y / A)))
        else:
            ka = k0 * RECT
            xi, eta = (y - fn) / ka, (x - fe) / ka
            dx, de = _clenshaw(BETA, xi, eta)
            xip, etap = xi - dx, eta - de
            sh = np.sinh(etap)
            cx = np.cos(xip)
            tp = np.sin(xip) / np.sqrt(sh * sh + cx * cx)
            tau = tp / (1.0 - E2)
            for _ in range(3):
                tpi = _taup(tau)
                tau = tau + (tp - tpi) / np.sqrt(1.0 + tpi * tpi) * (1.0 + (1.0 - E2) * tau * tau) / ((1.0 - E2) * np.sqrt(1.0 + tau * tau))
            lon, lat = lon0 + np.degrees(np.arctan2(sh, cx)), np.degrees(np.arctan(tau))
            lat = np.where(np.abs(xip) <= np.pi / 2, lat, np.nan)
        bad = ~(np.isfinite(lon) & np.isfinite(lat) & (np.abs(lat) <= LAT_MAX))
    return np.where(bad, np.nan, lon), np.where(bad, np.nan, lat)


def forward(crs, lon, lat):
    """(longitude, latitude) in degrees -> (x, y) of ``crs``, float64 arrays; NaN outside the domain (not finite, |latitude| > 89.9, 80
    degrees or more from the central meridian of a transverse Mercator system)."""
    kind, lon0, k0, fe, fn = (float(v) for v in tuple(crs)[:5])
    lon, lat = np.broadcast_arrays(np.asarray(lon, dtype=np.float64), np.asarray(lat, dtype=np.float64))
    with np.errstate(all="ignore"):
        bad = ~(np.isfinite(lon) & np.isfinite(lat) & (np.abs(lat) <= LAT_MAX))
        if kind == GEOGRAPHIC:
            x, y = lon.copy(), lat.copy()
        elif kind == WEB_MERCATOR:
            x, y = A * np.radians(lon), A * np.arcsinh(np.tan(np.radians(lat)))
        else:
            dl = np.remainder(lon - lon0 + 180.0, 360.0) - 180.0
            bad |= ~(np.abs(dl) < DLON_MAX)
            tp = _taup(np.tan(np.radians(lat)))
            lam = np.radians(dl)
            cl = np.cos(lam)
            xip, etap = np.arctan2(tp, cl), np.arcsinh(np.sin(lam) / np.sqrt(tp * tp + cl * cl))
            dx, de = _clenshaw(ALPHA, xip, etap)
            ka = k0 * RECT
            x, y = fe + ka * (etap + de), fn + ka * (xip + dx)
    return np.where(bad, np.nan, x), np.where(bad, np.nan, y)


def transform(dst_crs, src_crs, x, y):
    """(x, y) of ``dst_crs`` -> (x', y') of ``src_crs``; the identity where the five doubles are equal (no projection is evaluated)."""
    if tuple(float(v) for v in tuple(dst_crs)[:5]) == tuple(float(v) for v in tuple(src_crs)[:5]):
        x, y = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
        return x.copy(), y.copy()
    return forward(src_crs, *inverse(dst_crs, x, y))
