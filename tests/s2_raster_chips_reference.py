"""A sequential twin of the warped Sentinel-2 chip cut (include/instageo_hip.h: ig_s2_chip_warp) for the tests, and the
cases both test files share.  It does not import the product: the coordinates come from tests/warp_reference.py (the independent float64
projection twin), the per-class source pixel, the value chain, validity, labels and tallies are plain loops over pixels.

TIES.  The device and this twin may differ by ~1e-10 px in a coordinate, so a pixel whose u or v, in any class it reads, lies within 1e-6
of an integer could pick another source pixel.  ``cut`` counts those pixels (``ties``); every case below chooses its grids (sub-pixel
shifts) so that the count is zero, the tests assert that from the twin alone, and every comparison is then exact."""
import functools

import numpy as np

import raster_chips_reference as RR
import s2_chips_reference as SR
import warp_reference as WR

U36, U37, U36S = RR.U36, RR.U37, RR.U36S
X0, Y0, X0S, Y0S = RR.X0, RR.Y0, RR.X0S, RR.Y0S
SIZES = ((120, 110), (60, 55), (20, 19))  # the 10 m, 20 m and 60 m planes
STEPS = (10.0, 20.0, 60.0)
CLASS_BITS = SR.CLASS_BITS  # class 0 too: the fill outside a plane is masked
IDENTITY = (0.0, 0.0, 1.0, 1.0)


def class_grids(x0=X0, y0=Y0):
    return [(x0, y0, p, p) for p in STEPS]


def grid_ok(g):
    g = np.asarray(g, dtype=np.float64)
    return bool(np.isfinite(g).all() and g[2] > 0 and g[3] > 0)


def cut(planes, scl_planes, grids, src_crs, dst_crs, dst_grids, S, T, class_bits, strategy, nd=0, boa=0, valid_range=None, labels=None, bit=0,
        K=0):
    """planes: T * C (array (H, W) uint16, class index); scl_planes: T (array (H, W) uint8, class index) or None; grids: the (X0, Y0, sx, sy)
    of every class.  -> (chips, valid_values, validity, maps, valid_labels, hist, ties): pixel by pixel."""
    TC = len(planes)
    C = TC // T
    n = len(dst_grids)
    chips = np.zeros((n, TC, S, S), dtype=np.uint16)
    validity = np.zeros((n, S, S), dtype=np.uint8)
    valid_values = np.zeros(n, dtype=np.int32)
    maps = valid_labels = hist = None
    if labels is not None:
        maps, valid_labels = np.zeros_like(labels), np.zeros(n, dtype=np.int32)
        hist = np.zeros((n, K), dtype=np.int32) if K else None
    used = sorted({g for _, g in planes} | ({g for _, g in scl_planes} if scl_planes is not None else set()))
    usable = all(grid_ok(g) for g in grids)
    ties = 0

    def read(a, g, where):
        rc = where[g]
        return None if rc is None else int(a[rc])

    for i, dg in enumerate(dst_grids):
        if usable and grid_ok(dg):
            x, my = WR.coords(tuple(dst_crs), dg, (S, S), tuple(src_crs), IDENTITY)  # (x, -y) of the source system
        else:
            x = my = np.full((S, S), np.nan)
        for r in range(S):
            for c in range(S):
                where = {}
                for g in used:
                    gx0, gy0, sx, sy = grids[g]
                    u, v = (x[r, c] - gx0) / sx, (gy0 - -my[r, c]) / sy
                    where[g] = None
                    if u == u and v == v:
                        ties += abs(u - round(u)) < 1e-6 or abs(v - round(v)) < 1e-6
                        cs, rs = int(np.floor(u)), int(np.floor(v))
                        h, w = next(a.shape for a, k in list(planes) + list(scl_planes or []) if k == g)
                        if 0 <= rs < h and 0 <= cs < w:
                            where[g] = (rs, cs)
                masked = [False] * T
                if scl_planes is not None:
                    for t, (a, g) in enumerate(scl_planes):
                        k = read(a, g, where) or 0
                        masked[t] = k < 32 and ((class_bits >> k) & 1) == 1
                anyone = any(masked)
                differ = 0
                for b, (a, g) in enumerate(planes):
                    v = read(a, g, where)
                    if v is None:
                        v = nd
                    else:
                        if boa > 0 and v != 0:
                            v = max(v - boa, 0)
                        if (strategy == "each" and masked[b // C]) or (strategy == "any" and anyone):
                            v = nd
                        if valid_range is not None and not (valid_range[0] <= v <= valid_range[1]):
                            v = nd
                    chips[i, b, r, c] = v
                    differ += v != nd
                valid_values[i] += differ
                validity[i, r, c] = (1 if differ == TC else 0) | (2 if differ > 0 else 0)
                if labels is not None:
                    lab = labels[i, r, c]
                    if (bit and not (validity[i, r, c] & bit)) or lab != lab:
                        lab = labels.dtype.type(-1)
                    maps[i, r, c] = lab
                    if lab != -1:
                        valid_labels[i] += 1
                        if K and 0 <= int(lab) < K:
                            hist[i, int(lab)] += 1
    return chips, valid_values, validity, maps, valid_labels, hist, int(ties)


# ---- planes ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planes_of(T):
    """T dates of three bands (10 m, 20 m, 60 m: classes 0, 1, 2) and a 20 m SCL plane per date."""
    planes = [(SR.band_plane(*SIZES[c], seed=31 * t + c), c) for t in range(T) for c in range(3)]
    scls = [(SR.scl_plane(*SIZES[1], seed=500 + t), 1) for t in range(T)]
    return planes, scls


def pack(planes, dtype, lead=0):
    """-> (buffer with ``lead`` unused elements in front, starts int64, class index per plane)."""
    starts, at = [], lead
    for a, _ in planes:
        starts.append(at)
        at += a.size
    buf = np.zeros(at, dtype=dtype)
    for (a, _), s in zip(planes, starts):
        buf[s : s + a.size] = a.reshape(-1)
    return buf, np.array(starts, dtype=np.int64), [g for _, g in planes]


def sizes_array():
    return np.array(SIZES, dtype=np.int32)


# ---- geometries ------------------------------------------------------------------------------------------------------------------------------
def at(r0, c0, step=10.0, dx=3.3, dy=-2.7, x0=X0, y0=Y0):
    """The grid of pixel size ``step`` whose top-left corner lies at pixel (r0, c0) of the 10 m plane, moved by (dx, dy) metres."""
    return (x0 + 10.0 * c0 + dx, y0 - 10.0 * r0 + dy, step, step)


def _geographic(r0, c0, res, system=U36, x0=X0, y0=Y0, dx=1.3e-6, dy=-0.7e-6):
    lon, lat = WR.to_lonlat(system, x0 + 10.0 * c0, y0 - 10.0 * r0)
    return (float(lon) + dx, float(lat) + dy, res, res)


def _projected(system, r0, c0, step, dx, dy):
    x, y = WR.from_lonlat(system, *WR.to_lonlat(U36, X0 + 10.0 * c0, Y0 - 10.0 * r0))
    return (float(x) + dx, float(y) + dy, step, step)


FAR = at(4000, 4000)  # wholly outside every plane
# name -> (src_crs, the corner of the planes, dst_crs, dst_grids, S).  Every set has a chip over each edge of the tile and one outside it.
GEOMETRY = {
    "same_10m_s32": (U36, (X0, Y0), U36, [at(-10, -7), at(100, 90), at(-5, 90), at(100, -20), at(40, 30), FAR], 32),
    "same_20m_s65": (U36, (X0, Y0), U36, [at(-3, -4, 20.0), at(30, 35, 20.0), FAR], 65),
    "same_60m_s32": (U36, (X0, Y0), U36, [at(-30, -40, 60.0, 7.0, -11.0), at(20, 10, 60.0, 7.0, -11.0), FAR], 32),
    "next_zone_s65": (U36, (X0, Y0), U37, [_projected(U37, -8, -5, 10.0, 4.1, -6.3), _projected(U37, 70, 60, 10.0, 4.1, -6.3), FAR], 65),
    "south_s32": (U36S, (X0S, Y0S), WR.GEOGRAPHIC, [_geographic(-6, -9, 0.00011, U36S, X0S, Y0S), _geographic(100, 95, 0.00011, U36S, X0S, Y0S),
                                                    _geographic(50, 40, 0.00011, U36S, X0S, Y0S), (10.0, 10.0, 0.00011, 0.00011)], 32),
    "geographic_s65": (U36, (X0, Y0), WR.GEOGRAPHIC, [_geographic(-9, -12, 0.000131), _geographic(80, 75, 0.000131), (10.0, 10.0, 0.000131, 0.000131)], 65),
    "web_mercator_s32": (U36, (X0, Y0), WR.WEB_MERCATOR, [_projected(WR.WEB_MERCATOR, -4, -6, 13.1, 1.9, -2.3),
                                                         _projected(WR.WEB_MERCATOR, 105, 95, 13.1, 0.7, 1.1),
                                                         _projected(WR.WEB_MERCATOR, 30, 40, 13.1, 0.7, 1.1), (0.0, 0.0, 13.1, 13.1)], 32),
}
# (T, strategy, with SCL planes, boa_offset, valid_range, no_data)
SETTINGS = [(3, "each", True, 0, None, 0), (3, "any", True, 1000, (0, 10000), 0), (1, "each", False, 1000, None, 7),
            (1, "any", True, 0, (0, 10000), 65535)]
PAIRS = [(g, k) for g in GEOMETRY for k in range(len(SETTINGS)) if k < 2 or g in ("same_10m_s32", "geographic_s65")]


@functools.lru_cache(maxsize=None)
def twin(geometry, setting):
    """The twin's outputs for one geometry under one of SETTINGS, computed once per session."""
    sc, corner, dc, dg, S = GEOMETRY[geometry]
    T, strategy, with_scl, boa, rng, nd = SETTINGS[setting]
    planes, scls = planes_of(T)
    return cut(planes, scls if with_scl else None, class_grids(*corner), sc, dc, dg, S, T, CLASS_BITS, strategy, nd, boa, rng)


def run_args(geometry, setting, xp=lambda a: a, lead=0):
    """The positional and keyword arguments of ``s2_raster_chips.warp_cut`` for one geometry under one of SETTINGS."""
    sc, corner, dc, dg, S = GEOMETRY[geometry]
    T, strategy, with_scl, boa, rng, nd = SETTINGS[setting]
    planes, scls = planes_of(T)
    bands, starts, pc = pack(planes, np.uint16, lead)
    scl, scl_starts, spc = pack(scls, np.uint8, lead) if with_scl else (None, None, [])
    args = (xp(bands), starts, pc + spc, class_grids(*corner), sizes_array(), None if scl is None else xp(scl), scl_starts, sc, dc, dg, S)
    return args, dict(dates=T, class_bits=CLASS_BITS, strategy=strategy, no_data_value=nd, boa_offset=boa, valid_range=rng)
