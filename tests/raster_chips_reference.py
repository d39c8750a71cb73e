"""A sequential twin of the warped chip cut (include/instageo_hip.h) for the tests, and the cases both test files share.
It does not import the product: the coordinates come from tests/warp_reference.py (the independent float64 projection twin), masking,
clip, validity, labels and tallies are plain loops over pixels.

TIES.  The device and this twin may differ by ~1e-10 px in (u, v), so a pixel whose u or v lies within 1e-6 of an integer could pick
another source pixel.  ``cut`` counts those pixels (``near``); every case below chooses its grids (sub-pixel offsets) so that the count
is zero, the tests assert that from the twin alone, and every comparison is then exact."""
import functools

import numpy as np

import chips_reference as CR
import warp_reference as WR

U36, U37, U36S = WR.utm(36), WR.utm(37), WR.utm(36, south=True)
H, W, PX = 100, 90, 30.0
BITS = 2 | 4 | 8 | 32


def lattice(system, lon, lat):
    """The point (lon, lat) in ``system`` on a 30 m lattice."""
    return tuple(30.0 * round(float(v) / 30.0) for v in WR.from_lonlat(system, lon, lat))


X0, Y0 = lattice(U36, 34.0, 40.6)
SRC_GRID = (X0, Y0, PX, PX)
X0S, Y0S = lattice(U36S, 34.0, -40.6)


def grid_ok(g):
    return bool(np.isfinite(g).all() and g[2] > 0 and g[3] > 0)


def cut(tile, fmask, src_crs, src_grid, dst_crs, dst_grids, S, T, bits, strategy, nd, clip, labels=None, bit=0, K=0):
    """-> (chips, valid_values, validity, maps, valid_labels, hist, near): pixel by pixel.  ``near``: the pixels with u or v within 1e-6
    of an integer."""
    TC, h, w = tile.shape
    C = TC // T
    n = len(dst_grids)
    chips = np.zeros((n, TC, S, S), dtype=np.int16)
    validity = np.zeros((n, S, S), dtype=np.uint8)
    valid_values = np.zeros(n, dtype=np.int32)
    maps = valid_labels = hist = None
    if labels is not None:
        maps, valid_labels = np.zeros_like(labels), np.zeros(n, dtype=np.int32)
        hist = np.zeros((n, K), dtype=np.int32) if K else None
    near = 0
    for i, g in enumerate(dst_grids):
        if grid_ok(np.asarray(g, dtype=np.float64)) and grid_ok(np.asarray(src_grid, dtype=np.float64)):
            u, v = WR.coords(tuple(dst_crs), g, (S, S), tuple(src_crs), src_grid)
        else:
            u = v = np.full((S, S), np.nan)
        with np.errstate(invalid="ignore"):
            near += int(((np.abs(u - np.round(u)) < 1e-6) | (np.abs(v - np.round(v)) < 1e-6)).sum())
        for r in range(S):
            for c in range(S):
                uu, vv = u[r, c], v[r, c]
                values, flags = [nd] * TC, [0] * T
                if uu == uu and vv == vv:
                    cs, rs = int(np.floor(uu)), int(np.floor(vv))
                    if 0 <= rs < h and 0 <= cs < w:
                        values = [int(x) for x in tile[:, rs, cs]]
                        if fmask is not None:
                            flags = [int(x) for x in fmask[:, rs, cs]]
                masked = [(f & bits) != 0 for f in flags]
                if strategy == "any":
                    masked = [any(masked)] * T
                differ = 0
                for b in range(TC):
                    x = nd if masked[b // C] else values[b]
                    if clip is not None:
                        x = min(max(x, clip[0]), clip[1])
                    chips[i, b, r, c] = x
                    differ += x != nd
                valid_values[i] += differ
                validity[i, r, c] = (1 if differ == TC else 0) | (2 if differ > 0 else 0)
                if labels is not None:
                    x = labels[i, r, c]
                    if (bit and not (validity[i, r, c] & bit)) or x != x:
                        x = labels.dtype.type(-1)
                    maps[i, r, c] = x
                    if x != -1:
                        valid_labels[i] += 1
                        if K and 0 <= int(x) < K:
                            hist[i, int(x)] += 1
    return chips, valid_values, validity, maps, valid_labels, hist, near


@functools.lru_cache(maxsize=None)
def tile_of(T, C):
    return CR.make_tile(T, C, H, W, seed=10 * T + C, fully_masked=(40, 30), untouched=(5, 50), S=20)


def at(r0, c0, step=PX, dx=0.0, dy=0.0):
    """The grid of pixel size ``step`` whose top-left corner lies at pixel (r0, c0) of the tile, moved by (dx, dy) metres."""
    return (X0 + PX * c0 + dx, Y0 - PX * r0 + dy, step, step)


def _geographic(r0, c0, res=0.00027, system=U36, x0=X0, y0=Y0, dx=1.3e-5, dy=-0.7e-5):
    lon, lat = WR.to_lonlat(system, x0 + PX * c0, y0 - PX * r0)
    return (float(lon) + dx, float(lat) + dy, res, res)


def _projected(system, r0, c0, step, dx, dy):
    x, y = WR.from_lonlat(system, *WR.to_lonlat(U36, X0 + PX * c0, Y0 - PX * r0))
    return (float(x) + dx, float(y) + dy, step, step)


# name -> (src_crs, src_grid, dst_crs, dst_grids, S)
GEOMETRY = {
    # chips that hang over each edge of the tile, and one wholly outside it
    "edges_s32": (U36, SRC_GRID, U36, [at(-10, -7), at(80, 70), at(-5, 70), at(50, -20), at(30, 20), at(200, 200)], 32),
    "edges_s65": (U36, SRC_GRID, U36, [at(-20, 40), at(50, -30)], 65),
    "whole_s128": (U36, SRC_GRID, U36, [at(-10, -15)], 128),
    # one coordinate system, other pixel sizes: 10 m (every source pixel 3 x 3 times), 60 m (every second pixel), a 3.3 m shift
    "fine_10m_s128": (U36, SRC_GRID, U36, [at(20, 30, 10.0)], 128),
    "coarse_60m_s65": (U36, SRC_GRID, U36, [at(-5, -8, 60.0, 7.0, -11.0)], 65),
    "shift_3m3_s32": (U36, SRC_GRID, U36, [at(10, 12, PX, 3.3, -3.3), at(60, 70, PX, 3.3, 3.3)], 32),
    # other coordinate systems
    "geographic_s65": (U36, SRC_GRID, WR.GEOGRAPHIC, [_geographic(5, 4), _geographic(60, 50)], 65),
    "web_mercator_s32": (U36, SRC_GRID, WR.WEB_MERCATOR, [_projected(WR.WEB_MERCATOR, 8, 9, 39.7, 1.9, -2.3),
                                                         _projected(WR.WEB_MERCATOR, 70, 60, 39.7, 0.7, 1.1)], 32),
    "next_zone_s65": (U36, SRC_GRID, U37, [_projected(U37, 12, 3, 30.0, 4.1, -6.3)], 65),
    "south_s32": (U36S, (X0S, Y0S, PX, PX), WR.GEOGRAPHIC, [_geographic(20, 15, system=U36S, x0=X0S, y0=Y0S)], 32),
}
# (T, C, strategy, with an Fmask, clip, no_data)
SETTINGS = [(3, 2, "each", True, None, 0), (3, 2, "any", True, (0, 10000), 0), (1, 1, "each", False, (100, 5000), -9999),
            (3, 2, "each", True, None, -9999)]
PAIRS = [(g, k) for g in GEOMETRY for k in range(len(SETTINGS)) if k < 2 or g in ("edges_s32", "geographic_s65", "coarse_60m_s65")]


@functools.lru_cache(maxsize=None)
def twin(geometry, setting):
    """The twin's outputs for one geometry under one of SETTINGS, computed once per session."""
    sc, sg, dc, dg, S = GEOMETRY[geometry]
    T, C, strategy, with_mask, clip, nd = SETTINGS[setting]
    tile, fmask = tile_of(T, C)
    return cut(tile, fmask if with_mask else None, sc, sg, dc, dg, S, T, BITS, strategy, nd, clip)


def label_maps(n, S, dtype, seed):
    """Random label maps: int8 with values below and above K = 8 and -1; float32 the same + 0.25, with NaNs and -1."""
    rng = np.random.default_rng(seed)
    values = np.array([-1, 0, 1, 2, 3, 7, 8, 100], dtype=np.int8)
    lab = values[rng.integers(0, len(values), size=(n, S, S))]
    if dtype == np.int8:
        return lab
    out = lab.astype(np.float32) + np.float32(0.25)
    out[lab == -1] = -1.0
    out[rng.random(out.shape) < 0.05] = np.nan
    return out
