"""A sequential twin of the map-tile renderer (include/instageo_hip.h) for the tests, and the cases both test files
share.  It does not import the product: the coordinates come from tests/warp_reference.py (the independent float64 projection twin), the
pyramids from tests/overview_reference.py, sampling, colouring and the opaque counts are plain loops over pixels.

TIES.  The device, the product's host path and this twin may differ by ~1e-10 px in (u, v), so a pixel whose level-scaled u or v lies
within 1e-6 of an integer could pick another source pixel.  ``render`` counts those pixels; every case below offsets its source grid by a
few irrational-looking metres (or degrees) so that the count is zero, the tests assert that from the twin alone before anything is
compared, and every comparison is then exact equality on all bytes and all counts."""
import functools
import math

import numpy as np

import overview_reference as OR
import warp_reference as WR

WEBM = WR.WEB_MERCATOR
ORIGIN = math.pi * WR.A
H, W, NLEVELS = 100, 90, 3
NCOLORS, FILL = 5, -1
LO, HI = 0.0, 1.0
ORDER = (2, 1, 0)
U36, U36S = WR.utm(36), WR.utm(36, south=True)


def grid_ok(g):
    g = np.asarray(g, dtype=np.float64)
    return bool(np.isfinite(g).all() and g[2] > 0 and g[3] > 0)


def scaled_coords(src_crs, src_grid, grid, tile, level):
    """(u, v) / 2^level of the pixel centres of one tile, and the number of ties."""
    u, v = WR.coords(WEBM, grid, (tile, tile), tuple(src_crs), src_grid)
    u, v = u / float(1 << level), v / float(1 << level)
    with np.errstate(invalid="ignore"):
        ties = int(((np.abs(u - np.round(u)) < 1e-6) | (np.abs(v - np.round(v)) < 1e-6)).sum())
    return u, v, ties


def ramp_index(value, lo, hi):
    t = (float(np.float64(value)) - lo) / (hi - lo)
    t = 0.0 if t < 0.0 else 1.0 if t > 1.0 else t
    return int(np.rint(t * 255.0))


def render(levels, src_crs, src_grid, grids, lvls, tile, style, lut=None, ncolors=0, fill=-1, lo=0.0, hi=1.0, order=(0, 1, 2)):
    """-> (rgba (n, tile, tile, 4) uint8, opaque (n,) int32, ties): pixel by pixel."""
    n = len(grids)
    rgba = np.zeros((n, tile, tile, 4), dtype=np.uint8)
    opaque = np.zeros(n, dtype=np.int32)
    ties = 0
    for i, (g, k) in enumerate(zip(grids, lvls)):
        if not (0 <= k < len(levels)) or not grid_ok(g) or not grid_ok(src_grid):
            continue
        lv = levels[k] if levels[k].ndim == 3 else levels[k][None]
        hk, wk = lv.shape[-2:]
        u, v, near = scaled_coords(src_crs, src_grid, g, tile, k)
        ties += near
        for r in range(tile):
            for c in range(tile):
                uu, vv = u[r, c], v[r, c]
                if uu != uu or vv != vv:
                    continue
                cs, rs = math.floor(uu), math.floor(vv)
                if not (0 <= rs < hk and 0 <= cs < wk):
                    continue
                if style == "palette":
                    x = int(lv[0, rs, cs])
                    px = lut[x] if 0 <= x < ncolors and x != fill else None
                elif style == "ramp":
                    x = lv[0, rs, cs]
                    px = None if x != x else lut[ramp_index(x, lo, hi)]
                else:
                    xs = [lv[o, rs, cs] for o in order]
                    px = None if any(x != x for x in xs) else [ramp_index(x, lo, hi) for x in xs] + [255]
                if px is not None:
                    rgba[i, r, c] = px
                    opaque[i] += int(px[3]) != 0
    return rgba, opaque, ties


# ---- the sources -------------------------------------------------------------------------------------------------------------------------
def _lattice(system, lon, lat, step, dx, dy):
    x, y = WR.from_lonlat(system, lon, lat)
    return (step * round(float(x) / step) + dx, step * round(float(y) / step) + dy, step, step)


# name -> (coordinate system, grid): the origin on a lattice of the pixel size, moved by a few irrational-looking units
SOURCES = {
    "utm_north": (U36, _lattice(U36, 34.0, 40.6, 30.0, 7.3819, -11.1743)),
    "utm_south": (U36S, _lattice(U36S, 34.0, -40.6, 30.0, 3.7127, 5.9341)),
    "geographic": (WR.GEOGRAPHIC, _lattice(WR.GEOGRAPHIC, 34.0, 40.6, 0.00027, 1.3713e-5, -0.7391e-5)),
    "web_mercator": (WEBM, _lattice(WEBM, 34.0, 40.6, 38.2, 2.9173, -4.4419)),
}


@functools.lru_cache(maxsize=None)
def class_levels():
    """An int8 class map of classes 0..4 with fill (-1) and the stray values 5 (= NCOLORS), 9 and -7, and its MODE pyramid."""
    rng = np.random.default_rng(11)
    values = np.array([-1, 0, 1, 2, 3, 4, 4, 5, 9, -7], dtype=np.int8)
    cm = values[rng.integers(0, len(values), size=(H // 4 + 1, W // 4 + 1))].repeat(4, axis=0).repeat(4, axis=1)[:H, :W]
    cm = np.ascontiguousarray(cm)
    cm[rng.random((H, W)) < 0.1] = -1
    return [cm] + OR.pyramid(cm, "mode", NLEVELS - 1, FILL)


@functools.lru_cache(maxsize=None)
def float_levels(bands):
    """float32 values in [-0.5, 1.5] (so LO = 0 and HI = 1 clamp on both sides) with NaN holes, values exactly LO and HI, an infinity
    of each sign, and the MEAN pyramid."""
    rng = np.random.default_rng(20 + bands)
    a = (rng.random((bands, H, W)) * 2.0 - 0.5).astype(np.float32)
    a[rng.random((bands, H, W)) < 0.08] = np.nan
    a[:, 10:20, 10:20] = np.float32(LO)
    a[:, 30:40, 50:60] = np.float32(HI)
    a[:, 60, 60], a[:, 61, 61] = np.inf, -np.inf
    return [a if bands > 1 else a[0]] + [lv if bands > 1 else lv[0] for lv in OR.pyramid(a, "mean", NLEVELS - 1)]


def palette():
    """(256, 4) uint8: NCOLORS opaque colours (no byte of them is 0xA5), the rest zero."""
    lut = np.zeros((256, 4), dtype=np.uint8)
    lut[:NCOLORS] = [(200, 30, 30, 255), (30, 200, 30, 255), (30, 30, 200, 255), (220, 220, 40, 255), (40, 220, 220, 128)]
    return lut


def ramp():
    """(256, 4) uint8: entry i = (i, 255 - i, i // 2, 255)."""
    i = np.arange(256)
    return np.stack([i, 255 - i, i // 2, np.full(256, 255)], axis=1).astype(np.uint8)


def _centre(name):
    system, (X0, Y0, sx, sy) = SOURCES[name]
    x, y = X0 + 0.5 * W * sx, Y0 - 0.5 * H * sy
    if system != WEBM:
        x, y = WR.from_lonlat(WEBM, *WR.to_lonlat(system, x, y))
    return float(x), float(y)


def tile_cases(name, tile):
    """-> (grids, levels of the tiles) for source ``name``: tiles of ``tile`` pixels around the source's centre in EPSG:3857.  At 40.6
    degrees a 30 m (0.00027 degree) source pixel is about 39.5 m (39.6 m) of web Mercator, so a tile pixel of 39.7 * 2^k m reads level k
    at a little over one step per pixel.  tile 64: level 0 wholly inside, across the west / north / east / south edge, wholly outside
    (opaque 0), then level 1 and level 2 (both larger than the source: across every edge).  tile 128: one tile per level, the level 0
    one across every edge."""
    cx, cy = _centre(name)
    px = 39.7

    def at(k, dx, dy):  # the tile of level k whose centre lies (dx, dy) tile widths east / south of the source's centre
        p = px * (1 << k)
        ox, oy = (1.7321, -0.5773) if tile == 64 else (2.6458, -0.8317)
        return (cx + (dx - 0.5) * tile * p + ox, cy - (dy - 0.5) * tile * p + oy, p, p)

    if tile == 64:
        grids = [at(0, 0, 0), at(0, -0.9, 0.1), at(0, 0.1, -0.9), at(0, 0.9, -0.1), at(0, -0.1, 0.9), at(0, 4, 4), at(1, 0.1, -0.1), at(2, -0.2, 0.1)]
        return grids, [0, 0, 0, 0, 0, 0, 1, 2]
    return [at(0, 0.05, -0.05), at(1, -0.1, 0.1), at(2, 0.2, 0.2)], [0, 1, 2]


STYLE_ARGS = {
    "palette": dict(lut=palette(), ncolors=NCOLORS, fill=FILL),
    "ramp": dict(lut=ramp(), lo=LO, hi=HI),
    "rgb": dict(lo=LO, hi=HI, order=ORDER),
}


def levels_of(style):
    return class_levels() if style == "palette" else float_levels(3 if style == "rgb" else 1)


@functools.lru_cache(maxsize=None)
def twin(name, tile, style, fill=FILL):
    """The twin's (rgba, opaque, ties) for one source, tile size and style, computed once per session."""
    system, grid = SOURCES[name]
    grids, lvls = tile_cases(name, tile)
    kw = dict(STYLE_ARGS[style])
    if style == "palette":
        kw["fill"] = fill
    return render(levels_of(style), system, grid, grids, lvls, tile, style, **kw)


CASES = [(name, tile, style) for name in SOURCES for tile in (64, 128) for style in ("palette", "ramp", "rgb")
         if tile == 64 or name in ("utm_north", "web_mercator") or style == "palette"]
