"""Web Mercator map tiles of prediction and imagery mosaics, rendered on the device.

The reference's backend serves ``tiles/WebMercatorQuad/{z}/{x}/{y}@1x.png`` through TiTiler (``new_apps/backend/app/tiler_service.py``):
per request a warp into EPSG:3857, a choice of overview level, nearest sampling and a class colormap (segmentation), ``rescale=lo,hi``
plus a colour ramp (regression) or ``expression=b3;b2;b1&rescale=0,3000`` (the imagery, ``chips_merged.tif``).  GDAL and TiTiler are
absent here; this module is the stand-in.  It writes the whole pyramid of tiles once, as ``{z}/{x}/{y}.png`` files with a
``tilejson.json``, which any XYZ client (Leaflet, MapLibre, OpenLayers, QGIS) reads from a folder or a static file server.

The rule (stated in ``include/instageo_hip.h``).  The source is one raster as a pyramid in the level geometry of :mod:`instageo_amd.cog`
(MODE levels for class maps, MEAN levels for float32).  A tile is a ``tile`` x ``tile`` grid in EPSG:3857; the centre of each of its
pixels goes through the float64 chain of the warp to the source pixel coordinates (u, v), which are divided by 2^level; NEAREST takes the
pixel (floor(v), floor(u)) of that level, and a pixel outside it is transparent.  ``palette``: class v -> ``lut[v]``; ``ramp``:
``lut[rint(clamp((v - lo) / (hi - lo), 0, 1) * 255)]``; ``rgb``: three planes through the same index, alpha 255; ``fill`` / NaN are
transparent.  The LEVEL of a tile is chosen on the host (:func:`choose_levels`), for both paths alike.

Device tensors go through ``ig_tile_render``; host arrays take a numpy twin of the same rule on top of :mod:`instageo_amd.crs`, so the
export works (and is tested) without a GPU.  The PNG deflate runs on the host, in a thread pool.

Not done: bilinear or cubic tile resampling, ``@2x`` tiles, JPEG / WebP, MBTiles / PMTiles, an HTTP server, TMS y-numbering, tile matrix
sets other than WebMercatorQuad, rasters across the antimeridian, probability and uncertainty layers, and any claim of pixel equality with
TiTiler or GDAL (their overview choice and rounding differ; DESIGN.md 3.24 says where).
"""
from __future__ import annotations

import json
import math
import os
import struct
import time
import zlib
from concurrent.futures import ThreadPoolExecutor
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import cog as cogmod
from . import crs as crsmod
from . import tiff
from . import warp as warpmod
from .prep import is_device

R = 6378137.0
ORIGIN = math.pi * R  # 20037508.342789244: the web Mercator square spans +-ORIGIN
WEBM = crsmod.from_epsg(3857)
STYLES = ("palette", "ramp", "rgb")
MAX_ZOOM = 24
EDGE_POINTS = 33  # per edge of the raster's outline
PNG_THREADS = 16
BATCH_PIXELS = 1 << 26  # of one launch (256 MiB of RGBA); the kernel's own bound is n * tile^2 < 2^31
TIMINGS: Dict[str, float] = {}  # wall seconds of the phases of the latest export: pyramid, render, readback, png

# the project's own 16 class colours (cycled), and the five anchors of the ramp (dark blue, teal, green, yellow, red)
DEFAULT_PALETTE = ((68, 1, 84), (253, 231, 37), (33, 145, 140), (230, 85, 13), (49, 104, 142), (181, 222, 43), (214, 39, 110), (94, 201, 98),
                   (120, 80, 200), (255, 160, 122), (0, 109, 44), (158, 202, 225), (140, 81, 10), (250, 159, 181), (90, 90, 90), (255, 255, 255))
RAMP_ANCHORS = ((13, 8, 135), (0, 128, 160), (40, 180, 70), (250, 220, 40), (200, 20, 30))
_PNG_MAGIC = b"\x89PNG\r\n\x1a\n"


# ---- the tile lattice ------------------------------------------------------------------------------------------------------------------
def check_tile_size(tile) -> int:
    if isinstance(tile, bool) or not isinstance(tile, (int, np.integer)) or not 64 <= int(tile) <= 1024 or int(tile) % 64:
        raise ValueError(f"map_tiles_size must be a multiple of 64 in 64..1024 (got {tile!r})")
    return int(tile)


def _check_zxy(z, x, y) -> Tuple[int, int, int]:
    z, x, y = int(z), int(x), int(y)
    if not 0 <= z <= MAX_ZOOM or not 0 <= x < (1 << z) or not 0 <= y < (1 << z):
        raise ValueError(f"no tile ({z}, {x}, {y}) in WebMercatorQuad (0 <= z <= {MAX_ZOOM}, 0 <= x, y < 2^z)")
    return z, x, y


def tile_grid(z: int, x: int, y: int, tile: int = 256) -> Tuple[float, float, float, float]:
    """(X0, Y0, s, s) in EPSG:3857 of XYZ tile (z, x, y) rendered at ``tile`` x ``tile`` pixels: R = 6378137, y counted from the north."""
    z, x, y = _check_zxy(z, x, y)
    side = 2.0 * ORIGIN / (1 << z)
    return -ORIGIN + x * side, ORIGIN - y * side, side / tile, side / tile


def tile_bounds(z: int, x: int, y: int) -> Tuple[float, float, float, float]:
    """(west, south, east, north) of tile (z, x, y) in degrees."""
    z, x, y = _check_zxy(z, x, y)
    n = float(1 << z)
    lat = lambda j: math.degrees(math.atan(math.sinh(math.pi * (1.0 - 2.0 * j / n))))  # noqa: E731
    return x / n * 360.0 - 180.0, lat(y + 1), (x + 1) / n * 360.0 - 180.0, lat(y)


def _source(profile: Dict[str, Any]) -> Tuple[crsmod.Crs, Tuple[float, float, float, float]]:
    return crsmod.from_profile(profile), warpmod.grid_of(profile)


def outline(profile: Dict[str, Any], shape: Tuple[int, int]) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """The raster's border, ``EDGE_POINTS`` points per edge -> (x, y in EPSG:3857, longitude, latitude).  ValueError when a point lies
    outside the domain of web Mercator or the raster crosses the antimeridian (its longitudes span more than 180 degrees)."""
    system, (X0, Y0, sx, sy) = _source(profile)
    h, w = int(shape[0]), int(shape[1])
    t = np.linspace(0.0, 1.0, EDGE_POINTS)
    ex, ey = X0 + t * (w * sx), Y0 - t * (h * sy)
    bx = np.concatenate([ex, ex, np.full_like(t, X0), np.full_like(t, X0 + w * sx)])
    by = np.concatenate([np.full_like(t, Y0), np.full_like(t, Y0 - h * sy), ey, ey])
    lon, lat = crsmod.inverse(system, bx, by)
    x, y = crsmod.forward(WEBM, lon, lat)
    if not (np.isfinite(x).all() and np.isfinite(y).all()) or np.abs(y).max() > ORIGIN:
        raise ValueError("the raster reaches outside the web Mercator square (|latitude| > 85.05 degrees or outside its own domain)")
    if lon.max() - lon.min() > 180.0 or lon.min() < -180.0 or lon.max() > 180.0:
        raise ValueError("the raster crosses the antimeridian: its map tiles are not rendered")
    return x, y, lon, lat


def covering_tiles(profile: Dict[str, Any], shape: Tuple[int, int], z: int) -> List[Tuple[int, int, int]]:
    """The tiles (z, x, y) of zoom ``z`` that the bounding box of the raster's densified outline touches, row by row from the north-west.
    Conservative: a tile the raster misses renders fully transparent and is not written."""
    x, y, _, _ = outline(profile, shape)
    n = 1 << int(z)
    _check_zxy(z, 0, 0)
    side = 2.0 * ORIGIN / n
    clampi = lambda v: int(min(max(v, 0), n - 1))  # noqa: E731
    x0, x1 = clampi(math.floor((x.min() + ORIGIN) / side)), clampi(math.floor((x.max() + ORIGIN) / side))
    y0, y1 = clampi(math.floor((ORIGIN - y.max()) / side)), clampi(math.floor((ORIGIN - y.min()) / side))
    return [(int(z), i, j) for j in range(y0, y1 + 1) for i in range(x0, x1 + 1)]


def _steps(system, grid, px, py, step: float) -> np.ndarray:
    """The smaller of the source-pixel steps per step of ``step`` metres along x and along y at the EPSG:3857 points (px, py); NaN where
    a point leaves the source's domain."""
    px, py = np.asarray(px, dtype=np.float64), np.asarray(py, dtype=np.float64)
    xs = np.stack([px, px + step, px])
    ys = np.stack([py, py, py - step])
    sx_, sy_ = crsmod.transform(WEBM, system, xs, ys)
    u, v = (sx_ - grid[0]) / grid[2], (grid[1] - sy_) / grid[3]
    with np.errstate(invalid="ignore"):
        return np.minimum(np.hypot(u[1] - u[0], v[1] - v[0]), np.hypot(u[2] - u[0], v[2] - v[0]))


def _centre_3857(profile, shape) -> Tuple[float, float]:
    system, (X0, Y0, sx, sy) = _source(profile)
    x, y = crsmod.transform(system, WEBM, X0 + 0.5 * shape[1] * sx, Y0 - 0.5 * shape[0] * sy)
    return float(x), float(y)


def zoom_range(profile: Dict[str, Any], shape: Tuple[int, int], nlevels: int, tile: int = 256, minzoom: Union[str, int, None] = "auto",
               maxzoom: Union[str, int, None] = "auto") -> Tuple[int, int]:
    """-> (minzoom, maxzoom).  ``maxzoom`` ``auto``: the smallest z at which one tile pixel at the raster's centre is no larger than one
    source pixel (the step of :func:`choose_levels` <= 1), at most 24; ``minzoom`` ``auto``: max(0, maxzoom - nlevels), where the coarsest
    level is still at most two source steps per tile pixel."""
    for name, v in (("map_tiles_minzoom", minzoom), ("map_tiles_maxzoom", maxzoom)):
        if v in (None, "auto"):
            continue
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= MAX_ZOOM:
            raise ValueError(f"{name} must be 'auto' or an int in 0..{MAX_ZOOM} (got {v!r})")
    tile = check_tile_size(tile)
    if maxzoom in (None, "auto"):
        system, grid = _source(profile)
        cx, cy = _centre_3857(profile, shape)
        s0 = float(_steps(system, grid, cx, cy, 1.0)) * (2.0 * ORIGIN / tile)  # source steps per tile pixel at z = 0, from the local scale
        if not np.isfinite(s0) or s0 <= 0:
            raise ValueError("the raster's centre lies outside the domain of its own or the web Mercator projection")
        maxzoom = min(max(int(math.ceil(math.log2(s0) - 1e-9)), 0), MAX_ZOOM)
    maxzoom = int(maxzoom)
    minzoom = max(0, maxzoom - int(nlevels)) if minzoom in (None, "auto") else int(minzoom)
    if minzoom > maxzoom:
        raise ValueError(f"map_tiles_minzoom {minzoom} lies above map_tiles_maxzoom {maxzoom}")
    return minzoom, maxzoom


def choose_levels(profile: Dict[str, Any], shape: Tuple[int, int], tiles: Sequence[Tuple[int, int, int]], nlevels: int,
                  tile: int = 256) -> np.ndarray:
    """The pyramid level of every tile, (n,) int32: with s = the smaller of the source-pixel steps per tile pixel along x and along y at
    the tile's centre (through :func:`crs.transform`; where the centre lies outside the source's domain, at the tile's point nearest to
    the raster's centre), level = clamp(floor(log2(s (1 + 1e-9))), 0, nlevels - 1): the coarsest level that is still at least as fine as
    the tile.  -1 (a transparent tile) where s cannot be computed at all."""
    system, grid = _source(profile)
    out = np.zeros(len(tiles), dtype=np.int32)
    if not len(tiles):
        return out
    g = np.array([tile_grid(z, x, y, tile) for z, x, y in tiles], dtype=np.float64)
    half = 0.5 * tile * g[:, 2]
    s = _steps(system, grid, g[:, 0] + half, g[:, 1] - half, 1.0) * g[:, 2]
    bad = ~np.isfinite(s)
    if bad.any():
        cx, cy = _centre_3857(profile, shape)
        px, py = np.clip(cx, g[bad, 0], g[bad, 0] + 2 * half[bad]), np.clip(cy, g[bad, 1] - 2 * half[bad], g[bad, 1])
        s[bad] = _steps(system, grid, px, py, 1.0) * g[bad, 2]
    ok = np.isfinite(s) & (s > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        lv = np.floor(np.log2(np.where(ok, s, 1.0) * (1.0 + 1e-9)))
    out[:] = np.where(ok, np.clip(lv, 0, int(nlevels) - 1), -1).astype(np.int32)
    return out


# ---- colours ---------------------------------------------------------------------------------------------------------------------------
def default_ramp() -> np.ndarray:
    """(256, 4) uint8: integer linear interpolation between the five ``RAMP_ANCHORS``, alpha 255."""
    a = np.array(RAMP_ANCHORS, dtype=np.int64)
    i = np.arange(256, dtype=np.int64)
    seg = np.minimum(i * 4 // 255, 3)
    pos = i * 4 - seg * 255  # 0..255 within the segment
    rgb = a[seg] + ((a[seg + 1] - a[seg]) * pos[:, None] + 127) // 255
    return np.concatenate([rgb, np.full((256, 1), 255)], axis=1).astype(np.uint8)


def load_colors(path_or_list) -> np.ndarray:
    """A JSON file (or a list) of ``[r, g, b]`` / ``[r, g, b, a]`` entries, 1..256 of them, each 0..255 -> (k, 4) uint8 (alpha 255 where
    none is given)."""
    data = path_or_list
    if isinstance(path_or_list, (str, os.PathLike)):
        with open(path_or_list) as f:
            data = json.load(f)
    try:
        rows = [[int(v) for v in row] for row in data]
    except (TypeError, ValueError) as e:
        raise ValueError(f"map_tiles_palette must hold a list of [r, g, b] or [r, g, b, a] entries ({e})") from e
    if not 1 <= len(rows) <= 256 or any(len(r) not in (3, 4) or any(not 0 <= v <= 255 for v in r) for r in rows):
        raise ValueError("map_tiles_palette must hold 1..256 entries [r, g, b] or [r, g, b, a] with values in 0..255")
    return np.array([r + [255] * (4 - len(r)) for r in rows], dtype=np.uint8)


def palette_lut(ncolors: int, colors=None) -> np.ndarray:
    """(256, 4) uint8: entry v < ``ncolors`` is ``colors[v % len(colors)]`` (default: ``DEFAULT_PALETTE``, alpha 255), the rest zero."""
    c = load_colors(colors) if colors is not None else load_colors(DEFAULT_PALETTE)
    if not 0 <= int(ncolors) <= 256:
        raise ValueError(f"a palette has 0..256 classes (got {ncolors})")
    lut = np.zeros((256, 4), dtype=np.uint8)
    if ncolors:
        lut[: int(ncolors)] = c[np.arange(int(ncolors)) % len(c)]
    return lut


def ramp_lut(colors=None) -> np.ndarray:
    """(256, 4) uint8: :func:`default_ramp`, or the 256 entries of ``colors``."""
    if colors is None:
        return default_ramp()
    c = load_colors(colors)
    if len(c) != 256:
        raise ValueError(f"a colour ramp has 256 entries (got {len(c)})")
    return c


# ---- rendering -------------------------------------------------------------------------------------------------------------------------
def ramp_index(v: np.ndarray, lo: float, hi: float) -> np.ndarray:
    """rint(clamp((float64(v) - lo) / (hi - lo), 0, 1) * 255) as int64 (NaN -> 0: the caller masks it)."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = (v.astype(np.float64) - float(lo)) / (float(hi) - float(lo))
        t = np.where(t < 0.0, 0.0, np.where(t > 1.0, 1.0, t))
        return np.rint(np.where(np.isnan(t), 0.0, t) * 255.0).astype(np.int64)


def _render_host(levels, system, grid, grids, lvls, tile, style, lut, ncolors, fill, rescale, order):
    """numpy twin of ``ig_tile_render``, tile by tile, vectorised over the pixels."""
    n = len(grids)
    rgba = np.zeros((n, tile, tile, 4), dtype=np.uint8)
    opaque = np.zeros(n, dtype=np.int32)
    levels = [np.asarray(lv) for lv in levels]
    levels = [lv[None] if lv.ndim == 2 else lv for lv in levels]
    src_ok = bool(np.isfinite(grid).all() and grid[2] > 0 and grid[3] > 0)
    for i in range(n):
        g, k = grids[i], int(lvls[i])
        if not (0 <= k < len(levels)) or not src_ok or not (np.isfinite(g).all() and g[2] > 0 and g[3] > 0):
            continue
        lv = levels[k]
        hk, wk = lv.shape[-2:]
        u, v = warpmod.coords(WEBM.params, g, (tile, tile), system, grid)
        with np.errstate(invalid="ignore"):
            fc, fr = np.floor(u / float(1 << k)), np.floor(v / float(1 << k))
            inside = (fc >= 0) & (fc < wk) & (fr >= 0) & (fr < hk)
        c, r = np.where(inside, fc, 0).astype(np.int64), np.where(inside, fr, 0).astype(np.int64)
        if style == "palette":
            val = lv[0][r, c].astype(np.int64)
            show = inside & (val >= 0) & (val < ncolors) & (val != fill)
            px = lut[np.where(show, val, 0)]
        elif style == "ramp":
            val = lv[0][r, c]
            show = inside & ~np.isnan(val)
            px = lut[ramp_index(val, *rescale)]
        else:
            val = [lv[o][r, c] for o in order]
            show = inside & ~np.isnan(val[0]) & ~np.isnan(val[1]) & ~np.isnan(val[2])
            px = np.stack([ramp_index(x, *rescale) for x in val] + [np.full(c.shape, 255, dtype=np.int64)], axis=-1).astype(np.uint8)
        rgba[i] = np.where(show[..., None], px, 0)
        opaque[i] = int((rgba[i][..., 3] != 0).sum())
    return rgba, opaque


def _check_style(levels, style):
    first = levels[0]
    name = str(first.dtype).replace("torch.", "")
    bands = 1 if first.ndim == 2 else int(first.shape[0])
    if style is None:
        style = "palette" if name == "int8" else "rgb" if bands == 3 else "ramp"
    if style not in STYLES:
        raise ValueError(f"style must be one of {STYLES} (got {style!r})")
    want = ("int8", 1) if style == "palette" else ("float32", 3 if style == "rgb" else 1)
    if (name, bands) != want:
        raise ValueError(f"style {style!r} renders {want[0]} rasters of {want[1]} band(s) (got {name} with {bands})")
    return style


def render(levels, profile: Dict[str, Any], tiles: Sequence[Tuple[int, int, int]], style: Optional[str] = None, tile: int = 256, lut=None,
           ncolors: Optional[int] = None, fill: int = -1, rescale: Optional[Tuple[float, float]] = None, order: Tuple[int, int, int] = (0, 1, 2),
           levels_of_tiles=None):
    """Tiles ``tiles`` = [(z, x, y), ...] of the pyramid ``levels`` ([level 0, level 1, ...] of :func:`cog.build_overviews`) whose level 0
    has the georeferencing of ``profile`` -> (rgba (n, tile, tile, 4) uint8, opaque (n,) int32: the pixels with alpha != 0).  Device
    tensors go through ``ig_tile_render`` in batches of at most 2^26 pixels and give device tensors; anything else takes the numpy
    twin and gives arrays with the same bytes.  ``style`` None: ``palette`` for int8, ``ramp`` for one float32 band, ``rgb`` for three.
    ``lut``: (256, 4) uint8, default :func:`palette_lut` (``ncolors``: the classes, default the largest value of level 0 + 1) or
    :func:`default_ramp`; ``rescale`` = (lo, hi), default the finite minimum and maximum of level 0; ``order``: the plane behind R, G, B.
    ``levels_of_tiles``: the pyramid level per tile, default :func:`choose_levels`."""
    levels = list(levels)
    if not levels:
        raise ValueError("a pyramid has at least level 0")
    style = _check_style(levels, style)
    tile = check_tile_size(tile)
    dev = is_device(levels[0])
    if not dev:
        levels = [np.asarray(lv.cpu() if hasattr(lv, "cpu") else lv) for lv in levels]
    H, W = (int(v) for v in levels[0].shape[-2:])
    system, grid = _source(profile)
    if style == "palette":
        if ncolors is None:
            ncolors = max(int(levels[0].max()) + 1, 1)
        lut = palette_lut(ncolors) if lut is None else lut
    else:
        if rescale is None:
            rescale = finite_range(levels[0])
        lut = default_ramp() if lut is None and style == "ramp" else lut
    rescale = (0.0, 1.0) if rescale is None else (float(rescale[0]), float(rescale[1]))
    if style != "palette" and not (np.isfinite(rescale).all() and rescale[1] > rescale[0]):
        raise ValueError(f"map_tiles_rescale = (lo, hi) needs finite values with lo < hi (got {rescale})")
    grids = np.array([tile_grid(z, x, y, tile) for z, x, y in tiles], dtype=np.float64).reshape(-1, 4)
    lvls = choose_levels(profile, (H, W), tiles, len(levels), tile) if levels_of_tiles is None else np.asarray(levels_of_tiles, dtype=np.int32)
    if not dev:
        lut_h = None if lut is None else np.ascontiguousarray(lut, dtype=np.uint8)
        return _render_host(levels, system.params, np.array(grid), grids, lvls, tile, style, lut_h, int(ncolors or 0), int(fill), rescale, order)
    import torch

    from . import ops

    n = len(grids)
    if lut is not None and not torch.is_tensor(lut):
        lut = torch.from_numpy(np.ascontiguousarray(lut, dtype=np.uint8)).to(levels[0].device)
    rgba = torch.empty((n, tile, tile, 4), dtype=torch.uint8, device=levels[0].device)
    opaque = torch.empty((n,), dtype=torch.int32, device=levels[0].device)
    per = max(1, BATCH_PIXELS // (tile * tile))
    levels = [lv.contiguous() for lv in levels]
    for a in range(0, n, per):
        _, opaque[a : a + per] = ops.tile_render(levels, system.params, grid, grids[a : a + per], lvls[a : a + per], tile, style, lut,
                                                 int(ncolors or 0), int(fill), rescale, order, out=rgba[a : a + per])
    return rgba, opaque


def finite_range(raster) -> Tuple[float, float]:
    """(lo, hi): the finite minimum and maximum of ``raster`` (array or tensor); hi = lo + 1 where they coincide, (0, 1) where nothing
    is finite."""
    if is_device(raster):
        import torch

        ok = torch.isfinite(raster)
        if not bool(ok.any()):
            return 0.0, 1.0
        v = raster[ok]
        lo, hi = float(v.min()), float(v.max())
    else:
        a = np.asarray(raster)
        ok = np.isfinite(a)
        if not ok.any():
            return 0.0, 1.0
        lo, hi = float(a[ok].min()), float(a[ok].max())
    return (lo, hi) if hi > lo else (lo, lo + 1.0)


# ---- PNG -------------------------------------------------------------------------------------------------------------------------------
def _chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def encode_png(rgba: np.ndarray, level: int = 6) -> bytes:
    """(h, w, 4) uint8 -> the bytes of an 8-bit RGBA PNG (colour type 6, every row filter 0, one IDAT)."""
    a = np.ascontiguousarray(rgba, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] != 4 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"a PNG tile is (h, w, 4) uint8 (got {a.shape})")
    if isinstance(level, bool) or not isinstance(level, (int, np.integer)) or not 0 <= int(level) <= 9:
        raise ValueError(f"map_tiles_png_level must be an int in 0..9 (got {level!r})")
    h, w = a.shape[:2]
    raw = np.zeros((h, 1 + 4 * w), dtype=np.uint8)
    raw[:, 1:] = a.reshape(h, 4 * w)
    return (_PNG_MAGIC + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)) + _chunk(b"IDAT", zlib.compress(raw.tobytes(), int(level)))
            + _chunk(b"IEND", b""))


def write_png(path: str, rgba: np.ndarray, level: int = 6) -> str:
    data = encode_png(rgba, level)
    with open(path, "wb") as f:
        f.write(data)
    return path


def read_png(path: str) -> np.ndarray:
    """The (h, w, 4) uint8 pixels of an 8-bit RGBA, non-interlaced PNG whose rows all use filter 0 (what :func:`write_png` writes)."""
    with open(path, "rb") as f:
        buf = f.read()
    if buf[:8] != _PNG_MAGIC:
        raise ValueError(f"{path}: not a PNG file")
    pos, head, data = 8, None, b""
    while pos + 8 <= len(buf):
        size, kind = struct.unpack(">I4s", buf[pos : pos + 8])
        body = buf[pos + 8 : pos + 8 + size]
        if len(body) != size or zlib.crc32(kind + body) & 0xFFFFFFFF != struct.unpack(">I", buf[pos + 8 + size : pos + 12 + size])[0]:
            raise ValueError(f"{path}: a truncated or corrupt {kind!r} chunk")
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            data += body
        elif kind == b"IEND":
            break
        pos += 12 + size
    if head is None or head[2:] != (8, 6, 0, 0, 0):
        raise ValueError(f"{path}: only 8-bit RGBA PNGs without interlacing are read (IHDR {head})")
    w, h = head[:2]
    raw = np.frombuffer(zlib.decompress(data), dtype=np.uint8)
    if raw.size != h * (1 + 4 * w):
        raise ValueError(f"{path}: {raw.size} bytes of pixel data for {w} x {h} RGBA")
    raw = raw.reshape(h, 1 + 4 * w)
    if raw[:, 0].any():
        raise ValueError(f"{path}: a row filter other than 0")
    return raw[:, 1:].reshape(h, w, 4).copy()


# ---- export ----------------------------------------------------------------------------------------------------------------------------
def _follows(shapes) -> bool:
    return all(b == ((a[0] + 1) // 2, (a[1] + 1) // 2) for a, b in zip(shapes, shapes[1:]))


def load_pyramid(raster, profile=None, kind: Optional[str] = None, fill: int = -1, tile: int = 256, device: Optional[str] = None):
    """-> (levels, profile).  ``raster``: a GeoTIFF path (through :func:`tiff.read`; the overviews of a COG are used when they follow the
    ceil(/2) chain, not rebuilt), a list of levels already built (used as it is), or an array / tensor (H, W) or (bands, H, W) with
    ``profile``: the pyramid then comes from :func:`cog.build_overviews`, MODE for int8, MEAN for float32, down to one tile.  ``device``
    (e.g. "cuda") uploads a host raster before its pyramid is built (the kernels of ``cog.hip`` build it), and host levels as they are."""
    if isinstance(raster, (str, os.PathLike)):
        arr, profile = tiff.read(str(raster))
        levels = [arr]
        for k in range(1, tiff.overview_count(str(raster)) + 1):
            levels.append(tiff.read(str(raster), level=k)[0])
        if not _follows([lv.shape[-2:] for lv in levels]) or len(levels) > 13:
            levels = levels[:1]
        raster = levels if len(levels) > 1 else arr
    if profile is None:
        raise ValueError("map tiles need the raster's georeferencing (a profile)")
    if isinstance(raster, (list, tuple)):
        levels = list(raster)
    else:
        name = str(raster.dtype).replace("torch.", "")
        kind = kind or {"int8": "mode", "float32": "mean"}.get(name)
        if kind is None:
            raise ValueError(f"map tiles render int8 class maps and float32 rasters (got {name})")
        if raster.ndim == 3 and raster.shape[0] == 1:
            raster = raster[0]
        if device is not None and not is_device(raster):  # level 0 goes up first, so that the pyramid comes from the kernels of cog.hip
            import torch

            raster = torch.from_numpy(np.ascontiguousarray(raster)).to(device)
        levels = cogmod.build_overviews(raster, kind, "auto", fill, blocksize=tile)
    levels = [lv[0] if lv.ndim == 3 and lv.shape[0] == 1 else lv for lv in levels]
    if device is not None and not is_device(levels[0]):
        import torch

        levels = [torch.from_numpy(np.ascontiguousarray(lv)).to(device) for lv in levels]
    return levels, profile


def tilejson(profile, shape, minzoom: int, maxzoom: int, style: str, name: str = "instageo", colors=None, rescale=None) -> Dict[str, Any]:
    """The TileJSON 3.0.0 description of an exported pyramid."""
    _, _, lon, lat = outline(profile, shape)
    bounds = [float(lon.min()), float(lat.min()), float(lon.max()), float(lat.max())]
    doc = {"tilejson": "3.0.0", "name": name, "scheme": "xyz", "tiles": ["{z}/{x}/{y}.png"], "minzoom": int(minzoom), "maxzoom": int(maxzoom),
           "bounds": bounds, "center": [(bounds[0] + bounds[2]) / 2, (bounds[1] + bounds[3]) / 2, int(minzoom)], "style": style}
    if colors is not None:
        doc["colors"] = [[int(v) for v in c] for c in colors]
    if rescale is not None:
        doc["rescale"] = [float(rescale[0]), float(rescale[1])]
    return doc


def export(raster, out_dir: str, profile=None, style: Optional[str] = None, tile: int = 256, minzoom: Union[str, int, None] = "auto",
           maxzoom: Union[str, int, None] = "auto", palette=None, ncolors: Optional[int] = None, fill: int = -1, rescale=None,
           order: Tuple[int, int, int] = (0, 1, 2), png_level: int = 6, device: Optional[str] = None, name: str = "instageo") -> List[str]:
    """``raster`` (see :func:`load_pyramid`) -> ``out_dir/{z}/{x}/{y}.png`` for z = minzoom..maxzoom (:func:`zoom_range`) and
    ``out_dir/tilejson.json``; returns the written paths.  ``palette``: a JSON file or list of colours: the class colours for ``palette``
    (cycled), the 256 entries of the ramp for ``ramp``.  Tiles without an opaque pixel are not written.  PNGs are deflated at
    ``png_level`` in a pool of at most 16 threads."""
    tile = check_tile_size(tile)
    encode_png(np.zeros((1, 1, 4), dtype=np.uint8), png_level)  # checks png_level before any work
    t0 = time.perf_counter()
    levels, profile = load_pyramid(raster, profile, fill=fill, tile=tile, device=device)
    style = _check_style(levels, style)
    shape = tuple(int(v) for v in levels[0].shape[-2:])
    zmin, zmax = zoom_range(profile, shape, len(levels), tile, minzoom, maxzoom)
    colors = None
    if style == "palette":
        ncolors = int(ncolors) if ncolors is not None else max(int(levels[0].max()) + 1, 1)
        lut = palette_lut(ncolors, palette)
        colors = lut[:ncolors]
    else:
        rescale = finite_range(levels[0]) if rescale is None else (float(rescale[0]), float(rescale[1]))
        lut = ramp_lut(palette) if style == "ramp" else None
    t = {"pyramid": time.perf_counter() - t0, "render": 0.0, "readback": 0.0, "png": 0.0}
    written: List[str] = []
    os.makedirs(out_dir, exist_ok=True)
    dev = is_device(levels[0])
    for z in range(zmin, zmax + 1):
        tiles = covering_tiles(profile, shape, z)
        per = max(1, BATCH_PIXELS // (tile * tile))
        for a in range(0, len(tiles), per):
            part = tiles[a : a + per]
            t0 = time.perf_counter()
            rgba, opaque = render(levels, profile, part, style, tile, lut, ncolors, fill, rescale, order)
            if dev:
                import torch

                torch.cuda.synchronize()
            t1 = time.perf_counter()
            opaque = opaque.cpu().numpy() if dev else opaque
            keep = np.flatnonzero(opaque > 0)
            if dev:  # only the tiles that will be written come back
                import torch

                rgba = rgba[torch.from_numpy(keep).to(rgba.device)].cpu().numpy() if len(keep) else np.zeros((0, tile, tile, 4), dtype=np.uint8)
            else:
                rgba = rgba[keep]
            t2 = time.perf_counter()
            paths = []
            for k in keep:
                zz, x, y = part[int(k)]
                os.makedirs(os.path.join(out_dir, str(zz), str(x)), exist_ok=True)
                paths.append(os.path.join(out_dir, str(zz), str(x), f"{y}.png"))
            if paths:
                with ThreadPoolExecutor(max_workers=min(PNG_THREADS, len(paths))) as pool:  # zlib releases the GIL
                    list(pool.map(lambda pa: write_png(pa[0], pa[1], png_level), zip(paths, rgba)))
            written += paths
            t["render"] += t1 - t0
            t["readback"] += t2 - t1
            t["png"] += time.perf_counter() - t2
    doc = tilejson(profile, shape, zmin, zmax, style, name, colors, rescale if style != "palette" else None)
    path = os.path.join(out_dir, "tilejson.json")
    with open(path, "w") as f:
        json.dump(doc, f, sort_keys=True, indent=1)
    written.append(path)
    TIMINGS.clear()
    TIMINGS.update(t)
    return written


# ---- the imagery -----------------------------------------------------------------------------------------------------------------------
def merge_chips(chip_files: Sequence[str], bands: Tuple[int, int, int] = (0, 1, 2), no_data_value: Optional[float] = None,
                device: Optional[str] = None, out_path: Optional[str] = None, tile: int = 256, cog_blocksize: int = 256):
    """The input chips of a dataset -> one three-band float32 mosaic with NaN as NODATA and its MEAN pyramid: (levels, profile).  The chips
    are placed with :func:`mosaic.placement`; each of the three ``bands`` is pasted as float32 with rule ``last`` (on ``device`` by
    ``ig_mosaic_paste``, else by its numpy twin); a value equal to the file's own NODATA tag, or without one to ``no_data_value`` (default:
    that of ``chips.*``), becomes NaN.  Chips of several grids are refused (warp them first).  ``out_path``: also write the mosaic as a
    COG (``chips_merged.tif``: float32 with NaN NODATA, not the reference's int16)."""
    from . import mosaic

    paths = [str(p) for p in chip_files]
    if not paths:
        raise ValueError("map_tiles_imagery needs at least one chip file")
    if len(bands) != 3 or any(isinstance(b, bool) or int(b) < 0 for b in bands):
        raise ValueError(f"the imagery takes three band indices (got {bands!r})")
    if no_data_value is None:
        from . import chips

        no_data_value = chips.NO_DATA_VALUE
    arrays, profiles = [], []
    for p in paths:
        arr, prof = tiff.read(p, bands=[int(b) for b in bands])
        nd = prof.get("nodata")
        nd = float(no_data_value) if nd is None else float(nd)
        a = arr.astype(np.float32)
        a[arr == nd] = np.nan
        arrays.append(a)
        profiles.append(prof)
    groups = mosaic.placement(profiles, [a.shape[-2:] for a in arrays], paths, np.float32)
    if len(groups) != 1:
        raise ValueError(f"the chips lie on {len(groups)} pixel grids: map_tiles_imagery renders one (chips of one coordinate system)")
    g = groups[0]
    H, W = g.shape
    if device is None:
        canvas = np.stack([mosaic.paste([arrays[i][b] for i in g.members], g.rects, (H, W), "last") for b in range(3)])
    else:
        import torch

        from . import ops

        canvas = torch.empty((3, H, W), dtype=torch.float32, device=device)
        sizes = g.rects[:, 2].astype(np.int64) * g.rects[:, 3]
        ptr, idx = mosaic.bins(g.rects, H, W)
        for b in range(3):
            packed = torch.from_numpy(np.concatenate([arrays[i][b].reshape(-1) for i in g.members])).to(device)
            ops.mosaic_paste(packed, np.cumsum(sizes) - sizes, g.rects, ptr, idx, (H, W), "last", out=canvas[b])
    levels = cogmod.build_overviews(canvas, "mean", "auto", blocksize=min(tile, cog_blocksize))
    profile = dict(g.profile, count=3)
    if out_path is not None:
        cogmod.write_cog(out_path, levels, profile, cog_blocksize)
    return levels, profile
