"""Polygon labels burned into label rasters on the device (not in the reference, which expects label rasters made with GDAL beforehand;
``csrc/burn.hip``).  Field boundaries, flood extents, burn scars and building footprints arrive as polygons; this module
turns a GeoJSON of them into the ``label_x{..}_y{..}_{date}.tif`` rasters and the ``records.csv`` that ``mode=create_raster_chips``
takes.  :mod:`instageo_amd.zonal` rasterises polygons to count inside them; here the same scan conversion produces rasters.

The rule (stated in ``include/instageo_hip.h``).  Grid, fixed point and inside test are those of :mod:`instageo_amd.zonal`: vertices are
quantised to Q = 256 units per pixel, ``X = floor(x * 256 + 0.5)``, the pixel centre is (256 c + 128, 256 r + 128) and a pixel is inside a
feature iff an odd number of the feature's edges cross its row's centre line at or left of its centre, ties decided by ``(y0 <= Yc) !=
(y1 <= Yc)`` and ``xc <= Xc`` alone.  Features are an ordered list, in file order, each with one burn value: an int8 in [-1, 127] for
``seg`` (-1 burns the ignore value), a float32 for ``reg``.  A pixel takes the value of the LAST feature that contains its centre
(``gdal_rasterize`` burning the features one after the other); a pixel in no feature keeps what the raster held: ``background`` (0 for
``seg``, NaN for ``reg``), or, with a ``labelled_area``, the ignore value (-1 / NaN) outside that area's polygons, which are burned first
with the value ``background``: unlabelled ground is then ignored instead of counting as negative.  Everything is integer work or a
copy: the device and the numpy twin of this module give the same bytes, run after run.

Vertices go from the file's coordinate system to the grid's through :func:`crs.transform`, vertex by vertex.  Edges are NOT densified: a
long edge given in longitude / latitude is burned as the straight line between its transformed ends on the grid, not as the curve the
projection would make of it.

Device tensors go through ``ig_zone_edge_rows`` / ``ig_zone_toggle`` (as they are) and ``ig_burn_resolve``, 64 features per pass on a
canvas that covers only the pass's bounding rectangle; the cells are tallied by ``ig_label_cells``.  Host arrays take the numpy twin, which
scans feature by feature and row by row with int64 arithmetic, so the module works (and is tested) without a GPU.

``all_touched`` (default off; ``+polygon_labels.all_touched=true``): a pixel then belongs to a feature iff its centre is inside OR one of
the feature's edges touches it: the closed edge meets the pixel's OPEN square (the rule and its integer span form:
``include/instageo_hip.h``; the numpy twin: :func:`zonal.touch_spans`).  A field smaller than a pixel, which usually contains no centre,
is then burned; "last feature wins" still holds, over the pixels a feature contains or touches; the labelled area follows the same rule.
An edge along a pixel border touches neither side, so polygons on the pixel lattice burn the same pixels under both rules.  On the device
the touched bits go onto a second canvas (``ig_zone_touch_rows``, ``ig_zone_touch``) and ``ig_zone_touch_merge`` folds them into the
toggles; ``ig_burn_resolve`` runs as it is.

Out of scope: edge densification, an ignore band along boundaries, lines and points (under the open-square rule a line along a pixel
border burns nothing: they need a rule of their own), GeoPackage / Shapefile input, rotated grids.
"""
from __future__ import annotations

import csv
import json
import os
from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import crs as crsmod
from . import prep, tiff, zonal

Q, HALF = zonal.Q, zonal.Q // 2
PASS = 64  # features per pass: one bit of the uint64 canvas each
MAX_PIXELS = 2**31 - 1  # of one burn (the canvas of a pass may be the whole raster)
MAX_SIDE = 1 << 15
SEG_IGNORE = -1
SEG_CLASSES = 128  # cells of the class histogram: every non-negative int8
TASKS = {"seg": "int8", "reg": "float32"}


class Feature(NamedTuple):
    index: int  # its position in the file
    value: Any  # int in [-1, 127] (seg) or a finite float (reg)
    rings: List[np.ndarray]  # (n, 2) float64 (x, y) each, not closed
    date: Optional[str] = None


# ---- reading ---------------------------------------------------------------------------------------------------------------------------------
def read_features(path: str, value_property: Optional[str] = None, burn_value=None, class_map: Optional[Dict[str, int]] = None,
                  date_property: Optional[str] = None, task_type: str = "seg") -> List[Feature]:
    """Read a GeoJSON FeatureCollection of Polygon / MultiPolygon features -> one :class:`Feature` per feature, in file order (the ring
    handling is :func:`zonal.read_collection`, which parses the file once).  The burn value is the constant ``burn_value`` or the feature's ``value_property`` (neither:
    1 for ``seg``); for ``seg`` an integer property is used as it is and anything else is looked up, as a string, in ``class_map``
    ({name: class}); for ``reg`` the property is a number.  ValueError naming the feature for a missing property, an unmapped name, a
    class outside [-1, 127] and a regression value that is not finite (in float32).  ``date_property``: the feature's date, as text."""
    if task_type not in TASKS:
        raise ValueError(f"task_type must be seg or reg (got {task_type!r})")
    if value_property is not None and burn_value is not None:
        raise ValueError("give value_property or burn_value, not both")
    if value_property is None and burn_value is None:
        if task_type == "reg":
            raise ValueError("a regression burn needs value_property or burn_value")
        burn_value = 1
    out = []
    for i, props, rings in list(zonal.read_collection(path)):  # every geometry is read (and checked) before the first value
        raw = burn_value
        if value_property is not None:
            if value_property not in props:
                raise ValueError(f"{path}: feature {i} has no property {value_property!r}")
            raw = props[value_property]
        if task_type == "seg":
            if isinstance(raw, (int, np.integer)) and not isinstance(raw, bool):
                value = int(raw)
            else:
                if class_map is None or str(raw) not in class_map:
                    raise ValueError(f"{path}: feature {i} has the value {raw!r}, which is neither an integer nor a name of class_map")
                value = class_map[str(raw)]
                if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
                    raise ValueError(f"{path}: feature {i}: class_map[{str(raw)!r}] = {value!r} is not an integer")
                value = int(value)
            if not -1 <= value <= 127:
                raise ValueError(f"{path}: feature {i} has the class {value}, outside [-1, 127]")
        else:
            ok = isinstance(raw, (int, float, np.integer, np.floating)) and not isinstance(raw, bool)
            with np.errstate(over="ignore"):
                ok = ok and bool(np.isfinite(np.float32(raw)))
            if not ok:
                raise ValueError(f"{path}: feature {i} has the regression value {raw!r}, which is not a finite float32")
            value = float(raw)
        date = None
        if date_property is not None:
            if date_property not in props:
                raise ValueError(f"{path}: feature {i} has no property {date_property!r}")
            date = str(props[date_property])
        out.append(Feature(i, value, rings, date))
    return out


# ---- features -> fixed-point edges ------------------------------------------------------------------------------------------------------------
def _crs(c) -> crsmod.Crs:
    if isinstance(c, crsmod.Crs):
        return c
    if isinstance(c, str):
        return crsmod.parse(c)
    return crsmod.from_epsg(c)


def _check_grid(grid) -> Tuple[float, float, float, float]:
    g = tuple(float(v) for v in grid)
    if len(g) != 4 or not np.isfinite(g).all() or g[2] <= 0 or g[3] <= 0:
        raise ValueError(f"a grid is (X0, Y0, sx, sy) with finite values and positive pixel sizes (got {grid!r})")
    return g


def to_fixed(features: Sequence, shape: Tuple[int, int], grid, crs, src_crs=4326, stats: Optional[Dict[str, int]] = None,
             all_touched: bool = False):
    """``features`` (anything with ``.rings`` and ``.value``; map coordinates in ``src_crs``) on the grid ``grid`` = (X0, Y0, sx, sy) of
    ``crs`` with ``shape`` = (H, W) -> [(value, edges (E, 4) int32 {x0, y0, x1, y1})] in file order, in the fixed point of the rule.
    A feature whose bounding box cannot hold a pixel centre of the raster (with ``all_touched``: cannot meet the inside of a pixel) is
    dropped (``stats["outside"]``), as is one with fewer than
    three distinct vertices (``stats["degenerate"]``).  A vertex beyond the fixed-point limit, or outside the domain of the projection,
    raises the ValueError of :func:`zonal.quantise`, naming the feature."""
    H, W = int(shape[0]), int(shape[1])
    X0, Y0, sx, sy = _check_grid(grid)
    dst, src = _crs(crs), _crs(src_crs)
    stats = stats if stats is not None else {}
    stats.setdefault("outside", 0)
    stats.setdefault("degenerate", 0)
    items = []
    for k, feat in enumerate(features):
        parts = []
        for ring in feat.rings:
            a = np.asarray(ring, dtype=np.float64).reshape(-1, 2)
            if len(a) == 0:
                continue
            x, y = crsmod.transform(src, dst, a[:, 0], a[:, 1])
            try:
                parts.append(zonal.quantise(np.stack([(x - X0) / sx, (Y0 - y) / sy], axis=1)))
            except ValueError as e:
                raise ValueError(f"feature {getattr(feat, 'index', k)}: {e}") from None
        if not parts or len(np.unique(np.concatenate(parts), axis=0)) < 3:
            stats["degenerate"] += 1
            continue
        edges = np.concatenate([zonal.ring_edges(q) for q in parts])
        if _rect(edges, H, W, all_touched) is None:
            stats["outside"] += 1
            continue
        items.append((feat.value, np.ascontiguousarray(edges, dtype=np.int32)))
    return items


def _ceil_px(v: int) -> int:
    return -((HALF - int(v)) // Q)  # ceil((v - 128) / 256)


def _rect(edges: np.ndarray, H: int, W: int, all_touched: bool = False) -> Optional[Tuple[int, int, int, int]]:
    """The pixels that closed rings with these edges can contain, clipped to the raster -> (r0, c0, Hp, Wp), or None for none.  Row r is
    crossed only if ymin <= 256 r + 128 < ymax; a pixel in column c is inside only if xmin <= 256 c + 128 < xmax (a crossing lies at or
    left of it and, the crossings of a row being even in number, another one right of it).  ``all_touched``: the pixels whose open
    square the bounding box meets, rows floor(ymin / 256) .. ceil(ymax / 256) - 1 and the same for columns: they hold every touched
    pixel and every centre above."""
    if len(edges) == 0:
        return None
    xmin, ymin = int(edges[:, 0].min()), int(edges[:, 1].min())
    xmax, ymax = int(edges[:, 0].max()), int(edges[:, 1].max())
    if all_touched:
        r0, r1 = max(0, ymin // Q), min(H - 1, -((-ymax) // Q) - 1)
        c0, c1 = max(0, xmin // Q), min(W - 1, -((-xmax) // Q) - 1)
    else:
        r0, r1 = max(0, _ceil_px(ymin)), min(H - 1, (ymax - HALF - 1) // Q)
        c0, c1 = max(0, _ceil_px(xmin)), min(W - 1, (xmax - HALF - 1) // Q)
    if r1 < r0 or c1 < c0:
        return None
    return r0, c0, r1 - r0 + 1, c1 - c0 + 1


def _check_items(items, dtype: str) -> None:
    for value, edges in items:
        if not (isinstance(edges, np.ndarray) and edges.dtype == np.int32 and edges.ndim == 2 and edges.shape[1] == 4):
            raise ValueError("edges must be (E, 4) int32 (to_fixed)")
        if len(edges) and np.abs(edges.astype(np.int64)).max() > zonal.COORD_LIMIT:
            raise ValueError("an edge lies beyond 2^29 fixed-point units of the raster's origin")
        if dtype == "int8" and not (isinstance(value, (int, np.integer)) and not isinstance(value, bool) and -1 <= int(value) <= 127):
            raise ValueError(f"a seg burn value is an int in [-1, 127] (got {value!r})")


def _passes(items, H: int, W: int, all_touched: bool = False):
    """-> [(first item, items of the pass, rect)] for the passes of 64 features, in order, that can touch the raster."""
    out = []
    for first in range(0, len(items), PASS):
        part = items[first : first + PASS]
        edges = [e for _, e in part if len(e)]
        rect = _rect(np.concatenate(edges), H, W, all_touched) if edges else None
        if rect is not None:
            out.append((first, part, rect))
    return out


# ---- the rule on host arrays ----------------------------------------------------------------------------------------------------------------
def _inside_host(edges: np.ndarray, H: int, W: int, all_touched: bool = False):
    """One feature's inside mask by the rule, in int64: -> (r0, c0, mask (Hp, Wp) bool) over its own rectangle, or None.
    ``all_touched``: OR the pixels its edges touch (:func:`zonal.touch_spans`), over the rectangle that bounds those too."""
    rect = _rect(edges, H, W, all_touched)
    if rect is None:
        return None
    r0, c0, Hp, Wp = rect
    x0, y0, x1, y1 = (edges[:, k].astype(np.int64) for k in range(4))
    lo = np.maximum(-((HALF - np.minimum(y0, y1)) // Q), r0)  # the rows with min(y0, y1) <= Yc < max(y0, y1), inside the rectangle
    hi = np.minimum((np.maximum(y0, y1) - HALF - 1) // Q, r0 + Hp - 1)
    n = np.maximum(hi - lo + 1, 0)
    first = np.cumsum(n) - n
    e = np.repeat(np.arange(len(edges)), n)
    r = lo[e] + (np.arange(int(n.sum())) - first[e])
    yc = Q * r + HALF
    den = y1[e] - y0[e]
    num = (x0[e] - HALF) * den + (x1[e] - x0[e]) * (yc - y0[e])  # |num| < 2^61
    num = np.where(den < 0, -num, num)
    den = np.abs(den) * Q
    c = np.maximum(-((-num) // den), c0)  # the first column with xc <= Xc; left of the rectangle only where that is column 0
    keep = c < c0 + Wp
    toggles = np.zeros((Hp, Wp), dtype=np.uint8)
    np.bitwise_xor.at(toggles, (r[keep] - r0, c[keep] - c0), np.uint8(1))
    mask = np.bitwise_xor.accumulate(toggles, axis=1).astype(bool)
    if all_touched:
        mask |= zonal.touched_mask(edges, H, W, rect)
    return r0, c0, mask


def _burn_host(raster: np.ndarray, items, stats: Dict[str, int], all_touched: bool = False) -> None:
    H, W = raster.shape
    for _, part, (r0, c0, Hp, Wp) in _passes(items, H, W, all_touched):
        touched = np.zeros((Hp, Wp), dtype=bool)  # the pixels the pass writes: what ig_burn_resolve counts
        for value, edges in part:
            got = _inside_host(edges, H, W, all_touched)
            if got is None:
                continue
            fr, fc, mask = got
            view = raster[fr : fr + mask.shape[0], fc : fc + mask.shape[1]]
            view[mask] = value
            touched[fr - r0 : fr - r0 + mask.shape[0], fc - c0 : fc - c0 + mask.shape[1]] |= mask
        stats["passes"] += 1
        stats["pixels_written"] += int(touched.sum())


def _burn_device(raster, items, stats: Dict[str, int], all_touched: bool = False) -> None:
    import torch

    from . import ops

    H, W = raster.shape
    passes = _passes(items, H, W, all_touched)
    if not passes:
        return
    dev = raster.device
    np_dtype = np.int8 if raster.dtype == torch.int8 else np.float32
    tables = np.zeros((len(passes), PASS), dtype=np_dtype)
    edge_parts, bit_parts, spans = [], [], []
    at = 0
    for p, (_, part, (r0, c0, Hp, Wp)) in enumerate(passes):
        n = 0
        for b, (value, edges) in enumerate(part):
            tables[p, b] = value
            edge_parts.append(edges - np.array([Q * c0, Q * r0, Q * c0, Q * r0], dtype=np.int32))  # whole pixels: exact
            bit_parts.append(np.full(len(edges), b, dtype=np.uint8))
            n += len(edges)
        spans.append((at, at + n))
        at += n
    all_edges = np.ascontiguousarray(np.concatenate(edge_parts), dtype=np.int32)
    if np.abs(all_edges.astype(np.int64)).max() > zonal.COORD_LIMIT:
        raise ValueError("an edge lies beyond 2^29 fixed-point units of its pass rectangle")
    e_dev = torch.from_numpy(all_edges).to(dev)
    b_dev = torch.from_numpy(np.concatenate(bit_parts)).to(dev)
    t_dev = torch.from_numpy(tables).to(dev)
    scratch = torch.empty(max(r[2] * r[3] for _, _, r in passes), dtype=torch.int64, device=dev)  # one canvas, reused
    scratch2 = torch.empty_like(scratch) if all_touched else None  # the canvas of touched bits
    written = torch.zeros(1, dtype=torch.int64, device=dev)
    for p, (_, _, (r0, c0, Hp, Wp)) in enumerate(passes):
        a, b = spans[p]
        canvas = zonal.toggle_canvas(e_dev[a:b], b_dev[a:b], Hp, Wp, all_touched, scratch, scratch2)
        stats["passes"] += 1  # also a pass that crosses and touches no row
        if canvas is not None:
            ops.burn_resolve(canvas, t_dev[p], raster, r0, c0, written)
    stats["pixels_written"] += int(written.item())


def burn_fixed(raster, items, stats: Optional[Dict[str, int]] = None, all_touched: bool = False):
    """Burn ``items`` = [(value, edges)] (:func:`to_fixed`: closed rings in the raster's fixed point), in order, into ``raster`` (H, W)
    int8 | float32 IN PLACE by the rule of the module docstring -> ``raster``.  A tensor on the device goes through the kernels (it may be
    a view with any row pitch), a numpy array through the twin.  ``stats`` gains ``passes`` (those that can touch the raster) and
    ``pixels_written`` (per pass, the pixels inside at least one of its features, summed over the passes).  ``all_touched``: a feature
    also holds the pixels its edges touch (module docstring)."""
    stats = stats if stats is not None else {}
    stats.setdefault("passes", 0)
    stats.setdefault("pixels_written", 0)
    name = str(raster.dtype).replace("torch.", "")
    if name not in ("int8", "float32") or len(raster.shape) != 2:
        raise ValueError(f"a label raster is (H, W) int8 or float32 (got {name} {tuple(raster.shape)})")
    if int(raster.shape[0]) * int(raster.shape[1]) > MAX_PIXELS:
        raise ValueError(f"a raster of {raster.shape[0]} x {raster.shape[1]} pixels is beyond 2^31 - 1: burn it in row bands")
    _check_items(items, name)
    if isinstance(raster, np.ndarray):
        _burn_host(raster, items, stats, bool(all_touched))
    elif prep.is_device(raster):
        _burn_device(raster, items, stats, bool(all_touched))
    else:
        raise ValueError("burn_fixed takes a numpy array (host) or a tensor on the device")
    return raster


def _background(background, dtype: str):
    if dtype == "int8":
        background = 0 if background is None else background
        if isinstance(background, bool) or not isinstance(background, (int, np.integer)) or not -1 <= int(background) <= 127:
            raise ValueError(f"a seg background is an int in [-1, 127] (got {background!r})")
        return int(background)
    background = float("nan") if background is None else background
    if isinstance(background, bool) or not isinstance(background, (int, float, np.integer, np.floating)):
        raise ValueError(f"a reg background is a number or NaN (got {background!r})")
    return float(background)


def _new_raster(shape, dtype: str, value, device):
    if device is None:
        return np.full(shape, value, dtype=np.dtype(dtype))
    import torch

    return torch.full(tuple(shape), value, dtype=torch.int8 if dtype == "int8" else torch.float32, device=device)


def _dtype(dtype) -> str:
    name = str(dtype).replace("torch.", "")
    name = TASKS.get(name, name)
    if name not in ("int8", "float32"):
        raise ValueError(f"dtype must be int8 (seg) or float32 (reg) (got {dtype!r})")
    return name


def burn(features: Sequence, shape: Tuple[int, int], grid, crs, *, src_crs=4326, dtype, background=None, labelled_area: Optional[Sequence] = None,
         device: Optional[str] = None, stats: Optional[Dict[str, int]] = None, all_touched: bool = False):
    """``features`` (:func:`read_features`; coordinates in EPSG:``src_crs``) burned onto the (H, W) = ``shape`` raster of ``grid`` =
    (X0, Y0, sx, sy) in ``crs`` (an EPSG code, ``"EPSG:n"`` or a :class:`crs.Crs`) -> the raster, ``dtype`` int8 | float32: a numpy
    array with ``device=None``, a tensor on ``device`` otherwise; the same bytes either way.  ``background``: what a pixel in no feature
    holds (default 0 / NaN); ``labelled_area``: features (only their rings count) outside which a pixel holds the ignore value instead.
    ``stats`` gains ``outside``, ``degenerate`` (of ``features``), ``passes`` and ``pixels_written`` (:func:`burn_fixed`).
    ``all_touched``: features and labelled area alike also hold the pixels their edges touch."""
    prep.check_device(device)
    name = _dtype(dtype)
    H, W = int(shape[0]), int(shape[1])
    if H < 0 or W < 0 or H * W > MAX_PIXELS:
        raise ValueError(f"a raster of {H} x {W} pixels is beyond 2^31 - 1: burn it in row bands")
    bg = _background(background, name)
    ignore = SEG_IGNORE if name == "int8" else float("nan")
    at = bool(all_touched)
    items = to_fixed(features, (H, W), grid, crs, src_crs, stats, at)
    area = None
    if labelled_area is not None:
        area = [(bg, e) for _, e in to_fixed([Feature(i, bg, f.rings) for i, f in enumerate(labelled_area)], (H, W), grid, crs, src_crs, {}, at)]
    raster = _new_raster((H, W), name, bg if area is None else ignore, device)
    return burn_fixed(raster, (area or []) + items, stats, at)


# ---- cells -------------------------------------------------------------------------------------------------------------------------------------
def label_cells(raster, S: int, K: int = 0):
    """Per S x S cell of ``raster`` (ny * S, nx * S) -> (valid (ny, nx) int64, hist (ny, nx, K) int64 or None) as numpy: the pixels that
    are not -1 (int8) / not NaN (float32) and, for int8 with K > 0, those per value in [0, K).  ``ig_label_cells`` on the device, numpy
    on the host."""
    S, K = int(S), int(K)
    H, W = (int(v) for v in raster.shape)
    if S < 1 or H % S or W % S:
        raise ValueError(f"a raster of {H} x {W} pixels is not a whole number of {S} x {S} cells")
    if not isinstance(raster, np.ndarray):
        from . import ops

        valid, hist = ops.label_cells(raster, S, K, SEG_IGNORE)
        return valid.cpu().numpy(), None if hist is None else hist.cpu().numpy()
    ny, nx = H // S, W // S
    cells = raster.reshape(ny, S, nx, S).transpose(0, 2, 1, 3).reshape(ny, nx, S * S)
    ok = ~np.isnan(cells) if raster.dtype == np.float32 else cells != SEG_IGNORE
    valid = ok.sum(axis=2).astype(np.int64)
    hist = None
    if K:
        if raster.dtype != np.int8:
            raise ValueError("a class histogram needs an int8 raster")
        hist = np.zeros((ny, nx, K), dtype=np.int64)
        for cy in range(ny):
            for cx in range(nx):
                v = cells[cy, cx].astype(np.int64)
                hist[cy, cx] = np.bincount(v[(v >= 0) & (v < K)], minlength=K)
    return valid, hist


# ---- the grid --------------------------------------------------------------------------------------------------------------------------------
def utm_epsg(lon: float, lat: float) -> int:
    """The EPSG code of the UTM zone of (longitude, latitude): 32601-32660 north of the equator (and on it), 32701-32760 south."""
    zone = min(60, max(1, int(np.floor((float(lon) + 180.0) / 6.0)) + 1))
    return (32600 if lat >= 0 else 32700) + zone


def _all_vertices(features: Sequence) -> np.ndarray:
    parts = [np.asarray(r, dtype=np.float64).reshape(-1, 2) for f in features for r in f.rings if len(r)]
    if not parts:
        raise ValueError("the features have no vertices")
    return np.concatenate(parts)


def choose_grid(features: Sequence, chip_size: int, like: Optional[str] = None, crs: Optional[int] = None, src_crs=4326,
                spatial_resolution: float = 30.0):
    """The label grid -> (crs.Crs, (X0, Y0, sx, sy), ny, nx): ny x nx cells of ``chip_size`` pixels from the top-left corner.
    ``like``: that raster's grid (coordinate system, origin, pixel sizes) and its whole-chip grid (H // S) x (W // S).  Otherwise EPSG
    ``crs`` (default: the UTM zone of the centre of the features' bounds) at ``spatial_resolution``, the origin snapped to multiples of
    the resolution, X0 = res * floor(minx / res), Y0 = res * ceil(maxy / res) (the ``snap=True`` lattice of :mod:`raster_chips`), and as
    many cells as cover the bounds of the transformed vertices."""
    S = int(chip_size)
    if like is not None:
        from . import warp

        prof = tiff.read_profile(like)
        return crsmod.from_profile(prof), warp.grid_of(prof, str(like)), int(prof["height"]) // S, int(prof["width"]) // S
    src = _crs(src_crs)
    xy = _all_vertices(features)
    if crs is None:
        lon, lat = crsmod.inverse(src, 0.5 * (xy[:, 0].min() + xy[:, 0].max()), 0.5 * (xy[:, 1].min() + xy[:, 1].max()))
        if not (np.isfinite(lon) and np.isfinite(lat)):
            raise ValueError("the centre of the features' bounds lies outside the domain of src_crs: is src_crs right?")
        crs = utm_epsg(float(lon), float(lat))
    dst = _crs(crs)
    res = float(spatial_resolution)
    if not 0 < res < np.inf:
        raise ValueError(f"spatial_resolution must be a positive number (got {spatial_resolution!r})")
    x, y = crsmod.transform(src, dst, xy[:, 0], xy[:, 1])
    if not (np.isfinite(x).all() and np.isfinite(y).all()):
        raise ValueError(f"a vertex lies outside the domain of EPSG:{dst.epsg}")
    X0, Y0 = float(res * np.floor(x.min() / res)), float(res * np.ceil(y.max() / res))
    W, H = max(1, int(np.ceil((x.max() - X0) / res))), max(1, int(np.ceil((Y0 - y.min()) / res)))
    return dst, (X0, Y0, res, res), -(-H // S), -(-W // S)


# ---- files ------------------------------------------------------------------------------------------------------------------------------------
def _row_band(items, row0: int, rows: int, W: int, all_touched: bool = False):
    """The items that can touch rows [row0, row0 + rows) of the raster, their edges moved up by row0 whole pixels (exact)."""
    if row0 == 0:
        return [(v, e) for v, e in items if _rect(e, rows, W, all_touched) is not None]
    shift = np.array([0, Q * row0, 0, Q * row0], dtype=np.int64)
    out = []
    for v, e in items:
        moved = e.astype(np.int64) - shift
        if _rect(moved, rows, W, all_touched) is None:
            continue
        if np.abs(moved).max() > zonal.COORD_LIMIT:
            raise ValueError(f"a vertex lies beyond 2^29 fixed-point units ({zonal.COORD_LIMIT // Q} pixels) of the row band at row {row0}")
        out.append((v, moved.astype(np.int32)))
    return out


def label_name(x: int, y: int, date: str) -> str:
    """The naming of :func:`raster_chips.grid_polygons`; x = the cell's column, y = its row, counted from the top-left corner."""
    return f"label_x{x}_y{y}_{date}.tif"


def create_polygon_labels(features_file: str, output_directory: str, like: Optional[str] = None, crs: Optional[int] = None, src_crs: int = 4326,
                          spatial_resolution: float = 30.0, chip_size: int = 256, task_type: str = "seg", value_property: Optional[str] = None,
                          burn_value=None, class_map: Optional[Dict[str, int]] = None, background=None, labelled_area: Optional[str] = None,
                          date: Optional[str] = None, date_property: Optional[str] = None, mgrs_tile_id: Optional[str] = None,
                          min_foreground: int = 1, device: Optional[str] = None, max_pixels: int = MAX_PIXELS,
                          all_touched: bool = False) -> List[str]:
    """The polygons of ``features_file`` (GeoJSON, EPSG:``src_crs``) -> ``labels/label_x{x}_y{y}_{date}.tif`` (int8 for ``seg``, float32
    for ``reg``, each ``chip_size`` x ``chip_size`` with the GeoKeys ``create_raster_chips`` reads), ``records.csv`` (``label_filename,
    date[, mgrs_tile_id]``: the table ``create_raster_chips`` takes) and ``polygon_labels_stats.json`` under ``output_directory`` -> the
    label names.  The grid: :func:`choose_grid`.  ``date_property``: the features are grouped by that property and every date gets its
    own rasters; otherwise ``date`` names them all.  ``labelled_area``: a GeoJSON of the ground that was labelled (module docstring).  A
    cell with fewer than ``min_foreground`` pixels that are neither the ignore value nor ``background`` is dropped; an existing file is
    not rewritten but still listed.  A raster of more than ``max_pixels`` (2^31 - 1) pixels is burned in row bands of whole cells.
    ``device``: None = the numpy path, ``"cuda"`` / ``"cuda:n"`` = the kernels; both write the same bytes.  ``all_touched``: features and
    labelled area also hold the pixels their edges touch (module docstring), so a field smaller than a pixel is still burned."""
    prep.check_device(device)
    if not isinstance(all_touched, (bool, np.bool_)):
        raise ValueError(f"all_touched must be true or false (got {all_touched!r})")
    all_touched = bool(all_touched)
    if task_type not in TASKS:
        raise ValueError(f"task_type must be seg or reg (got {task_type!r})")
    name = TASKS[task_type]
    S = chip_size
    if isinstance(S, bool) or not isinstance(S, (int, np.integer)) or not 1 <= int(S) <= MAX_SIDE:
        raise ValueError(f"chip_size must be an int in [1, 2^15] (got {chip_size!r})")
    S = int(S)
    if isinstance(min_foreground, bool) or not isinstance(min_foreground, (int, np.integer)) or min_foreground < 0:
        raise ValueError(f"min_foreground must be an int >= 0 (got {min_foreground!r})")
    if date_property is None and date in (None, ""):
        raise ValueError("create_polygon_labels needs date or date_property (the label names carry a date)")
    bg = _background(background, name)
    feats = read_features(features_file, value_property, burn_value, class_map, date_property, task_type)
    area = zonal.read_zones(labelled_area) if labelled_area is not None else None
    dst, grid, ny, nx = choose_grid(feats, S, like, crs, src_crs, spatial_resolution)
    X0, Y0, sx, sy = grid
    H, W = ny * S, nx * S
    if S * W > int(max_pixels):
        raise ValueError(f"one row of cells ({S} x {W} pixels) is beyond {int(max_pixels)} pixels")
    groups: Dict[str, List[Feature]] = {}
    for f in feats:
        groups.setdefault(f.date if date_property is not None else str(date), []).append(f)
    counts = {"outside": 0, "degenerate": 0, "passes": 0, "pixels_written": 0}
    cells = {"kept": 0, "dropped": 0, "existing": 0}
    hist_sum = np.zeros(SEG_CLASSES, dtype=np.int64) if name == "int8" else None
    K = SEG_CLASSES if name == "int8" else 0
    ignore = SEG_IGNORE if name == "int8" else float("nan")
    label_dir = os.path.join(output_directory, "labels")
    os.makedirs(label_dir, exist_ok=True)
    geo = dict(crsmod.geokeys(dst.epsg))
    geo[33550] = (12, (sx, sy, 0.0))
    names: List[str] = []
    rows_out: List[Tuple[str, str]] = []
    band_cells = max(1, int(max_pixels) // (S * W)) if ny and nx else 1
    for day, group in groups.items():
        items = to_fixed(group, (H, W), grid, dst, src_crs, counts, all_touched)
        area_items = None
        if area is not None:
            area_items = [(bg, e) for _, e in to_fixed([Feature(i, bg, z.rings) for i, z in enumerate(area)], (H, W), grid, dst, src_crs, {},
                                                       all_touched)]
        for cy0 in range(0, ny if nx else 0, band_cells):
            rows = min(band_cells, ny - cy0) * S
            band = _row_band((area_items or []) + items, cy0 * S, rows, W, all_touched)
            raster = _new_raster((rows, W), name, bg if area_items is None else ignore, device)
            burn_fixed(raster, band, counts, all_touched)
            valid, hist = label_cells(raster, S, K)
            host = raster if isinstance(raster, np.ndarray) else raster.cpu().numpy()
            for by in range(rows // S):
                for cx in range(nx):
                    cell = host[by * S : (by + 1) * S, cx * S : (cx + 1) * S]
                    if name == "int8":
                        fg = int(valid[by, cx]) - (int(hist[by, cx, bg]) if bg >= 0 else 0)
                    else:  # a finite background is compared on the host copy that is written anyway
                        fg = int(valid[by, cx]) if bg != bg else int((~np.isnan(cell) & (cell != np.float32(bg))).sum())
                    if fg < min_foreground:
                        cells["dropped"] += 1
                        continue
                    fname = label_name(cx, cy0 + by, day)
                    path = os.path.join(label_dir, fname)
                    if os.path.exists(path):
                        cells["existing"] += 1
                    else:
                        tags = dict(geo)
                        tags[33922] = (12, (0.0, 0.0, 0.0, X0 + cx * S * sx, Y0 - (cy0 + by) * S * sy, 0.0))
                        tiff.write(path, np.ascontiguousarray(cell), {"tags": tags, "nodata": None})
                    cells["kept"] += 1
                    if hist_sum is not None:
                        hist_sum += hist[by, cx]
                    names.append(fname)
                    rows_out.append((fname, day))
    with open(os.path.join(output_directory, "records.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["label_filename", "date"] + (["mgrs_tile_id"] if mgrs_tile_id else []))
        for fname, day in rows_out:
            w.writerow([fname, day] + ([mgrs_tile_id] if mgrs_tile_id else []))
    stats: Dict[str, Any] = {"features": {"read": len(feats), "outside": counts["outside"], "degenerate": counts["degenerate"]},
                             "cells": cells, "passes": counts["passes"], "pixels_written": counts["pixels_written"],
                             "grid": {"epsg": dst.epsg, "origin": [X0, Y0], "pixel_size": [sx, sy], "cells": [ny, nx], "chip_size": S},
                             "dates": list(groups)}
    if hist_sum is not None:
        stats.update(prep.class_stats(hist_sum, trim=True))
    prep.write_stats(os.path.join(output_directory, "polygon_labels_stats.json"), stats)
    return names


# ---- mode=create_polygon_labels ---------------------------------------------------------------------------------------------------------------
CONFIG_KEYS = ("features", "output_directory", "like", "crs", "src_crs", "spatial_resolution", "chip_size", "task_type", "value_property",
               "burn_value", "class_map", "background", "labelled_area", "date", "date_property", "mgrs_tile_id", "min_foreground", "device")
# keys without a default: given as ``+polygon_labels.<key>=...`` on the command line, or in a YAML config.  all_touched: true | false
# (unset = false): features and labelled area also hold the pixels their edges touch
OPTIONAL_KEYS = ("all_touched",)


def polygon_labels_options(cfg: Dict[str, Any]) -> Dict[str, Any]:
    """The ``polygon_labels.*`` keys of ``mode=create_polygon_labels`` checked -> the keyword arguments of :func:`create_polygon_labels`
    (``all_touched`` only when it is on).  An unknown key or a bad value raises ValueError; the files are required only in that mode.
    ``device``: None = the device when there is one, ``host`` = the numpy path, ``cuda`` / ``cuda:n``."""
    c = prep.Section(cfg, "polygon_labels", CONFIG_KEYS + OPTIONAL_KEYS)
    size = c.integer("chip_size", 256, lo=1, hi=MAX_SIDE, what="must be an int in [1, 2^15]")
    task = c.choice("task_type", "seg", TASKS, "must be seg or reg")
    res = c.number("spatial_resolution", 30.0, lambda x: 0 < x < np.inf, "must be a positive number")
    fgmin = c.integer("min_foreground", 1, lo=0, what="must be an int >= 0")
    cmap = c.get("class_map")
    if cmap is not None:
        if not isinstance(cmap, dict) or not all(prep.is_int(v) and -1 <= v <= 127 for v in cmap.values()):
            raise c.bad("class_map", "must map names to classes in [-1, 127]", cmap)
        cmap = {str(k): int(v) for k, v in cmap.items()}
    bg = c.get("background")
    bg = float("nan") if isinstance(bg, str) and bg.lower() in ("nan", ".nan") else bg
    _background(bg, TASKS[task])
    bv = c.get("burn_value")
    if bv is not None and (isinstance(bv, bool) or not isinstance(bv, (int, float))):
        raise c.bad("burn_value", "must be a number", bv)
    if bv is not None and c.text("value_property") is not None:
        raise ValueError("polygon_labels.value_property and polygon_labels.burn_value exclude each other")
    dev = c.text("device")
    if dev is not None and dev != "host" and not dev.startswith("cuda"):
        raise c.bad("device", "must be None, host or a cuda device", dev)
    opts = dict(features_file=c.text("features"), output_directory=c.text("output_directory"), like=c.text("like"), crs=c.epsg("crs", None),
                src_crs=c.epsg("src_crs", 4326), spatial_resolution=res, chip_size=size, task_type=task,
                value_property=c.text("value_property"), burn_value=bv, class_map=cmap, background=bg, labelled_area=c.text("labelled_area"),
                date=c.text("date"), date_property=c.text("date_property"), mgrs_tile_id=c.text("mgrs_tile_id"), min_foreground=fgmin, device=dev)
    if c.flag("all_touched"):
        opts["all_touched"] = True
    if cfg.get("mode") == "create_polygon_labels":
        if opts["features_file"] is None or opts["output_directory"] is None:
            raise ValueError("mode=create_polygon_labels needs polygon_labels.features and polygon_labels.output_directory")
        if opts["date"] is None and opts["date_property"] is None:
            raise ValueError("mode=create_polygon_labels needs polygon_labels.date or polygon_labels.date_property")
    return opts


def run_from_config(cfg: Dict[str, Any], device: Optional[str] = None) -> int:
    """``mode=create_polygon_labels``: :func:`create_polygon_labels` under the ``polygon_labels.*`` keys; prints one JSON line with the
    counts.  ``device``: what ``polygon_labels.device=None`` stands for."""
    kw = polygon_labels_options(cfg)
    kw["device"] = device if kw["device"] is None else (None if kw["device"] == "host" else kw["device"])
    names = create_polygon_labels(**kw)
    with open(os.path.join(kw["output_directory"], "polygon_labels_stats.json")) as f:
        stats = json.load(f)
    print(json.dumps({"create_polygon_labels": {"labels": len(names), "dropped": stats["cells"]["dropped"], "features": stats["features"],
                                                "output_directory": kw["output_directory"]}}))
    return 0


def main(argv: Optional[List[str]] = None) -> int:
    """``python -m instageo_amd.polygon_labels polygon_labels.features=parcels.geojson polygon_labels.output_directory=out ...``:
    mode=create_polygon_labels without ``run.py``."""
    return prep.run_mode_cli("create_polygon_labels", run_from_config, argv)


if __name__ == "__main__":
    raise SystemExit(main())
