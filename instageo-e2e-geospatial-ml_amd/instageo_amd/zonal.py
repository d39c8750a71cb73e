"""Zonal statistics: the user's polygons (administrative units, parcels, catchments) rasterised onto a class map on the device and
tallied per zone and class (not in the reference; ``csrc/zonal.hip``).  The inverse of :mod:`instageo_amd.vectorize`,
in its coordinates.

Rule.  Pixel (r, c) covers [c, c+1] x [r, r+1] in lattice (x, y), y down.  Zone vertices are quantised to Q = 256 units per pixel,
``X = floor(x * 256 + 0.5)``, in float64 on the host; the pixel centre is (256 c + 128, 256 r + 128).  A zone is a set of closed rings
(exteriors and holes of a ``Polygon`` or ``MultiPolygon``, any orientation); a pixel is inside iff an odd number of the zone's edges
cross its row's centre line at or left of its centre (even-odd on pixel centres: GDAL and rasterio without ``all_touched``; the two
inequalities that decide every tie: ``include/instageo_hip.h``).  Zones are independent: a pixel inside several zones counts in each
of them, as rasterstats does.  Everything on the device is integer and unique: two runs give the same bits.

Values.  The same masks also summarise float32 rasters (regression predictions, probabilities, uncertainty, Sentinel-1 dB scenes,
composites): :func:`zone_values` gives per zone and band the count, sum, mean, population std, min and max of the values that are finite
and not the no-data value, and ``mode=zonal_stats`` (:func:`run_from_config`) does it from a GeoTIFF and a GeoJSON to a CSV.  The
variance comes from merged (n, sum, M2) triples in a fixed order, float64 (``include/instageo_hip.h``): no sum of squares, no atomics,
the same bits from run to run.

Order statistics.  :func:`zone_quantiles` gives the median and any percentiles of the same valid values: the device selects, per zone,
band and percentile, the two neighbouring order statistics by a radix selection on order-preserving keys (integer atomics only, exact,
the same bits from run to run) and the host interpolates between them in float64 as numpy's default ``linear`` method does
(``include/instageo_hip.h``).  :func:`zone_quantiles_host` is the numpy twin of the rule.  ``zonal_stats.percentiles`` adds them to the CSV.

all_touched.  Every function that takes zones also takes ``all_touched`` (default off): a pixel then belongs to a zone iff its centre is
inside OR one of the zone's edges touches it, i.e. the closed edge meets the pixel's OPEN square (``include/instageo_hip.h``).  A parcel
smaller than a pixel then still has pixels.  The square is open so that an edge along a pixel border touches neither side: polygons on the
pixel lattice (those of :mod:`instageo_amd.vectorize`) select the same pixels under both rules.  :func:`touch_spans` and
:func:`touched_mask` are the numpy twin of the rule.  It is expected to match rasterio's ``all_touched=True`` for vertices in general
position; that has not been verified.

Out of scope: lines and points (under the open-square rule a line along a pixel border burns nothing: they need a rule of their own),
``majority`` / ``minority`` / ``unique``, percentiles in ``test.zones`` of the inference modes, rotated or
sheared geotransforms, one table merged across chips or tiles, zone rasters written as TIFF.
"""
from __future__ import annotations

import csv
import json
import os
from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import crs as crsmod
from . import ops, prep, tiff
from .postprocess import georeference

Q = 256  # fixed-point units per pixel
COORD_LIMIT = 2**29  # |X|, |Y| of a quantised vertex


class Zone(NamedTuple):
    id: Any  # the feature's ``id_property``, else its index in the collection
    rings: List[np.ndarray]  # (n, 2) float64 (x, y) each, not closed (the first vertex is not repeated)


def check_zone_options(zones: Optional[str] = None, regression: bool = False) -> None:
    """ValueError for ``zones`` with a regression head (it has no class map) or a path that is no file.  ``None`` is off.  Touches no
    model or device."""
    if zones is None:
        return
    if regression:
        raise ValueError("zones needs a class map (a regression head has one output channel)")
    if not os.path.isfile(str(zones)):
        raise ValueError(f"zones: {str(zones)!r} is not a file (a GeoJSON FeatureCollection of Polygon / MultiPolygon features)")


def read_collection(path: str, id_property: Optional[str] = None):
    """One pass over a GeoJSON FeatureCollection: the file is opened and parsed once -> (index, properties, rings) per feature, in file
    order.  ``Polygon`` and ``MultiPolygon`` geometries are accepted (all their rings, exteriors and holes alike); anything else raises
    ValueError naming the feature, by its ``id_property`` when one is given (a feature without it raises too).  A ring's closing
    duplicate vertex is dropped; a third coordinate (height) is ignored."""
    with open(path) as f:
        doc = json.load(f)
    if not isinstance(doc, dict) or doc.get("type") != "FeatureCollection" or not isinstance(doc.get("features"), list):
        raise ValueError(f"{path}: not a GeoJSON FeatureCollection")
    for i, feat in enumerate(doc["features"]):
        props = (feat.get("properties") if isinstance(feat, dict) else None) or {}
        zid = i
        if id_property is not None:
            if id_property not in props:
                raise ValueError(f"{path}: feature {i} has no property {id_property!r}")
            zid = props[id_property]
        geom = (feat.get("geometry") if isinstance(feat, dict) else None) or {}
        kind = geom.get("type")
        if kind == "Polygon":
            polys = [geom.get("coordinates")]
        elif kind == "MultiPolygon":
            polys = geom.get("coordinates")
        else:
            raise ValueError(f"{path}: feature {i} (id {zid!r}) has geometry {kind!r}; zones are Polygon or MultiPolygon")
        rings = []
        try:
            for poly in polys:
                for ring in poly:
                    a = np.array([(p[0], p[1]) for p in ring], dtype=np.float64).reshape(-1, 2)
                    if len(a) > 1 and (a[0] == a[-1]).all():
                        a = a[:-1]
                    if len(a):
                        rings.append(a)
        except (TypeError, IndexError, ValueError) as e:
            raise ValueError(f"{path}: feature {i} (id {zid!r}) has malformed coordinates") from e
        yield i, props, rings


def read_zones(path: str, id_property: Optional[str] = None) -> List[Zone]:
    """Read a GeoJSON FeatureCollection -> one :class:`Zone` per feature, in file order, its id the feature's ``id_property`` or its
    index (:func:`read_collection` reads the geometries)."""
    return [Zone(i if id_property is None else props[id_property], rings) for i, props, rings in read_collection(path, id_property)]


def quantise(xy: np.ndarray) -> np.ndarray:
    """Lattice (x, y) float64 -> int32 fixed point, ``floor(v * 256 + 0.5)``; ValueError beyond ``|v| <= 2^29`` units (or not finite)."""
    q = np.floor(np.asarray(xy, dtype=np.float64) * Q + 0.5)
    if not (np.isfinite(q).all() and (np.abs(q) <= COORD_LIMIT).all()):
        raise ValueError(f"a zone vertex lies beyond 2^29 fixed-point units ({COORD_LIMIT // Q} pixels) of the raster's origin, or is not "
                         "finite: are the zones in the raster's coordinate system?")
    return q.astype(np.int32)


def ring_edges(q: np.ndarray) -> np.ndarray:
    """The closed, directed edges of a ring of vertices ``q`` (n, 2) -> (n, 4) {x0, y0, x1, y1}: one per vertex, the last one closes it."""
    return np.concatenate([q, np.roll(q, -1, axis=0)], axis=1)


def zones_to_pixels(zones: Sequence[Zone], profile: Optional[Dict[str, Any]] = None) -> Tuple[np.ndarray, np.ndarray]:
    """The directed edges of all zones in the raster's fixed-point lattice -> (edges (E, 4) int32 {x0, y0, x1, y1}, edge_zone (E,)
    int32 = the index of each edge's zone in ``zones``).  With a georeferenced ``profile`` (:func:`postprocess.georeference`) the
    coordinates are map coordinates and go through the inverse of the transform :func:`vectorize.write_geojson` writes with,
    ``X = (x - tie_x) / scale_x + tie_i``, ``Y = (tie_y - y) / scale_y + tie_j`` (north-up rasters); without one they are lattice
    coordinates already.  Then :func:`quantise`.  A ring contributes one edge per vertex (the last one closes it)."""
    geo = georeference(profile)
    parts, owner = [], []
    for z, zone in enumerate(zones):
        for ring in zone.rings:
            a = np.asarray(ring, dtype=np.float64).reshape(-1, 2)
            if len(a) == 0:
                continue
            if geo:
                sx, sy, ti, tj, tx, ty = geo
                a = np.stack([(a[:, 0] - tx) / sx + ti, (ty - a[:, 1]) / sy + tj], axis=1)
            try:
                q = quantise(a)
            except ValueError as e:
                raise ValueError(f"zone {z} (id {zone.id!r}): {e}") from None
            parts.append(ring_edges(q))
            owner.append(np.full(len(q), z, dtype=np.int32))
    if not parts:
        return np.zeros((0, 4), dtype=np.int32), np.zeros(0, dtype=np.int32)
    return np.concatenate(parts), np.concatenate(owner)


def _check_edges(edges: np.ndarray, edge_zone: np.ndarray, Z: int) -> Tuple[np.ndarray, np.ndarray]:
    edges, edge_zone = np.asarray(edges), np.asarray(edge_zone)
    if edges.dtype != np.int32 or edges.ndim != 2 or edges.shape[1] != 4 or edge_zone.shape != (len(edges),):
        raise ValueError("edges must be (E, 4) int32 with one zone index per edge (zones_to_pixels)")
    if len(edges) and (np.abs(edges.astype(np.int64)).max() > COORD_LIMIT or edge_zone.min() < 0 or edge_zone.max() >= Z):
        raise ValueError("an edge lies beyond 2^29 fixed-point units or names a zone outside [0, Z)")
    return edges, edge_zone.astype(np.int64)


def _touch_row_span(ymin: np.ndarray, ymax: np.ndarray, H: int) -> Tuple[np.ndarray, np.ndarray]:
    """The all_touched rows of edges with ordinates ``ymin`` <= ``ymax`` (int64): floor(ymin / 256) .. ceil(ymax / 256) - 1 in [0, H) ->
    (the first row, their number, 0 where there is none)."""
    lo = np.maximum(ymin // Q, 0)
    hi = np.minimum(-((-ymax) // Q) - 1, H - 1)
    return lo, np.maximum(hi - lo + 1, 0)


def touch_spans(edges: np.ndarray, H: int, W: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """The numpy twin of the all_touched span rule (``include/instageo_hip.h``), in int64: ``edges`` (E, 4) {x0, y0, x1, y1} -> (edge,
    row, first column, last column) of every (edge, touched row) pair whose span holds a column of the (H, W) raster.  Rows:
    floor(ymin / 256) .. ceil(ymax / 256) - 1 in [0, H); columns: floor(lo / 256) .. ceil(hi / 256) - 1 in [0, W) with lo / hi the
    abscissae at the two ends of the edge's part inside the row, exact rationals over abs(y1 - y0) (a horizontal edge: its own ends)."""
    H, W = int(H), int(W)
    x0, y0, x1, y1 = (np.asarray(edges)[:, k].astype(np.int64) for k in range(4))
    ymin, ymax = np.minimum(y0, y1), np.maximum(y0, y1)
    lo, n = _touch_row_span(ymin, ymax, H)
    first = np.cumsum(n) - n
    e = np.repeat(np.arange(len(n)), n)
    r = lo[e] + (np.arange(int(n.sum())) - first[e])
    den = y1[e] - y0[e]
    flat = den == 0
    ya, yb = np.maximum(ymin[e], Q * r), np.minimum(ymax[e], Q * r + Q)
    a = np.where(flat, x0[e], x0[e] * den + (x1[e] - x0[e]) * (ya - y0[e]))  # |a|, |b| < 2^61
    b = np.where(flat, x1[e], x0[e] * den + (x1[e] - x0[e]) * (yb - y0[e]))
    a, b = np.where(den < 0, -a, a), np.where(den < 0, -b, b)
    den = np.where(flat, 1, np.abs(den)) * Q
    c0 = np.maximum(np.minimum(a, b) // den, 0)
    c1 = np.minimum(-((-np.maximum(a, b)) // den) - 1, W - 1)
    keep = c1 >= c0
    return e[keep], r[keep], c0[keep], c1[keep]


def touch_rows(edges: np.ndarray, H: int) -> np.ndarray:
    """-> (E,) int64: the rows in [0, H) each edge touches, what ``ig_zone_touch_rows`` counts (a row counts whatever its columns are)."""
    y0, y1 = (np.asarray(edges)[:, k].astype(np.int64) for k in (1, 3))
    return _touch_row_span(np.minimum(y0, y1), np.maximum(y0, y1), int(H))[1]


def touched_mask(edges: np.ndarray, H: int, W: int, rect: Optional[Tuple[int, int, int, int]] = None) -> np.ndarray:
    """-> (H, W) bool: the pixels of the (H, W) raster at least one of ``edges`` touches (:func:`touch_spans` painted: +1 at a span's
    first column, -1 after its last, summed along the row).  ``rect`` = (r0, c0, Hp, Wp): only that rectangle of the raster, (Hp, Wp)."""
    r0, c0, Hp, Wp = (0, 0, int(H), int(W)) if rect is None else rect
    _, r, a, b = touch_spans(edges, H, W)
    a, b = np.maximum(a, c0), np.minimum(b, c0 + Wp - 1)
    keep = (r >= r0) & (r < r0 + Hp) & (b >= a)
    steps = np.zeros((Hp, Wp + 1), dtype=np.int64)
    np.add.at(steps, (r[keep] - r0, a[keep] - c0), 1)
    np.add.at(steps, (r[keep] - r0, b[keep] - c0 + 1), -1)
    return np.cumsum(steps, axis=1)[:, :Wp] > 0


def toggle_canvas(e: torch.Tensor, bit: torch.Tensor, H: int, W: int, all_touched: bool = False, canvas: Optional[torch.Tensor] = None,
                  touch: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """One pass, for zonal statistics and label burning alike: the edges ``e`` (E, 4) int32 of up to 64 zones on the device, bit ``bit``
    (E,) uint8 each -> the (H, W) int64 canvas of their toggles (rows counted, scanned, toggled; not yet prefix-XORed), or None when no
    edge crosses a row (a pass without a crossing has no inside pixel: nothing more is launched).  ``all_touched``: the touched pixels go
    onto a second canvas and are merged into the toggles (``ig_zone_touch_rows``, ``ig_zone_touch``, ``ig_zone_touch_merge``); None then
    only if no edge touches a row either.  ``canvas`` / ``touch``: flat int64 scratch of at least H * W elements to build them in (their
    first H * W elements are zeroed and used); without them fresh memory.  Two host reads: the crossed and the touched rows."""
    rows = ops.zone_edge_rows(e, H)
    first = torch.cumsum(rows, 0, dtype=torch.int64).sub_(rows)
    T = int(rows.sum(dtype=torch.int64).item())
    TT = 0
    if all_touched:
        trows = ops.zone_touch_rows(e, H)
        TT = int(trows.sum(dtype=torch.int64).item())
    if T == 0 and TT == 0:
        return None

    def zeroed(scratch):
        if scratch is None:
            return torch.zeros((H, W), dtype=torch.int64, device=e.device)
        return scratch[: H * W].view(H, W).zero_()

    canvas = zeroed(canvas)
    ops.zone_toggle(e, bit, first, canvas, T)
    if TT:
        touch = zeroed(touch)
        ops.zone_touch(e, bit, torch.cumsum(trows, 0, dtype=torch.int64).sub_(trows), touch, TT)
        ops.zone_touch_merge(canvas, touch)
    return canvas


def _passes(edges: np.ndarray, edge_zone: np.ndarray, Z: int, H: int, W: int, device, all_touched: bool = False):
    """Yield (pass, canvas) for those of the ceil(Z / 64) passes whose zones cross a row of the raster at all: the (H, W) int64 canvas
    holds their toggles, bit ``zone % 64`` each (:func:`toggle_canvas`, which also says what ``all_touched`` adds and when a pass is
    skipped)."""
    edges, edge_zone = _check_edges(edges, edge_zone, Z)
    if len(edges) == 0 or H * W == 0:
        return
    for p in range((Z + ops.ZONE_BITS - 1) // ops.ZONE_BITS):
        sel = (edge_zone // ops.ZONE_BITS) == p
        if not sel.any():
            continue
        e = torch.from_numpy(np.ascontiguousarray(edges[sel])).to(device)
        bit = torch.from_numpy((edge_zone[sel] % ops.ZONE_BITS).astype(np.uint8)).to(device)
        canvas = toggle_canvas(e, bit, H, W, all_touched)
        if canvas is not None:
            yield p, canvas


def zone_masks(edges: np.ndarray, edge_zone: np.ndarray, Z: int, H: int, W: int, device="cuda", all_touched: bool = False) -> torch.Tensor:
    """-> (ceil(Z / 64), H, W) int64 bit planes on the device: bit ``z % 64`` of plane ``z // 64`` at (r, c) = pixel (r, c) is inside
    zone z (bit 63 is the sign bit).  ``edges`` / ``edge_zone`` are those of :func:`zones_to_pixels`.  ``all_touched``: also the pixels
    the zone's edges touch (module docstring); the same in every function below."""
    Z, H, W = int(Z), int(H), int(W)
    planes = torch.zeros(((Z + ops.ZONE_BITS - 1) // ops.ZONE_BITS, H, W), dtype=torch.int64, device=device)
    for p, canvas in _passes(edges, edge_zone, Z, H, W, device, all_touched):
        ops.zone_tally(canvas, None, None, write_mask=True)
        planes[p] = canvas
    return planes


def zone_counts(classmap: torch.Tensor, edges: np.ndarray, edge_zone: np.ndarray, Z: int, ncls: int, fill: int = -1,
                all_touched: bool = False) -> np.ndarray:
    """Pixels per zone and class of one (H, W) int8 class map on the device -> (Z, ncls + 1) int64 numpy: ``[z][k]`` = the pixels of
    class k inside zone z for k < ncls, ``[z][ncls]`` = its pixels that are ``fill`` or lie outside [0, ncls).  2 <= ncls <= 127."""
    if classmap.dtype != torch.int8 or classmap.dim() != 2:
        raise ValueError("zone_counts takes one (H, W) int8 class map")
    if not 2 <= int(ncls) <= 127:
        raise ValueError(f"zone_counts: 2 <= ncls <= 127 (got {ncls})")
    Z, ncls = int(Z), int(ncls)
    H, W = classmap.shape
    cm = classmap.contiguous()
    out = np.zeros((Z, ncls + 1), dtype=np.int64)
    for p, canvas in _passes(edges, edge_zone, Z, H, W, cm.device, all_touched):
        counts = torch.zeros((ops.ZONE_BITS, ncls + 1), dtype=torch.int64, device=cm.device)
        ops.zone_tally(canvas, cm, counts, ncls, fill)
        lo = p * ops.ZONE_BITS
        out[lo:lo + ops.ZONE_BITS] = counts[: min(ops.ZONE_BITS, Z - lo)].cpu().numpy()
    return out


def write_zone_csv(path: str, ids: Sequence[Any], counts: np.ndarray, profile: Optional[Dict[str, Any]] = None) -> str:
    """Write one row per zone: ``zone`` (its index), ``id``, ``pixels`` (all its inside pixels), ``invalid`` (those that are fill or no
    class), ``count_<k>`` per class and, with a georeferenced ``profile``, ``area_map_<k>`` = count * scale_x * scale_y in squared map
    units.  Floats are written with ``repr`` (they read back exactly)."""
    counts = np.asarray(counts)
    if counts.ndim != 2 or counts.shape[0] != len(ids) or counts.shape[1] < 2:
        raise ValueError("counts must be (len(ids), ncls + 1)")
    ncls = counts.shape[1] - 1
    geo = georeference(profile)
    cols = ["zone", "id", "pixels", "invalid"] + [f"count_{k}" for k in range(ncls)] + ([f"area_map_{k}" for k in range(ncls)] if geo else [])
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(cols)
        for z, zid in enumerate(ids):
            row = [int(v) for v in counts[z]]
            out = [z, zid, sum(row), row[ncls]] + row[:ncls]
            if geo:
                out += [repr(float(v * geo[0] * geo[1])) for v in row[:ncls]]
            w.writerow(out)
    return path


def zone_table(classmap: torch.Tensor, zones: Sequence[Zone], ncls: int, fill: int = -1,
               profile: Optional[Dict[str, Any]] = None, all_touched: bool = False) -> Tuple[List[Any], np.ndarray]:
    """What inference writes: ``zones`` (:func:`read_zones`; map coordinates when ``profile`` is georeferenced) on ``classmap`` ->
    (ids, counts) for :func:`write_zone_csv`."""
    edges, edge_zone = zones_to_pixels(zones, profile)
    return [z.id for z in zones], zone_counts(classmap, edges, edge_zone, len(zones), ncls, fill, all_touched)


# ---- values: per-zone statistics of float rasters ---------------------------------------------------------------------------------------------
class ZoneValues(NamedTuple):
    pixels: np.ndarray  # (Z,) int64: all inside pixels of the zone
    valid: np.ndarray  # (Z, B) int64: those whose value is finite and not the no-data value
    sum: np.ndarray  # (Z, B) float64 each; NaN where valid is 0
    mean: np.ndarray
    std: np.ndarray  # population standard deviation, sqrt(M2 / valid)
    min: np.ndarray
    max: np.ndarray


def _check_nodata(nodata) -> Optional[float]:
    if nodata is None:
        return None
    if isinstance(nodata, bool) or not isinstance(nodata, (int, float, np.integer, np.floating)):
        raise ValueError(f"nodata must be None or a number (got {nodata!r})")
    nd = float(np.float32(nodata))
    return None if nd != nd else nd  # NaN is invalid anyway


def zone_values(raster: torch.Tensor, edges: np.ndarray, edge_zone: np.ndarray, Z: int, nodata: Optional[float] = None,
                all_touched: bool = False) -> ZoneValues:
    """Per zone and band the count, sum, mean, population std, min and max of one (H, W) or (B, H, W) float32 raster on the device ->
    :class:`ZoneValues`.  A value is valid when it is finite and differs from ``nodata`` (compared as float32); where a zone has no valid
    value its statistics are NaN.  ``edges`` / ``edge_zone`` are those of :func:`zones_to_pixels`.  One canvas per pass of 64 zones serves
    every group of ``ops.ZONE_VALUE_BANDS`` bands; the variance comes from merged (n, sum, M2) triples in a fixed order
    (include/instageo_hip.h): two runs give the same bits, and a band gives the same bits whatever other bands go with it."""
    if raster.dtype != torch.float32 or raster.dim() not in (2, 3):
        raise ValueError(f"zone_values takes one (H, W) or (B, H, W) float32 raster (got {tuple(raster.shape)} {raster.dtype})")
    r = (raster[None] if raster.dim() == 2 else raster).contiguous()
    B, H, W = r.shape
    if B < 1:
        raise ValueError("zone_values: the raster has no band")
    nd, Z = _check_nodata(nodata), int(Z)
    pixels = np.zeros(Z, dtype=np.int64)
    valid = np.zeros((Z, B), dtype=np.int64)
    stats = np.zeros((Z, B, 4), dtype=np.float64)  # mean, M2, min, max
    for p, canvas in _passes(edges, edge_zone, Z, H, W, r.device, all_touched):
        lo = p * ops.ZONE_BITS
        n = min(ops.ZONE_BITS, Z - lo)
        for b0 in range(0, B, ops.ZONE_VALUE_BANDS):
            pix, val, st = ops.zone_value_tally(canvas, r[b0:b0 + ops.ZONE_VALUE_BANDS], nd)
            if b0 == 0:
                pixels[lo:lo + n] = pix[:n].cpu().numpy()
            valid[lo:lo + n, b0:b0 + val.shape[1]] = val[:n].cpu().numpy()
            stats[lo:lo + n, b0:b0 + val.shape[1]] = st[:n].cpu().numpy()
    has = valid > 0
    nan = np.full((Z, B), np.nan)
    mean = np.where(has, stats[..., 0], nan)
    std = np.sqrt(np.divide(stats[..., 1], valid, out=nan.copy(), where=has))
    return ZoneValues(pixels, valid, mean * valid, mean, std, np.where(has, stats[..., 2], nan), np.where(has, stats[..., 3], nan))


# ---- order statistics: the median and percentiles -------------------------------------------------------------------------------------------
def check_percentiles(percentiles) -> List[float]:
    """A sequence of numbers in [0, 100] -> a list of float; ValueError for anything else (no sequence, empty, a bool, a string, NaN,
    a value outside the range)."""
    if isinstance(percentiles, (str, bytes)) or not isinstance(percentiles, (list, tuple, np.ndarray)) or len(percentiles) == 0:
        raise ValueError(f"percentiles must be a non-empty list of numbers in [0, 100] (got {percentiles!r})")
    out = []
    for q in percentiles:
        if isinstance(q, (bool, np.bool_)) or not isinstance(q, (int, float, np.integer, np.floating)) or not 0.0 <= float(q) <= 100.0:
            raise ValueError(f"percentiles must be a non-empty list of numbers in [0, 100] (got {q!r})")
        out.append(float(q))
    return out


def quantile_ranks(n, f) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The rule's ranks for ``n`` valid values (int, any shape) and fractions ``f`` = q / 100.0 (float64, broadcast against ``n``) ->
    (lo, hi int64, g float64): h = (n - 1) * f in float64, lo = floor(h), hi = min(lo + 1, n - 1), g = h - lo.  Where n is 0: (0, 0, 0)."""
    n = np.asarray(n, dtype=np.int64)
    h = np.maximum(n - 1, 0).astype(np.float64) * np.asarray(f, dtype=np.float64)
    lo = np.floor(h)
    hi = np.minimum(lo + 1, np.maximum(n - 1, 0))
    return lo.astype(np.int64), hi.astype(np.int64), h - lo


def quantile_lerp(a, b, g) -> np.ndarray:
    """numpy's ``linear`` method between the order statistics ``a`` = v(lo) and ``b`` = v(hi), widened to float64: a + (b - a) * g for
    g > 0, else a."""
    a, b, g = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(g, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(g > 0, a + (b - a) * g, a)


def zone_quantiles(raster: torch.Tensor, edges: np.ndarray, edge_zone: np.ndarray, Z: int, percentiles, nodata: Optional[float] = None,
                   pairs: bool = False, all_touched: bool = False):
    """Per zone and band the ``percentiles`` (numbers in [0, 100]; 50 is the median, 0 the minimum, 100 the maximum) of the valid values
    of one (H, W) or (B, H, W) float32 raster on the device -> (valid (Z, B) int64, values (Z, B, Q) float64), NaN where a zone has no
    valid value; with ``pairs`` also the order statistics themselves, (Z, B, Q, 2) float32 {v(lo), v(hi)}.  Validity, ``edges`` and
    ``edge_zone`` are those of :func:`zone_values`.  The device selects the pairs exactly (``ops.zone_value_quantiles``: groups of
    ``ops.ZONE_VALUE_BANDS`` bands and ``ops.ZONE_QUANTILES`` percentiles on one canvas per pass of 64 zones; a percentile given twice is
    selected once); the interpolation is :func:`quantile_lerp` on the host."""
    if raster.dtype != torch.float32 or raster.dim() not in (2, 3):
        raise ValueError(f"zone_quantiles takes one (H, W) or (B, H, W) float32 raster (got {tuple(raster.shape)} {raster.dtype})")
    qs = check_percentiles(percentiles)
    r = (raster[None] if raster.dim() == 2 else raster).contiguous()
    B, H, W = r.shape
    if B < 1:
        raise ValueError("zone_quantiles: the raster has no band")
    nd, Z = _check_nodata(nodata), int(Z)
    uniq = list(dict.fromkeys(qs))
    fr = [q / 100.0 for q in uniq]
    valid = np.zeros((Z, B), dtype=np.int64)
    order = np.full((Z, B, len(uniq), 2), np.nan, dtype=np.float32)
    for p, canvas in _passes(edges, edge_zone, Z, H, W, r.device, all_touched):
        lo = p * ops.ZONE_BITS
        n = min(ops.ZONE_BITS, Z - lo)
        for b0 in range(0, B, ops.ZONE_VALUE_BANDS):
            for q0 in range(0, len(fr), ops.ZONE_QUANTILES):
                val, od = ops.zone_value_quantiles(canvas, r[b0:b0 + ops.ZONE_VALUE_BANDS], fr[q0:q0 + ops.ZONE_QUANTILES], nd)
                valid[lo:lo + n, b0:b0 + val.shape[1]] = val[:n].cpu().numpy()
                order[lo:lo + n, b0:b0 + val.shape[1], q0:q0 + od.shape[2]] = od[:n].cpu().numpy()
    g = quantile_ranks(valid[..., None], np.array(fr, dtype=np.float64))[2]
    values = np.where(valid[..., None] > 0, quantile_lerp(order[..., 0], order[..., 1], g), np.nan)
    pick = [uniq.index(q) for q in qs]
    values, order = np.ascontiguousarray(values[:, :, pick]), np.ascontiguousarray(order[:, :, pick])
    return (valid, values, order) if pairs else (valid, values)


def zone_quantiles_host(mask: np.ndarray, raster: np.ndarray, percentiles, nodata: Optional[float] = None, pairs: bool = False):
    """The numpy twin of the rule, for one zone: ``mask`` (H, W) bool and ``raster`` (H, W) or (B, H, W) float32 -> (valid (B,) int64,
    values (B, Q) float64); with ``pairs`` also (B, Q, 2) float32 {v(lo), v(hi)}.  ``np.sort`` of the canonicalised (v + 0.0) valid
    values, then the rank and interpolation formulas of :func:`quantile_ranks` and :func:`quantile_lerp`."""
    qs = check_percentiles(percentiles)
    raster, mask = np.asarray(raster), np.asarray(mask, dtype=bool)
    if raster.dtype != np.float32 or raster.ndim not in (2, 3) or raster.shape[-2:] != mask.shape:
        raise ValueError("zone_quantiles_host takes a (H, W) mask and a (H, W) or (B, H, W) float32 raster")
    r = raster[None] if raster.ndim == 2 else raster
    nd = _check_nodata(nodata)
    fr = np.array([q / 100.0 for q in qs], dtype=np.float64)
    valid = np.zeros(len(r), dtype=np.int64)
    values = np.full((len(r), len(qs)), np.nan)
    order = np.full((len(r), len(qs), 2), np.nan, dtype=np.float32)
    for b, band in enumerate(r):
        v = band[mask]
        ok = np.isfinite(v)
        if nd is not None:
            ok &= v != np.float32(nd)
        v = np.sort(v[ok] + np.float32(0.0))
        valid[b] = v.size
        if v.size:
            lo, hi, g = quantile_ranks(v.size, fr)
            order[b, :, 0], order[b, :, 1] = v[lo], v[hi]
            values[b] = quantile_lerp(v[lo], v[hi], g)
    return (valid, values, order) if pairs else (valid, values)


def zone_value_table(raster: torch.Tensor, zones: Sequence[Zone], nodata: Optional[float] = None,
                     profile: Optional[Dict[str, Any]] = None, percentiles=None, all_touched: bool = False):
    """``zones`` (:func:`read_zones`; map coordinates when ``profile`` is georeferenced) on ``raster`` -> (ids, values) for
    :func:`write_zone_values_csv`: what :func:`zone_table` is to a class map.  With ``percentiles`` -> (ids, values, (Z, B, Q) float64 of
    :func:`zone_quantiles`)."""
    edges, edge_zone = zones_to_pixels(zones, profile)
    ids, values = [z.id for z in zones], zone_values(raster, edges, edge_zone, len(zones), nodata, all_touched)
    if percentiles is None:
        return ids, values
    return ids, values, zone_quantiles(raster, edges, edge_zone, len(zones), percentiles, nodata, all_touched=all_touched)[1]


VALUE_COLUMNS = ("valid", "mean", "std", "min", "max", "sum")  # per band, in this order


def write_zone_values_csv(path: str, ids: Sequence[Any], values: ZoneValues, band_names: Optional[Sequence[Any]] = None,
                          profile: Optional[Dict[str, Any]] = None, percentiles=None) -> str:
    """Write one row per zone: ``zone`` (its index), ``id``, ``pixels`` (all its inside pixels), then per band ``valid_<b>``, ``mean_<b>``,
    ``std_<b>``, ``min_<b>``, ``max_<b>``, ``sum_<b>`` (``<b>`` from ``band_names``, else the band's index) and, with a georeferenced
    ``profile``, ``area_map`` = pixels * scale_x * scale_y in squared map units.  Floats are written with ``repr`` (they read back
    exactly); the statistics of a zone without a valid value are empty cells.  ``percentiles`` = (the percentiles, their (Z, B, Q)
    values of :func:`zone_quantiles`) adds, per band after ``sum_<b>``, the columns ``percentile_<q>_<b>`` (``<q>`` written with ``%g``)."""
    valid = np.asarray(values.valid)
    if valid.ndim != 2 or valid.shape[0] != len(ids) or np.asarray(values.pixels).shape != (len(ids),):
        raise ValueError("values must hold (len(ids),) pixels and (len(ids), bands) statistics")
    B = valid.shape[1]
    names = [str(b) for b in (range(B) if band_names is None else band_names)]
    if len(names) != B or len(set(names)) != B:
        raise ValueError(f"band_names must give {B} distinct names (got {list(band_names)!r})")
    qnames, qvalues = [], None
    if percentiles is not None:
        qs, qvalues = percentiles
        qnames, qvalues = ["percentile_%g" % q for q in check_percentiles(qs)], np.asarray(qvalues)
        if len(set(qnames)) != len(qnames) or qvalues.shape != (len(ids), B, len(qnames)):
            raise ValueError(f"percentiles must be (distinct percentiles, their ({len(ids)}, {B}, Q) values)")
    geo = georeference(profile)
    cols = ["zone", "id", "pixels"] + [f"{k}_{b}" for b in names for k in VALUE_COLUMNS + tuple(qnames)] + (["area_map"] if geo else [])
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(cols)
        for z, zid in enumerate(ids):
            out = [z, zid, int(values.pixels[z])]
            for b in range(B):
                n = int(valid[z, b])
                out.append(n)
                out += [repr(float(getattr(values, k)[z, b])) if n else "" for k in VALUE_COLUMNS[1:]]
                out += [repr(float(qvalues[z, b, i])) if n else "" for i in range(len(qnames))]
            if geo:
                out.append(repr(float(int(values.pixels[z]) * geo[0] * geo[1])))
            w.writerow(out)
    return path


# ---- mode=zonal_stats -------------------------------------------------------------------------------------------------------------------------
CONFIG_KEYS = ("raster", "zones", "zone_id_property", "output", "bands", "nodata", "zones_crs")
# keys without a default: given as ``+zonal_stats.<key>=...`` on the command line, or in a YAML config.  percentiles: None, or a list of
# 1..MAX_PERCENTILES distinct numbers in [0, 100] (50 = the median): the columns percentile_<q>_<b> of the CSV.  all_touched: true | false
# (unset = false): a zone also holds the pixels its edges touch
OPTIONAL_KEYS = ("percentiles", "all_touched")
MAX_PERCENTILES = 32


def zonal_stats_options(cfg: Dict[str, Any]) -> Dict[str, Any]:
    """The ``zonal_stats.*`` keys checked -> {raster, zones (a list of :class:`Zone` in the raster's coordinate system), bands, nodata,
    output, profile, percentiles, all_touched}.  An unknown key, a bad value, a missing file, a band the file does not have, a feature that is no (Multi)Polygon,
    or ``zones_crs`` with a raster that carries no coordinate system raises ValueError naming the key.  Reads the raster's header and the
    GeoJSON; touches no device."""
    c = prep.Section(cfg, "zonal_stats", CONFIG_KEYS + OPTIONAL_KEYS)
    percentiles = c.get("percentiles")
    if percentiles is not None:
        try:
            percentiles = check_percentiles(list(percentiles) if isinstance(percentiles, (list, tuple)) else percentiles)
            if len(percentiles) > MAX_PERCENTILES or len(set(percentiles)) != len(percentiles):
                raise ValueError
        except ValueError:
            raise c.bad("percentiles", f"must be None or a list of 1..{MAX_PERCENTILES} distinct numbers in [0, 100]", c.get("percentiles")) from None
    all_touched = c.flag("all_touched")
    raster, zfile = c.text("raster"), c.text("zones")
    for key, path in (("raster", raster), ("zones", zfile)):
        if path is None:
            raise ValueError(f"mode=zonal_stats needs zonal_stats.{key}")
        if not os.path.isfile(path):
            raise c.bad(key, "is not a file", path)
    try:
        profile = tiff.read_profile(raster)
    except tiff.TiffError as e:
        raise ValueError(f"zonal_stats.raster: {e}") from None
    count = int(profile["count"])
    bands = c.get("bands")
    if bands is None:
        bands = list(range(count))
    elif not isinstance(bands, (list, tuple)) or not bands or not all(prep.is_int(b) for b in bands) or len(set(bands)) != len(bands):
        raise c.bad("bands", "must be None or a list of distinct band indices", bands)
    elif not all(0 <= b < count for b in bands):
        raise c.bad("bands", f"names a band outside [0, {count}): {raster} has {count} band{'s' if count != 1 else ''}", bands)
    nodata = c.get("nodata")
    try:
        nodata = _check_nodata(profile.get("nodata") if nodata is None else nodata)
    except ValueError:
        raise c.bad("nodata", "must be None (the file's own no-data tag) or a number", nodata) from None
    try:
        zones = read_zones(zfile, c.text("zone_id_property"))
    except ValueError as e:
        raise ValueError(f"zonal_stats.zones: {e}") from None
    epsg = c.get("zones_crs")
    if epsg is not None:
        if not prep.is_int(epsg):
            raise c.bad("zones_crs", "must be an EPSG code", epsg)
        try:
            crsmod.from_epsg(epsg)
        except ValueError as e:
            raise ValueError(f"zonal_stats.zones_crs: {e}") from None
        try:
            if georeference(profile) is None:
                raise ValueError("no pixel scale and tiepoint")
            dst = crsmod.from_profile(profile)
        except ValueError as e:
            raise ValueError(f"zonal_stats.zones_crs = {epsg} needs a raster with a coordinate system ({raster}: {e})") from None
        src, moved = crsmod.from_epsg(epsg), []
        for z in zones:
            rings = []
            for ring in z.rings:
                x, y = crsmod.transform(src, dst, ring[:, 0], ring[:, 1])
                rings.append(np.stack([x, y], axis=1))
            moved.append(Zone(z.id, rings))
        zones = moved
    try:
        zones_to_pixels(zones, profile)  # a vertex beyond the fixed-point range (or outside the projection's domain) stops here
    except ValueError as e:
        raise ValueError(f"zonal_stats.zones: {e}") from None
    output = c.text("output")
    if output is None:
        output = os.path.join(os.path.dirname(raster), f"zonevalues_{os.path.splitext(os.path.basename(raster))[0]}.csv")
    return dict(raster=raster, zones=zones, bands=[int(b) for b in bands], nodata=nodata, output=output, profile=profile,
                percentiles=percentiles, all_touched=all_touched)


def _to_float32(a: np.ndarray, device) -> torch.Tensor:
    """Samples of any dtype :mod:`tiff` reads -> float32 on the device.  The conversion runs there; unsigned 16 / 32 / 64-bit samples,
    which torch does not convert, are widened on the host first (without loss up to 32 bits)."""
    if a.dtype.kind == "u" and a.dtype.itemsize > 1:
        a = a.astype(np.int32 if a.dtype.itemsize == 2 else np.int64 if a.dtype.itemsize == 4 else np.float64)
    return torch.from_numpy(np.ascontiguousarray(a)).to(device).to(torch.float32)


def run_from_config(cfg: Dict[str, Any], device: Optional[str] = None) -> int:
    """``mode=zonal_stats``: the per-zone statistics of the GeoTIFF ``zonal_stats.raster`` over the polygons of ``zonal_stats.zones``,
    written as the CSV of :func:`write_zone_values_csv` (with ``zonal_stats.percentiles`` also the percentiles of :func:`zone_quantiles`);
    prints one JSON line (zones, bands, zones without a valid pixel, the output
    path).  Every option is checked before the device is touched; there is no host path."""
    kw = zonal_stats_options(cfg)
    if device is None:
        raise RuntimeError("mode=zonal_stats runs on a HIP device and there is none (the tally has no host path)")
    a, profile = tiff.read(kw["raster"], kw["bands"])
    qs = kw["percentiles"]
    ids, values, *rest = zone_value_table(_to_float32(a, device), kw["zones"], kw["nodata"], profile, qs, kw["all_touched"])
    write_zone_values_csv(kw["output"], ids, values, kw["bands"], profile, None if qs is None else (qs, rest[0]))
    print(json.dumps({"zonal_stats": {"zones": len(ids), "bands": len(kw["bands"]), "empty_zones": int((values.valid.sum(axis=1) == 0).sum()),
                                      "output": kw["output"]}}))
    return 0


def main(argv: Optional[List[str]] = None) -> int:
    """``python -m instageo_amd.zonal zonal_stats.raster=prediction.tif zonal_stats.zones=districts.geojson ...``: mode=zonal_stats
    without ``run.py``."""
    return prep.run_mode_cli("zonal_stats", run_from_config, argv)


if __name__ == "__main__":
    raise SystemExit(main())
