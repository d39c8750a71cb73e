"""Zonal statistics: the user's polygons (administrative units, parcels, catchments) rasterised onto a class map on the device and
tallied per zone and class (not in the reference; ``csrc/zonal.hip``).  The inverse of :mod:`instageo_amd.vectorize`,
in its coordinates.

Rule.  Pixel (r, c) covers [c, c+1] x [r, r+1] in lattice (x, y), y down.  Zone vertices are quantised to Q = 256 units per pixel,
``X = floor(x * 256 + 0.5)``, in float64 on the host; the pixel centre is (256 c + 128, 256 r + 128).  A zone is a set of closed rings
(exteriors and holes of a ``Polygon`` or ``MultiPolygon``, any orientation); a pixel is inside iff an odd number of the zone's edges
cross its row's centre line at or left of its centre (even-odd on pixel centres: GDAL and rasterio without ``all_touched``; the two
inequalities that decide every tie: ``include/instageo_hip.h``).  Zones are independent: a pixel inside several zones counts in each
of them, as rasterstats does.  Everything on the device is integer and unique: two runs give the same bits.

Out of scope: per-zone means of the probabilities, ``all_touched``, rotated or sheared geotransforms, one table merged across chips
or tiles, zone rasters written as TIFF.
"""
from __future__ import annotations

import csv
import json
import os
from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
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


def _passes(edges: np.ndarray, edge_zone: np.ndarray, Z: int, H: int, W: int, device):
    """Yield (pass, canvas) for those of the ceil(Z / 64) passes whose zones cross a row of the raster at all: the (H, W) int64 canvas
    holds their toggles, bit ``zone % 64`` each (rows counted, scanned, toggled; not yet prefix-XORed).  A pass without a crossing
    has no inside pixel and launches nothing."""
    edges, edge_zone = _check_edges(edges, edge_zone, Z)
    if len(edges) == 0 or H * W == 0:
        return
    for p in range((Z + ops.ZONE_BITS - 1) // ops.ZONE_BITS):
        sel = (edge_zone // ops.ZONE_BITS) == p
        if not sel.any():
            continue
        e = torch.from_numpy(np.ascontiguousarray(edges[sel])).to(device)
        bit = torch.from_numpy((edge_zone[sel] % ops.ZONE_BITS).astype(np.uint8)).to(device)
        rows = ops.zone_edge_rows(e, H)
        first = torch.cumsum(rows, 0, dtype=torch.int64).sub_(rows)
        T = int(rows.sum(dtype=torch.int64).item())
        if T == 0:
            continue
        canvas = torch.zeros((H, W), dtype=torch.int64, device=device)
        ops.zone_toggle(e, bit, first, canvas, T)
        yield p, canvas


def zone_masks(edges: np.ndarray, edge_zone: np.ndarray, Z: int, H: int, W: int, device="cuda") -> torch.Tensor:
    """-> (ceil(Z / 64), H, W) int64 bit planes on the device: bit ``z % 64`` of plane ``z // 64`` at (r, c) = pixel (r, c) is inside
    zone z (bit 63 is the sign bit).  ``edges`` / ``edge_zone`` are those of :func:`zones_to_pixels`."""
    Z, H, W = int(Z), int(H), int(W)
    planes = torch.zeros(((Z + ops.ZONE_BITS - 1) // ops.ZONE_BITS, H, W), dtype=torch.int64, device=device)
    for p, canvas in _passes(edges, edge_zone, Z, H, W, device):
        ops.zone_tally(canvas, None, None, write_mask=True)
        planes[p] = canvas
    return planes


def zone_counts(classmap: torch.Tensor, edges: np.ndarray, edge_zone: np.ndarray, Z: int, ncls: int, fill: int = -1) -> np.ndarray:
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
    for p, canvas in _passes(edges, edge_zone, Z, H, W, cm.device):
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
               profile: Optional[Dict[str, Any]] = None) -> Tuple[List[Any], np.ndarray]:
    """What inference writes: ``zones`` (:func:`read_zones`; map coordinates when ``profile`` is georeferenced) on ``classmap`` ->
    (ids, counts) for :func:`write_zone_csv`."""
    edges, edge_zone = zones_to_pixels(zones, profile)
    return [z.id for z in zones], zone_counts(classmap, edges, edge_zone, len(zones), ncls, fill)
