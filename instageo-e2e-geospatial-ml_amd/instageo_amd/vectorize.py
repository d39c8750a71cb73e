"""Class-map regions as polygon rings, traced on the device (not in the reference; ``csrc/vectorize.hip``), and the
GeoJSON writer for them.

Geometry.  Pixel (r, c) covers [c, c+1] x [r, r+1] in (x, y), y down.  Every valid pixel owns four directed unit edges with the pixel
on their right-hand side; an edge is *live* when the pixel across it has another region label (``ig_ccl_label``'s; fill and the outside
of the image count as no region).  Each live edge has exactly one live successor -- left turn, straight, right turn, decided by the
LABELS of the two pixels ahead, so a diagonal pair is joined under 4-connectivity only when it is one component -- and the cycles of
that map are the rings (the rule in full: ``include/instageo_hip.h``).  A ring starts at its smallest edge, keeps only the corners
(collinear points are dropped) and has twice the signed area ``sum (x1 y2 - x2 y1)``: positive for the one exterior ring of a region,
negative for its holes.  Under 4-connectivity every ring is simple.  Under 8-connectivity a ring may touch itself at a vertex (two
pixels of a region that meet only at a corner), as the polygons of GDAL's 8-connected polygoniser do; such a ring is still a valid
even-odd outline, but not a simple polygon.

Everything is integer and unique: two runs, or the device and a sequential tracer, give the same bits.  There is no simplification
(Douglas-Peucker and its kin move shared borders independently and tear neighbours apart): out of scope.
"""
from __future__ import annotations

from typing import Any, Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib, ops
from .postprocess import _check_labels, _check_map, georeference

RING_COLUMNS = ("image", "label", "cls", "n_vertices", "twice_area", "first")


def check_polygon_options(save_polygons: bool = False, regression: bool = False) -> None:
    """ValueError for ``save_polygons`` with a regression head (it has no class map).  Touches no file, model or device."""
    if regression and save_polygons:
        raise ValueError("save_polygons needs a class map (a regression head has one output channel)")


def _jump_rounds(n_edges: int) -> int:
    """ceil(log2 E): after that many doublings a pointer has gone round any ring."""
    return max(1, (int(n_edges) - 1).bit_length())


def _jump(phase: int, succ: torch.Tensor, root: Optional[torch.Tensor] = None, flag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Loop ``ig_ring_jump`` between two buffer pairs until a round reports no change (read from the device after every round) or
    ceil(log2 E) rounds have run -> the value buffer of the last round."""
    E = succ.numel()
    bufs = [torch.empty((2, E), dtype=torch.int32, device=succ.device) for _ in range(2)]
    changed = torch.zeros(1, dtype=torch.int32, device=succ.device)
    val_in, ptr_in = None, succ
    for k in range(_jump_rounds(E)):
        val_out, ptr_out = bufs[k & 1]
        changed.zero_()
        ops.ring_jump(phase, val_in, ptr_in, val_out, ptr_out, changed, root, flag)
        val_in, ptr_in = val_out, ptr_out
        if int(changed.item()) == 0:
            break
    return val_in


def _empty() -> Tuple[np.ndarray, np.ndarray]:
    return np.zeros((0, len(RING_COLUMNS)), dtype=np.int64), np.zeros((0, 2), dtype=np.int32)


def region_rings(classmap: torch.Tensor, connectivity: int = 4, fill: int = -1,
                 labels: Optional[torch.Tensor] = None) -> Tuple[np.ndarray, np.ndarray]:
    """The rings of every region of an (H, W) | (n, H, W) int8 class map on the device -> (rings, vertices) as numpy arrays.

    ``rings`` int64, one row per ring with the columns ``RING_COLUMNS``: ``image``, ``label`` (the region's root of
    :func:`postprocess.region_table`), ``cls``, ``n_vertices``, ``twice_area`` (> 0 exterior, < 0 hole) and ``first`` = its first row
    in ``vertices`` (V, 2) int32 (x, y) lattice corners; a ring is NOT closed there (the first vertex is not repeated).  Rows are ordered
    by (image, label, hole, root edge): a region's exterior ring, then its holes.  A region's rings sum to twice its pixel count.
    ``labels``: what :func:`postprocess.label_regions` gave for the same map, ``connectivity`` and ``fill``, when the caller has it
    already (the map is then not labelled again)."""
    _check_map(classmap, connectivity, fill)
    _check_labels(labels, classmap)
    cm3 = classmap.contiguous()
    cm3 = cm3 if cm3.dim() == 3 else cm3.unsqueeze(0)
    if cm3.numel() == 0:
        return _empty()
    HW = cm3.shape[1] * cm3.shape[2]
    labels = ops.ccl_label(cm3, connectivity, fill) if labels is None else labels.contiguous().view(cm3.shape)
    mask, total = ops.edge_mask(labels)
    E = int(total.item())
    if E == 0:
        return _empty()
    if E > ops.MAX_EDGES:
        raise ValueError(f"the map has {E} boundary edges; at most 2^31 - 1 can be traced at once (edge ids are int32): split the batch or the tile")
    cnt = torch.bitwise_right_shift(mask.view(-1), 4)
    off = torch.cumsum(cnt, 0, dtype=torch.int32).sub_(cnt)  # compact id of every pixel's first live edge
    del cnt
    succ, tail, flag = ops.edge_link(labels, mask, off.view(labels.shape), E)
    del mask
    root = _jump(0, succ)
    rank = _jump(1, succ, root, flag)  # turn edges from an edge to the end of its ring
    del succ
    isroot = root == torch.arange(E, dtype=torch.int32, device=root.device)
    ring_id = torch.cumsum(isroot, 0, dtype=torch.int32).sub_(1)
    roots = torch.nonzero(isroot).view(-1)  # ascending edge ids
    del isroot
    R = int(roots.numel())
    sums = ops.ring_sums(root, ring_id, tail, flag, R)
    nv, area2 = rank[roots].to(torch.int64), sums[:, 1]
    if not torch.equal(nv, sums[:, 0]):
        raise _lib.HipLibraryError("region_rings: the vertex ranks disagree with the vertex counts of the rings")
    pix = torch.searchsorted(off, roots.to(torch.int32), right=True) - 1  # image * HW + pixel of the root edge's owner
    image, label, cls = pix // HW, labels.view(-1)[pix].to(torch.int64), cm3.view(-1)[pix].to(torch.int64)
    # roots ascend, so a stable sort by (image, label, hole) leaves rings of equal keys in root order
    perm = torch.sort((image * HW + label) * 2 + (area2 < 0), stable=True).indices
    first_sorted = torch.cumsum(nv[perm], 0) - nv[perm]
    first = torch.empty_like(first_sorted)
    first[perm] = first_sorted
    vertices = ops.ring_emit(root, ring_id, rank, tail, flag, first, int(nv.sum().item()))
    rings = torch.stack([image, label, cls, nv, area2, first], dim=1)[perm]
    return rings.cpu().numpy(), vertices.cpu().numpy()


def rings_of_image(rings: np.ndarray, vertices: np.ndarray, image: int) -> Tuple[np.ndarray, np.ndarray]:
    """The rings of one image of a batch, renumbered as image 0, with their own vertex array."""
    keep = rings[:, 0] == image
    out = rings[keep].copy()
    if len(out) == 0:
        return out, vertices[:0].copy()
    lo, hi = int(out[0, 5]), int(out[-1, 5] + out[-1, 3])  # an image's rings are consecutive rows, and so are their vertices
    out[:, 0] = 0
    out[:, 5] -= lo
    return out, vertices[lo:hi].copy()


def write_geojson(path: str, rings: np.ndarray, vertices: np.ndarray, table: Dict[str, np.ndarray],
                  profile: Optional[Dict[str, Any]] = None) -> str:
    """Write the rings of :func:`region_rings` as a GeoJSON FeatureCollection: one Feature per region, in the order of ``table``
    (:func:`postprocess.region_table` of the same map, same connectivity).  The geometry is a ``Polygon``: the exterior ring, then the
    holes, each ring closed (first position repeated).  Properties: ``root``, ``cls``, ``area`` (pixels) and, with a georeferenced
    ``profile`` (:func:`postprocess.georeference`), ``area_map`` = area * scale_x * scale_y as in ``regions_*.csv``; a batch table also
    gives ``image``.

    Coordinates.  Georeferenced: a lattice corner (X, Y) maps to (tie_x + (X - tie_i) * scale_x, tie_y - (Y - tie_j) * scale_y).  The
    y flip mirrors every ring, so the rings are written backwards (still starting at their first vertex): exteriors come out
    counter-clockwise and holes clockwise in map coordinates, as RFC 7946 asks.  Without georeferencing the lattice (X, Y) are written
    as integers in tracing order: exteriors are counter-clockwise as numbers, which on a screen with y down looks clockwise (the
    screen winding).  Floats are written with ``repr`` (they read back exactly).  Under 8-connectivity a ring may touch itself at a
    vertex.  No simplification: out of scope (see the module docstring)."""
    geo = georeference(profile)
    key_r = [(int(a), int(b)) for a, b in zip(rings[:, 0], rings[:, 1])]
    key_t = [(int(a), int(b)) for a, b in zip(table["image"], table["root"])]
    if sorted(set(key_r)) != key_t:
        raise ValueError("the rings and the region table do not describe the same regions")
    batch = len(key_t) > 0 and key_t[-1][0] > 0
    if geo:
        sx, sy, ti, tj, tx, ty = geo
        xs = [repr(float(v)) for v in tx + (vertices[:, 0].astype(np.float64) - ti) * sx]
        ys = [repr(float(v)) for v in ty - (vertices[:, 1].astype(np.float64) - tj) * sy]
        backwards = sx * sy > 0  # the map transform mirrors the lattice
    else:
        xs, ys = [str(int(v)) for v in vertices[:, 0]], [str(int(v)) for v in vertices[:, 1]]
        backwards = False
    pts = [f"[{x},{y}]" for x, y in zip(xs, ys)]

    def ring_text(i: int) -> str:
        a, k = int(rings[i, 5]), int(rings[i, 3])
        p = pts[a:a + k]
        if backwards:
            p = p[:1] + p[:0:-1]
        return "[" + ",".join(p + p[:1]) + "]"

    with open(path, "w") as f:
        f.write('{"type":"FeatureCollection","features":[')
        i = 0
        for j, key in enumerate(key_t):
            parts = []
            while i < len(key_r) and key_r[i] == key:
                parts.append(ring_text(i))
                i += 1
            area = int(table["area"][j])
            props = ([f'"image":{key[0]}'] if batch else []) + [f'"root":{key[1]}', f'"cls":{int(table["cls"][j])}', f'"area":{area}']
            if geo:
                props.append(f'"area_map":{repr(float(area * sx * sy))}')
            f.write(("," if j else "") + '\n{"type":"Feature","properties":{' + ",".join(props) + '},"geometry":{"type":"Polygon","coordinates":['
                    + ",".join(parts) + "]}}")
        f.write("\n]}\n")
    return path
