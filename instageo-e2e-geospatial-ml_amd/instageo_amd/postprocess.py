"""Region post-processing of int8 class maps on the device (not in the reference): connected-component labelling, the
minimum-mapping-unit sieve and the region table of what is left (``csrc/regions.hip``).

A class map is an (H, W) or (n, H, W) int8 HIP tensor; ``fill`` marks invalid pixels, every other value is a class; images are
independent.  Every result is an integer (centroids: float64 quotients of integer sums, taken on the host) and unique, so two runs
give the same bits.

The sieve rule.  One pass works on the map as it stands at the start of the pass:

1. label it with ``connectivity``;
2. regions with area < ``min_region`` are *small*, all others *kept*;
3. a small region looks at the kept regions that share a 4-neighbour edge with it (always edge adjacency; fill never counts);
4. it takes the class of the one with the largest area, ties going to the smaller label;
5. a small region without a kept neighbour stays.

All reassignments of a pass are simultaneous.  Passes repeat until one changes nothing or ``max_passes`` have run: noisy maps peel
one layer per pass and can need tens of passes, so ``max_passes`` is a cap, and the result reports what it left behind.
"""
from __future__ import annotations

import csv
from typing import Any, Dict, Optional, Tuple

import numpy as np
import torch

from . import ops

TABLE_COLUMNS = ("image", "root", "cls", "area", "row_min", "row_max", "col_min", "col_max", "centroid_row", "centroid_col")


def check_region_options(min_region: int = 0, connectivity: int = 4, sieve_passes: int = 8, save_regions: bool = False,
                         regression: bool = False) -> None:
    """ValueError for options that cannot work: connectivity other than 4 / 8, negative values, or either option with a regression head
    (it has no class map).  Touches no file, model or device."""
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8 (got {connectivity!r})")
    if int(min_region) != min_region or min_region < 0:
        raise ValueError(f"min_region must be a non-negative integer (got {min_region!r})")
    if int(sieve_passes) != sieve_passes or sieve_passes < 0:
        raise ValueError(f"sieve_passes must be a non-negative integer (got {sieve_passes!r})")
    if regression and (min_region > 0 or save_regions):
        raise ValueError("min_region and save_regions need a class map (a regression head has one output channel)")


def _check_map(classmap: torch.Tensor, connectivity: int, fill: int) -> None:
    if not (isinstance(classmap, torch.Tensor) and classmap.dtype == torch.int8 and classmap.dim() in (2, 3)):
        raise ValueError("a class map is an (H, W) or (n, H, W) int8 tensor")
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8 (got {connectivity!r})")
    if not -128 <= int(fill) <= 127:
        raise ValueError(f"fill must fit int8 (got {fill!r})")
    if classmap.shape[-2] * classmap.shape[-1] > 2**31 - 1:
        raise ValueError("H * W must not exceed 2^31 - 1")


def label_regions(classmap: torch.Tensor, connectivity: int = 4, fill: int = -1) -> torch.Tensor:
    """int32 labels of the map's shape: a pixel's label is the smallest row-major index ``y * W + x`` among the pixels of its component
    (same class, connected under ``connectivity``); ``fill`` pixels get -1."""
    _check_map(classmap, connectivity, fill)
    if classmap.numel() == 0:
        return torch.empty(classmap.shape, dtype=torch.int32, device=classmap.device)
    return ops.ccl_label(classmap.contiguous(), connectivity, fill)


def sieve_class_map(classmap: torch.Tensor, min_region: int, connectivity: int = 4, fill: int = -1,
                    max_passes: int = 8) -> Tuple[torch.Tensor, Dict[str, int]]:
    """Remove regions below the minimum mapping unit (the rule of the module docstring) -> (new int8 map, info).  ``info``: "passes" =
    the passes that reassigned something, "changed" = the regions reassigned over all passes, "small_left" = the small regions of the
    returned map (those without a kept neighbour, or all that ``max_passes`` left behind).  ``min_region <= 1`` is the identity."""
    _check_map(classmap, connectivity, fill)
    if max_passes < 0:
        raise ValueError(f"max_passes must not be negative (got {max_passes!r})")
    out = classmap.contiguous().clone()
    info = {"passes": 0, "changed": 0, "small_left": 0}
    if min_region <= 1 or out.numel() == 0:
        return out, info
    labels = torch.empty(out.shape, dtype=torch.int32, device=out.device)
    area = torch.empty_like(labels)
    best = torch.empty(out.shape, dtype=torch.int64, device=out.device) if max_passes else None
    changed = torch.zeros(1, dtype=torch.int32, device=out.device)
    current = False  # labels / area describe ``out``
    for _ in range(max_passes):
        ops.ccl_label(out, connectivity, fill, out=labels)
        ops.region_area(labels, out=area)
        changed.zero_()
        ops.sieve_pass(out, labels, area, min_region, fill, best, changed)
        c = int(changed.item())
        if c == 0:
            current = True
            break
        info["passes"] += 1
        info["changed"] += c
    if not current:
        ops.ccl_label(out, connectivity, fill, out=labels)
        ops.region_area(labels, out=area)
    info["small_left"] = int(((area > 0) & (area < min_region)).sum().item())
    return out, info


def _check_labels(labels: Optional[torch.Tensor], classmap: torch.Tensor) -> None:
    if labels is not None and not (isinstance(labels, torch.Tensor) and labels.dtype == torch.int32 and labels.shape == classmap.shape):
        raise ValueError("labels must be the int32 tensor of the class map's shape that label_regions returns for it")


def region_table(classmap: torch.Tensor, connectivity: int = 4, fill: int = -1, labels: Optional[torch.Tensor] = None) -> Dict[str, np.ndarray]:
    """One row per region, ordered by (image, root): ``image``, ``root`` (the label), ``cls``, ``area``, the bounding box ``row_min,
    row_max, col_min, col_max`` (inclusive pixel indices) as int64 and the centroid ``centroid_row, centroid_col`` as float64 = the
    integer sums of the pixel indices / area, divided on the host.  ``labels``: what :func:`label_regions` gave for the same map,
    ``connectivity`` and ``fill``, when the caller has it already (the map is then not labelled again)."""
    _check_map(classmap, connectivity, fill)
    _check_labels(labels, classmap)
    cm = classmap.contiguous()
    cm3 = cm if cm.dim() == 3 else cm.unsqueeze(0)
    if cm3.numel() == 0:
        return {k: np.zeros(0, dtype=np.float64 if k.startswith("centroid") else np.int64) for k in TABLE_COLUMNS}
    HW = cm3.shape[1] * cm3.shape[2]
    labels = ops.ccl_label(cm3, connectivity, fill) if labels is None else labels.contiguous().view(cm3.shape)
    area = ops.region_area(labels)
    isroot = (area != 0).view(-1)
    rid = (torch.cumsum(isroot, 0, dtype=torch.int32) - 1).view(labels.shape)
    pos = torch.nonzero(isroot).view(-1)  # image * HW + root, ascending
    R = int(pos.numel())
    stats = ops.region_stats(labels, rid, R).cpu().numpy()
    cls = cm3.view(-1)[pos].cpu().numpy().astype(np.int64)
    pos = pos.cpu().numpy()
    a = stats[:, 0]
    assert R == 0 or np.array_equal(a, area.view(-1).cpu().numpy()[pos]), "region statistics disagree with the region areas"
    return {"image": pos // HW, "root": pos % HW, "cls": cls, "area": a, "row_min": stats[:, 1], "row_max": stats[:, 2],
            "col_min": stats[:, 3], "col_max": stats[:, 4], "centroid_row": stats[:, 5] / np.maximum(a, 1).astype(np.float64),
            "centroid_col": stats[:, 6] / np.maximum(a, 1).astype(np.float64)}


def table_of_image(table: Dict[str, np.ndarray], image: int) -> Dict[str, np.ndarray]:
    """The rows of one image of a batch table, renumbered as image 0."""
    keep = table["image"] == image
    out = {k: v[keep] for k, v in table.items()}
    out["image"] = np.zeros_like(out["image"])
    return out


def georeference(profile: Optional[Dict[str, Any]]) -> Optional[Tuple[float, float, float, float, float, float]]:
    """(scale_x, scale_y, tie_i, tie_j, tie_x, tie_y) when the GeoTIFF profile carries a pixel scale (tag 33550) and a tiepoint (tag
    33922), else None."""
    tags = (profile or {}).get("tags") or {}
    if 33550 not in tags or 33922 not in tags:
        return None
    scale, tie = tags[33550][1], tags[33922][1]
    if len(scale) < 2 or len(tie) < 6:
        return None
    return float(scale[0]), float(scale[1]), float(tie[0]), float(tie[1]), float(tie[3]), float(tie[4])


def write_region_csv(path: str, table: Dict[str, np.ndarray], profile: Optional[Dict[str, Any]] = None) -> str:
    """Write a region table as CSV.  The pixel columns (``TABLE_COLUMNS``) are always written.  With a georeferenced ``profile``
    (:func:`georeference`) three columns follow: ``x``, ``y`` = the map coordinates of the centroid (pixel (r, c) has its centre at
    tie_x + (c + 0.5 - tie_i) * scale_x, tie_y - (r + 0.5 - tie_j) * scale_y: north-up rasters) and ``area_map`` = area * scale_x *
    scale_y in squared map units.  Floats are written with ``repr`` (they read back exactly)."""
    geo = georeference(profile)
    cols = list(TABLE_COLUMNS) + (["x", "y", "area_map"] if geo else [])
    n = len(table["root"])
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(cols)
        for i in range(n):
            row = [int(table[k][i]) for k in TABLE_COLUMNS[:8]]
            cr, cc = float(table["centroid_row"][i]), float(table["centroid_col"][i])
            row += [repr(cr), repr(cc)]
            if geo:
                sx, sy, ti, tj, tx, ty = geo
                row += [repr(tx + (cc + 0.5 - ti) * sx), repr(ty - (cr + 0.5 - tj) * sy), repr(int(table["area"][i]) * sx * sy)]
            w.writerow(row)
    return path
