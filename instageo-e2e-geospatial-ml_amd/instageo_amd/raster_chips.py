"""Chips cut against label rasters: the granule stack warped onto every label's grid, on the device.

The reference's second way into a dataset is ``instageo/data/raster_chip_creator.py`` with ``HLSRasterPipeline.process_row`` and
``geo_utils.slice_xr_dataset`` / ``create_grid_polygons``: every label is itself a small raster (``label_*.tif`` / ``mask_*.tif`` of
``chip_size`` x ``chip_size`` pixels in the user's coordinate system and resolution); stackstac resamples the satellite stack onto that
system and resolution (nearest neighbour), and the chip is sliced, masked, clipped and quality-checked against the label.  With
``is_bbox_feature`` the same code cuts label-free inference chips over bounding boxes.  This module is the stand-in on
:mod:`instageo_amd.tiff`, :mod:`instageo_amd.crs` and the kernel of ``raster_chips.hip``.

The rule (stated in ``include/instageo_hip.h``).  The centre of every pixel of a chip's S x S destination grid is mapped into the
stack's grid by the chain of the warp (:mod:`instageo_amd.warp`); it takes the T * C values and T Fmask bytes of the source pixel
(floor(v), floor(u)), or ``no_data_value`` and Fmask 0 outside the tile; then the rule of :func:`instageo_amd.chips.cut` applies
unchanged (masking, ``each`` / ``any``, clip, ``valid_values``, the validity plane).  A label map keeps its pixels except where its
validity bit is clear, or where a float label is NaN: those become -1.

Device tensors go through ``ig_chip_warp``; host arrays take a numpy twin of the same rule, so the module works (and is tested) without a
GPU.

The destination grid of a record.  ``snap=True`` (the reference): stackstac snaps the resampled stack to the lattice of multiples of
``spatial_resolution`` and ``slice_xr_dataset`` takes S pixels from the lattice cell that holds the top-left corner of the record's
bounds, so X = res * floor(minx / res), Y = res * ceil(maxy / res), in float64 on the host.  ``snap=False``: the label raster's own
grid.  Either way the written chip and label carry the label raster's georeferencing (the reference's ``xr.align(join="override")``).

Not done: STAC search and download, GeoPackage records (a CSV stands in), bilinear / cubic resampling of reflectances,
rotated rasters.  Sentinel-2 band planes of several resolutions under SCL masks (``S2RasterPipeline``) go through
:mod:`instageo_amd.s2_raster_chips`, Sentinel-1 RTC scenes stacked per date through :mod:`instageo_amd.s1_raster_chips`.
"""
from __future__ import annotations

import json
import os
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import crs as crsmod
from . import prep, tiff, warp
from .chips import VALID_BITS, mask_bits
from .prep import MAX_DATES, STRATEGIES, is_device, to_host  # noqa: F401

MAX_SIDE = 1 << 15
MAX_CLASSES = 128  # cells of the class histogram: every non-negative int8
HLS_NO_DATA = 0  # the reference's NO_DATA_VALUES.HLS
SEG_NO_DATA = -1
_BATCH_VALUES = 1 << 28  # chip values of one launch


def params(c) -> np.ndarray:
    """A coordinate system (EPSG code, :class:`crs.Crs` or five doubles) -> its five doubles."""
    if isinstance(c, (int, np.integer)) and not isinstance(c, bool):
        c = crsmod.from_epsg(int(c))
    a = np.ascontiguousarray(tuple(c)[:5], dtype=np.float64).reshape(-1)
    if a.shape[0] != 5:
        raise ValueError(f"a coordinate system is five doubles (got {a.shape[0]})")
    return a


def grid_ok(g) -> bool:
    return bool(np.isfinite(g).all() and g[2] > 0 and g[3] > 0)


# ---- argument checks shared by the host path and ops.chip_warp ------------------------------------------------------------------------------
def check_warp(tile_shape, fmask_shape, src_crs, src_grid, dst_crs, dst_grids, S: int, T: int, bits: int, strategy: str, no_data_value: int,
               clip, labels_shape, labels_dtype, valid_bit: int, K: int):
    """ValueError unless the arguments of a warped cut obey include/instageo_hip.h -> (src_crs (5,), src_grid (4,), dst_crs (5,),
    dst_grids (n, 4)) as float64 arrays.  A destination grid may be unusable (it gives a no-data chip); the stack's grid may not."""
    if isinstance(S, bool) or not isinstance(S, (int, np.integer)) or not 1 <= int(S) <= MAX_SIDE:
        raise ValueError(f"chip_size must be an int in [1, 2^15] (got {S!r})")
    S = int(S)
    TC, H, W = prep.check_stack_args(tile_shape, fmask_shape, S, T, bits, strategy, no_data_value, clip)
    if H < 1 or W < 1 or H * W > 2**31 - 1:
        raise ValueError(f"a tile of {H} x {W} pixels is beyond 2^31 - 1 (source offsets are int32)")
    sg = np.ascontiguousarray(src_grid, dtype=np.float64).reshape(-1)
    if sg.shape[0] != 4 or not grid_ok(sg):
        raise ValueError(f"src_grid = (X0, Y0, sx, sy) needs finite values and positive pixel sizes (got {tuple(sg)})")
    dg = check_dst(dst_grids, S, TC, labels_shape, labels_dtype, valid_bit, K)
    return params(src_crs), sg, params(dst_crs), dg


def check_dst(dst_grids, S: int, TC: int, labels_shape, labels_dtype, valid_bit: int, K: int) -> np.ndarray:
    """The checks of the destination grids and the labels of a warped cut of ``TC`` planes per chip, shared by :func:`check_warp` and
    :func:`s1_raster_chips.check_warp` -> dst_grids (n, 4) float64.  A destination grid may be unusable (it gives a no-data chip)."""
    dg = np.ascontiguousarray(dst_grids, dtype=np.float64)
    if dg.size % 4:
        raise ValueError(f"dst_grids is (n, 4) = (X0, Y0, sx, sy) per chip (got shape {dg.shape})")
    dg = dg.reshape(-1, 4)
    n = dg.shape[0]
    if n * TC * S * S >= 2**40:
        raise ValueError(f"{n} chips of {TC} x {S} x {S} values are beyond 2^40")
    if valid_bit not in (0, 1, 2):
        raise ValueError(f"valid_bit must be 0 none, 1 any or 2 each (got {valid_bit!r})")
    if isinstance(K, bool) or not 0 <= int(K) <= MAX_CLASSES:
        raise ValueError(f"a class histogram has 0 <= K <= {MAX_CLASSES} cells (got {K!r})")
    if labels_shape is None:
        if K:
            raise ValueError("a class histogram needs labels")
    else:
        if tuple(labels_shape) != (n, S, S):
            raise ValueError(f"labels must be (n, S, S) = {(n, S, S)} (got {tuple(labels_shape)})")
        if str(labels_dtype) not in ("int8", "float32"):
            raise ValueError(f"labels are int8 (seg) or float32 (reg) (got {labels_dtype})")
        if K and str(labels_dtype) != "int8":
            raise ValueError(f"a class histogram (K = {K}) needs int8 labels")
    return dg


# ---- the rule on host arrays ---------------------------------------------------------------------------------------------------------------
def _warp_host(tile, fmask, sc, sg, dc, dg, S, T, bits, strategy, nd, clip, labels, bit, K):
    """numpy twin of ``ig_chip_warp``: chip by chip, vectorised over the pixels."""
    TC, H, W = tile.shape
    C = TC // T
    n = dg.shape[0]
    chips = np.empty((n, TC, S, S), dtype=np.int16)
    validity = np.empty((n, S, S), dtype=np.uint8)
    for i in range(n):
        a = np.full((TC, S, S), nd, dtype=np.int16)
        f = np.zeros((T, S, S), dtype=np.uint8)
        if grid_ok(dg[i]):
            u, v = warp.coords(dc, dg[i], (S, S), sc, sg)
            with np.errstate(invalid="ignore"):
                fc, fr = np.floor(u), np.floor(v)
                inside = (fc >= 0) & (fc < W) & (fr >= 0) & (fr < H)
            rs, cs = fr[inside].astype(np.int64), fc[inside].astype(np.int64)
            a[:, inside] = tile[:, rs, cs]
            if fmask is not None:
                f[:, inside] = fmask[:, rs, cs]
        if fmask is not None and bits:
            m = (f & np.uint8(bits)) != 0
            m = np.broadcast_to(m.any(axis=0), (TC, S, S)) if strategy == "any" else np.repeat(m, C, axis=0)
            a[m] = nd
        if clip is not None:
            np.clip(a, clip[0], clip[1], out=a)
        ok = a != nd
        chips[i] = a
        validity[i] = ok.all(axis=0).astype(np.uint8) | (ok.any(axis=0).astype(np.uint8) << 1)
    valid_values = (chips != np.int16(nd)).reshape(n, -1).sum(axis=1).astype(np.int32)
    return (chips, valid_values, validity) + label_maps_host(labels, validity, bit, K)


def label_maps_host(labels, validity, bit: int, K: int):
    """The label step of the host twins (``ig_chip_warp``'s label maps): ``labels`` (n, S, S) int8 | float32 or None under the validity
    planes -> (maps, valid_labels (n,) int32, hist (n, K) int32 or None with K = 0); three None without labels."""
    maps = valid_labels = hist = None
    if labels is not None:
        n = labels.shape[0]
        maps = labels.copy()
        blank = (validity & bit) == 0 if bit else np.zeros(maps.shape, dtype=bool)
        if maps.dtype == np.float32:
            blank = blank | np.isnan(maps)
        maps[blank] = SEG_NO_DATA
        live = maps != SEG_NO_DATA
        valid_labels = live.sum(axis=(1, 2)).astype(np.int32)
        if K:
            hist = np.zeros((n, K), dtype=np.int32)
            for i in range(n):
                x = maps[i][live[i]].astype(np.int64)
                hist[i] = np.bincount(x[(x >= 0) & (x < K)], minlength=K)
    return maps, valid_labels, hist


def warp_cut(tile, fmask, src_crs, src_grid, dst_crs, dst_grids, chip_size: int, dates: Optional[int] = None,
             mask: Union[int, Sequence[str]] = 0, strategy: str = "each", no_data_value: int = 0, clip: Optional[Tuple[int, int]] = None,
             labels=None, label_strategy: Optional[str] = None, num_classes: int = 0):
    """The stack ``tile`` ((T * C, H, W) int16, with ``fmask`` (T, H, W) uint8 or None) in ``src_crs`` on ``src_grid`` = (X0, Y0, sx, sy),
    resampled (nearest) onto the n grids ``dst_grids`` ((n, 4)) of side ``chip_size`` in ``dst_crs``, masked and clipped by the rule of the
    module docstring -> (chips (n, T * C, S, S) int16, valid_values (n,) int32, validity (n, S, S) uint8, maps, valid_labels, hist).
    A coordinate system is an EPSG code, a :class:`crs.Crs` or five doubles.  ``labels``: None, or (n, S, S) int8 (``seg``) | float32
    (``reg``): ``maps`` are the labels with -1 where the validity bit of ``label_strategy`` (any | each | None: no masking) is clear and
    where a float label is NaN, ``valid_labels`` (n,) int32 the pixels != -1, ``hist`` (n, num_classes) int32 (int8 only; None with 0
    classes).  Without labels the last three are None.  Tensors on the device go through ``ig_chip_warp`` and give device tensors;
    anything else takes the numpy twin and gives arrays."""
    bits = mask if isinstance(mask, (int, np.integer)) and not isinstance(mask, bool) else mask_bits(mask)
    T = int(dates) if dates is not None else (int(fmask.shape[0]) if fmask is not None else 1)
    if label_strategy not in VALID_BITS:
        raise ValueError(f"label_strategy must be any, each or None (got {label_strategy!r})")
    bit = VALID_BITS[label_strategy] if labels is not None else 0
    dev = is_device(tile)
    name = lambda a: str(a.dtype).replace("torch.", "")  # noqa: E731
    if not dev:
        tile = np.asarray(tile.cpu() if hasattr(tile, "cpu") else tile)
        fmask = None if fmask is None else np.asarray(fmask.cpu() if hasattr(fmask, "cpu") else fmask)
        labels = None if labels is None else np.ascontiguousarray(labels.cpu() if hasattr(labels, "cpu") else labels)
    if name(tile) != "int16" or (fmask is not None and name(fmask) != "uint8"):
        raise ValueError("a tile is int16 and an Fmask uint8")
    if dev:
        from . import ops

        return ops.chip_warp(tile, fmask, src_crs, src_grid, dst_crs, dst_grids, chip_size, T, bits, strategy, no_data_value, clip, labels, bit,
                             int(num_classes))  # checks the same arguments before the upload
    sc, sg, dc, dg = check_warp(tuple(tile.shape), None if fmask is None else tuple(fmask.shape), src_crs, src_grid, dst_crs, dst_grids, chip_size,
                                T, bits, strategy, no_data_value, clip, None if labels is None else tuple(labels.shape),
                                None if labels is None else name(labels), bit, num_classes)
    return _warp_host(tile, fmask, sc, sg, dc, dg, int(chip_size), T, int(bits), strategy, int(no_data_value), clip, labels, bit, int(num_classes))


# ---- records and grids (float64 on the host) -------------------------------------------------------------------------------------------------
def complete_chips_coords(coord_min: float, coord_max: float, spatial_resolution: float, chip_size: int, max_bound: float) -> np.ndarray:
    """The reference's ``get_complete_chips_coords``: the pixel coordinates of as many whole chips as cover [coord_min, coord_max], one
    chip fewer when they would reach beyond ``max_bound``."""
    n_chips = int(np.ceil((coord_max - coord_min) / (spatial_resolution * chip_size)))
    n_pixels = n_chips * chip_size
    if coord_min + n_pixels * spatial_resolution > max_bound:
        n_pixels = (n_chips - 1) * chip_size
    return np.arange(coord_min, coord_min + n_pixels * spatial_resolution, spatial_resolution)


def grid_polygons(bbox_list, date: str, chip_size: int, spatial_resolution: float) -> List[Dict[str, Any]]:
    """The reference's ``create_grid_polygons`` on plain numpy: every [x_min, y_min, x_max, y_max] of ``bbox_list`` is covered with whole
    chips from its lower left corner (reduced by one chip where they would pass 180 / 90) -> records ``{"label_filename":
    "label_x{x}_y{y}_{date}.tif", "date", "bounds": (minx, miny, maxx, maxy)}``, x outer and y inner as in the reference.  The bounds
    are those of the chip's pixel COORDINATES (``get_extent``), S - 1 pixel steps wide; chip y counts upwards from y_min."""
    S = int(chip_size)
    out: List[Dict[str, Any]] = []
    for bbox in bbox_list:
        x_min, y_min, x_max, y_max = (float(v) for v in bbox)
        xs = complete_chips_coords(x_min, x_max, spatial_resolution, S, 180)
        ys = complete_chips_coords(y_min, y_max, spatial_resolution, S, 90)
        for x in range(len(xs) // S):
            for y in range(len(ys) // S):
                cx, cy = xs[x * S : (x + 1) * S], ys[y * S : (y + 1) * S]
                out.append({"label_filename": f"label_x{x}_y{y}_{date}.tif", "date": date,
                            "bounds": (float(cx.min()), float(cy.min()), float(cx.max()), float(cy.max()))})
    return out


def snapped_grid(bounds, spatial_resolution: float) -> Tuple[float, float, float, float]:
    """The destination grid of a record with ``bounds`` = (minx, miny, maxx, maxy) under ``snap=True`` (the module docstring)."""
    res = float(spatial_resolution)
    return (float(res * np.floor(bounds[0] / res)), float(res * np.ceil(bounds[3] / res)), res, res)


def chip_names(label_filename: str, mgrs_tile_id: str) -> Tuple[str, str]:
    """The reference's names: ``<label stem>_<mgrs_tile_id>.tif`` for the label map and the same with ``mask -> merged`` and
    ``label -> chip`` for the chip -> (chip name, label name)."""
    stem = f"{os.path.splitext(os.path.basename(str(label_filename)))[0]}_{mgrs_tile_id}"
    return stem.replace("mask", "merged").replace("label", "chip") + ".tif", stem + ".tif"


def mgrs_of(first_tile_file: str) -> str:
    """Field 2 of an HLS file name (``HLS.S30.T38PMB.2022145T072619.v2.0.B02.tif`` -> ``T38PMB``)."""
    return prep.hls_name(first_tile_file).tile


def read_records(records) -> List[Dict[str, Any]]:
    import pandas as pd

    df = pd.read_csv(records, dtype={"mgrs_tile_id": str}) if isinstance(records, (str, os.PathLike)) else pd.DataFrame(records)
    for col in ("label_filename", "date"):
        if col not in df.columns:
            raise ValueError(f"the records table needs the columns label_filename and date (no {col!r})")
    rows = []
    for _, r in df.iterrows():
        tid = r["mgrs_tile_id"] if "mgrs_tile_id" in df.columns and isinstance(r["mgrs_tile_id"], str) and r["mgrs_tile_id"] else None
        rows.append({"label_filename": str(r["label_filename"]), "date": r["date"], "mgrs_tile_id": tid})
    return rows


def touches(dc, grid, S: int, sc, sg, H: int, W: int) -> bool:
    """Whether the chip of ``grid`` can reach the tile: a 9 x 9 lattice over its extent, projected on the host; its box in source pixels,
    grown by one, against the tile.  A lattice wholly outside the domain cannot."""
    coarse = (grid[0], grid[1], grid[2] * S / 8.0, grid[3] * S / 8.0)
    u, v = warp.coords(dc, coarse, (8, 8), sc, sg, at="corners")
    if np.isnan(u).all():
        return False
    return bool(np.nanmax(u) + 1 >= 0 and np.nanmin(u) - 1 < W and np.nanmax(v) + 1 >= 0 and np.nanmin(v) - 1 < H)


def seg_labels(a: np.ndarray, name: str) -> np.ndarray:
    if a.dtype.kind == "f":
        a = np.where(np.isnan(a), SEG_NO_DATA, a)
    if a.size and ((a != np.round(a)).any() or a.min() < -128 or a.max() > 127):
        raise ValueError(f"{name}: seg labels must be integers that fit int8")
    return a.astype(np.int8)


def box_records(path: str, date: str, S: int, res: float) -> List[Dict[str, Any]]:
    """The records of the bounding-box case: :func:`grid_polygons` of the JSON list of boxes in ``path``, none of them naming a tile."""
    with open(path) as f:
        rows = grid_polygons(json.load(f), date, S, res)
    for r in rows:
        r["mgrs_tile_id"] = None
    return rows


def create_from_records(rows: List[Dict[str, Any]], own_id: str, dst: crsmod.Crs, touches: Callable[[Tuple[float, float, float, float]], bool],
                        labels_of: Optional[Callable[[np.ndarray, str], np.ndarray]], warp_cut_at: Callable[[List[Any], Any], Tuple],
                        chip_values: int, chip_dtype, histogram: bool, stats_name: str, output_directory: str, chip_size: int,
                        raster_path: Optional[str], spatial_resolution: float, snap: bool, qa_check: bool) -> Tuple[List[str], List[Optional[str]]]:
    """The pipeline the label-raster modes share (:func:`create_raster_chips`, :func:`s2_raster_chips.create_s2_raster_chips`) from the
    records on.  ``rows``: records of ``label_filename``, ``mgrs_tile_id`` (None: ``own_id``) and, in the bounding-box case, ``bounds``;
    ``labels_of(array, path)``: a label raster as the kernel takes it, None in the bounding-box case (chips only, with the georeferencing
    of their destination grid in ``dst``); ``touches(grid)``: whether a chip on that grid can reach the source; ``warp_cut_at(grids,
    labels)``: the six results of a warped cut, called for at most ``_BATCH_VALUES // chip_values`` records at a time.  A record of another
    tile is left alone, one whose files exist is skipped and still listed, a label raster that is not S x S or misses the source is not
    cut; with ``qa_check`` a chip with ``valid_values == 0`` is dropped, then a pair with ``valid_labels == 0``; the label map is written
    before its chip (as ``chip_dtype``).  Writes ``chips_dataset.csv`` and ``stats_name`` (with the class histogram when ``histogram``).
    -> (chip names, label-map names)."""
    S, res, bbox = int(chip_size), float(spatial_resolution), labels_of is None
    reasons = ("other_tile", "existing", "invalid_shape", "outside_tile", "no_valid_values", "no_valid_labels")
    stats: Dict[str, Any] = {"records": len(rows), "kept": 0, "dropped": {k: 0 for k in reasons}}
    chip_dir, seg_dir = os.path.join(output_directory, "chips"), os.path.join(output_directory, "seg_maps")
    os.makedirs(chip_dir, exist_ok=True)
    if not bbox:
        os.makedirs(seg_dir, exist_ok=True)
    chips_out: List[str] = []
    segs_out: List[Optional[str]] = []
    todo: List[Dict[str, Any]] = []
    for r in rows:
        tid = r["mgrs_tile_id"] or own_id
        if tid.lstrip("T") != own_id.lstrip("T"):
            stats["dropped"]["other_tile"] += 1
            continue
        cname, lname = chip_names(r["label_filename"], tid)
        have_chip = os.path.exists(os.path.join(chip_dir, cname))
        if have_chip and (bbox or os.path.exists(os.path.join(seg_dir, lname))):
            stats["dropped"]["existing"] += 1
            chips_out.append(cname)
            segs_out.append(None if bbox else lname)
            continue
        item: Dict[str, Any] = {"chip": cname, "label": lname}
        if bbox:
            b = r["bounds"]
            g = item["grid"] = snapped_grid(b, res) if snap else (b[0], b[1] + S * res, res, res)
            tags = dict(crsmod.geokeys(dst.epsg))
            tags[33550] = (12, (g[2], g[3], 0.0))
            tags[33922] = (12, (0.0, 0.0, 0.0, g[0], g[1], 0.0))
            item["profile"] = {"tags": tags, "nodata": None}
        else:
            path = os.path.join(raster_path, r["label_filename"])
            lab, lprof = tiff.read(path)
            found = crsmod.from_profile(lprof)
            if found.epsg != dst.epsg:
                raise ValueError(f"{path}: the label raster is in EPSG:{found.epsg}, src_crs is EPSG:{dst.epsg}")
            if lab.shape != (1, S, S):
                stats["dropped"]["invalid_shape"] += 1
                continue
            own = warp.grid_of(lprof, path)
            bounds = (own[0], own[1] - S * own[3], own[0] + S * own[2], own[1])
            item["grid"] = snapped_grid(bounds, res) if snap else own
            item["labels"] = labels_of(lab[0], path)
            item["profile"] = {"tags": prep.geo_tags(lprof["tags"], tiepoint=True), "nodata": None}
        if not touches(item["grid"]):
            stats["dropped"]["outside_tile"] += 1
            continue
        todo.append(item)
    hist_sum = np.zeros(MAX_CLASSES, dtype=np.int64) if histogram else None
    step = max(1, _BATCH_VALUES // chip_values)
    for first in range(0, len(todo), step):
        part = todo[first : first + step]
        out = warp_cut_at([it["grid"] for it in part], None if bbox else np.stack([it["labels"] for it in part]))
        chips, valid_values, _, maps, valid_labels, hist = (None if o is None else to_host(o) for o in out)
        for k, it in enumerate(part):
            if qa_check and valid_values[k] == 0:
                stats["dropped"]["no_valid_values"] += 1
                continue
            if qa_check and not bbox and valid_labels[k] == 0:
                stats["dropped"]["no_valid_labels"] += 1
                continue
            if not bbox:
                tiff.write(os.path.join(seg_dir, it["label"]), maps[k], it["profile"])
                if hist_sum is not None:
                    hist_sum += hist[k]
            tiff.write(os.path.join(chip_dir, it["chip"]), chips[k].astype(chip_dtype), it["profile"])
            chips_out.append(it["chip"])
            segs_out.append(None if bbox else it["label"])
            stats["kept"] += 1
    prep.write_dataset_csv(output_directory, chips_out, segs_out, bbox)
    if hist_sum is not None:
        stats.update(prep.class_stats(hist_sum, trim=True))
    prep.write_stats(os.path.join(output_directory, stats_name), stats)
    return chips_out, segs_out


def create_raster_chips(tile_files: Sequence[str], fmask_files: Optional[Sequence[str]], records, raster_path: Optional[str],
                        output_directory: str, chip_size: int = 256, mask_types: Sequence[str] = (), masking_strategy: str = "each",
                        src_crs: int = 4326, spatial_resolution: float = 0.0002694945852358564, qa_check: bool = True, task_type: str = "seg",
                        is_bbox_feature: bool = False, bbox_feature_path: Optional[str] = None, date: Optional[str] = None, snap: bool = True,
                        device: Optional[str] = None) -> Tuple[List[str], List[Optional[str]]]:
    """The reference's raster chip creator (``process_row``) for every record that touches one granule stack.  ``tile_files``: the HLS
    band files ordered per date and band, one Fmask file per date in ``fmask_files`` (read only when ``mask_types`` asks for masks).
    ``records``: a CSV path or a table with ``label_filename``, ``date`` and optionally ``mgrs_tile_id`` (default: field 2 of the HLS
    file name; a record that names another tile is left to that tile's run); the label rasters lie under ``raster_path``, S x S pixels
    in EPSG:``src_crs`` (a raster whose GeoKeys name another system raises ValueError); the geometry of a record is the bounds of its
    raster, from the file's own tiepoint and scale.  ``snap`` selects the destination grid (the module docstring).

    Writes ``chips/<chip name>`` (all bands, clipped to [0, 10000], uint16) and ``seg_maps/<label name>`` (int8 for ``seg``, float32 for
    ``reg``, NaN -> -1) under ``output_directory`` with the names of :func:`chip_names`, both with the label raster's georeferencing.  A
    record whose files both exist is skipped and still listed; a label raster that is not S x S is skipped (``invalid_shape``); a record
    whose raster misses the tile entirely is not cut (``outside_tile``); with ``qa_check`` a chip with ``valid_values == 0`` is dropped,
    then, after the label map was masked by the chip's validity (``masking_strategy``), a pair with ``valid_labels == 0``.
    ``chips_dataset.csv`` gains the pairs and ``raster_chips_stats.json`` holds the counts by reason, the class histogram and its
    ``compute_class_weights``.  -> (chip names, label-map names).

    ``is_bbox_feature``: no labels; the records are :func:`grid_polygons` of the JSON list of boxes in ``bbox_feature_path`` (``date``:
    the date of the names, by default that of the HLS file name); chips only, with the georeferencing of their destination grid
    (``snap=False``: the box lattice itself, pixel (0, 0) of chip y at the top of its S rows); an existing chip is skipped and listed.
    ``device``: None = the numpy path, ``"cuda"`` / ``"cuda:n"`` = the kernel; both write the same bytes."""
    S = int(chip_size)
    bits = mask_bits(mask_types)
    if masking_strategy not in STRATEGIES:
        raise ValueError(f"masking_strategy must be one of {tuple(STRATEGIES)} (got {masking_strategy!r})")
    if task_type not in ("seg", "reg"):
        raise ValueError(f"task_type must be seg or reg (got {task_type!r})")
    prep.check_device(device)
    if not tile_files:
        raise ValueError("create_raster_chips needs at least one tile file")
    if bits and not fmask_files:
        raise ValueError("mask_types needs fmask_files")
    res = float(spatial_resolution)
    if not 0 < res < np.inf:
        raise ValueError(f"spatial_resolution must be a positive number (got {spatial_resolution!r})")
    dst = crsmod.from_epsg(src_crs)
    T = len(fmask_files) if fmask_files else 1
    if len(tile_files) % T:
        raise ValueError(f"{len(tile_files)} band files do not divide into {T} dates")
    tile, profile = prep.read_stack(tile_files, "tile", np.int16)
    fmask = prep.read_stack(fmask_files, "Fmask", np.uint8)[0] if bits else None
    H, W = tile.shape[1:]
    src = crsmod.from_profile(profile)
    sgrid = warp.grid_of(profile, str(tile_files[0]))
    own_id = mgrs_of(tile_files[0])
    bbox = bool(is_bbox_feature)
    if bbox:
        if not bbox_feature_path:
            raise ValueError("is_bbox_feature needs bbox_feature_path")
        rows = box_records(bbox_feature_path, date or prep.hls_date(tile_files[0]), S, res)
    else:
        if raster_path is None:
            raise ValueError("label records need raster_path")
        rows = read_records(records)
    histogram = not bbox and task_type == "seg"
    staged: List[Any] = []  # the stack and its Fmask where the cut runs, uploaded with the first batch

    def warp_cut_at(grids, labels):
        if not staged:
            staged.extend(prep.stage(tile, fmask, device))
        return warp_cut(staged[0], staged[1], src, sgrid, dst, grids, S, dates=T, mask=bits, strategy=masking_strategy, no_data_value=HLS_NO_DATA,
                        clip=(0, 10000), labels=labels, label_strategy=masking_strategy if qa_check else None,
                        num_classes=MAX_CLASSES if histogram else 0)

    labels_of = None if bbox else seg_labels if task_type == "seg" else lambda a, path: a.astype(np.float32)
    return create_from_records(rows, own_id, dst, lambda grid: touches(dst, grid, S, src, sgrid, H, W), labels_of, warp_cut_at, tile.shape[0] * S * S,
                               np.uint16, histogram, "raster_chips_stats.json", output_directory, S, raster_path, res, snap, qa_check)


# ---- mode=create_raster_chips --------------------------------------------------------------------------------------------------------------
CONFIG_KEYS = ("tiles", "fmasks", "records_file", "raster_path", "output_directory", "chip_size", "mask_types", "masking_strategy", "src_crs",
               "spatial_resolution", "qa_check", "task_type", "is_bbox_feature", "bbox_feature_path", "date", "snap")


def raster_chips_options(cfg: Dict[str, Any]) -> Dict[str, Any]:
    """The ``raster_chips.*`` keys of ``mode=create_raster_chips`` checked -> the keyword arguments of :func:`create_raster_chips`.  An
    unknown key or a bad value raises ValueError; the files are required only in that mode."""
    c = prep.Section(cfg, "raster_chips", CONFIG_KEYS)
    size = c.integer("chip_size", 256, lo=1, hi=MAX_SIDE, what="must be an int in [1, 2^15]")
    types = c.listing("mask_types", []) or []
    mask_bits(types)
    strategy = c.choice("masking_strategy", "each", STRATEGIES)
    task = c.choice("task_type", "seg", ("seg", "reg"), "must be seg or reg")
    src = c.epsg("src_crs", 4326)
    res = c.number("spatial_resolution", 0.0002694945852358564, lambda x: 0 < x < np.inf, "must be a positive number")
    tiles, fmasks = c.listing("tiles"), c.listing("fmasks")
    bbox = c.flag("is_bbox_feature", False)
    opts = dict(tile_files=tiles, fmask_files=fmasks, records=c.text("records_file"), raster_path=c.text("raster_path"),
                output_directory=c.text("output_directory"), chip_size=size, mask_types=types, masking_strategy=strategy, src_crs=src,
                spatial_resolution=res, qa_check=c.flag("qa_check", True), task_type=task, is_bbox_feature=bbox,
                bbox_feature_path=c.text("bbox_feature_path"), date=c.text("date"), snap=c.flag("snap", True))
    if cfg.get("mode") == "create_raster_chips":
        if not tiles or opts["output_directory"] is None:
            raise ValueError("mode=create_raster_chips needs raster_chips.tiles and raster_chips.output_directory")
        if types and not fmasks:
            raise ValueError("raster_chips.mask_types needs raster_chips.fmasks (one Fmask file per date)")
        if bbox and opts["bbox_feature_path"] is None:
            raise ValueError("raster_chips.is_bbox_feature needs raster_chips.bbox_feature_path")
        if not bbox and (opts["records"] is None or opts["raster_path"] is None):
            raise ValueError("mode=create_raster_chips needs raster_chips.records_file and raster_chips.raster_path (or is_bbox_feature)")
    return opts


def run_from_config(cfg: Dict[str, Any], device: Optional[str] = None) -> int:
    """``mode=create_raster_chips``: :func:`create_raster_chips` under the ``raster_chips.*`` keys; prints one JSON line with the counts."""
    return prep.run_creator("create_raster_chips", create_raster_chips, raster_chips_options(cfg), device)


def main(argv: Optional[List[str]] = None) -> int:
    """``python -m instageo_amd.raster_chips raster_chips.tiles=a.tif,b.tif raster_chips.output_directory=out ...``:
    mode=create_raster_chips without ``run.py``."""
    return prep.run_mode_cli("create_raster_chips", run_from_config, argv)


if __name__ == "__main__":
    raise SystemExit(main())
