"""Chips and label maps cut from HLS tiles, on the device.

Every entry point of ``run.py`` starts from a CSV of ``chip_*.tif`` / ``seg_map_*.tif`` pairs.  The reference makes those pairs in
``instageo/data`` (``data_pipeline.py``: ``apply_mask``, ``create_segmentation_map``, ``mask_segmentation_map``, ``get_chip_coords`` and
the loop of ``create_and_save_chips_with_seg_maps``; ``hls_utils.py``: ``decode_fmask_value``) on xarray, rioxarray, geopandas and
rasterio.  This module is the stand-in on top of :mod:`instageo_amd.tiff`, :mod:`instageo_amd.crs` and the kernels of ``chips.hip``.

The rule (stated in ``include/instageo_hip.h``).  A tile is (T * C, H, W) int16, band b of date b // C, with an Fmask (T, H, W) uint8.
Date t is masked at a pixel when ``fmask[t] & mask_bits != 0`` (``mask_bits``: the OR of ``1 << position``; cloud 1,
near_cloud_or_shadow 2, cloud_shadow 3, water 5).  ``each``: the C bands of a masked date become ``no_data_value``; ``any``: all bands
where any date is masked; clipping comes after masking.  A chip is an S x S window wholly inside the tile; with it come
``valid_values`` (its values that differ from ``no_data_value``) and a validity plane (bit 0: all values of the pixel differ, bit 1: at
least one).  A label map paints, for every point of the chip, the window of half-width w around it clipped to the chip; where windows
overlap the point with the largest original index wins; pixels without a point, and pixels whose validity bit is clear, are -1.

Device tensors go through ``ig_chip_cut`` / ``ig_chip_labels``; host arrays take a numpy twin of the same rule, so the module works
(and is tested) without a GPU.

A quirk of the reference kept on purpose: a point nominates its chip by the floor rule (col = floor((x - X0) / sx), chip = col // S),
but paints only when it lies inside the chip's pixel-centre bounds ([centre of the first column, centre of the last column] x [centre of
the first row, centre of the last row]), because the reference filters a chip's points with ``chip["x"].min() <= x <= chip["x"].max()``
on pixel-centre coordinates.  A point in the outer half-pixel fringe of a chip therefore selects the chip without labelling it.

Not done: STAC search and download, the S1 source, MGRS tile lookup, rotated rasters, and CSR point lists built on the device.  The
label-raster pipeline, which resamples a tile to another grid, is :mod:`instageo_amd.raster_chips`; Sentinel-2 L2A tiles, whose bands
differ in resolution and whose mask is a class raster, go through :mod:`instageo_amd.s2_chips`.
"""
from __future__ import annotations

import os
from typing import Any, Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np

from . import crs as crsmod
from . import prep, tiff, warp
from .prep import MAX_DATES, STRATEGIES, is_device, to_host  # noqa: F401  (the masking strategies and the date limit of include/instageo_hip.h)

MASK_POSITIONS = {"HLS": {"cloud": 1, "near_cloud_or_shadow": 2, "cloud_shadow": 3, "water": 5}}
NO_DATA_VALUE = 0  # of the written chips when the caller names none (create_chips; maptiles.merge_chips reads it for files without a tag)
VALID_BITS = {None: 0, "any": 1, "each": 2}  # the bit of the validity plane a label strategy looks at
MAX_CLASSES = 256
MAX_WINDOW = 1 << 20
SEG_NO_DATA = -1  # the reference's NO_DATA_VALUES.SEG_MAP


def decode_fmask_value(value, position: int):
    """Bit ``position`` of an Fmask value (the reference's ``decode_fmask_value``: ``quotient - (quotient // 2) * 2``)."""
    return (np.asarray(value) >> position) & 1


def mask_bits(mask_types: Sequence[str], data_source: str = "HLS") -> int:
    """The OR of ``1 << position`` over ``mask_types``.  ValueError for an unknown type, or a source whose masks are not single bits."""
    if data_source != "HLS":
        raise ValueError(f"mask types of data source {data_source!r} are not supported (S2 masks are lists of SCL classes, not Fmask "
                         "bits; HLS only)")
    if isinstance(mask_types, str):
        raise ValueError(f"mask_types is a list of names (got the string {mask_types!r})")
    bits = 0
    for m in mask_types:
        if m not in MASK_POSITIONS["HLS"]:
            raise ValueError(f"unknown mask type {m!r}: one of {sorted(MASK_POSITIONS['HLS'])}")
        bits |= 1 << MASK_POSITIONS["HLS"][m]
    return bits


# ---- argument checks shared by the host path and the device wrappers (ops.chip_cut / ops.chip_labels) -----------------------------------
def check_cut(tile_shape, fmask_shape, origins, S: int, T: int, bits: int, strategy: str, no_data_value: int, clip) -> np.ndarray:
    """ValueError unless the arguments of a cut obey include/instageo_hip.h -> origins as an (n, 2) int32 array."""
    if isinstance(S, bool) or int(S) < 1:
        raise ValueError(f"chip_size must be an int >= 1 (got {S!r})")
    _, H, W = prep.check_stack_args(tile_shape, fmask_shape, int(S), T, bits, strategy, no_data_value, clip)
    if S > H or S > W:
        raise ValueError(f"a chip of side {S} does not fit a tile of {H} x {W} pixels")
    return prep.check_origins(origins, S, H, W, "tile of")


def check_labels(origins, S: int, ptr, pts, P: int, w: int, K: int, task_type: str, label_strategy) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """ValueError unless the arguments of a label-map launch obey include/instageo_hip.h -> (origins, ptr, pts) as int32 arrays."""
    if isinstance(S, bool) or int(S) < 1:
        raise ValueError(f"chip_size must be an int >= 1 (got {S!r})")
    if task_type not in ("seg", "reg"):
        raise ValueError(f"task_type must be seg or reg (got {task_type!r})")
    if isinstance(w, bool) or not 0 <= int(w) <= MAX_WINDOW:
        raise ValueError(f"window_size must be an int in [0, 2^20] (got {w!r})")
    if not 0 <= int(K) <= MAX_CLASSES or (K and task_type != "seg"):
        raise ValueError(f"a class histogram has 0 <= K <= {MAX_CLASSES} cells and goes with task_type seg (got K = {K!r}, {task_type})")
    if label_strategy not in VALID_BITS:
        raise ValueError(f"label_strategy must be any, each or None (got {label_strategy!r})")
    o = np.ascontiguousarray(np.asarray(origins, dtype=np.int64).reshape(-1, 2), dtype=np.int32)
    n = o.shape[0]
    ptr = np.asarray(ptr, dtype=np.int64).reshape(-1)
    pts = np.asarray(pts, dtype=np.int64).reshape(-1, 3)
    if ptr.shape[0] != n + 1 or ptr[0] != 0 or (np.diff(ptr) < 0).any() or ptr[-1] != pts.shape[0]:
        raise ValueError(f"ptr must hold {n} + 1 ascending offsets into the points, from 0 to their number ({pts.shape[0]})")
    if pts.shape[0] > 2**31 - 1:
        raise ValueError("too many points for int32 lists")
    if pts.shape[0]:
        chip = np.repeat(np.arange(n), np.diff(ptr))
        rel = pts[:, :2] - o[chip].astype(np.int64)
        if (rel < 0).any() or (rel >= S).any():
            raise ValueError("a point lies outside the chip it is listed under")
        if pts[:, 2].min() < 0 or pts[:, 2].max() >= P:
            raise ValueError(f"a point's original index lies outside the {P} labels")
    return o, np.ascontiguousarray(ptr, dtype=np.int32), np.ascontiguousarray(pts, dtype=np.int32)


# ---- the rule on host arrays ---------------------------------------------------------------------------------------------------------------
def _cut_host(tile: np.ndarray, fmask: Optional[np.ndarray], origins: np.ndarray, S: int, T: int, bits: int, strategy: str, nd: int, clip):
    """numpy twin of ``ig_chip_cut``: chip by chip, vectorised over the pixels."""
    TC = tile.shape[0]
    C = TC // T
    n = origins.shape[0]
    chips = np.empty((n, TC, S, S), dtype=np.int16)
    validity = np.empty((n, S, S), dtype=np.uint8)
    for i, (r0, c0) in enumerate(origins.tolist()):
        a = tile[:, r0 : r0 + S, c0 : c0 + S].copy()
        if fmask is not None and bits:
            m = (fmask[:, r0 : r0 + S, c0 : c0 + S] & np.uint8(bits)) != 0  # (T, S, S)
            m = np.broadcast_to(m.any(axis=0), (TC, S, S)) if strategy == "any" else np.repeat(m, C, axis=0)
            a[m] = nd
        if clip is not None:
            np.clip(a, clip[0], clip[1], out=a)
        ok = a != nd
        chips[i] = a
        validity[i] = ok.all(axis=0).astype(np.uint8) | (ok.any(axis=0).astype(np.uint8) << 1)
    valid_values = (chips != np.int16(nd)).reshape(n, -1).sum(axis=1).astype(np.int32)
    return chips, valid_values, validity


def _labels_host(origins, S, ptr, pts, labels, w, validity, bit, K):
    """numpy twin of ``ig_chip_labels``: point by point in ascending original index (a later window overwrites), one slice per window."""
    n = origins.shape[0]
    maps = np.full((n, S, S), SEG_NO_DATA, dtype=labels.dtype)
    for i in range(n):
        mine = pts[ptr[i] : ptr[i + 1]]
        r0, c0 = origins[i]
        for row, col, idx in mine[np.argsort(mine[:, 2], kind="stable")].tolist():
            pr, pc = row - r0, col - c0
            maps[i, max(pr - w, 0) : min(pr + w, S - 1) + 1, max(pc - w, 0) : min(pc + w, S - 1) + 1] = labels[idx]
    if bit:
        maps[(validity & bit) == 0] = SEG_NO_DATA
    live = maps != SEG_NO_DATA
    valid_labels = live.reshape(n, -1).sum(axis=1).astype(np.int32)
    hist = None
    if K:
        hist = np.zeros((n, K), dtype=np.int32)
        for i in range(n):
            v = maps[i][live[i]].astype(np.int64)
            v = v[(v >= 0) & (v < K)]
            hist[i] = np.bincount(v, minlength=K)
    return maps, valid_labels, hist


# ---- building blocks on arrays and tensors -------------------------------------------------------------------------------------------------
def cut(tile, fmask, origins, chip_size: int, dates: Optional[int] = None, mask: Union[int, Sequence[str]] = 0, strategy: str = "each",
        no_data_value: int = 0, clip: Optional[Tuple[int, int]] = None):
    """Chips of side ``chip_size`` at ``origins`` ((n, 2): row0, col0) of ``tile`` ((T * C, H, W) int16) under ``fmask`` ((T, H, W) uint8 or
    None) -> (chips (n, T * C, S, S) int16, valid_values (n,) int32, validity (n, S, S) uint8) by the rule of the module docstring.
    ``dates``: T, by default that of ``fmask`` (1 without one); ``mask``: the bits, or a list of mask types for :func:`mask_bits`;
    ``clip``: None or (lo, hi).  Tensors on the device go through ``ig_chip_cut`` and give device tensors; anything else takes the numpy
    twin and gives arrays."""
    bits = mask if isinstance(mask, (int, np.integer)) and not isinstance(mask, bool) else mask_bits(mask)
    T = int(dates) if dates is not None else (int(fmask.shape[0]) if fmask is not None else 1)
    dev = is_device(tile)
    if not dev:
        tile = np.asarray(tile.cpu() if hasattr(tile, "cpu") else tile)
        fmask = None if fmask is None else np.asarray(fmask.cpu() if hasattr(fmask, "cpu") else fmask)
    if np.dtype(str(tile.dtype).replace("torch.", "")) != np.int16 or (fmask is not None and np.dtype(str(fmask.dtype).replace("torch.", "")) != np.uint8):
        raise ValueError("a tile is int16 and an Fmask uint8")
    if not dev:
        o = check_cut(tuple(tile.shape), None if fmask is None else tuple(fmask.shape), origins, chip_size, T, bits, strategy, no_data_value, clip)
        return _cut_host(tile, fmask, o, int(chip_size), T, int(bits), strategy, int(no_data_value), clip)
    from . import ops

    return ops.chip_cut(tile, fmask, origins, chip_size, T, bits, strategy, no_data_value, clip)  # checks the same arguments before the upload


def label_maps(origins, chip_size: int, ptr, pts, labels, window_size: int = 0, validity=None, label_strategy: Optional[str] = "any",
               task_type: str = "seg", num_classes: int = 0, device: Optional[str] = None):
    """Label maps of the chips at ``origins``: ``pts`` ((m, 3): row, col on the tile, original index) grouped by chip through ``ptr``
    (CSR), ``labels`` (P,) looked up by the original index -> (maps (n, S, S) int16 for ``seg`` / float32 for ``reg``, valid_labels (n,)
    int32, hist (n, num_classes) int32 or None).  ``validity``: the plane of :func:`cut` (None: no masking) read at the bit of
    ``label_strategy`` (any | each).  ``labels`` is a host array (the point lists are built on the host).  A ``validity`` tensor on the
    device selects ``ig_chip_labels``; without a plane ``device`` does (None: the numpy twin)."""
    if task_type not in ("seg", "reg"):
        raise ValueError(f"task_type must be seg or reg (got {task_type!r})")
    dt = np.int16 if task_type == "seg" else np.float32
    dev = is_device(validity) if validity is not None else device is not None
    S, w, K = int(chip_size), window_size, int(num_classes)
    strat = label_strategy if validity is not None else None
    lab_host = np.asarray(labels)
    if task_type == "seg" and lab_host.size and lab_host.dtype.kind in "iuf":
        if (lab_host != lab_host.astype(np.int16)).any():
            raise ValueError("seg labels must be integers that fit int16")
    lab_host = np.ascontiguousarray(lab_host.astype(dt))
    if label_strategy not in VALID_BITS:
        raise ValueError(f"label_strategy must be any, each or None (got {label_strategy!r})")
    n = np.asarray(origins).reshape(-1, 2).shape[0]
    if validity is not None and tuple(validity.shape) != (n, S, S):
        raise ValueError(f"validity must be (n, S, S) = {(n, S, S)} (got {tuple(validity.shape)})")
    if not dev:
        o, p, q = check_labels(origins, S, ptr, pts, lab_host.shape[0], w, K, task_type, strat)
        v = None if validity is None else np.asarray(validity.cpu() if hasattr(validity, "cpu") else validity)
        return _labels_host(o, S, p, q, lab_host, int(w), v, VALID_BITS[strat], K)
    from . import ops

    # checks the same arguments before the upload
    return ops.chip_labels(origins, S, ptr, pts, lab_host, w, validity, VALID_BITS[strat], K, device=validity.device if validity is not None else device)


# ---- point geometry (float64 on the host) ---------------------------------------------------------------------------------------------------
def locate_points(x, y, src_crs, profile: Dict[str, Any], shape: Tuple[int, int]):
    """Points (x, y) of ``src_crs`` (an EPSG code or :class:`crs.Crs`) on the tile of ``profile`` / ``shape`` = (H, W) -> (keep, rows, cols,
    tx, ty): the indices of the points inside the tile's pixel-centre bounds, their pixels row = floor((Y0 - y) / sy),
    col = floor((x - X0) / sx), and their coordinates in the tile's system."""
    H, W = int(shape[0]), int(shape[1])
    dst = crsmod.from_profile(profile)
    src = src_crs if isinstance(src_crs, crsmod.Crs) else crsmod.from_epsg(int(src_crs))
    X0, Y0, sx, sy = warp.grid_of(profile, "the tile")
    tx, ty = crsmod.transform(src, dst, np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
    xmin, xmax = X0 + 0.5 * sx, X0 + (W - 0.5) * sx
    ymax, ymin = Y0 - 0.5 * sy, Y0 - (H - 0.5) * sy
    keep = np.nonzero((xmin <= tx) & (tx <= xmax) & (ymin <= ty) & (ty <= ymax))[0]
    tx, ty = tx[keep], ty[keep]
    cols = np.floor((tx - X0) / sx).astype(np.int64)
    rows = np.floor((Y0 - ty) / sy).astype(np.int64)
    return keep, rows, cols, tx, ty


def group_points(rows, cols, tx, ty, index, chip_size: int, shape: Tuple[int, int], grid: Tuple[float, float, float, float]):
    """The unique chips (col // S, row // S) the points nominate, in the order of ``np.unique`` (by column index, then row index), without
    those at index >= W // S or H // S -> (chip_xy (n, 2) = (x, y) chip indices, skipped: the nominated chips beyond the grid, ptr, pts):
    the CSR lists of the points that PAINT, in stable original order: those inside their chip's pixel-centre bounds (the module docstring's
    quirk)."""
    S = int(chip_size)
    H, W = int(shape[0]), int(shape[1])
    X0, Y0, sx, sy = grid
    rows, cols, index = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64), np.asarray(index, dtype=np.int64)
    if rows.size == 0:
        return np.zeros((0, 2), dtype=np.int64), 0, np.zeros(1, dtype=np.int32), np.zeros((0, 3), dtype=np.int32)
    cxy = np.stack((cols // S, rows // S), axis=-1)
    uniq, inv = np.unique(cxy, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    inside = (uniq[:, 0] < W // S) & (uniq[:, 1] < H // S)
    new_id = np.cumsum(inside) - 1
    chip_xy = uniq[inside]
    c0, r0 = cxy[:, 0] * S, cxy[:, 1] * S
    paints = ((X0 + (c0 + 0.5) * sx <= tx) & (tx <= X0 + (c0 + S - 0.5) * sx) & (Y0 - (r0 + S - 0.5) * sy <= ty) & (ty <= Y0 - (r0 + 0.5) * sy))
    sel = np.nonzero(inside[inv] & paints)[0]
    chip_of = new_id[inv[sel]]
    order = np.lexsort((index[sel], chip_of))  # by chip, then original index
    sel, chip_of = sel[order], chip_of[order]
    ptr = np.concatenate([[0], np.cumsum(np.bincount(chip_of, minlength=chip_xy.shape[0]))]).astype(np.int32)
    pts = np.stack((rows[sel], cols[sel], index[sel]), axis=-1).astype(np.int32)
    return chip_xy, int((~inside).sum()), ptr, pts


# ---- files -> files -------------------------------------------------------------------------------------------------------------------------
def tile_id_of(first_tile_file: str) -> str:
    """The reference's tile id of an HLS file name: fields 1..3 of ``HLS.S30.T38PMB.2022145T072619.v2.0.B02.tif``."""
    return "_".join(prep.hls_name(first_tile_file))


def _read_points(points) -> Dict[str, np.ndarray]:
    import pandas as pd

    df = pd.read_csv(points) if isinstance(points, (str, os.PathLike)) else pd.DataFrame(points)
    for col in ("x", "y", "label", "date"):
        if col not in df.columns:
            raise ValueError(f"the points table needs the columns x, y, label, date (no {col!r})")
    return {"x": df["x"].to_numpy(dtype=np.float64), "y": df["y"].to_numpy(dtype=np.float64), "label": df["label"].to_numpy(),
            "date": pd.to_datetime(df["date"])}


def _chip_profile(profile: Dict[str, Any], grid, r0: int, c0: int) -> Dict[str, Any]:
    X0, Y0, sx, sy = grid
    tags = prep.geo_tags(profile["tags"], tiepoint=False)
    tags[33922] = (12, (0.0, 0.0, 0.0, X0 + c0 * sx, Y0 - r0 * sy, 0.0))
    return {"tags": tags, "nodata": None}


class PointSource(NamedTuple):
    """What a point mode has read and staged, as :func:`create_from_points` takes it."""

    profile: Dict[str, Any]  # the lattice the chips are cut on, as a raster profile
    grid: Tuple[float, float, float, float]  # (X0, Y0, sx, sy) of the lattice
    shape: Tuple[int, int]  # its (H, W)
    tile_id: str
    date: Optional[str]  # the YYYYMMDD of the names in the bounding-box case when the caller gives none
    noun: str  # of "no point lies inside the ..."
    cut: Callable[[np.ndarray, bool], Tuple[Any, Any, Any]]  # (origins, bbox) -> (chips, valid_values, validity)
    bbox_dtype: Optional[Any]  # what a bounding-box chip is written as (None: as cut)


def create_from_points(source: PointSource, points, output_directory: str, chip_size: int, window_size: int, task_type: str, src_crs,
                       label_strategy: Optional[str], num_classes: Optional[int], date: Optional[str]) -> Tuple[List[str], List[Optional[str]]]:
    """The pipeline the point modes share (:func:`create_chips`, :func:`s2_chips.create_s2_chips`, :func:`s1_chips.create_s1_chips`) from
    the lattice of ``source`` on: the chips the ``points`` nominate (None: every complete chip of the lattice), without those whose files
    exist, cut by one call of ``source.cut``; their label maps, masked at the validity bit of ``label_strategy``; a chip is dropped when
    ``valid_values == 0``, then a pair when ``valid_labels == 0``; the label map is written before its chip; ``chips_dataset.csv`` and
    ``chips_stats.json``.  ``num_classes`` None: the largest label + 1, ``MAX_CLASSES`` at most.  -> (chip names, label-map names)."""
    S = int(chip_size)
    profile, grid, (H, W), tile_id = source.profile, source.grid, source.shape, source.tile_id
    stats: Dict[str, Any] = {"nominated": 0, "kept": 0, "dropped": {"out_of_bounds": 0, "existing": 0, "no_valid_values": 0, "no_valid_labels": 0}}
    bbox = points is None
    if bbox:
        chip_xy = np.array([(cx, cy) for cx in range(W // S) for cy in range(H // S)], dtype=np.int64).reshape(-1, 2)
        date_id = date or source.date
        ptr = pts = labels = None
    else:
        tab = _read_points(points)
        keep, rows, cols, tx, ty = locate_points(tab["x"], tab["y"], src_crs, profile, (H, W))
        if keep.size == 0:
            raise ValueError(f"no point lies inside the {source.noun}")
        date_id = date or tab["date"].iloc[int(keep[0])].strftime("%Y%m%d")
        labels = np.asarray(tab["label"])
        chip_xy, beyond, ptr, pts = group_points(rows, cols, tx, ty, keep, S, (H, W), grid)
        stats["dropped"]["out_of_bounds"] = beyond
        stats["nominated"] = beyond
    stats["nominated"] += int(chip_xy.shape[0])
    chip_dir, seg_dir = os.path.join(output_directory, "chips"), os.path.join(output_directory, "seg_maps")
    os.makedirs(chip_dir, exist_ok=True)
    if not bbox:
        os.makedirs(seg_dir, exist_ok=True)
    names = [(f"chip_{date_id}_{tile_id}_{x}_{y}.tif", f"seg_map_{date_id}_{tile_id}_{x}_{y}.tif") for x, y in chip_xy.tolist()]
    fresh = np.array([not (os.path.exists(os.path.join(chip_dir, c)) or (not bbox and os.path.exists(os.path.join(seg_dir, s))))
                      for c, s in names], dtype=bool)
    stats["dropped"]["existing"] = int((~fresh).sum())
    sel = np.nonzero(fresh)[0]
    origins = np.stack((chip_xy[sel, 1] * S, chip_xy[sel, 0] * S), axis=-1).astype(np.int32).reshape(-1, 2)
    chips_out: List[str] = []
    segs_out: List[Optional[str]] = []
    hist_sum = None
    if sel.size:
        chips, valid_values, validity = source.cut(origins, bbox)
        valid_values = to_host(valid_values)
        maps = valid_labels = hist = None
        if not bbox:
            # the lists of the chips that are cut: the rows of the fresh ones, re-based
            cnt = np.diff(ptr)[sel]
            take = np.concatenate([np.arange(ptr[i], ptr[i + 1]) for i in sel])
            sub_ptr = np.concatenate([[0], np.cumsum(cnt)])
            lab = labels.astype(np.float32) if task_type == "reg" else labels
            K = int(num_classes) if num_classes is not None else 0
            if task_type == "seg" and num_classes is None:
                K = int(min(max(int(np.max(lab)) + 1, 1), MAX_CLASSES)) if lab.size else 1
            maps, valid_labels, hist = label_maps(origins, S, sub_ptr, pts[take.astype(np.int64)], lab, window_size, validity, label_strategy,
                                                  task_type, K if task_type == "seg" else 0)
            maps, valid_labels = to_host(maps), to_host(valid_labels)
            if hist is not None:
                hist_sum = np.zeros(K, dtype=np.int64)
                hist = to_host(hist)
        for k, i in enumerate(sel.tolist()):
            if valid_values[k] == 0:  # the reference's "no valid data pixels"
                stats["dropped"]["no_valid_values"] += 1
                continue
            if not bbox and valid_labels[k] == 0:  # "empty label"
                stats["dropped"]["no_valid_labels"] += 1
                continue
            prof = _chip_profile(profile, grid, int(origins[k, 0]), int(origins[k, 1]))
            chip = to_host(chips[k])
            if bbox:
                if source.bbox_dtype is not None:
                    chip = chip.astype(source.bbox_dtype)
                segs_out.append(None)
            else:
                tiff.write(os.path.join(seg_dir, names[i][1]), maps[k], prof)
                segs_out.append(names[i][1])
                if hist_sum is not None:
                    hist_sum += hist[k]
            tiff.write(os.path.join(chip_dir, names[i][0]), chip, prof)
            chips_out.append(names[i][0])
    stats["kept"] = len(chips_out)
    prep.write_dataset_csv(output_directory, chips_out, segs_out, bbox)
    if hist_sum is not None:
        stats.update(prep.class_stats(hist_sum))
    prep.write_stats(os.path.join(output_directory, "chips_stats.json"), stats)
    return chips_out, segs_out


def create_chips(tile_files: Sequence[str], fmask_files: Optional[Sequence[str]], points, output_directory: str, chip_size: int = 256,
                 mask_types: Sequence[str] = (), masking_strategy: str = "each", window_size: int = 0, task_type: str = "seg",
                 src_crs: int = 4326, no_data_value: int = NO_DATA_VALUE, num_classes: Optional[int] = None, device: Optional[str] = None,
                 date: Optional[str] = None) -> Tuple[List[str], List[Optional[str]]]:
    """The reference's chip creator for one HLS tile.  ``tile_files``: the band files ordered per date and band (``B02_0``, ``B03_0``,
    ...), one Fmask file per date in ``fmask_files`` (read only when ``mask_types`` asks for masks); ``points``: a CSV path or a table with
    ``x``, ``y`` (in EPSG:``src_crs``), ``label``, ``date``.  Writes ``chips/chip_{date}_{tile_id}_{x}_{y}.tif`` (int16, all bands) and
    ``seg_maps/seg_map_{...}.tif`` (int16 for ``seg``, float32 for ``reg``) under ``output_directory`` for every chip a point nominates,
    each with its own tiepoint and the tile's GeoKey tags; a chip is dropped when ``valid_values == 0``, then a pair when
    ``valid_labels == 0``; a chip whose file (or label file) exists is skipped.  ``chips_dataset.csv`` (``Input`` / ``Label``, relative
    paths: what ``dataloader.get_valid_filepaths`` reads) gains the new pairs and ``chips_stats.json`` holds the counts of this run by
    reason, the summed class histogram (``num_classes`` cells; None: the largest label + 1) and its ``compute_class_weights``.
    -> (chip names, label-map names).

    ``points=None`` (the reference's bounding-box case, for inference): every complete chip of the grid that has a valid value, clipped to
    [0, 10000] and written as uint16, no label maps (-> names, a list of None); ``date``: the YYYYMMDD of the names, by default from the
    HLS file name.  ``device``: None = the numpy path, ``"cuda"`` / ``"cuda:n"`` = the kernels; both write the same bytes.
    ``no_data_value``, ``num_classes`` and ``date`` have no ``chips.*`` config key (the keys are the reference's flags): tiles whose
    no-data value is not 0 go through this function from Python."""
    S = int(chip_size)
    bits = mask_bits(mask_types)
    if masking_strategy not in STRATEGIES:
        raise ValueError(f"masking_strategy must be one of {tuple(STRATEGIES)} (got {masking_strategy!r})")
    if task_type not in ("seg", "reg"):
        raise ValueError(f"task_type must be seg or reg (got {task_type!r})")
    prep.check_device(device)
    if not tile_files:
        raise ValueError("create_chips needs at least one tile file")
    use_mask = bool(bits) and fmask_files
    if bits and not fmask_files:
        raise ValueError("mask_types needs fmask_files")
    T = len(fmask_files) if fmask_files else 1
    if len(tile_files) % T:
        raise ValueError(f"{len(tile_files)} band files do not divide into {T} dates")
    tile_id = tile_id_of(tile_files[0])
    tile, profile = prep.read_stack(tile_files, "tile", np.int16)
    fmask = prep.read_stack(fmask_files, "Fmask", np.uint8)[0] if use_mask else None
    H, W = tile.shape[1:]
    grid = warp.grid_of(profile, str(tile_files[0]))
    def cut_at(origins, bbox):
        t_dev, f_dev = prep.stage(tile, fmask, device)
        return cut(t_dev, f_dev, origins, S, dates=T, mask=bits, strategy=masking_strategy, no_data_value=no_data_value,
                   clip=(0, 10000) if bbox else None)

    source = PointSource(profile, grid, (H, W), tile_id, prep.hls_date(tile_files[0]) if points is None else None, "tile", cut_at, np.uint16)
    return create_from_points(source, points, output_directory, S, window_size, task_type, src_crs, "any", num_classes, date)


# ---- mode=create_chips ---------------------------------------------------------------------------------------------------------------------
CONFIG_KEYS = ("chip_size", "mask_types", "masking_strategy", "window_size", "task_type", "src_crs", "tiles", "fmasks", "records_file",
               "output_directory")


def chips_options(cfg: Dict[str, Any]) -> Dict[str, Any]:
    """The ``chips.*`` keys of ``mode=create_chips`` checked -> the keyword arguments of :func:`create_chips`.  A bad value raises
    ValueError; ``tiles`` and ``output_directory`` are required only in that mode."""
    c = prep.Section(cfg, "chips", CONFIG_KEYS)
    size = c.integer("chip_size", 256, lo=1, what="must be an int >= 1")
    w = c.integer("window_size", 0, lo=0, hi=MAX_WINDOW, what="must be an int >= 0")
    types = c.listing("mask_types", []) or []
    mask_bits(types)
    strategy = c.choice("masking_strategy", "each", STRATEGIES)
    task = c.choice("task_type", "seg", ("seg", "reg"), "must be seg or reg")
    src = c.epsg("src_crs", 4326)
    tiles, fmasks = c.listing("tiles"), c.listing("fmasks")
    records, out = c.text("records_file"), c.text("output_directory")
    if cfg.get("mode") == "create_chips":
        if not tiles or out is None:
            raise ValueError("mode=create_chips needs chips.tiles and chips.output_directory")
        if types and not fmasks:
            raise ValueError("chips.mask_types needs chips.fmasks (one Fmask file per date)")
    return dict(tile_files=tiles, fmask_files=fmasks, points=records, output_directory=out, chip_size=size, mask_types=types,
                masking_strategy=strategy, window_size=w, task_type=task, src_crs=src)


def run_from_config(cfg: Dict[str, Any], device: Optional[str] = None) -> int:
    """``mode=create_chips``: :func:`create_chips` under the ``chips.*`` keys; prints one JSON line with the counts."""
    return prep.run_creator("create_chips", create_chips, chips_options(cfg), device)


def main(argv: Optional[List[str]] = None) -> int:
    """``python -m instageo_amd.chips chips.tiles=a.tif,b.tif chips.output_directory=out ...``: mode=create_chips without ``run.py``."""
    return prep.run_mode_cli("create_chips", run_from_config, argv)


if __name__ == "__main__":
    raise SystemExit(main())
