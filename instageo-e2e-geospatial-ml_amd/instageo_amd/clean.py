"""Dataset cleaning: the no-data chip filter and label buffering / limiting, on the device.

``mode=create_chips`` (:mod:`instageo_amd.chips`) makes ``chip_*.tif`` / ``seg_map_*.tif`` pairs and their CSV; the reference's next step is
``instageo/data/data_cleaner.py`` (``should_drop_chip``, ``buffer_observation_pixels``, ``limit_seg_map_to_observation_pixels``,
``clean_data``) on rasterio, pyproj and absl.  This module is the stand-in on top of :mod:`instageo_amd.tiff`, :mod:`instageo_amd.crs`
and the kernels of ``clean.hip``.

The rule (stated in ``include/instageo_hip.h``).  Chips are (n, B, H, W), 16-bit: a pixel is ``any``-no-data when at least one of its B
values equals ``no_data_value`` and ``all``-no-data when all do (plane bit 0 / bit 1, counts per chip); a chip is dropped when
``count[strategy] / float(H * W) > no_data_threshold``.  ``buffer``: a label pixel is a source when it ``!= ignore_index``; an output
pixel takes the value of the source with the largest row-major index within ``window_size`` in both directions (the later assignment of
numpy's repeated-index store wins), keeps its value without one, and becomes ``ignore_index`` where the chip is all-no-data.  ``limit``:
a pixel keeps its value where an observation point lies on it and becomes ``ignore_index`` elsewhere.  Both return ``valid_labels`` and
the class histogram of the cleaned map.  A quirk kept on purpose: a source is itself overwritten by a later source in its window, and
buffering twice buffers twice.

Device tensors go through ``ig_chip_nodata`` / ``ig_label_buffer`` / ``ig_label_limit``; host arrays take a vectorised numpy path that
gives the same arrays, so the module works (and is tested) without a GPU.

Deliberate difference: errors raise (the reference logs them and writes nothing).  Not done: deriving MGRS tile ids for an observation
table without ``mgrs_tile_id``, window sizes above 32.
"""
from __future__ import annotations

import json
import os
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import crs as crsmod
from . import prep, tiff, warp
from .prep import is_device, to_device, to_host

STRATEGIES = {"any": 0, "all": 1}  # the column of counts, the bit of the plane
METHODS = ("buffer", "limit")
MAX_WINDOW = 32
MAX_CLASSES = 256
BATCH_FILES = 256  # files of one shape and dtype per launch


# ---- argument checks shared by the host path and the device wrappers (ops.chip_nodata / label_buffer / label_limit) --------------------------
def check_nodata(shape, dtype: str, no_data_value) -> Optional[int]:
    """ValueError unless ``shape`` / ``dtype`` describe a batch of 16-bit chips -> ``no_data_value`` when the dtype can hold it, else None
    (it matches nothing)."""
    if len(shape) != 4 or dtype not in ("int16", "uint16"):
        raise ValueError(f"chips is (n, B, H, W) int16 or uint16 (got shape {tuple(shape)}, {dtype})")
    n, B, H, W = (int(v) for v in shape)
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"chips need B, H, W >= 1 (got {tuple(shape)})")
    if H * W > 2**31 - 1:
        raise ValueError(f"a plane of {H} x {W} pixels is beyond 2^31 - 1 (counts is int32)")
    if isinstance(no_data_value, bool) or int(no_data_value) != no_data_value:
        raise ValueError(f"no_data_value must be an integer (got {no_data_value!r})")
    info = np.iinfo(dtype)
    v = int(no_data_value)
    return v if info.min <= v <= info.max else None


def check_label_args(shape, dtype: str, ignore_index, K, w=None) -> None:
    """ValueError unless a label batch, its ``ignore_index``, the histogram size and (for buffer) the window obey include/instageo_hip.h."""
    if len(shape) != 3 or dtype not in ("int16", "float32"):
        raise ValueError(f"labels is (n, H, W) int16 or float32 (got shape {tuple(shape)}, {dtype})")
    if isinstance(ignore_index, bool) or int(ignore_index) != ignore_index:
        raise ValueError(f"ignore_index must be an integer (got {ignore_index!r})")
    lim = (-32768, 32767) if dtype == "int16" else (-(2**24), 2**24)
    if not lim[0] <= int(ignore_index) <= lim[1]:
        raise ValueError(f"ignore_index {ignore_index} is not representable in {dtype} labels")
    if isinstance(K, bool) or not 0 <= int(K) <= MAX_CLASSES or (K and dtype != "int16"):
        raise ValueError(f"a class histogram has 0 <= num_classes <= {MAX_CLASSES} cells and needs int16 labels (got {K!r}, {dtype})")
    if w is not None and (isinstance(w, bool) or int(w) != w or not 0 <= int(w) <= MAX_WINDOW):
        raise ValueError(f"window_size must be an int in [0, {MAX_WINDOW}] (got {w!r})")


def check_points(n: int, H: int, W: int, ptr, pts) -> Tuple[np.ndarray, np.ndarray]:
    """ValueError unless ``ptr`` holds n + 1 ascending offsets from 0 to the number of points -> (ptr, pts (P, 2)) as int32 arrays without
    the points outside their map (the host's fence; the kernel is the second)."""
    ptr = np.asarray(ptr, dtype=np.int64).reshape(-1)
    pts = np.asarray(pts)
    if pts.size and pts.dtype.kind not in "iu":
        raise ValueError("pts must be integers (row, col)")
    pts = pts.astype(np.int64).reshape(-1, 2)
    if ptr.shape[0] != n + 1 or ptr[0] != 0 or (np.diff(ptr) < 0).any() or ptr[-1] != pts.shape[0]:
        raise ValueError(f"ptr must hold {n} + 1 ascending offsets into the points, from 0 to their number ({pts.shape[0]})")
    if pts.shape[0] >= 2**30:
        raise ValueError("too many points for int32 lists")
    inside = (pts[:, 0] >= 0) & (pts[:, 0] < H) & (pts[:, 1] >= 0) & (pts[:, 1] < W)
    owner = np.repeat(np.arange(n), np.diff(ptr))[inside]
    ptr = np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=n))])
    return np.ascontiguousarray(ptr, dtype=np.int32), np.ascontiguousarray(pts[inside], dtype=np.int32)


# ---- the rule on host arrays ---------------------------------------------------------------------------------------------------------------
def _tally(out: np.ndarray, ign, K: int):
    n = out.shape[0]
    live = out != ign
    valid = live.reshape(n, -1).sum(axis=1).astype(np.int32)
    hist = None
    if K:
        hist = np.zeros((n, K), dtype=np.int32)
        for i in range(n):
            v = out[i][live[i]].astype(np.int64)
            hist[i] = np.bincount(v[(v >= 0) & (v < K)], minlength=K)
    return out, valid, hist


def _buffer_host(labels: np.ndarray, w: int, ignore_index: int, plane: Optional[np.ndarray], K: int):
    """numpy twin of ``ig_label_buffer``: the winner is a sliding maximum of the sources' row-major indices, one shifted maximum per offset."""
    n, H, W = labels.shape
    ign = labels.dtype.type(ignore_index)
    idx = np.where(labels != ign, np.arange(H * W, dtype=np.int64).reshape(1, H, W), -1)
    rows = idx.copy()
    for d in range(1, min(w, W - 1) + 1):
        np.maximum(rows[:, :, :-d], idx[:, :, d:], out=rows[:, :, :-d])
        np.maximum(rows[:, :, d:], idx[:, :, :-d], out=rows[:, :, d:])
    win = rows.copy()
    for d in range(1, min(w, H - 1) + 1):
        np.maximum(win[:, :-d], rows[:, d:], out=win[:, :-d])
        np.maximum(win[:, d:], rows[:, :-d], out=win[:, d:])
    flat = labels.reshape(n, H * W)
    out = np.where(win >= 0, np.take_along_axis(flat, np.maximum(win, 0).reshape(n, H * W), axis=1).reshape(n, H, W), labels)
    if plane is not None:
        out[(plane & 2) != 0] = ign
    return _tally(out, ign, K)


def _limit_host(labels: np.ndarray, ptr: np.ndarray, pts: np.ndarray, ignore_index: int, K: int):
    """numpy twin of ``ig_label_limit`` (``ptr`` / ``pts`` from :func:`check_points`: every point lies inside its map)."""
    n = labels.shape[0]
    ign = labels.dtype.type(ignore_index)
    mask = np.zeros(labels.shape, dtype=bool)
    mask[np.repeat(np.arange(n), np.diff(ptr)), pts[:, 0], pts[:, 1]] = True
    return _tally(np.where(mask, labels, ign), ign, K)


# ---- building blocks on arrays and tensors -------------------------------------------------------------------------------------------------
def nodata_planes(chips, no_data_value: int):
    """``chips`` (n, B, H, W) int16 | uint16 -> (plane (n, H, W) uint8: bit 0 = any of the pixel's B values equals ``no_data_value``, bit
    1 = all do; counts (n, 2) int32: the chip's any and all pixels).  A value the dtype cannot hold matches nothing.  Tensors on the device
    go through ``ig_chip_nodata`` and give device tensors; anything else takes numpy and gives arrays."""
    if is_device(chips):
        from . import ops

        return ops.chip_nodata(chips, no_data_value)
    a = to_host(chips)
    pattern = check_nodata(a.shape, a.dtype.name, no_data_value)
    n, _, H, W = a.shape
    if pattern is None:
        return np.zeros((n, H, W), dtype=np.uint8), np.zeros((n, 2), dtype=np.int32)
    eq = a == a.dtype.type(pattern)
    some, every = eq.any(axis=1), eq.all(axis=1)
    counts = np.stack((some.reshape(n, -1).sum(axis=1), every.reshape(n, -1).sum(axis=1)), axis=-1).astype(np.int32)
    return some.astype(np.uint8) | (every.astype(np.uint8) << 1), counts


def dropped(counts, pixels: int, strategy: str, no_data_threshold: float) -> np.ndarray:
    """The chips to drop: ``count[strategy] / float(H * W) > no_data_threshold`` in float64, as ``np.mean(mask) > threshold`` is."""
    if strategy not in STRATEGIES:
        raise ValueError(f"drop_chips_strategy must be one of {tuple(STRATEGIES)} (got {strategy!r})")
    c = to_host(counts).astype(np.int64).reshape(-1, 2)[:, STRATEGIES[strategy]]
    return c / float(pixels) > float(no_data_threshold)


def buffer_labels(labels, window_size: int, ignore_index: int, plane=None, num_classes: int = 0):
    """``labels`` (n, H, W) int16 | float32 buffered by the rule of the module docstring; ``plane``: that of :func:`nodata_planes` (None:
    no masking) -> (out like labels, valid_labels (n,) int32, hist (n, num_classes) int32 or None).  Tensors on the device go through
    ``ig_label_buffer``; anything else takes the numpy twin."""
    if is_device(labels):
        from . import ops

        return ops.label_buffer(labels, window_size, ignore_index, plane, int(num_classes))
    a = to_host(labels)
    check_label_args(a.shape, a.dtype.name, ignore_index, num_classes, window_size)
    p = None if plane is None else to_host(plane)
    if p is not None and (p.dtype != np.uint8 or p.shape != a.shape):
        raise ValueError(f"plane must be uint8 of the labels' shape {a.shape} (got {p.dtype} {p.shape})")
    return _buffer_host(a, int(window_size), int(ignore_index), p, int(num_classes))


def limit_labels(labels, ptr, pts, ignore_index: int, num_classes: int = 0):
    """``labels`` (n, H, W) int16 | float32 limited to the points ``pts`` ((P, 2): row, col) grouped by map through ``ptr`` (CSR, host
    arrays) -> (out, valid_labels, hist) as :func:`buffer_labels`.  Tensors on the device go through ``ig_label_limit``."""
    if is_device(labels):
        from . import ops

        return ops.label_limit(labels, ptr, pts, ignore_index, int(num_classes))
    a = to_host(labels)
    check_label_args(a.shape, a.dtype.name, ignore_index, num_classes)
    p, q = check_points(a.shape[0], a.shape[1], a.shape[2], ptr, pts)
    return _limit_host(a, p, q, int(ignore_index), int(num_classes))


# ---- files -> files -------------------------------------------------------------------------------------------------------------------------
def name_fields(seg_map_fname: str) -> Tuple[str, str]:
    """(date, MGRS tile) of ``seg_map_{date}_{sensor}_{Ttile}_{stamp}_{x}_{y}.tif`` as the reference parses them: fields 2 and 4 (without
    its leading T) of the name split at ``_``."""
    parts = os.path.basename(str(seg_map_fname)).split("_")
    if len(parts) < 5:
        raise ValueError(f"{seg_map_fname}: not a label-map name (seg_map_<date>_<sensor>_T<tile>_<stamp>_<x>_<y>.tif)")
    return parts[2], parts[4][1:]


def locate_observations(obs: Dict[str, np.ndarray], seg_map_fname: str, profile: Dict[str, Any]) -> Optional[np.ndarray]:
    """The (row, col) pixels of the observations of this map's tile and date (``obs``: x, y in EPSG:4326, mgrs_tile_id, date with the
    dashes removed) on the grid of ``profile``: row = floor((Y0 - y) / sy), col = floor((x - X0) / sx); points outside the map are kept
    here and dropped by :func:`check_points`.  None when no observation is relevant."""
    date, tile = name_fields(seg_map_fname)
    sel = (obs["mgrs_tile_id"] == tile) & (obs["date"] == date)
    if not sel.any():
        return None
    X0, Y0, sx, sy = warp.grid_of(profile, str(seg_map_fname))
    tx, ty = crsmod.transform(crsmod.from_epsg(4326), crsmod.from_profile(profile), obs["x"][sel], obs["y"][sel])
    rc = np.stack((np.floor((Y0 - ty) / sy), np.floor((tx - X0) / sx)), axis=-1)
    return np.clip(rc, -(2.0**31), 2.0**31 - 1).astype(np.int64)


def _read_observations(path) -> Dict[str, np.ndarray]:
    import pandas as pd

    df = pd.read_csv(path) if isinstance(path, (str, os.PathLike)) else pd.DataFrame(path)
    for col in ("x", "y", "date"):
        if col not in df.columns:
            raise ValueError("Observation points CSV must contain 'x', 'y', and 'date' columns")
    if "mgrs_tile_id" not in df.columns:
        raise ValueError("the observation points need a mgrs_tile_id column: deriving MGRS tile ids from coordinates is not supported")
    return {"x": df["x"].to_numpy(dtype=np.float64), "y": df["y"].to_numpy(dtype=np.float64),
            "mgrs_tile_id": df["mgrs_tile_id"].astype(str).to_numpy(dtype=object),
            "date": df["date"].astype(str).str.replace("-", "").to_numpy(dtype=object)}


def _batches(paths: Sequence[str]):
    """Read ``paths`` and yield (indices, stacked arrays, profiles) per group of equal shape and dtype, at most BATCH_FILES at a time."""
    groups: Dict[Tuple, List[int]] = {}
    for i, p in enumerate(paths):
        prof = tiff.read_profile(p)
        groups.setdefault((prof["count"], prof["height"], prof["width"], prof["dtype"]), []).append(i)
    for key, members in groups.items():
        for k in range(0, len(members), BATCH_FILES):
            idx = members[k : k + BATCH_FILES]
            arrays, profs = [], []
            for i in idx:
                a, prof = tiff.read(paths[i])
                arrays.append(a)
                profs.append(prof)
            yield idx, np.stack(arrays), profs


def _planes_of(paths: Sequence[str], no_data_value: int, device):
    """-> (planes: one (H, W) uint8 host array per chip file, counts (n, 2) int64, pixels (n,))."""
    n = len(paths)
    planes: List[Optional[np.ndarray]] = [None] * n
    counts, pixels = np.zeros((n, 2), dtype=np.int64), np.ones(n, dtype=np.int64)
    for idx, stack, _ in _batches(paths):
        if stack.dtype.name not in ("int16", "uint16"):
            raise ValueError(f"{paths[idx[0]]}: chips must be int16 or uint16 (got {stack.dtype.name})")
        plane, cnt = nodata_planes(to_device(stack, device), no_data_value)
        plane, cnt = to_host(plane), to_host(cnt)
        for k, i in enumerate(idx):
            planes[i], counts[i], pixels[i] = plane[k], cnt[k], plane[k].size
    return planes, counts, pixels


def clean_data(chips_dataset_csv: str, output_chips_dataset_csv: str, drop_chips: bool = False, drop_chips_strategy: str = "any",
               no_data_threshold: float = 0.5, no_data_value: int = -9999, clean_seg_maps: bool = False,
               observation_points_csv: Optional[str] = None, cleaning_method: str = "buffer", ignore_index: int = -1, window_size: int = 1,
               seg_map_output_dir: Optional[str] = None, device: Optional[str] = None, root_dir: Optional[str] = None,
               num_classes: Optional[int] = None) -> Dict[str, Any]:
    """The reference's ``clean_data``, in its order: read ``chips_dataset_csv`` (``Input`` / ``Label``), drop the chips whose share of
    ``drop_chips_strategy`` no-data pixels is above ``no_data_threshold``, then clean the label maps of the rows that remain (``buffer``:
    by ``window_size``, re-masked where the chip is all-no-data; ``limit``: to the pixels of ``observation_points_csv``: x, y in EPSG:4326,
    mgrs_tile_id, date; a map without a relevant point is dropped) and write ``output_chips_dataset_csv`` with, next to it,
    ``clean_stats.json`` (rows in / out, rows dropped by reason, the summed class histogram of the cleaned maps with ``num_classes`` cells
    (None: the largest label of the maps read + 1) and its ``compute_class_weights``).  -> the stats.

    Relative paths of the CSV are taken from ``root_dir`` (None: the CSV's folder, where ``create_chips`` writes them); the output CSV
    keeps the input's paths, with the label column re-pointed when ``seg_map_output_dir`` is given (relative to the same root where it
    lies under it).  ``seg_map_output_dir=None`` replaces the label maps in place.  int8 / uint8 label files are widened to int16 for
    the kernels and written back in their own dtype; every output file keeps the tags of its input.  ``device``: None = the numpy path,
    ``"cuda"`` / ``"cuda:n"`` = the kernels; both write the same bytes.  Errors raise."""
    import pandas as pd

    if drop_chips_strategy not in STRATEGIES:
        raise ValueError(f"drop_chips_strategy must be one of {tuple(STRATEGIES)} (got {drop_chips_strategy!r})")
    if cleaning_method not in METHODS:
        raise ValueError(f"Invalid cleaning method: {cleaning_method}")
    if not 0.0 <= float(no_data_threshold) <= 1.0:
        raise ValueError(f"no_data_threshold must lie in [0, 1] (got {no_data_threshold!r})")
    if isinstance(window_size, bool) or int(window_size) != window_size or not 1 <= int(window_size) <= MAX_WINDOW:
        raise ValueError(f"window_size must be an int in [1, {MAX_WINDOW}] (got {window_size!r})")
    prep.check_device(device)
    if clean_seg_maps and cleaning_method == "limit" and not observation_points_csv:
        raise ValueError("Observation points CSV is required for `limit` cleaning method")
    df = pd.read_csv(chips_dataset_csv)
    if not all(col in df.columns for col in ("Input", "Label")):
        raise ValueError("CSV must contain 'Input' and 'Label' columns")
    root = root_dir if prep.none(root_dir) is not None else os.path.dirname(os.path.abspath(chips_dataset_csv))
    full = lambda p: p if os.path.isabs(str(p)) else os.path.join(root, str(p))  # noqa: E731
    inputs, labels = [str(v) for v in df["Input"]], [str(v) for v in df["Label"]]
    keep = np.ones(len(df), dtype=bool)
    stats: Dict[str, Any] = {"rows_in": int(len(df)), "rows_out": 0, "dropped": {"no_data": 0, "no_points": 0}}
    planes: Optional[List[np.ndarray]] = None
    need_planes = clean_seg_maps and cleaning_method == "buffer"
    if drop_chips or need_planes:
        planes, counts, pixels = _planes_of([full(p) for p in inputs], no_data_value, device)
        if drop_chips:
            col = STRATEGIES[drop_chips_strategy]
            keep &= ~(counts[:, col] / pixels.astype(np.float64) > float(no_data_threshold))
            stats["dropped"]["no_data"] = int((~keep).sum())
    hist_sum: Optional[np.ndarray] = None
    if clean_seg_maps:
        rows = np.nonzero(keep)[0]
        obs = _read_observations(observation_points_csv) if cleaning_method == "limit" else None
        if seg_map_output_dir is not None:
            os.makedirs(seg_map_output_dir, exist_ok=True)
        if num_classes is not None and (isinstance(num_classes, bool) or not 1 <= int(num_classes) <= MAX_CLASSES):
            raise ValueError(f"num_classes must lie in [1, {MAX_CLASSES}] (got {num_classes!r})")
        cleaned: List[Tuple[int, np.ndarray, Dict[str, Any]]] = []  # row, map in its file's dtype, profile
        hist_all, top = np.zeros(MAX_CLASSES, dtype=np.int64), -1  # the histograms of the launches, summed; the largest label seen
        for idx, stack, profs in _batches([full(labels[i]) for i in rows]):
            if stack.shape[1] != 1:
                raise ValueError(f"{labels[rows[idx[0]]]}: a label map has one band (got {stack.shape[1]})")
            file_dt = stack.dtype
            if file_dt.name in ("int8", "uint8"):
                work = stack[:, 0].astype(np.int16)
            elif file_dt.name in ("int16", "float32"):
                work = np.ascontiguousarray(stack[:, 0])
            else:
                raise ValueError(f"{labels[rows[idx[0]]]}: label maps must be int8, uint8, int16 or float32 (got {file_dt.name})")
            if file_dt.kind in "iu" and not np.iinfo(file_dt).min <= int(ignore_index) <= np.iinfo(file_dt).max:
                raise ValueError(f"ignore_index {ignore_index} is not representable in the {file_dt.name} label map {labels[rows[idx[0]]]}")
            members = [int(rows[i]) for i in idx]
            K = 0  # histogram cells of this launch: int16 maps only
            if work.dtype == np.int16:
                top = max(top, int(work.max()))
                K = int(num_classes) if num_classes is not None else int(min(max(int(work.max()) + 1, 1), MAX_CLASSES))
            if cleaning_method == "buffer":
                pl = np.stack([planes[r] for r in members])
                if pl.shape != work.shape:
                    raise ValueError(f"{labels[members[0]]}: a label map of {work.shape[1:]} pixels does not go with a chip of {pl.shape[1:]}")
                out, _, hist = buffer_labels(to_device(work, device), int(window_size), int(ignore_index), to_device(pl, device), K)
            else:
                lists = [locate_observations(obs, labels[r], prof) for r, prof in zip(members, profs)]
                have = [k for k, q in enumerate(lists) if q is not None]
                for k, q in enumerate(lists):
                    if q is None:
                        keep[members[k]] = False
                        stats["dropped"]["no_points"] += 1
                if not have:
                    continue
                members, profs, work = [members[k] for k in have], [profs[k] for k in have], np.ascontiguousarray(work[have])
                ptr = np.concatenate([[0], np.cumsum([lists[k].shape[0] for k in have])])
                out, _, hist = limit_labels(to_device(work, device), ptr, np.concatenate([lists[k] for k in have]), int(ignore_index), K)
            out = to_host(out)
            if hist is not None:
                hist_all[:K] += to_host(hist).astype(np.int64).sum(axis=0)
            for k, r in enumerate(members):
                cleaned.append((r, out[k].astype(file_dt, copy=False), profs[k]))
        new_labels = list(labels)
        for r, arr, prof in cleaned:
            target = full(labels[r]) if seg_map_output_dir is None else os.path.join(seg_map_output_dir, os.path.basename(labels[r]))
            tiff.write(target, arr, prof)
            if seg_map_output_dir is not None:
                rel = os.path.relpath(os.path.abspath(target), os.path.abspath(root))
                new_labels[r] = target if os.path.isabs(labels[r]) or rel.startswith("..") else rel.replace(os.sep, "/")
        df["Label"] = new_labels
        if top >= 0 or (num_classes is not None and hist_all.any()):
            hist_sum = hist_all[: int(num_classes) if num_classes is not None else min(max(top + 1, 1), MAX_CLASSES)]
    df = df[keep]
    stats["rows_out"] = int(len(df))
    if hist_sum is not None:
        stats.update(prep.class_stats(hist_sum))
    out_dir = os.path.dirname(os.path.abspath(output_chips_dataset_csv))
    os.makedirs(out_dir, exist_ok=True)
    df.to_csv(output_chips_dataset_csv, index=False)
    prep.write_stats(os.path.join(out_dir, "clean_stats.json"), stats)
    return stats


# ---- mode=clean_chips ----------------------------------------------------------------------------------------------------------------------
CONFIG_KEYS = ("chips_dataset_csv", "output_chips_dataset_csv", "drop_chips", "drop_chips_strategy", "no_data_threshold", "no_data_value",
               "clean_seg_maps", "cleaning_method", "observation_points_csv", "seg_map_output_dir", "ignore_index", "window_size",
               "num_classes", "root_dir")


def clean_options(cfg: Dict[str, Any]) -> Dict[str, Any]:
    """The ``clean.*`` keys of ``mode=clean_chips`` checked -> the keyword arguments of :func:`clean_data`.  A bad value raises ValueError;
    the two CSV paths are required only in that mode."""
    c = prep.Section(cfg, "clean", CONFIG_KEYS)
    strategy = c.choice("drop_chips_strategy", "any", STRATEGIES)
    method = c.choice("cleaning_method", "buffer", METHODS)
    thr = c.number("no_data_threshold", 0.5, lambda x: 0.0 <= x <= 1.0, "must lie in [0, 1]")
    w = c.integer("window_size", 1, lo=1, hi=MAX_WINDOW, span=f"must lie in [1, {MAX_WINDOW}]")
    K = c.integer("num_classes", None, lo=1, hi=MAX_CLASSES, what=f"must be None or an int in [1, {MAX_CLASSES}]", optional=True)
    opts = dict(chips_dataset_csv=c.text("chips_dataset_csv"), output_chips_dataset_csv=c.text("output_chips_dataset_csv"),
                drop_chips=c.flag("drop_chips"), drop_chips_strategy=strategy, no_data_threshold=thr,
                no_data_value=c.integer("no_data_value", -9999), clean_seg_maps=c.flag("clean_seg_maps"), cleaning_method=method,
                observation_points_csv=c.text("observation_points_csv"), seg_map_output_dir=c.text("seg_map_output_dir"),
                ignore_index=c.integer("ignore_index", -1), window_size=w, num_classes=K, root_dir=c.text("root_dir"))
    if cfg.get("mode") == "clean_chips":
        if opts["chips_dataset_csv"] is None or opts["output_chips_dataset_csv"] is None:
            raise ValueError("mode=clean_chips needs clean.chips_dataset_csv and clean.output_chips_dataset_csv")
        if opts["clean_seg_maps"] and method == "limit" and opts["observation_points_csv"] is None:
            raise ValueError("clean.cleaning_method=limit needs clean.observation_points_csv")
    return opts


def run_from_config(cfg: Dict[str, Any], device: Optional[str] = None) -> int:
    """``mode=clean_chips``: :func:`clean_data` under the ``clean.*`` keys; prints one JSON line with the counts."""
    kw = clean_options(cfg)
    stats = clean_data(device=device, **kw)
    print(json.dumps({"clean_chips": {"rows_in": stats["rows_in"], "rows_out": stats["rows_out"], "dropped": stats["dropped"],
                                      "output_chips_dataset_csv": kw["output_chips_dataset_csv"]}}))
    return 0


def main(argv: Optional[List[str]] = None) -> int:
    """``python -m instageo_amd.clean clean.chips_dataset_csv=in.csv clean.output_chips_dataset_csv=out.csv ...``: mode=clean_chips
    without ``run.py``."""
    return prep.run_mode_cli("clean_chips", run_from_config, argv)


if __name__ == "__main__":
    raise SystemExit(main())
