"""Mosaic of per-chip predictions into one raster, pasted on the device.

``mode=chip_inference`` ends with one ``prediction_*.tif`` per chip.  The reference's serving layer reads that folder back, runs
``gdal_merge.py`` over it and serves the resulting ``predictions_merged.tif`` as a COG with its segmentation statistics
(``new_apps/backend/app/cog_converter.py``, ``merge_task_files_to_cog``).  GDAL is absent here; this module is the stand-in, a post-step
over the written files on top of :mod:`instageo_amd.tiff`, the kernel of ``mosaic.hip`` and the output writer of
:mod:`instageo_amd.infer_utils`.

The rule (stated in ``include/instageo_hip.h``).  Chip i is a rectangle (row0, col0, h, w) on an H x W canvas and may hang over its
edge.  It contributes to a canvas pixel when it covers the pixel and its value there is not transparent (int8: ``== fill``; float32:
NaN).  Contributors are ordered by chip index.  ``last``: the contributor with the largest index (``gdal_merge -n fill``: later files
win); ``first``: the smallest index; ``mode`` (int8): the value most contributors have, ties to the smallest value; ``mean`` (float32):
the float32 sum in index order divided by the count, bit for bit numpy float32 arithmetic; no contributor: ``fill`` / NaN.  ``cover``
counts the contributors, saturating at 255.

Device tensors go through ``ig_mosaic_paste``; host arrays take a numpy twin of the same rule, so the merge works (and is tested)
without a GPU.

Not done: reprojection or resampling between grids in this module (chips must share one pixel grid; chips of different coordinate
systems become separate mosaics, two pixel scales in one are refused; :func:`instageo_amd.warp.merge_reprojected` warps those mosaics
onto one canvas), rotated rasters, multi-band inputs (the reference's RGB ``chips_merged.tif`` is
:func:`instageo_amd.maptiles.merge_chips`), BigTIFF, a mosaic of
tensors still on the device inside ``chip_inference``, and chip lists built on the device.
"""
from __future__ import annotations

import glob
import json
import os
import time
from concurrent.futures import ThreadPoolExecutor
from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np

from . import cog as cogmod
from . import postprocess, tiff, vectorize, zonal
from .prep import is_device

RULES = ("last", "first", "mode", "mean")
BLOCK = 64  # side of the canvas block one workgroup owns (mosaic.hip), and of a bin
LIMIT = 1 << 30  # of |row0|, |col0|, h, w (include/instageo_hip.h)
GRID_TOLERANCE = 1e-3  # pixels a chip origin may lie off the canvas grid
READ_THREADS = 8
_NAN = np.uint32(0x7FC00000).view(np.float32)
_CRS_TAGS = (34735, 34736, 34737)
TIMINGS: Dict[str, float] = {}  # wall seconds of the phases of the latest merge_predictions: read, paste, products, write


class Group(NamedTuple):
    """One mosaic: the chips of one pixel grid."""
    rects: np.ndarray  # (n, 4) int32 (row0, col0, h, w) on the canvas
    shape: Tuple[int, int]  # (H, W) of the canvas
    profile: Dict[str, Any]  # of the mosaic
    members: np.ndarray  # (n,) the indices of the group's chips in the input, ascending


def check_rule(rule: str, dtype) -> None:
    """ValueError unless ``rule`` goes with rasters of ``dtype`` (int8: last | first | mode, float32: last | first | mean)."""
    name = np.dtype(str(dtype).replace("torch.", "")).name
    if rule not in RULES:
        raise ValueError(f"mosaic rule must be one of {RULES} (got {rule!r})")
    if name not in ("int8", "float32"):
        raise ValueError(f"a mosaic takes int8 class maps or float32 rasters (got {name})")
    if (rule == "mode" and name != "int8") or (rule == "mean" and name != "float32"):
        raise ValueError(f"mosaic rule {rule!r} does not go with {name} rasters (int8: last | first | mode, float32: last | first | mean)")


def check_fill(fill: int) -> int:
    if isinstance(fill, bool) or not isinstance(fill, (int, np.integer)) or not -128 <= int(fill) <= 127:
        raise ValueError(f"fill must be an int that fits int8 (got {fill!r})")
    return int(fill)


def check_canvas(H: int, W: int) -> None:
    """ValueError for a canvas beyond the limits of ``ig_mosaic_paste``."""
    if H < 0 or W < 0 or H * W > 2**31 - 1 or -(-H // BLOCK) > 65535:
        raise ValueError(f"a mosaic canvas of {H} x {W} pixels is beyond the kernel's limits (H * W <= 2^31 - 1, H <= 65535 * {BLOCK})")


# ---- where the chips go ----------------------------------------------------------------------------------------------------------------
def placement(profiles: Sequence[Optional[Dict[str, Any]]], shapes: Sequence[Tuple[int, int]], names: Optional[Sequence[str]] = None,
              dtype="int8", fill: int = -1) -> List[Group]:
    """Chips -> their rectangles on one canvas per pixel grid.  ``profiles``: the chips' GeoTIFF profiles (:func:`tiff.read`), north-up
    with a pixel scale (sx, sy) and a tiepoint (:func:`postprocess.georeference`); ``shapes``: their (h, w); ``names``: what to call them
    in error messages.  The origin of a chip is x0 = tie_x - tie_i * sx, y0 = tie_y + tie_j * sy; the canvas origin is (X0, Y0) = (min x0,
    max y0), and col0 = (x0 - X0) / sx, row0 = (Y0 - y0) / sy must lie within 1e-3 of an integer (chips cut from one grid are exact).
    Chips are grouped by the values of the GeoKey tags 34735 / 34736 / 34737, in order of first appearance: chips of two UTM zones do
    not share a grid.  The profile of a mosaic is its first chip's with the tiepoint (0, 0, 0, X0, Y0, 0), the canvas size, one band and
    NODATA = ``fill`` (int8) or NaN (float32), written the way tile inference writes them.

    ValueError, naming the chip: no georeferencing; a ModelTransformation tag (rotated rasters); a pixel scale that differs from that
    of the group's first chip (resampling is not done, and two mosaics of one place would be a surprise); an origin off the grid; a
    profile whose size differs from the array's; a canvas beyond the kernel's limits."""
    n = len(profiles)
    if len(shapes) != n:
        raise ValueError(f"{n} profiles but {len(shapes)} shapes")
    names = [str(x) for x in names] if names is not None else [f"chip {i}" for i in range(n)]
    keys: List[Any] = []
    geo: List[Tuple[float, ...]] = []
    for prof, (h, w), name in zip(profiles, shapes, names):
        tags = (prof or {}).get("tags") or {}
        if 34264 in tags:
            raise ValueError(f"{name}: a ModelTransformation tag (rotated or sheared raster) cannot be placed on a north-up canvas")
        g = postprocess.georeference(prof)
        if g is None or g[0] <= 0 or g[1] <= 0:
            raise ValueError(f"{name}: no georeferencing (needs a ModelPixelScale and a ModelTiepoint tag with positive scales)")
        if (prof.get("height", h), prof.get("width", w)) != (h, w):
            raise ValueError(f"{name}: the profile says {prof.get('height')} x {prof.get('width')} pixels, the array has {h} x {w}")
        if h < 1 or w < 1:
            raise ValueError(f"{name}: an empty raster")
        geo.append(g)
        keys.append(tuple(repr(tags.get(t)) for t in _CRS_TAGS))
    order: Dict[Any, List[int]] = {}
    for i, k in enumerate(keys):
        order.setdefault(k, []).append(i)
    groups = []
    for members in order.values():
        sx, sy = geo[members[0]][:2]
        for i in members:
            if geo[i][:2] != (sx, sy):
                raise ValueError(f"{names[i]}: pixel scale {geo[i][:2]}, but {names[members[0]]} of the same coordinate system has {(sx, sy)} "
                                 "(resampling between grids is not done)")
        x0 = np.array([geo[i][4] - geo[i][2] * sx for i in members], dtype=np.float64)
        y0 = np.array([geo[i][5] + geo[i][3] * sy for i in members], dtype=np.float64)
        X0, Y0 = float(x0.min()), float(y0.max())
        col, row = (x0 - X0) / sx, (Y0 - y0) / sy
        rects = np.zeros((len(members), 4), dtype=np.int64)
        for k, i in enumerate(members):
            rc = (round(row[k]), round(col[k]))
            if abs(row[k] - rc[0]) > GRID_TOLERANCE or abs(col[k] - rc[1]) > GRID_TOLERANCE:
                raise ValueError(f"{names[i]}: its origin lies at row {row[k]!r}, column {col[k]!r} of the mosaic grid, more than "
                                 f"{GRID_TOLERANCE} of a pixel off (resampling between grids is not done)")
            rects[k] = (*rc, *shapes[i])
        H, W = int((rects[:, 0] + rects[:, 2]).max()), int((rects[:, 1] + rects[:, 3]).max())
        if max(H, W) > LIMIT:
            raise ValueError(f"a mosaic canvas of {H} x {W} pixels is beyond the kernel's limits")
        check_canvas(H, W)
        first = dict(profiles[members[0]])
        tags = {k: v for k, v in first["tags"].items() if k != 42113}
        tags[33922] = (12, (0.0, 0.0, 0.0, X0, Y0, 0.0))
        if np.dtype(dtype) == np.float32:
            prof = dict(first, width=W, height=H, count=1, dtype="float32", nodata=None, tags={**tags, 42113: (2, "nan")})
        else:
            prof = dict(first, width=W, height=H, count=1, dtype=np.dtype(dtype).name, nodata=fill, tags=tags)
        groups.append(Group(rects.astype(np.int32), (H, W), prof, np.array(members, dtype=np.int64)))
    return groups


def bins(rects, H: int, W: int) -> Tuple[np.ndarray, np.ndarray]:
    """-> (bin_ptr (blocks + 1,) int32, bin_idx int32): for every 64 x 64 block of the H x W canvas (row-major, ceil(W / 64) to a row) the
    indices of the chips whose rectangle intersects it, ascending: the (block, chip) pairs sorted by block, then chip."""
    r = np.asarray(rects, dtype=np.int64).reshape(-1, 4)
    nbx, nby = -(-W // BLOCK), -(-H // BLOCK)
    r0, c0 = np.clip(r[:, 0], 0, H), np.clip(r[:, 1], 0, W)
    r1, c1 = np.clip(r[:, 0] + r[:, 2], 0, H), np.clip(r[:, 1] + r[:, 3], 0, W)
    ok = (r1 > r0) & (c1 > c0)
    by0, bx0 = r0 // BLOCK, c0 // BLOCK
    ny = np.where(ok, (r1 - 1) // BLOCK - by0 + 1, 0)
    nx = np.where(ok, (c1 - 1) // BLOCK - bx0 + 1, 0)
    cnt = ny * nx
    chip = np.repeat(np.arange(len(r), dtype=np.int64), cnt)
    k = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)  # the pair's number within its chip
    nxr = np.repeat(nx, cnt)
    blk = (np.repeat(by0, cnt) + k // np.maximum(nxr, 1)) * nbx + np.repeat(bx0, cnt) + k % np.maximum(nxr, 1)
    order = np.lexsort((chip, blk))
    ptr = np.concatenate([[0], np.cumsum(np.bincount(blk, minlength=nbx * nby))])
    if ptr[-1] > 2**31 - 1:
        raise ValueError("too many (block, chip) pairs for int32 chip lists")
    return ptr.astype(np.int32), chip[order].astype(np.int32)


# ---- the rule on host arrays -----------------------------------------------------------------------------------------------------------
def _paste_host(chips: Sequence[np.ndarray], rects: np.ndarray, H: int, W: int, rule: str, fill: int, dtype: np.dtype):
    """numpy twin of ``ig_mosaic_paste``: chip by chip, vectorised over the pixels -> (canvas, the unsaturated contributor counts)."""
    is_f = dtype == np.float32
    parts = []  # (canvas window, the chip's part inside the canvas, where it contributes)
    for a, (r0, c0, h, w) in zip(chips, rects.tolist()):
        ra, rb, ca, cb = max(r0, 0), min(r0 + h, H), max(c0, 0), min(c0 + w, W)
        if rb > ra and cb > ca:
            v = a[ra - r0 : rb - r0, ca - c0 : cb - c0]
            parts.append(((slice(ra, rb), slice(ca, cb)), v, ~np.isnan(v) if is_f else v != fill))
    count = np.zeros((H, W), dtype=np.int64)
    for win, _, ok in parts:
        count[win] += ok
    canvas = np.full((H, W), _NAN if is_f else fill, dtype=dtype)
    if rule in ("last", "first"):
        for win, v, ok in parts if rule == "last" else reversed(parts):  # the winner is pasted last
            canvas[win][ok] = v[ok]
    elif rule == "mean":
        s = np.zeros((H, W), dtype=np.float32)
        seen = np.zeros((H, W), dtype=bool)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            for win, v, ok in parts:
                s[win] = np.where(ok, np.where(seen[win], s[win] + v, v), s[win])
                seen[win] |= ok
            canvas = (s / count.astype(np.float32)).astype(np.float32)
        canvas[count == 0] = _NAN
    else:  # mode: the candidates in ascending order, a later one must have strictly more contributors
        values = sorted({int(x) for _, v, ok in parts for x in np.unique(v[ok])})
        bestn = np.zeros((H, W), dtype=np.int64)
        for x in values:
            n = np.zeros((H, W), dtype=np.int64)
            for win, v, ok in parts:
                n[win] += ok & (v == x)
            better = n > bestn
            canvas[better] = x
            bestn[better] = n[better]
    return canvas, count


def paste(chips, rects, shape: Tuple[int, int], rule: str = "last", fill: int = -1, cover: bool = False):
    """The mosaic of ``chips`` (a list of 2-D arrays / tensors of one dtype, int8 or float32, or one (N, h, w) array) at ``rects``
    ((N, 4): row0, col0, h, w) on a canvas of ``shape`` by ``rule`` (the module docstring) -> the canvas, or (canvas, cover uint8) with
    ``cover``.  Tensors on the device are packed and go through ``ig_mosaic_paste`` and give device tensors; anything else takes the
    numpy twin and gives arrays."""
    chips = list(chips)
    rects = np.asarray(rects, dtype=np.int64).reshape(-1, 4)
    H, W = int(shape[0]), int(shape[1])
    fill = check_fill(fill)
    if len(chips) != len(rects):
        raise ValueError(f"{len(chips)} chips but {len(rects)} rectangles")
    if not chips:
        raise ValueError("a mosaic needs at least one chip")
    dev = is_device(chips[0])
    if not dev:
        chips = [np.asarray(c.cpu() if hasattr(c, "cpu") else c) for c in chips]
    if any(c.dtype != chips[0].dtype for c in chips):
        raise ValueError("the chips of a mosaic have one dtype")
    check_rule(rule, chips[0].dtype)
    check_canvas(H, W)
    for i, (c, r) in enumerate(zip(chips, rects.tolist())):
        if c.ndim != 2 or tuple(c.shape) != (r[2], r[3]) or r[2] < 1 or r[3] < 1:
            raise ValueError(f"chip {i} is {tuple(c.shape)}, its rectangle says {r[2]} x {r[3]} (both at least 1)")
    if np.abs(rects).max() > LIMIT:
        raise ValueError("a chip rectangle needs |row0|, |col0|, h, w <= 2^30")
    if not dev:
        canvas, count = _paste_host(chips, rects, H, W, rule, fill, chips[0].dtype)
        return (canvas, np.minimum(count, 255).astype(np.uint8)) if cover else canvas
    import torch

    from . import ops

    packed = torch.cat([c.reshape(-1) for c in chips])
    sizes = rects[:, 2] * rects[:, 3]
    return ops.mosaic_paste(packed, np.cumsum(sizes) - sizes, rects, *bins(rects, H, W), (H, W), rule, fill, cover)


# ---- files -> files ----------------------------------------------------------------------------------------------------------------------
def _read_one(path: str) -> Tuple[np.ndarray, Dict[str, Any]]:
    arr, prof = tiff.read(path)
    if arr.shape[0] != 1:
        raise ValueError(f"{path}: {arr.shape[0]} bands (a mosaic takes single-band prediction rasters)")
    return arr[0], prof


def _write_cog_host(canvas: np.ndarray, kind: str, path: str, stats_path: Optional[str], profile, opts, fill: int, ncls: Optional[int]):
    """:func:`infer_utils.save_cog` for a canvas on the host: the numpy pyramid, the same file."""
    if ncls is not None and ncls > cogmod.MAX_CLASSES:
        ncls = None
    counts = np.zeros(ncls + 1, dtype=np.int64) if ncls is not None else None
    levels = cogmod.build_overviews(canvas, kind, opts.overview_levels, fill, opts.cog_blocksize, ncls=ncls, counts=counts)
    cogmod.write_cog(path, levels, profile, opts.cog_blocksize, opts.cog_compress)
    if counts is not None:
        with open(stats_path, "w") as f:
            json.dump(cogmod.seg_stats(counts), f, sort_keys=True)
    return path


class _Job(NamedTuple):
    """What :func:`merge_predictions` knows once its options are checked and its files are read."""
    opts: Any  # infer_utils.OutputOptions
    fill: int
    num_classes: Optional[int]
    host: bool
    dev: Optional[str]  # the torch device when not host
    products: bool
    paths: List[str]
    arrays: List[np.ndarray]
    profiles: List[Dict[str, Any]]
    regression: bool
    groups: List[Group]
    zone_list: Any
    t: Dict[str, float]  # wall seconds of the phases so far


def prepare(paths_or_folder, output_folder, rule, fill, num_classes, device, cog, cog_blocksize, overview_levels, cog_compress, min_region,
            connectivity, sieve_passes, save_regions, save_polygons, zones, zone_id_property) -> _Job:
    """The first half of :func:`merge_predictions`: every option checked, the files read and placed, the output folder made."""
    from .infer_utils import OutputOptions

    opts = OutputOptions(min_region=min_region, connectivity=connectivity, sieve_passes=sieve_passes, save_regions=save_regions,
                         save_polygons=save_polygons, zones=zones, zone_id_property=zone_id_property, cog=bool(cog),
                         cog_blocksize=cog_blocksize, overview_levels=overview_levels, cog_compress=cog_compress)
    opts.check(None)
    if rule not in RULES:
        raise ValueError(f"mosaic rule must be one of {RULES} (got {rule!r})")
    fill = check_fill(fill)
    if num_classes is not None and (isinstance(num_classes, bool) or int(num_classes) < 1):
        raise ValueError(f"num_classes must be a positive int or None (got {num_classes!r})")
    if device not in ("gpu", "cpu") and not str(device).startswith("cuda"):
        raise ValueError(f"device must be 'gpu', 'cpu' or a cuda device (got {device!r})")
    products = min_region > 0 or save_regions or save_polygons or zones is not None
    host = device == "cpu"
    if host and products:
        raise ValueError("device='cpu' pastes and writes the raster only: the sieve, regions, polygons and zones run on the device")
    if isinstance(paths_or_folder, (str, os.PathLike)):
        paths = sorted(glob.glob(os.path.join(glob.escape(str(paths_or_folder)), "prediction_*.tif")))
        if not paths:
            raise ValueError(f"no prediction_*.tif files in {paths_or_folder}")
    else:
        paths = [str(p) for p in paths_or_folder]
        if not paths:
            raise ValueError("a mosaic needs at least one file")
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=min(READ_THREADS, len(paths))) as pool:
        read = list(pool.map(_read_one, paths))
    arrays, profiles = [a for a, _ in read], [p for _, p in read]
    dtype = arrays[0].dtype
    for a, p in zip(arrays, paths):
        if a.dtype != dtype:
            raise ValueError(f"{p}: {a.dtype.name} samples, {paths[0]} has {dtype.name} (one mosaic, one sample type)")
    check_rule(rule, dtype)
    regression = dtype == np.float32
    postprocess.check_region_options(min_region, connectivity, sieve_passes, save_regions, regression)
    vectorize.check_polygon_options(save_polygons, regression)
    zonal.check_zone_options(zones, regression)
    groups = placement(profiles, [a.shape for a in arrays], paths, dtype, fill)
    zone_list = zonal.read_zones(zones, zone_id_property) if zones is not None else None
    os.makedirs(output_folder, exist_ok=True)
    t = {"read": time.perf_counter() - t0, "paste": 0.0, "products": 0.0, "write": 0.0}
    return _Job(opts, fill, None if num_classes is None else int(num_classes), host, None if host else "cuda" if device == "gpu" else device,
                products, paths, arrays, profiles, regression, groups, zone_list, t)


def paste_group(job: _Job, g: Group, rule: str, save_cover: bool):
    """The canvas of group ``g`` (and its cover, or None): on the host, or packed, uploaded and pasted by ``ig_mosaic_paste``."""
    mine = [job.arrays[i] for i in g.members]
    t0 = time.perf_counter()
    if job.host:
        res = paste(mine, g.rects, g.shape, rule, job.fill, save_cover)
    else:
        import torch

        from . import ops

        sizes = g.rects[:, 2].astype(np.int64) * g.rects[:, 3]
        packed = torch.from_numpy(np.concatenate([a.reshape(-1) for a in mine])).to(job.dev)
        res = ops.mosaic_paste(packed, np.cumsum(sizes) - sizes, g.rects, *bins(g.rects, *g.shape), g.shape, rule, job.fill, save_cover)
        torch.cuda.synchronize()
    job.t["paste"] += time.perf_counter() - t0
    return res if save_cover else (res, None)


def write_canvas(job: _Job, canvas, cover, name: str, profile: Dict[str, Any], output_folder: str) -> List[str]:
    """One finished canvas (and its cover, or None) -> the class products, the raster, its statistics and the cover file under ``name``
    -> the written paths."""
    from .infer_utils import _output_path, _write_products, _write_raster, save_prediction

    opts, fill, host = job.opts, job.fill, job.host
    written: List[str] = []
    t0 = time.perf_counter()
    classes = None
    if not job.regression:
        ncls = job.num_classes if job.num_classes is not None else max(2, int(canvas.max()) + 1)
        classes = (fill, ncls)
        if job.products:
            import torch

            canvas = _write_products(canvas[None], [(name, profile)], output_folder, fill, ncls, opts=opts, zone_list=job.zone_list)[0]
            torch.cuda.synchronize()
            written += [_output_path(name, output_folder, kind, ext) for on, kind, ext in (
                (opts.save_regions, "regions", ".csv"), (opts.save_polygons, "polygons", ".geojson"), (opts.zones is not None, "zones", ".csv")) if on]
    job.t["products"] += time.perf_counter() - t0
    t0 = time.perf_counter()
    kind = "mean" if job.regression else "mode"
    stats = _output_path(name, output_folder, "cogstats", ".json")
    if host and opts.cog:
        out = _write_cog_host(canvas, kind, _output_path(name, output_folder, "predictions"), stats, profile, opts, fill,
                              classes[1] if classes else None)
    elif host:
        out = save_prediction(canvas, name, output_folder, profile, kind="predictions")
    else:
        out = _write_raster(canvas, "predictions", kind, profile, name, output_folder, opts, classes=classes)
    written.append(out)
    if opts.cog and classes is not None and classes[1] <= cogmod.MAX_CLASSES:
        written.append(stats)
    if cover is not None:
        tags = {kk: v for kk, v in profile["tags"].items() if kk != 42113}
        cov = cover if host else cover.cpu().numpy()
        written.append(save_prediction(cov, name, output_folder, dict(profile, dtype="uint8", nodata=None, tags=tags), kind="cover"))
    job.t["write"] += time.perf_counter() - t0
    return written


def merge_predictions(paths_or_folder: Union[str, Sequence[str]], output_folder: str, rule: str = "last", fill: int = -1,
                      num_classes: Optional[int] = None, device: str = "gpu", cog: bool = True, cog_blocksize: int = 256,
                      overview_levels: Union[str, int] = "auto", cog_compress: Optional[str] = "deflate", min_region: int = 0,
                      connectivity: int = 4, sieve_passes: int = 8, save_regions: bool = False, save_polygons: bool = False,
                      zones: Optional[str] = None, zone_id_property: Optional[str] = None, save_cover: bool = False) -> List[str]:
    """The per-chip ``prediction_*.tif`` files of chip inference -> ``predictions_merged.tif`` (the reference's name), one raster on the
    chips' common grid.  ``paths_or_folder``: a folder (its ``prediction_*.tif`` files in sorted name order) or a list of files; that
    order is the chip index of ``rule`` (last | first | mode for int8 class maps, last | first | mean for the float32 files of
    regression heads), so ``last`` is reproducible.  Chips of several grids (:func:`placement`) give ``predictions_merged_<k>.tif``, k in
    order of first appearance.  Returns the written paths.

    The files are read in a pool of at most 8 threads, placed, packed, uploaded and pasted by ``ig_mosaic_paste``; the canvas then takes
    the way of a tile's class map through the output writer of :mod:`instageo_amd.infer_utils`: the sieve (``min_region``,
    ``connectivity``, ``sieve_passes``), ``regions_merged.csv`` (``save_regions``), ``polygons_merged.geojson`` (``save_polygons``),
    ``zones_merged.csv`` (``zones``, ``zone_id_property``), so regions, polygons and zones describe whole objects, not objects cut at
    chip seams; with ``cog`` the raster is a Cloud Optimized GeoTIFF (``cog_blocksize``, ``overview_levels``, ``cog_compress``; mode
    overviews that ignore ``fill`` for class maps, NaN-aware mean overviews for floats) and ``cogstats_merged.json`` holds the class
    histogram in the reference's form, else a strip file.  ``num_classes``: of the model; None = the largest value on the canvas + 1
    (at least 2).  ``save_cover`` also writes ``cover_merged.tif`` (uint8 strip file: the contributors of every pixel, at most 255).
    A float32 mosaic has no class products: asking for them raises as in chip inference.  All options are checked before a file is read.

    ``device="cpu"`` pastes and builds the pyramid on the host (the numpy twins of the kernels) and writes the same bytes; the class
    products run on the device only and are refused there."""
    job = prepare(paths_or_folder, output_folder, rule, fill, num_classes, device, cog, cog_blocksize, overview_levels, cog_compress, min_region,
                  connectivity, sieve_passes, save_regions, save_polygons, zones, zone_id_property)
    written: List[str] = []
    for k, g in enumerate(job.groups):
        name = "merged.tif" if len(job.groups) == 1 else f"merged_{k}.tif"
        canvas, cover = paste_group(job, g, rule, save_cover)
        written += write_canvas(job, canvas, cover, name, g.profile, output_folder)
    TIMINGS.clear()
    TIMINGS.update(job.t)
    return written
