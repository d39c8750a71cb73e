"""Reprojection and resampling of rasters onto one grid, on the device: one mosaic across UTM zones.

HLS chips live on MGRS tiles in UTM, and a prediction run over a country crosses zone borders.  :func:`instageo_amd.mosaic.merge_predictions`
gives one mosaic per coordinate system; :func:`merge_reprojected` warps those group canvases onto one target grid and hands the one canvas
to the same products and the same writer.  The reference's viewer reprojects with rasterio before display (``apps/viz.py``).

The rule (stated in ``include/instageo_hip.h``).  A grid is north-up, (X0, Y0, sx, sy) with its (h, w); the centre of destination pixel
(r, c) goes through the inverse projection of the destination's coordinate system and the forward projection of the source's to the
source pixel coordinates (u, v), pixel (r, c) of the source covering [c, c + 1) x [r, r + 1).  ``nearest`` takes the pixel (floor(v),
floor(u)); ``bilinear`` (float32) the four neighbours around (u - 1/2, v - 1/2) with float64 weights, those outside the source or NaN
dropped and the rest renormalised.  A value is transparent as in the mosaic (int8 ``== fill``, float32 NaN); of the sources that
contribute, ``last`` takes the one with the largest index, ``first`` the smallest; none: ``fill`` / NaN.

Device tensors go through ``ig_warp``; host arrays take a numpy twin of the same rule on top of :mod:`instageo_amd.crs`, so the merge
works (and is tested) without a GPU.

Not done: datums other than WGS84, polar stereographic, rotated rasters, cubic / average / class-mode resampling, an interpolated
approximate transformer, warping tile-inference canvases or zone polygons, multi-band inputs, more than 8 sources in one warp.
"""
from __future__ import annotations

import time
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import crs as crsmod
from . import mosaic, postprocess
from .prep import is_device

RESAMPLING = ("nearest", "bilinear")
RULES = ("last", "first")
BLOCK = mosaic.BLOCK
MAX_SOURCES = 8  # of one launch (include/instageo_hip.h)
EDGE_POINTS = 21  # per edge of a source's border, for the extent of the target grid
_NAN = np.uint32(0x7FC00000).view(np.float32)
TIMINGS: Dict[str, float] = {}  # wall seconds of the phases of the latest merge_reprojected: read, paste, warp, products, write


def grid_of(profile: Dict[str, Any], name: str = "the raster") -> Tuple[float, float, float, float]:
    """(X0, Y0, sx, sy) of a north-up GeoTIFF profile: the outer corner of its top-left pixel and its positive pixel sizes."""
    if 34264 in ((profile or {}).get("tags") or {}):
        raise ValueError(f"{name}: a ModelTransformation tag (rotated or sheared raster) is not a north-up grid")
    g = postprocess.georeference(profile)
    if g is None or g[0] <= 0 or g[1] <= 0:
        raise ValueError(f"{name}: no georeferencing (needs a ModelPixelScale and a ModelTiepoint tag with positive scales)")
    return float(g[4] - g[2] * g[0]), float(g[5] + g[3] * g[1]), float(g[0]), float(g[1])


def check_resampling(resampling: str, dtype) -> None:
    """ValueError unless ``resampling`` goes with rasters of ``dtype`` (int8: nearest, float32: nearest | bilinear)."""
    name = np.dtype(str(dtype).replace("torch.", "")).name
    if resampling not in RESAMPLING:
        raise ValueError(f"resampling must be one of {RESAMPLING} (got {resampling!r})")
    if name not in ("int8", "float32"):
        raise ValueError(f"a warp takes int8 class maps or float32 rasters (got {name})")
    if resampling == "bilinear" and name != "float32":
        raise ValueError("bilinear resampling does not go with int8 class maps (classes are not interpolated)")


# ---- the target grid ---------------------------------------------------------------------------------------------------------------------
def target_grid(profiles: Sequence[Dict[str, Any]], shapes: Sequence[Tuple[int, int]], crs: Union[str, crsmod.Crs] = "first",
                resolution: Optional[float] = None) -> Tuple[Dict[str, Any], Tuple[int, int]]:
    """The grid in ``crs`` (``"first"``: the first source's, ``"EPSG:n"`` or a :class:`crs.Crs`) that holds every source -> (profile,
    (H, W)).  The extent comes from every source's border, sampled at 21 points per edge and projected to the target; the origin and
    the far corner are snapped outward to multiples of ``resolution``, so the grid does not depend on the order of the files.
    ``resolution`` defaults to the first source's pixel size when source and target share a unit (metres or degrees); otherwise a
    ValueError asks for it.  The profile is the first source's with the target's GeoKeys (tags 34736 / 34737 dropped), pixel scale and
    tiepoint.  A canvas beyond ``mosaic.LIMIT`` or the kernel's limits raises."""
    if len(profiles) != len(shapes) or not profiles:
        raise ValueError(f"{len(profiles)} profiles but {len(shapes)} shapes (at least one of each)")
    systems = [crsmod.from_profile(p) for p in profiles]
    target = systems[0] if isinstance(crs, str) and crs == "first" else crs if isinstance(crs, crsmod.Crs) else crsmod.parse(crs)
    if resolution is None:
        if systems[0].unit != target.unit:
            raise ValueError(f"the first source is in {systems[0].unit}s and EPSG:{target.epsg} in {target.unit}s: give a resolution")
        g = grid_of(profiles[0])
        if g[2] != g[3]:
            raise ValueError(f"the first source has pixels of {g[2]} x {g[3]}: give a resolution")
        resolution = g[2]
    if isinstance(resolution, bool) or not isinstance(resolution, (int, float, np.integer, np.floating)) or not 0 < float(resolution) < np.inf:
        raise ValueError(f"resolution must be a positive number (got {resolution!r})")
    res = float(resolution)
    lo_x = lo_y = np.inf
    hi_x = hi_y = -np.inf
    t = np.linspace(0.0, 1.0, EDGE_POINTS)
    for k, (prof, (h, w), system) in enumerate(zip(profiles, shapes, systems)):
        X0, Y0, sx, sy = grid_of(prof, f"source {k}")
        ex, ey = X0 + t * (w * sx), Y0 - t * (h * sy)
        bx = np.concatenate([ex, ex, np.full_like(t, X0), np.full_like(t, X0 + w * sx)])
        by = np.concatenate([np.full_like(t, Y0), np.full_like(t, Y0 - h * sy), ey, ey])
        x, y = crsmod.transform(system, target, bx, by)  # source -> target: the target plays the "source system" of the forward step
        if not (np.isfinite(x).all() and np.isfinite(y).all()):
            raise ValueError(f"source {k} reaches outside the domain of EPSG:{target.epsg}")
        lo_x, hi_x, lo_y, hi_y = min(lo_x, x.min()), max(hi_x, x.max()), min(lo_y, y.min()), max(hi_y, y.max())
    X0, Y0 = float(np.floor(lo_x / res) * res), float(np.ceil(hi_y / res) * res)
    W, H = int(np.ceil(hi_x / res) - np.floor(lo_x / res)), int(np.ceil(hi_y / res) - np.floor(lo_y / res))
    H, W = max(H, 1), max(W, 1)
    if max(H, W) > mosaic.LIMIT:
        raise ValueError(f"a target canvas of {H} x {W} pixels is beyond the kernel's limits")
    mosaic.check_canvas(H, W)
    first = dict(profiles[0])
    tags = {k: v for k, v in first["tags"].items() if k not in (34735, 34736, 34737, 34264)}
    tags.update(crsmod.geokeys(target.epsg))
    tags[33550] = (12, (res, res, 0.0))
    tags[33922] = (12, (0.0, 0.0, 0.0, X0, Y0, 0.0))
    return dict(first, width=W, height=H, tags=tags), (H, W)


# ---- coordinates and block lists -----------------------------------------------------------------------------------------------------
def coords(dst_crs, dst_grid, shape: Tuple[int, int], src_crs, src_grid, at: str = "centres"):
    """numpy twin of ``ig_warp_coords``: (u, v) float64 (H, W) of the destination's pixel centres in the source grid, NaN outside the
    domain.  ``at="corners"``: of its (H + 1, W + 1) pixel corners instead."""
    H, W = int(shape[0]), int(shape[1])
    X0, Y0, sx, sy = (float(v) for v in dst_grid)
    off = 0.5 if at == "centres" else 0.0
    n = 0 if at == "centres" else 1
    x = X0 + (np.arange(W + n, dtype=np.float64) + off) * sx
    y = Y0 - (np.arange(H + n, dtype=np.float64) + off) * sy
    xs, ys = crsmod.transform(dst_crs, src_crs, *np.meshgrid(x, y))
    with np.errstate(invalid="ignore"):
        u, v = (xs - float(src_grid[0])) / float(src_grid[2]), (float(src_grid[1]) - ys) / float(src_grid[3])
    bad = np.isnan(u) | np.isnan(v)
    return np.where(bad, np.nan, u), np.where(bad, np.nan, v)


def block_lists(dst_crs, dst_grid, shape: Tuple[int, int], src_crs, src_grid, src_size, margin: float = 2.0) -> Tuple[np.ndarray, np.ndarray]:
    """-> (bin_ptr (blocks + 1,) int32, bin_idx int32): for every 64 x 64 block of the destination (row-major) the sources that can reach
    it, ascending.  Conservative: the host projection (:mod:`crs`) gives (u, v) at the block's four corners; a source is listed when the
    box of those, grown by ``margin`` source pixels plus an eighth of its own extent (the curvature of a projection across 64 pixels
    is far below that), meets the source grown by one pixel (the reach of a bilinear neighbour); a block with a corner outside the
    domain lists every source."""
    H, W = int(shape[0]), int(shape[1])
    nby, nbx = -(-H // BLOCK), -(-W // BLOCK)
    X0, Y0, sx, sy = (float(v) for v in dst_grid)
    # the corner lattice in destination pixels, the last row / column clipped to the raster's edge
    cx = np.minimum(np.arange(nbx + 1) * BLOCK, W).astype(np.float64)
    cy = np.minimum(np.arange(nby + 1) * BLOCK, H).astype(np.float64)
    gx, gy = np.meshgrid(X0 + cx * sx, Y0 - cy * sy)
    src_crs = np.asarray(src_crs, dtype=np.float64).reshape(-1, 5)
    src_grid = np.asarray(src_grid, dtype=np.float64).reshape(-1, 4)
    src_size = np.asarray(src_size, dtype=np.int64).reshape(-1, 2)
    hit = np.zeros((len(src_crs), nby, nbx), dtype=bool)
    for i, (c, g, (h, w)) in enumerate(zip(src_crs, src_grid, src_size)):
        xs, ys = crsmod.transform(dst_crs, c, gx, gy)
        with np.errstate(invalid="ignore"):
            u, v = (xs - g[0]) / g[2], (g[1] - ys) / g[3]
        four = lambda a: np.stack([a[:-1, :-1], a[:-1, 1:], a[1:, :-1], a[1:, 1:]])  # noqa: E731
        u4, v4 = four(u), four(v)
        nan = np.isnan(u4).any(axis=0) | np.isnan(v4).any(axis=0)
        with np.errstate(invalid="ignore"):
            ulo, uhi, vlo, vhi = u4.min(axis=0), u4.max(axis=0), v4.min(axis=0), v4.max(axis=0)
            mu, mv = margin + (uhi - ulo) / 8.0, margin + (vhi - vlo) / 8.0
            hit[i] = nan | ((uhi + mu >= -1.0) & (ulo - mu <= w + 1.0) & (vhi + mv >= -1.0) & (vlo - mv <= h + 1.0))
    per_block = hit.reshape(len(src_crs), -1).T  # (blocks, sources)
    ptr = np.concatenate([[0], np.cumsum(per_block.sum(axis=1))])
    idx = np.nonzero(per_block)[1]  # row-major: by block, then ascending source
    return ptr.astype(np.int32), idx.astype(np.int32)


# ---- the rule on host arrays -----------------------------------------------------------------------------------------------------------
def _sample_host(a: np.ndarray, u: np.ndarray, v: np.ndarray, resampling: str, fill: int):
    """-> (value, contributes) of source ``a`` at (u, v), the numpy twin of the kernel's sampling."""
    h, w = a.shape
    ok = ~(np.isnan(u) | np.isnan(v))
    u, v = np.where(ok, u, -9.0), np.where(ok, v, -9.0)
    if resampling == "nearest":
        fc, fr = np.floor(u), np.floor(v)
        ok &= (fc >= 0) & (fc < w) & (fr >= 0) & (fr < h)
        val = a[np.where(ok, fr, 0).astype(np.int64), np.where(ok, fc, 0).astype(np.int64)]
        ok &= ~np.isnan(val) if a.dtype == np.float32 else val != fill
        return val, ok
    fc, fr = np.floor(u - 0.5), np.floor(v - 0.5)
    near = ok & (fc >= -1) & (fc < w) & (fr >= -1) & (fr < h)
    fc, fr = np.where(near, fc, 0.0), np.where(near, fr, 0.0)
    wx, wy = np.where(near, u - 0.5 - fc, 0.0), np.where(near, v - 0.5 - fr, 0.0)
    acc, tot = np.zeros(u.shape), np.zeros(u.shape)
    for dr, dc, wt in ((0, 0, (1 - wx) * (1 - wy)), (0, 1, wx * (1 - wy)), (1, 0, (1 - wx) * wy), (1, 1, wx * wy)):
        rr, cc = (fr + dr).astype(np.int64), (fc + dc).astype(np.int64)
        inside = near & (rr >= 0) & (rr < h) & (cc >= 0) & (cc < w) & (wt > 0)
        x = a[np.where(inside, rr, 0), np.where(inside, cc, 0)].astype(np.float64)
        inside &= ~np.isnan(x)
        acc = np.where(inside, acc + wt * np.where(inside, x, 0.0), acc)
        tot = np.where(inside, tot + wt, tot)
    good = tot > 0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        val = (acc / np.where(good, tot, 1.0)).astype(np.float32)
    return val, good


def _warp_host(arrays, systems, grids, dst_crs, dst_grid, shape, resampling, rule, fill):
    H, W = shape
    dtype = arrays[0].dtype
    out = np.full((H, W), _NAN if dtype == np.float32 else fill, dtype=dtype)
    sid = np.full((H, W), 255, dtype=np.uint8)
    order = range(len(arrays)) if rule == "last" else reversed(range(len(arrays)))  # the winner is written last
    for i in order:
        u, v = coords(dst_crs, dst_grid, shape, systems[i], grids[i])
        val, ok = _sample_host(arrays[i], u, v, resampling, fill)
        out[ok] = val[ok]
        sid[ok] = i
    return out, sid


def warp(sources, profiles: Sequence[Dict[str, Any]], dst_profile: Dict[str, Any], shape: Tuple[int, int], resampling: str = "nearest",
         rule: str = "last", fill: int = -1, src_id: bool = False):
    """``sources`` (2-D arrays / tensors of one dtype, int8 or float32, at most 8) with their GeoTIFF ``profiles`` -> the raster of
    ``shape`` = (H, W) on the grid of ``dst_profile``, by ``resampling`` and ``rule`` (the module docstring); with ``src_id`` also the
    (H, W) uint8 index of the source that gave each pixel (255: none).  Tensors on the device are packed and go through ``ig_warp`` and
    give device tensors; anything else takes the numpy twin and gives arrays."""
    sources = list(sources)
    if not sources or len(sources) != len(profiles):
        raise ValueError(f"{len(sources)} sources but {len(profiles)} profiles (at least one of each)")
    if len(sources) > MAX_SOURCES:
        raise ValueError(f"one warp takes at most {MAX_SOURCES} sources (got {len(sources)})")
    dev = is_device(sources[0])
    if not dev:
        sources = [np.asarray(s.cpu() if hasattr(s, "cpu") else s) for s in sources]
    if any(s.dtype != sources[0].dtype for s in sources):
        raise ValueError("the sources of a warp have one dtype")
    check_resampling(resampling, sources[0].dtype)
    if rule not in RULES:
        raise ValueError(f"a warp composes its sources by rule {RULES} (got {rule!r})")
    fill = mosaic.check_fill(fill)
    H, W = int(shape[0]), int(shape[1])
    mosaic.check_canvas(H, W)
    for i, s in enumerate(sources):
        if s.ndim != 2 or min(s.shape) < 1 or max(s.shape) > mosaic.LIMIT:
            raise ValueError(f"source {i} is {tuple(s.shape)}: a raster is 2-D with 1 <= h, w <= 2^30")
    systems = [crsmod.from_profile(p).params for p in profiles]
    grids = [grid_of(p, f"source {i}") for i, p in enumerate(profiles)]
    dst_crs, dst_grid = crsmod.from_profile(dst_profile).params, grid_of(dst_profile, "the destination")
    if not dev:
        out, sid = _warp_host(sources, systems, grids, dst_crs, dst_grid, (H, W), resampling, rule, fill)
        return (out, sid) if src_id else out
    import torch

    from . import ops

    sizes = np.array([s.shape for s in sources], dtype=np.int64)
    n = sizes[:, 0] * sizes[:, 1]
    packed = torch.cat([s.reshape(-1) for s in sources]) if len(sources) > 1 else sources[0].reshape(-1)
    ptr, idx = block_lists(dst_crs, dst_grid, (H, W), systems, grids, sizes)
    return ops.warp(packed, np.cumsum(n) - n, systems, grids, sizes, ptr, idx, dst_crs, dst_grid, (H, W), resampling, rule, fill, src_id)


# ---- files -> files ----------------------------------------------------------------------------------------------------------------------
def merge_reprojected(paths_or_folder: Union[str, Sequence[str]], output_folder: str, crs: Union[str, crsmod.Crs] = "first",
                      resolution: Optional[float] = None, resampling: Optional[str] = None, rule: str = "last", fill: int = -1,
                      num_classes: Optional[int] = None, device: str = "gpu", cog: bool = True, cog_blocksize: int = 256,
                      overview_levels: Union[str, int] = "auto", cog_compress: Optional[str] = "deflate", min_region: int = 0,
                      connectivity: int = 4, sieve_passes: int = 8, save_regions: bool = False, save_polygons: bool = False,
                      zones: Optional[str] = None, zone_id_property: Optional[str] = None, save_cover: bool = False) -> List[str]:
    """:func:`mosaic.merge_predictions` across coordinate systems: ONE ``predictions_merged.tif`` in ``crs`` (``"first"``: the first
    file's, or ``"EPSG:n"``) at ``resolution`` (:func:`target_grid`), with one set of region, polygon and zone products, so an object on
    a UTM zone seam is one object.  The files are read and grouped by coordinate system (:func:`mosaic.placement`), every group is pasted
    on its own grid under ``rule`` exactly as ``merge_predictions`` does, and the group canvases are warped onto the target grid by
    ``ig_warp`` (``resampling``: None = nearest for int8 class maps, bilinear for float32 rasters; bilinear with class maps raises).
    Across groups the order is that of first appearance: ``first`` lets the earlier group win where two reach a pixel, every other rule
    the later one; ``mode`` and ``mean`` apply inside a group only (zones overlap only at their seam).  The canvas then goes through
    the same products and the same writer as in ``merge_predictions``, under the target's GeoKeys (the zone polygons are expected in
    the target's coordinates).  A single group already on the target grid is warped too (the same-system shortcut: affine arithmetic).
    ``save_cover`` is refused: contributor counts belong to a group's own grid.  At most 8 groups.  Returns the written paths.

    ``device="cpu"`` pastes, warps and builds the pyramid on the host (numpy twins) and writes the raster only, as there."""
    if save_cover:
        raise ValueError("a reprojected mosaic has no cover raster (contributor counts belong to a group's own grid)")
    if resampling is not None and resampling not in RESAMPLING:
        raise ValueError(f"resampling must be None or one of {RESAMPLING} (got {resampling!r})")
    target = crs if isinstance(crs, crsmod.Crs) or crs == "first" else crsmod.parse(crs)
    job = mosaic.prepare(paths_or_folder, output_folder, rule, fill, num_classes, device, cog, cog_blocksize, overview_levels, cog_compress,
                         min_region, connectivity, sieve_passes, save_regions, save_polygons, zones, zone_id_property)
    resampling = resampling or ("bilinear" if job.regression else "nearest")
    check_resampling(resampling, job.arrays[0].dtype)
    if len(job.groups) > MAX_SOURCES:
        raise ValueError(f"the files span {len(job.groups)} pixel grids; one warp takes at most {MAX_SOURCES}")
    profiles = [g.profile for g in job.groups]
    dst_profile, shape = target_grid(profiles, [g.shape for g in job.groups], target, resolution)
    canvases = [mosaic.paste_group(job, g, rule, False)[0] for g in job.groups]
    t0 = time.perf_counter()
    canvas = warp(canvases, profiles, dst_profile, shape, resampling, "first" if rule == "first" else "last", job.fill)
    if not job.host:
        import torch

        torch.cuda.synchronize()
    t_warp = time.perf_counter() - t0
    written = mosaic.write_canvas(job, canvas, None, "merged.tif", dst_profile, output_folder)
    TIMINGS.clear()
    TIMINGS.update(job.t, warp=t_warp)
    return written
