"""Chips and label maps cut from Sentinel-1 RTC scenes stacked per date, on the device.

The reference's radar source (``instageo/data/s1_utils.py``: ``S1PointsPipeline``) opens ``vv`` / ``vh`` of every scene of every date as
float32 through ``stackstac.stack(..., epsg, resolution, fill_value=-1)``, which resamples all of them (nearest) onto one lattice over the
union of their bounds, and then cuts chips as for HLS; there is no mask band (``NO_DATA_VALUES.S1 = -1``: validity comes from the values).
Here every scene stays on its own grid, in its own coordinate system, packed into one float32 buffer, and ``ig_s1_chip_cut``
(``s1_chips.hip``) reads each where it lies while it cuts.  This module is the host layer on top of :mod:`instageo_amd.prep`,
:mod:`instageo_amd.tiff`, :mod:`instageo_amd.crs` and the point geometry and label maps of :mod:`instageo_amd.chips`.

The rule (stated in ``include/instageo_hip.h``).  T dates of C bands; date t has n_t >= 1 scenes (the slices of its orbit), 32 scenes at
most in all; scene s has a coordinate system, a grid (X0, Y0, sx, sy), a size (H, W) and C float32 planes.  The centre of pixel (r, c) of
the chip at (row0, col0) of the stack lattice, ``x = X0 + (col0 + c + 0.5) sx``, ``y = Y0 - (row0 + r + 0.5) sy``, is mapped into every
scene by the chain of the warp (the affine arithmetic alone for a scene in the stack's system) and read at ``floor``.  Band b of date t
takes the value of the first scene of the date, in list order, that the pixel lies inside and whose value is present (not NaN, not
``src_nodata``), bits copied; without one it is ``no_data_value`` (-1).  ``clip`` bounds present values.  With the chips come
``valid_values`` and the validity plane of :func:`chips.cut`, which :func:`chips.label_maps` reads unchanged.

Device tensors go through ``ig_s1_chip_cut``; host arrays take a numpy twin of the same rule, so the module works (and is tested) without
a GPU and both write the same bytes.

Not done: STAC search and signing, SAFE / GRD input and calibration, any resampling but nearest, rotated rasters.  Chips on the grids of
label rasters are :mod:`instageo_amd.s1_raster_chips`.  Speckle filtering and dB conversion are :mod:`instageo_amd.s1_filter`, whose
output files this module takes as they are.
"""
from __future__ import annotations

import os
import re
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import chips as chipmod
from . import crs as crsmod
from . import prep, raster_chips, warp
from .prep import MAX_DATES, STRATEGIES, is_device, to_host  # noqa: F401  (the masking strategies and the date limit of include/instageo_hip.h)

NO_DATA_VALUE = -1.0  # the reference's NO_DATA_VALUES.S1, stackstac's fill_value
MAX_SCENES = 32  # of one launch, over all dates (include/instageo_hip.h)
MAX_SIDE = raster_chips.MAX_SIDE
BANDS = ("vv", "vh")


# ---- argument checks shared by the host path and the device wrapper (ops.s1_chip_cut) -------------------------------------------------------
def _f32(v, what: str, optional: bool = False) -> Optional[np.float32]:
    if v is None and optional:
        return None
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or np.isnan(np.float32(v)):
        raise ValueError(f"{what} must be a number that is not NaN (got {v!r})")
    return np.float32(v)


def check_scenes(size: int, starts, scene_crs, scene_grid, scene_size, date_scenes, S: int, no_data_value, src_nodata, clip):
    """The checks of the sources and of the value rule, shared by :func:`check_cut` and :func:`s1_raster_chips.check_warp`: ValueError
    unless they obey include/instageo_hip.h -> (starts int64 (N * C,), scene_crs (N, 5) float64, scene_grid (N, 4) float64, scene_size
    (N, 2) int32, first_bits, T, C, no_data, src_nodata or None, clip (lo, hi) or None) with the three values as float32.  A scene's
    grid may not be unusable."""
    if isinstance(S, bool) or not isinstance(S, (int, np.integer)) or not 1 <= int(S) <= MAX_SIDE:
        raise ValueError(f"chip_size must be an int in [1, 2^15] (got {S!r})")
    S = int(S)
    counts = [int(k) for k in np.asarray(date_scenes).reshape(-1).tolist()] if np.asarray(date_scenes).dtype.kind in "iu" else None
    if counts is None or not 1 <= len(counts) <= MAX_DATES:
        raise ValueError(f"date_scenes holds the number of scenes of each of 1 <= T <= {MAX_DATES} dates (got {date_scenes!r})")
    if min(counts) < 1:
        raise ValueError(f"every date needs at least one scene (got {counts})")
    T, N = len(counts), sum(counts)
    if N > MAX_SCENES:
        raise ValueError(f"{N} scenes in all: at most {MAX_SCENES} go into one stack")
    sc = np.stack([raster_chips.params(c) for c in scene_crs]).reshape(-1, 5) if len(scene_crs) else np.zeros((0, 5))
    sg = np.ascontiguousarray(scene_grid, dtype=np.float64)
    ss = np.asarray(scene_size)
    if sg.size != 4 * N or ss.size != 2 * N or sc.shape[0] != N or ss.size and ss.dtype.kind not in "iu":
        raise ValueError(f"{N} scenes need {N} coordinate systems, {N} grids (X0, Y0, sx, sy) and {N} integer sizes (H, W)")
    sg, ss = sg.reshape(N, 4), ss.astype(np.int64).reshape(N, 2)
    if not all(raster_chips.grid_ok(g) for g in sg):
        raise ValueError("a scene grid = (X0, Y0, sx, sy) needs finite values and positive pixel sizes")
    if (ss < 1).any() or (ss[:, 0] * ss[:, 1] > 2**31 - 1).any():
        raise ValueError("a scene has 1 <= H * W <= 2^31 - 1 pixels (source offsets are int32)")
    st = np.asarray(starts)
    if st.size and st.dtype.kind not in "iu":
        raise ValueError("the offsets of the planes must be integers")
    st = np.ascontiguousarray(st.astype(np.int64).reshape(-1))
    if st.shape[0] < N or st.shape[0] % N:
        raise ValueError(f"{st.shape[0]} planes do not divide into {N} scenes of C >= 1 bands")
    C = st.shape[0] // N
    if int(size) >= 2**40:
        raise ValueError("the packed planes hold 2^40 elements or more")
    if (st < 0).any() or (st + np.repeat(ss[:, 0] * ss[:, 1], C) > int(size)).any():
        raise ValueError(f"a plane does not lie inside the packed buffer of {size} elements")
    if T * C * S * S > 2**31 - 1:
        raise ValueError(f"a chip of {T * C} x {S} x {S} values is beyond 2^31 - 1 (valid_values is int32)")
    nd = _f32(no_data_value, "no_data_value")
    snd = _f32(src_nodata, "src_nodata", optional=True)
    if clip is not None:
        if not isinstance(clip, (list, tuple)) or len(clip) != 2:
            raise ValueError(f"clip must be None or (lo, hi) with lo <= hi (got {clip!r})")
        clip = (_f32(clip[0], "clip"), _f32(clip[1], "clip"))
        if not clip[0] <= clip[1]:
            raise ValueError(f"clip must be None or (lo, hi) with lo <= hi (got {clip!r})")
    first_bits = 0
    at = 0
    for k in counts:
        first_bits |= 1 << at
        at += k
    return (st, np.ascontiguousarray(sc, dtype=np.float64), sg, np.ascontiguousarray(ss, dtype=np.int32), first_bits, T, C, nd, snd, clip)


def check_cut(size: int, starts, scene_crs, scene_grid, scene_size, date_scenes, dst_crs, dst_grid, origins, S: int, no_data_value,
              src_nodata, clip):
    """ValueError unless the arguments of a cut obey include/instageo_hip.h -> (starts int64 (N * C,), scene_crs (N, 5) float64,
    scene_grid (N, 4) float64, scene_size (N, 2) int32, first_bits, T, C, dst_crs (5,), dst_grid (4,), origins (n, 2) int32, no_data,
    src_nodata or None, clip (lo, hi) or None) with the three values as float32.  The stack grid may be unusable (it gives no-data
    chips); a scene's grid may not."""
    st, sc, sg, ss, first_bits, T, C, nd, snd, clip = check_scenes(size, starts, scene_crs, scene_grid, scene_size, date_scenes, S,
                                                                   no_data_value, src_nodata, clip)
    S = int(S)
    dg = np.ascontiguousarray(dst_grid, dtype=np.float64).reshape(-1)
    if dg.shape[0] != 4:
        raise ValueError(f"the stack grid is (X0, Y0, sx, sy) (got {dst_grid!r})")
    o = np.asarray(origins)
    if o.size and o.dtype.kind not in "iu":
        raise ValueError("origins must be integers")
    o = o.astype(np.int64).reshape(-1, 2)
    if o.size and (o.min() < -(2**31) or o.max() > 2**31 - 1):
        raise ValueError("origins must fit int32")
    if o.shape[0] * T * C * S * S >= 2**40:
        raise ValueError(f"{o.shape[0]} chips of {T * C} x {S} x {S} values are beyond 2^40")
    return st, sc, sg, ss, first_bits, T, C, raster_chips.params(dst_crs), dg, np.ascontiguousarray(o, dtype=np.int32), nd, snd, clip


# ---- the rule on host arrays ---------------------------------------------------------------------------------------------------------------
def _cut_host(planes, st, sc, sg, ss, first_bits, T, C, dc, dg, origins, S, nd, snd, clip):
    """numpy twin of ``ig_s1_chip_cut``: chip by chip and scene by scene, vectorised over the pixels."""
    N = sg.shape[0]
    first = [s for s in range(N) if first_bits >> s & 1] + [N]
    n = origins.shape[0]
    chips = np.full((n, T * C, S, S), nd, dtype=np.float32)
    validity = np.empty((n, S, S), dtype=np.uint8)
    usable = raster_chips.grid_ok(dg)
    same = [tuple(sc[s]) == tuple(dc) for s in range(N)]
    step = np.arange(S, dtype=np.float64)
    for i, (r0, c0) in enumerate(origins.tolist()):
        got = np.zeros((T * C, S, S), dtype=bool)  # the values that a scene gave
        if usable:
            x, y = np.meshgrid(dg[0] + (float(c0) + step + 0.5) * dg[2], dg[1] - (float(r0) + step + 0.5) * dg[3])
            lonlat = None
            for t in range(T):
                for s in range(first[t], first[t + 1]):
                    mine = got[t * C : (t + 1) * C]
                    if mine.all():
                        break
                    xs, ys = x, y
                    if not same[s]:
                        if lonlat is None:
                            lonlat = crsmod.inverse(dc, x, y)  # once per pixel
                        xs, ys = crsmod.forward(sc[s], *lonlat)
                    H, W = int(ss[s, 0]), int(ss[s, 1])
                    with np.errstate(invalid="ignore"):
                        fc, fr = np.floor((xs - sg[s, 0]) / sg[s, 2]), np.floor((sg[s, 1] - ys) / sg[s, 3])
                        inside = (fc >= 0) & (fc < W) & (fr >= 0) & (fr < H)
                    at = fr[inside].astype(np.int64) * W + fc[inside].astype(np.int64)
                    for b in range(C):
                        k = int(st[s * C + b])
                        v = planes[k : k + H * W][at]
                        present = ~np.isnan(v)
                        if snd is not None:
                            present &= v != snd
                        take = np.zeros((S, S), dtype=bool)
                        take[inside] = present
                        take &= ~mine[b]
                        chips[i, t * C + b][take] = v[take[inside]]
                        mine[b] |= take
        if clip is not None:
            a = chips[i]
            a[got & (a < clip[0])] = clip[0]
            a[got & (a > clip[1])] = clip[1]
        ok = chips[i] != nd
        validity[i] = ok.all(axis=0).astype(np.uint8) | (ok.any(axis=0).astype(np.uint8) << 1)
    valid_values = (chips != nd).reshape(n, T * C * S * S).sum(axis=1).astype(np.int32)
    return chips, valid_values, validity


def cut(planes, starts, scene_crs, scene_grid, scene_size, date_scenes, dst_crs, dst_grid, origins, chip_size: int,
        no_data_value: float = NO_DATA_VALUE, src_nodata: Optional[float] = None, clip: Optional[Tuple[float, float]] = None):
    """Chips of side ``chip_size`` at ``origins`` ((n, 2): row0, col0 on the stack lattice ``dst_grid`` = (X0, Y0, sx, sy) in ``dst_crs``;
    any int32) from the packed planes ``planes`` (1-D float32).  ``date_scenes``: the number of scenes of every date; scene s (date after
    date) has the system ``scene_crs[s]``, the grid ``scene_grid[s]``, the size ``scene_size[s]`` = (H, W) and its C planes at
    ``starts[s * C ..]`` (C = planes per scene) -> (chips (n, T * C, S, S) float32, valid_values (n,) int32, validity (n, S, S) uint8) by
    the rule of the module docstring.  A coordinate system is an EPSG code, a :class:`crs.Crs` or five doubles.  ``src_nodata``: the
    source's own no-data value (None: only NaN is absent); ``clip``: None or (lo, hi) for present values.  A tensor on the device goes
    through ``ig_s1_chip_cut`` and gives device tensors; anything else takes the numpy twin and gives arrays."""
    dev = is_device(planes)
    if not dev:
        planes = to_host(planes)
    if str(planes.dtype).replace("torch.", "") != "float32" or planes.ndim != 1:
        raise ValueError("the planes are one packed 1-D float32 buffer")
    if dev:
        from . import ops

        # checks the same arguments before the upload
        return ops.s1_chip_cut(planes, starts, scene_crs, scene_grid, scene_size, date_scenes, dst_crs, dst_grid, origins, chip_size,
                               no_data_value, src_nodata, clip)
    st, sc, sg, ss, first_bits, T, C, dc, dg, o, nd, snd, clip = check_cut(planes.shape[0], starts, scene_crs, scene_grid, scene_size,
                                                                            date_scenes, dst_crs, dst_grid, origins, chip_size,
                                                                            no_data_value, src_nodata, clip)
    return _cut_host(planes, st, sc, sg, ss, first_bits, T, C, dc, dg, o, int(chip_size), nd, snd, clip)


# ---- the stack lattice ---------------------------------------------------------------------------------------------------------------------
def stack_grid(scenes: Sequence[Tuple[Dict[str, Any], Tuple[int, int]]], epsg: Optional[int] = None,
               resolution: float = 10.0) -> Tuple[Tuple[float, float, float, float], Tuple[int, int], crsmod.Crs]:
    """The lattice ``stackstac.stack(items, epsg, resolution)`` resamples onto: ``scenes`` = [(profile, (H, W))] -> (grid (X0, Y0, res,
    res), (H, W), coordinate system).  The union of the scenes' bounds in EPSG:``epsg`` (None: the first scene's system), where a scene in
    another system contributes the bounds of its outline sampled at 21 points per edge (``transform_bounds``), snapped outward to
    multiples of ``resolution`` (``snap_bounds``; the lattice arithmetic of :func:`raster_chips.snapped_grid`)."""
    if not scenes:
        raise ValueError("a stack needs at least one scene")
    if isinstance(resolution, bool) or not isinstance(resolution, (int, float, np.integer, np.floating)) or not 0 < float(resolution) < np.inf:
        raise ValueError(f"resolution must be a positive number (got {resolution!r})")
    res = float(resolution)
    systems = [crsmod.from_profile(p) for p, _ in scenes]
    target = systems[0] if epsg is None else crsmod.from_epsg(epsg)
    lo_x = lo_y = np.inf
    hi_x = hi_y = -np.inf
    t = np.linspace(0.0, 1.0, warp.EDGE_POINTS)
    for k, ((prof, (h, w)), system) in enumerate(zip(scenes, systems)):
        X0, Y0, sx, sy = warp.grid_of(prof, f"scene {k}")
        if tuple(system)[:5] == tuple(target)[:5]:
            bx, by = np.array([X0, X0 + w * sx]), np.array([Y0 - h * sy, Y0])
        else:
            ex, ey = X0 + t * (w * sx), Y0 - t * (h * sy)
            bx = np.concatenate([ex, ex, np.full_like(t, X0), np.full_like(t, X0 + w * sx)])
            by = np.concatenate([np.full_like(t, Y0), np.full_like(t, Y0 - h * sy), ey, ey])
            bx, by = crsmod.transform(system, target, bx, by)
            if not (np.isfinite(bx).all() and np.isfinite(by).all()):
                raise ValueError(f"scene {k} reaches outside the domain of EPSG:{target.epsg}")
        lo_x, hi_x, lo_y, hi_y = min(lo_x, bx.min()), max(hi_x, bx.max()), min(lo_y, by.min()), max(hi_y, by.max())
    grid = raster_chips.snapped_grid((lo_x, lo_y, hi_x, hi_y), res)
    W, H = int(np.ceil(hi_x / res) - np.floor(lo_x / res)), int(np.ceil(hi_y / res) - np.floor(lo_y / res))
    if max(H, 1) * max(W, 1) > 2**31 - 1:
        raise ValueError(f"a stack lattice of {H} x {W} pixels is beyond 2^31 - 1")
    return grid, (max(H, 1), max(W, 1)), target


# ---- files -> files -------------------------------------------------------------------------------------------------------------------------
def tile_id_of(first_file: str) -> Tuple[str, str]:
    """The reference's S1 tile id (parts 0, 1, 4 and 6..8 of the item id split at ``_``) and the acquisition date YYYYMMDD, from a band
    file named after its item: ``S1A_IW_GRDH_1SDV_20220525T033103_20220525T033128_043365_052DB0_rtc_vv.tif`` ->
    ``S1A_IW_20220525T033103_043365_052DB0_rtc``."""
    p = os.path.splitext(os.path.basename(str(first_file)))[0].split("_")
    if len(p) < 9 or not re.fullmatch(r"\d{8}T\d{6}", p[4]):
        raise ValueError(f"{first_file}: not a Sentinel-1 item name (<mission>_<mode>_<product>_<pol>_<start>_<stop>_<orbit>_<take>_<kind>...)")
    return "_".join(p[0:2] + [p[4]] + p[6:9]), p[4][:8]


def _dates_of(scenes, C: int) -> List[List[List[str]]]:
    """``scenes`` as [date][scene][band]: a date given as one flat list of C files is one scene."""
    if not isinstance(scenes, (list, tuple)) or not scenes:
        raise ValueError("scenes is a list of dates, each a list of scenes, each a list of band files")
    dates = []
    for d in scenes:
        if not isinstance(d, (list, tuple)) or not d:
            raise ValueError(f"a date is a list of scenes (got {d!r})")
        if all(isinstance(f, str) for f in d):
            d = [d]
        for s in d:
            if not isinstance(s, (list, tuple)) or len(s) != C or not all(isinstance(f, str) for f in s):
                raise ValueError(f"a scene is a list of {C} band files (got {s!r})")
        dates.append([list(s) for s in d])
    return dates


def scene_files(scenes, C: int) -> Tuple[List[str], List[int]]:
    """``scenes`` ([date][scene][band] files of ``C`` bands; a flat date is one scene) -> (the files in order, the number of scenes of every
    date).  ValueError for too many dates or scenes."""
    dates = _dates_of(scenes, C)
    counts = [len(d) for d in dates]
    if len(dates) > MAX_DATES or sum(counts) > MAX_SCENES:
        raise ValueError(f"{len(dates)} dates of {sum(counts)} scenes in all: at most {MAX_DATES} dates and {MAX_SCENES} scenes go into one stack")
    return [f for d in dates for s in d for f in s], counts


def read_scenes(files: Sequence[str], C: int):
    """The band files of :func:`scene_files` read -> (the packed float32 planes, their starts, [(profile, (H, W))] per scene).  ValueError
    for band files of one scene that differ in grid, size or coordinate system."""
    planes, starts, shapes, profiles = prep.read_planes(files, "band", np.float32)
    scene_profiles = []
    for k in range(0, len(files), C):
        key = (tuple(crsmod.from_profile(profiles[k]))[:5], warp.grid_of(profiles[k], files[k]), shapes[k])
        for j in range(k + 1, k + C):
            if (tuple(crsmod.from_profile(profiles[j]))[:5], warp.grid_of(profiles[j], files[j]), shapes[j]) != key:
                raise ValueError(f"{files[j]}: its grid, size or coordinate system differs from that of {files[k]}, a band of the same scene")
        scene_profiles.append((profiles[k], shapes[k]))
    return planes, starts, scene_profiles


def create_s1_chips(scenes, points, output_directory: str, chip_size: int = 256, bands: Sequence[str] = BANDS, masking_strategy: str = "each",
                    window_size: int = 0, task_type: str = "seg", src_crs: int = 4326, epsg: Optional[int] = None,
                    spatial_resolution: float = 10.0, no_data_value: float = NO_DATA_VALUE, src_nodata: Optional[float] = None,
                    clip: Optional[Tuple[float, float]] = None, num_classes: Optional[int] = None, device: Optional[str] = None,
                    date: Optional[str] = None) -> Tuple[List[str], List[Optional[str]]]:
    """The reference's ``S1PointsPipeline`` for one stack.  ``scenes``: a list of dates, each a list of scenes (orbit slices, in the order
    they are tried), each a list of ``len(bands)`` single-band float32 GeoTIFF / COG files, every scene on its own grid and in its own
    coordinate system; a date that is one flat list of files is one scene.  ``points``: a CSV path or a table with ``x``, ``y`` (in
    EPSG:``src_crs``), ``label``, ``date``.  The stack lattice is :func:`stack_grid` in EPSG:``epsg`` at ``spatial_resolution``.  Writes
    ``chips/chip_{date}_{tile_id}_{x}_{y}.tif`` (float32, all dates and bands) and ``seg_maps/seg_map_{...}.tif`` (int16 for ``seg``,
    float32 for ``reg``) for every complete chip a point nominates, each with its own tiepoint, the lattice's pixel size and GeoKeys.  The
    label maps are masked by ``masking_strategy`` (``any``: where any value of the pixel is no-data, ``each``: where all are).  A chip with
    no valid value is dropped, then a pair whose label map is empty.  ``chips_dataset.csv`` and ``chips_stats.json`` are those of
    :func:`chips.create_chips`.  ``points=None``: every complete chip of the lattice that has a valid value, no label maps; ``date``: the
    YYYYMMDD of the names then, by default from the first file's name.  ``device``: None = the numpy path, ``"cuda"`` / ``"cuda:n"`` =
    the kernels; both write the same bytes.  -> (chip names, label-map names)."""
    S = int(chip_size)
    if masking_strategy not in STRATEGIES:
        raise ValueError(f"masking_strategy must be one of {tuple(STRATEGIES)} (got {masking_strategy!r})")
    if task_type not in ("seg", "reg"):
        raise ValueError(f"task_type must be seg or reg (got {task_type!r})")
    prep.check_device(device)
    if isinstance(bands, str) or not bands:
        raise ValueError(f"bands is a list of at least one name (got {bands!r})")
    C = len(bands)
    files, counts = scene_files(scenes, C)
    tile_id, stamp_date = tile_id_of(files[0])
    planes, starts, scene_profiles = read_scenes(files, C)
    grid, (H, W), system = stack_grid(scene_profiles, epsg, spatial_resolution)
    tags = {33550: (12, (grid[2], grid[3], 0.0)), 33922: (12, (0.0, 0.0, 0.0, grid[0], grid[1], 0.0)), **crsmod.geokeys(system.epsg)}
    profile = {"tags": tags, "nodata": None}  # the stack lattice as a raster profile
    scene_crs = [crsmod.from_profile(p) for p, _ in scene_profiles]
    scene_grid = [warp.grid_of(p) for p, _ in scene_profiles]
    scene_size = [s for _, s in scene_profiles]
    def cut_at(origins, bbox):
        return cut(prep.to_device(planes, device), starts, scene_crs, scene_grid, scene_size, counts, system, grid, origins, S,
                   no_data_value=no_data_value, src_nodata=src_nodata, clip=clip)

    source = chipmod.PointSource(profile, grid, (H, W), tile_id, stamp_date, "stack", cut_at, None)
    return chipmod.create_from_points(source, points, output_directory, S, window_size, task_type, src_crs, masking_strategy, num_classes, date)


# ---- mode=create_s1_chips ------------------------------------------------------------------------------------------------------------------
CONFIG_KEYS = ("scenes", "records_file", "output_directory", "chip_size", "bands", "masking_strategy", "window_size", "task_type", "src_crs",
               "epsg", "spatial_resolution", "no_data_value", "src_nodata", "clip")


def value_options(c: prep.Section) -> Tuple[float, Optional[float], Optional[Tuple[float, float]]]:
    """The keys ``no_data_value``, ``src_nodata`` and ``clip`` of a Sentinel-1 section, checked."""
    nd = c.number("no_data_value", -1, lambda v: v == v, "must be a number that is not NaN")
    snd = c.get("src_nodata")
    if snd is not None:
        snd = c.number("src_nodata", None, lambda v: v == v, "must be None or a number that is not NaN")
    clip = c.get("clip")
    if clip is not None:
        ok = isinstance(clip, (list, tuple)) and len(clip) == 2 and all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in clip)
        if not ok or not float(clip[0]) <= float(clip[1]):
            raise c.bad("clip", "must be None or [lo, hi] with lo <= hi", clip)
        clip = (float(clip[0]), float(clip[1]))
    return nd, snd, clip


def scenes_option(c: prep.Section, C: int) -> Optional[List[List[List[str]]]]:
    """The key ``scenes`` of a Sentinel-1 section as [date][scene][band] of ``C`` band files, checked; unset gives None."""
    scenes = c.get("scenes")
    if scenes is not None:
        try:
            scenes = _dates_of(scenes, C)
        except ValueError as e:
            raise c.bad("scenes", f"must be a list of dates of scenes of {C} band files ({e})", scenes) from None
        if len(scenes) > MAX_DATES or sum(len(d) for d in scenes) > MAX_SCENES:
            raise c.bad("scenes", f"holds at most {MAX_DATES} dates and {MAX_SCENES} scenes in all", scenes)
    return scenes


def s1_chips_options(cfg: Dict[str, Any]) -> Dict[str, Any]:
    """The ``s1_chips.*`` keys of ``mode=create_s1_chips`` checked -> the keyword arguments of :func:`create_s1_chips`.  A bad value raises
    ValueError; ``scenes`` and ``output_directory`` are required only in that mode."""
    c = prep.Section(cfg, "s1_chips", CONFIG_KEYS)
    size = c.integer("chip_size", 256, lo=1, hi=MAX_SIDE, what="must be an int in [1, 2^15]")
    w = c.integer("window_size", 0, lo=0, hi=chipmod.MAX_WINDOW, what="must be an int >= 0")
    bands = c.listing("bands", list(BANDS))
    if not bands:
        raise c.bad("bands", "must be a list of at least one name", bands)
    strategy = c.choice("masking_strategy", "each", STRATEGIES)
    task = c.choice("task_type", "seg", ("seg", "reg"), "must be seg or reg")
    src = c.epsg("src_crs", 4326)
    epsg = c.epsg("epsg", None)
    res = c.number("spatial_resolution", 10, lambda v: 0 < v < np.inf, "must be a positive number")
    nd, snd, clip = value_options(c)
    scenes = scenes_option(c, len(bands))
    records, out = c.text("records_file"), c.text("output_directory")
    if cfg.get("mode") == "create_s1_chips" and (not scenes or out is None):
        raise ValueError("mode=create_s1_chips needs s1_chips.scenes and s1_chips.output_directory")
    return dict(scenes=scenes, points=records, output_directory=out, chip_size=size, bands=bands, masking_strategy=strategy, window_size=w,
                task_type=task, src_crs=src, epsg=epsg, spatial_resolution=res, no_data_value=nd, src_nodata=snd, clip=clip)


def run_from_config(cfg: Dict[str, Any], device: Optional[str] = None) -> int:
    """``mode=create_s1_chips``: :func:`create_s1_chips` under the ``s1_chips.*`` keys; prints one JSON line with the counts."""
    return prep.run_creator("create_s1_chips", create_s1_chips, s1_chips_options(cfg), device)


def main(argv: Optional[List[str]] = None) -> int:
    """``python -m instageo_amd.s1_chips s1_chips.scenes=[[[a_vv.tif,a_vh.tif]]] s1_chips.output_directory=out ...``: mode=create_s1_chips
    without ``run.py``."""
    return prep.run_mode_cli("create_s1_chips", run_from_config, argv)


if __name__ == "__main__":
    raise SystemExit(main())
