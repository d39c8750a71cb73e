"""Sentinel-1 chips cut against label rasters: RTC scenes stacked per date warped onto every label's grid, on the device.

The reference builds chips from label rasters for HLS and Sentinel-2 (``instageo/data/raster_chip_creator.py``) and Sentinel-1 chips from
point tables only (``S1PointsPipeline``); flood extents, water masks and burn scars, what people train on radar, are dense label rasters.
This module fills that hole from its two parents: the scenes, the slice rule and the value rule of :mod:`instageo_amd.s1_chips`, the
destination grids, the label maps and the records of :mod:`instageo_amd.raster_chips`.  ``ig_s1_chip_warp`` (``s1_raster_chips.hip``)
projects each output pixel once and reads every scene on its own grid, in its own coordinate system.

The rule (stated in ``include/instageo_hip.h``).  T dates of C float32 bands; date t has n_t >= 1 scenes, 32 at most in all, each with a
coordinate system, a grid (X0, Y0, sx, sy), a size (H, W) and C planes, as :func:`s1_chips.cut` takes them.  The centre of every pixel of
a chip's S x S destination grid is mapped into every scene by the chain of the warp and read at ``floor``; band b of date t takes the
value of the first scene of the date, in list order, that the pixel lies inside and whose value is present (not NaN, not ``src_nodata``),
bits copied; without one it is ``no_data_value`` (-1).  ``clip`` bounds present values.  ``valid_values``, the validity plane and the
label maps are those of :func:`raster_chips.warp_cut`.

Device tensors go through ``ig_s1_chip_warp``; host arrays take a numpy twin of the same rule, so the module works (and is tested)
without a GPU and both write the same bytes.

Scenes in dB (``mode=filter_s1`` with ``scale=db``) hold -1.0 as a valid value: cut them with ``no_data_value=-9999``.

Not done: STAC search and signing, SAFE / GRD input and calibration, any resampling but nearest, rotated rasters.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import crs as crsmod
from . import prep, raster_chips, s1_chips, warp
from .chips import VALID_BITS
from .prep import STRATEGIES, is_device, to_host
from .raster_chips import MAX_CLASSES, MAX_SIDE
from .s1_chips import BANDS, NO_DATA_VALUE


# ---- argument checks shared by the host path and ops.s1_chip_warp ----------------------------------------------------------------------------
def check_warp(size: int, starts, scene_crs, scene_grid, scene_size, date_scenes, dst_crs, dst_grids, S: int, no_data_value, src_nodata, clip,
               labels_shape, labels_dtype, valid_bit: int, K: int):
    """ValueError unless the arguments of a warped S1 cut obey include/instageo_hip.h: the scenes and the value rule by
    :func:`s1_chips.check_scenes`, the destination and the labels by :func:`raster_chips.check_dst` -> (starts int64 (N * C,), scene_crs
    (N, 5) float64, scene_grid (N, 4) float64, scene_size (N, 2) int32, first_bits, T, C, dst_crs (5,), dst_grids (n, 4), no_data,
    src_nodata or None, clip (lo, hi) or None).  A destination grid may be unusable (it gives a no-data chip); a scene's grid may not."""
    st, sc, sg, ss, first_bits, T, C, nd, snd, clip = s1_chips.check_scenes(size, starts, scene_crs, scene_grid, scene_size, date_scenes, S,
                                                                            no_data_value, src_nodata, clip)
    dg = raster_chips.check_dst(dst_grids, int(S), T * C, labels_shape, labels_dtype, valid_bit, K)
    return st, sc, sg, ss, first_bits, T, C, raster_chips.params(dst_crs), dg, nd, snd, clip


# ---- the rule on host arrays ---------------------------------------------------------------------------------------------------------------
def _warp_host(planes, st, sc, sg, ss, first_bits, T, C, dc, dg, S, nd, snd, clip, labels, bit, K):
    """numpy twin of ``ig_s1_chip_warp``: every chip is the chip at the origin of its own grid by the twin of ``ig_s1_chip_cut`` (whose
    pixel centres are then those of ``ig_chip_warp``: 0 + c + 0.5 is c + 0.5), then the label step of :mod:`raster_chips`."""
    n = dg.shape[0]
    chips = np.empty((n, T * C, S, S), dtype=np.float32)
    valid_values = np.empty((n,), dtype=np.int32)
    validity = np.empty((n, S, S), dtype=np.uint8)
    origin = np.zeros((1, 2), dtype=np.int32)
    for i in range(n):
        chips[i], valid_values[i], validity[i] = (o[0] for o in s1_chips._cut_host(planes, st, sc, sg, ss, first_bits, T, C, dc, dg[i], origin,
                                                                                  S, nd, snd, clip))
    return (chips, valid_values, validity) + raster_chips.label_maps_host(labels, validity, bit, K)


def warp_cut(planes, starts, scene_crs, scene_grid, scene_size, date_scenes, dst_crs, dst_grids, chip_size: int,
             no_data_value: float = NO_DATA_VALUE, src_nodata: Optional[float] = None, clip: Optional[Tuple[float, float]] = None, labels=None,
             label_strategy: Optional[str] = None, num_classes: int = 0):
    """The packed planes ``planes`` (1-D float32) with ``starts``, ``scene_crs``, ``scene_grid``, ``scene_size`` and ``date_scenes`` as
    :func:`s1_chips.cut` takes them, resampled (nearest) onto the n grids ``dst_grids`` ((n, 4) = X0, Y0, sx, sy) of side ``chip_size`` in
    ``dst_crs`` by the rule of the module docstring -> (chips (n, T * C, S, S) float32, valid_values (n,) int32, validity (n, S, S) uint8,
    maps, valid_labels, hist).  A coordinate system is an EPSG code, a :class:`crs.Crs` or five doubles.  ``labels``: None, or (n, S, S)
    int8 (``seg``) | float32 (``reg``): ``maps`` are the labels with -1 where the validity bit of ``label_strategy`` (any | each | None: no
    masking) is clear and where a float label is NaN, ``valid_labels`` (n,) int32 the pixels != -1, ``hist`` (n, num_classes) int32 (int8
    only; None with 0 classes).  Without labels the last three are None.  A tensor on the device goes through ``ig_s1_chip_warp`` and gives
    device tensors; anything else takes the numpy twin and gives arrays."""
    if label_strategy not in VALID_BITS:
        raise ValueError(f"label_strategy must be any, each or None (got {label_strategy!r})")
    bit = VALID_BITS[label_strategy] if labels is not None else 0
    dev = is_device(planes)
    if not dev:
        planes = to_host(planes)
        labels = None if labels is None else np.ascontiguousarray(to_host(labels))
    if str(planes.dtype).replace("torch.", "") != "float32" or planes.ndim != 1:
        raise ValueError("the planes are one packed 1-D float32 buffer")
    if dev:
        from . import ops

        # checks the same arguments before the upload
        return ops.s1_chip_warp(planes, starts, scene_crs, scene_grid, scene_size, date_scenes, dst_crs, dst_grids, chip_size, no_data_value,
                                src_nodata, clip, labels, bit, int(num_classes))
    st, sc, sg, ss, first_bits, T, C, dc, dg, nd, snd, clip = check_warp(planes.shape[0], starts, scene_crs, scene_grid, scene_size, date_scenes,
                                                                         dst_crs, dst_grids, chip_size, no_data_value, src_nodata, clip,
                                                                         None if labels is None else tuple(labels.shape),
                                                                         None if labels is None else str(labels.dtype), bit, num_classes)
    return _warp_host(planes, st, sc, sg, ss, first_bits, T, C, dc, dg, int(chip_size), nd, snd, clip, labels, bit, int(num_classes))


# ---- files -> files -------------------------------------------------------------------------------------------------------------------------
def create_s1_raster_chips(scenes, records, raster_path: Optional[str], output_directory: str, chip_size: int = 256,
                           bands: Sequence[str] = BANDS, masking_strategy: str = "each", src_crs: int = 4326,
                           spatial_resolution: float = 0.0002694945852358564, qa_check: bool = True, task_type: str = "seg",
                           is_bbox_feature: bool = False, bbox_feature_path: Optional[str] = None, date: Optional[str] = None, snap: bool = True,
                           no_data_value: float = NO_DATA_VALUE, src_nodata: Optional[float] = None,
                           clip: Optional[Tuple[float, float]] = None, tile_id: Optional[str] = None,
                           device: Optional[str] = None) -> Tuple[List[str], List[Optional[str]]]:
    """The label-raster chip creator for one Sentinel-1 stack.  ``scenes``: as :func:`s1_chips.create_s1_chips` takes them, a list of
    dates, each a list of scenes (orbit slices, in the order they are tried), each a list of ``len(bands)`` single-band float32 GeoTIFF /
    COG files, every scene on its own grid and in its own coordinate system; a date that is one flat list of files is one scene.
    ``records``: a CSV path or a table with ``label_filename``, ``date`` and optionally ``mgrs_tile_id`` (default: ``tile_id``, or the id
    :func:`s1_chips.tile_id_of` reads from the first file's name; a record that names another id is left to that run); the label rasters
    lie under ``raster_path``, S x S pixels in EPSG:``src_crs`` (a raster whose GeoKeys name another system raises ValueError).  ``snap``
    selects the destination grid as in :func:`raster_chips.create_raster_chips`.

    Writes ``chips/chip_*_<id>.tif`` (float32, all dates and bands) and ``seg_maps/label_*_<id>.tif`` (int8 for ``seg``, float32 for
    ``reg``, NaN -> -1) with the names of :func:`raster_chips.chip_names`, both with the label raster's georeferencing.  A record whose
    files both exist is skipped and still listed; a label raster that is not S x S is skipped (``invalid_shape``); a record whose raster
    misses every scene is not cut (``outside_tile``); with ``qa_check`` a chip with ``valid_values == 0`` is dropped, then, after the
    label map was masked by the chip's validity (``masking_strategy``), a pair with ``valid_labels == 0``.  ``chips_dataset.csv`` gains
    the pairs and ``s1_raster_chips_stats.json`` holds the counts by reason, for ``seg`` with the class histogram and its
    ``compute_class_weights``.  -> (chip names, label-map names).

    ``is_bbox_feature``: no labels; the records are :func:`raster_chips.grid_polygons` of the JSON list of boxes in ``bbox_feature_path``
    (``date``: the date of the names, by default that of the first file's name); chips only, with the georeferencing of their destination
    grid; an existing chip is skipped and listed.  ``device``: None = the numpy path, ``"cuda"`` / ``"cuda:n"`` = the kernel; both write
    the same bytes."""
    S = int(chip_size)
    if masking_strategy not in STRATEGIES:
        raise ValueError(f"masking_strategy must be one of {tuple(STRATEGIES)} (got {masking_strategy!r})")
    if task_type not in ("seg", "reg"):
        raise ValueError(f"task_type must be seg or reg (got {task_type!r})")
    prep.check_device(device)
    if isinstance(bands, str) or not bands:
        raise ValueError(f"bands is a list of at least one name (got {bands!r})")
    res = float(spatial_resolution)
    if not 0 < res < np.inf:
        raise ValueError(f"spatial_resolution must be a positive number (got {spatial_resolution!r})")
    dst = crsmod.from_epsg(src_crs)
    C = len(bands)
    files, counts = s1_chips.scene_files(scenes, C)
    own_id = tile_id or s1_chips.tile_id_of(files[0])[0]
    planes, starts, scene_profiles = s1_chips.read_scenes(files, C)
    scene_crs = [crsmod.from_profile(p) for p, _ in scene_profiles]
    scene_grid = [warp.grid_of(p) for p, _ in scene_profiles]
    scene_size = [s for _, s in scene_profiles]
    bbox = bool(is_bbox_feature)
    if bbox:
        if not bbox_feature_path:
            raise ValueError("is_bbox_feature needs bbox_feature_path")
        rows = raster_chips.box_records(bbox_feature_path, date or s1_chips.tile_id_of(files[0])[1], S, res)
    else:
        if raster_path is None or records is None:
            raise ValueError("label records need records and raster_path")
        rows = raster_chips.read_records(records)
    histogram = not bbox and task_type == "seg"
    staged: List[Any] = []  # the packed planes where the cut runs, uploaded with the first batch

    def warp_cut_at(grids, labels):
        if not staged:
            staged.append(prep.to_device(planes, device))
        return warp_cut(staged[0], starts, scene_crs, scene_grid, scene_size, counts, dst, grids, S, no_data_value=no_data_value,
                        src_nodata=src_nodata, clip=clip, labels=labels, label_strategy=masking_strategy if qa_check else None,
                        num_classes=MAX_CLASSES if histogram else 0)

    def touches(grid):
        return any(raster_chips.touches(dst, grid, S, c, g, H, W) for c, g, (H, W) in zip(scene_crs, scene_grid, scene_size))

    labels_of = None if bbox else raster_chips.seg_labels if task_type == "seg" else lambda a, path: a.astype(np.float32)
    return raster_chips.create_from_records(rows, own_id, dst, touches, labels_of, warp_cut_at, len(counts) * C * S * S, np.float32, histogram,
                                            "s1_raster_chips_stats.json", output_directory, S, raster_path, res, snap, qa_check)


# ---- mode=create_s1_raster_chips -------------------------------------------------------------------------------------------------------------
CONFIG_KEYS = ("scenes", "records_file", "raster_path", "output_directory", "chip_size", "bands", "masking_strategy", "src_crs",
               "spatial_resolution", "qa_check", "task_type", "is_bbox_feature", "bbox_feature_path", "date", "snap", "no_data_value",
               "src_nodata", "clip", "tile_id")


def s1_raster_chips_options(cfg: Dict[str, Any]) -> Dict[str, Any]:
    """The ``s1_raster_chips.*`` keys of ``mode=create_s1_raster_chips`` checked -> the keyword arguments of
    :func:`create_s1_raster_chips`.  An unknown key or a bad value raises ValueError; the files are required only in that mode."""
    c = prep.Section(cfg, "s1_raster_chips", CONFIG_KEYS)
    size = c.integer("chip_size", 256, lo=1, hi=MAX_SIDE, what="must be an int in [1, 2^15]")
    bands = c.listing("bands", list(BANDS))
    if not bands:
        raise c.bad("bands", "must be a list of at least one name", bands)
    strategy = c.choice("masking_strategy", "each", STRATEGIES)
    task = c.choice("task_type", "seg", ("seg", "reg"), "must be seg or reg")
    src = c.epsg("src_crs", 4326)
    res = c.number("spatial_resolution", 0.0002694945852358564, lambda x: 0 < x < np.inf, "must be a positive number")
    nd, snd, clip = s1_chips.value_options(c)
    scenes = s1_chips.scenes_option(c, len(bands))
    bbox = c.flag("is_bbox_feature", False)
    opts = dict(scenes=scenes, records=c.text("records_file"), raster_path=c.text("raster_path"), output_directory=c.text("output_directory"),
                chip_size=size, bands=bands, masking_strategy=strategy, src_crs=src, spatial_resolution=res, qa_check=c.flag("qa_check", True),
                task_type=task, is_bbox_feature=bbox, bbox_feature_path=c.text("bbox_feature_path"), date=c.text("date"),
                snap=c.flag("snap", True), no_data_value=nd, src_nodata=snd, clip=clip, tile_id=c.text("tile_id"))
    if cfg.get("mode") == "create_s1_raster_chips":
        if not scenes or opts["output_directory"] is None:
            raise ValueError("mode=create_s1_raster_chips needs s1_raster_chips.scenes and s1_raster_chips.output_directory")
        if bbox and opts["bbox_feature_path"] is None:
            raise ValueError("s1_raster_chips.is_bbox_feature needs s1_raster_chips.bbox_feature_path")
        if not bbox and (opts["records"] is None or opts["raster_path"] is None):
            raise ValueError("mode=create_s1_raster_chips needs s1_raster_chips.records_file and s1_raster_chips.raster_path (or is_bbox_feature)")
    return opts


def run_from_config(cfg: Dict[str, Any], device: Optional[str] = None) -> int:
    """``mode=create_s1_raster_chips``: :func:`create_s1_raster_chips` under the ``s1_raster_chips.*`` keys; prints one JSON line with the
    counts."""
    return prep.run_creator("create_s1_raster_chips", create_s1_raster_chips, s1_raster_chips_options(cfg), device)


def main(argv: Optional[List[str]] = None) -> int:
    """``python -m instageo_amd.s1_raster_chips s1_raster_chips.scenes=[[[a_vv.tif,a_vh.tif]]] s1_raster_chips.output_directory=out ...``:
    mode=create_s1_raster_chips without ``run.py``."""
    return prep.run_mode_cli("create_s1_raster_chips", run_from_config, argv)


if __name__ == "__main__":
    raise SystemExit(main())
