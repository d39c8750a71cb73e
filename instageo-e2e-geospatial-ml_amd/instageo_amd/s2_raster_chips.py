"""Sentinel-2 chips cut against label rasters: band planes of several resolutions warped onto every label's grid, on the device
(DESIGN.md 3.28).

The reference's ``instageo/data/raster_chip_creator.py`` builds chips from label rasters through two pipelines: ``HLSRasterPipeline``
(:mod:`instageo_amd.raster_chips`) and ``S2RasterPipeline`` (``instageo/data/s2_utils.py``), its default.  The latter opens the bands and
the scene classification (SCL) through stackstac, which resamples all of them onto the label's coordinate system and resolution on the
host, then masks by SCL class, replaces values outside [0, 10000] by 0 and quality-checks against the label.  Here every plane stays on
its own grid (10 m, 20 m, 60 m; any corner) and ``ig_s2_chip_warp`` (``s2_raster_chips.hip``) projects each output pixel once and reads
every plane at its own resolution.  This module is the host layer on :mod:`instageo_amd.prep`, built from its two parents:
the float64 chain and the records of :mod:`instageo_amd.raster_chips`, the planes and the value chain of :mod:`instageo_amd.s2_chips`.

The rule (stated in ``include/instageo_hip.h``).  T * C band planes, uint16, and T SCL planes, uint8, packed as :func:`s2_chips.cut`
takes them, all in one coordinate system; every plane belongs to one of G <= 8 geometry classes (a grid (X0, Y0, sx, sy) and a size
(H, W)).  The centre of every pixel of a chip's S x S destination grid is mapped to source map coordinates once, by the chain of the warp;
per class, ``cs = floor((x - X0) / sx)``, ``rs = floor((Y0 - y) / sy)``; inside the plane the pixel reads (rs, cs) of every plane of the
class, outside it takes ``no_data_value`` in the class's bands and SCL class 0.  A value that was read goes through the chain of
:func:`s2_chips.cut` (``boa_offset``, the SCL date mask ``each`` / ``any``, replacement outside ``valid_range``).  ``valid_values``, the
validity plane and the label maps are those of :func:`raster_chips.warp_cut`.

Device tensors go through ``ig_s2_chip_warp``; host arrays take a numpy twin of the same rule, so the module works (and is tested)
without a GPU and both write the same bytes.

Not done: JPEG 2000 / SAFE archives (there is no decoder here: the inputs are GeoTIFF / COG), STAC search and download, Sentinel-1, any
resampling but nearest, per-band offsets read from product metadata (``boa_offset`` is one number for all bands), rotated rasters, and
float (``reg``) label maps in the files-to-files mode (the reference's S2 pipeline writes int8).
"""
from __future__ import annotations

import os
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import crs as crsmod
from . import prep, raster_chips, s2_chips, warp
from .chips import VALID_BITS
from .prep import MAX_DATES, STRATEGIES, is_device, to_host  # noqa: F401
from .raster_chips import MAX_CLASSES, MAX_SIDE, SEG_NO_DATA
from .s2_chips import NO_DATA_VALUE

MAX_GEOMETRIES = 8  # geometry classes of one launch (include/instageo_hip.h)


# ---- argument checks shared by the host path and ops.s2_chip_warp ----------------------------------------------------------------------------
def check_warp(band_size: int, starts, plane_class, class_grid, class_size, scl_size: Optional[int], scl_starts, src_crs, dst_crs, dst_grids,
               S: int, T: int, class_bits: int, strategy: str, no_data_value: int, boa_offset: int, valid_range, labels_shape, labels_dtype,
               valid_bit: int, K: int):
    """ValueError unless the arguments of a warped S2 cut obey include/instageo_hip.h -> (starts int64, scl_starts int64 or None,
    plane_class int32, class_grid (G, 4) float64, class_size (G, 2) int32, src_crs (5,), dst_crs (5,), dst_grids (n, 4)).  A destination
    grid may be unusable (it gives a no-data chip); a class grid may not."""
    if isinstance(S, bool) or not isinstance(S, (int, np.integer)) or not 1 <= int(S) <= MAX_SIDE:
        raise ValueError(f"chip_size must be an int in [1, 2^15] (got {S!r})")
    S = int(S)
    st = np.asarray(starts)
    if st.size and st.dtype.kind not in "iu":
        raise ValueError("the offsets of the band planes must be integers")
    st = np.ascontiguousarray(st.astype(np.int64).reshape(-1))
    TC = int(st.shape[0])
    if isinstance(T, bool) or not 1 <= int(T) <= MAX_DATES or TC % int(T) or TC < 1:
        raise ValueError(f"{TC} bands do not divide into {T} dates (1 <= dates <= {MAX_DATES})")
    T = int(T)
    sst = None
    if scl_size is not None:
        sst = np.asarray(scl_starts)
        if sst.size and sst.dtype.kind not in "iu":
            raise ValueError("the offsets of the SCL planes must be integers")
        sst = np.ascontiguousarray(sst.astype(np.int64).reshape(-1))
        if sst.shape[0] != T:
            raise ValueError(f"{T} dates need {T} SCL planes (got {sst.shape[0]} offsets)")
    cg = np.ascontiguousarray(class_grid, dtype=np.float64)
    cs = np.asarray(class_size)
    if cg.size % 4 or cs.size % 2 or cs.size and cs.dtype.kind not in "iu":
        raise ValueError("class_grid is (G, 4) = (X0, Y0, sx, sy) and class_size (G, 2) = (H, W) integers per geometry class")
    cg, cs = cg.reshape(-1, 4), cs.astype(np.int64).reshape(-1, 2)
    G = cg.shape[0]
    if not 1 <= G <= MAX_GEOMETRIES or cs.shape[0] != G:
        raise ValueError(f"1 <= G <= {MAX_GEOMETRIES} geometry classes, one grid and one size each (got {G} grids, {cs.shape[0]} sizes)")
    if not all(raster_chips.grid_ok(g) for g in cg):
        raise ValueError("a class grid = (X0, Y0, sx, sy) needs finite values and positive pixel sizes")
    if (cs < 1).any() or (cs[:, 0] * cs[:, 1] > 2**31 - 1).any():
        raise ValueError("a geometry class has 1 <= H * W <= 2^31 - 1 pixels (source offsets are int32)")
    pc = np.asarray(plane_class)
    if pc.size and pc.dtype.kind not in "iu":
        raise ValueError("plane_class must be integers")
    pc = pc.astype(np.int64).reshape(-1)
    planes = TC + (T if sst is not None else 0)
    if pc.shape[0] != planes:
        raise ValueError(f"plane_class has one entry per band plane and then one per SCL plane: {planes} (got {pc.shape[0]})")
    if pc.size and (pc.min() < 0 or pc.max() >= G):
        raise ValueError(f"plane_class must lie in [0, G) = [0, {G})")
    area = cs[:, 0] * cs[:, 1]
    for what, size, s, cls in (("band", int(band_size), st, pc[:TC]), ("SCL", scl_size, sst, pc[TC:])):
        if s is None:
            continue
        if int(size) >= 2**40:
            raise ValueError(f"the packed {what} planes hold 2^40 elements or more")
        if (s < 0).any() or (s + area[cls] > int(size)).any():
            raise ValueError(f"a {what} plane does not lie inside its packed buffer of {size} elements")
    if TC * S * S > 2**31 - 1:
        raise ValueError(f"a chip of {TC} x {S} x {S} values is beyond 2^31 - 1 (valid_values is int32)")
    if isinstance(class_bits, bool) or not 0 <= int(class_bits) <= 2**32 - 1:
        raise ValueError(f"class_bits holds one bit per SCL class 0..31 (got {class_bits!r})")
    if strategy not in STRATEGIES:
        raise ValueError(f"masking_strategy must be one of {tuple(STRATEGIES)} (got {strategy!r})")
    if isinstance(no_data_value, bool) or not 0 <= int(no_data_value) <= 65535:
        raise ValueError(f"no_data_value must fit uint16 (got {no_data_value!r})")
    if isinstance(boa_offset, bool) or not 0 <= int(boa_offset) <= 65535:
        raise ValueError(f"boa_offset must be an int in [0, 65535] (got {boa_offset!r})")
    if valid_range is not None and not (len(valid_range) == 2 and 0 <= int(valid_range[0]) <= int(valid_range[1]) <= 65535):
        raise ValueError(f"valid_range must be None or (lo, hi) inside uint16 with lo <= hi (got {valid_range!r})")
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
    return (st, sst, np.ascontiguousarray(pc, dtype=np.int32), cg, np.ascontiguousarray(cs, dtype=np.int32), raster_chips.params(src_crs),
            raster_chips.params(dst_crs), dg)


# ---- the rule on host arrays ---------------------------------------------------------------------------------------------------------------
def _warp_host(bands, st, scl, sst, pc, cg, cs, sc, dc, dg, S, T, bits, strategy, nd, boa, valid_range, labels, bit, K):
    """numpy twin of ``ig_s2_chip_warp``: chip by chip and class by class, vectorised over the pixels."""
    TC = st.shape[0]
    C = TC // T
    n = dg.shape[0]
    chips = np.empty((n, TC, S, S), dtype=np.uint16)
    validity = np.empty((n, S, S), dtype=np.uint8)
    table = np.array([(bits >> k) & 1 if k < 32 else 0 for k in range(256)], dtype=bool)
    for i in range(n):
        a = np.full((TC, S, S), nd, dtype=np.int32)
        read = np.zeros((TC, S, S), dtype=bool)
        f = np.zeros((T, S, S), dtype=np.uint8)
        if raster_chips.grid_ok(dg[i]):
            X0, Y0, sx, sy = (float(v) for v in dg[i])
            x = X0 + (np.arange(S, dtype=np.float64) + 0.5) * sx
            y = Y0 - (np.arange(S, dtype=np.float64) + 0.5) * sy
            xs, ys = crsmod.transform(dc, sc, *np.meshgrid(x, y))
            for g in range(cg.shape[0]):
                H, W = int(cs[g, 0]), int(cs[g, 1])
                with np.errstate(invalid="ignore"):
                    fc, fr = np.floor((xs - cg[g, 0]) / cg[g, 2]), np.floor((cg[g, 1] - ys) / cg[g, 3])
                    inside = (fc >= 0) & (fc < W) & (fr >= 0) & (fr < H)
                at = fr[inside].astype(np.int64) * W + fc[inside].astype(np.int64)
                for b in np.nonzero(pc[:TC] == g)[0]:
                    a[b, inside] = bands[int(st[b]) : int(st[b]) + H * W][at]
                    read[b] = inside
                if scl is not None:
                    for t in np.nonzero(pc[TC:] == g)[0]:
                        f[t, inside] = scl[int(sst[t]) : int(sst[t]) + H * W][at]
        if boa > 0:
            a = np.where(read & (a != 0), np.maximum(a - boa, 0), a)
        if scl is not None and bits:
            m = table[f]
            m = np.broadcast_to(m.any(axis=0), (TC, S, S)) if strategy == "any" else np.repeat(m, C, axis=0)
            a[m] = nd
        if valid_range is not None:
            a[read & ((a < int(valid_range[0])) | (a > int(valid_range[1])))] = nd
        ok = a != nd
        chips[i] = a.astype(np.uint16)
        validity[i] = ok.all(axis=0).astype(np.uint8) | (ok.any(axis=0).astype(np.uint8) << 1)
    valid_values = (chips != np.uint16(nd)).reshape(n, TC * S * S).sum(axis=1).astype(np.int32)
    return (chips, valid_values, validity) + raster_chips.label_maps_host(labels, validity, bit, K)


def _dtype_name(a) -> str:
    return str(a.dtype).replace("torch.", "")


def warp_cut(bands, starts, plane_class, class_grid, class_size, scl, scl_starts, src_crs, dst_crs, dst_grids, chip_size: int,
             dates: Optional[int] = None, class_bits: int = 0, strategy: str = "each", no_data_value: int = NO_DATA_VALUE, boa_offset: int = 0,
             valid_range: Optional[Tuple[int, int]] = None, labels=None, valid_bit: int = 0, classes: int = 0):
    """The packed planes ``bands`` (1-D uint16; plane k at ``starts[k]``) under the packed SCL planes ``scl`` (1-D uint8 with
    ``scl_starts``, or None), all in ``src_crs``; plane k (the bands, then the SCL planes) has the grid ``class_grid[plane_class[k]]`` =
    (X0, Y0, sx, sy) and the size ``class_size[plane_class[k]]`` = (H, W).  Resampled (nearest) onto the n grids ``dst_grids`` ((n, 4)) of
    side ``chip_size`` in ``dst_crs`` by the rule of the module docstring -> (chips (n, T * C, S, S) uint16, valid_values (n,) int32,
    validity (n, S, S) uint8, maps, valid_labels, hist).  A coordinate system is an EPSG code, a :class:`crs.Crs` or five doubles.
    ``dates``: T, by default the number of SCL planes (1 without them); ``class_bits``: from :func:`s2_chips.scl_class_bits`;
    ``valid_range``: None or (lo, hi).  ``labels``: None, or (n, S, S) int8 | float32: ``maps`` are the labels with -1 where the validity
    bit ``valid_bit`` (1 any, 2 each, 0: no masking) is clear and where a float label is NaN, ``valid_labels`` (n,) int32 the pixels
    != -1, ``hist`` (n, classes) int32 (int8 only; None with 0 classes); without labels the last three are None.  Tensors on the device go
    through ``ig_s2_chip_warp`` and give device tensors; anything else takes the numpy twin and gives arrays."""
    T = int(dates) if dates is not None else (int(np.asarray(scl_starts).reshape(-1).shape[0]) if scl is not None else 1)
    bit = int(valid_bit) if labels is not None else 0
    dev = is_device(bands)
    if not dev:
        bands = to_host(bands)
        scl = None if scl is None else to_host(scl)
        labels = None if labels is None else np.ascontiguousarray(to_host(labels))
    if _dtype_name(bands) != "uint16" or (scl is not None and _dtype_name(scl) != "uint8") or bands.ndim != 1 or (scl is not None and scl.ndim != 1):
        raise ValueError("the band planes are one packed 1-D uint16 buffer and the SCL planes one packed 1-D uint8 buffer")
    if dev:
        from . import ops

        # checks the same arguments before the upload
        return ops.s2_chip_warp(bands, starts, plane_class, class_grid, class_size, scl, scl_starts, src_crs, dst_crs, dst_grids, chip_size, T,
                                class_bits, strategy, no_data_value, boa_offset, valid_range, labels, bit, int(classes))
    st, sst, pc, cg, cs, sc, dc, dg = check_warp(bands.shape[0], starts, plane_class, class_grid, class_size, None if scl is None else scl.shape[0],
                                                 scl_starts, src_crs, dst_crs, dst_grids, chip_size, T, class_bits, strategy, no_data_value,
                                                 boa_offset, valid_range, None if labels is None else tuple(labels.shape),
                                                 None if labels is None else _dtype_name(labels), bit, classes)
    return _warp_host(bands, st, scl, sst, pc, cg, cs, sc, dc, dg, int(chip_size), T, int(class_bits), strategy, int(no_data_value),
                      int(boa_offset), valid_range, labels, bit, int(classes))


# ---- files -> files -------------------------------------------------------------------------------------------------------------------------
def geometry_classes(profiles, shapes, files, system=None, known=None):
    """The planes ``files`` grouped by equal grid and size -> (class index per plane, [(grid, (H, W))], coordinate system).  ``known``: the
    classes found so far (extended in place order), ``system``: the coordinate system every file must have (None: the first file's)."""
    classes: List[Tuple[Tuple[float, float, float, float], Tuple[int, int]]] = list(known or [])
    index = []
    for prof, shape, f in zip(profiles, shapes, files):
        here = crsmod.from_profile(prof)
        if system is None:
            system = here
        if tuple(here)[:5] != tuple(system)[:5]:
            raise ValueError(f"{f}: its coordinate system differs from that of {files[0]}")
        key = (tuple(float(v) for v in warp.grid_of(prof, str(f))), (int(shape[0]), int(shape[1])))
        if key not in classes:
            classes.append(key)
        index.append(classes.index(key))
    if len(classes) > MAX_GEOMETRIES:
        raise ValueError(f"the planes have {len(classes)} different grids; at most {MAX_GEOMETRIES} geometry classes are supported")
    return index, classes, system


def create_s2_raster_chips(band_files: Sequence[str], scl_files: Optional[Sequence[str]], records, raster_path: Optional[str],
                           output_directory: str, chip_size: int = 256, mask_types: Sequence[str] = (), mask_classes: Sequence[int] = (),
                           masking_strategy: str = "each", src_crs: int = 4326, spatial_resolution: float = 0.0002694945852358564,
                           snap: bool = True, qa_check: bool = True, is_bbox_feature: bool = False, boa_offset: int = 0,
                           valid_range: Optional[Tuple[int, int]] = (0, 10000), granule_id: Optional[str] = None,
                           device: Optional[str] = None) -> Tuple[List[str], List[Optional[str]]]:
    """The reference's ``S2RasterPipeline.process_row`` for every record that touches one Sentinel-2 granule.  ``band_files``: single-band
    GeoTIFF / COG files ordered per date and band, each on its own grid (read from its own tags; 10 m, 20 m, 60 m, any corner) in one
    coordinate system; one SCL file per date in ``scl_files`` (read only when ``mask_types`` / ``mask_classes`` ask for masks).
    ``records``: a CSV path or a table with ``label_filename``, ``date`` and optionally ``mgrs_tile_id`` (default: the tile of the
    granule, :func:`s2_chips.tile_id_of`; a record that names another tile is left to that tile's run); the label rasters lie under
    ``raster_path``, S x S pixels in EPSG:``src_crs`` (a raster whose GeoKeys name another system raises ValueError).  ``snap`` selects
    the destination grid as in :func:`raster_chips.create_raster_chips`.

    Writes ``chips/chip_*_<mgrs>.tif`` (uint16, all bands, values outside ``valid_range`` replaced by 0) and
    ``seg_maps/label_*_<mgrs>.tif`` (int8, NaN -> -1) with the names of :func:`raster_chips.chip_names`, both with the label raster's
    georeferencing.  A record whose files both exist is skipped and still listed; a label raster that is not S x S is skipped
    (``invalid_shape``); a record whose raster misses every plane is not cut (``outside_tile``); with ``qa_check`` a chip with
    ``valid_values == 0`` is dropped, then, after the label map was masked by the chip's validity (``masking_strategy``), a pair with
    ``valid_labels == 0``.  ``chips_dataset.csv`` gains the pairs and ``s2_raster_chips_stats.json`` holds the counts by reason, the class
    histogram and its ``compute_class_weights``.  -> (chip names, label-map names).

    ``is_bbox_feature``: no labels; ``records`` is the path of a JSON list of boxes [x_min, y_min, x_max, y_max] in EPSG:``src_crs`` and the
    records are their :func:`raster_chips.grid_polygons` under the granule's date; chips only, with the georeferencing of their
    destination grid; an existing chip is skipped and listed.  ``device``: None = the numpy path, ``"cuda"`` / ``"cuda:n"`` = the kernel;
    both write the same bytes."""
    S = int(chip_size)
    bits = s2_chips.scl_class_bits(mask_types, mask_classes)
    if masking_strategy not in STRATEGIES:
        raise ValueError(f"masking_strategy must be one of {tuple(STRATEGIES)} (got {masking_strategy!r})")
    prep.check_device(device)
    if not band_files:
        raise ValueError("create_s2_raster_chips needs at least one band file")
    if bits and not scl_files:
        raise ValueError("mask_types / mask_classes need scl_files")
    res = float(spatial_resolution)
    if not 0 < res < np.inf:
        raise ValueError(f"spatial_resolution must be a positive number (got {spatial_resolution!r})")
    dst = crsmod.from_epsg(src_crs)
    use_mask = bool(bits) and bool(scl_files)
    T = len(scl_files) if scl_files else 1
    if len(band_files) % T:
        raise ValueError(f"{len(band_files)} band files do not divide into {T} dates")
    tile_id, stamp_date = s2_chips.tile_id_of(band_files[0], granule_id)
    own_id = tile_id.split("_")[2]
    bands, starts, shapes, profiles = prep.read_planes(band_files, "band", np.uint16)
    plane_class, classes, src = geometry_classes(profiles, shapes, band_files)
    scl = scl_starts = None
    if use_mask:
        scl, scl_starts, scl_shapes, scl_profiles = prep.read_planes(scl_files, "SCL", np.uint8)
        scl_class, classes, _ = geometry_classes(scl_profiles, scl_shapes, scl_files, src, classes)
        plane_class = plane_class + scl_class
    class_grid = np.array([g for g, _ in classes], dtype=np.float64).reshape(-1, 4)
    class_size = np.array([s for _, s in classes], dtype=np.int32).reshape(-1, 2)
    bbox = bool(is_bbox_feature)
    if bbox:
        if not records or not isinstance(records, (str, os.PathLike)):
            raise ValueError("is_bbox_feature needs records: the path of a JSON list of boxes")
        rows = raster_chips.box_records(records, stamp_date, S, res)
    else:
        if raster_path is None or records is None:
            raise ValueError("label records need records and raster_path")
        rows = raster_chips.read_records(records)
    staged: List[Any] = []  # the packed planes where the cut runs, uploaded with the first batch

    def warp_cut_at(grids, labels):
        if not staged:
            staged.extend(prep.stage(bands, scl, device))
        return warp_cut(staged[0], starts, plane_class, class_grid, class_size, staged[1], scl_starts, src, dst, grids, S, dates=T, class_bits=bits,
                        strategy=masking_strategy, no_data_value=NO_DATA_VALUE, boa_offset=boa_offset, valid_range=valid_range, labels=labels,
                        valid_bit=VALID_BITS[masking_strategy] if qa_check and not bbox else 0, classes=0 if bbox else MAX_CLASSES)

    def touches(grid):
        return any(raster_chips.touches(dst, grid, S, src, g, H, W) for g, (H, W) in classes)

    return raster_chips.create_from_records(rows, own_id, dst, touches, None if bbox else raster_chips.seg_labels, warp_cut_at, len(band_files) * S * S,
                                            np.uint16, not bbox, "s2_raster_chips_stats.json", output_directory, S, raster_path, res, snap, qa_check)


# ---- mode=create_s2_raster_chips -------------------------------------------------------------------------------------------------------------
CONFIG_KEYS = ("tiles", "scl", "records_file", "raster_path", "output_directory", "chip_size", "mask_types", "mask_classes", "masking_strategy",
               "src_crs", "spatial_resolution", "snap", "qa_check", "is_bbox_feature", "boa_offset", "valid_range", "granule_id")


def s2_raster_chips_options(cfg: Dict[str, Any]) -> Dict[str, Any]:
    """The ``s2_raster_chips.*`` keys of ``mode=create_s2_raster_chips`` checked -> the keyword arguments of
    :func:`create_s2_raster_chips`.  An unknown key or a bad value raises ValueError; the files are required only in that mode."""
    c = prep.Section(cfg, "s2_raster_chips", CONFIG_KEYS)
    size = c.integer("chip_size", 256, lo=1, hi=MAX_SIDE, what="must be an int in [1, 2^15]")
    types = c.listing("mask_types", []) or []
    classes = c.get("mask_classes", []) or []
    if not isinstance(classes, (list, tuple)):
        raise c.bad("mask_classes", "must be a list of SCL class numbers in 0..31", classes)
    try:
        s2_chips.scl_class_bits([], classes)
    except ValueError:
        raise c.bad("mask_classes", "must be a list of SCL class numbers in 0..31", classes) from None
    s2_chips.scl_class_bits(types)
    strategy = c.choice("masking_strategy", "each", STRATEGIES)
    src = c.epsg("src_crs", 4326)
    res = c.number("spatial_resolution", 0.0002694945852358564, lambda x: 0 < x < np.inf, "must be a positive number")
    boa = c.integer("boa_offset", 0, lo=0, hi=65535, what="must be an int in [0, 65535]")
    rng = c.get("valid_range", [0, 10000])
    if rng is not None:
        if not isinstance(rng, (list, tuple)) or len(rng) != 2 or not all(prep.is_int(v) for v in rng) or not 0 <= rng[0] <= rng[1] <= 65535:
            raise c.bad("valid_range", "must be None or [lo, hi] inside uint16 with lo <= hi", rng)
        rng = (int(rng[0]), int(rng[1]))
    tiles, scl = c.listing("tiles"), c.listing("scl")
    bbox = c.flag("is_bbox_feature", False)
    opts = dict(band_files=tiles, scl_files=scl, records=c.text("records_file"), raster_path=c.text("raster_path"),
                output_directory=c.text("output_directory"), chip_size=size, mask_types=types, mask_classes=[int(k) for k in classes],
                masking_strategy=strategy, src_crs=src, spatial_resolution=res, snap=c.flag("snap", True), qa_check=c.flag("qa_check", True),
                is_bbox_feature=bbox, boa_offset=boa, valid_range=rng, granule_id=c.text("granule_id"))
    if cfg.get("mode") == "create_s2_raster_chips":
        if not tiles or opts["output_directory"] is None:
            raise ValueError("mode=create_s2_raster_chips needs s2_raster_chips.tiles and s2_raster_chips.output_directory")
        if (types or classes) and not scl:
            raise ValueError("s2_raster_chips.mask_types / s2_raster_chips.mask_classes need s2_raster_chips.scl (one SCL file per date)")
        if opts["records"] is None:
            raise ValueError("mode=create_s2_raster_chips needs s2_raster_chips.records_file (with is_bbox_feature: the JSON list of boxes)")
        if not bbox and opts["raster_path"] is None:
            raise ValueError("mode=create_s2_raster_chips needs s2_raster_chips.raster_path (or is_bbox_feature)")
    return opts


def run_from_config(cfg: Dict[str, Any], device: Optional[str] = None) -> int:
    """``mode=create_s2_raster_chips``: :func:`create_s2_raster_chips` under the ``s2_raster_chips.*`` keys; prints one JSON line with the
    counts."""
    return prep.run_creator("create_s2_raster_chips", create_s2_raster_chips, s2_raster_chips_options(cfg), device)


def main(argv: Optional[List[str]] = None) -> int:
    """``python -m instageo_amd.s2_raster_chips s2_raster_chips.tiles=a.tif,b.tif s2_raster_chips.output_directory=out ...``:
    mode=create_s2_raster_chips without ``run.py``."""
    return prep.run_mode_cli("create_s2_raster_chips", run_from_config, argv)


if __name__ == "__main__":
    raise SystemExit(main())
