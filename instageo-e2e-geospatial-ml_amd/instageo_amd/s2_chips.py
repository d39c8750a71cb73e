"""Chips and label maps cut from Sentinel-2 L2A tiles, on the device.

The reference's second data source (``instageo/data/s2_utils.py``: ``S2PointsPipeline``, ``create_mask_from_scl``,
``MASK_DECODING_POS["S2"]``) opens the six HLS-equivalent bands and the scene classification (SCL) through stackstac, which resamples
them onto one resolution, and then cuts chips as for HLS.  Here every plane stays on its own grid: B02 / B03 / B04 at 10 m, B8A / B11 / B12
and SCL at 20 m, anything at 60 m, packed into one buffer, and ``ig_s2_chip_cut`` (``s2_chips.hip``) reads each at its own resolution while it
cuts.  This module is the host layer on top of :mod:`instageo_amd.prep`, :mod:`instageo_amd.tiff`, :mod:`instageo_amd.crs` and the point
geometry and label maps of :mod:`instageo_amd.chips`.

The rule (stated in ``include/instageo_hip.h``).  T * C band planes, uint16, band b of date b // C, and T SCL planes, uint8; plane k is
H_k x W_k pixels of p_k metres (an integer) and all planes share the top-left corner with the output grid of p_o metres.  Output pixel
(r, c) reads source pixel ``((2 r + 1) p_o) // (2 p_k)``, ``((2 c + 1) p_o) // (2 p_k)``: nearest, in exact integers; outside the plane
the band value is 0 and the SCL class 0.  A value v != 0 loses ``boa_offset`` (never below 0); date t is masked at a pixel whose SCL class
is one of ``class_bits`` (``each``: the C bands of that date become ``no_data_value``; ``any``: all bands where any date is masked); with a
``valid_range`` a value outside it becomes ``no_data_value`` (replaced, not clipped).  With the chips come ``valid_values`` and the
validity plane of :func:`chips.cut`, which :func:`chips.label_maps` reads unchanged.

Device tensors go through ``ig_s2_chip_cut``; host arrays take a numpy twin of the same rule, so the module works (and is tested) without
a GPU and both write the same bytes.

Not done: JPEG 2000 / SAFE archives (there is no decoder here: the inputs are GeoTIFF / COG), STAC search and download, Sentinel-1, any
resampling but nearest, and per-band offsets read from product metadata (``boa_offset`` is one number for all bands).  The S2 label-raster
pipeline (``S2RasterPipeline``) is :mod:`instageo_amd.s2_raster_chips`.
"""
from __future__ import annotations

import os
import re
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import chips as chipmod
from . import crs as crsmod
from . import prep, warp
from .prep import MAX_DATES, STRATEGIES, is_device, to_host  # noqa: F401  (the masking strategies and the date limit of include/instageo_hip.h)

# the reference's MASK_DECODING_POS["S2"] (cloud: medium and high probability, water) and three more classes of the L2A scene classification
SCL_CLASSES = {"cloud": (8, 9), "water": (6,), "cloud_shadow": (3,), "cirrus": (10,), "snow": (11,)}
NO_DATA_VALUE = 0  # the reference's NO_DATA_VALUES.S2
MAX_PIXEL_SIZE = 1 << 15


def scl_class_bits(mask_types: Sequence[str], mask_classes: Sequence[int] = ()) -> int:
    """The OR of ``1 << class`` over the SCL classes of ``mask_types`` (names of ``SCL_CLASSES``) and the class numbers ``mask_classes``
    (0..31).  ValueError for an unknown name or a number outside 0..31."""
    if isinstance(mask_types, str):
        raise ValueError(f"mask_types is a list of names (got the string {mask_types!r})")
    bits = 0
    for m in mask_types:
        if m not in SCL_CLASSES:
            raise ValueError(f"unknown S2 mask type {m!r}: one of {sorted(SCL_CLASSES)}")
        for k in SCL_CLASSES[m]:
            bits |= 1 << k
    for k in mask_classes:
        if not prep.is_int(k) and not isinstance(k, np.integer) or not 0 <= int(k) <= 31:
            raise ValueError(f"mask_classes are SCL class numbers in 0..31 (got {k!r})")
        bits |= 1 << int(k)
    return bits


def source_index(n: int, po: int, pk: int, first: int = 0) -> np.ndarray:
    """The source pixel of output pixels first .. first + n - 1 along one axis: ``((2 x + 1) po) // (2 pk)`` in int64."""
    x = np.arange(first, first + n, dtype=np.int64)
    return ((2 * x + 1) * int(po)) // (2 * int(pk))


# ---- argument checks shared by the host path and the device wrapper (ops.s2_chip_cut) -------------------------------------------------------
def _check_planes(size: int, starts, geom, count: int, what: str) -> Tuple[np.ndarray, np.ndarray]:
    st = np.asarray(starts)
    g = np.asarray(geom)
    if st.size and st.dtype.kind not in "iu" or g.size and g.dtype.kind not in "iu":
        raise ValueError(f"the offsets and the geometry of the {what} planes must be integers")
    st, g = st.astype(np.int64).reshape(-1), g.astype(np.int64).reshape(-1, 3)
    if st.shape[0] != count or g.shape[0] != count:
        raise ValueError(f"{count} {what} planes need {count} offsets and {count} rows (H, W, pixel size) (got {st.shape[0]}, {g.shape[0]})")
    if (g[:, :2] < 1).any() or (g[:, 0] * g[:, 1] > 2**31 - 1).any():
        raise ValueError(f"a {what} plane has 1 <= H * W <= 2^31 - 1 pixels")
    if (g[:, 2] < 1).any() or (g[:, 2] > MAX_PIXEL_SIZE).any():
        raise ValueError(f"the pixel size of a {what} plane is an integer in [1, 2^15]")
    if size >= 2**40:
        raise ValueError(f"the packed {what} planes hold 2^40 elements or more")
    if (st < 0).any() or (st + g[:, 0] * g[:, 1] > size).any():
        raise ValueError(f"a {what} plane does not lie inside its packed buffer of {size} elements")
    return np.ascontiguousarray(st), np.ascontiguousarray(g, dtype=np.int32)


def check_cut(band_size: int, starts, geom, scl_size: Optional[int], scl_starts, scl_geom, origins, S: int, out_grid, T: int, class_bits: int,
              strategy: str, no_data_value: int, boa_offset: int, valid_range):
    """ValueError unless the arguments of a cut obey include/instageo_hip.h -> (starts int64, geom (T * C, 3) int32, scl_starts, scl_geom
    (None without SCL planes), origins (n, 2) int32)."""
    if isinstance(S, bool) or int(S) < 1:
        raise ValueError(f"chip_size must be an int >= 1 (got {S!r})")
    S = int(S)
    if len(tuple(out_grid)) != 3:
        raise ValueError(f"the output grid is (H_o, W_o, pixel size) (got {out_grid!r})")
    Ho, Wo, po = (int(v) for v in out_grid)
    if Ho < 1 or Wo < 1 or Ho * Wo > 2**31 - 1:
        raise ValueError(f"the output grid has 1 <= H_o * W_o <= 2^31 - 1 pixels (got {Ho} x {Wo})")
    if not 1 <= po <= MAX_PIXEL_SIZE:
        raise ValueError(f"the pixel size of the output grid is an integer in [1, 2^15] (got {po})")
    TC = int(np.asarray(starts).reshape(-1).shape[0])
    if isinstance(T, bool) or not 1 <= int(T) <= MAX_DATES or TC % int(T) or TC < 1:
        raise ValueError(f"{TC} bands do not divide into {T} dates (1 <= dates <= {MAX_DATES})")
    st, g = _check_planes(int(band_size), starts, geom, TC, "band")
    sst = sg = None
    if scl_size is not None:
        sst, sg = _check_planes(int(scl_size), scl_starts, scl_geom, int(T), "SCL")
    if TC * S * S > 2**31 - 1:
        raise ValueError(f"a chip of {TC} x {S} x {S} values is beyond 2^31 - 1 (valid_values is int32)")
    if isinstance(class_bits, bool) or not 0 <= int(class_bits) <= 2**32 - 1:
        raise ValueError(f"class_bits holds one bit per SCL class 0..31 (got {class_bits!r})")
    if strategy not in STRATEGIES:
        raise ValueError(f"masking_strategy must be one of {tuple(STRATEGIES)} (got {strategy!r})")
    if not 0 <= int(no_data_value) <= 65535:
        raise ValueError(f"no_data_value must fit uint16 (got {no_data_value!r})")
    if isinstance(boa_offset, bool) or not 0 <= int(boa_offset) <= 65535:
        raise ValueError(f"boa_offset must be an int in [0, 65535] (got {boa_offset!r})")
    if valid_range is not None and not (len(valid_range) == 2 and 0 <= int(valid_range[0]) <= int(valid_range[1]) <= 65535):
        raise ValueError(f"valid_range must be None or (lo, hi) inside uint16 with lo <= hi (got {valid_range!r})")
    if S > Ho or S > Wo:
        raise ValueError(f"a chip of side {S} does not fit an output grid of {Ho} x {Wo} pixels")
    o = prep.check_origins(origins, S, Ho, Wo, "output grid of")
    if o.shape[0] * TC * S * S >= 2**40:
        raise ValueError("the chips hold 2^40 values or more")
    return st, g, sst, sg, o


# ---- the rule on host arrays ---------------------------------------------------------------------------------------------------------------
def _window(buf: np.ndarray, start: int, H: int, W: int, pk: int, po: int, r0: int, c0: int, S: int) -> np.ndarray:
    """The S x S output window at (r0, c0) of one packed plane: its nearest source pixels, 0 outside the plane."""
    rs, cs = source_index(S, po, pk, r0), source_index(S, po, pk, c0)
    plane = buf[start : start + H * W].reshape(H, W)
    out = plane[np.minimum(rs, H - 1)[:, None], np.minimum(cs, W - 1)[None, :]]
    out[rs >= H, :] = 0
    out[:, cs >= W] = 0
    return out


def _cut_host(bands, st, g, scl, sst, sg, origins, S: int, po: int, T: int, bits: int, strategy: str, nd: int, boa: int, valid_range):
    """numpy twin of ``ig_s2_chip_cut``: chip by chip and plane by plane, vectorised over the pixels."""
    TC = g.shape[0]
    C = TC // T
    n = origins.shape[0]
    chips = np.empty((n, TC, S, S), dtype=np.uint16)
    validity = np.empty((n, S, S), dtype=np.uint8)
    table = np.array([(bits >> k) & 1 if k < 32 else 0 for k in range(256)], dtype=bool)
    for i, (r0, c0) in enumerate(origins.tolist()):
        a = np.stack([_window(bands, int(st[k]), int(g[k, 0]), int(g[k, 1]), int(g[k, 2]), po, r0, c0, S) for k in range(TC)]).astype(np.int32)
        if boa > 0:
            a = np.where(a != 0, np.maximum(a - boa, 0), a)
        if scl is not None and bits:
            m = np.stack([table[_window(scl, int(sst[t]), int(sg[t, 0]), int(sg[t, 1]), int(sg[t, 2]), po, r0, c0, S)] for t in range(T)])
            m = np.broadcast_to(m.any(axis=0), (TC, S, S)) if strategy == "any" else np.repeat(m, C, axis=0)
            a[m] = nd
        if valid_range is not None:
            a[(a < int(valid_range[0])) | (a > int(valid_range[1]))] = nd
        ok = a != nd
        chips[i] = a.astype(np.uint16)
        validity[i] = ok.all(axis=0).astype(np.uint8) | (ok.any(axis=0).astype(np.uint8) << 1)
    valid_values = (chips != np.uint16(nd)).reshape(n, -1).sum(axis=1).astype(np.int32)
    return chips, valid_values, validity


def _dtype_name(a) -> str:
    return str(a.dtype).replace("torch.", "")


def cut(bands, starts, geom, scl, scl_starts, scl_geom, origins, chip_size: int, out_grid, dates: Optional[int] = None, class_bits: int = 0,
        strategy: str = "each", no_data_value: int = NO_DATA_VALUE, boa_offset: int = 0, valid_range: Optional[Tuple[int, int]] = None):
    """Chips of side ``chip_size`` at ``origins`` ((n, 2): row0, col0 on the output grid ``out_grid`` = (H_o, W_o, pixel size)) from the
    packed planes ``bands`` (1-D uint16; plane k at ``starts[k]`` with ``geom[k]`` = (H, W, pixel size)) under the packed SCL planes
    ``scl`` (1-D uint8 with ``scl_starts`` / ``scl_geom``, or None) -> (chips (n, T * C, S, S) uint16, valid_values (n,) int32, validity
    (n, S, S) uint8) by the rule of the module docstring.  ``dates``: T, by default the number of SCL planes (1 without them);
    ``class_bits``: from :func:`scl_class_bits`; ``valid_range``: None or (lo, hi).  Tensors on the device go through ``ig_s2_chip_cut``
    and give device tensors; anything else takes the numpy twin and gives arrays."""
    T = int(dates) if dates is not None else (int(np.asarray(scl_starts).reshape(-1).shape[0]) if scl is not None else 1)
    dev = is_device(bands)
    if not dev:
        bands = to_host(bands)
        scl = None if scl is None else to_host(scl)
    if _dtype_name(bands) != "uint16" or (scl is not None and _dtype_name(scl) != "uint8") or bands.ndim != 1 or (scl is not None and scl.ndim != 1):
        raise ValueError("the band planes are one packed 1-D uint16 buffer and the SCL planes one packed 1-D uint8 buffer")
    if dev:
        from . import ops

        # checks the same arguments before the upload
        return ops.s2_chip_cut(bands, starts, geom, scl, scl_starts, scl_geom, origins, chip_size, out_grid, T, class_bits, strategy,
                               no_data_value, boa_offset, valid_range)
    st, g, sst, sg, o = check_cut(bands.shape[0], starts, geom, None if scl is None else scl.shape[0], scl_starts, scl_geom, origins, chip_size,
                                  out_grid, T, class_bits, strategy, no_data_value, boa_offset, valid_range)
    return _cut_host(bands, st, g, scl, sst, sg, o, int(chip_size), int(out_grid[2]), T, int(class_bits), strategy, int(no_data_value),
                     int(boa_offset), valid_range)


# ---- files -> files -------------------------------------------------------------------------------------------------------------------------
def tile_id_of(first_band_file: str, granule_id: Optional[str] = None) -> Tuple[str, str]:
    """The reference's S2 tile id ``{mission}_{level}_{tile}_{stamp}`` and the acquisition date YYYYMMDD: from ``granule_id``, a product name
    such as ``S2B_MSIL2A_20220525T072619_N0400_R049_T38PMB_20220525T101530``, else from a band file name
    ``T38PMB_20220525T072619_B02_10m.tif`` (mission ``S2``, level ``MSIL2A``)."""
    if granule_id:
        p = os.path.basename(str(granule_id).rstrip("/")).replace(".SAFE", "").split("_")
        if len(p) < 7 or not re.fullmatch(r"\d{8}T\d{6}", p[2]) or not p[5].startswith("T"):
            raise ValueError(f"{granule_id}: not a Sentinel-2 product name (<mission>_<level>_<stamp>_N<baseline>_R<orbit>_T<tile>_<stamp>)")
        return f"{p[0]}_{p[1]}_{p[5]}_{p[2]}", p[2][:8]
    p = os.path.splitext(os.path.basename(str(first_band_file)))[0].split("_")
    if len(p) < 3 or not p[0].startswith("T") or not re.fullmatch(r"\d{8}T\d{6}", p[1]):
        raise ValueError(f"{first_band_file}: not a Sentinel-2 band file name (T<tile>_<stamp>_<band>_<resolution>.tif); name the product "
                         "with granule_id")
    return f"S2_MSIL2A_{p[0]}_{p[1]}", p[1][:8]


def _plane_geometry(profiles, shapes, files, corner=None, system=None):
    """(H, W, pixel size) of every file, checked: a north-up grid with one integer pixel size, the corner and coordinate system of the
    first -> (geom (k, 3) int64, corner (X0, Y0), coordinate system)."""
    rows = []
    for prof, (H, W), f in zip(profiles, shapes, files):
        X0, Y0, sx, sy = warp.grid_of(prof, str(f))
        if sx != sy or sx != round(sx) or not 1 <= sx <= MAX_PIXEL_SIZE:
            raise ValueError(f"{f}: the pixel size must be one integer number of metres in [1, 2^15] (got {sx} x {sy})")
        here = crsmod.from_profile(prof)
        if corner is None:
            corner, system = (X0, Y0), here
        if (X0, Y0) != corner:
            raise ValueError(f"{f}: its top-left corner {(X0, Y0)} is not the shared corner {corner} of the planes")
        if tuple(here)[:5] != tuple(system)[:5]:
            raise ValueError(f"{f}: its coordinate system differs from that of {files[0]}")
        rows.append((H, W, int(sx)))
    return np.array(rows, dtype=np.int64).reshape(-1, 3), corner, system


def create_s2_chips(band_files: Sequence[str], scl_files: Optional[Sequence[str]], points, output_directory: str, chip_size: int = 256,
                    mask_types: Sequence[str] = (), mask_classes: Sequence[int] = (), masking_strategy: str = "each", window_size: int = 0,
                    task_type: str = "seg", src_crs: int = 4326, spatial_resolution: Optional[int] = None, boa_offset: int = 0,
                    valid_range: Optional[Tuple[int, int]] = None, granule_id: Optional[str] = None, num_classes: Optional[int] = None,
                    device: Optional[str] = None, date: Optional[str] = None) -> Tuple[List[str], List[Optional[str]]]:
    """The reference's ``S2PointsPipeline`` for one Sentinel-2 tile.  ``band_files``: single-band GeoTIFF / COG files ordered per date and
    band, each on its own grid (the pixel size comes from its own tags) with one shared top-left corner; one SCL file per date in
    ``scl_files`` (read only when ``mask_types`` / ``mask_classes`` ask for masks); ``points``: a CSV path or a table with ``x``, ``y`` (in
    EPSG:``src_crs``), ``label``, ``date``.  The output grid starts at the shared corner with pixels of ``spatial_resolution`` metres (None:
    the first band file's) and covers the first band file's extent.  Writes ``chips/chip_{date}_{tile_id}_{x}_{y}.tif`` (uint16, all
    bands, no-data 0) and ``seg_maps/seg_map_{...}.tif`` (int16 for ``seg``, float32 for ``reg``) for every chip a point nominates, each
    with its own tiepoint, the output pixel size and the tile's GeoKey tags.  The label maps are masked by ``masking_strategy`` (``any``:
    where any value of the pixel is no-data, ``each``: where all are), as the reference passes it to ``mask_segmentation_map``.  Drop
    rules, ``chips_dataset.csv`` and ``chips_stats.json`` are those of :func:`chips.create_chips`.  ``points=None``: every complete chip of
    the grid that has a valid value, no label maps; ``date``: the YYYYMMDD of the names then, by default from the tile id.  ``device``:
    None = the numpy path, ``"cuda"`` / ``"cuda:n"`` = the kernels; both write the same bytes.  -> (chip names, label-map names)."""
    S = int(chip_size)
    bits = scl_class_bits(mask_types, mask_classes)
    if masking_strategy not in STRATEGIES:
        raise ValueError(f"masking_strategy must be one of {tuple(STRATEGIES)} (got {masking_strategy!r})")
    if task_type not in ("seg", "reg"):
        raise ValueError(f"task_type must be seg or reg (got {task_type!r})")
    prep.check_device(device)
    if not band_files:
        raise ValueError("create_s2_chips needs at least one band file")
    if bits and not scl_files:
        raise ValueError("mask_types / mask_classes need scl_files")
    use_mask = bool(bits) and bool(scl_files)
    T = len(scl_files) if scl_files else 1
    if len(band_files) % T:
        raise ValueError(f"{len(band_files)} band files do not divide into {T} dates")
    tile_id, stamp_date = tile_id_of(band_files[0], granule_id)
    bands, starts, shapes, profiles = prep.read_planes(band_files, "band", np.uint16)
    geom, corner, system = _plane_geometry(profiles, shapes, band_files)
    scl = scl_starts = scl_geom = None
    if use_mask:
        scl, scl_starts, scl_shapes, scl_profiles = prep.read_planes(scl_files, "SCL", np.uint8)
        scl_geom = _plane_geometry(scl_profiles, scl_shapes, scl_files, corner, system)[0]
    po = int(geom[0, 2]) if spatial_resolution is None else spatial_resolution
    if isinstance(po, bool) or not isinstance(po, (int, np.integer)) or not 1 <= po <= MAX_PIXEL_SIZE:
        raise ValueError(f"spatial_resolution must be an integer number of metres in [1, 2^15] (got {spatial_resolution!r})")
    po = int(po)
    H, W = int(geom[0, 0] * geom[0, 2]) // po, int(geom[0, 1] * geom[0, 2]) // po  # the first band file's extent in output pixels
    grid = (corner[0], corner[1], float(po), float(po))
    tags = dict(profiles[0]["tags"])
    tags[33550] = (12, (float(po), float(po), 0.0))
    profile = {"tags": tags, "nodata": None}  # the output grid as a raster profile
    def cut_at(origins, bbox):
        b_dev, s_dev = prep.stage(bands, scl, device)
        return cut(b_dev, starts, geom, s_dev, scl_starts, scl_geom, origins, S, (H, W, po), dates=T, class_bits=bits, strategy=masking_strategy,
                   no_data_value=NO_DATA_VALUE, boa_offset=boa_offset, valid_range=valid_range)

    source = chipmod.PointSource(profile, grid, (H, W), tile_id, stamp_date, "tile", cut_at, None)
    return chipmod.create_from_points(source, points, output_directory, S, window_size, task_type, src_crs, masking_strategy, num_classes, date)


# ---- mode=create_s2_chips ------------------------------------------------------------------------------------------------------------------
CONFIG_KEYS = ("chip_size", "mask_types", "mask_classes", "masking_strategy", "window_size", "task_type", "src_crs", "spatial_resolution",
               "boa_offset", "valid_range", "tiles", "scl", "granule_id", "records_file", "output_directory")


def s2_chips_options(cfg: Dict[str, Any]) -> Dict[str, Any]:
    """The ``s2_chips.*`` keys of ``mode=create_s2_chips`` checked -> the keyword arguments of :func:`create_s2_chips`.  A bad value raises
    ValueError; ``tiles`` and ``output_directory`` are required only in that mode."""
    c = prep.Section(cfg, "s2_chips", CONFIG_KEYS)
    size = c.integer("chip_size", 256, lo=1, what="must be an int >= 1")
    w = c.integer("window_size", 0, lo=0, hi=chipmod.MAX_WINDOW, what="must be an int >= 0")
    types = c.listing("mask_types", []) or []
    classes = c.get("mask_classes", []) or []
    if not isinstance(classes, (list, tuple)):
        raise c.bad("mask_classes", "must be a list of SCL class numbers in 0..31", classes)
    try:
        scl_class_bits([], classes)
    except ValueError:
        raise c.bad("mask_classes", "must be a list of SCL class numbers in 0..31", classes) from None
    scl_class_bits(types)
    strategy = c.choice("masking_strategy", "each", STRATEGIES)
    task = c.choice("task_type", "seg", ("seg", "reg"), "must be seg or reg")
    src = c.epsg("src_crs", 4326)
    res = c.integer("spatial_resolution", None, lo=1, hi=MAX_PIXEL_SIZE, what="must be an integer number of metres in [1, 2^15]", optional=True)
    boa = c.integer("boa_offset", 0, lo=0, hi=65535, what="must be an int in [0, 65535]")
    rng = c.get("valid_range")
    if rng is not None:
        if not isinstance(rng, (list, tuple)) or len(rng) != 2 or not all(prep.is_int(v) for v in rng) or not 0 <= rng[0] <= rng[1] <= 65535:
            raise c.bad("valid_range", "must be None or [lo, hi] inside uint16 with lo <= hi", rng)
        rng = (int(rng[0]), int(rng[1]))
    tiles, scl = c.listing("tiles"), c.listing("scl")
    granule, records, out = c.text("granule_id"), c.text("records_file"), c.text("output_directory")
    if cfg.get("mode") == "create_s2_chips":
        if not tiles or out is None:
            raise ValueError("mode=create_s2_chips needs s2_chips.tiles and s2_chips.output_directory")
        if (types or classes) and not scl:
            raise ValueError("s2_chips.mask_types / s2_chips.mask_classes need s2_chips.scl (one SCL file per date)")
    return dict(band_files=tiles, scl_files=scl, points=records, output_directory=out, chip_size=size, mask_types=types,
                mask_classes=[int(k) for k in classes], masking_strategy=strategy, window_size=w, task_type=task, src_crs=src,
                spatial_resolution=res, boa_offset=boa, valid_range=rng, granule_id=granule)


def run_from_config(cfg: Dict[str, Any], device: Optional[str] = None) -> int:
    """``mode=create_s2_chips``: :func:`create_s2_chips` under the ``s2_chips.*`` keys; prints one JSON line with the counts."""
    return prep.run_creator("create_s2_chips", create_s2_chips, s2_chips_options(cfg), device)


def main(argv: Optional[List[str]] = None) -> int:
    """``python -m instageo_amd.s2_chips s2_chips.tiles=a.tif,b.tif s2_chips.output_directory=out ...``: mode=create_s2_chips without
    ``run.py``."""
    return prep.run_mode_cli("create_s2_chips", run_from_config, argv)


if __name__ == "__main__":
    raise SystemExit(main())
