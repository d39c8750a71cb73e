"""The host layer shared by the dataset-preparation modes: what :mod:`instageo_amd.chips`, :mod:`instageo_amd.raster_chips`,
:mod:`instageo_amd.s2_chips`, :mod:`instageo_amd.s2_raster_chips`, :mod:`instageo_amd.s1_chips`, :mod:`instageo_amd.clean` and
:mod:`instageo_amd.polygon_labels` have in common around their kernels, each defined once.  A leaf module: it imports only
:mod:`instageo_amd.tiff` and :mod:`instageo_amd.crs` at module level (``torch``, ``pandas`` and the config loader inside the functions that
need them), so every mode, and :mod:`mosaic` / :mod:`cog` / :mod:`maptiles` / :mod:`warp`, can import it without a cycle.

Here belongs what is the same for every files-in / files-out mode: telling device tensors from host arrays and moving between them, HLS
file names, reading a band stack or packed planes, the dataset CSV, the georeferencing tags a written chip keeps, the class statistics and
``*_stats.json``, the checks common to the cut entry points (the stack arguments, the origins), the reader of one config section, the
tail of a chip creator's ``run_from_config`` and the command-line entry.  A mode's rule, its numpy twin and its own checks stay in its
module.  The two pipelines the chip creators share sit on top of this layer, each in the module of its first mode:
:func:`chips.create_from_points` (the point modes: HLS, Sentinel-2, Sentinel-1) and :func:`raster_chips.create_from_records` (the
label-raster modes: HLS, Sentinel-2); a mode keeps its argument checks and its reading and makes one call of its driver.
"""
from __future__ import annotations

import datetime
import json
import os
from typing import Any, Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import crs as crsmod
from . import tiff

STRATEGIES = {"each": 0, "any": 1}  # masking strategies of a cut (include/instageo_hip.h)
MAX_DATES = 32
# The georeferencing a written chip takes from the raster it was cut against: pixel scale, GeoKey directory, GeoKey doubles and ASCII.
# The model transformation (34264: rotated rasters are not supported) and GDAL's metadata / no-data tags (42112, 42113: they describe
# the source's samples, not the chip's) are left behind.  The tiepoint (33922) goes with ``tiepoint=True`` of :func:`geo_tags` only.
CHIP_GEO_TAGS = (33550, 34735, 34736, 34737)
TIEPOINT = 33922


# ---- arrays and tensors --------------------------------------------------------------------------------------------------------------------
def is_device(a) -> bool:
    """Whether ``a`` is a tensor on the device (anything else, a host tensor included, takes a numpy path)."""
    return type(a).__module__.startswith("torch") and bool(getattr(a, "is_cuda", False))


def to_host(a) -> np.ndarray:
    """A tensor (device or host) or an array -> a numpy array."""
    return np.asarray(a.cpu() if hasattr(a, "cpu") else a)


def to_device(a: np.ndarray, device):
    """``a`` as a tensor on ``device``; with ``device=None`` (the numpy path) ``a`` itself."""
    if device is None:
        return a
    import torch

    return torch.from_numpy(a).to(device)


def check_device(device) -> None:
    if device is not None and not str(device).startswith("cuda"):
        raise ValueError(f"device must be None (host) or a cuda device (got {device!r})")


def stage(tile: np.ndarray, fmask: Optional[np.ndarray], device):
    """The band stack and its Fmask (or None) where the cut runs: uploaded once when a device is named."""
    return to_device(tile, device), None if fmask is None else to_device(fmask, device)


def default_device() -> Optional[str]:
    """``"cuda"`` when there is a device, else None (the numpy path); also None without torch."""
    try:
        import torch

        return "cuda" if torch.cuda.is_available() else None
    except ImportError:
        return None


# ---- HLS file names ------------------------------------------------------------------------------------------------------------------------
class HlsName(NamedTuple):
    sensor: str  # S30 | L30
    tile: str  # the MGRS tile with its leading T
    stamp: str  # YYYYDDDTHHMMSS


def hls_name(path: str) -> HlsName:
    """Fields 1..3 of an HLS file name (``HLS.S30.T38PMB.2022145T072619.v2.0.B02.tif``)."""
    parts = os.path.basename(str(path)).split(".")
    if len(parts) < 4:
        raise ValueError(f"{path}: not an HLS file name (HLS.<sensor>.<tile>.<date>...)")
    return HlsName(parts[1], parts[2], parts[3])


def hls_date(path: str) -> str:
    """The acquisition date of an HLS file name as YYYYMMDD (its stamp counts the day of the year)."""
    return datetime.datetime.strptime(hls_name(path).stamp[:7], "%Y%j").strftime("%Y%m%d")


# ---- files ---------------------------------------------------------------------------------------------------------------------------------
def read_stack(files: Sequence[str], what: str, dtype) -> Tuple[np.ndarray, Dict[str, Any]]:
    """The rasters ``files`` (one size) stacked along the band axis as ``dtype`` -> (stack, the first file's profile).  ValueError for a
    file of another size, or samples ``dtype`` cannot hold (``what`` names them: tile | Fmask)."""
    planes, first = [], None
    for f in files:
        a, prof = tiff.read(str(f))
        if first is None:
            first = prof
        if a.shape[1:] != planes[0].shape[1:] if planes else False:
            raise ValueError(f"{f}: {a.shape[1]} x {a.shape[2]} pixels, {files[0]} has {planes[0].shape[1]} x {planes[0].shape[2]}")
        if a.dtype != dtype:
            if a.dtype.kind not in "iu" or a.size and (a.min() < np.iinfo(dtype).min or a.max() > np.iinfo(dtype).max):
                raise ValueError(f"{f}: {what} samples must fit {np.dtype(dtype).name} (got {a.dtype.name})")
            a = a.astype(dtype)
        planes.append(a)
    return np.ascontiguousarray(np.concatenate(planes, axis=0)), first


def read_planes(files: Sequence[str], what: str, dtype) -> Tuple[np.ndarray, np.ndarray, List[Tuple[int, int]], List[Dict[str, Any]]]:
    """The single-band rasters ``files``, whose sizes may differ, packed row-major into one 1-D buffer of ``dtype`` -> (buffer, starts: the
    int64 element offset of every plane, [(H, W)], the files' profiles).  ValueError for a file with more than one band, or samples
    ``dtype`` cannot hold (``what`` names them)."""
    planes, shapes, profiles = [], [], []
    for f in files:
        a, prof = tiff.read(str(f))
        if a.shape[0] != 1:
            raise ValueError(f"{f}: {what} files hold one band each (got {a.shape[0]})")
        if a.dtype != dtype:
            if a.dtype.kind not in "iu" or a.size and (a.min() < np.iinfo(dtype).min or a.max() > np.iinfo(dtype).max):
                raise ValueError(f"{f}: {what} samples must fit {np.dtype(dtype).name} (got {a.dtype.name})")
            a = a.astype(dtype)
        planes.append(a.reshape(-1))
        shapes.append((int(a.shape[1]), int(a.shape[2])))
        profiles.append(prof)
    starts = np.concatenate([[0], np.cumsum([p.size for p in planes])[:-1]]).astype(np.int64) if planes else np.zeros(0, dtype=np.int64)
    buf = np.ascontiguousarray(np.concatenate(planes)) if planes else np.zeros(0, dtype=dtype)
    return buf, starts, shapes, profiles


def write_dataset_csv(output_directory: str, chips: List[str], segs: List[Optional[str]], bbox: bool) -> str:
    """``chips_dataset.csv``: the rows already there plus the new pairs (``Input`` [, ``Label``], paths relative to the folder)."""
    import csv

    path = os.path.join(output_directory, "chips_dataset.csv")
    header = ["Input"] if bbox else ["Input", "Label"]
    rows: List[List[str]] = []
    if os.path.exists(path):
        with open(path, newline="") as f:
            old = list(csv.reader(f))
        if old and old[0] == header:
            rows = old[1:]
    for c, s in zip(chips, segs):
        row = [f"chips/{c}"] if bbox else [f"chips/{c}", f"seg_maps/{s}"]
        if row not in rows:
            rows.append(row)
    with open(path, "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(header)
        wr.writerows(rows)
    return path


def geo_tags(tags: Dict[int, Any], tiepoint: bool) -> Dict[int, Any]:
    """The tags of ``CHIP_GEO_TAGS`` among ``tags``.  ``tiepoint=False``: without the source's tiepoint, for a chip cut out of a tile, which
    writes its own; ``tiepoint=True``: with it, for a chip warped onto a label raster, which keeps the label's."""
    keep = CHIP_GEO_TAGS + ((TIEPOINT,) if tiepoint else ())
    return {k: v for k, v in tags.items() if k in keep}


def class_stats(hist, trim: bool = False) -> Dict[str, Any]:
    """A summed class histogram -> the ``class_histogram`` / ``class_weights`` (``compute_class_weights`` of the classes present) entries
    of a stats file.  ``trim``: without the cells after the last class present (at least one cell stays)."""
    from .pipeline_utils import compute_class_weights

    hist = np.asarray(hist)
    if trim:
        hist = hist[: int(np.nonzero(hist)[0].max()) + 1 if hist.any() else 1]
    cells = [int(v) for v in hist.tolist()]
    present = {c: v for c, v in enumerate(cells) if v}
    return {"class_histogram": cells, "class_weights": compute_class_weights(present) if present else []}


def write_stats(path: str, stats: Dict[str, Any]) -> None:
    """A mode's ``*_stats.json``: one line, keys sorted."""
    with open(path, "w") as f:
        json.dump(stats, f, sort_keys=True)


# ---- argument checks shared by chips.check_cut and raster_chips.check_warp -------------------------------------------------------------------
def check_stack_args(tile_shape, fmask_shape, S: int, T: int, bits: int, strategy: str, no_data_value: int, clip) -> Tuple[int, int, int]:
    """ValueError unless a stack, its Fmask and the masking arguments of a cut of side ``S`` obey include/instageo_hip.h -> (T * C, H, W)."""
    if len(tile_shape) != 3:
        raise ValueError(f"a tile is (T * C, H, W) (got shape {tuple(tile_shape)})")
    TC, H, W = (int(v) for v in tile_shape)
    if not 1 <= T <= MAX_DATES or TC % T or TC < 1:
        raise ValueError(f"{TC} bands do not divide into {T} dates (1 <= dates <= {MAX_DATES})")
    if fmask_shape is not None and tuple(fmask_shape) != (T, H, W):
        raise ValueError(f"fmask must be (T, H, W) = {(T, H, W)} (got {tuple(fmask_shape)})")
    if TC * S * S > 2**31 - 1:
        raise ValueError(f"a chip of {TC} x {S} x {S} values is beyond 2^31 - 1 (valid_values is int32)")
    if not 0 <= int(bits) <= 255:
        raise ValueError(f"mask_bits must be a byte (got {bits!r})")
    if strategy not in STRATEGIES:
        raise ValueError(f"masking_strategy must be one of {tuple(STRATEGIES)} (got {strategy!r})")
    if not -32768 <= int(no_data_value) <= 32767:
        raise ValueError(f"no_data_value must fit int16 (got {no_data_value!r})")
    if clip is not None and not (len(clip) == 2 and -32768 <= int(clip[0]) <= int(clip[1]) <= 32767):
        raise ValueError(f"clip must be None or (lo, hi) inside int16 with lo <= hi (got {clip!r})")
    return TC, H, W


def check_origins(origins, S: int, H: int, W: int, what: str) -> np.ndarray:
    """ValueError unless ``origins`` are integers and every chip of side ``S`` at one of them lies wholly inside the ``H`` x ``W`` pixels of
    ``what`` (``tile of`` | ``output grid of``) -> origins as an (n, 2) int32 array."""
    o = np.asarray(origins)
    if o.size and o.dtype.kind not in "iu":
        raise ValueError("origins must be integers")
    o = o.astype(np.int64).reshape(-1, 2)
    if o.size and (o.min() < 0 or (o[:, 0] > H - S).any() or (o[:, 1] > W - S).any()):
        raise ValueError(f"a chip of side {S} at one of the origins does not lie wholly inside the {what} {H} x {W} pixels")
    return np.ascontiguousarray(o, dtype=np.int32)


# ---- one config section ----------------------------------------------------------------------------------------------------------------------
def none(v, also: Tuple[str, ...] = ()):
    """``v``, or None where it is unset: None, the string ``"None"`` (what an override ``key=None`` gives) or one of ``also``."""
    return None if v in (None, "None") + also else v


def is_int(v) -> bool:
    """An int that is not a bool (``True`` is an int to ``isinstance``)."""
    return isinstance(v, int) and not isinstance(v, bool)


class Section:
    """The keys of one section of the config (``cfg[name]``), read and checked.  An unknown key raises ValueError on construction; a bad
    value raises ``ValueError("<section>.<key> <what> (got <value>)")`` from the member that reads it."""

    def __init__(self, cfg: Dict[str, Any], name: str, keys: Sequence[str]):
        self.name, self.c = name, dict(cfg.get(name) or {})
        unknown = set(self.c) - set(keys)
        if unknown:
            raise ValueError(f"unknown {name} keys {sorted(unknown)}")

    def bad(self, key: str, what: str, v) -> ValueError:
        return ValueError(f"{self.name}.{key} {what} (got {v!r})")

    def get(self, key: str, default=None):
        """The raw value, None where it is unset."""
        return none(self.c.get(key, default))

    def text(self, key: str) -> Optional[str]:
        v = self.get(key)
        return None if v is None else str(v)

    def flag(self, key: str, default: bool = False) -> bool:
        v = self.c.get(key, default)
        if not isinstance(v, bool):
            raise self.bad(key, "must be true or false", v)
        return v

    def integer(self, key: str, default, lo: Optional[int] = None, hi: Optional[int] = None, what: str = "must be an int",
                span: Optional[str] = None, optional: bool = False) -> Optional[int]:
        """An int in [lo, hi] (either may be None).  ``what``: the message of a value that is no int, and of one out of range unless
        ``span`` words that; ``optional``: unset gives None."""
        v = self.get(key, default) if optional else self.c.get(key, default)
        if v is None and optional:
            return None
        if not is_int(v):
            raise self.bad(key, what, v)
        if (lo is not None and v < lo) or (hi is not None and v > hi):
            raise self.bad(key, span or what, v)
        return v

    def number(self, key: str, default, ok: Callable[[float], bool], what: str) -> float:
        v = self.c.get(key, default)
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not ok(float(v)):
            raise self.bad(key, what, v)
        return float(v)

    def listing(self, key: str, default=None) -> Optional[List[str]]:
        """A list of names, or one string of them separated by commas; unset gives None."""
        v = self.c.get(key, default)
        if v is None or v == "None":
            return None
        if isinstance(v, str):
            v = [s for s in v.split(",") if s]
        if not isinstance(v, (list, tuple)) or not all(isinstance(s, str) for s in v):
            raise self.bad(key, "must be a list of names", v)
        return list(v)

    def epsg(self, key: str, default: Optional[int]) -> Optional[int]:
        """An EPSG code :mod:`crs` knows; with ``default=None`` unset gives None."""
        v = self.c.get(key, default)
        if default is None and none(v) is None:
            return None
        if not is_int(v):
            raise self.bad(key, "must be an EPSG code", v)
        crsmod.from_epsg(v)
        return v

    def choice(self, key: str, default, allowed, what: Optional[str] = None):
        v = self.c.get(key, default)
        if v not in allowed:
            raise self.bad(key, what or f"must be one of {tuple(allowed)}", v)
        return v


# ---- the entry points of a mode --------------------------------------------------------------------------------------------------------------
def run_creator(mode: str, create: Callable[..., Tuple[List[str], List[Optional[str]]]], kw: Dict[str, Any], device: Optional[str]) -> int:
    """The tail of a chip-creation mode's ``run_from_config``: ``create(device=device, **kw)`` -> (chip names, label-map names), then one
    JSON line with the counts under ``mode``."""
    chips, segs = create(device=device, **kw)
    print(json.dumps({mode: {"chips": len(chips), "seg_maps": sum(s is not None for s in segs), "output_directory": kw["output_directory"]}}))
    return 0


def run_mode_cli(mode: str, run_from_config: Callable[[Dict[str, Any], Optional[str]], int], argv: Optional[List[str]] = None) -> int:
    """``python -m instageo_amd.<module> key=value ...``: ``mode`` without ``run.py``, on the device when there is one."""
    import sys

    from .config import load_config

    cfg = load_config("config", [f"mode={mode}"] + list(sys.argv[1:] if argv is None else argv))
    return run_from_config(cfg, default_device())
