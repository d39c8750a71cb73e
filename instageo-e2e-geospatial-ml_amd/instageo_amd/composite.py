"""Cloud-free temporal composites of HLS scenes, on the device.

Every chip creator takes one scene per temporal step, as the reference does (``instageo/data/hls_utils.py``: ``add_hls_stac_items`` picks
the single least cloudy granule near a step's date); what Fmask flags in that scene is lost.  HLS revisits a tile every two or three days,
so the clear pixels are in the neighbouring scenes: this module turns the N scenes of one MGRS tile, grouped into T temporal steps, into
one composite "scene" per step, written under HLS-style file names so that ``chips.tiles`` and ``raster_chips.tiles`` take it unchanged
with ``fmasks=None``.  It is the host layer on top of :mod:`instageo_amd.prep`, :mod:`instageo_amd.tiff` and ``ig_composite``
(``composite.hip``).

The rule (stated in ``include/instageo_hip.h``).  All scenes share one grid.  A candidate of a step is CLEAR at a pixel when
``fmask & mask_bits == 0`` (the bit positions of :func:`chips.mask_bits`; a fill of 255 is masked by any bits) and none of its C values
equals ``no_data``.  ``count`` is the number of clear candidates; a pixel with ``count < min_clear`` gets ``no_data`` and source 255.
``nearest``: the first clear candidate in list order (the host orders candidates by |acquisition date - target date|, the earlier date
on a tie).  ``median``: per band the lower median of the clear values, the ``(count - 1) // 2``-th smallest.  ``medoid``: the clear
candidate with the smallest sum over the bands of |value - median|, the earliest in list order on a tie: an observed spectrum.

Device tensors go through ``ig_composite``; host arrays take a numpy twin of the same rule, so the module works (and is tested) without a
GPU and both write the same bytes.

Not done: max-NDVI and geometric-median rules, per-band clear tests, a synthesised Fmask for the composite, Sentinel-2 / Sentinel-1
inputs, scenes on different grids, and the STAC search that finds the candidates.
"""
from __future__ import annotations

import datetime
import json
import os
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import chips as chipmod
from . import prep, tiff
from .prep import MAX_DATES, is_device, to_host

METHODS = {"nearest": 0, "median": 1, "medoid": 2}  # include/instageo_hip.h
MAX_CANDIDATES = 16  # of one step
CELLS = MAX_CANDIDATES + 1  # of the count histogram
NO_DATA_VALUE = -9999  # HLS's fill
MASK_TYPES = ("cloud", "near_cloud_or_shadow", "cloud_shadow")
GRID_TAGS = (prep.TIEPOINT,) + prep.CHIP_GEO_TAGS  # what all scenes of a composite must share
_CHUNK = 1 << 18  # pixels the host path works on at a time


# ---- argument checks shared by the host path and the device wrapper (ops.composite) ----------------------------------------------------------
def check_composite(size: int, starts, fmask_size: Optional[int], fmask_starts, step_ptr, C: int, shape, bits: int, no_data_value: int,
                    min_clear: int, method: str):
    """ValueError unless the arguments of a composite obey include/instageo_hip.h -> (starts int64 (N * C,), fmask_starts int64 (N,) or
    None, step_ptr int32 (T + 1,), T, N, max_m, H, W)."""
    if not prep.is_int(C) and not isinstance(C, np.integer) or not 1 <= int(C) <= 32767:
        raise ValueError(f"a scene has 1 <= C <= 32767 bands (got {C!r})")
    C = int(C)
    if len(tuple(shape)) != 2 or min(int(v) for v in shape) < 0 or int(shape[0]) * int(shape[1]) > 2**31 - 1:
        raise ValueError(f"the grid is (H, W) with H * W <= 2^31 - 1 (got {shape!r})")
    H, W = int(shape[0]), int(shape[1])
    ptr = np.asarray(step_ptr)
    if ptr.ndim != 1 or ptr.size < 1 or ptr.dtype.kind not in "iu":
        raise ValueError(f"step_ptr holds T + 1 ascending integers from 0 (got {step_ptr!r})")
    ptr = ptr.astype(np.int64)
    T = ptr.shape[0] - 1
    if T > MAX_DATES:
        raise ValueError(f"{T} steps: at most {MAX_DATES} go into one composite")
    if ptr[0] != 0 or (np.diff(ptr) < 0).any():
        raise ValueError(f"step_ptr holds T + 1 ascending integers from 0 (got {ptr.tolist()})")
    N = int(ptr[-1])
    max_m = int(np.diff(ptr).max()) if T else 0
    if max_m > MAX_CANDIDATES:
        raise ValueError(f"a step has {max_m} candidates: at most {MAX_CANDIDATES}")
    st = np.asarray(starts)
    if st.size and st.dtype.kind not in "iu":
        raise ValueError("the offsets of the planes must be integers")
    st = np.ascontiguousarray(st.astype(np.int64).reshape(-1))
    if st.shape[0] != N * C:
        raise ValueError(f"{st.shape[0]} band planes do not go with {N} scenes of {C} bands")
    if int(size) >= 2**40:
        raise ValueError("the packed planes hold 2^40 elements or more")
    if (st < 0).any() or (st + H * W > int(size)).any():
        raise ValueError(f"a band plane does not lie inside the packed buffer of {size} elements")
    fst = None
    if fmask_size is not None:
        fst = np.asarray(fmask_starts)
        if fst.size and fst.dtype.kind not in "iu":
            raise ValueError("the offsets of the Fmask planes must be integers")
        fst = np.ascontiguousarray(fst.astype(np.int64).reshape(-1))
        if fst.shape[0] != N:
            raise ValueError(f"{fst.shape[0]} Fmask planes do not go with {N} scenes")
        if (fst < 0).any() or (fst + H * W > int(fmask_size)).any():
            raise ValueError(f"an Fmask plane does not lie inside the packed buffer of {fmask_size} elements")
    elif fmask_starts is not None:
        raise ValueError("fmask_starts goes with an Fmask buffer")
    if isinstance(bits, bool) or not 0 <= int(bits) <= 255:
        raise ValueError(f"mask_bits must be a byte (got {bits!r})")
    if isinstance(no_data_value, bool) or not -32768 <= int(no_data_value) <= 32767:
        raise ValueError(f"no_data must fit int16 (got {no_data_value!r})")
    if isinstance(min_clear, bool) or not isinstance(min_clear, (int, np.integer)) or not 1 <= int(min_clear) <= MAX_CANDIDATES:
        raise ValueError(f"min_clear must be an int in [1, {MAX_CANDIDATES}] (got {min_clear!r})")
    if method not in METHODS:
        raise ValueError(f"method must be one of {tuple(METHODS)} (got {method!r})")
    if T * C * H * W >= 2**40:
        raise ValueError(f"{T} composites of {C} x {H} x {W} values are beyond 2^40")
    return st, fst, np.ascontiguousarray(ptr, dtype=np.int32), T, N, max_m, H, W


# ---- the rule on host arrays ---------------------------------------------------------------------------------------------------------------
def _composite_host(bands, st, fmasks, fst, ptr, C, H, W, bits, nd, min_clear, method):
    """numpy twin of ``ig_composite``: step by step, vectorised over chunks of pixels."""
    T, HW = ptr.shape[0] - 1, H * W
    comp = np.full((T, C, HW), nd, dtype=np.int16)
    count = np.zeros((T, HW), dtype=np.uint8)
    source = np.full((T, HW), 255, dtype=np.uint8)
    hist = np.zeros((T, CELLS), dtype=np.int32)
    for t in range(T):
        cand = range(int(ptr[t]), int(ptr[t + 1]))
        m = len(cand)
        for p0 in range(0, HW if m else 0, _CHUNK):
            p1 = min(p0 + _CHUNK, HW)
            v = np.stack([np.stack([bands[st[n * C + c] + p0 : st[n * C + c] + p1] for c in range(C)]) for n in cand])  # (m, C, P)
            clear = (v != np.int16(nd)).all(axis=1)
            if fmasks is not None and bits:
                clear &= np.stack([(fmasks[fst[n] + p0 : fst[n] + p1] & np.uint8(bits)) == 0 for n in cand])
            cnt = clear.sum(axis=0)
            live = cnt >= min_clear
            count[t, p0:p1] = cnt
            win = None
            if method == "nearest":
                win = np.argmax(clear, axis=0)
            else:
                keys = np.where(clear[:, None, :], v.astype(np.int32), np.int32(1 << 15))
                keys.sort(axis=0)
                k = np.maximum(cnt.astype(np.int64) - 1, 0) >> 1
                med = np.take_along_axis(keys, np.broadcast_to(k[None, None, :], (1, C, p1 - p0)), axis=0)[0]  # (C, P)
                if method == "median":
                    comp[t, :, p0:p1] = np.where(live[None, :], med, nd).astype(np.int16)
                else:
                    dist = np.abs(v.astype(np.int32) - med[None]).sum(axis=1, dtype=np.int64)
                    dist[~clear] = np.iinfo(np.int64).max
                    win = np.argmin(dist, axis=0)  # the first of the smallest
            if win is not None:
                got = np.take_along_axis(v, np.broadcast_to(win[None, None, :], (1, C, p1 - p0)), axis=0)[0]
                comp[t, :, p0:p1] = np.where(live[None, :], got, np.int16(nd))
                source[t, p0:p1] = np.where(live, win, 255).astype(np.uint8)
        hist[t] = np.bincount(count[t], minlength=CELLS)
    return comp.reshape(T, C, H, W), count.reshape(T, H, W), source.reshape(T, H, W), hist


def composite(bands, starts, fmasks, fmask_starts, step_ptr, bands_per_scene: int, shape: Tuple[int, int], mask: Union[int, Sequence[str]] = MASK_TYPES,
              no_data_value: int = NO_DATA_VALUE, min_clear: int = 1, method: str = "medoid"):
    """The composites of T steps from the packed planes ``bands`` (1-D int16; band c of scene n at element ``starts[n * C + c]``,
    C = ``bands_per_scene``) and ``fmasks`` (1-D uint8, scene n at ``fmask_starts[n]``; None: only ``no_data_value`` decides what is
    clear), every plane ``shape`` = (H, W).  ``step_ptr``: T + 1 ascending integers, the candidates of step t are the scenes
    ``step_ptr[t] .. step_ptr[t + 1] - 1`` in list order.  ``mask``: the bits, or a list of mask types for :func:`chips.mask_bits`.
    -> (composite (T, C, H, W) int16, count (T, H, W) uint8, source (T, H, W) uint8, hist (T, 17) int32) by the rule of the module
    docstring.  A tensor on the device goes through ``ig_composite`` and gives device tensors; anything else takes the numpy twin and
    gives arrays."""
    bits = mask if isinstance(mask, (int, np.integer)) and not isinstance(mask, bool) else chipmod.mask_bits(mask)
    dev = is_device(bands)
    if not dev:
        bands = to_host(bands)
        fmasks = None if fmasks is None else to_host(fmasks)
    if str(bands.dtype).replace("torch.", "") != "int16" or bands.ndim != 1:
        raise ValueError("the band planes are one packed 1-D int16 buffer")
    if fmasks is not None and (str(fmasks.dtype).replace("torch.", "") != "uint8" or fmasks.ndim != 1):
        raise ValueError("the Fmask planes are one packed 1-D uint8 buffer")
    if dev:
        from . import ops

        # checks the same arguments before the upload
        return ops.composite(bands, starts, fmasks, fmask_starts, step_ptr, bands_per_scene, shape, bits, no_data_value, min_clear, method)
    st, fst, ptr, T, N, max_m, H, W = check_composite(bands.shape[0], starts, None if fmasks is None else fmasks.shape[0], fmask_starts, step_ptr,
                                                      bands_per_scene, shape, bits, no_data_value, min_clear, method)
    return _composite_host(bands, st, fmasks, fst, ptr, int(bands_per_scene), H, W, int(bits), int(no_data_value), int(min_clear), method)


# ---- dates and order -------------------------------------------------------------------------------------------------------------------------
def parse_date(d) -> datetime.date:
    """YYYYMMDD, YYYY-MM-DD (text or int) or a date -> a date."""
    if isinstance(d, datetime.datetime):
        return d.date()
    if isinstance(d, datetime.date):
        return d
    s = str(d).replace("-", "")
    if isinstance(d, bool) or len(s) != 8 or not s.isdigit():
        raise ValueError(f"a date is YYYYMMDD or YYYY-MM-DD (got {d!r})")
    return datetime.datetime.strptime(s, "%Y%m%d").date()


def order_candidates(acquired: Sequence, target) -> List[int]:
    """The positions of the candidates by |acquisition date - target date|, the earlier date on a tie; list order among equal dates."""
    tgt = parse_date(target)
    days = [parse_date(a) for a in acquired]
    return sorted(range(len(days)), key=lambda i: (abs((days[i] - tgt).days), days[i]))


# ---- files -> files -------------------------------------------------------------------------------------------------------------------------
def _steps_of(scenes, what: str = "scenes") -> List[List[List[str]]]:
    """``scenes`` as [step][scene][band]; the steps may be empty, the scenes of a composite have one number of bands."""
    if not isinstance(scenes, (list, tuple)) or not scenes:
        raise ValueError(f"{what} is a list of steps, each a list of scenes, each a list of band files")
    C = None
    steps = []
    for d in scenes:
        if not isinstance(d, (list, tuple)):
            raise ValueError(f"a step is a list of scenes (got {d!r})")
        for s in d:
            if not isinstance(s, (list, tuple)) or not s or not all(isinstance(f, str) for f in s):
                raise ValueError(f"a scene is a list of band files (got {s!r})")
            C = len(s) if C is None else C
            if len(s) != C:
                raise ValueError(f"a scene is a list of {C} band files (got {s!r})")
        steps.append([list(s) for s in d])
    return steps


def _grid_key(profile: Dict[str, Any], shape) -> Tuple:
    return (tuple(shape),) + tuple(profile["tags"].get(k) for k in GRID_TAGS)


def create_composite(scenes, fmasks, output_directory: str, dates: Optional[Sequence] = None, method: str = "medoid",
                     mask_types: Sequence[str] = MASK_TYPES, min_clear: int = 1, no_data: int = NO_DATA_VALUE,
                     device: Optional[str] = None) -> Tuple[List[str], Dict[str, Any]]:
    """One composite scene per temporal step from the HLS scenes of one MGRS tile.  ``scenes``: a list of steps, each a list of scenes,
    each a list of C single-band int16 GeoTIFF files named as HLS names them (``HLS.S30.T38PMB.2022145T072619.v2.0.B02.tif``); ``fmasks``:
    the same nesting without the band level, one uint8 Fmask file per scene (None: only ``no_data`` decides what is clear).  All files share
    one size, tiepoint, pixel scale and GeoKeys (ValueError otherwise).  ``dates``: one target date per step (YYYYMMDD or YYYY-MM-DD); the
    candidates of a step are ordered by |acquisition date - target|, the earlier date on a tie; None: the date of the step's first scene,
    list order kept.  Writes under ``output_directory``, per step and band, ``HLS.M30.<tile>.<YYYYDDD>T000000.v2.0.<band>.tif`` (int16; the
    band field of the step's first candidate), per step ``composite_<tile>_<YYYYDDD>_count.tif`` and ``..._source.tif`` (uint8), all with
    the scenes' georeferencing, and ``composite_stats.json`` (per step the candidates in the order used, the count histogram, the covered
    share and ``tiles``, the band files in the order ``chips.tiles`` wants).  ``device``: None = the numpy path, ``"cuda"`` / ``"cuda:n"``
    = the kernel; both write the same bytes.  -> (the band files written, step after step, the stats)."""
    if method not in METHODS:
        raise ValueError(f"method must be one of {tuple(METHODS)} (got {method!r})")
    bits = chipmod.mask_bits(mask_types)
    prep.check_device(device)
    steps = _steps_of(scenes)
    if len(steps) > MAX_DATES or max(len(d) for d in steps) > MAX_CANDIDATES:
        raise ValueError(f"{len(steps)} steps of up to {max(len(d) for d in steps)} scenes: at most {MAX_DATES} steps of {MAX_CANDIDATES} candidates")
    if not any(steps):
        raise ValueError("a composite needs at least one scene")
    fsteps = None
    if fmasks is not None:
        if not isinstance(fmasks, (list, tuple)) or [len(d) if isinstance(d, (list, tuple)) else -1 for d in fmasks] != [len(d) for d in steps]:
            raise ValueError("fmasks has the nesting of scenes without the band level: one Fmask file per scene")
        fsteps = [[str(f) for f in d] for d in fmasks]
    if dates is not None and (isinstance(dates, str) or len(dates) != len(steps)):
        raise ValueError(f"dates holds one target date per step ({len(steps)})")
    # the order of the candidates and the date of every step
    targets = []
    for t, d in enumerate(steps):
        if dates is not None:
            target = parse_date(dates[t])
            order = order_candidates([prep.hls_date(s[0]) for s in d], target)
            steps[t] = [d[i] for i in order]
            if fsteps is not None:
                fsteps[t] = [fsteps[t][i] for i in order]
        elif d:
            target = parse_date(prep.hls_date(d[0][0]))
        else:
            raise ValueError(f"step {t} has no scene to take its date from: give dates")
        targets.append(target)
    flat = [s for d in steps for s in d]
    C = len(flat[0])
    tile = prep.hls_name(flat[0][0]).tile
    for s in flat:
        if any(prep.hls_name(f).tile != tile for f in s):
            raise ValueError(f"{s[0]}: the scenes of a composite belong to one MGRS tile ({tile})")
    files = [f for s in flat for f in s]
    bands, starts, shapes, profiles = prep.read_planes(files, "band", np.int16)
    key = _grid_key(profiles[0], shapes[0])
    for f, p, sh in zip(files, profiles, shapes):
        if _grid_key(p, sh) != key:
            raise ValueError(f"{f}: its size, tiepoint, pixel scale or GeoKeys differ from those of {files[0]}: the scenes share one grid")
    fm = fst = None
    if fsteps is not None:
        ffiles = [f for d in fsteps for f in d]
        fm, fst, fshapes, fprofiles = prep.read_planes(ffiles, "Fmask", np.uint8)
        for f, p, sh in zip(ffiles, fprofiles, fshapes):
            if _grid_key(p, sh) != key:
                raise ValueError(f"{f}: its size, tiepoint, pixel scale or GeoKeys differ from those of {files[0]}: the scenes share one grid")
    H, W = shapes[0]
    ptr = np.concatenate([[0], np.cumsum([len(d) for d in steps])]).astype(np.int32)
    comp, count, source, hist = composite(prep.to_device(bands, device), starts, None if fm is None else prep.to_device(fm, device), fst, ptr, C,
                                          (H, W), bits, no_data, min_clear, method)
    comp, count, source, hist = to_host(comp), to_host(count), to_host(source), to_host(hist)
    os.makedirs(output_directory, exist_ok=True)
    profile = {"tags": prep.geo_tags(profiles[0]["tags"], tiepoint=True), "nodata": None}
    written: List[str] = []
    stats: Dict[str, Any] = {"tile": tile, "method": method, "mask_types": list(mask_types), "min_clear": int(min_clear), "no_data": int(no_data),
                             "steps": [], "tiles": []}
    for t, d in enumerate(steps):
        doy = targets[t].strftime("%Y%j")
        names = d[0] if d else flat[0]  # a step without candidates borrows the band names
        tiles = []
        for c in range(C):
            band = os.path.basename(names[c]).split(".")[-2]
            tiles.append(f"HLS.M30.{tile}.{doy}T000000.v2.0.{band}.tif")
            tiff.write(os.path.join(output_directory, tiles[-1]), comp[t, c], profile)
        aux = [f"composite_{tile}_{doy}_count.tif", f"composite_{tile}_{doy}_source.tif"]
        tiff.write(os.path.join(output_directory, aux[0]), count[t], profile)
        tiff.write(os.path.join(output_directory, aux[1]), source[t], profile)
        covered = float(hist[t, int(min_clear):].sum()) / float(H * W) if H * W else 0.0
        stats["steps"].append({"date": targets[t].strftime("%Y%m%d"), "candidates": [[os.path.basename(f) for f in s] for s in d],
                               "histogram": [int(v) for v in hist[t]], "covered": covered, "tiles": tiles, "count": aux[0], "source": aux[1]})
        stats["tiles"] += tiles
        written += tiles
    prep.write_stats(os.path.join(output_directory, "composite_stats.json"), stats)
    return written, stats


# ---- mode=create_composite -----------------------------------------------------------------------------------------------------------------
CONFIG_KEYS = ("scenes", "fmasks", "dates", "method", "mask_types", "min_clear", "no_data", "output_directory", "device")


def composite_options(cfg: Dict[str, Any]) -> Dict[str, Any]:
    """The ``composite.*`` keys of ``mode=create_composite`` checked -> the keyword arguments of :func:`create_composite`.  A bad value
    raises ValueError; ``scenes`` and ``output_directory`` are required only in that mode."""
    c = prep.Section(cfg, "composite", CONFIG_KEYS)
    method = c.choice("method", "medoid", METHODS)
    types = c.listing("mask_types", list(MASK_TYPES)) or []
    try:
        chipmod.mask_bits(types)
    except ValueError as e:
        raise c.bad("mask_types", f"must be a list of Fmask types ({e})", types) from None
    min_clear = c.integer("min_clear", 1, lo=1, hi=MAX_CANDIDATES, what=f"must be an int in [1, {MAX_CANDIDATES}]")
    nd = c.integer("no_data", NO_DATA_VALUE, lo=-32768, hi=32767, what="must be an int that fits int16")
    device = c.get("device")
    if device is not None and device != "host":
        try:
            prep.check_device(device)
        except ValueError:
            raise c.bad("device", "must be None, host or a cuda device", device) from None
    scenes = c.get("scenes")
    if scenes is not None:
        try:
            scenes = _steps_of(scenes)
        except ValueError as e:
            raise c.bad("scenes", f"must be a list of steps of scenes of band files ({e})", scenes) from None
        if len(scenes) > MAX_DATES or max(len(d) for d in scenes) > MAX_CANDIDATES:
            raise c.bad("scenes", f"holds at most {MAX_DATES} steps of {MAX_CANDIDATES} scenes", scenes)
    fmasks = c.get("fmasks")
    if fmasks is not None:
        ok = isinstance(fmasks, (list, tuple)) and all(isinstance(d, (list, tuple)) and all(isinstance(f, str) for f in d) for d in fmasks)
        if not ok or (scenes is not None and [len(d) for d in fmasks] != [len(d) for d in scenes]):
            raise c.bad("fmasks", "must have the nesting of scenes without the band level", fmasks)
        fmasks = [list(d) for d in fmasks]
    dates = c.get("dates")
    if dates is not None:
        if not isinstance(dates, (list, tuple)) or (scenes is not None and len(dates) != len(scenes)):
            raise c.bad("dates", "must hold one target date per step", dates)
        try:
            dates = [parse_date(d).strftime("%Y%m%d") for d in dates]
        except ValueError as e:
            raise c.bad("dates", f"must hold one target date per step ({e})", dates) from None
    out = c.text("output_directory")
    if cfg.get("mode") == "create_composite" and (not scenes or out is None):
        raise ValueError("mode=create_composite needs composite.scenes and composite.output_directory")
    return dict(scenes=scenes, fmasks=fmasks, output_directory=out, dates=dates, method=method, mask_types=types, min_clear=min_clear, no_data=nd,
                device=device)


def run_from_config(cfg: Dict[str, Any], device: Optional[str] = None) -> int:
    """``mode=create_composite``: :func:`create_composite` under the ``composite.*`` keys; prints one JSON line.  ``composite.device``:
    None = ``device`` (the device when there is one), ``host`` = the numpy path."""
    kw = composite_options(cfg)
    chosen = kw.pop("device")
    device = device if chosen is None else (None if chosen == "host" else chosen)
    written, stats = create_composite(device=device, **kw)
    print(json.dumps({"create_composite": {"steps": len(stats["steps"]), "files": len(written), "covered": [s["covered"] for s in stats["steps"]],
                                           "output_directory": kw["output_directory"]}}))
    return 0


def main(argv: Optional[List[str]] = None) -> int:
    """``python -m instageo_amd.composite composite.scenes=[[[a_B02.tif,a_B03.tif],[b_B02.tif,b_B03.tif]]] composite.output_directory=out
    ...``: mode=create_composite without ``run.py``."""
    return prep.run_mode_cli("create_composite", run_from_config, argv)


if __name__ == "__main__":
    raise SystemExit(main())
