"""Speckle filtering and dB scaling of Sentinel-1 RTC scenes, on the device.

``mode=create_s1_chips`` copies linear-power gamma0 into its chips as the reference does (``instageo/data/s1_utils.py``).  Linear gamma0
is heavy-tailed and carries multiplicative noise (speckle); radar segmentation pipelines filter it and train on dB.  This module turns
band files into filtered band files UNDER THE SAME BASE NAMES in another folder, so that ``s1_chips.scenes`` takes them unchanged
(``s1_chips.tile_id_of`` still parses them).  It is the host layer on top of :mod:`instageo_amd.prep`, :mod:`instageo_amd.tiff` and
``ig_s1_speckle`` (``s1_filter.hip``).

The rule (stated in ``include/instageo_hip.h``).  A value is present when it is finite and differs from ``src_nodata``.  The window of
``window`` x ``window`` pixels (odd, 3..15) around a pixel is clipped to the plane; the sum A, the sum of squares Q and the number n of its
present values are formed in float64 in a fixed order (per window row left to right, then the rows top to bottom).  An absent centre
stays absent (NaN).  For a present centre x: m = A / n, v = max(Q / n - m m, 0), s = 1 / looks, and

* ``boxcar``: y = m;
* ``lee`` (Lee 1980, the MMSE form): y = m + b (x - m) with b = vx / v, vx = (v - m m s) / (1 + s), b = 0 unless v > 0 and vx > 0;
* ``gamma_map`` (Lopes et al. 1990): y = m where ci2 = v / (m m) <= s (or m <= 0), y = x where ci2 >= 2 s, in between
  y = (B m + sqrt(D)) / (2 a) with a = (1 + s) / (ci2 - s), B = a - looks - 1, D = m m B B + 4 a looks m x;
* ``refined_lee`` (Lee 1981, the default speckle filter of ESA's SNAP; ``window`` must be 7): where the 7 x 7 window is homogeneous
  (``lee``'s b = 0) y = m.  Elsewhere the means of nine 3 x 3 sub-windows, two pixels apart, give four gradients; the largest names
  the edge's direction, and ``lee`` is applied to the 28 pixels of the half window on the centre's side of it (E, W, S, N, SE, NW, NE
  or SW).  A pixel one of whose sub-windows is empty (the outermost ring of a plane, large holes) gets ``lee`` of the full window.  The
  header states the order of every sum, the ties and the masks.

``scale="linear"`` writes (float32)y; ``scale="db"`` writes (float32)(10 log10 y) where y > 0 and NaN (a DROPPED pixel) elsewhere.
``looks`` is the equivalent number of looks, a user setting (4.4: the nominal value of IW GRD), not a measurement.

Device tensors go through ``ig_s1_speckle``; host arrays take a numpy twin of the same rule, so the module works (and is tested) without
a GPU (``refined_lee`` goes through ``ig_s1_refined_lee``).  ``boxcar``, ``lee`` and ``refined_lee`` in linear scale use correctly
rounded operations only: both paths write the same bytes.  ``sqrt`` and
``log10`` are each side's library function, so ``gamma_map`` and dB values may differ in the last float32 bit.

A dB value of exactly -1.0 collides with the default ``no_data_value`` of ``create_s1_chips``: cut dB chips with
``s1_chips.no_data_value=-9999``.

Multi-temporal (Quegan) filtering of a stack of dates is :mod:`instageo_amd.s1_temporal`.  Not done: refined Lee at other window sizes
or with SNAP's ``edgeThreshold`` (the homogeneity test stands in for it), Lee-sigma and Frost, a vv / vh ratio band, calibration of GRD,
SAFE input.
"""
from __future__ import annotations

import json
import os
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

from . import prep, tiff
from .prep import is_device, to_host

METHODS = {"boxcar": 0, "lee": 1, "gamma_map": 2, "refined_lee": 3}  # include/instageo_hip.h: 0..2 ig_s1_speckle, 3 ig_s1_refined_lee
REFINED_LEE = METHODS["refined_lee"]
REFINED_WINDOW = 7  # the only window of refined_lee
SCALES = {"linear": 0, "db": 1}
MAX_HALF = 7  # window = 2 h + 1 <= 15
LOOKS = 4.4  # the nominal equivalent number of looks of IW GRD
TILE_W, TILE_H = 64, 32  # the tile of one workgroup of ig_s1_speckle (s1_filter.hip)
NODATA_TAG = 42113  # GDAL_NODATA
_ROWS = 512  # rows of a plane the host path works on at a time
_QNAN = np.array([0x7FC00000], dtype=np.uint32).view(np.float32)[0]


# ---- argument checks shared by the host path and the device wrapper (ops.s1_speckle) --------------------------------------------------------
def check_speckle(size: int, starts, sizes, window, method, looks, src_nodata, scale):
    """ValueError unless the arguments of a filter run obey include/instageo_hip.h -> (starts int64 (N,), sizes int32 (N, 2), h, method
    code, looks float32, src_nodata float32 or None, to_db 0 | 1).  Every plane lies inside the buffer of ``size`` elements and no two
    planes overlap (every output element is written once)."""
    if isinstance(window, bool) or not isinstance(window, (int, np.integer)) or not 3 <= int(window) <= 2 * MAX_HALF + 1 or int(window) % 2 == 0:
        raise ValueError(f"window must be an odd int in [3, {2 * MAX_HALF + 1}] (got {window!r})")
    if method not in METHODS:
        raise ValueError(f"method must be one of {tuple(METHODS)} (got {method!r})")
    if method == "refined_lee" and int(window) != REFINED_WINDOW:
        raise ValueError(f"window must be {REFINED_WINDOW} with method refined_lee (got {window!r})")
    if scale not in SCALES:
        raise ValueError(f"scale must be one of {tuple(SCALES)} (got {scale!r})")
    if isinstance(looks, bool) or not isinstance(looks, (int, float, np.integer, np.floating)):
        raise ValueError(f"looks must be a finite number > 0 (got {looks!r})")
    with np.errstate(over="ignore"):
        lk = np.float32(looks)
    if not (lk > 0 and np.isfinite(lk)):
        raise ValueError(f"looks must be a finite number > 0 as float32 (got {looks!r})")
    snd = None
    if src_nodata is not None:
        if isinstance(src_nodata, bool) or not isinstance(src_nodata, (int, float, np.integer, np.floating)) or np.isnan(np.float32(src_nodata)):
            raise ValueError(f"src_nodata must be None or a number that is not NaN (got {src_nodata!r})")
        snd = np.float32(src_nodata)
    st = np.asarray(starts)
    ss = np.asarray(sizes)
    if st.size and st.dtype.kind not in "iu" or ss.size and ss.dtype.kind not in "iu":
        raise ValueError("the offsets and sizes of the planes must be integers")
    st = np.ascontiguousarray(st.astype(np.int64).reshape(-1))
    N = st.shape[0]
    if ss.size != 2 * N:
        raise ValueError(f"{N} planes need {N} sizes (H, W)")
    ss = ss.astype(np.int64).reshape(N, 2)
    if int(size) >= 2**40:
        raise ValueError("the packed planes hold 2^40 elements or more")
    if N:
        hw = ss[:, 0] * ss[:, 1]
        if (ss < 1).any() or (hw > 2**31 - 1).any():
            raise ValueError("a plane has 1 <= H * W <= 2^31 - 1 pixels")
        if (st < 0).any() or (st + hw > int(size)).any():
            raise ValueError(f"a plane does not lie inside the packed buffer of {size} elements")
        order = np.argsort(st, kind="stable")
        if (st[order][1:] < (st + hw)[order][:-1]).any():
            raise ValueError("two planes overlap: every output element is written once")
    return st, np.ascontiguousarray(ss, dtype=np.int32), int(window) // 2, METHODS[method], lk, snd, SCALES[scale]


def tile_table(sizes: np.ndarray) -> np.ndarray:
    """The prefix table of workgroup tiles ``ig_s1_speckle`` wants: N + 1 ascending int64 from 0."""
    ss = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
    per = ((ss[:, 0] + TILE_H - 1) // TILE_H) * ((ss[:, 1] + TILE_W - 1) // TILE_W)
    return np.concatenate([[0], np.cumsum(per)]).astype(np.int64)


# ---- the rule on host arrays ---------------------------------------------------------------------------------------------------------------
# the half windows of refined_lee in the order SE, NW, NE, SW, E, W, S, N: (8, 7, 7) bool over (dy + 3, dx + 3)
_DY, _DX = np.mgrid[-3:4, -3:4]
HALF_MASKS = np.stack([_DX + _DY >= 0, _DX + _DY <= 0, _DX - _DY >= 0, _DX - _DY <= 0, _DX >= 0, _DX <= 0, _DY >= 0, _DY <= 0])


def _lee(A, Q, dn, x, s):
    """``lee`` from the sums of a window, each operation rounded on its own -> (y, m, v, vx)."""
    m = A / dn
    mm = m * m
    v = Q / dn - mm
    v = np.where(v < 0, 0.0, v)
    vx = (v - mm * s) / (1.0 + s)
    b = np.where((v > 0) & (vx > 0), vx / v, 0.0)
    return m + b * (x - m), m, v, vx


def _refined_lee(Z: np.ndarray, pres: np.ndarray, rows: int, W: int, A, Q, dn, x, s) -> np.ndarray:
    """Steps 1 to 4 of the refined Lee rule of include/instageo_hip.h for every pixel at once.  ``Z``, ``pres``: the staged rows with
    their halo of 3 (absent values +0.0 / False); (A, Q, dn): the sums of the full window -> y float64 (anything at an absent centre)."""
    lee, m, v, vx = _lee(A, Q, dn, x, s)
    # the mean of the 3 x 3 window whose top left corner is the staged value (a, b): per row left to right, then top to bottom
    R3 = np.zeros((rows + 6, W + 4), dtype=np.float64)
    K3 = np.zeros((rows + 6, W + 4), dtype=np.int64)
    for j in range(3):
        R3 += Z[:, j : j + W + 4]
        K3 += pres[:, j : j + W + 4]
    A3 = np.zeros((rows + 4, W + 4), dtype=np.float64)
    n3 = np.zeros((rows + 4, W + 4), dtype=np.int64)
    for i in range(3):
        A3 += R3[i : i + rows + 4]
        n3 += K3[i : i + rows + 4]
    mean = np.where(n3 > 0, A3 / np.where(n3 > 0, n3, 1), np.nan)
    M = [[mean[2 * i : 2 * i + rows, 2 * j : 2 * j + W] for j in range(3)] for i in range(3)]  # the sub-window (i, j) of every pixel
    whole = np.ones((rows, W), dtype=bool)
    for i in range(3):
        for j in range(3):
            whole &= ~np.isnan(M[i][j])
    c0 = M[1][1]
    g = [np.abs(((M[1][2] + M[2][1]) + M[2][2]) - ((M[0][0] + M[0][1]) + M[1][0])),
         np.abs(((M[0][1] + M[0][2]) + M[1][2]) - ((M[1][0] + M[2][0]) + M[2][1])),
         np.abs(((M[0][2] + M[1][2]) + M[2][2]) - ((M[0][0] + M[1][0]) + M[2][0])),
         np.abs(((M[2][0] + M[2][1]) + M[2][2]) - ((M[0][0] + M[0][1]) + M[0][2]))]
    first = [np.abs(M[2][2] - c0) <= np.abs(M[0][0] - c0), np.abs(M[0][2] - c0) <= np.abs(M[2][0] - c0),
             np.abs(M[1][2] - c0) <= np.abs(M[1][0] - c0), np.abs(M[2][1] - c0) <= np.abs(M[0][1] - c0)]
    best = g[0]
    half = np.where(first[0], 0, 1)
    for k in range(1, 4):  # a later gradient wins only when it is larger
        win = g[k] > best
        best = np.where(win, g[k], best)
        half = np.where(win, np.where(first[k], 2 * k, 2 * k + 1), half)
    # the half window: one pass over the 49 offsets, a value outside the pixel's mask adds +0.0
    Ah = np.zeros((rows, W), dtype=np.float64)
    Qh = np.zeros_like(Ah)
    nh = np.zeros((rows, W), dtype=np.int64)
    for i in range(7):
        Ar = np.zeros((rows, W), dtype=np.float64)
        Qr = np.zeros_like(Ar)
        for j in range(7):
            take = HALF_MASKS[:, i, j][half] & pres[i : i + rows, j : j + W]
            xv = np.where(take, Z[i : i + rows, j : j + W], 0.0)
            Ar += xv
            Qr += xv * xv
            nh += take
        Ah += Ar
        Qh += Qr
    edge = _lee(Ah, Qh, np.where(nh > 0, nh, 1).astype(np.float64), x, s)[0]
    return np.where((v > 0) & (vx > 0), np.where(whole, edge, lee), m)


def _filter_rows(P: np.ndarray, rows: int, W: int, h: int, code: int, looks: np.float32, to_db: int) -> Tuple[np.ndarray, int, int]:
    """``P``: (rows + 2 h, W + 2 h) float32, the rows of a plane with their halo, absent values and what lies outside the plane as NaN
    -> (the rows filtered, present outputs, dropped pixels).  A Python loop over the window's offsets in the rule's order."""
    w = 2 * h + 1
    pres = ~np.isnan(P)
    Z = np.where(pres, P, np.float32(0)).astype(np.float64)  # an absent value adds +0.0, which changes no bit of a sum that began at +0.0
    Ai = np.zeros((rows + 2 * h, W), dtype=np.float64)
    Qi = np.zeros_like(Ai)
    Ki = np.zeros((rows + 2 * h, W), dtype=np.int64)
    for j in range(w):  # left to right
        x = Z[:, j : j + W]
        Ai += x
        Qi += x * x
        Ki += pres[:, j : j + W]
    A = np.zeros((rows, W), dtype=np.float64)
    Q = np.zeros_like(A)
    n = np.zeros((rows, W), dtype=np.int64)
    for i in range(w):  # top to bottom
        A += Ai[i : i + rows]
        Q += Qi[i : i + rows]
        n += Ki[i : i + rows]
    centre = pres[h : h + rows, h : h + W]
    x = Z[h : h + rows, h : h + W]
    lk = np.float64(looks)
    s = np.float64(1.0) / lk
    with np.errstate(all="ignore"):
        dn = np.where(centre, n, 1).astype(np.float64)
        m = A / dn
        mm = m * m
        v = Q / dn - mm
        v = np.where(v < 0, 0.0, v)
        if code == 0:
            y = m
        elif code == 1:
            t = mm * s
            vx = (v - t) / (1.0 + s)
            b = np.where((v > 0) & (vx > 0), vx / v, 0.0)
            y = m + b * (x - m)
        elif code == REFINED_LEE:
            y = _refined_lee(Z, pres, rows, W, A, Q, dn, x, s)
        else:
            ci2 = v / mm
            a = (1.0 + s) / (ci2 - s)
            B = a - lk - 1.0
            D = mm * (B * B) + ((4.0 * a) * lk) * (m * x)
            mid = np.where(D >= 0, (B * m + np.sqrt(D)) / (2.0 * a), m)
            y = np.where(m <= 0, m, np.where(ci2 <= s, m, np.where(ci2 >= 2.0 * s, x, mid)))
        if to_db:
            keep = centre & (y > 0)
            val = (10.0 * np.log10(np.where(keep, y, 1.0))).astype(np.float32)
        else:
            keep = centre
            val = y.astype(np.float32)
    out = np.where(keep, val, _QNAN)
    return out, int(keep.sum()), int((centre & ~keep).sum())


def _speckle_host(planes, st, ss, h, code, looks, snd, to_db):
    """numpy twin of ``ig_s1_speckle`` and, for code 3 (h = 3), of ``ig_s1_refined_lee``: plane by plane, ``_ROWS`` rows at a time with
    their halo of h rows, vectorised over the pixels."""
    out = np.zeros(planes.shape[0], dtype=np.float32)
    counts = np.zeros((st.shape[0], 2), dtype=np.int32)
    for p in range(st.shape[0]):
        H, W = int(ss[p, 0]), int(ss[p, 1])
        src = planes[int(st[p]) : int(st[p]) + H * W].reshape(H, W)
        dst = out[int(st[p]) : int(st[p]) + H * W].reshape(H, W)
        for r0 in range(0, H, _ROWS):
            r1 = min(r0 + _ROWS, H)
            lo, hi = max(r0 - h, 0), min(r1 + h, H)
            P = np.full((r1 - r0 + 2 * h, W + 2 * h), np.nan, dtype=np.float32)
            blk = src[lo:hi]
            absent = ~np.isfinite(blk)
            if snd is not None:
                absent |= blk == snd
            P[lo - (r0 - h) : hi - (r0 - h), h : h + W] = np.where(absent, np.float32(np.nan), blk)
            dst[r0:r1], present, dropped = _filter_rows(P, r1 - r0, W, h, code, looks, to_db)
            counts[p, 0] += present
            counts[p, 1] += dropped
    return out, counts


def speckle(planes, starts, sizes, window: int = 7, method: str = "lee", looks: float = LOOKS, src_nodata: Optional[float] = None,
            scale: str = "linear"):
    """The packed float32 planes ``planes`` (1-D; plane p of ``sizes[p]`` = (H, W) at element ``starts[p]``) filtered by the rule of the
    module docstring -> (out: float32 with the layout of ``planes``, absent and dropped pixels NaN, elements outside every plane 0;
    counts (N, 2) int32: per plane the present outputs and the pixels the dB step dropped).  A tensor on the device goes through
    ``ig_s1_speckle`` (``refined_lee``: ``ig_s1_refined_lee``) and gives device tensors; anything else takes the numpy twin and gives
    arrays."""
    dev = is_device(planes)
    if not dev:
        planes = to_host(planes)
    if str(planes.dtype).replace("torch.", "") != "float32" or planes.ndim != 1:
        raise ValueError("the planes are one packed 1-D float32 buffer")
    if dev:
        from . import ops

        if method == "refined_lee":
            check_speckle(0, [], [], window, method, looks, src_nodata, scale)  # the window: the op has none
            return ops.s1_refined_lee(planes, starts, sizes, looks, src_nodata, scale)
        return ops.s1_speckle(planes, starts, sizes, window, method, looks, src_nodata, scale)  # checks the same arguments before the upload
    st, ss, h, code, lk, snd, to_db = check_speckle(planes.shape[0], starts, sizes, window, method, looks, src_nodata, scale)
    return _speckle_host(planes, st, ss, h, code, lk, snd, to_db)


# ---- files -> files -------------------------------------------------------------------------------------------------------------------------
def _flatten(scenes, files: List[str]):
    """The files of ``scenes`` in order appended to ``files`` -> the nesting with every file replaced by its position."""
    if isinstance(scenes, str):
        files.append(scenes)
        return len(files) - 1
    if not isinstance(scenes, (list, tuple)) or not scenes:
        raise ValueError(f"scenes is a list of band files, or the nesting s1_chips.scenes takes (got {scenes!r})")
    return [_flatten(s, files) for s in scenes]


def _rebuild(nest, names: List[str]):
    return names[nest] if isinstance(nest, int) else [_rebuild(s, names) for s in nest]


def filter_s1(scenes, output_directory: str, method: str = "lee", window: int = 7, looks: float = LOOKS, scale: str = "linear",
              src_nodata: Optional[float] = None, device: Optional[str] = None, max_bytes: int = 1 << 31):
    """Every single-band float32 GeoTIFF of ``scenes`` (the nesting ``s1_chips.scenes`` takes: dates of scenes of band files, or a flat
    list of files) filtered and written as a float32 GeoTIFF under the same base name in ``output_directory``, with the source's tiepoint,
    pixel scale and GeoKeys and NaN as its no-data.  ``src_nodata``: None = each file's own no-data tag (a file without one: only what is
    not finite is absent).  The planes are filtered in batches of at most ``max_bytes`` of input (a scene of 11000 x 11000 is 484 MB);
    ``filter_stats.json`` holds the settings and per file the pixels, the present outputs and the pixels dropped by the dB step.  An
    output that would replace an input, or two inputs of one base name, raise ValueError before anything is written.  ``device``: None =
    the numpy path, ``"cuda"`` / ``"cuda:n"`` = the kernel.  -> the written paths in the nesting of ``scenes``."""
    check_speckle(0, [], [], window, method, looks, src_nodata, scale)
    prep.check_device(device)
    if isinstance(max_bytes, bool) or not isinstance(max_bytes, (int, np.integer)) or max_bytes < 1:
        raise ValueError(f"max_bytes must be a positive int (got {max_bytes!r})")
    files: List[str] = []
    nest = _flatten(scenes, files)
    names = [os.path.join(output_directory, os.path.basename(f)) for f in files]
    if len({os.path.basename(f) for f in files}) != len(files):
        raise ValueError("two input files share a base name: their outputs would replace one another")
    ins = {os.path.realpath(f) for f in files}
    for n in names:
        if os.path.realpath(n) in ins:
            raise ValueError(f"{n}: the output would replace an input; choose another output_directory")
    # what every file needs, from its header: its size in bytes and its own no-data value
    pixels, nodata = [], []
    for f in files:
        prof = tiff.read_profile(f)
        pixels.append(int(prof["height"]) * int(prof["width"]))
        nd = src_nodata if src_nodata is not None else prof.get("nodata")
        nodata.append(None if nd is None or nd != nd else float(np.float32(nd)))
    os.makedirs(output_directory, exist_ok=True)
    stats: Dict[str, Any] = {"method": method, "window": int(window), "looks": float(looks), "scale": scale,
                             "src_nodata": None if src_nodata is None else float(src_nodata), "files": {}}
    k = 0
    while k < len(files):
        e, held = k + 1, 4 * pixels[k]  # a batch: consecutive files of one no-data value inside the byte budget, at least one
        while e < len(files) and nodata[e] == nodata[k] and held + 4 * pixels[e] <= max_bytes:
            held += 4 * pixels[e]
            e += 1
        planes, starts, shapes, profiles = prep.read_planes(files[k:e], "band", np.float32)
        out, counts = speckle(prep.to_device(planes, device), starts, shapes, window, method, looks, nodata[k], scale)
        out, counts = to_host(out), to_host(counts)
        for i in range(e - k):
            H, W = shapes[i]
            tags = prep.geo_tags(profiles[i]["tags"], tiepoint=True)
            tags[NODATA_TAG] = (2, "nan")
            tiff.write(names[k + i], out[int(starts[i]) : int(starts[i]) + H * W].reshape(H, W), {"tags": tags, "nodata": None})
            stats["files"][os.path.basename(names[k + i])] = {"pixels": H * W, "present": int(counts[i, 0]), "dropped": int(counts[i, 1]),
                                                              "src_nodata": nodata[k]}
        k = e
    prep.write_stats(os.path.join(output_directory, "filter_stats.json"), stats)
    return _rebuild(nest, names)


# ---- mode=filter_s1 ------------------------------------------------------------------------------------------------------------------------
CONFIG_KEYS = ("scenes", "output_directory", "method", "window", "looks", "scale", "src_nodata")


def s1_filter_options(cfg: Dict[str, Any]) -> Dict[str, Any]:
    """The ``s1_filter.*`` keys of ``mode=filter_s1`` checked -> the keyword arguments of :func:`filter_s1`.  A bad value raises
    ValueError; ``scenes`` and ``output_directory`` are required only in that mode."""
    c = prep.Section(cfg, "s1_filter", CONFIG_KEYS)
    method = c.choice("method", "lee", METHODS)
    scale = c.choice("scale", "linear", SCALES)
    window = c.integer("window", 7, lo=3, hi=2 * MAX_HALF + 1, what=f"must be an odd int in [3, {2 * MAX_HALF + 1}]")
    if window % 2 == 0:
        raise c.bad("window", f"must be an odd int in [3, {2 * MAX_HALF + 1}]", window)
    if method == "refined_lee" and window != REFINED_WINDOW:
        raise c.bad("window", f"must be {REFINED_WINDOW} with method=refined_lee", window)
    looks = c.number("looks", LOOKS, lambda v: 0 < v < np.inf and np.isfinite(np.float32(v)) and np.float32(v) > 0,
                     "must be a finite number > 0")
    snd = c.get("src_nodata")
    if snd is not None:
        snd = c.number("src_nodata", None, lambda v: v == v, "must be None or a number that is not NaN")
    scenes = c.get("scenes")
    if scenes is not None:
        try:
            _flatten(scenes, [])
        except ValueError as e:
            raise c.bad("scenes", f"must be a list of band files or of dates of scenes of band files ({e})", scenes) from None
    out = c.text("output_directory")
    if cfg.get("mode") == "filter_s1" and (not scenes or out is None):
        raise ValueError("mode=filter_s1 needs s1_filter.scenes and s1_filter.output_directory")
    return dict(scenes=scenes, output_directory=out, method=method, window=window, looks=looks, scale=scale, src_nodata=snd)


def run_from_config(cfg: Dict[str, Any], device: Optional[str] = None) -> int:
    """``mode=filter_s1``: :func:`filter_s1` under the ``s1_filter.*`` keys; prints one JSON line."""
    kw = s1_filter_options(cfg)
    written: List[str] = []
    _flatten(filter_s1(device=device, **kw), written)
    with open(os.path.join(kw["output_directory"], "filter_stats.json")) as f:
        per = json.load(f)["files"]
    print(json.dumps({"filter_s1": {"files": len(written), "present": sum(v["present"] for v in per.values()),
                                    "dropped": sum(v["dropped"] for v in per.values()), "output_directory": kw["output_directory"]}}))
    return 0


def main(argv: Optional[List[str]] = None) -> int:
    """``python -m instageo_amd.s1_filter s1_filter.scenes=[a_vv.tif,a_vh.tif] s1_filter.output_directory=out ...``: mode=filter_s1
    without ``run.py``."""
    return prep.run_mode_cli("filter_s1", run_from_config, argv)


if __name__ == "__main__":
    raise SystemExit(main())
