"""Multi-temporal (Quegan and Yu) speckle filtering of Sentinel-1 RTC stacks, on the device.

``mode=filter_s1`` (:mod:`instageo_amd.s1_filter`) despeckles one scene at a time with a spatial window, which blurs field edges and narrow
water bodies.  A stack of dates allows better: every date is filtered by borrowing the OTHER dates at the same pixel (Quegan and Yu 2001),
which takes out speckle at the spatial resolution of the input.  This module turns the band files of a stack into filtered band files
UNDER THE SAME BASE NAMES in another folder, in the nesting they came in, so that ``s1_chips.scenes`` or ``s1_filter.scenes`` takes them
unchanged.  It is the host layer on top of :mod:`instageo_amd.prep`, :mod:`instageo_amd.tiff` and ``ig_s1_temporal`` (``s1_temporal.hip``).

The rule (stated in ``include/instageo_hip.h``).  Every plane belongs to one group (one band on one pixel lattice) and one date, and sits
at an integer offset on its group's lattice.  A value is present when it is finite and differs from ``src_nodata``.  The local mean m of
a plane at a pixel is ``ig_s1_speckle``'s boxcar mean: the ``window`` x ``window`` neighbourhood (odd, 3..15) clipped to the plane, present
values only, float64 in a fixed order.  At a lattice pixel the dates are walked in order; the value of a date is that of its first member
(orbit slice) that covers the pixel and is present there; where that member's m > 0 the date adds x / m to R and 1 to c.  A present
centre of plane k with m_k > 0 and c >= 1 becomes y = m_k (R / c); any other present centre passes through (y = x_k); an absent centre
stays NaN.  ``scale="db"`` writes 10 log10 y where y > 0 and NaN (a DROPPED pixel) elsewhere.  On D dates of uncorrelated speckle and a
window of N pixels the equivalent number of looks rises by D N / (D + N - 1), and no pixel is blurred.

Device tensors go through ``ig_s1_temporal``; host arrays take a numpy twin of the same rule, so the module works (and is tested) without
a GPU.  The linear scale uses correctly rounded operations only: both paths write the same bytes.  ``log10`` is each side's library
function, so dB values may differ in the last float32 bit.

Not done: dates on different lattices or coordinate systems (warp them first: such files land in groups of their own and come back
unfiltered, listed as ``alone``), a Lee, refined Lee (``s1_filter``'s edge-aligned window) or other estimator in place of the boxcar mean, the vv / vh ratio band, host tiling of a group
that exceeds ``max_bytes``.
"""
from __future__ import annotations

import json
import os
from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import crs as crsmod
from . import prep, tiff, warp
from . import s1_filter as F
from .prep import MAX_DATES, is_device, to_host

BANDS = ("vv", "vh")
MAX_MEMBERS = 64  # planes of one group (include/instageo_hip.h)
TILE_W, TILE_H = 64, 32  # the lattice tile of one workgroup of ig_s1_temporal (s1_temporal.hip)
LATTICE_TOL = 1e-6  # pixels: two files share a lattice when their origins differ by integers within this
_ROWS = 512  # rows of a lattice the host path works on at a time
_QNAN = np.array([0x7FC00000], dtype=np.uint32).view(np.float32)[0]


class Tables(NamedTuple):
    """What ``ig_s1_temporal`` wants next to the planes (include/instageo_hip.h)."""

    place: np.ndarray  # (N, 3) int32: row0, col0, date
    lattice: np.ndarray  # (G, 2) int32: H_g, W_g
    member_ptr: np.ndarray  # (G + 1,) int32
    members: np.ndarray  # (N,) int32: the planes of group 0, then of group 1, ...; by date, then by the order given
    tile_ptr: np.ndarray  # (G + 1,) int64
    ids: np.ndarray  # (G,) the callers' group ids, ascending


# ---- argument checks shared by the host path and the device wrapper (ops.s1_temporal) ------------------------------------------------------
def _ints(a, shape, what: str) -> np.ndarray:
    a = np.asarray(a)
    if a.size and a.dtype.kind not in "iu":
        raise ValueError(f"{what} must be integers")
    a = a.astype(np.int64)
    if a.size != int(np.prod(shape)):
        raise ValueError(f"{what}: {shape[0]} planes need {int(np.prod(shape))} values (got {a.size})")
    a = a.reshape(shape)
    if (a < 0).any() or (a > 2**31 - 1).any():
        raise ValueError(f"{what} must lie in [0, 2^31 - 1]")
    return a


def check_temporal(size: int, starts, sizes, group, date, offsets, window, src_nodata, scale):
    """ValueError unless the arguments of a run obey include/instageo_hip.h -> (starts int64 (N,), sizes int32 (N, 2), h, src_nodata
    float32 or None, to_db 0 | 1, :class:`Tables`).  ``group`` (N,) names every plane's group (any ints >= 0), ``date`` (N,) its date
    index, ``offsets`` (N, 2) its (row0, col0) >= 0 on the group's lattice, which is the union of its members' extents.  The planes obey
    ``s1_filter.check_speckle``; a group holds at most 64 planes and ``MAX_DATES`` dates and its lattice at most 2^31 - 1 pixels."""
    st, ss, h, _, _, snd, to_db = F.check_speckle(size, starts, sizes, window, "boxcar", F.LOOKS, src_nodata, scale)
    N = st.shape[0]
    grp, dt, off = _ints(group, (N,), "group"), _ints(date, (N,), "date"), _ints(offsets, (N, 2), "offsets")
    ids, gi = np.unique(grp, return_inverse=True)
    G = ids.shape[0]
    end = off + ss.astype(np.int64)
    lattice = np.zeros((G, 2), dtype=np.int64)
    np.maximum.at(lattice, gi, end)
    if (lattice > 2**31 - 1).any() or (lattice[:, 0] * lattice[:, 1] > 2**31 - 1).any():
        raise ValueError("a group's lattice, the union of its planes' extents, holds at most 2^31 - 1 pixels")
    members = np.lexsort((np.arange(N), dt, gi)).astype(np.int32)  # by group, then date, then the order given
    per = np.bincount(gi, minlength=G) if N else np.zeros(0, dtype=np.int64)
    if (per > MAX_MEMBERS).any():
        raise ValueError(f"a group holds at most {MAX_MEMBERS} planes (got {int(per.max())})")
    member_ptr = np.concatenate([[0], np.cumsum(per)]).astype(np.int32)
    for g in range(G):
        if np.unique(dt[members[member_ptr[g] : member_ptr[g + 1]]]).shape[0] > MAX_DATES:
            raise ValueError(f"a group holds at most {MAX_DATES} dates")
    place = np.ascontiguousarray(np.concatenate([off, dt[:, None]], axis=1), dtype=np.int32)
    tiles = ((lattice[:, 0] + TILE_H - 1) // TILE_H) * ((lattice[:, 1] + TILE_W - 1) // TILE_W)
    tile_ptr = np.concatenate([[0], np.cumsum(tiles)]).astype(np.int64)
    if int(tile_ptr[-1]) > 2**31 - 1:
        raise ValueError("the lattices hold more than 2^31 - 1 tiles")
    return st, ss, h, snd, to_db, Tables(place, lattice.astype(np.int32), member_ptr, members, tile_ptr, ids)


# ---- the rule on host arrays ---------------------------------------------------------------------------------------------------------------
def _local_mean(src: np.ndarray, r0: int, r1: int, h: int, snd) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Rows r0..r1 of the plane ``src`` -> (m float64, present bool, x float64): the boxcar mean of ``ig_s1_speckle`` in its order, a Python
    loop over the window's offsets.  ``m`` means something where ``present`` only."""
    H, W = src.shape
    rows, w = r1 - r0, 2 * h + 1
    lo, hi = max(r0 - h, 0), min(r1 + h, H)
    P = np.full((rows + 2 * h, W + 2 * h), np.nan, dtype=np.float32)
    blk = src[lo:hi]
    absent = ~np.isfinite(blk)
    if snd is not None:
        absent |= blk == snd
    P[lo - (r0 - h) : hi - (r0 - h), h : h + W] = np.where(absent, np.float32(np.nan), blk)
    pres = ~np.isnan(P)
    Z = np.where(pres, P, np.float32(0)).astype(np.float64)  # an absent value adds +0.0, which changes no bit of a sum that began at +0.0
    Ai = np.zeros((rows + 2 * h, W), dtype=np.float64)
    Ki = np.zeros((rows + 2 * h, W), dtype=np.int64)
    for j in range(w):  # left to right
        Ai += Z[:, j : j + W]
        Ki += pres[:, j : j + W]
    A = np.zeros((rows, W), dtype=np.float64)
    n = np.zeros((rows, W), dtype=np.int64)
    for i in range(w):  # top to bottom
        A += Ai[i : i + rows]
        n += Ki[i : i + rows]
    centre = pres[h : h + rows, h : h + W]
    return A / np.where(centre, n, 1).astype(np.float64), centre, Z[h : h + rows, h : h + W]


def _temporal_host(planes, st, ss, h, snd, to_db, T: Tables):
    """numpy twin of ``ig_s1_temporal``: group by group, ``_ROWS`` lattice rows at a time, vectorised over the pixels, the members in the
    rule's order."""
    out = np.zeros(planes.shape[0], dtype=np.float32)
    counts = np.zeros((st.shape[0], 4), dtype=np.int32)
    for g in range(T.lattice.shape[0]):
        Hg, Wg = int(T.lattice[g, 0]), int(T.lattice[g, 1])
        mem = [int(p) for p in T.members[T.member_ptr[g] : T.member_ptr[g + 1]]]
        for R0 in range(0, Hg, _ROWS):
            R1 = min(R0 + _ROWS, Hg)
            Rsum = np.zeros((R1 - R0, Wg), dtype=np.float64)
            c = np.zeros((R1 - R0, Wg), dtype=np.int64)
            last = np.full((R1 - R0, Wg), -1, dtype=np.int64)
            kept = []
            for p in mem:  # sweep 1: the ratio sum
                H, W = int(ss[p, 0]), int(ss[p, 1])
                row0, col0, d = (int(v) for v in T.place[p])
                a0, a1 = max(R0, row0), min(R1, row0 + H)
                if a0 >= a1:
                    continue
                src = planes[int(st[p]) : int(st[p]) + H * W].reshape(H, W)
                m, pres, x = _local_mean(src, a0 - row0, a1 - row0, h, snd)
                win = (slice(a0 - R0, a1 - R0), slice(col0, col0 + W))
                take = pres & (last[win] != d)  # the first present member of its date decides for the date
                last[win][take] = d
                add = take & (m > 0)
                with np.errstate(all="ignore"):
                    r = x / np.where(add, m, 1.0)
                Rsum[win][add] += r[add]
                c[win][add] += 1
                kept.append((p, win, a0 - row0, a1 - row0, m, pres, x))
            for p, win, p0, p1, m, pres, x in kept:  # sweep 2: the outputs
                H, W = int(ss[p, 0]), int(ss[p, 1])
                cv = c[win]
                ok = pres & (m > 0) & (cv >= 1)
                with np.errstate(all="ignore"):
                    y = np.where(ok, m * (Rsum[win] / np.where(cv >= 1, cv, 1).astype(np.float64)), x)
                    if to_db:
                        keep = pres & (y > 0)
                        val = (10.0 * np.log10(np.where(keep, y, 1.0))).astype(np.float32)
                    else:
                        keep = pres
                        val = y.astype(np.float32)
                out[int(st[p]) : int(st[p]) + H * W].reshape(H, W)[p0:p1] = np.where(keep, val, _QNAN)
                counts[p] += (int(keep.sum()), int((pres & ~keep).sum()), int((pres & ~ok).sum()), int((keep & (cv == 1)).sum()))
    return out, counts


def temporal(planes, starts, sizes, group, date, offsets, window: int = 7, src_nodata: Optional[float] = None, scale: str = "linear"):
    """The packed float32 planes ``planes`` (1-D; plane p of ``sizes[p]`` = (H, W) at element ``starts[p]``, in group ``group[p]``, of date
    ``date[p]``, at ``offsets[p]`` = (row0, col0) on its group's lattice) filtered by the rule of the module docstring -> (out: float32
    with the layout of ``planes``, absent and dropped pixels NaN, elements outside every plane 0; counts (N, 4) int32: per plane the
    present outputs, the pixels the dB step dropped, the pixels passed through and the present outputs where only one date contributed).
    Planes of one group and date are tried in the order given.  A tensor on the device goes through ``ig_s1_temporal`` and gives device
    tensors; anything else takes the numpy twin and gives arrays."""
    dev = is_device(planes)
    if not dev:
        planes = to_host(planes)
    if str(planes.dtype).replace("torch.", "") != "float32" or planes.ndim != 1:
        raise ValueError("the planes are one packed 1-D float32 buffer")
    if dev:
        from . import ops

        return ops.s1_temporal(planes, starts, sizes, group, date, offsets, window, src_nodata, scale)  # checks the same arguments before the upload
    st, ss, h, snd, to_db, T = check_temporal(planes.shape[0], starts, sizes, group, date, offsets, window, src_nodata, scale)
    return _temporal_host(planes, st, ss, h, snd, to_db, T)


# ---- files -> files -------------------------------------------------------------------------------------------------------------------------
def _near_int(v: float) -> bool:
    return abs(v - round(v)) <= LATTICE_TOL


def group_files(profiles: Sequence[Dict[str, Any]], shapes: Sequence[Tuple[int, int]], band_of: Sequence[int], names: Sequence[str]):
    """The files grouped per band by coordinate system and lattice -> [{"band", "files": [positions in order], "offsets": [(row0, col0)],
    "grid": (X0, Y0, sx, sy), "size": (H, W), "crs"}].  Two files share a lattice when their pixel scales are equal and their origins differ
    by whole pixels within ``LATTICE_TOL`` (float64 UTM coordinates carry about 1e-10 px of rounding at 10 m; a real misregistration is
    far larger); the group lattice is the union of the members' extents."""
    groups: List[Dict[str, Any]] = []
    for k, (prof, b) in enumerate(zip(profiles, band_of)):
        system = tuple(crsmod.from_profile(prof))[:5]
        X0, Y0, sx, sy = warp.grid_of(prof, names[k])
        for g in groups:
            if g["band"] == b and g["crs"] == system and g["ref"][2:] == (sx, sy) and _near_int((X0 - g["ref"][0]) / sx) and _near_int((Y0 - g["ref"][1]) / sy):
                break
        else:
            g = {"band": b, "crs": system, "ref": (X0, Y0, sx, sy), "files": [], "at": []}
            groups.append(g)
        g["files"].append(k)
        g["at"].append((int(round((g["ref"][1] - Y0) / sy)), int(round((X0 - g["ref"][0]) / sx))))  # rows grow southwards
    for g in groups:
        at = np.array(g["at"], dtype=np.int64)
        lo = at.min(axis=0)
        X0, Y0, sx, sy = g.pop("ref")
        g["offsets"] = [(int(r - lo[0]), int(c - lo[1])) for r, c in g.pop("at")]
        g["grid"] = (X0 + float(lo[1]) * sx, Y0 - float(lo[0]) * sy, sx, sy)
        g["size"] = (max(o[0] + shapes[k][0] for o, k in zip(g["offsets"], g["files"])), max(o[1] + shapes[k][1] for o, k in zip(g["offsets"], g["files"])))
    return groups


def filter_s1_temporal(scenes, output_directory: str, bands: Sequence[str] = BANDS, window: int = 7, scale: str = "linear",
                       src_nodata: Optional[float] = None, device: Optional[str] = None, max_bytes: int = 1 << 33):
    """Every single-band float32 GeoTIFF of ``scenes`` ([date][scene][band] files of ``len(bands)`` bands, the nesting ``s1_chips.scenes``
    takes; a date that is one flat list of files is one scene) filtered over the dates and written as a float32 GeoTIFF under the same
    base name in ``output_directory``, with the source's tiepoint, pixel scale and GeoKeys and NaN as its no-data.  The files are grouped per
    band by coordinate system and lattice (:func:`group_files`); they are neither warped nor refused: a file whose group holds one date is
    written with its input's values and listed in the stats as ``alone``.  The scenes of one date are tried in the order given.
    ``src_nodata``: None = each file's own no-data tag (a file without one: only what is not finite is absent).  A group goes to the
    device whole, several groups together while they fit ``max_bytes`` of input; a group beyond ``max_bytes`` raises ValueError.
    ``temporal_stats.json`` holds the settings, the groups (files, lattice, dates) and per file the four counts.  An output that would
    replace an input, or two inputs of one base name, raise ValueError before anything is written.  ``device``: None = the numpy path,
    ``"cuda"`` / ``"cuda:n"`` = the kernel.  -> the written paths in the nesting of ``scenes``."""
    from . import s1_chips as V

    check_temporal(0, [], [], [], [], [], window, src_nodata, scale)
    prep.check_device(device)
    if isinstance(max_bytes, bool) or not isinstance(max_bytes, (int, np.integer)) or max_bytes < 1:
        raise ValueError(f"max_bytes must be a positive int (got {max_bytes!r})")
    if isinstance(bands, str) or not bands or not all(isinstance(b, str) for b in bands):
        raise ValueError(f"bands is a list of at least one name (got {bands!r})")
    C = len(bands)
    dates = V._dates_of(scenes, C)
    if len(dates) > MAX_DATES:
        raise ValueError(f"{len(dates)} dates: at most {MAX_DATES} go into one stack")
    files: List[str] = []
    nest = F._flatten(scenes, files)  # the same files in the same order, with the nesting as it was given
    date_of = [d for d, scs in enumerate(dates) for s in scs for _ in s]
    band_of = [b for scs in dates for s in scs for b in range(C)]
    names = [os.path.join(output_directory, os.path.basename(f)) for f in files]
    if len({os.path.basename(f) for f in files}) != len(files):
        raise ValueError("two input files share a base name: their outputs would replace one another")
    ins = {os.path.realpath(f) for f in files}
    for n in names:
        if os.path.realpath(n) in ins:
            raise ValueError(f"{n}: the output would replace an input; choose another output_directory")
    # what every file needs, from its header: its lattice, its size and its own no-data value
    profiles = [tiff.read_profile(f) for f in files]
    shapes = [(int(p["height"]), int(p["width"])) for p in profiles]
    nodata = []
    for p in profiles:
        nd = src_nodata if src_nodata is not None else p.get("nodata")
        nodata.append(None if nd is None or nd != nd else float(np.float32(nd)))
    groups = group_files(profiles, shapes, band_of, files)
    for gi, g in enumerate(groups):
        g["bytes"] = 4 * sum(shapes[k][0] * shapes[k][1] for k in g["files"])
        label = f"group {gi} (band {bands[g['band']]}, {len(g['files'])} files from {os.path.basename(files[g['files'][0]])})"
        if len(g["files"]) > MAX_MEMBERS:
            raise ValueError(f"{label} holds more than {MAX_MEMBERS} files")
        if g["bytes"] > max_bytes:
            raise ValueError(f"{label} holds {g['bytes']} bytes, more than max_bytes = {max_bytes}: a group goes to the device whole")
    os.makedirs(output_directory, exist_ok=True)
    stats: Dict[str, Any] = {"window": int(window), "scale": scale, "src_nodata": None if src_nodata is None else float(src_nodata),
                             "bands": list(bands), "groups": [], "files": {}}
    k = 0
    while k < len(groups):
        e, held = k + 1, groups[k]["bytes"]  # a batch: consecutive groups inside the byte budget, at least one
        while e < len(groups) and held + groups[e]["bytes"] <= max_bytes:
            held += groups[e]["bytes"]
            e += 1
        idx = [f for g in groups[k:e] for f in g["files"]]
        planes, starts, shp, _ = prep.read_planes([files[f] for f in idx], "band", np.float32)
        nds = {nodata[f] for f in idx}
        nd = nodata[idx[0]]
        if len(nds) > 1:  # the kernel takes one value: files that disagree get their own value replaced by NaN, which is absent anyway
            nd = None
            for i, f in enumerate(idx):
                if nodata[f] is not None:
                    v = planes[int(starts[i]) : int(starts[i]) + shp[i][0] * shp[i][1]]
                    v[v == np.float32(nodata[f])] = np.nan
        grp = [gi for gi, g in enumerate(groups[k:e]) for _ in g["files"]]
        off = [o for g in groups[k:e] for o in g["offsets"]]
        out, counts = temporal(prep.to_device(planes, device), starts, shp, grp, [date_of[f] for f in idx], off, window, nd, scale)
        out, counts = to_host(out), to_host(counts)
        for gi, g in enumerate(groups[k:e]):
            alone = len({date_of[f] for f in g["files"]}) == 1
            stats["groups"].append({"band": bands[g["band"]], "files": [os.path.basename(files[f]) for f in g["files"]],
                                    "dates": [date_of[f] for f in g["files"]], "offsets": [list(o) for o in g["offsets"]],
                                    "lattice": {"grid": list(g["grid"]), "height": g["size"][0], "width": g["size"][1], "crs": list(g["crs"])},
                                    "alone": alone})
        for i, f in enumerate(idx):
            H, W = shp[i]
            tags = prep.geo_tags(profiles[f]["tags"], tiepoint=True)
            tags[F.NODATA_TAG] = (2, "nan")
            tiff.write(names[f], out[int(starts[i]) : int(starts[i]) + H * W].reshape(H, W), {"tags": tags, "nodata": None})
            stats["files"][os.path.basename(names[f])] = {"pixels": H * W, "present": int(counts[i, 0]), "dropped": int(counts[i, 1]),
                                                          "passed": int(counts[i, 2]), "single": int(counts[i, 3]), "src_nodata": nodata[f],
                                                          "group": k + grp[i], "date": date_of[f], "alone": stats["groups"][k + grp[i]]["alone"]}
        k = e
    prep.write_stats(os.path.join(output_directory, "temporal_stats.json"), stats)
    return F._rebuild(nest, names)


# ---- mode=filter_s1_temporal ---------------------------------------------------------------------------------------------------------------
CONFIG_KEYS = ("scenes", "output_directory", "bands", "window", "scale", "src_nodata")


def s1_temporal_options(cfg: Dict[str, Any]) -> Dict[str, Any]:
    """The ``s1_temporal.*`` keys of ``mode=filter_s1_temporal`` checked -> the keyword arguments of :func:`filter_s1_temporal`.  A bad
    value raises ValueError; ``scenes`` and ``output_directory`` are required only in that mode."""
    from . import s1_chips as V

    c = prep.Section(cfg, "s1_temporal", CONFIG_KEYS)
    bands = c.listing("bands", list(BANDS))
    if not bands:
        raise c.bad("bands", "must be a list of at least one name", bands)
    scale = c.choice("scale", "linear", F.SCALES)
    window = c.integer("window", 7, lo=3, hi=2 * F.MAX_HALF + 1, what=f"must be an odd int in [3, {2 * F.MAX_HALF + 1}]")
    if window % 2 == 0:
        raise c.bad("window", f"must be an odd int in [3, {2 * F.MAX_HALF + 1}]", window)
    snd = c.get("src_nodata")
    if snd is not None:
        snd = c.number("src_nodata", None, lambda v: v == v, "must be None or a number that is not NaN")
    scenes = c.get("scenes")
    if scenes is not None:
        try:
            dates = V._dates_of(scenes, len(bands))
        except ValueError as e:
            raise c.bad("scenes", f"must be a list of dates of scenes of {len(bands)} band files ({e})", scenes) from None
        if len(dates) > MAX_DATES:
            raise c.bad("scenes", f"holds at most {MAX_DATES} dates", scenes)
    out = c.text("output_directory")
    if cfg.get("mode") == "filter_s1_temporal" and (not scenes or out is None):
        raise ValueError("mode=filter_s1_temporal needs s1_temporal.scenes and s1_temporal.output_directory")
    return dict(scenes=scenes, output_directory=out, bands=bands, window=window, scale=scale, src_nodata=snd)


def run_from_config(cfg: Dict[str, Any], device: Optional[str] = None) -> int:
    """``mode=filter_s1_temporal``: :func:`filter_s1_temporal` under the ``s1_temporal.*`` keys; prints one JSON line."""
    kw = s1_temporal_options(cfg)
    written: List[str] = []
    F._flatten(filter_s1_temporal(device=device, **kw), written)
    with open(os.path.join(kw["output_directory"], "temporal_stats.json")) as f:
        stats = json.load(f)
    per = stats["files"]
    print(json.dumps({"filter_s1_temporal": {"files": len(written), "groups": len(stats["groups"]), "alone": sum(v["alone"] for v in per.values()),
                                             "present": sum(v["present"] for v in per.values()), "dropped": sum(v["dropped"] for v in per.values()),
                                             "output_directory": kw["output_directory"]}}))
    return 0


def main(argv: Optional[List[str]] = None) -> int:
    """``python -m instageo_amd.s1_temporal s1_temporal.scenes=[[[a_vv.tif,a_vh.tif]],[[b_vv.tif,b_vh.tif]]] s1_temporal.output_directory=out
    ...``: mode=filter_s1_temporal without ``run.py``."""
    return prep.run_mode_cli("filter_s1_temporal", run_from_config, argv)


if __name__ == "__main__":
    raise SystemExit(main())
