"""Spatially blocked train / val / test splitting of a chip dataset, with a leakage audit and a guard band, on the device.

The data-preparation modes end in a dataset CSV (``Input`` / ``Label``); training starts from ``train_filepath`` / ``valid_filepath`` /
``test_filepath``.  The reference makes the three files in ``instageo/data/data_splitter.py``: k-means over scaled longitude / latitude
(sklearn), whole clusters handed to the sets, maps drawn with cartopy; it never checks what it produced.  This module is the stand-in, on a
rule of its own that needs none of those packages, on top of :mod:`instageo_amd.tiff`, :mod:`instageo_amd.crs` and the kernels of
``split.hip``.

The rule (stated in ``include/instageo_hip.h``).  The location of a row is the centre of its ``Input`` GeoTIFF's grid, from the file's
profile alone, as longitude / latitude in float64; its position is the unit vector quantised to int32 at 2^29 per unit (about 1.2 cm);
the distance of two positions is the squared chord d2 as a 64-bit integer, so the antimeridian and the poles are no special case and every
comparison is exact.  ``strategy=kmeans``: spherical k-means from farthest-point initial centres, one ``ig_split_assign`` launch per
Lloyd round (nearest centre, ties to the smallest index; per-centre int64 coordinate sums and counts; the number of changed assignments),
the centre update in float64 on the host; whole clusters go to test (seeded by the most recent cluster, grown by nearest centre), then to
val (seeded by the generator), the rest is train.  ``strategy=year``: whole years, the most recent to test.  ``strategy=random``: a
permutation -- the baseline the audit is meant to expose.  For every strategy the audit finds, per train row, the nearest val or test row
and, per val row, the nearest test row (``ig_split_nearest``: Na x Nb exact integer distances); ``buffer_km > 0`` removes the train rows
nearer than that to val or test, then the val rows nearer than that to test.

Device tensors go through ``ig_split_assign`` / ``ig_split_nearest``; host arrays take numpy twins that give the same arrays, so the
module works (and is tested) without a GPU, and both paths write the same bytes.

Not done: the reference's MGRS-proximity grouping, ``allow_group_overlap``, PNG maps (``splits.geojson`` stands in for them),
stratification by class histogram.
"""
from __future__ import annotations

import json
import os
import re
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import crs as crsmod
from . import prep, tiff, warp
from .prep import is_device, to_host

SCALE = 1 << 29  # int32 units per unit of the sphere's radius
EARTH_KM = 6371.0088  # the mean radius
MAX_CLUSTERS = 256
MAX_POINTS = 1 << 30
STRATEGIES = ("kmeans", "year", "random")
SETS = ("train", "val", "test")
TRAIN, VAL, TEST = 0, 1, 2
_YEAR = re.compile(r"(19[0-9]{2}|20[0-9]{2})")  # the reference's extract_year


# ---- argument checks shared by the host twins and the device wrappers (ops.split_assign / split_nearest) -------------------------------------
def check_points(shape, dtype: str, what: str) -> int:
    """ValueError unless ``shape`` / ``dtype`` describe (N, 3) int32 positions with N < 2^30 -> N."""
    if len(shape) != 2 or shape[1] != 3 or dtype != "int32":
        raise ValueError(f"{what} is (N, 3) int32 (got shape {tuple(shape)}, {dtype})")
    if shape[0] >= MAX_POINTS:
        raise ValueError(f"{what}: {shape[0]} points are beyond 2^30 - 1")
    return int(shape[0])


def check_assign(pts_shape, pts_dtype: str, centres: np.ndarray, assign_shape, assign_dtype: str) -> Tuple[int, int]:
    """ValueError unless the arguments of one Lloyd round obey include/instageo_hip.h (``centres`` is a host array: its values are
    checked too) -> (N, K)."""
    N = check_points(pts_shape, pts_dtype, "pts")
    K = check_points(centres.shape, centres.dtype.name, "centres")
    if not 1 <= K <= MAX_CLUSTERS:
        raise ValueError(f"need 1 <= K <= {MAX_CLUSTERS} centres (got {K})")
    if np.abs(centres.astype(np.int64)).max() > SCALE:
        raise ValueError("centres must be quantised unit vectors: |coordinate| <= 2^29")
    if tuple(assign_shape) != (N,) or assign_dtype != "int32":
        raise ValueError(f"assign is (N,) = ({N},) int32 (got shape {tuple(assign_shape)}, {assign_dtype})")
    return N, K


def check_nearest(a_shape, a_dtype: str, b_shape, b_dtype: str) -> Tuple[int, int]:
    """ValueError unless ``a`` and ``b`` are position arrays and ``b`` holds at least one row -> (Na, Nb)."""
    Na, Nb = check_points(a_shape, a_dtype, "a"), check_points(b_shape, b_dtype, "b")
    if Nb < 1:
        raise ValueError("b needs at least one row to search (got 0)")
    return Na, Nb


def _check_range(a: np.ndarray, what: str) -> None:
    if a.size and np.abs(a.astype(np.int64)).max() > SCALE:
        raise ValueError(f"{what} must be quantised unit vectors: |coordinate| <= 2^29")


# ---- positions and distances ---------------------------------------------------------------------------------------------------------------
def quantise_vectors(v) -> np.ndarray:
    """Unit vectors (N, 3) float64 -> int32 positions: every component times 2^29, rounded half to even."""
    return np.rint(np.asarray(v, dtype=np.float64) * float(SCALE)).astype(np.int32).reshape(-1, 3)


def quantise(lon, lat) -> np.ndarray:
    """Longitude / latitude in degrees -> (N, 3) int32 positions (cos lat cos lon, cos lat sin lon, sin lat) * 2^29."""
    lam, phi = np.radians(np.asarray(lon, dtype=np.float64)).reshape(-1), np.radians(np.asarray(lat, dtype=np.float64)).reshape(-1)
    return quantise_vectors(np.stack((np.cos(phi) * np.cos(lam), np.cos(phi) * np.sin(lam), np.sin(phi)), axis=-1))


def km(d2) -> np.ndarray:
    """Squared chords (integers, any integer dtype) -> great-circle kilometres in float64: 2 R asin(sqrt(d2) / 2^30)."""
    half = np.sqrt(np.asarray(d2).astype(np.uint64).astype(np.float64)) / float(1 << 30)
    return 2.0 * EARTH_KM * np.arcsin(np.minimum(half, 1.0))


def _d2(p: np.ndarray, q: np.ndarray) -> np.ndarray:
    """(n, 3) x (m, 3) int32 -> (n, m) uint64 squared distances (at most 3 * 2^60: exact in int64 too)."""
    d = p.astype(np.int64)[:, None, :] - q.astype(np.int64)[None, :, :]
    return (d * d).sum(axis=-1).view(np.uint64)


# ---- the two kernels' numpy twins ----------------------------------------------------------------------------------------------------------
def _assign_host(pts: np.ndarray, centres: np.ndarray, assign: np.ndarray, block: int = 8192):
    """numpy twin of ``ig_split_assign`` -> (the new assignment, sums (K, 4) int64, changed (1,) int32); ``assign`` is left alone."""
    N, K = pts.shape[0], centres.shape[0]
    new = np.empty(N, dtype=np.int32)
    for s in range(0, N, block):
        new[s : s + block] = _d2(pts[s : s + block], centres).argmin(axis=1)  # the first minimum: the smallest centre index
    sums = np.zeros((K, 4), dtype=np.int64)
    np.add.at(sums[:, :3], new, pts.astype(np.int64))
    sums[:, 3] = np.bincount(new, minlength=K)
    return new, sums, np.array([(new != assign).sum()], dtype=np.int32)


def _nearest_host(a: np.ndarray, b: np.ndarray, rows: int = 256, cols: int = 4096):
    """numpy twin of ``ig_split_nearest``, block by block (rows x cols distances at a time) -> (d2 (Na,) uint64, idx (Na,) int32)."""
    Na = a.shape[0]
    best, idx = np.full(Na, np.iinfo(np.uint64).max, dtype=np.uint64), np.zeros(Na, dtype=np.int32)
    for r in range(0, Na, rows):
        bd, bi = best[r : r + rows], idx[r : r + rows]  # views
        for c in range(0, b.shape[0], cols):
            d = _d2(a[r : r + rows], b[c : c + cols])
            j = d.argmin(axis=1)  # the first minimum of the block: its smallest index
            dj = d[np.arange(d.shape[0]), j]
            win = dj < bd  # strict: an earlier block keeps a tie
            bd[win], bi[win] = dj[win], (j[win] + c).astype(np.int32)
    return best, idx


# ---- building blocks on arrays and tensors -------------------------------------------------------------------------------------------------
def assign_round(pts, centres, assign, check_range: bool = True):
    """One Lloyd round: ``pts`` (N, 3) int32, ``centres`` (K, 3) int32 (a host array), ``assign`` (N,) int32: the previous assignment
    -> (assign, sums (K, 4) int64, changed (1,) int32).  Tensors on the device go through ``ig_split_assign`` (``assign`` is overwritten
    and returned) and give device tensors; anything else takes the numpy twin and gives arrays.  ``check_range=False`` skips the check of
    |coordinate| <= 2^29 over ``pts`` (a caller that quantised them itself)."""
    if is_device(pts):
        from . import ops

        sums, changed = ops.split_assign(pts, centres, assign, check_range)
        return assign, sums, changed
    p, c, a = to_host(pts), np.ascontiguousarray(to_host(centres)), to_host(assign)
    check_assign(p.shape, p.dtype.name, c, a.shape, a.dtype.name)
    if check_range:
        _check_range(p, "pts")
    return _assign_host(p, c, a)


def nearest(a, b):
    """Per row of ``a`` (Na, 3) int32 the squared distance to the nearest row of ``b`` (Nb, 3) int32 and the smallest index that attains
    it -> (d2 (Na,), idx (Na,) int32).  Tensors on the device go through ``ig_split_nearest`` (d2 int64: the same bits, at most
    3 * 2^60); anything else takes the blockwise numpy twin (d2 uint64)."""
    if is_device(a):
        from . import ops

        return ops.split_nearest(a, b)
    p, q = to_host(a), to_host(b)
    check_nearest(p.shape, p.dtype.name, q.shape, q.dtype.name)
    _check_range(p, "a"), _check_range(q, "b")
    return _nearest_host(p, q)


def initial_centres(pts: np.ndarray, n_clusters: int, rng) -> np.ndarray:
    """Farthest-point centres (host): the point at ``rng.integers(N)``, then always the point with the largest d2 to its nearest chosen
    centre (the smallest index among equals), for K = min(n_clusters, the number of distinct positions) centres -> (K, 3) int32."""
    N = pts.shape[0]
    K = min(int(n_clusters), np.unique(pts, axis=0).shape[0])
    first = int(rng.integers(N))
    chosen = [first]
    near = _d2(pts, pts[first : first + 1])[:, 0]
    while len(chosen) < K:
        nxt = int(near.argmax())  # the first maximum
        chosen.append(nxt)
        near = np.minimum(near, _d2(pts, pts[nxt : nxt + 1])[:, 0])
    return np.ascontiguousarray(pts[chosen])


def update_centres(centres: np.ndarray, sums: np.ndarray) -> np.ndarray:
    """The centres after a round (host, float64): the mean vector of every centre's points, normalised to unit length and quantised; an
    empty centre, or one whose mean vector is zero, keeps its position."""
    s = sums.astype(np.int64)
    cnt = s[:, 3].astype(np.float64)
    with np.errstate(all="ignore"):
        mean = s[:, :3].astype(np.float64) / cnt[:, None]
        norm = np.sqrt(mean[:, 0] * mean[:, 0] + mean[:, 1] * mean[:, 1] + mean[:, 2] * mean[:, 2])  # in this order
        ok = (s[:, 3] > 0) & (norm > 0)
        new = quantise_vectors(np.where(ok[:, None], mean / norm[:, None], 0.0))
    return np.ascontiguousarray(np.where(ok[:, None], new, centres).astype(np.int32))


def kmeans(pts, n_clusters: int = 20, rng=None, max_iter: int = 100, device: Optional[str] = None):
    """Spherical k-means of ``pts`` (N, 3) int32 host positions, N >= 1, by the rule of the module docstring -> (assign (N,) int32,
    centres (K, 3) int32, sizes (K,) int64, rounds), host arrays.  ``rng``: the generator that picks the first centre (None:
    ``default_rng(42)``); ``device``: None = the numpy twin, ``"cuda"`` = one ``ig_split_assign`` launch per round."""
    p = np.ascontiguousarray(to_host(pts))
    N = check_points(p.shape, p.dtype.name, "pts")
    if N < 1:
        raise ValueError("k-means needs at least one point")
    if isinstance(n_clusters, bool) or not 1 <= int(n_clusters) <= MAX_CLUSTERS:
        raise ValueError(f"n_clusters must lie in [1, {MAX_CLUSTERS}] (got {n_clusters!r})")
    if isinstance(max_iter, bool) or int(max_iter) < 1:
        raise ValueError(f"max_iter must be at least 1 (got {max_iter!r})")
    _check_range(p, "pts")
    prep.check_device(device)
    centres = initial_centres(p, n_clusters, np.random.default_rng(42) if rng is None else rng)
    work = prep.to_device(p, device)
    assign = prep.to_device(np.full(N, -1, dtype=np.int32), device)
    sizes, rounds = np.zeros(centres.shape[0], dtype=np.int64), 0
    while rounds < int(max_iter):
        assign, sums, changed = assign_round(work, centres, assign, check_range=False)
        rounds += 1
        sums = to_host(sums)
        sizes = sums[:, 3].astype(np.int64)
        if int(to_host(changed)[0]) == 0:
            break
        centres = update_centres(centres, sums)
    return to_host(assign).astype(np.int32), centres, sizes, rounds


def extract_year(path: str) -> Optional[int]:
    """The first 19xx | 20xx in the file name, as the reference's ``extract_year``; None without one."""
    m = _YEAR.search(os.path.basename(str(path)))
    return int(m.group(1)) if m else None


def _grow(seed: int, target: int, free: List[int], sizes: np.ndarray, centres: np.ndarray) -> List[int]:
    """Clusters taken from ``free`` (ascending indices) until they hold ``target`` rows: ``seed`` first, then always the free cluster whose
    centre is nearest to any taken centre (the smallest index among equals)."""
    taken: List[int] = []
    rows, nxt = 0, seed
    while rows < target and free:
        free.remove(nxt)
        taken.append(nxt)
        rows += int(sizes[nxt])
        if free:
            d = _d2(centres[free], centres[taken]).min(axis=1)
            nxt = free[int(d.argmin())]
    return taken


def assign_sets(sizes, centres, N: int, test_ratio: float = 0.2, val_ratio: float = 0.2, include_test: bool = True, include_val: bool = True,
                mean_year=None, rng=None) -> np.ndarray:
    """Clusters to sets by the rule of the module docstring: ``sizes`` (K,) rows per cluster, ``centres`` (K, 3) int32, ``mean_year`` (K,)
    float64 or None (not every row has a year), ``rng``: the generator of :func:`kmeans`, after it -> (K,) int8: 0 train, 1 val, 2 test.
    ValueError when test or val would take every cluster, or when none is left for train."""
    sizes, centres = np.asarray(sizes, dtype=np.int64), np.asarray(centres, dtype=np.int32)
    K = sizes.shape[0]
    sets = np.zeros(K, dtype=np.int8)
    free = list(range(K))
    rng = np.random.default_rng(42) if rng is None else rng
    for code, on, ratio in ((TEST, include_test, test_ratio), (VAL, include_val, val_ratio)):
        if not on:
            continue
        target = int(np.floor(N * float(ratio)))
        if not free:
            raise ValueError(f"no cluster is left for {SETS[code]}: lower the ratios or raise n_clusters")
        if code == TEST:
            seed = int(np.where(sizes > 0, mean_year, -np.inf).argmax()) if mean_year is not None else 0
        else:
            seed = free[int(rng.integers(len(free)))]
        taken = _grow(seed, target, free, sizes, centres)
        if len(taken) == K:
            raise ValueError(f"{SETS[code]} would take every one of the {K} clusters: lower {SETS[code]}_ratio or raise n_clusters")
        sets[taken] = code
    if not free:
        raise ValueError("no cluster is left for train: lower the ratios or raise n_clusters")
    return sets


def _by_year(years: np.ndarray, N: int, test_ratio: float, val_ratio: float, include_test: bool, include_val: bool) -> np.ndarray:
    """``strategy=year`` -> the set of every row: the most recent years to test until its target is reached, the next to val, the rest to
    train; a year is never cut and every set keeps at least one."""
    distinct = sorted(set(int(y) for y in years), reverse=True)
    wanted = 1 + bool(include_test) + bool(include_val)
    if len(distinct) < wanted:
        raise ValueError(f"strategy=year needs at least {wanted} distinct years for {wanted} sets (got {len(distinct)})")
    sets = np.zeros(N, dtype=np.int8)
    left = wanted - 1  # sets still to be served after the current one
    for code, on, ratio in ((TEST, include_test, test_ratio), (VAL, include_val, val_ratio)):
        if not on:
            continue
        target, rows = int(np.floor(N * float(ratio))), 0
        while rows < target and len(distinct) > left:
            sel = years == distinct.pop(0)
            sets[sel], rows = code, rows + int(sel.sum())
        left -= 1
    return sets


# ---- files -> files -------------------------------------------------------------------------------------------------------------------------
def locations(csv: str, root_dir: Optional[str] = None):
    """The dataset CSV ``csv`` (an ``Input`` column; relative paths start at ``root_dir``, None: the CSV's folder) -> (the table, lon (n,),
    lat (n,) float64).  The location of a row is the centre of its file's grid, from the profile alone (``tiff.read_profile``,
    ``crs.from_profile``, ``crs.inverse``); NaN where the file has no georeferencing or the centre lies outside its projection."""
    import pandas as pd

    df = pd.read_csv(csv)
    if "Input" not in df.columns:
        raise ValueError("CSV must contain an 'Input' column")
    root = root_dir if prep.none(root_dir) is not None else os.path.dirname(os.path.abspath(csv))
    n = len(df)
    x, y, code = np.full(n, np.nan), np.full(n, np.nan), np.zeros(n, dtype=np.int64)
    systems: Dict[int, Any] = {}
    for i, p in enumerate(str(v) for v in df["Input"]):
        prof = tiff.read_profile(p if os.path.isabs(p) else os.path.join(root, p))
        try:
            c = crsmod.from_profile(prof)
            X0, Y0, sx, sy = warp.grid_of(prof, p)
        except ValueError:
            continue
        systems[c.epsg] = c
        x[i], y[i], code[i] = X0 + sx * prof["width"] / 2.0, Y0 - sy * prof["height"] / 2.0, c.epsg
    lon, lat = np.full(n, np.nan), np.full(n, np.nan)
    for epsg, c in systems.items():
        sel = code == epsg
        lon[sel], lat[sel] = crsmod.inverse(c, x[sel], y[sel])
    return df, lon, lat


def _audit(pos: np.ndarray, sets: np.ndarray, buffer_km: float, device) -> Tuple[Dict[str, Any], np.ndarray, np.ndarray]:
    """The nearest-row search train -> (val u test) and val -> test over the rows of ``pos`` with their ``sets`` -> (the report per pair,
    km of every train row to its nearest val or test row (inf without one), km of every val row to its nearest test row)."""
    report: Dict[str, Any] = {}
    out = []
    for name, src, dst in (("train_to_heldout", sets == TRAIN, sets != TRAIN), ("val_to_test", sets == VAL, sets == TEST)):
        dist = np.full(int(src.sum()), np.inf)
        if src.any() and dst.any():
            d2, _ = nearest(prep.to_device(np.ascontiguousarray(pos[src]), device), prep.to_device(np.ascontiguousarray(pos[dst]), device))
            dist = km(to_host(d2))
        have = dist.size > 0 and bool(np.isfinite(dist).all())
        report[name] = {"rows": int(src.sum()), "against": int(dst.sum()), "min_km": float(dist.min()) if have else None,
                        "median_km": float(np.median(dist)) if have else None, "within_buffer": int((dist < buffer_km).sum())}
        out.append(dist)
    return report, out[0], out[1]


def split_dataset(input_file: str, output_dir: str, test_ratio: float = 0.2, val_ratio: float = 0.2, include_val: bool = True,
                  include_test: bool = True, random_state: int = 42, n_clusters: int = 20, strategy: str = "kmeans", buffer_km: float = 0.0,
                  max_iter: int = 100, root_dir: Optional[str] = None, save_geojson: bool = True, device: Optional[str] = None) -> Dict[str, Any]:
    """Split the dataset CSV ``input_file`` by the rule of the module docstring and write, under ``output_dir``, ``splits/train.csv`` /
    ``val.csv`` / ``test.csv`` (every column of the input, rows in input order; a skipped set writes no file), ``dropped.csv`` (the rows
    left out, with a ``reason``: ``no_location`` | ``buffer``), ``split_stats.json`` and ``splits.geojson`` (one Point per located row with
    ``row``, ``set``, ``cluster`` and ``year``).  -> the stats.  ``device``: None = the numpy path, ``"cuda"`` / ``"cuda:n"`` = the
    kernels; both write the same bytes.  Errors raise."""
    if strategy not in STRATEGIES:
        raise ValueError(f"strategy must be one of {STRATEGIES} (got {strategy!r})")
    for name, v in (("test_ratio", test_ratio), ("val_ratio", val_ratio)):
        if isinstance(v, bool) or not 0.0 <= float(v) < 1.0:
            raise ValueError(f"{name} must lie in [0, 1) (got {v!r})")
    if (float(test_ratio) if include_test else 0.0) + (float(val_ratio) if include_val else 0.0) >= 1.0:
        raise ValueError("test_ratio + val_ratio must stay below 1: nothing would be left for train")
    if isinstance(buffer_km, bool) or not 0.0 <= float(buffer_km) < float("inf"):
        raise ValueError(f"buffer_km must be a finite distance >= 0 (got {buffer_km!r})")
    if isinstance(n_clusters, bool) or not 1 <= int(n_clusters) <= MAX_CLUSTERS:
        raise ValueError(f"n_clusters must lie in [1, {MAX_CLUSTERS}] (got {n_clusters!r})")
    if isinstance(max_iter, bool) or int(max_iter) < 1:
        raise ValueError(f"max_iter must be at least 1 (got {max_iter!r})")
    prep.check_device(device)
    buffer_km = float(buffer_km)
    df, lon, lat = locations(input_file, root_dir)
    n = len(df)
    located = np.isfinite(lon) & np.isfinite(lat)
    rows = np.nonzero(located)[0]  # the rows that take part, in input order
    N = rows.shape[0]
    if N >= MAX_POINTS:
        raise ValueError(f"{N} rows are beyond 2^30 - 1")
    if N < 1:
        raise ValueError(f"{input_file}: no row has a location")
    pos = quantise(lon[rows], lat[rows])
    year_of = [extract_year(str(v)) for v in df["Input"]]
    years = np.array([-1 if year_of[i] is None else year_of[i] for i in rows], dtype=np.int64)
    all_years = bool((years >= 0).all())
    rng = np.random.default_rng(random_state)
    cluster = np.full(N, -1, dtype=np.int32)
    stats: Dict[str, Any] = {"rows_in": int(n), "strategy": strategy, "buffer_km": buffer_km, "dropped": {"no_location": int(n - N), "buffer": 0}}
    if strategy == "kmeans":
        cluster, centres, sizes, rounds = kmeans(pos, n_clusters, rng, max_iter, device)
        mean_year = None
        if all_years:
            with np.errstate(all="ignore"):
                mean_year = np.bincount(cluster, weights=years.astype(np.float64), minlength=sizes.shape[0]) / sizes.astype(np.float64)
        cluster_sets = assign_sets(sizes, centres, N, test_ratio, val_ratio, include_test, include_val, mean_year, rng)
        sets = cluster_sets[cluster]
        stats.update({"n_clusters": int(sizes.shape[0]), "rounds": int(rounds), "cluster_sizes": [int(v) for v in sizes],
                      "cluster_sets": [SETS[int(v)] for v in cluster_sets]})
    elif strategy == "year":
        if not all_years:
            raise ValueError("strategy=year needs a year (19xx | 20xx) in every Input file name")
        sets = _by_year(years, N, test_ratio, val_ratio, include_test, include_val)
    else:
        order = rng.permutation(N)
        n_test = int(np.floor(N * float(test_ratio))) if include_test else 0
        n_val = int(np.floor(N * float(val_ratio))) if include_val else 0
        sets = np.zeros(N, dtype=np.int8)
        sets[order[:n_test]], sets[order[n_test : n_test + n_val]] = TEST, VAL
    # the audit, the guard band, and the audit of what is left
    before, d_train, d_val = _audit(pos, sets, buffer_km, device)
    keep = np.ones(N, dtype=bool)
    if buffer_km > 0.0:
        keep[np.nonzero(sets == TRAIN)[0][d_train < buffer_km]] = False
        keep[np.nonzero(sets == VAL)[0][d_val < buffer_km]] = False
    stats["dropped"]["buffer"] = int((~keep).sum())
    after = _audit(pos[keep], sets[keep], buffer_km, device)[0] if not keep.all() else before
    stats["nearest"] = {pair: {"rows": after[pair]["rows"], "against": after[pair]["against"], "min_km": after[pair]["min_km"],
                               "median_km": after[pair]["median_km"], "within_buffer_before": before[pair]["within_buffer"],
                               "within_buffer_after": after[pair]["within_buffer"]} for pair in before}
    stats["rows"] = {name: int(((sets == code) & keep).sum()) for code, name in enumerate(SETS)}
    stats["years"] = {name: {str(int(y)): int(c) for y, c in zip(*np.unique(years[(sets == code) & keep & (years >= 0)], return_counts=True))}
                      for code, name in enumerate(SETS)}
    # the files
    folder = os.path.join(output_dir, "splits")
    os.makedirs(folder, exist_ok=True)
    for code, name in enumerate(SETS):
        if (name == "val" and not include_val) or (name == "test" and not include_test):
            continue
        df.iloc[rows[(sets == code) & keep]].to_csv(os.path.join(folder, f"{name}.csv"), index=False)
    reason = np.full(n, "", dtype=object)
    reason[~located] = "no_location"
    reason[rows[~keep]] = "buffer"
    out = df[reason != ""].copy()
    out["reason"] = reason[reason != ""]
    out.to_csv(os.path.join(output_dir, "dropped.csv"), index=False)
    prep.write_stats(os.path.join(output_dir, "split_stats.json"), stats)
    if save_geojson:
        feats = [{"type": "Feature", "geometry": {"type": "Point", "coordinates": [float(lon[r]), float(lat[r])]},
                  "properties": {"row": int(r), "set": SETS[int(sets[k])] if keep[k] else "dropped",
                                 "cluster": int(cluster[k]) if cluster[k] >= 0 else None, "year": year_of[r]}} for k, r in enumerate(rows)]
        with open(os.path.join(output_dir, "splits.geojson"), "w") as f:
            json.dump({"type": "FeatureCollection", "features": feats}, f)
    return stats


# ---- mode=split_dataset --------------------------------------------------------------------------------------------------------------------
CONFIG_KEYS = ("input_file", "output_dir", "test_ratio", "val_ratio", "include_val", "include_test", "random_state", "n_clusters", "strategy",
               "buffer_km", "max_iter", "root_dir", "save_geojson", "device")


def split_options(cfg: Dict[str, Any]) -> Dict[str, Any]:
    """The ``split.*`` keys of ``mode=split_dataset`` checked -> the keyword arguments of :func:`split_dataset`.  A bad value raises
    ValueError; the two paths are required only in that mode."""
    c = prep.Section(cfg, "split", CONFIG_KEYS)
    ratio = lambda key: c.number(key, 0.2, lambda x: 0.0 <= x < 1.0, "must lie in [0, 1)")  # noqa: E731
    device = c.get("device")
    if device is not None and device != "host":
        try:
            prep.check_device(device)
        except ValueError:
            raise c.bad("device", "must be None, host or a cuda device", device) from None
    opts = dict(input_file=c.text("input_file"), output_dir=c.text("output_dir"), test_ratio=ratio("test_ratio"), val_ratio=ratio("val_ratio"),
                include_val=c.flag("include_val", True), include_test=c.flag("include_test", True),
                random_state=c.integer("random_state", 42, lo=0), n_clusters=c.integer("n_clusters", 20, lo=1, hi=MAX_CLUSTERS,
                                                                                       span=f"must lie in [1, {MAX_CLUSTERS}]"),
                strategy=c.choice("strategy", "kmeans", STRATEGIES),
                buffer_km=c.number("buffer_km", 0.0, lambda x: 0.0 <= x < float("inf"), "must be a finite distance >= 0"),
                max_iter=c.integer("max_iter", 100, lo=1), root_dir=c.text("root_dir"), save_geojson=c.flag("save_geojson", True), device=device)
    if (opts["test_ratio"] if opts["include_test"] else 0.0) + (opts["val_ratio"] if opts["include_val"] else 0.0) >= 1.0:
        raise ValueError("split.test_ratio + split.val_ratio must stay below 1: nothing would be left for train")
    if cfg.get("mode") == "split_dataset" and (opts["input_file"] is None or opts["output_dir"] is None):
        raise ValueError("mode=split_dataset needs split.input_file and split.output_dir")
    return opts


def run_from_config(cfg: Dict[str, Any], device: Optional[str] = None) -> int:
    """``mode=split_dataset``: :func:`split_dataset` under the ``split.*`` keys; prints one JSON line with the counts.  ``split.device``:
    None = ``device`` (the device when there is one), ``host`` = the numpy path."""
    kw = split_options(cfg)
    chosen = kw.pop("device")
    device = device if chosen is None else (None if chosen == "host" else chosen)
    stats = split_dataset(device=device, **kw)
    print(json.dumps({"split_dataset": {"rows_in": stats["rows_in"], **stats["rows"], "dropped": stats["dropped"],
                                        "output_dir": kw["output_dir"]}}))
    return 0


def main(argv: Optional[List[str]] = None) -> int:
    """``python -m instageo_amd.split split.input_file=chips_dataset.csv split.output_dir=out ...``: mode=split_dataset without ``run.py``."""
    return prep.run_mode_cli("split_dataset", run_from_config, argv)


if __name__ == "__main__":
    raise SystemExit(main())
