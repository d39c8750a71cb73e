"""Reference for the per-zone order statistics (order statistics): the numpy twin ``zonal.zone_quantiles_host`` run zone by
zone on the masks of tests/zonal_reference.py, the key transform of the radix selection restated in numpy, and the seeded rasters the
selection is tried on besides those of tests/zonal_values_reference.py.

    valid values as in zonal_values_reference (finite, != nodata), canonicalised as v + 0.0, sorted ascending: v(0) <= ... <= v(n-1)
    f = q / 100.0,  h = (n - 1) * f (float64),  lo = floor(h),  hi = min(lo + 1, n - 1),  g = h - lo
    the pair (v(lo), v(hi)) as float32;  p = a + (b - a) * g for g > 0, else a, in float64;  NaN where n = 0
"""
from functools import lru_cache
from typing import NamedTuple, Optional

import numpy as np

import zonal_reference as ZR
from instageo_amd import zonal

QS = (0, 2.5, 10, 50, 90, 100)


class Twin(NamedTuple):
    valid: np.ndarray  # (Z, B) int64
    values: np.ndarray  # (Z, B, Q) float64, NaN where valid is 0
    pairs: np.ndarray  # (Z, B, Q, 2) float32 {v(lo), v(hi)}, NaN where valid is 0


def twin_on_masks(raster: np.ndarray, masks: np.ndarray, percentiles, nodata: Optional[float] = None) -> Twin:
    Z, B, Q = len(masks), raster.shape[0], len(percentiles)
    out = Twin(np.zeros((Z, B), dtype=np.int64), np.full((Z, B, Q), np.nan), np.full((Z, B, Q, 2), np.nan, dtype=np.float32))
    for z in range(Z):
        out.valid[z], out.values[z], out.pairs[z] = zonal.zone_quantiles_host(masks[z], raster, percentiles, nodata, pairs=True)
    return out


def twin(name: str, raster: np.ndarray, percentiles=QS, nodata: Optional[float] = None) -> Twin:
    """:func:`twin_on_masks` on the masks of ``ZR.reference(name)``."""
    return twin_on_masks(raster, ZR.reference(name)[3], list(percentiles), nodata)


# ---- the key transform ----------------------------------------------------------------------------------------------------------------------
def keys(v: np.ndarray) -> np.ndarray:
    """float32 -> uint32, ascending with the values: u = bits(v + 0.0f), key = u ^ (u >> 31 ? 0xFFFFFFFF : 0x80000000)."""
    u = (np.asarray(v, dtype=np.float32) + np.float32(0.0)).view(np.uint32)
    return u ^ np.where(u >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def unkeys(k: np.ndarray) -> np.ndarray:
    k = np.asarray(k, dtype=np.uint32)
    return (k ^ np.where(k >> np.uint32(31), np.uint32(0x80000000), np.uint32(0xFFFFFFFF))).view(np.float32)


# ---- rasters --------------------------------------------------------------------------------------------------------------------------------
TIE_VALUES = (-1.5, -0.0, 0.0, 0.25)


def tie_raster(seed: int, B: int, H: int, W: int) -> np.ndarray:
    """Four values only, two of them the two zeros: every wanted rank lies deep inside one bin in every round of the selection."""
    rng = np.random.default_rng(seed)
    return rng.choice(np.array(TIE_VALUES, dtype=np.float32), size=(B, H, W))


def sign_raster(seed: int, B: int, H: int, W: int) -> np.ndarray:
    """Negative and positive normals over many exponents and negative and positive denormals: both branches of the key transform, and
    keys that differ in every byte."""
    rng = np.random.default_rng(seed)
    normal = (rng.standard_normal((B, H, W)) * 10.0 ** rng.integers(-20, 21, size=(B, H, W))).astype(np.float32)
    denormal = (rng.integers(1, 2**23, size=(B, H, W)).astype(np.uint32) | (rng.integers(0, 2, size=(B, H, W)).astype(np.uint32) << 31)).view(np.float32)
    return np.where(rng.random((B, H, W)) < 0.25, denormal, normal)


@lru_cache(maxsize=None)
def constant_case(H: int = 3, W: int = 9000, value: float = 0.3125):
    """One zone over all of a constant raster -> (raster (1, H, W), edges, edge_zone)."""
    edges, edge_zone = ZR.edges_of([[ZR.rect(-1, -1, W + 1, H + 1)]])
    raster = np.full((1, H, W), value, dtype=np.float32)
    for a in (raster, edges, edge_zone):
        a.setflags(write=False)
    return raster, edges, edge_zone
