"""Reference for the zonal statistics of float rasters (values): pure numpy on the masks of tests/zonal_reference.py.

    a value v is VALID  iff  np.isfinite(v) and v != nodata
    per zone and band: pixels = the inside pixels, valid = the valid ones among them, and of the valid values in float64
    sum, mean = sum / valid, std = sqrt(mean((v - mean)^2)) (two passes, population), min, max;  NaN where valid == 0.

``integer_raster``, ``offset_raster`` and ``normal_raster`` build the seeded test rasters, ``hand_case`` the 4 x 4 square with a 2 x 2 hole
whose numbers are worked by hand.
"""
from typing import NamedTuple, Optional

import numpy as np

import zonal_reference as ZR


class Ref(NamedTuple):
    pixels: np.ndarray  # (Z,) int64
    valid: np.ndarray  # (Z, B) int64
    sum: np.ndarray  # (Z, B) float64 each
    mean: np.ndarray
    std: np.ndarray
    min: np.ndarray
    max: np.ndarray
    abs_sum: np.ndarray  # sum |v| of the valid values: what the summation bound is stated in


def valid_mask(raster: np.ndarray, nodata: Optional[float] = None) -> np.ndarray:
    ok = np.isfinite(raster)
    return ok if nodata is None else ok & (raster != nodata)


def ref_values(raster: np.ndarray, masks: np.ndarray, nodata: Optional[float] = None) -> Ref:
    """raster (B, H, W) float32, masks (Z, H, W) bool -> :class:`Ref`."""
    raster = np.asarray(raster)
    assert raster.dtype == np.float32 and raster.ndim == 3 and raster.shape[1:] == masks.shape[1:]
    Z, B = len(masks), raster.shape[0]
    ok = valid_mask(raster, nodata)
    out = Ref(masks.reshape(Z, -1).sum(axis=1).astype(np.int64), np.zeros((Z, B), dtype=np.int64),
              *(np.full((Z, B), np.nan) for _ in range(6)))
    for z in range(Z):
        for b in range(B):
            v = raster[b][masks[z] & ok[b]].astype(np.float64)
            out.valid[z, b] = v.size
            if v.size:
                mean = v.sum() / v.size
                out.sum[z, b], out.mean[z, b], out.std[z, b] = v.sum(), mean, np.sqrt(((v - mean) ** 2).sum() / v.size)
                out.min[z, b], out.max[z, b], out.abs_sum[z, b] = v.min(), v.max(), np.abs(v).sum()
    return out


def reference(name: str, raster: np.ndarray, nodata: Optional[float] = None) -> Ref:
    """:func:`ref_values` on the masks of ``ZR.reference(name)``."""
    return ref_values(raster, ZR.reference(name)[3], nodata)


# ---- rasters ------------------------------------------------------------------------------------------------------------------------------
NODATA = -9999.0


def poke_invalid(raster: np.ndarray, rng, nodata: float = NODATA) -> np.ndarray:
    """About one pixel in six of every band becomes NaN, +Inf or ``nodata`` (a third each); a raster of six pixels or more gets all
    three kinds whatever the draw (a smaller one, the 1 x 1 case, keeps what it drew)."""
    flat = raster.reshape(raster.shape[0], -1)
    kinds = (np.nan, np.inf, nodata)
    for b in range(flat.shape[0]):
        hit = rng.random(flat.shape[1]) < 1 / 6
        flat[b, hit] = rng.choice(kinds, size=int(hit.sum()))
        if flat.shape[1] >= 6:
            flat[b, rng.permutation(flat.shape[1])[:3]] = kinds
    return raster


def integer_raster(seed: int, B: int, H: int, W: int) -> np.ndarray:
    """Integer-valued float32 in [-1000, 1000] with the three kinds of invalid pixels."""
    rng = np.random.default_rng(seed)
    return poke_invalid(rng.integers(-1000, 1001, size=(B, H, W)).astype(np.float32), rng)


def offset_raster(seed: int, B: int, H: int, W: int) -> np.ndarray:
    """2^23 + k, k an integer in -3..3: exact in float32, a std of about 2 on an offset of 8.4 million."""
    rng = np.random.default_rng(seed)
    return (2.0**23 + rng.integers(-3, 4, size=(B, H, W))).astype(np.float32)


def normal_raster(seed: int, B: int, H: int, W: int) -> np.ndarray:
    """Seeded normal values times 1e3 plus 5e4, with the three kinds of invalid pixels."""
    rng = np.random.default_rng(seed)
    return poke_invalid((rng.standard_normal((B, H, W)) * 1e3 + 5e4).astype(np.float32), rng)


def hand_case():
    """A 6 x 6 raster with one zone: the square [1, 5] x [1, 5] (4 x 4 pixels) with the hole [2, 4] x [2, 4] (2 x 2 pixels), 12 inside
    pixels.  Band 0 holds r * 6 + c; band 1 the same with one NaN, one +Inf and one no-data value among the inside pixels.
    -> (raster (2, 6, 6), masks (1, 6, 6), nodata, want, (edges, edge_zone)) with ``want`` worked by hand:
    band 0: the ring is rows 1 and 4 whole (7 + 8 + 9 + 10 = 34, 25 + 26 + 27 + 28 = 106) and columns 1 and 4 of rows 2 and 3
    (13 + 16 + 19 + 22 = 70): sum 210, mean 17.5, min 7, max 28; the squared deviations: rows 1 and 4 give 2 (10.5^2 + 9.5^2 + 8.5^2 +
    7.5^2) = 658, the sides 4.5^2 + 1.5^2 + 1.5^2 + 4.5^2 = 45: M2 = 703, std = sqrt(703 / 12).
    band 1: pixels 7 (NaN), 28 (+Inf) and 16 (no-data) drop out: 9 valid, sum 210 - 51 = 159, mean 159 / 9, min 8, max 27."""
    raster = np.arange(36, dtype=np.float32).reshape(6, 6)
    raster = np.stack([raster, raster.copy()])
    raster[1, 1, 1], raster[1, 4, 4], raster[1, 2, 4] = np.nan, np.inf, NODATA
    zones = [[ZR.rect(1, 1, 5, 5), ZR.rect(2, 2, 4, 4)]]
    edges, edge_zone = ZR.edges_of(zones)
    masks = ZR.ref_masks(edges, edge_zone, 1, 6, 6)
    mean1 = 159.0 / 9.0
    left = [8, 9, 10, 13, 19, 22, 25, 26, 27]
    want = dict(pixels=[12], valid=[[12, 9]], sum=[[210.0, 159.0]], mean=[[17.5, mean1]],
                std=[[np.sqrt(703.0 / 12.0), np.sqrt(sum((v - mean1) ** 2 for v in left) / 9.0)]], min=[[7.0, 8.0]], max=[[28.0, 27.0]])
    return raster, masks, NODATA, want, (edges, edge_zone)
