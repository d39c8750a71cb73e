"""Pixel-by-pixel reference of the two overview rules of include/instageo_hip.h (mode with a fill value, NaN-aware mean), the inputs the
GPU tests run on and the table of their shapes.  Plain loops over the children and collections.Counter: nothing here is shared with
instageo_amd.cog.

Level k has ceil(H_{k-1} / 2) x ceil(W_{k-1} / 2) pixels; the children of (r, c) are the pixels (2r..2r+1, 2c..2c+1) of level k-1 that lie
inside it, in row-major order; level k is computed from level k-1."""
import functools
from collections import Counter

import numpy as np

NAN_BITS = 0x7FC00000

# name -> (H, W, levels): what each shape can break
CASES = {
    "one_1x1": (1, 1, 2),            # degenerate raster (the levels stay 1 x 1)
    "odd_37x67": (37, 67, 7),        # odd at several levels, W no multiple of 16 or 64
    "block_64x64": (64, 64, 6),      # exactly one block
    "block_65x129": (65, 129, 7),    # a block boundary plus one, in both directions
    "wide_3x9000": (3, 9000, 6),     # many blocks in a row, the last one partial
    "deep_130x70": (130, 70, 8),     # more than six levels: the second launch on level 6
    "d4_128x192": (128, 192, 6),     # multiples of 2^6: the mode rule commutes with the D4 maps
}


def children(a, r, c):
    """The children of pixel (r, c) of the next level of the 2-D array ``a``, in row-major order."""
    H, W = a.shape
    return [a[y, x] for y in (2 * r, 2 * r + 1) if y < H for x in (2 * c, 2 * c + 1) if x < W]


def mode_of(values, fill):
    """Children equal to fill are ignored; none left: fill; else the value with the most children, ties to the smallest value."""
    tally = Counter(int(v) for v in values if int(v) != fill)
    if not tally:
        return fill
    top = max(tally.values())
    return min(v for v, n in tally.items() if n == top)


def mean_of(values):
    """float32 sum of the children that are not NaN in the given order, divided by their number in float32; NaN (0x7fc00000) if none."""
    valid = [np.float32(v) for v in values if not np.isnan(v)]
    if not valid:
        return np.uint32(NAN_BITS).view(np.float32)
    s = valid[0]
    for v in valid[1:]:
        s = np.float32(s + v)
    return np.float32(s / np.float32(len(valid)))


def next_level(a, kind, fill=-1):
    """One level of a (H, W) or (bands, H, W) array."""
    if a.ndim == 3:
        return np.stack([next_level(b, kind, fill) for b in a])
    H, W = a.shape
    out = np.empty(((H + 1) // 2, (W + 1) // 2), dtype=a.dtype)
    for r in range(out.shape[0]):
        for c in range(out.shape[1]):
            kids = children(a, r, c)
            out[r, c] = mode_of(kids, fill) if kind == "mode" else mean_of(kids)
    return out


def pyramid(a, kind, levels, fill=-1):
    """Levels 1..levels, each from the one before."""
    out = []
    for _ in range(levels):
        a = next_level(a, kind, fill)
        out.append(a)
    return out


def seg_stats(classmap, ncls, fill=-1):
    """The reference's dictionary (compute_seg_stats) of an int8 class map: valid = a class in [0, ncls) that is not fill."""
    tally = Counter(int(v) for v in np.asarray(classmap).ravel())
    cc = {str(v): n for v, n in sorted(tally.items()) if v != fill and 0 <= v < ncls}
    return {"valid_pixels": sum(cc.values()), "class_counts": cc, "unique_values": len(cc)}


def histogram(classmap, ncls, fill=-1):
    """(ncls + 1,) int64, the last slot for fill or any value that is not a class: np.bincount of the map with those values moved there."""
    v = np.asarray(classmap).astype(np.int64).ravel()
    v[(v == fill) | (v < 0) | (v >= ncls)] = ncls
    return np.bincount(v, minlength=ncls + 1)


def class_map(seed, H, W, ncls, fill=-1, extra=()):
    """Random classes; a fifth of the pixels fill; a few stray values that are no class; then columns 64..127 (where they exist) all fill,
    written last, so whole 64 x 64 blocks are empty (:func:`empty_blocks` counts them)."""
    rng = np.random.default_rng(seed)
    cm = rng.integers(0, ncls, size=(H, W)).astype(np.int8)
    cm[rng.random((H, W)) < 0.2] = fill
    for v in extra:
        cm[rng.random((H, W)) < 0.03] = v
    cm[:, 64:128] = fill
    cm.setflags(write=False)
    return cm


def empty_blocks(a, fill=None, block=64):
    """The block-aligned ``block`` x ``block`` blocks of the (H, W) or (bands, H, W) array (clipped at the raster's edge, but a full ``block``
    columns wide) that hold nothing but ``fill`` (None: NaN)."""
    a = a if a.ndim == 3 else a[None]
    empty = np.isnan(a).all(axis=0) if fill is None else (a == fill).all(axis=0)
    H, W = empty.shape
    return sum(bool(empty[y : y + block, x : x + block].all()) for y in range(0, H, block) for x in range(0, W - block + 1, block))


def float_raster(seed, bands, H, W, dyadic=False):
    """Values in [0, 1] (``dyadic``: multiples of 1/8 up to 4, exactly representable with exact sums), NaN holes on a fifth of the pixels and
    on columns 64..127 (whole blocks).  No subnormals: the smallest non-zero magnitude is far above 2^-126."""
    rng = np.random.default_rng(seed)
    a = (rng.integers(0, 33, size=(bands, H, W)) / 8.0 if dyadic else rng.random((bands, H, W))).astype(np.float32)
    a[rng.random((bands, H, W)) < 0.2] = np.nan
    a[:, :, 64:128] = np.nan
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def mode_case(name, ncls=3, fill=-1, extra=(3, 100, -128)):
    H, W, levels = CASES[name]
    cm = class_map(len(name) + ncls, H, W, ncls, fill, extra)
    return cm, pyramid(cm, "mode", levels, fill)


@functools.lru_cache(maxsize=None)
def mean_case(name, bands=1, dyadic=False):
    H, W, levels = CASES[name]
    a = float_raster(len(name) + bands, bands, H, W, dyadic)
    return a, pyramid(a, "mean", levels)


def bits(a):
    """The uint32 view of a float32 array: NaN positions (and payloads) count in a comparison."""
    return np.ascontiguousarray(a).view(np.uint32)
