"""Sequential twin of the cleaning rule of include/instageo_hip.h: one Python loop per pixel, written from the rule alone and sharing
nothing with instageo_amd/clean.py.  It is the oracle of the numpy host path and of the kernels (ig_chip_nodata, ig_label_buffer,
ig_label_limit); the cases both test files use are built here too."""
import numpy as np


def nodata(chips, no_data_value):
    """-> (plane (n, H, W) uint8: bit 0 any, bit 1 all; counts (n, 2) int32).  A value the dtype cannot hold matches nothing."""
    n, B, H, W = chips.shape
    plane = np.zeros((n, H, W), dtype=np.uint8)
    counts = np.zeros((n, 2), dtype=np.int32)
    info = np.iinfo(chips.dtype)
    if not info.min <= no_data_value <= info.max:
        return plane, counts
    for i in range(n):
        for r in range(H):
            for c in range(W):
                hits = sum(int(chips[i, b, r, c]) == no_data_value for b in range(B))
                some, every = hits > 0, hits == B
                plane[i, r, c] = (1 if some else 0) | (2 if every else 0)
                counts[i, 0] += some
                counts[i, 1] += every
    return plane, counts


def drop(count, pixels, threshold):
    return count / float(pixels) > threshold


def _tally(out, ign, K):
    n, H, W = out.shape
    valid = np.zeros(n, dtype=np.int32)
    hist = np.zeros((n, K), dtype=np.int32) if K else None
    for i in range(n):
        for r in range(H):
            for c in range(W):
                if out[i, r, c] != ign:
                    valid[i] += 1
                    if K and 0 <= int(out[i, r, c]) < K:
                        hist[i, int(out[i, r, c])] += 1
    return valid, hist


def buffer(labels, w, ignore_index, plane=None, K=0):
    """-> (out, valid_labels (n,) int32, hist (n, K) int32 or None).  Per output pixel: the source of the INPUT map with the largest
    row-major index inside the window clipped to the map (the last set flag of the window read row by row)."""
    n, H, W = labels.shape
    ign = labels.dtype.type(ignore_index)
    source = labels != ign
    out = labels.copy()
    for i in range(n):
        for r in range(H):
            ra, rb = max(r - w, 0), min(r + w, H - 1)
            for c in range(W):
                ca, cb = max(c - w, 0), min(c + w, W - 1)
                hits = np.flatnonzero(source[i, ra : rb + 1, ca : cb + 1])
                if hits.size:
                    last = int(hits[-1])
                    out[i, r, c] = labels[i, ra + last // (cb - ca + 1), ca + last % (cb - ca + 1)]
                if plane is not None and int(plane[i, r, c]) & 2:
                    out[i, r, c] = ign
    return (out,) + _tally(out, ign, K)


def limit(labels, ptr, pts, ignore_index, K=0):
    """pts rows: (row, col) on the map; a point outside the map paints nothing."""
    n, H, W = labels.shape
    ign = labels.dtype.type(ignore_index)
    out = np.full_like(labels, ign)
    for i in range(n):
        for row, col in pts[ptr[i] : ptr[i + 1]]:
            if 0 <= row < H and 0 <= col < W:
                out[i, row, col] = labels[i, row, col]
    return (out,) + _tally(out, ign, K)


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------
def make_chips(n, B, H, W, nd, seed, dtype=np.int16):
    """Chips with ``nd`` in exactly one band of some pixels, in all bands of others, and in the last pixel of the last chip."""
    rng = np.random.default_rng(seed)
    chips = rng.integers(1, 3000, size=(n, B, H, W)).astype(dtype)
    one = rng.random((n, H, W)) < 0.2
    band = rng.integers(0, B, size=(n, H, W))
    for b in range(B):
        chips[:, b][one & (band == b)] = nd
    every = rng.random((n, H, W)) < 0.1
    chips[np.broadcast_to(every[:, None], chips.shape)] = nd
    chips[n - 1, :, H - 1, W - 1] = nd
    return chips


def seam_sources(H, W):
    """(row, col) on both sides of every 64-pixel block seam, at the corners where blocks meet, and on the map border."""
    rows = sorted({0, H - 1, H // 2} | {r for s in range(64, H, 64) for r in (s - 1, s)})
    cols = sorted({0, W - 1, W // 2} | {c for s in range(64, W, 64) for c in (s - 1, s)})
    return [(r, c) for r in rows for c in cols]


def make_labels(n, H, W, density, seed, ign=-1, dtype=np.int16):
    """Maps of ``ign`` with sources of classes 0..6 (and 300, outside a K = 7 histogram): ``density`` 'one' = a single source, else
    the share of source pixels; map 0 also has the seam / corner / border sources and two adjacent pairs of different classes."""
    rng = np.random.default_rng(seed)
    values = np.array([0, 1, 2, 3, 4, 5, 6, 300], dtype=dtype)
    maps = np.full((n, H, W), ign, dtype=dtype)
    if density == "one":
        maps[:, H // 3, W // 3] = 4
        return maps
    k = rng.random((n, H, W)) < density
    maps[k] = values[rng.integers(0, len(values), size=int(k.sum()))]
    for j, (r, c) in enumerate(seam_sources(H, W)):
        maps[0, r, c] = values[j % 7]
    if H > 8 and W > 8:
        maps[0, 5, 5:7] = (1, 2)  # horizontally adjacent: the later one (2) wins both pixels
        maps[0, 7:9, 2] = (3, 5)  # vertically adjacent
    return maps
