"""Host reference of the region post-processing (numpy + plain Python, no scipy): labelling, the sieve rule and the region table, as
instageo_amd/postprocess.py states them.  A simple union-find that always hangs the larger root under the smaller, so the root of a
set is its smallest row-major index.  Used by test_cpu_regions.py and test_gpu_regions.py."""
import numpy as np


def ref_label(cm, connectivity=4, fill=-1):
    """(H, W) int8 -> (H, W) int32: the smallest row-major index of the pixel's component, -1 at fill."""
    assert connectivity in (4, 8)
    cm = np.asarray(cm)
    H, W = cm.shape
    flat = cm.reshape(-1).tolist()
    par = list(range(H * W))

    def find(a):
        r = a
        while par[r] != r:
            r = par[r]
        while par[a] != r:
            par[a], a = r, par[a]
        return r

    def union(a, b):
        a, b = find(a), find(b)
        if a != b:
            par[max(a, b)] = min(a, b)

    back = [(0, -1), (-1, 0)] + ([(-1, -1), (-1, 1)] if connectivity == 8 else [])
    for y in range(H):
        for x in range(W):
            p = y * W + x
            c = flat[p]
            if c == fill:
                continue
            for dy, dx in back:
                yy, xx = y + dy, x + dx
                if 0 <= yy and 0 <= xx < W and flat[yy * W + xx] == c:
                    union(p, yy * W + xx)
    out = np.array([-1 if flat[p] == fill else find(p) for p in range(H * W)], dtype=np.int32)
    return out.reshape(H, W)


def ref_label_batch(cms, connectivity=4, fill=-1):
    cms = np.asarray(cms)
    return np.stack([ref_label(c, connectivity, fill) for c in cms]) if cms.ndim == 3 else ref_label(cms, connectivity, fill)


def ref_area(labels):
    """(H, W) labels -> (H * W,) int64: pixel count at root positions, 0 elsewhere."""
    lab = labels.reshape(-1)
    return np.bincount(lab[lab >= 0], minlength=lab.size).astype(np.int64)


def ref_sieve_pass(cm, min_region, connectivity=4, fill=-1):
    """One pass -> (new map, number of small regions reassigned)."""
    H, W = cm.shape
    lab = ref_label(cm, connectivity, fill)
    area = ref_area(lab)
    best = {}  # small root -> (area of the winner, -label of the winner): the maximum wins
    for y in range(H):
        for x in range(W):
            R = int(lab[y, x])
            if R < 0 or area[R] >= min_region:
                continue
            for yy, xx in ((y - 1, x), (y, x - 1), (y, x + 1), (y + 1, x)):
                if not (0 <= yy < H and 0 <= xx < W):
                    continue
                S = int(lab[yy, xx])
                if S < 0 or S == R or area[S] < min_region:
                    continue
                key = (int(area[S]), -S)
                if R not in best or key > best[R]:
                    best[R] = key
    out = cm.copy()
    flat_in = cm.reshape(-1)
    for R, (_, negS) in best.items():
        out[lab == R] = flat_in[-negS]
    return out, len(best)


def ref_sieve(cm, min_region, connectivity=4, fill=-1, max_passes=8):
    """-> (new map, {"passes", "changed", "small_left"}) with sieve_class_map's definitions; one (H, W) map."""
    out = np.array(cm, copy=True)
    info = {"passes": 0, "changed": 0, "small_left": 0}
    if min_region <= 1:
        return out, info
    for _ in range(max_passes):
        out, c = ref_sieve_pass(out, min_region, connectivity, fill)
        if c == 0:
            break
        info["passes"] += 1
        info["changed"] += c
    area = ref_area(ref_label(out, connectivity, fill))
    info["small_left"] = int(((area > 0) & (area < min_region)).sum())
    return out, info


def ref_table(cms, connectivity=4, fill=-1):
    """Rows ordered by (image, root); the columns of postprocess.TABLE_COLUMNS."""
    cms = np.asarray(cms)
    if cms.ndim == 2:
        cms = cms[None]
    cols = {k: [] for k in ("image", "root", "cls", "area", "row_min", "row_max", "col_min", "col_max", "centroid_row", "centroid_col")}
    for i, cm in enumerate(cms):
        H, W = cm.shape
        lab = ref_label(cm, connectivity, fill)
        for root in np.unique(lab[lab >= 0]):
            ys, xs = np.nonzero(lab == root)
            a = int(ys.size)
            vals = (i, int(root), int(cm.reshape(-1)[root]), a, int(ys.min()), int(ys.max()), int(xs.min()), int(xs.max()),
                    int(ys.sum()) / a, int(xs.sum()) / a)
            for k, v in zip(cols, vals):
                cols[k].append(v)
    return {k: np.array(v, dtype=np.float64 if k.startswith("centroid") else np.int64) for k, v in cols.items()}


# ---- test patterns -----------------------------------------------------------------------------------------------------------------
def blobs(H, W, ncls, seed, fill_frac=0.02, fill=-1, smooth=3):
    """Smoothed-noise blobs: argmax over ncls box-filtered noise planes, then fill on a random fill_frac of the pixels."""
    rng = np.random.default_rng(seed)
    planes = rng.standard_normal((ncls, H + 2 * smooth, W + 2 * smooth))
    k = 2 * smooth + 1
    c = np.cumsum(np.cumsum(np.pad(planes, ((0, 0), (1, 0), (1, 0))), axis=1), axis=2)
    box = c[:, k:, k:] - c[:, :-k, k:] - c[:, k:, :-k] + c[:, :-k, :-k]
    cm = box[:, :H, :W].argmax(0).astype(np.int8)
    if fill == 0:
        cm += 1  # classes 1..ncls, 0 is free for fill
    if fill_frac > 0:
        cm[rng.random((H, W)) < fill_frac] = fill
    return cm


def noise(H, W, ncls, seed):
    return np.random.default_rng(seed).integers(0, ncls, size=(H, W)).astype(np.int8)


def checkerboard(H, W):
    y, x = np.mgrid[:H, :W]
    return ((y + x) & 1).astype(np.int8)


def stripes(H, W, vertical=False):
    y, x = np.mgrid[:H, :W]
    return ((x if vertical else y) & 1).astype(np.int8)


def rings(H, W):
    """Concentric one-pixel square rings around the centre, ring d (from the border) of class d % 127."""
    y, x = np.mgrid[:H, :W]
    d = np.minimum(np.minimum(y, H - 1 - y), np.minimum(x, W - 1 - x))
    return (d % 127).astype(np.int8)


def serpentine(S):
    """A one-pixel corridor of class 1 that winds through every second row of an S x S map of class 0 walls: one component through
    every tile."""
    cm = np.zeros((S, S), dtype=np.int8)
    cm[0::2, :] = 1
    for j, y in enumerate(range(1, S, 2)):
        cm[y, S - 1 if j % 2 == 0 else 0] = 1
    return cm
