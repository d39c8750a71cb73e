"""Host reference of the boundary-quality primitives (pure numpy, no scipy): the class-boundary distance transform by brute force over
every shift of the search window, and the Boundary-IoU / trimap count tables, as include/instageo_hip.h states them.  Used by
test_cpu_boundary.py, test_gpu_boundary.py and test_gpu_boundary_ranks.py."""
import numpy as np

from regions_reference import blobs, checkerboard, rings, stripes  # noqa: F401  (the map generators of the region tests)

FAR = 0x7FFFFFFF


def ref_dist2(cls, rmax, fill=-1):
    """(..., H, W) int8 -> int32 of the same shape: min (dy^2 + dx^2) over the pixels q inside the image with cls[q] != fill and
    cls[q] != cls[p], when that is <= rmax^2, else FAR; -1 at fill.  Brute force over the shifts (dy, dx) of the (2 rmax + 1)^2 window
    in the order of their length: a pixel looks at every shift until the first one that lands on a source, which is its minimum (the
    list of pixels still looking shrinks, which is all that keeps rmax = 32 affordable).  Positions outside the image read as fill."""
    c = np.asarray(cls).astype(np.int8)
    H, W = c.shape[-2:]
    flat = c.reshape(-1, H, W)
    pad = np.full((flat.shape[0], H + 2 * rmax, W + 2 * rmax), fill, dtype=np.int8)
    pad[:, rmax : rmax + H, rmax : rmax + W] = flat
    best = np.where(flat == fill, -1, FAR).astype(np.int32)
    n, y, x = np.nonzero(flat != fill)
    own = flat[n, y, x]
    span = range(-rmax, rmax + 1)
    for d, dy, dx in sorted((dy * dy + dx * dx, dy, dx) for dy in span for dx in span if 0 < dy * dy + dx * dx <= rmax * rmax):
        if n.size == 0:
            break
        q = pad[n, y + (rmax + dy), x + (rmax + dx)]
        hit = (q != fill) & (q != own)
        if hit.any():
            best[n[hit], y[hit], x[hit]] = d
            keep = ~hit
            n, y, x, own = n[keep], y[keep], x[keep], own[keep]
    return best.reshape(c.shape)


def ref_counts(gt, pred, thresholds, ncls, fill=-1, rmax=None):
    """-> (band [K][ncls][3], trimap [K][ncls][ncls]) int64 of gt / pred maps ((H, W) or (n, H, W) int8), distances from ref_dist2 with
    ``rmax`` (default: the smallest radius that covers the largest threshold)."""
    gt, pred = np.asarray(gt), np.asarray(pred)
    if rmax is None:
        rmax = int(np.ceil(np.sqrt(max(thresholds))))
    gd, pd = ref_dist2(gt, rmax, fill).astype(np.int64), ref_dist2(pred, rmax, fill).astype(np.int64)
    g, p = gt.astype(np.int64), pred.astype(np.int64)
    ok = (g != fill) & (p != fill) & (g >= 0) & (g < ncls) & (p >= 0) & (p < ncls)
    K = len(thresholds)
    band = np.zeros((K, ncls, 3), dtype=np.int64)
    trimap = np.zeros((K, ncls, ncls), dtype=np.int64)
    for k, t in enumerate(thresholds):
        in_g, in_p = ok & (gd <= t), ok & (pd <= t)
        band[k, :, 0] = np.bincount(g[in_g], minlength=ncls)
        band[k, :, 1] = np.bincount(p[in_p], minlength=ncls)
        band[k, :, 2] = np.bincount(g[in_g & in_p & (g == p)], minlength=ncls)
        trimap[k] = np.bincount(g[in_g] * ncls + p[in_g], minlength=ncls * ncls).reshape(ncls, ncls)
    return band, trimap


def ref_maps(labels, preds, ncls, ignore_index, fill=-1):
    """The int8 maps RunningBoundaryMetrics builds: labels (any numeric dtype, truncated toward zero) valid iff != ignore_index and in
    [0, ncls); preds fill wherever the ground truth is."""
    lab = np.trunc(np.asarray(labels, dtype=np.float64)).astype(np.int64)
    valid = (lab >= 0) & (lab < ncls)
    if ignore_index is not None:
        valid &= lab != ignore_index
    gt = np.where(valid, lab, fill).astype(np.int8)
    return gt, np.where(valid, np.asarray(preds).astype(np.int64), fill).astype(np.int8)


def ref_metrics(band, trimap):
    """Per k: (biou_per_class, biou, trimap_acc, trimap_iou) in float64, written out independently of instageo_amd.boundary."""
    out = []
    for b, t in zip(np.asarray(band, dtype=np.int64), np.asarray(trimap, dtype=np.int64)):
        union = b[:, 0] + b[:, 1] - b[:, 2]
        per = [float(i) / float(u) if u > 0 else float("nan") for i, u in zip(b[:, 2], union)]
        have = [v for v, u in zip(per, union) if u > 0]
        tp = np.diag(t)
        den = t.sum(0) + t.sum(1) - tp
        iou = [float(a) / float(d) if d else 0.0 for a, d in zip(tp, den)]
        out.append((per, float(np.mean(have)) if have else float("nan"), float(tp.sum() / t.sum()) if t.sum() else float("nan"), float(np.mean(iou))))
    return out


def shifted(cm, dy=0, dx=1):
    """The map moved by (dy, dx) with edge replication (a prediction whose outlines are one pixel off)."""
    H, W = cm.shape[-2:]
    ys = np.clip(np.arange(H) - dy, 0, H - 1)
    xs = np.clip(np.arange(W) - dx, 0, W - 1)
    return np.ascontiguousarray(cm[..., ys, :][..., :, xs])
