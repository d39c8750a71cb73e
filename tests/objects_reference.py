"""The host twin of the object metrics (instageo_amd/objects.py, csrc/objects.hip): pure numpy and Python integers, no code shared with
the product.  Labels by a sequential flood fill, the overlap table by ``np.unique`` on packed keys, the matches by a loop over its rows
with ``fractions.Fraction`` for the threshold test."""
from fractions import Fraction

import numpy as np

N4 = ((-1, 0), (1, 0), (0, -1), (0, 1))
N8 = N4 + ((-1, -1), (-1, 1), (1, -1), (1, 1))


def ref_labels(cls, connectivity=4, fill=-1):
    """(H, W) int8 -> int32: the smallest row-major index of the pixel's component, -1 at fill.  Pixels are visited in row-major order,
    so the seed of a fill is the smallest index of its component."""
    H, W = cls.shape
    lab = np.full((H, W), -1, np.int32)
    nb = N4 if connectivity == 4 else N8
    for y0 in range(H):
        for x0 in range(W):
            c = cls[y0, x0]
            if c == fill or lab[y0, x0] >= 0:
                continue
            root = y0 * W + x0
            lab[y0, x0] = root
            stack = [(y0, x0)]
            while stack:
                y, x = stack.pop()
                for dy, dx in nb:
                    v, u = y + dy, x + dx
                    if 0 <= v < H and 0 <= u < W and lab[v, u] < 0 and cls[v, u] == c:
                        lab[v, u] = root
                        stack.append((v, u))
    return lab


def ref_regions(cls, connectivity=4, fill=-1):
    """-> (labels, {label: (area, class)})."""
    lab = ref_labels(cls, connectivity, fill)
    roots, areas = np.unique(lab[lab >= 0], return_counts=True)
    W = cls.shape[1]
    return lab, {int(r): (int(a), int(cls[r // W, r % W])) for r, a in zip(roots, areas)}


def ref_table(gt, pred, connectivity=4, fill=-1):
    """(n, H, W) int8 maps -> int64 rows (image, gt_label, pred_label, intersection, gt_area, pred_area, gt_class, pred_class) sorted by
    (image, gt_label, pred_label)."""
    rows = []
    for i in range(gt.shape[0]):
        lg, rg = ref_regions(gt[i], connectivity, fill)
        lp, rp = ref_regions(pred[i], connectivity, fill)
        both = (lg >= 0) & (lp >= 0)
        packed = (lg[both].astype(np.uint64) << np.uint64(32)) | lp[both].astype(np.uint64)
        keys, counts = np.unique(packed, return_counts=True)
        for k, c in zip(keys.tolist(), counts.tolist()):
            g, p = k >> 32, k & 0xFFFFFFFF
            rows.append((i, g, p, c, rg[g][0], rp[p][0], rg[g][1], rp[p][1]))
    return np.array(rows, dtype=np.int64).reshape(-1, 8)


def ref_counts(gt, pred, ratios, ncls, connectivity=4, min_area=1, fill=-1):
    """-> (tp [K][ncls], iou_q [K][ncls], n_gt [ncls], n_pred [ncls]) as lists of Python integers; ratios = [(num, den), ...]."""
    K = len(ratios)
    tp = [[0] * ncls for _ in range(K)]
    iou_q = [[0] * ncls for _ in range(K)]
    n_gt, n_pred = [0] * ncls, [0] * ncls
    for i in range(gt.shape[0]):
        for cls, tally in ((gt[i], n_gt), (pred[i], n_pred)):
            for area, c in ref_regions(cls, connectivity, fill)[1].values():
                if 0 <= c < ncls and area >= min_area:
                    tally[c] += 1
    for _, _, _, cnt, ag, ap, cg, cp in ref_table(gt, pred, connectivity, fill).tolist():
        if cg != cp or not 0 <= cg < ncls or ag < min_area or ap < min_area:
            continue
        u = ag + ap - cnt
        for k, (num, den) in enumerate(ratios):
            if Fraction(cnt, u) > Fraction(num, den):
                tp[k][cg] += 1
                iou_q[k][cg] += (cnt * 2**25 + u) // (2 * u)
    return tp, iou_q, n_gt, n_pred


def add_counts(a, b):
    """The sum of two results of :func:`ref_counts`."""
    add = lambda x, y: [add(p, q) for p, q in zip(x, y)] if isinstance(x, list) else x + y  # noqa: E731
    return tuple(add(x, y) for x, y in zip(a, b))


def ref_metrics(tp, iou_q, n_gt, n_pred, classes=None):
    """One dict per threshold: per-class lists and means, floats (NaN where undefined) from exact rationals.  The rule of
    ``object_metrics_from_counts``: a class with regions and no match has pq = 0; a mean runs over the listed classes with
    tp + fp + fn > 0 on which the value is defined."""
    ncls = len(n_gt)
    chosen = range(ncls) if classes is None else classes
    nan = float("nan")
    frac = lambda a, b: float(Fraction(a, b)) if b else nan  # noqa: E731
    out = []
    for T, Q in zip(tp, iou_q):
        rec = {k: [nan] * ncls for k in ("precision", "recall", "f1", "sq", "rq", "pq")}
        rec["tp"], rec["fp"], rec["fn"] = list(T), [n_pred[c] - T[c] for c in range(ncls)], [n_gt[c] - T[c] for c in range(ncls)]
        for c in range(ncls):
            t, fp, fn = T[c], rec["fp"][c], rec["fn"][c]
            rec["precision"][c], rec["recall"][c] = frac(t, t + fp), frac(t, t + fn)
            rec["f1"][c] = frac(2 * t, 2 * t + fp + fn)
            rec["rq"][c] = frac(2 * t, 2 * t + fp + fn)
            rec["sq"][c] = float(Fraction(Q[c], 2**24 * t)) if t else nan
            if t:
                rec["pq"][c] = rec["sq"][c] * rec["rq"][c]  # the float64 product of the two rounded ratios, as defined
            elif fp + fn:
                rec["pq"][c] = 0.0
        means = {}
        for k in ("precision", "recall", "f1", "sq", "rq", "pq"):
            v = [rec[k][c] for c in chosen if T[c] + rec["fp"][c] + rec["fn"][c] > 0 and rec[k][c] == rec[k][c]]
            means[k] = sum(v) / len(v) if v else nan
        rec["mean"] = means
        out.append(rec)
    return out


def ref_maps(labels, preds, ncls, ignore_index):
    """The int8 maps the running metric builds: gt = the label where it is valid (not ignore_index, in [0, ncls)), -1 elsewhere; pred =
    the prediction with -1 wherever gt is -1."""
    lab = np.asarray(labels).astype(np.int64)
    valid = (lab >= 0) & (lab < ncls)
    if ignore_index is not None:
        valid &= lab != ignore_index
    return np.where(valid, lab, -1).astype(np.int8), np.where(valid, np.asarray(preds), -1).astype(np.int8)


def blobs(H, W, ncls, seed, fill_frac=0.02, cell=9):
    """A map of irregular patches: a coarse random grid of classes read through a jittered index, with a fraction of fill pixels."""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, ncls, size=(H // cell + 3, W // cell + 3))
    jy, jx = rng.integers(0, cell, size=(H, W)) // 3, rng.integers(0, cell, size=(H, W)) // 3
    yy, xx = np.mgrid[0:H, 0:W]
    out = coarse[(yy + jy) // cell, (xx + jx) // cell].astype(np.int8)
    out[rng.random((H, W)) < fill_frac] = -1
    return out


def noise(H, W, ncls, seed):
    return np.random.default_rng(seed).integers(0, ncls, size=(H, W)).astype(np.int8)
