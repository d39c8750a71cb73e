"""Object-level metrics of class maps (not in the reference).

The confusion matrix, the boundary metrics and the calibration count pixels; what the region tables and the polygons deliver is objects.
Here a *region* is a connected component of one class (``ig_ccl_label``), and two maps are compared region by region:

* :func:`overlap_table` -- the shared pixels of every ground-truth region with every predicted region it meets (``ig_object_pairs``: a
  sparse pair tally on the device), with the areas and classes of both: the general tool behind over- / under-segmentation measures or
  object-level change tables.
* **Detection F1** at an IoU threshold t: a ground-truth and a predicted region of one class are a match when their IoU is strictly above
  t.  For t >= 1/2 a region matches at most one region of the other map, so the matches are unique and need no assignment step.
  TP = matches, FP = predicted regions without one, FN = ground-truth regions without one.
* **Panoptic quality** (Kirillov et al., CVPR 2019): SQ = the mean IoU of the matches, RQ = TP / (TP + FP / 2 + FN / 2), PQ = SQ RQ.

:class:`RunningObjectMetrics` streams four integer tables on the device (``ig_object_match``, ``ig_object_count``; they add across batches
and ranks like a confusion matrix); :func:`object_metrics_from_counts` takes the float64 ratios on the host once per epoch.
"""
from __future__ import annotations

import math
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .boundary import FILL, class_maps

__all__ = ["check_object_options", "threshold_ratios", "overlap_table", "RunningObjectMetrics", "object_metrics_from_counts", "MAX_THRESHOLDS",
           "MIN_CAPACITY", "AUTO_CAPACITY", "MAX_CAPACITY", "IOU_UNIT", "FILL"]

MAX_THRESHOLDS = 10  # ig_object_match tests at most 10 thresholds per launch
MIN_CAPACITY, MAX_CAPACITY = 1 << 10, 1 << 30  # ig_object_pairs' table sizes
AUTO_CAPACITY = 1 << 24  # the largest table taken without evidence that it is needed (192 MiB of keys and counts)
IOU_UNIT = 1 << 24  # iou_q counts IoU in units of 2^-24


def check_object_options(thresholds, num_classes: int = 2, connectivity: int = 4, min_area: int = 1, classes=None,
                         regression: bool = False) -> List[float]:
    """The ``test.object_*`` keys (with ``test.object_metrics``) -> the IoU thresholds as floats of at most three decimals."""
    if regression:
        raise ValueError("test.object_metrics needs class maps: a regression task (is_reg_task) has none")
    if not isinstance(thresholds, (list, tuple)) or not 1 <= len(thresholds) <= MAX_THRESHOLDS:
        raise ValueError(f"test.object_iou_thresholds must be a list of 1 to {MAX_THRESHOLDS} thresholds (got {thresholds!r})")
    ts = []
    for t in thresholds:
        if not isinstance(t, (int, float)) or isinstance(t, bool) or not math.isfinite(t) or not 0.5 <= t <= 0.999:
            raise ValueError(f"test.object_iou_thresholds: every threshold must be a finite number in [0.5, 0.999] (got {t!r}); below 0.5 a "
                             "region can match several and the matching is no longer unique")
        if abs(t * 1000 - round(t * 1000)) > 1e-9:
            raise ValueError(f"test.object_iou_thresholds: at most three decimals (got {t!r}); the test is exact in thousandths")
        ts.append(round(t * 1000) / 1000)
    for a, b in zip(ts, ts[1:]):
        if b <= a:
            raise ValueError(f"test.object_iou_thresholds must be strictly ascending (got {thresholds!r})")
    if not isinstance(num_classes, int) or isinstance(num_classes, bool) or not 2 <= num_classes <= 127:
        raise ValueError(f"test.object_metrics: class maps are int8, 2 <= num_classes <= 127 (got {num_classes!r})")
    if connectivity not in (4, 8) or isinstance(connectivity, bool):
        raise ValueError(f"test.object_connectivity must be 4 or 8 (got {connectivity!r})")
    if not isinstance(min_area, int) or isinstance(min_area, bool) or not 1 <= min_area <= 2**31 - 1:
        raise ValueError(f"test.object_min_area must be an integer >= 1 (got {min_area!r})")
    if classes is not None:
        ok = isinstance(classes, (list, tuple)) and len(classes) >= 1 and len(set(classes)) == len(classes)
        if not ok or any(not isinstance(c, int) or isinstance(c, bool) or not 0 <= c < num_classes for c in classes):
            raise ValueError(f"test.object_classes must be None or a list of distinct class ids in [0, {num_classes}) (got {classes!r})")
    return ts


def threshold_ratios(thresholds: Sequence[float]) -> List[Tuple[int, int]]:
    """IoU thresholds of at most three decimals -> the exact rationals (round(1000 t), 1000) that ``ig_object_match`` compares with."""
    return [(int(round(t * 1000)), 1000) for t in thresholds]


def _capacity_for(pixels: int) -> int:
    """The smallest power of two >= 2 * pixels, clamped to [MIN_CAPACITY, AUTO_CAPACITY]: distinct pairs cannot outnumber the pixels, so
    below the clamp the table is at most half full and cannot overflow."""
    return min(max(1 << max(2 * pixels - 1, 1).bit_length(), MIN_CAPACITY), AUTO_CAPACITY)


class _Table:
    """The (keys, counts, status) buffers of one user, grown when a larger table is asked for and reused otherwise."""

    def __init__(self) -> None:
        self.keys: Optional[torch.Tensor] = None
        self.counts: Optional[torch.Tensor] = None
        self.status: Optional[torch.Tensor] = None

    def take(self, capacity: int, device) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        if self.keys is None or self.keys.numel() < capacity or self.keys.device != torch.device(device):
            self.keys = torch.empty(capacity, dtype=torch.int64, device=device)
            self.counts = torch.empty(capacity, dtype=torch.int32, device=device)
            self.status = torch.zeros(1, dtype=torch.int32, device=device)
        return self.keys[:capacity], self.counts[:capacity], self.status

    def tally(self, gt_labels: torch.Tensor, pred_labels: torch.Tensor, capacity: int, check: bool):
        """-> (keys, counts) of ``ig_object_pairs``.  ``check``: read the status and run again at twice the capacity while the table
        overflows (it is bounded by the pixels, so this ends); without it nothing is copied to the host."""
        while True:
            keys, counts, status = self.take(capacity, gt_labels.device)
            status.zero_()
            ops.object_pairs(gt_labels, pred_labels, keys, counts, status)
            if not check or not int(status.item()) & 1:
                return keys, counts
            if capacity >= MAX_CAPACITY:
                raise RuntimeError(f"ig_object_pairs: more than {MAX_CAPACITY} pairs of overlapping regions; split the map")
            capacity *= 2


def _labels_and_areas(gt: torch.Tensor, pred: torch.Tensor, connectivity: int, fill: int):
    """Both maps labelled in ONE ``ig_ccl_label`` call on the stacked maps (and one ``ig_region_area``) -> labels (2, n, H, W), areas."""
    n, H, W = gt.shape
    if 2 * n * H * W > ops.OBJECT_MAX_PIXELS:  # the stack would pass 2^31 - 1 elements: one map at a time
        labels = torch.stack((ops.ccl_label(gt, connectivity, fill), ops.ccl_label(pred, connectivity, fill)))
    else:
        labels = ops.ccl_label(torch.stack((gt, pred)).view(2 * n, H, W), connectivity, fill).view(2, n, H, W)
    return labels, torch.stack((ops.region_area(labels[0]), ops.region_area(labels[1])))


def _maps3(gt: torch.Tensor, pred: torch.Tensor):
    if gt.dtype != torch.int8 or pred.dtype != torch.int8 or gt.shape != pred.shape or gt.dim() not in (2, 3):
        raise ValueError(f"class maps must be two int8 tensors of one shape (H, W) or (n, H, W) (got {gt.dtype} {tuple(gt.shape)}, "
                         f"{pred.dtype} {tuple(pred.shape)})")
    shape = (1,) * (3 - gt.dim()) + tuple(gt.shape)
    if math.prod(shape) > ops.OBJECT_MAX_PIXELS:
        raise ValueError(f"{math.prod(shape)} pixels: at most 2^31 - 1 can be tallied at once (keys hold image * H * W + label in 32 bits): "
                         "split the batch")
    return gt.contiguous().view(shape), pred.contiguous().view(shape)


def overlap_table(gt: torch.Tensor, pred: torch.Tensor, connectivity: int = 4, fill: int = FILL) -> torch.Tensor:
    """Two int8 class maps (n, H, W) | (H, W) on the device -> int64 rows (image, gt_label, pred_label, intersection, gt_area, pred_area,
    gt_class, pred_class), one per pair of a ground-truth and a predicted region that share a pixel, sorted by (image, gt_label,
    pred_label).  A label is the region's smallest row-major pixel index in its image (``ig_ccl_label``); ``fill`` pixels of either map
    belong to no pair.  Regions of different classes are listed too: the table is the overlap, not the matching."""
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8 (got {connectivity!r})")
    gt3, pred3 = _maps3(gt, pred)
    n, H, W = gt3.shape
    if n * H * W == 0:
        return torch.empty((0, 8), dtype=torch.int64, device=gt.device)
    labels, areas = _labels_and_areas(gt3, pred3, connectivity, fill)
    keys, counts = _Table().tally(labels[0], labels[1], _capacity_for(n * H * W), check=True)
    used = keys != ops.OBJECT_EMPTY
    key, order = torch.sort(keys[used])  # the key orders by (image, gt_label, pred_label): image * HW + gt_label sits in its upper half
    inter = counts[used][order].long()
    HW = H * W
    gi, p = key >> 32, key & 0xFFFFFFFF
    image = gi // HW
    pi = image * HW + p
    return torch.stack((image, gi - image * HW, p, inter, areas[0].view(-1)[gi].long(), areas[1].view(-1)[pi].long(),
                        gt3.view(-1)[gi].long(), pred3.view(-1)[pi].long()), dim=1)


def object_metrics_from_counts(tp, iou_q, n_gt, n_pred, thresholds: Sequence[float], classes: Optional[Sequence[int]] = None) -> List[Dict[str, Any]]:
    """One record per threshold from the integer tables tp [K][ncls], iou_q [K][ncls] (IoU sums in units of 2^-24), n_gt [ncls] and
    n_pred [ncls], in float64.  Per class: ``tp``, ``fp`` = n_pred - tp, ``fn`` = n_gt - tp, ``precision`` = tp / n_pred, ``recall`` =
    tp / n_gt, ``f1`` = 2 tp / (n_pred + n_gt), ``sq`` = iou_q / 2^24 / tp, ``rq`` = tp / (tp + fp / 2 + fn / 2) (= f1), ``pq`` = sq rq,
    each NaN where its denominator is 0 -- except that a class with regions but no match has pq = 0, the value of Kirillov et al.'s
    sum-of-IoU form, not NaN from its undefined sq.  The unsuffixed values are means over the classes of ``classes`` (all when None) that
    have a region in either map (tp + fp + fn > 0), leaving out the NaN of a class where the value is not defined; NaN when none is left."""
    tp_, q_ = np.asarray(tp, dtype=np.int64), np.asarray(iou_q, dtype=np.int64)
    ng, npd = np.asarray(n_gt, dtype=np.int64), np.asarray(n_pred, dtype=np.int64)
    K = len(thresholds)
    if tp_.ndim != 2 or tp_.shape[0] != K or q_.shape != tp_.shape or ng.shape != (tp_.shape[1],) or npd.shape != ng.shape:
        raise ValueError(f"object counts must be [K][ncls], [K][ncls], [ncls] and [ncls] with K = {K} (got {tp_.shape}, {q_.shape}, {ng.shape}, "
                         f"{npd.shape})")
    ncls = tp_.shape[1]
    sel = np.zeros(ncls, dtype=bool)
    sel[list(range(ncls)) if classes is None else [int(c) for c in classes]] = True

    def ratio(a, b):
        out = np.full(ncls, np.nan)
        np.divide(a, b, out=out, where=b > 0)
        return out

    def mean(v, present):
        v = v[present & ~np.isnan(v)]
        return float(v.mean()) if v.size else float("nan")

    out = []
    for k, t in enumerate(thresholds):
        T = tp_[k].astype(np.float64)
        fp, fn = npd - tp_[k], ng - tp_[k]
        present = sel & (tp_[k] + fp + fn > 0)
        rec = {"threshold": float(t), "tp": tp_[k].tolist(), "fp": fp.tolist(), "fn": fn.tolist()}
        sq = ratio(q_[k].astype(np.float64) / IOU_UNIT, T)
        rq = ratio(T, T + 0.5 * fp + 0.5 * fn)
        pq = sq * rq
        pq[(tp_[k] == 0) & (fp + fn > 0)] = 0.0
        per = {"precision": ratio(T, npd.astype(np.float64)), "recall": ratio(T, ng.astype(np.float64)),
               "f1": ratio(2 * T, (npd + ng).astype(np.float64)), "sq": sq, "rq": rq, "pq": pq}
        for name, v in per.items():
            rec[f"{name}_per_class"] = v.tolist()
            rec[name] = mean(v, present)
        out.append(rec)
    return out


class RunningObjectMetrics:
    """Streaming object F1 and panoptic quality at a few IoU thresholds, device resident (the shape of
    :class:`boundary.RunningBoundaryMetrics`)."""

    def __init__(self, num_classes: int, thresholds: Sequence[float] = (0.5,), ignore_index: Optional[int] = None, connectivity: int = 4,
                 min_area: int = 1, device: Optional[str] = None) -> None:
        self.thresholds = check_object_options(list(thresholds), num_classes, connectivity, min_area)
        self.ratios = threshold_ratios(self.thresholds)
        self.num_classes, self.ignore_index, self._device = num_classes, ignore_index, device
        self.connectivity, self.min_area = connectivity, min_area
        self._counts: Optional[Tuple[torch.Tensor, ...]] = None
        self._table = _Table()  # one table buffer per instance

    def device_counts(self, device=None):
        """(tp int64 [K, ncls], iou_q int64 [K, ncls], n_gt int64 [ncls], n_pred int64 [ncls]): integer sums, they add across ranks."""
        if self._counts is None:
            dev, K = device or self._device or "cuda", len(self.thresholds)
            self._counts = (torch.zeros(K, self.num_classes, dtype=torch.int64, device=dev),
                            torch.zeros(K, self.num_classes, dtype=torch.int64, device=dev),
                            torch.zeros(self.num_classes, dtype=torch.int64, device=dev),
                            torch.zeros(self.num_classes, dtype=torch.int64, device=dev))
        return self._counts

    def update(self, logits_or_preds: torch.Tensor, labels: torch.Tensor) -> None:
        """logits (B, ncls, H, W) f32 or predictions (B, H, W), labels (B, H, W), on the device.  The maps are those of the boundary
        metric (:func:`boundary.class_maps`): gt is fill where the label is invalid and pred is fill wherever gt is.  The batch is walked
        in groups of images whose table (2 slots per pixel) stays within 2^24 slots: it cannot overflow and nothing is copied to the
        host.  Only a single image beyond that is tallied with a look at the status, and again at twice the size if need be."""
        if labels.numel() == 0:
            return
        gt, pred = class_maps(logits_or_preds, labels, self.num_classes, self.ignore_index)
        if gt.dim() not in (2, 3):
            raise ValueError(f"labels must be (B, H, W) or (H, W) (got {tuple(labels.shape)})")
        gt, pred = gt.view((-1,) + tuple(gt.shape[-2:])), pred.view((-1,) + tuple(gt.shape[-2:]))
        n, H, W = gt.shape
        if H * W > ops.OBJECT_MAX_PIXELS:
            raise ValueError(f"an image of {H * W} pixels: at most 2^31 - 1 can be tallied at once")
        tp, iou_q, n_gt, n_pred = self.device_counts(gt.device)
        group = max(1, (AUTO_CAPACITY // 2) // (H * W))
        for i0 in range(0, n, group):
            g, p = gt[i0:i0 + group], pred[i0:i0 + group]
            pixels = g.numel()
            labels2, areas = _labels_and_areas(g, p, self.connectivity, FILL)
            keys, counts = self._table.tally(labels2[0], labels2[1], _capacity_for(pixels), check=2 * pixels > AUTO_CAPACITY)
            ops.object_match(keys, counts, g, p, areas[0], areas[1], self.ratios, tp, iou_q, self.num_classes, self.min_area)
            ops.object_count(g, labels2[0], areas[0], n_gt, self.num_classes, self.min_area)
            ops.object_count(p, labels2[1], areas[1], n_pred, self.num_classes, self.min_area)

    def compute(self, classes: Optional[Sequence[int]] = None) -> List[Dict[str, Any]]:
        return object_metrics_from_counts(*(c.cpu().numpy() for c in self.device_counts()), self.thresholds, classes)

    def reset(self) -> None:
        if self._counts is not None:
            for c in self._counts:
                c.zero_()
