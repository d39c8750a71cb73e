"""Boundary-quality metrics of class maps (not in the reference).

Whole-image metrics are area-weighted: interior pixels outnumber outline pixels by orders of magnitude.  The metrics here count only
the pixels within a distance d of a class boundary, where the boundary distance of a pixel is the Euclidean distance to the nearest
pixel of ANOTHER class (``ig_boundary_dist2``; invalid pixels are transparent, the image border is no boundary):

* **Boundary IoU** (Cheng et al., CVPR 2021), per class c: G_d = {gt = c, within d of a gt boundary}, P_d = {pred = c, within d of a pred
  boundary}; bIoU_c = |G_d and P_d| / |G_d or P_d|.
* **Trimap accuracy / IoU** (Kohli et al. 2009): accuracy and mean IoU of the confusion matrix restricted to the pixels within d of a
  ground-truth boundary.

:class:`RunningBoundaryMetrics` streams the integer count tables on the device (``ig_boundary_update``; they add across batches and
ranks like a confusion matrix); :func:`boundary_metrics_from_counts` takes the float64 ratios on the host once per epoch.
"""
from __future__ import annotations

import math
from typing import Any, Dict, List, Optional, Sequence

import numpy as np
import torch

from . import ops
from .metrics import metrics_from_matrix

__all__ = ["check_boundary_options", "boundary_distance", "class_maps", "RunningBoundaryMetrics", "boundary_metrics_from_counts", "MAX_DISTANCES",
           "MAX_RADIUS", "FILL"]

MAX_DISTANCES = 8  # ig_boundary_update counts at most 8 distances per launch
MAX_RADIUS = 32  # ig_boundary_dist2 searches at most 32 pixels far
FILL = -1  # the int8 value of an invalid pixel in the maps built here (class ids are 0..126)


def check_boundary_options(distances, num_classes: int = 2, regression: bool = False) -> List[float]:
    """The ``test.boundary_distances`` key (with ``test.boundary_metrics``) -> the distances as floats."""
    if regression:
        raise ValueError("test.boundary_metrics needs class maps: a regression task (is_reg_task) has none")
    if not isinstance(distances, (list, tuple)) or not 1 <= len(distances) <= MAX_DISTANCES:
        raise ValueError(f"test.boundary_distances must be a list of 1 to {MAX_DISTANCES} distances (got {distances!r})")
    for d in distances:
        if not isinstance(d, (int, float)) or isinstance(d, bool) or not math.isfinite(d) or not 1 <= d <= MAX_RADIUS:
            raise ValueError(f"test.boundary_distances: every distance must be a finite number in [1, {MAX_RADIUS}] (got {d!r})")
    ds = [float(d) for d in distances]
    for a, b in zip(ds, ds[1:]):
        if b < a:
            raise ValueError(f"test.boundary_distances must be ascending (got {distances!r})")
        if math.floor(a * a) == math.floor(b * b):
            raise ValueError(f"test.boundary_distances: {a:g} and {b:g} cover the same pixels (the same floor(d^2) = {math.floor(a * a)})")
    if not isinstance(num_classes, int) or isinstance(num_classes, bool) or not 2 <= num_classes <= 127:
        raise ValueError(f"test.boundary_metrics: class maps are int8, 2 <= num_classes <= 127 (got {num_classes!r})")
    return ds


def boundary_distance(classmap: torch.Tensor, rmax: int = MAX_RADIUS, fill: int = FILL) -> torch.Tensor:
    """(n, H, W) | (H, W) int8 class maps on the device -> int32 squared distance to the nearest pixel of another class where it is
    <= rmax^2, ``ops.BOUNDARY_FAR`` beyond, -1 at ``fill``."""
    if not isinstance(rmax, int) or isinstance(rmax, bool) or not 1 <= rmax <= MAX_RADIUS:
        raise ValueError(f"rmax must be an integer in [1, {MAX_RADIUS}] (got {rmax!r})")
    return ops.boundary_dist2(classmap.contiguous(), rmax, fill)


def boundary_metrics_from_counts(band, trimap, distances: Sequence[float]) -> List[Dict[str, Any]]:
    """One record per distance from the integer tables band [K][ncls][3] = (gt band, pred band, intersection) and trimap
    [K][ncls][ncls]: ``biou_per_class`` = inter / (gt + pred - inter), NaN where that union is 0; ``biou`` = its mean over the classes
    with a union > 0 (NaN when there is none); ``trimap_acc`` = trace / sum (NaN for an empty band); ``trimap_iou`` = the macro IoU of
    :func:`metrics_from_matrix`; ``band_pixels`` = the pixels within the distance of a ground-truth boundary."""
    b = np.asarray(band, dtype=np.int64)
    t = np.asarray(trimap, dtype=np.int64)
    K = len(distances)
    if b.ndim != 3 or b.shape[0] != K or b.shape[2] != 3 or t.shape != (K, b.shape[1], b.shape[1]):
        raise ValueError(f"boundary counts must be [K][ncls][3] and [K][ncls][ncls] with K = {K} (got {b.shape}, {t.shape})")
    out = []
    for k, d in enumerate(distances):
        inter = b[k, :, 2].astype(np.float64)
        union = (b[k, :, 0] + b[k, :, 1] - b[k, :, 2]).astype(np.float64)
        per = np.full(union.shape, np.nan)
        np.divide(inter, union, out=per, where=union > 0)
        present = union > 0
        total = int(t[k].sum())
        out.append({"distance": float(d), "biou_per_class": per.tolist(), "biou": float(per[present].mean()) if present.any() else float("nan"),
                    "trimap_acc": float(np.trace(t[k]) / total) if total else float("nan"),
                    "trimap_iou": float(metrics_from_matrix(t[k], include_per_class=False)["jaccard"]), "band_pixels": total})
    return out


def class_maps(logits_or_preds: torch.Tensor, labels: torch.Tensor, num_classes: int, ignore_index: Optional[int] = None):
    """-> (gt, pred) int8 maps of the labels' shape, on the device: gt = the label where it is valid (``ig_ce_loss``'s predicate:
    label != ignore_index and 0 <= label < ncls), fill elsewhere; pred = ``ops.argmax_i8`` of logits (B, ncls, H, W), or the given
    class map, with fill wherever gt is fill."""
    lab = labels if labels.dtype in (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8) else labels.long()
    valid = (lab >= 0) & (lab < num_classes)
    if ignore_index is not None:
        valid &= lab != int(ignore_index)
    fill = torch.full((), FILL, dtype=torch.int8, device=lab.device)
    gt = torch.where(valid, lab.to(torch.int8), fill)
    p = logits_or_preds
    if p.dim() == labels.dim() + 1:
        p = ops.argmax_i8(p.contiguous())
    elif p.dtype != torch.int8:
        p = p.clamp(-1, 127).to(torch.int8)  # a class id beyond int8 is no class of this map: 127 >= ncls never counts
    if p.shape != gt.shape:
        raise ValueError(f"predictions {tuple(p.shape)} and labels {tuple(gt.shape)} differ in shape")
    return gt.contiguous(), torch.where(valid, p, fill).contiguous()


class RunningBoundaryMetrics:
    """Streaming Boundary IoU and trimap counts at a few distances, device resident (the pattern of :class:`metrics.RunningAUC`)."""

    def __init__(self, num_classes: int, distances: Sequence[float] = (1, 2, 4), ignore_index: Optional[int] = None,
                 device: Optional[str] = None) -> None:
        self.distances = check_boundary_options(list(distances), num_classes)
        self.num_classes, self.ignore_index, self._device = num_classes, ignore_index, device
        self.rmax = int(math.ceil(max(self.distances)))
        self.thresholds = [int(math.floor(d * d)) for d in self.distances]
        self._band: Optional[torch.Tensor] = None
        self._trimap: Optional[torch.Tensor] = None

    def device_counts(self, device=None):
        """(band int64 [K, ncls, 3], trimap int64 [K, ncls, ncls]): integer sums, they add across ranks."""
        if self._band is None:
            dev, K = device or self._device or "cuda", len(self.distances)
            self._band = torch.zeros(K, self.num_classes, 3, dtype=torch.int64, device=dev)
            self._trimap = torch.zeros(K, self.num_classes, self.num_classes, dtype=torch.int64, device=dev)
        return self._band, self._trimap

    def class_maps(self, logits_or_preds: torch.Tensor, labels: torch.Tensor):
        """:func:`class_maps` with this instance's classes and ignore_index."""
        return class_maps(logits_or_preds, labels, self.num_classes, self.ignore_index)

    def update(self, logits_or_preds: torch.Tensor, labels: torch.Tensor) -> None:
        """logits (B, ncls, H, W) f32 or predictions (B, H, W), labels (B, H, W), on the device; no host copy."""
        if labels.numel() == 0:
            return
        gt, pred = self.class_maps(logits_or_preds, labels)
        band, trimap = self.device_counts(gt.device)
        both = ops.boundary_dist2(torch.stack((gt, pred)).view((-1,) + tuple(gt.shape[-2:])), self.rmax, FILL).view((2,) + tuple(gt.shape))
        ops.boundary_update(gt, pred, both[0], both[1], self.thresholds, band, trimap, self.num_classes, FILL)

    def compute(self) -> List[Dict[str, Any]]:
        band, trimap = self.device_counts()
        return boundary_metrics_from_counts(band.cpu().numpy(), trimap.cpu().numpy(), self.distances)

    def reset(self) -> None:
        if self._band is not None:
            self._band.zero_()
            self._trimap.zero_()
