"""Post-hoc calibration of the class probabilities (not in the reference).

* :class:`TemperatureFitter` fits ONE temperature T on a labelled split by minimising the cross-entropy of ``softmax(logits / T)``.
  Logits are never stored: every pass runs the network over the split once and ``ig_calib_nll_grid`` evaluates the loss at a whole
  grid of temperatures while a batch's logits are on the device.  Pass 1 is a coarse log-spaced grid, every later pass a grid inside
  the bracket around the best point, and the vertex of the parabola through the three best points (in ln T) is the result.
* :class:`RunningNLL` and :class:`RunningReliability` measure calibration at a given temperature: mean cross-entropy, and the
  reliability histograms (``ig_reliability_update``) behind the expected / maximum / class-wise calibration error.
* ``write_calibration_json`` / ``read_calibration_json`` and the option checks of ``mode=calibrate`` and ``test.temperature`` /
  ``test.calibration``.

All ratios are float64 quotients of the device sums, taken on the host once per pass.
"""
from __future__ import annotations

import json
import math
from typing import Any, Dict, List, Optional, Sequence

import numpy as np
import torch

from . import ops

__all__ = ["TemperatureFitter", "RunningNLL", "RunningReliability", "reliability_from_histogram", "write_calibration_json",
           "read_calibration_json", "check_calibrate_options", "check_temperature", "resolve_temperature", "CONF_SCALE", "MAX_POINTS"]

CONF_SCALE = float(2**24)  # hist[:, 2] holds confidences in units of 2^-24
MAX_POINTS = 32  # ig_calib_nll_grid evaluates at most 32 temperatures per launch
MAX_BINS, MAX_CELLS = 64, 4096  # ig_reliability_update


def _is_number(v) -> bool:
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def check_temperature(value, key: str = "test.temperature") -> float:
    if not _is_number(value) or not math.isfinite(value) or value <= 0:
        raise ValueError(f"{key} must be a finite number > 0 (got {value!r})")
    return float(value)


def check_calibrate_options(points=32, passes=2, t_min=0.125, t_max=8.0, nbins=15, num_classes: Optional[int] = None) -> None:
    """The ``calibrate.*`` keys (and the constructor arguments of the classes below)."""
    if not isinstance(points, int) or isinstance(points, bool) or not 3 <= points <= MAX_POINTS:
        raise ValueError(f"calibrate.points must be an integer in [3, {MAX_POINTS}] (got {points!r})")
    if not isinstance(passes, int) or isinstance(passes, bool) or not 1 <= passes <= 8:
        raise ValueError(f"calibrate.passes must be an integer in [1, 8] (got {passes!r})")
    if not (_is_number(t_min) and _is_number(t_max) and math.isfinite(t_min) and math.isfinite(t_max) and 0 < t_min < t_max):
        raise ValueError(f"calibrate.t_min / t_max must be finite with 0 < t_min < t_max (got {t_min!r}, {t_max!r})")
    if not isinstance(nbins, int) or isinstance(nbins, bool) or not 1 <= nbins <= MAX_BINS:
        raise ValueError(f"calibrate.nbins must be an integer in [1, {MAX_BINS}] (got {nbins!r})")
    if num_classes is not None and num_classes * nbins > MAX_CELLS:
        raise ValueError(f"calibrate.nbins = {nbins} with {num_classes} classes exceeds {MAX_CELLS} histogram cells")


def resolve_temperature(test_cfg: Dict[str, Any]) -> float:
    """The temperature in force for the probability products: ``test.temperature`` (None = 1.0) or the one stored in the
    ``calibration.json`` named by ``test.calibration``; giving both is an error."""
    t, path = test_cfg.get("temperature"), test_cfg.get("calibration")
    path = None if path in (None, "None") else path
    if t is not None and path is not None:
        raise ValueError("test.temperature and test.calibration are both given: choose one")
    if path is not None:
        return read_calibration_json(str(path))["temperature"]
    return 1.0 if t is None else check_temperature(t)


def _labels_for_kernel(labels: torch.Tensor) -> torch.Tensor:
    if labels.dtype not in (torch.int64, torch.int32, torch.float32):
        labels = labels.long()
    return labels.contiguous()


class TemperatureFitter:
    """Streaming fit of one softmax temperature.  Per pass: ``update`` for every batch, (sum ``device_sums()`` and ``device_count()``
    over ranks,) ``end_pass()``; after ``passes`` passes ``result()``.  ``done`` tells when no pass is left."""

    def __init__(self, t_min: float = 0.125, t_max: float = 8.0, points: int = 32, passes: int = 2, device: Optional[str] = None) -> None:
        check_calibrate_options(points, passes, t_min, t_max)
        self.points, self.passes = points, passes
        self._device = device
        self._ln_grid = np.linspace(math.log(t_min), math.log(t_max), points)
        self._sums: Optional[torch.Tensor] = None  # f64 [points + 1]: the grid, then the beta = 1 slot
        self._count: Optional[torch.Tensor] = None  # int64 [2]: #valid of the grid launch, of the beta = 1 launch
        self.history: List[Dict[str, Any]] = []
        self.at_bound = False

    @property
    def done(self) -> bool:
        return len(self.history) >= self.passes

    def grid(self) -> List[float]:
        """Temperatures of the current pass, ascending and log-spaced."""
        return np.exp(self._ln_grid).tolist()

    def device_sums(self, device=None) -> torch.Tensor:
        if self._sums is None:
            self._sums = torch.zeros(self.points + 1, dtype=torch.float64, device=device or self._device or "cuda")
        return self._sums

    def device_count(self, device=None) -> torch.Tensor:
        if self._count is None:
            self._count = torch.zeros(2, dtype=torch.int64, device=device or self._device or "cuda")
        return self._count

    def update(self, logits: torch.Tensor, labels: torch.Tensor, ignore_index: Optional[int]) -> None:
        """Add a batch: logits (B, ncls, H, W) f32, labels (B, H, W) on the device.  One ``ig_calib_nll_grid`` launch carries the grid
        and the beta = 1 slot; a grid of 32 points fills the launch, the slot then takes a second one."""
        labels = _labels_for_kernel(labels)
        logits = logits.contiguous()
        sums, count = self.device_sums(logits.device), self.device_count(logits.device)
        betas = [1.0 / t for t in self.grid()]
        if self.points + 1 <= MAX_POINTS:
            ops.calib_nll_grid(logits, labels, ignore_index, betas + [1.0], sums, count[:1])
        else:
            ops.calib_nll_grid(logits, labels, ignore_index, betas, sums, count[:1])
            ops.calib_nll_grid(logits, labels, ignore_index, [1.0], sums[self.points :], count[1:])

    def end_pass(self, sums: Optional[Sequence[float]] = None, count: Optional[int] = None) -> None:
        """Close the pass: record its sums and set the next grid to the bracket [T_(i-1), T_(i+1)] around the best grid point i.  At
        an end of the grid the bracket extends outward by one grid ratio and ``at_bound`` is set.  ``sums`` (points + 1 values) /
        ``count`` replace the device state (sums computed elsewhere)."""
        if self.done:
            raise RuntimeError(f"TemperatureFitter: all {self.passes} passes are closed")
        if sums is None:
            s = self.device_sums().cpu().numpy().astype(np.float64)
            n = int(self.device_count()[0].item())
        else:
            s = np.asarray(sums, dtype=np.float64)
            n = int(count or 0)
        if s.shape != (self.points + 1,):
            raise ValueError(f"end_pass: expected {self.points + 1} sums (the grid and the T = 1 slot), got {s.shape}")
        self.history.append({"temperatures": self.grid(), "nll_sums": s[: self.points].tolist(), "nll_sum_t1": float(s[self.points]), "n_valid": n})
        if self._sums is not None:
            self._sums.zero_()
        if self._count is not None:
            self._count.zero_()
        i = int(np.argmin(s[: self.points]))
        step = self._ln_grid[1] - self._ln_grid[0]
        if i == 0 or i == self.points - 1:
            self.at_bound = True
        lo = self._ln_grid[i] - step  # beyond the grid at an end: the same ratio outward
        hi = self._ln_grid[i] + step
        if not self.done:
            self._ln_grid = np.linspace(lo, hi, self.points)

    def result(self) -> Dict[str, Any]:
        """The fit after the last pass.  T = the vertex of the parabola through the best point of the last grid and its two neighbours
        in ln T, or that grid point when it is an end of the grid or the second difference is <= 0 (flat or non-convex triple).
        ``nll_before`` / ``nll_after`` are mean losses per valid pixel at T = 1 and at the fitted T (the parabola's value there)."""
        if not self.history:
            raise RuntimeError("TemperatureFitter.result() before any end_pass()")
        last = self.history[-1]
        f = np.asarray(last["nll_sums"], dtype=np.float64)
        x = np.log(np.asarray(last["temperatures"], dtype=np.float64))
        n = last["n_valid"]
        i = int(np.argmin(f))
        ln_t, f_min, vertex = float(x[i]), float(f[i]), False
        if 0 < i < self.points - 1:
            h = x[1] - x[0]
            d2 = f[i - 1] - 2.0 * f[i] + f[i + 1]
            if d2 > 0 and np.isfinite(d2):
                d1 = f[i + 1] - f[i - 1]
                ln_t = float(x[i] - h * d1 / (2.0 * d2))
                f_min = float(f[i] - d1 * d1 / (8.0 * d2))
                vertex = True
        nan = float("nan")
        return {"temperature": math.exp(ln_t), "ln_temperature": ln_t, "vertex": vertex, "at_bound": self.at_bound,
                "nll_before": last["nll_sum_t1"] / n if n else nan, "nll_after": f_min / n if n else nan, "n_valid": n,
                "grids": self.history}  # fmt: skip


class RunningNLL:
    """Mean cross-entropy of ``softmax(logits / T)`` over the valid pixels at each of a few fixed temperatures, device resident."""

    def __init__(self, temperatures: Sequence[float], ignore_index: Optional[int] = None, device: Optional[str] = None) -> None:
        self.temperatures = [check_temperature(t, "temperature") for t in temperatures]
        if not 1 <= len(self.temperatures) <= MAX_POINTS:
            raise ValueError(f"RunningNLL: 1 to {MAX_POINTS} temperatures")
        self.ignore_index, self._device = ignore_index, device
        self._sums: Optional[torch.Tensor] = None
        self._count: Optional[torch.Tensor] = None

    def device_sums(self, device=None) -> torch.Tensor:
        if self._sums is None:
            self._sums = torch.zeros(len(self.temperatures), dtype=torch.float64, device=device or self._device or "cuda")
        return self._sums

    def device_count(self, device=None) -> torch.Tensor:
        if self._count is None:
            self._count = torch.zeros(1, dtype=torch.int64, device=device or self._device or "cuda")
        return self._count

    def update(self, logits: torch.Tensor, labels: torch.Tensor) -> None:
        ops.calib_nll_grid(logits.contiguous(), _labels_for_kernel(labels), self.ignore_index, [1.0 / t for t in self.temperatures],
                           self.device_sums(logits.device), self.device_count(logits.device))

    def compute(self) -> List[float]:
        n = int(self.device_count().item())
        return [(v / n if n else float("nan")) for v in self.device_sums().cpu().tolist()]

    def reset(self) -> None:
        for t in (self._sums, self._count):
            if t is not None:
                t.zero_()


def reliability_from_histogram(hist) -> Dict[str, Any]:
    """ece / mce / classwise_ece and the per-bin table from the integer histogram [ncls][3][nbins] = (count, hits, confidence in 2^-24
    units) per (predicted class, bin).  ece = sum_b n_b / N |acc_b - conf_b| over the bins of all classes together, mce = the largest
    |acc_b - conf_b| of a non-empty bin, classwise_ece = the mean over the predicted classes present of the same sum inside a class.
    Empty bins have NaN accuracy / confidence and do not enter; N = 0 gives NaN everywhere."""
    h = np.asarray(hist, dtype=np.int64)
    if h.ndim != 3 or h.shape[1] != 3:
        raise ValueError(f"reliability histogram must be [ncls][3][nbins] (got {h.shape})")
    nan = float("nan")

    def gaps(cnt, hit, conf):
        c = cnt.astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            acc = np.where(cnt > 0, hit.astype(np.float64) / c, np.nan)
            cf = np.where(cnt > 0, conf.astype(np.float64) / CONF_SCALE / c, np.nan)
        return c, acc, cf

    cnt, acc, cf = gaps(h[:, 0].sum(0), h[:, 1].sum(0), h[:, 2].sum(0))
    N = float(cnt.sum())
    table = {"count": [int(v) for v in cnt], "accuracy": acc.tolist(), "confidence": cf.tolist()}
    if N == 0:
        return {"ece": nan, "mce": nan, "classwise_ece": nan, "n": 0, "bins": table}
    gap = np.abs(acc - cf)
    full = cnt > 0
    per_class = []
    for c in range(h.shape[0]):
        cc, ca, cfc = gaps(h[c, 0], h[c, 1], h[c, 2])
        if cc.sum() > 0:
            m = cc > 0
            per_class.append(float((cc[m] / cc.sum() * np.abs(ca[m] - cfc[m])).sum()))
    return {"ece": float((cnt[full] / N * gap[full]).sum()), "mce": float(gap[full].max()), "classwise_ece": float(np.mean(per_class)),
            "n": int(N), "bins": table}  # fmt: skip


class RunningReliability:
    """Streaming reliability histograms of the top-class confidence of ``softmax(logits / temperature)``, device resident (the pattern
    of :class:`instageo_amd.metrics.RunningAUC`): integer sums, so ``device_hist()`` adds across ranks like a confusion matrix."""

    def __init__(self, num_classes: int, nbins: int = 15, temperature: float = 1.0, ignore_index: Optional[int] = None,
                 device: Optional[str] = None) -> None:
        check_calibrate_options(nbins=nbins, num_classes=num_classes)
        if not 2 <= num_classes <= 127:
            raise ValueError(f"RunningReliability: 2 <= num_classes <= 127 (got {num_classes})")
        self.num_classes, self.nbins = num_classes, nbins
        self.temperature = check_temperature(temperature, "temperature")
        self.ignore_index, self._device = ignore_index, device
        self._hist: Optional[torch.Tensor] = None

    def device_hist(self, device=None) -> torch.Tensor:
        if self._hist is None:
            self._hist = torch.zeros(self.num_classes, 3, self.nbins, dtype=torch.int64, device=device or self._device or "cuda")
        return self._hist

    def update(self, logits: torch.Tensor, labels: torch.Tensor) -> None:
        """logits (B, ncls, H, W) f32, labels (B, H, W) int64|int32|f32 on the device; invalid pixels are skipped."""
        ops.reliability_update(logits.contiguous(), _labels_for_kernel(labels), self.ignore_index, 1.0 / self.temperature,
                               self.device_hist(logits.device))

    def compute(self) -> Dict[str, Any]:
        return reliability_from_histogram(self.device_hist().cpu().numpy())

    def reset(self) -> None:
        if self._hist is not None:
            self._hist.zero_()


# ---- calibration.json -----------------------------------------------------------------------------------------------------------
CALIBRATION_KEYS = ("temperature", "nll_before", "nll_after", "ece_before", "ece_after", "mce_before", "mce_after", "classwise_ece_before",
                    "classwise_ece_after", "n_valid", "at_bound", "bins_before", "bins_after", "grids")


def _jsonable(v):
    """Non-finite floats become null: the file stays standard JSON."""
    if isinstance(v, dict):
        return {k: _jsonable(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_jsonable(x) for x in v]
    if isinstance(v, (np.floating, np.integer)):
        v = v.item()
    if isinstance(v, float) and not math.isfinite(v):
        return None
    return v


def write_calibration_json(path: str, record: Dict[str, Any]) -> str:
    """Write a calibration record (the keys of ``CALIBRATION_KEYS``; the temperature must be usable) and return its one-line JSON."""
    missing = [k for k in CALIBRATION_KEYS if k not in record]
    if missing:
        raise ValueError(f"calibration record lacks {missing}")
    check_temperature(record["temperature"], "temperature")
    line = json.dumps(_jsonable(record), allow_nan=False)
    with open(path, "w") as f:
        f.write(line + "\n")
    return line


def read_calibration_json(path: str) -> Dict[str, Any]:
    with open(path) as f:
        record = json.load(f)
    if not isinstance(record, dict) or "temperature" not in record:
        raise ValueError(f"{path}: no temperature (not a calibration.json)")
    record["temperature"] = check_temperature(record["temperature"], f"{path}: temperature")
    return record
