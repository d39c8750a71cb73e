"""Thin torch-tensor wrappers over the C-ABI (``include/instageo_hip.h``).

PyTorch is plumbing only: it owns device memory and the current HIP stream; every arithmetic op on
the hot path is a HIP kernel reached through :func:`instageo_amd._lib.call`.  All wrappers require
contiguous CUDA(HIP) tensors and raise otherwise -- there is no CPU fallback.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib

BF16 = torch.bfloat16


class BT:
    """A bf16 device tensor, optionally *split* (hi + lo) for the bf16x3 precision mode."""

    __slots__ = ("hi", "lo")

    def __init__(self, hi: torch.Tensor, lo: Optional[torch.Tensor] = None):
        assert hi.dtype == BF16 and (lo is None or (lo.dtype == BF16 and lo.shape == hi.shape))
        self.hi, self.lo = hi, lo

    @staticmethod
    def _alloc(shape, split: bool, device, zero: bool) -> "BT":
        """hi [, lo] of one allocation, lo a fixed distance (a multiple of 256 bytes) ABOVE hi: the paired split-mode kernels (gemm8.hip
        NSEG = 2) fetch a K-tile's hi and lo chunks with ONE LDS-DMA instruction and carry that distance in the lo lanes' 32-bit offsets.
        Slices of both halves at the same position keep the distance."""
        make = torch.zeros if zero else torch.empty
        if not split:
            return BT(make(shape, dtype=BF16, device=device))
        shape = tuple(shape) if isinstance(shape, (tuple, list, torch.Size)) else (int(shape),)
        n = 1
        for d in shape:
            n *= int(d)
        pitch = (n + 127) // 128 * 128
        buf = make((2 * pitch,), dtype=BF16, device=device)
        return BT(buf[:n].view(shape), buf[pitch : pitch + n].view(shape))

    @staticmethod
    def empty(shape, split: bool, device) -> "BT":
        return BT._alloc(shape, split, device, False)

    @staticmethod
    def zeros(shape, split: bool, device) -> "BT":
        return BT._alloc(shape, split, device, True)

    @staticmethod
    def from_float(x: torch.Tensor, split: bool) -> "BT":
        x = x.contiguous().float()
        out = BT.empty(x.shape, split, x.device)
        split_bf16(x, out)
        return out

    @property
    def split(self) -> bool:
        return self.lo is not None

    @property
    def shape(self):
        return self.hi.shape

    def view(self, *shape) -> "BT":
        return BT(self.hi.view(*shape), None if self.lo is None else self.lo.view(*shape))

    def float(self) -> torch.Tensor:
        out = torch.empty(self.hi.shape, dtype=torch.float32, device=self.hi.device)
        _lib.call("ig_merge_bf16", _p(self.hi), _p(self.lo), _p(out), out.numel(), _stream())
        return out


def _p(t: Optional[torch.Tensor]):
    if t is None:
        return None
    if not t.is_cuda:
        raise _lib.HipLibraryError("instageo_amd ops need HIP device tensors (no CPU fallback)")
    if not t.is_contiguous():
        raise _lib.HipLibraryError("instageo_amd ops need contiguous tensors")
    return t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- optional per-launch HIP-event profiling (bench.py: roofline of the dominant kernels) ----------------
# PROF maps entry point -> {"work": flops or bytes summed over bracketed launches, "events": [(start, end, kernel), ...]}.
# torch.cuda.Event records on torch's current stream, which is the stream every kernel here is launched on.  Every profiled
# launch is also counted under the name of the KERNEL it started (``ig_last_kernel``: rocprofv3's name minus namespaces).
PROF = None
PROF_STRIDE = 1
PROF_KERNELS = None


def profile_begin(names, stride: int = 1) -> None:
    """Start per-launch event profiling of the named entry points.

    ``stride`` > 1 brackets only every stride-th launch of each entry point: an event pair drains the queue around the
    kernel (a few microseconds of bubble per pair), so inside a timed region only a sample is bracketed.  Pick a stride
    coprime with the per-layer launch pattern (7 is) so the sample keeps the mix of shapes.
    """
    global PROF, PROF_STRIDE, PROF_KERNELS
    PROF = {n: {"work": 0.0, "events": [], "seen": 0} for n in names}
    PROF_KERNELS = {}
    PROF_STRIDE = max(1, int(stride))


def profile_end():
    """Synchronise and return ``{"ops": {entry point: (bracketed launches, total_ms, total_work)}, "kernels": {kernel name:
    {"op", "calls" (all launches seen), "n" (bracketed), "ms", "work"}}}``."""
    global PROF, PROF_KERNELS
    prof, kern, PROF, PROF_KERNELS = PROF, PROF_KERNELS, None, None
    torch.cuda.synchronize()
    ops_out = {}
    for n, d in prof.items():
        tot = 0.0
        for a, b, k, w in d["events"]:
            ms = a.elapsed_time(b)
            tot += ms
            r = kern[k]
            r["n"] += 1
            r["ms"] += ms
            r["work"] += w
        ops_out[n] = (len(d["events"]), tot, d["work"])
    return {"ops": ops_out, "kernels": kern}


def _kernel_label(name: str) -> str:
    k = (_lib.load().ig_last_kernel() or b"").decode()
    return k or name


def _call(name: str, work: float, *args, entry: Optional[str] = None) -> None:
    """Call entry point ``entry`` (default ``name``); ``name`` is the key the launch is profiled under."""
    entry = entry or name
    if PROF is None or name not in PROF:
        _lib.call(entry, *args)
        return
    d = PROF[name]
    d["seen"] += 1
    bracket = (d["seen"] - 1) % PROF_STRIDE == 0
    if bracket:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
    _lib.load().ig_note_reset()
    _lib.call(entry, *args)
    k = _kernel_label(name)
    r = PROF_KERNELS.get(k)
    if r is None:
        r = PROF_KERNELS[k] = {"op": name, "calls": 0, "n": 0, "ms": 0.0, "work": 0.0}
    r["calls"] += 1
    if bracket:
        b.record()
        d["events"].append((a, b, k, work))
        d["work"] += work


def reserved_cus() -> int:
    return int(_lib.load().ig_get_reserved_cus())


def set_reserved_cus(n: int) -> None:
    """Compute units the persistent GEMM kernels leave free (for RCCL's kernels under data parallelism)."""
    _lib.call("ig_set_reserved_cus", int(n))


# ---- run-to-run deterministic reductions (include/instageo_hip.h: ig_set_deterministic) --------------------------------
_DET = {"grad": None, "shadow": None}


def set_deterministic(grad_flat: Optional[torch.Tensor]) -> None:
    """Register ``grad_flat`` (the flat fp32 gradient buffer) for order-independent reductions, or switch the mode off (None).

    While registered, the kernels add their bias / norm / head gradient contributions as 2^44 fixed-point integers into an int64
    shadow of the buffer; ``det_fold(lo, hi)`` adds the shadow into the gradients.  One buffer per process at a time.
    """
    if grad_flat is None:
        if _DET["grad"] is not None:
            torch.cuda.synchronize()
            _lib.call("ig_set_deterministic", None, None, 0, _stream())
        _DET["grad"] = _DET["shadow"] = None
        return
    g = _f32(grad_flat)
    if _DET["grad"] is not None and _DET["grad"].data_ptr() == g.data_ptr() and _DET["grad"].numel() == g.numel():
        return
    torch.cuda.synchronize()
    shadow = torch.zeros(g.numel(), dtype=torch.int64, device=g.device)
    _lib.call("ig_set_deterministic", _p(shadow), _p(g), g.numel(), _stream())
    _DET["grad"], _DET["shadow"] = g, shadow


def last_kernel() -> str:
    """Name of the kernel the most recent MFMA entry point of this thread launched (``ig_last_kernel``)."""
    return (_lib.load().ig_last_kernel() or b"").decode()


def last_grid() -> int:
    """Workgroups of the launch :func:`last_kernel` names, where the entry point notes its grid (``ig_last_grid``)."""
    return int(_lib.load().ig_last_grid())


def deterministic() -> bool:
    return bool(_lib.load().ig_get_deterministic())


def det_fold(lo: int, hi: int) -> None:
    """Add the fixed-point shadow sums of flat gradient range [lo, hi) into the gradients and clear them (no-op when off)."""
    if _DET["grad"] is not None and hi > lo:
        _lib.call("ig_det_fold", int(lo), int(hi), _stream())


class ZeroRanges:
    """Prepared argument block of one ``ig_zero_ranges`` launch: ``base[lo:hi] = 0`` for a device table of flat ranges."""

    __slots__ = ("n", "ranges", "_table", "_longest")

    def __init__(self, ranges, device):
        self.ranges = [(int(a), int(b)) for a, b in ranges if b > a]
        self.n = len(self.ranges)
        self._table = torch.tensor(self.ranges or [(0, 0)], dtype=torch.int64).to(device)
        self._longest = max([b - a for a, b in self.ranges], default=0)

    def launch(self, base: torch.Tensor) -> None:
        if self.n:
            _lib.call("ig_zero_ranges", _p(_f32(base)), self.n, _p(self._table), self._longest, _stream())


class DetFoldRanges:
    """Prepared argument block of one ``ig_det_fold_ranges`` launch: a device table of flat ranges [(lo, hi), ...]."""

    __slots__ = ("n", "ranges", "_table", "_longest")

    def __init__(self, ranges, device):
        self.ranges = [(int(a), int(b)) for a, b in ranges if b > a]
        self.n = len(self.ranges)
        self._table = torch.tensor(self.ranges or [(0, 0)], dtype=torch.int64).to(device)
        self._longest = max([b - a for a, b in self.ranges], default=0)

    def launch(self) -> None:
        if _DET["grad"] is not None and self.n:
            _lib.call("ig_det_fold_ranges", self.n, _p(self._table), self._longest, _stream())


def _f32(t: torch.Tensor) -> torch.Tensor:
    assert t.dtype == torch.float32, t.dtype
    return t


# ------------------------------------------------------------------------------------------------------
def split_bf16(src: torch.Tensor, out: BT) -> None:
    _lib.call("ig_split_bf16", _p(_f32(src)), _p(out.hi), _p(out.lo), src.numel(), _stream())


def normalize_chips(src: torch.Tensor, mean: torch.Tensor, std: torch.Tensor, temporal: int,
                    constant_multiplier: Optional[float] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(B, T*C, H, W) int16|f32 -> (B, C, T, H, W) f32 normalised  (dataloader.py:495-524)."""
    B, TC, H, W = src.shape
    C = TC // temporal
    assert C * temporal == TC and mean.numel() == C and std.numel() == C
    dt = {torch.int16: 0, torch.float32: 1}[src.dtype]
    if out is None:
        out = torch.empty((B, C, temporal, H, W), dtype=torch.float32, device=src.device)
    mult = 1.0 if constant_multiplier is None else float(constant_multiplier)
    _call("ig_normalize_chips", float(src.numel()) * (src.element_size() + 4), _p(src), dt, _p(_f32(mean)), _p(_f32(std)), mult,
          int(constant_multiplier is not None), _p(out), B, temporal, C, H, W, _stream())
    return out


def crop_flip_normalize(src: torch.Tensor, params: torch.Tensor, mean: torch.Tensor, std: torch.Tensor, temporal: int, im: int,
                        constant_multiplier: Optional[float] = None, labels: Optional[torch.Tensor] = None,
                        out: Optional[torch.Tensor] = None):
    """(B, T*C, Hs, Ws) int16|f32 -> (B, C, T, im, im) f32: per-chip crop at params[b] = (top, left) + optional
    hflip/vflip (params[b, 2:4]) + normalisation in one kernel; ``labels`` (B, Hs, Ws) f32 follow (dataloader.py:58-141, 527-585)."""
    B, TC, Hs, Ws = src.shape
    C = TC // temporal
    assert C * temporal == TC and mean.numel() == C and std.numel() == C
    assert params.dtype == torch.int32 and params.shape == (B, 4)
    dt = {torch.int16: 0, torch.float32: 1}[src.dtype]
    if out is None:
        out = torch.empty((B, C, temporal, im, im), dtype=torch.float32, device=src.device)
    lab_out = None
    if labels is not None:
        labels = _f32(labels)
        assert labels.shape == (B, Hs, Ws)
        lab_out = torch.empty((B, im, im), dtype=torch.float32, device=src.device)
    mult = 1.0 if constant_multiplier is None else float(constant_multiplier)
    work = float(B) * TC * im * im * (src.element_size() + 4) + (float(B) * im * im * 8 if labels is not None else 0.0)
    _call("ig_crop_flip_normalize", work, _p(src), dt, _p(_f32(mean)), _p(_f32(std)), mult, int(constant_multiplier is not None), _p(params),
          _p(out), _p(labels), _p(lab_out), B, temporal, C, Hs, Ws, im, _stream())
    return out, lab_out


def aug_rotate(buf: torch.Tensor, params: torch.Tensor, fill: float, labels: Optional[torch.Tensor] = None, label_fill: float = -1.0):
    """RandomRotation of a raw-domain batch (B, T*C, S, S) f32 [+ labels (B, S, S) f32]: nearest neighbour about the centre with
    constant fill, params (B, 8) int32 = {apply, 16.16 fixed-point inverse affine} (dataloader.py:144-187).  Returns new tensors."""
    B, CT, S, S2 = buf.shape
    assert S == S2 and buf.dtype == torch.float32 and params.dtype == torch.int32 and params.shape == (B, 8)
    out = torch.empty_like(buf)
    lab_out = None
    if labels is not None:
        labels = _f32(labels)
        assert labels.shape == (B, S, S)
        lab_out = torch.empty_like(labels)
    _call("ig_aug_rotate", float(buf.numel() + (0 if labels is None else labels.numel())) * 8, _p(buf), _p(out), _p(labels), _p(lab_out),
          _p(params), float(fill), float(label_fill), B, CT, S, _stream())
    return out, lab_out


def aug_brightness_contrast(buf: torch.Tensor, params: torch.Tensor, max_pixel: float) -> torch.Tensor:
    """RandomBrightnessContrast in place: params (B, 4) f32 = {apply, bright, contrast, 0} (dataloader.py:190-260)."""
    B, CT, S, _ = buf.shape
    assert buf.dtype == torch.float32 and params.dtype == torch.float32 and params.shape == (B, 4)
    _call("ig_aug_brightness_contrast", float(buf.numel()) * 12, _p(buf), _p(params), float(max_pixel), B, CT, S, _stream())
    return buf


def aug_blur(buf: torch.Tensor, apply: torch.Tensor, kernel2d: torch.Tensor, max_pixel: float) -> torch.Tensor:
    """RandomGaussianBlur: apply (B,) int32, kernel2d (k, k) f32 (dataloader.py:263-333).  Returns a new tensor."""
    B, CT, S, _ = buf.shape
    assert buf.dtype == torch.float32 and apply.dtype == torch.int32 and apply.numel() == B
    k = kernel2d.shape[0]
    out = torch.empty_like(buf)
    _call("ig_aug_blur", float(buf.numel()) * 8, _p(buf), _p(out), _p(apply), _p(_f32(kernel2d)), k, float(max_pixel), B, CT, S, _stream())
    return out


def aug_noise(buf: torch.Tensor, params: torch.Tensor, noise_std: float, max_pixel: float, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
    """RandomGaussianNoise in place: params (B, 2) int32 = {apply, seed}; ``noise`` = optional standard-normal field of buf's
    shape, else generated on the device from the per-chip seed (dataloader.py:336-386)."""
    B, CT, S, _ = buf.shape
    assert buf.dtype == torch.float32 and params.dtype == torch.int32 and params.shape == (B, 2)
    if noise is not None:
        noise = _f32(noise)
        assert noise.shape == buf.shape
    _call("ig_aug_noise", float(buf.numel()) * (8 if noise is None else 12), _p(buf), _p(params), _p(noise), float(noise_std), float(max_pixel),
          B, CT, S, _stream())
    return buf


def normalize_windows(tile: torch.Tensor, origins: torch.Tensor, mean: torch.Tensor, std: torch.Tensor, temporal: int, crop: int,
                      constant_multiplier: Optional[float] = None, labels: Optional[torch.Tensor] = None,
                      out: Optional[torch.Tensor] = None):
    """Sliding-window gather + normalise in ONE launch: tile (T*C, Hs, Ws) int16|f32, origins (n, 2) int32 rows (top, left) on the
    device -> (n, C, T, crop, crop) f32 normalised [+ the same windows of ``labels`` (Hs, Ws) f32 -> (n, crop, crop)]
    (process_test / crop_array, dataloader.py:588-669)."""
    TC, Hs, Ws = tile.shape
    C = TC // temporal
    n = origins.shape[0]
    assert C * temporal == TC and mean.numel() == C and std.numel() == C
    assert origins.dtype == torch.int32 and origins.dim() == 2 and origins.shape[1] == 2 and origins.device == tile.device
    dt = {torch.int16: 0, torch.float32: 1}[tile.dtype]
    if out is None:
        out = torch.empty((n, C, temporal, crop, crop), dtype=torch.float32, device=tile.device)
    else:
        assert out.shape == (n, C, temporal, crop, crop) and out.dtype == torch.float32
    lab_out = None
    if labels is not None:
        labels = _f32(labels)
        assert labels.shape == (Hs, Ws)
        lab_out = torch.empty((n, crop, crop), dtype=torch.float32, device=tile.device)
    mult = 1.0 if constant_multiplier is None else float(constant_multiplier)
    work = float(n) * TC * crop * crop * (tile.element_size() + 4) + (float(n) * crop * crop * 8 if labels is not None else 0.0)
    _call("ig_normalize_windows", work, _p(tile), dt, _p(_f32(mean)), _p(_f32(std)), mult, int(constant_multiplier is not None),
          _p(origins.contiguous()), _p(out), _p(labels), _p(lab_out), n, temporal, C, Hs, Ws, crop, _stream())
    return out, lab_out


def chip_stats(x: torch.Tensor, sums: torch.Tensor) -> None:
    """x (B, C, T, H, W) f32; sums (2C,) f64: sums[c] += per-chip mean, sums[C+c] += per-chip biased variance (mode=stats)."""
    B, C = x.shape[0], x.shape[1]
    n = x.numel() // max(B * C, 1)
    assert sums.dtype == torch.float64 and sums.numel() == 2 * C
    _call("ig_chip_stats", float(x.numel()) * 8, _p(_f32(x)), _p(sums), B, C, n, _stream())


def label_hist(labels: torch.Tensor, counts: torch.Tensor, lo: int = -1) -> None:
    """counts (nbins + 1,) int64: counts[v - lo] += #pixels with integer label v; counts[-1] collects everything else."""
    assert counts.dtype == torch.int64
    _call("ig_label_hist", float(labels.numel()) * 4, _p(_f32(labels)), _p(counts), labels.numel(), lo, counts.numel() - 1, _stream())


def patchify(img: torch.Tensor, p: int, out: BT) -> None:
    B, C, T, H, W = img.shape
    _lib.call("ig_patchify", _p(_f32(img)), _p(out.hi), _p(out.lo), B, C, T, H, W, p, _stream())


def cls_rows(x: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor, B: int, ntok: int, D: int) -> None:
    _lib.call("ig_cls_rows", _p(x), _p(cls), _p(pos), B, ntok, D, _stream())


def patch_embed_fwd(patches: BT, w: BT, bias, pos, x, batch: int, tpc: int, D: int, K: int) -> None:
    _call("ig_patch_embed_fwd", 2.0 * batch * tpc * D * K, _p(patches.hi), _p(patches.lo), _p(w.hi), _p(w.lo), _p(bias), _p(pos), _p(x), batch, tpc, D, K,
              _stream())


def layernorm_fwd(x, gamma, beta, out: BT, mean, rstd, M: int, D: int, eps: float = 1e-5, feat_T: int = 0, feat_G: int = 0,
                  ntok: int = 0) -> None:
    # algorithmic bytes: fp32 residual stream in, bf16 (hi [+ lo]) out
    _call("ig_layernorm_fwd", float(M) * D * (4 + (4 if out.lo is not None else 2)), _p(x), _p(gamma), _p(beta), _p(out.hi), _p(out.lo),
          _p(mean), _p(rstd), M, D, eps, feat_T, feat_G, ntok, _stream())


def layernorm_bwd(dy: BT, x, mean, rstd, gamma, dx, accumulate: bool, dxb: Optional[BT], dgamma, dbeta, dcol, M: int, D: int,
                  feat_T: int = 0, feat_G: int = 0, ntok: int = 0) -> None:
    nb = 2 if dy.lo is None else 4
    work = float(M) * D * (nb + 4 + 4 + (4 if accumulate else 0) + (nb if dxb else 0))  # dy, x, dx (r)w, bf16 copy of dx
    _call("ig_layernorm_bwd", work, _p(dy.hi), _p(dy.lo), _p(x), _p(mean), _p(rstd), _p(gamma), _p(dx), int(accumulate),
          _p(dxb.hi) if dxb else None, _p(dxb.lo) if dxb else None, _p(dgamma), _p(dbeta), _p(dcol), M, D, feat_T, feat_G, ntok,
          _stream())


def linear_fwd(x: BT, w: BT, bias, y: BT, M: int, N: int, K: int, act: int = 0, pre: Optional[BT] = None) -> None:
    """y = act(x @ w^T + b).  With act=1 and ``pre`` given, ``pre`` receives gelu'(x @ w^T + b) -- the elementwise factor
    :func:`linear_dgrad` applies in backward (the pre-activation itself is never needed again)."""
    _call("ig_linear_fwd", 2.0 * M * N * K, _p(x.hi), _p(x.lo), _p(w.hi), _p(w.lo), _p(bias), _p(y.hi), _p(y.lo),
              _p(pre.hi) if pre else None, _p(pre.lo) if pre else None, M, N, K, act, _stream())


def linear_residual_fwd(x: BT, w: BT, bias, resid, out, M: int, N: int, K: int) -> None:
    _call("ig_linear_residual_fwd", 2.0 * M * N * K, _p(x.hi), _p(x.lo), _p(w.hi), _p(w.lo), _p(bias), _p(resid), _p(out), M, N, K, _stream())


def linear_dgrad(dy: BT, w: Optional[BT], dx: BT, M: int, N: int, K: int, pre: Optional[BT] = None, colsum=None,
                 wt: Optional[BT] = None) -> None:
    """dx = dy @ w [* pre, the gelu' saved by linear_fwd]; ``colsum`` (fp32 [K]) additionally accumulates the column sums of dx.
    ``wt`` = the same weight stored transposed ([K][N], :func:`transpose_bf16`): the K-contiguous form (``ig_linear_dgrad_wt``)."""
    if wt is not None:
        _call("ig_linear_dgrad", 2.0 * M * N * K, _p(dy.hi), _p(dy.lo), _p(wt.hi), _p(wt.lo), _p(dx.hi), _p(dx.lo),
              _p(pre.hi) if pre else None, _p(pre.lo) if pre else None, _p(colsum), M, N, K, 1 if pre else 0, _stream(),
              entry="ig_linear_dgrad_wt")
        return
    _call("ig_linear_dgrad", 2.0 * M * N * K, _p(dy.hi), _p(dy.lo), _p(w.hi), _p(w.lo), _p(dx.hi), _p(dx.lo),
              _p(pre.hi) if pre else None, _p(pre.lo) if pre else None, _p(colsum), M, N, K, 1 if pre else 0, _stream())


def transpose_bf16(src: BT, dst: BT, R: int, C: int, batch: int = 1, src_stride: int = 0, dst_stride: int = 0) -> None:
    """dst[b] (C, R) = src[b] (R, C)^T for b < batch (strides in elements between consecutive matrices)."""
    _lib.call("ig_transpose_bf16", _p(src.hi), _p(src.lo), _p(dst.hi), _p(dst.lo), R, C, batch, src_stride, dst_stride, _stream())


def linear_wgrad(dy: BT, x: BT, dw, M: int, N: int, K: int) -> None:
    _call("ig_linear_wgrad", 2.0 * M * N * K, _p(dy.hi), _p(dy.lo), _p(x.hi), _p(x.lo), _p(dw), M, N, K, _stream())


class WgradGroup:
    """Prepared argument block of one grouped weight-gradient launch: ``items`` = [(dy, x, dw, N, K), ...] sharing the token
    count M.  The ctypes pointer / size arrays are built ONCE (building them per call costs tens of microseconds of Python --
    at small batches the step is bound by the host's launch rate), the tensors are kept alive by the object."""

    __slots__ = ("items", "M", "work", "_args")

    def __init__(self, items, M: int):
        import ctypes

        n = len(items)
        vp, ip = ctypes.c_void_p * n, ctypes.c_int * n
        split = items[0][0].lo is not None
        arrs = [vp(*[_p(it[0].hi) for it in items]), vp(*[_p(it[0].lo) for it in items]) if split else None,
                vp(*[_p(it[1].hi) for it in items]), vp(*[_p(it[1].lo) for it in items]) if split else None,
                vp(*[_p(it[2]) for it in items]), ip(*[int(it[3]) for it in items]), ip(*[int(it[4]) for it in items])]
        self.items, self.M = list(items), int(M)
        self.work = sum(2.0 * M * it[3] * it[4] for it in items)
        self._args = (n, *[None if a is None else ctypes.cast(a, ctypes.c_void_p) for a in arrs], int(M)), arrs  # arrs: keep-alive

    def launch(self, overwrite: bool = False) -> None:
        """``overwrite``: dW = dy^T x instead of dW += (the first backward of a step: no zeroed dW needed, its old contents not read)."""
        _call("ig_linear_wgrad_group", self.work, *self._args[0], int(overwrite), _stream())


def linear_wgrad_group(items, M: int, overwrite: bool = False) -> None:
    """``items`` = [(dy, x, dw, N, K), ...]: dw_g[N_g][K_g] += dy_g[M][N_g]^T @ x_g[M][K_g] for all g in ONE launch (the weight
    gradients of a Block's linears share the token count; grouped, their output tiles fill the CUs with 2-3 token ranges per
    tile instead of 7-28 and the split-K fold shrinks accordingly).  Hot loops keep a :class:`WgradGroup` instead."""
    WgradGroup(items, M).launch(overwrite)


def attention_fwd(qkv: BT, out: BT, lse, B: int, N: int, H: int, hd: int = 64) -> None:
    _call("ig_attention_fwd", 4.0 * B * H * N * N * hd, _p(qkv.hi), _p(qkv.lo), _p(out.hi), _p(out.lo), _p(lse), B, N, H, hd, _stream())


def attention_bwd(qkv: BT, out: BT, dout: BT, lse, delta, dqkv: BT, B: int, N: int, H: int, hd: int = 64, dbias=None) -> None:
    """``dbias`` (fp32 [3*H*hd], optional) += column sums of dqkv over the tokens: the bias gradient of the fused qkv Linear."""
    _call("ig_attention_bwd", 10.0 * B * H * N * N * hd, _p(qkv.hi), _p(qkv.lo), _p(out.hi), _p(out.lo), _p(dout.hi), _p(dout.lo), _p(lse), _p(delta),
              _p(dqkv.hi), _p(dqkv.lo), _p(dbias), B, N, H, hd, _stream())


def colsum(x: BT, out, M: int, C: int) -> None:
    _call("ig_colsum", float(M) * C * (2 if x.lo is None else 4), _p(x.hi), _p(x.lo), _p(out), M, C, _stream())


def patch_grad_prep(dx, out: BT, dcls, dbias, B: int, ntok: int, D: int) -> None:
    _lib.call("ig_patch_grad_prep", _p(dx), _p(out.hi), _p(out.lo), _p(dcls), _p(dbias), B, ntok, D, _stream())


def convT_fwd(x: BT, w: BT, bias, y: BT, B, H, W, Cin, Cout, seed: int = 0, p: float = 0.0, seed_dev=None) -> None:
    _call("ig_convT_fwd", 2.0 * B * H * W * Cin * Cout * 9, _p(x.hi), _p(x.lo), _p(w.hi), _p(w.lo), _p(bias), _p(y.hi), _p(y.lo), B, H, W, Cin, Cout, seed, _p(seed_dev), p,
              _stream())


def convT_dgrad(dy: BT, w: BT, dx: BT, B, H, W, Cin, Cout) -> None:
    _call("ig_convT_dgrad", 2.0 * B * H * W * Cin * Cout * 9, _p(dy.hi), _p(dy.lo), _p(w.hi), _p(w.lo), _p(dx.hi), _p(dx.lo), B, H, W, Cin, Cout, _stream())


def convT_wgrad(dy: BT, x: BT, dw, B, H, W, Cin, Cout, dbias=None) -> None:
    """dw += per-tap dy^T x; ``dbias`` (fp32 [Cout]) additionally accumulates the column sums of dy (the bias gradient)."""
    _call("ig_convT_wgrad", 2.0 * B * H * W * Cin * Cout * 9, _p(dy.hi), _p(dy.lo), _p(x.hi), _p(x.lo), _p(dw), _p(dbias), B, H, W, Cin, Cout, _stream())


def _conv_entry(op: str, B, H, W, Cin, Cout, ks: int):
    """(profiling key, work estimate, entry point, its kernel-size argument) of nn.Conv2d(kernel_size=ks, padding=1): ks = 3 has
    entry points of its own (``ig_conv3x3_*``, no size argument); 5 / 7 (the 600M head) shrink the map to H + 3 - ks and run
    ``ig_convk_*``, profiled under the 3 x 3 keys."""
    work = 2.0 * B * (H + 3 - ks) * (W + 3 - ks) * Cin * Cout * ks * ks
    return f"ig_conv3x3_{op}", work, (f"ig_conv3x3_{op}", ()) if ks == 3 else (f"ig_convk_{op}", (ks,))


def conv_fwd(x: BT, w: BT, bias, y: BT, B, H, W, Cin, Cout, ks: int = 3, bn_scale=None, bn_shift=None) -> None:
    """Convolution (+bias); with bn_scale/bn_shift also eval-mode BatchNorm + ReLU in the same epilogue."""
    key, work, (entry, k) = _conv_entry("fwd", B, H, W, Cin, Cout, ks)
    _call(key, work, _p(x.hi), _p(x.lo), _p(w.hi), _p(w.lo), _p(bias), _p(bn_scale), _p(bn_shift), _p(y.hi), _p(y.lo), B, H, W, Cin, Cout,
          *k, _stream(), entry=entry)


def conv_dgrad(dy: BT, w: BT, dx: BT, B, H, W, Cin, Cout, ks: int = 3, seed: int = 0, p: float = 0.0, seed_dev=None) -> None:
    key, work, (entry, k) = _conv_entry("dgrad", B, H, W, Cin, Cout, ks)
    _call(key, work, _p(dy.hi), _p(dy.lo), _p(w.hi), _p(w.lo), _p(dx.hi), _p(dx.lo), B, H, W, Cin, Cout, *k, seed, _p(seed_dev), p, _stream(),
          entry=entry)


def conv_wgrad(dy: BT, x: BT, dw, B, H, W, Cin, Cout, ks: int = 3, dbias=None) -> None:
    """dw += dy^T x_gathered; ``dbias`` (fp32 [Cout]) additionally accumulates the column sums of dy (the bias gradient)."""
    key, work, (entry, k) = _conv_entry("wgrad", B, H, W, Cin, Cout, ks)
    _call(key, work, _p(dy.hi), _p(dy.lo), _p(x.hi), _p(x.lo), _p(dw), _p(dbias), B, H, W, Cin, Cout, *k, _stream(), entry=entry)


def conv3x3_fwd(x: BT, w: BT, bias, y: BT, B, H, W, Cin, Cout, bn_scale=None, bn_shift=None) -> None:
    conv_fwd(x, w, bias, y, B, H, W, Cin, Cout, 3, bn_scale, bn_shift)


def conv3x3_dgrad(dy: BT, w: BT, dx: BT, B, H, W, Cin, Cout, seed: int = 0, p: float = 0.0, seed_dev=None) -> None:
    conv_dgrad(dy, w, dx, B, H, W, Cin, Cout, 3, seed, p, seed_dev)


def conv3x3_wgrad(dy: BT, x: BT, dw, B, H, W, Cin, Cout, dbias=None) -> None:
    conv_wgrad(dy, x, dw, B, H, W, Cin, Cout, 3, dbias)


def bn_eval_affine(gamma, beta, rmean, rvar, scale, shift, C: int, eps: float = 1e-5) -> None:
    _lib.call("ig_bn_eval_affine", _p(gamma), _p(beta), _p(rmean), _p(rvar), _p(scale), _p(shift), C, eps, _stream())


def bn_relu_fwd(x: BT, gamma, beta, rmean, rvar, y: BT, scale, shift, mean, rstd, sums, M: int, C: int, training: bool,
                update_running: bool, eps: float = 1e-5, momentum: float = 0.1, stats_ready: bool = False) -> None:
    """``stats_ready``: ``sums`` already holds the batch statistics (:func:`conv3x3_fwd_stats` returned True): no statistics pass."""
    nb = 2 if x.lo is None else 4
    # training: statistics pass (read) + apply pass (read + write); eval: one read + write pass
    mode = (2 if stats_ready else 1) if training else 0
    _call("ig_bn_relu_fwd", float(M) * C * nb * (3 if mode == 1 else 2), _p(x.hi), _p(x.lo), _p(gamma), _p(beta), _p(rmean), _p(rvar), _p(y.hi), _p(y.lo), _p(scale), _p(shift),
          _p(mean), _p(rstd), _p(sums), M, C, eps, momentum, mode, int(update_running), _stream())


def bn_relu_bwd(x: BT, dy: BT, scale, shift, mean, rstd, dx: BT, dgamma, dbeta, sums, M: int, C: int) -> None:
    nb = 2 if x.lo is None else 4
    # reduction pass reads x, dy; apply pass reads x, dy and writes dx
    _call("ig_bn_relu_bwd", float(M) * C * nb * 5, _p(x.hi), _p(x.lo), _p(dy.hi), _p(dy.lo), _p(scale), _p(shift), _p(mean), _p(rstd),
          _p(dx.hi), _p(dx.lo), _p(dgamma), _p(dbeta), _p(sums), M, C, _stream())


def classifier_fwd(f: BT, w, bias, logits, B: int, HW: int, C: int, ncls: int, seed: int = 0, p: float = 0.0, seed_dev=None) -> None:
    _call("ig_classifier_fwd", float(B) * HW * (C * (2 if f.lo is None else 4) + ncls * 4), _p(f.hi), _p(f.lo), _p(w), _p(bias), _p(logits), B, HW, C, ncls, seed, _p(seed_dev), p, _stream())


def classifier_bwd(dlogits, f: BT, w, df: BT, dw, db, count, B: int, HW: int, C: int, ncls: int, seed: int = 0, p: float = 0.0,
                   seed_dev=None) -> None:
    _call("ig_classifier_bwd", float(B) * HW * (2 * C * (2 if f.lo is None else 4) + ncls * 4), _p(dlogits), _p(f.hi), _p(f.lo), _p(w),
          _p(df.hi), _p(df.lo), _p(dw), _p(db), _p(count), B, HW, C, ncls, seed, _p(seed_dev), p, _stream())


def bn_stats(x: BT, gamma, beta, rmean, rvar, scale, shift, mean, rstd, sums, M: int, C: int, update_running: bool, eps: float = 1e-5,
             momentum: float = 0.1) -> None:
    """Training-mode BatchNorm statistics only (scale / shift / mean / rstd, running update): the consumer applies them."""
    _call("ig_bn_relu_fwd", float(M) * C * (2 if x.lo is None else 4), _p(x.hi), _p(x.lo), _p(gamma), _p(beta), _p(rmean), _p(rvar), None, None,
          _p(scale), _p(shift), _p(mean), _p(rstd), _p(sums), M, C, eps, momentum, 1, int(update_running), _stream())


def conv3x3_fwd_stats(x: BT, w: BT, bias, y: BT, sums, B, H, W, Cin, Cout) -> bool:
    """nn.Conv2d(k=3, padding=1) in front of a training-mode BatchNorm; True when the kernel also left the per-channel sum / sum of squares
    of its outputs in ``sums`` (f64 [2 Cout]): the BatchNorm then needs :func:`bn_finalize` only, not a statistics pass."""
    import ctypes

    fused = ctypes.c_int(0)
    _call("ig_conv3x3_fwd", 2.0 * B * H * W * Cin * Cout * 9, _p(x.hi), _p(x.lo), _p(w.hi), _p(w.lo), _p(bias), _p(y.hi), _p(y.lo), _p(sums),
          ctypes.cast(ctypes.byref(fused), ctypes.c_void_p), B, H, W, Cin, Cout, _stream(), entry="ig_conv3x3_fwd_stats")
    return bool(fused.value)


def conv3x3_cls_fwd(x: BT, w: BT, bias, bn_scale, bn_shift, y: Optional[BT], cls_w, cls_b, logits, B, H, W, C, ncls) -> bool:
    """Inference tail in one kernel: the last 3 x 3 convolution (+ eval-mode BatchNorm + ReLU) and the 1 x 1 classifier.  True when it ran
    (direct 48-channel kernel, <= 2 classes, plain bf16); False: nothing was computed, run :func:`conv3x3_fwd` + :func:`classifier_fwd`.
    ``y`` may be None: the activation is then not stored."""
    import ctypes

    if x.lo is not None:
        return False
    fused = ctypes.c_int(0)
    _call("ig_conv3x3_fwd", 2.0 * B * H * W * C * C * 9, _p(x.hi), None, _p(w.hi), None, _p(bias), _p(bn_scale), _p(bn_shift), _p(y.hi) if y is not None else None,
          _p(cls_w), _p(cls_b), _p(logits), ctypes.cast(ctypes.byref(fused), ctypes.c_void_p), B, H, W, C, C, ncls, _stream(), entry="ig_conv3x3_cls_fwd")
    return bool(fused.value)


def bn_finalize(sums, gamma, beta, rmean, rvar, scale, shift, mean, rstd, M: int, C: int, update_running: bool, eps: float = 1e-5,
                momentum: float = 0.1) -> None:
    _lib.call("ig_bn_finalize", _p(sums), _p(gamma), _p(beta), _p(rmean), _p(rvar), _p(scale), _p(shift), _p(mean), _p(rstd), M, C, eps, momentum,
              int(update_running), _stream())


def classifier_bn_fwd(x: BT, scale, shift, w, bias, logits, B: int, HW: int, C: int, ncls: int, seed: int = 0, p: float = 0.0, seed_dev=None) -> None:
    _call("ig_classifier_bn_fwd", float(B) * HW * (C * (2 if x.lo is None else 4) + ncls * 4), _p(x.hi), _p(x.lo), _p(scale), _p(shift), _p(w),
          _p(bias), _p(logits), B, HW, C, ncls, seed, _p(seed_dev), p, _stream())


def classifier_bn_bwd(dlogits, x: BT, scale, shift, mean, rstd, w, dx: BT, dw, db, dgamma, dbeta, sums, count, B: int, HW: int, C: int,
                      ncls: int, seed: int = 0, p: float = 0.0, seed_dev=None) -> None:
    # two passes over x (+ dlogits), one write of dx
    _call("ig_classifier_bn_bwd", float(B) * HW * (3 * C * (2 if x.lo is None else 4) + 2 * ncls * 4), _p(dlogits), _p(x.hi), _p(x.lo), _p(scale),
          _p(shift), _p(mean), _p(rstd), _p(w), _p(dx.hi), _p(dx.lo), _p(dw), _p(db), _p(dgamma), _p(dbeta), _p(sums), _p(count), B, HW, C, ncls,
          seed, _p(seed_dev), p, _stream())


_LABEL_DT = {torch.int64: 0, torch.int32: 1, torch.float32: 2}


def _pixel_shape(logits):
    """(B, HW, ncls) of (B, ncls, ...) logits; HW = 0 for an empty batch (the entry points return at once on B * HW == 0)."""
    B, ncls = logits.shape[0], logits.shape[1]
    return B, (logits.numel() // (B * ncls) if B * ncls else 0), ncls


def _pixel_args(logits, labels, ignore_index):
    """What every per-pixel loss / metric entry point takes: B, HW, ncls, the label pointer, the label dtype code of the C ABI and the
    ignore value (``None`` = no label is ignored: a value no label takes)."""
    return _pixel_shape(logits) + (_p(labels), _LABEL_DT[labels.dtype], -(2**62) if ignore_index is None else int(ignore_index))


def ce_loss(logits, labels, class_weights, ignore_index: int, stats, dlogits=None, preds=None, preds_i8=None, confusion=None) -> None:
    B, HW, ncls, lab, dt, ign = _pixel_args(logits, labels, ignore_index)
    work = float(B) * HW * (ncls * 4 + labels.element_size() + (ncls * 4 if dlogits is not None else 0) + (8 if preds is not None else 0)
                            + (1 if preds_i8 is not None else 0))
    _call("ig_ce_loss", work, _p(_f32(logits)), lab, dt, _p(class_weights), ign, _p(stats),
          _p(dlogits), _p(preds), _p(preds_i8), _p(confusion), B, HW, ncls, _stream())


def seg_loss(logits, labels, class_weights, ignore_index: int, stats, dlogits=None, preds=None, preds_i8=None, confusion=None, *,
             focal_gamma: float = 0.0, pixel_term: bool = True, region_weight: float = 0.0, region_smooth: float = 1.0,
             tversky=(0.5, 0.5), parts=None) -> None:
    """Focal + region (Dice / Tversky) loss, the arguments of :func:`ce_loss` first: ``stats`` (f64 [2]) += (pixel-term sum + #valid * region
    term, #valid), ``dlogits`` = the un-normalised gradient of ``stats[0]``, ``parts`` (f64 [2], optional) += the two summands.  The class
    sums of the region term run over the tensors given -- the local batch of a data-parallel rank, like the loss count."""
    B, HW, ncls, lab, dt, ign = _pixel_args(logits, labels, ignore_index)
    assert stats is None or stats.dtype == torch.float64
    assert parts is None or (parts.dtype == torch.float64 and parts.numel() >= 2)
    passes = 2 if region_weight > 0 and dlogits is not None else 1  # the region gradient re-reads logits, labels and dlogits
    work = float(B) * HW * (passes * (ncls * 4 + labels.element_size()) + (ncls * 4 * (2 * passes - 1) if dlogits is not None else 0)
                            + (8 if preds is not None else 0) + (1 if preds_i8 is not None else 0))
    _call("ig_seg_loss", work, _p(_f32(logits)), lab, dt, _p(class_weights), ign, float(focal_gamma),
          int(bool(pixel_term)), float(region_weight), float(region_smooth), float(tversky[0]), float(tversky[1]), _p(stats), _p(parts), _p(dlogits),
          _p(preds), _p(preds_i8), _p(confusion), B, HW, ncls, _stream())


def kd_loss(student_logits, teacher_logits, labels, ignore_index: Optional[int], kl_sum, dlogits=None) -> None:
    """KLDivLoss(batchmean) numerator over the valid pixels into ``kl_sum`` (f64 [1]); ``dlogits`` += softmax(s) - softmax(t)."""
    B, HW, ncls, lab, dt, ign = _pixel_args(student_logits, labels, ignore_index)
    assert teacher_logits.shape == student_logits.shape and kl_sum.dtype == torch.float64
    _call("ig_kd_loss", float(B) * HW * ncls * 12, _p(_f32(student_logits)), _p(_f32(teacher_logits)), lab, dt, ign,
          _p(kl_sum), _p(dlogits), B, HW, ncls, _stream())


def mse_loss(pred, labels, ignore_index: float, use_log_scale: bool, stats, dpred=None, msums=None, ee_bias: float = 0.05,
             ee_coef: float = 0.15, include_ee: bool = False) -> None:
    """Masked MSE of the regression head + streaming regression-metric sums (regression.py:141-191, metrics.py:330-352)."""
    n = pred.numel()
    assert labels.numel() == n and stats.dtype == torch.float64
    work = float(n) * (8 + (4 if dpred is not None else 0))
    _call("ig_mse_loss", work, _p(_f32(pred)), _p(_f32(labels)), float(ignore_index), int(use_log_scale), _p(stats), _p(dpred), _p(msums),
          float(ee_bias), float(ee_coef), int(include_ee), n, _stream())


def kd_mse_loss(pred, teacher, labels, ignore_index: float, use_log_scale: bool, total, dpred=None) -> None:
    """Regression distillation term: ``total`` (f64 [1]) += sum over valid pixels of (pred - teacher')^2; ``dpred`` += 2 (pred - teacher')
    (regression.py:477-534)."""
    n = pred.numel()
    assert teacher.numel() == n and labels.numel() == n and total.dtype == torch.float64
    _call("ig_kd_mse_loss", float(n) * (12 + (8 if dpred is not None else 0)), _p(_f32(pred)), _p(_f32(teacher)), _p(_f32(labels)),
          float(ignore_index), int(use_log_scale), _p(total), _p(dpred), n, _stream())


def auc_update(logits, labels, ignore_index: Optional[int], hist, nbins: int, min_score: float = 0.0, max_score: float = 1.0) -> None:
    """RunningAUC histograms of softmax(logits): hist int64 [2, ncls, nbins] (0 positives, 1 negatives of each class)."""
    B, HW, ncls, lab, dt, ign = _pixel_args(logits, labels, ignore_index)
    assert hist.dtype == torch.int64 and hist.numel() == 2 * ncls * nbins
    _call("ig_auc_update", float(B) * HW * (ncls * 4 + labels.element_size()), _p(_f32(logits)), lab, dt, ign,
          _p(hist), B, HW, ncls, nbins, float(min_score), float(max_score), _stream())


def calib_nll_grid(logits, labels, ignore_index: Optional[int], inv_temps, nll, count) -> None:
    """Cross-entropy of softmax(beta_k * logits) at every beta_k = 1 / T_k of ``inv_temps`` (a host sequence of 1..32 finite positive
    floats) in one pass: ``nll`` (f64 [K]) += the sums over the valid pixels, ``count`` (int64 [1]) += #valid.  Bit-reproducible."""
    import ctypes

    B, HW, ncls, lab, dt, ign = _pixel_args(logits, labels, ignore_index)
    betas = [float(b) for b in inv_temps]
    K = len(betas)
    assert nll.dtype == torch.float64 and nll.numel() >= K and count.dtype == torch.int64 and count.numel() >= 1
    _call("ig_calib_nll_grid", float(B) * HW * (ncls * 4 + labels.element_size()), _p(_f32(logits)), lab, dt, ign,
          (ctypes.c_float * max(K, 1))(*betas), K, _p(nll), _p(count), B, HW, ncls, _stream())


def reliability_update(logits, labels, ignore_index: Optional[int], inv_temp: float, hist) -> None:
    """Reliability histograms of the top-class confidence of softmax(inv_temp * logits): ``hist`` int64 [ncls, 3, nbins] += (count,
    hits, confidence in units of 2^-24) per (predicted class, confidence bin) over the valid pixels.  Integer sums: order-independent."""
    B, HW, ncls, lab, dt, ign = _pixel_args(logits, labels, ignore_index)
    assert hist.dtype == torch.int64 and hist.dim() == 3 and hist.shape[0] == ncls and hist.shape[1] == 3
    _call("ig_reliability_update", float(B) * HW * (ncls * 4 + labels.element_size()), _p(_f32(logits)), lab, dt, ign, float(inv_temp), _p(hist),
          B, HW, ncls, int(hist.shape[2]), _stream())


def softmax_prob(logits, cls: int = 1, out=None):
    """softmax(logits, dim=1)[:, cls] -> (B, H, W) f32 (predict_step, segmentation.py:202-213)."""
    B, HW, ncls = _pixel_shape(logits)
    if out is None:
        out = torch.empty((B,) + tuple(logits.shape[2:]), dtype=torch.float32, device=logits.device)
    _call("ig_softmax_prob", float(B) * HW * (ncls * 4 + 4), _p(_f32(logits)), _p(out), B, HW, ncls, int(cls), _stream())
    return out


def argmax_i8(logits, out=None):
    B, HW, ncls = _pixel_shape(logits)
    if out is None:
        out = torch.empty((B,) + tuple(logits.shape[2:]), dtype=torch.int8, device=logits.device)
    _call("ig_argmax_i8", float(B) * HW * (ncls * 4 + 1), _p(_f32(logits)), _p(out), B, HW, ncls, _stream())
    return out


def blend_weights(crop: int, blend: str, sigma_scale: float = 0.125) -> torch.Tensor:
    """(crop,) f32 window weight of one axis (the 2-D weight is the outer product): "mean" = ones; "gaussian" =
    exp(-(i - (crop-1)/2)^2 / (2 sigma^2)), sigma = sigma_scale * crop, clamped to >= 1e-3, computed in float64 and rounded once."""
    if blend == "mean":
        return torch.ones(crop, dtype=torch.float32)
    if blend != "gaussian":
        raise ValueError(f"blend must be 'mean' or 'gaussian' (got {blend!r})")
    if not sigma_scale > 0:
        raise ValueError(f"sigma_scale must be positive (got {sigma_scale})")
    i = torch.arange(crop, dtype=torch.float64) - (crop - 1) / 2.0
    sigma = float(sigma_scale) * crop
    return torch.exp(-(i * i) / (2.0 * sigma * sigma)).clamp_min(1e-3).to(torch.float32)


def window_blend_accumulate(logits, tops, lefts, w0: int, wvec, acc, wsum, H: int, y0: int = 0, rows: Optional[Tuple[int, int]] = None) -> None:
    """Add windows [w0, w0 + n) of the row-major grid tops x lefts (int32 device tensors) to a canvas band (include/instageo_hip.h):
    logits (n, ncls, crop, crop) f32, acc (ncls, Hb, W) / wsum (Hb, W) f32 = canvas rows [y0, y0 + Hb) of an H x W tile.  ``rows`` =
    (ylo, yhi), the canvas rows the batch covers (default: the whole band)."""
    n, ncls, crop = logits.shape[0], logits.shape[1], logits.shape[-1]
    Hb, W = wsum.shape
    assert acc.shape == (ncls, Hb, W) and wvec.numel() == crop and tops.dtype == torch.int32 and lefts.dtype == torch.int32
    ylo, yhi = rows if rows is not None else (y0, y0 + Hb)
    # HBM bytes: the logits once + one read and write of the canvas rows the batch covers ((ncls + 1) f32 per pixel)
    work = float(logits.numel()) * 4 + float(max(0, min(yhi, y0 + Hb) - max(ylo, y0))) * W * (ncls + 1) * 8
    _call("ig_window_blend_accumulate", work, _p(_f32(logits)), _p(tops), _p(lefts), tops.numel(), lefts.numel(), int(w0), n,
          _p(_f32(wvec)), _p(_f32(acc)), _p(_f32(wsum)), ncls, crop, int(H), W, int(y0), Hb, int(ylo), int(yhi), _stream())


def window_blend_finalize(acc, wsum, tile: Optional[torch.Tensor] = None, no_data_value: Optional[float] = None, fill: int = -1,
                          probabilities: bool = False):
    """acc (ncls, H, W) / wsum (H, W) -> (classmap (H, W) int8, prob (ncls, H, W) f32 or None); ncls == 1 (regression): (None, the
    blended value (1, H, W)).  Pixels with wsum == 0 or any band of ``tile`` (T*C, H, W) int16|f32 == ``no_data_value``: fill / NaN."""
    ncls, H, W = acc.shape
    assert wsum.shape == (H, W)
    classmap = torch.empty((H, W), dtype=torch.int8, device=acc.device) if ncls > 1 else None
    prob = torch.empty((ncls, H, W), dtype=torch.float32, device=acc.device) if (probabilities or ncls == 1) else None
    check = tile is not None and no_data_value is not None
    if check:
        assert tile.shape[1:] == (H, W)
    dt = {torch.int16: 0, torch.float32: 1}[tile.dtype] if check else 0
    work = float(H) * W * ((ncls + 1) * 4 + (tile.shape[0] * tile.element_size() if check else 0) + (1 if classmap is not None else 0)
                           + (ncls * 4 if prob is not None else 0))
    _call("ig_window_blend_finalize", work, _p(_f32(acc)), _p(_f32(wsum)), _p(tile.contiguous()) if check else None, dt,
          tile.shape[0] if check else 0, float(no_data_value) if check else 0.0, int(check), _p(classmap), _p(prob), ncls, H * W, int(fill),
          _stream())
    return classmap, prob


def d4_apply(src, codes, expand: bool, out=None):
    """The D4 transforms ``codes`` (host ints 0..7, K of them; :func:`dataloader.d4_codes`) of S x S f32 planes, bits copied.  ``expand``:
    src (m, ..., S, S) -> (m * K, ..., S, S) with out[i * K + j] = G_codes[j](src[i]); otherwise src is (m * K, ..., S, S) and
    out[i * K + j] = G_codes[j](src[i * K + j]) (the logits back in the canvas frame, with the inverse codes)."""
    import ctypes

    codes = [int(k) for k in codes]
    K, S = len(codes), src.shape[-1]
    assert src.dim() >= 3 and src.shape[-2] == S and src.dtype == torch.float32
    if not expand and src.shape[0] % max(K, 1):
        raise ValueError(f"d4_apply: {src.shape[0]} images are not whole groups of {K} transforms")
    m = src.shape[0] if expand else src.shape[0] // max(K, 1)
    P = src.numel() // (src.shape[0] * S * S) if src.shape[0] else 1
    shape = (m * K,) + tuple(src.shape[1:])
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=src.device)
    assert tuple(out.shape) == shape and out.dtype == torch.float32
    # HBM bytes: every destination element is read once and written once
    _call("ig_d4_apply", float(out.numel()) * 8, _p(src), _p(out), (ctypes.c_int * max(K, 1))(*codes), K, m, P, S, int(bool(expand)), _stream())
    return out


def window_blend_accumulate_tta(logits, tops, lefts, w0: int, wvec, acc, wsum, H: int, y0: int = 0,
                                rows: Optional[Tuple[int, int]] = None) -> None:
    """:func:`window_blend_accumulate` with K logit sets per window: logits (n, K, ncls, crop, crop) f32 in the canvas frame, a window's
    sets added in order j = 0..K-1 (bit-identical for any batching; K = 1 is :func:`window_blend_accumulate` bit for bit)."""
    n, K, ncls, crop = logits.shape[0], logits.shape[1], logits.shape[2], logits.shape[-1]
    Hb, W = wsum.shape
    assert logits.dim() == 5 and acc.shape == (ncls, Hb, W) and wvec.numel() == crop and tops.dtype == torch.int32 and lefts.dtype == torch.int32
    ylo, yhi = rows if rows is not None else (y0, y0 + Hb)
    # HBM bytes: the K logit sets once + one read and write of the canvas rows the batch covers ((ncls + 1) f32 per pixel)
    work = float(logits.numel()) * 4 + float(max(0, min(yhi, y0 + Hb) - max(ylo, y0))) * W * (ncls + 1) * 8
    _call("ig_window_blend_accumulate_tta", work, _p(_f32(logits)), _p(tops), _p(lefts), tops.numel(), lefts.numel(), int(w0), n, K,
          _p(_f32(wvec)), _p(_f32(acc)), _p(_f32(wsum)), ncls, crop, int(H), W, int(y0), Hb, int(ylo), int(yhi), _stream())


def window_blend_uncertainty(acc, wsum, tile: Optional[torch.Tensor] = None, no_data_value: Optional[float] = None, entropy: bool = True,
                             margin: bool = True, out: Optional[torch.Tensor] = None):
    """acc (ncls, H, W) / wsum (H, W) of a finished canvas -> (entropy (H, W) f32 or None, margin (H, W) f32 or None): the entropy of
    p = acc / wsum normalised by ln(ncls) and the gap between the two largest p; NaN where :func:`window_blend_finalize` writes fill.
    ``out`` (2, H, W) f32 receives [entropy, margin] (both are computed)."""
    ncls, H, W = acc.shape
    assert wsum.shape == (H, W)
    if out is not None:
        assert out.shape == (2, H, W) and out.dtype == torch.float32 and out.is_contiguous() and entropy and margin
        ent, mar = out[0], out[1]
    else:
        ent = torch.empty((H, W), dtype=torch.float32, device=acc.device) if entropy else None
        mar = torch.empty((H, W), dtype=torch.float32, device=acc.device) if margin else None
    check = tile is not None and no_data_value is not None
    if check:
        assert tile.shape[1:] == (H, W)
    dt = {torch.int16: 0, torch.float32: 1}[tile.dtype] if check else 0
    work = float(H) * W * ((ncls + 1) * 4 + (tile.shape[0] * tile.element_size() if check else 0) + 4 * (int(entropy) + int(margin)))
    _call("ig_window_blend_uncertainty", work, _p(_f32(acc)), _p(_f32(wsum)), _p(tile.contiguous()) if check else None, dt,
          tile.shape[0] if check else 0, float(no_data_value) if check else 0.0, int(check), _p(ent), _p(mar), ncls, H * W, _stream())
    return ent, mar


def _class_maps(classmap) -> Tuple[int, int, int]:
    assert classmap.dtype == torch.int8 and classmap.dim() in (2, 3), "a class map is (H, W) or (n, H, W) int8"
    H, W = classmap.shape[-2:]
    return (classmap.shape[0] if classmap.dim() == 3 else 1), H, W


def ccl_label(classmap, connectivity: int = 4, fill: int = -1, out=None):
    """Connected-component labels of (n, H, W) | (H, W) int8 class maps -> int32 of the same shape: the smallest row-major index of the
    pixel's component, -1 at ``fill`` (include/instageo_hip.h).  Raises when a capped union-find loop of the kernels gave up."""
    n, H, W = _class_maps(classmap)
    if out is None:
        out = torch.empty(classmap.shape, dtype=torch.int32, device=classmap.device)
    assert out.shape == classmap.shape and out.dtype == torch.int32
    status = torch.zeros(1, dtype=torch.int32, device=classmap.device)
    # HBM bytes: the map twice (tiles, borders) + labels written, then read and written by the flatten pass
    _call("ig_ccl_label", float(n) * H * W * 14, _p(classmap), _p(out), n, H, W, int(connectivity), int(fill), _p(status), _stream())
    if n and int(status.item()):
        raise _lib.HipLibraryError(f"ig_ccl_label: a union-find loop reached its iteration cap (status {int(status.item())}); labels are not valid")
    return out


def region_area(labels, out=None):
    """labels (n, H, W) | (H, W) int32 of :func:`ccl_label` -> int32 of the same shape: the pixel count at root positions, 0 elsewhere."""
    assert labels.dtype == torch.int32 and labels.dim() in (2, 3)
    n = labels.shape[0] if labels.dim() == 3 else 1
    if out is None:
        out = torch.empty(labels.shape, dtype=torch.int32, device=labels.device)
    assert out.shape == labels.shape and out.dtype == torch.int32
    _call("ig_region_area", float(labels.numel()) * 8, _p(labels), _p(out), n, labels.shape[-2] * labels.shape[-1], _stream())
    return out


def sieve_pass(classmap, labels, area, min_region: int, fill: int, best, changed) -> None:
    """One sieve pass on ``classmap`` in place (include/instageo_hip.h): ``best`` uint64-sized scratch (int64 tensor) of the map's shape,
    ``changed`` (1,) int32 on the device, incremented by the number of small regions reassigned."""
    n, H, W = _class_maps(classmap)
    assert labels.shape == classmap.shape and area.shape == classmap.shape and labels.dtype == torch.int32 and area.dtype == torch.int32
    assert best.numel() == classmap.numel() and best.dtype == torch.int64 and changed.dtype == torch.int32
    _call("ig_sieve_pass", float(classmap.numel()) * 30, _p(classmap), _p(labels), _p(area), int(min_region), n, H, W, int(fill), _p(best),
          _p(changed), _stream())


def region_stats(labels, rid, n_regions: int):
    """-> (n_regions, 7) int64 {area, row_min, row_max, col_min, col_max, row_sum, col_sum}; ``rid`` int32 of the labels' shape holds the
    dense region id at root positions."""
    assert labels.dtype == torch.int32 and rid.dtype == torch.int32 and rid.shape == labels.shape and labels.dim() in (2, 3)
    n = labels.shape[0] if labels.dim() == 3 else 1
    H, W = labels.shape[-2:]
    stats = torch.empty((int(n_regions), 7), dtype=torch.int64, device=labels.device)
    _call("ig_region_stats", float(labels.numel()) * 4, _p(labels), _p(rid), _p(stats), int(n_regions), n, H, W, _stream())
    return stats


BOUNDARY_FAR = 0x7FFFFFFF  # IG_BOUNDARY_FAR: no pixel of another class within rmax


def boundary_dist2(classmap, rmax: int, fill: int = -1, out=None):
    """Squared Euclidean distance of every pixel of (n, H, W) | (H, W) int8 class maps to the nearest pixel of another class -> int32 of
    the same shape: the distance when it is <= rmax^2 (1 <= rmax <= 32), else ``BOUNDARY_FAR``; -1 at ``fill``, which is transparent; the
    image border is no boundary (include/instageo_hip.h)."""
    n, H, W = _class_maps(classmap)
    if out is None:
        out = torch.empty(classmap.shape, dtype=torch.int32, device=classmap.device)
    assert out.shape == classmap.shape and out.dtype == torch.int32
    # HBM bytes: the map once (halo re-reads are L2 hits) + dist2 written
    _call("ig_boundary_dist2", float(n) * H * W * 5, _p(classmap), _p(out), n, H, W, int(rmax), int(fill), _stream())
    return out


def boundary_update(gt, pred, gt_d2, pred_d2, thresholds, band, trimap, ncls: int, fill: int = -1) -> None:
    """Boundary-band and trimap counts of class maps ``gt`` / ``pred`` (int8) and their :func:`boundary_dist2` rasters at the squared
    distances ``thresholds`` (a host sequence of 1..8 strictly ascending ints in [1, 1024]): ``band`` int64 [K, ncls, 3] += (gt band,
    pred band, their intersection) per class, ``trimap`` int64 [K, ncls, ncls] += the confusion matrix inside the gt band.  Integer sums:
    order-independent."""
    import ctypes

    ts = [int(t) for t in thresholds]
    K = len(ts)
    n, H, W = _class_maps(gt)
    assert pred.shape == gt.shape and pred.dtype == torch.int8 and gt_d2.shape == gt.shape and pred_d2.shape == gt.shape
    assert gt_d2.dtype == torch.int32 and pred_d2.dtype == torch.int32
    assert band.dtype == torch.int64 and tuple(band.shape) == (K, ncls, 3) and trimap.dtype == torch.int64 and tuple(trimap.shape) == (K, ncls, ncls)
    _call("ig_boundary_update", float(gt.numel()) * 10, _p(gt), _p(pred), _p(gt_d2), _p(pred_d2), (ctypes.c_int * max(K, 1))(*ts), K,
          _p(band), _p(trimap), n, H * W, int(ncls), int(fill), _stream())


OBJECT_EMPTY = -1  # the empty key of ig_object_pairs' table (all ones) as int64
OBJECT_MAX_PIXELS = 2**31 - 1  # n * H * W per call of the object entry points


def _object_table(keys, counts, capacity: int) -> None:
    assert keys.dtype == torch.int64 and counts.dtype == torch.int32 and keys.dim() == 1 and counts.dim() == 1
    assert keys.numel() == capacity and counts.numel() == capacity and keys.is_contiguous() and counts.is_contiguous()


def object_pairs(gt_labels, pred_labels, keys, counts, status) -> None:
    """The sparse overlap table of two label maps of :func:`ccl_label` (int32, the same shape (n, H, W) | (H, W)): ``keys`` int64 and
    ``counts`` int32 of one length, a power of two in [1024, 2^30], are cleared and then hold one entry
    ``((image * HW + gt label) << 32) | pred label`` -> shared pixels per pair of overlapping regions, ``OBJECT_EMPTY`` elsewhere, at
    positions that mean nothing.  ``status`` (1,) int32 on the device: bit 0 is set when the table was too small (then it is not valid)
    (include/instageo_objects.h)."""
    assert gt_labels.dtype == torch.int32 and pred_labels.dtype == torch.int32 and gt_labels.dim() in (2, 3)
    assert pred_labels.shape == gt_labels.shape and status.dtype == torch.int32 and status.numel() == 1
    capacity = keys.numel()
    _object_table(keys, counts, capacity)
    n = gt_labels.shape[0] if gt_labels.dim() == 3 else 1
    _call("ig_object_pairs", float(gt_labels.numel()) * 8 + capacity * 12.0, _p(gt_labels.contiguous()), _p(pred_labels.contiguous()), _p(keys),
          _p(counts), capacity, _p(status), n, gt_labels.shape[-2] * gt_labels.shape[-1], _stream())


def object_match(keys, counts, gt, pred, gt_area, pred_area, ratios, tp, iou_q, ncls: int, min_area: int = 1) -> None:
    """Matches among the entries of an :func:`object_pairs` table: a pair of regions of one class (both of at least ``min_area`` pixels)
    is a match at ``ratios[k] = (num, den)`` iff its IoU is strictly above num / den (1 to 10 host pairs in [1/2, 1)); ``tp`` int64
    [K, ncls] += 1 and ``iou_q`` int64 [K, ncls] += the IoU in units of 2^-24 per match.  ``gt`` / ``pred`` int8 class maps with their
    :func:`region_area` rasters.  Integer sums: order-independent."""
    import ctypes

    rs = [(int(a), int(b)) for a, b in ratios]
    K = len(rs)
    n, H, W = _class_maps(gt)
    assert pred.shape == gt.shape and pred.dtype == torch.int8 and gt_area.shape == gt.shape and pred_area.shape == gt.shape
    assert gt_area.dtype == torch.int32 and pred_area.dtype == torch.int32
    assert tp.dtype == torch.int64 and tuple(tp.shape) == (K, ncls) and iou_q.dtype == torch.int64 and tuple(iou_q.shape) == (K, ncls)
    capacity = keys.numel()
    _object_table(keys, counts, capacity)
    arr = ctypes.c_int * max(K, 1)
    _call("ig_object_match", capacity * 12.0, _p(keys), _p(counts), capacity, _p(gt.contiguous()), _p(pred.contiguous()),
          _p(gt_area.contiguous()), _p(pred_area.contiguous()), arr(*[a for a, _ in rs]), arr(*[b for _, b in rs]), K, _p(tp), _p(iou_q), n,
          H * W, int(ncls), int(min_area), _stream())


def object_count(classmap, labels, area, n_regions, ncls: int, min_area: int = 1) -> None:
    """``n_regions`` int64 [ncls] += the regions of every class in (n, H, W) | (H, W) int8 class maps that have at least ``min_area``
    pixels, given the maps' :func:`ccl_label` labels and :func:`region_area` areas."""
    n, H, W = _class_maps(classmap)
    assert labels.shape == classmap.shape and area.shape == classmap.shape and labels.dtype == torch.int32 and area.dtype == torch.int32
    assert n_regions.dtype == torch.int64 and tuple(n_regions.shape) == (ncls,)
    _call("ig_object_count", float(classmap.numel()) * 9, _p(classmap.contiguous()), _p(labels.contiguous()), _p(area.contiguous()),
          _p(n_regions), n, H * W, int(ncls), int(min_area), _stream())


MAX_EDGES = 2**31 - 1  # compact edge ids are int32


def edge_mask(labels):
    """labels (n, H, W) | (H, W) int32 of :func:`ccl_label` -> (mask uint8 of the same shape: bits 0-3 the live sides of the pixel, bits
    4-6 their number; total (1,) int64 on the device = the live edges of all images) (include/instageo_hip.h)."""
    assert labels.dtype == torch.int32 and labels.dim() in (2, 3)
    n = labels.shape[0] if labels.dim() == 3 else 1
    H, W = labels.shape[-2:]
    mask = torch.empty(labels.shape, dtype=torch.uint8, device=labels.device)
    total = torch.zeros(1, dtype=torch.int64, device=labels.device)
    # HBM bytes: the labels once (the rows above and below are L2 hits) + the mask written
    _call("ig_edge_mask", float(labels.numel()) * 5, _p(labels), _p(mask), _p(total), n, H, W, _stream())
    return mask, total


def edge_link(labels, mask, off, n_edges: int):
    """-> (succ (E,) int32, tail (E, 2) int32 (x, y), flag (E,) uint8 = heading | turn << 2) of the ``n_edges`` live edges; ``off`` int32 of
    the labels' shape = the exclusive scan of ``mask >> 4``.  Raises when a successor is not live (mask / off of other labels)."""
    assert labels.dtype == torch.int32 and labels.dim() in (2, 3) and mask.dtype == torch.uint8 and off.dtype == torch.int32
    assert mask.shape == labels.shape and off.shape == labels.shape
    n = labels.shape[0] if labels.dim() == 3 else 1
    H, W = labels.shape[-2:]
    E = int(n_edges)
    dev = labels.device
    succ = torch.empty(E, dtype=torch.int32, device=dev)
    tail = torch.empty((E, 2), dtype=torch.int32, device=dev)
    flag = torch.empty(E, dtype=torch.uint8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _call("ig_edge_link", float(labels.numel()) * 9 + float(E) * 17, _p(labels), _p(mask), _p(off), _p(succ), _p(tail), _p(flag), n, H, W, E,
          _p(status), _stream())
    if E and n and int(status.item()):
        raise _lib.HipLibraryError(f"ig_edge_link: an edge's successor is not live (status {int(status.item())}); mask / off do not belong to these labels")
    return succ, tail, flag


def ring_jump(phase: int, val_in, ptr_in, val_out, ptr_out, changed, root=None, flag=None) -> None:
    """One round of pointer jumping over the E edges (include/instageo_hip.h): phase 0 min-propagation, phase 1 ranking; ``val_in`` None =
    the first round (``ptr_in`` is succ; phase 1 then needs ``root`` and ``flag``).  Out of place; ``changed`` (1,) int32 on the device."""
    E = ptr_in.numel()
    for t in (val_in, ptr_in, val_out, ptr_out, root):
        assert t is None or (t.dtype == torch.int32 and t.numel() == E)
    assert changed.dtype == torch.int32 and (flag is None or (flag.dtype == torch.uint8 and flag.numel() == E))
    _call("ig_ring_jump", float(E) * 24, int(phase), _p(val_in), _p(ptr_in), _p(val_out), _p(ptr_out), _p(root), _p(flag), E, _p(changed),
          _stream())


def ring_sums(root, ring_id, tail, flag, n_rings: int):
    """-> (n_rings, 2) int64 {vertices, twice the signed area} of every ring; ``ring_id`` int32 holds the ring's row at root positions."""
    E = root.numel()
    assert root.dtype == torch.int32 and ring_id.dtype == torch.int32 and ring_id.numel() == E and flag.dtype == torch.uint8
    assert tail.dtype == torch.int32 and tuple(tail.shape) == (E, 2) and flag.numel() == E
    sums = torch.zeros((int(n_rings), 2), dtype=torch.int64, device=root.device)
    _call("ig_ring_sums", float(E) * 17, _p(root), _p(ring_id), _p(tail), _p(flag), _p(sums), E, int(n_rings), _stream())
    return sums


def ring_emit(root, ring_id, rank, tail, flag, first, n_vertices: int):
    """-> (n_vertices, 2) int32: every turn edge's tail at ``first[ring] + position`` (``rank`` = the result of the ranking rounds,
    ``first`` (n_rings,) int64).  Raises when a destination lies outside the output."""
    E = root.numel()
    assert all(t.dtype == torch.int32 and t.numel() == E for t in (root, ring_id, rank)) and flag.dtype == torch.uint8 and flag.numel() == E
    assert tail.dtype == torch.int32 and tuple(tail.shape) == (E, 2) and first.dtype == torch.int64
    V = int(n_vertices)
    vertices = torch.empty((V, 2), dtype=torch.int32, device=root.device)
    status = torch.zeros(1, dtype=torch.int32, device=root.device)
    _call("ig_ring_emit", float(E) * 9 + float(V) * 36, _p(root), _p(ring_id), _p(rank), _p(tail), _p(flag), _p(first), _p(vertices), E,
          first.numel(), V, _p(status), _stream())
    if E and int(status.item()):
        raise _lib.HipLibraryError(f"ig_ring_emit: a vertex lies outside the output (status {int(status.item())}); first / rank are not consistent")
    return vertices


ZONE_BITS = 64  # zones per pass: one bit of the uint64 canvas each


def _zone_rows(entry: str, edges, H: int):
    assert edges.dtype == torch.int32 and edges.dim() == 2 and edges.shape[1] == 4
    E = edges.shape[0]
    rows = torch.zeros(E, dtype=torch.int32, device=edges.device)
    if E:
        _call(entry, float(E) * 20, _p(edges), _p(rows), E, int(H), _stream())
    return rows


def _zone_items(entry: str, edges, bit, first, out, n_items: int) -> None:
    """One launch over ``n_items`` (edge, row) pairs that writes the (H, W) canvas ``out``."""
    E = edges.shape[0]
    assert edges.dtype == torch.int32 and edges.dim() == 2 and edges.shape[1] == 4 and bit.dtype == torch.uint8 and bit.numel() == E
    assert first.dtype == torch.int64 and first.numel() == E and out.dtype == torch.int64 and out.dim() == 2
    H, W = out.shape
    T = int(n_items)
    if E == 0 or T == 0 or H * W == 0:
        return
    # HBM bytes: per item one 8-byte atomic (ig_zone_touch: at least; how many more depends on the slopes of the edges); the edge and the
    # steps of the search are cache hits
    _call(entry, float(T) * 8, _p(edges), _p(bit), _p(first), _p(out), E, T, H, W, _stream())


def zone_edge_rows(edges, H: int):
    """edges (E, 4) int32 {x0, y0, x1, y1} in Q = 256 fixed point -> (E,) int32: the rows in [0, H) whose centre line each edge crosses
    (include/instageo_hip.h)."""
    return _zone_rows("ig_zone_edge_rows", edges, H)


def zone_toggle(edges, bit, first, canvas, n_crossings: int) -> None:
    """Flip, for each of the ``n_crossings`` (edge, crossed row) pairs, bit ``bit[e]`` of ``canvas`` (H, W) int64 at the first column whose
    centre lies at or right of the crossing; ``first`` (E,) int64 = the exclusive scan of :func:`zone_edge_rows`, ``bit`` (E,) uint8 in
    0..63.  The caller zeroes the canvas."""
    _zone_items("ig_zone_toggle", edges, bit, first, canvas, n_crossings)


def zone_tally(canvas, classmap, counts, ncls: int = 2, fill: int = -1, write_mask: bool = False) -> None:
    """Row-wise prefix XOR of the toggles in ``canvas`` (H, W) int64 = the inside masks of 64 zones, and ``counts`` (64, ncls + 1) int64 +=
    the pixels of every class inside every zone (last column: ``fill`` and values outside [0, ncls)) of ``classmap`` (H, W) int8.
    ``write_mask`` leaves the inside masks in ``canvas``; ``classmap`` None (then ``write_mask``) computes the masks only."""
    assert canvas.dtype == torch.int64 and canvas.dim() == 2
    if classmap is None:
        assert write_mask, "without a class map there is nothing to do but the masks"
        counts = None
    else:
        assert classmap.dtype == torch.int8 and classmap.shape == canvas.shape
        assert counts.dtype == torch.int64 and tuple(counts.shape) == (ZONE_BITS, int(ncls) + 1)
    H, W = canvas.shape
    if H * W == 0:
        return
    # HBM bytes: the canvas read (and written back as masks) + the class map
    _call("ig_zone_tally", float(H) * W * (8 + 8 * bool(write_mask) + (classmap is not None)), _p(canvas), _p(classmap), _p(counts), H, W,
          int(ncls), int(fill), int(bool(write_mask)), _stream())


def zone_touch_rows(edges, H: int):
    """edges (E, 4) int32 {x0, y0, x1, y1} in Q = 256 fixed point -> (E,) int32: the rows in [0, H) each edge touches under the
    all_touched rule (include/instageo_hip.h): the counterpart of :func:`zone_edge_rows`."""
    return _zone_rows("ig_zone_touch_rows", edges, H)


def zone_touch(edges, bit, first, touch, n_rows: int) -> None:
    """Set, for each of the ``n_rows`` (edge, touched row) pairs, bit ``bit[e]`` of ``touch`` (H, W) int64 in every column whose open
    square the edge meets in that row; ``first`` (E,) int64 = the exclusive scan of :func:`zone_touch_rows`.  The caller zeroes ``touch``."""
    assert touch.is_contiguous()
    _zone_items("ig_zone_touch", edges, bit, first, touch, n_rows)


def zone_touch_merge(canvas, touch) -> None:
    """``canvas`` (H, W) int64, the toggles of a pass (:func:`zone_toggle`), becomes IN PLACE the toggles of (their prefix XOR | ``touch``):
    every consumer of a toggle canvas then sees the all_touched masks.  ``touch`` (:func:`zone_touch`) is only read."""
    assert canvas.dtype == torch.int64 and canvas.dim() == 2 and touch.dtype == torch.int64 and touch.shape == canvas.shape
    assert canvas.is_contiguous() and touch.is_contiguous()
    H, W = canvas.shape
    if H * W == 0:
        return
    _call("ig_zone_touch_merge", float(H) * W * 24, _p(canvas), _p(touch), H, W, _stream())


ZONE_VALUE_BANDS = 8  # bands per launch of ig_zone_value_tally (its LDS accumulators: 32 bytes per wave, zone bit and band)


def zone_value_tally(canvas, raster, nodata: Optional[float] = None):
    """The values of ``raster`` (B, H, W) float32, 1 <= B <= ``ZONE_VALUE_BANDS``, under the inside masks of the toggles in ``canvas``
    (H, W) int64, which is read and left as it is -> (pixels (64,) int64: the inside pixels per zone bit; valid (64, B) int64: those whose
    value is finite and not ``nodata``; stats (64, B, 4) float64 {mean, M2 = sum of squared deviations from the mean, min, max} of the
    valid values; where valid is 0: 0, 0, +inf, -inf).  Merged (n, sum, M2) triples in a fixed order (include/instageo_hip.h): the same
    bits from run to run, and for a band in any group of bands."""
    if canvas.dtype != torch.int64 or canvas.dim() != 2:
        raise ValueError(f"zone_value_tally: canvas must be (H, W) int64 (got {tuple(canvas.shape)} {canvas.dtype})")
    if raster.dtype != torch.float32 or raster.dim() != 3 or tuple(raster.shape[1:]) != tuple(canvas.shape):
        raise ValueError(f"zone_value_tally: raster must be (B, H, W) float32 on the canvas's {tuple(canvas.shape)} pixels "
                         f"(got {tuple(raster.shape)} {raster.dtype})")
    B, H, W = raster.shape
    if not 1 <= B <= ZONE_VALUE_BANDS:
        raise ValueError(f"zone_value_tally: 1 <= bands <= {ZONE_VALUE_BANDS} per call (got {B}); zonal.zone_values loops over groups")
    if not (canvas.is_contiguous() and raster.is_contiguous()):
        raise ValueError("zone_value_tally: canvas and raster must be contiguous")
    dev = raster.device
    pixels = torch.zeros(ZONE_BITS, dtype=torch.int64, device=dev)
    valid = torch.zeros((ZONE_BITS, B), dtype=torch.int64, device=dev)
    stats = torch.zeros((ZONE_BITS, B, 4), dtype=torch.float64, device=dev)
    if H * W == 0:
        stats[..., 2], stats[..., 3] = float("inf"), float("-inf")
        return pixels, valid, stats
    G = int(_lib.load().ig_zone_value_grid(H))
    partials = torch.empty((G, B, ZONE_BITS, 4), dtype=torch.float64, device=dev)  # every cell is written
    pix_partials = torch.empty((G, ZONE_BITS), dtype=torch.int64, device=dev)
    # HBM bytes: the canvas and the bands read once
    _call("ig_zone_value_tally", float(H) * W * (8 + 4 * B), _p(canvas), _p(raster), _p(partials), _p(pix_partials), H, W, B,
          int(nodata is not None), float(0.0 if nodata is None else nodata), _stream())
    _call("ig_zone_value_reduce", float(G) * ZONE_BITS * (32 * B + 8), _p(partials), _p(pix_partials), _p(valid), _p(stats), _p(pixels), G, B,
          _stream())
    return pixels, valid, stats


ZONE_QUANTILES = 8  # fractions per selection of ig_zone_quantile_hist / ig_zone_quantile_pick (two rank slots each)
ZONE_QUANTILE_ROUNDS = 4  # radix rounds of 8 bits over the 32-bit keys


def zone_value_quantiles(canvas, raster, fractions, nodata: Optional[float] = None):
    """Order statistics of ``raster`` (B, H, W) float32, 1 <= B <= ``ZONE_VALUE_BANDS``, under the inside masks of the toggles in
    ``canvas`` (H, W) int64, which is read and left as it is; ``fractions``: a host sequence of 1..``ZONE_QUANTILES`` float64 in [0, 1]
    -> (valid (64, B) int64: the values that are finite and not ``nodata``, as :func:`zone_value_tally` counts them; order (64, B, Q, 2)
    float32: the sorted valid values at ranks lo = floor((valid - 1) f) and hi = min(lo + 1, valid - 1), exactly; NaN where valid is 0).
    A radix selection in ``ZONE_QUANTILE_ROUNDS`` rounds of two launches, integer atomics only (include/instageo_hip.h): the same bits
    from run to run."""
    import ctypes

    if canvas.dtype != torch.int64 or canvas.dim() != 2:
        raise ValueError(f"zone_value_quantiles: canvas must be (H, W) int64 (got {tuple(canvas.shape)} {canvas.dtype})")
    if raster.dtype != torch.float32 or raster.dim() != 3 or tuple(raster.shape[1:]) != tuple(canvas.shape):
        raise ValueError(f"zone_value_quantiles: raster must be (B, H, W) float32 on the canvas's {tuple(canvas.shape)} pixels "
                         f"(got {tuple(raster.shape)} {raster.dtype})")
    B, H, W = raster.shape
    if not 1 <= B <= ZONE_VALUE_BANDS:
        raise ValueError(f"zone_value_quantiles: 1 <= bands <= {ZONE_VALUE_BANDS} per call (got {B}); zonal.zone_quantiles loops over groups")
    fr = [float(f) for f in fractions]
    Q = len(fr)
    if not 1 <= Q <= ZONE_QUANTILES:
        raise ValueError(f"zone_value_quantiles: 1 <= fractions <= {ZONE_QUANTILES} per call (got {Q}); zonal.zone_quantiles loops over groups")
    if not all(0.0 <= f <= 1.0 for f in fr):
        raise ValueError(f"zone_value_quantiles: every fraction must lie in [0, 1] (got {fr!r})")
    if not (canvas.is_contiguous() and raster.is_contiguous()):
        raise ValueError("zone_value_quantiles: canvas and raster must be contiguous")
    dev = raster.device
    valid = torch.zeros((ZONE_BITS, B), dtype=torch.int64, device=dev)
    order = torch.full((ZONE_BITS, B, Q, 2), float("nan"), dtype=torch.float32, device=dev)
    if H * W == 0:
        return valid, order
    hist = torch.zeros((B, ZONE_BITS, 2 * Q, 256), dtype=torch.int32, device=dev)
    state = torch.empty((B, ZONE_BITS, 2 * Q, 4), dtype=torch.int32, device=dev)  # round 0 writes it
    host = (ctypes.c_double * Q)(*fr)
    nd = (int(nodata is not None), float(0.0 if nodata is None else nodata))
    for rnd in range(ZONE_QUANTILE_ROUNDS):
        # HBM bytes: the canvas and the bands read once per round; the histograms live in L2
        _call("ig_zone_quantile_hist", float(H) * W * (8 + 4 * B), _p(canvas), _p(raster), _p(state), _p(hist), H, W, B, Q, rnd, *nd, _stream())
        _call("ig_zone_quantile_pick", float(B) * ZONE_BITS * 2 * Q * (2 * 1024 + 32), _p(hist), _p(state), host, _p(valid), _p(order), B, Q, rnd,
              _stream())
    return valid, order


def burn_resolve(canvas, table, out, r0: int, c0: int, written=None) -> None:
    """One pass of the polygon burn (include/instageo_hip.h): ``canvas`` (Hp, Wp) int64 holds the toggles of up to 64 features
    (:func:`zone_toggle`); where the prefix XOR along a row is not zero, ``out[r0 + r, c0 + c] = table[highest set bit]``; other pixels
    are not written.  ``out`` (H, W) int8 | float32 may be a view with any row pitch (its columns contiguous); ``table`` (64,) of its
    dtype; ``written`` (1,) int64, when given, += the pixels stored."""
    assert canvas.dtype == torch.int64 and canvas.dim() == 2
    assert out.dim() == 2 and out.dtype in (torch.int8, torch.float32) and table.dtype == out.dtype and table.numel() == ZONE_BITS
    assert written is None or (written.dtype == torch.int64 and written.numel() == 1)
    Hp, Wp = canvas.shape
    H, W = out.shape
    if Hp * Wp == 0:
        return
    if not out.is_cuda or (W > 1 and out.stride(1) != 1) or (H > 1 and out.stride(0) < W):
        raise _lib.HipLibraryError("burn_resolve: out must be a HIP tensor with contiguous columns and a row pitch >= W")
    pitch = int(out.stride(0)) if H > 1 else W
    # HBM bytes: the canvas read once; the stores depend on the polygons (at most the rectangle)
    _call("ig_burn_resolve", float(Hp) * Wp * 8, _p(canvas), Hp, Wp, _p(table), out.element_size(), out.data_ptr(), H, W, pitch, int(r0),
          int(c0), _p(written), _stream())


def label_cells(raster, S: int, K: int = 0, ignore: int = -1):
    """Per S x S cell of ``raster`` (ny * S, nx * S) int8 | float32 -> (valid (ny, nx) int64, hist (ny, nx, K) int64 or None): the pixels
    that are not ``ignore`` (int8) / not NaN (float32), and for int8 with K > 0 those per value in [0, K)."""
    assert raster.dim() == 2 and raster.dtype in (torch.int8, torch.float32)
    S, K = int(S), int(K)
    H, W = raster.shape
    if S < 1 or H % S or W % S:
        raise _lib.HipLibraryError(f"label_cells: a raster of {H} x {W} pixels is not a whole number of {S} x {S} cells")
    ny, nx = H // S, W // S
    valid = torch.zeros((ny, nx), dtype=torch.int64, device=raster.device)
    hist = torch.zeros((ny, nx, K), dtype=torch.int64, device=raster.device) if K else None
    if ny * nx:
        _call("ig_label_cells", float(H) * W * raster.element_size(), _p(raster), ny, nx, S, raster.element_size(), int(ignore), K, _p(valid),
              _p(hist), _stream())
    return valid, hist


def pyramid_shapes(H: int, W: int, levels: int):
    """[(H_k, W_k) for k = 1..levels] with H_k = ceil(H_{k-1} / 2), W_k = ceil(W_{k-1} / 2) (include/instageo_hip.h)."""
    out = []
    for _ in range(int(levels)):
        H, W = (H + 1) // 2, (W + 1) // 2
        out.append((H, W))
    return out


def overview_mode(classmap, levels: int, fill: int = -1, ncls: int = 2, counts=None):
    """Levels 1..``levels`` of the (H, W) int8 ``classmap`` by the MODE rule (include/instageo_hip.h) -> list of int8 tensors, views of one
    buffer.  ``counts`` (ncls + 1,) int64, when given, += the class histogram of ``classmap`` (last slot: ``fill`` and values that are
    no class)."""
    assert classmap.dtype == torch.int8 and classmap.dim() == 2, "a class map is (H, W) int8"
    H, W = classmap.shape
    shapes = pyramid_shapes(H, W, levels)
    if counts is not None:
        assert counts.dtype == torch.int64 and tuple(counts.shape) == (int(ncls) + 1,)
    dst = torch.empty(sum(h * w for h, w in shapes), dtype=torch.int8, device=classmap.device)
    if H * W:
        # HBM bytes: the map read once, the levels (a third of it) written
        _call("ig_overview_mode", float(H) * W + dst.numel(), _p(classmap), H, W, int(fill), int(ncls), int(levels), _p(dst), _p(counts),
              _stream())
    out, o = [], 0
    for h, w in shapes:
        out.append(dst[o : o + h * w].view(h, w))
        o += h * w
    return out


def overview_mean(raster, levels: int):
    """Levels 1..``levels`` of the (bands, H, W) float32 ``raster`` by the MEAN rule (NaN = NODATA; include/instageo_hip.h) -> list of
    (bands, H_k, W_k) float32 tensors, views of one buffer."""
    assert raster.dtype == torch.float32 and raster.dim() == 3, "a raster is (bands, H, W) float32"
    B, H, W = raster.shape
    shapes = pyramid_shapes(H, W, levels)
    dst = torch.empty(B * sum(h * w for h, w in shapes), dtype=torch.float32, device=raster.device)
    if B * H * W:
        _call("ig_overview_mean", 4.0 * (raster.numel() + dst.numel()), _p(raster), B, H, W, int(levels), _p(dst), _stream())
    out, o = [], 0
    for h, w in shapes:
        out.append(dst[o : o + B * h * w].view(B, h, w))
        o += B * h * w
    return out


def cog_tiles(raster, tile: int, pad: int = 0, predictor: int = 1):
    """(bands, H, W) of 1-, 2- or 4-byte elements -> (bands, ny, nx, tile, tile) of the same dtype: the raster cut into tiles, the part of the
    edge tiles outside it set to the bit pattern ``pad`` (low bytes), with TIFF horizontal differencing along each tile row when
    ``predictor`` is 2 (integers only)."""
    assert raster.dim() == 3 and raster.element_size() in (1, 2, 4), "a raster is (bands, H, W) of 1-, 2- or 4-byte elements"
    B, H, W = raster.shape
    tile = int(tile)
    assert tile > 0 and tile % 16 == 0, "tile must be a multiple of 16"
    ny, nx = -(-H // tile), -(-W // tile)
    out = torch.empty((B, ny, nx, tile, tile), dtype=raster.dtype, device=raster.device)
    es = raster.element_size()
    if out.numel():
        _call("ig_cog_tiles", float(es) * (raster.numel() + out.numel()), _p(raster), B, H, W, es, int(raster.dtype.is_floating_point), tile,
              int(pad) & 0xFFFFFFFF, int(predictor), _p(out), _stream())
    return out


# ---- the marshalling layer of the raster wrappers below (mosaic_paste .. label_limit) -------------------------------------------------------
def _upload(dev, *arrays):
    """Host arrays of ONE dtype -> one tensor on ``dev`` per array, of the array's shape: views of a single transfer, in the order given, so
    no caller computes an offset and every view starts on a multiple of its element size.  An empty array still gets a valid pointer (one
    zero of its own): a kernel that is handed a list of length 0 never sees null.  The caller's names keep the views alive until the
    launch is queued; the copy is stream-ordered."""
    arrays = [a if a.size else np.zeros(1, dtype=a.dtype) for a in arrays]
    assert all(a.dtype == arrays[0].dtype for a in arrays), "one upload holds one dtype"
    buf = torch.from_numpy(arrays[0] if len(arrays) == 1 else np.concatenate(arrays, axis=None)).to(dev)
    assert buf.data_ptr() % buf.element_size() == 0, "the upload starts off its element size"  # every view a whole number of elements further
    if len(arrays) == 1:
        return [buf]
    return [v if a.ndim == 1 else v.view(a.shape) for v, a in zip(buf.split([a.size for a in arrays]), arrays)]


def _labels_on(labels, dev):
    """The labels of a warped cut (None, a tensor or a host array) -> (the labels on ``dev`` or None, their element size or 1)."""
    if labels is None:
        return None, 1
    if not torch.is_tensor(labels):
        labels = torch.from_numpy(np.ascontiguousarray(labels))
    return labels.to(dev), labels.element_size()


def _label_tail(labels, es: int, valid_bit: int, K: int, outs):
    """The arguments the three label-taking warps end on; ``outs`` as :func:`_chip_outputs` returns them."""
    return (_p(labels), es, int(valid_bit), int(K), *(_p(t) for t in outs), _stream())


# an optional (lo, hi) pair and an optional scalar as the kernels take them: a flag, then the values as ``cast`` makes them (0 without)
def _opt_pair(v, cast):
    return (1, cast(v[0]), cast(v[1])) if v is not None else (0, cast(0), cast(0))


def _opt_value(v, cast=float):
    return (1, cast(v)) if v is not None else (0, cast(0))


def _plane_outputs(planes, sizes, out, columns: int):
    """The outputs of the speckle family over the packed ``planes`` of ``sizes`` (N, 2) -> (out, counts (N, columns) int32 zeros, the
    pixels of all planes).  A new ``out`` is zeroed only where the planes leave elements of the buffer out: theirs are all written."""
    total, dev = int(planes.shape[0]), planes.device
    pixels = int((sizes[:, 0].astype(np.int64) * sizes[:, 1]).sum())
    if out is None:
        out = (torch.empty if pixels == total else torch.zeros)(total, dtype=torch.float32, device=dev)
    assert out.dtype == torch.float32 and out.shape == planes.shape and out.device == dev, "out is a float32 tensor of the size of planes"
    return out, torch.zeros((sizes.shape[0], columns), dtype=torch.int32, device=dev), pixels


def _check_bins(bin_ptr, bin_idx, blocks: int, n: int, what: str) -> None:
    """ValueError unless ``bin_ptr`` / ``bin_idx`` are the CSR lists of ``blocks`` canvas blocks over ``n`` chips or sources (``what``)."""
    if bin_ptr.shape[0] != blocks + 1 or bin_ptr[0] != 0 or (np.diff(bin_ptr) < 0).any() or bin_ptr[-1] != bin_idx.shape[0]:
        raise ValueError(f"bin_ptr must hold {blocks} + 1 ascending offsets into bin_idx, from 0 to its length")
    if bin_idx.size and (bin_idx.min() < 0 or bin_idx.max() >= n):
        raise ValueError(f"bin_idx holds a {what}")


MOSAIC_RULES = {"last": 0, "first": 1, "mode": 2, "mean": 3}  # include/instageo_hip.h
MOSAIC_BLOCK = 64  # side of the canvas block one workgroup owns, and of a bin of the chip lists
MOSAIC_LIMIT = 1 << 30  # |row0|, |col0|, h, w of a chip rectangle


def mosaic_paste(chips, starts, rects, bin_ptr, bin_idx, shape: Tuple[int, int], rule: str = "last", fill: int = -1, cover: bool = False,
                 out=None, cover_out=None):
    """The mosaic of ``ig_mosaic_paste`` (include/instageo_hip.h): ``chips`` the packed pixels of all chips, a 1-D int8 or float32 tensor
    on the device; ``starts`` (n,) int64, ``rects`` (n, 4) int32 = (row0, col0, h, w), ``bin_ptr`` / ``bin_idx`` the CSR chip lists of the
    64 x 64 canvas blocks (:func:`instageo_amd.mosaic.bins`) as host arrays: they are checked here, so that no chip read can leave
    ``chips``, and uploaded.  -> the (H, W) canvas of ``chips``' dtype, or (canvas, cover (H, W) uint8) with ``cover``.  ``out`` /
    ``cover_out``: write into these contiguous (H, W) tensors instead of new ones (every pixel is written)."""
    assert chips.dim() == 1 and chips.dtype in (torch.int8, torch.float32), "chips is the packed 1-D int8 or float32 buffer"
    es = chips.element_size()
    code = MOSAIC_RULES.get(rule)
    if code is None or (code == 2 and es != 1) or (code == 3 and es != 4):
        raise ValueError(f"rule {rule!r} does not go with {chips.dtype} chips (int8: last | first | mode, float32: last | first | mean)")
    H, W = int(shape[0]), int(shape[1])
    rects = np.ascontiguousarray(rects, dtype=np.int32).reshape(-1, 4)
    starts = np.ascontiguousarray(starts, dtype=np.int64).reshape(-1)
    bin_ptr = np.ascontiguousarray(bin_ptr, dtype=np.int32).reshape(-1)
    bin_idx = np.ascontiguousarray(bin_idx, dtype=np.int32).reshape(-1)
    n = rects.shape[0]
    blocks = -(-H // MOSAIC_BLOCK) * -(-W // MOSAIC_BLOCK)
    if starts.shape[0] != n:
        raise ValueError(f"{n} rectangles but {starts.shape[0]} starts")
    if n:
        r0, c0, h, w = (rects[:, k].astype(np.int64) for k in range(4))
        if (h < 1).any() or (w < 1).any() or max(h.max(), w.max(), np.abs(r0).max(), np.abs(c0).max()) > MOSAIC_LIMIT:
            raise ValueError("a chip rectangle needs h, w >= 1 and |row0|, |col0|, h, w <= 2^30")
        if (starts < 0).any() or (starts + h * w > chips.numel()).any():
            raise ValueError(f"a chip's pixels lie outside the packed buffer of {chips.numel()} elements")
        _check_bins(bin_ptr, bin_idx, blocks, n, "chip index outside the rectangles")
    dev = chips.device
    dst = out if out is not None else torch.empty((H, W), dtype=chips.dtype, device=dev)
    cover = cover or cover_out is not None
    cov = cover_out if cover_out is not None else torch.empty((H, W), dtype=torch.uint8, device=dev) if cover else None
    assert dst.dtype == chips.dtype and tuple(dst.shape) == (H, W) and (cov is None or (cov.dtype == torch.uint8 and tuple(cov.shape) == (H, W)))
    if H * W:
        # without chips the kernel takes null for them and their lists
        st, rc, bp, bi = (*_upload(dev, starts), *_upload(dev, rects, bin_ptr, bin_idx)) if n else (None,) * 4
        # HBM bytes: the chips read once (an upper bound where they overhang or a rule stops early) + the canvas (+ cover) written
        _call("ig_mosaic_paste", float(es) * (chips.numel() + H * W) + (H * W if cover else 0), _p(chips) if n else None, _p(st), _p(rc), n,
              _p(bp), _p(bi), H, W, es, code, int(fill), _p(dst), _p(cov), _stream())
    return (dst, cov) if cover else dst


WARP_RESAMPLING = {"nearest": 0, "bilinear": 1}  # include/instageo_hip.h
WARP_RULES = {"last": 0, "first": 1}
WARP_MAX_SOURCES = 8


def _warp_doubles(values, n: int, what: str):
    a = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
    if a.shape[0] != n:
        raise ValueError(f"{what} holds {n} doubles (got {a.shape[0]})")
    return a


def _warp_grid(grid, what: str):
    g = _warp_doubles(grid, 4, what)
    if not (np.isfinite(g).all() and g[2] > 0 and g[3] > 0):
        raise ValueError(f"{what} = (X0, Y0, sx, sy) needs finite values and positive pixel sizes (got {tuple(g)})")
    return g


def warp_coords(dst_crs, dst_grid, shape: Tuple[int, int], src_crs, src_grid, device="cuda"):
    """``ig_warp_coords`` (include/instageo_hip.h): the source pixel coordinates of every pixel centre of the ``shape`` = (H, W)
    destination grid -> a (2, H, W) float64 tensor (u, v), NaN outside the domain.  ``dst_crs`` / ``src_crs``: five doubles (kind, lon0,
    k0, FE, FN); ``dst_grid`` / ``src_grid``: (X0, Y0, sx, sy); host values, uploaded here."""
    H, W = int(shape[0]), int(shape[1])
    if H < 0 or W < 0 or H * W > 2**31 - 1 or -(-H // 4) > 65535:
        raise ValueError(f"a destination of {H} x {W} pixels is beyond the kernel's limits (H * W <= 2^31 - 1, H <= 262140)")
    meta = [_warp_doubles(dst_crs, 5, "dst_crs"), _warp_grid(dst_grid, "dst_grid"), _warp_doubles(src_crs, 5, "src_crs"),
            _warp_grid(src_grid, "src_grid")]
    uv = torch.empty((2, H, W), dtype=torch.float64, device=device)
    if H * W:
        dc, dg, sc, sg = _upload(uv.device, *meta)
        _call("ig_warp_coords", 16.0 * H * W, _p(dc), _p(dg), H, W, _p(sc), _p(sg), _p(uv), _stream())
    return uv


def warp(src, starts, src_crs, src_grid, src_size, bin_ptr, bin_idx, dst_crs, dst_grid, shape: Tuple[int, int], resampling: str = "nearest",
         rule: str = "last", fill: int = -1, src_id: bool = False, out=None, src_id_out=None):
    """The warp of ``ig_warp`` (include/instageo_hip.h): ``src`` the packed pixels of all sources, a 1-D int8 or float32 tensor on the
    device; ``starts`` (n,) int64, ``src_crs`` (n, 5), ``src_grid`` (n, 4) float64, ``src_size`` (n, 2) int32 = (h, w), ``bin_ptr`` /
    ``bin_idx`` the CSR source lists of the 64 x 64 destination blocks (:func:`instageo_amd.warp.block_lists`), ``dst_crs`` (5,),
    ``dst_grid`` (4,) as host arrays: they are checked here, so that no source read can leave ``src``, and uploaded.  -> the (H, W)
    raster of ``src``'s dtype, or (raster, src_id (H, W) uint8) with ``src_id``.  ``out`` / ``src_id_out``: write into these contiguous
    (H, W) tensors instead of new ones (every pixel is written)."""
    assert src.dim() == 1 and src.dtype in (torch.int8, torch.float32), "src is the packed 1-D int8 or float32 buffer"
    es = src.element_size()
    mode, code = WARP_RESAMPLING.get(resampling), WARP_RULES.get(rule)
    if mode is None or (mode == 1 and es != 4):
        raise ValueError(f"resampling {resampling!r} does not go with {src.dtype} rasters (int8: nearest, float32: nearest | bilinear)")
    if code is None:
        raise ValueError(f"a warp composes its sources by rule last or first (got {rule!r})")
    if isinstance(fill, bool) or not -128 <= int(fill) <= 127:
        raise ValueError(f"fill must be an int that fits int8 (got {fill!r})")
    H, W = int(shape[0]), int(shape[1])
    if H < 0 or W < 0 or H * W > 2**31 - 1 or -(-H // MOSAIC_BLOCK) > 65535:
        raise ValueError(f"a destination of {H} x {W} pixels is beyond the kernel's limits (H * W <= 2^31 - 1, H <= 65535 * {MOSAIC_BLOCK})")
    starts = np.ascontiguousarray(starts, dtype=np.int64).reshape(-1)
    n = starts.shape[0]
    if n > WARP_MAX_SOURCES:
        raise ValueError(f"one launch warps at most {WARP_MAX_SOURCES} sources (got {n})")
    src_crs = _warp_doubles(src_crs, 5 * n, "src_crs")
    src_grid = _warp_doubles(src_grid, 4 * n, "src_grid")
    for i in range(n):
        _warp_grid(src_grid[4 * i : 4 * i + 4], f"src_grid[{i}]")
    src_size = np.ascontiguousarray(src_size, dtype=np.int32).reshape(-1, 2)
    bin_ptr = np.ascontiguousarray(bin_ptr, dtype=np.int32).reshape(-1)
    bin_idx = np.ascontiguousarray(bin_idx, dtype=np.int32).reshape(-1)
    dst_crs, dst_grid = _warp_doubles(dst_crs, 5, "dst_crs"), _warp_grid(dst_grid, "dst_grid")
    blocks = -(-H // MOSAIC_BLOCK) * -(-W // MOSAIC_BLOCK)
    if src_size.shape[0] != n:
        raise ValueError(f"{n} starts but {src_size.shape[0]} sizes")
    if n:
        h, w = src_size[:, 0].astype(np.int64), src_size[:, 1].astype(np.int64)
        if (h < 1).any() or (w < 1).any() or max(h.max(), w.max()) > MOSAIC_LIMIT:
            raise ValueError("a source needs 1 <= h, w <= 2^30")
        if (starts < 0).any() or (starts + h * w > src.numel()).any():
            raise ValueError(f"a source's pixels lie outside the packed buffer of {src.numel()} elements")
        _check_bins(bin_ptr, bin_idx, blocks, n, "source index outside the sources")
    dev = src.device
    dst = out if out is not None else torch.empty((H, W), dtype=src.dtype, device=dev)
    src_id = src_id or src_id_out is not None
    sid = src_id_out if src_id_out is not None else torch.empty((H, W), dtype=torch.uint8, device=dev) if src_id else None
    assert dst.dtype == src.dtype and tuple(dst.shape) == (H, W) and (sid is None or (sid.dtype == torch.uint8 and tuple(sid.shape) == (H, W)))
    if H * W:
        dc, dg, sc, sg = _upload(dev, dst_crs, dst_grid, src_crs, src_grid)
        # without sources the kernel takes null for them, their descriptions and their lists
        st, sz, bp, bi = (*_upload(dev, starts), *_upload(dev, src_size.reshape(-1), bin_ptr, bin_idx)) if n else (None,) * 4
        # HBM bytes: the destination (+ src_id) written, and as many source pixels gathered
        _call("ig_warp", 2.0 * es * H * W + (H * W if src_id else 0), _p(src) if n else None, _p(st), _p(sc) if n else None,
              _p(sg) if n else None, _p(sz), n, _p(bp), _p(bi), _p(dc), _p(dg), H, W, es, mode, code, int(fill), _p(dst), _p(sid), _stream())
    return (dst, sid) if src_id else dst


def _chip_outputs(out, dev, shape, dtype, labels=None, K: int = 0):
    """The output tensors of a chip launch, checked.  ``out``: None, or a dict with any of ``chips``, ``validity`` and (with ``labels``, on
    the device) ``maps``: contiguous tensors to write into instead of new ones.  -> (chips ``shape`` = (n, T * C, S, S) of ``dtype``,
    valid_values (n,) int32 zeros, validity (n, S, S) uint8, maps like ``labels``, valid_labels (n,) int32 zeros, hist (n, K) int32 zeros),
    the order the wrappers return them in and the kernels take them in: the last three None without labels, hist None with K = 0."""
    n, S = shape[0], shape[-1]
    out = dict(out or {})
    chips = out.pop("chips", None)
    plane = out.pop("validity", None)
    maps = out.pop("maps", None) if labels is not None else None
    assert not out, f"unknown outputs {sorted(out)}"
    chips = chips if chips is not None else torch.empty(shape, dtype=dtype, device=dev)
    plane = plane if plane is not None else torch.empty((n, S, S), dtype=torch.uint8, device=dev)
    assert chips.dtype == dtype and tuple(chips.shape) == tuple(shape) and plane.dtype == torch.uint8 and tuple(plane.shape) == (n, S, S)
    valid = torch.zeros((n,), dtype=torch.int32, device=dev)
    valid_labels = hist = None
    if labels is not None:
        maps = maps if maps is not None else torch.empty_like(labels)
        assert maps.dtype == labels.dtype and tuple(maps.shape) == (n, S, S)
        valid_labels = torch.zeros((n,), dtype=torch.int32, device=dev)
        hist = torch.zeros((n, K), dtype=torch.int32, device=dev) if K else None
    return chips, valid, plane, maps, valid_labels, hist


def chip_cut(tile, fmask, origins, S: int, T: int, mask_bits: int = 0, strategy: str = "each", no_data_value: int = 0, clip=None):
    """``ig_chip_cut`` (include/instageo_hip.h): ``tile`` (T * C, H, W) int16 and ``fmask`` (T, H, W) uint8 or None on the device,
    ``origins`` (n, 2) = (row0, col0) as a host array: it is checked here, so that every chip lies wholly inside the tile, and uploaded.
    -> (chips (n, T * C, S, S) int16, valid_values (n,) int32, validity (n, S, S) uint8)."""
    from . import chips as C

    assert tile.dtype == torch.int16 and tile.dim() == 3, "a tile is (T * C, H, W) int16"
    assert fmask is None or fmask.dtype == torch.uint8, "an Fmask is (T, H, W) uint8"
    o = C.check_cut(tuple(tile.shape), None if fmask is None else tuple(fmask.shape), origins, S, T, mask_bits, strategy, no_data_value, clip)
    n, (TC, H, W) = o.shape[0], tile.shape
    dev = tile.device
    chips, valid, plane = _chip_outputs(None, dev, (n, TC, S, S), torch.int16)[:3]
    if n:
        (od,) = _upload(dev, o)
        # HBM bytes: the chips' windows of the tile and the Fmask read, the chips and the validity plane written
        _call("ig_chip_cut", float(n) * S * S * (4 * TC + (T if fmask is not None else 0) + 1), _p(tile), _p(fmask), _p(od), n, int(T), TC // int(T),
              H, W, int(S), int(mask_bits), C.STRATEGIES[strategy], int(no_data_value), *_opt_pair(clip, int), _p(chips), _p(valid), _p(plane),
              _stream())
    return chips, valid, plane


def s2_chip_cut(bands, starts, geom, scl, scl_starts, scl_geom, origins, S: int, out_grid, T: int, class_bits: int = 0,
                strategy: str = "each", no_data_value: int = 0, boa_offset: int = 0, valid_range=None):
    """``ig_s2_chip_cut`` (include/instageo_hip.h): ``bands`` the packed uint16 planes and ``scl`` the packed uint8 SCL planes (or None) as
    1-D tensors on the device; ``starts`` / ``geom`` ((T * C,) element offsets, (T * C, 3) = H, W, pixel size), ``scl_starts`` /
    ``scl_geom`` (T of each) and ``origins`` (n, 2) as host arrays: they are checked here (every plane inside its buffer, every chip
    wholly inside the output grid ``out_grid`` = (H_o, W_o, p_o)) and uploaded.
    -> (chips (n, T * C, S, S) uint16, valid_values (n,) int32, validity (n, S, S) uint8)."""
    from . import s2_chips as S2

    assert bands.dtype == torch.uint16 and bands.dim() == 1, "the band planes are one packed 1-D uint16 buffer"
    assert scl is None or (scl.dtype == torch.uint8 and scl.dim() == 1), "the SCL planes are one packed 1-D uint8 buffer"
    st, g, sst, sg, o = S2.check_cut(int(bands.shape[0]), starts, geom, None if scl is None else int(scl.shape[0]), scl_starts, scl_geom,
                                     origins, S, out_grid, T, class_bits, strategy, no_data_value, boa_offset, valid_range)
    n, TC, S = o.shape[0], g.shape[0], int(S)
    Ho, Wo, po = (int(v) for v in out_grid)
    dev = bands.device
    chips, valid, plane = _chip_outputs(None, dev, (n, TC, S, S), torch.uint16)[:3]
    if n:
        od, gd = _upload(dev, o, np.concatenate([g, sg]) if scl is not None else g)  # one geometry table: the bands' rows, then the SCL planes'
        sd, ssd = _upload(dev, st, sst) if scl is not None else (*_upload(dev, st), None)
        # HBM bytes: the chips and the validity plane written, the bands read at their own resolution (at most the bytes written)
        _call("ig_s2_chip_cut", float(n) * S * S * (4 * TC + (T if scl is not None else 0) + 1), _p(bands), _p(sd), _p(scl), _p(ssd), _p(gd),
              _p(od), n, int(T), TC // int(T), Ho, Wo, po, S, int(class_bits), S2.STRATEGIES[strategy], int(no_data_value), int(boa_offset),
              *_opt_pair(valid_range, int), _p(chips), _p(valid), _p(plane), _stream())
    return chips, valid, plane


def chip_labels(origins, S: int, ptr, pts, labels, w: int, validity, valid_bit: int, K: int, device="cuda"):
    """``ig_chip_labels`` (include/instageo_hip.h): ``origins`` (n, 2), ``ptr`` (n + 1,), ``pts`` (m, 3) = (row, col, original index) and
    ``labels`` (P,) int16 | float32 as host arrays: they are checked here (ptr monotone, every point inside its chip, every index inside
    the labels) and uploaded; ``validity`` the (n, S, S) uint8 plane of :func:`chip_cut` on the device, or None with ``valid_bit`` 0.
    -> (maps (n, S, S) of the labels' dtype, valid_labels (n,) int32, hist (n, K) int32 or None)."""
    from . import chips as C

    labels = np.ascontiguousarray(labels)
    assert labels.dtype in (np.int16, np.float32) and labels.ndim == 1, "labels is a 1-D int16 or float32 array"
    task = "seg" if labels.dtype == np.int16 else "reg"
    strat = {0: None, 1: "any", 2: "each"}[int(valid_bit)]
    assert (validity is None) == (strat is None), "a validity plane goes with valid_bit 1 or 2"
    o, p, q = C.check_labels(origins, S, ptr, pts, labels.shape[0], w, K, task, strat)
    n = o.shape[0]
    dev = validity.device if validity is not None else torch.device(device)
    assert validity is None or (validity.dtype == torch.uint8 and tuple(validity.shape) == (n, S, S))
    maps = torch.empty((n, S, S), dtype=torch.int16 if task == "seg" else torch.float32, device=dev)
    valid = torch.zeros((n,), dtype=torch.int32, device=dev)
    hist = torch.zeros((n, K), dtype=torch.int32, device=dev) if K else None
    if n:
        (od, pd, qd), (ld,) = _upload(dev, o, p, q.reshape(-1)), _upload(dev, labels)
        _call("ig_chip_labels", float(n) * S * S * (labels.itemsize + (validity is not None)), _p(od), n, int(S), _p(pd), _p(qd), _p(ld),
              labels.shape[0], labels.itemsize, int(w), _p(validity), int(valid_bit), int(K), _p(maps), _p(valid), _p(hist), _stream())
    return maps, valid, hist


def chip_warp(tile, fmask, src_crs, src_grid, dst_crs, dst_grids, S: int, T: int, mask_bits: int = 0, strategy: str = "each",
              no_data_value: int = 0, clip=None, labels=None, valid_bit: int = 0, K: int = 0, out=None):
    """``ig_chip_warp`` (include/instageo_hip.h): ``tile`` (T * C, H, W) int16 and ``fmask`` (T, H, W) uint8 or None on the device;
    ``src_crs`` / ``dst_crs`` five doubles, ``src_grid`` (X0, Y0, sx, sy) and ``dst_grids`` (n, 4) as host values: they are checked here,
    before the upload.  ``labels``: None, or (n, S, S) int8 | float32 as a device tensor or a host array.  -> (chips (n, T * C, S, S)
    int16, valid_values (n,) int32, validity (n, S, S) uint8, maps, valid_labels, hist): the last three None without labels, hist None
    with K = 0.  ``out``: a dict with any of ``chips``, ``validity``, ``maps``: contiguous tensors to write into instead of new ones
    (every element is written)."""
    from . import raster_chips as R

    assert tile.dtype == torch.int16 and tile.dim() == 3, "a tile is (T * C, H, W) int16"
    assert fmask is None or fmask.dtype == torch.uint8, "an Fmask is (T, H, W) uint8"
    lab_dtype = None if labels is None else str(labels.dtype).replace("torch.", "")
    sc, sg, dc, dg = R.check_warp(tuple(tile.shape), None if fmask is None else tuple(fmask.shape), src_crs, src_grid, dst_crs, dst_grids, S, T,
                                  mask_bits, strategy, no_data_value, clip, None if labels is None else tuple(labels.shape), lab_dtype,
                                  valid_bit, K)
    n, (TC, H, W), S = dg.shape[0], tile.shape, int(S)
    dev = tile.device
    labels, es = _labels_on(labels, dev)
    outs = _chip_outputs(out, dev, (n, TC, S, S), torch.int16, labels, K)
    if n:
        scd, sgd, dcd, dgd = _upload(dev, sc, sg, dc, dg.reshape(-1))
        # HBM bytes: as many tile values and Fmask bytes gathered as chip values written, the validity plane, the labels in and out
        work = float(n) * S * S * (4 * TC + (T if fmask is not None else 0) + 1 + (2 * es if labels is not None else 0))
        _call("ig_chip_warp", work, _p(tile), _p(fmask), _p(scd), _p(sgd), _p(dcd), _p(dgd), n, int(T), TC // int(T), H, W, S, int(mask_bits),
              R.STRATEGIES[strategy], int(no_data_value), *_opt_pair(clip, int), *_label_tail(labels, es, valid_bit, K, outs))
    return outs


def s2_chip_warp(bands, starts, plane_class, class_grid, class_size, scl, scl_starts, src_crs, dst_crs, dst_grids, S: int, T: int,
                 class_bits: int = 0, strategy: str = "each", no_data_value: int = 0, boa_offset: int = 0, valid_range=None, labels=None,
                 valid_bit: int = 0, K: int = 0, out=None):
    """``ig_s2_chip_warp`` (include/instageo_hip.h): ``bands`` the packed uint16 planes and ``scl`` the packed uint8 SCL planes (or None)
    as 1-D tensors on the device; ``starts`` (T * C,), ``scl_starts`` (T,), ``plane_class`` (one entry per band plane, then one per SCL
    plane), ``class_grid`` (G, 4) = (X0, Y0, sx, sy), ``class_size`` (G, 2) = (H, W), ``src_crs`` / ``dst_crs`` five doubles and
    ``dst_grids`` (n, 4) as host values: they are checked here (every class index in [0, G), every plane inside its buffer) and
    uploaded.  ``labels``: None, or (n, S, S) int8 | float32 as a device tensor or a host array.  -> (chips (n, T * C, S, S) uint16,
    valid_values (n,) int32, validity (n, S, S) uint8, maps, valid_labels, hist): the last three None without labels, hist None with
    K = 0.  ``out``: a dict with any of ``chips``, ``validity``, ``maps``: contiguous tensors to write into instead of new ones (every
    element is written)."""
    from . import s2_raster_chips as R

    assert bands.dtype == torch.uint16 and bands.dim() == 1, "the band planes are one packed 1-D uint16 buffer"
    assert scl is None or (scl.dtype == torch.uint8 and scl.dim() == 1), "the SCL planes are one packed 1-D uint8 buffer"
    lab_dtype = None if labels is None else str(labels.dtype).replace("torch.", "")
    st, sst, pc, cg, cs, sc, dc, dg = R.check_warp(int(bands.shape[0]), starts, plane_class, class_grid, class_size,
                                                   None if scl is None else int(scl.shape[0]), scl_starts, src_crs, dst_crs, dst_grids, S, T,
                                                   class_bits, strategy, no_data_value, boa_offset, valid_range,
                                                   None if labels is None else tuple(labels.shape), lab_dtype, valid_bit, K)
    n, TC, G, S, T = dg.shape[0], st.shape[0], cg.shape[0], int(S), int(T)
    dev = bands.device
    labels, es = _labels_on(labels, dev)
    outs = _chip_outputs(out, dev, (n, TC, S, S), torch.uint16, labels, K)
    if n:
        scd, dcd, cgd, dgd = _upload(dev, sc, dc, cg.reshape(-1), dg.reshape(-1))
        pcd, csd = _upload(dev, pc, cs.reshape(-1))
        sd, ssd = _upload(dev, st, sst) if scl is not None else (*_upload(dev, st), None)
        # HBM bytes: the chips and the validity plane written, at most as many band values and SCL bytes gathered, the labels in and out
        work = float(n) * S * S * (4 * TC + (T if scl is not None else 0) + 1 + (2 * es if labels is not None else 0))
        _call("ig_s2_chip_warp", work, _p(bands), _p(sd), _p(scl), _p(ssd), _p(pcd), _p(cgd), _p(csd), G, _p(scd), _p(dcd), _p(dgd), n, T, TC // T, S,
              int(class_bits), R.STRATEGIES[strategy], int(no_data_value), int(boa_offset), *_opt_pair(valid_range, int),
              *_label_tail(labels, es, valid_bit, K, outs))
    return outs


def s1_chip_cut(planes, starts, scene_crs, scene_grid, scene_size, date_scenes, dst_crs, dst_grid, origins, S: int, no_data_value: float = -1.0,
                src_nodata=None, clip=None, out=None):
    """``ig_s1_chip_cut`` (include/instageo_hip.h): ``planes`` the packed float32 planes as a 1-D tensor on the device; ``date_scenes`` the
    number of scenes of every date, ``starts`` (N * C,), ``scene_crs`` (N systems), ``scene_grid`` (N, 4) = (X0, Y0, sx, sy), ``scene_size``
    (N, 2) = (H, W), ``dst_crs``, ``dst_grid`` (4,) and ``origins`` (n, 2) as host values: they are checked here (every plane inside the
    buffer) and uploaded.  -> (chips (n, T * C, S, S) float32, valid_values (n,) int32, validity (n, S, S) uint8).  ``out``: a dict with
    any of ``chips``, ``validity``: contiguous tensors to write into instead of new ones (every element is written)."""
    from . import s1_chips as V

    assert planes.dtype == torch.float32 and planes.dim() == 1, "the planes are one packed 1-D float32 buffer"
    st, sc, sg, ss, first_bits, T, C, dc, dg, o, nd, snd, clip = V.check_cut(int(planes.shape[0]), starts, scene_crs, scene_grid, scene_size,
                                                                            date_scenes, dst_crs, dst_grid, origins, S, no_data_value,
                                                                            src_nodata, clip)
    n, N, S = o.shape[0], sg.shape[0], int(S)
    dev = planes.device
    chips, valid, plane = _chip_outputs(out, dev, (n, T * C, S, S), torch.float32)[:3]
    if n:
        dcd, dgd, scd, sgd = _upload(dev, dc, dg, sc.reshape(-1), sg.reshape(-1))
        ssd, od = _upload(dev, ss.reshape(-1), o.reshape(-1))
        (sd,) = _upload(dev, st)
        # HBM bytes: the chips and the validity plane written, at least as many values gathered
        work = float(n) * S * S * (8 * T * C + 1)
        _call("ig_s1_chip_cut", work, _p(planes), _p(sd), _p(scd), _p(sgd), _p(ssd), N, int(first_bits), _p(dcd), _p(dgd), _p(od), n, T, C, S,
              float(nd), *_opt_value(snd), *_opt_pair(clip, float), _p(chips), _p(valid), _p(plane), _stream())
    return chips, valid, plane


def s1_chip_warp(planes, starts, scene_crs, scene_grid, scene_size, date_scenes, dst_crs, dst_grids, S: int, no_data_value: float = -1.0,
                 src_nodata=None, clip=None, labels=None, valid_bit: int = 0, K: int = 0, out=None):
    """``ig_s1_chip_warp`` (include/instageo_hip.h): ``planes`` the packed float32 planes as a 1-D tensor on the device; ``date_scenes``,
    ``starts``, ``scene_crs``, ``scene_grid`` and ``scene_size`` as :func:`s1_chip_cut` takes them, ``dst_crs`` and ``dst_grids`` (n, 4) as
    :func:`chip_warp` does, all as host values: they are checked here (every plane inside the buffer) and uploaded.  ``labels``: None, or
    (n, S, S) int8 | float32 as a device tensor or a host array.  -> (chips (n, T * C, S, S) float32, valid_values (n,) int32, validity
    (n, S, S) uint8, maps, valid_labels, hist): the last three None without labels, hist None with K = 0.  ``out``: a dict with any of
    ``chips``, ``validity``, ``maps``: contiguous tensors to write into instead of new ones (every element is written)."""
    from . import s1_raster_chips as R

    assert planes.dtype == torch.float32 and planes.dim() == 1, "the planes are one packed 1-D float32 buffer"
    lab_dtype = None if labels is None else str(labels.dtype).replace("torch.", "")
    st, sc, sg, ss, first_bits, T, C, dc, dg, nd, snd, clip = R.check_warp(int(planes.shape[0]), starts, scene_crs, scene_grid, scene_size,
                                                                          date_scenes, dst_crs, dst_grids, S, no_data_value, src_nodata, clip,
                                                                          None if labels is None else tuple(labels.shape), lab_dtype,
                                                                          valid_bit, K)
    n, N, S = dg.shape[0], sg.shape[0], int(S)
    dev = planes.device
    labels, es = _labels_on(labels, dev)
    outs = _chip_outputs(out, dev, (n, T * C, S, S), torch.float32, labels, K)
    if n:
        dcd, scd, sgd, dgd = _upload(dev, dc, sc.reshape(-1), sg.reshape(-1), dg.reshape(-1))
        (ssd,), (sd,) = _upload(dev, ss.reshape(-1)), _upload(dev, st)
        # HBM bytes: the chips and the validity plane written, at least as many values gathered, the labels in and out
        work = float(n) * S * S * (8 * T * C + 1 + (2 * es if labels is not None else 0))
        _call("ig_s1_chip_warp", work, _p(planes), _p(sd), _p(scd), _p(sgd), _p(ssd), N, int(first_bits), _p(dcd), _p(dgd), n, T, C, S, float(nd),
              *_opt_value(snd), *_opt_pair(clip, float), *_label_tail(labels, es, valid_bit, K, outs))
    return outs


def composite(bands, starts, fmasks, fmask_starts, step_ptr, C: int, shape: Tuple[int, int], mask_bits: int = 0, no_data_value: int = -9999,
              min_clear: int = 1, method: str = "medoid"):
    """``ig_composite`` (include/instageo_hip.h): ``bands`` the packed int16 planes and ``fmasks`` the packed uint8 Fmask planes (or None)
    as 1-D tensors on the device; ``starts`` (N * C,), ``fmask_starts`` (N,) and ``step_ptr`` (T + 1,) as host arrays: they are checked
    here (every plane of ``shape`` = (H, W) inside its buffer, step_ptr ascending from 0, at most 16 candidates per step) and uploaded.
    -> (composite (T, C, H, W) int16, count (T, H, W) uint8, source (T, H, W) uint8, hist (T, 17) int32)."""
    from . import composite as K

    assert bands.dtype == torch.int16 and bands.dim() == 1, "the band planes are one packed 1-D int16 buffer"
    assert fmasks is None or (fmasks.dtype == torch.uint8 and fmasks.dim() == 1), "the Fmask planes are one packed 1-D uint8 buffer"
    st, fst, ptr, T, N, max_m, H, W = K.check_composite(int(bands.shape[0]), starts, None if fmasks is None else int(fmasks.shape[0]), fmask_starts,
                                                        step_ptr, C, shape, mask_bits, no_data_value, min_clear, method)
    C, dev = int(C), bands.device
    comp = torch.empty((T, C, H, W), dtype=torch.int16, device=dev)
    count = torch.empty((T, H, W), dtype=torch.uint8, device=dev)
    source = torch.empty((T, H, W), dtype=torch.uint8, device=dev)
    hist = torch.zeros((T, K.CELLS), dtype=torch.int32, device=dev)
    if T and H * W:
        sd, fd = _upload(dev, st, fst) if fst is not None else (*_upload(dev, st), None)
        (pd,) = _upload(dev, ptr)
        # HBM bytes: every value and Fmask byte of every candidate read once, the composites, counts and sources written
        work = float(H * W) * (N * (2 * C + 1 if fst is not None else 2 * C) + T * (2 * C + 2))
        # without scenes the kernel takes null for them and their offsets
        _call("ig_composite", work, _p(bands) if N else None, _p(sd) if N else None, _p(fmasks) if fst is not None and N else None,
              _p(fd) if N else None, _p(pd), T, N, max_m, C, H, W, int(mask_bits), int(no_data_value), int(min_clear), K.METHODS[method], _p(comp),
              _p(count), _p(source), _p(hist), _stream())
    return comp, count, source, hist


def _s1_filter(entry: str, planes, starts, sizes, window, method, looks, src_nodata, scale, out):
    """``s1_speckle`` and ``s1_refined_lee``: the same checks, tables and outputs; ``ig_s1_speckle`` also takes the half window and the
    method's code."""
    from . import s1_filter as F

    assert planes.dtype == torch.float32 and planes.dim() == 1, "the planes are one packed 1-D float32 buffer"
    assert (method == "refined_lee") == (entry == "ig_s1_refined_lee"), "refined_lee has an entry point of its own: ops.s1_refined_lee"
    st, ss, h, code, lk, snd, to_db = F.check_speckle(int(planes.shape[0]), starts, sizes, window, method, looks, src_nodata, scale)
    N, total = st.shape[0], int(planes.shape[0])
    out, counts, pixels = _plane_outputs(planes, ss, out, 2)
    if N:
        tp = F.tile_table(ss)
        (sd, td), (zd,) = _upload(planes.device, st, tp), _upload(planes.device, ss.reshape(-1))
        # HBM bytes: every value read once (the halo comes from the caches) and written once
        _call(entry, 8.0 * pixels, _p(planes), _p(sd), _p(zd), _p(td), N, total, int(tp[-1]), *((h, code) if entry == "ig_s1_speckle" else ()),
              float(lk), *_opt_value(snd), to_db, _p(out), _p(counts), _stream())
    return out, counts


def s1_speckle(planes, starts, sizes, window: int = 7, method: str = "lee", looks: float = 4.4, src_nodata=None, scale: str = "linear",
               out=None):
    """``ig_s1_speckle`` (include/instageo_hip.h): ``planes`` the packed float32 planes as a 1-D tensor on the device; ``starts`` (N,) and
    ``sizes`` (N, 2) = (H, W) as host arrays: they are checked here (every plane inside the buffer, no two overlapping) and uploaded with
    the prefix table of tiles.  -> (out: float32 with the layout of ``planes``, elements outside every plane 0; counts (N, 2) int32: the
    present outputs and the pixels the dB step dropped).  ``out``: a contiguous float32 tensor of the size of ``planes`` to write into
    instead of a new one (only the elements of the planes are written)."""
    return _s1_filter("ig_s1_speckle", planes, starts, sizes, window, method, looks, src_nodata, scale, out)


def s1_refined_lee(planes, starts, sizes, looks: float = 4.4, src_nodata=None, scale: str = "linear", out=None):
    """``ig_s1_refined_lee`` (include/instageo_hip.h): the refined Lee filter on the packed planes of :func:`s1_speckle`, with the same
    host-side checks of ``starts`` and ``sizes``, the same tile table and the same outputs.  The window is 7 x 7."""
    from .s1_filter import REFINED_WINDOW

    return _s1_filter("ig_s1_refined_lee", planes, starts, sizes, REFINED_WINDOW, "refined_lee", looks, src_nodata, scale, out)


def s1_temporal(planes, starts, sizes, group, date, offsets, window: int = 7, src_nodata=None, scale: str = "linear", out=None):
    """``ig_s1_temporal`` (include/instageo_hip.h): ``planes`` the packed float32 planes as a 1-D tensor on the device; ``starts`` (N,),
    ``sizes`` (N, 2) = (H, W), ``group`` (N,), ``date`` (N,) and ``offsets`` (N, 2) = (row0, col0) as host arrays: they are checked here
    (every plane inside the buffer, no two overlapping, the lattices and member lists built from them, at most 64 planes and 32 dates per
    group) and uploaded with the prefix table of tiles.  -> (out: float32 with the layout of ``planes``, elements outside every plane 0;
    counts (N, 4) int32: the present outputs, the pixels the dB step dropped, the pixels passed through and the present outputs where one
    date contributed).  ``out``: a contiguous float32 tensor of the size of ``planes`` to write into instead of a new one (only the
    elements of the planes are written)."""
    from . import s1_temporal as Q

    assert planes.dtype == torch.float32 and planes.dim() == 1, "the planes are one packed 1-D float32 buffer"
    st, ss, h, snd, to_db, T = Q.check_temporal(int(planes.shape[0]), starts, sizes, group, date, offsets, window, src_nodata, scale)
    N, dev, total = st.shape[0], planes.device, int(planes.shape[0])
    out, counts, pixels = _plane_outputs(planes, ss, out, 4)
    if N:
        G = T.lattice.shape[0]
        sd, td = _upload(dev, st, T.tile_ptr)
        zd, pl, la, mp, mm = _upload(dev, ss.reshape(-1), T.place.reshape(-1), T.lattice.reshape(-1), T.member_ptr, T.members)
        # HBM bytes: every value read once (the second sweep and the halo come from the caches) and written once
        _call("ig_s1_temporal", 8.0 * pixels, _p(planes), _p(sd), _p(zd), _p(pl), _p(la), _p(mp), _p(mm), _p(td), N, G, N, total,
              int(T.tile_ptr[-1]), h, *_opt_value(snd), to_db, _p(out), _p(counts), _stream())
    return out, counts


TILE_STYLES = {"palette": 0, "ramp": 1, "rgb": 2}  # include/instageo_hip.h
TILE_MAX_LEVELS = 13


def tile_render(levels, src_crs, src_grid, tile_grids, tile_level, tile: int, style: str, lut=None, ncolors: int = 0, fill: int = -1,
                rescale=(0.0, 1.0), order=(0, 1, 2), out=None):
    """``ig_tile_render`` (include/instageo_hip.h): ``levels`` the pyramid, a list of device tensors (level 0 first; (H_k, W_k) or
    (bands, H_k, W_k), int8 for ``palette``, float32 for ``ramp`` (1 band) and ``rgb`` (3 bands)) that stay where they are: only a table
    of their addresses is uploaded.  ``src_crs`` five doubles, ``src_grid`` (X0, Y0, sx, sy), ``tile_grids`` (n, 4) float64 (EPSG:3857)
    and ``tile_level`` (n,) int32 as host values; ``lut`` (256, 4) uint8 (host array or device tensor); ``rescale`` = (lo, hi).  The level
    shapes are checked here, so that no read can leave a level.  -> (rgba (n, tile, tile, 4) uint8, opaque (n,) int32).  ``out``: a
    contiguous (n, tile, tile, 4) uint8 tensor to write into instead of a new one (every pixel is written)."""
    code = TILE_STYLES.get(style)
    if code is None:
        raise ValueError(f"style must be one of {tuple(TILE_STYLES)} (got {style!r})")
    levels = list(levels)
    if not 1 <= len(levels) <= TILE_MAX_LEVELS:
        raise ValueError(f"a pyramid has 1..{TILE_MAX_LEVELS} levels (got {len(levels)})")
    want, bands = (torch.int8, 1) if code == 0 else (torch.float32, 3 if code == 2 else 1)
    first = levels[0]
    H, W = int(first.shape[-2]), int(first.shape[-1])
    if H < 1 or W < 1 or H * W > 2**31 - 1:
        raise ValueError(f"a source of {H} x {W} pixels is beyond the kernel's limits (1 <= H * W <= 2^31 - 1)")
    h, w = H, W
    for k, lv in enumerate(levels):
        shape = tuple(lv.shape)
        if lv.dtype != want or shape not in (((h, w), (1, h, w)) if bands == 1 else ((3, h, w),)) or lv.device != first.device:
            raise ValueError(f"level {k} must be {want} of {'(3, ' if bands == 3 else '('}{h}, {w}) on {first.device} for style {style!r} "
                             f"(got {lv.dtype} {shape} on {lv.device})")
        h, w = (h + 1) // 2, (w + 1) // 2
    tile = int(tile)
    if tile < 64 or tile > 1024 or tile % 64:
        raise ValueError(f"tile must be a multiple of 64 in 64..1024 (got {tile})")
    grids = np.ascontiguousarray(tile_grids, dtype=np.float64).reshape(-1, 4)
    lvl = np.ascontiguousarray(tile_level, dtype=np.int32).reshape(-1)
    n = grids.shape[0]
    if lvl.shape[0] != n:
        raise ValueError(f"{n} tile grids but {lvl.shape[0]} tile levels")
    if n * tile * tile >= 2**31:
        raise ValueError(f"{n} tiles of {tile} x {tile} reach 2^31 pixels: render in batches")
    lo, hi = float(rescale[0]), float(rescale[1])
    if code != 0 and not (np.isfinite(lo) and np.isfinite(hi) and hi - lo > 0 and np.isfinite(hi - lo)):
        raise ValueError(f"rescale = (lo, hi) needs finite values with lo < hi (got {rescale!r})")
    order = tuple(int(o) for o in order)
    if code == 2 and (len(order) != 3 or any(not 0 <= o < 3 for o in order)):
        raise ValueError(f"order names three planes in 0..2 (got {order!r})")
    if isinstance(fill, bool) or not -128 <= int(fill) <= 127:
        raise ValueError(f"fill must be an int that fits int8 (got {fill!r})")
    if not 0 <= int(ncolors) <= 256:
        raise ValueError(f"ncolors must lie in 0..256 (got {ncolors!r})")
    dev = first.device
    if code != 2:
        if lut is None:
            raise ValueError(f"style {style!r} needs a lut")
        if not torch.is_tensor(lut):
            lut = torch.from_numpy(np.ascontiguousarray(lut, dtype=np.uint8))
        lut = lut.to(dev)
        assert lut.dtype == torch.uint8 and tuple(lut.shape) == (256, 4), "lut is (256, 4) uint8"
    else:
        lut = None
    rgba = out if out is not None else torch.empty((n, tile, tile, 4), dtype=torch.uint8, device=dev)
    assert rgba.dtype == torch.uint8 and tuple(rgba.shape) == (n, tile, tile, 4)
    opaque = torch.zeros((n,), dtype=torch.int32, device=dev)
    if n:
        sc, sg = _warp_doubles(src_crs, 5, "src_crs"), _warp_doubles(src_grid, 4, "src_grid")
        (scd, sgd, gd), (lv_d,) = _upload(dev, sc, sg, grids.reshape(-1)), _upload(dev, lvl)
        table = torch.tensor([_p(lv) for lv in levels], dtype=torch.int64).to(dev)  # alive until the launch is queued, as the uploads are
        # HBM bytes: the tiles written and as many source values gathered
        _call("ig_tile_render", float(n) * tile * tile * (4 + first.element_size() * bands), _p(table), len(levels), first.element_size(), bands, H, W,
              _p(scd), _p(sgd), _p(gd), _p(lv_d), n, tile, code, _p(lut), int(ncolors), int(fill), lo, hi - lo, order[0], order[1], order[2],
              _p(rgba), _p(opaque), _stream())
    return rgba, opaque


def chip_nodata(chips, no_data_value: int):
    """``ig_chip_nodata`` (include/instageo_hip.h): ``chips`` (n, B, H, W) int16 | uint16 on the device -> (plane (n, H, W) uint8: bit 0
    any, bit 1 all; counts (n, 2) int32).  A ``no_data_value`` the chips' dtype cannot hold matches nothing: zeros without a launch."""
    from . import clean as C

    assert chips.dim() == 4 and chips.dtype in (torch.int16, torch.uint16), "chips is (n, B, H, W) int16 or uint16"
    n, B, H, W = chips.shape
    pattern = C.check_nodata((n, B, H, W), "int16" if chips.dtype == torch.int16 else "uint16", no_data_value)
    plane = torch.zeros((n, H, W), dtype=torch.uint8, device=chips.device)
    counts = torch.zeros((n, 2), dtype=torch.int32, device=chips.device)
    if n and pattern is not None:
        # HBM bytes: the chips read once, the plane written
        _call("ig_chip_nodata", float(n) * H * W * (2 * B + 1), _p(chips), n, B, H, W, pattern, _p(plane), _p(counts), _stream())
    return plane, counts


def _label_outputs(labels, K: int):
    assert labels.dim() == 3 and labels.dtype in (torch.int16, torch.float32), "labels is (n, H, W) int16 or float32"
    n = labels.shape[0]
    out = torch.empty_like(labels)
    valid = torch.zeros((n,), dtype=torch.int32, device=labels.device)
    hist = torch.zeros((n, K), dtype=torch.int32, device=labels.device) if K else None
    return out, valid, hist


def label_buffer(labels, w: int, ignore_index: int, plane=None, K: int = 0):
    """``ig_label_buffer`` (include/instageo_hip.h): ``labels`` (n, H, W) int16 | float32 and ``plane`` (n, H, W) uint8 of
    :func:`chip_nodata` (or None: no masking) on the device -> (out like labels, valid_labels (n,) int32, hist (n, K) int32 or None)."""
    from . import clean as C

    out, valid, hist = _label_outputs(labels, K)
    n, H, W = labels.shape
    C.check_label_args((n, H, W), "int16" if labels.dtype == torch.int16 else "float32", ignore_index, K, w)
    assert plane is None or (plane.dtype == torch.uint8 and plane.shape == labels.shape and plane.device == labels.device)
    if n and H and W:
        es = labels.element_size()
        _call("ig_label_buffer", float(n) * H * W * (2 * es + (plane is not None)), _p(labels), n, H, W, es, int(w), int(ignore_index), _p(plane),
              int(K), _p(out), _p(valid), _p(hist), _stream())
    return out, valid, hist


def label_limit(labels, ptr, pts, ignore_index: int, K: int = 0):
    """``ig_label_limit`` (include/instageo_hip.h): ``labels`` (n, H, W) int16 | float32 on the device, ``ptr`` (n + 1,) and ``pts``
    (P, 2) = (row, col) as host arrays: ptr is checked here and the points outside their map are dropped, then both are uploaded.
    -> (out like labels, valid_labels (n,) int32, hist (n, K) int32 or None)."""
    from . import clean as C

    out, valid, hist = _label_outputs(labels, K)
    n, H, W = labels.shape
    C.check_label_args((n, H, W), "int16" if labels.dtype == torch.int16 else "float32", ignore_index, K)
    p, q = C.check_points(n, H, W, ptr, pts)
    if n and H and W:
        pd, qd = _upload(labels.device, p, q.reshape(-1))
        es = labels.element_size()
        _call("ig_label_limit", float(n) * H * W * 2 * es, _p(labels), n, H, W, es, _p(pd), _p(qd), q.shape[0], int(ignore_index), int(K), _p(out),
              _p(valid), _p(hist), _stream())
    return out, valid, hist


def _split_dtype(t) -> str:
    return str(t.dtype).replace("torch.", "")


def split_assign(pts, centres, assign, check_range: bool = True):
    """``ig_split_assign`` (include/instageo_hip.h): one Lloyd round.  ``pts`` (N, 3) int32 and ``assign`` (N,) int32 on the device
    (``assign`` is read and overwritten), ``centres`` (K, 3) int32 as a host array or a tensor -> (sums (K, 4) int64: sum x, sum y, sum z,
    count per centre; changed (1,) int32), both on the device.  ``check_range=False`` skips the device reduction that checks
    |coordinate| <= 2^29 of ``pts`` (a caller that quantised them itself)."""
    from . import split as S

    cen = np.ascontiguousarray(centres.cpu().numpy() if torch.is_tensor(centres) else centres)
    N, K = S.check_assign(tuple(pts.shape), _split_dtype(pts), cen, tuple(assign.shape), _split_dtype(assign))
    assert assign.device == pts.device, "assign must live on the device of pts"
    if check_range and N and int(pts.abs().max()) > S.SCALE:
        raise ValueError(f"pts must be quantised unit vectors: |coordinate| <= 2^29 (got {int(pts.abs().max())})")
    sums = torch.zeros((K, 4), dtype=torch.int64, device=pts.device)
    changed = torch.zeros((1,), dtype=torch.int32, device=pts.device)
    if N:
        cen_d = torch.from_numpy(cen).to(pts.device)  # alive until the launch is queued; the copy is stream-ordered
        # integer work: three multiply-adds per (point, centre)
        _call("ig_split_assign", 3.0 * N * K, _p(pts), N, _p(cen_d), K, _p(assign), _p(sums), _p(changed), _stream())
    return sums, changed


def split_nearest(a, b, check_range: bool = True):
    """``ig_split_nearest`` (include/instageo_hip.h): ``a`` (Na, 3) and ``b`` (Nb, 3) int32 on the device, Nb >= 1 -> (d2 (Na,) int64: the
    smallest squared distance of every row of ``a`` to a row of ``b`` (the library's uint64, at most 3 * 2^60, so the int64 holds it
    exactly); idx (Na,) int32: the smallest index of ``b`` that attains it)."""
    from . import split as S

    Na, Nb = S.check_nearest(tuple(a.shape), _split_dtype(a), tuple(b.shape), _split_dtype(b))
    assert a.device == b.device, "a and b must live on one device"
    if check_range and max(int(a.abs().max()) if Na else 0, int(b.abs().max())) > S.SCALE:
        raise ValueError("a and b must be quantised unit vectors: |coordinate| <= 2^29")
    d2 = torch.empty((Na,), dtype=torch.int64, device=a.device)
    idx = torch.empty((Na,), dtype=torch.int32, device=a.device)
    if Na:
        _call("ig_split_nearest", 3.0 * Na * Nb, _p(a), Na, _p(b), Nb, _p(d2), _p(idx), _stream())
    return d2, idx


def confusion_update(y_true, y_pred, confusion, k: int, ignore_index: Optional[int]) -> None:
    assert y_true.dtype == torch.int64 and y_pred.dtype == torch.int64 and confusion.dtype == torch.int64
    _lib.call("ig_confusion_update", _p(y_true), _p(y_pred), _p(confusion), y_true.numel(), k,
              0 if ignore_index is None else int(ignore_index), int(ignore_index is not None), _stream())


def adamw_advance(hyper) -> None:
    _lib.call("ig_adamw_advance", _p(hyper), _stream())


def adamw_step(p, g, m, v, shadow: Optional[BT], hyper, n: int) -> None:
    # 28 B/param fp32 state (read p, g, m, v; write p, m, v) + the refreshed bf16 shadow
    work = float(n) * (28 + (0 if not shadow else 2 if shadow.lo is None else 4))
    _call("ig_adamw_step", work, _p(p), _p(g), _p(m), _p(v), _p(shadow.hi) if shadow else None,
          _p(shadow.lo) if shadow and shadow.lo is not None else None, _p(hyper), n, _stream())
