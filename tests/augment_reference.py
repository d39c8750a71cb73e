"""Float64 restatements of the four augmentation operations (``ig_aug_rotate``, ``ig_aug_brightness_contrast``, ``ig_aug_blur``,
``ig_aug_noise``; instageo/model/dataloader.py:144-386) with the acceptance rules of tests/test_gpu_augment.py, and the inputs of every
blur / noise case that file runs (tests/test_cpu_augment.py checks the rules' preconditions on them without a GPU).

Rotation is integer arithmetic: :func:`rotate` IS ``oracle.augment_oracle.rotate_nearest`` (pinned against Pillow, int64 walk); the
comparison is bit for bit.  The other three are fp32 arithmetic on the device and are compared with float64 evaluations of the same
formula on the SAME fp32 inputs (pixels, kernel weights, factors, noise field, noise_std and max_pixel as the fp32 values handed over).

Blur and noise end in a uint16 truncation, so an fp32 last-bit difference next to an integer moves the result by one count.  The rule
(:func:`accept_range`, :func:`compare_truncated`): with ``pre`` the float64 value before the clamp and the truncation,

* a pixel is DECIDED when clamp(pre) is farther than delta from every integer, or lies on a clamp plateau; it must match exactly;
* it is AMBIGUOUS otherwise and may be either neighbouring integer (the one below when clamp(pre) is within delta above an integer, the
  one above when it is within delta below one).

Two refinements, both on the strict side of "what can fp32 arithmetic that is off by at most delta produce": (a) the upper plateau
counts only from ``pre >= max_pixel + delta`` on -- a value a hair above max_pixel in float64 may be a hair below it in fp32 and truncate
to ``max_pixel - 1``; (b) within delta ABOVE 0 the only possible result is 0 (there is no integer below), so 0 alone is accepted; such
pixels still COUNT as ambiguous in the caps.  A case may leave at most :data:`AMBIGUOUS_CAP` of its pixels ambiguous and none in its
border set (:func:`border_mask`); the case builders below nudge their seeded inputs until that holds.
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np

from oracle import augment_oracle as AO

U = 2.0 ** -24  # fp32 unit roundoff: |fl(v) - v| <= U * |v| for every fp32 operation that is correctly rounded (+, -, *, /, fma)
AMBIGUOUS_CAP = 0.10
MAX_PIXEL = 10000.0
ATPB, GRID_CAP = 256, 16384
ONE_PASS = ATPB * GRID_CAP  # elements one pass of the augmentation kernels' grid-stride loops covers (csrc/augment.hip: aug_grid)

rotate = AO.rotate_nearest  # bit-exact already: reused, not restated
ROT_SIZES = (1, 2, 3, 17, 33, 64, 225)
ROT_ANGLES = (0.0, 1e-3, 7.3, -14.9, 45.0, 90.0, -90.0, 180.0, -180.0, 270.0, 359.9, 725.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# brightness / contrast
def brightness_contrast(arr: np.ndarray, bright: float, contrast: float, max_pixel: float = MAX_PIXEL) -> Tuple[np.ndarray, np.ndarray]:
    """One band of ``random_brightness_contrast`` (dataloader.py:230-238) in float64 -> (result, per-pixel tolerance).

    Exact: p = x * b, m = mean(p), d = p - m, r = d * c + m, result = clamp(r, 0, max).  The kernel (csrc/augment.hip) rounds to fp32 at
    p^ = fl(x * b); m^ = fl32(fp64 mean of the p^); d^ = fl(p^ - m^); then fl(fl(d^ * c) + m^), or one fma; the clamp is exact and
    1-Lipschitz.  With |fl(v) - v| <= U |v|, first order in U, A = mean|p|:
        |p^ - p| <= U |p|
        |m^ - m| <= U A (the p^ under the exact fp64 mean) + U |m| (its fp32 rounding: where the kernel differs from torch's fp32
                    mean) <= 2 U A
        |d^ - d| <= U |p| + 2 U A + U |d|
        |fl(d^ c) - d c| <= |c| (U |p| + 2 U A + U |d|) + U |d c|
        |r^ - r| <= U * ( |c| (|p| + 2 A + 2 |d|) + 2 A + |r| )
    The fp64 accumulation (<= 2^16 terms, 2^-53 each) and the second-order terms are below 2^-20 of this bound; the factor (1 + 2^-20)
    covers them.  The tolerance scales with the magnitudes: 0 on a band of zeros, ~3.5e-3 at 9000 +- 2, and it replaces a fixed 4e-3."""
    x = np.asarray(arr, dtype=np.float32).astype(np.float64)
    b, c = float(np.float32(bright)), float(np.float32(contrast))
    p = x * b
    m = p.mean()
    a = np.abs(p).mean()
    d = p - m
    r = d * c + m
    tol = U * (abs(c) * (np.abs(p) + 2.0 * a + 2.0 * np.abs(d)) + 2.0 * a + np.abs(r)) * (1.0 + 2.0 ** -20)
    return np.clip(r, 0.0, float(max_pixel)), tol


# ---------------------------------------------------------------------------------------------------------------------------------
# blur / noise: value before the truncation, and the rule
def blur_delta(ksize: int, max_pixel: float = MAX_PIXEL) -> float:
    """delta of ``aug_blur_kernel``: acc = sum_j k2_j * (clip(x_j) / max), result = clamp(acc, 0, 1) * max.  fp32 roundings on the path,
    each bounded by U times the magnitude of the value rounded, in units of [0, 1] (weights positive with sum 1, taps and partial sums
    <= 1):
      * k^2 additions into acc (the multiply-add's rounding when it is fused): <= U each                      -> k^2 U
      * the clips are exact; the k^2 products k2_j * a_j when NOT fused: <= U k2_j a_j each, sum <= U          -> U
      * the k^2 divides a_j = x_j / max: <= U a_j each, weighted by k2_j in acc, sum <= U                      -> U
      * the scale by max: <= U acc max                                                                         -> U
    so |kernel - exact| <= (k^2 + 3) * 2^-24 * max_pixel before the truncation, fused or not."""
    return (ksize * ksize + 3) * U * float(max_pixel)


def noise_delta(max_pixel: float = MAX_PIXEL) -> float:
    """delta of ``aug_noise_kernel``: a = clip(x) / max (1 rounding, a <= 1); t = a + z * std (2 roundings, or 1 fused); clamp; * max (1).
    For a pixel that is not on a clamp plateau t lies in [0, 1], so |z * std| <= 1 and each rounding is <= U in units of [0, 1]:
    |kernel - exact| <= 4 * 2^-24 * max_pixel before the truncation."""
    return 4 * U * float(max_pixel)


def blur_pre(arr: np.ndarray, k2: np.ndarray, max_pixel: float = MAX_PIXEL) -> np.ndarray:
    """``add_gaussian_blur`` (dataloader.py:296-314) of (..., S, S) bands with the (k, k) fp32 kernel ``k2`` (correlation with reflect
    padding, torchvision's gaussian_blur) in float64, times max_pixel: the value BEFORE the clamp and the uint16 truncation."""
    a = np.clip(np.asarray(arr).astype(np.float64), 0.0, max_pixel) / max_pixel
    k2 = np.asarray(k2, dtype=np.float32).astype(np.float64)
    k = k2.shape[0]
    h = k // 2
    S = a.shape[-1]
    assert k2.shape == (k, k) and k % 2 == 1 and h < S and a.shape[-2] == S
    pad = np.pad(a, [(0, 0)] * (a.ndim - 2) + [(h, h), (h, h)], mode="reflect") if h else a
    acc = np.zeros_like(a)
    for dy in range(k):
        for dx in range(k):
            acc += k2[dy, dx] * pad[..., dy : dy + S, dx : dx + S]
    return acc * max_pixel


def noise_pre(arr: np.ndarray, z: np.ndarray, noise_std: float, max_pixel: float = MAX_PIXEL) -> np.ndarray:
    """``add_gaussian_noise`` (dataloader.py:356-368) with the standard-normal field given, in float64, times max_pixel: the value
    BEFORE the clamp and the uint16 truncation."""
    a = np.clip(np.asarray(arr).astype(np.float64), 0.0, max_pixel) / max_pixel
    return (a + np.asarray(z, dtype=np.float32).astype(np.float64) * float(np.float32(noise_std))) * max_pixel


def truncate(pre: np.ndarray, max_pixel: float = MAX_PIXEL) -> np.ndarray:
    """clamp + uint16 truncation of a pre-truncation value: the reference's result where the pixel is decided."""
    return np.floor(np.clip(pre, 0.0, max_pixel))


def accept_range(pre: np.ndarray, delta: float, max_pixel: float = MAX_PIXEL) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(lo, hi, ambiguous) per pixel: the kernel's result must lie in [lo, hi] (module docstring); lo == hi on decided pixels.
    ``ambiguous`` is the wider notion the caps count: within delta of an integer and not on a plateau."""
    c = np.clip(pre, 0.0, max_pixel)
    f = np.floor(c)
    frac = c - f
    plateau = (pre <= 0.0) | (pre >= max_pixel + delta)
    below, above = (frac <= delta) & ~plateau, ((1.0 - frac) <= delta) & ~plateau
    lo = np.where(below & (f >= 1.0), f - 1.0, f)
    hi = np.where(above, f + 1.0, f)
    return lo, hi, below | above


def border_mask(S: int, ksize: int = 1) -> np.ndarray:
    """The border set of an S x S band: the four corners and the outermost ``ksize / 2`` rows and columns."""
    m = np.zeros((S, S), dtype=bool)
    h = ksize // 2
    if h:
        m[:h], m[-h:], m[:, :h], m[:, -h:] = True, True, True, True
    m[0, 0] = m[0, -1] = m[-1, 0] = m[-1, -1] = True
    return m


def case_conditions(pre: np.ndarray, delta: float, ksize: int = 1, max_pixel: float = MAX_PIXEL) -> Tuple[float, int]:
    """(ambiguous share, ambiguous pixels in the border set) of a case's applied bands (..., S, S): the test conditions are
    share <= AMBIGUOUS_CAP and 0."""
    amb = accept_range(pre, delta, max_pixel)[2]
    return float(amb.mean()), int((amb & border_mask(pre.shape[-1], ksize)).sum())


def compare_truncated(got: np.ndarray, pre: np.ndarray, delta: float, ksize: int = 1, max_pixel: float = MAX_PIXEL) -> Dict[str, float]:
    """The comparison of a device result with the rule.  Returns the figures a test prints and asserts on:
    ``bad`` pixels outside [lo, hi] (decided pixels that differ, or ambiguous ones off by more than their neighbour), the ambiguous
    ``share``, ambiguous pixels in the ``border`` set, the pixels that ``flipped`` (differ from the float64 truncation) and
    ``margin``: the largest distance between a flipped pixel's float64 value and the integer it crossed -- a measured lower bound of
    the kernel's error, to be read beside delta."""
    got = np.asarray(got, dtype=np.float64)
    lo, hi, amb = accept_range(pre, delta, max_pixel)
    ref = truncate(pre, max_pixel)
    c = np.clip(pre, 0.0, max_pixel)
    flipped = got != ref
    cross = np.where(got < ref, c - ref, ref + 1.0 - c)  # distance to the integer between the two results
    return {"bad": int(((got < lo) | (got > hi)).sum()), "share": float(amb.mean()),
            "border": int((amb & border_mask(pre.shape[-1], ksize)).sum()), "flipped": int(flipped.sum()),
            "margin": float(cross[flipped].max()) if flipped.any() else 0.0, "delta": float(delta)}


# ---------------------------------------------------------------------------------------------------------------------------------
# seeded inputs of the blur / noise cases (shared by the CPU checks of the caps and by the GPU comparisons)
def gaussian_kernel2d(ksize: int, sigma: Sequence[float]) -> np.ndarray:
    """torchvision's ``gaussian_blur`` kernel as fp32 (what ``dataloader.gaussian_kernel2d`` builds; checked equal on the CPU)."""
    import torch

    kx, ky = AO.gaussian_kernel1d(ksize, float(sigma[0])), AO.gaussian_kernel1d(ksize, float(sigma[1]))
    return torch.mm(ky[:, None], kx[None, :]).numpy()


def asymmetric_kernel2d(ksize: int, seed: int = 3) -> np.ndarray:
    """A positive (k, k) fp32 kernel of sum ~1 with no symmetry: a flipped, transposed or shifted tap shows in an impulse response."""
    w = np.random.default_rng(seed).uniform(0.2, 1.0, (ksize, ksize))
    return (w / w.sum()).astype(np.float32)


def _raster(rng, shape, floats: bool) -> np.ndarray:
    """Reflectance-like values in [0, max) with a band of rows below 0 at the top, scattered single pixels below 0 and above max
    (blur and noise clip first).  ``floats``: generic fractional parts (a blur of ksize 1 keeps the input's)."""
    x = rng.uniform(0.0, MAX_PIXEL, shape) if floats else rng.integers(0, 10000, shape).astype(np.float64)
    S = shape[-1]
    hot = rng.random(shape)
    x[hot < 0.01] = 12000.0
    x[hot > 0.99] = -300.0
    x[..., : S // 8, :] = -50.0  # a whole band of zeros after the clip: its blur is the plateau 0 exactly (no stray pixel inside it)
    return x.astype(np.float32)


def _settle(x: np.ndarray, pre_of, delta: float, ksize: int, step: float) -> np.ndarray:
    """Nudge the pixels of ``x`` (..., S, S) whose result is ambiguous inside the border set by ``step`` until none is left
    (deterministic; the conditions are asserted afterwards by tests/test_cpu_augment.py, not assumed)."""
    bm = border_mask(x.shape[-1], ksize)
    for _ in range(200):
        amb = accept_range(pre_of(x), delta)[2] & bm
        if not amb.any():
            return x
        v = x[amb]
        v = np.where((v < 0.0) | (v > MAX_PIXEL), 3333.3, v)  # a clipped pixel does not move under a nudge: give it a value that does
        x[amb] = np.where(v > MAX_PIXEL / 2, v - step, v + step).astype(np.float32)
    raise AssertionError("border set still ambiguous after 200 rounds of nudging")


def blur_case(name: str) -> Dict:
    """Inputs of a blur case: ``x`` (B, CT, S, S) fp32, ``apply`` (B,), ``k2`` (k, k) fp32, ``ksize``.  Every applied chip's border
    set is decided and its ambiguous share is below the cap (asserted on the CPU)."""
    B, CT, S, apply, k2, seed = {
        "k1": (2, 6, 224, [1, 0], gaussian_kernel2d(1, (0.1, 2.0)), 101),
        "k3": (2, 6, 224, [0, 1], gaussian_kernel2d(3, (0.1, 2.0)), 103),
        "k5": (2, 6, 224, [1, 0], gaussian_kernel2d(5, (1.0, 1.0)), 105),
        "k7": (2, 6, 224, [1, 1], gaussian_kernel2d(7, (1.5, 0.8)), 107),
        "s4k7": (2, 3, 4, [1, 1], gaussian_kernel2d(7, (1.5, 0.8)), 47),  # ksize = 2 S - 1: every tap row reflects
        "s2k3": (3, 2, 2, [1, 1, 1], asymmetric_kernel2d(3), 23),  # the reflected index is the far edge
        "s2k3g": (1, 2, 2, [1], gaussian_kernel2d(3, (1.0, 1.0)), 24),
        "pass2": (3, 18, 288, [1, 0, 1], gaussian_kernel2d(3, (0.1, 2.0)), 288),  # 4 478 976 elements: a second grid pass
    }[name]
    ksize = k2.shape[0]
    x = _raster(np.random.default_rng(seed), (B, CT, S, S), floats=True)
    on = [b for b in range(B) if apply[b]]
    delta = blur_delta(ksize)
    x[on] = _settle(x[on], lambda v: blur_pre(v, k2), delta, ksize, step=3.0 * delta / float(k2[ksize // 2, ksize // 2]))
    return {"name": name, "x": x, "apply": apply, "k2": k2, "ksize": ksize, "delta": delta}


BLUR_CASES = ("k1", "k3", "k5", "k7", "s4k7", "s2k3", "s2k3g", "pass2")
IMPULSE_S = 9


def impulse_positions(S: int = IMPULSE_S) -> List[Tuple[int, int]]:
    """Four corners, four edge midpoints, and the four pixels one step inside the corners (their reflected taps fold onto real ones)."""
    e, m = S - 1, S // 2
    return [(0, 0), (0, e), (e, 0), (e, e), (0, m), (m, 0), (e, m), (m, e), (1, 1), (1, e - 1), (e - 1, 1), (e - 1, e - 1)]


def impulse_case(ksize: int) -> Dict:
    """One band per impulse position: zeros and one pixel of height h, blurred with the asymmetric kernel.  The response is the
    reflected kernel times h; h is the first of 5000.5, 5001.5, ... at which every response pixel is decided (zeros elsewhere are the
    clamp plateau), so the comparison is exact everywhere."""
    S, k2, delta = IMPULSE_S, asymmetric_kernel2d(ksize, seed=10 + ksize), blur_delta(ksize)
    pos = impulse_positions(S)
    for i in range(2000):
        x = np.zeros((1, len(pos), S, S), dtype=np.float32)
        for c, (r, q) in enumerate(pos):
            x[0, c, r, q] = 5000.5 + i
        if not accept_range(blur_pre(x, k2), delta)[2].any():
            return {"name": f"impulse_k{ksize}", "x": x, "apply": [1], "k2": k2, "ksize": ksize, "delta": delta, "positions": pos}
    raise AssertionError("no impulse height leaves every tap decided")


def noise_case(noise_std: float) -> Dict:
    """Inputs of the given-field noise cases: ``x`` (3, 18, 288, 288) integer-valued fp32 (4 478 976 elements: a second grid pass),
    ``z`` the standard-normal field, chip 1 skipped.  For noise_std > 0 the corners of the applied bands are decided (z nudged)."""
    B, CT, S = 3, 18, 288
    rng = np.random.default_rng(2024)
    x = _raster(rng, (B, CT, S, S), floats=False)
    x[..., -S // 8 :, :] = 12000.0  # above max_pixel: the clip's upper side on whole rows
    z = rng.standard_normal((B, CT, S, S)).astype(np.float32)
    apply, on = [1, 0, 1], [0, 2]
    if noise_std > 0:
        delta = noise_delta()
        bm = border_mask(S, 1)
        zo = z[on]
        for _ in range(200):
            amb = accept_range(noise_pre(x[on], zo, noise_std), delta)[2] & bm
            if not amb.any():
                break
            zo[amb] += np.float32(0.37123)  # moves the value by a generic fraction of a count at both noise_std
        z[on] = zo
    return {"name": f"std{noise_std}", "x": x, "z": z, "apply": apply, "noise_std": noise_std, "delta": noise_delta()}


NOISE_STDS = (0.0, 0.05, 1.0)


def noise_std0_expected(x: np.ndarray, max_pixel: float = MAX_PIXEL) -> np.ndarray:
    """The noise operation at noise_std = 0 in exact fp32 operations: trunc(fl(fl(clip(x) / max) * max)) -- a + z * 0 is a, fused or not.
    Every step is a correctly rounded IEEE operation on the device as here, so the comparison is bit for bit."""
    m = np.float32(max_pixel)
    a = np.clip(np.asarray(x, dtype=np.float32), np.float32(0), m) / m
    return np.floor(np.clip(a, np.float32(0), np.float32(1)) * m).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
# the generated field's counter hash (csrc/augment.hip: aug_hash is the public "lowbias32" integer hash), restated to aim a seed
M32 = 0xFFFFFFFF


def lowbias32(x: int) -> int:
    x &= M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def lowbias32_inverse(h: int) -> int:
    h ^= h >> 16
    h = (h * pow(0x846CA68B, -1, 1 << 32)) & M32
    h ^= (h >> 15) ^ (h >> 30)
    h = (h * pow(0x7FEB352D, -1, 1 << 32)) & M32
    h ^= h >> 16
    return h


def seed_with_u1(idx: int, top24: int) -> int:
    """The int32 seed under which element ``idx`` of a chip draws h1 >> 8 == top24 in ``aug_noise_kernel`` (h1 = hash(2 idx +
    0x9e3779b9 * seed)): top24 = 0xFFFFFF is u1 = 1 exactly (log 0 side: z = 0), top24 = 0 is u1 = 2^-24 (the largest radius)."""
    v = lowbias32_inverse((top24 << 8) | 0x5A)
    s = ((v - 2 * idx) * pow(0x9E3779B9, -1, 1 << 32)) & M32
    assert lowbias32((2 * idx + 0x9E3779B9 * s) & M32) >> 8 == top24
    return s - (1 << 32) if s >= (1 << 31) else s


# ---------------------------------------------------------------------------------------------------------------------------------
# the whole chain (crop + flips -> rotate -> brightness -> blur -> noise) under the same rule
CHAIN_MEAN = [0.14245495, 0.13921481, 0.12434631, 0.31420089, 0.20743526, 0.12046503]
CHAIN_STD = [0.04036231, 0.04186983, 0.05267646, 0.0822221, 0.06834774, 0.05294205]


def chain_case() -> Dict:
    """``process_and_augment_batch`` with every augmentation on: 4 chips of T = 3 x 6 bands, 80 x 80 cropped to 64 x 64; the host draws
    are seeded and replayed here, the noise step of the plan carries a given standard-normal field.  Returns the inputs, the plan and
    per chip the accepted interval (lo, hi, ambiguous) of the raw-domain result and the expected label."""
    import random

    import torch

    from instageo_amd import dataloader as DL
    from oracle import prithvi_oracle as O

    B, T, C, Hs, im = 4, 3, 6, 80, 64
    g = torch.Generator().manual_seed(12)
    raw = torch.randint(0, 10000, (B, T * C, Hs, Hs), generator=g).to(torch.int16)
    lab = torch.randint(-1, 2, (B, Hs, Hs), generator=g).float()
    augs = {"hflip": {"use": True, "p": 0.5}, "vflip": {"use": True, "p": 0.5}, "rotate": {"use": True, "p": 0.7, "degrees": 10},
            "brightness": {"use": True, "p": 0.7, "brightness_range": [0.8, 1.2], "contrast_range": [0.8, 1.2]},
            "blur": {"use": True, "p": 0.7, "kernel_size": 3, "sigma_range": [0.1, 2.0]}, "noise": {"use": True, "p": 1.0, "noise_std": 0.05}}
    params = DL.draw_augment_params(B, (Hs, Hs), im, True, augs, torch.Generator().manual_seed(4))
    plan = DL.draw_photometric_params(B, im, augs, random.Random(8))
    z = torch.randn((B, T * C, im, im), generator=torch.Generator().manual_seed(6))
    plan[-1]["noise"] = z
    k2 = gaussian_kernel2d(3, (0.1, 2.0))
    r = random.Random(8)
    chips = []
    for b in range(B):
        top, left, hf, vf = params[b].tolist()
        cx, cy = O.crop_flip_chip(raw[b].numpy(), lab[b].numpy(), top, left, bool(hf), bool(vf), im)
        rot = r.random() < 0.7
        ang = r.uniform(-10, 10) if rot else 0.0
        bc = r.random() < 0.7
        bright, contrast = (r.uniform(0.8, 1.2), r.uniform(0.8, 1.2)) if bc else (1.0, 1.0)
        blur = r.random() < 0.7
        assert r.random() < 1.0
        r.getrandbits(31)
        x = cx.astype(np.float32)
        if rot:
            x = np.stack([rotate(v, ang, 0.0) for v in x])
        x = x.astype(np.float64)
        tol = np.zeros_like(x)
        if bc:
            pairs = [brightness_contrast(v, bright, contrast) for v in x]
            x, tol = np.stack([p for p, _ in pairs]), np.stack([t for _, t in pairs])
        if blur:  # uncertain input (tol, through the 1-Lipschitz clip and positive weights of sum 1) on top of the blur's own delta
            lo_b, hi_b, amb = accept_range(blur_pre(x, k2), blur_delta(3) + float(tol.max()))
        else:  # the float64 value is within tol of the kernel's fp32 one: carried into the noise stage's delta
            lo_b, hi_b, amb = x, x, np.zeros(x.shape, dtype=bool)
        d_n = noise_delta() + (0.0 if blur else float(tol.max()))
        lo, _, a1 = accept_range(noise_pre(lo_b, z[b].numpy(), 0.05), d_n)
        _, hi, a2 = accept_range(noise_pre(hi_b, z[b].numpy(), 0.05), d_n)
        chips.append({"lo": lo, "hi": hi, "ambiguous": amb | a1 | a2 | (lo != hi),
                      "label": rotate(cy.astype(np.float32), ang, -1.0) if rot else cy.astype(np.float32),
                      "stages": (rot, bc, blur)})
    return {"raw": raw, "lab": lab, "augs": augs, "params": params, "plan": plan, "T": T, "im": im, "chips": chips}
