"""Oracle of the rotate / brightness / blur / noise augmentations (oracle/augment_oracle.py) and the host side of their device
path: pinned against Pillow (the library the reference's RandomRotation calls through torchvision) -- no GPU needed."""
import math
import random

import numpy as np
import pytest
import torch

from oracle import augment_oracle as AO
from instageo_amd import dataloader as DL

PIL = pytest.importorskip("PIL.Image")


@pytest.mark.parametrize("shape", [(224, 224), (32, 32), (17, 23)])
def test_rotation_oracle_is_pillow_bit_for_bit(shape):
    rng = np.random.default_rng(shape[0])
    arr = rng.uniform(0, 10000, shape).astype(np.float32)
    angles = [0, 90, 180, 270, -90, 5.3, -10, 10, 45, -45, 123.456, 359.9, 1e-3, -1e-3] + list(rng.uniform(-15, 15, 12))
    for ang in angles:
        ref = np.array(PIL.fromarray(arr).rotate(ang, resample=PIL.NEAREST, expand=False, fillcolor=-1))
        assert np.array_equal(AO.rotate_nearest(arr, ang, -1), ref), f"angle {ang}"


def test_host_rotate_coeffs_equal_the_oracle():
    for ang in (0.0, 3.7, -14.2, 90.0, 180.0, 271.3):
        assert DL.rotate_coeffs(ang, 224) == AO.rotate_fixed_coeffs(ang, 224, 224)


def test_gaussian_kernel_matches_the_oracle_and_sums_to_one():
    k2 = DL.gaussian_kernel2d(3, (0.1, 2.0))
    kx, ky = AO.gaussian_kernel1d(3, 0.1), AO.gaussian_kernel1d(3, 2.0)
    assert torch.equal(k2, torch.mm(ky[:, None], kx[None, :]))
    assert abs(float(k2.sum()) - 1.0) < 1e-6
    # sigma_x = 0.1: practically no blur along x, sigma_y = 2.0: ~box along y (the reference's fixed pair, dataloader.py:303-305)
    assert k2[1, 1] > 0.3 and k2[1, 0] < 1e-6 and k2[0, 1] > 0.3


def test_blur_and_noise_oracle_known_answers():
    flat = np.full((8, 8), 5000.0, np.float32)
    assert np.all(AO.gaussian_blur(flat, 3, (0.1, 2.0), 10000.0) == 5000)  # a constant image stays constant (reflect padding)
    z = np.zeros((8, 8), np.float32)
    assert np.all(AO.gaussian_noise(flat, z, 0.05, 10000.0) == 5000)
    assert np.all(AO.gaussian_noise(flat, z + 1.0, 0.05, 10000.0) == 5500)
    assert np.all(AO.gaussian_noise(flat, z - 100.0, 0.05, 10000.0) == 0) and np.all(AO.gaussian_noise(flat, z + 100.0, 0.05, 10000.0) == 10000)
    bc = AO.brightness_contrast(np.array([[1000.0, 3000.0]], np.float32), 1.0, 2.0, 10000.0)
    assert np.allclose(bc, [[0.0, 4000.0]])  # contrast doubles the distance to the mean (2000), clamp at 0


def test_photometric_draws_follow_the_config_order_and_python_random():
    augs = {"hflip": {"use": True, "p": 0.5}, "rotate": {"use": True, "p": 0.5, "degrees": 10},
            "brightness": {"use": True, "p": 0.5, "brightness_range": [0.8, 1.2], "contrast_range": [0.9, 1.1]},
            "blur": {"use": False, "p": 0.5}, "noise": {"use": True, "p": 1.0, "noise_std": 0.05}}
    plan = DL.draw_photometric_params(5, 224, augs, random.Random(3))
    assert [s["name"] for s in plan] == ["rotate", "brightness", "noise"]
    # replay the reference's per-chip stream: random() < p, then the uniform draws, augmentation after augmentation
    r = random.Random(3)
    for b in range(5):
        rot = r.random() < 0.5
        ang = r.uniform(-10, 10) if rot else 0.0
        row = plan[0]["table"][b].tolist()
        assert row[0] == int(rot) and tuple(row[1:7]) == DL.rotate_coeffs(ang, 224)
        br = r.random() < 0.5
        exp = [1.0, r.uniform(0.8, 1.2), r.uniform(0.9, 1.1)] if br else [0.0, 1.0, 1.0]
        assert np.allclose(plan[1]["table"][b, :3].numpy(), exp, rtol=1e-6)
        assert r.random() < 1.0
        assert plan[2]["table"][b, 0] == 1 and plan[2]["table"][b, 1] == r.getrandbits(31)
    assert DL.draw_photometric_params(4, 224, {"hflip": {"use": True}}, random.Random(0)) == []
    with pytest.raises(NotImplementedError):
        DL.draw_augment_params(2, (256, 256), 224, True, {"rotate": {"use": True}, "hflip": {"use": True}})


# ---- the float64 reference helpers and the cases of tests/test_gpu_augment.py (tests/augment_reference.py) ---------------------------
import augment_reference as R  # noqa: E402

NEW_SIZES = (1, 2, 3, 17, 33, 225)


@pytest.mark.parametrize("S", NEW_SIZES)
def test_rotation_at_small_and_odd_sizes_is_pillow_and_the_host_coefficients_agree(S):
    """Pillow's centre S / 2 and the fixed-point walk at odd sizes and at S = 1 to 3, at every angle the GPU file uses: the oracle equals
    ``PIL.Image.rotate`` bit for bit and ``DL.rotate_coeffs`` equals the oracle's coefficients."""
    arr = np.random.default_rng(S).uniform(0, 10000, (S, S)).astype(np.float32)
    for ang in R.ROT_ANGLES:
        ref = np.array(PIL.fromarray(arr).rotate(ang, resample=PIL.NEAREST, expand=False, fillcolor=-7))
        assert np.array_equal(R.rotate(arr, ang, -7.0), ref), (S, ang)
        assert DL.rotate_coeffs(ang, S) == AO.rotate_fixed_coeffs(ang, S, S), (S, ang)


def test_rotate_sums_stay_inside_int32_at_the_largest_size():
    """``aug_rotate_kernel`` evaluates (a2 + a1 * y) + a0 * x in int32.  At the accepted maximum S = 4096 every product, partial sum and
    sum stays inside int32 for every angle used (int64 evaluation; the sums are separable, so their extremes over the grid are the sums
    of the extremes over y and over x)."""
    S = 4096
    idx = np.arange(S, dtype=np.int64)
    lim = 2 ** 31
    for ang in R.ROT_ANGLES + (-45.0, 135.0, 225.0, 315.0):
        c = DL.rotate_coeffs(ang, S)
        assert c == AO.rotate_fixed_coeffs(ang, S, S)
        for a0, a1, a2 in (c[:3], c[3:]):
            row, col = a2 + a1 * idx, a0 * idx
            for v in (a1 * idx, col, row, row.max() + col.max(), row.min() + col.min()):
                assert -lim <= np.min(v) and np.max(v) < lim, (ang, int(np.min(v)), int(np.max(v)))
    assert abs(DL.rotate_coeffs(45.0, S)[0] * (S - 1)) < lim // 4  # the products closest to 2^31 use a quarter of the range


def test_accept_range_rule_on_hand_values():
    d = 0.01
    pre = np.array([[-3.0, 0.0, 0.004, 0.5, 0.995, 1.0, 1.005, 7.3, 9999.995, 10000.0, 10000.005, 10000.02, 12000.0]])
    lo, hi, amb = R.accept_range(pre, d)
    assert lo.tolist() == [[0, 0, 0, 0, 0, 0, 0, 7, 9999, 9999, 9999, 10000, 10000]]
    assert hi.tolist() == [[0, 0, 0, 0, 1, 1, 1, 7, 10000, 10000, 10000, 10000, 10000]]
    assert amb.tolist() == [[False, False, True, False, True, True, True, False, True, True, True, False, False]]
    assert R.truncate(pre).tolist() == [[0, 0, 0, 0, 0, 1, 1, 7, 9999, 10000, 10000, 10000, 10000]]
    got = np.array([[0.0, 0, 0, 0, 1, 0, 1, 7, 10000, 9999, 10000, 10000, 10000]])
    st = R.compare_truncated(got, pre, d)
    assert st["bad"] == 0 and st["flipped"] == 4 and abs(st["margin"] - 0.005) < 1e-9
    got[0, 7] = 8.0  # a decided pixel off by one count
    assert R.compare_truncated(got, pre, d)["bad"] == 1
    bm = R.border_mask(5, 3)
    assert bm.sum() == 16 and not bm[1:4, 1:4].any() and R.border_mask(5, 1).sum() == 4 and R.border_mask(2, 3).all()


def test_reference_helpers_match_the_fp32_oracle():
    """The float64 helpers against ``augment_oracle`` (torch fp32): blur and noise under the rule (no decided pixel differs),
    brightness / contrast within the derived tolerance plus torch's fp32 mean (n sequentially rounded additions: n U A (1 + |c|))."""
    rng = np.random.default_rng(5)
    for ksize, sigma in ((1, (0.1, 2.0)), (3, (0.1, 2.0)), (5, (1.0, 1.0)), (7, (1.5, 0.8))):
        k2 = R.gaussian_kernel2d(ksize, sigma)
        assert np.array_equal(k2, DL.gaussian_kernel2d(ksize, sigma).numpy())
        for S in (4, 17, 33):
            if ksize // 2 >= S:
                continue
            x = R._raster(rng, (S, S), floats=True)
            st = R.compare_truncated(AO.gaussian_blur(x, ksize, sigma, 10000.0), R.blur_pre(x, k2), R.blur_delta(ksize), ksize)
            assert st["bad"] == 0, (ksize, S, st)
    for S in NEW_SIZES:
        x = R._raster(rng, (S, S), floats=False)
        z = rng.standard_normal((S, S)).astype(np.float32)
        for std in (0.05, 1.0):
            st = R.compare_truncated(AO.gaussian_noise(x, z, std, 10000.0), R.noise_pre(x, z, std), R.noise_delta())
            assert st["bad"] == 0, (S, std, st)
    for S in (2, 6, 34):
        for x in (rng.uniform(0, 10000, (S, S)), 9000.0 + rng.uniform(-2, 2, (S, S)), rng.uniform(-3000, 14000, (S, S))):
            x = x.astype(np.float32)
            ref, tol = R.brightness_contrast(x, 0.83, 1.17)
            slack = S * S * R.U * np.abs(x * 0.83).mean() * (1 + 1.17)
            assert (np.abs(AO.brightness_contrast(x, 0.83, 1.17, 10000.0) - ref) <= tol + slack).all(), S
    ref, tol = R.brightness_contrast(np.array([[1000.0, 3000.0]], np.float32), 1.0, 2.0)
    assert np.array_equal(ref, [[0.0, 4000.0]]) and tol.max() < 2e-3
    ref, tol = R.brightness_contrast(np.zeros((4, 4), np.float32), 1.2, 0.8)
    assert not ref.any() and not tol.any()
    ref, tol = R.brightness_contrast(9000.0 + rng.uniform(-2, 2, (34, 34)).astype(np.float32), 1.0, 1.2)
    assert 2e-3 < tol.max() < 4e-3  # the offset band: the bound follows the magnitude, not the spread


@pytest.mark.parametrize("name", R.BLUR_CASES)
def test_blur_cases_meet_the_ambiguity_cap_and_have_a_decided_border(name):
    c = R.blur_case(name)
    on = [b for b, a in enumerate(c["apply"]) if a]
    assert c["delta"] == (c["ksize"] ** 2 + 3) * 2.0 ** -24 * 10000.0 and c["ksize"] // 2 < c["x"].shape[-1]
    share, border = R.case_conditions(R.blur_pre(c["x"][on], c["k2"]), c["delta"], c["ksize"])
    print(f"{name}: delta {c['delta']:.4f}, ambiguous share {share:.4f}, ambiguous in the border set {border}")
    assert share <= R.AMBIGUOUS_CAP and border == 0
    if c["x"].shape[-1] >= 224:
        assert (c["x"] < 0).any() and (c["x"] > 10000).any()  # the clip has both sides to act on
    assert np.array_equal(c["x"], R.blur_case(name)["x"])  # deterministic
    if name == "pass2":
        assert c["x"].size > R.ONE_PASS and c["apply"] == [1, 0, 1]


@pytest.mark.parametrize("ksize", [3, 5])
def test_impulse_cases_are_decided_everywhere(ksize):
    c = R.impulse_case(ksize)
    pre = R.blur_pre(c["x"], c["k2"])
    assert not R.accept_range(pre, c["delta"])[2].any()
    resp = R.truncate(pre)
    k2 = c["k2"].astype(np.float64)
    h = float(c["x"].max())
    assert not np.array_equal(c["k2"], c["k2"].T) and not np.array_equal(c["k2"], c["k2"][::-1, ::-1])
    for band, (r, q) in enumerate(c["positions"]):
        # correlation: out[y, x] takes tap (r - y + half, q - x + half) of the kernel, plus the taps that reflect onto (r, q)
        half, S = ksize // 2, R.IMPULSE_S
        exp = np.zeros((S, S))
        for y in range(S):
            for x in range(S):
                for dy in range(ksize):
                    for dx in range(ksize):
                        yy, xx = y + dy - half, x + dx - half
                        yy = -yy if yy < 0 else (2 * S - 2 - yy if yy >= S else yy)
                        xx = -xx if xx < 0 else (2 * S - 2 - xx if xx >= S else xx)
                        if (yy, xx) == (r, q):
                            exp[y, x] += k2[dy, dx]
        assert np.array_equal(resp[0, band], np.floor(exp * (h / 10000.0) * 10000.0)), (ksize, r, q)


@pytest.mark.parametrize("std", [0.05, 1.0])
def test_noise_cases_meet_the_ambiguity_cap_and_have_decided_corners(std):
    c = R.noise_case(std)
    assert c["x"].size > R.ONE_PASS and c["apply"] == [1, 0, 1] and c["delta"] == 4 * 2.0 ** -24 * 10000.0
    share, border = R.case_conditions(R.noise_pre(c["x"][[0, 2]], c["z"][[0, 2]], std), c["delta"])
    print(f"noise std {std}: delta {c['delta']:.4f}, ambiguous share {share:.4f}, ambiguous corners {border}")
    assert share <= R.AMBIGUOUS_CAP and border == 0
    assert np.array_equal(c["x"], R.noise_case(0.0)["x"])  # the three noise_std share one raster


def test_noise_at_std_zero_is_the_fp32_scale_round_trip():
    """At noise_std = 0 the operation is trunc(fl(fl(clip(x) / max) * max)) in fp32.  That is trunc(clip(x)) for most integers but NOT
    all: for 570 of the integers 0..10000 (7, 14, 28, 45, ...) the round trip lands one ulp below x and the truncation gives x - 1 -- in
    the reference's own torch arithmetic too.  The GPU test therefore expects the fp32 round trip (exact IEEE operations), which
    equals the oracle on every integer and equals trunc(clip(x)) wherever the round trip does not fall short."""
    x = np.arange(0, 10001, dtype=np.float32)
    rt = R.noise_std0_expected(x)
    assert np.array_equal(rt, AO.gaussian_noise(x[None], np.zeros((1, 10001), np.float32), 0.0, 10000.0)[0].astype(np.float32))
    short = rt != x
    assert short.sum() == 570 and np.array_equal(rt[short], x[short] - 1) and x[short][:4].tolist() == [7, 14, 28, 45]
    assert np.array_equal(R.noise_std0_expected(np.array([-50.0, 12000.0, 10000.0], np.float32)), [0.0, 10000.0, 10000.0])
    c = R.noise_case(0.0)
    assert np.array_equal(c["x"], np.round(c["x"]))  # integer-valued: the expectation above applies to every pixel


def test_chain_case_meets_the_ambiguity_cap():
    c = R.chain_case()
    stages = [ch["stages"] for ch in c["chips"]]
    assert any(all(s) for s in stages) and not all(all(s) for s in stages)  # applied and skipped stages both occur
    for b, ch in enumerate(c["chips"]):
        share = float(ch["ambiguous"].mean())
        print(f"chain chip {b}: stages {ch['stages']}, ambiguous share {share:.4f}")
        assert share <= R.AMBIGUOUS_CAP and (ch["hi"] - ch["lo"]).max() <= 2
    assert c["plan"][-1]["name"] == "noise" and c["plan"][-1]["noise"].shape == (4, 18, 64, 64)


def test_counter_hash_inverse_aims_a_seed():
    for v in (0, 1, 0x9E3779B9, 0xFFFFFFFF, 123456789):
        assert R.lowbias32_inverse(R.lowbias32(v)) == v and R.lowbias32(R.lowbias32_inverse(v)) == v
    for idx, top in ((5, 0xFFFFFF), (70000, 0)):
        s = R.seed_with_u1(idx, top)
        assert -2 ** 31 <= s < 2 ** 31 and R.lowbias32((2 * idx + 0x9E3779B9 * (s & R.M32)) & R.M32) >> 8 == top


def test_odd_chip_size_with_brightness_is_refused_before_any_kernel_runs():
    plan = DL.draw_photometric_params(2, 33, {"brightness": {"use": True, "p": 1.0}}, random.Random(0))
    with pytest.raises(ValueError, match="even chip size"):
        DL.apply_photometric(torch.zeros(2, 6, 33, 33), None, plan)
