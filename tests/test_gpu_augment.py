"""The four augmentation kernels of csrc/augment.hip at their edges (-m gpu), entry through ``instageo_amd.ops``: rotation bit for bit
against the Pillow-pinned oracle; brightness / contrast within the tolerance derived from its operation count; blur and noise exact on
every pixel the float64 reference decides, either neighbour on the ambiguous ones (tests/augment_reference.py holds the rule, the
derivations and the seeded inputs; tests/test_cpu_augment.py checks the ambiguity caps of every case without a GPU).  Each of rotate,
blur and noise has a case past one pass of its grid-stride loop (16384 workgroups x 256 threads = 4 194 304 elements), compared in full.
Every comparison prints its figures before it asserts."""
import functools
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import augment_reference as R  # noqa: E402
from instageo_amd import _lib  # noqa: E402
from instageo_amd import dataloader as DL  # noqa: E402
from instageo_amd import ops  # noqa: E402

DEV = "cuda"
MAXP = R.MAX_PIXEL


def _bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _rot_table(apply, angles, S):
    return torch.tensor([[a, *DL.rotate_coeffs(ang, S), 0] for a, ang in zip(apply, angles)], dtype=torch.int32)


def _check_rotation(raw, lab, apply, angles, fill, lab_fill, out, lab_out):
    B, CT = raw.shape[:2]
    got, gl = out.cpu().numpy(), lab_out.cpu().numpy()
    for b in range(B):
        for c in range(CT):
            ref = R.rotate(raw[b, c].numpy(), angles[b], fill) if apply[b] else raw[b, c].numpy()
            assert np.array_equal(_bits(got[b, c]), _bits(ref)), (b, c, angles[b])
        ref = R.rotate(lab[b].numpy(), angles[b], lab_fill) if apply[b] else lab[b].numpy()
        assert np.array_equal(_bits(gl[b]), _bits(ref)), (b, "label", angles[b])


# ---- rotate ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", R.ROT_SIZES)
def test_rotate_every_angle_at_small_odd_and_even_sizes(S):
    """Bit for bit, images and labels, at S = 1 to 3, odd and even sizes and every special, wrapped and sub-pixel angle; two chips of the
    batch are skipped (their rows still carry coefficients: the copy branch must ignore them); image fill negative, label fill not."""
    angles = list(R.ROT_ANGLES) + [33.3, -7.0]
    apply = [1] * len(angles)
    apply[3], apply[12] = 0, 0
    B, CT = len(angles), 2
    g = torch.Generator().manual_seed(100 + S)
    raw = (torch.rand((B, CT, S, S), generator=g) * 10000.0).float()
    lab = torch.randint(-1, 3, (B, S, S), generator=g).float()
    prm = _rot_table(apply, angles, S)
    out, lo = ops.aug_rotate(raw.to(DEV), prm.to(DEV), -3.5, lab.to(DEV), 255.0)
    _check_rotation(raw, lab, apply, angles, -3.5, 255.0, out, lo)
    o2, l2 = ops.aug_rotate(raw.to(DEV), prm.to(DEV), -3.5)  # labels=None: the same images
    assert l2 is None and torch.equal(o2.view(torch.int32), out.view(torch.int32))
    if S == 17:  # a NaN image fill, compared by bits
        on, ln = ops.aug_rotate(raw.to(DEV), prm.to(DEV), float("nan"), lab.to(DEV), -1.0)
        assert bool(torch.isnan(on[4]).any()) and not bool(torch.isnan(on[3]).any()) and not bool(torch.isnan(ln).any())
        _check_rotation(raw, lab, apply, angles, float("nan"), -1.0, on, ln)


def test_rotate_past_one_grid_pass():
    """4 chips x (18 bands + label) x 256^2 = 4 980 736 elements: the second pass of the grid-stride loop starts inside chip 3 (own
    angle); chip 2 is skipped, so the copy branch is crossed too.  Every plane is compared."""
    B, CT, S = 4, 18, 256
    assert B * (CT + 1) * S * S > R.ONE_PASS > 3 * (CT + 1) * S * S
    g = torch.Generator().manual_seed(7)
    raw = torch.randint(0, 10000, (B, CT, S, S), generator=g).float()
    lab = torch.randint(-1, 13, (B, S, S), generator=g).float()
    angles, apply = [7.3, -14.9, 45.0, 33.3], [1, 1, 0, 1]
    out, lo = ops.aug_rotate(raw.to(DEV), _rot_table(apply, angles, S).to(DEV), 0.0, lab.to(DEV), -1.0)
    _check_rotation(raw, lab, apply, angles, 0.0, -1.0, out, lo)


def test_rotate_at_the_largest_accepted_size():
    """S = 4096, 45 degrees: the 16.16 products of the walk are at their largest; against the oracle's int64 evaluation."""
    S = 4096
    raw = torch.randint(0, 10000, (1, 1, S, S), generator=torch.Generator().manual_seed(9)).float()
    out, _ = ops.aug_rotate(raw.to(DEV), _rot_table([1], [45.0], S).to(DEV), -1.0)
    assert np.array_equal(out[0, 0].cpu().numpy(), R.rotate(raw[0, 0].numpy(), 45.0, -1.0))


def test_rotate_entry_point_checks():
    S = 8
    raw = torch.zeros((2, 3, S, S), device=DEV)
    lab = torch.zeros((2, S, S), device=DEV)
    prm = _rot_table([1, 1], [5.0, 6.0], S).to(DEV)
    out = torch.empty_like(raw)
    p, st = ops._p, ops._stream()
    with pytest.raises(_lib.HipLibraryError, match="src and dst must differ"):
        _lib.call("ig_aug_rotate", p(raw), p(raw), None, None, p(prm), 0.0, 0.0, 2, 3, S, st)
    for li, lo in ((p(lab), None), (None, p(lab))):
        with pytest.raises(_lib.HipLibraryError, match="go together"):
            _lib.call("ig_aug_rotate", p(raw), p(out), li, lo, p(prm), 0.0, 0.0, 2, 3, S, st)
    with pytest.raises(_lib.HipLibraryError, match="S <= 4096"):
        _lib.call("ig_aug_rotate", p(raw), p(out), None, None, p(prm), 0.0, 0.0, 2, 3, 4097, st)
    e = torch.empty((0, 3, S, S), device=DEV)
    r, l = ops.aug_rotate(e, torch.empty((0, 8), dtype=torch.int32, device=DEV), 0.0, torch.empty((0, S, S), device=DEV), -1.0)
    assert r.shape == e.shape and l.shape == (0, S, S)


# ---- brightness / contrast -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 6, 34, 224])
def test_brightness_contrast_within_the_derived_tolerance(S):
    """n = 4, 36, 1156, 50176 pixels per band (most threads idle; not a multiple of the 1024-element stride; many strides).  Chips:
    0 constant bands (the mean is the value, contrast cancels: clamp(fl(v * bright)) exactly), 1 an offset band 9000 +- 2, 2 values
    below 0 and above max_pixel, 3 zeros (exactly 0), 4 skipped with a NaN planted (unchanged bit for bit); own factors per chip."""
    g = torch.Generator().manual_seed(200 + S)
    CT = 3
    u = lambda: torch.rand((CT, S, S), generator=g)
    const = torch.tensor([1234.5, 9000.0, 0.37]).view(CT, 1, 1).expand(CT, S, S)
    raw = torch.stack([const, 9000.0 + (u() * 4.0 - 2.0), u() * 17000.0 - 3000.0, torch.zeros(CT, S, S), u() * 10000.0]).float().contiguous()
    raw[4, 1, S // 2, 0] = float("nan")
    bp = torch.tensor([[1, 1.17, 0.83, 0], [1, 1.0, 1.2, 0], [1, 0.8, 1.17, 0], [1, 1.2, 0.8, 0], [0, 1.3, 0.7, 0]], dtype=torch.float32)
    got = ops.aug_brightness_contrast(raw.clone().to(DEV), bp.to(DEV), MAXP).cpu().numpy()
    for b in (1, 2):
        for c in range(CT):
            ref, tol = R.brightness_contrast(raw[b, c].numpy(), float(bp[b, 1]), float(bp[b, 2]))
            err = np.abs(got[b, c] - ref)
            print(f"brightness S={S} chip {b} band {c}: worst |error| {err.max():.3e}, derived bound there {tol.flat[err.argmax()]:.3e}, "
                  f"worst error / bound {np.max(err / np.maximum(tol, 1e-30)):.3f}")
            assert (err <= tol).all(), (S, b, c, float(err.max()))
    for c in range(CT):
        exp = np.clip(np.float32(const[c, 0, 0].item()) * np.float32(bp[0, 1].item()), np.float32(0), np.float32(MAXP))
        assert np.array_equal(got[0, c], np.full((S, S), exp, np.float32)), (S, c)
    assert got[0, 1, 0, 0] == MAXP  # 9000 * 1.17 is clamped
    assert not got[3].any()
    assert np.array_equal(_bits(got[4]), _bits(raw[4].numpy())) and np.isnan(got[4, 1, S // 2, 0])


def test_brightness_contrast_refuses_odd_sizes():
    """The kernel reads float4: the entry point reports S * S % 4 != 0.  The data loader never gets that far with an odd chip size:
    ``process_and_augment_batch`` raises at its first kernel (the crop needs a multiple of 4) instead of skipping the augmentation or
    corrupting the batch, and ``apply_photometric`` on its own refuses an odd size with brightness on before any kernel runs."""
    with pytest.raises(_lib.HipLibraryError, match="multiple of 4"):
        ops.aug_brightness_contrast(torch.zeros((1, 2, 33, 33), device=DEV), torch.tensor([[1.0, 1.0, 1.0, 0.0]], device=DEV), MAXP)
    x = torch.randint(0, 10000, (2, 6, 40, 40), generator=torch.Generator().manual_seed(1)).to(torch.int16).to(DEV)
    y = torch.zeros((2, 40, 40), device=DEV)
    augs = {"rotate": {"use": True, "p": 1.0}, "brightness": {"use": True, "p": 1.0}}
    with pytest.raises(_lib.HipLibraryError, match=r"multiple of 4 \(got 33\)"):
        DL.process_and_augment_batch(x, y, [0.0] * 6, [1.0] * 6, 1, 33, True, augs, 1.0, rng=random.Random(0))
    buf = torch.full((2, 6, 33, 33), 7.0, device=DEV)
    plan = DL.draw_photometric_params(2, 33, augs, random.Random(0))
    with pytest.raises(ValueError, match="even chip size"):
        DL.apply_photometric(buf, None, plan)
    assert float(buf.min()) == 7.0 and float(buf.max()) == 7.0


# ---- blur ------------------------------------------------------------------------------------------------------------------------
def _assert_rule(tag, st):
    print(f"{tag}: delta {st['delta']:.4f}, ambiguous share {st['share']:.4f}, ambiguous in the border set {st['border']}, "
          f"pixels one count off the float64 truncation {st['flipped']}, farthest such pixel from its integer {st['margin']:.2e}, "
          f"pixels outside the accepted range {st['bad']}")
    assert st["bad"] == 0 and st["share"] <= R.AMBIGUOUS_CAP and st["border"] == 0, (tag, st)


@pytest.mark.parametrize("name", R.BLUR_CASES)
def test_blur_every_band_under_the_decided_rule(name):
    """ksize 1, 3, 5, 7 at S = 224; ksize = 2 S - 1 at S = 4 and ksize = 3 at S = 2 (the reflected index is the far edge); 3 x 18 x 288^2 =
    4 478 976 elements with the middle chip skipped (second grid pass).  Values below 0 and above max_pixel are clipped first.  Exact on
    every decided pixel of every band; skipped chips are copied bit for bit."""
    c = R.blur_case(name)
    x = torch.from_numpy(c["x"])
    got = ops.aug_blur(x.to(DEV), torch.tensor(c["apply"], dtype=torch.int32, device=DEV), torch.from_numpy(c["k2"]).to(DEV), MAXP).cpu().numpy()
    on = [b for b, a in enumerate(c["apply"]) if a]
    for b, a in enumerate(c["apply"]):
        if not a:
            assert np.array_equal(_bits(got[b]), _bits(c["x"][b])), (name, b)
    _assert_rule(f"blur {name}", R.compare_truncated(got[on], R.blur_pre(c["x"][on], c["k2"]), c["delta"], c["ksize"]))


@pytest.mark.parametrize("ksize", [3, 5])
def test_blur_impulse_response_is_the_reflected_kernel(ksize):
    """One impulse per corner, per edge midpoint and per pixel next to a corner, an asymmetric kernel, a height at which every tap is
    decided: the response is compared exactly, so a shifted reflection index or a transposed tap shows."""
    c = R.impulse_case(ksize)
    got = ops.aug_blur(torch.from_numpy(c["x"]).to(DEV), torch.ones(1, dtype=torch.int32, device=DEV), torch.from_numpy(c["k2"]).to(DEV), MAXP)
    pre = R.blur_pre(c["x"], c["k2"])
    st = R.compare_truncated(got.cpu().numpy(), pre, c["delta"], ksize)
    assert st["share"] == 0.0
    _assert_rule(c["name"], st)
    assert np.array_equal(got.cpu().numpy(), R.truncate(pre))


def test_blur_entry_point_checks():
    x = torch.zeros((1, 1, 2, 2), device=DEV)
    ap = torch.ones(1, dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.HipLibraryError, match="ksize / 2 < S"):
        ops.aug_blur(x, ap, torch.full((2, 2), 0.25, device=DEV), MAXP)  # even
    with pytest.raises(_lib.HipLibraryError, match="ksize / 2 < S"):
        ops.aug_blur(x, ap, torch.full((5, 5), 0.04, device=DEV), MAXP)  # 5 / 2 >= 2: a second reflection would be needed
    assert "2*S" not in _lib.last_error()


# ---- noise -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _noise_case(std):
    return R.noise_case(std)


@pytest.mark.parametrize("std", R.NOISE_STDS)
def test_noise_with_a_given_field_under_the_decided_rule(std):
    """3 x 18 x 288^2 = 4 478 976 elements (second grid pass), chip 1 skipped, every band.  noise_std 0.05 and 1.0 under the rule; at 0 the
    result is the fp32 scale round trip, bit for bit (tests/test_cpu_augment.py: trunc(clip(x)) except where fp32 falls one ulp short)."""
    c = _noise_case(std)
    prm = torch.tensor([[a, 5 + b] for b, a in enumerate(c["apply"])], dtype=torch.int32)
    got = ops.aug_noise(torch.from_numpy(c["x"]).clone().to(DEV), prm.to(DEV), std, MAXP, torch.from_numpy(c["z"]).to(DEV)).cpu().numpy()
    assert np.array_equal(_bits(got[1]), _bits(c["x"][1]))
    on = [0, 2]
    if std == 0.0:
        exp = R.noise_std0_expected(c["x"][on])
        assert np.array_equal(got[on], exp)
        same = exp == np.floor(np.clip(c["x"][on], 0, MAXP))
        print(f"noise std 0: {got[on].size} pixels equal the fp32 round trip; {same.mean():.4f} of them equal trunc(clip(x))")
        assert same.mean() > 0.9
        return
    _assert_rule(f"noise std {std}", R.compare_truncated(got[on], R.noise_pre(c["x"][on], c["z"][on], std), c["delta"]))


def test_generated_noise_depends_on_the_seed_alone():
    """(a) two runs are bit-identical; (b) a chip's field depends on its seed only: position 3 of a 4 x 18 x 256^2 batch (4 718 592
    elements, the second grid pass starts inside that chip) equals position 0 of a batch of one; (c) other seeds give other fields."""
    B, CT, S = 4, 18, 256
    assert B * CT * S * S > R.ONE_PASS > 3 * CT * S * S
    x = torch.randint(2000, 8000, (B, CT, S, S), generator=torch.Generator().manual_seed(3)).float()
    prm = torch.tensor([[1, 11], [1, 12], [0, 13], [1, 987654321]], dtype=torch.int32)
    n1 = ops.aug_noise(x.clone().to(DEV), prm.to(DEV), 0.05, MAXP).cpu()
    n2 = ops.aug_noise(x.clone().to(DEV), prm.to(DEV), 0.05, MAXP).cpu()
    assert torch.equal(n1, n2) and torch.equal(n1[2], x[2])
    one = ops.aug_noise(x[3:4].clone().to(DEV), prm[3:4].to(DEV), 0.05, MAXP).cpu()
    assert torch.equal(one[0], n1[3])
    same_input = x[3:4].repeat(2, 1, 1, 1)
    two = ops.aug_noise(same_input.to(DEV), torch.tensor([[1, 987654321], [1, 987654322]], dtype=torch.int32, device=DEV), 0.05, MAXP).cpu()
    assert torch.equal(two[0], n1[3]) and not torch.equal(two[0], two[1])
    assert float((two[0] != two[1]).float().mean()) > 0.99


def test_generated_noise_is_finite_and_in_range_at_the_ends_of_u1():
    """(d) seeds 0, 1, -1, 2^31 - 1, and two seeds aimed (by inverting the counter hash) so that one known element draws u1 = 1 (log 0
    side: z is 0, the pixel keeps its value) and another u1 = 2^-24 (the largest radius): every output is finite and in [0, max]."""
    CT, S, idx = 6, 64, 5
    seeds = [0, 1, -1, 2 ** 31 - 1, R.seed_with_u1(idx, 0xFFFFFF), R.seed_with_u1(idx, 0)]
    x = torch.full((len(seeds), CT, S, S), 5000.0)
    x[:, 1], x[:, 2] = 0.0, 10000.0
    prm = torch.tensor([[1, s] for s in seeds], dtype=torch.int32)
    for std in (0.05, 1.0):
        out = ops.aug_noise(x.clone().to(DEV), prm.to(DEV), std, MAXP).cpu()
        assert bool(torch.isfinite(out).all()) and float(out.min()) >= 0.0 and float(out.max()) <= MAXP and torch.equal(out, out.floor())
        assert float(out[4].flatten()[idx]) == 5000.0  # u1 = 1: radius sqrt(-2 log 1) = 0
        assert float((out[:, 0] != 5000.0).float().mean()) > 0.9
    r = (out[5].flatten()[idx] - 5000.0) / 10000.0  # u1 = 2^-24: |z| <= sqrt(48 ln 2) = 5.77
    assert abs(float(r)) <= 0.5


def test_generated_noise_moments():
    """(e) the moment checks of test_gpu_pipeline.py on their shape, with their bounds."""
    mid = torch.full((2, 6, 224, 224), 5000.0)
    seeds = torch.tensor([[1, 42], [1, 43]], dtype=torch.int32)
    n1 = ops.aug_noise(mid.clone().to(DEV), seeds.to(DEV), 0.05, MAXP).cpu()
    r = (n1 - 5000.0) / 500.0
    assert abs(float(r.mean())) < 5e-3 and abs(float(r.std()) - 1.0) < 5e-3
    assert abs(float((r > 1.0).float().mean()) - 0.1587) < 3e-3 and abs(float((r.abs() > 2.0).float().mean()) - 0.0455) < 2e-3


# ---- chain -----------------------------------------------------------------------------------------------------------------------
def test_chain_with_every_augmentation_and_a_given_noise_field():
    """``process_and_augment_batch`` with crop, flips, rotate, brightness, blur and noise (p = 1.0) on, T = 3 (18 bands), 4 chips, against
    the chain of the reference helpers chip by chip with the host draws replayed.  The plan's noise step carries a given standard-normal
    field, so the WHOLE chain is compared under the decided / ambiguous rule (the interval each stage can reach is carried through
    the next, tests/augment_reference.py: chain_case); labels bit for bit."""
    c = R.chain_case()
    T, im, B = c["T"], c["im"], len(c["chips"])
    plan = [dict(s) for s in c["plan"]]
    plan[-1]["noise"] = plan[-1]["noise"].to(DEV)
    out, lo = DL.process_and_augment_batch(c["raw"].to(DEV), c["lab"].to(DEV), R.CHAIN_MEAN, R.CHAIN_STD, T, im, True, c["augs"], 1.0,
                                           params=c["params"], plan=plan, label_no_data_value=-1, chip_no_data_value=0, max_pixel_value=MAXP)
    assert out.shape == (B, 6, T, im, im) and lo.shape == (B, im, im)
    mean, std = np.array(R.CHAIN_MEAN)[:, None, None, None], np.array(R.CHAIN_STD)[:, None, None, None]
    slack = 4 * R.U * (MAXP + 1.0)  # (v - mean) / std in fp32 and back: two roundings each way, in raw counts
    for b, ch in enumerate(c["chips"]):
        raw = out[b].cpu().numpy().astype(np.float64) * std + mean  # (C, T, im, im), raw counts again
        v = np.rint(raw)
        assert np.abs(raw - v).max() <= slack, (b, float(np.abs(raw - v).max()))
        lo_b, hi_b, amb = (a.reshape(T, 6, im, im).transpose(1, 0, 2, 3) for a in (ch["lo"], ch["hi"], ch["ambiguous"]))
        bad = int(((v < lo_b) | (v > hi_b)).sum())
        print(f"chain chip {b}: stages (rotate, brightness, blur) {ch['stages']}, ambiguous share {amb.mean():.4f}, outside the range {bad}")
        assert bad == 0 and amb.mean() <= R.AMBIGUOUS_CAP, (b, bad)
        assert np.array_equal(lo[b].cpu().numpy(), ch["label"]), b
