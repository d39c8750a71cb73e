"""CPU checks of what tests/test_gpu_value_ranges_train.py stands on: the summation bound n 2^-52 sum |term_i| holds for numpy's own fp64 sums
against ``math.fsum`` in four orders on every family (so the reference side alone stays inside the bar), fp32 products do not (the bar sees the
defect it was written for), the metric bars cover what those sums do to the metrics, the seeds leave next to no pixel on the expected-error
threshold, and the AdamW / label-map references are what they claim to be."""
import math

import numpy as np
import pytest
import torch

import test_gpu_value_ranges_train as T

CASES = [(f, s) for f in T.REG_FAMILIES for s in T.REG_SHAPES]


def orders(n, seed):
    fwd = np.arange(n)
    return {"forward": fwd, "reversed": fwd[::-1], "permuted": np.random.default_rng(seed).permutation(n)}


@pytest.mark.parametrize("family,shape", CASES)
def test_numpy_sums_stay_inside_the_summation_bound(family, shape):
    v = T.reg_values(family, shape, T.reg_seed(family, shape))
    r = T.reg_terms(v["pred"], v["lab"])
    for name, t in r["terms"].items():
        s, bound = T.fsum_and_bound(t)
        for oname, o in orders(t.size, 7).items():
            for how, got in (("pairwise", float(np.sum(t[o]))), ("recursive", float(np.cumsum(t[o])[-1]))):
                assert abs(got - s) <= bound, (name, oname, how, abs(got - s), bound)


@pytest.mark.parametrize("shape", T.REG_SHAPES)
@pytest.mark.parametrize("family", ["off0", "off300", "off3000", "off30000"])
def test_fp32_products_miss_the_summation_bound(family, shape):
    """x * x, x * y, y * y rounded to fp32 before they are widened (what the kernels did): outside the bar at every offset,
    zero included."""
    v = T.reg_values(family, shape, T.reg_seed(family, shape))
    r = T.reg_terms(v["pred"], v["lab"])
    x, y = r["terms"]["Sx"].astype(np.float32), r["terms"]["Sy"].astype(np.float32)
    for name, prod in (("Sxx", x * x), ("Sxy", x * y), ("Syy", y * y)):
        s, bound = T.fsum_and_bound(r["terms"][name])
        err = abs(math.fsum(prod.astype(np.float64)) - s)
        assert err > bound, (name, err, bound)


@pytest.mark.parametrize("family,shape", CASES)
def test_metric_bars_cover_the_metrics_of_numpy_sums(family, shape):
    v = T.reg_values(family, shape, T.reg_seed(family, shape))
    r = T.reg_terms(v["pred"], v["lab"])
    sums, bounds = T.reference_sums([r])
    ref = T.regression_metrics_from_sums(sums[1:], T.EE_BIAS, T.EE_COEF, True)
    bars = T.metric_bars(sums[1:], bounds[1:])
    for o in orders(int(sums[1]), 11).values():
        got = T.regression_metrics_from_sums([float(np.cumsum(r["terms"][k][o])[-1]) for k in T.SUM_NAMES[1:-1]] + [sums[9]])
        for k in T.METRICS:
            if math.isnan(ref[k]):
                assert family == "const" and k in ("r2_score", "pearson_corrcoef") and math.isnan(got[k])
            else:
                assert abs(got[k] - ref[k]) <= bars[k], (k, got[k], ref[k], bars[k])
    assert (family == "const") == math.isnan(ref["r2_score"])


def test_the_families_are_what_they_say():
    for family, shape in CASES:
        for positive in (False, True):
            v = T.reg_values(family, shape, T.reg_seed(family, shape) + (500 if positive else 0), positive)
            ign, lab = v["ignored"], v["lab"]
            pred, tch = v["pred"].reshape(lab.shape), v["teacher"].reshape(lab.shape)
            assert 0 < int(ign.sum()) < ign.numel() // 5 and (lab[ign] == T.IGNORE).all() and (lab[~ign] != T.IGNORE).all()
            assert not torch.isfinite(pred[ign]).any() and not torch.isfinite(tch[ign]).any()
            assert torch.isfinite(pred[~ign]).all() and torch.isfinite(tch[~ign]).all()
            if ign.numel() > 1000:
                assert all(bool(f(pred[ign]).any()) for f in (torch.isnan, torch.isposinf, torch.isneginf))
            x = lab[~ign].double()
            if positive:
                assert (x >= 0).all() and (tch[~ign] >= 0).all() and (pred[~ign] >= 0).all()
            if family.startswith("off") and family != "off0":
                assert abs(x.mean().item() / float(family[3:]) - 1) < 0.01 and 0.8 < x.std().item() < 1.2
            elif family == "tiny":
                assert 0 <= x.min().item() and x.max().item() <= 1e-3
            elif family == "const":
                assert (x == T.CONST_LABEL).all()
            elif family == "wide":
                assert x.min().item() < 1e-2 and x.max().item() > 1e3


def test_expected_error_threshold_is_rarely_ambiguous():
    """At most 0.1 % of the pixels of every case the GPU tests use sit within 2 fp32 ulps of |e| = bias + coef x."""
    cases = [(f, s, T.reg_seed(f, s)) for f, s in CASES] + [("off3000", T.REG_SHAPES[0], 2001), ("off300", T.REG_SHAPES[1], 2002),
                                                             ("off300", T.REG_SHAPES[1], 2003)]
    for family, shape, seed in cases:
        v = T.reg_values(family, shape, seed)
        r = T.reg_terms(v["pred"], v["lab"])
        assert int(r["ambiguous"].sum()) <= 1e-3 * int(r["valid"].sum()), (family, shape)
        assert 0 < int(r["ee"].sum()), (family, shape)  # the count is not trivially zero


def test_adamw_references_agree_with_each_other():
    """The fp32 torch.optim.AdamW yardstick, started from a preset state at a late step, follows the float64 restatement."""
    for case, step0 in (("plain", 0), ("plain", 999), ("zero_grad", 9), ("cold", 0)):
        p0, g, m0, v0 = T.adamw_state(4 * 257, 3, case)
        ref, t32 = T.adamw_refs(p0, g, m0, v0, steps=2, step0=step0)
        for r, t in zip(ref, t32):
            assert torch.isfinite(t).all() and (t.double() - r).abs().max().item() <= 1e-6 * max(1.0, r.abs().max().item())
    p0, g, m0, v0 = T.adamw_state(4 * 1031, 304, "huge")
    ref, t32 = T.adamw_refs(p0, g, m0, v0)
    big = g.abs() > 1e20
    assert int(big.sum()) == 4 * 1031 // 100 and torch.isinf(t32[2][big]).all() and torch.isfinite(t32[2][~big]).all()
    assert torch.isfinite(t32[0]).all() and torch.isfinite(t32[1]).all() and torch.isfinite(ref[2]).all()
    p0, g, m0, v0 = T.adamw_state(4 * 1031, 304, "span")
    assert g.abs().min().item() < 1e-11 and g.abs().max().item() > 1e3 and (g < 0).any() and (g > 0).any()
    cap4 = T.adamw_one_pass_float4s()
    assert cap4 > 0 and cap4 % 64 == 0


@pytest.mark.parametrize("nbins", [3, 4096])
def test_label_map_expectation_equals_numpy_unique(nbins):
    lab, want = T.label_map(-1, nbins, seed=500 + nbins)
    a = lab.numpy().ravel()
    vals, cnts = np.unique(a[np.isfinite(a)], return_counts=True)  # -0.0 and 0.0 are one value here too
    for val, cnt in zip(vals, cnts):
        if val == np.floor(val) and -1 <= val < -1 + nbins:
            assert want[int(val) + 1] == cnt
    assert want.sum() == a.size and want[nbins] >= 2 * 9
    for s in (0.5, -2.0, float(nbins - 1), float("inf"), float("-inf"), 2.0**31, -(2.0**31), 3e9):
        assert (a == np.float32(s)).sum() >= 2, s
    assert np.isnan(a).sum() >= 2 and (np.signbit(a) & (a == 0)).sum() == 2
