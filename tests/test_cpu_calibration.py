"""Post-hoc calibration, host side (no GPU): the streaming temperature fit on injected sums of a closed-form problem, the ratio arithmetic
of the reliability histograms, calibration.json, the config keys and the argument checks of the two HIP entry points."""
import ctypes
import json
import math
import os

import numpy as np
import pytest

import calibration_reference as CR
from instageo_amd import calibration as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "instageo-e2e-geospatial-ml_amd")
NAMES = {"ig_calib_nll_grid", "ig_reliability_update"}


@pytest.fixture(scope="module")
def built_lib():
    import subprocess

    from instageo_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j4"], check=True)
    return _lib


# ---- TemperatureFitter on a closed-form problem ---------------------------------------------------------------------------------
# Two classes, logits (d, 0): n1 pixels labelled 0 (right, margin d) and n2 labelled 1 (wrong).  With beta = 1 / T
#   NLL(beta) = n1 log(1 + exp(-beta d)) + n2 log(1 + exp(beta d)),  convex in beta, minimal at exp(-beta d) = n2 / n1:
#   T* = d / ln(n1 / n2).
def analytic(n1, n2, d):
    f = lambda T: n1 * np.logaddexp(0.0, -d / T) + n2 * np.logaddexp(0.0, d / T)  # noqa: E731
    return f, d / math.log(n1 / n2)


def drive(fit, f, n):
    while not fit.done:
        fit.end_pass(sums=[f(T) for T in fit.grid()] + [f(1.0)], count=n)
    return fit.result()


@pytest.mark.parametrize("points,passes", [(32, 2), (9, 2), (32, 3), (5, 4)])
@pytest.mark.parametrize("d", [4.0, 1.0, 11.0])
def test_fitter_finds_the_analytic_optimum_within_one_fine_step(d, points, passes):
    f, t_star = analytic(900, 100, d)
    fit = C.TemperatureFitter(points=points, passes=passes)
    g0 = fit.grid()
    assert len(g0) == points and math.isclose(g0[0], 0.125) and math.isclose(g0[-1], 8.0)
    ratios = np.diff(np.log(g0))
    assert np.allclose(ratios, ratios[0])  # log-spaced
    res = drive(fit, f, 1000)
    last = res["grids"][-1]["temperatures"]
    fine_step = math.log(last[-1] / last[0]) / (points - 1)
    # the last grid spans [T_(i-1), T_(i+1)] of the one before: its step is that bracket / (points - 1), which is the bound
    prev = res["grids"][-2]["temperatures"] if passes > 1 else None
    if prev is not None:
        assert math.isclose(fine_step, 2 * math.log(prev[1] / prev[0]) / (points - 1), rel_tol=1e-9)
    assert abs(res["ln_temperature"] - math.log(t_star)) <= fine_step, (res["temperature"], t_star)
    assert res["vertex"] and res["n_valid"] == 1000
    # T* = 5.0 (d = 11) is nearer to the last point of the 5-point grid (8) than to the one before (2.8): that fit legitimately starts at a bound
    assert res["at_bound"] == (points == 5 and d == 11.0)
    assert math.isclose(res["nll_before"], f(1.0) / 1000) and res["nll_after"] <= res["nll_before"]
    assert res["nll_after"] <= min(res["grids"][-1]["nll_sums"]) / 1000  # the vertex lies below the three points it interpolates
    if points == 32:  # interpolation error of a parabola over a step h = 8.7e-3 (2.9e-4 at three passes): O(h^3) of a loss of order 0.3
        assert abs(res["nll_after"] - f(t_star) / 1000) < 1e-6
    assert len(res["grids"]) == passes and all(len(g["nll_sums"]) == points for g in res["grids"])
    with pytest.raises(RuntimeError):
        fit.end_pass(sums=[0.0] * (points + 1), count=1)


def test_default_fit_has_the_documented_fine_step():
    f, _ = analytic(900, 100, 4.0)
    res = drive(C.TemperatureFitter(), f, 1000)
    last = res["grids"][-1]["temperatures"]
    assert abs(math.log(last[-1] / last[0]) / 31 - 8.66e-3) < 1e-5


@pytest.mark.parametrize("d,side", [(40.0, "high"), (0.2, "low")])
def test_optimum_outside_the_range_moves_the_bracket_outward(d, side):
    f, t_star = analytic(900, 100, d)  # T* = 18.2 above t_max = 8, or 0.091 below t_min = 1 / 8
    fit = C.TemperatureFitter()
    g0 = fit.grid()
    fit.end_pass(sums=[f(T) for T in g0] + [f(1.0)], count=1000)
    g1 = fit.grid()
    ratio = g0[1] / g0[0]
    if side == "high":
        assert math.isclose(g1[0], g0[-2]) and math.isclose(g1[-1], g0[-1] * ratio) and g1[-1] > 8.0
    else:
        assert math.isclose(g1[-1], g0[1]) and math.isclose(g1[0], g0[0] / ratio) and g1[0] < 0.125
    fit.end_pass(sums=[f(T) for T in g1] + [f(1.0)], count=1000)
    res = fit.result()
    assert res["at_bound"] and fit.at_bound
    assert (res["temperature"] > 8.0) if side == "high" else (res["temperature"] < 0.125)


def test_flat_or_broken_triples_fall_back_to_the_grid_point():
    fit = C.TemperatureFitter(points=7, passes=1)
    g = fit.grid()
    fit.end_pass(sums=[3.0] * 7 + [3.0], count=10)  # flat: no curvature anywhere
    res = fit.result()
    assert not res["vertex"] and res["temperature"] == pytest.approx(g[0]) and res["nll_after"] == pytest.approx(0.3)
    fit = C.TemperatureFitter(points=7, passes=1)
    fit.end_pass(sums=[9.0, 8.0, math.inf, 1.0, math.inf, 8.0, 9.0, 2.0], count=10)  # second difference not finite
    res = fit.result()
    assert not res["vertex"] and res["temperature"] == pytest.approx(g[3]) and not res["at_bound"]
    fit = C.TemperatureFitter(points=7, passes=1)
    fit.end_pass(sums=[9.0, 8.0, 2.0, 1.0, 2.0, 8.0, 9.0, 2.0], count=0)  # nothing valid: ratios are NaN, not a division error
    res = fit.result()
    assert res["vertex"] and res["temperature"] == pytest.approx(g[3]) and math.isnan(res["nll_before"]) and math.isnan(res["nll_after"])
    with pytest.raises(ValueError):
        C.TemperatureFitter(points=7, passes=1).end_pass(sums=[1.0] * 7, count=1)  # the T = 1 slot is missing
    with pytest.raises(RuntimeError):
        C.TemperatureFitter().result()


# ---- reliability arithmetic -------------------------------------------------------------------------------------------------------
def test_reliability_from_hand_written_histograms():
    S = 2**24
    h = np.zeros((3, 3, 4), dtype=np.int64)
    # class 0: bin 1 holds 10 pixels, 4 right, mean confidence 0.3; bin 3 holds 30 pixels, 27 right, mean confidence 0.95
    h[0, :, 1] = [10, 4, 3 * S]
    h[0, :, 3] = [30, 27, int(28.5 * S)]
    # class 2: bin 3 holds 10 pixels, 5 right, mean confidence 0.8; class 1 is never predicted; bins 0 and 2 are empty
    h[2, :, 3] = [10, 5, 8 * S]
    r = C.reliability_from_histogram(h)
    # all classes together: bin 1: |0.4 - 0.3| = 0.1 (n 10); bin 3: acc 32 / 40 = 0.8, conf 36.5 / 40 = 0.9125 (n 40)
    assert r["n"] == 50 and r["bins"]["count"] == [0, 10, 0, 40]
    assert r["ece"] == pytest.approx(10 / 50 * 0.1 + 40 / 50 * 0.1125)
    assert r["mce"] == pytest.approx(0.1125)
    # class 0: 10 / 40 * 0.1 + 30 / 40 * 0.05 = 0.0625; class 2: 0.3; class 1 absent -> mean of two
    assert r["classwise_ece"] == pytest.approx((0.0625 + 0.3) / 2)
    acc, conf = r["bins"]["accuracy"], r["bins"]["confidence"]
    assert math.isnan(acc[0]) and math.isnan(conf[2]) and acc[1] == pytest.approx(0.4) and conf[3] == pytest.approx(0.9125)
    empty = C.reliability_from_histogram(np.zeros((3, 3, 4), dtype=np.int64))
    assert empty["n"] == 0 and all(math.isnan(empty[k]) for k in ("ece", "mce", "classwise_ece"))
    with pytest.raises(ValueError):
        C.reliability_from_histogram(np.zeros((3, 2, 4), dtype=np.int64))


def test_histogram_arithmetic_equals_the_per_pixel_definition():
    rng = np.random.default_rng(5)
    z = rng.normal(size=(2, 4, 9, 11)) * 2
    lab = rng.integers(0, 4, size=(2, 9, 11))
    lab[0, 0, :3] = -1
    ref = CR.reliability(z, lab, -1, 0.7, 15)
    r = C.reliability_from_histogram(ref["hist"])
    ece, mce = CR.ece_from_pixels(ref["conf"], ref["pred"] == ref["y"], 15)
    assert r["n"] == len(ref["y"]) == 2 * 99 - 3
    assert r["ece"] == pytest.approx(ece, abs=2**-24) and r["mce"] == pytest.approx(mce, abs=2**-24)


# ---- calibration.json, keys ---------------------------------------------------------------------------------------------------------
def _record(**kw):
    rec = {k: 0.25 for k in C.CALIBRATION_KEYS}
    rec.update(temperature=1.75, n_valid=10, at_bound=False, bins_before={"count": [0, 10], "accuracy": [float("nan"), 0.5]},
               bins_after={"count": [10, 0]}, grids=[])
    rec.update(kw)
    return rec


def test_calibration_json_round_trip(tmp_path):
    path = str(tmp_path / "calibration.json")
    line = C.write_calibration_json(path, _record())
    assert "\n" not in line and "NaN" not in line
    back = C.read_calibration_json(path)
    assert back == json.loads(line) and back["temperature"] == 1.75 and back["bins_before"]["accuracy"] == [None, 0.5]
    assert set(C.CALIBRATION_KEYS) <= set(back)
    assert C.resolve_temperature({"calibration": path}) == 1.75
    for bad in (0.0, -2.0, float("nan"), float("inf"), "warm", True):
        with pytest.raises(ValueError):
            C.write_calibration_json(path, _record(temperature=bad))
    with pytest.raises(ValueError):
        C.write_calibration_json(path, {"temperature": 1.0})
    for text in ('{"temperature": 0}', '{"temperature": -1.5}', '{"temperature": null}', '{"ece_after": 0.1}', "[1.0]"):
        (tmp_path / "bad.json").write_text(text)
        with pytest.raises(ValueError):
            C.read_calibration_json(str(tmp_path / "bad.json"))


def test_config_keys_and_their_checks(tmp_path):
    from instageo_amd.config import DEFAULTS, load_config
    from instageo_amd.factory import create_model

    t = DEFAULTS["test"]
    assert t["temperature"] is None and t["calibration"] is None and t["calibration_metrics"] is False
    assert DEFAULTS["calibrate"] == {"points": 32, "passes": 2, "t_min": 0.125, "t_max": 8.0, "nbins": 15}
    assert C.resolve_temperature(t) == 1.0 and C.resolve_temperature({"temperature": 2.5}) == 2.5
    for bad in (0, -1.0, float("nan"), float("inf"), "hot"):
        with pytest.raises(ValueError, match="temperature"):
            C.resolve_temperature({"temperature": bad})
    path = str(tmp_path / "calibration.json")
    C.write_calibration_json(path, _record())
    with pytest.raises(ValueError, match="both"):
        C.resolve_temperature({"temperature": 2.0, "calibration": path})
    C.check_calibrate_options()
    for kw, word in ((dict(points=2), "points"), (dict(points=33), "points"), (dict(points=8.0), "points"), (dict(passes=0), "passes"),
                     (dict(nbins=0), "nbins"), (dict(nbins=65), "nbins"), (dict(nbins=64, num_classes=65), "cells"),
                     (dict(t_min=0.0), "t_min"), (dict(t_min=2.0, t_max=1.0), "t_min"), (dict(t_max=float("inf")), "t_max")):
        with pytest.raises(ValueError, match=word):
            C.check_calibrate_options(**kw)
    with pytest.raises(ValueError):
        C.TemperatureFitter(points=40)
    with pytest.raises(ValueError):
        C.RunningReliability(5, nbins=0)
    # create_model checks the keys before it builds anything: no device is touched by these
    base = ["valid_filepath=synthetic:2", "checkpoint_path=/nonexistent.ckpt"]
    for ov, word in ((["mode=calibrate", "is_reg_task=true"], "regression"), (["mode=calibrate", "calibrate.points=40"], "points"),
                     (["mode=calibrate", "calibrate.nbins=0"], "nbins"), (["mode=eval", "test.temperature=-1"], "temperature"),
                     (["mode=eval", "test.temperature=.nan"], "temperature"),
                     (["mode=eval", "test.temperature=2.0", f"test.calibration={path}"], "both"),
                     (["mode=eval", "is_reg_task=true", "test.temperature=2.0"], "class probabilities")):
        with pytest.raises(ValueError, match=word):
            create_model(load_config("config", base + ov), device="cpu")
    with pytest.raises(KeyError):
        load_config("config", ["calibrate.bins=3"])


def test_tile_inference_checks_the_temperature_before_any_work():
    from instageo_amd.infer_utils import tile_inference

    args = ("/nonexistent/tile.tif", "/nonexistent/out", None, [0.0], [1.0])
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="temperature"):
            tile_inference(*args, blend="gaussian", temperature=bad)
    with pytest.raises(OSError):
        tile_inference(*args, blend="gaussian", temperature=2.0)


# ---- entry points ---------------------------------------------------------------------------------------------------------------
def test_entry_points_exported_and_validated_without_gpu(built_lib):
    """IG_REQUIRE rejects bad arguments before any launch (safe on a CPU-only box)."""
    assert NAMES <= set(built_lib.declared_symbols())
    lib = built_lib.load()
    err = built_lib.last_error
    one = ctypes.c_void_p(4096)
    f32 = lambda *v: (ctypes.c_float * len(v))(*v)  # noqa: E731

    nll = lib.ig_calib_nll_grid
    ok = f32(*([1.0] * 33))
    assert nll(one, one, 0, -1, ok, 0, one, one, 1, 64, 5, None) == -1 and "K" in err()
    assert nll(one, one, 0, -1, ok, 33, one, one, 1, 64, 5, None) == -1 and "K" in err()
    assert nll(one, one, 0, -1, None, 4, one, one, 1, 64, 5, None) == -1 and "inv_temps" in err()
    for bad in (0.0, -0.5, float("nan"), float("inf")):
        assert nll(one, one, 0, -1, f32(1.0, bad), 2, one, one, 1, 64, 5, None) == -1 and "inv_temps[1]" in err()
    assert nll(one, one, 0, -1, ok, 4, one, one, 1, 64, 1, None) == -1 and "ncls" in err()
    assert nll(one, one, 0, -1, ok, 4, one, one, 1, 64, 128, None) == -1 and "ncls" in err()
    assert nll(one, one, 3, -1, ok, 4, one, one, 1, 64, 5, None) == -1 and "label_dtype" in err()
    assert nll(one, one, 0, -1, ok, 4, one, one, -1, 64, 5, None) == -1
    assert nll(None, one, 0, -1, ok, 4, one, one, 1, 64, 5, None) == -1 and "null pointer" in err()
    assert nll(one, one, 0, -1, ok, 4, None, one, 1, 64, 5, None) == -1 and "null pointer" in err()
    assert nll(one, one, 0, -1, ok, 4, one, None, 1, 64, 5, None) == -1 and "null pointer" in err()
    assert nll(None, None, 0, -1, ok, 32, None, None, 0, 64, 5, None) == 0  # B = 0: nothing to do, no pointer touched
    assert nll(None, None, 0, -1, ok, 1, None, None, 3, 0, 127, None) == 0  # HW = 0

    rel = lib.ig_reliability_update
    assert rel(one, one, 0, -1, 1.0, one, 1, 64, 5, 0, None) == -1 and "nbins" in err()
    assert rel(one, one, 0, -1, 1.0, one, 1, 64, 5, 65, None) == -1 and "nbins" in err()
    assert rel(one, one, 0, -1, 1.0, one, 1, 64, 65, 64, None) == -1 and "4096" in err()
    assert rel(one, one, 0, -1, 1.0, one, 1, 64, 1, 15, None) == -1 and "ncls" in err()
    assert rel(one, one, 0, -1, 1.0, one, 1, 64, 128, 15, None) == -1 and "ncls" in err()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert rel(one, one, 0, -1, bad, one, 1, 64, 5, 15, None) == -1 and "inv_temp" in err()
    assert rel(one, one, 0, -1, 1.0, None, 1, 64, 5, 15, None) == -1 and "null pointer" in err()
    assert rel(one, None, 0, -1, 1.0, one, 1, 64, 5, 15, None) == -1 and "null pointer" in err()
    assert rel(None, None, 0, -1, 1.0, None, 0, 64, 5, 15, None) == 0
    assert rel(None, None, 2, -1, 0.5, None, 4, 0, 64, 64, None) == 0
    with pytest.raises(built_lib.HipLibraryError):
        built_lib.call("ig_reliability_update", one, one, 0, -1, 1.0, one, 1, 64, 5, 0, None)


def test_generated_custom_ops_follow_the_header():
    from instageo_amd import torch_ops

    raw = torch_ops.register()
    assert "calib_nll_grid" not in raw  # its temperatures are a HOST array: ops.calib_nll_grid is the wrapper
    assert "Tensor? logits" in raw["reliability_update"] and "Tensor(a!)? hist" in raw["reliability_update"]
    assert "float inv_temp" in raw["reliability_update"] and "int nbins" in raw["reliability_update"]
