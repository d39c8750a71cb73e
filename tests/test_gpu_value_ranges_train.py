"""Value-range parity tests (-m gpu), second module: the regression head (ig_mse_loss, ig_kd_mse_loss and the nine streaming sums of
RunningRegressionMetrics), the optimizer (ig_adamw_advance, ig_adamw_step) and the dataset statistics (ig_chip_stats, ig_label_hist) on
offset, extreme and degenerate inputs.  The ``check`` helper, its table (``-s``) and its bar are those of test_gpu_value_ranges.py:

    max |kernel - f64|  <=  max(4 * max |torch fp32 - f64|, floor)

Regression sums without the log scale have an exact bar instead.  d = pred - label and e = |y - x| are single IEEE fp32 operations, which numpy
reproduces bit for bit; the product of two fp32 numbers is exact in fp64; so every term of every sum is known exactly, ``math.fsum`` gives
the correctly rounded sum, and what is left to the kernel is the order of n fp64 additions:

    |kernel sum - fsum|  <=  n * 2^-52 * sum |term_i|

the textbook bound (n - 1) u sum |term_i| (u = 2^-53) of a recursive sum in any order, doubled.  tests/test_cpu_value_range_refs.py shows that
numpy's own fp64 sums stay inside it in three orders and that fp32 products do not.  The metrics follow from the sums by the host formulas;
their bar is that bound carried through the formulas to first order, doubled (``metric_bars``).

Under the log scale log1pf / expm1f differ from torch's by ulps: the 4x rule applies, the yardstick being the kernel's formulas with torch fp32
per-element values and all products and sums in float64.  The head predicts log1p of a non-negative quantity there: labels, teacher and
de-scaled predictions of every family are folded to |.| (log1p needs more than -1).
"""
import math
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from instageo_amd import ops  # noqa: E402
from instageo_amd._lib import HipLibraryError  # noqa: E402
from instageo_amd.metrics import RunningRegressionMetrics, regression_metrics_from_sums  # noqa: E402
from instageo_amd.ops import BT  # noqa: E402
from test_gpu_exact_parity import split_ref  # noqa: E402
from test_gpu_value_ranges import DEV, FLOOR_F32, check  # noqa: E402

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "instageo-e2e-geospatial-ml_amd", "csrc")


def bits32(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------------------------
# Regression head
# ---------------------------------------------------------------------------------------------------------------------------------
REG_SHAPES = [(3, 64, 80), (1, 17, 9)]  # 15360 pixels; 153: less than one workgroup, no multiple of 4 or 64
REG_FAMILIES = ["off0", "off300", "off3000", "off30000", "tiny", "const", "wide"]
IGNORE = -100.0
EE_BIAS, EE_COEF = 0.05, 0.15
# 29 / 4: every partial sum k c and k c^2 (k <= 2^14) is an fp64 number, so Sxx - n xm^2 is exactly 0 in any summation order
CONST_LABEL = 7.25
SUM_NAMES = ("sse", "n", "Sx", "Sy", "Sxy", "Sxx", "Syy", "S|e|", "See", "#EE")  # stats[0], then msums[0..8] (stats[1] = msums[0] = n)
METRICS = ("mae", "rmse", "r2_score", "pearson_corrcoef")


def reg_seed(family, shape):
    return 1000 + 10 * REG_FAMILIES.index(family) + REG_SHAPES.index(tuple(shape))


def reg_values(family, shape, seed, positive=False):
    """fp32 CPU tensors of one family: labels x [B, H, W], predictions y = x + 0.3 noise [B, 1, H, W], a teacher x + 0.3 noise' and an existing
    gradient buffer.  About 10 % of the pixels carry the ignore value; predictions and teacher there are +inf, -inf and NaN in turn.
    ``positive`` (log scale): x, y and the teacher folded to |.|, the prediction handed over as log1p(y)."""
    B, H, W = shape
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, H, W, generator=g, dtype=torch.float64)
    u = torch.rand(B, H, W, generator=g, dtype=torch.float64)
    if family.startswith("off"):
        x = float(family[3:]) + z
    elif family == "tiny":
        x = 1e-3 * u
    elif family == "const":
        x = torch.full((B, H, W), CONST_LABEL, dtype=torch.float64)
    else:
        assert family == "wide"
        x = 10.0 ** (-3.0 + 7.0 * u)
    y = x + 0.3 * torch.randn(B, H, W, generator=g, dtype=torch.float64)
    t = x + 0.3 * torch.randn(B, H, W, generator=g, dtype=torch.float64)
    if positive:
        x, y, t = x.abs(), y.abs(), t.abs()
        y = torch.log1p(y)
    ign = torch.rand(B, H, W, generator=g) < 0.1
    bad = torch.tensor([float("inf"), float("-inf"), float("nan")], dtype=torch.float64)[torch.arange(B * H * W).reshape(B, H, W) % 3]
    lab = torch.where(ign, torch.full_like(x, IGNORE), x).float()
    pred = torch.where(ign, bad, y).float().reshape(B, 1, H, W)
    teacher = torch.where(ign, bad.flip(0), t).float().reshape(B, 1, H, W)
    dpred0 = torch.randn(B, 1, H, W, generator=g)
    return dict(pred=pred, lab=lab, teacher=teacher, dpred0=dpred0, ignored=ign)


def reg_terms(pred, lab, ignore=IGNORE, ee_bias=EE_BIAS, ee_coef=EE_COEF):
    """use_log = False, exactly as the kernel: d = pred - label and e = |y - x| in fp32, then every product in fp64 (exact).  Returns the valid
    mask, the fp32 gradient 2 d (0 on ignored pixels), the terms of each sum (float64, valid pixels only), the fp32 evaluation of the
    expected-error test and the pixels where it is ambiguous: |e - (bias + coef x)| in float64 within 2 fp32 ulps of the threshold (the
    device may contract bias + coef x to an FMA)."""
    p = pred.detach().cpu().numpy().astype(np.float32).ravel()
    lb = lab.detach().cpu().numpy().astype(np.float32).ravel()
    valid = lb != np.float32(ignore)
    with np.errstate(invalid="ignore"):
        d32 = p - lb
    grad = np.where(valid, np.float32(2.0) * d32, np.float32(0.0)).astype(np.float32)
    x32, d32 = lb[valid], d32[valid]
    e32 = np.abs(d32)
    x, y, d, e = x32.astype(np.float64), p[valid].astype(np.float64), d32.astype(np.float64), e32.astype(np.float64)
    terms = {"sse": d * d, "n": np.ones_like(x), "Sx": x, "Sy": y, "Sxy": x * y, "Sxx": x * x, "Syy": y * y, "S|e|": e, "See": e * e}
    thr32 = np.float32(ee_bias) + np.float32(ee_coef) * x32
    thr = float(np.float32(ee_bias)) + float(np.float32(ee_coef)) * x
    ambiguous = np.abs(e - thr) <= 2.0 * np.spacing(np.abs(thr32)).astype(np.float64)
    return dict(valid=valid, grad=grad, terms=terms, ee=e32 <= thr32, ambiguous=ambiguous)


def fsum_and_bound(terms):
    """Correctly rounded sum of the float64 terms and the bar n 2^-52 sum |term_i| (module docstring)."""
    t = np.asarray(terms, dtype=np.float64)
    return math.fsum(t), t.size * 2.0**-52 * math.fsum(np.abs(t))


def reference_sums(term_sets):
    """(sums, bounds) in the order of SUM_NAMES from the ``reg_terms`` results of the calls that accumulated into the same buffers."""
    sums, bounds = [], []
    for name in SUM_NAMES[:-1]:
        s, b = fsum_and_bound(np.concatenate([r["terms"][name] for r in term_sets]))
        sums.append(s), bounds.append(b)
    sums.append(float(sum(int(r["ee"].sum()) for r in term_sets))), bounds.append(float(sum(int(r["ambiguous"].sum()) for r in term_sets)))
    return sums, bounds


def metric_bars(s, b):
    """Bars of mae / rmse / r2 / pearson from the bounds ``b`` of the nine sums ``s`` ({n, Sx, Sy, Sxy, Sxx, Syy, S|e|, See, #EE}): the error
    of each sum carried through regression_metrics_from_sums to first order (n is exact), plus the fp64 roundings of the evaluation itself on
    both sides (8 u |S| on each difference S - n xm ym, 8 u |metric| at the end), the whole doubled for the higher orders."""
    n, sx, sy, sxy, sxx, syy, sae, sse, _ = s
    _, bx, by, bxy, bxx, byy, bae, bse, _ = b
    u = 2.0**-53
    out = {"mae": bae / n, "rmse": bse / (2 * n * math.sqrt(sse / n)) if sse > 0 else math.sqrt(bse / n)}
    if n >= 2:
        xm, ym = sx / n, sy / n
        varx, vary, cov = sxx - n * xm * xm, syy - n * ym * ym, sxy - n * xm * ym
        dvx = bxx + 2 * abs(xm) * bx + 8 * u * abs(sxx)
        dvy = byy + 2 * abs(ym) * by + 8 * u * abs(syy)
        dcov = bxy + abs(ym) * bx + abs(xm) * by + 8 * u * (abs(sxy) + abs(n * xm * ym))
        if varx > 0:
            out["r2_score"] = bse / varx + sse * dvx / varx**2
            if vary > 0:
                out["pearson_corrcoef"] = dcov / math.sqrt(varx * vary) + abs(cov) / math.sqrt(varx * vary) * (dvx / (2 * varx) + dvy / (2 * vary))
    ref = regression_metrics_from_sums(s)
    return {k: 2 * v + 8 * u * abs(ref[k]) for k, v in out.items()}


def reg_log_sums(pred, lab, teacher, dt, ignore=IGNORE, ee_bias=EE_BIAS, ee_coef=EE_COEF):
    """use_log = True: the kernel's formulas with the per-element values in ``dt`` on the CPU, all products and sums in float64.  Returns the
    ten sums (SUM_NAMES), the gradient 2 d (0 on ignored pixels), the distillation sum and its gradient term, and x, e per valid pixel."""
    valid = lab.reshape(-1) != ignore
    p, lb, tch = pred.reshape(-1)[valid].to(dt), lab.reshape(-1)[valid].to(dt), teacher.reshape(-1)[valid].to(dt)
    t = torch.log1p(lb)
    d = p - t
    y, x = torch.expm1(p), torch.expm1(t)
    e = (y - x).abs()
    ee = e <= torch.tensor(ee_bias, dtype=torch.float32).to(dt) + torch.tensor(ee_coef, dtype=torch.float32).to(dt) * x
    d, x, y, e = (a.double().numpy() for a in (d, x, y, e))
    sums = [math.fsum(v) for v in (d * d, np.ones_like(x), x, y, x * y, x * x, y * y, e, e * e)] + [float(ee.sum())]
    grad = torch.zeros(valid.numel(), dtype=torch.float64)
    grad[valid] = torch.from_numpy(2.0 * d)
    dk = (p - torch.log1p(tch)).double().numpy()
    kgrad = torch.zeros(valid.numel(), dtype=torch.float64)
    kgrad[valid] = torch.from_numpy(2.0 * dk)
    return dict(sums=sums, grad=grad, kd=math.fsum(dk * dk), kgrad=kgrad, x=x, e=e, valid=valid)


def check_sum(got, ref, bound, what):
    err = abs(got - ref)
    print(f"VR {what}: err {err:.3e} bar {bound:.3e} (n 2^-52 sum|term|) scale {abs(ref):.3e} ratio {err / max(bound, 1e-300):.3g}")
    assert err <= bound, f"{what}: |{got!r} - {ref!r}| = {err:.3e} > {bound:.3e}"


def check_sums_exact_bar(stats, msums, sums, bounds, what):
    """Assertions 1 and 3 of the module docstring's exact case on stats[2] / msums[9] (device tensors) against ``reference_sums``."""
    got = [stats[0].item()] + msums.cpu().tolist()
    assert stats[1].item() == sums[1] and got[1] == sums[1], f"{what}: n {stats[1].item()} / {got[1]} != {sums[1]}"
    for i, name in enumerate(SUM_NAMES):
        if name not in ("n", "#EE"):
            check_sum(got[i], sums[i], bounds[i], f"{what} {name}")
    print(f"VR {what} #EE: {got[9]:.0f} vs {sums[9]:.0f}, {bounds[9]:.0f} ambiguous pixels of {sums[1]:.0f}")
    assert got[9] == int(got[9]) and abs(got[9] - sums[9]) <= bounds[9], f"{what}: #EE {got[9]} vs {sums[9]} with {bounds[9]} ambiguous pixels"
    assert bounds[9] <= 1e-3 * sums[1], "the seed leaves more than 0.1 % of the pixels on the expected-error threshold"


def check_metrics(got, sums, bounds, what):
    """Assertion 4: the metrics of the device sums against those of the reference sums, NaN in the same places."""
    ref = regression_metrics_from_sums(sums[1:], EE_BIAS, EE_COEF, True)
    bars = metric_bars(sums[1:], bounds[1:]) if sums[1] else {}
    for k in METRICS:
        if math.isnan(ref[k]):
            assert math.isnan(got[k]), f"{what}: {k} = {got[k]} where the reference is NaN"
            continue
        err = abs(got[k] - ref[k])
        print(f"VR {what} {k}: err {err:.3e} bar {bars[k]:.3e} (sum bounds carried through) scale {abs(ref[k]):.3e} ratio {err / max(bars[k], 1e-300):.3g}")
        assert err <= bars[k], f"{what}: {k} {got[k]!r} vs {ref[k]!r}: {err:.3e} > {bars[k]:.3e}"
    if sums[1]:
        assert abs(got["ee_percentage"] - ref["ee_percentage"]) <= 100.0 * bounds[9] / sums[1] + 1e-12
    else:
        assert math.isnan(got["ee_percentage"])
    return ref


def run_mse(v, use_log, stats, met, with_grad=True):
    dl = torch.full(v["pred"].shape, 7.0, device=DEV) if with_grad else None
    ops.mse_loss(v["pred"].to(DEV), v["lab"].to(DEV), IGNORE, use_log, stats, dl, met.device_sums(DEV), met.ee_bias, met.ee_coef, True)
    return dl


@pytest.mark.parametrize("shape", REG_SHAPES)
@pytest.mark.parametrize("family", REG_FAMILIES)
def test_mse_loss_sums_value_ranges(family, shape):
    """ig_mse_loss, use_log = False: sums, gradient, expected-error count and metrics (assertions 1-4 of the exact case)."""
    v = reg_values(family, shape, reg_seed(family, shape))
    r = reg_terms(v["pred"], v["lab"])
    assert 0 < int((~r["valid"]).sum()) < r["valid"].size // 5
    stats = torch.zeros(2, dtype=torch.float64, device=DEV)
    met = RunningRegressionMetrics(EE_BIAS, EE_COEF, include_ee=True, device=DEV)
    dl = run_mse(v, False, stats, met)
    what = f"mse {family} {shape[0]}x{shape[1]}x{shape[2]}"
    sums, bounds = reference_sums([r])
    check_sums_exact_bar(stats, met.device_sums(), sums, bounds, what)
    assert torch.equal(bits32(dl).reshape(-1), torch.from_numpy(r["grad"]).view(torch.int32)), f"{what}: dpred is not 2 (pred - label) in fp32 / 0"
    ref = check_metrics(met.compute(), sums, bounds, what)
    assert math.isnan(ref["r2_score"]) == math.isnan(ref["pearson_corrcoef"]) == (family == "const")
    # the evaluation form (no gradient buffer) accumulates the same numbers
    stats2 = torch.zeros(2, dtype=torch.float64, device=DEV)
    met2 = RunningRegressionMetrics(EE_BIAS, EE_COEF, include_ee=True, device=DEV)
    run_mse(v, False, stats2, met2, with_grad=False)
    assert torch.equal(stats2, stats) and torch.equal(met2.device_sums(), met.device_sums())


def test_mse_loss_accumulates_across_batches():
    """Two calls into the same stats / msums (how the metric is used): the sums of both batches together, within the bound at their total n."""
    va = reg_values("off3000", REG_SHAPES[0], 2001)
    vb = reg_values("off300", REG_SHAPES[1], 2002)
    stats = torch.zeros(2, dtype=torch.float64, device=DEV)
    met = RunningRegressionMetrics(EE_BIAS, EE_COEF, include_ee=True, device=DEV)
    run_mse(va, False, stats, met)
    run_mse(vb, False, stats, met)
    sums, bounds = reference_sums([reg_terms(va["pred"], va["lab"]), reg_terms(vb["pred"], vb["lab"])])
    check_sums_exact_bar(stats, met.device_sums(), sums, bounds, "mse two batches")
    check_metrics(met.compute(), sums, bounds, "mse two batches")


@pytest.mark.parametrize("nvalid", [0, 1])
def test_mse_loss_degenerate_counts(nvalid):
    """Every pixel ignored (all metrics NaN, nothing accumulated) and a single valid pixel (mae / rmse defined, r2 / pearson NaN)."""
    v = reg_values("off300", REG_SHAPES[1], 2003)
    keep = torch.zeros_like(v["ignored"])
    if nvalid:
        keep.view(-1)[int((~v["ignored"]).view(-1).nonzero()[5])] = True
    v["lab"] = torch.where(keep, v["lab"], torch.full_like(v["lab"], IGNORE))
    r = reg_terms(v["pred"], v["lab"])
    assert int(r["valid"].sum()) == nvalid
    stats = torch.full((2,), 0.0, dtype=torch.float64, device=DEV)
    met = RunningRegressionMetrics(EE_BIAS, EE_COEF, include_ee=True, device=DEV)
    dl = run_mse(v, False, stats, met)
    sums, bounds = reference_sums([r])
    check_sums_exact_bar(stats, met.device_sums(), sums, bounds, f"mse {nvalid} valid")
    assert torch.equal(bits32(dl).reshape(-1), torch.from_numpy(r["grad"]).view(torch.int32))
    got = met.compute()
    check_metrics(got, sums, bounds, f"mse {nvalid} valid")
    assert math.isnan(got["r2_score"]) and math.isnan(got["pearson_corrcoef"]) and math.isnan(got["mae"]) == (nvalid == 0)


# a variance below the fp64 rounding of its own evaluation (Sxx - n xm^2 of a constant whose squares are not exact) is noise in the float64
# reference too: r2 and pearson are not compared there (the log-scaled ``const`` family; without the log scale it is exactly 0, see CONST_LABEL)
def _variance_is_resolved(s):
    n, sx, sxx = s[1], s[2], s[5]
    return n >= 2 and sxx - sx * sx / n > 2.0**-40 * sxx


@pytest.mark.parametrize("shape", REG_SHAPES)
@pytest.mark.parametrize("family", REG_FAMILIES)
def test_mse_and_kd_loss_log_scale_value_ranges(family, shape):
    """ig_mse_loss and ig_kd_mse_loss with use_log = True under the 4x rule: sums, metrics, gradients."""
    v = reg_values(family, shape, reg_seed(family, shape) + 500, positive=True)
    ref = reg_log_sums(v["pred"], v["lab"], v["teacher"], torch.float64)
    t32 = reg_log_sums(v["pred"], v["lab"], v["teacher"], torch.float32)
    stats = torch.zeros(2, dtype=torch.float64, device=DEV)
    met = RunningRegressionMetrics(EE_BIAS, EE_COEF, include_ee=True, device=DEV)
    dl = run_mse(v, True, stats, met)
    what = f"log mse {family} {shape[0]}x{shape[1]}x{shape[2]}"
    got = [stats[0].item()] + met.device_sums().cpu().tolist()
    assert stats[1].item() == ref["sums"][1] == got[1]
    one = lambda a: torch.tensor([a], dtype=torch.float64)  # noqa: E731
    for i, name in enumerate(SUM_NAMES):
        if name not in ("n", "#EE"):
            check(one(got[i]), one(ref["sums"][i]), one(t32["sums"][i]), FLOOR_F32, f"{what} {name}")
    # expected error: a pixel may change sides where the float64 |e - threshold| is within the fp32 error bar of e and x (4 x torch's
    # largest, or 2 fp32 ulps of the threshold)
    thr = float(np.float32(EE_BIAS)) + float(np.float32(EE_COEF)) * ref["x"]
    perr = 4.0 * float(np.max(np.abs(t32["e"] - ref["e"]) + EE_COEF * np.abs(t32["x"] - ref["x"])))
    near = int((np.abs(ref["e"] - thr) <= np.maximum(perr, 2.0 * np.spacing(thr.astype(np.float32)).astype(np.float64))).sum())
    print(f"VR {what} #EE: {got[9]:.0f} vs {ref['sums'][9]:.0f}, {near} pixels near the threshold")
    assert abs(got[9] - ref["sums"][9]) <= near
    gm = met.compute()
    rm, tm = (regression_metrics_from_sums(s["sums"][1:], EE_BIAS, EE_COEF, True) for s in (ref, t32))
    for k in METRICS:
        if k in ("mae", "rmse") or _variance_is_resolved(ref["sums"]):
            check(one(gm[k]), one(rm[k]), one(tm[k]), FLOOR_F32, f"{what} {k}")
    assert _variance_is_resolved(ref["sums"]) == (family != "const")
    ign = v["ignored"].reshape(-1)
    assert (dl.reshape(-1).cpu()[ign] == 0).all(), "gradient on ignored pixels"
    check(dl.reshape(-1), ref["grad"], t32["grad"], FLOOR_F32, f"{what} dpred")
    # distillation term: adds to the existing gradient, skips ignored pixels whatever the teacher holds there
    kd = torch.zeros(1, dtype=torch.float64, device=DEV)
    dp = v["dpred0"].to(DEV)
    ops.kd_mse_loss(v["pred"].to(DEV), v["teacher"].to(DEV), v["lab"].to(DEV), IGNORE, True, kd, dp)
    check(kd, one(ref["kd"]), one(t32["kd"]), FLOOR_F32, f"{what} kd sum")
    d0 = v["dpred0"].reshape(-1).double()
    check(dp.reshape(-1), d0 + ref["kgrad"], (v["dpred0"].reshape(-1) + t32["kgrad"].float()).double(), FLOOR_F32, f"{what} kd dpred")
    assert torch.equal(bits32(dp).reshape(-1)[ign], bits32(v["dpred0"]).reshape(-1)[ign]), "kd touched the gradient of ignored pixels"
    kd2 = torch.zeros(1, dtype=torch.float64, device=DEV)
    ops.kd_mse_loss(v["pred"].to(DEV), v["teacher"].to(DEV), v["lab"].to(DEV), IGNORE, True, kd2, None)
    assert torch.equal(kd2, kd), "the evaluation form (no gradient buffer) gives another sum"


@pytest.mark.parametrize("shape", REG_SHAPES)
@pytest.mark.parametrize("family", REG_FAMILIES)
def test_kd_mse_loss_value_ranges(family, shape):
    """ig_kd_mse_loss, use_log = False: the sum within the exact bar, dpred += 2 (pred - teacher) bit for bit in fp32, ignored pixels (teacher
    non-finite there) untouched, and the evaluation form."""
    v = reg_values(family, shape, reg_seed(family, shape) + 900)
    p, t, lb = (v[k].numpy().ravel() for k in ("pred", "teacher", "lab"))
    valid = lb != np.float32(IGNORE)
    assert not np.isfinite(t[~valid]).any() and np.isfinite(t[valid]).all()
    with np.errstate(invalid="ignore"):
        d32 = p - t
    want = np.where(valid, v["dpred0"].numpy().ravel() + np.float32(2.0) * d32, v["dpred0"].numpy().ravel()).astype(np.float32)
    d = d32[valid].astype(np.float64)
    s, b = fsum_and_bound(d * d)
    kd = torch.full((1,), 3.0, dtype=torch.float64, device=DEV)  # the sum is added to what the buffer holds
    dp = v["dpred0"].to(DEV)
    ops.kd_mse_loss(v["pred"].to(DEV), v["teacher"].to(DEV), v["lab"].to(DEV), IGNORE, False, kd, dp)
    what = f"kd mse {family} {shape[0]}x{shape[1]}x{shape[2]}"
    check_sum(kd.item() - 3.0, s, b + 2.0**-52 * (abs(s) + 3.0), f"{what} sum")  # + the two roundings of 3 + s and back
    assert torch.equal(bits32(dp).reshape(-1), torch.from_numpy(want).view(torch.int32)), f"{what}: dpred"
    kd2 = torch.full((1,), 3.0, dtype=torch.float64, device=DEV)
    ops.kd_mse_loss(v["pred"].to(DEV), v["teacher"].to(DEV), v["lab"].to(DEV), IGNORE, False, kd2, None)
    assert torch.equal(kd2, kd), "the evaluation form (no gradient buffer) gives another sum"


# ---------------------------------------------------------------------------------------------------------------------------------
# AdamW
# ---------------------------------------------------------------------------------------------------------------------------------
LR, B1, B2, ADAM_EPS, WD = 1e-3, 0.9, 0.999, 1e-8, 1e-2


def make_hyper(step=0, clip=None, gscale=None):
    h = torch.zeros(16)
    h[:5] = torch.tensor([LR, B1, B2, ADAM_EPS, WD])
    h[10], h[11], h[12] = float(step), 1 - B1, 1 - B2  # the host forms 1 - beta in double, as torch does
    if clip is not None:
        h[7], h[8], h[9] = clip[0], clip[1], 1.0
    if gscale is not None:
        h[13] = gscale
    return h.to(DEV)


def adamw_device(p0, g, m0, v0, steps=3, step0=0, clip=None, gscale=None, split=True):
    """``steps`` x (advance, step) on copies of the fp32 CPU state; returns (p, m, v, shadow, hyper) on the device."""
    p, m, v = p0.clone().to(DEV), m0.clone().to(DEV), v0.clone().to(DEV)
    gd = g.to(DEV)
    hyper = make_hyper(step0, clip, gscale)
    shadow = None if split is None else BT.empty((p0.numel(),), split, DEV)
    for _ in range(steps):
        ops.adamw_advance(hyper)
        ops.adamw_step(p, gd, m, v, shadow, hyper, p0.numel())
    return p, m, v, shadow, hyper


def adamw_refs(p0, g, m0, v0, steps=3, step0=0, clip=None):
    """(float64 restatement, torch.optim.AdamW(foreach=False) in fp32) from the same fp32 inputs: (p, m, v) each."""
    from oracle import prithvi_oracle as O

    p, m, v = p0.double().clone(), m0.double().clone(), v0.double().clone()
    for s in range(steps):
        O.adamw_step(p, g.double(), m, v, step0 + s + 1, lr=LR, wd=WD, b1=B1, b2=B2, eps=ADAM_EPS)
        if clip is not None:
            p.clamp_(clip[0], clip[1])
    q = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([q], lr=LR, betas=(B1, B2), eps=ADAM_EPS, weight_decay=WD, foreach=False)
    opt.state[q] = {"step": torch.tensor(float(step0)), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
    for _ in range(steps):
        q.grad = g.clone()
        opt.step()
        if clip is not None:
            q.data.clamp_(clip[0], clip[1])
    st = opt.state[q]
    assert st["step"].item() == step0 + steps
    return (p, m, v), (q.detach(), st["exp_avg"], st["exp_avg_sq"])


def check_shadow(shadow, p, what):
    hi, lo = split_ref(p.cpu())
    assert torch.equal(shadow.hi.cpu().view(torch.int16), hi.view(torch.int16)), f"{what}: shadow hi is not the bf16 of p"
    if shadow.lo is not None:
        assert torch.equal(shadow.lo.cpu().view(torch.int16), lo.view(torch.int16)), f"{what}: shadow lo is not the bf16 of p - hi"


def adamw_state(n, seed, case="span"):
    g_ = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=g_)
    m0, v0 = 0.1 * torch.randn(n, generator=g_), 0.01 * torch.rand(n, generator=g_)
    sign = torch.where(torch.rand(n, generator=g_) < 0.5, -1.0, 1.0)
    if case == "span":  # |g| log-uniform over [1e-12, 1e4], random sign
        g = sign * (10.0 ** (-12.0 + 16.0 * torch.rand(n, generator=g_, dtype=torch.float64))).float()
        m0, v0 = torch.zeros(n), torch.zeros(n)
    elif case == "zero_grad":
        g = torch.zeros(n)
    elif case == "cold":
        g, m0, v0 = torch.zeros(n), torch.zeros(n), torch.zeros(n)
    elif case == "huge":
        g = torch.randn(n, generator=g_)
        g[torch.randperm(n, generator=g_)[: n // 100]] = 1e25
        g = g * sign
    else:
        assert case == "plain"
        g = torch.randn(n, generator=g_)
    return p0, g, m0, v0


@pytest.mark.parametrize("case", ["span", "zero_grad", "cold", "huge"])
def test_adamw_value_ranges(case):
    n = 4 * 1031
    p0, g, m0, v0 = adamw_state(n, 300 + len(case), case)
    p, m, v, shadow, _ = adamw_device(p0, g, m0, v0)
    ref, t32 = adamw_refs(p0, g, m0, v0)
    check_shadow(shadow, p, f"adamw {case}")
    assert torch.isfinite(p).all() and torch.isfinite(ref[0]).all(), "p must stay finite"
    groups = {"": torch.ones(n, dtype=torch.bool)}
    if case == "huge":
        big = g.abs() > 1e20
        assert 0 < int(big.sum()) == n // 100 and torch.isinf(t32[2][big]).all()  # g * g overflows fp32 in torch too
        groups = {" |g| = 1e25": big, " others": ~big}
    elif case == "span":  # one row per decade of |g|: m and v scale with g and g^2, the largest must not hide the smallest
        dec = torch.floor(torch.log10(g.abs().double())).clamp(-12, 3).long()
        groups.update({f" |g| ~ 1e{d}": dec == d for d in range(-12, 4)})
    for name, sel in groups.items():
        for got, r, t, nm in zip((p, m, v), ref, t32, "pmv"):
            fin = torch.isfinite(t) & sel
            assert torch.equal(torch.isfinite(got.cpu())[sel], torch.isfinite(t)[sel]), f"adamw {case}{name}: {nm} finite where torch's is not, or not"
            assert int((~torch.isfinite(t)).sum()) <= n // 100  # at most the injected elements
            if nm == "p" and name.startswith(" |g| ~"):
                continue  # p has one scale: checked once, over all elements
            if fin.any():
                check(got.cpu()[fin], r[fin], t[fin], FLOOR_F32, f"adamw {case}{name} {nm}")
    if case == "cold":
        assert torch.equal(m.cpu(), torch.zeros(n)) and torch.equal(v.cpu(), torch.zeros(n))


@pytest.mark.parametrize("step0", [9, 999, 99999])
def test_adamw_late_steps(step0):
    """ig_adamw_advance at late steps: the bias corrections within 1 fp32 ulp of the float64 values (1 - beta^step with the double betas, as
    torch forms them), then one step against the reference at that step number."""
    hyper = make_hyper(step0)
    ops.adamw_advance(hyper)
    h = hyper.cpu().double()
    step = step0 + 1
    assert h[10].item() == step
    for i, want in ((5, 1.0 - B1**step), (6, math.sqrt(1.0 - B2**step))):
        w32 = np.float32(want)
        ulps = (h[i].item() - float(w32)) / float(np.spacing(w32))
        print(f"VR adamw advance step {step} hyper[{i}]: {h[i].item()!r} vs {float(w32)!r}: {ulps:+.0f} fp32 ulps")
        assert abs(ulps) <= 1.0, f"hyper[{i}] at step {step}: {ulps:+.0f} ulps from fp32({want!r})"
    n = 4 * 1031
    p0, g, m0, v0 = adamw_state(n, 320, "plain")
    p, m, v, shadow, _ = adamw_device(p0, g, m0, v0, steps=1, step0=step0)
    ref, t32 = adamw_refs(p0, g, m0, v0, steps=1, step0=step0)
    for got, r, t, nm in zip((p, m, v), ref, t32, "pmv"):
        check(got, r, t, FLOOR_F32, f"adamw step {step} {nm}")
    check_shadow(shadow, p, f"adamw step {step}")


def test_adamw_gradient_scale():
    """hyper[13] multiplies the gradient: 0.125 (a power of two) equals a run on g / 8 bit for bit; 0 means 1."""
    n = 4 * 1031
    p0, g, m0, v0 = adamw_state(n, 330, "plain")
    scaled = adamw_device(p0, g, m0, v0, gscale=0.125)
    pre = adamw_device(p0, g * 0.125, m0, v0)
    zero = adamw_device(p0, g, m0, v0, gscale=0.0)
    one = adamw_device(p0, g, m0, v0, gscale=1.0)
    for a, b, what in ((scaled, pre, "scale 0.125 vs g / 8"), (zero, one, "scale 0 vs 1")):
        for x, y, nm in zip(a[:3], b[:3], "pmv"):
            assert torch.equal(bits32(x), bits32(y)), f"adamw {what}: {nm} differs"
        assert torch.equal(a[3].hi, b[3].hi) and torch.equal(a[3].lo, b[3].lo), f"adamw {what}: shadow differs"
    assert not torch.equal(scaled[0], one[0])
    ref, t32 = adamw_refs(p0, g * 0.125, m0, v0)
    for got, r, t, nm in zip(scaled[:3], ref, t32, "pmv"):
        check(got, r, t, FLOOR_F32, f"adamw gradient scale {nm}")


@pytest.mark.parametrize("split", [False, True])
def test_adamw_clip_with_shadow(split):
    n = 4 * 1031
    p0, g, m0, v0 = adamw_state(n, 340, "plain")
    clip = (-0.75, 0.5)
    p, m, v, shadow, _ = adamw_device(p0, g, m0, v0, clip=clip, split=split)
    ref, t32 = adamw_refs(p0, g, m0, v0, clip=clip)
    assert p.min().item() >= clip[0] and p.max().item() <= clip[1]
    assert int((p == clip[0]).sum()) > n // 20 and int((p == clip[1]).sum()) > n // 20 and int(((p > clip[0]) & (p < clip[1])).sum()) > n // 4
    check_shadow(shadow, p, "adamw clip")  # the split of the CLIPPED value
    for got, r, t, nm in zip((p, m, v), ref, t32, "pmv"):
        check(got, r, t, FLOOR_F32, f"adamw clip {nm}")


def adamw_one_pass_float4s():
    """What one pass of adamw_kernel's grid-stride loop covers, in float4s: the grid cap of ig_adamw_step times the block size, both read
    from elementwise.hip."""
    with open(os.path.join(CSRC, "elementwise.hip")) as f:
        src = f.read()
    tpb = int(re.search(r"constexpr int TPB = (\d+);", src).group(1))
    cap = int(re.search(r"adamw_kernel, dim3\(grid_for\(n / 4, TPB, (\d+)\)\)", src).group(1))
    return cap * tpb


@pytest.mark.parametrize("n", ["one_pass_plus_300", 4, 4 * 257])
def test_adamw_lengths(n):
    """A length whose float4 count exceeds one pass of the grid-stride loop by 300 (the loop body runs twice for 300 threads, once for the
    others), one float4, and one float4 more than a workgroup."""
    cap4 = adamw_one_pass_float4s()
    if n == "one_pass_plus_300":
        n = 4 * (cap4 + 300)
    p0, g, m0, v0 = adamw_state(n, 350, "plain")
    p, m, v, shadow, _ = adamw_device(p0, g, m0, v0)
    ref, t32 = adamw_refs(p0, g, m0, v0)
    tails = [("", slice(None))] + ([(" second pass", slice(4 * cap4, None))] if n > 4 * cap4 else [])
    for name, sl in tails:
        for got, r, t, nm in zip((p, m, v), ref, t32, "pmv"):
            check(got[sl], r[sl], t[sl], FLOOR_F32, f"adamw n={n}{name} {nm}")
    check_shadow(shadow, p, f"adamw n={n}")


def test_adamw_length_must_be_a_multiple_of_4():
    p0, g, m0, v0 = (t.to(DEV) for t in adamw_state(8, 360, "plain"))
    hyper = make_hyper(1)
    for n in (6, 7, 1):
        with pytest.raises(HipLibraryError):
            ops.adamw_step(p0, g, m0, v0, None, hyper, n)


@pytest.mark.parametrize("split", [False, True])
def test_adamw_sub_range(split):
    """The step on flat[lo:hi] with lo = 4 k, k odd (16-byte but not 64-byte aligned: how FusedAdamW._adam_range calls it): the range
    against the reference, everything outside it (p, m, v, both shadow halves) unchanged bit for bit."""
    N, lo = 4 * 1200, 4 * 37
    hi = lo + 4 * 301
    p0, g, m0, v0 = adamw_state(N, 370, "plain")
    p, m, v, gd = p0.clone().to(DEV), m0.clone().to(DEV), v0.clone().to(DEV), g.to(DEV)
    sh = BT.empty((N,), split, DEV)
    halves = [sh.hi] + ([sh.lo] if split else [])
    for h in halves:
        h.view(torch.int16).fill_(0x1234)
    hyper = make_hyper(0)
    for _ in range(3):
        ops.adamw_advance(hyper)
        ops.adamw_step(p[lo:hi], gd[lo:hi], m[lo:hi], v[lo:hi], BT(sh.hi[lo:hi], sh.lo[lo:hi] if split else None), hyper, hi - lo)
    ref, t32 = adamw_refs(p0[lo:hi], g[lo:hi], m0[lo:hi], v0[lo:hi])
    for got, r, t, nm in zip((p, m, v), ref, t32, "pmv"):
        check(got[lo:hi], r, t, FLOOR_F32, f"adamw sub-range {nm}")
    check_shadow(BT(sh.hi[lo:hi], sh.lo[lo:hi] if split else None), p[lo:hi], "adamw sub-range")
    out = torch.ones(N, dtype=torch.bool)
    out[lo:hi] = False
    for got, was, nm in zip((p, m, v), (p0, m0, v0), "pmv"):
        assert torch.equal(bits32(got)[out], bits32(was)[out]), f"adamw sub-range: {nm} changed outside [lo, hi)"
    for h in halves:
        assert (h.cpu().view(torch.int16)[out] == 0x1234).all(), "adamw sub-range: shadow written outside [lo, hi)"


# ---------------------------------------------------------------------------------------------------------------------------------
# Dataset statistics
# ---------------------------------------------------------------------------------------------------------------------------------
STAT_KINDS = ["r0", "r64", "r4096", "const"]


def chip_values(B, C, T, H, W, shift, seed):
    """(B, C, T, H, W) fp32: band c holds, in every chip, values of kind STAT_KINDS[(c + shift) % 4]: mean / std = 0, 64 or 4096 (sigma and
    the sign of the mean drawn per chip and band), or one constant per chip and band."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, C, T, H, W, generator=g, dtype=torch.float64)
    sig = 0.5 + 1.5 * torch.rand(B, C, 1, 1, 1, generator=g, dtype=torch.float64)
    sign = torch.where(torch.rand(B, C, 1, 1, 1, generator=g) < 0.5, -1.0, 1.0).double()
    x = torch.empty_like(z)
    kinds = [STAT_KINDS[(c + shift) % 4] for c in range(C)]
    for c, kind in enumerate(kinds):
        if kind == "const":
            x[:, c] = (3000.0 * sign * sig)[:, c].expand(B, T, H, W)
        else:
            x[:, c] = (sig * (z + float(kind[1:]) * sign))[:, c]
    return x.float(), kinds


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("B,C,T,H,W", [(2, 3, 1, 8, 12), (5, 6, 3, 16, 16)])
def test_chip_stats_value_ranges(B, C, T, H, W, shift):
    x, kinds = chip_values(B, C, T, H, W, shift, seed=400 + C)
    sums = torch.zeros(2 * C, dtype=torch.float64, device=DEV)
    ops.chip_stats(x.to(DEV), sums)
    xd = x.double().reshape(B, C, -1)
    x32 = x.reshape(B, C, -1)
    mean64, var64 = xd.mean(2).sum(0), xd.var(2, unbiased=False).sum(0)
    mean32, var32 = x32.mean(2).double().sum(0), x32.var(2, unbiased=False).double().sum(0)
    for c, kind in enumerate(kinds):
        what = f"chip_stats {B}x{C}x{T}x{H}x{W} band {c} ({kind})"
        check(sums[c : c + 1], mean64[c : c + 1], mean32[c : c + 1], FLOOR_F32, f"{what} mean")
        if kind == "const":
            assert sums[C + c].item() == 0.0, f"{what}: variance {sums[C + c].item()!r} of a constant band"
        else:
            check(sums[C + c : C + c + 1], var64[c : c + 1], var32[c : c + 1], FLOOR_F32, f"{what} variance")


def test_chip_stats_length_must_be_a_multiple_of_4():
    for shape in [(1, 2, 1, 3, 3), (2, 1, 3, 5, 2)]:
        with pytest.raises(HipLibraryError):
            ops.chip_stats(torch.zeros(shape, device=DEV), torch.zeros(2 * shape[1], dtype=torch.float64, device=DEV))


def label_map(lo, nbins, seed):
    """One float label map: integers of [lo, lo + nbins) among -0.0, 0.5, lo - 1, lo + nbins, NaN, +-inf, 2^31, -2^31 and 3e9 (twice each to
    seven times).  Returns (map [40, 150], expected counts [nbins + 1]: -0.0 counts as 0, everything else out of range lands in the last)."""
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(lo, lo + nbins, (6000,), generator=g).float()
    specials = [-0.0, 0.5, lo - 1.0, float(lo + nbins), float("nan"), float("inf"), float("-inf"), 2.0**31, -(2.0**31), 3e9]
    pos = torch.randperm(6000, generator=g)
    k = 0
    for i, s in enumerate(specials):
        lab[pos[k : k + 2 + i % 6]] = s
        k += 2 + i % 6
    want = np.zeros(nbins + 1, dtype=np.int64)
    a = lab.numpy().astype(np.float64)
    inr = np.isfinite(a) & (a == np.floor(a)) & (a >= lo) & (a < lo + nbins)
    np.add.at(want, (a[inr] - lo).astype(np.int64), 1)
    want[nbins] = (~inr).sum()
    assert want[nbins] == k - 2 and want[-lo] >= 2  # every special but -0.0
    return lab.reshape(40, 150), want


@pytest.mark.parametrize("nbins", [3, 4096])
def test_label_hist_edge_values(nbins):
    lo = -1
    lab, want = label_map(lo, nbins, seed=500 + nbins)
    counts = torch.zeros(nbins + 1, dtype=torch.int64, device=DEV)
    ops.label_hist(lab.to(DEV), counts, lo=lo)
    got = counts.cpu().numpy()
    print(f"VR label_hist nbins {nbins}: overflow {got[nbins]} (expected {want[nbins]}), total {got.sum()} of {lab.numel()}")
    assert got.sum() == lab.numel()
    assert np.array_equal(got, want), f"bins that differ: {np.nonzero(got != want)[0][:10]}"
    ops.label_hist(lab.to(DEV), counts, lo=lo)  # accumulates
    assert np.array_equal(counts.cpu().numpy(), 2 * want)


def test_compute_stats_rejects_non_integer_labels():
    from instageo_amd.pipeline_utils import compute_stats

    lab, _ = label_map(-1, 3, seed=503)
    data = torch.rand(1, 2, 1, 40, 150)
    with pytest.raises(ValueError):
        compute_stats([(data, lab.reshape(1, 40, 150))], device=DEV)
    clean = torch.where(torch.isfinite(lab) & (lab == lab.round()) & (lab >= -1) & (lab < 2), lab, torch.zeros_like(lab))
    mean, std, weights = compute_stats([(data, clean.reshape(1, 40, 150))], device=DEV)
    assert len(weights) == 2 and len(mean) == 2
