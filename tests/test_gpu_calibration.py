"""Post-hoc calibration on the device (-m gpu): ``ig_calib_nll_grid`` and ``ig_reliability_update`` against the float64 formulas of
tests/calibration_reference.py, recovery of a planted temperature, and the product paths (mode=calibrate, calibrated tile inference,
``test.calibration_metrics``).

Accuracy bar of the loss sums (the rule of test_gpu_value_ranges.py), on each nll[k]: |kernel - f64| <= max(4 x |the same formula in
fp32 torch on the device - f64|, 2^-22 x |f64|).  The kernel's partials stay in double: there is no fixed-point quantum to add.
Every check prints its error, the bar, the fp32 error and err / bar (``-s`` shows the table)."""
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import calibration_reference as CR  # noqa: E402
from instageo_amd import calibration as C  # noqa: E402
from instageo_amd import dataloader as DL  # noqa: E402
from instageo_amd import ops, tiff  # noqa: E402

DEV = "cuda"
IGN = -1
FLOOR_F32 = 2.0**-22
SHAPES = [(3, 2, 8, 12), (2, 13, 7, 9), (1, 16, 4, 4), (1, 127, 5, 3), (8, 5, 224, 224)]
NBINS = [15, 10, 64, 15, 15]  # per shape
FAMILIES = ["randn3", "confident", "offset"]
LABEL_DTYPES = [torch.int64, torch.int32, torch.float32]
KS = [1, 7, 32]
ids = lambda s: "x".join(map(str, s))  # noqa: E731

_CASES = {}


def make_case(shape, family):
    """(logits f32 as the kernel sees them, logits f64 of the un-offset problem, labels int64) on the device, built once per case.
    Labels: uniform over the classes, ~10 % ignore_index, out-of-range values (K and -5)."""
    key = (shape, family)
    if key in _CASES:
        return _CASES[key]
    B, K, H, W = shape
    g = torch.Generator().manual_seed(1000 * K + B)
    z = torch.randn(B, K, H, W, generator=g) * (30.0 if family == "confident" else 3.0)
    z = (z * 1024).round() / 1024  # multiples of 2^-10: z + 1000 is exact in fp32, so the offset case is the same problem
    z64 = z.double()
    if family == "offset":
        z = z + 1000.0
        assert torch.equal(z.double() - 1000.0, z64)
    lab = torch.randint(0, K, (B, H, W), generator=g)
    flat = lab.view(-1)
    n = flat.numel()
    perm = torch.randperm(n, generator=g)
    flat[perm[: n // 10]] = IGN
    flat[perm[n // 10]] = K
    flat[perm[n // 10 + 1]] = -5
    _CASES[key] = (z.to(DEV), z64.to(DEV), lab.to(DEV))
    return _CASES[key]


def betas_of(K):
    """K inverse temperatures over [1/8, 8], log-spaced, as the float32 values the entry point receives."""
    b = np.exp(np.linspace(math.log(0.125), math.log(8.0), K)) if K > 1 else np.array([0.75])
    return [float(v) for v in b.astype(np.float32)]


def nll_torch(z, lab, betas):
    """sum over valid pixels of logsumexp_c(beta z_c) - beta z_y in the dtype of ``z``, on the device -> (K,) and #valid."""
    K = z.shape[1]
    valid = (lab != IGN) & (lab >= 0) & (lab < K)
    yc = lab.clamp(0, K - 1)[:, None]
    out = []
    for b in betas:
        a = z * torch.tensor(b, dtype=z.dtype, device=z.device)
        out.append(((torch.logsumexp(a, 1) - a.gather(1, yc)[:, 0]) * valid.to(z.dtype)).sum())
    return torch.stack(out), int(valid.sum().item())


def run_nll(z, lab, betas, nll=None, count=None):
    nll = torch.zeros(len(betas), dtype=torch.float64, device=DEV) if nll is None else nll
    count = torch.zeros(1, dtype=torch.int64, device=DEV) if count is None else count
    ops.calib_nll_grid(z, lab, IGN, betas, nll, count)
    return nll, count


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_nll_grid_matches_float64(shape, family):
    z, z64, lab = make_case(shape, family)
    worst = 0.0
    for i, K in enumerate(KS):
        betas = betas_of(K)
        ref, n_ref = nll_torch(z64, lab, betas)
        t32, _ = nll_torch(z64.float(), lab, betas)  # the fp32 yardstick works on the un-offset problem
        ldt = LABEL_DTYPES[(i + len(family)) % 3]
        got, count = run_nll(z, lab.to(ldt), betas)
        assert count.item() == n_ref > 0
        assert torch.isfinite(got).all() and torch.isfinite(ref).all()
        for k in range(K):
            err = abs(got[k].item() - ref[k].item())
            terr = abs(t32[k].double().item() - ref[k].item())
            bar = max(4.0 * terr, FLOOR_F32 * abs(ref[k].item()))
            worst = max(worst, err / bar)
            print(f"CAL {family} {ids(shape)} K{K} k{k} {str(ldt)[6:]}: err {err:.3e} bar {bar:.3e} torch32 {terr:.3e} f64 {ref[k].item():.6e} "
                  f"ratio {err / bar:.3g}")
            assert err <= bar, f"{family} K={K} k={k}: err {err:.3e} > bar {bar:.3e} (fp32 torch {terr:.3e})"
        # the float64 host formulas of the reference helper say the same
        host, n_host = CR.nll_sums(z64.cpu().numpy(), lab.cpu().numpy(), IGN, betas)
        assert n_host == n_ref and np.allclose(host, ref.cpu().numpy(), rtol=1e-12)
    print(f"CAL worst ratio {family} {ids(shape)}: {worst:.3g}")


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[4]], ids=ids)
def test_nll_grid_repeats_bit_for_bit_and_accumulates(shape):
    z, _, lab = make_case(shape, "randn3")
    betas = betas_of(32)
    a, ca = run_nll(z, lab, betas)
    b, cb = run_nll(z, lab, betas)
    assert torch.equal(a, b) and torch.equal(ca, cb)
    for ldt in LABEL_DTYPES[1:]:
        c, cc = run_nll(z, lab.to(ldt), betas)
        assert torch.equal(a, c) and torch.equal(ca, cc)
    # the engine's deterministic-reduction mode does not enter: registered or not, the bits are the same
    grad = torch.zeros(1024, dtype=torch.float32, device=DEV)
    try:
        ops.set_deterministic(grad)
        assert ops.deterministic()
        on, _ = run_nll(z, lab, betas)
    finally:
        ops.set_deterministic(None)
    assert not ops.deterministic()
    off, _ = run_nll(z, lab, betas)
    assert torch.equal(on, a) and torch.equal(off, a)
    # a second call on the same outputs: the count doubles exactly, the sums are a + a (one rounding of an exact doubling: none)
    run_nll(z, lab, betas, a, ca)
    assert ca.item() == 2 * cb.item() and torch.equal(a, b + b)
    # the first K' columns do not depend on how many temperatures ride along
    few, _ = run_nll(z, lab, betas[:7])
    assert torch.equal(few, b[:7])


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[1]], ids=ids)
def test_all_ignored_batch_leaves_the_outputs_untouched(shape):
    B, K, H, W = shape
    z, _, lab = make_case(shape, "randn3")
    for labels in (torch.full_like(lab, IGN), torch.full_like(lab, K + 3), torch.full_like(lab, -5).float()):
        nll = torch.full((7,), 1.25, dtype=torch.float64, device=DEV)
        count = torch.full((1,), 11, dtype=torch.int64, device=DEV)
        run_nll(z, labels, betas_of(7), nll, count)
        hist = torch.full((K, 3, 15), 3, dtype=torch.int64, device=DEV)
        ops.reliability_update(z, labels, IGN, 0.5, hist)
        torch.cuda.synchronize()
        assert count.item() == 11 and bool((nll == 1.25).all()) and bool((hist == 3).all())
    empty = torch.zeros(0, K, H, W, device=DEV)
    run_nll(empty, lab[:0], betas_of(7), nll, count)
    ops.reliability_update(empty, lab[:0], IGN, 0.5, hist)
    assert count.item() == 11 and bool((hist == 3).all())


# ---- reliability histograms -------------------------------------------------------------------------------------------------------
EDGE = 2.0**-20


def _slack(ref, K, nbins):
    """Pixels whose cell the fp32 kernel may legitimately choose differently: float64 confidence within 2^-20 of an INTERIOR bin edge
    (conf = 1 belongs to the top bin and is no edge), or top-two float64 probabilities closer than 2^-20.  Each such pixel may sit in, or
    be missing from, the cells {its class, the runner-up} x {its bin and the two neighbours}: -> (slack per cell [K][nbins], #risky)."""
    conf, b, pred, second = ref["conf"], ref["bin"], ref["pred"], ref["second"]
    pos = conf * nbins
    near_edge = (np.abs(pos - np.round(pos)) < EDGE * nbins) & (np.round(pos) >= 1) & (np.round(pos) <= nbins - 1)
    risky = near_edge | (ref["gap"] < EDGE)
    slack = np.zeros((K, nbins), dtype=np.int64)
    for i in np.nonzero(risky)[0]:
        for c in {int(pred[i]), int(second[i])}:
            for bb in range(max(0, b[i] - 1), min(nbins, b[i] + 2)):
                slack[c, bb] += 1
    return slack, int(risky.sum())


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_reliability_histograms_match_float64(shape, family):
    B, K, H, W = shape
    nbins = NBINS[SHAPES.index(shape)]
    z, z64, lab = make_case(shape, family)
    for i, beta in enumerate([1.0, 0.4, 2.5]):
        beta = float(np.float32(beta))
        ldt = LABEL_DTYPES[i]
        hist = torch.zeros(K, 3, nbins, dtype=torch.int64, device=DEV)
        ops.reliability_update(z, lab.to(ldt), IGN, beta, hist)
        again = torch.zeros_like(hist)
        ops.reliability_update(z, lab.to(ldt), IGN, beta, again)
        assert torch.equal(hist, again)  # integers: bit-identical on repetition
        ops.reliability_update(z, lab.to(ldt), IGN, beta, again)
        assert torch.equal(again, 2 * hist)  # accumulated
        got = hist.cpu().numpy()
        ref = CR.reliability(z64.cpu().numpy(), lab.cpu().numpy(), IGN, beta, nbins)
        n_valid = len(ref["y"])
        assert got[:, 0].sum() == n_valid  # every valid pixel lands in exactly one cell
        assert (got[:, 1] <= got[:, 0]).all() and (got >= 0).all()
        slack, risky = _slack(ref, K, nbins)
        assert risky < 0.01 * n_valid, f"{risky} of {n_valid} pixels sit on a bin edge or a tie: change the seed"
        d_cnt = np.abs(got[:, 0] - ref["hist"][:, 0])
        d_hit = np.abs(got[:, 1] - ref["hist"][:, 1])
        assert (d_cnt <= slack).all() and (d_hit <= slack).all(), (d_cnt.max(), d_hit.max(), slack.max())
        # confidence sums: fixed point of 2^-24 rounded per pixel (2^-25) + the fp32 bar on conf; a pixel that changes cells carries <= 1
        p32 = torch.softmax(z64.float() * beta, 1).amax(1).double()
        p64 = torch.softmax(z64 * beta, 1).amax(1)
        conf_bar = max(4.0 * (p32 - p64).abs().max().item(), FLOOR_F32)
        n_cell = np.maximum(got[:, 0], ref["hist"][:, 0])
        err = np.abs(got[:, 2] / C.CONF_SCALE - ref["conf_sum"])
        bar = n_cell * (2.0**-25 + conf_bar) + slack
        ratio = float((err / np.maximum(bar, 1e-300))[n_cell > 0].max())
        print(f"REL {family} {ids(shape)} beta {beta:g} {str(ldt)[6:]}: cells moved {int(d_cnt.sum())} risky {risky}/{n_valid} conf err "
              f"{err.max():.3e} conf bar/pixel {2.0**-25 + conf_bar:.3e} worst ratio {ratio:.3g}")
        assert (err <= bar).all()
        # and the ratios the host takes from them
        r_got, r_ref = C.reliability_from_histogram(got), C.reliability_from_histogram(ref["hist"])
        if risky == 0:
            assert abs(r_got["ece"] - r_ref["ece"]) <= 2.0**-25 + conf_bar


# ---- a planted temperature, end to end on the device --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(4, 5, 32, 32, 2.5), (2, 13, 24, 24, 0.5), (4, 2, 32, 32, 3.0)], ids=ids)
def test_planted_temperature_is_recovered(case):
    B, K, H, W, T0 = case
    rng = np.random.default_rng(100 * K + B)
    z_cal = 2.0 * rng.standard_normal((B, K, H, W))
    p = CR.softmax_rows(np.moveaxis(z_cal.reshape(B, K, -1), 1, 2).reshape(-1, K))
    lab = (p.cumsum(1) < rng.random((p.shape[0], 1))).sum(1).clip(0, K - 1).reshape(B, H, W)
    logits = np.round(T0 * z_cal * 1024) / 1024
    z, y = torch.from_numpy(logits).float().to(DEV), torch.from_numpy(lab).to(DEV)
    assert torch.equal(z.double().cpu(), torch.from_numpy(logits))
    fit = C.TemperatureFitter(points=32, passes=2)
    while not fit.done:
        for i in range(B):  # streamed: one chip per update
            fit.update(z[i : i + 1], y[i : i + 1], IGN)
        fit.end_pass()
    res = fit.result()
    ln_ref = CR.best_ln_temperature(logits, lab, IGN)
    step = 2.0 * math.log(64.0) / 31 / 31  # the fine grid spans two coarse steps with 32 points: 8.66e-3
    print(f"FIT {ids(case)}: T {res['temperature']:.6f} golden section {math.exp(ln_ref):.6f} |d ln T| {abs(res['ln_temperature'] - ln_ref):.3e} "
          f"step {step:.3e} nll {res['nll_before']:.5f} -> {res['nll_after']:.5f}")
    assert abs(res["ln_temperature"] - ln_ref) <= step
    assert res["vertex"] and not res["at_bound"] and res["n_valid"] == B * H * W and res["nll_after"] < res["nll_before"]
    assert abs(math.log(res["temperature"] / T0)) < 0.25  # and that is the planted one, up to the sampling noise of >= 1152 labels
    rel = [C.RunningReliability(K, 15, t, IGN) for t in (1.0, res["temperature"])]
    for r in rel:
        r.update(z, y)
    before, after = (r.compute() for r in rel)
    print(f"FIT {ids(case)}: ece {before['ece']:.4f} -> {after['ece']:.4f}, mce {before['mce']:.4f} -> {after['mce']:.4f}")
    assert after["ece"] <= before["ece"] / 2
    nll = C.RunningNLL([1.0, res["temperature"]], IGN)
    nll.update(z, y)
    nb, na = nll.compute()
    assert abs(nb - res["nll_before"]) <= 1e-12 * nb and abs(na - res["nll_after"]) < 1e-5


# ---- through the product --------------------------------------------------------------------------------------------------------
TAGS = {33550: (12, (30.0, 30.0, 0.0)), 33922: (12, (0.0, 0.0, 0.0, 399960.0, 4500000.0, 0.0)),
        34735: (3, (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 32613))}
COMMON = ["model.model_name=prithvi_eo_tiny", "model.load_pretrained_weights=False", "train.batch_size=64", "train.ignore_index=-1",
          "model.num_classes=3", "train.class_weights=[1,2,1]"]


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    from instageo_amd.config import load_config
    from instageo_amd.factory import create_model

    d = tmp_path_factory.mktemp("calib")
    mod = create_model(load_config("config", ["mode=train"] + COMMON), device=DEV)
    ck = str(d / "ck.ckpt")
    torch.save({"state_dict": mod.checkpoint_state_dict()}, ck)
    return ck


def _json_lines(capsys):
    return [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]


def test_mode_calibrate_writes_calibration_json(tmp_path, checkpoint, capsys):
    from instageo_amd import run

    out = str(tmp_path / "out")
    common = COMMON + [f"root_dir={tmp_path}", f"checkpoint_path={checkpoint}"]
    assert run.main(["--output-dir", out, "mode=calibrate", "valid_filepath=synthetic:3", "calibrate.nbins=10"] + common) == 0
    rec = C.read_calibration_json(os.path.join(out, "calibration.json"))
    assert _json_lines(capsys)[-1] == rec
    assert set(C.CALIBRATION_KEYS) <= set(rec)
    assert math.isfinite(rec["temperature"]) and rec["temperature"] > 0 and rec["nll_after"] <= rec["nll_before"]
    assert rec["n_valid"] > 0 and sum(rec["bins_before"]["count"]) == rec["n_valid"] == sum(rec["bins_after"]["count"])
    assert len(rec["bins_after"]["count"]) == 10 and len(rec["grids"]) == 2 and len(rec["grids"][0]["temperatures"]) == 32
    assert isinstance(rec["at_bound"], bool) and 0 <= rec["ece_after"] <= 1 and 0 <= rec["mce_before"] <= 1
    with pytest.raises(RuntimeError):
        run.main(["--output-dir", out, "mode=calibrate", "checkpoint_path=" + checkpoint] + COMMON)  # valid_filepath required
    # mode=eval: the calibration keys appear only on request
    assert run.main(["--output-dir", out, "mode=eval", "test_filepath=synthetic:2"] + common) == 0
    plain = _json_lines(capsys)[-1]["Evaluation results"]
    assert run.main(["--output-dir", out, "mode=eval", "test_filepath=synthetic:2", "test.calibration_metrics=True",
                     f"test.calibration={os.path.join(out, 'calibration.json')}"] + common) == 0
    cal = _json_lines(capsys)[-1]["Evaluation results"]
    assert set(cal) - set(plain) == {"test_nll", "test_ece", "test_mce"} and set(plain) <= set(cal)
    assert not {k for k in plain if "nll" in k or "ece" in k or "mce" in k}
    assert math.isfinite(cal["test_nll"]) and 0 <= cal["test_ece"] <= cal["test_mce"] <= 1
    for k in ("test_loss", "test_IoU", "test_Acc"):  # the loss and the confusion matrix see the raw logits
        assert cal[k] == plain[k]


def _read_rasters(pdir):
    return {n: tiff.read(str(pdir / n))[0] for n in sorted(os.listdir(pdir))}


def test_tile_inference_with_a_temperature(tmp_path, checkpoint):
    from instageo_amd import run
    from instageo_amd.config import load_config
    from instageo_amd.factory import create_model

    H, W = 300, 260
    rng = np.random.default_rng(4)
    arr = rng.integers(0, 10000, size=(6, H, W)).astype(np.int16)
    arr[:, 100:120, 200:240] = -9999
    runs = {}
    for name, extra in (("plain", []), ("t1", ["test.temperature=1.0"]), ("t2", ["test.temperature=2.0"])):
        root = tmp_path / name
        os.makedirs(root)
        tiff.write(str(root / "tile_a.tif"), arr, {"tags": TAGS, "nodata": -9999}, compress="deflate")
        assert run.main(["--output-dir", str(root / "out"), "mode=tile_inference", "test_filepath=tile_a.tif", f"checkpoint_path={checkpoint}",
                         f"root_dir={root}", "test.stride=112", "test.blend=gaussian", "test.cover_edges=true", "test.save_probabilities=true",
                         "test.save_uncertainty=true", "dataloader.constant_multiplier=0.0001"] + COMMON + extra) == 0
        runs[name] = root / "predictions"
    names = ["prediction_tile_a.tif", "probability_tile_a.tif", "uncertainty_tile_a.tif"]
    assert sorted(os.listdir(runs["plain"])) == names
    for n in names:  # T = 1 multiplies nothing: the files are the same bytes
        assert (runs["plain"] / n).read_bytes() == (runs["t1"] / n).read_bytes(), n
    # T = 2 against the blend kernels driven directly with the same logits multiplied by 0.5
    cfg = load_config("config", ["mode=tile_inference", f"checkpoint_path={checkpoint}"] + COMMON)
    model = create_model(cfg, device=DEV)
    model.net.eval()
    d = cfg["dataloader"]
    tile = torch.from_numpy(arr).to(DEV)
    tops, lefts = DL.window_grid(H, W, 224, 112, True)
    origins = DL.origins_tensor([(t, l) for t in tops for l in lefts], DEV)
    x, _ = DL.gather_windows(tile, origins, d["mean"], d["std"], 1, 224, 1e-4)
    with torch.no_grad():
        logits = model.net.engine.forward(x, training=False, save=False).clone()
    canvas = torch.zeros((4, H, W), dtype=torch.float32, device=DEV)
    ops.window_blend_accumulate(logits * 0.5, torch.tensor(tops, dtype=torch.int32, device=DEV), torch.tensor(lefts, dtype=torch.int32, device=DEV),
                                0, ops.blend_weights(224, "gaussian").to(DEV), canvas[:3], canvas[3], H, 0, (0, H))
    cmap, prob = ops.window_blend_finalize(canvas[:3], canvas[3], tile, -9999, -1, True)
    unc = torch.empty((2, H, W), dtype=torch.float32, device=DEV)
    ops.window_blend_uncertainty(canvas[:3], canvas[3], tile, -9999, out=unc)
    got = {n: torch.from_numpy(a).to(DEV) for n, a in _read_rasters(runs["t2"]).items()}
    bits = lambda t: t.contiguous().view(torch.int32)  # noqa: E731
    assert torch.equal(got[names[0]][0], cmap) and torch.equal(bits(got[names[1]]), bits(prob)) and torch.equal(bits(got[names[2]]), bits(unc))
    base = torch.from_numpy(_read_rasters(runs["plain"])[names[2]]).to(DEV)
    ok = ~torch.isnan(base[0])
    e1, e2 = base[0][ok].double().mean().item(), got[names[2]][0][ok].double().mean().item()
    print(f"TILE mean normalised entropy: T = 1 {e1:.6f}, T = 2 {e2:.6f}")
    assert e2 > e1
    # test.calibration=<json> equals test.temperature=<its value>
    cal = str(tmp_path / "calibration.json")
    C.write_calibration_json(cal, dict({k: 0.0 for k in C.CALIBRATION_KEYS}, temperature=2.0, at_bound=False, n_valid=1, grids=[],
                                       bins_before={}, bins_after={}))
    root = tmp_path / "json"
    os.makedirs(root)
    tiff.write(str(root / "tile_a.tif"), arr, {"tags": TAGS, "nodata": -9999}, compress="deflate")
    assert run.main(["--output-dir", str(root / "out"), "mode=tile_inference", "test_filepath=tile_a.tif", f"checkpoint_path={checkpoint}",
                     f"root_dir={root}", "test.stride=112", "test.blend=gaussian", "test.cover_edges=true", "test.save_probabilities=true",
                     "test.save_uncertainty=true", "dataloader.constant_multiplier=0.0001", f"test.calibration={cal}"] + COMMON) == 0
    for n in names:
        assert (root / "predictions" / n).read_bytes() == (runs["t2"] / n).read_bytes(), n


def test_predict_step_uses_the_temperature(checkpoint):
    from instageo_amd.config import load_config
    from instageo_amd.factory import create_model

    x = torch.randn(2, 6, 1, 224, 224, generator=torch.Generator().manual_seed(3)).to(DEV)
    out = {}
    for t in (None, 1.0, 2.0):
        ov = [] if t is None else [f"test.temperature={t}"]
        m = create_model(load_config("config", ["mode=eval", f"checkpoint_path={checkpoint}"] + COMMON + ov), device=DEV)
        out[t] = m.predict_step(x)
        if t == 2.0:
            with torch.no_grad():
                logits = m.net.engine.forward(x, training=False, save=False).clone()
            assert torch.equal(out[t], ops.softmax_prob(logits * 0.5, 1))
    assert torch.equal(out[None], out[1.0]) and not torch.equal(out[None], out[2.0])
