"""Boundary-quality metrics on the device (-m gpu): ``ig_boundary_dist2`` and ``ig_boundary_update`` against the host reference
(tests/boundary_reference.py), and ``test.boundary_metrics`` through ``mode=eval``.  Every check is exact equality: of integers, or of
float64 ratios taken in the same way from equal integers."""
import functools
import json
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import boundary_reference as BR  # noqa: E402
from instageo_amd import boundary as B  # noqa: E402
from instageo_amd import ops  # noqa: E402

DEV = "cuda"
FAR = BR.FAR
SHAPES = [(1, 1), (1, 300), (300, 1), (64, 64), (37, 53), (130, 257)]  # kernel tiles are 64 wide and 16 high (test_gpu_regions.py)
PAIR_SHAPES = [(37, 53), (130, 257)]


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the shared patterns are read-only


@functools.lru_cache(maxsize=None)
def _patterns(H, W):
    """The maps of one shape, stacked (8, H, W): blobs with 2 and 13 classes and 2 % fill, one class, all fill, checkerboard, stripes
    both ways, rings.  Read-only (shared between tests)."""
    maps = [BR.blobs(H, W, 2, 10 + H), BR.blobs(H, W, 13, 20 + W), np.full((H, W), 5, np.int8), np.full((H, W), -1, np.int8),
            BR.checkerboard(H, W), BR.stripes(H, W), BR.stripes(H, W, vertical=True), BR.rings(H, W)]
    out = np.stack(maps)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _ref_dist2(H, W, rmax):
    out = BR.ref_dist2(_patterns(H, W), rmax)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("rmax", [1, 3, 32])
@pytest.mark.parametrize("H,W", SHAPES)
def test_dist2_equals_the_reference_on_every_shape_and_pattern(H, W, rmax):
    """All patterns of a shape in one call: n = 8 different maps per launch."""
    cms = _patterns(H, W)
    got = B.boundary_distance(_dev(cms), rmax)
    assert got.dtype == torch.int32 and got.shape == cms.shape
    got, ref = got.cpu().numpy(), _ref_dist2(H, W, rmax)
    for i in range(len(cms)):
        assert np.array_equal(got[i], ref[i]), (i, int((got[i] != ref[i]).sum()))
    assert (got[2] == FAR).all() and (got[3] == -1).all()  # one class: no boundary anywhere, the image border is none; all fill
    if H > 1 or W > 1:
        assert (got[4] == 1).all()  # checkerboard: every pixel touches the other class


@pytest.mark.parametrize("rmax,q,hits", [
    (5, (16, 64), {(13, 60): 25, (11, 64): 25, (16, 59): 25, (12, 61): 25, (21, 64): 25, (16, 69): 25, (19, 68): 25}),  # 3-4-5 across the corner
    (4, (16, 64), {(13, 60): FAR, (11, 64): FAR, (16, 59): FAR, (12, 64): 16, (16, 60): 16, (14, 61): 13}),  # the same pixels at rmax + 1
    (32, (48, 128), {(16, 128): 1024, (48, 96): 1024, (15, 128): FAR, (48, 95): FAR, (80, 128): 1024, (48, 160): 1024, (81, 128): FAR,
                     (26, 105): 1013, (25, 105): FAR}),  # axially across two tile rows / half a tile column; 22^2 + 23^2 = 1013, 23^2 + 23^2 > 1024
])  # fmt: skip
def test_a_single_source_exactly_rmax_away_across_tile_corners(rmax, q, hits):
    """One pixel of class 1 at the first pixel of a tile in a map of class 0: the pixels at distance exactly rmax (axially and, for the
    3-4-5 triangle, diagonally) lie in the neighbouring tiles and report rmax^2; one step further is FAR."""
    cm = np.zeros((100, 200), np.int8)
    cm[q] = 1
    got = ops.boundary_dist2(_dev(cm), rmax).cpu().numpy()
    assert np.array_equal(got, BR.ref_dist2(cm, rmax))
    for (y, x), want in hits.items():
        assert got[y, x] == want, (y, x, int(got[y, x]), want)
    assert got[q] == 1 and ((got == FAR) | (got <= rmax * rmax)).all()


@pytest.mark.parametrize("fill", [-1, 0])
def test_the_nearest_other_class_behind_a_strip_of_fill(fill):
    cm = np.full((40, 150), 1, np.int8)
    cm[:, 70:] = 2
    cm[:, 62:70] = fill  # the strip straddles the tile border at column 64
    cm[5:9, 10:14] = fill
    got = ops.boundary_dist2(_dev(cm), 12, fill).cpu().numpy()
    assert np.array_equal(got, BR.ref_dist2(cm, 12, fill))
    assert got[20, 61] == 81 and got[20, 70] == 81 and got[20, 58] == 144 and got[20, 57] == FAR and (got[:, 62:70] == -1).all()
    out = torch.full((2, 40, 150), 7, dtype=torch.int32, device=DEV)
    assert ops.boundary_dist2(_dev(cm), 12, fill, out=out[1]) is not None  # ``out`` is written in place, its neighbour is not touched
    assert np.array_equal(out[1].cpu().numpy(), got) and (out[0] == 7).all()
    assert ops.boundary_dist2(torch.empty((0, 40, 150), dtype=torch.int8, device=DEV), 12, fill).shape == (0, 40, 150)


# ---- counts -----------------------------------------------------------------------------------------------------------------------------
KS = {1: [4], 8: [1, 2, 4, 5, 8, 9, 10, 16]}  # squared distances; rmax = 4


@functools.lru_cache(maxsize=None)
def _pairs(H, W, ncls):
    """(3, H, W) gt and pred maps: independent blobs, pred == gt, pred = gt moved by one pixel.  Class ids are spread over [0, ncls)
    and, for ncls < 127, two pixels hold classes outside [0, ncls), which do not count."""
    nb = min(ncls, 13)
    scale = (ncls - 1) // (nb - 1)  # spreads the ids over [0, ncls)
    gt = (BR.blobs(H, W, nb, 31 + ncls) * scale).astype(np.int8)
    other = (BR.blobs(H, W, nb, 32 + ncls) * scale).astype(np.int8)
    gt[gt < 0], other[other < 0] = -1, -1
    if ncls < 127:
        gt[3 % H, 5 % W], other[7 % H, 11 % W] = ncls, 126
    gts = np.stack([gt, gt, gt])
    preds = np.stack([other, gt, BR.shifted(gt)])
    gts.setflags(write=False), preds.setflags(write=False)
    return gts, preds


@functools.lru_cache(maxsize=None)
def _ref_counts(H, W, ncls, K):
    gts, preds = _pairs(H, W, ncls)
    return [BR.ref_counts(g, p, KS[K], ncls, rmax=4) for g, p in zip(gts, preds)]


def _counts(gt, pred, thresholds, ncls, rmax=4, fill=-1, tables=None):
    K = len(thresholds)
    band, tri = tables or (torch.zeros(K, ncls, 3, dtype=torch.int64, device=DEV), torch.zeros(K, ncls, ncls, dtype=torch.int64, device=DEV))
    gt, pred = _dev(gt), _dev(pred)
    ops.boundary_update(gt, pred, ops.boundary_dist2(gt, rmax, fill), ops.boundary_dist2(pred, rmax, fill), thresholds, band, tri, ncls, fill)
    return band, tri


@pytest.mark.parametrize("ncls", [2, 13, 127])  # K * ncls * (ncls + 3) <= 8192 cells are aggregated in LDS: 127 classes take global atomics
@pytest.mark.parametrize("K", [1, 8])
@pytest.mark.parametrize("H,W", PAIR_SHAPES)
def test_counts_equal_the_reference(H, W, K, ncls):
    gts, preds = _pairs(H, W, ncls)
    for i, (rb, rt) in enumerate(_ref_counts(H, W, ncls, K)):
        band, tri = _counts(gts[i], preds[i], KS[K], ncls)
        assert np.array_equal(band.cpu().numpy(), rb) and np.array_equal(tri.cpu().numpy(), rt), i
        assert rb[-1, :, 0].sum() > 0 and rt[-1].sum() == rb[-1, :, 0].sum()
        if i == 1:  # pred == gt: both bands are the intersection, the trimap is diagonal
            assert (rb[..., 0] == rb[..., 2]).all() and (rb[..., 1] == rb[..., 2]).all()
            assert all(np.array_equal(t, np.diag(np.diag(t))) for t in rt)
    # the three pairs in one launch add up, and a second call accumulates
    band, tri = _counts(gts, preds, KS[K], ncls)
    want_b, want_t = sum(r[0] for r in _ref_counts(H, W, ncls, K)), sum(r[1] for r in _ref_counts(H, W, ncls, K))
    assert np.array_equal(band.cpu().numpy(), want_b) and np.array_equal(tri.cpu().numpy(), want_t)
    _counts(gts, preds, KS[K], ncls, tables=(band, tri))
    assert np.array_equal(band.cpu().numpy(), 2 * want_b) and np.array_equal(tri.cpu().numpy(), 2 * want_t)


@pytest.mark.parametrize("ncls", [13, 127])
def test_one_call_with_eight_maps_equals_eight_calls(ncls):
    H, W = 37, 53
    gts = np.stack([BR.blobs(H, W, 13, 40 + i) for i in range(8)])
    preds = np.stack([BR.blobs(H, W, 13, 60 + i) for i in range(8)])
    band, tri = _counts(gts, preds, KS[8], ncls)
    tables = (torch.zeros_like(band), torch.zeros_like(tri))
    for g, p in zip(gts, preds):
        _counts(g, p, KS[8], ncls, tables=tables)
    assert torch.equal(band, tables[0]) and torch.equal(tri, tables[1]) and int(tri.sum()) > 0


def _d4(a, k):
    """The eight symmetries of the pixel grid on the last two axes: bit 2 transposes, bit 1 flips the rows, bit 0 the columns."""
    if k & 4:
        a = np.swapaxes(a, -1, -2)
    if k & 2:
        a = a[..., ::-1, :]
    if k & 1:
        a = a[..., ::-1]
    return np.ascontiguousarray(a)


@pytest.mark.parametrize("H,W", PAIR_SHAPES)
def test_counts_do_not_change_under_the_eight_d4_transforms(H, W):
    """Distances are Euclidean and the image border is no boundary: flips and transposes move pixels between tiles and halos, the
    counts stay."""
    gts, preds = _pairs(H, W, 13)
    base = _counts(gts[0], preds[0], KS[8], 13)
    assert np.array_equal(base[0].cpu().numpy(), _ref_counts(H, W, 13, 8)[0][0])
    for k in range(1, 8):
        band, tri = _counts(_d4(gts[0], k), _d4(preds[0], k), KS[8], 13)
        assert torch.equal(band, base[0]) and torch.equal(tri, base[1]), k
        d2 = ops.boundary_dist2(_dev(_d4(gts[0], k)), 4).cpu().numpy()
        assert np.array_equal(d2, _d4(BR.ref_dist2(gts[0], 4), k)), k


def test_running_metrics_build_the_maps_of_the_loss_predicate():
    """Logits or class maps, labels of any dtype with ignore_index and out-of-range values: the device maps equal the reference's."""
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(2, 5, 37, 53, generator=g)
    labels = torch.from_numpy(np.stack([BR.blobs(37, 53, 5, 1), BR.blobs(37, 53, 5, 2)]).astype(np.float32))
    labels[0, 0, :7], labels[1, 5, 5], labels[1, 6, 6] = -1.0, 5.0, -3.0
    m = B.RunningBoundaryMetrics(5, [1, 2.5], ignore_index=-1)
    preds = logits.argmax(1).numpy()
    gt, pred = BR.ref_maps(labels.numpy(), preds, 5, -1)
    for lab in (labels, labels.long(), labels.int()):
        dg, dp = m.class_maps(logits.to(DEV), lab.to(DEV))
        assert dg.dtype == torch.int8 and np.array_equal(dg.cpu().numpy(), gt) and np.array_equal(dp.cpu().numpy(), pred)
        m.update(logits.to(DEV), lab.to(DEV))
    m.update(torch.from_numpy(preds).to(DEV), labels.to(DEV))  # predictions instead of logits
    rb, rt = BR.ref_counts(gt, pred, [1, 6], 5, rmax=3)
    band, tri = m.device_counts()
    assert m.rmax == 3 and m.thresholds == [1, 6]
    assert np.array_equal(band.cpu().numpy(), 4 * rb) and np.array_equal(tri.cpu().numpy(), 4 * rt)
    recs = m.compute()
    for r, (per, biou, acc, iou) in zip(recs, BR.ref_metrics(4 * rb, 4 * rt)):
        assert str(r["biou_per_class"]) == str(per) and r["biou"] == biou and r["trimap_acc"] == acc and r["trimap_iou"] == iou
    m.reset()
    assert int(band.sum()) == 0 and int(tri.sum()) == 0 and math.isnan(m.compute()[0]["biou"])


# ---- through the product --------------------------------------------------------------------------------------------------------------
COMMON = ["model.model_name=prithvi_eo_tiny", "model.load_pretrained_weights=False", "train.ignore_index=-1", "model.num_classes=3",
          "train.class_weights=[1,2,1]"]
DISTANCES = [1, 2.5, 4]


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    from instageo_amd.config import load_config
    from instageo_amd.factory import create_model

    d = tmp_path_factory.mktemp("boundary")
    mod = create_model(load_config("config", ["mode=train"] + COMMON), device=DEV)
    ck = str(d / "ck.ckpt")
    torch.save({"state_dict": mod.checkpoint_state_dict()}, ck)
    return ck


def _eval_cfg(checkpoint, extra=()):
    from instageo_amd.config import load_config

    return load_config("config", COMMON + ["mode=eval", "test_filepath=synthetic:3", f"checkpoint_path={checkpoint}"] + list(extra))


def _smooth_labels(y, ncls):
    """Labels with outlines: the synthetic ones are per-pixel noise.  Blobs, with the dataset's ignore_index pixels kept."""
    blob = torch.from_numpy(BR.blobs(y.shape[-2], y.shape[-1], ncls, 7, fill_frac=0).astype(np.float32)).to(y.device)
    return torch.where(y == -1, y, blob.expand_as(y))


def _same(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))


def _test_batches(cfg, labels_of):
    """The (inputs, labels) batches evaluate() feeds the model, one per chip."""
    from instageo_amd import run
    from instageo_amd.dataloader import process_test

    ds = run.create_dataset(cfg["test_filepath"], cfg, "test", DEV)
    d, t = cfg["dataloader"], cfg["test"]
    for i in range(len(ds)):
        x, y = process_test(*ds.raw(i), d["mean"], d["std"], d["temporal_dim"], t["img_size"], t["crop_size"], t["stride"], ds.mult, DEV)
        yield x, labels_of(y)


def _reference_log(model, cfg, labels_of):
    """The boundary keys of the test epoch from the model's own argmax maps, by the host reference."""
    ncls = cfg["model"]["num_classes"]
    ts = [int(math.floor(v * v)) for v in DISTANCES]
    band, tri = 0, 0
    for x, y in _test_batches(cfg, labels_of):
        with torch.no_grad():
            logits = model.net.engine.forward(x, training=False, save=False)
        gt, pred = BR.ref_maps(y.cpu().numpy(), ops.argmax_i8(logits).cpu().numpy(), ncls, -1)
        b, tr = BR.ref_counts(gt, pred, ts, ncls, rmax=4)
        band, tri = band + b, tri + tr
    out = {}
    for dist, (per, biou, acc, iou) in zip(DISTANCES, BR.ref_metrics(band, tri)):
        tag = "%g" % dist
        out[f"test_bIoU_d{tag}"], out[f"test_trimap_Acc_d{tag}"], out[f"test_trimap_IoU_d{tag}"] = biou, acc, iou
        out.update({f"test_bIoU_d{tag}_{c}": v for c, v in enumerate(per)})
    return out, band


def test_mode_eval_logs_the_reference_values_and_nothing_without_the_switch(checkpoint, tmp_path, capsys, monkeypatch):
    """``run.main`` (the fused_eval_step path): with the switch the boundary keys equal the reference's, bit for bit before the
    printout rounds them; without it no such key exists and every other value is that of the run with it.  Then ``test_step`` (the
    Lightning-style path) on labels with outlines and ignore_index pixels."""
    from instageo_amd import run

    seen = {}
    evaluate = run.evaluate

    def spy(cfg, model, rank, world):
        res = evaluate(cfg, model, rank, world)
        seen["res"], seen["model"], seen["cfg"] = res, model, cfg
        return res

    monkeypatch.setattr(run, "evaluate", spy)
    printed = lambda: [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1]["Evaluation results"]  # noqa: E731
    args = ["--output-dir", str(tmp_path / "out"), "mode=eval", "test_filepath=synthetic:3", f"checkpoint_path={checkpoint}"] + COMMON
    assert run.main(args) == 0
    plain, printed_plain = seen["res"], printed()
    assert seen["model"].test_boundary is None and not [k for k in plain if "bIoU" in k or "trimap" in k]
    assert run.main(args + ["test.boundary_metrics=true", f"test.boundary_distances={DISTANCES}"]) == 0
    res, model, cfg, printed_on = seen["res"], seen["model"], seen["cfg"], printed()
    want, band = _reference_log(model, cfg, lambda y: y)
    assert band[0, :, 0].sum() > 0 and set(want) == {k for k in res if "bIoU" in k or "trimap" in k} and len(want) == 3 * (3 + 3)
    for k, v in want.items():
        assert _same(res[k], v), (k, res[k], v)
    assert set(res) - set(want) == set(plain) and all(_same(res[k], plain[k]) for k in plain)  # every other logged value keeps its bits
    assert set(printed_on) == set(res) and all(_same(printed_on[k], printed_plain[k]) for k in printed_plain)
    # test_step on labels with real outlines (the synthetic ones are per-pixel noise) and the dataset's ignore_index pixels
    model.logged.clear()
    ign = 0
    for x, y in _test_batches(cfg, lambda y: _smooth_labels(y, 3)):
        ign += int((y == -1).sum())
        model.test_step((x, y))
    model.on_test_epoch_end()
    want, band = _reference_log(model, cfg, lambda y: _smooth_labels(y, 3))
    assert ign > 0 and band[0, :, 0].sum() > 0
    for k, v in want.items():
        assert _same(model.logged[k], v), (k, model.logged[k], v)
    assert int(model.test_boundary.device_counts()[0].sum()) == 0  # reset at the end of the epoch
    # the regression module refuses the switch
    from instageo_amd.regression import PrithviRegressionModule

    with pytest.raises(ValueError, match="regression"):
        PrithviRegressionModule.set_boundary_metrics(model, [1, 2])
    PrithviRegressionModule.set_boundary_metrics(model, None)
