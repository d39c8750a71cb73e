"""Object metrics on the device (-m gpu): ``ig_object_pairs``, ``ig_object_match`` and ``ig_object_count`` against the host twin
(tests/objects_reference.py), the running metric, and ``test.object_metrics`` through ``mode=eval``.  Every comparison of counts is
exact equality; ratios are float64 values taken in the same way from equal integers."""
import functools
import json
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import objects_reference as OR  # noqa: E402
from instageo_amd import objects as O  # noqa: E402
from instageo_amd import ops  # noqa: E402

DEV = "cuda"
HALF = [(500, 1000)]


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the shared maps are read-only


@functools.lru_cache(maxsize=None)
def _blob_pair():
    """2 x 37 x 53 maps of 3 classes with fill pixels: the odd width makes waves straddle rows and the image seam."""
    gt = np.stack([OR.blobs(37, 53, 3, 1), OR.blobs(37, 53, 3, 2)])
    pred = np.stack([OR.blobs(37, 53, 3, 3), OR.blobs(37, 53, 3, 4)])
    gt.setflags(write=False), pred.setflags(write=False)
    return gt, pred


@functools.lru_cache(maxsize=None)
def _twin_table(name, connectivity=4):
    gt, pred = MAPS[name]()
    t = OR.ref_table(gt, pred, connectivity)
    t.setflags(write=False)
    return t


def _noise_pair(side, ncls, seed):
    return OR.noise(side, side, ncls, seed)[None], OR.noise(side, side, ncls, 100 + seed)[None]


MAPS = {"blobs": _blob_pair, "noise40": functools.partial(_noise_pair, 40, 2, 1), "noise64": functools.partial(_noise_pair, 64, 3, 1)}


def _entries(table, HW):
    """Rows of an overlap table -> the sorted (key, count) entries the device table must hold."""
    return sorted((((int(r[0]) * HW + int(r[1])) << 32) | int(r[2]), int(r[3])) for r in table)


def _tally(gt, pred, capacity, connectivity=4):
    """``ops.object_pairs`` on buffers full of leftovers -> (sorted (key, count) entries, status, labels (2, n, H, W))."""
    labels = torch.stack((ops.ccl_label(_dev(gt), connectivity), ops.ccl_label(_dev(pred), connectivity)))
    keys = torch.full((capacity,), 0x0000000500000007, dtype=torch.int64, device=DEV)  # what an earlier launch could have left
    counts = torch.full((capacity,), 9, dtype=torch.int32, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.object_pairs(labels[0], labels[1], keys, counts, status)
    k, c = keys.cpu().numpy(), counts.cpu().numpy()
    used = k != ops.OBJECT_EMPTY
    assert (c[~used] == 0).all()
    return sorted(zip(k[used].tolist(), c[used].tolist())), int(status.item()), (keys, counts, labels)


# ---- the table ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [4, 8])
def test_overlap_table_equals_the_twin(connectivity):
    gt, pred = _blob_pair()
    want = _twin_table("blobs", connectivity)
    assert len(want) > 50 and (gt == -1).any() and (pred == -1).any()
    got = O.overlap_table(_dev(gt), _dev(pred), connectivity)
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want)
    one = O.overlap_table(_dev(gt[1]), _dev(pred[1]), connectivity).cpu().numpy()  # (H, W) maps: image 0
    second = want[want[:, 0] == 1].copy()
    second[:, 0] = 0
    assert np.array_equal(one, second)


def test_identical_images_give_separate_rows_per_image():
    gt, pred = _blob_pair()
    got = O.overlap_table(_dev(np.stack([gt[0], gt[0], gt[0]])), _dev(np.stack([pred[0], pred[0], pred[0]]))).cpu().numpy()
    first = _twin_table("blobs")
    first = first[first[:, 0] == 0]
    assert len(got) == 3 * len(first)
    for i in range(3):
        rows = got[got[:, 0] == i]
        assert np.array_equal(rows[:, 1:], first[:, 1:]), i


def test_a_uniform_pair_is_one_row():
    """Every lane of every wave holds the same key: one insert per wave, 4096 pixels in one entry."""
    a = np.full((64, 64), 2, np.int8)
    assert O.overlap_table(_dev(a), _dev(a)).cpu().tolist() == [[0, 0, 0, 4096, 4096, 4096, 2, 2]]
    entries, status, _ = _tally(a[None], a[None], 1024)
    assert entries == [(0, 4096)] and status == 0


def test_single_pixel_columns_give_every_lane_its_own_key():
    """Columns of alternating classes in both maps (period 2 against period 3): every column is a region of both maps, so the 64 lanes
    of a wave hold 64 different keys: more than the merge rounds take."""
    x = np.arange(64)
    gt, pred = np.tile((x % 2).astype(np.int8), (16, 1))[None], np.tile((x % 3).astype(np.int8), (16, 1))[None]
    want = OR.ref_table(gt, pred)
    assert len(want) == 64 and (want[:, 3] == 16).all()
    assert np.array_equal(O.overlap_table(_dev(gt), _dev(pred)).cpu().numpy(), want)


def test_probing_under_load():
    """Independent single-pixel noise on 40 x 40: the twin's distinct pairs fill the smallest table to more than half."""
    gt, pred = MAPS["noise40"]()
    want = _twin_table("noise40")
    assert 600 <= len(want) <= 1000
    entries, status, _ = _tally(gt, pred, 1024)
    assert status == 0 and entries == _entries(want, 1600)


def test_overflow_is_a_status_and_overlap_table_retries(monkeypatch):
    gt, pred = MAPS["noise64"]()
    want = _twin_table("noise64")
    assert len(want) > 1024
    entries, status, _ = _tally(gt, pred, 1024)
    assert status == 1 and len(entries) <= 1024  # it returned, and says that the table is not valid
    assert np.array_equal(O.overlap_table(_dev(gt), _dev(pred)).cpu().numpy(), want)
    sizes = []
    pairs = ops.object_pairs
    monkeypatch.setattr(O, "_capacity_for", lambda pixels: 1024)  # start too small: 1024 and 2048 overflow, 4096 holds the table
    monkeypatch.setattr(ops, "object_pairs", lambda g, p, keys, counts, status: (sizes.append(keys.numel()), pairs(g, p, keys, counts, status))[1])
    assert np.array_equal(O.overlap_table(_dev(gt), _dev(pred)).cpu().numpy(), want)
    assert sizes == [1024, 2048, 4096]


def test_the_table_does_not_depend_on_the_capacity_or_the_run():
    gt, pred = _blob_pair()
    want = _entries(_twin_table("blobs"), 37 * 53)
    raw = {}
    for capacity in (1024, 4096, 65536):
        entries, status, (keys, counts, _) = _tally(gt, pred, capacity)
        assert status == 0 and entries == want, capacity
        raw[capacity] = keys.cpu().numpy(), counts.cpu().numpy()
    again = _tally(gt, pred, 4096)
    assert again[0] == want
    # two runs at one capacity: the same set of entries, hence the same bits once the slots (which mean nothing) are sorted away
    assert np.array_equal(np.sort(again[2][0].cpu().numpy()), np.sort(raw[4096][0]))
    assert np.array_equal(np.sort(again[2][1].cpu().numpy()), np.sort(raw[4096][1]))


# ---- matching -------------------------------------------------------------------------------------------------------------------------
def _device_counts(gt, pred, ratios, ncls, connectivity=4, min_area=1, capacity=1024):
    """The four tables through the raw ops, as lists of Python integers."""
    _, status, (keys, counts, labels) = _tally(gt, pred, capacity, connectivity)
    assert status == 0
    g, p = _dev(gt), _dev(pred)
    areas = ops.region_area(labels[0]), ops.region_area(labels[1])
    tp = torch.zeros(len(ratios), ncls, dtype=torch.int64, device=DEV)
    iou_q, n_gt, n_pred = torch.zeros_like(tp), torch.zeros(ncls, dtype=torch.int64, device=DEV), torch.zeros(ncls, dtype=torch.int64, device=DEV)
    ops.object_match(keys, counts, g, p, areas[0], areas[1], ratios, tp, iou_q, ncls, min_area)
    ops.object_count(g, labels[0], areas[0], n_gt, ncls, min_area)
    ops.object_count(p, labels[1], areas[1], n_pred, ncls, min_area)
    return tp.tolist(), iou_q.tolist(), n_gt.tolist(), n_pred.tolist()


def _maps(*rows):
    return np.array(rows, dtype=np.int8)[None]


Q35 = 10066330  # 3/5 in units of 2^-24, rounded half up
EDGE_CASES = {
    # intersection 2 of union 4: IoU = 1/2 exactly, no match at t = 0.5
    "half": (_maps([1, 1, 1, -1, -1]), _maps([-1, 1, 1, 1, -1]), HALF, 1, ([[0, 0, 0]], [[0, 0, 0]], [0, 1, 0], [0, 1, 0])),
    # intersection 3 of union 5: a match at 0.5, none at 0.6
    "three_fifths": (_maps([2, 2, 2, 2, -1, -1]), _maps([-1, 2, 2, 2, 2, -1]), [(500, 1000), (600, 1000)], 1,
                     ([[0, 0, 1], [0, 0, 0]], [[0, 0, Q35], [0, 0, 0]], [0, 0, 1], [0, 0, 1])),
    # equal shapes of different classes are never a match
    "other_class": (_maps([1, 1, -1, 2, 2]), _maps([2, 2, -1, 1, 1]), HALF, 1, ([[0, 0, 0]], [[0, 0, 0]], [0, 1, 1], [0, 1, 1])),
    # min_area at the smaller area (3 against 4): both count and match; one above it: the smaller region is no object, so no match
    "min_area_at": (_maps([1, 1, 1, 1, -1]), _maps([1, 1, 1, -1, -1]), HALF, 3, ([[0, 1, 0]], [[0, 3 << 22, 0]], [0, 1, 0], [0, 1, 0])),
    "min_area_above": (_maps([1, 1, 1, 1, -1]), _maps([1, 1, 1, -1, -1]), HALF, 4, ([[0, 0, 0]], [[0, 0, 0]], [0, 1, 0], [0, 0, 0])),
    # a gt region under two pred halves (2 of 5 each): no match, 1 FN and 2 FP
    "two_halves": (_maps([1, 1, 1, 1, 1]), _maps([1, 1, -1, 1, 1]), HALF, 1, ([[0, 0, 0]], [[0, 0, 0]], [0, 1, 0], [0, 2, 0])),
}


@pytest.mark.parametrize("name", sorted(EDGE_CASES))
def test_matching_at_the_edge(name):
    gt, pred, ratios, min_area, by_hand = EDGE_CASES[name]
    twin = OR.ref_counts(gt, pred, ratios, 3, min_area=min_area)
    assert twin == by_hand
    assert _device_counts(gt, pred, ratios, 3, min_area=min_area) == twin
    tp, _, n_gt, n_pred = twin
    if name == "two_halves":
        assert (n_gt[1] - tp[0][1], n_pred[1] - tp[0][1]) == (1, 2)  # FN, FP


@pytest.mark.parametrize("connectivity,min_area", [(4, 1), (8, 1), (4, 6)])
def test_counts_equal_the_twin_on_blobs_against_their_noisy_copy(connectivity, min_area):
    """A prediction that is the ground truth with 4 % of its pixels redrawn: large regions that match well beside many tiny ones."""
    gt, _ = _blob_pair()
    rng = np.random.default_rng(11)
    pred = np.where(rng.random(gt.shape) < 0.04, rng.integers(0, 3, gt.shape), gt).astype(np.int8)
    ratios = [(500, 1000), (750, 1000), (900, 1000), (999, 1000)]
    twin = OR.ref_counts(gt, pred, ratios, 3, connectivity, min_area)
    assert sum(twin[0][0]) > sum(twin[0][3]) > 0  # matches at 0.5 that are none at 0.999, and some that still are
    assert _device_counts(gt, pred, ratios, 3, connectivity, min_area, capacity=4096) == twin
    assert _device_counts(gt, pred, ratios, 5, connectivity, min_area, capacity=65536) == tuple(
        [r + [0, 0] for r in t] if isinstance(t[0], list) else t + [0, 0] for t in twin)  # more classes than occur, another capacity


# ---- the running metric ---------------------------------------------------------------------------------------------------------------
def _batches():
    """Three batches of 2 x 48 x 48: int64 labels of 5 classes with ignored (-1) and out-of-range pixels, predictions that follow them."""
    rng = np.random.default_rng(5)
    out = []
    for b in range(3):
        lab = np.stack([OR.blobs(48, 48, 5, 20 + 2 * b, fill_frac=0.03), OR.blobs(48, 48, 5, 21 + 2 * b, fill_frac=0.03)]).astype(np.int64)
        lab[0, 3, 3], lab[1, 4, 4] = 5, -7  # no class of the map: invalid like the ignored ones
        pred = np.where(rng.random(lab.shape) < 0.05, rng.integers(0, 5, lab.shape), np.where(lab < 0, 0, lab) % 5).astype(np.int64)
        out.append((lab, pred))
    return out


def test_running_metric_equals_the_twin_over_the_concatenation(monkeypatch):
    batches = _batches()
    ts, ncls = [0.5, 0.75], 5
    total = None
    for lab, pred in batches:
        gt, pm = OR.ref_maps(lab, pred, ncls, -1)
        assert (gt == -1).sum() > 50 and np.array_equal(pm == -1, gt == -1)
        c = OR.ref_counts(gt, pm, O.threshold_ratios(ts), ncls)
        total = c if total is None else OR.add_counts(total, c)
    assert min(total[0][1]) >= 0 and sum(total[0][1]) > 10 and sum(total[2]) > sum(total[0][0])

    def feed(m, order):
        for b in order:
            lab, pred = batches[b]
            if b == 0:  # logits whose argmax is the prediction
                logits = torch.randn(2, ncls, 48, 48, generator=torch.Generator().manual_seed(b)) * 0.1
                logits.scatter_add_(1, torch.from_numpy(pred)[:, None], torch.full((2, 1, 48, 48), 4.0))
                assert np.array_equal(logits.argmax(1).numpy(), pred)
                m.update(logits.to(DEV), _dev(lab))
            elif b == 1:  # int maps
                m.update(_dev(pred.astype(np.int32)), _dev(lab))
            else:
                m.update(_dev(pred.astype(np.int8)), _dev(lab))
        return tuple(c.tolist() for c in m.device_counts())

    m = O.RunningObjectMetrics(ncls, ts, ignore_index=-1)
    assert feed(m, (0, 1, 2)) == total
    for r, w in zip(m.compute(), OR.ref_metrics(*total)):
        assert str(r["f1_per_class"]) == str(w["f1"]) and str(r["pq_per_class"]) == str(w["pq"]) and str(r["sq_per_class"]) == str(w["sq"])
        assert r["pq"] == pytest.approx(w["mean"]["pq"], rel=1e-15) and r["f1"] == pytest.approx(w["mean"]["f1"], rel=1e-15)
    sub = m.compute(classes=[1, 3])
    assert sub[0]["pq"] == pytest.approx(OR.ref_metrics(*total, classes=[1, 3])[0]["mean"]["pq"], rel=1e-15)
    m.reset()
    assert all(int(c.sum()) == 0 for c in m.device_counts()) and math.isnan(m.compute()[0]["pq"])
    assert feed(m, (2, 0, 1)) == total  # after a reset, in another order, on the buffer of before
    # groups of one image (the table's bound reached by a batch), then an image beyond the bound: the tally that looks at the status
    monkeypatch.setattr(O, "AUTO_CAPACITY", 8192)
    assert feed(O.RunningObjectMetrics(ncls, ts, ignore_index=-1), (1, 2, 0)) == total
    monkeypatch.setattr(O, "AUTO_CAPACITY", 2048)
    assert feed(O.RunningObjectMetrics(ncls, ts, ignore_index=-1), (2, 1, 0)) == total


# ---- through the product --------------------------------------------------------------------------------------------------------------
COMMON = ["model.model_name=prithvi_eo_tiny", "model.load_pretrained_weights=False", "train.ignore_index=-1", "model.num_classes=3",
          "train.class_weights=[1,2,1]"]
THRESHOLDS = [0.5, 0.75]
MARKS = ("_obj_", "_PQ_", "_SQ_", "_RQ_")


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    from instageo_amd.config import load_config
    from instageo_amd.factory import create_model

    d = tmp_path_factory.mktemp("objects")
    mod = create_model(load_config("config", ["mode=train"] + COMMON), device=DEV)
    ck = str(d / "ck.ckpt")
    torch.save({"state_dict": mod.checkpoint_state_dict()}, ck)
    return ck


def _same(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))


def _smooth_labels(y, ncls):
    """Labels with regions: the synthetic ones are per-pixel noise.  Blobs, with the dataset's ignore_index pixels kept."""
    blob = torch.from_numpy(OR.blobs(y.shape[-2], y.shape[-1], ncls, 7, fill_frac=0, cell=28).astype(np.float32)).to(y.device)
    return torch.where(y == -1, y, blob.expand_as(y))


def _test_batches(cfg, labels_of):
    """The (inputs, labels) batches evaluate() feeds the model, one per chip."""
    from instageo_amd import run
    from instageo_amd.dataloader import process_test

    ds = run.create_dataset(cfg["test_filepath"], cfg, "test", DEV)
    d, t = cfg["dataloader"], cfg["test"]
    for i in range(len(ds)):
        x, y = process_test(*ds.raw(i), d["mean"], d["std"], d["temporal_dim"], t["img_size"], t["crop_size"], t["stride"], ds.mult, DEV)
        yield x, labels_of(y)


def _reference_log(model, cfg, labels_of, classes=None):
    """The object keys of the test epoch: ``object_metrics_from_counts`` of the twin's tables on the model's own argmax maps."""
    ncls = cfg["model"]["num_classes"]
    total = None
    for x, y in _test_batches(cfg, labels_of):
        with torch.no_grad():
            logits = model.net.engine.forward(x, training=False, save=False)
        gt, pred = OR.ref_maps(y.cpu().numpy(), ops.argmax_i8(logits).cpu().numpy(), ncls, -1)
        c = OR.ref_counts(gt, pred, O.threshold_ratios(THRESHOLDS), ncls)
        total = c if total is None else OR.add_counts(total, c)
    out = {}
    for r in O.object_metrics_from_counts(*total, THRESHOLDS, classes):
        t = "%g" % r["threshold"]
        for key, name in (("obj_F1", "f1"), ("obj_P", "precision"), ("obj_R", "recall"), ("PQ", "pq"), ("SQ", "sq"), ("RQ", "rq")):
            out[f"test_{key}_t{t}"] = r[name]
        for c in range(ncls):
            out[f"test_obj_F1_t{t}_{c}"], out[f"test_PQ_t{t}_{c}"] = r["f1_per_class"][c], r["pq_per_class"][c]
    return out, total


def test_mode_eval_logs_the_twins_values_and_nothing_without_the_switch(checkpoint, tmp_path, capsys, monkeypatch):
    """``run.main`` (the fused_eval_step path): with the switch the object keys equal those of the twin's tables; without it no such key
    exists, nothing is built, and every other value is that of the run with it.  Then ``test_step`` (the Lightning-style path) on labels
    with regions and ignore_index pixels."""
    from instageo_amd import run

    seen = {}
    evaluate = run.evaluate

    def spy(cfg, model, rank, world):
        res = evaluate(cfg, model, rank, world)
        seen["res"], seen["model"], seen["cfg"] = res, model, cfg
        return res

    monkeypatch.setattr(run, "evaluate", spy)
    printed = lambda: [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1]["Evaluation results"]  # noqa: E731
    args = ["--output-dir", str(tmp_path / "out"), "mode=eval", "test_filepath=synthetic:5", f"checkpoint_path={checkpoint}"] + COMMON
    assert run.main(args) == 0
    plain, printed_plain = seen["res"], printed()
    assert seen["model"].test_objects is None and not [k for k in plain if any(m in k for m in MARKS)]
    assert run.main(args + ["test.object_metrics=true", f"test.object_iou_thresholds={THRESHOLDS}"]) == 0
    res, model, cfg, printed_on = seen["res"], seen["model"], seen["cfg"], printed()
    want, total = _reference_log(model, cfg, lambda y: y)
    assert sum(total[2]) > 0 and set(want) == {k for k in res if any(m in k for m in MARKS)} and len(want) == 2 * (6 + 2 * 3)
    for k, v in want.items():
        assert _same(res[k], v), (k, res[k], v)
    assert set(res) - set(want) == set(plain) and all(_same(res[k], plain[k]) for k in plain)  # every other logged value keeps its bits
    assert set(printed_on) == set(res) and all(_same(printed_on[k], printed_plain[k]) for k in printed_plain)
    # test_step on labels with real regions (the synthetic ones are per-pixel noise), the means over a subset of the classes
    model.set_object_metrics(THRESHOLDS, classes=[0, 2])
    model.logged.clear()
    ign = 0
    for x, y in _test_batches(cfg, lambda y: _smooth_labels(y, 3)):
        ign += int((y == -1).sum())
        model.test_step((x, y))
    model.on_test_epoch_end()
    want, total = _reference_log(model, cfg, lambda y: _smooth_labels(y, 3), classes=[0, 2])
    assert ign > 0 and sum(total[2]) > 0
    for k, v in want.items():
        assert _same(model.logged[k], v), (k, model.logged[k], v)
    assert all(int(c.sum()) == 0 for c in model.test_objects.device_counts())  # reset at the end of the epoch
    model.set_object_metrics(None)  # off again
    assert model.test_objects is None and model.object_classes is None
    # the regression module refuses the switch
    from instageo_amd.regression import PrithviRegressionModule

    with pytest.raises(ValueError, match="regression"):
        PrithviRegressionModule.set_object_metrics(model, [0.5])
    PrithviRegressionModule.set_object_metrics(model, None)
