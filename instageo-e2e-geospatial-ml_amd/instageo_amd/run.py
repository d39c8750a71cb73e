"""Runner entry point with the reference's ``run.py`` surface (``instageo/model/run.py:60-245``).

    python -m instageo_amd.run [--config-name sen1floods11] [--config-path DIR] key=value ...

Modes ``stats | train | eval | chip_inference`` and every config key are those of the reference; ``calibrate`` (temperature fit on the
validation split -> ``calibration.json``; ``calibrate.*``, ``test.temperature`` / ``calibration`` / ``calibration_metrics``) and ``tile_inference``
(whole GeoTIFF tiles -> maps, ``test.blend`` / ``cover_edges`` / ``sigma_scale`` / ``save_probabilities`` / ``tta`` /
``save_uncertainty``) is this project's, as are the region keys of both inference modes (``test.min_region`` / ``connectivity`` /
``sieve_passes`` / ``save_regions`` / ``save_polygons`` / ``zones``) and the COG keys of ``tile_inference`` (``test.cog`` / ``cog_blocksize`` /
``overview_levels`` / ``cog_compress``); ``create_chips`` (``chips.*``: HLS tiles and a table of labelled points -> chips, label maps and
the dataset CSV the other modes read; the reference's ``instageo/data`` chip creator, :mod:`instageo_amd.chips`), ``create_s2_chips``
(``s2_chips.*``: the same from Sentinel-2 L2A band planes of several resolutions under the scene classification, the reference's
``S2PointsPipeline``, :mod:`instageo_amd.s2_chips`), ``create_raster_chips`` (``raster_chips.*``: HLS tiles
resampled onto the grids of label rasters, the reference's ``raster_chip_creator.py``, :mod:`instageo_amd.raster_chips`),
``create_s2_raster_chips`` (``s2_raster_chips.*``: Sentinel-2 band planes of several resolutions warped onto the grids of label rasters, the
reference's ``S2RasterPipeline``, :mod:`instageo_amd.s2_raster_chips`), ``clean_chips``
(``clean.*``: the reference's ``data_cleaner.py``: the no-data chip filter and label buffering / limiting, :mod:`instageo_amd.clean`),
``split_dataset`` (``split.*``: the dataset CSV cut into spatially blocked ``splits/train.csv`` / ``val.csv`` / ``test.csv`` with a leakage
audit and a guard band, the step of the reference's ``data_splitter.py``, :mod:`instageo_amd.split`) and
``create_polygon_labels`` (``polygon_labels.*``: a GeoJSON of polygons burned into the label rasters and the records table that
``create_raster_chips`` takes, :mod:`instageo_amd.polygon_labels`) build no model; neither does ``create_composite`` (``composite.*``: the
HLS scenes near each temporal step's date become one cloud-free composite scene per step, nearest clear date, median or medoid, written
under HLS-style names that ``chips.tiles`` takes with ``fmasks=None``, :mod:`instageo_amd.composite`) and ``filter_s1`` (``s1_filter.*``:
Sentinel-1 RTC band files speckle-filtered, optionally to dB, under the same names for ``s1_chips.scenes``, :mod:`instageo_amd.s1_filter`) and ``filter_s1_temporal`` (``s1_temporal.*``: the band files of a
stack of dates filtered by Quegan and Yu's multi-temporal rule, every date borrowing the others at the same pixel, under the same names,
:mod:`instageo_amd.s1_temporal`);
``create_s1_raster_chips`` (``s1_raster_chips.*``: Sentinel-1 RTC scenes stacked per date warped onto the grids of label rasters,
:mod:`instageo_amd.s1_raster_chips`) is the radar sibling of ``create_raster_chips``.  Hydra, Lightning and Neptune are replaced by :mod:`instageo_amd.config` and the explicit loop below, which logs the
same metric names and writes ``instageo_best_checkpoint.ckpt`` (``{"state_dict": ...}``) on the best
``val_IoU`` (pipeline_utils.py:347-355).  Data: ``*_filepath`` may be ``synthetic:<n>`` (on-device HLS-shaped
chips), an ``.npz`` with ``chips (N,T*C,H,W)`` and ``labels (N,H,W)``, or the reference's own CSV of chip / label GeoTIFF paths
(``InstaGeoDataset`` on the host TIFF codec), relative to ``root_dir``.  Multi-GPU: launch with ``python -m torch.distributed.run``; ranks shard the
dataset and average gradients over RCCL (:mod:`instageo_amd.distributed`).
"""
from __future__ import annotations

import argparse
import json
import os
import random
import sys
import time
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch

from . import distributed as D
from . import prep
from .config import check_required_flags, load_config
from .dataloader import (ArrayChipDataset, InstaGeoDataset, SyntheticChipDataset, eval_collate_fn, infer_collate_fn, normalize_batch,
                         process_and_augment, process_and_augment_batch, process_test)
from .factory import create_model, object_options
from .infer_utils import chip_inference
from .pipeline_utils import compute_stats

SEED = 1042  # pl.seed_everything(1042) in the reference (run.py:50)
# the dataset-preparation modes -> the module whose ``run_from_config(cfg, device)`` runs them
PREP_MODES = {"create_chips": "chips",  # HLS tiles + points -> chips, label maps and the dataset CSV
              "create_s2_chips": "s2_chips",  # Sentinel-2 band planes of several resolutions + points -> chips, label maps, the dataset CSV
              "create_raster_chips": "raster_chips",  # HLS tiles + label rasters -> chips on the labels' grids
              "create_s2_raster_chips": "s2_raster_chips",  # Sentinel-2 band planes + label rasters -> chips on the labels' grids
              "create_s1_chips": "s1_chips",  # Sentinel-1 RTC scenes stacked per date + points -> float32 chips, label maps, the dataset CSV
              "create_s1_raster_chips": "s1_raster_chips",  # Sentinel-1 RTC scenes stacked per date + label rasters -> float32 chips on the labels' grids
              "create_composite": "composite",  # the HLS scenes near each step's date -> one cloud-free composite scene per step
              "filter_s1": "s1_filter",  # Sentinel-1 RTC band files -> speckle-filtered (and dB) band files under the same names
              "filter_s1_temporal": "s1_temporal",  # the Sentinel-1 RTC band files of a stack of dates -> multi-temporally filtered band files
              "clean_chips": "clean",  # drop no-data chips, buffer / limit the label maps of a chip dataset
              "split_dataset": "split",  # a dataset CSV -> spatially blocked train / val / test CSVs with a leakage audit and a guard band
              "create_polygon_labels": "polygon_labels",  # a GeoJSON of polygons -> label rasters + records.csv
              "zonal_stats": "zonal"}  # a float raster + a GeoJSON of zones -> per-zone count, mean, std, min, max, sum as CSV


def get_device() -> str:
    """pipeline_utils.py:58-75 returns gpu/cpu; there is no CPU path here."""
    if not torch.cuda.is_available():
        raise RuntimeError("instageo_amd needs a HIP device (MI355X): no CPU fallback")
    return "gpu"


def create_dataset(spec: Optional[str], cfg: Dict[str, Any], kind: str, device: str):
    """``synthetic:<n>`` or an .npz archive -> dataset following the reference item contract."""
    d = cfg["dataloader"]
    T, mean, std = d["temporal_dim"], d["mean"], d["std"]
    mult = d.get("constant_multiplier", 1.0)
    mult = None if mult in (None, 1, 1.0) else float(mult)
    ncls, ign = cfg["model"]["num_classes"], cfg["train"]["ignore_index"]
    if spec is None or str(spec) == "None":
        raise RuntimeError(f"{kind}_filepath is required")
    if str(spec).startswith("synthetic:"):
        n = int(str(spec).split(":")[1])
        size = cfg["test"]["img_size"] if kind == "test" and cfg["mode"] == "eval" else d["img_size"]
        return SyntheticChipDataset(n, T, ncls, mean, std, im_size=size, ignore_index=ign, constant_multiplier=1e-4, seed=SEED, device=device,
                                    regression=bool(cfg.get("is_reg_task", False)))
    path = spec if os.path.isabs(str(spec)) or cfg.get("root_dir") in (None, "None") else os.path.join(cfg["root_dir"], spec)
    if str(path).endswith(".csv"):
        # the reference's own input: a CSV of chip / label GeoTIFF paths (dataloader.py:786-906) through the TIFF codec
        from functools import partial

        t = cfg["test"]
        if kind == "test" and cfg["mode"] == "eval":
            pre = partial(process_test, mean=mean, std=std, temporal_size=T, img_size=t["img_size"], crop_size=t["crop_size"],
                          stride=t["stride"], device=device)
        else:
            size = t["img_size"] if kind == "test" else d["img_size"]
            pre = partial(process_and_augment, mean=mean, std=std, temporal_size=T, im_size=size, crop=(kind != "test"),
                          augmentations=None, device=device)
        return InstaGeoDataset(path, cfg.get("root_dir") or "", pre, d.get("no_data_value", -9999), ign, d.get("replace_label"),
                               bool(d.get("reduce_to_zero", False)), 1.0 if mult is None else mult, d.get("bands"),
                               include_filenames=(kind == "test"), mean=mean, std=std, temporal_size=T, device=device)
    z = np.load(path)
    return ArrayChipDataset(z["chips"], z["labels"], mean, std, T, mult, include_filenames=(kind == "test"), device=device,
                            replace_label=d.get("replace_label"), reduce_to_zero=bool(d.get("reduce_to_zero", False)))


def shard_indices(n: int, shuffle: bool, epoch: int, rank: int, world: int, equal: bool) -> List[int]:
    """Item indices of one rank for one epoch.

    ``equal=True`` is ``torch.utils.data.DistributedSampler`` (what Lightning DDP gives the reference's train loader): the
    (shuffled) index list is padded by wrap-around to ``ceil(n / world) * world`` and rank r takes ``idx[r::world]``, so EVERY
    rank gets the same number of items and therefore the same number of optimizer steps -- a rank with one batch fewer would
    leave the others waiting in a gradient all-reduce while it has already entered the epoch-end metric all-reduce.
    ``equal=False`` is an exact contiguous partition (no duplicates; sizes differ by at most one): used for validation /
    test, whose steps contain no collective, so that the reduced metrics count every item exactly once."""
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(SEED + epoch)).tolist() if shuffle else list(range(n))
    if not equal or world == 1:
        lo, hi = D.shard_range(n, rank, world)
        return idx[lo:hi]
    if n == 0:
        return []
    total = -(-n // world) * world
    while len(idx) < total:
        idx += idx[: total - len(idx)]
    return idx[rank:total:world]


def _batches(ds, batch_size: int, shuffle: bool, epoch: int, rank: int, world: int, equal: bool = False):
    """Rank-sharded batch index lists (same shuffle seed on all ranks; see :func:`shard_indices`)."""
    idx = shard_indices(len(ds), shuffle, epoch, rank, world, equal)
    for i in range(0, len(idx), batch_size):
        yield idx[i : i + batch_size]


def _stack(ds, ids: List[int]) -> Tuple[torch.Tensor, torch.Tensor]:
    items = [ds[i] for i in ids]
    items = [it[0] if isinstance(it[0], tuple) else it for it in items]
    return torch.stack([it[0] for it in items]), torch.stack([it[1] for it in items])


def _reduce_metrics(metrics, dev, model=None, step_type: Optional[str] = None) -> None:
    """Sum the rank-local streaming state over ranks before the epoch-end hooks: the confusion matrix (or the regression
    sums), the (sum of batch losses, #batches) pair behind ``<step>_loss`` and, for the test epoch, the ROC-AUC histograms."""
    D.reduce_confusion(metrics.device_matrix(dev) if hasattr(metrics, "device_matrix") else metrics.device_sums(dev))
    if model is None or not D.dp_active():
        return
    acc = model._loss_sums.get(step_type)
    if acc is None:  # a rank whose shard was empty still has to take part in the collective
        acc = torch.zeros(2, dtype=torch.float64, device=dev)
        model._loss_sums[step_type] = acc
    D.reduce_loss_stats(acc)
    if step_type == "test" and hasattr(model, "test_auc"):
        D.reduce_confusion(model.test_auc.device_hist(dev))
        if getattr(model, "test_nll", None) is not None:  # test.calibration_metrics
            D.reduce_loss_stats(model.test_nll.device_sums(dev))
            D.reduce_confusion(model.test_nll.device_count(dev))
            D.reduce_confusion(model.test_reliability.device_hist(dev))
        if getattr(model, "test_boundary", None) is not None:  # test.boundary_metrics
            for counts in model.test_boundary.device_counts(dev):
                D.reduce_confusion(counts)
        if getattr(model, "test_objects", None) is not None:  # test.object_metrics: tp, iou_q, n_gt, n_pred
            for counts in model.test_objects.device_counts(dev):
                D.reduce_confusion(counts)


def train(cfg: Dict[str, Any], model, out_dir: str, rank: int, world: int) -> Dict[str, float]:
    dev = str(model.net.store.flat.device)
    train_ds = create_dataset(cfg["train_filepath"], cfg, "train", dev)
    valid_ds = create_dataset(cfg["valid_filepath"], cfg, "valid", dev)
    bs = cfg["train"]["batch_size"]
    opt = model.optimizer()
    sched = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(opt, T_0=10, T_mult=2, eta_min=0) if cfg["train"].get("scheduler") else None
    D.attach_data_parallel(model)
    reg = bool(cfg.get("is_reg_task", False))
    best, history = (-float("inf") if reg else -1.0), {}
    augs = cfg["dataloader"].get("augmentations") or {}
    train_augs = {k: v for k, v in augs.items() if v.get("use", False)}  # config order = order of application
    aug_rng = random.Random(SEED + 104729 * rank)  # rotate / brightness / blur / noise draws (Python's random, like the reference)
    aug_gen = torch.Generator().manual_seed(SEED + 7919 * rank)  # different crops/flips per rank, reproducible
    for epoch in range(cfg["train"]["num_epochs"]):
        model.net.train()
        for ids in _batches(train_ds, bs, True, epoch, rank, world, equal=True):
            # training items go through process_and_augment (dataloader.py:527-585): random crop to img_size + the enabled
            # flips + normalise as ONE kernel per batch on the raw chips; rotate / brightness / blur / noise (off in
            # sen1floods11.yaml) add one ig_aug_* launch each between the crop and the normalisation
            xr, yr = train_ds.raw_batch(ids)
            x, y = process_and_augment_batch(xr, yr, train_ds.mean, train_ds.std, train_ds.T, cfg["dataloader"]["img_size"], True,
                                             train_augs, train_ds.mult, aug_gen,
                                             label_no_data_value=cfg["train"].get("ignore_index", -1),  # run.py:128-129
                                             chip_no_data_value=cfg["dataloader"].get("no_data_value", -9999),
                                             max_pixel_value=cfg["dataloader"].get("max_pixel_value", 10000.0), rng=aug_rng)
            model.fused_train_step(x, y)
        _reduce_metrics(model.train_metrics, dev, model, "train")
        model.on_train_epoch_end()
        for ids in _batches(valid_ds, bs, False, epoch, rank, world):
            x, y = _stack(valid_ds, ids)
            model.fused_eval_step(x, y, "val")
        _reduce_metrics(model.val_metrics, dev, model, "val")
        model.on_validation_epoch_end()
        if sched is not None:
            sched.step()
        model.log("learning_rate", opt.param_groups[0]["lr"])
        history = {k: (float(v) if not isinstance(v, (list, tuple)) else v) for k, v in model.logged.items()}
        model.sync_master_params()  # data parallel: the fp32 masters are sharded between checkpoints (collective, every rank)
        if rank == 0:
            print(json.dumps({"epoch": epoch, **{k: round(v, 6) for k, v in history.items() if isinstance(v, float)}}))
            # ModelCheckpoint(monitor = "val_RMSE" (min) for regression else "val_IoU" (max), save_top_k=1)  (run.py:163-164)
            score = -history.get("val_RMSE", float("inf")) if reg else history.get("val_IoU", 0.0)
            if score > best:
                best = score
                torch.save({"state_dict": model.checkpoint_state_dict(), "epoch": epoch}, os.path.join(out_dir, "instageo_best_checkpoint.ckpt"))
    return history


def evaluate(cfg: Dict[str, Any], model, rank: int, world: int) -> Dict[str, float]:
    dev = str(model.net.store.flat.device)
    test_ds = create_dataset(cfg["test_filepath"], cfg, "test", dev)
    d, t = cfg["dataloader"], cfg["test"]
    model.net.eval()
    lo, hi = D.shard_range(len(test_ds), rank, world)
    for i in range(lo, hi):
        raw_x, raw_y = test_ds.raw(i) if hasattr(test_ds, "raw") else (test_ds.chips[i], test_ds.labels[i])
        mult = getattr(test_ds, "mult", None)  # the constant multiplier applies in every mode (dataloader.py:707-750)
        x, y = process_test(raw_x, raw_y, d["mean"], d["std"], d["temporal_dim"], t["img_size"], t["crop_size"], t["stride"], mult, dev)
        model.fused_eval_step(x, y, "test")
    _reduce_metrics(model.test_metrics, dev, model, "test")
    model.on_test_epoch_end()
    return {k: float(v) for k, v in model.logged.items() if k.startswith("test_") and not isinstance(v, (list, tuple))}


def calibrate(cfg: Dict[str, Any], model, out_dir: str, rank: int, world: int) -> Optional[Dict[str, Any]]:
    """mode=calibrate: fit one softmax temperature on the validation split and measure calibration before and after.

    The split is walked exactly as :func:`evaluate` walks the test set (``process_test`` windows, eval mode, rank sharding), once per
    pass of the fit -- logits are never stored, ``ig_calib_nll_grid`` evaluates a batch's loss at the whole temperature grid while
    the logits are on the device -- and once more for the loss and the reliability histograms at T = 1 and at the fitted T.  Rank 0
    writes ``<out_dir>/calibration.json`` and returns the record."""
    from .calibration import RunningNLL, RunningReliability, TemperatureFitter, write_calibration_json

    dev = str(model.net.store.flat.device)
    ds = create_dataset(cfg["valid_filepath"], {**cfg, "mode": "eval"}, "test", dev)  # the windows of the test path on the valid split
    d, t, c = cfg["dataloader"], cfg["test"], cfg["calibrate"]
    ign, ncls = cfg["train"]["ignore_index"], cfg["model"]["num_classes"]
    eng = model.net.engine
    model.net.eval()
    lo, hi = D.shard_range(len(ds), rank, world)
    mult = getattr(ds, "mult", None)

    def batches():
        with torch.no_grad():
            for i in range(lo, hi):
                raw_x, raw_y = ds.raw(i) if hasattr(ds, "raw") else (ds.chips[i], ds.labels[i])
                x, y = process_test(raw_x, raw_y, d["mean"], d["std"], d["temporal_dim"], t["img_size"], t["crop_size"], t["stride"], mult, dev)
                yield eng.forward(x, training=False, save=False), y

    fit = TemperatureFitter(float(c["t_min"]), float(c["t_max"]), int(c["points"]), int(c["passes"]), device=dev)
    while not fit.done:
        for logits, y in batches():
            fit.update(logits, y, ign)
        D.reduce_loss_stats(fit.device_sums(dev))  # a rank with an empty shard still takes part
        D.reduce_confusion(fit.device_count(dev))
        fit.end_pass()
    res = fit.result()
    T = res["temperature"]
    nll = RunningNLL([1.0, T], ign, dev)
    rel = [RunningReliability(ncls, int(c["nbins"]), temp, ign, dev) for temp in (1.0, T)]
    for logits, y in batches():
        nll.update(logits, y)
        for r in rel:
            r.update(logits, y)
    D.reduce_loss_stats(nll.device_sums(dev))
    D.reduce_confusion(nll.device_count(dev))
    for r in rel:
        D.reduce_confusion(r.device_hist(dev))
    if rank != 0:
        return None
    before, after = (r.compute() for r in rel)
    nll_before, nll_after = nll.compute()
    record = {"temperature": T, "nll_before": nll_before, "nll_after": nll_after, "ece_before": before["ece"], "ece_after": after["ece"],
              "mce_before": before["mce"], "mce_after": after["mce"], "classwise_ece_before": before["classwise_ece"],
              "classwise_ece_after": after["classwise_ece"], "n_valid": res["n_valid"], "at_bound": res["at_bound"],
              "bins_before": before["bins"], "bins_after": after["bins"], "grids": res["grids"], "nbins": int(c["nbins"]),
              "fit": {"vertex": res["vertex"], "nll_before": res["nll_before"], "nll_after": res["nll_after"]}}  # fmt: skip
    print(write_calibration_json(os.path.join(out_dir, "calibration.json"), record))
    return record


def tile_paths(cfg: Dict[str, Any]) -> List[str]:
    """mode=tile_inference input: ``test_filepath`` is one GeoTIFF tile or a CSV whose ``Input`` column lists tiles (paths relative
    to ``root_dir`` unless absolute)."""
    spec = str(cfg["test_filepath"])
    root = cfg.get("root_dir")
    rel = lambda p: p if os.path.isabs(p) or root in (None, "None") else os.path.join(root, p)  # noqa: E731
    path = rel(spec)
    if not path.lower().endswith(".csv"):
        return [path]
    import pandas as pd

    return [rel(str(p)) for p in pd.read_csv(path)["Input"]]


def run_tile_inference(cfg: Dict[str, Any], model, tile: str, output_dir: str, dev: str) -> Optional[str]:
    """One tile -> ``prediction_*.tif`` (+ ``probability_*.tif``) with the ``test.*`` window keys; windows shard over ranks."""
    from .infer_utils import tile_inference

    d, t = cfg["dataloader"], cfg["test"]
    mult = d.get("constant_multiplier", 1.0)
    mult = None if mult in (None, 1, 1.0) else float(mult)
    return tile_inference(tile, output_dir, model, d["mean"], d["std"], temporal_size=d["temporal_dim"], crop_size=t["crop_size"],
                          stride=t["stride"], batch_size=cfg["train"]["batch_size"], constant_multiplier=mult,
                          no_data_value=d.get("no_data_value", -9999), device=dev, blend=t.get("blend", "nearest"),
                          cover_edges=bool(t.get("cover_edges", False)), sigma_scale=float(t.get("sigma_scale", 0.125)),
                          save_probabilities=bool(t.get("save_probabilities", False)), tta=str(t.get("tta", "none")),
                          save_uncertainty=bool(t.get("save_uncertainty", False)), temperature=float(getattr(model, "temperature", 1.0)),
                          **region_options(cfg), **polygon_options(cfg), **zone_options(cfg), **cog_options(cfg))


def region_options(cfg: Dict[str, Any]) -> Dict[str, Any]:
    """The ``test.*`` keys of the region post-processing (sieve + region table) as keyword arguments of chip / tile inference."""
    t = cfg["test"]
    return dict(min_region=int(t.get("min_region", 0)), connectivity=int(t.get("connectivity", 4)),
                sieve_passes=int(t.get("sieve_passes", 8)), save_regions=bool(t.get("save_regions", False)))


def polygon_options(cfg: Dict[str, Any]) -> Dict[str, Any]:
    """The ``test.save_polygons`` key (``polygons_*.geojson``, vectorize.py) as a keyword argument of chip / tile inference."""
    return dict(save_polygons=bool(cfg["test"].get("save_polygons", False)))


def zone_options(cfg: Dict[str, Any]) -> Dict[str, Any]:
    """The ``test.zones`` / ``test.zone_id_property`` keys (``zones_*.csv``, zonal.py) as keyword arguments of chip / tile inference; a
    relative ``zones`` path is taken from ``root_dir`` like the tiles."""
    t, root = cfg["test"], cfg.get("root_dir")
    none = lambda v: None if prep.none(v) is None else str(v)  # noqa: E731  (the string "None" counts as unset, as for the required flags)
    zones = none(t.get("zones"))
    if zones is not None and not os.path.isabs(zones) and root not in (None, "None"):
        zones = os.path.join(root, zones)
    return dict(zones=zones, zone_id_property=none(t.get("zone_id_property")))


def cog_options(cfg: Dict[str, Any]) -> Dict[str, Any]:
    """The ``test.cog`` / ``cog_blocksize`` / ``overview_levels`` / ``cog_compress`` keys (Cloud Optimized GeoTIFF output, cog.py) as
    keyword arguments of tile inference, checked: a bad value raises ValueError, and so does ``cog`` with ``mode=chip_inference``."""
    from .cog import check_cog_options

    t = cfg["test"]
    compress = t.get("cog_compress", "deflate")
    compress = "none" if compress in (None, "None") else compress
    opts = dict(cog=bool(t.get("cog", False)), cog_blocksize=t.get("cog_blocksize", 256), overview_levels=t.get("overview_levels", "auto"),
                cog_compress=compress)
    check_cog_options(opts["cog"], opts["cog_blocksize"], opts["overview_levels"], compress, chip_mode=cfg.get("mode") == "chip_inference")
    return opts


def mosaic_options(cfg: Dict[str, Any]) -> Dict[str, Any]:
    """The ``test.mosaic`` / ``mosaic_rule`` / ``mosaic_cog`` / ``mosaic_cover`` keys (the mosaic of the per-chip predictions, mosaic.py),
    checked: a bad value raises ValueError, and so do ``mosaic`` outside ``mode=chip_inference`` and a rule the task's head cannot have
    (``mode`` needs class maps, ``mean`` a regression head)."""
    from .mosaic import RULES

    t = cfg["test"]
    opts = dict(mosaic=t.get("mosaic", False), rule=t.get("mosaic_rule", "last"), cog=t.get("mosaic_cog", True),
                save_cover=t.get("mosaic_cover", False))
    for key, name in (("mosaic", "mosaic"), ("cog", "mosaic_cog"), ("save_cover", "mosaic_cover")):
        if not isinstance(opts[key], bool):
            raise ValueError(f"test.{name} must be true or false (got {opts[key]!r})")
    if opts["rule"] not in RULES:
        raise ValueError(f"test.mosaic_rule must be one of {RULES} (got {opts['rule']!r})")
    if opts["mosaic"]:
        if cfg.get("mode") != "chip_inference":
            raise ValueError("test.mosaic needs mode=chip_inference: it merges the per-chip prediction files (tile inference writes one raster)")
        regression = bool(cfg.get("is_reg_task", False)) or cfg["model"].get("num_classes") == 1
        if opts["rule"] == ("mode" if regression else "mean"):
            raise ValueError(f"test.mosaic_rule={opts['rule']} does not go with a {'regression' if regression else 'classification'} head "
                             "(class maps: last | first | mode, regression: last | first | mean)")
    return opts


def warp_options(cfg: Dict[str, Any]) -> Dict[str, Any]:
    """The ``test.mosaic_crs`` / ``mosaic_resolution`` / ``mosaic_resampling`` keys (one mosaic across coordinate systems, warp.py),
    checked: a bad value raises ValueError, and so do a key without ``test.mosaic=true``, ``bilinear`` with a classification head and
    ``test.mosaic_cover`` beside ``mosaic_crs``.  ``crs`` None: the mosaic stays one per coordinate system."""
    from . import crs as crsmod
    from .warp import RESAMPLING

    t = cfg["test"]
    none = lambda v: prep.none(v, ("none", "null"))  # noqa: E731
    opts = dict(crs=none(t.get("mosaic_crs")), resolution=none(t.get("mosaic_resolution")), resampling=none(t.get("mosaic_resampling")))
    if opts["crs"] is not None and opts["crs"] != "first":
        if not isinstance(opts["crs"], str):
            raise ValueError(f"test.mosaic_crs must be None, first or EPSG:<code> (got {opts['crs']!r})")
        crsmod.parse(opts["crs"])
    res = opts["resolution"]
    if res is not None and (isinstance(res, bool) or not isinstance(res, (int, float)) or not 0 < res < float("inf")):
        raise ValueError(f"test.mosaic_resolution must be None or a positive number (got {res!r})")
    if opts["resampling"] is not None and opts["resampling"] not in RESAMPLING:
        raise ValueError(f"test.mosaic_resampling must be None or one of {RESAMPLING} (got {opts['resampling']!r})")
    for key, name in (("crs", "mosaic_crs"), ("resolution", "mosaic_resolution"), ("resampling", "mosaic_resampling")):
        if opts[key] is not None and not (t.get("mosaic", False) is True and cfg.get("mode") == "chip_inference"):
            raise ValueError(f"test.{name} needs test.mosaic=true with mode=chip_inference: it describes the merged raster")
        if opts[key] is not None and key != "crs" and opts["crs"] is None:
            raise ValueError(f"test.{name} needs test.mosaic_crs: without it the mosaics stay on their chips' grids")
    regression = bool(cfg.get("is_reg_task", False)) or cfg["model"].get("num_classes") == 1
    if opts["resampling"] == "bilinear" and not regression:
        raise ValueError("test.mosaic_resampling=bilinear does not go with a classification head (classes are not interpolated)")
    if opts["crs"] is not None and t.get("mosaic_cover", False):
        raise ValueError("test.mosaic_cover does not go with test.mosaic_crs (contributor counts belong to a group's own grid)")
    return opts


def map_tiles_options(cfg: Dict[str, Any]) -> Dict[str, Any]:
    """The ``test.map_tiles*`` keys (Web Mercator map tiles, maptiles.py), checked: a bad value raises ValueError that names the key, and
    so do ``map_tiles`` in a mode that writes no raster, ``map_tiles`` with ``mode=chip_inference`` but no ``test.mosaic``, and
    ``map_tiles_imagery`` without ``map_tiles`` and a mosaic.  -> ``on``, ``imagery`` and the keyword arguments of ``maptiles.export``."""
    from . import maptiles as M

    t, mode = cfg["test"], cfg.get("mode")
    none = lambda v: prep.none(v, ("none", "null"))  # noqa: E731
    on, imagery = t.get("map_tiles", False), t.get("map_tiles_imagery", False)
    for name, v in (("map_tiles", on), ("map_tiles_imagery", imagery)):
        if not isinstance(v, bool):
            raise ValueError(f"test.{name} must be true or false (got {v!r})")
    tile = M.check_tile_size(t.get("map_tiles_size", 256))
    zooms = {}
    for name in ("map_tiles_minzoom", "map_tiles_maxzoom"):
        v = none(t.get(name, "auto"))
        if v not in (None, "auto") and (isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= M.MAX_ZOOM):
            raise ValueError(f"test.{name} must be 'auto' or an int in 0..{M.MAX_ZOOM} (got {v!r})")
        zooms[name[10:]] = "auto" if v is None else v
    if "auto" not in zooms.values() and zooms["minzoom"] > zooms["maxzoom"]:
        raise ValueError(f"test.map_tiles_minzoom {zooms['minzoom']} lies above test.map_tiles_maxzoom {zooms['maxzoom']}")
    rescale = none(t.get("map_tiles_rescale"))
    if rescale is not None:
        ok = isinstance(rescale, (list, tuple)) and len(rescale) == 2 and all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in rescale)
        if not ok or not float(rescale[0]) < float(rescale[1]) < float("inf") or rescale[0] == float("-inf"):
            raise ValueError(f"test.map_tiles_rescale must be None or [lo, hi] with finite lo < hi (got {rescale!r})")
        rescale = (float(rescale[0]), float(rescale[1]))
    level = t.get("map_tiles_png_level", 6)
    if isinstance(level, bool) or not isinstance(level, int) or not 0 <= level <= 9:
        raise ValueError(f"test.map_tiles_png_level must be an int in 0..9 (got {level!r})")
    palette = none(t.get("map_tiles_palette"))
    if palette is not None:
        root = cfg.get("root_dir")
        if not os.path.isabs(str(palette)) and root not in (None, "None"):
            palette = os.path.join(root, str(palette))
        M.load_colors(str(palette))
    regression = bool(cfg.get("is_reg_task", False)) or cfg["model"].get("num_classes") == 1
    if rescale is not None and on and not regression and not imagery and mode != "map_tiles":
        raise ValueError("test.map_tiles_rescale does not go with a classification head (class maps take test.map_tiles_palette)")
    if on and mode not in ("tile_inference", "chip_inference", "map_tiles"):
        raise ValueError(f"test.map_tiles needs mode=tile_inference, chip_inference or map_tiles (mode={mode} writes no raster)")
    if on and mode == "chip_inference" and t.get("mosaic", False) is not True:
        raise ValueError("test.map_tiles needs test.mosaic=true with mode=chip_inference: the tiles show the merged raster")
    if imagery and not (on and mode == "chip_inference" and t.get("mosaic", False) is True):
        raise ValueError("test.map_tiles_imagery needs test.map_tiles=true and test.mosaic=true with mode=chip_inference: the imagery is the "
                         "mosaic of the input chips")
    if mode == "map_tiles" and none(t.get("input")) is None:
        raise ValueError("mode=map_tiles needs test.input=<a GeoTIFF>")
    return dict(on=on or mode == "map_tiles", imagery=imagery,
                export=dict(tile=tile, palette=palette, rescale=rescale, png_level=level, **zooms))


def write_map_tiles(raster_path: str, opts: Dict[str, Any], device: Optional[str], name: Optional[str] = None) -> List[str]:
    """``tiles_<name>/`` beside ``raster_path`` (a written prediction raster; the overviews of a COG are reused), through
    ``maptiles.export``; an int8 raster is a class map (palette), a float32 one goes through the ramp."""
    from . import maptiles as M
    from . import tiff as tiffmod

    stem = name or os.path.splitext(os.path.basename(raster_path))[0]
    out = os.path.join(os.path.dirname(os.path.abspath(raster_path)), f"tiles_{stem}")
    kw = dict(opts["export"])
    prof = tiffmod.read_profile(raster_path)
    if str(prof.get("dtype")) == "int8":
        kw["rescale"] = None
        nd = prof.get("nodata")
        kw["fill"] = int(nd) if nd is not None and -128 <= nd <= 127 and float(nd) == int(nd) else -1
    return M.export(raster_path, out, device=device, name=stem, **kw)


def main(argv: Optional[List[str]] = None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config-name", default="config")
    ap.add_argument("--config-path", default=None)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "bf16x3"])
    ap.add_argument("--output-dir", default=None, help="replaces the Hydra run dir (checkpoint + resolved config)")
    ap.add_argument("overrides", nargs="*")
    args = ap.parse_args(argv)
    cfg = load_config(args.config_name, args.overrides, args.config_path)
    cog_options(cfg)  # a bad COG key, or test.cog with mode=chip_inference, stops here: before the model is built
    mosaic = mosaic_options(cfg)  # likewise a bad mosaic key, or test.mosaic outside mode=chip_inference
    reproject = warp_options(cfg)  # likewise the keys of the reprojected mosaic
    tiles = map_tiles_options(cfg)  # likewise the keys of the map tiles
    object_options(cfg)  # likewise the keys of the object metrics (create_model reads them again)
    if cfg["mode"] == "map_tiles":  # no model: an existing GeoTIFF -> tiles_<name>/{z}/{x}/{y}.png + tilejson.json (maptiles.py)
        inp = str(cfg["test"]["input"])
        root = cfg.get("root_dir")
        inp = inp if os.path.isabs(inp) or root in (None, "None") else os.path.join(root, inp)
        print(json.dumps({"map_tiles": write_map_tiles(inp, tiles, prep.default_device())[-1]}))
        return 0
    if cfg["mode"] in PREP_MODES:  # no model: files in, files out; the module is imported only when its mode runs
        import importlib

        return importlib.import_module(f".{PREP_MODES[cfg['mode']]}", __package__).run_from_config(cfg, prep.default_device())
    start = time.time()
    torch.manual_seed(SEED)
    np.random.seed(SEED)
    rank, local_rank, world = D.init_from_env()
    get_device()
    torch.cuda.set_device(local_rank)
    dev = f"cuda:{local_rank}"
    out_dir = args.output_dir or os.path.join(os.getcwd(), "outputs", time.strftime("%Y-%m-%d_%H-%M-%S"))
    if rank == 0:
        os.makedirs(os.path.join(out_dir, ".hydra"), exist_ok=True)
        import yaml

        yaml.safe_dump(cfg, open(os.path.join(out_dir, ".hydra", "config.yaml"), "w"), sort_keys=False)

    if cfg["mode"] == "stats":
        # run.py:89-111: the train set with mean 0 / std 1 and no augmentation, reduced to per-band mean/std + class weights
        check_required_flags(["train_filepath"], cfg)
        scfg = {**cfg, "dataloader": {**cfg["dataloader"], "mean": [0.0] * len(cfg["dataloader"]["mean"]),
                                      "std": [1.0] * len(cfg["dataloader"]["std"])}}  # fmt: skip
        ds = create_dataset(cfg["train_filepath"], scfg, "train", dev)
        bs = cfg["train"]["batch_size"]
        loader = (_stack(ds, ids) for ids in _batches(ds, bs, False, 0, 0, 1))
        mean, std, class_weights = compute_stats(loader, is_reg_task=bool(cfg.get("is_reg_task", False)), device=dev)
        if rank == 0:
            print(json.dumps({"mean": mean, "std": std, "class_weights": class_weights}))
        return 0
    model = create_model(cfg, precision=args.precision, device=dev)
    if cfg["mode"] == "train":
        check_required_flags(["train_filepath", "valid_filepath"], cfg)
        hist = train(cfg, model, out_dir, rank, world)
        if rank == 0:
            print(f"Elapsed time: {time.time() - start:.2f} seconds")
    elif cfg["mode"] == "eval":
        check_required_flags(["test_filepath", "checkpoint_path"], cfg)
        res = evaluate(cfg, model, rank, world)
        if rank == 0:
            print(json.dumps({"Evaluation results": {k: round(v, 6) for k, v in res.items()}}))
            print(f"Elapsed time: {time.time() - start:.2f} seconds")
    elif cfg["mode"] == "calibrate":
        check_required_flags(["valid_filepath", "checkpoint_path"], cfg)
        calibrate(cfg, model, out_dir, rank, world)
    elif cfg["mode"] == "chip_inference":
        check_required_flags(["root_dir", "test_filepath", "checkpoint_path"], cfg)
        model.net.eval()
        output_dir = os.path.join(cfg["root_dir"], "predictions")
        ds = create_dataset(cfg["test_filepath"], cfg, "test", dev)
        if isinstance(ds, SyntheticChipDataset):
            ds = ArrayChipDataset([ds.raw(i)[0] for i in range(len(ds))], [ds.raw(i)[1] for i in range(len(ds))], ds.mean, ds.std, ds.T,
                                  1e-4, include_filenames=True, device=dev)
        lo, hi = D.shard_range(len(ds), rank, world)
        bs = cfg["train"]["batch_size"]
        loader = (infer_collate_fn([ds[j] for j in range(i, min(i + bs, hi))]) for i in range(lo, hi, bs))
        info = chip_inference(loader, output_dir, model, device="gpu", **region_options(cfg), **polygon_options(cfg), **zone_options(cfg))
        if rank == 0:
            print(f"Carbon tracking information: {info}")
        if mosaic.pop("mosaic"):
            if D.dp_active():
                torch.distributed.barrier()  # every rank's chips are on disk
            if rank == 0:
                from .mosaic import merge_predictions
                from .warp import merge_reprojected

                ncls = int(model.net.cfg.num_classes)
                cog = {k: v for k, v in cog_options(cfg).items() if k != "cog"}
                keys = dict(fill=-1, num_classes=None if ncls == 1 else ncls, device=dev, **mosaic, **cog, **region_options(cfg),
                            **polygon_options(cfg), **zone_options(cfg))
                if reproject["crs"] is not None:
                    merged = merge_reprojected(output_dir, output_dir, **reproject, **keys)
                else:
                    merged = merge_predictions(output_dir, output_dir, **keys)
                print(json.dumps({"mosaic": merged}))
                if tiles["on"]:
                    for path in merged:
                        base = os.path.basename(path)
                        if base.startswith("predictions_merged") and base.endswith(".tif"):
                            print(json.dumps({"map_tiles": write_map_tiles(path, tiles, dev, base[len("predictions_") : -4])[-1]}))
                if tiles["imagery"]:
                    from . import maptiles as M

                    levels, prof = M.merge_chips(tile_paths(cfg), device=dev, out_path=os.path.join(output_dir, "chips_merged.tif"),
                                                 tile=tiles["export"]["tile"])
                    kw = dict(tiles["export"], palette=None, rescale=tiles["export"]["rescale"] or (0.0, 3000.0))
                    print(json.dumps({"map_tiles": M.export(levels, os.path.join(output_dir, "tiles_chips"), prof, order=(2, 1, 0),
                                                            name="chips", **kw)[-1]}))
    elif cfg["mode"] == "tile_inference":
        check_required_flags(["root_dir", "test_filepath", "checkpoint_path"], cfg)
        for tile in tile_paths(cfg):
            out = run_tile_inference(cfg, model, tile, os.path.join(cfg["root_dir"], "predictions"), dev)
            if rank == 0:
                print(json.dumps({"tile": tile, "prediction": out}))
                if tiles["on"] and out is not None:
                    stem = os.path.splitext(os.path.basename(tile))[0]
                    print(json.dumps({"map_tiles": write_map_tiles(out, tiles, dev, stem)[-1]}))
    else:
        raise ValueError(f"unknown mode {cfg['mode']!r}")
    if D.dp_active():
        torch.distributed.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
