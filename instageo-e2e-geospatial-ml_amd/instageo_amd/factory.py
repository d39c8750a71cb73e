"""Model factory (reference: ``instageo/model/factory.py:35-116``): config -> task module (+ checkpoint)."""
from __future__ import annotations

from typing import Any, Dict

import torch

from .boundary import check_boundary_options
from .calibration import check_calibrate_options, resolve_temperature
from .objects import check_object_options
from .regression import PrithviDistillationRegressionModule, PrithviRegressionModule
from .segmentation import LOSS_CHOICES, PrithviDistillationSegmentationModule, PrithviSegmentationModule


def object_options(cfg: Dict[str, Any]) -> Dict[str, Any]:
    """The ``test.object_*`` keys (objects.py) as keyword arguments of ``set_object_metrics``, checked: a bad value raises ValueError.
    With ``test.object_metrics`` off the thresholds are None and nothing is built."""
    test_cfg = cfg.get("test", {})
    if not test_cfg.get("object_metrics", False):
        return dict(thresholds=None)
    opts = dict(thresholds=test_cfg.get("object_iou_thresholds", [0.5]), connectivity=test_cfg.get("object_connectivity", 4),
                min_area=test_cfg.get("object_min_area", 1), classes=test_cfg.get("object_classes"))
    if opts["classes"] == "None":
        opts["classes"] = None
    opts["thresholds"] = check_object_options(opts["thresholds"], cfg["model"]["num_classes"], opts["connectivity"], opts["min_area"],
                                              opts["classes"], bool(cfg.get("is_reg_task", False)))
    return opts


def create_model(cfg: Dict[str, Any], precision: str = "bf16", device=None) -> PrithviSegmentationModule:
    """Build the segmentation (or, with ``is_reg_task``, regression) module from a run.py config; non-train modes load ``checkpoint_path`` strictly
    (``torch.load(path)["state_dict"]``, factory.py:113-115)."""
    m, t, d = cfg["model"], cfg["train"], cfg["dataloader"]
    train_mode = cfg["mode"] == "train"
    common = dict(
        image_size=d["img_size"] if train_mode else cfg["test"]["crop_size"],
        learning_rate=t["learning_rate"],
        freeze_backbone=m["freeze_backbone"],
        load_pretrained_weights=bool(m["load_pretrained_weights"]) and train_mode and cfg.get("allow_hub_download", False),
        temporal_step=d["temporal_dim"],
        ignore_index=t["ignore_index"],
        weight_decay=t["weight_decay"],
        scheduler=t.get("scheduler", False),
        model_name=m["model_name"],
        weight_clip_range=m.get("weight_clip_range"),
        depth=m.get("depth", -1),
        precision=precision,
        device=device,
    )
    test_cfg, cal = cfg.get("test", {}), cfg.get("calibrate", {})
    temperature = resolve_temperature(test_cfg)
    check_calibrate_options(cal.get("points", 32), cal.get("passes", 2), cal.get("t_min", 0.125), cal.get("t_max", 8.0), cal.get("nbins", 15),
                            None if cfg.get("is_reg_task", False) else m["num_classes"])
    if cfg.get("is_reg_task", False):
        if cfg["mode"] == "calibrate":
            raise ValueError("mode=calibrate fits a softmax temperature: a regression task (is_reg_task) has no class probabilities")
        if temperature != 1.0 or test_cfg.get("calibration_metrics", False):
            raise ValueError("test.temperature / test.calibration / test.calibration_metrics need class probabilities (not is_reg_task)")
    boundary = None
    if test_cfg.get("boundary_metrics", False):
        boundary = check_boundary_options(test_cfg.get("boundary_distances", [1, 2, 4]), m["num_classes"], bool(cfg.get("is_reg_task", False)))
    objects = object_options(cfg)
    loss = t.get("loss", "ce")
    if loss not in LOSS_CHOICES:
        raise ValueError(f"train.loss={loss!r}: choose one of {', '.join(LOSS_CHOICES)}")
    if cfg.get("is_reg_task", False) and loss != "ce":
        raise ValueError(f"train.loss={loss!r} is a segmentation objective: a regression task (is_reg_task) trains on its masked MSE")
    seg_loss = dict(loss=loss, focal_gamma=t.get("focal_gamma", 2.0), region_weight=t.get("region_weight", 1.0),
                    region_smooth=t.get("region_smooth", 1.0), tversky=tuple(t.get("tversky", (0.5, 0.5))))
    distill = bool(t.get("distillation", False)) and train_mode
    if distill and cfg.get("is_reg_task", False):  # factory.py:61-69
        common_d = {k: v for k, v in common.items() if k != "depth"}
        model = PrithviDistillationRegressionModule(teacher_ckpt_path=t["teacher_ckpt_path"], depth=t.get("teacher_depth", -1),
                                                    student_depth=m.get("depth", -1), use_log_scale=m.get("use_log_scale", False),
                                                    plot_reg_results=m.get("plot_reg_results", False),
                                                    include_ee=m.get("include_ee_metric", False), **common_d)
    elif distill:  # factory.py:84-91: frozen teacher from train.teacher_ckpt_path, student of model.depth blocks
        common_d = {k: v for k, v in common.items() if k != "depth"}
        model = PrithviDistillationSegmentationModule(teacher_ckpt_path=t["teacher_ckpt_path"], num_classes=m["num_classes"],
                                                      class_weights=t["class_weights"], depth=t.get("teacher_depth", -1),
                                                      student_depth=m.get("depth", -1), **seg_loss, **common_d)
    elif cfg.get("is_reg_task", False):  # factory.py:58-76, 97-104
        model = PrithviRegressionModule(use_log_scale=m.get("use_log_scale", False), plot_reg_results=m.get("plot_reg_results", False),
                                        include_ee=m.get("include_ee_metric", False), **common)
    else:
        model = PrithviSegmentationModule(num_classes=m["num_classes"], class_weights=t["class_weights"], **seg_loss, **common)
    if not cfg.get("is_reg_task", False):
        model.set_calibration(temperature, bool(test_cfg.get("calibration_metrics", False)), int(cal.get("nbins", 15)))
        model.set_boundary_metrics(boundary)
        model.set_object_metrics(**objects)
    if not train_mode:
        ckpt = cfg.get("checkpoint_path")
        if not ckpt or str(ckpt) == "None":
            raise RuntimeError("checkpoint_path is required for eval / calibrate / chip_inference")
        sd = torch.load(ckpt, map_location="cpu")["state_dict"]
        model.load_checkpoint_state_dict(sd, strict=True)
    return model
