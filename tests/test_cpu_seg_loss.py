"""CPU tests (-m "not gpu") of the focal / Dice / Tversky segmentation losses: the C-ABI entry point is declared and exported, its
dispatcher op is generated from the header, bad arguments are refused before any launch, and the config surface and the factory know
the new objective."""
import ctypes
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "instageo-e2e-geospatial-ml_amd")


@pytest.fixture(scope="module")
def lib_mod():
    from instageo_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j4"], check=True)
    return _lib


def test_seg_loss_is_declared_and_exported(lib_mod):
    assert "ig_seg_loss" in lib_mod.declared_symbols()
    ret, types = lib_mod.parse_header()["ig_seg_loss"]
    assert ret == "int" and types.count("float") == 5 and types[-1] == "void*"
    assert hasattr(lib_mod.load(), "ig_seg_loss")
    # ig_ce_loss keeps its prototype
    assert lib_mod.parse_header()["ig_ce_loss"][1] == ["const float*", "const void*", "int", "const float*", "long", "double*", "float*",
                                                       "long long*", "signed char*", "unsigned long long*", "int", "long", "int", "void*"]


def test_seg_loss_torch_op_marks_its_outputs_mutated():
    from instageo_amd import torch_ops

    assert "seg_loss" in torch_ops.register()
    sch = str(torch.ops.instageo_mi355x.seg_loss.default._schema)
    for out in ("stats", "parts", "dlogits", "preds", "preds_i8", "confusion"):
        assert f"!)? {out}" in sch, (out, sch)
    for inp in ("logits", "labels", "class_weights"):
        assert f"Tensor? {inp}" in sch, (inp, sch)
    for scalar in ("float focal_gamma", "int pixel_term", "float region_weight", "float region_smooth", "float tversky_alpha",
                   "float tversky_beta"):
        assert scalar in sch, (scalar, sch)


def _call(lib, logits, labels, gamma=2.0, lam=1.0, smooth=1.0, alpha=0.5, beta=0.5, ncls=2):
    return lib.ig_seg_loss(logits, labels, 0, None, -1, gamma, 1, lam, smooth, alpha, beta, None, None, None, None, None, None, 1, 4, ncls, None)


def test_seg_loss_argument_validation_without_gpu(lib_mod):
    """IG_REQUIRE refuses each of these before any HIP call, so the calls are safe without a GPU."""
    lib = lib_mod.load()
    one = ctypes.c_void_p(16)
    assert _call(lib, None, one) == -1 and "null pointer" in lib_mod.last_error()
    assert _call(lib, one, None) == -1 and "null pointer" in lib_mod.last_error()
    assert _call(lib, one, one, ncls=17) == -1 and "ncls" in lib_mod.last_error()
    assert _call(lib, one, one, gamma=0.5) == -1 and "focal_gamma" in lib_mod.last_error()
    assert _call(lib, one, one, gamma=8.5) == -1 and "focal_gamma" in lib_mod.last_error()
    assert _call(lib, one, one, alpha=0.0) == -1 and "tversky_alpha" in lib_mod.last_error()
    assert _call(lib, one, one, beta=-0.1) == -1 and "tversky_beta" in lib_mod.last_error()
    assert _call(lib, one, one, smooth=-1.0) == -1 and "region_smooth" in lib_mod.last_error()
    assert _call(lib, one, one, lam=-1.0) == -1 and "region_weight" in lib_mod.last_error()


def test_seg_loss_wrapper_refuses_cpu_tensors(lib_mod):
    from instageo_amd import ops

    z = torch.zeros(1, 2, 2, 2)
    y = torch.zeros(1, 2, 2, dtype=torch.int64)
    with pytest.raises(lib_mod.HipLibraryError):
        ops.seg_loss(z, y, None, -1, torch.zeros(2, dtype=torch.float64), focal_gamma=2.0, region_weight=1.0)


def test_config_carries_the_loss_keys():
    from instageo_amd.config import DEFAULTS, load_config

    t = DEFAULTS["train"]
    assert (t["loss"], t["focal_gamma"], t["region_weight"], t["region_smooth"], t["tversky"]) == ("ce", 2.0, 1.0, 1.0, [0.5, 0.5])
    c = load_config("config", ["train.loss=focal_dice", "train.focal_gamma=1.5"])
    assert c["train"]["loss"] == "focal_dice" and c["train"]["focal_gamma"] == 1.5 and c["train"]["tversky"] == [0.5, 0.5]
    c = load_config("sen1floods11", ["train.tversky=[0.3,0.7]"])
    assert c["train"]["tversky"] == [0.3, 0.7] and c["train"]["loss"] == "ce"


def test_loss_spec():
    from instageo_amd.segmentation import LOSS_CHOICES, loss_spec

    assert LOSS_CHOICES == ("ce", "focal", "dice", "ce_dice", "focal_dice")
    assert loss_spec("ce") is None
    assert loss_spec("focal", focal_gamma=3.0) == dict(focal_gamma=3.0, pixel_term=True, region_weight=0.0, region_smooth=1.0, tversky=(0.5, 0.5))
    assert loss_spec("dice", focal_gamma=3.0, region_weight=2.0)["pixel_term"] is False
    assert loss_spec("dice", focal_gamma=3.0)["focal_gamma"] == 0.0
    s = loss_spec("ce_dice", focal_gamma=3.0, region_weight=0.5, region_smooth=0.0, tversky=[0.3, 0.7])
    assert s == dict(focal_gamma=0.0, pixel_term=True, region_weight=0.5, region_smooth=0.0, tversky=(0.3, 0.7))
    assert loss_spec("focal_dice")["focal_gamma"] == 2.0 and loss_spec("focal_dice")["region_weight"] == 1.0
    with pytest.raises(ValueError, match="focal_dice"):
        loss_spec("nope")
    with pytest.raises(ValueError):
        loss_spec("focal", focal_gamma=0.5)
    with pytest.raises(ValueError):
        loss_spec("dice", tversky=(0.0, 1.0))
    with pytest.raises(ValueError):
        loss_spec("ce_dice", region_weight=0.0)


def test_factory_rejects_unknown_and_regression_losses():
    """Both are refused before any module (and so any device memory) is made."""
    from instageo_amd.config import load_config
    from instageo_amd.factory import create_model

    with pytest.raises(ValueError, match="ce, focal, dice, ce_dice, focal_dice"):
        create_model(load_config("config", ["train.loss=nope"]))
    with pytest.raises(ValueError, match="regression"):
        create_model(load_config("config", ["train.loss=focal", "is_reg_task=True"]))
