"""D4 test-time augmentation and uncertainty rasters of the blended tile path, host side (no GPU): the transform codes against numpy,
argument checks of the three HIP entry points and the config keys of mode=tile_inference."""
import ctypes
import os

import numpy as np
import pytest

from instageo_amd import dataloader as DL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "instageo-e2e-geospatial-ml_amd")


@pytest.fixture(scope="module")
def built_lib():
    import subprocess

    from instageo_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j4"], check=True)
    return _lib


def _g(a, k):
    """The test's own restatement of G_k: G_k(a)[y][x] = a[sy][sx]."""
    S = a.shape[0]
    h, v, t = k & 1, (k >> 1) & 1, (k >> 2) & 1
    out = np.empty_like(a)
    for y in range(S):
        for x in range(S):
            y1, x1 = (x, y) if t else (y, x)
            out[y, x] = a[S - 1 - y1 if v else y1, S - 1 - x1 if h else x1]
    return out


def test_d4_codes_and_inverse_against_numpy():
    assert DL.d4_codes("none") == [0] and DL.d4_codes("flips") == [0, 1, 2, 3] and DL.d4_codes("d4") == list(range(8))
    with pytest.raises(ValueError):
        DL.d4_codes("rot")
    a = np.arange(64).reshape(8, 8)
    names = [a, np.fliplr(a), np.flipud(a), np.rot90(a, 2), a.T, np.rot90(a, 1), np.rot90(a, -1), np.rot90(a, 2).T]
    imgs = [_g(a, k) for k in range(8)]
    for k in range(8):
        assert np.array_equal(imgs[k], names[k]), k
    assert len({im.tobytes() for im in imgs}) == 8
    inv = DL.d4_inverse(range(8))
    assert inv == [0, 1, 2, 3, 4, 6, 5, 7] and DL.d4_inverse([5, 1]) == [6, 1]
    for k in range(8):
        assert np.array_equal(_g(_g(a, k), inv[k]), a), k
    with pytest.raises(ValueError):
        DL.d4_inverse([8])


def test_tta_entry_points_exported_and_validated_without_gpu(built_lib):
    """IG_REQUIRE rejects bad arguments before any launch (safe on a CPU-only box); the messages name the argument."""
    names = {"ig_d4_apply", "ig_window_blend_accumulate_tta", "ig_window_blend_uncertainty"}
    assert names <= set(built_lib.declared_symbols())
    lib = built_lib.load()
    assert all(hasattr(lib, n) for n in names)
    err = built_lib.last_error
    one, two = ctypes.c_void_p(16), ctypes.c_void_p(4096)

    def codes(*k):
        return (ctypes.c_int * len(k))(*k)

    d4 = lib.ig_d4_apply
    assert d4(None, two, codes(0), 1, 1, 1, 8, 1, None) == -1 and "null pointer" in err()
    assert d4(one, None, codes(0), 1, 1, 1, 8, 1, None) == -1 and "null pointer" in err()
    assert d4(one, two, None, 1, 1, 1, 8, 1, None) == -1 and "null pointer" in err() and "codes" in err()
    assert d4(one, two, codes(0), 0, 1, 1, 8, 1, None) == -1 and "K" in err()
    assert d4(one, two, codes(*range(8), 0), 9, 1, 1, 8, 1, None) == -1 and "K" in err()
    assert d4(one, two, codes(0, 8), 2, 1, 1, 8, 1, None) == -1 and "codes[1]" in err()
    assert d4(one, two, codes(-1), 1, 1, 1, 8, 1, None) == -1 and "codes[0]" in err()
    assert d4(one, one, codes(0), 1, 1, 1, 8, 1, None) == -1 and "src == dst" in err()
    assert d4(one, two, codes(0), 1, 1, 1, 0, 1, None) == -1 and "S" in err()
    assert d4(None, None, codes(0, 5), 2, 0, 3, 8, 1, None) == 0  # m = 0: nothing to do

    acc = lib.ig_window_blend_accumulate_tta
    assert acc(None, one, one, 2, 2, 0, 4, 4, one, one, one, 2, 64, 128, 128, 0, 128, 0, 128, None) == -1 and "null pointer" in err()
    assert acc(one, one, one, 2, 2, 0, 4, 0, one, one, one, 2, 64, 128, 128, 0, 128, 0, 128, None) == -1 and "K" in err()
    assert acc(one, one, one, 2, 2, 0, 4, 9, one, one, one, 2, 64, 128, 128, 0, 128, 0, 128, None) == -1 and "K" in err()
    assert acc(one, one, one, 2, 2, 0, 4, 4, one, one, one, 0, 64, 128, 128, 0, 128, 0, 128, None) == -1 and "ncls" in err()
    assert acc(one, one, one, 2, 2, 0, 4, 4, one, one, one, 2, 256, 128, 300, 0, 128, 0, 128, None) == -1 and "crop" in err()
    assert acc(one, one, one, 2, 2, 1, 4, 4, one, one, one, 2, 64, 128, 128, 0, 128, 0, 128, None) == -1 and "w0 + n" in err()
    assert acc(one, one, one, 2, 2, 0, 4, 4, one, one, one, 2, 64, 128, 128, 100, 64, 0, 128, None) == -1 and "band" in err()

    unc = lib.ig_window_blend_uncertainty
    assert unc(None, one, None, 0, 0, 0.0, 0, one, one, 2, 100, None) == -1 and "null pointer" in err()
    assert unc(one, one, None, 0, 0, 0.0, 0, None, None, 2, 100, None) == -1 and "null pointer" in err() and "entropy and margin" in err()
    assert unc(one, one, None, 0, 6, -9999.0, 1, one, one, 2, 100, None) == -1 and "null pointer" in err() and "tile" in err()
    assert unc(one, one, None, 0, 0, 0.0, 0, one, one, 1, 100, None) == -1 and "ncls" in err()
    assert unc(one, one, None, 0, 0, 0.0, 0, one, None, 128, 100, None) == -1 and "ncls" in err()
    with pytest.raises(built_lib.HipLibraryError):
        built_lib.call("ig_window_blend_uncertainty", one, one, None, 0, 0, 0.0, 0, one, one, 2, -1, None)


def test_d4_apply_is_not_a_generated_custom_op():
    """Its codes are a HOST array, so the header-generated torch op (device tensors only) leaves it out, like the grouped launch."""
    from instageo_amd import torch_ops

    raw = torch_ops.register()
    assert "d4_apply" not in raw and "window_blend_accumulate_tta" in raw and "window_blend_uncertainty" in raw
    assert "Tensor(a!)? entropy" in raw["window_blend_uncertainty"] and "int K" in raw["window_blend_accumulate_tta"]


def test_config_carries_tta_and_uncertainty_with_legacy_defaults():
    from instageo_amd.config import DEFAULTS, load_config

    t = DEFAULTS["test"]
    assert t["tta"] == "none" and t["save_uncertainty"] is False
    cfg = load_config("sen1floods11", ["mode=tile_inference", "test.blend=gaussian", "test.tta=d4", "test.save_uncertainty=true"])
    assert cfg["test"]["tta"] == "d4" and cfg["test"]["save_uncertainty"] is True
    assert load_config("sen1floods11", ["test.tta=flips"])["test"]["tta"] == "flips"


def test_tile_inference_refuses_tta_on_the_nearest_path_before_any_work():
    from instageo_amd.infer_utils import tile_inference

    # the tile does not exist and the model is None: the options are checked before the file, the model or a device is touched
    args = ("/nonexistent/tile.tif", "/nonexistent/out", None, [0.0], [1.0])
    with pytest.raises(ValueError, match="tta"):
        tile_inference(*args, blend="nearest", tta="d4")
    with pytest.raises(ValueError, match="save_uncertainty"):
        tile_inference(*args, blend="nearest", save_uncertainty=True)
    with pytest.raises(ValueError, match="rot"):
        tile_inference(*args, blend="gaussian", tta="rot")
    with pytest.raises(ValueError, match="rot"):
        tile_inference(*args, tta="rot")
