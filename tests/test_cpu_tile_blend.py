"""Blended tile inference, host side (no GPU): the window grid, the blend weights, argument checks of the two HIP entry points,
the config keys of mode=tile_inference and the rank-ordered band reduction."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from instageo_amd import dataloader as DL
from instageo_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "instageo-e2e-geospatial-ml_amd")


@pytest.fixture(scope="module")
def built_lib():
    import subprocess

    from instageo_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j4"], check=True)
    return _lib


def test_window_grid_reproduces_window_origins_on_square_tiles():
    for S, crop, stride in [(512, 224, 224), (700, 224, 224), (10980, 224, 224), (500, 224, 92), (40, 16, 8), (224, 224, 224)]:
        tops, lefts = DL.window_grid(S, S, crop, stride)
        assert tops == lefts and [(t, l) for t in tops for l in lefts] == DL.window_origins(S, crop, stride)


@pytest.mark.parametrize("H,W,crop,stride", [(300, 410, 64, 40), (500, 500, 224, 224), (10980, 10980, 224, 224), (225, 700, 224, 112),
                                             (64, 64, 64, 7), (100, 257, 32, 50), (333, 97, 97, 1000)])
def test_window_grid_cover_edges_covers_every_pixel(H, W, crop, stride):
    tops, lefts = DL.window_grid(H, W, crop, stride, cover_edges=True)
    for o, size in ((tops, H), (lefts, W)):
        assert o == sorted(set(o)) and o[0] == 0 and o[-1] == size - crop
        assert o[:-1] == list(range(0, size - crop + 1, stride))[: len(o) - 1]
        covered = np.zeros(size, dtype=bool)
        for v in o:
            covered[v : v + crop] = True
        assert covered[-1] and (covered.all() or stride > crop)  # stride > crop leaves gaps between windows, never at the edge
    # without cover_edges the remainder strip of the same tile stays uncovered when size - crop is off the stride grid
    t0, _ = DL.window_grid(H, W, crop, stride)
    assert (t0[-1] == H - crop) == (tops == t0)


def test_window_grid_rejects_bad_arguments():
    with pytest.raises(ValueError):
        DL.window_grid(100, 300, 128, 64)
    with pytest.raises(ValueError):
        DL.window_grid(300, 100, 128, 64, cover_edges=True)
    with pytest.raises(ValueError):
        DL.window_grid(300, 300, 128, 0)


@pytest.mark.parametrize("crop,sigma_scale", [(224, 0.125), (64, 0.125), (63, 0.3), (5, 0.01)])
def test_blend_weights_match_a_float64_restatement(crop, sigma_scale):
    i = np.arange(crop, dtype=np.float64) - (crop - 1) / 2.0
    sigma = sigma_scale * crop
    ref = np.maximum(np.exp(-(i**2) / (2 * sigma**2)), 1e-3).astype(np.float32)
    g = ops.blend_weights(crop, "gaussian", sigma_scale)
    assert g.dtype == torch.float32 and g.shape == (crop,) and np.array_equal(g.numpy(), ref)
    assert torch.equal(ops.blend_weights(crop, "mean"), torch.ones(crop))
    with pytest.raises(ValueError):
        ops.blend_weights(crop, "nearest")


def test_blend_entry_points_exported_and_validated_without_gpu(built_lib):
    """IG_REQUIRE rejects bad arguments before any launch (safe on a CPU-only box)."""
    assert {"ig_window_blend_accumulate", "ig_window_blend_finalize"} <= set(built_lib.declared_symbols())
    lib = built_lib.load()
    one = ctypes.c_void_p(16)
    acc = lib.ig_window_blend_accumulate
    assert acc(None, one, one, 2, 2, 0, 4, one, one, one, 2, 64, 128, 128, 0, 128, 0, 128, None) == -1
    assert "null pointer" in built_lib.last_error()
    assert acc(one, one, one, 2, 2, 0, 4, one, one, one, 0, 64, 128, 128, 0, 128, 0, 128, None) == -1
    assert "ncls" in built_lib.last_error()
    assert acc(one, one, one, 2, 2, 0, 4, one, one, one, 2, 256, 128, 300, 0, 128, 0, 128, None) == -1
    assert "crop" in built_lib.last_error()
    assert acc(one, one, one, 2, 2, 1, 4, one, one, one, 2, 64, 128, 128, 0, 128, 0, 128, None) == -1
    assert "w0 + n" in built_lib.last_error()
    assert acc(one, one, one, 2, 2, 0, 4, one, one, one, 2, 64, 128, 128, 100, 64, 0, 128, None) == -1
    assert "band" in built_lib.last_error()
    fin = lib.ig_window_blend_finalize
    assert fin(None, one, None, 0, 0, 0.0, 0, one, None, 2, 100, -1, None) == -1 and "null pointer" in built_lib.last_error()
    assert fin(one, one, None, 0, 6, -9999.0, 1, one, None, 2, 100, -1, None) == -1 and "null pointer" in built_lib.last_error()
    assert fin(one, one, None, 0, 0, 0.0, 0, one, None, 128, 100, -1, None) == -1 and "ncls" in built_lib.last_error()
    assert fin(one, one, None, 0, 0, 0.0, 0, one, None, 1, 100, -1, None) == -1 and "regression" in built_lib.last_error()
    with pytest.raises(built_lib.HipLibraryError):
        built_lib.call("ig_window_blend_finalize", one, one, None, 0, 0, 0.0, 0, one, None, 2, 100, 300, None)


def test_config_carries_the_tile_keys_with_legacy_defaults():
    from instageo_amd.config import DEFAULTS, load_config

    t = DEFAULTS["test"]
    assert t["blend"] == "nearest" and t["cover_edges"] is False and t["sigma_scale"] == 0.125 and t["save_probabilities"] is False
    cfg = load_config("sen1floods11", ["mode=tile_inference", "test.blend=gaussian", "test.cover_edges=true", "test.save_probabilities=True"])
    assert cfg["test"]["blend"] == "gaussian" and cfg["test"]["cover_edges"] is True and cfg["test"]["save_probabilities"] is True


def test_tile_paths_single_tile_or_csv(tmp_path):
    from instageo_amd.run import tile_paths

    (tmp_path / "tiles.csv").write_text("Input,Other\na.tif,x\n/abs/b.tif,y\n")
    assert tile_paths({"root_dir": str(tmp_path), "test_filepath": "tiles.csv"}) == [str(tmp_path / "a.tif"), "/abs/b.tif"]
    assert tile_paths({"root_dir": str(tmp_path), "test_filepath": "t.tif"}) == [str(tmp_path / "t.tif")]


def test_tile_inference_refuses_nearest_with_cover_edges_before_any_work():
    from instageo_amd.infer_utils import tile_inference

    # the tile does not exist and the model is None: the options are checked before the file, the model or a device is touched
    with pytest.raises(ValueError, match="cover_edges"):
        tile_inference("/nonexistent/tile.tif", "/nonexistent/out", None, [0.0], [1.0], blend="nearest", cover_edges=True)
    with pytest.raises(ValueError):
        tile_inference("/nonexistent/tile.tif", "/nonexistent/out", None, [0.0], [1.0], save_probabilities=True)
    with pytest.raises(ValueError):
        tile_inference("/nonexistent/tile.tif", "/nonexistent/out", None, [0.0], [1.0], blend="median")


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _bands_worker(rank: int, world: int, port: int, q) -> None:
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "instageo-e2e-geospatial-ml_amd"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import torch.distributed as dist

    from instageo_amd import distributed as D

    D.init_from_env(backend="gloo")
    try:
        bands = [(0, 5), (3, 4), (0, 0)][:world]
        y0, hb = bands[rank]
        local = torch.full((2, hb, 3), float(rank + 1))
        out = D.reduce_row_bands(local, bands, 9)
        q.put((rank, None if out is None else out.numpy().copy()))
    except Exception:  # pragma: no cover
        import traceback

        q.put((rank, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def test_reduce_row_bands_adds_bands_in_rank_order():
    """Three gloo ranks on the CPU: bands rows [0, 5), [3, 7) and an empty one land on a 9-row canvas, overlapping rows summed."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_bands_worker, args=(r, 3, port, q)) for r in range(3)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    assert res[1] is None and res[2] is None, (res[1], res[2])
    exp = np.zeros((2, 9, 3), dtype=np.float32)
    exp[:, 0:5] += 1
    exp[:, 3:7] += 2
    assert np.array_equal(res[0], exp)
    # one process, no process group: the band is placed on the canvas
    from instageo_amd import distributed as D

    assert torch.equal(D.reduce_row_bands(torch.ones(1, 2, 2), [(1, 2)], 4), torch.tensor([[[0.0, 0], [1, 1], [1, 1], [0, 0]]]))
