"""mode=calibrate over two gloo ranks that share the device (-m gpu; the pattern of test_gpu_data_parallel.py): the integer reliability
histograms of the two-rank run equal the one-rank run exactly, the fitted temperature agrees to 1e-9 relative (the double sums of the
temperature grid are re-associated across ranks)."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON = ["model.model_name=prithvi_eo_tiny", "model.load_pretrained_weights=False", "train.ignore_index=-1", "model.num_classes=3",
          "train.class_weights=[1,2,1]", "valid_filepath=synthetic:5", "mode=calibrate"]


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _calibrate(ck, out_dir, rank, world):
    from instageo_amd import run
    from instageo_amd.config import load_config
    from instageo_amd.factory import create_model

    cfg = load_config("config", COMMON + [f"checkpoint_path={ck}"])
    return run.calibrate(cfg, create_model(cfg, device=DEV), out_dir, rank, world)


def _rank_worker(rank, world, port, ck, out_dir, q):
    import sys

    sys.path[:0] = [ROOT, os.path.join(ROOT, "instageo-e2e-geospatial-ml_amd")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist

    from instageo_amd import distributed as D

    try:
        D.init_from_env(backend="gloo")
        torch.cuda.set_device(0)
        q.put((rank, _calibrate(ck, out_dir, rank, world)))
    except Exception:  # pragma: no cover
        import traceback

        q.put((rank, traceback.format_exc()))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_two_gloo_ranks_equal_one_rank(tmp_path):
    """Five chips: three on rank 0, two on rank 1."""
    from instageo_amd.config import load_config
    from instageo_amd.factory import create_model

    mod = create_model(load_config("config", ["mode=train"] + COMMON[:5]), device=DEV)
    ck = str(tmp_path / "ck.ckpt")
    torch.save({"state_dict": mod.checkpoint_state_dict()}, ck)
    del mod
    os.makedirs(tmp_path / "two")
    os.makedirs(tmp_path / "one")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, ck, str(tmp_path / "two"), q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=600) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    assert res[1] is None and isinstance(res[0], dict), res
    two = res[0]
    one = _calibrate(ck, str(tmp_path / "one"), 0, 1)
    assert os.path.exists(tmp_path / "two" / "calibration.json") and os.path.exists(tmp_path / "one" / "calibration.json")
    assert two["n_valid"] == one["n_valid"] > 0
    assert two["bins_before"]["count"] == one["bins_before"]["count"]  # integer sums: exact, and so is every ratio taken from them
    for k in ("ece_before", "mce_before", "classwise_ece_before"):
        assert two[k] == one[k], k
    assert str(two["bins_before"]) == str(one["bins_before"])
    assert abs(two["temperature"] - one["temperature"]) <= 1e-9 * one["temperature"]
    assert abs(two["nll_before"] - one["nll_before"]) <= 1e-12 * abs(one["nll_before"])
    if two["temperature"] == one["temperature"]:  # the same temperature bit for bit: then the second histogram is the same too
        assert str(two["bins_after"]) == str(one["bins_after"]) and two["ece_after"] == one["ece_after"]
