"""mode=eval with test.object_metrics over two gloo ranks that share the device (-m gpu; the pattern of test_gpu_boundary_ranks.py):
chips are whole on one rank, so the reduced integer tables of the two-rank run, and every ratio logged from them, equal the one-rank
run exactly."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON = ["model.model_name=prithvi_eo_tiny", "model.load_pretrained_weights=False", "train.ignore_index=-1", "model.num_classes=3",
          "train.class_weights=[1,2,1]", "test_filepath=synthetic:5", "mode=eval", "test.object_metrics=true",
          "test.object_iou_thresholds=[0.5,0.75]"]
MARKS = ("_obj_", "_PQ_", "_SQ_", "_RQ_")


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _evaluate(ck, rank, world):
    """-> (the logged test_* values, the four tables as they stand when the epoch ends: after the rank reduction)."""
    from instageo_amd import run
    from instageo_amd.config import load_config
    from instageo_amd.factory import create_model

    cfg = load_config("config", COMMON + [f"checkpoint_path={ck}"])
    model = create_model(cfg, device=DEV)
    counts = []
    epoch_end = model.on_test_epoch_end

    def keep_counts():
        counts.extend(c.cpu().numpy() for c in model.test_objects.device_counts())
        epoch_end()

    model.on_test_epoch_end = keep_counts
    return run.evaluate(cfg, model, rank, world), counts


def _rank_worker(rank, world, port, ck, q):
    import sys

    sys.path[:0] = [ROOT, os.path.join(ROOT, "instageo-e2e-geospatial-ml_amd")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist

    from instageo_amd import distributed as D

    try:
        D.init_from_env(backend="gloo")
        torch.cuda.set_device(0)
        q.put((rank, _evaluate(ck, rank, world)))
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
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, ck, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=600) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    assert all(isinstance(res[r], tuple) for r in range(2)), res
    one_log, one_counts = _evaluate(ck, 0, 1)
    keys = [k for k in one_log if any(m in k for m in MARKS)]
    assert len(keys) == 2 * (6 + 2 * 3) and int(one_counts[2].sum()) > 0 and int(one_counts[3].sum()) > 0
    for r in range(2):  # the all-reduce leaves the sums on every rank
        log, counts = res[r]
        assert len(counts) == 4 and all(np.array_equal(a, b) for a, b in zip(counts, one_counts)), r
        assert str({k: log[k] for k in keys}) == str({k: one_log[k] for k in keys}), r
