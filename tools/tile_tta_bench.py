"""Test-time augmentation of blended tile inference on a full tile (Prithvi-100M, bf16, batch 108): windows/s for
tta = none | flips | d4 and the time in the three TTA / uncertainty kernels per tile.

    python tools/tile_tta_bench.py [--stride 224] [--reps 3] [--out profiles/tile_tta_bench.json]

Timing: a resident 6 x 10980 x 10980 int16 tile; one warm-up pass of each mode, then ``--reps`` passes alternating the modes (gaussian,
no cover_edges, no probability raster), each ending in a device synchronise; windows/s = windows / median pass time.  ``tta=none`` is
the plain blended path (``ig_window_blend_accumulate``), so ``expected`` = its time x K is what K forward passes per window cost without
the transforms, and ``over_expected`` the share the TTA path adds to that.  Kernel time: one more pass per mode with HIP events around
every launch of ``ig_d4_apply``, ``ig_window_blend_accumulate_tta`` and ``ig_window_blend_uncertainty`` (``ops.profile_begin``; the
events drain the queue, so this pass is not the timed one), reported per tile with the achieved GB/s of the wrappers' byte counts.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "instageo-e2e-geospatial-ml_amd"))

MEAN = [0.14245495, 0.13921481, 0.12434631, 0.31420089, 0.20743526, 0.12046503]
STD = [0.04036231, 0.04186983, 0.05267646, 0.0822221, 0.06834774, 0.05294205]
MODES = ("none", "flips", "d4")
ENTRIES = ("ig_d4_apply", "ig_window_blend_accumulate_tta", "ig_window_blend_uncertainty", "ig_window_blend_accumulate")


def run(args):
    import torch

    from instageo_amd import ops
    from instageo_amd.dataloader import d4_codes, window_grid
    from instageo_amd.infer_utils import blended_window_inference
    from instageo_amd.model import PrithviSeg

    dev = "cuda"
    net = PrithviSeg(temporal_step=1, num_classes=2, load_pretrained_weights=False, freeze_backbone=True, variant="prithvi_eo_v1_100",
                     precision="bf16", device=dev)
    S, B = args.tile_size, args.batch
    tile = torch.randint(0, 10000, (6, S, S), generator=torch.Generator(device=dev).manual_seed(7), device=dev, dtype=torch.int16)
    tops, lefts = window_grid(S, S, 224, args.stride)
    n = len(tops) * len(lefts)

    def one(tta, uncertainty=False):
        return blended_window_inference(tile, net, MEAN, STD, 1, 224, args.stride, batch_size=B, constant_multiplier=1e-4, blend="gaussian",
                                        cover_edges=False, tta=tta, uncertainty=uncertainty)

    times = {m: [] for m in MODES}
    for m in MODES:  # warm-up: workspaces of every batch size
        one(m)
    torch.cuda.synchronize()
    for _ in range(args.reps):
        for m in MODES:
            t0 = time.perf_counter()
            res = one(m)
            torch.cuda.synchronize()
            times[m].append(time.perf_counter() - t0)
            del res
    out = {"workload": f"resident 6x{S}x{S} int16 tile, prithvi_eo_v1_100 bf16, batch {B}, crop 224, stride {args.stride}", "windows": n,
           "modes": {}}
    base = statistics.median(times["none"])
    for m in MODES:
        K, t = len(d4_codes(m)), statistics.median(times[m])
        row = {"K": K, "windows_per_s": round(n / t, 1), "images_per_s": round(n * K / t, 1), "seconds": [round(x, 4) for x in times[m]],
               "expected_seconds": round(base * K, 4), "over_expected": round(t / (base * K) - 1.0, 4)}
        ops.profile_begin(ENTRIES)
        res = one(m, uncertainty=True)
        prof = ops.profile_end()["ops"]
        del res
        row["kernels_ms_per_tile"] = {e: {"launches": c, "ms": round(ms, 3), "GBps": round(w / (ms * 1e-3) / 1e9, 1) if ms > 0 else None}
                                      for e, (c, ms, w) in prof.items() if c}
        new_ms = sum(v["ms"] for e, v in row["kernels_ms_per_tile"].items() if e != "ig_window_blend_accumulate")
        row["new_kernels_share_of_pass"] = round(new_ms * 1e-3 / t, 4)
        out["modes"][m] = row
        print(json.dumps({"tta": m, **row}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--stride", type=int, default=224)
    ap.add_argument("--tile-size", type=int, default=10980)
    ap.add_argument("--batch", type=int, default=108)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = run(args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
