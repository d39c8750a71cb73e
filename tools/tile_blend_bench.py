"""Blended tile inference against the legacy nearest-centre path on a full tile (Prithvi-100M, bf16, batch 108).

    python tools/tile_blend_bench.py [--strides 224 112] [--reps 3] [--out profiles/tile_blend_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -o tb -- python tools/tile_blend_bench.py --reps 1 --no-legacy
    python tools/tile_blend_bench.py --report DIR/.../tb_kernel_stats.csv [--out profiles/tile_blend_kernels.json]

Timing: a resident 6 x 10980 x 10980 int16 tile; per stride, one warm-up pass of each path, then ``--reps`` passes alternating
legacy (``sliding_window_inference`` + ``stitch_windows``) and blended (``blended_window_inference``, gaussian, no cover_edges, no
probability raster), each ending in a device synchronise; windows/s = windows / median pass time.
``--report``: the two blend kernels' time per tile from a rocprofv3 stats CSV, and their HBM bytes (``blend_bytes``, from the
window grid) over that time against the 6.3 TB/s ceiling.
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "instageo-e2e-geospatial-ml_amd"))

import numpy as np  # noqa: E402

MEAN = [0.14245495, 0.13921481, 0.12434631, 0.31420089, 0.20743526, 0.12046503]
STD = [0.04036231, 0.04186983, 0.05267646, 0.0822221, 0.06834774, 0.05294205]
HBM_TBPS = 6.3
KERNELS = ("window_blend_accumulate_kernel", "window_blend_finalize_kernel")


def batches(n: int, batch: int):
    """sliding_window_inference's balanced batches: [(first window, count)]."""
    nb = max(1, -(-n // batch))
    bs = -(-n // nb) if n else 1
    return [(i, min(bs, n - i)) for i in range(0, n, bs)]


def blend_bytes(S: int, crop: int, stride: int, batch: int, ncls: int = 2):
    """HBM bytes of one tile: accumulate = every batch's logits (read once) + one read and one write of acc (ncls planes) and
    wsum at every pixel a batch window covers; finalize = acc + wsum read, int8 class map written (no NODATA test, no probabilities)."""
    from instageo_amd.dataloader import window_grid

    tops, lefts = window_grid(S, S, crop, stride)
    nc = len(lefts)
    acc = 0
    for w0, k in batches(len(tops) * nc, batch):
        y0 = tops[w0 // nc]
        mask = np.zeros((tops[(w0 + k - 1) // nc] + crop - y0, S), dtype=bool)  # canvas pixels this batch covers
        for w in range(w0, w0 + k):
            t, l = tops[w // nc] - y0, lefts[w % nc]
            mask[t : t + crop, l : l + crop] = True
        acc += k * ncls * crop * crop * 4 + int(mask.sum()) * (ncls + 1) * 8
    fin = S * S * ((ncls + 1) * 4 + 1)
    return {"accumulate": acc, "finalize": fin, "windows": len(tops) * nc}


def run(args):
    import torch

    from instageo_amd.infer_utils import blended_window_inference, sliding_window_inference, stitch_windows
    from instageo_amd.model import PrithviSeg

    dev = "cuda"
    net = PrithviSeg(temporal_step=1, num_classes=2, load_pretrained_weights=False, freeze_backbone=True, variant="prithvi_eo_v1_100",
                     precision="bf16", device=dev)
    S, B = args.tile_size, args.batch
    tile = torch.randint(0, 10000, (6, S, S), generator=torch.Generator(device=dev).manual_seed(7), device=dev, dtype=torch.int16)

    def legacy(stride):
        maps, origins = sliding_window_inference(tile, net, MEAN, STD, 1, 224, stride, batch_size=B, constant_multiplier=1e-4)
        return stitch_windows(maps, origins, S)

    def blended(stride):
        return blended_window_inference(tile, net, MEAN, STD, 1, 224, stride, batch_size=B, constant_multiplier=1e-4, blend="gaussian",
                                        cover_edges=False)[0]

    out = {"workload": f"resident 6x{S}x{S} int16 tile, prithvi_eo_v1_100 bf16, batch {B}, crop 224", "strides": {}}
    for stride in args.strides:
        paths = [("blended", blended)] if args.no_legacy else [("legacy", legacy), ("blended", blended)]
        times = {name: [] for name, _ in paths}
        for name, fn in paths:  # warm-up: workspaces of every batch size
            fn(stride)
        torch.cuda.synchronize()
        for _ in range(args.reps):
            for name, fn in paths:
                t0 = time.perf_counter()
                res = fn(stride)
                torch.cuda.synchronize()
                times[name].append(time.perf_counter() - t0)
                del res
        n = blend_bytes(S, 224, stride, B)["windows"]
        row = {name: {"windows_per_s": round(n / statistics.median(t), 1), "seconds": [round(x, 4) for x in t]} for name, t in times.items()}
        row["windows"] = n
        if "legacy" in row:
            row["blended_vs_legacy"] = round(row["blended"]["windows_per_s"] / row["legacy"]["windows_per_s"] - 1.0, 4)
        out["strides"][str(stride)] = row
        print(json.dumps({"stride": stride, **row}), flush=True)
    return out


def report(args):
    """Kernel stats CSV of a ``--reps 1 --no-legacy`` run: warm-up + 1 timed pass per stride = 2 tiles per stride."""
    rows = list(csv.DictReader(open(args.report)))
    tiles = 2 * len(args.strides)
    out = {"source": os.path.basename(args.report), "tiles_in_trace": tiles, "hbm_ceiling_TBps": HBM_TBPS, "kernels": {}}
    for r in rows:
        name = r["Name"]
        for k in KERNELS:
            if k in name:
                out["kernels"][k] = {"calls": int(r["Calls"]), "total_ms": float(r["TotalDurationNs"]) / 1e6}
    # per stride the trace cannot separate the two strides' launches: bytes and time are summed over all traced tiles
    nbytes = {"accumulate": 0, "finalize": 0}
    for s in args.strides:
        b = blend_bytes(args.tile_size, 224, s, args.batch)
        nbytes["accumulate"] += 2 * b["accumulate"]
        nbytes["finalize"] += 2 * b["finalize"]
    for short, k in zip(("accumulate", "finalize"), KERNELS):
        if k in out["kernels"]:
            d = out["kernels"][k]
            d["ms_per_tile"] = round(d["total_ms"] / tiles, 3)
            d["bytes"] = nbytes[short]
            d["TBps"] = round(nbytes[short] / (d["total_ms"] * 1e-3) / 1e12, 2)
            d["share_of_hbm_ceiling"] = round(d["TBps"] / HBM_TBPS, 3)
    print(json.dumps(out, indent=1))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--strides", type=int, nargs="+", default=[224, 112])
    ap.add_argument("--tile-size", type=int, default=10980)
    ap.add_argument("--batch", type=int, default=108)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-legacy", action="store_true", help="blended path only (the kernel-trace run)")
    ap.add_argument("--report", default=None, help="rocprofv3 kernel_stats.csv -> blend kernel time and bandwidth")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = report(args) if args.report else run(args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
