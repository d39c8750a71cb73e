"""Mosaic paste: HIP-event times of ``ig_mosaic_paste`` on 256 chips of 256 x 256 on a 4096 x 4096 canvas, the numpy twin's wall time on
the same inputs, and the wall time of ``merge_predictions`` split into its phases.

    python tools/mosaic_bench.py [--reps 20] [--out profiles/mosaic_paste.txt]

Layouts: ``grid`` = a 16 x 16 grid without overlap; ``dates`` = 128 places (the upper half of the canvas) with two dates each, so every
covered pixel has two candidates and the lower half stays fill.  Class maps: 32 x 32 blocks of one of three classes with 5 % fill pixels
(for the files of merge_predictions: with a quarter of the blocks fill instead); floats: uniform values with 5 % NaN.  The kernel is launched ``--reps`` times back to back between two HIP events after a warm-up launch,
through the generated custom op on tensors that are already on the device; bytes = the chips read once + the canvas written, the rate is
held against the 4.78 TB/s copy rate of profiles/r03_hbm_ceiling.txt.  IG_MOSAIC_VEC=0 repeats the int8 ``last`` run without 16-byte loads.
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "instageo-e2e-geospatial-ml_amd"))
COPY_TBS = 4.78
N, C, S = 256, 256, 4096


def inputs(layout, dtype, seed=0, salt=True):
    rng = np.random.default_rng(seed)
    if layout == "grid":
        rects = [(C * (i // 16), C * (i % 16), C, C) for i in range(N)]
    else:
        rects = [(C * ((i % 128) // 16), C * (i % 16), C, C) for i in range(N)]
    chips = []
    for _ in range(N):
        if dtype == "int8":
            a = np.kron(rng.integers(0 if salt else -1, 3, size=(C // 32, C // 32)), np.ones((32, 32), dtype=np.int64)).astype(np.int8)
            if salt:
                a[rng.random((C, C)) < 0.05] = -1
        else:
            a = rng.random((C, C)).astype(np.float32)
            a[rng.random((C, C)) < 0.05] = np.nan
        chips.append(a)
    return chips, np.array(rects, dtype=np.int32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from instageo_amd import mosaic, ops, tiff, torch_ops

    torch_ops.register()
    op = torch.ops.instageo_mi355x.mosaic_paste
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"ig_mosaic_paste: {N} chips of {C} x {C} on a {S} x {S} canvas, {args.reps} launches back to back after a warm-up")
    for dtype, rules in (("int8", ("last", "first", "mode")), ("float32", ("mean",))):
        for layout in ("grid", "dates"):
            chips, rects = inputs(layout, dtype)
            es = chips[0].dtype.itemsize
            sizes = rects[:, 2].astype(np.int64) * rects[:, 3]
            ptr, idx = mosaic.bins(rects, S, S)
            dev = [torch.from_numpy(a).cuda() for a in (np.concatenate([c.reshape(-1) for c in chips]), np.cumsum(sizes) - sizes, rects, ptr, idx)]
            dst = torch.empty((S, S), dtype=dev[0].dtype, device="cuda")
            for rule in rules:
                for vec in (("1", "0") if (dtype, rule) == ("int8", "last") else ("1",)):
                    os.environ["IG_MOSAIC_VEC"] = vec
                    call = lambda: op(dev[0], dev[1], dev[2], N, dev[3], dev[4], S, S, es, ops.MOSAIC_RULES[rule], -1, dst, None)  # noqa: E731
                    call()
                    torch.cuda.synchronize()
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(args.reps):
                        call()
                    b.record()
                    torch.cuda.synchronize()
                    us = a.elapsed_time(b) * 1e3 / args.reps
                    nbytes = es * (N * C * C + S * S)
                    tbs = nbytes / us / 1e6
                    t0 = time.perf_counter()
                    host = mosaic.paste(chips, rects, (S, S), rule) if vec == "1" else None
                    twin = time.perf_counter() - t0
                    same = "" if host is None else f", numpy twin {twin * 1e3:.0f} ms, equal {bool(np.array_equal(host.view(f'u{es}'), dst.cpu().numpy().view(f'u{es}')))}"
                    emit(f"  {dtype:7s} {layout:5s} {rule:5s} vec={vec}: {us:8.1f} us, {nbytes / 1e6:6.1f} MB, {tbs:5.2f} TB/s = {100 * tbs / COPY_TBS:4.1f} % of copy{same}")
    os.environ["IG_MOSAIC_VEC"] = "1"
    # files -> files: the phases of merge_predictions on the int8 layouts (uncompressed strip files, as chip inference writes them)
    tags = lambda r, c: {33550: (12, (30.0, 30.0, 0.0)), 33922: (12, (0.0, 0.0, 0.0, 399960.0 + 30.0 * c, 4500000.0 - 30.0 * r, 0.0)),  # noqa: E731
                         34735: (3, (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 32613))}
    for layout in ("grid", "dates"):
        chips, rects = inputs(layout, "int8", salt=False)  # whole blocks of fill: the regions stay few, the tables small
        with tempfile.TemporaryDirectory() as tmp:
            src = os.path.join(tmp, "predictions")
            os.makedirs(src)
            for i, (a, (r, c, _, _)) in enumerate(zip(chips, rects.tolist())):
                tiff.write(os.path.join(src, f"prediction_{i:04d}.tif"), a, {"tags": tags(r, c)})
            for label, kw in (("raster only", {}), ("regions + polygons", dict(save_regions=True, save_polygons=True))):
                for device in ("gpu", "cpu") if not kw else ("gpu",):
                    t0 = time.perf_counter()
                    mosaic.merge_predictions(src, os.path.join(tmp, f"out_{device}_{len(kw)}"), num_classes=3, device=device, **kw)
                    wall = time.perf_counter() - t0
                    t = mosaic.TIMINGS
                    emit(f"  merge_predictions {layout:5s} {device} {label}: {wall:6.2f} s = read {t['read']:.2f} + paste (pack, upload, kernel) "
                         f"{t['paste']:.2f} + products {t['products']:.2f} + COG write {t['write']:.2f}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
