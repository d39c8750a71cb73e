"""Warp: HIP-event times of ``ig_warp`` on a 4096 x 4096 destination, the numpy host path's wall time on the same inputs, and the wall time
of ``merge_reprojected`` split into its phases.

    python tools/warp_bench.py [--reps 20] [--out profiles/warp.txt]

Cases: (1) int8 nearest from two UTM zones (two 2300 x 4200 sources of EPSG:32636 / 32637 that overlap at 36 E onto an EPSG:32636 canvas);
(2) the same as float32 bilinear; (3) the same-system shortcut (both sources in the canvas's system: affine arithmetic only); and
``ig_warp_coords`` alone, which is the projections without the gather.  The kernel is launched ``--reps`` times back to back between two HIP
events after a warm-up launch, through the generated custom op on tensors that are already on the device.  Bytes = the destination written
+ as many source pixels gathered (x4 neighbours for bilinear hit the caches); the rate is held against the 4.78 TB/s copy rate of
profiles/r03_hbm_ceiling.txt.  The other floor is float64 arithmetic: a reprojected pixel costs one inverse and one forward transverse
Mercator projection, counted below as float64 operations per pixel from the source (transcendentals as one each), so pixels / s shows
which floor binds.
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "instageo-e2e-geospatial-ml_amd"))
COPY_TBS = 4.78
S = 4096
U36 = (1.0, 33.0, 0.9996, 500000.0, 0.0)
U37 = (1.0, 39.0, 0.9996, 500000.0, 0.0)


def inputs(dtype, same, seed=0):
    """Two sources that share a 400-pixel band of the canvas -> (arrays, systems, grids, dst system, dst grid)."""
    from instageo_amd import crs

    rng = np.random.default_rng(seed)
    x36, y36 = (30.0 * round(float(v) / 30.0) for v in crs.forward(U36, 36.0, 40.6))
    x37, y37 = (30.0 * round(float(v) / 30.0) for v in crs.forward(U37, 36.0, 40.6))
    dgrid = (x36 - 30.0 * 2048, y36 + 30.0 * 2048, 30.0, 30.0)
    h, w = 4200, 2300
    arrays = []
    for _ in range(2):
        if dtype == "int8":
            a = np.kron(rng.integers(0, 3, size=(h // 100, w // 100)), np.ones((100, 100), dtype=np.int64)).astype(np.int8)
            a[rng.random((h, w)) < 0.05] = -1
        else:
            a = rng.random((h, w)).astype(np.float32)
            a[rng.random((h, w)) < 0.05] = np.nan
        arrays.append(a)
    if same:
        systems = [U36, U36]
        grids = [(x36 - 30.0 * 2100 + 7.0, y36 + 30.0 * 2100 - 11.0, 30.0, 30.0), (x36 - 30.0 * 200 + 7.0, y36 + 30.0 * 2100 - 11.0, 30.0, 30.0)]
    else:
        systems = [U36, U37]
        grids = [(x36 - 30.0 * 2100, y36 + 30.0 * 2100, 30.0, 30.0), (x37 - 30.0 * 200, y37 + 30.0 * 2100, 30.0, 30.0)]
    return arrays, systems, grids, U36, dgrid


def timed(call, reps):
    import torch

    call()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        call()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy host path (about a minute)")
    args = ap.parse_args()
    import torch

    from instageo_amd import ops, tiff, torch_ops, warp

    torch_ops.register()
    op, cop = torch.ops.instageo_mi355x.warp, torch.ops.instageo_mi355x.warp_coords
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"ig_warp: two 4200 x 2300 sources onto a {S} x {S} EPSG:32636 canvas, {args.reps} launches back to back after a warm-up")
    for label, dtype, resampling, same in (("two zones", "int8", "nearest", False), ("two zones", "float32", "bilinear", False),
                                           ("same system", "int8", "nearest", True), ("same system", "float32", "bilinear", True)):
        arrays, systems, grids, dcrs, dgrid = inputs(dtype, same)
        es = arrays[0].dtype.itemsize
        sizes = np.array([a.shape for a in arrays], dtype=np.int64)
        n = sizes[:, 0] * sizes[:, 1]
        t0 = time.perf_counter()
        ptr, idx = warp.block_lists(dcrs, dgrid, (S, S), systems, grids, sizes)
        t_lists = time.perf_counter() - t0
        up = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, dtype=t)).cuda()  # noqa: E731
        packed = torch.from_numpy(np.concatenate([a.reshape(-1) for a in arrays])).cuda()
        dev = [up(np.cumsum(n) - n, np.int64), up(np.array(systems).reshape(-1), np.float64), up(np.array(grids).reshape(-1), np.float64),
               up(sizes.reshape(-1), np.int32), up(ptr, np.int32), up(idx, np.int32), up(dcrs, np.float64), up(dgrid, np.float64)]
        dst = torch.empty((S, S), dtype=packed.dtype, device="cuda")
        call = lambda: op(packed, dev[0], dev[1], dev[2], dev[3], 2, dev[4], dev[5], dev[6], dev[7], S, S, es, ops.WARP_RESAMPLING[resampling], 0, -1, dst, None)  # noqa: E731
        us = timed(call, args.reps)
        covered = float((dst == dst).float().mean()) if dtype == "float32" else float((dst != -1).float().mean())
        nbytes = 2 * es * S * S
        tbs = nbytes / us / 1e6
        host = ""
        if not args.no_host:
            tags = lambda g, e: {"tags": {33550: (12, (g[2], g[3], 0.0)), 33922: (12, (0.0, 0.0, 0.0, g[0], g[1], 0.0)),  # noqa: E731
                                          34735: (3, (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, e))}}
            t0 = time.perf_counter()
            ref = warp.warp(arrays, [tags(g, 32636 if s == U36 else 32637) for g, s in zip(grids, systems)], tags(dgrid, 32636), (S, S), resampling)
            twin = time.perf_counter() - t0
            got = dst.cpu().numpy()
            if resampling == "nearest":
                diff = float((got.view(f"u{es}") != ref.view(f"u{es}")).mean())
            else:
                diff = float((np.isnan(got) != np.isnan(ref)).mean())
            host = f", numpy host path {twin:.1f} s, pixels that differ (ties) {diff:.1e}"
        emit(f"  {label:11s} {dtype:7s} {resampling:8s}: {us:8.1f} us, {S * S / us / 1e3:6.2f} Gpixel/s, {nbytes / 1e6:6.1f} MB, {tbs:5.2f} TB/s = "
             f"{100 * tbs / COPY_TBS:4.1f} % of copy, covered {covered:.2f}, block lists {t_lists * 1e3:.0f} ms{host}")
    uv = torch.empty((2, S, S), dtype=torch.float64, device="cuda")
    _, systems, grids, dcrs, dgrid = inputs("int8", False)
    dev = [torch.from_numpy(np.array(a, dtype=np.float64)).cuda() for a in (dcrs, dgrid, systems[1], grids[1], systems[0], grids[0])]
    for label, k in (("32636 -> 32637 (inverse + forward projection)", 2), ("same system (affine)", 4)):
        us = timed(lambda: cop(dev[0], dev[1], S, S, dev[k], dev[k + 1], uv), args.reps)
        emit(f"  ig_warp_coords {label}: {us:8.1f} us, {S * S / us / 1e3:6.2f} Gpixel/s, {16 * S * S / us / 1e6:5.2f} TB/s written")
    # files -> files: 2 x 64 chips of 512 x 512 from two zones
    from instageo_amd import crs

    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "predictions")
        os.makedirs(src)
        rng = np.random.default_rng(1)
        for epsg, system, col0 in ((32636, U36, -8), (32637, U37, 0)):
            x, y = (30.0 * round(float(v) / 30.0) for v in crs.forward(system, 36.0, 40.6))
            for i in range(64):
                a = np.kron(rng.integers(-1, 3, size=(16, 16)), np.ones((32, 32), dtype=np.int64)).astype(np.int8)
                t = {33550: (12, (30.0, 30.0, 0.0)), 33922: (12, (0.0, 0.0, 0.0, x + 15360.0 * (col0 + i % 8), y + 15360.0 * (4 - i // 8), 0.0)),
                     34735: (3, (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, epsg))}
                tiff.write(os.path.join(src, f"prediction_{epsg}_{i:03d}.tif"), a, {"tags": t})
        for device in ("gpu",) if args.no_host else ("gpu", "cpu"):
            t0 = time.perf_counter()
            out = warp.merge_reprojected(src, os.path.join(tmp, f"out_{device}"), num_classes=3, device=device)
            wall = time.perf_counter() - t0
            t = warp.TIMINGS
            shape = tiff.read(out[0])[0].shape[1:]
            emit(f"  merge_reprojected 128 chips of 512 x 512, two zones -> {shape[0]} x {shape[1]}, {device}: {wall:6.2f} s = read {t['read']:.2f} + paste "
                 f"{t['paste']:.2f} + warp (lists, upload, kernel) {t['warp']:.2f} + products {t['products']:.2f} + COG write {t['write']:.2f}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
