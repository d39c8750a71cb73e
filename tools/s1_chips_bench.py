"""Sentinel-1 chips: HIP-event time of ``ig_s1_chip_cut`` for 196 chips of 256 x 256 x (3 dates x 2 bands) from three synthetic 10 m RTC
scenes of 11000 x 11000 pixels, every scene in the stack's UTM zone (the affine path) and with the second date in the next zone (the
projection path), next to a device copy of the same output bytes and to ``ig_chip_cut`` on the same number of values.

    python tools/s1_chips_bench.py [--reps 10] [--out profiles/s1_chips.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "instageo-e2e-geospatial-ml_amd"))


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) * 1e3)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from instageo_amd import crs, s1_chips, torch_ops

    torch_ops.register()
    ns = torch.ops.instageo_mi355x
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731

    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    side, S, T, C, n = 11000, 256, 3, 2, 196
    u36, u37 = crs.from_epsg(32636), crs.from_epsg(32637)
    x0, y0 = 600000.0, 4500000.0
    gen = torch.Generator(device="cuda").manual_seed(1)
    planes = torch.rand(T * C * side * side, generator=gen, device="cuda", dtype=torch.float32)
    planes[torch.randint(0, planes.shape[0], (planes.shape[0] // 64,), generator=gen, device="cuda")] = float("nan")
    starts = np.arange(T * C, dtype=np.int64) * side * side
    corners = [(x0, y0), (x0 + 300.0, y0 - 500.0), (x0 - 200.0, y0 + 100.0)]
    grid = (x0 - 200.0, y0 + 100.0, 10.0, 10.0)
    origins = [(400 + 700 * (i // 14), 400 + 700 * (i % 14)) for i in range(n)]  # 14 x 14 chips spread over the scenes
    tx, ty = crs.transform(u36, u37, np.array([corners[1][0]]), np.array([corners[1][1]]))
    next_zone = (float(tx[0]) + 3.3, float(ty[0]) - 4.1, 10.0, 10.0)
    written = n * T * C * S * S * 4 + n * S * S
    emit(f"{torch.cuda.get_device_name(0)}; {n} chips of {S} x {S} x ({T} dates x {C} bands) float32 from {T} scenes of {side} x {side}; best of {args.reps}")
    dst = torch.empty(written, dtype=torch.uint8, device="cuda")
    src = torch.empty_like(dst)
    copy_us = timed(lambda: dst.copy_(src), args.reps)
    emit(f"  device copy of the {written / 1e6:.1f} MB written: {copy_us:8.1f} us")
    tile = torch.randint(1, 3000, (T * C, 3660, 3660), dtype=torch.int16, device="cuda", generator=gen)
    o16 = [(10 + 240 * (i // 14), 10 + 240 * (i % 14)) for i in range(n)]
    o16, c16 = dev(np.array(o16, dtype=np.int32)), torch.empty((n, T * C, S, S), dtype=torch.int16, device="cuda")
    v16, p16 = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.empty((n, S, S), dtype=torch.uint8, device="cuda")
    cut_us = timed(lambda: ns.chip_cut(tile, None, o16, n, T, C, 3660, 3660, S, 0, 0, 0, 0, 0, 0, c16, v16, p16), args.reps)
    emit(f"  ig_chip_cut, the same number of values (int16): {cut_us:8.1f} us = {cut_us / copy_us:5.2f} x the copy's time")
    out = torch.empty((n, T * C, S, S), dtype=torch.float32, device="cuda")
    plane = torch.empty((n, S, S), dtype=torch.uint8, device="cuda")
    for what, systems, grids in (("one zone (affine)", [u36] * 3, [(cx, cy, 10.0, 10.0) for cx, cy in corners]),
                                 ("the second date in the next zone", [u36, u37, u36], [(*corners[0], 10.0, 10.0), next_zone, (*corners[2], 10.0, 10.0)])):
        st, sc, sg, ss, bits, _, _, dc, dg, o, nd, _, _ = s1_chips.check_cut(planes.shape[0], starts, systems, grids, [(side, side)] * 3, [1, 1, 1], u36,
                                                                             grid, origins, S, -1.0, None, None)
        tab = [dev(a) for a in (st, sc, sg, ss, dc, dg, o)]
        valid_values = torch.zeros(n, dtype=torch.int32, device="cuda")
        run = lambda: ns.s1_chip_cut(planes, tab[0], tab[1], tab[2], tab[3], 3, bits, tab[4], tab[5], tab[6], n, T, C, S, float(nd), 0, 0.0, 0, 0.0,  # noqa: E731
                                     0.0, out, valid_values, plane)
        us = timed(run, args.reps)
        valid_values.zero_()
        run()
        valid = int(valid_values.sum().item())
        emit(f"  ig_s1_chip_cut, {what}: {us:8.1f} us = {us / copy_us:5.2f} x the copy's time, "
             f"{us / cut_us:5.2f} x ig_chip_cut; {written / us / 1e6:5.2f} TB/s stored; {valid} valid values")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
