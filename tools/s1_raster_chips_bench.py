"""Sentinel-1 chips on label grids: HIP-event time of ``ig_s1_chip_warp`` for 196 label grids of 256 x 256 x (3 dates x 2 bands) over three
synthetic 10 m RTC scenes of 11000 x 11000 pixels, with int8 label maps and the class histogram: the label grids once in the scenes' UTM
zone (the affine path) and once in EPSG:4326 (the projection path for every scene), next to a device copy of the same output bytes and to
``ig_s1_chip_cut`` on the same number of values in both of its cases (one zone; the second date in the next zone), measured in the same
session.

    python tools/s1_raster_chips_bench.py [--reps 10] [--out FILE]
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
    from instageo_amd import crs, s1_chips, s1_raster_chips, torch_ops

    torch_ops.register()
    ns = torch.ops.instageo_mi355x
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731

    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    side, S, T, C, n, K = 11000, 256, 3, 2, 196, 8
    u36, u37, geo = crs.from_epsg(32636), crs.from_epsg(32637), crs.from_epsg(4326)
    x0, y0 = 600000.0, 4500000.0
    gen = torch.Generator(device="cuda").manual_seed(1)
    planes = torch.rand(T * C * side * side, generator=gen, device="cuda", dtype=torch.float32)
    planes[torch.randint(0, planes.shape[0], (planes.shape[0] // 64,), generator=gen, device="cuda")] = float("nan")
    starts = np.arange(T * C, dtype=np.int64) * side * side
    corners = [(x0, y0), (x0 + 300.0, y0 - 500.0), (x0 - 200.0, y0 + 100.0)]
    stack = (x0 - 200.0, y0 + 100.0, 10.0, 10.0)
    origins = [(400 + 700 * (i // 14), 400 + 700 * (i % 14)) for i in range(n)]  # 14 x 14 chips spread over the scenes
    one_zone = [(cx, cy, 10.0, 10.0) for cx, cy in corners]
    tx, ty = crs.transform(u36, u37, np.array([corners[1][0]]), np.array([corners[1][1]]))
    two_zones = [one_zone[0], (float(tx[0]) + 3.3, float(ty[0]) - 4.1, 10.0, 10.0), one_zone[2]]
    written = n * T * C * S * S * 4 + n * S * S
    emit(f"{torch.cuda.get_device_name(0)}; {n} chips of {S} x {S} x ({T} dates x {C} bands) float32 from {T} scenes of {side} x {side}; best of {args.reps}")
    dst = torch.empty(written, dtype=torch.uint8, device="cuda")
    src = torch.empty_like(dst)
    copy_us = timed(lambda: dst.copy_(src), args.reps)
    emit(f"  device copy of the {written / 1e6:.1f} MB of chips and validity: {copy_us:8.1f} us")
    out = torch.empty((n, T * C, S, S), dtype=torch.float32, device="cuda")
    plane = torch.empty((n, S, S), dtype=torch.uint8, device="cuda")
    valid_values = torch.zeros(n, dtype=torch.int32, device="cuda")

    # the yardsticks: ig_s1_chip_cut in its two cases
    yard = {}
    for what, systems, grids in (("one zone (affine)", [u36] * 3, one_zone), ("the second date in the next zone", [u36, u37, u36], two_zones)):
        st, sc, sg, ss, bits, _, _, dc, dg, o, nd, _, _ = s1_chips.check_cut(planes.shape[0], starts, systems, grids, [(side, side)] * 3, [1, 1, 1], u36,
                                                                             stack, origins, S, -1.0, None, None)
        tab = [dev(a) for a in (st, sc, sg, ss, dc, dg, o)]
        run = lambda: ns.s1_chip_cut(planes, tab[0], tab[1], tab[2], tab[3], 3, bits, tab[4], tab[5], tab[6], n, T, C, S, float(nd), 0, 0.0, 0, 0.0,  # noqa: E731
                                     0.0, out, valid_values, plane)
        yard[what] = timed(run, args.reps)
        emit(f"  ig_s1_chip_cut, {what}: {yard[what]:8.1f} us = {yard[what] / copy_us:5.2f} x the copy's time")

    # the label grids: the chips of the yardstick as windows of the stack lattice, and the same places at 0.00009 degrees
    labels = torch.randint(-1, K + 2, (n, S, S), generator=gen, device="cuda", dtype=torch.int8)
    maps = torch.empty_like(labels)
    valid_labels = torch.zeros(n, dtype=torch.int32, device="cuda")
    hist = torch.zeros((n, K), dtype=torch.int32, device="cuda")
    utm_grids = [(stack[0] + 10.0 * c, stack[1] - 10.0 * r, 10.0, 10.0) for r, c in origins]
    lon, lat = crs.transform(u36, geo, np.array([g[0] for g in utm_grids]), np.array([g[1] for g in utm_grids]))
    geo_grids = [(float(a), float(b), 0.00009, 0.00009) for a, b in zip(lon, lat)]
    for what, dst_crs, grids, against in (("label grids in the scenes' zone (affine)", u36, utm_grids, "one zone (affine)"),
                                          ("label grids in EPSG:4326 (projection)", geo, geo_grids, "the second date in the next zone")):
        for with_labels in (True, False):
            st, sc, sg, ss, bits, _, _, dc, dg, nd, _, _ = s1_raster_chips.check_warp(planes.shape[0], starts, [u36] * 3, one_zone, [(side, side)] * 3,
                                                                                     [1, 1, 1], dst_crs, grids, S, -1.0, None, None,
                                                                                     (n, S, S) if with_labels else None, "int8" if with_labels else None,
                                                                                     2 if with_labels else 0, K if with_labels else 0)
            tab = [dev(a) for a in (st, sc, sg, ss, dc, dg)]
            lab = (labels, 1, 2, K, maps, valid_labels, hist) if with_labels else (None, 1, 0, 0, None, None, None)
            run = lambda: ns.s1_chip_warp(planes, tab[0], tab[1], tab[2], tab[3], 3, bits, tab[4], tab[5], n, T, C, S, float(nd), 0, 0.0, 0, 0.0, 0.0,  # noqa: E731
                                          lab[0], lab[1], lab[2], lab[3], out, valid_values, plane, lab[4], lab[5], lab[6])
            us = timed(run, args.reps)
            valid_values.zero_()
            run()
            valid = int(valid_values.sum().item())
            extra = 2 * n * S * S if with_labels else 0
            emit(f"  ig_s1_chip_warp, {what}, {'int8 labels + histogram' if with_labels else 'no labels'}: {us:8.1f} us = "
                 f"{us / copy_us:5.2f} x the copy's time, {us / yard[against]:5.2f} x ig_s1_chip_cut ({against}); "
                 f"{(written + extra) / us / 1e6:5.2f} TB/s stored and label bytes; {valid} valid values")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
