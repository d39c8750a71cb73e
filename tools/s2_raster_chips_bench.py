"""Sentinel-2 raster chips: HIP-event time of ``ig_s2_chip_warp`` on one synthetic L2A granule (3 dates x 6 bands: per date three planes of
10980 x 10980 at 10 m, two of 5490 x 5490 at 20 m and one of 1830 x 1830 at 60 m, uint16, with one 20 m SCL plane per date, built on the
device) warped onto ``--chips`` label grids of 256 x 256 at 10 m in the NEXT UTM zone, against (a) a device-to-device copy of the same
output bytes and (b) ``ig_chip_warp`` producing the same number of output values from a single-resolution int16 stack (18 x 3660 x 3660
at 30 m with an Fmask) on grids in the next zone.

    python tools/s2_raster_chips_bench.py [--reps 10] [--chips 300] [--out profiles/s2_raster_chips.txt]

Each kernel is launched ``--reps`` times back to back between two HIP events after a warm-up launch, through the generated custom op on
tensors that are already on the device.  A few chips are compared with the numpy host path.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "instageo-e2e-geospatial-ml_amd"))
T, C, S = 3, 6, 256
SIDES = (10980, 5490, 1830)
STEPS = (10.0, 20.0, 60.0)
X0, Y0 = 399960.0, 4500000.0  # the corner of a tile in UTM 36 N
HLS = 3660


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--chips", type=int, default=300)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from instageo_amd import crs, s2_chips, s2_raster_chips, torch_ops

    torch_ops.register()
    ns = torch.ops.instageo_mi355x
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def timed(call):
        call()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.reps):
            call()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / args.reps  # us

    g = torch.Generator(device="cuda").manual_seed(0)
    classes = [0, 0, 0, 1, 1, 2] * T
    sides = [SIDES[k] for k in classes]
    starts = np.concatenate([[0], np.cumsum([h * h for h in sides])[:-1]]).astype(np.int64)
    raw = torch.empty(int(sum(h * h for h in sides)), dtype=torch.int16, device="cuda")
    for k, h in enumerate(sides):  # plane by plane: the random draws stay small
        seg = raw[int(starts[k]) : int(starts[k]) + h * h]
        seg.copy_(torch.randint(1, 11000, (h * h,), generator=g, device="cuda", dtype=torch.int16))
        seg[torch.rand(h * h, generator=g, device="cuda") < 0.02] = 0
    bands = raw.view(torch.uint16)
    kinds = torch.tensor([4, 4, 4, 5, 6, 8, 9, 3, 10], dtype=torch.uint8, device="cuda")
    half = SIDES[1]
    coarse = kinds[torch.randint(0, len(kinds), (T, -(-half // 32), -(-half // 32)), generator=g, device="cuda")]
    scl = coarse.repeat_interleave(32, 1).repeat_interleave(32, 2)[:, :half, :half].contiguous().reshape(-1)
    scl_starts = np.arange(T, dtype=np.int64) * half * half
    plane_class = classes + [1] * T
    class_grid = np.array([(X0, Y0, p, p) for p in STEPS], dtype=np.float64)
    class_size = np.array([(h, h) for h in SIDES], dtype=np.int32)
    src, dst = crs.from_epsg(32636), crs.from_epsg(32637)
    sc, dc = np.array(tuple(src)[:5], dtype=np.float64), np.array(tuple(dst)[:5], dtype=np.float64)
    # label grids in the next zone: the top-left corners of random 10 m pixels of the tile, projected on the host, off the lattice
    rng = np.random.default_rng(0)
    n = args.chips
    r0, c0 = rng.integers(0, SIDES[0] - S, n), rng.integers(0, SIDES[0] - S, n)
    gx, gy = crs.transform(sc, dc, X0 + 10.0 * c0, Y0 - 10.0 * r0)
    grids = np.stack([gx + 3.3, gy - 2.7, np.full(n, 10.0), np.full(n, 10.0)], axis=1)
    dbl = torch.from_numpy(np.concatenate([sc, dc, class_grid.reshape(-1), grids.reshape(-1)])).cuda()
    ints = torch.from_numpy(np.concatenate([np.array(plane_class, dtype=np.int32), class_size.reshape(-1)])).cuda()
    P, G = len(plane_class), 3
    sd, ssd = torch.from_numpy(starts).cuda(), torch.from_numpy(scl_starts).cuda()
    labels = torch.randint(0, 3, (n, S, S), generator=g, device="cuda", dtype=torch.int8)
    out = torch.empty((n, T * C, S, S), dtype=torch.uint16, device="cuda")
    valid, vlab = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    hist = torch.zeros((n, 8), dtype=torch.int32, device="cuda")
    plane = torch.empty((n, S, S), dtype=torch.uint8, device="cuda")
    maps = torch.empty_like(labels)
    bits = s2_chips.scl_class_bits(["cloud", "water", "cloud_shadow"])
    px = n * S * S
    written = px * (2 * T * C + 2)  # the chips, the validity plane, the label map
    a_buf = torch.empty(written, dtype=torch.uint8, device="cuda")
    b_buf = torch.empty_like(a_buf)
    copy_us = timed(lambda: b_buf.copy_(a_buf))
    del a_buf, b_buf
    emit(f"s2 raster chips: {T} dates x (3 x {SIDES[0]}^2 + 2 x {SIDES[1]}^2 + {SIDES[2]}^2) uint16 + SCL {SIDES[1]}^2 in UTM 36 N -> {n} label grids of "
         f"{S} x {S} at 10 m in UTM 37 N, int8 labels with a histogram, {args.reps} launches back to back after a warm-up")
    emit(f"  device-to-device copy of the output bytes, {written / 1e6:.1f} MB: {copy_us:8.1f} us, {written / copy_us / 1e6:5.2f} TB/s stored")

    def s2(strategy, with_scl, boa, rng_on, lab=True):
        return lambda: ns.s2_chip_warp(bands, sd, scl if with_scl else None, ssd if with_scl else None, ints[:P], dbl[10 : 10 + 4 * G], ints[P:], G,
                                       dbl[0:5], dbl[5:10], dbl[10 + 4 * G :], n, T, C, S, bits, strategy, 0, boa, rng_on, 0, 10000,
                                       labels if lab else None, 1, 2 if lab else 0, 8 if lab else 0, out, valid, plane, maps if lab else None,
                                       vlab if lab else None, hist if lab else None)

    results = {}
    for what, call in (("each, SCL mask, range [0, 10000]", s2(0, True, 0, 1)), ("any , SCL mask, range [0, 10000]", s2(1, True, 0, 1)),
                       ("without SCL, boa_offset 1000, range", s2(0, False, 1000, 1)), ("each, SCL mask, range, no labels", s2(0, True, 0, 1, False))):
        us = results[what] = timed(call)
        emit(f"  ig_s2_chip_warp {what}: {us:8.1f} us = {us / copy_us:5.2f} x the copy's time; {written / us / 1e6:5.2f} TB/s stored")
    # the single-grid kernel on the same number of output values: an HLS stack in UTM 36 N, the same number of grids in UTM 37 N at 30 m
    tile = torch.randint(1, 11000, (T * C, HLS, HLS), generator=g, device="cuda", dtype=torch.int16)
    fmask = (torch.randint(0, 4, (T, HLS, HLS), generator=g, device="cuda", dtype=torch.uint8) == 0).to(torch.uint8) * 2
    hr, hc = rng.integers(0, HLS - S, n), rng.integers(0, HLS - S, n)
    hx, hy = crs.transform(sc, dc, X0 + 30.0 * hc, Y0 - 30.0 * hr)
    hgrids = np.stack([hx + 3.3, hy - 2.7, np.full(n, 30.0), np.full(n, 30.0)], axis=1)
    hd = torch.from_numpy(np.concatenate([sc, np.array([X0, Y0, 30.0, 30.0]), dc, hgrids.reshape(-1)])).cuda()
    hout = out.view(torch.int16)
    hls_us = timed(lambda: ns.chip_warp(tile, fmask, hd[0:5], hd[5:9], hd[9:14], hd[14:], n, T, C, HLS, HLS, S, 2 | 4 | 8 | 32, 0, 0, 1, 0, 10000, labels,
                                        1, 2, 8, hout, valid, plane, maps, vlab, hist))
    emit(f"  ig_chip_warp, one {T * C} x {HLS}^2 int16 stack at 30 m with an Fmask, {n} grids of {S} x {S} at 30 m in UTM 37 N, each, clip, labels: "
         f"{hls_us:8.1f} us = {hls_us / copy_us:5.2f} x the copy's time")
    first = results["each, SCL mask, range [0, 10000]"]
    emit(f"  ig_s2_chip_warp (each, SCL, range, labels) / ig_chip_warp: {first / hls_us:5.2f}")
    # a few chips against the numpy host path
    for t in (valid, vlab, hist):
        t.zero_()
    s2(0, True, 0, 1)()
    some = [0, 1, n // 2, n - 1]
    host = s2_raster_chips.warp_cut(bands.cpu().numpy(), starts, plane_class, class_grid, class_size, scl.cpu().numpy(), scl_starts, src, dst,
                                    grids[some], S, dates=T, class_bits=bits, strategy="each", valid_range=(0, 10000),
                                    labels=labels[some].cpu().numpy(), valid_bit=2, classes=8)
    idx = torch.tensor(some, device="cuda")
    got = (out.view(torch.int16)[idx].cpu().numpy().view(np.uint16), valid[idx].cpu().numpy(), plane[idx].cpu().numpy(), maps[idx].cpu().numpy(),
           vlab[idx].cpu().numpy(), hist[idx].cpu().numpy())
    emit(f"  chips {some} equal the numpy host path: {all(np.array_equal(a, b) for a, b in zip(got, host))}; valid values {got[1].tolist()}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
