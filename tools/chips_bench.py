"""Chip cutting: HIP-event times of ``ig_chip_cut`` and ``ig_chip_labels`` on one synthetic HLS granule stack (3 dates x 6 bands x 3660 x
3660 int16 with its Fmask, built in memory) cut into its 14 x 14 chips of 256 x 256, the time of a device-to-device copy that moves the
same number of bytes (read + written), and the wall time of the numpy host path on the same inputs.

    python tools/chips_bench.py [--reps 20] [--out profiles/chips.txt]

The kernels are launched ``--reps`` times back to back between two HIP events after a warm-up launch, through the generated custom ops on
tensors that are already on the device.  Bytes of the cut = per chip pixel 2 x T x C x 2 (the bands read and written) + T (Fmask) + 1
(validity); the copy moves half of that from one buffer to another.  The label maps get 40 points per chip with a window of 3 x 3.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "instageo-e2e-geospatial-ml_amd"))
T, C, HW, S = 3, 6, 3660, 256
PER_CHIP = 40


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from instageo_amd import chips, torch_ops

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
    tile = torch.randint(1, 10000, (T * C, HW, HW), generator=g, device="cuda", dtype=torch.int16)
    tile[torch.rand((T * C, HW, HW), generator=g, device="cuda") < 0.02] = 0
    # Fmask: clear, cloud, shadow, water, near cloud, in blobs of 64 x 64 with salt
    kinds = torch.tensor([0, 0, 0, 2, 8, 32, 4, 64], dtype=torch.uint8, device="cuda")
    coarse = kinds[torch.randint(0, 8, (T, -(-HW // 64), -(-HW // 64)), generator=g, device="cuda")]
    fmask = coarse.repeat_interleave(64, 1).repeat_interleave(64, 2)[:, :HW, :HW].contiguous()
    n = (HW // S) ** 2
    origins = np.array([(S * y, S * x) for x in range(HW // S) for y in range(HW // S)], dtype=np.int32)
    od = torch.from_numpy(origins).cuda()
    out = torch.empty((n, T * C, S, S), dtype=torch.int16, device="cuda")
    valid = torch.zeros(n, dtype=torch.int32, device="cuda")
    plane = torch.empty((n, S, S), dtype=torch.uint8, device="cuda")
    bits = chips.mask_bits(["cloud", "near_cloud_or_shadow", "cloud_shadow", "water"])
    nbytes = n * S * S * (4 * T * C + T + 1)
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    copy_us = timed(lambda: dst.copy_(src))
    copy_tbs = nbytes / copy_us / 1e6
    emit(f"chips: {T} x {C} x {HW} x {HW} int16 + Fmask -> {n} chips of {S} x {S}, {args.reps} launches back to back after a warm-up")
    emit(f"  device-to-device copy of {nbytes / 2e6:.1f} MB ({nbytes / 1e6:.1f} MB read + written): {copy_us:8.1f} us, {copy_tbs:5.2f} TB/s")
    th, fh = tile.cpu().numpy(), fmask.cpu().numpy()
    for strategy in ("each", "any"):
        code = chips.STRATEGIES[strategy]
        us = timed(lambda: ns.chip_cut(tile, fmask, od, n, T, C, HW, HW, S, bits, code, 0, 0, 0, 0, out, valid, plane))
        valid.zero_()
        ns.chip_cut(tile, fmask, od, n, T, C, HW, HW, S, bits, code, 0, 0, 0, 0, out, valid, plane)
        t0 = time.perf_counter()
        host = chips.cut(th, fh, origins, S, mask=bits, strategy=strategy)
        wall = time.perf_counter() - t0
        same = bool(np.array_equal(host[0], out.cpu().numpy()) and np.array_equal(host[1], valid.cpu().numpy()) and np.array_equal(host[2], plane.cpu().numpy()))
        tbs = nbytes / us / 1e6
        emit(f"  ig_chip_cut {strategy:4s}: {us:8.1f} us, {tbs:5.2f} TB/s = {100 * tbs / copy_tbs:5.1f} % of the copy rate; numpy host path "
             f"{wall * 1e3:7.0f} ms = {wall * 1e6 / us:6.0f} x, equal {same}")
    us = timed(lambda: ns.chip_cut(tile, None, od, n, T, C, HW, HW, S, 0, 0, 0, 1, 0, 10000, out, valid, plane))
    nb = n * S * S * (4 * T * C + 1)
    emit(f"  ig_chip_cut without Fmask, clip [0, 10000]: {us:8.1f} us, {nb / us / 1e6:5.2f} TB/s = {100 * nb / us / 1e6 / copy_tbs:5.1f} % of the copy rate")
    # label maps: PER_CHIP points per chip, 3 x 3 windows, against the validity plane of the last cut with Fmask
    valid.zero_()
    ns.chip_cut(tile, fmask, od, n, T, C, HW, HW, S, bits, 0, 0, 0, 0, 0, out, valid, plane)
    rng = np.random.default_rng(1)
    rows = np.repeat(origins[:, 0], PER_CHIP) + rng.integers(0, S, n * PER_CHIP)
    cols = np.repeat(origins[:, 1], PER_CHIP) + rng.integers(0, S, n * PER_CHIP)
    pts = np.stack((rows, cols, np.arange(n * PER_CHIP)), axis=-1).astype(np.int32)
    ptr = (np.arange(n + 1) * PER_CHIP).astype(np.int32)
    labels = rng.integers(0, 4, n * PER_CHIP).astype(np.int16)
    dev = [torch.from_numpy(a).cuda() for a in (ptr, pts.reshape(-1), labels)]
    maps = torch.empty((n, S, S), dtype=torch.int16, device="cuda")
    vl = torch.zeros(n, dtype=torch.int32, device="cuda")
    hist = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    us = timed(lambda: ns.chip_labels(od, n, S, dev[0], dev[1], dev[2], labels.size, 2, 1, plane, 1, 4, maps, vl, hist))
    vl.zero_(), hist.zero_()
    ns.chip_labels(od, n, S, dev[0], dev[1], dev[2], labels.size, 2, 1, plane, 1, 4, maps, vl, hist)
    t0 = time.perf_counter()
    host = chips.label_maps(origins, S, ptr, pts, labels, 1, plane.cpu().numpy(), "any", "seg", 4)
    wall = time.perf_counter() - t0
    same = bool(np.array_equal(host[0], maps.cpu().numpy()) and np.array_equal(host[1], vl.cpu().numpy()) and np.array_equal(host[2], hist.cpu().numpy()))
    nb = n * S * S * 3
    emit(f"  ig_chip_labels {PER_CHIP} points per chip, w = 1: {us:8.1f} us, {nb / us / 1e6:5.2f} TB/s of maps written + validity read; numpy host path "
         f"{wall * 1e3:7.0f} ms = {wall * 1e6 / us:6.0f} x, equal {same}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
