"""Dataset cleaning: HIP-event times of ``ig_chip_nodata`` and ``ig_label_buffer`` on 196 synthetic chips of 18 x 256 x 256 int16 and their
196 label maps (built in memory), the time of a device-to-device copy that reads the same number of bytes as ``ig_chip_nodata``, and the
wall time of the numpy host path on the same arrays.

    python tools/clean_bench.py [--reps 20] [--out profiles/clean.txt]

The kernels are launched ``--reps`` times back to back between two HIP events after a warm-up launch, through the generated custom ops on
tensors that are already on the device.  Bytes of ``ig_chip_nodata`` = per chip pixel 2 x B read + 1 written; the copy reads as many bytes
as the kernel reads and, unlike the kernel, writes as many again.  Bytes of ``ig_label_buffer`` = per pixel 2 read + 2 written + 1 of the
plane.  The label maps have 40 sources each.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "instageo-e2e-geospatial-ml_amd"))
N, B, S = 196, 18, 256
PER_MAP = 40
ND = -9999


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from instageo_amd import clean, torch_ops

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
    chips = torch.randint(1, 10000, (N, B, S, S), generator=g, device="cuda", dtype=torch.int16)
    chips[torch.rand((N, B, S, S), generator=g, device="cuda") < 0.02] = ND
    chips[:, :, :40, :60] = ND  # a corner without data in any band
    plane = torch.empty((N, S, S), dtype=torch.uint8, device="cuda")
    counts = torch.zeros((N, 2), dtype=torch.int32, device="cuda")
    read = N * B * S * S * 2
    src = torch.empty(read, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    copy_us = timed(lambda: dst.copy_(src))
    copy_tbs = read / copy_us / 1e6
    emit(f"clean: {N} chips of {B} x {S} x {S} int16 and their label maps, {args.reps} launches back to back after a warm-up")
    emit(f"  device-to-device copy reading {read / 1e6:.1f} MB (and writing as many): {copy_us:8.1f} us, {copy_tbs:5.2f} TB/s read")
    us = timed(lambda: ns.chip_nodata(chips, N, B, S, S, ND, plane, counts))
    counts.zero_()
    ns.chip_nodata(chips, N, B, S, S, ND, plane, counts)
    ch = chips.cpu().numpy()
    t0 = time.perf_counter()
    host = clean.nodata_planes(ch, ND)
    wall = time.perf_counter() - t0
    same = bool(np.array_equal(host[0], plane.cpu().numpy()) and np.array_equal(host[1], counts.cpu().numpy()))
    nb = read + N * S * S
    emit(f"  ig_chip_nodata: {us:8.1f} us, {nb / us / 1e6:5.2f} TB/s ({read / us / 1e6:5.2f} TB/s read) = {100 * read / us / 1e6 / copy_tbs:5.1f} % of "
         f"the copy's read rate; numpy host path {wall * 1e3:7.0f} ms = {wall * 1e6 / us:6.0f} x, equal {same}")
    rng = np.random.default_rng(1)
    labels = np.full((N, S, S), -1, dtype=np.int16)
    labels[np.repeat(np.arange(N), PER_MAP), rng.integers(0, S, N * PER_MAP), rng.integers(0, S, N * PER_MAP)] = rng.integers(0, 4, N * PER_MAP)
    lab = torch.from_numpy(labels).cuda()
    out = torch.empty_like(lab)
    vl = torch.zeros(N, dtype=torch.int32, device="cuda")
    hist = torch.zeros((N, 4), dtype=torch.int32, device="cuda")
    ph = plane.cpu().numpy()
    nb = N * S * S * 5
    for w in (1, 32):
        us = timed(lambda: ns.label_buffer(lab, N, S, S, 2, w, -1, plane, 4, out, vl, hist))
        vl.zero_(), hist.zero_()
        ns.label_buffer(lab, N, S, S, 2, w, -1, plane, 4, out, vl, hist)
        t0 = time.perf_counter()
        host = clean.buffer_labels(labels, w, -1, ph, 4)
        wall = time.perf_counter() - t0
        same = bool(np.array_equal(host[0], out.cpu().numpy()) and np.array_equal(host[1], vl.cpu().numpy()) and np.array_equal(host[2], hist.cpu().numpy()))
        emit(f"  ig_label_buffer {PER_MAP} sources per map, w = {w:2d}: {us:8.1f} us, {nb / us / 1e6:5.2f} TB/s of maps read + written + plane read; "
             f"numpy host path {wall * 1e3:7.0f} ms = {wall * 1e6 / us:6.0f} x, equal {same}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
