"""Dataset splitting: HIP-event times of one ``ig_split_assign`` round (N = 10^5 and 10^6 points, K = 20) and of the ``ig_split_nearest``
search (8 x 10^4 rows against 2 x 10^4 and 8 x 10^5 against 2 x 10^5) on synthetic quantised positions, the time of a device-to-device copy
of the point array (the memory floor of an assign round), and the wall time of the numpy host path at the smaller size of each
(DESIGN.md 3.34).

    python tools/split_bench.py [--reps 10] [--out profiles/split.txt]

The kernels are launched ``--reps`` times back to back between two HIP events after a warm-up launch, through the generated custom ops on
tensors that are already on the device (the large nearest search: ``max(1, reps // 5)`` times).  A pair of the nearest search is three
subtractions and three 32 x 32 + 64-bit multiply-adds; the rate is pairs (Na x Nb) per second.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "instageo-e2e-geospatial-ml_amd"))
K = 20


def positions(n, seed):
    """n quantised unit vectors scattered around 40 places."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(40, 3))[rng.integers(0, 40, size=n)] + 0.05 * rng.normal(size=(n, 3))
    return np.rint(v / np.linalg.norm(v, axis=1, keepdims=True) * 2.0**29).astype(np.int32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from instageo_amd import split, torch_ops

    torch_ops.register()
    ns = torch.ops.instageo_mi355x
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def timed(call, reps):
        call()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            call()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / reps  # us

    emit(f"split: synthetic quantised positions, {args.reps} launches back to back after a warm-up")
    for N in (10**5, 10**6):
        pts = positions(N, N)
        centres = split.initial_centres(pts[:: max(1, N // 20000)], K, np.random.default_rng(0))
        p, c = torch.from_numpy(pts).cuda(), torch.from_numpy(centres).cuda()
        assign = torch.full((N,), -1, dtype=torch.int32, device="cuda")
        sums = torch.zeros((K, 4), dtype=torch.int64, device="cuda")
        changed = torch.zeros(1, dtype=torch.int32, device="cuda")
        dst = torch.empty_like(p)
        copy_us = timed(lambda: dst.copy_(p), args.reps)
        us = timed(lambda: ns.split_assign(p, N, c, K, assign, sums, changed), args.reps)
        assign.fill_(-1), sums.zero_(), changed.zero_()
        ns.split_assign(p, N, c, K, assign, sums, changed)
        line = (f"  ig_split_assign N = {N:8d}, K = {K}: {us:9.1f} us, {N * K / us / 1e3:7.2f} G point-centre pairs/s; device copy of the "
                f"{12 * N / 1e6:.1f} MB of points {copy_us:8.1f} us = {100 * copy_us / us:5.1f} % of the round")
        if N == 10**5:
            t0 = time.perf_counter()
            host = split.assign_round(pts, centres, np.full(N, -1, dtype=np.int32))
            wall = time.perf_counter() - t0
            same = bool(np.array_equal(host[0], assign.cpu().numpy()) and np.array_equal(host[1], sums.cpu().numpy())
                        and host[2][0] == int(changed))
            line += f"; numpy host path {wall * 1e3:7.0f} ms = {wall * 1e6 / us:6.0f} x, equal {same}"
        emit(line)
    for Na, Nb in ((8 * 10**4, 2 * 10**4), (8 * 10**5, 2 * 10**5)):
        a, b = positions(Na, Na), positions(Nb, Nb + 1)
        ad, bd = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        d2 = torch.empty(Na, dtype=torch.int64, device="cuda")
        idx = torch.empty(Na, dtype=torch.int32, device="cuda")
        us = timed(lambda: ns.split_nearest(ad, Na, bd, Nb, d2, idx), args.reps if Na < 10**5 else max(1, args.reps // 5))
        line = f"  ig_split_nearest {Na:7d} x {Nb:7d}: {us:11.1f} us, {Na * Nb / us / 1e6:7.3f} T pairs/s"
        if Na < 10**5:
            t0 = time.perf_counter()
            host = split.nearest(a, b)
            wall = time.perf_counter() - t0
            same = bool(np.array_equal(host[0].view(np.int64), d2.cpu().numpy()) and np.array_equal(host[1], idx.cpu().numpy()))
            line += f"; numpy host path {wall:7.1f} s = {wall * 1e6 / us:6.0f} x, equal {same}"
        emit(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
