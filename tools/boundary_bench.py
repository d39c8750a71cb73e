"""Boundary-quality kernels: HIP-event times of ``ig_boundary_dist2`` and ``ig_boundary_update`` on a batch of chips (16, 224, 224) and on
one full tile (1, S, S) (default 10980), for rmax 4 and 32, on synthetic blob class maps with 2 and with 13 classes.

    python tools/boundary_bench.py [--size 10980] [--reps 5] [--out profiles/boundary_metrics.txt]

The maps: box-filtered noise planes, arg-maxed on the device (blobs a few pixels across), 2 % fill, as they are and with every pixel
repeated 16 x 16 times (regions tens of pixels across: most pixels search far); the prediction is the ground truth moved by one pixel.  Each entry point is timed alone between two HIP events after a warm-up call, median of ``--reps``; GB/s counts
the algorithmic bytes (dist2: 1 read + 4 written per pixel; update: 10 read per pixel).
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "instageo-e2e-geospatial-ml_amd"))


def blob_maps(n, S, ncls, seed, dev, scale=1):
    """``scale`` > 1: the map is made at S / scale and every pixel repeated scale x scale times (regions tens of pixels across)."""
    import torch

    if scale > 1:
        small = blob_maps(n, -(-S // scale), ncls, seed, dev)
        return small.repeat_interleave(scale, 1).repeat_interleave(scale, 2)[:, :S, :S].contiguous()
    g = torch.Generator(device=dev).manual_seed(seed)
    out = torch.empty((n, S, S), dtype=torch.int8, device=dev)
    for i in range(n):
        best = torch.full((S, S), -float("inf"), device=dev)
        for c in range(ncls):  # one plane at a time: 13 planes of 10980^2 floats are not held together
            plane = torch.nn.functional.avg_pool2d(torch.randn((1, 1, S + 6, S + 6), generator=g, device=dev), 7, stride=1)[0, 0]
            take = plane > best
            out[i][take] = c
            best = torch.where(take, plane, best)
        out[i][torch.rand((S, S), generator=g, device=dev) < 0.02] = -1
    return out


def timed(fn, reps):
    import torch

    fn()  # warm-up
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def run(args, emit):
    import torch

    from instageo_amd import ops

    dev = "cuda"
    emit(f"boundary metrics, int8 blob maps with 2 % fill, pred = gt moved by one pixel, median of {args.reps}")
    for n, S, scale in ((16, 224, 1), (16, 224, 16), (1, args.size, 1), (1, args.size, 16)):
        emit(f"maps ({n}, {S}, {S}), blobs x {scale}")
        for ncls in (2, 13):
            gt = blob_maps(n, S, ncls, 5 + ncls, dev, scale)
            pred = torch.roll(gt, 1, dims=2)
            pred[gt == -1] = -1
            gd, pd = torch.empty((n, S, S), dtype=torch.int32, device=dev), torch.empty((n, S, S), dtype=torch.int32, device=dev)
            px = float(n) * S * S
            for rmax in (4, 32):
                t_d = timed(lambda: ops.boundary_dist2(gt, rmax, -1, out=gd), args.reps)
                ops.boundary_dist2(pred, rmax, -1, out=pd)
                far = float((gd == ops.BOUNDARY_FAR).sum().item()) / px
                for ts in ([rmax * rmax], [1, 4, 9, 16] if rmax == 4 else [1, 4, 16, 64, 256, 1024]):
                    band = torch.zeros(len(ts), ncls, 3, dtype=torch.int64, device=dev)
                    tri = torch.zeros(len(ts), ncls, ncls, dtype=torch.int64, device=dev)
                    t_u = timed(lambda: ops.boundary_update(gt, pred, gd, pd, ts, band, tri, ncls, -1), args.reps)
                    emit(f"({n}, {S}, {S}) classes {ncls:2d} rmax {rmax:2d} K {len(ts)}: ig_boundary_dist2 {t_d:9.3f} ms ({px * 5e-6 / t_d:7.1f} GB/s, "
                         f"{100 * far:4.1f} % FAR)  ig_boundary_update {t_u:8.3f} ms ({px * 10e-6 / t_u:7.1f} GB/s)")
            del gt, pred, gd, pd


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=10980)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    run(args, emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
