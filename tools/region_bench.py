"""Region post-processing on a full tile: HIP-event times of labelling, areas, one sieve pass and the region statistics on a synthetic
S x S blob class map (default 10980) with 2 and with 13 classes, the whole sieve per pass, and the same labelling with
``scipy.ndimage.label`` on the host where scipy is present.

    python tools/region_bench.py [--size 10980] [--min-region 16] [--reps 3] [--out profiles/region_postprocess.txt]

The map: box-filtered noise planes, arg-maxed on the device (blobs a few pixels across), 2 % fill.  Each entry point is timed alone
between two HIP events after a warm-up call, median of ``--reps``; the sieve loop (``postprocess.sieve_class_map``, 8 passes at most)
is timed as a whole with a device synchronise and reported per pass.  scipy labels every class plane in turn (one call per class).
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "instageo-e2e-geospatial-ml_amd"))


def blob_map(S, ncls, seed, dev):
    import torch

    g = torch.Generator(device=dev).manual_seed(seed)
    best = torch.full((S, S), -float("inf"), device=dev)
    cm = torch.zeros((S, S), dtype=torch.int8, device=dev)
    for c in range(ncls):  # one plane at a time: 13 planes of 10980^2 floats are not held together
        plane = torch.nn.functional.avg_pool2d(torch.randn((1, 1, S + 6, S + 6), generator=g, device=dev), 7, stride=1)[0, 0]
        take = plane > best
        cm[take] = c
        best = torch.where(take, plane, best)
    cm[torch.rand((S, S), generator=g, device=dev) < 0.02] = -1
    return cm


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
    from instageo_amd import postprocess as PP

    dev, S = "cuda", args.size
    emit(f"region post-processing, {S} x {S} int8 blob map, 2 % fill, min_region {args.min_region}, median of {args.reps}")
    for ncls in (2, 13):
        cm = blob_map(S, ncls, 5 + ncls, dev)
        for conn in (4, 8):
            labels = torch.empty((S, S), dtype=torch.int32, device=dev)
            t_label = timed(lambda: ops.ccl_label(cm, conn, -1, out=labels), args.reps)
            area = torch.empty_like(labels)
            t_area = timed(lambda: ops.region_area(labels, out=area), args.reps)
            regions = int((area != 0).sum().item())
            emit(f"classes {ncls:2d} connectivity {conn}: {regions} regions; ig_ccl_label {t_label:9.3f} ms  ig_region_area {t_area:8.3f} ms")
            if conn == 4:
                best = torch.empty((S, S), dtype=torch.int64, device=dev)
                changed = torch.zeros(1, dtype=torch.int32, device=dev)
                work = cm.clone()
                t_pass = timed(lambda: (work.copy_(cm), ops.sieve_pass(work, labels, area, args.min_region, -1, best, changed)), args.reps)
                t_copy = timed(lambda: work.copy_(cm), args.reps)
                del best, work
                rid = (torch.cumsum((area != 0).view(-1), 0, dtype=torch.int32) - 1).view(S, S)
                t_stats = timed(lambda: ops.region_stats(labels, rid, regions), args.reps)
                del rid
                emit(f"    ig_sieve_pass {t_pass - t_copy:9.3f} ms  ig_region_stats {t_stats:8.3f} ms")
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, info = PP.sieve_class_map(cm, args.min_region, conn, -1, 8)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                # every pass labels, counts and sieves; a last labelling counts what is left when the cap ended the loop
                rounds = info["passes"] + 1
                emit(f"    sieve_class_map: {dt * 1e3:9.1f} ms for {info} = {dt * 1e3 / rounds:8.1f} ms per labelling round ({rounds} rounds)")
        if args.scipy:
            try:
                from scipy import ndimage
            except ImportError:
                emit("    scipy is not installed: no host comparison")
                continue
            host = cm.cpu().numpy()
            t0 = time.perf_counter()
            total = 0
            for c in range(ncls):
                total += ndimage.label(host == c)[1]
            emit(f"    host: scipy.ndimage.label over {ncls} class planes (4-connectivity): {(time.perf_counter() - t0) * 1e3:9.1f} ms, {total} regions")
        del cm


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=10980)
    ap.add_argument("--min-region", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-scipy", dest="scipy", action="store_false")
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
