"""Object-metric kernels: HIP-event times of ``ig_object_pairs``, ``ig_object_match`` and ``ig_object_count`` on one blob map pair
(1, S, S) (default 4096) and on a batch of chips (16, 224, 224), beside the two ``ig_ccl_label`` calls that precede them and a device copy
of the bytes the pair kernel reads (two int32 label rasters), all in one session.

    python tools/objects_bench.py [--size 4096] [--reps 5] [--out profiles/object_metrics.txt]

The maps: box-filtered noise planes, arg-maxed on the device (blobs a few pixels across), 2 % fill, 3 classes; the prediction is the ground
truth moved by one pixel.  Each entry point is timed alone between two HIP events after a warm-up call, median of ``--reps``.  The table has
the capacity ``overlap_table`` takes (the smallest power of two >= 2 x pixels, at most 2^24); its clearing is part of ``ig_object_pairs``.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "instageo-e2e-geospatial-ml_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def run(args, emit):
    import torch
    from boundary_bench import blob_maps, timed

    from instageo_amd import objects as O
    from instageo_amd import ops

    dev, ncls = "cuda", 3
    emit(f"object metrics, int8 blob maps of {ncls} classes with 2 % fill, pred = gt moved by one pixel, median of {args.reps}")
    for n, S in ((1, args.size), (16, 224)):
        gt = blob_maps(n, S, ncls, 8, dev)
        pred = torch.roll(gt, 1, dims=2)
        pred[gt == -1] = -1
        px = n * S * S
        gl, pl = torch.empty((n, S, S), dtype=torch.int32, device=dev), torch.empty((n, S, S), dtype=torch.int32, device=dev)
        ccl_status = torch.zeros(1, dtype=torch.int32, device=dev)

        def label():  # the entry point itself: ops.ccl_label also copies the status to the host, which is no kernel time
            for m, l in ((gt, gl), (pred, pl)):
                ops._call("ig_ccl_label", 0.0, ops._p(m), ops._p(l), n, S, S, 4, -1, ops._p(ccl_status), ops._stream())

        t_ccl = timed(label, args.reps)
        assert int(ccl_status.item()) == 0
        ga, pa = ops.region_area(gl), ops.region_area(pl)
        capacity = O._capacity_for(px)
        keys, counts = torch.empty(capacity, dtype=torch.int64, device=dev), torch.empty(capacity, dtype=torch.int32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        t_pairs = timed(lambda: ops.object_pairs(gl, pl, keys, counts, status), args.reps)
        entries = int((keys != ops.OBJECT_EMPTY).sum().item())
        assert int(status.item()) == 0
        ratios = O.threshold_ratios([0.5, 0.75])
        tp, iou_q = torch.zeros(2, ncls, dtype=torch.int64, device=dev), torch.zeros(2, ncls, dtype=torch.int64, device=dev)
        n_gt = torch.zeros(ncls, dtype=torch.int64, device=dev)
        t_match = timed(lambda: ops.object_match(keys, counts, gt, pred, ga, pa, ratios, tp, iou_q, ncls, 1), args.reps)
        t_count = timed(lambda: ops.object_count(gt, gl, ga, n_gt, ncls, 1), args.reps)
        both, sink = torch.stack((gl, pl)), torch.empty((2, n, S, S), dtype=torch.int32, device=dev)
        t_copy = timed(lambda: sink.copy_(both), args.reps)
        regions = int(n_gt.sum().item()) // (args.reps + 1)
        emit(f"maps ({n}, {S}, {S}): {px} pixels, {regions} gt regions, {entries} pairs in {capacity} slots")
        emit(f"  2 x ig_ccl_label           {t_ccl:9.3f} ms")
        emit(f"  ig_object_pairs            {t_pairs:9.3f} ms ({px * 8e-6 / t_pairs:7.1f} GB/s of labels read; {t_pairs / t_ccl:5.2f} x the labelling)")
        emit(f"  ig_object_match (K = 2)    {t_match:9.3f} ms ({capacity * 12e-6 / t_match:7.1f} GB/s of slots read)")
        emit(f"  ig_object_count (one map)  {t_count:9.3f} ms ({px * 9e-6 / t_count:7.1f} GB/s)")
        emit(f"  device copy of the labels  {t_copy:9.3f} ms ({px * 16e-6 / t_copy:7.1f} GB/s read + written)")
        del gt, pred, gl, pl, ga, pa, keys, counts, both, sink


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=4096)
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
