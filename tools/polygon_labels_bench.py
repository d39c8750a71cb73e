"""Polygon labels: stage times of the burn on a 3660 x 3660 int8 label grid (one HLS tile):

  (a) about 10 000 parcels of 8-40 vertices, in FILE ORDER = row-major over the grid (spatially sorted: the pass rectangles are strips of
      the raster) and the same parcels SHUFFLED (every pass rectangle is nearly the whole raster);
  (b) one polygon of 100 000 vertices that covers most of the raster (one pass over the whole raster);
  (c) ``ig_burn_resolve`` alone on the whole-raster canvas of (b), next to a device-to-device copy of the same bytes (the 8-byte canvas
      read + the pixels written);
  (d) the numpy host path on the same inputs;
  (e), (f) with ``--all-touched`` (and nothing else then): the parcels of (a) burned with and without ``all_touched`` in one session, the
      three all_touched launches alone, and ``ig_zone_touch`` on items that span a whole row against as many items of one pixel.

    python tools/polygon_labels_bench.py [--reps 5] [--out profiles/polygon_labels.txt]
    python tools/polygon_labels_bench.py --all-touched --out profiles/all_touched.txt

Burns are wall times around ``burn_fixed`` with a device synchronisation (they include the host's pass bookkeeping, the uploads and one
read-back per pass); (c) is between HIP events after a warm-up.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "instageo-e2e-geospatial-ml_amd"))
HW, Q = 3660, 256


def ring_edges(xy):
    q = np.floor(np.asarray(xy) * Q + 0.5).astype(np.int32)
    return np.ascontiguousarray(np.concatenate([q, np.roll(q, -1, axis=0)], axis=1))


def parcels(rng, side=100):
    """side x side star-shaped parcels of 8-40 vertices, one per lattice cell, row-major."""
    step = HW / side
    items = []
    for k in range(side * side):
        cy, cx = (k // side + 0.5) * step, (k % side + 0.5) * step
        n = int(rng.integers(8, 41))
        ang = np.sort(rng.random(n)) * 2 * np.pi
        rad = step * (0.3 + 0.35 * rng.random(n))
        items.append((int(1 + k % 4), ring_edges(np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], axis=1))))
    return items


def all_touched_legs(args, emit, items):
    """(e) the parcels of (a), sorted, burned with and without all_touched in one session, and the three all_touched launches alone on
    the whole-raster canvas of those parcels' first 64; (f) ig_zone_touch on HW items that each span a whole row (near-horizontal edges)
    against HW items of one pixel each (one steep edge), per written pixel."""
    import torch

    from instageo_amd import ops, zonal
    from instageo_amd import polygon_labels as P

    def timed(call, reset=None):
        us = []
        for i in range(max(args.reps, 10) + 1):
            if reset is not None:
                reset()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            torch.cuda.synchronize()
            if i:
                us.append(a.elapsed_time(b) * 1e3)
        return float(np.median(us)), float(min(us))

    prop = torch.cuda.get_device_properties(0)
    emit(f"all_touched on {torch.cuda.get_device_name(0)} ({prop.gcnArchName}, {prop.multi_processor_count} CUs): {HW} x {HW}; median (fastest)")
    for flag in (False, True, False, True):
        wall = []
        for _ in range(args.reps):
            raster = torch.zeros((HW, HW), dtype=torch.int8, device="cuda")
            stats = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            P.burn_fixed(raster, items, stats, all_touched=flag)
            torch.cuda.synchronize()
            wall.append(time.perf_counter() - t0)
        emit(f"  (e) {len(items)} parcels, sorted, burn_fixed(all_touched={flag}): {np.median(wall) * 1e3:8.1f} ms ({min(wall) * 1e3:.1f}); {stats['passes']} "
             f"passes, {stats['pixels_written']} pixels written")
    edges = torch.from_numpy(np.concatenate([e for _, e in items[:64]])).cuda()
    bit = torch.from_numpy(np.concatenate([np.full(len(e), b, dtype=np.uint8) for b, (_, e) in enumerate(items[:64])])).cuda()
    rows = ops.zone_edge_rows(edges, HW)
    canvas = zonal.toggle_canvas(edges, bit, HW, HW)
    toggles = canvas.clone()
    touch = torch.zeros_like(canvas)
    trows = ops.zone_touch_rows(edges, HW)
    first, T = torch.cumsum(trows, 0, dtype=torch.int64).sub_(trows), int(trows.sum().item())
    a = timed(lambda: ops.zone_touch_rows(edges, HW))
    b = timed(lambda: ops.zone_touch(edges, bit, first, touch, T))
    c = timed(lambda: ops.zone_touch_merge(canvas, touch), reset=lambda: canvas.copy_(toggles))
    d = timed(lambda: ops.zone_toggle(edges, bit, torch.cumsum(rows, 0, dtype=torch.int64).sub_(rows), canvas, int(rows.sum().item())))
    z = timed(lambda: touch.zero_())
    emit(f"      one pass of 64 parcels ({len(edges)} edges, {T} touched rows) on a whole-raster canvas: ig_zone_touch_rows (with its output "
         f"allocation) {a[0]:.1f} us ({a[1]:.1f}), ig_zone_touch {b[0]:.1f} us ({b[1]:.1f}), ig_zone_touch_merge {c[0]:.1f} us ({c[1]:.1f}) for "
         f"{HW * HW * 24 / 1e6:.1f} MB (two canvases read, one written) = {HW * HW * 24 / c[0] / 1e6:.2f} TB/s, zeroing the second canvas {z[0]:.1f} us "
         f"({z[1]:.1f}); for scale, ig_zone_toggle with its scan and host read of T {d[0]:.1f} us ({d[1]:.1f})")
    # (f) HW items either way
    r = np.arange(HW, dtype=np.int64)
    flat = np.stack([np.full(HW, -50), Q * r + 100, np.full(HW, HW * Q + 50), Q * r + 150], axis=1).astype(np.int32)  # one row each, every column
    steep = np.array([[Q * 1000 + 7, -5, Q * 1000 + 9, HW * Q + 5]], dtype=np.int32)  # every row, one column each
    for name, e in (("near-horizontal", flat), ("steep", steep)):
        ed = torch.from_numpy(e).cuda()
        bt = torch.zeros(len(e), dtype=torch.uint8, device="cuda")
        tr = ops.zone_touch_rows(ed, HW)
        fs, n = torch.cumsum(tr, 0, dtype=torch.int64).sub_(tr), int(tr.sum().item())
        touch.zero_()
        med, fast = timed(lambda: ops.zone_touch(ed, bt, fs, touch, n))
        px = int((touch != 0).sum().item())
        emit(f"  (f) ig_zone_touch, {n} items from {len(e)} {name} edge{'s' if len(e) > 1 else ''}: {med:8.1f} us ({fast:.1f}); {px} pixels written = "
             f"{med * 1e3 / px:.3f} ns per pixel, {px * 8 / med / 1e6:.3f} TB/s of 8-byte atomics")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--all-touched", action="store_true", help="only the all_touched legs (e) and (f)")
    args = ap.parse_args()
    import torch

    from instageo_amd import ops, zonal
    from instageo_amd import polygon_labels as P

    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def burn_time(items, device):
        best, stats, raster = [], {}, None
        for _ in range(args.reps if device else 1):
            raster = torch.zeros((HW, HW), dtype=torch.int8, device=device) if device else np.zeros((HW, HW), dtype=np.int8)
            stats = {}
            if device:
                torch.cuda.synchronize()
            t0 = time.perf_counter()
            P.burn_fixed(raster, items, stats)
            if device:
                torch.cuda.synchronize()
            best.append(time.perf_counter() - t0)
        return float(np.median(best)), min(best), stats, raster

    rng = np.random.default_rng(0)
    sorted_items = parcels(rng)
    if args.all_touched:
        all_touched_legs(args, emit, sorted_items)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    shuffled =[sorted_items[i] for i in rng.permutation(len(sorted_items))]
    ang = np.linspace(0, 2 * np.pi, 100000, endpoint=False)
    big = [(1, ring_edges(np.stack([HW / 2 + HW * 0.47 * (1 + 0.03 * np.sin(40 * ang)) * np.cos(ang),
                                    HW / 2 + HW * 0.47 * (1 + 0.03 * np.sin(40 * ang)) * np.sin(ang)], axis=1)))]
    prop = torch.cuda.get_device_properties(0)
    emit(f"polygon labels on {torch.cuda.get_device_name(0)} ({prop.gcnArchName}, {prop.multi_processor_count} CUs): {HW} x {HW} int8; burns are wall "
         f"times of burn_fixed, median (fastest) of {args.reps}")
    results = {}
    for name, items in (("(a) 10 000 parcels, file order row-major (sorted)", sorted_items), ("(a) the same parcels shuffled", shuffled),
                        ("(b) one polygon of 100 000 vertices", big)):
        med, fast, stats, raster = burn_time(items, "cuda")
        px = sum(r[2] * r[3] for _, _, r in P._passes(items, HW, HW))
        results[name] = raster
        emit(f"  {name}: {med * 1e3:8.1f} ms ({fast * 1e3:.1f}); {stats['passes']} passes = {med * 1e6 / max(1, stats['passes']):7.1f} us per pass; pass "
             f"rectangles {px / 1e6:8.1f} M pixels in all; {stats['pixels_written']} pixels written")
    # (c) ig_burn_resolve alone on the canvas of (b)
    edges = torch.from_numpy(big[0][1]).cuda()
    canvas = zonal.toggle_canvas(edges, torch.zeros(len(edges), dtype=torch.uint8, device="cuda"), HW, HW)
    table = torch.ones(64, dtype=torch.int8, device="cuda")
    out = torch.zeros((HW, HW), dtype=torch.int8, device="cuda")
    written = torch.zeros(1, dtype=torch.int64, device="cuda")

    def timed(call):
        call()
        torch.cuda.synchronize()
        us = []
        for _ in range(max(args.reps, 10)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            torch.cuda.synchronize()
            us.append(a.elapsed_time(b) * 1e3)
        return float(np.median(us)), float(min(us))

    rm, rf = timed(lambda: ops.burn_resolve(canvas, table, out, 0, 0, written))
    n_written = int((out != 0).sum().item())
    nbytes = HW * HW * 8 + n_written
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    cm, cf = timed(lambda: dst.copy_(src))
    zm, zf = timed(lambda: canvas.zero_())
    emit(f"  (c) ig_burn_resolve alone, whole-raster canvas: {rm:8.1f} us ({rf:.1f}) for {nbytes / 1e6:.1f} MB (canvas read + {n_written} pixels written) = "
         f"{nbytes / rm / 1e6:5.2f} TB/s; a device copy of the same bytes {cm:8.1f} us ({cf:.1f}) = {nbytes / cm / 1e6:5.2f} TB/s; resolve = "
         f"{100 * cm / rm:5.1f} % of the copy rate; zeroing the canvas {zm:8.1f} us ({zf:.1f})")
    emit("      (the canvas and the raster of (c) fit the 256 MiB Infinity Cache: both rates are cache-assisted, not HBM rates)")
    for name, items in (("(a) sorted", sorted_items), ("(b) one polygon", big)):
        med, _, stats, raster = burn_time(items, None)
        key = [k for k in results if k.startswith(name[:3])][0]
        emit(f"  (d) numpy host path, {name}: {med * 1e3:8.0f} ms; equal to the device raster {bool(np.array_equal(raster, results[key].cpu().numpy()))}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
