"""Sentinel-2 chip cutting: HIP-event time of ``ig_s2_chip_cut`` on one synthetic L2A stack (3 dates x 6 bands: three planes of 10980 x 10980
at 10 m and three of 5490 x 5490 at 20 m per date, uint16, with one 20 m SCL plane per date, built on the device) cut into its 42 x 42
chips of 256 x 256 at 10 m, against the time of a device-to-device copy of the same output bytes.

    python tools/s2_chips_bench.py [--reps 10] [--out profiles/s2_chips.txt]

The kernel is launched ``--reps`` times back to back between two HIP events after a warm-up launch, through the generated custom op on
tensors that are already on the device.  Output bytes per chip pixel = 2 x T x C (the chips) + 1 (validity); the copy reads and writes
that many from one buffer to another.  The kernel reads less than it writes: a 20 m plane has a quarter of the pixels it fans out into.
A few chips are compared with the numpy host path.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "instageo-e2e-geospatial-ml_amd"))
T, C, S = 3, 6, 256
FULL, HALF = 10980, 5490


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from instageo_amd import s2_chips, torch_ops

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
    sides = ([FULL] * 3 + [HALF] * 3) * T
    geom = np.array([(h, h, 10 if h == FULL else 20) for h in sides], dtype=np.int32)
    starts = np.concatenate([[0], np.cumsum([h * h for h in sides])[:-1]]).astype(np.int64)
    total = int(sum(h * h for h in sides))
    raw = torch.empty(total, dtype=torch.int16, device="cuda")
    for k, h in enumerate(sides):  # plane by plane: the random draws stay small
        seg = raw[int(starts[k]) : int(starts[k]) + h * h]
        seg.copy_(torch.randint(1, 11000, (h * h,), generator=g, device="cuda", dtype=torch.int16))
        seg[torch.rand(h * h, generator=g, device="cuda") < 0.02] = 0
    bands = raw.view(torch.uint16)
    # SCL: vegetation, soil, water, cloud (medium, high), shadow, cirrus in blobs of 32 x 32 source pixels
    kinds = torch.tensor([4, 4, 4, 5, 6, 8, 9, 3, 10], dtype=torch.uint8, device="cuda")
    coarse = kinds[torch.randint(0, len(kinds), (T, -(-HALF // 32), -(-HALF // 32)), generator=g, device="cuda")]
    scl = coarse.repeat_interleave(32, 1).repeat_interleave(32, 2)[:, :HALF, :HALF].contiguous().reshape(-1)
    scl_starts = (np.arange(T, dtype=np.int64) * HALF * HALF).astype(np.int64)
    scl_geom = np.array([(HALF, HALF, 20)] * T, dtype=np.int32)
    per = FULL // S
    n = per * per
    origins = np.array([(S * y, S * x) for x in range(per) for y in range(per)], dtype=np.int32)
    od, sd, ssd = (torch.from_numpy(a).cuda() for a in (origins, starts, scl_starts))
    gd = torch.from_numpy(np.concatenate([geom, scl_geom])).cuda()
    out = torch.empty((n, T * C, S, S), dtype=torch.uint16, device="cuda")
    valid = torch.zeros(n, dtype=torch.int32, device="cuda")
    plane = torch.empty((n, S, S), dtype=torch.uint8, device="cuda")
    bits = s2_chips.scl_class_bits(["cloud", "water", "cloud_shadow"])
    px = n * S * S
    written = px * (2 * T * C + 1)
    read = px * (2 * 9 + 0.5 * 9 + 0.25 * T)  # nine planes at 10 m, nine at 20 m, the SCL at 20 m
    src = torch.empty(written, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    copy_us = timed(lambda: dst.copy_(src))
    del src, dst
    emit(f"s2 chips: {T} dates x (3 x {FULL}^2 + 3 x {HALF}^2) uint16 + SCL {HALF}^2 -> {n} chips of {S} x {S} at 10 m, {args.reps} launches back to "
         "back after a warm-up")
    emit(f"  device-to-device copy of the output bytes, {written / 1e6:.1f} MB ({2 * written / 1e6:.1f} MB read + written): {copy_us:8.1f} us, "
         f"{2 * written / copy_us / 1e6:5.2f} TB/s, {written / copy_us / 1e6:5.2f} TB/s stored")

    def report(what, us, rd, wr):
        emit(f"  ig_s2_chip_cut {what}: {us:8.1f} us = {us / copy_us:5.2f} x the copy's time; {wr / us / 1e6:5.2f} TB/s stored = "
             f"{100 * copy_us / us:5.1f} % of the copy's store rate; {(rd + wr) / us / 1e6:5.2f} TB/s read + written")

    for strategy in ("each", "any"):
        code = s2_chips.STRATEGIES[strategy]
        us = timed(lambda: ns.s2_chip_cut(bands, sd, scl, ssd, gd, od, n, T, C, FULL, FULL, 10, S, bits, code, 0, 0, 0, 0, 0, out, valid, plane))
        report(f"{strategy:4s}, SCL mask", us, read, written)
    us = timed(lambda: ns.s2_chip_cut(bands, sd, None, None, gd[: T * C], od, n, T, C, FULL, FULL, 10, S, 0, 0, 0, 1000, 1, 0, 10000, out, valid, plane))
    report("without SCL, boa_offset 1000, valid range [0, 10000]", us, read - px * 0.25 * T, written)
    # the 10 m planes alone (ratio 1) and the 20 m planes alone (each source pixel fans out into 2 x 2): where the time goes
    ten = [k for k, h in enumerate(sides) if h == FULL]
    twenty = [k for k, h in enumerate(sides) if h == HALF]
    for what, pick, rd in (("the nine 10 m planes alone", ten, 2.0), ("the nine 20 m planes alone", twenty, 0.5)):
        sub_g, sub_s = torch.from_numpy(geom[pick]).cuda(), torch.from_numpy(starts[pick]).cuda()
        sub_out = out.view(-1)[: n * len(pick) * S * S].view(n, len(pick), S, S)
        us = timed(lambda: ns.s2_chip_cut(bands, sub_s, None, None, sub_g, od, n, T, len(pick) // T, FULL, FULL, 10, S, 0, 0, 0, 0, 0, 0, 0, sub_out, valid, plane))
        wr = px * (2 * len(pick) + 1)
        nb = torch.empty(wr, dtype=torch.uint8, device="cuda")
        nb2 = torch.empty_like(nb)
        c_us = timed(lambda: nb2.copy_(nb))
        del nb, nb2
        emit(f"  {what}: {us:8.1f} us, {wr / us / 1e6:5.2f} TB/s stored, {px * rd * len(pick) / us / 1e6:5.2f} TB/s read; a copy of its output bytes "
             f"{c_us:8.1f} us: {100 * c_us / us:5.1f} % of the copy's store rate")
    # a few chips against the numpy host path
    valid.zero_()
    ns.s2_chip_cut(bands, sd, scl, ssd, gd, od, n, T, C, FULL, FULL, 10, S, bits, 0, 0, 0, 0, 0, 0, out, valid, plane)
    some = [0, 1, per, n // 2 + 7, n - 1]
    bh, sh = bands.cpu().numpy(), scl.cpu().numpy()
    host = s2_chips.cut(bh, starts, geom, sh, scl_starts, scl_geom, origins[some], S, (FULL, FULL, 10), dates=T, class_bits=bits, strategy="each")
    idx = torch.tensor(some, device="cuda")
    same = bool(np.array_equal(host[0], out.view(torch.int16)[idx].cpu().numpy().view(np.uint16)) and np.array_equal(host[1], valid[idx].cpu().numpy())
                and np.array_equal(host[2], plane[idx].cpu().numpy()))
    emit(f"  chips {some} equal the numpy host path: {same}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
