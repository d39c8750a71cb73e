"""Chips warped onto label grids: HIP-event times of ``ig_chip_warp`` on one synthetic HLS granule stack (3 dates x 6 bands x 3660 x 3660
int16 with its Fmask, built in memory) cut into 196 chips of 256 x 256:

  (a) on the stack's own grid, next to ``ig_chip_cut`` on the same inputs and a device-to-device copy of the same bytes;
  (b) onto EPSG:4326 grids of 0.00027 degrees, next to ONE ``ig_warp`` launch (nearest, one band) over a canvas of the same pixels, which
      a band-by-band warp would repeat T * C times as float32 and T times as int8;
  (c) the wall time of the numpy host path on both.

    python tools/raster_chips_bench.py [--reps 20] [--out profiles/raster_chips.txt]

After a warm-up launch every launch is bracketed by its own pair of HIP events; the median and the fastest of ``--reps`` are reported.
Bytes of a cut = per chip pixel 2 x T x C x 2 (the bands read and written) + T (Fmask) + 1 (validity); the copy moves half of that from
one buffer to another.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "instageo-e2e-geospatial-ml_amd"))
T, C, HW, S = 3, 6, 3660, 256
RES = 0.00027


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from instageo_amd import chips, crs, torch_ops, warp
    from instageo_amd import raster_chips as R

    torch_ops.register()
    ns = torch.ops.instageo_mi355x
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def timed(call):
        call()
        torch.cuda.synchronize()
        us = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            torch.cuda.synchronize()
            us.append(a.elapsed_time(b) * 1e3)
        return float(np.median(us)), float(min(us))

    g = torch.Generator(device="cuda").manual_seed(0)
    tile = torch.randint(1, 10000, (T * C, HW, HW), generator=g, device="cuda", dtype=torch.int16)
    tile[torch.rand((T * C, HW, HW), generator=g, device="cuda") < 0.02] = 0
    kinds = torch.tensor([0, 0, 0, 2, 8, 32, 4, 64], dtype=torch.uint8, device="cuda")
    coarse = kinds[torch.randint(0, 8, (T, -(-HW // 64), -(-HW // 64)), generator=g, device="cuda")]
    fmask = coarse.repeat_interleave(64, 1).repeat_interleave(64, 2)[:, :HW, :HW].contiguous()
    side = HW // S
    n = side * side
    utm = crs.from_epsg(32636)
    X0, Y0 = 399960.0, 4500000.0
    sgrid = (X0, Y0, 30.0, 30.0)
    origins = np.array([(S * y, S * x) for x in range(side) for y in range(side)], dtype=np.int32)
    same_grids = np.array([(X0 + 30.0 * c0, Y0 - 30.0 * r0, 30.0, 30.0) for r0, c0 in origins.tolist()])
    lon0, lat0 = (float(v) for v in crs.transform(utm, crs.from_epsg(4326), X0 + 3000.0, Y0 - 1500.0))
    geo_grids = np.array([(lon0 + 1.3e-5 + S * RES * x, lat0 - 0.7e-5 - S * RES * y, RES, RES) for x in range(side) for y in range(side)])
    od = torch.from_numpy(origins).cuda()
    meta = torch.from_numpy(np.concatenate([utm.params, sgrid, utm.params, crs.from_epsg(4326).params, same_grids.reshape(-1),
                                            geo_grids.reshape(-1)])).cuda()
    m_utm, m_sg, m_utm2, m_geo = meta[0:5], meta[5:9], meta[9:14], meta[14:19]
    m_same, m_gg = meta[19 : 19 + 4 * n], meta[19 + 4 * n :]
    out = torch.empty((n, T * C, S, S), dtype=torch.int16, device="cuda")
    ref = torch.empty_like(out)
    valid = torch.zeros(n, dtype=torch.int32, device="cuda")
    plane = torch.empty((n, S, S), dtype=torch.uint8, device="cuda")
    labels = torch.randint(-1, 4, (n, S, S), generator=g, device="cuda", dtype=torch.int8)
    maps, vl, hist = torch.empty_like(labels), torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    bits = chips.mask_bits(["cloud", "near_cloud_or_shadow", "cloud_shadow", "water"])
    nbytes = n * S * S * (4 * T * C + T + 1)
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)

    def warp_cut(dc, dg, lab=False):
        return ns.chip_warp(tile, fmask, m_utm, m_sg, dc, dg, n, T, C, HW, HW, S, bits, 0, 0, 1, 0, 10000, labels if lab else None, 1, 1 if lab else 0,
                            4 if lab else 0, out, valid, plane, maps if lab else None, vl if lab else None, hist if lab else None)

    emit(f"raster chips on {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs): {T} x {C} x {HW} x {HW} int16 + Fmask -> {n} chips of {S} x {S}, clip [0, 10000]; "
         f"median (fastest) of {args.reps} launches, each between its own HIP events, after a warm-up")
    cm, cf = timed(lambda: dst.copy_(src))
    copy_tbs = nbytes / cm / 1e6
    emit(f"  device-to-device copy of {nbytes / 2e6:.1f} MB ({nbytes / 1e6:.1f} MB read + written): {cm:8.1f} us ({cf:.1f}), {copy_tbs:5.2f} TB/s")
    um, uf = timed(lambda: ns.chip_cut(tile, fmask, od, n, T, C, HW, HW, S, bits, 0, 0, 1, 0, 10000, ref, valid, plane))
    emit(f"  (a) ig_chip_cut, the stack's grid:             {um:8.1f} us ({uf:.1f}), {nbytes / um / 1e6:5.2f} TB/s = {100 * nbytes / um / 1e6 / copy_tbs:5.1f} % of the copy rate")
    wm, wf = timed(lambda: warp_cut(m_utm2, m_same))
    emit(f"  (a) ig_chip_warp, the stack's grid:            {wm:8.1f} us ({wf:.1f}), {nbytes / wm / 1e6:5.2f} TB/s = {100 * nbytes / wm / 1e6 / copy_tbs:5.1f} % of the copy rate, "
         f"{wm / um:.2f} x ig_chip_cut, equal {bool(torch.equal(out, ref))}")
    lm, lf = timed(lambda: warp_cut(m_utm2, m_same, True))
    emit(f"  (a) ig_chip_warp with int8 label maps, K = 4:  {lm:8.1f} us ({lf:.1f})")
    gm, gf = timed(lambda: warp_cut(m_geo, m_gg))
    px = n * S * S
    emit(f"  (b) ig_chip_warp, EPSG:4326 grids of {RES}: {gm:8.1f} us ({gf:.1f}), {nbytes / gm / 1e6:5.2f} TB/s; the float64 chain costs "
         f"{(gm - wm) * 1e3 / px:.3f} ns per destination pixel over (a)")
    # one band of the same pixels through ig_warp: a canvas of side * S pixels in EPSG:4326 from one source
    canvas = (side * S, side * S)
    cgrid = tuple(geo_grids[0])
    band = tile[0].float().reshape(-1).contiguous()
    sizes = np.array([[HW, HW]], dtype=np.int32)
    geo = crs.from_epsg(4326)
    ptr, idx = warp.block_lists(geo.params, cgrid, canvas, [utm.params], [sgrid], sizes)
    one = torch.empty(canvas, dtype=torch.float32, device="cuda")
    wmeta = torch.from_numpy(np.concatenate([geo.params, cgrid, utm.params, sgrid])).cuda()
    up = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (np.zeros(1, dtype=np.int64), sizes.reshape(-1), ptr, idx)]

    def one_band(src_, es, fill, dst_):
        return ns.warp(src_, up[0], wmeta[9:14], wmeta[14:18], up[1], 1, up[2], up[3], wmeta[0:5], wmeta[5:9], canvas[0], canvas[1], es, 0, 0, fill,
                       dst_, None)

    fm_, ff_ = timed(lambda: one_band(band, 4, -1, one))
    band8 = fmask[0].view(torch.int8).reshape(-1).contiguous()
    one8 = torch.empty(canvas, dtype=torch.int8, device="cuda")
    im_, if_ = timed(lambda: one_band(band8, 1, -128, one8))
    emit(f"  (b) ONE ig_warp launch (nearest) over the same {canvas[0]} x {canvas[1]} pixels: float32 {fm_:8.1f} us ({ff_:.1f}), int8 {im_:8.1f} us "
         f"({if_:.1f}); band by band = {T * C} x float32 + {T} x int8 = {T * C * fm_ + T * im_:8.1f} us = {(T * C * fm_ + T * im_) / gm:.1f} x ig_chip_warp")
    # (c) the numpy host path
    th, fh = tile.cpu().numpy(), fmask.cpu().numpy()
    for name, dcrs, grids, dc, dg in (("the stack's grid", utm, same_grids, m_utm2, m_same), ("EPSG:4326", geo, geo_grids, m_geo, m_gg)):
        valid.zero_()
        warp_cut(dc, dg)
        t0 = time.perf_counter()
        host = R.warp_cut(th, fh, utm, sgrid, dcrs, grids, S, mask=bits, clip=(0, 10000))
        wall = time.perf_counter() - t0
        diff = int((torch.from_numpy(host[0]) != out.cpu()).any(dim=1).sum())
        emit(f"  (c) numpy host path, {name}: {wall * 1e3:7.0f} ms = {wall * 1e6 / (wm if dcrs is utm else gm):6.0f} x the kernel; pixels that differ from the "
             f"device {diff} of {px}, valid_values equal {bool(np.array_equal(host[1], valid.cpu().numpy()))}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
