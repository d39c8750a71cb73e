"""Sentinel-2 chips warped onto label grids on the device (-m gpu): ``ig_s2_chip_warp`` against the sequential twin
(tests/s2_raster_chips_reference.py) over 10 m / 20 m / 60 m planes, chips that leave the tile, other pixel sizes and other coordinate
systems; against ``ig_chip_warp`` with one class and ``ig_s2_chip_cut`` on a shared corner; label maps; stores into poisoned outputs from
planes at odd starts; determinism; unusable grids and table entries; and create_s2_raster_chips on the device against the host path,
file for file.

Every case is one the twin reports free of ties (no pixel with u or v within 1e-6 of an integer in any class it reads: asserted before
anything is compared), so every comparison is exact equality on all elements and all counts."""
import os

import numpy as np
import pytest
import torch

import raster_chips_reference as RR
import s2_chips_reference as SR
import s2_raster_chips_reference as QR
from instageo_amd import _lib, ops, raster_chips, s2_chips
from instageo_amd import s2_raster_chips as Q
from test_cpu_s2_raster_chips import KW, LABEL_CASES, label_case, write_granule

pytestmark = pytest.mark.gpu
POISON_CHIP, POISON_PLANE, POISON_I8, POISON_F32 = 0x7F7F, 0xFF, 127, 0x7FC00001


def cuda(a):
    return torch.from_numpy(a).cuda()


def _same(got, want):
    for g, w in zip(got, want):
        if w is None:
            assert g is None
            continue
        g, w = g.cpu().numpy(), np.asarray(w)
        assert g.dtype == w.dtype and np.array_equal(g.view(f"u{g.itemsize}"), w.view(f"u{w.itemsize}"))


@pytest.mark.parametrize("geometry,setting", QR.PAIRS)
def test_s2_chip_warp_equals_the_twin(geometry, setting):
    """Chips over every tile edge and wholly outside; the same zone at 10 / 20 / 60 m, the next UTM zone, the southern hemisphere,
    EPSG:4326 and EPSG:3857; both strategies, with and without SCL, offset and range on and off."""
    want = QR.twin(geometry, setting)
    assert want[6] == 0
    args, kw = QR.run_args(geometry, setting, cuda)
    got = Q.warp_cut(*args, **kw)
    assert all(g.is_cuda for g in got[:3]) and got[3] is got[4] is got[5] is None
    _same(got[:3], want[:3])
    nd = QR.SETTINGS[setting][5]
    assert got[1][-1].item() == 0 and not got[2][-1].any() and (got[0][-1] == nd).all()  # the chip wholly outside


@pytest.mark.parametrize("geometry", ["edges_s32", "edges_s65", "geographic_s65", "coarse_60m_s65"])
def test_one_class_equals_ig_chip_warp(geometry):
    sc, sg, dc, dg, S = RR.GEOMETRY[geometry]
    tile, _ = RR.tile_of(3, 2)
    tile = np.maximum(tile, 0)
    TC, H, W = tile.shape
    labels = cuda(RR.label_maps(len(dg), S, np.int8, seed=2))
    want = raster_chips.warp_cut(cuda(tile), None, sc, sg, dc, dg, S, dates=3, no_data_value=0, labels=labels, label_strategy="any", num_classes=8)
    got = Q.warp_cut(cuda(tile.astype(np.uint16).reshape(-1)), np.arange(TC) * H * W, [0] * TC, [sg], [(H, W)], None, None, sc, dc, dg, S, dates=3,
                     labels=labels, valid_bit=1, classes=8)
    assert torch.equal(got[0].view(torch.int16), want[0])
    assert all(g.dtype == w.dtype and torch.equal(g, w) for g, w in zip(got[1:], want[1:]))


@pytest.mark.parametrize("name,option", [("c6_10m", "each"), ("c6_10m", "any_boa_nd7"), ("sixty", "each_boa_range"), ("t3c2", "any_range_nd65535"),
                                         ("t3c2", "no_scl")])
def test_a_shared_corner_equals_ig_s2_chip_cut(name, option):
    k, planes, scls = SR.make_case(name)
    bands, starts, geom = SR.pack(planes, np.uint16)
    scl, scl_starts, scl_geom = SR.pack(scls, np.uint8)
    strategy, with_scl, boa, rng, nd = SR.OPTIONS[option]
    S, origins = 32, SR.SIZES[32]
    b, s = cuda(bands), cuda(scl) if with_scl else None
    want = s2_chips.cut(b, starts, geom, s, scl_starts, scl_geom, origins, S, k["grid"], dates=k["T"], class_bits=SR.CLASS_BITS, strategy=strategy,
                        no_data_value=nd, boa_offset=boa, valid_range=rng)
    rows = [tuple(int(v) for v in g) for g in np.concatenate([geom, scl_geom] if with_scl else [geom])]
    classes = sorted(set(rows))
    grids = [(QR.X0, QR.Y0, float(p), float(p)) for _, _, p in classes]
    dst = [(QR.X0 + 10.0 * c0, QR.Y0 - 10.0 * r0, 10.0, 10.0) for r0, c0 in origins]
    got = Q.warp_cut(b, starts, [classes.index(r) for r in rows], grids, [(h, w) for h, w, _ in classes], s, scl_starts if with_scl else None,
                     QR.U36, QR.U36, dst, S, dates=k["T"], class_bits=SR.CLASS_BITS, strategy=strategy, no_data_value=nd, boa_offset=boa,
                     valid_range=rng)
    assert all(g.dtype == w.dtype and torch.equal(g, w) for g, w in zip(got[:3], want))


@pytest.mark.parametrize("geometry,setting,dtype,K", LABEL_CASES)
def test_label_maps_equal_the_twin(geometry, setting, dtype, K):
    args, kw = QR.run_args(geometry, setting, cuda)
    for bit in (0, 1, 2):
        labels, want = label_case(geometry, setting, dtype, K, bit)
        assert want[6] == 0
        got = Q.warp_cut(*args, labels=cuda(labels) if bit else labels, valid_bit=bit, classes=K, **kw)
        _same(got, want[:6])


@pytest.mark.parametrize("dtype,K", [(np.int8, 5), (np.float32, 0)])
def test_every_output_element_is_stored_and_nothing_beyond_from_odd_plane_starts(dtype, K):
    """Outputs pre-filled with values the kernel never writes, inside larger poisoned buffers; every plane starts at an odd element."""
    geometry, setting = ("same_20m_s65", 1) if dtype == np.int8 else ("geographic_s65", 0)
    args, kw = QR.run_args(geometry, setting, cuda, lead=3)
    assert all(int(s) % 2 == 1 for s in args[1]) and all(int(s) % 2 == 1 for s in args[6])
    labels, want = label_case(geometry, setting, dtype, K, 1)
    assert want[6] == 0
    n, S, TC = len(args[9]), args[10], len(args[1])
    pad = 64
    big = {"chips": torch.full((n * TC * S * S + 2 * pad,), POISON_CHIP, dtype=torch.uint16, device="cuda"),
           "validity": torch.full((n * S * S + 2 * pad,), POISON_PLANE, dtype=torch.uint8, device="cuda"),
           "maps": torch.full((n * S * S + 2 * pad,), POISON_I8, dtype=torch.int8, device="cuda") if dtype == np.int8
           else torch.full((n * S * S + 2 * pad,), POISON_F32, dtype=torch.int32, device="cuda").view(torch.float32)}
    out = {"chips": big["chips"][pad:-pad].view(n, TC, S, S), "validity": big["validity"][pad:-pad].view(n, S, S),
           "maps": big["maps"][pad:-pad].view(n, S, S)}
    got = ops.s2_chip_warp(*args[:10], S, kw["dates"], kw["class_bits"], kw["strategy"], kw["no_data_value"], kw["boa_offset"], kw["valid_range"],
                           labels, 1, K, out=out)
    assert got[0] is out["chips"] and got[2] is out["validity"] and got[3] is out["maps"]
    assert not (got[0] == POISON_CHIP).any() and not (got[2] == POISON_PLANE).any()
    bits = (lambda t: t.view(torch.int32)) if dtype == np.float32 else (lambda t: t)
    poison_map = POISON_F32 if dtype == np.float32 else POISON_I8
    assert not (bits(got[3]) == poison_map).any()
    _same(got, want[:6])
    for name, poison in (("chips", POISON_CHIP), ("validity", POISON_PLANE)):  # the guard bands are untouched
        assert (big[name][:pad] == poison).all() and (big[name][-pad:] == poison).all()
    assert (bits(big["maps"])[:pad] == poison_map).all() and (bits(big["maps"])[-pad:] == poison_map).all()


def test_two_launches_give_the_same_bits():
    args, kw = QR.run_args("geographic_s65", 1, cuda)
    labels = cuda(RR.label_maps(3, 65, np.int8, seed=1))
    a = Q.warp_cut(*args, labels=labels, valid_bit=2, classes=8, **kw)
    b = Q.warp_cut(*args, labels=labels, valid_bit=2, classes=8, **kw)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_unusable_grids_and_no_chips():
    args, kw = QR.run_args("same_10m_s32", 0, cuda)
    host, _ = QR.run_args("same_10m_s32", 0)
    grids = [QR.at(3, 3), (QR.X0, QR.Y0, 0.0, 10.0), (np.nan, QR.Y0, 10.0, 10.0), (QR.X0, QR.Y0, 10.0, np.inf)]
    got = Q.warp_cut(*args[:9], grids, 16, **{**kw, "no_data_value": 9})
    _same(got[:3], Q.warp_cut(*host[:9], grids, 16, **{**kw, "no_data_value": 9})[:3])
    assert got[1][0].item() > 0 and got[1].tolist()[1:] == [0, 0, 0] and (got[0][1:] == 9).all()
    none = Q.warp_cut(*args[:9], np.zeros((0, 4)), 16, **kw)
    assert tuple(none[0].shape) == (0, 9, 16, 16) and none[1].numel() == 0


def _raw(bands, starts, scl, scl_starts, plane_class, class_grid, class_size, dst_grids, S, T, nd):
    """``ig_s2_chip_warp`` without the host checks of ops.s2_chip_warp: tables as given -> (chips, valid_values, validity) on the host."""
    n, TC, G = len(dst_grids), len(starts), len(class_grid)
    dbl = cuda(np.concatenate([np.asarray(QR.U36, dtype=np.float64), np.asarray(QR.U36, dtype=np.float64),
                               np.asarray(class_grid, dtype=np.float64).reshape(-1), np.asarray(dst_grids, dtype=np.float64).reshape(-1)]))
    sd, ssd = cuda(np.asarray(starts, dtype=np.int64)), cuda(np.asarray(scl_starts, dtype=np.int64))
    pc, cs = cuda(np.asarray(plane_class, dtype=np.int32)), cuda(np.asarray(class_size, dtype=np.int32).reshape(-1))
    chips = torch.full((n, TC, S, S), POISON_CHIP, dtype=torch.uint16, device="cuda")
    valid = torch.zeros(n, dtype=torch.int32, device="cuda")
    plane = torch.full((n, S, S), POISON_PLANE, dtype=torch.uint8, device="cuda")
    p = lambda t: t.data_ptr()  # noqa: E731
    _lib.call("ig_s2_chip_warp", p(bands), p(sd), p(scl), p(ssd), p(pc), p(dbl[10 : 10 + 4 * G]), p(cs), G, p(dbl[0:5]), p(dbl[5:10]),
              p(dbl[10 + 4 * G :]), n, T, TC // T, S, QR.CLASS_BITS, 0, nd, 0, 0, 0, 0, None, 1, 0, 0, p(chips), p(valid), p(plane), None, None, None,
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return chips.cpu().numpy(), valid.cpu().numpy(), plane.cpu().numpy()


def test_a_table_entry_out_of_bounds_reads_nothing_and_gives_the_fill():
    """The kernel's own fence (ops.s2_chip_warp refuses these tables on the host): a class index outside [0, G), a negative start and a
    class of more than 2^31 - 1 pixels read nothing; their bands are no_data, their SCL planes class 0; the other planes are unaffected."""
    args, kw = QR.run_args("same_10m_s32", 0, cuda)
    bands, starts, pc, grids, sizes, scl, scl_starts = args[:7]
    dst, S, T, nd = [QR.at(40, 30), QR.at(-10, -7)], 32, 3, 9
    good = _raw(bands, starts, scl, scl_starts, pc, grids, sizes, dst, S, T, nd)
    planes, scls = QR.planes_of(3)
    want = QR.cut(planes, scls, QR.class_grids(), QR.U36, QR.U36, dst, S, T, QR.CLASS_BITS, "each", nd)
    assert want[6] == 0 and all(np.array_equal(g, w) for g, w in zip(good, want[:3]))
    bad_pc, bad_st, bad_sst = list(pc), np.array(starts), np.array(scl_starts)
    bad_pc[0], bad_pc[4] = 3, -1  # bands 0 and 4
    bad_st[8] = -5  # band 8
    bad_sst[1] = -1  # the SCL plane of date 1: class 0 everywhere, which CLASS_BITS masks
    big = np.array(sizes).copy()
    got = _raw(bands, bad_st, scl, bad_sst, bad_pc, grids, big, dst, S, T, nd)
    for b in (0, 4, 8):
        assert (got[0][:, b] == nd).all()
    assert (got[0][:, 3:6] == nd).all()  # date 1 is masked everywhere
    for b in (1, 2, 6, 7):
        assert np.array_equal(got[0][:, b], good[0][:, b])
    assert got[1].tolist() == [(got[0][i] != nd).sum() for i in range(2)] and not (got[2] == POISON_PLANE).any()
    big[0] = (65536, 65536)  # the 10 m class: every plane of it reads nothing
    got = _raw(bands, starts, scl, scl_starts, pc, grids, big, dst, S, T, nd)
    for b in (0, 3, 6):
        assert (got[0][:, b] == nd).all()
    for b in (1, 2, 4, 5, 7, 8):
        assert np.array_equal(got[0][:, b], good[0][:, b])


def test_create_s2_raster_chips_on_the_device_writes_the_bytes_of_the_host_path(tmp_path):
    planes, scls, files, scl_files, records, rasters = write_granule(str(tmp_path))
    outs = {}
    for dev in (None, "cuda"):
        out = str(tmp_path / f"out_{dev}")
        outs[dev] = (out, Q.create_s2_raster_chips(files, scl_files, records, rasters, out, device=dev, **KW))
    a, b = outs[None], outs["cuda"]
    assert a[1] == b[1] and len(a[1][0]) == 2
    seen = 0
    for root, _, names in os.walk(a[0]):
        for n in names:
            pa = os.path.join(root, n)
            assert open(pa, "rb").read() == open(os.path.join(b[0], os.path.relpath(pa, a[0])), "rb").read(), n
            seen += 1
    assert seen == 6 and sum(len(f) for _, _, f in os.walk(b[0])) == 6  # 2 chips, 2 label maps, the stats JSON and the dataset CSV
