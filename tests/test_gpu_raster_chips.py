"""Chips warped onto label grids on the device (-m gpu): ``ig_chip_warp`` against ``ig_chip_cut`` on the same grid, against the sequential
twin (tests/raster_chips_reference.py) on chips that leave the tile, other pixel sizes and other coordinate systems, label maps, stores
into poisoned outputs from an unaligned tile, determinism, and create_raster_chips on the device against the host path, file for file.

Every case is one the twin reports free of ties (no pixel with u or v within 1e-6 of an integer: asserted before anything is compared;
the reasoning is that of tests/test_gpu_warp.py), so every comparison is ``torch.equal`` on all elements and all counts."""
import os

import numpy as np
import pytest
import torch

import raster_chips_reference as RR
from instageo_amd import chips, ops
from instageo_amd import raster_chips as R
from test_cpu_raster_chips import KW, LABEL_CASES, inputs, label_case, write_granule

pytestmark = pytest.mark.gpu
POISON_CHIP, POISON_PLANE, POISON_I8, POISON_F32 = 0x7F7F, 0xFF, 127, 0x7FC00001


def _dev(tile, fmask):
    return torch.from_numpy(tile).cuda(), None if fmask is None else torch.from_numpy(fmask).cuda()


def _same(got, want):
    for g, w in zip(got, want):
        if w is None:
            assert g is None
            continue
        g, w = g.cpu().numpy(), np.asarray(w)
        assert g.dtype == w.dtype and np.array_equal(g.view(f"u{g.itemsize}"), w.view(f"u{w.itemsize}"))


@pytest.mark.parametrize("S", [32, 65])
@pytest.mark.parametrize("T,C", [(1, 1), (3, 2)])
def test_same_grid_equals_ig_chip_cut(S, T, C):
    origins = [(0, 0), (100 - S, 90 - S), (7, 3)]
    grids = [RR.at(r, c) for r, c in origins]
    tile, fmask = RR.tile_of(T, C)
    t, f = _dev(tile, fmask)
    for strategy in ("each", "any"):
        for fm in (f, None):
            for clip in (None, (0, 10000)):
                for nd in (0, -9999):
                    want = chips.cut(t, fm, origins, S, dates=T, mask=RR.BITS, strategy=strategy, no_data_value=nd, clip=clip)
                    got = R.warp_cut(t, fm, RR.U36, RR.SRC_GRID, RR.U36, grids, S, dates=T, mask=RR.BITS, strategy=strategy, no_data_value=nd,
                                     clip=clip)
                    assert all(g.is_cuda and g.dtype == w.dtype and torch.equal(g, w) for g, w in zip(got[:3], want))
                    assert got[3] is got[4] is got[5] is None


@pytest.mark.parametrize("geometry,setting", RR.PAIRS)
def test_chip_warp_equals_the_twin(geometry, setting):
    """Chips over every tile edge and wholly outside, 10 m / 60 m / shifted grids, EPSG:4326 / 3857 / the next UTM zone / the southern
    hemisphere."""
    want = RR.twin(geometry, setting)
    assert want[6] == 0
    tile, fmask, kw = inputs(geometry, setting)
    t, f = _dev(tile, fmask)
    got = R.warp_cut(t, f, **kw)
    _same(got[:3], want[:3])
    if geometry == "edges_s32" and kw["clip"] is None:  # (a clip moves no_data itself when it lies outside the range)
        nd = kw["no_data_value"]
        assert got[1][5].item() == 0 and not got[2][5].any() and (got[0][5] == nd).all()  # the chip wholly outside
        assert (got[0][0][:, :10] == nd).all() and (got[0][0][:, :, :7] == nd).all() and not got[2][0][:10].any()
        assert got[1][0].item() == (got[0][0][:, 10:, 7:] != nd).sum().item() > 0


@pytest.mark.parametrize("geometry,setting,dtype,K", LABEL_CASES)
def test_label_maps_equal_the_twin(geometry, setting, dtype, K):
    tile, fmask, kw = inputs(geometry, setting)
    t, f = _dev(tile, fmask)
    for strat in (None, "any", "each"):
        labels, want = label_case(geometry, setting, dtype, K, strat)
        assert want[6] == 0
        got = R.warp_cut(t, f, labels=torch.from_numpy(labels).cuda() if strat else labels, label_strategy=strat, num_classes=K, **kw)
        _same(got, want[:6])


def test_unusable_grids_and_no_chips():
    tile, fmask = RR.tile_of(3, 2)
    t, f = _dev(tile, fmask)
    grids = [RR.at(3, 3), (RR.X0, RR.Y0, 0.0, 30.0), (np.nan, RR.Y0, 30.0, 30.0), (RR.X0, RR.Y0, 30.0, np.inf)]
    got = R.warp_cut(t, f, RR.U36, RR.SRC_GRID, RR.U36, grids, 16, mask=RR.BITS, no_data_value=-9999)
    _same(got[:3], R.warp_cut(tile, fmask, RR.U36, RR.SRC_GRID, RR.U36, grids, 16, mask=RR.BITS, no_data_value=-9999)[:3])
    assert got[1].tolist()[1:] == [0, 0, 0] and (got[0][1:] == -9999).all()
    none = R.warp_cut(t, f, RR.U36, RR.SRC_GRID, RR.U36, np.zeros((0, 4)), 16)
    assert tuple(none[0].shape) == (0, 6, 16, 16) and none[1].numel() == 0


@pytest.mark.parametrize("dtype,K", [(np.int8, 8), (np.float32, 0)])
def test_every_output_element_is_stored_from_an_unaligned_tile(dtype, K):
    """Outputs pre-filled with values the kernel never writes; the tile starts 2 bytes off a 16-byte boundary."""
    geometry, setting = "edges_s65", 0
    tile, fmask, kw = inputs(geometry, setting)
    labels, want = label_case(geometry, setting, dtype, K, "any")
    buf = torch.zeros(tile.size + 1, dtype=torch.int16, device="cuda")
    t = buf[1:].view(tile.shape)
    t.copy_(torch.from_numpy(tile))
    assert t.data_ptr() % 16 == 2
    n, S, TC = len(kw["dst_grids"]), kw["chip_size"], tile.shape[0]
    out = {"chips": torch.full((n, TC, S, S), POISON_CHIP, dtype=torch.int16, device="cuda"),
           "validity": torch.full((n, S, S), POISON_PLANE, dtype=torch.uint8, device="cuda"),
           "maps": torch.full((n, S, S), POISON_I8, dtype=torch.int8, device="cuda") if dtype == np.int8
           else torch.full((n, S, S), POISON_F32, dtype=torch.int32, device="cuda").view(torch.float32)}
    got = ops.chip_warp(t, torch.from_numpy(fmask).cuda(), kw["src_crs"], kw["src_grid"], kw["dst_crs"], kw["dst_grids"], S, kw["dates"], RR.BITS,
                        kw["strategy"], kw["no_data_value"], kw["clip"], labels, 1, K, out=out)
    assert got[0] is out["chips"] and got[2] is out["validity"] and got[3] is out["maps"]
    assert not (got[0] == POISON_CHIP).any() and not (got[2] == POISON_PLANE).any()
    m = got[3].view(torch.int32) if dtype == np.float32 else got[3]
    assert not (m == (POISON_F32 if dtype == np.float32 else POISON_I8)).any()
    _same(got, want[:6])


def test_two_launches_give_the_same_bits():
    tile, fmask, kw = inputs("geographic_s65", 0)
    t, f = _dev(tile, fmask)
    labels = torch.from_numpy(RR.label_maps(2, 65, np.int8, seed=1)).cuda()
    a = R.warp_cut(t, f, labels=labels, label_strategy="each", num_classes=8, **kw)
    b = R.warp_cut(t, f, labels=labels, label_strategy="each", num_classes=8, **kw)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_create_raster_chips_on_the_device_writes_the_bytes_of_the_host_path(tmp_path):
    tile, fmask, files, fmasks, records, rasters = write_granule(str(tmp_path))
    outs = {}
    for dev in (None, "cuda"):
        out = str(tmp_path / f"out_{dev}")
        outs[dev] = (out, R.create_raster_chips(files, fmasks, records, rasters, out, device=dev, **KW))
    a, b = outs[None], outs["cuda"]
    assert a[1] == b[1] and len(a[1][0]) == 2
    seen = 0
    for root, _, names in os.walk(a[0]):
        for n in names:
            pa = os.path.join(root, n)
            assert open(pa, "rb").read() == open(os.path.join(b[0], os.path.relpath(pa, a[0])), "rb").read(), n
            seen += 1
    assert seen == 6 and sum(len(f) for _, _, f in os.walk(b[0])) == 6  # 2 chips, 2 label maps, the stats JSON and the dataset CSV
