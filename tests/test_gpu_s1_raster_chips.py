"""Sentinel-1 chips on label grids on the device (-m gpu): ``ig_s1_chip_warp`` against the sequential twin
(tests/s1_raster_chips_reference.py) on the cases the host path is compared on, stores into poisoned outputs from an unaligned buffer,
determinism, the identity with ``ig_s1_chip_cut`` on an exact lattice, and create_s1_raster_chips on the device against the host path, file
for file.

Every case is one the twin reports free of ties (no pixel with u or v within 1e-6 of an integer for any scene: asserted before anything is
compared; the reasoning is that of tests/test_gpu_warp.py), so every comparison is ``array_equal`` on the bit patterns of all elements and
all counts."""
import os

import numpy as np
import pytest
import torch

import s1_chips_reference as VR
import s1_raster_chips_reference as XR
from instageo_amd import ops, s1_chips
from instageo_amd import s1_raster_chips as M
from test_cpu_s1_raster_chips import KW, exact_lattice, write_labels, write_stack

pytestmark = pytest.mark.gpu
POISON_CHIP, POISON_BYTE = 0x7FC0BEEF, 0xFF  # a NaN pattern the kernel never writes (NaN is never copied), a byte above 3 / an int8 of -1's bits


def _host(t):
    return None if t is None else t.cpu().numpy()


def _warp(name, **extra):
    k = XR.case(name)
    return M.warp_cut(torch.from_numpy(k["planes"]).cuda(), **{**XR.product_args(k), **extra})


@pytest.mark.parametrize("name", XR.CASES)
def test_warp_cut_equals_the_twin(name):
    """S in {8, 64, 80} (80: a ragged second block), (T, C) in {(1, 1), (3, 2)}; label grids in the scenes' zone (the affine path) with a
    finer and a coarser pixel, in EPSG:4326 and 3857 (the projection path for every scene), in the next zone, over a southern stack; chips
    inside, over each edge, outside, on unusable grids; slices in either order; int8 / float32 / no labels, valid_bit 0 / 1 / 2, K 0 / 8."""
    want = XR.twin(name)
    assert want[6] == 0
    got = _warp(name)
    assert all(g is None or g.is_cuda for g in got)
    assert all(XR.same_bits(_host(g), w) for g, w in zip(got, want[:6]))


@pytest.mark.parametrize("name", ["affine_s80_t3c2", "slices", "next_zone"])
def test_every_output_element_is_stored_from_an_unaligned_buffer(name):
    """Outputs pre-filled with patterns the kernel never writes in a chip or a validity plane (0xFF in an int8 map is -1, which it does
    write: the maps are compared with the twin element for element); the three counters pre-loaded: they are only added to (the raw op;
    the wrapper zeroes them); the planes start 4 bytes past a 16-byte boundary; a second run, through the wrapper's ``out=``, gives the
    same bits."""
    from instageo_amd import torch_ops

    torch_ops.register()
    k, want = XR.case(name), XR.twin(name)
    assert want[6] == 0 and k["labels"].dtype == np.int8 and k["K"] == 8 and k["clip"] is None
    buf = torch.zeros(k["planes"].size + 1, dtype=torch.float32, device="cuda")
    planes = buf[1:]
    planes.copy_(torch.from_numpy(k["planes"]))
    assert planes.data_ptr() % 16 == 4
    a = XR.product_args(k)
    st, sc, sg, ss, first_bits, T, C, dc, dg, nd, snd, _ = M.check_warp(k["planes"].size, a["starts"], a["scene_crs"], a["scene_grid"], a["scene_size"],
                                                                       a["date_scenes"], a["dst_crs"], a["dst_grids"], k["S"], a["no_data_value"],
                                                                       a["src_nodata"], None, k["labels"].shape, "int8", k["bit"], k["K"])
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    n, S, K = dg.shape[0], k["S"], k["K"]

    def poisoned():
        return {"chips": torch.full((n, T * C, S, S), POISON_CHIP, dtype=torch.int32, device="cuda").view(torch.float32),
                "validity": torch.full((n, S, S), POISON_BYTE, dtype=torch.uint8, device="cuda"),
                "maps": torch.full((n, S, S), POISON_BYTE, dtype=torch.uint8, device="cuda").view(torch.int8)}

    out = poisoned()
    valid, valid_labels = (torch.full((n,), v, dtype=torch.int32, device="cuda") for v in (1000, 2000))
    hist = torch.full((n, K), 3000, dtype=torch.int32, device="cuda")
    torch.ops.instageo_mi355x.s1_chip_warp(planes, dev(st), dev(sc), dev(sg), dev(ss), sg.shape[0], first_bits, dev(dc), dev(dg), n, T, C, S, float(nd),
                                           int(snd is not None), float(snd) if snd is not None else 0.0, 0, 0.0, 0.0, dev(k["labels"]), 1, k["bit"], K,
                                           out["chips"], valid, out["validity"], out["maps"], valid_labels, hist)
    first = (out["chips"], valid - 1000, out["validity"], out["maps"], valid_labels - 2000, hist - 3000)
    out = poisoned()
    second = ops.s1_chip_warp(planes, a["starts"], a["scene_crs"], a["scene_grid"], a["scene_size"], a["date_scenes"], a["dst_crs"], a["dst_grids"], S,
                              a["no_data_value"], a["src_nodata"], None, a["labels"], k["bit"], K, out=out)
    assert second[0] is out["chips"] and second[2] is out["validity"] and second[3] is out["maps"]
    for got in (first, second):
        assert not (got[0].view(torch.int32) == POISON_CHIP).any() and not (got[2] == POISON_BYTE).any()
        assert all(XR.same_bits(_host(g), w) for g, w in zip(got, want[:6]))
    assert (want[3] != -1).any() and want[5].sum() > 0
    assert all(torch.equal(x.view(torch.uint8) if x.dtype == torch.float32 else x, y.view(torch.uint8) if y.dtype == torch.float32 else y)
               for x, y in zip(first, second))


def test_windows_of_the_stack_lattice_give_the_chips_of_ig_s1_chip_cut():
    planes, scene, grid, origins = exact_lattice()
    p = torch.from_numpy(planes).cuda()
    for size in (24, 65):
        want = s1_chips.cut(p, **scene, dst_crs=32636, dst_grid=grid, origins=origins, chip_size=size, src_nodata=-32768.0)
        windows = [(grid[0] + 10.0 * c, grid[1] - 10.0 * r, 10.0, 10.0) for r, c in origins]
        got = M.warp_cut(p, **scene, dst_crs=32636, dst_grids=windows, chip_size=size, src_nodata=-32768.0)
        assert all(g.is_cuda and VR.same_bits(_host(g), _host(w)) for g, w in zip(got[:3], want)) and got[3] is None
        assert int(want[1][0]) > 0 and int(want[1][4]) == 0


def test_no_chips_and_an_unusable_destination_grid():
    k = XR.case("affine_s8_t1c1")
    none = _warp("affine_s8_t1c1", dst_grids=np.zeros((0, 4)))
    assert tuple(none[0].shape) == (0, 1, 8, 8) and none[1].numel() == 0 and none[3] is None
    grids = [(VR.X0, VR.Y0, float("nan"), 10.0), (VR.X0, VR.Y0, 10.0, -10.0), (float("inf"), VR.Y0, 10.0, 10.0)]
    lab = np.ones((3, 8, 8), dtype=np.int8)
    dead = _warp("affine_s8_t1c1", dst_grids=grids, labels=lab, label_strategy="each", num_classes=4)
    assert (dead[0] == -1).all() and not dead[1].any() and not dead[2].any() and dead[0].shape[0] == 3
    assert (dead[3] == -1).all() and not dead[4].any() and not dead[5].any()
    assert k["labels"] is None


def test_create_s1_raster_chips_on_the_device_writes_the_bytes_of_the_host_path(tmp_path):
    scenes, _, _, _ = write_stack(str(tmp_path / "in"))
    table, _ = write_labels(str(tmp_path / "labels"))
    outs = {}
    for dev in (None, "cuda"):
        out = str(tmp_path / f"out_{dev}")
        outs[dev] = (out, M.create_s1_raster_chips(scenes, table, str(tmp_path / "labels"), out, masking_strategy="any", device=dev, **KW))
    a, b = outs[None], outs["cuda"]
    assert a[1] == b[1] and len(a[1][0]) == 3
    seen = 0
    for root, _, names in os.walk(a[0]):
        for n in names:
            pa = os.path.join(root, n)
            assert open(pa, "rb").read() == open(os.path.join(b[0], os.path.relpath(pa, a[0])), "rb").read(), n
            seen += 1
    assert seen == 8 and sum(len(f) for _, _, f in os.walk(b[0])) == 8  # 3 chips, 3 label maps, the stats JSON and the dataset CSV
