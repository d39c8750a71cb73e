"""Sentinel-1 chips on the device (-m gpu): ``ig_s1_chip_cut`` against the sequential twin (tests/s1_chips_reference.py) on the cases the
host path is compared on (values and fills, slices in either order, a corner per date, the next UTM zone, the southern hemisphere, a
clip), label maps from its validity plane, stores into poisoned outputs from an unaligned buffer, determinism, and create_s1_chips on the
device against the host path, file for file.

Every case is one the twin reports free of ties (no pixel with u or v within 1e-6 of an integer for any scene: asserted before anything is
compared; the reasoning is that of tests/test_gpu_warp.py), so every comparison is ``array_equal`` on the bit patterns of all elements and
all counts."""
import os

import numpy as np
import pytest
import torch

import chips_reference as CR
import s1_chips_reference as VR
from instageo_amd import chips, ops
from instageo_amd import s1_chips as V
from test_cpu_s1_chips import S as FILE_S
from test_cpu_s1_chips import write_stack

pytestmark = pytest.mark.gpu
POISON_CHIP, POISON_PLANE = 0x7FC0BEEF, 0xFF  # a NaN pattern the kernel never writes (NaN is never copied), a byte above 3


def _cut(name, **extra):
    k = VR.case(name)
    return V.cut(torch.from_numpy(k["planes"]).cuda(), **{**VR.product_args(k), **extra})


@pytest.mark.parametrize("name", VR.CASES)
def test_cut_equals_the_twin(name):
    """S in {8, 64, 80} (80: a ragged second block), (T, C) in {(1, 1), (3, 2)}, chips inside, over each edge, wholly outside and at
    negative origins, NaN / src_nodata / -1 / -0.0 / denormals / infinities copied or skipped, two overlapping slices in either order, a
    corner per date (the affine path), a date in the next UTM zone and a southern stack (the projection path), a clip."""
    want = VR.twin(name)
    assert want[3] == 0
    got = _cut(name)
    assert all(g.is_cuda for g in got)
    assert all(VR.same_bits(g.cpu().numpy(), w) for g, w in zip(got, want[:3]))


@pytest.mark.parametrize("name", ["values_s80_t3c2", "slices", "next_zone"])
def test_every_output_element_is_stored_from_an_unaligned_buffer(name):
    """Outputs pre-filled with values the kernel never writes, counters pre-loaded (they are only added to); the planes start 4 bytes past
    a 16-byte boundary; two runs give the same bits."""
    k, want = VR.case(name), VR.twin(name)
    assert want[3] == 0
    buf = torch.zeros(k["planes"].size + 1, dtype=torch.float32, device="cuda")
    planes = buf[1:]
    planes.copy_(torch.from_numpy(k["planes"]))
    assert planes.data_ptr() % 16 == 4
    a = VR.product_args(k)
    n, S, TC = len(k["origins"]), k["S"], want[0].shape[1]
    runs = []
    for _ in range(2):
        out = {"chips": torch.full((n, TC, S, S), POISON_CHIP, dtype=torch.int32, device="cuda").view(torch.float32),
               "validity": torch.full((n, S, S), POISON_PLANE, dtype=torch.uint8, device="cuda")}
        got = ops.s1_chip_cut(planes, a["starts"], a["scene_crs"], a["scene_grid"], a["scene_size"], a["date_scenes"], a["dst_crs"], a["dst_grid"],
                              a["origins"], S, a["no_data_value"], a["src_nodata"], a["clip"], out=out)
        assert got[0] is out["chips"] and got[2] is out["validity"]
        assert not (got[0].view(torch.int32) == POISON_CHIP).any() and not (got[2] == POISON_PLANE).any()
        assert all(VR.same_bits(g.cpu().numpy(), w) for g, w in zip(got, want[:3]))
        runs.append(got)
    assert all(torch.equal(x.view(torch.uint8) if x.dtype == torch.float32 else x, y.view(torch.uint8) if y.dtype == torch.float32 else y)
               for x, y in zip(*runs))


def test_counters_are_only_added_to():
    """valid_values is added to what the caller left there (the wrapper zeroes it; the raw op does not)."""
    from instageo_amd import torch_ops

    torch_ops.register()
    k, want = VR.case("values_s8_t3c2"), VR.twin("values_s8_t3c2")
    st, sc, sg, ss, first_bits, T, C, dc, dg, o, nd, snd, clip = V.check_cut(k["planes"].size, **{kk: v for kk, v in VR.product_args(k).items() if kk != "chip_size"},
                                                                            S=k["S"])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    n, S = o.shape[0], k["S"]
    chips_ = torch.empty((n, T * C, S, S), dtype=torch.float32, device="cuda")
    valid = torch.full((n,), 1000, dtype=torch.int32, device="cuda")
    torch.ops.instageo_mi355x.s1_chip_cut(dev(k["planes"]), dev(st), dev(sc), dev(sg), dev(ss), sg.shape[0], first_bits, dev(dc), dev(dg), dev(o), n, T, C, S,
                                          float(nd), 1, float(snd), 0, 0.0, 0.0, chips_, valid, None)
    assert np.array_equal(valid.cpu().numpy(), want[1] + 1000) and VR.same_bits(chips_.cpu().numpy(), want[0])


@pytest.mark.parametrize("task,dtype", [("seg", np.int16), ("reg", np.float32)])
def test_label_maps_from_the_validity_plane_equal_the_twin(task, dtype):
    name = "slices"
    k, want = VR.case(name), VR.twin(name)
    assert want[3] == 0
    got = _cut(name)
    S, origins = k["S"], k["origins"]
    ptr, pts, labels = CR.random_points(origins, S, [9, 7, 8, 3, 4], seed=5, label_values=(0, 1, 2, 3, 7))
    lab = labels.astype(dtype)
    for strategy, bit in (("each", 2), ("any", 1)):
        maps, valid_labels, hist = chips.label_maps(origins, S, ptr, pts, lab, 2, got[2], strategy, task, 8 if task == "seg" else 0)
        w_maps, w_valid, w_hist = CR.label_maps(origins, S, ptr, pts, lab, 2, want[2], bit, 8 if task == "seg" else 0, dtype)
        assert maps.is_cuda and VR.same_bits(maps.cpu().numpy(), w_maps) and np.array_equal(valid_labels.cpu().numpy(), w_valid)
        assert (hist is None) == (w_hist is None) and (hist is None or np.array_equal(hist.cpu().numpy(), w_hist))


def test_no_chips_and_an_unusable_stack_grid():
    k = VR.case("values_s8_t1c1")
    none = _cut("values_s8_t1c1", origins=np.zeros((0, 2), dtype=np.int32))
    assert tuple(none[0].shape) == (0, 1, 8, 8) and none[1].numel() == 0
    dead = _cut("values_s8_t1c1", dst_grid=(VR.X0, VR.Y0, float("nan"), 10.0))
    assert (dead[0] == -1).all() and not dead[1].any() and not dead[2].any() and dead[0].shape[0] == len(k["origins"])


def test_create_s1_chips_on_the_device_writes_the_bytes_of_the_host_path(tmp_path):
    scenes, _, _, table = write_stack(str(tmp_path / "in"))
    outs = {}
    for dev in (None, "cuda"):
        out = str(tmp_path / f"out_{dev}")
        outs[dev] = (out, V.create_s1_chips(scenes, table, out, chip_size=FILE_S, src_nodata=-32768.0, masking_strategy="any", device=dev))
    a, b = outs[None], outs["cuda"]
    assert a[1] == b[1] and len(a[1][0]) == 3
    seen = 0
    for root, _, names in os.walk(a[0]):
        for n in names:
            pa = os.path.join(root, n)
            assert open(pa, "rb").read() == open(os.path.join(b[0], os.path.relpath(pa, a[0])), "rb").read(), n
            seen += 1
    assert seen == 8 and sum(len(f) for _, _, f in os.walk(b[0])) == 8  # 3 chips, 3 label maps, the stats JSON and the dataset CSV
