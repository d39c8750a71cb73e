"""Chips and label maps on the device (-m gpu): ``ig_chip_cut`` and ``ig_chip_labels`` against the sequential twin of the rule
(tests/chips_reference.py), run-to-run determinism, and create_chips on the device against the host path, file for file.  Every
comparison is ``torch.equal``: all outputs are integers or copies."""
import os

import numpy as np
import pytest
import torch

import chips_reference as CR
from instageo_amd import chips
from test_cpu_chips import CUT_CASES, _points, _write_tile, cut_case

pytestmark = pytest.mark.gpu
BITS = 2 | 4 | 8 | 32
_twin_cache = {}


def _twin_cut(name, strategy, with_mask, clip):
    key = (name, strategy, with_mask, clip)
    if key not in _twin_cache:
        k, tile, fmask = cut_case(name)
        _twin_cache[key] = CR.cut(tile, fmask if with_mask else None, k["origins"], k["S"], k["T"], BITS, strategy, 0, clip)
    return _twin_cache[key]


def _same(got, want):
    for g, w in zip(got, want):
        w = torch.from_numpy(w)
        assert g.dtype == w.dtype and torch.equal(g.cpu(), w)


@pytest.mark.parametrize("name", list(CUT_CASES))
@pytest.mark.parametrize("strategy", ["each", "any"])
@pytest.mark.parametrize("with_mask,clip", [(True, None), (False, None), (True, (0, 10000))])
def test_chip_cut_equals_the_twin(name, strategy, with_mask, clip):
    k, tile, fmask = cut_case(name)
    t = torch.from_numpy(tile).cuda()
    f = torch.from_numpy(fmask).cuda() if with_mask else None
    got = chips.cut(t, f, k["origins"], k["S"], dates=k["T"], mask=BITS, strategy=strategy, clip=clip)
    assert all(g.is_cuda for g in got)
    _same(got, _twin_cut(name, strategy, with_mask, clip))
    if k["fully"] is not None and with_mask:
        i = k["origins"].index(k["fully"])
        assert got[1][i].item() == 0
        j = k["origins"].index(k["clean"])
        if clip is None:
            r, c = k["clean"]
            assert torch.equal(got[0][j], t[:, r : r + k["S"], c : c + k["S"]])


def test_chip_cut_single_bits_on_an_unaligned_view():
    """Each bit alone, a no-data value that is not 0, and a tile that starts 2 bytes off a 16-byte boundary."""
    k, tile, fmask = cut_case("t3c2_70x75_s32")
    buf = torch.zeros(tile.size + 1, dtype=torch.int16, device="cuda")
    t = buf[1:].view(tile.shape)
    t.copy_(torch.from_numpy(tile))
    f = torch.from_numpy(fmask).cuda()
    for name, pos in CR.POSITIONS.items():
        got = chips.cut(t, f, k["origins"], 32, mask=[name], strategy="each", no_data_value=-9999)
        _same(got, CR.cut(tile, fmask, k["origins"][:6], 32, 3, 1 << pos, "each", -9999))


LABEL_CASES = [  # S, w, points per chip
    (32, 0, [0, 1, 7]),
    (32, 2, [5, 0, 9]),
    (64, 3, [300]),
    (65, 3, [40, 3]),
    (128, 5, [25, 0]),
]


@pytest.mark.parametrize("S,w,counts", LABEL_CASES)
@pytest.mark.parametrize("dtype", [np.int16, np.float32])
def test_chip_labels_equal_the_twin(S, w, counts, dtype):
    rng = np.random.default_rng(S + w)
    origins = [(3 * i, 5 * i) for i in range(len(counts))]
    ptr, pts, labels = CR.random_points(origins, S, counts, seed=S * 7 + w)
    labels = labels.astype(dtype) + (dtype(0.25) if dtype == np.float32 else dtype(0))
    validity = rng.integers(0, 4, size=(len(counts), S, S)).astype(np.uint8)
    vd = torch.from_numpy(validity).cuda()
    K, task = (8, "seg") if dtype == np.int16 else (0, "reg")
    strategies = (("any", 1), ("each", 2)) if S != 128 else (("any", 1),)
    for strat, bit in strategies:
        got = chips.label_maps(origins, S, ptr, pts, labels, w, vd, strat, task, K)
        want = CR.label_maps(origins, S, ptr, pts, labels, w, validity, bit, K, dtype)
        _same(got[:2], want[:2])
        if K:
            _same(got[2:], want[2:])
        else:
            assert got[2] is None
    if S == 64:  # the same without a validity plane, and twice: the result does not depend on the order the atomics land in
        a = chips.label_maps(origins, S, ptr, pts, labels, w, None, None, task, K, device="cuda")
        b = chips.label_maps(origins, S, ptr, pts, labels, w, None, None, task, K, device="cuda")
        assert a[0].is_cuda
        _same(a[:2], CR.label_maps(origins, S, ptr, pts, labels, w, None, 0, K, dtype)[:2])
        assert all(torch.equal(x, y) for x, y in zip(a[:2], b[:2])) and (a[2] is None or torch.equal(a[2], b[2]))


def test_chip_labels_without_points_are_all_no_data():
    """No point in any chip: the kernel is handed the lists' stand-in pointers and a count of 0."""
    v = torch.full((1, 8, 8), 3, dtype=torch.uint8, device="cuda")
    none = np.zeros((0, 3), dtype=np.int32)
    for labels in (np.zeros(0, dtype=np.int16), np.array([1, 2], dtype=np.int16)):
        got = chips.label_maps([(0, 0)], 8, [0, 0], none, labels, 1, v, "any", "seg", 8)
        _same(got, CR.label_maps([(0, 0)], 8, [0, 0], none, labels, 1, v.cpu().numpy(), 1, 8, np.int16))
        assert (got[0] == -1).all() and not got[1].any() and not got[2].any()


def test_both_kernels_are_deterministic():
    k, tile, fmask = cut_case("t3c2_70x75_s32")
    t, f = torch.from_numpy(tile).cuda(), torch.from_numpy(fmask).cuda()
    a = chips.cut(t, f, k["origins"], 32, mask=BITS, strategy="any")
    b = chips.cut(t, f, k["origins"], 32, mask=BITS, strategy="any")
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    ptr, pts, labels = CR.random_points([(0, 0)], 64, [300], seed=11)
    v = torch.full((1, 64, 64), 3, dtype=torch.uint8, device="cuda")
    a = chips.label_maps([(0, 0)], 64, ptr, pts, labels, 3, v, "any", "seg", 8)
    b = chips.label_maps([(0, 0)], 64, ptr, pts, labels, 3, v, "any", "seg", 8)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_create_chips_on_the_device_writes_the_bytes_of_the_host_path(tmp_path):
    tile, fmask, files, fmasks = _write_tile(str(tmp_path / "tiles"))
    kw = dict(chip_size=16, mask_types=["cloud", "water"], masking_strategy="each", window_size=1, src_crs=32613)
    outs = {}
    for dev in (None, "cuda"):
        out = str(tmp_path / f"out_{dev}")
        outs[dev] = (out, chips.create_chips(files, fmasks, _points(), out, device=dev, **kw))
        out = str(tmp_path / f"grid_{dev}")
        outs[(dev, "grid")] = (out, chips.create_chips(files, fmasks, None, out, device=dev, chip_size=16, mask_types=["cloud"], masking_strategy="any"))
    for a, b in ((outs[None], outs["cuda"]), (outs[(None, "grid")], outs[("cuda", "grid")])):
        assert a[1] == b[1] and len(a[1][0]) >= 2
        for root, _, names in os.walk(a[0]):
            for n in names:
                pa = os.path.join(root, n)
                assert open(pa, "rb").read() == open(os.path.join(b[0], os.path.relpath(pa, a[0])), "rb").read(), n
