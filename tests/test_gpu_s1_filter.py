"""``ig_s1_speckle`` on the device against the sequential twin of the rule (tests/s1_filter_reference.py) at the smallest shapes where the
kernel can go wrong: 1 x 1 and 3 x 2 (smaller than any window), 5 x 37 (narrower than a tile, an odd pitch), 17 x 129 and 70 x 70 (several
tiles of 64 x 32 both ways with ragged edges: halos cross the seams), three planes of different sizes in one launch (every second one
starts at an odd element) and a plane with nothing present; h = 1, 3 and 7, src_nodata given and not.  The input buffer starts one
element off, so a plane starts 4-byte but not 16-byte aligned.

boxcar and lee in linear scale use correctly rounded float64 operations only: bit for bit.  gamma_map (sqrt) and every dB output (log10)
go through a library function on either side, each within about one float64 ulp of the exact value, so the float32 roundings can differ
only next to a rounding tie: at most 1 float32 ulp, measured on the int32 bit views, with equal absent / dropped patterns and counts.  For
gamma_map the inputs are strictly positive, so that y > 0 does not hinge on the last bit."""
import os

import numpy as np
import pytest
import torch

import s1_filter_reference as R
from instageo_amd import s1_filter as F

pytestmark = pytest.mark.gpu


def on_device(k):
    planes = torch.from_numpy(k["planes"].copy()).cuda()[1:]
    assert planes.data_ptr() % 16 == 4
    return planes


def check(name, positive, method, scale, exact):
    k = R.case(name, positive)
    planes = on_device(k)
    for h, with_snd in R.RUNS[positive]:
        out, counts = F.speckle(planes, k["starts"], k["sizes"], 2 * h + 1, method, R.LOOKS, R.SND if with_snd else None, scale)
        assert out.is_cuda and counts.is_cuda and out.dtype == torch.float32 and counts.dtype == torch.int32
        got, want = R.bits_of(out.cpu().numpy()), R.expected(name, positive, h, with_snd, method, scale)
        assert np.array_equal(counts.cpu().numpy(), want[1]), (h, counts.cpu().tolist(), want[1].tolist())
        absent = want[0] == R.QNAN
        assert np.array_equal(got == R.QNAN, absent), (h, "the absent / dropped pattern")
        worst = R.ulps(got, want[0])
        print(f"{name} positive={positive} h={h} {method} {scale}: {int((got != want[0]).sum())} of {got.size} differ, at most {worst} ulp")
        if exact:
            assert np.array_equal(got, want[0]), (h, int((got != want[0]).sum()), worst)
        else:
            assert np.isfinite(got.view(np.float32)[~absent]).all() and worst <= 1, (h, worst)


@pytest.mark.parametrize("method", ["boxcar", "lee"])
@pytest.mark.parametrize("name", list(R.CASES))
def test_boxcar_and_lee_linear_equal_the_twin_bit_for_bit(name, method):
    check(name, False, method, "linear", exact=True)
    check(name, True, method, "linear", exact=True)


@pytest.mark.parametrize("name", list(R.CASES))
def test_gamma_map_within_one_ulp_on_positive_values(name):
    check(name, True, "gamma_map", "linear", exact=False)
    check(name, True, "gamma_map", "db", exact=False)


@pytest.mark.parametrize("method", ["boxcar", "lee"])
@pytest.mark.parametrize("name", list(R.CASES))
def test_db_within_one_ulp_with_equal_dropped_patterns(name, method):
    check(name, False, method, "db", exact=False)
    check(name, True, method, "db", exact=False)


def _tables(k):
    sizes = np.array(k["sizes"], dtype=np.int32)
    return [torch.from_numpy(a).cuda() for a in (k["starts"].copy(), sizes.reshape(-1), F.tile_table(sizes))]


@pytest.mark.parametrize("name", ["three", "seams"])
def test_every_element_is_written_once_and_runs_repeat(name):
    """The raw op on poisoned outputs: an element that is not written keeps the poison; the counts add up to the pixels."""
    from instageo_amd import torch_ops

    torch_ops.register()
    k = R.case(name, True)
    planes = on_device(k)
    starts, sizes, tile_ptr = _tables(k)
    N, total = len(k["sizes"]), planes.shape[0]
    runs = []
    for poison in (0x5A5A5A5A, 0x25252525):
        out = torch.full((total + 1,), poison, dtype=torch.int32, device="cuda")[1:].view(torch.float32)
        counts = torch.zeros((N, 2), dtype=torch.int32, device="cuda")
        torch.ops.instageo_mi355x.s1_speckle(planes, starts, sizes, tile_ptr, N, total, int(tile_ptr[-1]), 7, 1, R.LOOKS, 1, R.SND, 0, out, counts)
        got = R.bits_of(out.cpu().numpy())
        assert not (got == poison).any()
        runs.append((got, counts.cpu().numpy()))
    want = R.expected(name, True, 7, True, "lee", "linear")
    pixels = np.array([H * W for H, W in k["sizes"]])
    for got, counts in runs:
        assert np.array_equal(got, want[0]) and np.array_equal(counts, want[1])
        absent = np.array([int((want[0][int(s) : int(s) + p] == R.QNAN).sum()) for s, p in zip(k["starts"], pixels)])
        assert (counts.sum(axis=1) + absent == pixels).all()
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    # nothing absent: the counts are the pixels
    ones = torch.ones(total, dtype=torch.float32, device="cuda")
    out = torch.full((total,), float("inf"), dtype=torch.float32, device="cuda")
    counts = torch.zeros((N, 2), dtype=torch.int32, device="cuda")
    torch.ops.instageo_mi355x.s1_speckle(ones, starts, sizes, tile_ptr, N, total, int(tile_ptr[-1]), 3, 2, R.LOOKS, 0, 0.0, 1, out, counts)
    assert (out == 0).all() and counts.cpu().tolist() == [[int(p), 0] for p in pixels]  # 10 log10(1)


def test_a_plane_whose_stated_size_is_not_positive_is_skipped():
    """The second fence: the tables are on the device, so the kernel does not trust them."""
    from instageo_amd import torch_ops

    torch_ops.register()
    k = R.case("three", False)
    planes = on_device(k)
    starts, sizes, tile_ptr = _tables(k)
    N, total = 3, planes.shape[0]
    want = R.expected("three", False, 3, False, "boxcar", "linear")
    lo, hi = int(k["starts"][1]), int(k["starts"][2])
    for bad in ((0, 65), (33, -1), (2**16, 2**16)):  # H = 0, W < 0, H * W beyond 2^31 - 1: the tiles of the plane find nothing to do
        broken = sizes.clone()
        broken[2], broken[3] = bad
        out = torch.full((total,), 0x5A5A5A5A, dtype=torch.int32, device="cuda").view(torch.float32)
        counts = torch.zeros((N, 2), dtype=torch.int32, device="cuda")
        torch.ops.instageo_mi355x.s1_speckle(planes, starts, broken, tile_ptr, N, total, int(tile_ptr[-1]), 3, 0, R.LOOKS, 0, 0.0, 0, out, counts)
        got = R.bits_of(out.cpu().numpy())
        assert (got[lo:hi] == 0x5A5A5A5A).all() and np.array_equal(got[:lo], want[0][:lo]) and np.array_equal(got[hi:], want[0][hi:])
        assert counts.cpu().tolist() == [want[1][0].tolist(), [0, 0], want[1][2].tolist()]
    # a start that is negative or whose plane would end beyond the buffer, and a workgroup beyond its plane's own tiles
    for at in (-1, total - 33 * 65 + 1):
        moved = starts.clone()
        moved[1] = at
        out = torch.full((total,), 0x5A5A5A5A, dtype=torch.int32, device="cuda").view(torch.float32)
        counts = torch.zeros((N, 2), dtype=torch.int32, device="cuda")
        torch.ops.instageo_mi355x.s1_speckle(planes, moved, sizes, tile_ptr, N, total, int(tile_ptr[-1]), 3, 0, R.LOOKS, 0, 0.0, 0, out, counts)
        got = R.bits_of(out.cpu().numpy())
        assert (got[lo:hi] == 0x5A5A5A5A).all() and np.array_equal(got[:lo], want[0][:lo]) and np.array_equal(got[hi:], want[0][hi:])
    more = tile_ptr.clone()
    more[3] += 5
    out = torch.full((total,), 0x5A5A5A5A, dtype=torch.int32, device="cuda").view(torch.float32)
    counts = torch.zeros((N, 2), dtype=torch.int32, device="cuda")
    torch.ops.instageo_mi355x.s1_speckle(planes, starts, sizes, more, N, total, int(more[-1]), 3, 0, R.LOOKS, 0, 0.0, 0, out, counts)
    assert np.array_equal(R.bits_of(out.cpu().numpy()), want[0]) and np.array_equal(counts.cpu().numpy(), want[1])


def test_filter_s1_on_the_device_writes_the_bytes_of_the_host_path(tmp_path):
    scenes, _ = R.write_scenes(str(tmp_path / "in"), tagged=True)
    names = [os.path.basename(f) for d in scenes for s in d for f in s]
    for method in ("boxcar", "lee"):
        host, dev = str(tmp_path / f"host_{method}"), str(tmp_path / f"dev_{method}")
        F.filter_s1(scenes, host, method=method, window=7)
        written = F.filter_s1(scenes, dev, method=method, window=7, device="cuda")
        assert [os.path.basename(f) for d in written for s in d for f in s] == names
        for n in names + ["filter_stats.json"]:
            assert open(os.path.join(host, n), "rb").read() == open(os.path.join(dev, n), "rb").read(), (method, n)
