"""``ig_s1_refined_lee`` on the device against the sequential twin of the rule (tests/s1_refined_lee_reference.py) on the shared cases of
tests/s1_filter_reference.py: 1 x 1 and 3 x 2 (smaller than the window), 5 x 37 (narrower than a tile, an odd pitch), 17 x 129 and 70 x 70
(several tiles of 64 x 32 both ways with ragged edges: the halo and the sub-window centres cross the seams), three planes of different
sizes in one launch and a plane with nothing present; src_nodata given and not.  The input buffer starts one element off, so a plane
starts 4-byte but not 16-byte aligned.

Only correctly rounded float64 operations occur before the dB step: the linear scale is compared bit for bit.  dB goes through log10 on
either side, each within about one float64 ulp of the exact value, so the float32 roundings can differ only next to a rounding tie: at
most 1 float32 ulp on the int32 bit views, with equal absent / dropped patterns and counts."""
import os

import numpy as np
import pytest
import torch

import s1_filter_reference as R
import s1_refined_lee_reference as RL
from instageo_amd import s1_filter as F

pytestmark = pytest.mark.gpu


def on_device(k):
    planes = torch.from_numpy(k["planes"].copy()).cuda()[1:]
    assert planes.data_ptr() % 16 == 4
    return planes


@pytest.mark.parametrize("positive", [False, True])
@pytest.mark.parametrize("name", list(R.CASES))
def test_device_equals_the_twin(name, positive):
    k = R.case(name, positive)
    planes = on_device(k)
    for with_snd in (False, True):
        for scale in R.SCALES:
            out, counts = F.speckle(planes, k["starts"], k["sizes"], 7, "refined_lee", R.LOOKS, R.SND if with_snd else None, scale)
            assert out.is_cuda and counts.is_cuda and out.dtype == torch.float32 and counts.dtype == torch.int32
            got, (want, wcounts) = R.bits_of(out.cpu().numpy()), RL.expected(name, positive, with_snd, scale)
            worst = R.ulps(got, want)
            print(f"{name} positive={positive} src_nodata={with_snd} {scale}: {int((got != want).sum())} of {got.size} differ, at most {worst} ulp")
            assert np.array_equal(counts.cpu().numpy(), wcounts), (with_snd, scale, counts.cpu().tolist(), wcounts.tolist())
            assert np.array_equal(got == R.QNAN, want == R.QNAN), (with_snd, scale, "the absent / dropped pattern")
            if scale == "linear":
                assert np.array_equal(got, want), (with_snd, int((got != want).sum()), worst)
            else:
                assert np.isfinite(got.view(np.float32)[want != R.QNAN]).all() and worst <= 1, (with_snd, worst)


@pytest.mark.parametrize("name", ["three", "seams"])
def test_runs_repeat_and_elements_outside_every_plane_stay(name):
    """The raw op on poisoned outputs: every element of a plane is written, and two runs give the same bits and counts; through the
    wrapper, with a gap between the planes, the elements outside every plane are 0."""
    from instageo_amd import torch_ops

    torch_ops.register()
    k = R.case(name, True)
    planes = on_device(k)
    sizes_h = np.array(k["sizes"], dtype=np.int32)
    starts, sizes, tile_ptr = [torch.from_numpy(a).cuda() for a in (k["starts"].copy(), sizes_h.reshape(-1), F.tile_table(sizes_h))]
    N, total = len(k["sizes"]), planes.shape[0]
    want = RL.expected(name, True, True, "linear")
    runs = []
    for poison in (0x5A5A5A5A, 0x25252525):
        out = torch.full((total + 1,), poison, dtype=torch.int32, device="cuda")[1:].view(torch.float32)
        counts = torch.zeros((N, 2), dtype=torch.int32, device="cuda")
        torch.ops.instageo_mi355x.s1_refined_lee(planes, starts, sizes, tile_ptr, N, total, int(tile_ptr[-1]), R.LOOKS, 1, R.SND, 0, out, counts)
        got = R.bits_of(out.cpu().numpy())
        assert not (got == poison).any()
        assert np.array_equal(got, want[0]) and np.array_equal(counts.cpu().numpy(), want[1])
        runs.append((got, counts.cpu().numpy()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    # the planes moved apart by 5 elements each: what lies between them is left 0, the planes get the same bits
    gap = 5
    moved = k["starts"] + gap * (1 + np.arange(N))
    spread = torch.full((total + gap * (N + 1),), float("nan"), dtype=torch.float32, device="cuda")
    for s, m, (H, W) in zip(k["starts"], moved, k["sizes"]):
        spread[int(m) : int(m) + H * W] = planes[int(s) : int(s) + H * W]
    out, counts = F.speckle(spread, moved, k["sizes"], 7, "refined_lee", R.LOOKS, R.SND, "linear")
    got = R.bits_of(out.cpu().numpy())
    inside = np.zeros(got.shape[0], dtype=bool)
    for s, m, (H, W) in zip(k["starts"], moved, k["sizes"]):
        inside[int(m) : int(m) + H * W] = True
        assert np.array_equal(got[int(m) : int(m) + H * W], want[0][int(s) : int(s) + H * W])
    assert (got[~inside] == 0).all() and (~inside).sum() == gap * (N + 1) and np.array_equal(counts.cpu().numpy(), want[1])


def test_noiseless_steps_are_preserved_on_the_device():
    """The planes of tests/test_cpu_s1_refined_lee.py::test_noiseless_steps_are_preserved, 138 in one launch: every pixel outside the
    outermost ring keeps its input's bits, and the whole output has the bits of the host path."""
    names, flat, starts, sizes = RL.steps()
    n = RL.STEP_SIDE
    out, _ = F.speckle(torch.from_numpy(flat.copy()).cuda(), starts, sizes, 7, "refined_lee", RL.STEP_LOOKS)
    got = R.bits_of(out.cpu().numpy())
    host = R.bits_of(F.speckle(flat, starts, sizes, 7, "refined_lee", RL.STEP_LOOKS)[0])
    assert np.array_equal(got, host)
    inner = (slice(None), slice(1, n - 1), slice(1, n - 1))
    changed = (got.reshape(-1, n, n)[inner] != R.bits_of(flat).reshape(-1, n, n)[inner]).reshape(len(names), -1).sum(axis=1)
    assert not changed.any(), [(names[i], int(changed[i])) for i in np.nonzero(changed)[0]]


def test_filter_s1_on_the_device_writes_the_bytes_of_the_host_path(tmp_path):
    scenes, _ = R.write_scenes(str(tmp_path / "in"), tagged=True)
    names = [os.path.basename(f) for d in scenes for s in d for f in s]
    host, dev = str(tmp_path / "host"), str(tmp_path / "dev")
    F.filter_s1(scenes, host, method="refined_lee")
    written = F.filter_s1(scenes, dev, method="refined_lee", device="cuda")
    assert [os.path.basename(f) for d in written for s in d for f in s] == names
    for n in names + ["filter_stats.json"]:
        assert open(os.path.join(host, n), "rb").read() == open(os.path.join(dev, n), "rb").read(), n
