"""``ig_composite`` on the device against the sequential twin of the rule (tests/composite_reference.py), bit for bit over every pixel, at the
smallest shapes where the kernel can go wrong: 5 x 36 (an int16 pitch of 72 bytes, 8 mod 16), 3 x 7 (narrower than one vector), 17 x 129
(several workgroups, an odd plane size: every second plane starts at an odd element) and 2 x 3660 (the real pitch); 0, 1, 2, 3, 4, 5, 8, 15
and 16 candidates, several steps of different counts in one launch; C = 1 and 6 (values kept in registers) and 5 (read again).  The input
buffers start one element off alignment; the outputs are pre-filled with poison."""
import numpy as np
import pytest
import torch

import composite_reference as R
from instageo_amd import composite as K

pytestmark = pytest.mark.gpu


def on_device(k):
    return torch.from_numpy(k["bands"].copy()).cuda()[1:], torch.from_numpy(k["fmasks"].copy()).cuda()[1:]


def run_device(k, method, min_clear=1, with_fmask=True):
    bands, fmasks = on_device(k)
    assert bands.data_ptr() % 4 == 2 and fmasks.data_ptr() % 2 == 1
    out = K.composite(bands, k["starts"], fmasks if with_fmask else None, k["fmask_starts"] if with_fmask else None, k["step_ptr"], k["C"],
                      (k["H"], k["W"]), R.BITS, R.ND, min_clear, method)
    assert all(o.is_cuda for o in out)
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize("method", R.METHODS)
@pytest.mark.parametrize("name", list(R.CASES))
def test_kernel_equals_the_twin(name, method):
    k = R.case(name)
    got, want = run_device(k, method), R.expected(name, method)
    for g, w, what in zip(got, want, ("composite", "count", "source", "hist")):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, int((g != w).sum()))
    assert (got[3].sum(axis=1) == k["H"] * k["W"]).all()


@pytest.mark.parametrize("method", R.METHODS)
def test_min_clear_and_no_fmask(method):
    k = R.case("p36_c6")
    assert all(np.array_equal(g, w) for g, w in zip(run_device(k, method, min_clear=3), R.expected("p36_c6", method, 3)))
    assert all(np.array_equal(g, w) for g, w in zip(run_device(k, method, with_fmask=False), R.expected("p36_c6", method, 1, False)))


@pytest.mark.parametrize("name", ["blocks_c6", "narrow_c1", "pitch_c5"])
def test_every_output_is_written_once_and_runs_repeat(name):
    """The raw op on poisoned outputs: a pixel that is not written keeps the poison, one that is tallied twice breaks the histogram's sum."""
    from instageo_amd import torch_ops

    torch_ops.register()
    k = R.case(name)
    bands, fmasks = on_device(k)
    T, C, H, W = len(k["step_ptr"]) - 1, k["C"], k["H"], k["W"]
    N = int(k["step_ptr"][-1])
    tab = [torch.from_numpy(a.copy()).cuda() for a in (k["starts"], k["fmask_starts"], k["step_ptr"])]
    runs = []
    for poison in (0x5A5A, 0x2525):
        comp = torch.full((T, C, H, W), poison, dtype=torch.int16, device="cuda")
        count = torch.full((T, H, W), poison & 0xFF, dtype=torch.uint8, device="cuda")
        source = torch.full((T, H, W), poison & 0xFF, dtype=torch.uint8, device="cuda")
        hist = torch.zeros((T, 17), dtype=torch.int32, device="cuda")
        torch.ops.instageo_mi355x.composite(bands, tab[0], fmasks, tab[1], tab[2], T, N, int(np.diff(k["step_ptr"]).max()), C, H, W, R.BITS, R.ND, 1, 2,
                                            comp, count, source, hist)
        runs.append([a.cpu().numpy() for a in (comp, count, source, hist)])
    want = R.expected(name, "medoid")
    for got in runs:
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
        assert (got[3].sum(axis=1) == H * W).all()
    assert all(np.array_equal(a, b) for a, b in zip(*runs))  # two runs, different poison: identical bits


def test_a_stated_max_m_below_a_step_cuts_it_and_broken_bounds_read_nothing():
    """The second fence: the tables are on the device, so the kernel does not trust them."""
    from instageo_amd import torch_ops

    torch_ops.register()
    k = R.case("narrow_c1")  # steps of 4, 2 and 15 candidates
    bands, fmasks = on_device(k)
    T, H, W = 3, k["H"], k["W"]
    st, fst = (torch.from_numpy(a.copy()).cuda() for a in (k["starts"], k["fmask_starts"]))

    def launch(ptr, N, max_m):
        comp = torch.full((T, 1, H, W), 77, dtype=torch.int16, device="cuda")
        count = torch.full((T, H, W), 99, dtype=torch.uint8, device="cuda")
        source = torch.full((T, H, W), 99, dtype=torch.uint8, device="cuda")
        hist = torch.zeros((T, 17), dtype=torch.int32, device="cuda")
        torch.ops.instageo_mi355x.composite(bands, st, fmasks, fst, torch.tensor(ptr, dtype=torch.int32, device="cuda"), T, N, max_m, 1, H, W, R.BITS, R.ND,
                                            1, 0, comp, count, source, hist)
        return comp.cpu().numpy(), count.cpu().numpy(), source.cpu().numpy(), hist.cpu().numpy()

    ptr = k["step_ptr"].tolist()
    cut = launch(ptr, 21, 8)  # the third step states 15 candidates: its first 8 are used
    want = R.twin(k["bands"][1:], k["starts"], k["fmasks"][1:], k["fmask_starts"], ptr[:3] + [ptr[2] + 8], 1, H, W, R.BITS, R.ND, 1, "nearest")
    assert all(np.array_equal(g, w) for g, w in zip(cut, want))
    broken = launch([0, -3, 6, 40], 21, 16)  # step 0 runs backwards, step 1 starts below 0, step 2 ends beyond N
    assert (broken[0] == R.ND).all() and not broken[1].any() and (broken[2] == 255).all() and (broken[3][:, 0] == H * W).all()


def test_create_composite_on_the_device_writes_the_bytes_of_the_host_path(tmp_path):
    import os

    from test_cpu_composite import write_scenes

    scenes, fmasks, _, _ = write_scenes(str(tmp_path / "in"))
    for method in R.METHODS:
        a, b = str(tmp_path / f"host_{method}"), str(tmp_path / f"dev_{method}")
        wa, sa = K.create_composite([scenes, scenes[:2]], [fmasks, fmasks[:2]], a, dates=["20220526", "20220519"], method=method, device=None)
        wb, sb = K.create_composite([scenes, scenes[:2]], [fmasks, fmasks[:2]], b, dates=["20220526", "20220519"], method=method, device="cuda")
        assert wa == wb and sa == sb and sorted(os.listdir(a)) == sorted(os.listdir(b)) and len(os.listdir(a)) == 9
        for n in os.listdir(a):
            assert open(os.path.join(a, n), "rb").read() == open(os.path.join(b, n), "rb").read(), n
