"""Dataset splitting on the device (-m gpu): ``ig_split_assign`` and ``ig_split_nearest`` against the numpy twins of instageo_amd/split.py
(which tests/test_cpu_split.py pins to the sequential twin of the rule), run-to-run equality, and split_dataset on the device against the
host path, file for file.  Every comparison is ``torch.equal``: all outputs are integers."""
import os

import numpy as np
import pytest
import torch

import split_reference as R
from instageo_amd import _lib, split
from test_cpu_split import ASSIGN_K, ASSIGN_N, BUFFER_KM, NEAREST_SHAPES, _files, write_dataset

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(a).cuda()


def _same(got, want):
    for g, w in zip(got, want):
        w = torch.from_numpy(w.view(np.int64) if w.dtype == np.uint64 else w)
        assert g.is_cuda and g.dtype == w.dtype and g.shape == w.shape and torch.equal(g.cpu(), w)


def _round_twice(pts, centres):
    """One round from -1 and one more with the same centres, each run twice -> the first round's results."""
    N = pts.shape[0]
    start = np.full(N, -1, dtype=np.int32)
    want = split.assign_round(pts, centres, start)
    first = split.assign_round(_dev(pts), centres, _dev(start))
    _same(first, want)
    again = split.assign_round(_dev(pts), centres, _dev(start))
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    assert int(first[2]) == N
    second = split.assign_round(_dev(pts), centres, first[0].clone())
    assert int(second[2]) == 0 and torch.equal(second[0], first[0]) and torch.equal(second[1], first[1])
    return first


@pytest.mark.parametrize("N", ASSIGN_N)
@pytest.mark.parametrize("K", ASSIGN_K)
def test_assign_equals_the_twin(N, K):
    """Identical centres, a point equidistant from two centres, an antipodal pair (d2 = 2^60) and duplicated points are in every case
    the sizes allow (split_reference.assign_case)."""
    pts, centres = R.assign_case(N, K, N + K)
    assign = _round_twice(pts, centres)[0]
    if K >= 2:
        assert not (assign == K - 1).any()  # the copy of centre 0 at the last index takes nothing


@pytest.mark.parametrize("N,K", [(1000, 20), (5000, 256), (65, 2)])
def test_assign_every_cluster_but_one_empty(N, K):
    pts, centres = R.lonely_case(N, K)
    assign, sums, _ = _round_twice(pts, centres)
    assert (assign == K - 1).all() and int(sums[K - 1, 3]) == N and not sums[: K - 1].any()


def test_assign_through_the_entry_point_adds_to_what_the_caller_left():
    """sums and changed are added to, not overwritten (the caller zeroes them): two launches give twice the sums."""
    pts, centres = R.assign_case(1000, 20, 5)
    p, c = _dev(pts), _dev(centres)
    assign = torch.full((1000,), -1, dtype=torch.int32, device="cuda")
    sums = torch.zeros((20, 4), dtype=torch.int64, device="cuda")
    changed = torch.zeros(1, dtype=torch.int32, device="cuda")
    for _ in range(2):
        _lib.call("ig_split_assign", p.data_ptr(), 1000, c.data_ptr(), 20, assign.data_ptr(), sums.data_ptr(), changed.data_ptr(),
                  torch.cuda.current_stream().cuda_stream)
    want = split.assign_round(pts, centres, np.full(1000, -1, dtype=np.int32))
    assert torch.equal(sums.cpu(), torch.from_numpy(2 * want[1])) and int(changed) == 1000 and torch.equal(assign.cpu(), torch.from_numpy(want[0]))


@pytest.mark.parametrize("Na,Nb", NEAREST_SHAPES)
def test_nearest_equals_the_twin(Na, Nb):
    """A point present in both sets (d2 = 0, the smallest index), duplicated rows of b at the minimum across tiles and ranges, and an
    antipodal pair as the only candidate are in every case the sizes allow (split_reference.nearest_case)."""
    a, b = R.nearest_case(Na, Nb, Na + Nb)
    want = split.nearest(a, b)
    got = split.nearest(_dev(a), _dev(b))
    _same(got, want)
    again = split.nearest(_dev(a), _dev(b))
    assert all(torch.equal(x, y) for x, y in zip(got, again))
    if Nb == 1:
        assert int(got[0][0]) == 1 << 60
    if Nb >= 5:
        assert int(got[0][0]) == 0 and int(got[1][0]) == 3
    if Na >= 3 and Nb >= 1023:
        assert int(got[0][2]) == 0 and int(got[1][2]) == 40


def test_nearest_walks_several_tiles_per_range_and_merges():
    """3 x 10^5 rows against 5000: so many blocks of a that b is cut into fewer ranges than it has LDS tiles, so a workgroup walks more
    than one tile and the ranges are merged (no smaller shape reaches that path on a 256-CU device).  The twin takes every 997th row,
    the seams of the first block and the last row: a row's result does not depend on the other rows."""
    Na, Nb = 300000, 5000
    a, b = R.nearest_case(Na, Nb, 11)
    b[1024], b[2047], b[2048], b[4999] = a[997], a[997], a[1994], a[1994]  # minima at the seams of tiles and ranges
    rows = np.unique(np.concatenate([np.arange(0, Na, 997), [255, 256, 1023, 1024, Na - 1]]))
    want = split.nearest(np.ascontiguousarray(a[rows]), b)
    got = split.nearest(_dev(a), _dev(b))
    sel = torch.from_numpy(rows).cuda()
    _same((got[0][sel], got[1][sel]), want)
    assert int(got[1][997]) == 1024 and int(got[1][1994]) == 2048 and int(got[0][997]) == 0
    again = split.nearest(_dev(a), _dev(b))
    assert all(torch.equal(x, y) for x, y in zip(got, again))


@pytest.mark.parametrize("strategy,buffer_km", [("kmeans", 0.0), ("kmeans", BUFFER_KM), ("random", BUFFER_KM)])
def test_split_dataset_on_the_device_writes_the_bytes_of_the_host_path(tmp_path, strategy, buffer_km):
    csv, _ = write_dataset(str(tmp_path / "data"))
    outs = {}
    for dev in (None, "cuda"):
        outs[dev] = str(tmp_path / f"out_{dev}")
        split.split_dataset(csv, outs[dev], strategy=strategy, buffer_km=buffer_km, device=dev)
    host, device = _files(outs[None]), _files(outs["cuda"])
    assert sorted(host) == ["dropped.csv", "split_stats.json", "splits.geojson", "splits/test.csv", "splits/train.csv", "splits/val.csv"]
    assert host == device
