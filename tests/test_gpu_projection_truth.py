"""ig_warp_coords against the 50-digit truth of tests/golden/projection_truth.npz (-m gpu): one launch per lattice of the fixture.

The fixture (made by tests/projection_truth.py from the definition of the projections, nothing shared with Krueger's series) holds, per
lattice, a small destination grid, a source system with the grid (0, 0, 1, 1), and the true float64 (u, v) = (x', -y') of every pixel
centre, NaN where the header's domain rule says NaN, with the true longitude and latitude.  This module needs numpy, torch and that file
only; mpmath is not imported.  The series' own error in the outer band is read from the float64 twin (tests/warp_reference.py).

Errors are ground metres: projected outputs are metres already, a geographic output counts as hypot(dlon * 111320 * cos(lat), dlat *
111320).  BARS (reasoned in tests/test_cpu_projection_truth.py, which holds the twin and the host path to the same).  Every lattice: the
fixture's NaN pattern exactly, and a repeated launch bit-identical.  Core lattices: |device - truth| <= 1e-6 m at every point.  Outer
band (40 to 79.9 degrees from the central meridian, forward): |device - truth| <= 2 |twin - truth| + 1e-6 m point by point.

MEASURED on an MI355X, worst |device - truth| per lattice, metres (the twin's and the host path's stand in the CPU module):
  fwd_utm36_wide 3.9e-9 | fwd_origin_micro 8.1e-10 | fwd_near_pole 2.0e-9 | fwd_zone1_east_of_180 1.9e-9 | fwd_zone1_west_of_180 1.9e-9
  fwd_zone60_east_of_180 1.9e-9 | fwd_zone60_west_of_180 1.9e-9 | fwd_utm21_south 1.4e-9 | fwd_custom_tm 1.9e-9 | inv_utm36_wide 2.5e-9
  inv_origin_micro 9.7e-14 | inv_near_pole 1.8e-9 | inv_beyond_pole 1.7e-9 | inv_utm21_south 1.6e-9 | inv_custom_tm 1.6e-9
  wm_from_geographic 7.5e-9 | wm_to_geographic 1.6e-9 | wm_to_utm36_lat0p1 4.7e-10 | wm_from_utm36_lat0p1 9.3e-10
  wm_to_utm36_lat40 9.9e-10 | wm_from_utm36_lat40 2.8e-9 | wm_to_utm36_lat80 1.9e-9 | wm_from_utm36_lat80 1.1e-8
  tm_utm37_to_utm36_lat0p1 4.7e-10 | tm_utm37_to_utm36_lat40p6 1.9e-9 | tm_utm37_to_utm36_lat80 1.9e-9
  tm_utm36_to_utm37_lat40p6 1.9e-9 | tm_north_to_south_equator 3.5e-10 | tm_south_to_north_equator 4.7e-10 | tm_zone1_to_zone60 3.7e-9
  tm_zone60_to_zone1 3.6e-9 | outer_east 4.7 | outer_edge 118.1 | outer_west 118.1
Every core lattice within 1.2e-8 m; in the outer band the device's error is the series' own (the twin's 4.741 m and 118.1 m to four digits).
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import warp_reference as WR  # noqa: E402
from instageo_amd import ops  # noqa: E402

DEV = "cuda"
CORE_BAR = 1e-6  # metres
SRC_GRID = (0.0, 0.0, 1.0, 1.0)
_Z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "projection_truth.npz"))
NAMES = [str(n) for n in _Z["names"]]


def _case(name):
    i = NAMES.index(name)
    return dict(dst_crs=tuple(_Z["dst_crs"][i]), dst_grid=tuple(_Z["dst_grid"][i]), shape=tuple(int(v) for v in _Z["shape"][i]),
                src_crs=tuple(_Z["src_crs"][i]), outer=bool(_Z["outer"][i]), **{k: _Z[f"{name}/{k}"] for k in ("u", "v", "lon", "lat")})


def _metres(case, u, v):
    du, dv = u - case["u"], v - case["v"]
    if case["src_crs"][0] == 0:
        return np.hypot(du * 111320.0 * np.cos(np.radians(case["lat"])), dv * 111320.0)
    return np.hypot(du, dv)


def test_fixture_is_the_one_the_cpu_tests_pinned():
    assert len(NAMES) == 34 and sum(bool(o) for o in _Z["outer"]) == 3 and sum(_Z[f"{n}/u"].size for n in NAMES) == 3197


@pytest.mark.parametrize("name", NAMES)
def test_device_coordinates_against_the_truth(name):
    c = _case(name)
    first = ops.warp_coords(c["dst_crs"], c["dst_grid"], c["shape"], c["src_crs"], SRC_GRID, device=DEV)
    again = ops.warp_coords(c["dst_crs"], c["dst_grid"], c["shape"], c["src_crs"], SRC_GRID, device=DEV)
    assert torch.equal(first.view(torch.int64), again.view(torch.int64))
    u, v = first.cpu().numpy()
    assert u.shape == c["u"].shape
    assert np.array_equal(np.isnan(u), np.isnan(c["u"])) and np.array_equal(np.isnan(v), np.isnan(c["v"]))
    ok = ~np.isnan(c["u"])
    err = _metres(c, u, v)
    bar = np.full(err.shape, CORE_BAR)
    if c["outer"]:
        bar = 2.0 * _metres(c, *WR.coords(c["dst_crs"], c["dst_grid"], c["shape"], c["src_crs"], SRC_GRID)) + CORE_BAR
    print(f"{name}: worst |device - truth| = {err[ok].max():.3e} m (worst bar {bar[ok].max():.3e} m)")
    assert ok.any() and (err[ok] <= bar[ok]).all()
