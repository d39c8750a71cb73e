"""The map projections against the 50-digit reference of tests/projection_truth.py (no GPU): the fixture tests/golden/projection_truth.npz
regenerates bit for bit and has converged, the reference is consistent with itself, and the float64 twin (tests/warp_reference.py) and
the host path (instageo_amd.warp.coords, instageo_amd.crs.transform) meet the bars that tests/test_gpu_projection_truth.py sets for the
device.  Only the tests that evaluate the reference need mpmath; everything else reads the fixture.

Errors are ground metres: projected outputs are metres already, a geographic output counts as hypot(dlon * 111320 * cos(lat), dlat *
111320).  BARS.  Core lattices: the NaN pattern of the fixture exactly, and |x - truth| <= 1e-6 m at every point: ten times below what
1e-6 px of tests/test_gpu_warp.py means on a 10 m grid, 2.5 times the twin's worst, yet below the n^4 terms of the series (1e-5 m), every
constant and a missing Newton step.  Outer band (40 to 79.9 degrees from the central meridian, forward): |x - truth| <= 2 |twin - truth|
+ 1e-6 m point by point: an implementation may not be worse than the truncated series it evaluates, whose own error is read from the
twin, never from the code under test.

MEASURED worst |x - truth| per lattice, metres (twin, host path):
  fwd_utm36_wide 3.7e-9 2.8e-9 | fwd_origin_micro 2.3e-13 1.6e-9 | fwd_near_pole 3.7e-9 2.0e-9 | fwd_zone1_east_of_180 2.8e-9 1.9e-9
  fwd_zone1_west_of_180 1.9e-9 1.9e-9 | fwd_zone60_east_of_180 1.9e-9 1.9e-9 | fwd_zone60_west_of_180 2.8e-9 1.9e-9
  fwd_utm21_south 1.9e-9 1.9e-9 | fwd_custom_tm 2.8e-9 1.0e-9 | inv_utm36_wide 7.4e-8 2.0e-9 | inv_origin_micro 1.9e-13 9.7e-14
  inv_near_pole 4.0e-7 1.8e-9 | inv_beyond_pole 3.3e-9 1.1e-9 | inv_utm21_south 4.8e-9 1.6e-9 | inv_custom_tm 4.0e-9 1.6e-9
  wm_from_geographic 7.5e-9 7.5e-9 | wm_to_geographic 1.8e-9 1.6e-9 | wm_to_utm36_lat0p1 1.2e-9 8.7e-10 | wm_from_utm36_lat0p1 1.6e-9 9.3e-10
  wm_to_utm36_lat40 2.8e-9 1.1e-9 | wm_from_utm36_lat40 3.8e-9 2.8e-9 | wm_to_utm36_lat80 3.7e-9 1.9e-9 | wm_from_utm36_lat80 5.8e-8 1.1e-8
  tm_utm37_to_utm36_lat0p1 7.0e-10 2.0e-9 | tm_utm37_to_utm36_lat40p6 2.8e-9 2.0e-9 | tm_utm37_to_utm36_lat80 7.5e-9 3.7e-9
  tm_utm36_to_utm37_lat40p6 2.8e-9 1.9e-9 | tm_north_to_south_equator 4.7e-10 1.6e-9 | tm_south_to_north_equator 3.9e-10 1.8e-9
  tm_zone1_to_zone60 4.0e-9 3.7e-9 | tm_zone60_to_zone1 4.0e-9 6.3e-9
  outer_east 4.74 4.74 | outer_edge 118.1 118.1 | outer_west 118.1 118.1   (the series' own truncation error; host - twin <= 1e-6 there)
The twin's 4.0e-7 m on inv_near_pole (7.4e-8 m on inv_utm36_wide) is its own rounding, not the reference's: it takes the isometric latitude
as atanh(sin xi' / cosh eta'), and within 0.6 degrees of a pole 1 - sin xi' / cosh eta' is 2e-6, so one rounding of the quotient is 6e-11
of it, 3e-11 in psi and 5e-14 rad = 3e-7 m in latitude; the host path and the kernels take tan of the conformal latitude and stay at 2e-9 m
on the same points.
"""
import os

import numpy as np
import pytest

import projection_truth as PT
import warp_reference as WR
from instageo_amd import crs, warp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = PT.load()
CORE_BAR = 1e-6  # metres
needs_mpmath = pytest.mark.skipif(PT.mpmath is None, reason="mpmath is not installed: the reference cannot be evaluated")


def metres(case, u, v):
    """|(u, v) - truth| on the ground, NaN where either is NaN."""
    du, dv = u - case["u"], v - case["v"]
    if case["src_crs"][0] == 0:
        return np.hypot(du * 111320.0 * np.cos(np.radians(case["lat"])), dv * 111320.0)
    return np.hypot(du, dv)


@pytest.fixture(scope="module")
def twin():
    """name -> the twin's (u, v), computed once."""
    return {n: WR.coords(c["dst_crs"], c["dst_grid"], c["shape"], c["src_crs"], c["src_grid"]) for n, c in FIX.items()}


def check(name, u, v, twin_uv):
    """The bars of the module docstring -> the worst error."""
    case = FIX[name]
    assert u.shape == case["u"].shape and np.array_equal(np.isnan(u), np.isnan(case["u"])) and np.array_equal(np.isnan(v), np.isnan(case["v"]))
    err = metres(case, u, v)
    ok = ~np.isnan(case["u"])
    bar = np.full(err.shape, CORE_BAR)
    if case["outer"]:
        bar = 2.0 * metres(case, *twin_uv) + CORE_BAR
    print(f"{name}: worst |x - truth| = {err[ok].max():.3e} m (worst bar {bar[ok].max():.3e} m)")
    assert (err[ok] <= bar[ok]).all()
    return err[ok].max()


# ---- the fixture -------------------------------------------------------------------------------------------------------------------------
def test_fixture_holds_the_regions_it_is_meant_to():
    assert os.path.getsize(PT.FIXTURE) < 256 * 1024
    assert 3000 <= sum(c["u"].size for c in FIX.values()) <= 3500 and max(max(c["shape"]) for c in FIX.values()) <= 17
    for name, c in FIX.items():
        nan = np.isnan(c["u"])
        assert c["src_grid"] == PT.UNIT_GRID and c["dst_crs"] != c["src_crs"] and c["outer"] == name.startswith("outer_")
        assert np.array_equal(nan, np.isnan(c["v"])) and np.array_equal(nan, np.isnan(c["lon"])) and np.array_equal(nan, np.isnan(c["lat"]))
        assert nan.any() == (name in ("fwd_near_pole", "inv_near_pole", "inv_beyond_pole")) and not nan.all()
        if c["dst_crs"][0] == 0:  # a geographic destination: the true longitude and latitude are the centres themselves
            x, y = PT.centres(c["dst_grid"], c["shape"])
            assert np.array_equal(c["lon"][~nan], np.broadcast_to(x, c["shape"])[~nan]) and np.array_equal(c["lat"][~nan], np.broadcast_to(y[:, None], c["shape"])[~nan])
    x, y = PT.centres(FIX["fwd_near_pole"]["dst_grid"], FIX["fwd_near_pole"]["shape"])
    assert np.array_equal(np.isnan(FIX["fwd_near_pole"]["u"]), np.broadcast_to((y > 89.9)[:, None], (15, 11))) and (y > 89.9).sum() == 1
    c = FIX["inv_near_pole"]  # in the domain, inside the 89.9 degree circle and beyond the pole, all three
    assert (c["lat"][~np.isnan(c["lat"])] > 89.0).all() and np.isnan(c["u"][:3]).all() and np.isnan(c["u"][3, 6]) and not np.isnan(c["u"][-1]).any()
    c = FIX["inv_beyond_pole"]
    assert np.isnan(c["u"][[0, -1]]).all() and not np.isnan(c["u"][1:-1]).any()
    # the date line: zone 1 and zone 60 see the same points from both sides of 180 degrees at mirrored eastings
    for zone in ("zone1", "zone60"):
        east, west = FIX[f"fwd_{zone}_east_of_180"], FIX[f"fwd_{zone}_west_of_180"]
        assert np.abs(east["u"][:, 0] - west["u"][:, -1]).max() < 1e-8  # -180 and +180 are one meridian
        assert 1e5 < np.abs(east["u"] - 5e5).max() < 2e6 and 1e5 < np.abs(west["u"] - 5e5).max() < 2e6  # and near it, not 360 degrees away
    # sign symmetry about the equator and the central meridian, in absolute terms
    c = FIX["fwd_origin_micro"]
    assert np.abs((c["u"] - 5e5) + (c["u"] - 5e5)[:, ::-1]).max() < 1e-9 and np.abs(c["v"] + c["v"][::-1]).max() < 1e-9
    assert np.abs(c["u"][:, 5] - 5e5).max() < 1e-8 and np.abs(c["v"][5]).max() < 1e-8


def _sample():
    """One point of every lattice, and one outside the domain where a lattice has any."""
    picks = []
    for i, (name, c) in enumerate(FIX.items()):
        n = c["u"].size
        picks.append((name, divmod(n * (2 * i + 1) // (2 * len(FIX)), c["shape"][1])))  # from the first rows of the first lattice to the last of the last
        if np.isnan(c["u"]).any():
            picks.append((name, tuple(int(k) for k in np.argwhere(np.isnan(c["u"]))[len(picks) % 3])))
    return picks


def _recompute(name, rc, dps):
    c = FIX[name]
    x, y = PT.centres(c["dst_grid"], c["shape"])
    got = PT.point(c["dst_crs"], c["src_crs"], float(x[rc[1]]), float(y[rc[0]]), dps=dps)
    return np.array(got), np.array([c[k][rc] for k in ("u", "v", "lon", "lat")])


@needs_mpmath
def test_fixture_regenerates_bit_for_bit_and_has_converged():
    table = PT.lattices()
    assert list(table) == list(FIX)
    for name, (dst_crs, grid, shape, src_crs, outer) in table.items():
        c = FIX[name]
        assert (dst_crs, tuple(grid), tuple(shape), src_crs, outer) == (c["dst_crs"], c["dst_grid"], c["shape"], c["src_crs"], c["outer"]), name
    picks = _sample()
    assert len(picks) >= 30
    for name, rc in picks:
        got, want = _recompute(name, rc, PT.DPS)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (name, rc, got, want)
    for name, rc in [p for p in picks if p[0] in ("fwd_near_pole", "inv_near_pole", "inv_utm36_wide", "tm_zone1_to_zone60", "wm_from_utm36_lat80",
                                                  "outer_edge")]:
        got, want = _recompute(name, rc, 80)  # 30 more digits round to the same float64: 50 digits and the quadrature have converged
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (name, rc, got, want)


# ---- the reference against itself --------------------------------------------------------------------------------------------------------
POINTS = [(0.0, 0.5), (3.0, 40.6), (-40.0, -80.0), (25.0, 89.9), (70.0, 20.0), (-79.9, 0.0), (1e-3, -1e-3)]  # (lon - lon0, lat), degrees


@needs_mpmath
def test_reference_inverse_undoes_its_forward():
    mp, mpf = PT.mp, PT.mpf
    system = PT.utm(36)
    with mp.workdps(PT.DPS):
        for dl, lat in POINTS:
            lon, lat = mpf(33) + mpf(dl), mpf(lat)
            back = PT.tm_inverse(system, *PT.tm_forward(system, lon, lat))
            err = max(abs(back[0] - lon), abs(back[1] - lat))
            print(f"({dl}, {float(lat)}): round trip {float(err):.1e} degrees")
            assert err <= mpf("1e-40")


@needs_mpmath
def test_reference_satisfies_the_cauchy_riemann_equations():
    """N + i E is an analytic function of psi + i lambda: d/dphi = psi'(phi) d/dpsi and d/dlambda = i d/dpsi, so (N + i E)_phi =
    -i psi'(phi) (N + i E)_lambda.  Central differences with h = 1e-15 rad leave h^2 = 1e-30 of the third derivative."""
    mp, mpf, mpc = PT.mp, PT.mpf, PT.mpc
    system = PT.utm(36)
    with mp.workdps(PT.DPS):
        h = mp.degrees(mpf("1e-15"))

        def f(lon, lat):
            x, y = PT.tm_forward(system, lon, lat)
            return mpc(y, x)

        for dl, lat in POINTS:
            lon, lat = mpf(33) + mpf(dl), mpf(lat)
            d_phi = (f(lon, lat + h) - f(lon, lat - h)) / mpf("2e-15")
            d_lam = (f(lon + h, lat) - f(lon - h, lat)) / mpf("2e-15")
            miss = abs(d_phi + mpc(0, 1) * PT.dpsi(mp.radians(lat)) * d_lam) / abs(d_phi)
            print(f"({dl}, {float(lat)}): Cauchy-Riemann miss {float(miss):.1e}")
            assert miss <= mpf("1e-25")


@needs_mpmath
def test_reference_northing_on_the_central_meridian_is_the_meridian_arc():
    """k0 a (E(phi | e^2) - e^2 sin phi cos phi / sqrt(1 - e^2 sin^2 phi)) with mpmath's incomplete elliptic integral: no quadrature."""
    mp, mpf = PT.mp, PT.mpf
    system = PT.utm(36)
    with mp.workdps(PT.DPS):
        e2 = PT._e2()
        for lat in (0.5, 20.0, 45.0, 70.0, 85.0, 89.9):
            phi = mp.radians(mpf(lat))
            arc = PT._a() * (mp.ellipe(phi, e2) - e2 * mp.sin(phi) * mp.cos(phi) / mp.sqrt(1 - e2 * mp.sin(phi) ** 2))
            x, y = PT.tm_forward(system, mpf(33), mpf(lat))
            assert abs(x - 500000) <= mpf("1e-40") and abs(y - mpf(system[2]) * arc) <= mpf("1e-40") * arc, lat


# ---- the twin and the host path against the fixture ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FIX))
def test_twin_meets_the_bars(name, twin):
    worst = check(name, *twin[name], twin[name])
    assert FIX[name]["outer"] or worst <= 5e-7  # measured 4.0e-7 at most (the docstring says where and why)


@pytest.mark.parametrize("name", list(FIX))
def test_host_path_meets_the_bars(name, twin):
    c = FIX[name]
    check(name, *warp.coords(c["dst_crs"], c["dst_grid"], c["shape"], c["src_crs"], c["src_grid"]), twin[name])
    x, y = np.meshgrid(*PT.centres(c["dst_grid"], c["shape"]))
    xs, ys = crs.transform(c["dst_crs"], c["src_crs"], x, y)
    check(name, xs, -ys, twin[name])


@pytest.mark.parametrize("fault", ["alpha2 13/46", "alpha1 without n^4", "beta2 without n^4", "e off in the 9th digit"])
def test_a_subtly_wrong_series_misses_the_core_bar(fault, twin, monkeypatch):
    """What the bar is for: a mistyped coefficient, a lost n^4 term (of a coefficient above 0.1) or a wrong literal fails some core lattice on the host path."""
    if fault == "alpha2 13/46":
        monkeypatch.setattr(crs, "ALPHA", crs.ALPHA + np.eye(6)[1] * (13 / 46 - 13 / 48) * crs.N**2)
    elif fault == "alpha1 without n^4":
        monkeypatch.setattr(crs, "ALPHA", crs.ALPHA - np.eye(6)[0] * (41 / 180) * crs.N**4)
    elif fault == "beta2 without n^4":
        monkeypatch.setattr(crs, "BETA", crs.BETA + np.eye(6)[1] * (437 / 1440) * crs.N**4)
    else:
        monkeypatch.setattr(crs, "E", crs.E + 1e-9)
    failed = []
    for name, c in FIX.items():
        if not c["outer"]:
            u, v = warp.coords(c["dst_crs"], c["dst_grid"], c["shape"], c["src_crs"], c["src_grid"])
            if np.nanmax(metres(c, u, v)) > CORE_BAR:
                failed.append(name)
    print(f"{fault}: {len(failed)} core lattices fail: {failed}")
    assert failed


# ---- what the header says ------------------------------------------------------------------------------------------------------------------
def test_accuracy_table_of_the_header_is_the_fixtures(twin):
    rows = {0.0: [], 20.0: [], 45.0: []}
    high = 0.0
    for lo, hi in ((40.0, 50.0), (50.0, 60.0), (60.0, 70.0), (70.0, 79.9)):
        worst = dict.fromkeys(rows, 0.0)
        for name in ("outer_east", "outer_edge"):
            c = FIX[name]
            x, y = PT.centres(c["dst_grid"], c["shape"])
            err = metres(c, *twin[name])
            cols = (np.round(x - 33.0, 9) > lo) & (np.round(x - 33.0, 9) <= hi)
            assert cols.sum() >= 3 or name == "outer_edge"
            for lat in rows:
                (r,) = np.nonzero(np.round(y, 9) == lat)[0]
                worst[lat] = max(worst[lat], err[r, cols].max(initial=0.0))
            high = max(high, err[np.round(y, 9) >= 45.0].max())
        for lat in rows:
            rows[lat].append(worst[lat])
    fmt = lambda e: f"{e:.0f} m" if e >= 10 else f"{e:.1e} m".replace("e-0", "e-")  # noqa: E731
    lines = [f"{lat:.0f}".rjust(2) + "        " + "    ".join(fmt(e) for e in rows[lat]) for lat in rows]
    print("\n".join(lines), f"\nfrom 45 degrees up: {high:.2e} m")
    core_fwd = max(np.nanmax(metres(FIX[n], *twin[n])) for n in FIX if n.startswith("fwd_"))
    core_inv = max(np.nanmax(metres(FIX[n], *twin[n])) for n in FIX if n.startswith("inv_"))
    assert core_fwd <= 3.8e-9 and 7.0e-8 < np.nanmax(metres(FIX["inv_utm36_wide"], *twin["inv_utm36_wide"])) <= 7.5e-8 and 3.5e-7 < core_inv <= 4.1e-7
    assert high <= 3.5e-8 and 4.6 < np.nanmax(metres(FIX["outer_east"], *twin["outer_east"])) < 4.8
    for path in (os.path.join(ROOT, "include", "instageo_hip.h"), os.path.join(ROOT, "DESIGN.md")):
        text = " ".join(open(path, encoding="utf-8").read().replace("*", " ").replace("|", " ").split())
        assert "ACCURACY" in text
        for line in lines:
            assert " ".join(line.split()) in text, (path, line)
