"""Reprojection and resampling, host side (no GPU): the twin (tests/warp_reference.py) and instageo_amd.crs pinned each on its own (a
published grid position, the meridian arc by quadrature, the Cauchy-Riemann equations, the round trip, closed forms) and against each
other; GeoKey parsing and writing; the target grid; the config keys; the argument checks of the HIP entry points; the numpy host path
against the twin; merge_reprojected on the host path, file to file."""
import ctypes
import os

import numpy as np
import pytest

import warp_reference as WR
from instageo_amd import crs, mosaic, tiff, warp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "instageo-e2e-geospatial-ml_amd")
CN_TOWER = (-(79 + 23 / 60 + 13.7 / 3600), 43 + 38 / 60 + 33.24 / 3600)  # 43 38 33.24 N, 79 23 13.7 W: UTM 17N 630084 / 4833438


@pytest.fixture(scope="module")
def built_lib():
    import subprocess

    from instageo_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j4"], check=True)
    return _lib


def _tags(x, y, epsg, scale=30.0):
    model = 2 if epsg == 4326 else 1
    return {33550: (12, (scale, scale, 0.0)), 33922: (12, (0.0, 0.0, 0.0, float(x), float(y), 0.0)),
            34735: (3, (1, 1, 0, 3, 1024, 0, 1, model, 1025, 0, 1, 1, 2048 if model == 2 else 3072, 0, 1, epsg))}


def _profile(x, y, epsg, h=16, w=16, scale=30.0, dtype="int8"):
    return {"width": w, "height": h, "count": 1, "dtype": dtype, "nodata": None, "tags": _tags(x, y, epsg, scale)}


def _both():
    """(name, forward(crs5, lon, lat), inverse(crs5, x, y)) of the twin and of the product."""
    return (("twin", WR.from_lonlat, WR.to_lonlat), ("crs.py", crs.forward, crs.inverse))


# ---- the projections, each implementation on its own -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,fwd,inv", _both(), ids=["twin", "crs"])
def test_cn_tower_lands_on_its_published_grid_position(name, fwd, inv):
    x, y = fwd(WR.utm(17), *CN_TOWER)
    assert abs(x - 630084.3) <= 1.0 and abs(y - 4833438.5) <= 1.0, (name, float(x), float(y))


@pytest.mark.parametrize("name,fwd,inv", _both(), ids=["twin", "crs"])
def test_northing_on_the_central_meridian_is_the_meridian_arc(name, fwd, inv):
    from scipy.integrate import quad

    e2 = WR.F * (2 - WR.F)
    for lat in (10.0, 45.0, 80.0):
        arc = quad(lambda p: WR.A * (1 - e2) / (1 - e2 * np.sin(p) ** 2) ** 1.5, 0.0, np.radians(lat), epsabs=1e-7, epsrel=1e-13)[0]
        x, y = fwd(WR.utm(36), 33.0, lat)
        assert abs(x - 500000.0) <= 1e-6 and abs(y - 0.9996 * arc) <= 1e-6, (name, lat, float(y) - 0.9996 * arc)


@pytest.mark.parametrize("name,fwd,inv", _both(), ids=["twin", "crs"])
def test_cauchy_riemann_equations_hold(name, fwd, inv):
    """x + i y is an analytic function of longitude + i (isometric latitude): dx/dlam = dy/dpsi, dx/dpsi = -dy/dlam, by central
    differences of step 1e-5 rad (truncation ~ 1e-10 relative, rounding ~ 1e-9 relative of derivatives of ~ 6e6 m / rad)."""
    rng = np.random.default_rng(3)
    h = 1e-5
    for lon, lat in zip(33.0 + rng.uniform(-6, 6, 20), rng.uniform(-75, 80, 20)):
        psi = float(WR.isometric(lat))
        at = lambda dl, dp: fwd(WR.utm(36), lon + np.degrees(dl), WR.latitude_of_isometric(psi + dp))  # noqa: E731
        (xe, ye), (xw, yw), (xn, yn), (xs, ys) = at(h, 0), at(-h, 0), at(0, h), at(0, -h)
        dxl, dyl, dxp, dyp = (xe - xw) / (2 * h), (ye - yw) / (2 * h), (xn - xs) / (2 * h), (yn - ys) / (2 * h)
        size = np.hypot(dxl, dyl)
        assert abs(dxl - dyp) <= 1e-6 * size and abs(dxp + dyl) <= 1e-6 * size, (name, lon, lat)


@pytest.mark.parametrize("name,fwd,inv", _both(), ids=["twin", "crs"])
def test_round_trip_over_a_widened_zone(name, fwd, inv):
    rng = np.random.default_rng(4)
    lat, lon = rng.uniform(-80, 84, 4000), 33.0 + rng.uniform(-6, 6, 4000)
    for system in (WR.utm(36), WR.utm(36, south=True)):
        lon2, lat2 = inv(system, *fwd(system, lon, lat))
        assert np.abs(lon2 - lon).max() <= 1e-9 and np.abs(lat2 - lat).max() <= 1e-9, name


def test_crs_equals_the_twin():
    rng = np.random.default_rng(5)
    lat, lon = rng.uniform(-80, 84, 4000), 33.0 + rng.uniform(-8, 8, 4000)
    for system in (WR.utm(36), WR.utm(36, south=True), WR.WEB_MERCATOR, WR.GEOGRAPHIC):
        xa, ya = WR.from_lonlat(system, lon, lat)
        xb, yb = crs.forward(system, lon, lat)
        assert np.abs(xa - xb).max() <= 1e-6 and np.abs(ya - yb).max() <= 1e-6
        la, pa = WR.to_lonlat(system, xa, ya)
        lb, pb = crs.inverse(system, xa, ya)
        assert np.abs(la - lb).max() <= 1e-11 and np.abs(pa - pb).max() <= 1e-11  # 1e-11 degrees are 1e-6 m


@pytest.mark.parametrize("name,fwd,inv", _both(), ids=["twin", "crs"])
def test_south_zone_web_mercator_and_geographic_closed_forms(name, fwd, inv):
    lon, lat = np.array([31.0, 33.0, 36.5]), np.array([-33.9, -1.0, -60.0])
    xn, yn = fwd(WR.utm(36), lon, lat)
    xs, ys = fwd(WR.utm(36, south=True), lon, lat)
    assert np.array_equal(xn, xs) and np.abs(ys - (yn + 1e7)).max() <= 2e-9 and (ys > 0).all() and (yn < 0).all()
    x, y = fwd(WR.WEB_MERCATOR, np.array([0.0, 180.0, -90.0]), np.array([0.0, 45.0, -60.0]))
    want_y = WR.A * np.arctanh(np.sin(np.radians([0.0, 45.0, -60.0])))  # the Gudermannian's inverse, a third closed form
    assert np.abs(x - WR.A * np.pi * np.array([0.0, 1.0, -0.5])).max() <= 1e-8 and np.abs(y - want_y).max() <= 1e-8
    lo, la = inv(WR.WEB_MERCATOR, np.array([WR.A * np.pi / 2]), np.array([WR.A * np.arctanh(np.sin(np.radians(30.0)))]))
    assert abs(lo[0] - 90.0) <= 1e-12 and abs(la[0] - 30.0) <= 1e-12
    assert [float(v[0]) for v in fwd(WR.GEOGRAPHIC, [12.5], [-7.25])] == [12.5, -7.25]
    assert [float(v[0]) for v in inv(WR.GEOGRAPHIC, [12.5], [-7.25])] == [12.5, -7.25]
    # outside the domain: beyond 89.9 degrees, 80 degrees from the central meridian, not finite
    assert np.isnan(fwd(WR.utm(36), [33.0], [89.95])[0][0]) and np.isfinite(fwd(WR.utm(36), [33.0], [89.85])[0][0])
    assert np.isnan(fwd(WR.utm(36), [113.0], [10.0])[0][0]) and np.isfinite(fwd(WR.utm(36), [112.9], [10.0])[0][0])
    assert np.isnan(fwd(WR.utm(36), [33.0 - 360.0 + 80.0], [10.0])[0][0]) and np.isfinite(fwd(WR.utm(36), [33.0 + 360.0 + 79.0], [10.0])[0][0])
    assert np.isnan(inv(WR.WEB_MERCATOR, [0.0], [np.inf])[1][0]) and np.isnan(inv(WR.WEB_MERCATOR, [0.0], [6e7])[1][0])  # 6e7 m: 89.99 degrees
    assert np.isnan(inv(WR.GEOGRAPHIC, [np.nan], [0.0])[0][0]) and np.isnan(inv(WR.GEOGRAPHIC, [0.0], [89.95])[1][0])


# ---- GeoKeys ---------------------------------------------------------------------------------------------------------------------------
def test_geokeys_are_read_written_and_refused():
    assert crs.from_profile(_profile(0, 0, 32636)) == crs.Crs(1.0, 33.0, 0.9996, 500000.0, 0.0, 32636)
    assert crs.from_profile(_profile(0, 0, 32736)).params == WR.utm(36, south=True)
    assert crs.from_profile(_profile(0, 0, 32601)).lon0 == -177.0 and crs.from_profile(_profile(0, 0, 32660)).lon0 == 177.0
    assert crs.from_profile(_profile(0, 0, 3857)).params == WR.WEB_MERCATOR and crs.from_profile(_profile(0, 0, 4326)).params == WR.GEOGRAPHIC
    assert crs.parse("EPSG:32636") == crs.from_profile(_profile(0, 0, 32636)) == crs.parse(" epsg:32636 ")
    for code in (32636, 32760, 3857, 4326):
        tags = crs.geokeys(code)
        assert set(tags) == {34735} and crs.from_profile({"tags": tags}).epsg == code
    assert crs.geokeys(32636)[34735] == _tags(0, 0, 32636)[34735] and crs.geokeys(4326)[34735] == _tags(0, 0, 4326)[34735]
    for code in (32600, 32661, 32700, 32761, 27700, 4269, 0):
        with pytest.raises(ValueError, match=f"EPSG:{code}"):
            crs.from_epsg(code)
        with pytest.raises(ValueError, match=f"EPSG:{code}"):
            crs.from_profile(_profile(0, 0, code))
    for bad in ("32636", "EPSG:", "EPSG:36N", "utm36"):
        with pytest.raises(ValueError, match="EPSG:<code>"):
            crs.parse(bad)
    with pytest.raises(ValueError, match="34735"):
        crs.from_profile({"tags": {}})
    user_defined = {34735: (3, (1, 1, 0, 2, 1024, 0, 1, 1, 3072, 34736, 1, 0))}
    with pytest.raises(ValueError, match="another tag"):
        crs.from_profile({"tags": user_defined})


# ---- the target grid -----------------------------------------------------------------------------------------------------------------------
def _seam_sources():
    """Five 16 x 16 chips in EPSG:32636 and three in EPSG:32637 around 36 E, 40.6 N, on 30 m grids -> [(name, epsg, x0, y0)]."""
    x36, y36 = (float(v) for v in WR.from_lonlat(WR.utm(36), 36.0, 40.6))
    x37, y37 = (float(v) for v in WR.from_lonlat(WR.utm(37), 36.0, 40.6))
    x36, y36, x37, y37 = (30.0 * round(v / 30.0) for v in (x36, y36, x37, y37))
    out = [(f"a{k}", 32636, x36 - 480.0 * (k % 3) - 360.0, y36 + 240.0 - 480.0 * (k // 3)) for k in range(5)]
    out += [(f"b{k}", 32637, x37 - 120.0 + 480.0 * k, y37 + 210.0 - 240.0 * (k % 2)) for k in range(3)]
    return out


def test_target_grid_is_order_independent_snaps_outward_and_needs_a_unit():
    src = _seam_sources()
    profs = [_profile(x, y, e) for _, e, x, y in src]
    shapes = [(16, 16)] * len(src)
    base, (H, W) = warp.target_grid(profs, shapes, "EPSG:32636")
    X0, Y0, sx, sy = warp.grid_of(base)
    assert (sx, sy) == (30.0, 30.0) and X0 % 30.0 == 0 and Y0 % 30.0 == 0 and crs.from_profile(base).epsg == 32636
    assert 34736 not in base["tags"] and 34737 not in base["tags"] and (base["height"], base["width"]) == (H, W)
    for perm in ([7, 6, 5, 4, 3, 2, 1, 0], [5, 0, 6, 1, 7, 2, 3, 4]):
        p, s = warp.target_grid([profs[i] for i in perm], shapes, "EPSG:32636")
        assert s == (H, W) and warp.grid_of(p) == (X0, Y0, sx, sy)
    # every source corner, projected by the twin, lies inside; a grid one pixel smaller on any side would lose one
    lo_x = lo_y = np.inf
    hi_x = hi_y = -np.inf
    for _, e, x, y in src:
        system = WR.utm(e - 32600)
        for cx, cy in ((x, y), (x + 480, y), (x, y - 480), (x + 480, y - 480)):
            tx, ty = (cx, cy) if e == 32636 else WR.from_lonlat(WR.utm(36), *WR.to_lonlat(system, cx, cy))  # no projection within one system
            lo_x, hi_x, lo_y, hi_y = min(lo_x, tx), max(hi_x, tx), min(lo_y, ty), max(hi_y, ty)
    assert X0 <= lo_x and X0 + 30.0 * W >= hi_x and Y0 >= hi_y and Y0 - 30.0 * H <= lo_y
    assert X0 + 30.0 > lo_x - 1.0 and X0 + 30.0 * (W - 1) < hi_x + 1.0 and Y0 - 30.0 < hi_y + 1.0 and Y0 - 30.0 * (H - 1) > lo_y - 1.0
    # "first" = the first source's system; another resolution; an off-multiple extent still snaps outward
    first, _ = warp.target_grid(profs[::-1], shapes, "first")
    assert crs.from_profile(first).epsg == 32637
    coarse, (h2, w2) = warp.target_grid(profs, shapes, "EPSG:32636", resolution=100)
    g = warp.grid_of(coarse)
    assert g[2:] == (100.0, 100.0) and g[0] % 100 == 0 and g[0] <= lo_x < g[0] + 100 and g[0] + 100 * (w2 - 1) < hi_x <= g[0] + 100 * w2
    with pytest.raises(ValueError, match="give a resolution"):
        warp.target_grid(profs, shapes, "EPSG:4326")
    deg, (h3, w3) = warp.target_grid(profs, shapes, "EPSG:4326", resolution=0.0005)
    assert crs.from_profile(deg).epsg == 4326 and abs(warp.grid_of(deg)[0] - 36.0) < 0.05 and 2 <= h3 <= 200
    assert warp.target_grid(profs[:1], shapes[:1], "EPSG:3857")[1][0] >= 16  # metres to metres: the resolution is taken over
    for bad in (0, -30.0, float("nan"), "30", True):
        with pytest.raises(ValueError, match="resolution"):
            warp.target_grid(profs, shapes, "EPSG:32636", resolution=bad)
    with pytest.raises(ValueError, match="beyond the kernel's limits"):
        warp.target_grid(profs, shapes, "EPSG:32636", resolution=1e-6)


# ---- config --------------------------------------------------------------------------------------------------------------------------------
def test_config_carries_the_warp_keys_and_they_default_to_off():
    from instageo_amd import run
    from instageo_amd.config import DEFAULTS, load_config

    t = DEFAULTS["test"]
    assert (t["mosaic_crs"], t["mosaic_resolution"], t["mosaic_resampling"]) == (None, None, None)
    off = dict(crs=None, resolution=None, resampling=None)
    assert run.warp_options(load_config("config", [])) == off
    assert run.warp_options(load_config("config", ["mode=chip_inference", "test.mosaic=true"])) == off
    on = ["mode=chip_inference", "test.mosaic=true"]
    cfg = load_config("config", on + ["test.mosaic_crs=EPSG:3857", "test.mosaic_resolution=60", "test.mosaic_resampling=nearest"])
    assert run.warp_options(cfg) == dict(crs="EPSG:3857", resolution=60, resampling="nearest")
    assert run.warp_options(load_config("config", on + ["test.mosaic_crs=first"]))["crs"] == "first"
    reg = on + ["is_reg_task=true", "model.num_classes=1", "test.mosaic_crs=first"]
    assert run.warp_options(load_config("config", reg + ["test.mosaic_resampling=bilinear"]))["resampling"] == "bilinear"
    for ov, what in (("test.mosaic_crs=EPSG:27700", "EPSG:27700"), ("test.mosaic_crs=utm", "EPSG:<code>"), ("test.mosaic_crs=36", "mosaic_crs"),
                     ("test.mosaic_resolution=-1", "mosaic_resolution"), ("test.mosaic_resolution=fine", "mosaic_resolution"),
                     ("test.mosaic_resampling=cubic", "mosaic_resampling")):
        with pytest.raises(ValueError, match=what):
            run.warp_options(load_config("config", on + ["test.mosaic_crs=first", ov]))
    for ov in ("test.mosaic_crs=first", "test.mosaic_resolution=30", "test.mosaic_resampling=nearest"):
        with pytest.raises(ValueError, match="needs test.mosaic"):
            run.warp_options(load_config("config", ["mode=chip_inference", ov]))
    with pytest.raises(ValueError, match="needs test.mosaic_crs"):
        run.warp_options(load_config("config", on + ["test.mosaic_resolution=30"]))
    with pytest.raises(ValueError, match="bilinear does not go with a classification head"):
        run.warp_options(load_config("config", on + ["test.mosaic_crs=first", "test.mosaic_resampling=bilinear"]))
    with pytest.raises(ValueError, match="mosaic_cover does not go with test.mosaic_crs"):
        run.warp_options(load_config("config", on + ["test.mosaic_crs=first", "test.mosaic_cover=true"]))
    # what run.py hands to merge_reprojected binds to its signature, which is merge_predictions' plus the three new keywords
    import inspect

    params = list(inspect.signature(warp.merge_reprojected).parameters)
    assert params[:2] + params[5:] == list(inspect.signature(mosaic.merge_predictions).parameters) and params[2:5] == ["crs", "resolution", "resampling"]
    assert set(run.warp_options(cfg)) == set(params[2:5])


# ---- the entry points ------------------------------------------------------------------------------------------------------------------------
def test_header_states_the_rule():
    import re

    text = open(os.path.join(ROOT, "include", "instageo_hip.h")).read()
    block = " ".join(" ".join(re.sub(r"\n \*", " ", c).split()) for c in re.findall(r"/\*.*?\*/", text, flags=re.S) if "ig_warp:" in c)
    for phrase in ("(kind, lon0, k0, FE, FN)", "to n^6", "[c, c + 1) x [r, r + 1)", "|latitude| > 89.9", ">= 80 degrees", "c = floor(u)",
                   "floor(u - 0.5)", "rounded once to float32", "0x7fc00000", "255 for none", "bit-identical from run to run", "no atomics"):
        assert phrase in block, phrase


def test_entry_points_exported_and_validated_without_gpu(built_lib):
    """IG_REQUIRE rejects bad arguments before any launch, and an empty destination returns before a pointer is looked at."""
    assert {"ig_warp", "ig_warp_coords"} <= set(built_lib.declared_symbols())
    lib, err = built_lib.load(), built_lib.last_error
    one, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    ok = dict(src=one, starts=one, src_crs=one, src_grid=one, src_size=one, nsrc=1, bin_ptr=one, bin_idx=one, dst_crs=one, dst_grid=one, H=8, W=8,
              elem_size=1, resampling=0, rule=0, fill=-1, dst=one, src_id=None, stream=None)
    call = lambda **kw: lib.ig_warp(*{**ok, **kw}.values())  # noqa: E731
    for kw, what in ((dict(elem_size=2), "elem_size"), (dict(resampling=2), "resampling"), (dict(resampling=1), "bilinear resampling needs float32"),
                     (dict(rule=2), "rule"), (dict(rule=3), "rule"), (dict(fill=128), "fill"), (dict(H=-1), "H >= 0"), (dict(H=65536, W=65536), "2^31"),
                     (dict(nsrc=9), "nsrc"), (dict(nsrc=-1), "nsrc"), (dict(dst=None), "null"), (dict(dst_crs=None), "null"), (dict(src=None), "null"),
                     (dict(src_grid=None), "null"), (dict(bin_ptr=None), "null"), (dict(dst_grid=odd), "aligned"), (dict(src_crs=odd), "aligned"),
                     (dict(starts=odd), "aligned"), (dict(elem_size=4, dst=ctypes.c_void_p(4098)), "aligned"),
                     (dict(elem_size=4, src=ctypes.c_void_p(4098)), "aligned"), (dict(H=64 * 65535 + 1, W=1), "65535 blocks")):
        assert call(**kw) == -1 and what in err(), (kw, err())
    assert call(H=0, dst=None, src=None) == 0 and call(W=0, dst=None, dst_crs=None) == 0  # H * W = 0
    cok = dict(dst_crs=one, dst_grid=one, H=8, W=8, src_crs=one, src_grid=one, uv=one, stream=None)
    ccall = lambda **kw: lib.ig_warp_coords(*{**cok, **kw}.values())  # noqa: E731
    for kw, what in ((dict(W=-1), "W >= 0"), (dict(H=65536, W=65536), "2^31"), (dict(uv=None), "null"), (dict(src_crs=None), "null"),
                     (dict(uv=odd), "aligned"), (dict(dst_grid=odd), "aligned"), (dict(H=4 * 65535 + 1, W=1), "65535 workgroups")):
        assert ccall(**kw) == -1 and what in err(), (kw, err())
    assert ccall(H=0, uv=None) == 0
    with pytest.raises(built_lib.HipLibraryError, match="bilinear resampling needs float32"):
        built_lib.call("ig_warp", *{**ok, "resampling": 1}.values())


def test_generated_custom_ops_follow_the_header():
    from instageo_amd import torch_ops

    raw = torch_ops.register()
    s = raw["warp"]
    assert "Tensor? src," in s and "Tensor? src_crs" in s and "Tensor? bin_idx" in s and "Tensor? dst_grid" in s and "Tensor(a!)? dst" in s
    assert "Tensor(b!)? src_id" in s and "int nsrc" in s and "int resampling" in s and "int rule" in s and "stream" not in s
    c = raw["warp_coords"]
    assert "Tensor? dst_crs" in c and "Tensor? src_grid" in c and "Tensor(a!)? uv" in c and "int H" in c


def test_warp_refuses_what_it_cannot_do():
    i8, f32 = np.zeros((4, 4), dtype=np.int8), np.zeros((4, 4), dtype=np.float32)
    p = _profile(300000.0, 4500000.0, 32636, 4, 4)
    assert warp.warp([i8], [p], p, (4, 4)).dtype == np.int8
    for args, what in ((([i8], [p], p, (4, 4), "bilinear"), "bilinear resampling does not go with int8"),
                       (([f32], [p], p, (4, 4), "cubic"), "resampling must be one of"),
                       (([i8], [p], p, (4, 4), "nearest", "mode"), "rule"),
                       (([i8, f32], [p, p], p, (4, 4)), "one dtype"),
                       (([i8], [p, p], p, (4, 4)), "1 sources but 2 profiles"),
                       (([i8] * 9, [p] * 9, p, (4, 4)), "at most 8"),
                       (([i8.astype(np.int16)], [p], p, (4, 4)), "int8 class maps or float32"),
                       (([i8], [p], p, (4, 4), "nearest", "last", 300), "fill"),
                       (([i8], [{"tags": {}}], p, (4, 4)), "34735"),
                       (([i8], [p], _profile(0, 0, 27700), (4, 4)), "EPSG:27700"),
                       (([i8], [p], p, (1 << 16, 1 << 16)), "beyond the kernel's limits")):
        with pytest.raises(ValueError, match=what):
            warp.warp(*args)
    with pytest.raises(ValueError, match="ModelTransformation"):
        warp.warp([i8], [dict(p, tags={**p["tags"], 34264: (12, (0.0,) * 16)})], p, (4, 4))


# ---- the host path against the twin ------------------------------------------------------------------------------------------------------
def _raster(rng, h, w, dtype):
    if dtype == "int8":
        a = rng.integers(0, 4, size=(h, w)).astype(np.int8)
        a[rng.random((h, w)) < 0.05] = -1
    else:
        a = rng.normal(size=(h, w)).astype(np.float32)
        a[rng.random((h, w)) < 0.05] = np.nan
    return a


@pytest.mark.parametrize("dtype,resampling", [("int8", "nearest"), ("float32", "nearest"), ("float32", "bilinear")])
def test_host_path_equals_the_twin_across_zones(dtype, resampling):
    rng = np.random.default_rng(11)
    x36, y36 = (30.0 * round(float(v) / 30.0) for v in WR.from_lonlat(WR.utm(36), 36.0, 40.6))
    x37, y37 = (30.0 * round(float(v) / 30.0) for v in WR.from_lonlat(WR.utm(37), 36.0, 40.6))
    # the first source lies 7 m / 11 m off the 30 m target grid: on it, every bilinear sample would sit on a half-integer tie
    srcs = [(_raster(rng, 40, 36, dtype), 32636, x36 - 893.0, y36 + 611.0), (_raster(rng, 38, 44, dtype), 32637, x37 - 300.0, y37 + 500.0)]
    arrays = [a for a, *_ in srcs]
    profs = [_profile(x, y, e, *a.shape, dtype=dtype) for a, e, x, y in srcs]
    dst, shape = warp.target_grid(profs, [a.shape for a in arrays], "EPSG:32636")
    systems, grids = [WR.utm(e - 32600) for _, e, _, _ in srcs], [(x, y, 30.0, 30.0) for _, _, x, y in srcs]
    dgrid = warp.grid_of(dst)
    for i in range(2):  # the coordinates first: the host path is the device's yardstick in the end-to-end test
        ua, va = WR.coords(WR.utm(36), dgrid, shape, systems[i], grids[i])
        ub, vb = warp.coords(WR.utm(36), dgrid, shape, systems[i], grids[i])
        assert np.abs(ua - ub).max() <= 1e-6 and np.abs(va - vb).max() <= 1e-6
    for rule in ("last", "first"):
        want, want_id, ties, _ = WR.warp(arrays, systems, grids, WR.utm(36), dgrid, shape, resampling, rule)
        got, got_id = warp.warp(arrays, profs, dst, shape, resampling, rule, src_id=True)
        keep = ~ties
        assert ties.mean() <= 1e-3 and {0, 1, 255} == set(np.unique(want_id))
        assert np.array_equal(got_id[keep], want_id[keep])
        if resampling == "nearest":
            assert np.array_equal(got.view(f"u{got.itemsize}")[keep], want.view(f"u{want.itemsize}")[keep])
        else:
            assert np.array_equal(np.isnan(got)[keep], np.isnan(want)[keep])
            both = keep & ~np.isnan(want)
            assert (np.abs(got[both].astype(np.float64) - want[both]) <= 2.0**-22 * np.abs(arrays[0][~np.isnan(arrays[0])]).max()).all()
    ptr, idx = warp.block_lists(WR.utm(36), dgrid, shape, systems, grids, [a.shape for a in arrays])
    assert len(ptr) == -(-shape[0] // 64) * -(-shape[1] // 64) + 1 and ptr[-1] == len(idx) and set(idx) == {0, 1}


# ---- files -> files, on the host ---------------------------------------------------------------------------------------------------------
def _write_seam_chips(folder, dtype="int8"):
    rng = np.random.default_rng(6)
    os.makedirs(folder, exist_ok=True)
    paths = []
    for name, epsg, x, y in _seam_sources():
        a = _raster(rng, 16, 16, dtype)
        p = os.path.join(folder, f"prediction_{name}.tif")
        tiff.write(p, a, {"tags": _tags(x, y, epsg), "nodata": None})
        paths.append(p)
    return paths


def test_merge_reprojected_on_the_host(tmp_path):
    src, out = str(tmp_path / "predictions"), str(tmp_path / "merged")
    paths = _write_seam_chips(src)
    written = warp.merge_reprojected(src, out, crs="EPSG:32636", num_classes=4, device="cpu", cog=False)
    merged = os.path.join(out, "predictions_merged.tif")
    assert written == [merged] and os.listdir(out) == ["predictions_merged.tif"]
    got, prof = tiff.read(merged)
    assert crs.from_profile(prof).epsg == 32636 and prof["tags"][34735] == crs.geokeys(32636)[34735] and got.dtype == np.int8
    assert 34736 not in prof["tags"] and 34737 not in prof["tags"] and prof["tags"][42113] == (2, "-1")
    # the same from the pieces: the two group mosaics as merge_predictions pastes them, warped by the twin
    arrays = [tiff.read(p)[0][0] for p in paths]
    groups = mosaic.placement([tiff.read(p)[1] for p in paths], [a.shape for a in arrays], paths)
    assert len(groups) == 2
    canvases = [mosaic.paste([arrays[i] for i in g.members], g.rects, g.shape, "last") for g in groups]
    dgrid, shape = warp.grid_of(prof), got.shape[1:]
    want, want_id, ties, _ = WR.warp(canvases, [WR.utm(36), WR.utm(37)], [warp.grid_of(g.profile) for g in groups], WR.utm(36), dgrid, shape)
    assert np.array_equal(got[0][~ties], want[~ties]) and ties.mean() <= 1e-3 and {0, 1} <= set(np.unique(want_id))
    assert (got[0] >= 0).mean() > 0.3
    # as a COG with statistics; the default target is the first file's system; first lets the earlier group win
    cogged = warp.merge_reprojected(paths[::-1], str(tmp_path / "cog"), num_classes=4, device="cpu", cog_blocksize=128, overview_levels=1, rule="first")
    assert [os.path.basename(p) for p in cogged] == ["predictions_merged.tif", "cogstats_merged.json"]
    assert crs.from_profile(tiff.read(cogged[0])[1]).epsg == 32637 and tiff.overview_count(cogged[0]) == 1
    assert sorted(warp.TIMINGS) == ["paste", "products", "read", "warp", "write"]
    for kw, what in ((dict(save_cover=True), "no cover raster"), (dict(resampling="bilinear"), "bilinear resampling does not go with int8"),
                     (dict(resampling="cubic"), "resampling must be"), (dict(crs="EPSG:27700"), "EPSG:27700"), (dict(rule="mean"), "mean"),
                     (dict(save_regions=True), "device='cpu'"), (dict(crs="EPSG:4326"), "give a resolution")):
        with pytest.raises(ValueError, match=what):
            warp.merge_reprojected(src, str(tmp_path / "no"), device="cpu", **kw)
    assert not os.path.exists(str(tmp_path / "no")) or os.listdir(str(tmp_path / "no")) == []


def test_merge_reprojected_floats_default_to_bilinear(tmp_path):
    src = str(tmp_path / "p")
    paths = _write_seam_chips(src, "float32")
    out = warp.merge_reprojected(src, str(tmp_path / "m"), crs="EPSG:32637", resolution=20, device="cpu", cog=False, rule="mean")  # 20 m: no sample on a half-integer tie
    got, prof = tiff.read(out[0])
    arrays = [tiff.read(p)[0][0] for p in paths]
    groups = mosaic.placement([tiff.read(p)[1] for p in paths], [a.shape for a in arrays], paths, "float32")
    canvases = [mosaic.paste([arrays[i] for i in g.members], g.rects, g.shape, "mean") for g in groups]
    want, _, ties, scale = WR.warp(canvases, [WR.utm(36), WR.utm(37)], [warp.grid_of(g.profile) for g in groups], WR.utm(37), warp.grid_of(prof),
                                   got.shape[1:], "bilinear", "last")
    keep = ~ties
    assert got.dtype == np.float32 and np.array_equal(np.isnan(got[0])[keep], np.isnan(want)[keep]) and prof["tags"][42113] == (2, "nan")
    both = keep & ~np.isnan(want)
    assert both.sum() > 500 and (np.abs(got[0][both].astype(np.float64) - want[both]) <= 2.0**-22 * scale[both]).all()


def test_without_a_target_the_mosaics_stay_one_per_zone_byte_for_byte(tmp_path):
    """``test.mosaic_crs`` unset: run.py calls merge_predictions as before, and its files hold the bytes they always held -- the canvas of
    the paste rule under the group's profile, written by tiff.write."""
    from instageo_amd import run
    from instageo_amd.config import load_config

    assert run.warp_options(load_config("config", ["mode=chip_inference", "test.mosaic=true"]))["crs"] is None
    src, out = str(tmp_path / "p"), str(tmp_path / "m")
    paths = _write_seam_chips(src)
    written = mosaic.merge_predictions(src, out, num_classes=4, device="cpu", cog=False)
    assert [os.path.basename(p) for p in written] == ["predictions_merged_0.tif", "predictions_merged_1.tif"] == sorted(os.listdir(out))
    arrays = [tiff.read(p)[0][0] for p in paths]
    groups = mosaic.placement([tiff.read(p)[1] for p in paths], [a.shape for a in arrays], paths)
    import mosaic_reference as MR

    for k, g in enumerate(groups):
        want = MR.reference([arrays[i] for i in g.members], g.rects.tolist(), g.shape, "last", -1)[0]
        ref = str(tmp_path / f"ref_{k}.tif")
        tiff.write(ref, want, g.profile)
        assert open(written[k], "rb").read() == open(ref, "rb").read()
