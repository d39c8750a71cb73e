"""A 50-digit reference of the map projections of include/instageo_hip.h, and the fixture made from it.

It shares nothing with Krueger's series (csrc/warp_proj.h, instageo_amd/crs.py, tests/warp_reference.py): no series coefficients, no
rectifying radius, no third flattening.  Transverse Mercator is computed from its definition, the conformal map of the ellipsoid that is
true to scale (times k0) along the central meridian:
  1. the complex isometric latitude  w = psi(phi) + i lambda,  psi(phi) = asinh(tan phi) - e atanh(e sin phi);
  2. the complex latitude z with psi(z) = w, by Newton from atan(sinh w) with psi'(z) = (1 - e^2) / ((1 - e^2 sin^2 z) cos z);
  3. N + i E = k0 M(z),  M(z) = a (1 - e^2) int_0^z (1 - e^2 sin^2 t)^(-3/2) dt  (the meridian arc, continued analytically), by
     ``mp.quad`` along the straight path from 0 to z;
  4. the inverse by Newton on 3 (M' is the integrand), then w = psi(z): lambda = Im w and phi from Re w by Newton on the real psi.
The line Re z = pi / 2 is the image of the line xi' = pi / 2 of the header's domain rule (both maps commute with the reflection in the
pole), so "beyond the pole" is |Re z| > pi / 2 here.  Spherical web Mercator is x = R lambda, y = R asinh(tan phi); geographic is the
identity.  A chain goes destination -> (longitude, latitude) -> source without rounding in between.

This module imports neither the product nor ``warp_reference``.  ``python tests/projection_truth.py`` writes
tests/golden/projection_truth.npz (a few minutes on one core, a pool of workers is used where there are more): for every lattice of
``lattices()`` the float64 (u, v) of its pixel centres in the source grid (0, 0, 1, 1) -- so u = x' and v = -y' in the source's own units
-- and the true longitude and latitude, NaN where the header's domain rule says NaN.  Pixel centres are the float64 values
``X0 + (c + 0.5) * sx`` and ``Y0 - (r + 0.5) * sy``; the reference is evaluated AT those float64 values and rounded once, to nearest.
"""
import os

import numpy as np

try:
    import mpmath
    from mpmath import mp, mpc, mpf
except ImportError:  # the fixture alone is enough for everything but regeneration
    mpmath = None

DPS = 50
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "projection_truth.npz")
GEOGRAPHIC = (0.0, 0.0, 0.0, 0.0, 0.0)
WEB_MERCATOR = (2.0, 0.0, 0.0, 0.0, 0.0)
UNIT_GRID = (0.0, 0.0, 1.0, 1.0)
LAT_MAX, DLON_MAX = 89.9, 80.0  # the header's domain rule
GUARD_DEG, GUARD_RAD = 1e-9, 1e-11  # no pixel centre of the fixture lies closer than this to an edge of the domain


def utm(zone, south=False):
    return (1.0, 6.0 * zone - 183.0, 0.9996, 500000.0, 1e7 if south else 0.0)


# ---- the ellipsoid ---------------------------------------------------------------------------------------------------------------------
def _a():
    return mpf(6378137)


def _e2():
    f = 1 / mpf("298.257223563")
    return f * (2 - f)


def _tiny():
    return mpf(10) ** (-(mp.dps - 6))


def psi(z):
    e = mp.sqrt(_e2())
    return mp.asinh(mp.tan(z)) - e * mp.atanh(e * mp.sin(z))


def dpsi(z):
    e2 = _e2()
    return (1 - e2) / ((1 - e2 * mp.sin(z) ** 2) * mp.cos(z))


def _newton(f, df, z, what):
    """Newton from z; ends after the first step below 10^-(dps - 6) of the scale (the next iterate is then right to working precision)."""
    for _ in range(200):
        step = f(z) / df(z)
        z = z - step
        if abs(step) <= _tiny() * (1 + abs(z)):
            return z
    raise ArithmeticError(f"Newton for {what} did not converge")


def complex_latitude(w):
    return _newton(lambda z: psi(z) - w, dpsi, mp.atan(mp.sinh(w)), "the complex latitude")


def meridian(z):
    """M(z) in metres, z real or complex."""
    e2 = _e2()
    return _a() * (1 - e2) * mp.quad(lambda t: (1 - e2 * mp.sin(t) ** 2) ** mpf(-1.5), [0, z])


def dmeridian(z):
    e2 = _e2()
    return _a() * (1 - e2) * (1 - e2 * mp.sin(z) ** 2) ** mpf(-1.5)


def wrap180(d):
    """Degrees into [-180, 180] by the IEEE remainder (ties do not matter: they are outside the domain)."""
    return d - 360 * mp.nint(d / 360)


# ---- transverse Mercator ---------------------------------------------------------------------------------------------------------------
def tm_forward(crs, lon, lat):
    """(longitude, latitude) in degrees -> (x, y) in metres of the transverse Mercator system ``crs``; no domain rule."""
    _, lon0, k0, fe, fn = (mpf(v) for v in crs)
    w = mpc(psi(mp.radians(mpf(lat))), mp.radians(wrap180(mpf(lon) - lon0)))
    m = k0 * meridian(complex_latitude(w))
    return fe + m.imag, fn + m.real


def tm_complex_latitude(crs, x, y):
    """The complex latitude of the point (x, y) of ``crs`` (Re beyond +-pi / 2: beyond the pole)."""
    _, _, k0, fe, fn = (mpf(v) for v in crs)
    target = mpc(mpf(y) - fn, mpf(x) - fe) / k0
    return _newton(lambda z: meridian(z) - target, dmeridian, target / _a(), "the inverse transverse Mercator")


def tm_inverse(crs, x, y):
    """(x, y) -> (longitude, latitude) in degrees, the longitude as lon0 + lambda (not wrapped); None beyond the pole."""
    z = tm_complex_latitude(crs, x, y)
    if abs(z.real) > mp.pi / 2:
        return None
    w = psi(z)
    phi = _newton(lambda p: psi(p) - w.real, dpsi, mp.atan(mp.sinh(w.real)), "the latitude")
    return mpf(crs[1]) + mp.degrees(w.imag), mp.degrees(phi)


# ---- the chain of the header -------------------------------------------------------------------------------------------------------------
def to_lonlat(crs, x, y):
    """-> (lon, lat) in degrees as mpf, or None outside the domain."""
    kind = int(crs[0])
    x, y = mpf(x), mpf(y)
    if kind == 0:
        lon, lat = x, y
    elif kind == 2:
        lon, lat = mp.degrees(x / _a()), mp.degrees(mp.atan(mp.sinh(y / _a())))
    else:
        got = tm_inverse(crs, x, y)
        if got is None:
            return None
        lon, lat = got
    return (lon, lat) if abs(lat) <= mpf(LAT_MAX) else None


def from_lonlat(crs, lon, lat):
    """-> (x, y) as mpf, or None outside the domain."""
    kind = int(crs[0])
    if kind == 0:
        return lon, lat
    if kind == 2:
        return _a() * mp.radians(lon), _a() * mp.asinh(mp.tan(mp.radians(lat)))
    if not abs(wrap180(lon - mpf(crs[1]))) < mpf(DLON_MAX):
        return None
    return tm_forward(crs, lon, lat)


def near_edge(dst_crs, src_crs, x, y):
    """True where the point lies within the guard of an edge of the domain (the fixture must hold no such point: there the float64 rule
    and the truth may fall on different sides)."""
    with mp.workdps(25):  # the guards are coarse: half the digits do
        x, y = mpf(x), mpf(y)
        kind = int(dst_crs[0])
        if kind == 0:
            lon, lat = x, y
        elif kind == 2:
            lon, lat = mp.degrees(x / _a()), mp.degrees(mp.atan(mp.sinh(y / _a())))
        else:
            z = tm_complex_latitude(dst_crs, x, y)
            if abs(abs(z.real) - mp.pi / 2) < GUARD_RAD:
                return True
            if abs(z.real) > mp.pi / 2:
                return False
            w = psi(z)
            lon, lat = mpf(dst_crs[1]) + mp.degrees(w.imag), mp.degrees(mp.atan(mp.sinh(w.real)))  # the conformal latitude, within 0.2 degrees
            if abs(abs(lat) - LAT_MAX) < 0.3:
                lon, lat = tm_inverse(dst_crs, x, y)
        if abs(abs(lat) - LAT_MAX) < GUARD_DEG:
            return True
        return int(src_crs[0]) == 1 and abs(lat) <= LAT_MAX and abs(abs(wrap180(lon - mpf(src_crs[1]))) - DLON_MAX) < GUARD_DEG


def _f64(x):
    return mpmath.libmp.to_float(mpf(x)._mpf_, rnd="n")  # float() would truncate


def point(dst_crs, src_crs, x, y, dps=DPS):
    """One destination point (float64 x, y) -> float64 (u, v, lon, lat) in the source grid (0, 0, 1, 1), NaN outside the domain."""
    nan = float("nan")
    with mp.workdps(dps):
        ll = to_lonlat(dst_crs, x, y)
        if ll is None:
            return nan, nan, nan, nan
        xy = from_lonlat(src_crs, *ll)
        if xy is None:
            return nan, nan, nan, nan
        return _f64(xy[0]), _f64(-xy[1]), _f64(ll[0]), _f64(ll[1])


# ---- the lattices ------------------------------------------------------------------------------------------------------------------------
def centres(grid, shape):
    """The float64 pixel centres of a grid, as the header states them -> (x (W,), y (H,))."""
    X0, Y0, sx, sy = (float(v) for v in grid)
    return X0 + (np.arange(shape[1], dtype=np.float64) + 0.5) * sx, Y0 - (np.arange(shape[0], dtype=np.float64) + 0.5) * sy


def _span(xlo, xhi, ylo, yhi, W, H):
    """The grid whose W x H pixel centres run from (xlo, yhi) at the top left to (xhi, ylo)."""
    sx, sy = (xhi - xlo) / (W - 1), (yhi - ylo) / (H - 1)
    return (xlo - sx / 2, yhi + sy / 2, sx, sy), (H, W)


def _around(crs, lon, lat, half_w, half_h, n=7):
    """An n x n lattice of ``crs`` around the point (lon, lat), on whole metres (float64 arithmetic is enough to place a lattice)."""
    with mp.workdps(30):
        x, y = (round(float(v)) for v in from_lonlat(crs, mpf(lon), mpf(lat)))
    return _span(x - half_w, x + half_w, y - half_h, y + half_h, n, n)


def lattices():
    """name -> (dst_crs, dst_grid, (H, W), src_crs, outer).  The source grid is always (0, 0, 1, 1)."""
    U36, U37, U36S, U37S, U21S, U1, U60 = utm(36), utm(37), utm(36, True), utm(37, True), utm(21, True), utm(1), utm(60)
    CUSTOM = (1.0, 9.5, 1.0, 1.5e6, -2e5)
    G, WM = GEOGRAPHIC, WEB_MERCATOR
    out = {}

    def add(name, dst_crs, span, src_crs, outer=False):
        out[name] = (tuple(dst_crs), span[0], span[1], tuple(src_crs), outer)

    # core, forward: geographic -> transverse Mercator
    add("fwd_utm36_wide", G, _span(-7.0, 73.0, -89.8, 89.8, 15, 15), U36)
    add("fwd_origin_micro", G, _span(33.0 - 5e-3, 33.0 + 5e-3, -5e-3, 5e-3, 11, 11), U36)
    add("fwd_near_pole", G, _span(-7.0, 73.0, 89.0, 89.96, 11, 15), U36)
    add("fwd_zone1_east_of_180", G, _span(-180.0, -170.0, -80.0, 80.0, 9, 9), U1)
    add("fwd_zone1_west_of_180", G, _span(170.0, 180.0, -80.0, 80.0, 9, 9), U1)
    add("fwd_zone60_east_of_180", G, _span(-180.0, -170.0, -80.0, 80.0, 9, 9), U60)
    add("fwd_zone60_west_of_180", G, _span(170.0, 180.0, -80.0, 80.0, 9, 9), U60)
    add("fwd_utm21_south", G, _span(-60.5, -53.5, -80.0, 0.5, 9, 11), U21S)
    add("fwd_custom_tm", G, _span(-10.5, 29.5, -60.0, 75.0, 9, 11), CUSTOM)
    # core, inverse: transverse Mercator -> geographic
    add("inv_utm36_wide", U36, _span(5e5 - 4.8e6, 5e5 + 4.8e6, 0.0, 9.98e6, 13, 13), G)
    add("inv_origin_micro", U36, _span(5e5 - 500.0, 5e5 + 500.0, -500.0, 500.0, 11, 11), G)
    add("inv_near_pole", U36, _span(5e5 - 6e4, 5e5 + 6e4, 9.93e6, 1.002e7, 13, 13), G)
    add("inv_beyond_pole", U36, _span(5e5 - 3e6, 5e5 + 3e6, -1.2e7, 1.2e7, 7, 9), G)
    add("inv_utm21_south", U21S, _span(1e5, 9e5, 1.1e6, 1.0035e7, 9, 11), G)
    add("inv_custom_tm", CUSTOM, _span(1.5e6 - 1.4e6, 1.5e6 + 1.4e6, -6.8e6, 8.1e6, 9, 11), G)
    # web Mercator
    add("wm_from_geographic", G, _span(-180.0, 180.0, -85.06, 85.06, 13, 13), WM)
    add("wm_to_geographic", WM, _span(-2.0037e7, 2.0037e7, -2.0037e7, 2.0037e7, 13, 13), G)
    for lat in (0.1, 40.0, 80.0):
        tag = f"{lat:g}".replace(".", "p")
        add(f"wm_to_utm36_lat{tag}", WM, _around(WM, 34.0, lat, 3e5, 2e5), U36)
        add(f"wm_from_utm36_lat{tag}", U36, _around(U36, 34.0, lat, 1.5e5 if lat > 60 else 3e5, 2e5), WM)
    # transverse Mercator -> transverse Mercator
    for lat in (0.1, 40.6, 80.0):
        tag = f"{lat:g}".replace(".", "p")
        add(f"tm_utm37_to_utm36_lat{tag}", U37, _around(U37, 36.0, lat, 5e4 if lat > 60 else 1.5e5, 1e5), U36)
    add("tm_utm36_to_utm37_lat40p6", U36, _around(U36, 36.0, 40.6, 1.5e5, 1e5), U37)
    add("tm_north_to_south_equator", U36, _span(2e5, 8e5, -3e5, 3e5, 7, 7), U36S)
    add("tm_south_to_north_equator", U36S, _span(6e5, 9e5, 1e7 - 3e5, 1e7 + 3e5, 7, 7), U37)
    add("tm_zone1_to_zone60", U1, _around(U1, 180.0, 40.0, 2e5, 2e5), U60)
    add("tm_zone60_to_zone1", U60, _around(U60, -179.5, -35.0, 2e5, 2e5), U1)
    # the outer band, forward only: beyond 40 degrees from the central meridian the series' own truncation error grows
    add("outer_east", G, ((33.0 + 38.75, 82.5, 2.5, 5.0), (17, 16)), U36, outer=True)  # 40 ... 77.5 degrees x 80 ... 0
    add("outer_edge", G, _span(33.0 + 78.0, 33.0 + 79.9, 0.0, 80.0, 5, 17), U36, outer=True)
    add("outer_west", G, _span(33.0 - 79.9, 33.0 - 40.0, -60.0, 60.0, 9, 7), U36, outer=True)
    return out


def _row(args):
    dst_crs, src_crs, xs, y = args
    for x in xs:
        if near_edge(dst_crs, src_crs, x, y):
            raise ValueError(f"the centre ({x}, {y}) lies on an edge of the domain: move the lattice")
    return [point(dst_crs, src_crs, x, y) for x in xs]


def evaluate(lattice, pool=None):
    """One lattice of :func:`lattices` -> (u, v, lon, lat), float64 (H, W)."""
    dst_crs, grid, shape, src_crs, _ = lattice
    xs, ys = centres(grid, shape)
    jobs = [(dst_crs, src_crs, [float(x) for x in xs], float(y)) for y in ys]
    with mp.workdps(DPS):
        rows = pool.map(_row, jobs) if pool is not None else [_row(j) for j in jobs]
    return tuple(np.array(rows, dtype=np.float64)[:, :, k] for k in range(4))


def generate(path=FIXTURE):
    """Write the fixture: per lattice ``<name>/u``, ``/v``, ``/lon``, ``/lat`` and the table of their descriptions."""
    import multiprocessing

    table = lattices()
    data = {
        "names": np.array(list(table)),
        "dst_crs": np.array([t[0] for t in table.values()], dtype=np.float64),
        "dst_grid": np.array([t[1] for t in table.values()], dtype=np.float64),
        "shape": np.array([t[2] for t in table.values()], dtype=np.int64),
        "src_crs": np.array([t[3] for t in table.values()], dtype=np.float64),
        "outer": np.array([t[4] for t in table.values()], dtype=bool),
    }
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        for name, lattice in table.items():
            for key, plane in zip("u v lon lat".split(), evaluate(lattice, pool)):
                data[f"{name}/{key}"] = plane
            print(f"{name}: {lattice[2][0]} x {lattice[2][1]}, {int(np.isnan(data[name + '/u']).sum())} outside the domain", flush=True)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **data)
    return path


def load(path=FIXTURE):
    """The fixture as a dict name -> dict(dst_crs, dst_grid, shape, src_crs, src_grid, outer, u, v, lon, lat).  numpy only."""
    z = np.load(path)
    out = {}
    for i, name in enumerate(z["names"]):
        name = str(name)
        out[name] = dict(dst_crs=tuple(z["dst_crs"][i]), dst_grid=tuple(z["dst_grid"][i]), shape=tuple(int(v) for v in z["shape"][i]),
                         src_crs=tuple(z["src_crs"][i]), src_grid=UNIT_GRID, outer=bool(z["outer"][i]),
                         **{k: z[f"{name}/{k}"] for k in ("u", "v", "lon", "lat")})
    return out


# ---- truth at pixel scale: the picks of the value kernels ---------------------------------------------------------------------------------
# The lattices above have pixels of 16 to 830 km and cross no 64 x 64 block seam: a raster under them would forgive kilometres.  The pick
# cases have 10 to 30 m pixels (or that fraction of a degree) and a destination larger than one block; the truth is kept at a SAMPLE of
# their pixels, as the source's own map coordinates (x', y'), so that tests/warp_pick_reference.py can lay any source grid under them.
PICK_FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "warp_pick_truth.npz")
PICK_POINTS = 250  # per case
SEAM_LINES = (0, 63, 64, 127, 128)  # rows and columns on both sides of the 64 x 64 block seams, with the last one
WM_ORIGIN = 6378137.0 * float(np.pi)  # the web Mercator square spans +-WM_ORIGIN


def _px_around(crs, lon, lat, px, shape):
    """The H x W grid of ``crs`` with square pixels ``px`` whose centre is the multiple of ``px`` nearest to the point (lon, lat)."""
    H, W = shape
    with mp.workdps(30):
        x, y = (float(v) for v in from_lonlat(crs, mpf(lon), mpf(lat)))
    return (round(x / px) * px - (W // 2) * px, round(y / px) * px + (H // 2) * px, px, px), (H, W)


def _wm_tile_corner(lon, lat, z, tile, shape):
    """The H x W grid on the pixel lattice of the XYZ tiles of zoom ``z`` (``tile`` pixels a side) from the north-west corner of the tile
    that holds (lon, lat)."""
    side = 2.0 * WM_ORIGIN / (1 << z)
    with mp.workdps(30):
        x, y = (float(v) for v in from_lonlat(WEB_MERCATOR, mpf(lon), mpf(lat)))
    return (-WM_ORIGIN + np.floor((x + WM_ORIGIN) / side) * side, WM_ORIGIN - np.floor((WM_ORIGIN - y) / side) * side, side / tile, side / tile), shape


def pick_lattices():
    """name -> (dst_crs, dst_grid, (H, W), src_crs): core domain only, every point within 40 degrees of both central meridians."""
    U36, U37, U36S, U21S, U1, U60, U32 = utm(36), utm(37), utm(36, True), utm(21, True), utm(1), utm(60), utm(32)
    CUSTOM = (1.0, 9.5, 1.0, 1.5e6, -2e5)
    G, WM = GEOGRAPHIC, WEB_MERCATOR
    DEG = 2.0**-13  # 13.6 m of latitude
    out = {}

    def add(name, dst_crs, span, src_crs):
        out[name] = (tuple(dst_crs), tuple(float(v) for v in span[0]), tuple(span[1]), tuple(src_crs))

    add("utm37_to_utm36_lat40p6", U37, _px_around(U37, 36.0, 40.6, 10.0, (200, 150)), U36)
    add("utm37_to_utm36_lat80", U37, _px_around(U37, 36.0, 80.0, 20.0, (130, 200)), U36)
    add("utm36_north_to_south_equator", U36, ((618000.0, 1000.0, 10.0, 10.0), (200, 200)), U36S)
    add("utm60_to_utm1_across_180", U60, _px_around(U60, 180.0, -35.0, 30.0, (129, 200)), U1)
    add("wm_to_utm36", WM, _wm_tile_corner(34.0, 40.0, 13, 256, (192, 192)), U36)
    add("utm36_to_wm", U36, _px_around(U36, 34.0, 40.0, 10.0, (150, 200)), WM)
    add("geographic_to_utm36", G, ((34.5, 40.3125, DEG, DEG), (200, 200)), U36)
    add("utm21s_to_geographic", U21S, _px_around(U21S, -56.2, -23.4, 10.0, (200, 160)), G)
    add("custom_tm_to_utm32", CUSTOM, _px_around(CUSTOM, 10.7, 52.1, 15.0, (160, 200)), U32)
    add("utm36_same_system", U36, ((512345.25, 4489012.5, 10.0, 10.0), (200, 200)), U36)
    add("utm36_to_utm37_thin", U36, _px_around(U36, 36.0, 40.6, 20.0, (3, 200)), U37)
    add("utm36_to_utm37_partly_outside", U36, _px_around(U36, 35.9, -12.3, 30.0, (150, 150)), U37)
    return out


def pick_sample(name, shape, n=PICK_POINTS):
    """The sampled pixels of a pick case, (n, 2) int64 (row, col) in row-major order: every crossing of the rows and the columns 0, 63, 64,
    127, 128 and the last that the grid has (the four corners among them), eight seeded pixels on each of those rows and columns, and a
    seeded scatter up to ``n`` pixels in all."""
    import zlib

    H, W = shape
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    rows = sorted({r for r in SEAM_LINES + (H - 1,) if r < H})
    cols = sorted({c for c in SEAM_LINES + (W - 1,) if c < W})
    pts = {(r, c) for r in rows for c in cols}
    for r in rows:
        pts |= {(r, int(c)) for c in rng.choice(W, min(8, W), replace=False)}
    for c in cols:
        pts |= {(int(r), c) for r in rng.choice(H, min(8, H), replace=False)}
    while len(pts) < min(n, H * W):
        pts.add((int(rng.integers(H)), int(rng.integers(W))))
    return np.array(sorted(pts), dtype=np.int64)


def _pick_point(args):
    """One destination pixel centre (float64 x, y) -> the true float64 (x', y') of the source system."""
    dst_crs, src_crs, x, y = args
    if tuple(dst_crs) == tuple(src_crs):
        return x, y  # the header's affine shortcut: the centre itself, no projection (the grid arithmetic is the reference module's)
    with mp.workdps(DPS):
        ll = to_lonlat(dst_crs, x, y)
        xy = None if ll is None else from_lonlat(src_crs, *ll)
        if xy is None:
            raise ValueError(f"the centre ({x}, {y}) lies outside the domain: a pick case stays in the core")
        if int(src_crs[0]) == 1 and not abs(wrap180(ll[0] - mpf(src_crs[1]))) < 40:
            raise ValueError(f"the centre ({x}, {y}) lies in the outer band of the source: a pick case stays in the core")
        return _f64(xy[0]), _f64(xy[1])


def _exact_centres(grid, rc):
    """The pixel centres X0 + (c + 1/2) sx, Y0 - (r + 1/2) sy of the float64 grid in rational arithmetic, rounded once."""
    from fractions import Fraction as Fr

    X0, Y0, sx, sy = (Fr(float(v)) for v in grid)
    return [(float(X0 + (int(c) + Fr(1, 2)) * sx), float(Y0 - (int(r) + Fr(1, 2)) * sy)) for r, c in rc]


def generate_picks(path=PICK_FIXTURE):
    """Write the pick fixture: the table of the cases and per case ``<name>/rc`` (n, 2) int16 and ``<name>/xy`` (n, 2) float64.  Asserts,
    case by case, that at most 1 % of the sample lies in the tie zone of the source grids that tests/warp_pick_reference.py lays under it."""
    import multiprocessing

    import warp_pick_reference as PR

    table = pick_lattices()
    data = {
        "names": np.array(list(table)),
        "dst_crs": np.array([t[0] for t in table.values()], dtype=np.float64),
        "dst_grid": np.array([t[1] for t in table.values()], dtype=np.float64),
        "shape": np.array([t[2] for t in table.values()], dtype=np.int64),
        "src_crs": np.array([t[3] for t in table.values()], dtype=np.float64),
    }
    with multiprocessing.Pool(min(16, os.cpu_count() or 1)) as pool:
        for name, (dst_crs, grid, shape, src_crs) in table.items():
            rc = pick_sample(name, shape)
            xy = np.array(pool.map(_pick_point, [(dst_crs, src_crs, x, y) for x, y in _exact_centres(grid, rc)], chunksize=4), dtype=np.float64)
            assert np.isfinite(xy).all()
            data[f"{name}/rc"], data[f"{name}/xy"] = rc.astype(np.int16), xy
            case = dict(name=name, dst_crs=dst_crs, dst_grid=grid, shape=shape, src_crs=src_crs, rc=rc, xy=xy)
            ties = [int(PR.picks(case, s)["tie"].sum()) for s in [PR.single(case)] + PR.pair(case) + PR.s2_classes(case)]
            print(f"{name}: {shape[0]} x {shape[1]}, {len(rc)} points, in the tie zone of each source grid: {ties}", flush=True)
            assert max(ties) <= 0.01 * len(rc), f"{name}: more than 1 % of the sample lies in a tie zone"
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **data)
    return path


def load_picks(path=PICK_FIXTURE):
    """The pick fixture as a dict name -> dict(name, dst_crs, dst_grid, shape, src_crs, rc (n, 2) int64, xy (n, 2) float64).  numpy only."""
    z = np.load(path)
    out = {}
    for i, name in enumerate(z["names"]):
        name = str(name)
        out[name] = dict(name=name, dst_crs=tuple(z["dst_crs"][i]), dst_grid=tuple(z["dst_grid"][i]), shape=tuple(int(v) for v in z["shape"][i]),
                         src_crs=tuple(z["src_crs"][i]), rc=z[f"{name}/rc"].astype(np.int64), xy=z[f"{name}/xy"])
    return out


if __name__ == "__main__":
    import sys

    print(generate_picks() if sys.argv[1:] == ["picks"] else generate())
