"""Source rasters that say which of their pixels was read, under the 50-digit truth of tests/golden/warp_pick_truth.npz.

The fixture (tests/projection_truth.py, ``generate_picks``) holds, per case, a destination grid with 10 to 30 m pixels, a source system and
the true float64 map coordinates (x', y') of a sample of destination pixel centres in that source system.  This module lays source grids
(X0, Y0, sx, sy) of a few hundred pixels a side under those points, says which source pixel each point truly falls into, and builds
rasters whose values encode their own indices, so that ONE value read by a kernel names the pixel it was read from.  numpy only; neither
the product nor ``warp_reference`` is imported: the grid arithmetic below is written from the rule's words (pixel (r, c) covers
[X0 + c sx, X0 + (c + 1) sx) x (Y0 - (r + 1) sy, Y0 - r sy], north up), not from the header's text.

TRUE PICK, float64:  c = floor((x' - X0) / sx),  r = floor((Y0 - y') / sy);  inside where 0 <= c < w and 0 <= r < h.

TIE ZONE.  A point is left out of a pick comparison when its distance to a pixel boundary, in ground metres, is at most the project's own
coordinate bar (1e-6 m, ``CORE_BAR`` of tests/test_gpu_projection_truth.py) plus 4 ulp of the coordinate: there a kernel that is right to
its bar may fall on the other side.  A degree counts as 111320 m (times cos(latitude) along a parallel).  The share of such points is
about 2e-6 m / 10 m; ``generate_picks`` asserts that it is at most 1 % for every source grid of this module.

NEAREST.  float32 rasters hold r * w + c (exact below 2^24); 16-bit rasters hold c and r in two planes; int8 rasters hold c mod 127,
r mod 127 and (c div 127) + 8 (r div 127) in three planes (0 ... 126 each: never the fill -1).

BILINEAR (float32).  The raster holds the affine field a c + b r + k with small integers, every pixel exact.  Bilinear interpolation of
an affine field is the field itself at the point: with pixel centres at c + 1/2 the true value is a (u - 1/2) + b (v - 1/2) + k wherever
all four neighbours lie inside the source.  BAR, all derived: the coordinate bar through the field's slope, (|a| / sx + |b| / sy) * 1e-6;
one float32 half-ulp of the value (the kernel rounds its float64 result once); and the float64 rounding of u, v and of the weighted sum,
2^-49 (|a| (|x'| + |X0|) / sx + |b| (|y'| + |Y0|) / sy + |value|) (a few ulp of each term).  No tie zone: the field is continuous.
"""
import numpy as np

CORE_BAR = 1e-6  # metres: the bar of ig_warp_coords against the same truth
METRES_PER_DEGREE = 111320.0
DEG = 2.0**-13

# the pixel sizes of the source grids, per case: (sx, sy) in the source's unit; not square wherever a swap of the two could hide
SRC_PIXELS = {
    "utm37_to_utm36_lat40p6": (10.0, 12.5),
    "utm37_to_utm36_lat80": (20.0, 20.0),
    "utm36_north_to_south_equator": (12.5, 10.0),
    "utm60_to_utm1_across_180": (30.0, 25.0),
    "wm_to_utm36": (10.0, 15.0),
    "utm36_to_wm": (12.5, 15.0),
    "geographic_to_utm36": (10.0, 10.0),
    "utm21s_to_geographic": (DEG, DEG * 0.75),
    "custom_tm_to_utm32": (15.0, 10.0),
    "utm36_same_system": (15.0, 12.5),
    "utm36_to_utm37_thin": (20.0, 25.0),
    "utm36_to_utm37_partly_outside": (30.0, 20.0),
}
CROPPED = ("utm36_to_utm37_partly_outside",)  # the single source covers only a part of the sample
# the cases under the Sentinel-2 classes: destinations of at most 3 km a side, so that a 10 m grid under them stays below 500 pixels
S2_CASES = ("utm37_to_utm36_lat40p6", "utm36_north_to_south_equator", "wm_to_utm36", "geographic_to_utm36", "custom_tm_to_utm32",
            "utm36_same_system")


class Source:
    """A north-up source grid with its size."""

    def __init__(self, grid, size):
        self.grid, self.size = tuple(float(v) for v in grid), (int(size[0]), int(size[1]))

    def __repr__(self):
        return f"Source(grid={self.grid}, size={self.size})"


def _cover(xy, sx, sy, lo=(0.0, 0.0), hi=(1.0, 1.0), shift=(0.25, 0.375)):
    """The grid of pixels (sx, sy) over the fractions lo ... hi of the points' extent (x eastward, y southward), 2 pixels of margin where
    the fraction is 0 or 1, its corner ``shift`` of a pixel off the lattice of multiples of the pixel size."""
    x0, x1, y0, y1 = xy[:, 0].min(), xy[:, 0].max(), xy[:, 1].min(), xy[:, 1].max()
    west, east = x0 + lo[0] * (x1 - x0), x0 + hi[0] * (x1 - x0)
    north, south = y1 - lo[1] * (y1 - y0), y1 - hi[1] * (y1 - y0)
    X0 = (np.floor(west / sx) - (2 if lo[0] == 0 else 0) + shift[0]) * sx
    Y0 = (np.ceil(north / sy) + (2 if lo[1] == 0 else 0) - shift[1]) * sy
    w = int(np.ceil((east - X0) / sx)) + (2 if hi[0] == 1 else 0)
    h = int(np.ceil((Y0 - south) / sy)) + (2 if hi[1] == 1 else 0)
    return Source((X0, Y0, sx, sy), (max(h, 1), max(w, 1)))


def single(case):
    """The one source of a case: the whole extent of the sample, or (``CROPPED``) its western 70 % below the northern 20 %."""
    sx, sy = SRC_PIXELS[case["name"]]
    if case["name"] in CROPPED:
        return _cover(case["xy"], sx, sy, lo=(0.0, 0.2), hi=(0.7, 1.0))
    return _cover(case["xy"], sx, sy)


def pair(case):
    """Two sources of the case's source system, laid so that both cover some samples: the western 65 % and the eastern 65 %, the second
    with transposed pixel sizes and another corner."""
    sx, sy = SRC_PIXELS[case["name"]]
    return [_cover(case["xy"], sx, sy, hi=(0.65, 1.0)), _cover(case["xy"], sy, sx, lo=(0.35, 0.0), shift=(0.625, 0.125))]


def s2_classes(case):
    """The two geometry classes of the Sentinel-2 test: a 10 m and a 20 m grid with different corners (``S2_CASES`` only)."""
    if case["name"] not in S2_CASES:
        return []
    return [_cover(case["xy"], 10.0, 10.0), _cover(case["xy"], 20.0, 20.0, shift=(0.4, 0.7))]


def uv(case, src):
    """float64 (u, v) of the sample in the pixel coordinates of ``src``."""
    X0, Y0, sx, sy = src.grid
    return (case["xy"][:, 0] - X0) / sx, (Y0 - case["xy"][:, 1]) / sy


def picks(case, src):
    """-> dict(r, c int64, inside bool, tie bool) of the sample in ``src``."""
    X0, Y0, sx, sy = src.grid
    h, w = src.size
    x, y = case["xy"][:, 0], case["xy"][:, 1]
    u, v = uv(case, src)
    c, r = np.floor(u), np.floor(v)
    mx = my = 1.0
    if case["src_crs"][0] == 0.0:  # degrees
        mx, my = METRES_PER_DEGREE * np.cos(np.radians(y)), METRES_PER_DEGREE
    dx = np.minimum(u - c, c + 1.0 - u) * sx * mx
    dy = np.minimum(v - r, r + 1.0 - v) * sy * my
    tie = (dx <= CORE_BAR + 4.0 * np.spacing(np.abs(x)) * mx) | (dy <= CORE_BAR + 4.0 * np.spacing(np.abs(y)) * my)
    c, r = c.astype(np.int64), r.astype(np.int64)
    return dict(r=r, c=c, inside=(c >= 0) & (c < w) & (r >= 0) & (r < h), tie=tie)


def winners(case, srcs, rule):
    """The true composition of opaque sources by ``rule`` (last | first) -> dict(sid int64 (255: none), r, c of the winner's pick, tie bool:
    the point lies in the tie zone of some source)."""
    n = len(case["xy"])
    sid, r, c, tie = np.full(n, 255, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool)
    order = range(len(srcs)) if rule == "last" else reversed(range(len(srcs)))  # the winner is written last
    for i in order:
        p = picks(case, srcs[i])
        tie |= p["tie"]
        sid[p["inside"]], r[p["inside"]], c[p["inside"]] = i, p["r"][p["inside"]], p["c"][p["inside"]]
    return dict(sid=sid, r=r, c=c, tie=tie)


# ---- rasters that encode their own indices ------------------------------------------------------------------------------------------------
def index_raster(src):
    """float32 (h, w): r * w + c."""
    h, w = src.size
    assert h * w < 2**24
    return np.arange(h * w, dtype=np.float32).reshape(h, w)


def rc_planes(src, dtype):
    """(2, h, w) of a 16-bit ``dtype``: the column index, the row index."""
    h, w = src.size
    assert max(h, w) < 2**15
    r, c = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return np.stack([c, r]).astype(dtype)


def mod_planes(src, dtype=np.int8):
    """(3, h, w): c mod 127, r mod 127, (c div 127) + 8 (r div 127)."""
    h, w = src.size
    assert w < 8 * 127 and h < 16 * 127
    r, c = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return np.stack([c % 127, r % 127, c // 127 + 8 * (r // 127)]).astype(dtype)


def decode_mod(cm, rm, q):
    """-> (r, c) of the three values of :func:`mod_planes`."""
    cm, rm, q = (np.asarray(a).astype(np.int64) for a in (cm, rm, q))
    return rm + 127 * (q // 8), cm + 127 * (q % 8)


def affine_raster(src, a, b, k):
    """float32 (h, w): a c + b r + k, exact."""
    h, w = src.size
    r, c = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    f = a * c + b * r + k
    assert np.abs(f).max() < 2**24
    return f.astype(np.float32)


def bilinear_truth(case, src, a, b, k):
    """-> dict(value float64, bar float64, full bool: all four neighbours inside; out bool: no neighbour can count) of the field of
    :func:`affine_raster` under bilinear resampling.  A point that is neither ``full`` nor ``out`` lies in the clipped border."""
    X0, Y0, sx, sy = src.grid
    h, w = src.size
    u, v = uv(case, src)
    value = a * (u - 0.5) + b * (v - 0.5) + k
    mx = my = 1.0
    if case["src_crs"][0] == 0.0:
        mx, my = METRES_PER_DEGREE * np.cos(np.radians(case["xy"][:, 1])), METRES_PER_DEGREE
    slope = abs(a) / (sx * mx) + abs(b) / (sy * my)  # field units per ground metre
    half_ulp = 0.5 * np.spacing(np.abs(value).astype(np.float32)).astype(np.float64)
    rounding = 2.0**-49 * (abs(a) * (np.abs(case["xy"][:, 0]) + abs(X0)) / sx + abs(b) * (np.abs(case["xy"][:, 1]) + abs(Y0)) / sy + np.abs(value))
    eu, ev = 2.0 * CORE_BAR / (sx * mx), 2.0 * CORE_BAR / (sy * my)  # the classification keeps twice the bar off its own edges
    full = (u - 0.5 >= eu) & (u - 0.5 <= w - 1 - eu) & (v - 0.5 >= ev) & (v - 0.5 <= h - 1 - ev)
    out = (u < -0.5 - eu) | (u > w + 0.5 + eu) | (v < -0.5 - ev) | (v > h + 0.5 + ev)
    return dict(value=value, bar=slope * CORE_BAR + half_ulp + rounding, full=full, out=out)


# ---- destinations cut into chips ------------------------------------------------------------------------------------------------------------
def chip_grids(case, S):
    """The case's destination cut into S x S chips, row-major -> (grids (n, 4) float64, chips per row)."""
    X0, Y0, sx, sy = case["dst_grid"]
    H, W = case["shape"]
    ny, nx = -(-H // S), -(-W // S)
    return np.array([(X0 + j * S * sx, Y0 - i * S * sy, sx, sy) for i in range(ny) for j in range(nx)], dtype=np.float64), nx


def at_samples(chips, case, S, nx):
    """``chips`` (n, ..., S, S) -> (..., points): the values at the case's sampled pixels."""
    r, c = case["rc"][:, 0], case["rc"][:, 1]
    got = chips[(r // S) * nx + c // S, ..., r % S, c % S]
    return np.moveaxis(got, 0, -1)
