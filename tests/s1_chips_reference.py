"""A sequential twin of the Sentinel-1 chip cut (include/instageo_hip.h) for the tests, and the cases both test files
share.  It does not import the product: the projections are those of tests/raster_chips_reference.py (tests/warp_reference.py, the
independent float64 twin); the walk over the slices, presence, clip, validity and tallies are plain loops over pixels and values, on the
32-bit patterns.

TIES.  The device and this twin may differ by ~1e-10 px in (u, v), so a pixel whose u or v lies within 1e-6 of an integer for ANY scene
could pick another source pixel.  ``cut`` counts those pixels (``near``); every case below chooses its grids (scenes on the stack's 10 m
lattice see every centre at .5; the scenes of other zones have sub-pixel corners) so that the count is zero, the tests assert that from
the twin alone, and every comparison is then exact."""
import functools

import numpy as np

import raster_chips_reference as RR

WR = RR.WR
U36, U37, U36S, U37S = RR.U36, RR.U37, RR.U36S, WR.utm(37, south=True)
PX = 10.0
SH, SW = 150, 171  # a scene: the row pitch is odd
SRC_NODATA = np.float32(-32768.0)


def f32(v):
    return None if v is None else np.float32(v)


def cut(planes, starts, scenes, date_scenes, dst_crs, dst_grid, origins, S, nd=-1.0, snd=None, clip=None):
    """``scenes``: [(crs, grid, (H, W))] date after date, ``date_scenes``: the number of scenes per date -> (chips float32, valid_values,
    validity, near): pixel by pixel and value by value.  ``near``: the pixels with u or v within 1e-6 of an integer for some scene."""
    N, T = len(scenes), len(date_scenes)
    C = len(starts) // N
    nd, snd = f32(nd), f32(snd)
    bits = planes.view(np.uint32)
    n = len(origins)
    chips = np.zeros((n, T * C, S, S), dtype=np.uint32)
    validity = np.zeros((n, S, S), dtype=np.uint8)
    valid_values = np.zeros(n, dtype=np.int32)
    first = np.concatenate([[0], np.cumsum(date_scenes)]).tolist()
    near = 0
    X0, Y0, sx, sy = dst_grid
    for i, (r0, c0) in enumerate(origins):
        uv = []
        if RR.grid_ok(np.asarray(dst_grid, dtype=np.float64)):
            x, y = np.meshgrid(X0 + (float(c0) + np.arange(S) + 0.5) * sx, Y0 - (float(r0) + np.arange(S) + 0.5) * sy)
            lonlat = None
            for crs, g, _ in scenes:
                xs, ys = x, y
                if tuple(crs) != tuple(dst_crs):
                    if lonlat is None:
                        lonlat = WR.to_lonlat(tuple(dst_crs), x, y)
                    xs, ys = WR.from_lonlat(tuple(crs), *lonlat)
                u, v = (xs - g[0]) / g[2], (g[1] - ys) / g[3]
                bad = np.isnan(u) | np.isnan(v)
                u, v = np.where(bad, np.nan, u), np.where(bad, np.nan, v)
                with np.errstate(invalid="ignore"):
                    near += int(((np.abs(u - np.round(u)) < 1e-6) | (np.abs(v - np.round(v)) < 1e-6)).sum())
                uv.append((u, v))
        else:
            uv = [(np.full((S, S), np.nan),) * 2] * N
        for r in range(S):
            for c in range(S):
                differ = 0
                for t in range(T):
                    where = []  # the source offset of the pixel in each scene of the date, None outside
                    for s in range(first[t], first[t + 1]):
                        uu, vv = uv[s][0][r, c], uv[s][1][r, c]
                        h, w = scenes[s][2]
                        at = None
                        if uu == uu and vv == vv:
                            cs, rs = int(np.floor(uu)), int(np.floor(vv))
                            if 0 <= rs < h and 0 <= cs < w:
                                at = rs * w + cs
                        where.append(at)
                    for b in range(C):
                        out, value = nd.view(np.uint32), nd
                        for k, s in enumerate(range(first[t], first[t + 1])):
                            if where[k] is None:
                                continue
                            word = bits[int(starts[s * C + b]) + where[k]]
                            x = word.view(np.float32)
                            if x != x or (snd is not None and x == snd):
                                continue
                            if clip is not None:
                                if x < f32(clip[0]):
                                    x = f32(clip[0])
                                if x > f32(clip[1]):
                                    x = f32(clip[1])
                                word = x.view(np.uint32)
                            out, value = word, x
                            break
                        chips[i, t * C + b, r, c] = out
                        differ += bool(value != nd)
                valid_values[i] += differ
                validity[i, r, c] = (1 if differ == T * C else 0) | (2 if differ > 0 else 0)
    return chips.view(np.float32), valid_values, validity, near


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------
X0, Y0 = (PX * round(float(v) / PX) for v in WR.from_lonlat(U36, 35.6, 40.6))  # the stack lattice, close to the edge of zone 36
STACK = (X0, Y0, PX, PX)
X0S, Y0S = (PX * round(float(v) / PX) for v in WR.from_lonlat(U36S, 35.6, -40.6))
SPECIAL = np.array([0x7FC00000, 0xFFC00001, 0xC7000000, 0xBF800000, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000],
                   dtype=np.uint32)  # NaN, NaN, -32768 (src_nodata), -1 (no_data), -0.0, two denormals, +inf, -inf


def plane(seed, holes=()):
    """One SH x SW plane: backscatter-like values with the SPECIAL patterns sprinkled in and rectangular ``holes`` (r0, r1, c0, c1, word)."""
    rng = np.random.default_rng(seed)
    a = rng.gamma(2.0, 0.05, size=(SH, SW)).astype(np.float32).view(np.uint32)
    pick = rng.random((SH, SW)) < 0.12
    a[pick] = SPECIAL[rng.integers(0, len(SPECIAL), size=int(pick.sum()))]
    for r0, r1, c0, c1, word in holes:
        a[r0:r1, c0:c1] = word
    return a.view(np.float32)


def at(row, col, system=U36, x0=X0, y0=Y0, dx=0.0, dy=0.0):
    """The scene of SH x SW 10 m pixels whose corner lies at (row, col) of the stack lattice, in ``system``, moved by (dx, dy) metres."""
    x, y = x0 + PX * col, y0 - PX * row
    if system not in (U36, U36S):
        x, y = (float(v) for v in WR.from_lonlat(system, *WR.to_lonlat(U36 if y0 == Y0 else U36S, x, y)))
    return (system, (x + dx, y + dy, PX, PX), (SH, SW))


def pack(planes_per_scene):
    """[[plane per band] per scene] -> (buffer that starts 4 bytes past a 16-byte boundary when uploaded whole, starts)."""
    flat = [p.reshape(-1) for s in planes_per_scene for p in s]
    starts = np.concatenate([[0], np.cumsum([p.size for p in flat])[:-1]]).astype(np.int64)
    return np.concatenate(flat), starts


def origins_of(S):
    """Inside, over the top-left and the bottom-right edge of the first scene (at row -10, column -12), negative and outside, far outside,
    over the top edge."""
    return [(5, 7), (-10 - S // 2, -12 - S // 2), (-10 + SH - S // 2, -12 + SW - S // 2), (-S - 3, 20), (3000, 3000), (-17, 100)]


CORNERS = [(-10, -12), (25, 30), (60, -40)]  # three dates, three corners on the stack lattice


def _values(S, T, C):
    scenes = [at(*CORNERS[t]) for t in range(T)]
    planes, starts = pack([[plane(100 * t + b) for b in range(C)] for t in range(T)])
    return dict(planes=planes, starts=starts, scenes=scenes, date_scenes=[1] * T, dst_crs=U36, dst_grid=STACK, origins=origins_of(S), S=S,
                nd=-1.0, snd=SRC_NODATA, clip=None)


def _slices(swap):
    """Date 0: two slices that overlap in rows 100..149 of the first; holes of NaN / src_nodata in each, different per band.  Date 1: one
    scene."""
    nan, snd = SPECIAL[0], SPECIAL[2]
    a = [plane(1, [(110, 130, 20, 60, nan)]), plane(2, [(105, 140, 80, 120, snd)])]
    b = [plane(3, [(5, 25, 30, 50, nan)]), plane(4, [(0, 40, 90, 110, snd)])]
    one = [plane(5), plane(6)]
    first, second = (at(-10, -12), a), (at(90, -12), b)
    if swap:
        first, second = second, first
    planes, starts = pack([first[1], second[1], one])
    S = 64
    origins = [(70, 0), (100, 60), (40, 110), (230, 20), (-30, -30)]
    return dict(planes=planes, starts=starts, scenes=[first[0], second[0], at(25, 30)], date_scenes=[2, 1], dst_crs=U36, dst_grid=STACK,
                origins=origins, S=S, nd=-1.0, snd=SRC_NODATA, clip=None)


def _next_zone():
    scenes = [at(-10, -12), at(25, 30, U37, dx=3.3, dy=-4.1), at(60, -40)]
    planes, starts = pack([[plane(200 + 10 * t + b) for b in range(2)] for t in range(3)])
    return dict(planes=planes, starts=starts, scenes=scenes, date_scenes=[1, 1, 1], dst_crs=U36, dst_grid=STACK,
                origins=[(5, 7), (40, 60), (150, 180), (3000, 3000)], S=64, nd=-1.0, snd=None, clip=None)


def _south():
    scenes = [at(-10, -12, U36S, X0S, Y0S), at(25, 30, U37S, X0S, Y0S, dx=2.7, dy=3.9), at(40, 20, U36S, X0S, Y0S)]
    planes, starts = pack([[plane(300 + 10 * t + b) for b in range(2)] for t in range(3)])
    return dict(planes=planes, starts=starts, scenes=scenes, date_scenes=[1, 2], dst_crs=U36S, dst_grid=(X0S, Y0S, PX, PX),
                origins=[(5, 7), (100, 120), (-20, -20)], S=32, nd=-1.0, snd=SRC_NODATA, clip=None)


def _clip():
    k = _values(8, 3, 2)
    return dict(k, clip=(0.0, 0.125), nd=0.0)  # a present -1 or -0.0 clips to the fill's value and counts as no-data


BUILDERS = {f"values_s{S}_t{T}c{C}": functools.partial(_values, S, T, C) for S in (8, 64, 80) for T, C in ((1, 1), (3, 2))}
BUILDERS.update({"slices": functools.partial(_slices, False), "slices_swapped": functools.partial(_slices, True), "next_zone": _next_zone,
                 "south": _south, "clip_s8": _clip})
CASES = sorted(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def twin(name):
    """The twin's outputs for one case, computed once per session and never changed."""
    k = case(name)
    out = cut(k["planes"], k["starts"], k["scenes"], k["date_scenes"], k["dst_crs"], k["dst_grid"], k["origins"], k["S"], k["nd"], k["snd"],
              k["clip"])
    for a in out[:3]:
        a.setflags(write=False)
    return out


def product_args(k):
    """The arguments of ``s1_chips.cut`` after the planes for a case."""
    return dict(starts=k["starts"], scene_crs=[s[0] for s in k["scenes"]], scene_grid=[s[1] for s in k["scenes"]],
                scene_size=[s[2] for s in k["scenes"]], date_scenes=k["date_scenes"], dst_crs=k["dst_crs"], dst_grid=k["dst_grid"],
                origins=k["origins"], chip_size=k["S"], no_data_value=k["nd"], src_nodata=None if k["snd"] is None else float(k["snd"]),
                clip=k["clip"])


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(f"u{got.itemsize}"), want.view(f"u{want.itemsize}"))
