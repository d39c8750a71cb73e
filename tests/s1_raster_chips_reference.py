"""A sequential twin of the warped Sentinel-1 chip cut (include/instageo_hip.h) for the tests, and the cases both test
files share.  It does not import the product and was written from the header's text: the projections are those of
tests/warp_reference.py (the independent float64 twin); the pixel centres, the walk over the slices, presence, clip, validity, labels and
tallies are plain loops over pixels and values, on the 32-bit patterns.  From tests/s1_chips_reference.py it takes the scene builders
(planes, corners, packing) and nothing of its chip loop.

TIES.  The device and this twin may differ by ~1e-10 px in (u, v), so a pixel whose u or v lies within 1e-6 of an integer for ANY scene
could pick another source pixel.  ``warp_cut`` counts those pixels (``ties``); every case below moves its grids by a fraction of a pixel
so that the count is zero, the tests assert that from the twin alone, and every comparison is then exact."""
import functools

import numpy as np

import raster_chips_reference as RR
import s1_chips_reference as VR

WR = VR.WR
U36, U37, U36S, U37S = VR.U36, VR.U37, VR.U36S, VR.U37S
GEO, MERC = WR.GEOGRAPHIC, WR.WEB_MERCATOR
PX, SH, SW = VR.PX, VR.SH, VR.SW


def f32(v):
    return None if v is None else np.float32(v)


def grid_ok(g):
    g = np.asarray(g, dtype=np.float64)
    return bool(np.isfinite(g).all() and g[2] > 0 and g[3] > 0)


def warp_cut(planes, starts, scenes, date_scenes, dst_crs, dst_grids, S, nd=-1.0, snd=None, clip=None, labels=None, bit=0, K=0):
    """``scenes``: [(crs, grid, (H, W))] date after date, ``date_scenes``: the number of scenes per date, ``dst_grids``: one (X0, Y0, sx,
    sy) per chip -> (chips float32, valid_values, validity, maps, valid_labels, hist, ties): pixel by pixel and value by value.  ``ties``:
    the pixels with u or v within 1e-6 of an integer for some scene."""
    N, T = len(scenes), len(date_scenes)
    C = len(starts) // N
    nd, snd = f32(nd), f32(snd)
    words = planes.view(np.uint32)
    n = len(dst_grids)
    chips = np.zeros((n, T * C, S, S), dtype=np.uint32)
    validity = np.zeros((n, S, S), dtype=np.uint8)
    valid_values = np.zeros(n, dtype=np.int32)
    maps = valid_labels = hist = None
    if labels is not None:
        maps, valid_labels = np.zeros_like(labels), np.zeros(n, dtype=np.int32)
        hist = np.zeros((n, K), dtype=np.int32) if K else None
    first = np.concatenate([[0], np.cumsum(date_scenes)]).tolist()
    ties = 0
    for i, g in enumerate(dst_grids):
        # (u, v) of every pixel centre in every scene; NaN: none
        uv = [(np.full((S, S), np.nan),) * 2] * N
        if grid_ok(g):
            gx0, gy0, gsx, gsy = (float(t) for t in g)
            x, y = np.meshgrid(gx0 + (np.arange(S) + 0.5) * gsx, gy0 - (np.arange(S) + 0.5) * gsy)
            lonlat = None  # the inverse projection of dst_crs, once per pixel
            uv = []
            for crs, sg, _ in scenes:
                xs, ys = x, y
                if tuple(crs) != tuple(dst_crs):
                    if lonlat is None:
                        lonlat = WR.to_lonlat(tuple(dst_crs), x, y)
                    xs, ys = WR.from_lonlat(tuple(crs), *lonlat)
                u, v = (xs - sg[0]) / sg[2], (sg[1] - ys) / sg[3]
                bad = np.isnan(u) | np.isnan(v)
                u, v = np.where(bad, np.nan, u), np.where(bad, np.nan, v)
                with np.errstate(invalid="ignore"):
                    ties += int(((np.abs(u - np.round(u)) < 1e-6) | (np.abs(v - np.round(v)) < 1e-6)).sum())
                uv.append((u, v))
        for r in range(S):
            for c in range(S):
                differ = 0
                for t in range(T):
                    for b in range(C):
                        word, value = nd.view(np.uint32), nd
                        for s in range(first[t], first[t + 1]):  # the first scene the pixel lies inside and whose value is present
                            uu, vv = uv[s][0][r, c], uv[s][1][r, c]
                            if uu != uu or vv != vv:
                                continue
                            cs, rs = int(np.floor(uu)), int(np.floor(vv))
                            h, w = scenes[s][2]
                            if not (0 <= rs < h and 0 <= cs < w) or starts[s * C + b] < 0:
                                continue
                            found = words[int(starts[s * C + b]) + rs * w + cs]
                            x_ = found.view(np.float32)
                            if x_ != x_ or (snd is not None and x_ == snd):
                                continue
                            if clip is not None:
                                if x_ < f32(clip[0]):
                                    x_ = f32(clip[0])
                                if x_ > f32(clip[1]):
                                    x_ = f32(clip[1])
                                found = x_.view(np.uint32)
                            word, value = found, x_
                            break
                        chips[i, t * C + b, r, c] = word
                        differ += bool(value != nd)
                valid_values[i] += differ
                validity[i, r, c] = (1 if differ == T * C else 0) | (2 if differ > 0 else 0)
                if labels is not None:
                    lab = labels[i, r, c]
                    if (bit and not (validity[i, r, c] & bit)) or lab != lab:
                        lab = labels.dtype.type(-1)
                    maps[i, r, c] = lab
                    if lab != -1:
                        valid_labels[i] += 1
                        if K and 0 <= int(lab) < K:
                            hist[i, int(lab)] += 1
    return chips.view(np.float32), valid_values, validity, maps, valid_labels, hist, ties


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------
# The first scene of every northern stack has its corner at row -10, column -12 of the lattice (VR.X0, VR.Y0): these are map points of it
# in UTM 36 (x, y), the places the chips are centred on.
def point(row, col, x0=VR.X0, y0=VR.Y0):
    return (x0 + PX * (col - 12), y0 - PX * (row - 10))


INSIDE, TOP_LEFT, BOTTOM_RIGHT, TOP, FAR = point(70, 90), point(0, 0), point(SH, SW), point(0, 100), point(5000, 5000)
NAN_GRID, FLAT_GRID = (float("nan"), 4.5e6, 10.0, 10.0), (5.0e5, 4.5e6, 0.0, 10.0)


def centred(dst, pt, S, px, base=U36):
    """The grid of S x S pixels of size ``px`` (in the units of ``dst``) centred on the map point ``pt`` of ``base``, moved by a fraction of
    a pixel."""
    x, y = pt
    if tuple(dst) != tuple(base):
        x, y = (float(v) for v in WR.from_lonlat(dst, *WR.to_lonlat(base, x, y)))
    return (x - px * (S / 2 - 0.137), y + px * (S / 2 + 0.221), px, px)


def labels_of(n, S, kind, seed):
    return None if kind is None else RR.label_maps(n, S, np.int8 if kind == "int8" else np.float32, seed)


def _affine(S, T, C, kind, bit, K):
    """Label grids in the scenes' UTM zone (the affine path) with another origin and a finer and a coarser pixel than the scenes': inside,
    over the top-left and the bottom-right corner, over the top edge, far outside, and one grid that is not finite."""
    k = VR._values(S, T, C)
    grids = [centred(U36, INSIDE, S, 7.3), centred(U36, TOP_LEFT, S, 13.7), centred(U36, BOTTOM_RIGHT, S, 10.0), NAN_GRID,
             centred(U36, FAR, S, 10.0), centred(U36, TOP, S, 4.1)]
    return dict(planes=k["planes"], starts=k["starts"], scenes=k["scenes"], date_scenes=k["date_scenes"], dst_crs=U36, dst_grids=grids, S=S,
                nd=-1.0, snd=VR.SRC_NODATA, clip=None, labels=labels_of(len(grids), S, kind, 7 * S + T), bit=bit, K=K)


def _projected(dst, S, px, kind, bit, K):
    """Label grids in EPSG:4326 / 3857: the projection path for every scene of three dates, a corner per date."""
    k = VR._values(S, 3, 2)
    grids = [centred(dst, INSIDE, S, px), centred(dst, TOP_LEFT, S, 1.9 * px), centred(dst, BOTTOM_RIGHT, S, 0.6 * px), FLAT_GRID,
             centred(dst, FAR, S, px)]
    return dict(planes=k["planes"], starts=k["starts"], scenes=k["scenes"], date_scenes=k["date_scenes"], dst_crs=dst, dst_grids=grids, S=S,
                nd=-1.0, snd=VR.SRC_NODATA, clip=None, labels=labels_of(len(grids), S, kind, 11 * S), bit=bit, K=K)


def _next_zone():
    """Label grids in UTM 37, the zone of the second date's scene (affine for it, projected for the two dates in zone 36)."""
    k = VR._next_zone()
    S = 64
    grids = [centred(U37, point(60, 100), S, 10.0), centred(U37, point(25 + 10, 30 + 12), S, 6.1), centred(U37, FAR, S, 10.0),
             centred(U37, point(150, 150), S, 17.3)]
    return dict(planes=k["planes"], starts=k["starts"], scenes=k["scenes"], date_scenes=k["date_scenes"], dst_crs=U37, dst_grids=grids, S=S,
                nd=-1.0, snd=None, clip=None, labels=labels_of(len(grids), S, "int8", 3), bit=2, K=8)


def _south():
    """A southern stack whose second date has scenes in two zones; label grids in EPSG:4326."""
    k = VR._south()
    S = 32
    pts = [point(60, 80, VR.X0S, VR.Y0S), point(0, 0, VR.X0S, VR.Y0S), point(120, 160, VR.X0S, VR.Y0S)]
    grids = [centred(GEO, p, S, r, U36S) for p, r in zip(pts, (0.00009, 0.00027, 0.00013))]
    return dict(planes=k["planes"], starts=k["starts"], scenes=k["scenes"], date_scenes=k["date_scenes"], dst_crs=GEO, dst_grids=grids, S=S,
                nd=-1.0, snd=VR.SRC_NODATA, clip=None, labels=labels_of(len(grids), S, "float32", 5), bit=1, K=0)


def _slices(swap):
    """Two overlapping slices on the first date, in either order, with holes that differ per band (vv and vh of one pixel come from
    different slices); label grids over the overlap, coarser and finer than the scenes."""
    k = VR._slices(swap)
    S = 64
    grids = [centred(U36, point(125, 85), S, 13.7), centred(U36, point(120, 60), S, 7.3), centred(U36, point(240, SW), S, 10.0),
             centred(U36, FAR, S, 10.0)]
    return dict(planes=k["planes"], starts=k["starts"], scenes=k["scenes"], date_scenes=k["date_scenes"], dst_crs=U36, dst_grids=grids, S=S,
                nd=-1.0, snd=VR.SRC_NODATA, clip=None, labels=labels_of(len(grids), S, "int8", 9), bit=2, K=8)


def _clip():
    k = _affine(8, 3, 2, "int8", 1, 8)
    return dict(k, clip=(0.0, 0.125), nd=0.0)  # a present -1 or -0.0 clips to the fill's value and counts as no-data


BUILDERS = {
    "affine_s8_t1c1": functools.partial(_affine, 8, 1, 1, None, 0, 0),
    "affine_s64_t1c1": functools.partial(_affine, 64, 1, 1, "int8", 1, 8),
    "affine_s80_t1c1": functools.partial(_affine, 80, 1, 1, "float32", 2, 0),
    "affine_s8_t3c2": functools.partial(_affine, 8, 3, 2, "int8", 0, 0),
    "affine_s64_t3c2": functools.partial(_affine, 64, 3, 2, "float32", 0, 0),
    "affine_s80_t3c2": functools.partial(_affine, 80, 3, 2, "int8", 2, 8),
    "geographic_s80": functools.partial(_projected, GEO, 80, 0.00009, "int8", 1, 8),
    "geographic_s8": functools.partial(_projected, GEO, 8, 0.0009, None, 0, 0),
    "web_mercator_s64": functools.partial(_projected, MERC, 64, 13.1, "float32", 1, 0),
    "next_zone": _next_zone,
    "south": _south,
    "slices": functools.partial(_slices, False),
    "slices_swapped": functools.partial(_slices, True),
    "clip_s8": _clip,
}
CASES = sorted(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def twin(name):
    """The twin's outputs for one case, computed once per session and never changed."""
    k = case(name)
    out = warp_cut(k["planes"], k["starts"], k["scenes"], k["date_scenes"], k["dst_crs"], k["dst_grids"], k["S"], k["nd"], k["snd"], k["clip"],
                   k["labels"], k["bit"], k["K"])
    for a in out[:6]:
        if a is not None:
            a.setflags(write=False)
    return out


STRATEGY = {0: None, 1: "any", 2: "each"}


def product_args(k):
    """The arguments of ``s1_raster_chips.warp_cut`` after the planes for a case."""
    return dict(starts=k["starts"], scene_crs=[s[0] for s in k["scenes"]], scene_grid=[s[1] for s in k["scenes"]],
                scene_size=[s[2] for s in k["scenes"]], date_scenes=k["date_scenes"], dst_crs=k["dst_crs"], dst_grids=k["dst_grids"],
                chip_size=k["S"], no_data_value=k["nd"], src_nodata=None if k["snd"] is None else float(k["snd"]), clip=k["clip"],
                labels=k["labels"], label_strategy=STRATEGY[k["bit"]], num_classes=k["K"])


def same_bits(got, want):
    if got is None or want is None:
        return got is None and want is None
    return VR.same_bits(got, want)
