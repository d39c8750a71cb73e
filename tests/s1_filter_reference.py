"""Sequential twin of the speckle-filter rule of include/instageo_hip.h (``ig_s1_speckle``), written pixel by pixel from the header's text
with Python floats (IEEE float64, every operation rounded on its own): independent of the vectorised host path of
instageo_amd/s1_filter.py.  ``sqrt`` and ``log10`` are numpy's, the functions the host path calls, so the two can be compared bit for bit
on one machine.  Also the packed test planes both suites share, and cached expectations."""
import functools
import math
import os

import numpy as np

QNAN = 0x7FC00000
METHODS = ("boxcar", "lee", "gamma_map")
SCALES = ("linear", "db")
LOOKS = 4.4
SND = -32768.0


def _present(f, snd):
    return math.isfinite(f) and (snd is None or np.float32(f) != np.float32(snd))


def window_sums(plane, H, W, h, snd):
    """-> per pixel (A, Q, n) of its clipped window, or None where the centre is absent.  A row moment depends on its row and the
    pixel's column only, so it is formed once per (row, column) and shared by the pixels whose windows hold it."""
    x = [[float(v) for v in row] for row in plane.reshape(H, W).tolist()]
    ok = [[_present(v, snd) for v in row] for row in x]
    rows = {}

    def row_moment(i, c):
        if (i, c) not in rows:
            A, Q, K = 0.0, 0.0, 0
            for j in range(max(c - h, 0), min(c + h, W - 1) + 1):  # left to right
                if ok[i][j]:
                    A += x[i][j]
                    Q += x[i][j] * x[i][j]
                    K += 1
            rows[(i, c)] = (A, Q, K)
        return rows[(i, c)]

    sums = []
    for r in range(H):
        for c in range(W):
            if not ok[r][c]:
                sums.append(None)
                continue
            A, Q, n = 0.0, 0.0, 0
            for i in range(max(r - h, 0), min(r + h, H - 1) + 1):  # top to bottom
                Ai, Qi, Ki = row_moment(i, c)
                A += Ai
                Q += Qi
                n += Ki
            sums.append((A, Q, n, x[r][c]))
    return sums


def value(A, Q, n, x, method, looks):
    lk = float(np.float32(looks))
    s = 1.0 / lk
    m = A / n
    v = Q / n - m * m
    if v < 0:
        v = 0.0
    if method == "boxcar":
        return m
    if method == "lee":
        t = (m * m) * s
        vx = (v - t) / (1.0 + s)
        b = vx / v if v > 0 and vx > 0 else 0.0
        return m + b * (x - m)
    if m <= 0:
        return m
    ci2 = v / (m * m)
    if ci2 <= s:
        return m
    if ci2 >= 2.0 * s:
        return x
    a = (1.0 + s) / (ci2 - s)
    B = a - lk - 1.0
    D = (m * m) * (B * B) + ((4.0 * a) * lk) * (m * x)
    if not D >= 0:
        return m
    return (B * m + float(np.sqrt(np.float64(D)))) / (2.0 * a)


def finish(sums, method, looks, to_db):
    """-> (the int32 bit views of the outputs, present, dropped) of one plane."""
    bits = np.full(len(sums), QNAN, dtype=np.uint32)
    present = dropped = 0
    for k, sm in enumerate(sums):
        if sm is None:
            continue
        y = value(*sm, method, looks)
        if to_db:
            if not y > 0:
                dropped += 1
                continue
            y = 10.0 * float(np.log10(np.float64(y)))
        with np.errstate(over="ignore"):
            bits[k] = np.array([y], dtype=np.float64).astype(np.float32).view(np.uint32)[0]
        present += 1
    return bits, present, dropped


def twin(planes, starts, sizes, h, method, looks, snd, to_db):
    """-> (out as uint32 bit views with the layout of planes, elements outside every plane 0; counts (N, 2) int32)."""
    out = np.zeros(planes.shape[0], dtype=np.uint32)
    counts = np.zeros((len(starts), 2), dtype=np.int32)
    for p, (at, (H, W)) in enumerate(zip(starts, sizes)):
        at = int(at)
        bits, counts[p, 0], counts[p, 1] = finish(window_sums(planes[at : at + H * W], H, W, h, snd), method, looks, to_db)
        out[at : at + H * W] = bits
    return out, counts


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
# name -> the (H, W) of its planes.  one / small: smaller than any window; narrow: narrower than a tile, an odd pitch; tiles / seams:
# several tiles of 64 x 32 both ways with ragged edges, so halos cross the seams (70 = the tile width + 6, and two tile heights + 6);
# three: planes of different sizes in one launch, every second one starting at an odd element; absent: nothing present at all.
CASES = {"one": [(1, 1)], "small": [(3, 2)], "narrow": [(5, 37)], "tiles": [(17, 129)], "seams": [(70, 70)],
         "three": [(7, 9), (33, 65), (5, 3)], "absent": [(6, 5)]}
# (h, src_nodata given) of the runs on the general values and on the strictly positive ones: every h, src_nodata given and not
RUNS = {False: ((1, True), (3, False), (7, True)), True: ((1, False), (3, True), (7, False))}


def _plane(rng, H, W, positive, absent):
    """Lognormal texture over six decades, constant on blocks of 8 x 8 so that a window's coefficient of variation lands on every branch
    of gamma_map, times gamma speckle of 4.4 looks; NaN islands, one whole absent row, an inf, src_nodata values; unless ``positive``
    also zeros and a few negatives."""
    base = 10.0 ** rng.uniform(-4.0, 2.0, size=((H + 7) // 8, (W + 7) // 8))
    a = (np.kron(base, np.ones((8, 8)))[:H, :W] * rng.gamma(LOOKS, 1.0 / LOOKS, size=(H, W))).astype(np.float32)
    if absent:
        a[:] = np.nan
        a[0, 0] = SND
        return a
    if H * W >= 6:
        a[rng.random((H, W)) < 0.04] = SND
        a[rng.random((H, W)) < 0.03] = np.nan
        if not positive:
            a[rng.random((H, W)) < 0.05] = 0.0
            a[rng.random((H, W)) < 0.02] *= -1.0
    if H >= 5:
        a[H // 2, :] = np.nan  # a whole absent row
        a[1 : 1 + min(4, H - 1), W // 3 : W // 3 + 5] = np.nan  # an island wider than the smallest window
        a[H - 1, W - 1] = np.inf
        a[0, W // 2] = -np.inf
    return a


@functools.lru_cache(maxsize=None)
def case(name, positive=False):
    """-> {planes (with one leading element, so a view from element 1 starts 4-byte but not 16-byte aligned), starts, sizes}."""
    rng = np.random.default_rng(sorted(CASES).index(name) * 2 + int(positive) + 100)
    sizes = CASES[name]
    planes = [_plane(rng, H, W, positive, name == "absent") for H, W in sizes]
    starts = np.concatenate([[0], np.cumsum([p.size for p in planes])[:-1]]).astype(np.int64)
    flat = np.concatenate([np.zeros(1, dtype=np.float32)] + [p.reshape(-1) for p in planes])
    for a in (flat, starts):
        a.setflags(write=False)
    return {"planes": flat, "starts": starts, "sizes": sizes}


@functools.lru_cache(maxsize=None)
def _sums(name, positive, h, with_snd):
    k = case(name, positive)
    flat = k["planes"][1:]
    return [window_sums(flat[int(at) : int(at) + H * W], H, W, h, SND if with_snd else None) for at, (H, W) in zip(k["starts"], k["sizes"])]


@functools.lru_cache(maxsize=None)
def expected(name, positive, h, with_snd, method, scale):
    """The twin's result for a case, computed once: (bits uint32 with the layout of the planes, counts)."""
    k = case(name, positive)
    out = np.zeros(k["planes"].shape[0] - 1, dtype=np.uint32)
    counts = np.zeros((len(k["sizes"]), 2), dtype=np.int32)
    for p, (sm, at, (H, W)) in enumerate(zip(_sums(name, positive, h, with_snd), k["starts"], k["sizes"])):
        out[int(at) : int(at) + H * W], counts[p, 0], counts[p, 1] = finish(sm, method, LOOKS, scale == "db")
    out.setflags(write=False)
    counts.setflags(write=False)
    return out, counts


def bits_of(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def ulps(got_bits, want_bits):
    """The largest difference of the int32 bit views over the elements that are finite on both sides (0 when there is none)."""
    g, w = got_bits.view(np.int32).astype(np.int64), want_bits.view(np.int32).astype(np.int64)
    fin = np.isfinite(got_bits.view(np.float32)) & np.isfinite(want_bits.view(np.float32))
    return int(np.abs(g - w)[fin].max()) if fin.any() else 0


# ---- band files for the files -> files runs -----------------------------------------------------------------------------------------------
ITEMS = ("S1A_IW_GRDH_1SDV_20220525T033103_20220525T033128_043365_052DB0_rtc", "S1A_IW_GRDH_1SDV_20220606T033104_20220606T033129_043540_0532E6_rtc")
FX, FY, S = 600000.0, 4400000.0, 16


def write_scenes(root, tagged):
    """Two dates of one scene of 32 x 48 pixels, vv and vh: rows 0..15 of columns 16..31 are the files' no-data value (-32768, named in
    their no-data tag when ``tagged``), so chip (1, 0) has nothing present; NaN elsewhere at random."""
    os.makedirs(root, exist_ok=True)
    rng = np.random.default_rng(11)
    from instageo_amd import crs, tiff

    tags = {33550: (12, (10.0, 10.0, 0.0)), 33922: (12, (0.0, 0.0, 0.0, FX, FY, 0.0)), **crs.geokeys(32636)}
    scenes, planes = [], []
    for item in ITEMS:
        files = []
        for band in ("vv", "vh"):
            a = rng.gamma(4.4, 0.02, size=(32, 48)).astype(np.float32)
            a[rng.random(a.shape) < 0.05] = np.nan
            a[0:16, 16:32] = -32768.0
            files.append(os.path.join(root, f"{item}_{band}.tif"))
            tiff.write(files[-1], a, {"tags": dict(tags), "nodata": -32768.0 if tagged else None})
            planes.append(a)
        scenes.append([files])
    return scenes, planes
