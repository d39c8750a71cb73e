"""Sequential twin of the Sentinel-2 chip rule of include/instageo_hip.h (ig_s2_chip_cut): plain Python integers, one loop per pixel, written
from the rule alone and sharing nothing with instageo_amd/s2_chips.py.  It is the oracle of the numpy host path and of the kernel; the
deterministic planes and the cases both test files use are built here too."""
import numpy as np

SCL_TABLE = {"cloud": [8, 9], "water": [6], "cloud_shadow": [3], "cirrus": [10], "snow": [11]}
BAND_VALUES = [0, 1, 999, 1000, 1001, 10000, 10001, 32768, 65535]  # every plane holds all of them
SCL_VALUES = list(range(12)) + [12, 31, 32, 255]


def src_index(x, po, pk):
    """The source pixel of output pixel x along one axis: floor(((2 x + 1) po) / (2 pk)) in exact integers."""
    return ((2 * int(x) + 1) * int(po)) // (2 * int(pk))


def cut(planes, scl_planes, origins, S, out_grid, T, class_bits, strategy, nd=0, boa=0, valid_range=None):
    """planes: a list of T * C (array (H, W) uint16, pixel size); scl_planes: a list of T (array (H, W) uint8, pixel size) or None.
    -> (chips (n, TC, S, S) uint16, valid_values (n,) int32, validity (n, S, S) uint8)."""
    Ho, Wo, po = out_grid
    TC = len(planes)
    C = TC // T
    n = len(origins)
    chips = np.zeros((n, TC, S, S), dtype=np.uint16)
    valid = np.zeros(n, dtype=np.int32)
    plane = np.zeros((n, S, S), dtype=np.uint8)

    def read(a, p, r, c):
        rs, cs = src_index(r, po, p), src_index(c, po, p)
        return int(a[rs, cs]) if rs < a.shape[0] and cs < a.shape[1] else 0

    for i, (r0, c0) in enumerate(origins):
        assert 0 <= r0 <= Ho - S and 0 <= c0 <= Wo - S
        for r in range(S):
            for c in range(S):
                masked = [False] * T
                if scl_planes is not None:
                    for t, (a, p) in enumerate(scl_planes):
                        k = read(a, p, r0 + r, c0 + c)
                        masked[t] = k < 32 and ((class_bits >> k) & 1) == 1
                anyone = any(masked)
                nvalid = 0
                for b, (a, p) in enumerate(planes):
                    v = read(a, p, r0 + r, c0 + c)
                    if boa > 0 and v != 0:
                        v = max(v - boa, 0)
                    if (strategy == "each" and masked[b // C]) or (strategy == "any" and anyone):
                        v = nd
                    if valid_range is not None and not (valid_range[0] <= v <= valid_range[1]):
                        v = nd
                    chips[i, b, r, c] = v
                    nvalid += v != nd
                valid[i] += nvalid
                plane[i, r, c] = (1 if nvalid == TC else 0) | (2 if nvalid > 0 else 0)
    return chips, valid, plane


# ---- planes ----------------------------------------------------------------------------------------------------------------------------------
def band_plane(H, W, seed):
    """A uint16 plane: mostly reflectances around the BOA offset and the valid range, the BAND_VALUES sprinkled in and set along the first
    row, and a no-data patch in the top-left corner."""
    rng = np.random.default_rng(seed)
    a = rng.integers(900, 10400, size=(H, W)).astype(np.uint16)
    pick = rng.random((H, W))
    special = np.array(BAND_VALUES, dtype=np.uint16)[rng.integers(0, len(BAND_VALUES), size=(H, W))]
    a = np.where(pick < 0.25, special, a).astype(np.uint16)
    a[: max(H // 12, 1), : max(W // 12, 1)] = 0
    a[-1, : len(BAND_VALUES)] = BAND_VALUES
    return a


def scl_plane(H, W, seed):
    """A uint8 SCL plane in which every class 0..11 and the values 12, 31, 32 and 255 occur."""
    rng = np.random.default_rng(seed)
    a = np.array(SCL_VALUES, dtype=np.uint8)[rng.integers(0, len(SCL_VALUES), size=(H, W))]
    a[rng.random((H, W)) < 0.4] = 4  # vegetation: clear
    a[-1, : len(SCL_VALUES)] = SCL_VALUES
    return a


# name -> the output grid (H_o, W_o, p_o), T, the band planes (H, W, p) and the SCL planes (H, W, p), chip sizes and origins.  The 10 m grid
# is 140 x 150; a 20 m plane is 70 x 75, a 60 m plane 24 x 25 (the last source row covers output rows 138..143, the last column 144..149).
_TEN, _TWENTY, _SIXTY = (140, 150, 10), (70, 75, 20), (24, 25, 60)
CASES = {
    # the workload in small: three 10 m and three 20 m bands under a 20 m SCL
    "c6_10m": dict(grid=(140, 150, 10), T=1, bands=[_TEN, _TEN, _TEN, _TWENTY, _TWENTY, _TWENTY], scl=[_TWENTY]),
    # one 20 m band and the SCL stored one row short: output rows 138..139 take the fill (SCL class 0, which CLASS_BITS masks)
    "short_plane": dict(grid=(140, 150, 10), T=1, bands=[_TEN, (69, 75, 20), _TWENTY], scl=[(69, 75, 20)]),
    # a 60 m band next to a 10 m and a 20 m one
    "sixty": dict(grid=(140, 150, 10), T=1, bands=[_SIXTY, _TEN, _TWENTY], scl=[_TWENTY]),
    # three dates of two bands
    "t3c2": dict(grid=(140, 150, 10), T=3, bands=[_TEN, _TWENTY] * 3, scl=[_TWENTY] * 3),
    # downsampling: the same planes onto a 20 m grid
    "down_20m": dict(grid=(70, 75, 20), T=1, bands=[_TEN, _TEN, _TEN, _TWENTY, _TWENTY, _TWENTY], scl=[_TWENTY]),
}
SIZES = {  # chip side -> origins on a 140 x 150 grid (odd and even, (1, 1), (7, 13) and the last position); 130 crosses the 128-column block
    32: [(0, 0), (1, 1), (7, 13), (64, 32), (108, 118)],
    130: [(0, 0), (1, 1), (7, 13), (10, 20)],
}
SIZES_DOWN = {32: [(0, 0), (1, 1), (7, 13), (38, 43)]}  # on the 70 x 75 grid


def sizes_of(name):
    return SIZES_DOWN if name == "down_20m" else SIZES


def make_case(name, fully_masked=None, S=32):
    """-> (k, planes [(array, p)], scl_planes [(array, p)]).  ``fully_masked``: (row0, col0) of an S x S output window whose SCL is cloud
    (class 9) on every date."""
    k = CASES[name]
    po = k["grid"][2]
    planes = [(band_plane(H, W, seed=17 * i + len(name)), p) for i, (H, W, p) in enumerate(k["bands"])]
    scls = [(scl_plane(H, W, seed=101 * t + len(name)), p) for t, (H, W, p) in enumerate(k["scl"])]
    if fully_masked is not None:
        r0, c0 = fully_masked
        for a, p in scls:
            a[src_index(r0, po, p) : src_index(r0 + S - 1, po, p) + 1, src_index(c0, po, p) : src_index(c0 + S - 1, po, p) + 1] = 9
    return k, planes, scls


def pack(planes, dtype, lead=0):
    """-> (buffer with ``lead`` unused elements in front, starts int64, geom (k, 3) int64)."""
    starts, at = [], lead
    for a, _ in planes:
        starts.append(at)
        at += a.size
    buf = np.zeros(at, dtype=dtype)
    for (a, _), s in zip(planes, starts):
        buf[s : s + a.size] = a.reshape(-1)
    geom = np.array([(a.shape[0], a.shape[1], p) for a, p in planes], dtype=np.int64).reshape(-1, 3)
    return buf, np.array(starts, dtype=np.int64), geom


# ---- the option sets both test files run, and the twin's results, computed once per session ------------------------------------------------
CLASS_BITS = (1 << 8) | (1 << 9) | (1 << 6) | (1 << 3) | (1 << 0)  # class 0 too: the fill outside a short SCL plane is masked
OPTIONS = {  # strategy, with SCL, boa_offset, valid_range, no_data
    "each": ("each", True, 0, None, 0),
    "any": ("any", True, 0, None, 0),
    "no_scl": ("each", False, 0, None, 0),
    "each_boa_range": ("each", True, 1000, (0, 10000), 0),
    "any_boa_nd7": ("any", True, 1000, None, 7),
    "any_range_nd65535": ("any", True, 0, (0, 10000), 65535),
}
_twin_cache = {}


def twin(name, S, option, origins=None):
    """The twin's (chips, valid_values, validity) of case ``name`` at chip side S under OPTIONS[option], on the case's own origins."""
    key = (name, S, option, None if origins is None else tuple(origins))
    if key not in _twin_cache:
        k, planes, scls = make_case(name)
        strategy, with_scl, boa, rng, nd = OPTIONS[option]
        o = sizes_of(name)[S] if origins is None else list(origins)
        _twin_cache[key] = cut(planes, scls if with_scl else None, o, S, k["grid"], k["T"], CLASS_BITS, strategy, nd, boa, rng)
    return _twin_cache[key]
