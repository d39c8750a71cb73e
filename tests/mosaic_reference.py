"""Pixel-by-pixel reference of the mosaic rule of include/instageo_hip.h (ig_mosaic_paste), the inputs the tests run on and the table of
their shapes.  Plain loops over the chips and the pixels, lists of contributors and collections.Counter: nothing here is shared with
instageo_amd.mosaic.

Chip i is the rectangle (row0, col0, h, w) on an H x W canvas; it contributes to a pixel it covers unless its value there is transparent
(int8: == fill, float32: NaN); contributors are ordered by chip index.  last / first: the contributor with the largest / smallest index;
mode: the value most contributors have, ties to the smallest; mean: the float32 sum in index order over the count; none: fill / NaN."""
import functools
from collections import Counter

import numpy as np

NAN_BITS = 0x7FC00000
NAN = np.uint32(NAN_BITS).view(np.float32)
RULES = {"int8": ("last", "first", "mode"), "float32": ("last", "first", "mean")}


def contributors(chips, rects, H, W, fill):
    """{(row, col): [values in chip order]} for the canvas pixels with at least one contributor."""
    out = {}
    for a, (r0, c0, h, w) in zip(chips, rects):
        assert a.shape == (h, w)
        is_f = a.dtype == np.float32
        for r in range(max(0, -r0), min(h, H - r0)):
            for c in range(max(0, -c0), min(w, W - c0)):
                v = a[r, c]
                if np.isnan(v) if is_f else int(v) == fill:
                    continue
                out.setdefault((r0 + r, c0 + c), []).append(v)
    return out


def value_of(values, rule):
    if rule == "last":
        return values[-1]
    if rule == "first":
        return values[0]
    if rule == "mode":
        tally = Counter(int(v) for v in values)
        top = max(tally.values())
        return min(v for v, n in tally.items() if n == top)
    assert rule == "mean"
    s = np.float32(values[0])
    for v in values[1:]:
        s = np.float32(s + np.float32(v))
    return np.float32(s / np.float32(len(values)))


def reference(chips, rects, shape, rule, fill=-1):
    """-> (canvas, cover uint8)."""
    H, W = shape
    dtype = chips[0].dtype
    assert rule in RULES[dtype.name]
    canvas = np.full((H, W), NAN if dtype == np.float32 else fill, dtype=dtype)
    cover = np.zeros((H, W), dtype=np.uint8)
    for (r, c), values in contributors(chips, [tuple(int(x) for x in r) for r in rects], H, W, fill).items():
        canvas[r, c] = value_of(values, rule)
        cover[r, c] = min(len(values), 255)
    return canvas, cover


def bits(a):
    """The uint32 view of a float32 array: NaN positions (and payloads) and the sign of zero count in a comparison."""
    return np.ascontiguousarray(a).view(np.uint32)


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    return np.array_equal(bits(got), bits(want)) if want.dtype == np.float32 else np.array_equal(got, want)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
# name -> what the shape can break in a kernel whose workgroup owns a 64 x 64 block, whose threads own 16 pixels of a row and whose chip
# list goes through LDS in chunks
CASES = {
    "one": "a 1 x 1 chip on a 1 x 1 canvas",
    "corner": "130 x 130: three 5 x 7 chips across a block corner (four blocks see all three; odd w: unaligned chip rows)",
    "empty": "65 x 129: chips only in columns < 64, so one whole block has an empty list; partial blocks at the right and bottom edge",
    "overhang": "chips with negative row0 / col0 and beyond the right / bottom edge, one larger than the canvas, one wholly outside",
    "row": "3 x 9000: 141 blocks in a row, the last one partial; 37 chips of 3 x 250 overlapping by 7 columns",
    "stack": "300 chips of 3 x 3 inside one block: a list longer than any chunk; values 0..126, a stray -128, fill = a class value (5)",
}
FLOAT_CASES = ("one", "corner", "stack")
CORNER_TIE = (63, 63)  # chips 0 and 1 hold 1 and 2 there, chip 2 is transparent: mode takes the smaller, last the larger
CORNER_NONE = (64, 64)  # inside all three chips, transparent in all of them
CORNER_ALL = ((62, 62), (62, 65), (64, 62), (64, 65))  # one pixel in each of the four blocks where all three chips contribute
STACK_ALL = (32, 32)  # all 300 chips contribute there


def _ints(rng, h, w, lo, hi, fill, holes):
    a = rng.integers(lo, hi, size=(h, w)).astype(np.int8)
    a[rng.random((h, w)) < holes] = fill
    return a


def _floats(rng, h, w, holes):
    a = (0.5 + rng.random((h, w))).astype(np.float32)  # [0.5, 1.5): no subnormals, sums of hundreds stay far from overflow
    a[rng.random((h, w)) < holes] = np.nan
    return a


@functools.lru_cache(maxsize=None)
def case(name, dtype="int8"):
    """-> (chips (read-only arrays), rects [(row0, col0, h, w)], (H, W), fill)."""
    assert name in CASES and (dtype == "int8" or name in FLOAT_CASES)
    rng = np.random.default_rng(len(name) + (7 if dtype == "int8" else 11))
    is_f = dtype == "float32"
    fill = -1
    make = (lambda h, w, holes=0.25: _floats(rng, h, w, holes)) if is_f else (lambda h, w, holes=0.25: _ints(rng, h, w, 0, 3, fill, holes))
    if name == "one":
        shape, rects = (1, 1), [(0, 0, 1, 1)]
        chips = [np.array([[0.75 if is_f else 1]], dtype=dtype)]
    elif name == "corner":
        shape, rects = (130, 130), [(61, 60, 5, 7), (62, 59, 5, 7), (60, 61, 5, 7)]
        chips = [make(5, 7) for _ in rects]
        clear = np.nan if is_f else fill
        for i, (a, (r0, c0, _, _), tie) in enumerate(zip(chips, rects, (1, 2, clear))):
            for r, c in CORNER_ALL:
                a[r - r0, c - c0] = (1.5, 1.75, 1.75)[i] if is_f else (i + 1) % 3  # the sum 5: 5 / 3 and 5 * (1 / 3) differ in float32
            a[CORNER_NONE[0] - r0, CORNER_NONE[1] - c0] = clear
            if not is_f:
                a[CORNER_TIE[0] - r0, CORNER_TIE[1] - c0] = tie
    elif name == "empty":
        shape, rects = (65, 129), [(5, 10, 20, 30), (60, 20, 5, 40), (0, 0, 3, 64), (40, 33, 25, 31)]
        chips = [make(h, w) for _, _, h, w in rects]
    elif name == "overhang":
        shape = (70, 100)
        rects = [(-10, -10, 90, 120), (-3, -5, 10, 20), (65, 90, 10, 20), (-2, 95, 8, 10), (60, -4, 20, 9), (200, 200, 3, 3), (-20, 10, 5, 5),
                 (30, 47, 9, 33)]
        chips = [make(h, w, 0.5) for _, _, h, w in rects]
    elif name == "row":
        shape, rects = (3, 9000), [(0, 243 * i, 3, 250) for i in range(37)]
        chips = [make(3, 250) for _ in rects]
    else:  # stack
        fill = 5
        shape = (70, 70)
        rects = [(30 + i % 3, 30 + (i // 3) % 3, 3, 3) for i in range(300)]
        chips = []
        for i, (r0, c0, _, _) in enumerate(rects):
            a = _floats(rng, 3, 3, 0.2) if is_f else _ints(rng, 3, 3, 0, 127, fill, 0.1)
            if not is_f and i % 17 == 0:
                a[0, 0] = -128
            v = i % 127
            a[STACK_ALL[0] - r0, STACK_ALL[1] - c0] = 0.5 + v / 128.0 if is_f else (v if v != fill else 6)
            chips.append(a)
    for a in chips:
        a.setflags(write=False)
    return tuple(chips), rects, shape, fill


@functools.lru_cache(maxsize=None)
def expected(name, dtype, rule):
    chips, rects, shape, fill = case(name, dtype)
    out = reference(chips, rects, shape, rule, fill)
    for a in out:
        a.setflags(write=False)
    return out


def all_cases():
    """(name, dtype, rule) of every combination the tests run."""
    return [(n, d, r) for d in ("int8", "float32") for n in (CASES if d == "int8" else FLOAT_CASES) for r in RULES[d]]


def brute_bins(rects, H, W, block=64):
    """For every block (row-major): the ascending chip indices whose rectangle intersects it, by testing every pair."""
    out = []
    for y in range(0, H, block):
        for x in range(0, W, block):
            y1, x1 = min(y + block, H), min(x + block, W)
            out.append([i for i, (r0, c0, h, w) in enumerate(rects) if r0 < y1 and r0 + h > y and c0 < x1 and c0 + w > x])
    return out
