"""Reference for all_touched rasterisation (the rule in include/instageo_hip.h), slow and independent of the span rule:

    an edge TOUCHES pixel (r, c)  iff  the closed segment (x0, y0)-(x1, y1) meets the OPEN square (256 c, 256 c + 256) x (256 r, 256 r + 256)

decided per pixel and edge with ``fractions.Fraction``: the segment is P(t) = P0 + t (P1 - P0), 0 <= t <= 1, and each of the four strict
inequalities 256 c < x(t) < 256 c + 256, 256 r < y(t) < 256 r + 256 is an open half-line in t (or, for a coordinate that does not change,
true or false for every t): a Liang-Barsky clip with strict inequalities.  The open interval they leave meets [0, 1] iff it is not empty,
starts before 1 and ends after 0; that includes a segment with an end inside the square and a segment that is one point.  No rows, no
spans, no floor or ceiling division: it shares no formula with ``instageo_amd.zonal.touch_spans`` or the kernels.

Zones are lists of rings of QUANTISED integer vertices, as in tests/zonal_reference.py, whose centre-rule masks complete the picture:
the all_touched mask of a zone is ``zonal_reference.ref_masks | touched``.
"""
from fractions import Fraction
from functools import lru_cache

import numpy as np

import zonal_reference as ZR

Q = 256
LIM = 2**29


def touches(edge, r, c):
    """The definition for one edge and one pixel, in rational arithmetic."""
    x0, y0, x1, y1 = (int(v) for v in edge)
    lo, hi = None, None  # the open interval of t; None = unbounded
    for p, d, a in ((x0, x1 - x0, Q * c), (y0, y1 - y0, Q * r)):
        if d == 0:
            if not a < p < a + Q:
                return False
            continue
        t0, t1 = Fraction(a - p, d), Fraction(a + Q - p, d)  # where the coordinate equals the square's two sides
        if t0 > t1:
            t0, t1 = t1, t0
        lo = t0 if lo is None or t0 > lo else lo
        hi = t1 if hi is None or t1 < hi else hi
    if lo is None:  # a point, strictly inside
        return True
    return lo < hi and lo < 1 and hi > 0


def touched(edges, H, W):
    """-> (H, W) bool: the pixels at least one of ``edges`` touches.  Pixels the edge's bounding box cannot meet are skipped by a test on
    plain integers (the box of a segment that meets an open square meets it too)."""
    out = np.zeros((H, W), dtype=bool)
    for e in np.asarray(edges).tolist():
        x0, y0, x1, y1 = e
        for r in range(H):
            if not (min(y0, y1) < Q * r + Q and max(y0, y1) > Q * r):
                continue
            for c in range(W):
                if min(x0, x1) < Q * c + Q and max(x0, x1) > Q * c and not out[r, c]:
                    out[r, c] = touches(e, r, c)
    return out


def touched_rows(edges, H):
    """-> (E,) int64: per edge the rows r in [0, H) with a y of the edge strictly between 256 r and 256 r + 256 (what ig_zone_touch_rows
    counts: a row counts whatever its columns are)."""
    out = []
    for _, y0, _, y1 in np.asarray(edges).tolist():
        out.append(sum(1 for r in range(H) if min(y0, y1) < Q * r + Q and max(y0, y1) > Q * r))
    return np.array(out, dtype=np.int64)


# ---- cases ------------------------------------------------------------------------------------------------------------------------------------
def _sliver(x0, y0, x1, y1, h=7):
    """A triangle with two long sides: (x0, y0) -> (x1, y1) and back from (x1, y1 + h)."""
    return [[(x0, y0), (x1, y1), (x1, y1 + h)]]


def _hand():
    """Hand-built zones on 8 x 9 pixels; tests/test_cpu_all_touched.py states what each of them must select."""
    sq = lambda d=(0, 0): [(512 + d[0], 512 + d[1]), (1280 + d[0], 512 + d[1]), (1280 + d[0], 1024 + d[1]), (512 + d[0], 1024 + d[1])]  # noqa: E731
    return [
        [sq()],  # 0: columns 2-4, rows 2-3, on the lattice
        [sq((1, 0))], [sq((-1, 0))], [sq((0, 1))], [sq((0, -1))],  # 1-4: shifted by one unit right, left, down, up
        [[(768, 100), (768, 900)]],  # 5: a vertical edge (there and back) on a column border
        [[(100, 768), (900, 768)]],  # 6: a horizontal edge on a row border
        [[(769, 100), (769, 900)]],  # 7: one unit off the border
        [[(100, 767), (900, 767)]],  # 8
        [[(512, 512), (600, 700), (530, 680)]],  # 9: a vertex exactly on the corner of pixels (1..2, 1..2)
        [[(256, 256), (1024, 1024), (1024, 1030)]],  # 10: a 45 degree edge through pixel corners
        [[(1300, 300), (1350, 310), (1320, 360)]],  # 11: smaller than a pixel, strictly inside (1, 5), away from its centre
        [[(1000, 1000), (1050, 1010), (1020, 1050)]],  # 12: smaller than a pixel, straddling the corner (1024, 1024): four pixels
        [[(-900, 300), (-10, 310), (-10, 700)]],  # 13: wholly left of column 0: nothing
        [[(-300, -300), (300, 200), (-200, 400)]],  # 14: partly outside, top left, negative coordinates
        [[(9 * 256 + 5, 100), (9 * 256 + 400, 900), (9 * 256 + 100, 1000)]],  # 15: wholly right
        [[(2000, 7 * 256 + 100), (2600, 8 * 256 + 300), (2100, 9 * 256)]],  # 16: partly below and right
        [[(100, -700), (2000, -3), (900, -1)]],  # 17: wholly above
        [[(300, 1300), (2000, 1300), (2000, 1900), (300, 1900)], [(700, 1500), (1700, 1500), (1700, 1540), (700, 1540)]],  # 18: a hole 40 units thin
        [[(-LIM, -LIM), (LIM, LIM), (LIM, LIM - 1)]],  # 19: coordinates at +-2^29
        [[(-LIM, 900), (LIM, 901), (LIM, 1000)]],  # 20
    ]


def _wide(W=1500):
    """3 x 1500: a sliver whose two long edges each span all 1500 columns inside row 1 (the wave-wide path, over the 1024-column chunk of
    the merge), one spanning 65 columns (one step of 64 and one more), a polygon with sub-pixel vertices across column 1024 whose inside
    mask the merge has to carry from chunk to chunk, a hole thinner than a pixel across the same column, and steep random ones."""
    zones = [_sliver(-50, 300, W * Q + 50, 310, 20), _sliver(100 * Q + 10, 100, 165 * Q - 10, 120, 9),
             [[(900 * Q + 77, 51), (1100 * Q + 179, 40), (1100 * Q + 150, 666), (900 * Q + 99, 700)]],
             [[(1000 * Q + 3, 10), (1050 * Q + 5, 10), (1050 * Q + 5, 760), (1000 * Q + 3, 760)],
              [(1010 * Q, 300), (1040 * Q + 9, 300), (1040 * Q + 9, 330), (1010 * Q, 330)]]]
    return zones + ZR.random_zones(1500, 5, 3, W, spread=0.05)


def _many(H=9, W=70):
    """65 zones: two passes, bit 63 in use; the only zone of the second pass lies strictly inside pixel (4, 30) away from its centre, so
    that pass crosses no centre line and still has a pixel."""
    zones = ZR.random_zones(65, 64, H, W, vmin=3, vmax=4, spread=0.1)
    return zones + [[[(30 * Q + 10, 4 * Q + 10), (30 * Q + 60, 4 * Q + 20), (30 * Q + 30, 4 * Q + 70)]]]


def cases():
    """name -> (H, W, zones)."""
    return {
        "random_5x7": (5, 7, ZR.random_zones(57, 8, 5, 7)),
        "random_23x41": (23, 41, ZR.random_zones(2341, 20, 23, 41)),
        "hand_8x9": (8, 9, _hand()),
        "wave_37x130": (37, 130, ZR.random_zones(37130, 24, 37, 130) + [_sliver(-40, 9 * Q + 30, 130 * Q + 40, 9 * Q + 200, 30),
                                                                        _sliver(3 * Q + 1, 20 * Q + 5, 72 * Q - 1, 20 * Q + 250, 1)]),
        "wide_3x1500": (3, 1500, _wide()),
        "zones65_9x70": (9, 70, _many()),
    }


@lru_cache(maxsize=None)
def reference(name):
    """-> (edges, edge_zone, Z, touched (Z, H, W) bool by the Fraction rule); read-only arrays, computed once per process."""
    H, W, zones = cases()[name]
    edges, edge_zone = ZR.edges_of(zones)
    out = np.stack([touched(edges[edge_zone == z], H, W) for z in range(len(zones))])
    for a in (edges, edge_zone, out):
        a.setflags(write=False)
    return edges, edge_zone, len(zones), out


@lru_cache(maxsize=None)
def twin_masks(name):
    """-> (Z, H, W) bool: the all_touched masks the device has to produce, centre rule (tests/zonal_reference.py) OR the numpy twin of
    the span rule (tests/test_cpu_all_touched.py holds the twin against ``reference``)."""
    from instageo_amd import zonal

    H, W, zones = cases()[name]
    edges, edge_zone = ZR.edges_of(zones)
    out = ZR.ref_masks(edges, edge_zone, len(zones), H, W)
    for z in range(len(zones)):
        out[z] |= zonal.touched_mask(edges[edge_zone == z], H, W)
    out.setflags(write=False)
    return out
