"""Reference for the zonal statistics: the definition of include/instageo_hip.h evaluated directly, pixel by pixel.

    a directed edge (x0, y0) -> (x1, y1) crosses row r  iff  (y0 <= Yc) != (y1 <= Yc),        Yc = 256 r + 128
    its crossing lies at or left of the centre of (r, c)  iff  xc <= Xc,                      Xc = 256 c + 128
    with xc = x0 + (x1 - x0)(Yc - y0)/(y1 - y0);  a pixel is inside a zone iff the number of such edges is odd.

No toggle canvas and no scan: every pixel counts its own crossings.  ``inside`` does it with ``fractions.Fraction`` on Python ints, one
pixel at a time; ``ref_masks`` decides ``xc <= Xc`` by the sign of a cross product, (x1 - x0)(Yc - y0) <= (Xc - x0)(y1 - y0) for
y1 > y0 and >= for y1 < y0, for all columns of a row at once (int64, after asserting on Python ints that nothing can reach 2^62); the CPU
tests hold the two against each other.  Zones here are lists of rings of QUANTISED integer vertices (Q = 256 units per pixel), so ties
can be placed exactly; ``edges_of`` strings them into the (E, 4) edge array by itself (not through instageo_amd.zonal).
"""
from fractions import Fraction
from functools import lru_cache

import numpy as np

Q, HALF = 256, 128


def edges_of(zones):
    """zones: a list of zones, each a list of rings, each a list of (X, Y) ints -> (edges (E, 4) int32, edge_zone (E,) int32)."""
    edges, owner = [], []
    for z, rings in enumerate(zones):
        for ring in rings:
            n = len(ring)
            for i in range(n):
                (x0, y0), (x1, y1) = ring[i], ring[(i + 1) % n]
                edges.append((int(x0), int(y0), int(x1), int(y1)))
                owner.append(z)
    return np.array(edges, dtype=np.int32).reshape(-1, 4), np.array(owner, dtype=np.int32)


def inside(zone_edges, r, c):
    """The definition for one pixel, in rational arithmetic."""
    yc, xc_pix = Q * r + HALF, Q * c + HALF
    n = 0
    for x0, y0, x1, y1 in zone_edges:
        x0, y0, x1, y1 = int(x0), int(y0), int(x1), int(y1)
        if (y0 <= yc) != (y1 <= yc):
            n += x0 + Fraction((x1 - x0) * (yc - y0), y1 - y0) <= xc_pix
    return n % 2 == 1


def ref_masks(edges, edge_zone, Z, H, W):
    """-> (Z, H, W) bool: pixel (r, c) inside zone z."""
    odd = np.zeros((Z, H, W), dtype=bool)
    xs = Q * np.arange(W, dtype=np.int64) + HALF
    for (x0, y0, x1, y1), z in zip(edges.tolist(), edge_zone.tolist()):
        if y0 == y1:
            continue
        for r in range(H):
            yc = Q * r + HALF
            if (y0 <= yc) == (y1 <= yc):
                continue
            lhs, dy = (x1 - x0) * (yc - y0), y1 - y0
            assert abs(lhs) < 2**62 and (abs(Q * W + HALF) + abs(x0)) * abs(dy) < 2**62
            rhs = (xs - x0) * dy
            odd[z, r] ^= (lhs <= rhs) if dy > 0 else (lhs >= rhs)
    return odd


def to_planes(masks):
    """(Z, H, W) bool -> (ceil(Z / 64), H, W) int64 bit planes: bit z % 64 of plane z // 64."""
    Z, H, W = masks.shape
    planes = np.zeros(((Z + 63) // 64, H, W), dtype=np.uint64)
    for z in range(Z):
        planes[z // 64] |= masks[z].astype(np.uint64) << np.uint64(z % 64)
    return planes.view(np.int64)


def ref_counts(cm, masks, ncls, fill=-1):
    """-> (Z, ncls + 1) int64: the inside pixels of every class; last column: fill, or a value outside [0, ncls)."""
    k = np.where((cm != fill) & (cm >= 0) & (cm < ncls), cm, ncls).astype(np.int64)
    out = np.zeros((len(masks), ncls + 1), dtype=np.int64)
    for z, m in enumerate(masks):
        out[z] = np.bincount(k[m], minlength=ncls + 1)
    return out


# ---- cases --------------------------------------------------------------------------------------------------------------------------------
def px(*pts):
    """A ring from pixel coordinates (exact multiples of 1/256 only)."""
    out = []
    for x, y in pts:
        X, Y = x * Q, y * Q
        assert X == int(X) and Y == int(Y)
        out.append((int(X), int(Y)))
    return out


def rect(x0, y0, x1, y1):
    return px((x0, y0), (x1, y0), (x1, y1), (x0, y1))


def random_zones(seed, n, H, W, vmin=3, vmax=9, spread=0.4):
    """n zones of one ring each, vmin..vmax vertices drawn anywhere in the raster widened by ``spread`` on every side, at any of the
    256 sub-pixel positions: off the lattice, partly outside, self-intersecting as they come."""
    rng = np.random.default_rng(seed)
    zones = []
    for _ in range(n):
        k = int(rng.integers(vmin, vmax + 1))
        xs = rng.integers(int(-spread * W * Q), int((1 + spread) * W * Q) + 1, size=k)
        ys = rng.integers(int(-spread * H * Q), int((1 + spread) * H * Q) + 1, size=k)
        zones.append([[(int(x), int(y)) for x, y in zip(xs, ys)]])
    return zones


def class_map(seed, H, W, ncls, fill=-1, extra=()):
    """A seeded map of classes 0..ncls-1 with about one pixel in six at ``fill`` and, from ``extra``, values that are no class."""
    rng = np.random.default_rng(seed)
    cm = rng.integers(0, ncls, size=(H, W)).astype(np.int8)
    cm[rng.random((H, W)) < 1 / 6] = fill
    for v in extra:
        cm[rng.random((H, W)) < 1 / 12] = v
    return cm


def _seventy(H=24, W=40):
    """70 zones on 24 x 40: two passes; zones 63 (bit 63) and 64 (bit 0 of the second pass) cover real ground."""
    zones = [
        [rect(-5, -5, W + 5, H + 5)],                             # 0 covers everything
        [rect(0, 0, W, H)],                                       # 1 exactly the raster
        [rect(-30, 2, -3, 9)], [rect(W + 2, 2, W + 20, 9)],       # 2, 3 wholly outside, left and right
        [rect(3, -40, 9, -2)], [rect(3, H + 1, 9, H + 30)],       # 4, 5 wholly outside, above and below
        [px((-7.5, 3.25), (12.5, 8.0), (-3.0, 20.5))],            # 6 crosses left of column 0
        [px((W + 9.25, 1.5), (W - 11.0, 12.0), (W + 2.5, 22.75))],  # 7 crosses right of column W - 1
        [px((5.0, -3.0), (9.5, H + 4.0), (20.25, H + 4.0))],      # 8 an edge that spans every row
        [rect(4, 4, 20, 16)], [rect(10, 8, 30, 20)], [rect(12, 10, 18, 14)],  # 9, 10, 11 overlap
        [rect(2, 2, 30, 22), rect(6, 6, 14, 12), rect(16, 6, 28, 18)],  # 12 two holes
        [rect(1, 1, 8, 8), rect(20, 10, 38, 23)],                 # 13 MultiPolygon-like: two exteriors
    ]
    zones += random_zones(70, 70 - len(zones), H, W)
    zones[63] = [rect(7, 3, 33, 21), rect(15, 9, 22, 14)]         # bit 63 of the first pass
    zones[64] = [rect(-2, 5, W + 2, 17)]                          # bit 0 of the second pass
    return zones


def _ties():
    c = lambda i: Q * i + HALF  # noqa: E731  the centre of pixel i
    return [
        [[(c(1), c(1)), (c(5), c(1)), (c(5), c(4)), (c(1), c(4))]],         # every vertex on a pixel centre, edges along centre lines
        [[(c(0), c(0)), (c(6), c(6)), (c(0), c(6))]],                       # a diagonal edge through seven centres
        [[(c(6), c(0)), (c(0), c(6)), (c(6), c(6))]],                       # the other diagonal
        [[(40, c(2)), (7 * Q, c(2)), (7 * Q, c(5)), (40, c(5))]],           # horizontal edges on centre lines
        [[(c(1), 30), (c(4), 6 * Q + 3), (c(1), 30)], [(Q, Q), (5 * Q, 5 * Q), (3 * Q, 3 * Q)]],  # zero-area rings
        [[(Q, Q), (3 * Q, 3 * Q), (5 * Q, Q), (5 * Q, 5 * Q), (3 * Q, 3 * Q), (Q, 5 * Q)]],  # a ring that touches itself at (3, 3)
        [[(c(3), c(3)), (c(6), c(1)), (c(6), c(7)), (c(3), c(3)), (c(0), c(7)), (c(0), c(1))]],  # ... at a pixel centre
        [[(0, 0), (8 * Q, 0), (8 * Q, 8 * Q), (0, 8 * Q)], [(c(2), c(2)), (c(5), c(2)), (c(5), c(5)), (c(2), c(5))]],  # hole on centres
        [[(c(2), c(-1)), (c(2), c(9)), (c(4), c(9)), (c(4), c(-1))]],       # vertical edges through centres, ends outside
        [[(c(3), c(3)), (c(3) + 1, c(3)), (c(3) + 1, c(3) + 1), (c(3), c(3) + 1)]],  # a sliver that holds exactly one centre
    ]


def _wide(W=9000):
    """3 x 9000: rows of nine chunks of 1024 columns (ZCHUNK in zonal.hip), the last one partial."""
    zones = [
        [rect(5, 0, W - 10, 3)],                                  # inside from chunk 0 to chunk 8
        [rect(1023, 0, 1025, 2)], [rect(1024, 1, 2048, 3)],       # across and on chunk borders
        [rect(-3, 0.25, W + 3, 2.75), rect(3000, 0, 6100.5, 3)],  # a hole over three chunks
        [px((100.5, -1), (8900.25, 4), (4000, -2))],
        [rect(W - 1, 0, W, 3)], [rect(0, 0, 1, 1)],               # the last and the first column
    ]
    return zones + random_zones(9000, 6, 3, W, spread=0.05)


def cases():
    """name -> (H, W, zones)."""
    return {
        "odd_37x67": (37, 67, [[rect(-1, -1, 70, 40)], [rect(10.5, 3.5, 64.5, 30.5), rect(20, 10, 40, 20)]] + random_zones(37, 10, 37, 67)),
        "wide_3x9000": (3, 9000, _wide()),
        "one_pixel": (1, 1, [[rect(0, 0, 1, 1)], [rect(0.75, 0, 1, 1)], [[(HALF, HALF), (HALF + 1, HALF), (HALF, HALF + 1)]],
                             [[(HALF, HALF - 1), (HALF + 9, HALF + 5), (HALF - 9, HALF + 5)]]]),
        "seventy_24x40": (24, 40, _seventy()),
        "ties_8x8": (8, 8, _ties()),
        "random_19x23": (19, 23, random_zones(1923, 50, 19, 23)),
    }


@lru_cache(maxsize=None)
def reference(name):
    """-> (edges, edge_zone, Z, masks (Z, H, W) bool) of a case, computed once; the arrays are read-only."""
    H, W, zones = cases()[name]
    edges, edge_zone = edges_of(zones)
    masks = ref_masks(edges, edge_zone, len(zones), H, W)
    for a in (edges, edge_zone, masks):
        a.setflags(write=False)
    return edges, edge_zone, len(zones), masks
