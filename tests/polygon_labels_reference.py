"""Reference for the polygon burn: the rule of include/instageo_hip.h evaluated directly, pixel by pixel, independently of
instageo_amd/polygon_labels.py.

    pixel (r, c) is inside feature i  iff  an odd number of i's edges satisfy (y0 <= Yc) != (y1 <= Yc) and xc <= Xc   (zonal_reference)
    the pixel takes the value of the LAST feature, in order, that contains it; a pixel in no feature keeps what the raster held

No canvas, no passes, no scan: ``ZR.ref_masks`` decides every (feature, pixel) pair on Python ints / int64 cross products over all edges of
the feature, and ``burn`` assigns the features in order.  ``burn_rational`` does the same with ``ZR.inside`` (fractions.Fraction), one
pixel at a time; the CPU tests hold the two against each other.  Features are (value, rings) with rings of QUANTISED integer vertices
(Q = 256 units per pixel), so ties can be placed exactly.
"""
import json
from functools import lru_cache

import numpy as np

import zonal_reference as ZR

Q, HALF = ZR.Q, ZR.HALF
PASS = 64


def masks_of(feats, H, W):
    """-> (len(feats), H, W) bool."""
    edges, owner = ZR.edges_of([rings for _, rings in feats])
    return ZR.ref_masks(edges, owner, len(feats), H, W)


def burn(init, feats, masks=None):
    """``init`` (H, W) with the features assigned in order -> a new array."""
    out = np.array(init, copy=True)
    masks = masks_of(feats, *out.shape) if masks is None else masks
    for (value, _), m in zip(feats, masks):
        out[m] = value
    return out


def burn_rational(init, feats):
    out = np.array(init, copy=True)
    per_feature = [ZR.edges_of([rings])[0].tolist() for _, rings in feats]
    for r in range(out.shape[0]):
        for c in range(out.shape[1]):
            for (value, _), edges in zip(feats, per_feature):
                if ZR.inside(edges, r, c):
                    out[r, c] = value
    return out


def pixels_written(masks):
    """What the passes of 64 features store: per pass the pixels inside at least one of its features, summed."""
    return sum(int(masks[k : k + PASS].any(axis=0).sum()) for k in range(0, len(masks), PASS))


def items_of(feats):
    """[(value, edges (E, 4) int32)]: what polygon_labels.burn_fixed takes, strung together here (not through the module)."""
    return [(value, ZR.edges_of([rings])[0]) for value, rings in feats]


def map_features(feats, H):
    """The features in the map coordinates of the grid (X0, Y0, sx, sy) = (0, H, 1, 1): x = X / 256, y = H - Y / 256, exact in float64."""
    from instageo_amd.polygon_labels import Feature

    return [Feature(i, value, [np.array([(X / Q, H - Y / Q) for X, Y in ring], dtype=np.float64) for ring in rings])
            for i, (value, rings) in enumerate(feats)]


# ---- cases --------------------------------------------------------------------------------------------------------------------------------
def seg_values(n, avoid=()):
    """n int8 burn values in [-1, 127] that cycle through all of them but ``avoid``."""
    pool = [v for v in range(-1, 128) if v not in avoid]
    return [pool[(37 * k + 5) % len(pool)] for k in range(n)]


def reg_values(n):
    return [float(np.float32(0.37 * k - 11.5)) for k in range(n)]


def overlapping(n, H, W, seed):
    """n rectangles and triangles piled on one another around the raster's middle: a pixel is claimed by many, across passes."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        x0, y0 = rng.integers(-2 * Q, (W // 2) * Q), rng.integers(-2 * Q, (H // 2) * Q)
        x1, y1 = x0 + rng.integers((W // 4) * Q, (W + 3) * Q), y0 + rng.integers((H // 4) * Q, (H + 3) * Q)
        ring = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)] if k % 3 else [(x0, y0), (x1, y1), (x0, y1)]
        out.append([[(int(x), int(y)) for x, y in ring]])
    return out


def _adjacent():
    """Two features that share an edge through pixel centres (x = 4.5), one that shares a horizontal edge on a centre line (y = 3.5)."""
    return [[ZR.px((1, 1), (4.5, 1), (4.5, 6), (1, 6))], [ZR.px((4.5, 1), (7, 1), (7, 6), (4.5, 6))],
            [ZR.px((1, 6), (7, 6), (7, 7.5), (1, 7.5))]]


def cases():
    """name -> (H, W, zones): lists of rings per feature; values are given per test."""
    H, W, seventy = ZR.cases()["seventy_24x40"]
    return {
        "ties_8x8": (8, 8, ZR.cases()["ties_8x8"][2]),
        "adjacent_8x8": (8, 8, _adjacent()),
        "seventy_24x40": (H, W, seventy),  # holes, two exteriors, overlaps, outside on every side, crossings left of column 0
        "overlap65_24x40": (24, 40, overlapping(65, 24, 40, 65)),
        "overlap130_24x40": (24, 40, overlapping(130, 24, 40, 130)),
        "cover_5x7": (5, 7, [[ZR.rect(1, 1, 3, 3)], [ZR.rect(-5, -5, 12, 10)]]),  # all crossings of the second left of column 0
        "outside_5x7": (5, 7, [[ZR.rect(-9, 1, -2, 4)], [ZR.rect(1, 9, 3, 12)], [ZR.rect(8, 1, 12, 3)]]),
        "odd_37x67": ZR.cases()["odd_37x67"],
    }


@lru_cache(maxsize=None)
def reference(name):
    """-> (H, W, zones, masks) of a case, computed once; the masks are read-only."""
    H, W, zones = cases()[name]
    masks = masks_of([(0, z) for z in zones], H, W)
    masks.setflags(write=False)
    return H, W, zones, masks


# ---- files -----------------------------------------------------------------------------------------------------------------------------------
def square(x, y, side=1.0):
    return [[x, y], [x + side, y], [x + side, y + side], [x, y + side], [x, y]]


def write_geojson(path, feats):
    """feats: (properties, list of polygons, each a list of rings)."""
    out = []
    for props, polys in feats:
        geom = {"type": "Polygon", "coordinates": polys[0]} if len(polys) == 1 else {"type": "MultiPolygon", "coordinates": polys}
        out.append({"type": "Feature", "properties": props, "geometry": geom})
    with open(path, "w") as f:
        json.dump({"type": "FeatureCollection", "features": out}, f)
    return str(path)


S = 16


def parcels(tmp_path, name="parcels.geojson"):
    """Parcels on a 30 m UTM 36N grid with its origin at (399960, 4500000): cells (0, 0), (0, 1) and (1, 2) of 16 pixels get polygons."""
    X0, Y0 = 399960.0, 4500000.0
    at = lambda c, r: [X0 + 30.0 * c, Y0 - 30.0 * r]  # noqa: E731
    quad = lambda c0, r0, c1, r1: [at(c0, r0), at(c1, r0), at(c1, r1), at(c0, r1), at(c0, r0)]  # noqa: E731
    feats = [({"crop": "maize", "day": "2022-06-01"}, [[quad(0.0, 0.0, 12.5, 9.5)]]),
             ({"crop": "wheat", "day": "2022-06-01"}, [[quad(10.25, 5.0, 27.0, 14.0), quad(20.0, 8.0, 23.0, 11.0)]]),
             ({"crop": "maize", "day": "2022-07-11"}, [[quad(36.0, 20.0, 44.5, 29.0)], [quad(33.0, 17.0, 35.0, 19.0)]]),
             ({"crop": "unknown", "day": "2022-07-11"}, [[quad(40.0, 24.0, 47.0, 31.0)]]),
             ({"crop": "wheat", "day": "2022-07-11"}, [[quad(60.6, 40.6, 60.9, 40.9)]])]  # its box holds no pixel centre (outside): its cell stays empty
    return write_geojson(tmp_path / name, feats), (X0, Y0)


CLASSES = {"maize": 1, "wheat": 2, "unknown": -1}
KW = dict(crs=32636, src_crs=32636, spatial_resolution=30.0, chip_size=S, value_property="crop", class_map=CLASSES)
