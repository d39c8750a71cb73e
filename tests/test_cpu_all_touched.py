"""all_touched rasterisation, host side (no GPU): the numpy twin of the span rule (instageo_amd.zonal.touch_spans / touched_mask) against
the Fraction reference of tests/all_touched_reference.py, array for array, on random and hand-built zones; the burn's host path; the
option parsing; the round trip of the tracer's polygons; the header's statement of the rule and the argument checks of the three HIP
entry points.  Every comparison is exact."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import all_touched_reference as AR
import regions_reference as RR
import vector_reference as VR
import zonal_reference as ZR
from instageo_amd import polygon_labels as P
from instageo_amd import vectorize, zonal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "instageo-e2e-geospatial-ml_amd")
NAMES = ("ig_zone_touch_rows", "ig_zone_touch", "ig_zone_touch_merge")
GRID = (500000.0, 4000000.0, 30.0, 30.0)  # X0, Y0 and 30 m pixels in EPSG:32636


@pytest.fixture(scope="module")
def built_lib():
    import subprocess

    from instageo_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j4"], check=True)
    return _lib


def _pixels(mask):
    return sorted(map(tuple, np.argwhere(mask).tolist()))


# ---- the twin against the reference --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(AR.cases()))
def test_twin_equals_the_fraction_reference(name):
    H, W, _ = AR.cases()[name]
    edges, edge_zone, Z, want = AR.reference(name)
    for z in range(Z):
        assert np.array_equal(zonal.touched_mask(edges[edge_zone == z], H, W), want[z]), (name, z)
    for h in (H, 1):
        rows = zonal.touch_rows(edges, h)
        assert rows.dtype == np.int64 and np.array_equal(rows, AR.touched_rows(edges, h)), (name, h)
    # the spans themselves: inside the raster, one per (edge, row), and together exactly the mask
    e, r, c0, c1 = zonal.touch_spans(edges, H, W)
    assert (r >= 0).all() and (r < H).all() and (c0 >= 0).all() and (c1 < W).all() and (c0 <= c1).all()
    assert len(np.unique(np.stack([e, r]), axis=1).T) == len(e)
    painted = np.zeros((H, W), dtype=bool)
    for rr, a, b in zip(r.tolist(), c0.tolist(), c1.tolist()):
        painted[rr, a : b + 1] = True
    assert np.array_equal(painted, want.any(axis=0))
    # a rectangle of the raster is that rectangle of the mask
    rect = (H // 3, W // 4, H - H // 3 - H // 5, W - W // 4 - 1)
    got = zonal.touched_mask(edges, H, W, rect)
    assert np.array_equal(got, want.any(axis=0)[rect[0] : rect[0] + rect[2], rect[1] : rect[1] + rect[3]])


@pytest.mark.parametrize("name", sorted(AR.cases()))
def test_touch_rows_are_the_rows_of_the_spans(name):
    """touch_rows and touch_spans share one row helper: on a raster wide enough for every abscissa (the edges moved right by whole pixels
    until none lies left of column 0) an edge has exactly one span per touched row.  The exception follows from the rule: a vertical edge
    on a column border touches rows (a row counts whatever its columns are) but no open square, so it has no span."""
    H = AR.cases()[name][0]
    edges = np.array(AR.reference(name)[0]).astype(np.int64)
    edges[:, [0, 2]] -= int(edges[:, [0, 2]].min()) // zonal.Q * zonal.Q
    W = int(edges[:, [0, 2]].max()) // zonal.Q + 1
    on_border = (edges[:, 0] == edges[:, 2]) & (edges[:, 0] % zonal.Q == 0)
    for h in (H, 1):
        rows = zonal.touch_rows(edges, h)
        per_edge = np.bincount(zonal.touch_spans(edges, h, W)[0], minlength=len(edges))
        assert rows.sum() > 0 and np.array_equal(per_edge, np.where(on_border, 0, rows)), (name, h)


def test_hand_built_zones_select_what_the_rule_says():
    H, W, zones = AR.cases()["hand_8x9"]
    edges, edge_zone, Z, touched = AR.reference("hand_8x9")
    centre = ZR.ref_masks(edges, edge_zone, Z, H, W)
    full = AR.twin_masks("hand_8x9")
    assert np.array_equal(full, centre | touched)
    block = {(r, c) for r in (2, 3) for c in (2, 3, 4)}
    assert not touched[0].any() and set(_pixels(full[0])) == set(_pixels(centre[0])) == block  # on the lattice: the centre rule's pixels
    for z, ring in ((1, {(2, 5), (3, 5)}), (2, {(2, 1), (3, 1)}), (3, {(4, 2), (4, 3), (4, 4)}), (4, {(1, 2), (1, 3), (1, 4)})):
        assert set(_pixels(centre[z])) == block and set(_pixels(full[z])) == block | ring, z  # one unit over a border: that side of the ring
    assert not full[5].any() and not full[6].any()  # edges exactly on a border touch nothing
    assert _pixels(full[7]) == [(0, 3), (1, 3), (2, 3), (3, 3)] and _pixels(full[8]) == [(2, 0), (2, 1), (2, 2), (2, 3)]  # one unit off
    assert _pixels(touched[9]) == [(2, 2)]  # a vertex on a pixel corner touches only the pixel the polygon enters
    assert _pixels(touched[10])[:3] == [(1, 1), (2, 1), (2, 2)] and (0, 0) not in _pixels(touched[10])  # 45 degrees through corners
    assert not centre[11].any() and _pixels(full[11]) == [(1, 5)]  # smaller than a pixel, inside one
    assert not centre[12].any() and _pixels(full[12]) == [(3, 3), (3, 4), (4, 3), (4, 4)]  # straddling a corner
    for z in (13, 15, 17):  # wholly left, right, above: a span left of column 0 is not moved onto it
        assert not full[z].any(), z
    assert _pixels(touched[14]) == [(0, 0), (0, 1), (1, 0)] and _pixels(touched[16]) == [(7, 7), (7, 8)]
    assert centre[18].sum() == 14 and full[18].sum() == 21 and full[18, 5:8, 1:8].all()  # the thin hole is touched shut
    assert touched[19].sum() == 16 and _pixels(touched[20]) == [(3, c) for c in range(9)]  # +-2^29: nothing overflows
    # floor division of negatives: a span that ends at X = -1 belongs to column -1, one that ends at X = 1 to column 0
    for x1, want in ((-1, []), (0, []), (1, [(0, 0)])):
        assert _pixels(zonal.touched_mask(np.array([[-700, 100, x1, 100]], dtype=np.int32), 3, 3)) == want, x1


def test_polygons_of_the_tracer_hold_exactly_their_regions(tmp_path):
    """Region polygons have their vertices on the pixel lattice: no edge touches a pixel, so all_touched changes nothing."""
    cm = np.array(VR.cases()["blobs_33x31_x3"][0])
    rings, vertices = VR.ref_rings(cm)
    table = RR.ref_table(cm, 4)
    path = vectorize.write_geojson(str(tmp_path / "p.geojson"), rings, vertices, table, None)
    zones = zonal.read_zones(path, "root")
    edges, edge_zone = zonal.zones_to_pixels(zones, None)
    H, W = cm.shape
    labels = VR.bfs_label(cm, 4, -1)
    centre = ZR.ref_masks(edges, edge_zone, len(zones), H, W)
    assert len(zones) > 10 and not zonal.touched_mask(edges, H, W).any()
    for z, zone in enumerate(zones):
        assert np.array_equal(centre[z] | zonal.touched_mask(edges[edge_zone == z], H, W), labels == zone.id), zone.id


# ---- burn, host path --------------------------------------------------------------------------------------------------------------------------
def _field(x0, y0, w, h, value=1, index=0):
    """A w x h metre rectangle whose top-left corner lies x0 metres right of and y0 metres below the grid's origin."""
    X, Y = GRID[0] + x0, GRID[1] - y0
    return P.Feature(index, value, [np.array([(X, Y), (X + w, Y), (X + w, Y - h), (X, Y - h)])])


def _burn(feats, shape=(4, 5), **kw):
    return P.burn(feats, shape, GRID, 32636, src_crs=32636, dtype=kw.pop("dtype", "int8"), **kw)


def test_a_field_smaller_than_a_pixel_is_burned_only_with_all_touched():
    field = _field(50.0, 48.0, 20.0, 25.0)  # 20 m x 25 m between the centres at 45 / 75 m: it contains none
    stats = {}
    assert not _burn([field], stats=stats).any() and stats["outside"] == 1 and stats["pixels_written"] == 0
    stats = {}
    got = _burn([field], stats=stats, all_touched=True)
    assert got.dtype == np.int8 and _pixels(got == 1) == [(1, 1), (1, 2), (2, 1), (2, 2)] and got.sum() == 4
    assert stats["outside"] == 0 and stats["passes"] == 1 and stats["pixels_written"] == 4
    inside = _field(62.0, 62.0, 10.0, 10.0)  # strictly inside pixel (2, 2), short of its centre at 75 m
    assert _pixels(_burn([inside], all_touched=True) == 1) == [(2, 2)] and not _burn([inside]).any()


def test_last_feature_wins_and_the_labelled_area_follows_the_rule():
    a, b = _field(50.0, 48.0, 20.0, 25.0, 3, 0), _field(65.0, 50.0, 20.0, 5.0, 7, 1)  # both touch pixel (1, 2)
    got = _burn([a, b], all_touched=True)
    assert got[1, 2] == 7 and got[1, 1] == 3 and got[2, 1] == 3 and got[2, 2] == 3 and _burn([b, a], all_touched=True)[1, 2] == 3
    reg = _burn([a, b], dtype="float32", all_touched=True)
    assert reg.dtype == np.float32 and reg[1, 2] == 7.0 and np.isnan(reg[0, 0]) and np.nansum(reg) == 3.0 * 3 + 7.0
    # the labelled area is burned first, by the same rule: its touched pixels become background, the rest stays ignore
    area = [_field(35.0, 35.0, 50.0, 50.0)]  # holds the centres of pixels (1..2, 1..2), touches the ring around them... up to 85 m: (2, 2)
    off = _burn([a], labelled_area=area)
    on = _burn([a], labelled_area=area, all_touched=True)
    assert _pixels(off == 0) == [(1, 1), (1, 2), (2, 1), (2, 2)] and (off == -1).sum() == 16 and not (off == 3).any()
    assert _pixels(on == 3) == [(1, 1), (1, 2), (2, 1), (2, 2)] and (on == -1).sum() == 20 - 4 and not (on == 0).any()
    wide = _burn([a], labelled_area=[_field(25.0, 35.0, 50.0, 50.0)], all_touched=True)  # from 25 m: it touches column 0 as well
    assert _pixels(wide == 0) == [(1, 0), (2, 0)] and _pixels(wide == 3) == [(1, 1), (1, 2), (2, 1), (2, 2)]


def test_the_flag_off_writes_the_bytes_of_the_existing_path():
    H, W, zones = AR.cases()["random_23x41"]
    items = [(z % 100, np.ascontiguousarray(ZR.edges_of([rings])[0])) for z, rings in enumerate(zones)]
    base, s0 = P.burn_fixed(np.zeros((H, W), dtype=np.int8), items, {}), {}
    off = P.burn_fixed(np.zeros((H, W), dtype=np.int8), items, s0, all_touched=False)
    assert off.tobytes() == base.tobytes() and s0["passes"] == 1
    # and on: the last zone that contains or touches a pixel
    full = AR.twin_masks("random_23x41")
    want = np.zeros((H, W), dtype=np.int8)
    for z in range(len(zones)):
        want[full[z]] = z % 100
    s1 = {}
    on = P.burn_fixed(np.zeros((H, W), dtype=np.int8), items, s1, all_touched=True)
    assert np.array_equal(on, want) and s1["pixels_written"] == int(full.any(axis=0).sum()) and not np.array_equal(on, off)
    assert P._rect(items[0][1], H, W) == P._rect(items[0][1], H, W, False)
    tiny = np.array(ZR.edges_of([AR.cases()["hand_8x9"][2][11]])[0])
    assert P._rect(tiny, 8, 9) is None and P._rect(tiny, 8, 9, True) == (1, 5, 1, 1)  # the rectangle bounds the touched pixels too


# ---- options ------------------------------------------------------------------------------------------------------------------------------------
def test_option_parsing(tmp_path):
    from instageo_amd import tiff
    from instageo_amd.config import load_config

    base = ["mode=create_polygon_labels", "polygon_labels.features=a.geojson", "polygon_labels.output_directory=out", "polygon_labels.date=d"]
    assert "all_touched" not in P.polygon_labels_options(load_config("config", base))  # off: the keywords are those of before
    assert "all_touched" not in P.polygon_labels_options(load_config("config", base + ["+polygon_labels.all_touched=false"]))
    assert P.polygon_labels_options(load_config("config", base + ["+polygon_labels.all_touched=true"]))["all_touched"] is True
    for bad in ("1", "maybe", "None"):
        with pytest.raises(ValueError, match="polygon_labels.all_touched must be true or false"):
            P.polygon_labels_options(load_config("config", base + [f"+polygon_labels.all_touched={bad}"]))
    with pytest.raises(ValueError, match="all_touched must be true or false"):
        P.create_polygon_labels("a.geojson", str(tmp_path), date="d", all_touched=1)
    raster = str(tmp_path / "r.tif")
    tiff.write(raster, np.zeros((4, 5), dtype=np.float32), None)
    zfile = str(tmp_path / "z.geojson")
    with open(zfile, "w") as f:
        json.dump({"type": "FeatureCollection", "features": [
            {"type": "Feature", "properties": {}, "geometry": {"type": "Polygon", "coordinates": [[[1, 1], [2, 1], [2, 2], [1, 1]]]}}]}, f)
    cfg = lambda **k: {"mode": "zonal_stats", "zonal_stats": dict(raster=raster, zones=zfile, **k)}  # noqa: E731
    assert zonal.zonal_stats_options(cfg())["all_touched"] is False and zonal.zonal_stats_options(cfg(all_touched=True))["all_touched"] is True
    assert "all_touched" in zonal.OPTIONAL_KEYS and "all_touched" in P.OPTIONAL_KEYS
    for bad in (1, "true", None):
        with pytest.raises(ValueError, match="zonal_stats.all_touched must be true or false"):
            zonal.zonal_stats_options(cfg(all_touched=bad))
    assert load_config("config", ["+zonal_stats.all_touched=true"])["zonal_stats"]["all_touched"] is True


# ---- header, library, custom ops ------------------------------------------------------------------------------------------------------------
def test_header_states_the_rule():
    text = open(os.path.join(ROOT, "include", "instageo_hip.h")).read()
    block = [c for c in re.findall(r"/\*.*?\*/", text, flags=re.S) if "ig_zone_touch_rows:" in c]
    assert len(block) == 1
    block = " ".join(block[0].replace("\n *", " ").split())
    for phrase in ("Q = 256", "|X|, |Y| <= 2^29", "meets the OPEN square (256 c, 256 c + 256) x (256 r, 256 r + 256)", "centre is inside",
                   "floor(ymin / 256) <= r <= ceil(ymax / 256) - 1", "floor(lo / 256) <= c <= ceil(hi / 256) - 1", "atomic OR",
                   "m[c] ^ m[c - 1]", "Nothing is clamped ONTO column 0", "has not been verified"):
        assert phrase in block, phrase
    for n in NAMES:
        assert re.search(r"\bint %s\(" % n, text) and n + ":" in block


def test_entry_points_exported_and_validated_without_gpu(built_lib):
    assert set(NAMES) <= set(built_lib.declared_symbols()) and len(built_lib.declared_symbols()) == 125
    lib = built_lib.load()
    err = built_lib.last_error
    one, two, odd = ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(4100)

    rows = lib.ig_zone_touch_rows
    assert rows(None, one, 4, 8, None) == -1 and "null pointer" in err()
    assert rows(one, None, 4, 8, None) == -1 and "null pointer" in err()
    assert rows(odd, one, 4, 8, None) == -1 and "aligned" in err()
    assert rows(one, one, -1, 8, None) == -1 and rows(one, one, 2**31, 8, None) == -1 and "2^31 - 1" in err()
    assert rows(one, one, 4, -1, None) == -1 and "H" in err()
    assert rows(None, None, 0, 8, None) == 0  # E = 0

    touch = lib.ig_zone_touch
    for k in range(4):
        a = [one] * 4
        a[k] = None
        assert touch(*a, 4, 9, 8, 8, None) == -1 and "null pointer" in err()
    for k in (0, 2, 3):
        a = [one] * 4
        a[k] = odd
        assert touch(*a, 4, 9, 8, 8, None) == -1 and "aligned" in err()
    assert touch(one, one, one, one, 4, -1, 8, 8, None) == -1 and touch(one, one, one, one, 4, 2**38 + 1, 8, 8, None) == -1 and "2^38" in err()
    assert touch(one, one, one, one, 4, 9, 65536, 32768, None) == -1 and "2^31" in err()
    assert touch(None, None, None, None, 0, 9, 8, 8, None) == 0 and touch(None, None, None, None, 4, 0, 8, 8, None) == 0
    assert touch(None, None, None, None, 4, 9, 0, 8, None) == 0 and touch(None, None, None, None, 4, 9, 8, 0, None) == 0

    merge = lib.ig_zone_touch_merge
    assert merge(None, one, 8, 8, None) == -1 and "null pointer" in err()
    assert merge(one, None, 8, 8, None) == -1 and "null pointer" in err()
    assert merge(odd, one, 8, 8, None) == -1 and "aligned" in err() and merge(one, odd, 8, 8, None) == -1 and "aligned" in err()
    assert merge(one, one, 8, 8, None) == -1 and "two canvases" in err()
    assert merge(one, two, 65536, 32768, None) == -1 and "2^31" in err() and merge(one, two, -1, 8, None) == -1
    assert merge(None, None, 0, 8, None) == 0 and merge(None, None, 8, 0, None) == 0


def test_generated_custom_ops_follow_the_header():
    from instageo_amd import torch_ops

    raw = torch_ops.register()
    assert {n[3:] for n in NAMES} <= set(raw)
    assert "Tensor? edges" in raw["zone_touch_rows"] and "Tensor(a!)? rows" in raw["zone_touch_rows"]
    assert "Tensor? first" in raw["zone_touch"] and "Tensor(a!)? touch" in raw["zone_touch"] and "int T" in raw["zone_touch"]
    assert "Tensor(a!)? canvas" in raw["zone_touch_merge"] and "Tensor? touch" in raw["zone_touch_merge"]


def test_empty_inputs_need_no_device():
    import torch

    none = np.zeros((0, 4), dtype=np.int32), np.zeros(0, dtype=np.int32)
    assert not zonal.zone_masks(*none, 70, 5, 7, "cpu", all_touched=True).any()
    assert zonal.zone_counts(torch.zeros((0, 7), dtype=torch.int8), *ZR.edges_of([[ZR.rect(0, 0, 1, 1)]]), 1, 2, all_touched=True).tolist() == [[0, 0, 0]]
    assert zonal.touch_spans(none[0], 5, 7)[0].shape == (0,) and not zonal.touched_mask(none[0], 5, 7).any()
