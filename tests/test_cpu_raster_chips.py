"""Chips cut against label rasters, host side (no GPU): the numpy host path of instageo_amd/raster_chips.py against the sequential twin
(tests/raster_chips_reference.py) bit for bit on cases the twin reports free of ties, the same-grid case against chips.cut, the grid of
boxes and the snap rule by hand, the names, create_raster_chips file to file with its skip / drop reasons, the config keys and the mode
through run.py, the argument checks of ig_chip_warp through the library, and the generated custom op."""
import ctypes
import json
import os

import numpy as np
import pytest

import raster_chips_reference as RR
import warp_reference as WR
from instageo_amd import chips, crs, tiff
from instageo_amd import raster_chips as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "instageo-e2e-geospatial-ml_amd")


@pytest.fixture(scope="module")
def built_lib():
    import subprocess

    from instageo_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j4"], check=True)
    return _lib


def inputs(geometry, setting):
    sc, sg, dc, dg, S = RR.GEOMETRY[geometry]
    T, C, strategy, with_mask, clip, nd = RR.SETTINGS[setting]
    tile, fmask = RR.tile_of(T, C)
    return tile, fmask if with_mask else None, dict(src_crs=sc, src_grid=sg, dst_crs=dc, dst_grids=dg, chip_size=S, dates=T, mask=RR.BITS,
                                                   strategy=strategy, no_data_value=nd, clip=clip)


def same(got, want):
    for g, w in zip(got, want):
        assert (g is None and w is None) or (g.dtype == w.dtype and np.array_equal(g.view(f"u{g.itemsize}"), w.view(f"u{w.itemsize}")))


# ---- host path == twin -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry,setting", RR.PAIRS)
def test_host_path_equals_the_twin(geometry, setting):
    want = RR.twin(geometry, setting)
    assert want[6] == 0, "the case has pixels within 1e-6 of a source pixel edge: choose other offsets"
    tile, fmask, kw = inputs(geometry, setting)
    same(R.warp_cut(tile, fmask, **kw)[:3], want[:3])


def test_chips_that_leave_the_tile():
    chips_, valid, plane = RR.twin("edges_s32", 3)[:3]  # no_data -9999, no clip
    tile, fmask = RR.tile_of(3, 2)
    assert valid[5] == 0 and (chips_[5] == -9999).all() and not plane[5].any()  # wholly outside
    inside = np.zeros((32, 32), dtype=bool)
    inside[10:, 7:] = True  # chip 0 starts at tile pixel (-10, -7)
    assert (chips_[0][:, ~inside] == -9999).all() and not plane[0][~inside].any()
    assert valid[0] == (chips_[0][:, inside] != -9999).sum() > 0
    got = R.warp_cut(tile, fmask, RR.U36, RR.SRC_GRID, RR.U36, [RR.at(-10, -7)], 32, mask=0, no_data_value=-9999)[0]
    assert np.array_equal(got[0][:, 10:, 7:], tile[:, :22, :25])


@pytest.mark.parametrize("S", [32, 65])
def test_same_grid_equals_the_chip_cut(S):
    origins = [(0, 0), (100 - S, 90 - S), (7, 3)]
    grids = [RR.at(r, c) for r, c in origins]
    for T, C in ((1, 1), (3, 2)):
        tile, fmask = RR.tile_of(T, C)
        for strategy in ("each", "any"):
            for fm in (fmask, None):
                for clip in (None, (0, 10000)):
                    for nd in (0, -9999):
                        want = chips.cut(tile, fm, origins, S, dates=T, mask=RR.BITS, strategy=strategy, no_data_value=nd, clip=clip)
                        got = R.warp_cut(tile, fm, RR.U36, RR.SRC_GRID, RR.U36, grids, S, dates=T, mask=RR.BITS, strategy=strategy,
                                         no_data_value=nd, clip=clip)
                        same(got[:3], want)
                        assert got[3] is got[4] is got[5] is None


LABEL_CASES = [("edges_s65", 0, np.int8, 8), ("edges_s65", 1, np.float32, 0), ("geographic_s65", 0, np.int8, 8), ("edges_s32", 3, np.float32, 0)]


def label_case(geometry, setting, dtype, K, strat):
    """-> (labels, the twin's outputs) for one of LABEL_CASES under a label strategy."""
    sc, sg, dc, dg, S = RR.GEOMETRY[geometry]
    T, C, strategy, with_mask, clip, nd = RR.SETTINGS[setting]
    tile, fmask = RR.tile_of(T, C)
    labels = RR.label_maps(len(dg), S, dtype, seed=S + K)
    return labels, RR.cut(tile, fmask if with_mask else None, sc, sg, dc, dg, S, T, RR.BITS, strategy, nd, clip, labels, chips.VALID_BITS[strat], K)


@pytest.mark.parametrize("geometry,setting,dtype,K", LABEL_CASES)
def test_label_maps_equal_the_twin(geometry, setting, dtype, K):
    tile, fmask, kw = inputs(geometry, setting)
    for strat in (None, "any", "each"):
        labels, want = label_case(geometry, setting, dtype, K, strat)
        assert want[6] == 0
        got = R.warp_cut(tile, fmask, labels=labels, label_strategy=strat, num_classes=K, **kw)
        same(got, want[:6])
        assert (got[3] == -1).sum() >= (labels == -1).sum() + (np.isnan(labels).sum() if dtype == np.float32 else 0)
    if K:
        assert want[5].sum() < want[4].sum()  # values >= K are valid labels outside the histogram


def test_an_unusable_destination_grid_gives_a_no_data_chip():
    tile, fmask = RR.tile_of(3, 2)
    grids = [RR.at(3, 3), (RR.X0, RR.Y0, 0.0, 30.0), (np.nan, RR.Y0, 30.0, 30.0), (RR.X0, RR.Y0, 30.0, np.inf)]
    got = R.warp_cut(tile, fmask, RR.U36, RR.SRC_GRID, RR.U36, grids, 16, mask=RR.BITS, no_data_value=-9999)
    assert got[1][0] > 0 and got[1][1:].tolist() == [0, 0, 0] and (got[0][1:] == -9999).all() and not got[2][1:].any()
    with pytest.raises(ValueError, match="src_grid"):
        R.warp_cut(tile, fmask, RR.U36, (RR.X0, RR.Y0, -30.0, 30.0), RR.U36, grids, 16)


def test_host_argument_checks():
    tile = np.zeros((2, 20, 30), dtype=np.int16)
    ok = dict(tile=tile, fmask=None, src_crs=RR.U36, src_grid=RR.SRC_GRID, dst_crs=4326, dst_grids=[(34.0, 40.6, 1e-4, 1e-4)], chip_size=8)
    assert R.warp_cut(**ok)[0].shape == (1, 2, 8, 8)
    lab8 = np.zeros((1, 8, 8), dtype=np.int8)
    for change, what in ((dict(chip_size=0), "chip_size"), (dict(chip_size=2**15 + 1), "chip_size"), (dict(dates=3), "dates"),
                         (dict(fmask=np.zeros((1, 20, 29), dtype=np.uint8)), "fmask must be"), (dict(strategy="all"), "masking_strategy"),
                         (dict(no_data_value=40000), "no_data_value"), (dict(clip=(5, 1)), "clip"), (dict(tile=tile.astype(np.int32)), "int16"),
                         (dict(dst_grids=[(1.0, 2.0, 3.0)]), "dst_grids"), (dict(dst_crs=(1.0, 2.0)), "five doubles"),
                         (dict(dst_crs=1234), "EPSG"), (dict(labels=lab8.astype(np.int16)), "int8"), (dict(labels=lab8[:, :7]), "labels must be"),
                         (dict(labels=lab8.astype(np.float32), num_classes=4), "needs int8"), (dict(num_classes=4), "needs labels"),
                         (dict(labels=lab8, num_classes=129), "histogram"), (dict(labels=lab8, label_strategy="all"), "label_strategy")):
        with pytest.raises(ValueError, match=what):
            R.warp_cut(**{**ok, **change})
    with pytest.raises(ValueError, match="valid_values is int32"):
        R.check_warp((18, 100, 100), None, RR.U36, RR.SRC_GRID, RR.U36, [RR.SRC_GRID], 11000, 3, 0, "each", 0, None, None, None, 0, 0)
    with pytest.raises(ValueError, match="2\\^31 - 1"):
        R.check_warp((1, 50000, 50000), None, RR.U36, RR.SRC_GRID, RR.U36, [RR.SRC_GRID], 8, 1, 0, "each", 0, None, None, None, 0, 0)


# ---- boxes, the snap rule, names -----------------------------------------------------------------------------------------------------------
def test_grid_polygons_by_hand():
    rec = R.grid_polygons([[10.0, 20.0, 10.9, 20.4]], "2022-06-08", 4, 0.1)
    # x: ceil(0.9 / 0.4) = 3 chips, y: ceil(0.4 / 0.4) = 1 chip; x outer, y inner
    assert [r["label_filename"] for r in rec] == [f"label_x{x}_y0_2022-06-08.tif" for x in range(3)]
    assert all(r["date"] == "2022-06-08" for r in rec)
    for x, r in enumerate(rec):
        assert r["bounds"] == pytest.approx((10.0 + 0.4 * x, 20.0, 10.0 + 0.4 * x + 0.3, 20.3), abs=1e-12)
    two = R.grid_polygons([[0.0, 0.0, 0.5, 0.9]], "d", 4, 0.1)
    assert [r["label_filename"] for r in two] == ["label_x0_y0_d.tif", "label_x0_y1_d.tif", "label_x0_y2_d.tif", "label_x1_y0_d.tif",
                                                  "label_x1_y1_d.tif", "label_x1_y2_d.tif"]
    assert two[1]["bounds"] == pytest.approx((0.0, 0.4, 0.3, 0.7), abs=1e-12)


def test_grid_polygons_give_up_one_chip_at_180_and_90():
    # chips of 8 x 0.125 = 1 degree.  178.5 + 2 chips = 180.5 > 180: one chip; 89.5 + 1 chip > 90: none at all; reaching 180 exactly is allowed
    assert [r["label_filename"] for r in R.grid_polygons([[178.5, 10.0, 180.0, 10.5]], "d", 8, 0.125)] == ["label_x0_y0_d.tif"]
    assert R.grid_polygons([[10.0, 89.5, 10.5, 90.0]], "d", 8, 0.125) == []
    assert len(R.complete_chips_coords(178.5, 180.0, 0.125, 8, 180)) == 8 and len(R.complete_chips_coords(178.0, 180.0, 0.125, 8, 180)) == 16
    assert [r["bounds"] for r in R.grid_polygons([[178.0, 88.0, 180.0, 89.0]], "d", 8, 0.125)] == [(178.0, 88.0, 178.875, 88.875), (179.0, 88.0, 179.875, 88.875)]
    assert len(R.grid_polygons([[-180.0, -90.0, -179.5, -89.5]], "d", 5, 0.1)) == 1  # the lower bounds are not a limit


def test_snap_rule_on_multiples_and_negative_coordinates():
    assert R.snapped_grid((60.0, 0.0, 0.0, 90.0), 30.0) == (60.0, 90.0, 30.0, 30.0)  # exact multiples stay
    assert R.snapped_grid((61.0, 0.0, 0.0, 89.0), 30.0) == (60.0, 90.0, 30.0, 30.0)
    assert R.snapped_grid((-61.0, 0.0, 0.0, -89.0), 30.0) == (-90.0, -60.0, 30.0, 30.0)  # floor and ceil, not truncation
    assert R.snapped_grid((-60.0, 0.0, 0.0, -90.0), 30.0) == (-60.0, -90.0, 30.0, 30.0)
    g = R.snapped_grid((34.00001, 0.0, 0.0, 40.59999), 0.00027)
    assert g[0] == 0.00027 * np.floor(34.00001 / 0.00027) <= 34.00001 < g[0] + 0.00027 and g[1] - 0.00027 < 40.59999 <= g[1]


def test_names_follow_the_reference():
    assert R.chip_names("mask_0012.tif", "T36TVK") == ("merged_0012_T36TVK.tif", "mask_0012_T36TVK.tif")
    assert R.chip_names("sub/label_x3_y4_2022-06-08.tif", "36TVK") == ("chip_x3_y4_2022-06-08_36TVK.tif", "label_x3_y4_2022-06-08_36TVK.tif")
    assert R.chip_names("flood_7.tif", "T1") == ("flood_7_T1.tif", "flood_7_T1.tif")
    assert R.mgrs_of("/a/HLS.S30.T36TVK.2022145T072619.v2.0.B02.tif") == "T36TVK"
    with pytest.raises(ValueError, match="HLS file name"):
        R.mgrs_of("tile.tif")


# ---- create_raster_chips, file to file -------------------------------------------------------------------------------------------------------
STAMPS = ("2022145T072619", "2022161T072619", "2022177T072619")
BANDS = ("B02", "B03")
S, RES = 32, 0.00027
CLOUD, HOLE = (slice(36, 84), slice(0, 34)), (slice(50, 62), slice(46, 58))  # tile windows masked on every date
KEEP_A, KEEP_B, CLOUDY, EMPTY, FAR = (3, 3), (3, 33), (44, 4), (40, 40), (400, 400)  # the top-left tile pixel of each label raster


def write_granule(root, task="seg"):
    """A granule of 3 dates x 2 bands in UTM 36 N and six label rasters in EPSG:4326 -> (tile, fmask, tile files, Fmask files, records
    CSV, raster folder).  mask_keep_a / mask_keep_b are kept, mask_cloudy lies under cloud on every date, mask_empty has labels only where
    the chip is masked on every date, mask_shape is 31 x 32 and mask_far misses the tile."""
    tiles, rasters = os.path.join(root, "tiles"), os.path.join(root, "labels")
    os.makedirs(tiles, exist_ok=True)
    os.makedirs(rasters, exist_ok=True)
    T, C = len(STAMPS), len(BANDS)
    tile, fmask = RR.tile_of(T, C)
    tile, fmask = np.maximum(tile, 0), fmask.copy()
    fmask[:, :36] &= np.uint8(~RR.BITS & 255)  # the rows of the two chips that are kept: clear on every date
    for win in (CLOUD, HOLE):
        fmask[(slice(None),) + win] = 2
    tags = {33550: (12, (RR.PX, RR.PX, 0.0)), 33922: (12, (0.0, 0.0, 0.0, RR.X0, RR.Y0, 0.0)), **crs.geokeys(32636)}
    files, fmasks = [], []
    for t, stamp in enumerate(STAMPS):
        for c, band in enumerate(BANDS):
            files.append(os.path.join(tiles, f"HLS.S30.T36TVK.{stamp}.v2.0.{band}.tif"))
            tiff.write(files[-1], tile[t * C + c], {"tags": tags, "nodata": None})
        fmasks.append(os.path.join(tiles, f"HLS.S30.T36TVK.{stamp}.v2.0.Fmask.tif"))
        tiff.write(fmasks[-1], fmask[t], {"tags": tags, "nodata": None})
    rng = np.random.default_rng(5)
    rows = []
    for name, (r0, c0), shape in (("keep_a", KEEP_A, (S, S)), ("keep_b", KEEP_B, (S, S)), ("cloudy", CLOUDY, (S, S)), ("empty", EMPTY, (S, S)),
                                  ("shape", KEEP_A, (S - 1, S)), ("far", FAR, (S, S))):
        lon, lat = (float(v) for v in WR.to_lonlat(RR.U36, RR.X0 + RR.PX * c0, RR.Y0 - RR.PX * r0))
        lon, lat = lon + 0.31 * RES, lat - 0.43 * RES  # off the lattice of multiples of RES
        lab = rng.integers(0, 3, size=shape).astype(np.int8)
        lab[rng.random(shape) < 0.2] = -1
        if name == "empty":  # labels only where the source pixel lies in the window masked on every date
            u, v = WR.coords(WR.GEOGRAPHIC, R.snapped_grid((lon, 0.0, 0.0, lat), RES), shape, RR.U36, RR.SRC_GRID)
            hole = (np.floor(v) >= HOLE[0].start + 1) & (np.floor(v) < HOLE[0].stop - 1) & (np.floor(u) >= HOLE[1].start + 1) & (np.floor(u) < HOLE[1].stop - 1)
            assert hole.sum() > 20
            lab = np.where(hole, lab, -1).astype(np.int8)
        ltags = {33550: (12, (RES, RES, 0.0)), 33922: (12, (0.0, 0.0, 0.0, lon, lat, 0.0)), **crs.geokeys(4326)}
        tiff.write(os.path.join(rasters, f"mask_{name}.tif"), lab if task == "seg" else lab.astype(np.float32) * np.float32(0.5), {"tags": ltags, "nodata": None})
        rows.append(f"mask_{name}.tif,2022-05-25")
    records = os.path.join(root, "records.csv")
    with open(records, "w") as f:
        f.write("label_filename,date\n" + "\n".join(rows) + "\n")
    return tile, fmask, files, fmasks, records, rasters


KW = dict(chip_size=S, mask_types=["cloud", "water"], masking_strategy="each", src_crs=4326, spatial_resolution=RES)
KEPT = (["merged_keep_a_T36TVK.tif", "merged_keep_b_T36TVK.tif"], ["mask_keep_a_T36TVK.tif", "mask_keep_b_T36TVK.tif"])
REASONS = {"other_tile": 0, "existing": 0, "invalid_shape": 1, "outside_tile": 1, "no_valid_values": 1, "no_valid_labels": 1}


def test_create_raster_chips_end_to_end(tmp_path):
    from instageo_amd.dataloader import get_valid_filepaths

    tile, fmask, files, fmasks, records, rasters = write_granule(str(tmp_path))
    out = str(tmp_path / "out")
    names, segs = R.create_raster_chips(files, fmasks, records, rasters, out, **KW)
    assert (names, segs) == KEPT
    stats = json.load(open(os.path.join(out, "raster_chips_stats.json")))
    assert stats["records"] == 6 and stats["kept"] == 2 and stats["dropped"] == REASONS
    bits = chips.mask_bits(KW["mask_types"])
    maps = []
    for name, seg, raster in zip(names, segs, ("mask_keep_a.tif", "mask_keep_b.tif")):
        lab, lprof = tiff.read(os.path.join(rasters, raster))
        own = (lprof["tags"][33922][1][3], lprof["tags"][33922][1][4], RES, RES)
        grid = R.snapped_grid((own[0], 0.0, 0.0, own[1]), RES)
        assert grid[0] <= own[0] < grid[0] + RES and grid != own
        want = RR.cut(tile, fmask, RR.U36, RR.SRC_GRID, WR.GEOGRAPHIC, [grid], S, 3, bits, "each", 0, (0, 10000), lab, 2, 0)
        assert want[6] == 0 and want[1][0] > 0
        a, prof = tiff.read(os.path.join(out, "chips", name))
        assert a.dtype == np.uint16 and np.array_equal(a, want[0][0].astype(np.uint16)) and a.max() <= 10000
        m, mprof = tiff.read(os.path.join(out, "seg_maps", seg))
        assert m.dtype == np.int8 and np.array_equal(m[0], want[3][0])
        for p in (prof, mprof):  # the label raster's georeferencing, not the snapped grid's
            assert all(p["tags"][k] == lprof["tags"][k] for k in (33550, 33922, 34735))
        maps.append(m[0])
    hist = [int((np.stack(maps) == k).sum()) for k in range(3)]
    assert stats["class_histogram"] == hist and sum(hist) == int((np.stack(maps) != -1).sum())
    assert stats["class_weights"] == pytest.approx([sum(hist) / (3 * v) for v in hist])
    pairs = get_valid_filepaths(os.path.join(out, "chips_dataset.csv"), out, no_data_value=0, ignore_index=-1)
    assert [(os.path.basename(a), os.path.basename(b)) for a, b in pairs] == list(zip(*KEPT))
    # again: the pairs exist, are skipped and still listed; nothing is rewritten
    before = {n: os.path.getmtime(os.path.join(out, "chips", n)) for n in names}
    assert R.create_raster_chips(files, fmasks, records, rasters, out, **KW) == KEPT
    stats2 = json.load(open(os.path.join(out, "raster_chips_stats.json")))
    assert stats2["dropped"] == {**REASONS, "existing": 2} and stats2["kept"] == 0
    assert before == {n: os.path.getmtime(os.path.join(out, "chips", n)) for n in names}
    assert len(get_valid_filepaths(os.path.join(out, "chips_dataset.csv"), out, no_data_value=0, ignore_index=-1)) == 2


def test_without_qa_check_nothing_is_dropped_and_labels_are_not_masked(tmp_path):
    tile, fmask, files, fmasks, records, rasters = write_granule(str(tmp_path), task="reg")
    out = str(tmp_path / "out")
    names, segs = R.create_raster_chips(files, fmasks, records, rasters, out, qa_check=False, task_type="reg", snap=False, **KW)
    assert len(names) == 4 and segs[2:] == ["mask_cloudy_T36TVK.tif", "mask_empty_T36TVK.tif"]
    stats = json.load(open(os.path.join(out, "raster_chips_stats.json")))
    assert stats["dropped"] == {**REASONS, "no_valid_values": 0, "no_valid_labels": 0} and "class_histogram" not in stats
    lab, lprof = tiff.read(os.path.join(rasters, "mask_cloudy.tif"))
    m, _ = tiff.read(os.path.join(out, "seg_maps", "mask_cloudy_T36TVK.tif"))
    assert m.dtype == np.float32 and np.array_equal(m, lab)
    assert not tiff.read(os.path.join(out, "chips", "merged_cloudy_T36TVK.tif"))[0].any()
    # snap=False: the label raster's own grid
    own = (lprof["tags"][33922][1][3], lprof["tags"][33922][1][4], RES, RES)
    lab_a, pa = tiff.read(os.path.join(rasters, "mask_keep_a.tif"))
    own = (pa["tags"][33922][1][3], pa["tags"][33922][1][4], RES, RES)
    want = RR.cut(tile, fmask, RR.U36, RR.SRC_GRID, WR.GEOGRAPHIC, [own], S, 3, chips.mask_bits(KW["mask_types"]), "each", 0, (0, 10000))
    assert want[6] == 0
    assert np.array_equal(tiff.read(os.path.join(out, "chips", "merged_keep_a_T36TVK.tif"))[0], want[0][0].astype(np.uint16))


def test_records_of_other_tiles_and_rasters_of_other_systems(tmp_path):
    tile, fmask, files, fmasks, records, rasters = write_granule(str(tmp_path))
    table = {"label_filename": ["mask_keep_a.tif", "mask_keep_b.tif", "mask_keep_a.tif"], "date": ["2022-05-25"] * 3,
             "mgrs_tile_id": ["36TVK", "36TVL", "T36TVK"]}
    names, segs = R.create_raster_chips(files, fmasks, table, rasters, str(tmp_path / "out"), **KW)
    assert names == ["merged_keep_a_36TVK.tif", "merged_keep_a_T36TVK.tif"] and segs == ["mask_keep_a_36TVK.tif", "mask_keep_a_T36TVK.tif"]
    assert json.load(open(tmp_path / "out" / "raster_chips_stats.json"))["dropped"]["other_tile"] == 1
    with pytest.raises(ValueError, match="EPSG:4326, src_crs is EPSG:3857"):
        R.create_raster_chips(files, fmasks, records, rasters, str(tmp_path / "o2"), **{**KW, "src_crs": 3857})
    with pytest.raises(ValueError, match="label_filename"):
        R.create_raster_chips(files, fmasks, {"date": ["2022-05-25"]}, rasters, str(tmp_path / "o3"), **KW)


def test_bbox_features_cut_chips_only(tmp_path):
    tile, fmask, files, fmasks, records, rasters = write_granule(str(tmp_path))
    lon0, lat0 = (float(v) for v in WR.to_lonlat(RR.U36, RR.X0 + RR.PX * 4, RR.Y0 - RR.PX * 34))  # the lower left corner of the box
    boxes = str(tmp_path / "boxes.json")
    json.dump([[lon0, lat0, lon0 + 2 * S * RES - 1e-9, lat0 + S * RES - 1e-9]], open(boxes, "w"))
    out = str(tmp_path / "out")
    kw = dict(KW, is_bbox_feature=True, bbox_feature_path=boxes, date="2022-06-08")
    names, segs = R.create_raster_chips(files, fmasks, None, None, out, **kw)
    assert names == ["chip_x0_y0_2022-06-08_T36TVK.tif", "chip_x1_y0_2022-06-08_T36TVK.tif"] and segs == [None, None]
    assert not os.path.exists(os.path.join(out, "seg_maps")) and open(os.path.join(out, "chips_dataset.csv")).read().splitlines()[0] == "Input"
    rec = R.grid_polygons(json.load(open(boxes)), "2022-06-08", S, RES)
    for name, r in zip(names, rec):
        grid = R.snapped_grid(r["bounds"], RES)
        want = RR.cut(tile, fmask, RR.U36, RR.SRC_GRID, WR.GEOGRAPHIC, [grid], S, 3, chips.mask_bits(KW["mask_types"]), "each", 0, (0, 10000))
        a, prof = tiff.read(os.path.join(out, "chips", name))
        assert want[6] == 0 and a.dtype == np.uint16 and np.array_equal(a, want[0][0].astype(np.uint16))
        assert prof["tags"][33922][1] == (0.0, 0.0, 0.0, grid[0], grid[1], 0.0) and prof["tags"][34735] == crs.geokeys(4326)[34735]
    assert R.create_raster_chips(files, fmasks, None, None, out, **kw) == (names, segs)  # existing chips are skipped and listed
    assert json.load(open(os.path.join(out, "raster_chips_stats.json")))["dropped"]["existing"] == 2


# ---- config and modes --------------------------------------------------------------------------------------------------------------------------
def test_config_carries_the_raster_chips_keys():
    from instageo_amd.config import DEFAULTS, load_config

    assert set(DEFAULTS["raster_chips"]) == set(R.CONFIG_KEYS)
    d = DEFAULTS["raster_chips"]
    assert (d["chip_size"], d["mask_types"], d["masking_strategy"], d["src_crs"], d["spatial_resolution"], d["qa_check"], d["task_type"],
            d["is_bbox_feature"], d["snap"]) == (256, [], "each", 4326, 0.0002694945852358564, True, "seg", False, True)
    assert all(d[k] is None for k in ("tiles", "fmasks", "records_file", "raster_path", "output_directory", "bbox_feature_path", "date"))
    opts = R.raster_chips_options(load_config("config", []))  # nothing required outside the mode
    assert opts["tile_files"] is None and opts["chip_size"] == 256 and opts["snap"] is True
    with pytest.raises(ValueError, match="needs raster_chips.tiles"):
        R.raster_chips_options(load_config("config", ["mode=create_raster_chips"]))
    base = ["mode=create_raster_chips", "raster_chips.tiles=[a.tif,b.tif]", "raster_chips.output_directory=out"]
    full = base + ["raster_chips.records_file=r.csv", "raster_chips.raster_path=labels"]
    opts = R.raster_chips_options(load_config("config", full + ["raster_chips.mask_types=[cloud]", "raster_chips.fmasks=[f.tif]", "raster_chips.snap=false",
                                                                "raster_chips.task_type=reg", "raster_chips.src_crs=32636", "raster_chips.spatial_resolution=30",
                                                                "raster_chips.qa_check=false", "raster_chips.date=2022-06-08"]))
    assert opts == dict(tile_files=["a.tif", "b.tif"], fmask_files=["f.tif"], records="r.csv", raster_path="labels", output_directory="out",
                        chip_size=256, mask_types=["cloud"], masking_strategy="each", src_crs=32636, spatial_resolution=30.0, qa_check=False,
                        task_type="reg", is_bbox_feature=False, bbox_feature_path=None, date="2022-06-08", snap=False)
    for ov, what in (("raster_chips.chip_size=0", "chip_size"), ("raster_chips.mask_types=[snow]", "unknown mask type"),
                     ("raster_chips.masking_strategy=all", "masking_strategy"), ("raster_chips.task_type=cls", "task_type"),
                     ("raster_chips.src_crs=1234", "EPSG"), ("raster_chips.spatial_resolution=0", "spatial_resolution"),
                     ("raster_chips.qa_check=maybe", "qa_check"), ("raster_chips.snap=1", "snap"), ("raster_chips.mask_types=[cloud]", "needs raster_chips.fmasks"),
                     ("raster_chips.is_bbox_feature=true", "bbox_feature_path")):
        with pytest.raises(ValueError, match=what):
            R.raster_chips_options(load_config("config", full + [ov]))
    with pytest.raises(ValueError, match="records_file"):
        R.raster_chips_options(load_config("config", base))
    with pytest.raises(ValueError, match="unknown raster_chips keys"):
        R.raster_chips_options({"raster_chips": {"chipsize": 3}})
    with pytest.raises(KeyError):
        load_config("config", ["raster_chips.chipsize=3"])
    assert load_config("config", [])["mode"] == "train" and "chip_size" in DEFAULTS["chips"]  # the chips.* keys are untouched


def test_mode_create_raster_chips_through_run_main_and_the_cleaner_takes_its_csv(tmp_path, capsys, monkeypatch):
    import torch

    from instageo_amd import run

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    tile, fmask, files, fmasks, records, rasters = write_granule(str(tmp_path))
    out = str(tmp_path / "out")
    assert run.main(["mode=create_raster_chips", f"raster_chips.tiles=[{','.join(files)}]", f"raster_chips.fmasks=[{','.join(fmasks)}]",
                     f"raster_chips.records_file={records}", f"raster_chips.raster_path={rasters}", f"raster_chips.output_directory={out}",
                     f"raster_chips.chip_size={S}", "raster_chips.mask_types=[cloud,water]", f"raster_chips.spatial_resolution={RES}"]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])["create_raster_chips"]
    assert line["chips"] == 2 and line["seg_maps"] == 2
    assert sorted(os.listdir(os.path.join(out, "chips"))) == KEPT[0] and sorted(os.listdir(os.path.join(out, "seg_maps"))) == KEPT[1]
    csv, clean_csv = os.path.join(out, "chips_dataset.csv"), os.path.join(out, "clean.csv")
    assert run.main(["mode=clean_chips", f"clean.chips_dataset_csv={csv}", f"clean.output_chips_dataset_csv={clean_csv}", "clean.drop_chips=true",
                     "clean.drop_chips_strategy=all", "clean.no_data_value=0", "clean.no_data_threshold=0.9"]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])["clean_chips"]
    assert line["rows_in"] == 2 and line["rows_out"] == 2
    assert R.main([f"raster_chips.tiles=[{','.join(files)}]", f"raster_chips.fmasks=[{','.join(fmasks)}]", f"raster_chips.records_file={records}",
                   f"raster_chips.raster_path={rasters}", f"raster_chips.output_directory={out}", f"raster_chips.chip_size={S}",
                   "raster_chips.mask_types=[cloud,water]", f"raster_chips.spatial_resolution={RES}"]) == 0  # python -m instageo_amd.raster_chips


# ---- the library -----------------------------------------------------------------------------------------------------------------------------
def test_entry_point_exported_and_validated_without_gpu(built_lib):
    """IG_REQUIRE rejects every bad argument before any launch, and n = 0 returns before a pointer is looked at."""
    assert "ig_chip_warp" in built_lib.declared_symbols()
    lib, err = built_lib.load(), built_lib.last_error
    one = ctypes.c_void_p(4096)
    ok = dict(tile=one, fmask=one, src_crs=one, src_grid=one, dst_crs=one, dst_grids=one, n=1, T=3, C=6, H=3660, W=3660, S=256, mask_bits=46,
              strategy=0, no_data=0, clip=0, clip_lo=0, clip_hi=0, labels=one, elem_size=1, valid_bit=1, K=4, chips=one, valid_values=one,
              validity=one, maps=one, valid_labels=one, hist=one, stream=None)

    def call(**kw):
        return lib.ig_chip_warp(*{**ok, **kw}.values())

    for kw, what in ((dict(n=-1), "n >= 0"), (dict(T=0), "dates"), (dict(T=33), "dates"), (dict(C=0), "C >= 1"), (dict(H=0), "H >= 1"),
                     (dict(S=0), "chip side"), (dict(S=(1 << 15) + 1), "chip side"), (dict(H=46341, W=46341), "H * W"),
                     (dict(n=1 << 20), "2^40"), (dict(S=1 << 15, T=1, C=2), "valid_values is int32"),
                     (dict(mask_bits=256), "mask_bits"), (dict(strategy=2), "strategy"), (dict(no_data=40000), "no_data"),
                     (dict(no_data=-40000), "no_data"), (dict(clip=2), "clip"), (dict(clip=1, clip_lo=5, clip_hi=1), "clip range"),
                     (dict(clip=1, clip_hi=40000), "clip range"), (dict(clip=1, clip_lo=-40000), "clip range"), (dict(elem_size=2), "elem_size"),
                     (dict(elem_size=2, labels=None, K=0), "elem_size"), (dict(valid_bit=3), "valid_bit"), (dict(K=-1), "histogram"),
                     (dict(K=129), "histogram"), (dict(K=4, elem_size=4), "int8 labels"), (dict(K=4, labels=None), "null pointer"),
                     (dict(hist=None), "null pointer"), (dict(tile=None), "null pointer"), (dict(dst_grids=None), "null pointer"),
                     (dict(src_crs=None), "null pointer"), (dict(chips=None), "null pointer"), (dict(valid_values=None), "null pointer"),
                     (dict(maps=None), "null pointer"), (dict(valid_labels=None), "null pointer"), (dict(tile=ctypes.c_void_p(4097)), "aligned"),
                     (dict(dst_grids=ctypes.c_void_p(4100)), "8-byte aligned"), (dict(valid_values=ctypes.c_void_p(4098)), "aligned"),
                     (dict(elem_size=4, K=0, maps=ctypes.c_void_p(4098)), "aligned")):
        assert call(**kw) == -1 and what in err(), (kw, err())
    assert call(n=0, tile=None, src_crs=None, src_grid=None, dst_crs=None, dst_grids=None, chips=None, valid_values=None, labels=None, maps=None,
                valid_labels=None, hist=None) == 0
    with pytest.raises(built_lib.HipLibraryError, match="strategy must be 0 each or 1 any"):
        built_lib.call("ig_chip_warp", *{**ok, "strategy": 7}.values())


def test_prototype_is_declared_and_the_custom_op_follows_it():
    import re

    from instageo_amd import torch_ops

    text = open(os.path.join(ROOT, "include", "instageo_hip.h")).read()
    assert re.search(r"\bint ig_chip_warp\(", text) and "raster_chips.hip" in open(os.path.join(PKG, "csrc", "Makefile")).read()
    s = torch_ops.register()["chip_warp"]
    assert all(p in s for p in ("Tensor? tile", "Tensor? fmask", "Tensor? dst_grids", "Tensor? labels", "Tensor(a!)? chips", "Tensor(d!)? maps",
                                "Tensor(f!)? hist", "int valid_bit", "int elem_size", "int K")) and "stream" not in s
