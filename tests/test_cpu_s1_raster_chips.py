"""Sentinel-1 chips on label grids without a GPU: the host path of ``s1_raster_chips.warp_cut`` against the sequential twin
(tests/s1_raster_chips_reference.py), the refusals of ``check_warp``, the identity with ``s1_chips.cut`` on an exact lattice,
``create_s1_raster_chips`` file to file, the config section, the CLI, and the chains polygon labels -> chips and speckle filter -> chips.

Every case is one the twin reports free of ties (asserted before anything is compared), so every comparison is ``array_equal`` on the bit
patterns of all elements and all counts."""
import ctypes
import json
import os

import numpy as np
import pytest

import polygon_labels_reference as PR
import s1_chips_reference as VR
import s1_raster_chips_reference as XR
from instageo_amd import crs, polygon_labels, s1_chips, s1_filter, tiff
from instageo_amd import s1_raster_chips as M
from test_cpu_s1_chips import FX, FY, ITEMS, TILE_ID, _profile, built_lib, write_stack  # noqa: F401  (built_lib is a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "instageo-e2e-geospatial-ml_amd")
WR = VR.WR
S = 16


# ---- host path == twin -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", XR.CASES)
def test_warp_cut_host_path_equals_the_twin(name):
    """S in {8, 64, 80}, (T, C) in {(1, 1), (3, 2)}; label grids in the scenes' zone with a finer and a coarser pixel, in EPSG:4326 and
    3857, in the next zone, over a southern stack; chips inside, over each edge, outside, on grids that are not finite or flat; slices in
    either order, scenes of two zones in one date; int8 and float32 labels, valid_bit 0 / 1 / 2, K 0 / 8, no labels; a clip."""
    want = XR.twin(name)
    assert want[6] == 0
    k = XR.case(name)
    got = M.warp_cut(k["planes"], **XR.product_args(k))
    assert len(got) == 6 and all(XR.same_bits(g, w) for g, w in zip(got, want[:6]))
    assert got[0].dtype == np.float32 and got[1].dtype == np.int32 and got[2].dtype == np.uint8


def test_the_cases_cover_what_they_claim():
    k, w = XR.case("affine_s64_t3c2"), XR.twin("affine_s64_t3c2")
    words = w[0].view(np.uint32)
    for special in VR.SPECIAL[4:]:  # -0.0, the denormals and the infinities are copied
        assert (words == special).any()
    assert not np.isnan(w[0]).any() and not (w[0] == VR.SRC_NODATA).any()  # NaN and src_nodata never are
    for dead in (3, 4):  # the grid that is not finite and the chip far outside
        assert w[1][dead] == 0 and (w[0][dead] == -1).all() and not w[2][dead].any()
    assert set(np.unique(w[2]).tolist()) == {0, 2, 3} and 0 < w[1][1] < w[1][0]
    assert np.isnan(k["labels"]).any() and not np.isnan(w[3]).any() and (w[3] == -1).any()
    a, b = XR.twin("slices"), XR.twin("slices_swapped")
    assert not np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))  # the order of the slices matters where both are present
    # vv and vh of one pixel come from different slices: where exactly one band of the first slice has a hole, the swapped order differs
    # in that band alone
    differ = a[0][:, 0:2].view(np.uint32) != b[0][:, 0:2].view(np.uint32)
    assert (differ[:, 0] & ~differ[:, 1]).any() and (differ[:, 1] & ~differ[:, 0]).any()
    h = XR.twin("affine_s80_t3c2")
    lab = XR.case("affine_s80_t3c2")["labels"]
    assert (lab == 100).any() and h[5].shape == (6, 8) and h[5].sum() < h[4].sum()  # labels outside [0, K) are valid but not counted
    assert XR.twin("affine_s8_t1c1")[3] is None and XR.twin("affine_s8_t3c2")[5] is None
    z = XR.case("south")
    assert z["date_scenes"] == [1, 2] and tuple(z["scenes"][1][0]) != tuple(z["scenes"][2][0])  # two zones within one date


def test_check_warp_refuses_what_the_header_refuses():
    k = XR.case("affine_s8_t1c1")
    ok = XR.product_args(k)
    n = len(k["dst_grids"])
    i8 = np.zeros((n, 8, 8), dtype=np.int8)
    for change, what in ((dict(chip_size=0), "chip_size"), (dict(chip_size=2**15 + 1), "chip_size"), (dict(date_scenes=[0, 1]), "at least one scene"),
                         (dict(date_scenes=[2]), "need 2 coordinate systems"), (dict(date_scenes=[]), "date_scenes"),
                         (dict(scene_grid=[(0.0, 0.0, 0.0, 10.0)]), "scene grid"), (dict(scene_size=[(0, 5)]), "1 <= H \\* W"),
                         (dict(starts=[-1]), "inside the packed buffer"), (dict(starts=[1]), "inside the packed buffer"),
                         (dict(no_data_value=float("nan")), "no_data_value"), (dict(src_nodata=float("nan")), "src_nodata"),
                         (dict(clip=(1.0, 0.0)), "clip"), (dict(clip=(0.0,)), "clip"), (dict(dst_grids=[(0.0, 0.0, 1.0)]), "dst_grids is \\(n, 4\\)"),
                         (dict(dst_crs=(1.0, 2.0)), "five doubles"), (dict(label_strategy="all"), "label_strategy"),
                         (dict(num_classes=8), "needs labels"), (dict(labels=i8, num_classes=129), "0 <= K <= 128"),
                         (dict(labels=i8[:, :4]), "labels must be"), (dict(labels=i8.astype(np.int16)), "int8 \\(seg\\) or float32"),
                         (dict(labels=i8.astype(np.float32), num_classes=8), "needs int8 labels")):
        with pytest.raises(ValueError, match=what):
            M.warp_cut(k["planes"], **{**ok, **change})
    scenes33 = dict(starts=[0] * 33, scene_crs=[VR.U36] * 33, scene_grid=[(0.0, 0.0, 1.0, 1.0)] * 33, scene_size=[(1, 1)] * 33)
    with pytest.raises(ValueError, match="at most 32"):
        M.check_warp(10, **scenes33, date_scenes=[2] * 16 + [1], dst_crs=VR.U36, dst_grids=[], S=8, no_data_value=-1, src_nodata=None, clip=None,
                     labels_shape=None, labels_dtype=None, valid_bit=0, K=0)
    with pytest.raises(ValueError, match="dates"):
        M.check_warp(10, **scenes33, date_scenes=[1] * 33, dst_crs=VR.U36, dst_grids=[], S=8, no_data_value=-1, src_nodata=None, clip=None,
                     labels_shape=None, labels_dtype=None, valid_bit=0, K=0)
    one = dict(starts=[0, 0], scene_crs=[VR.U36], scene_grid=[(0.0, 0.0, 1.0, 1.0)], scene_size=[(1, 1)], date_scenes=[1], dst_crs=VR.U36,
               no_data_value=-1, src_nodata=None, clip=None, labels_shape=None, labels_dtype=None, K=0)
    with pytest.raises(ValueError, match="valid_values is int32"):
        M.check_warp(10, **one, dst_grids=[], S=2**15, valid_bit=0)
    with pytest.raises(ValueError, match="beyond 2\\^40"):
        M.check_warp(10, **one, dst_grids=np.zeros((2**12, 4)), S=2**14, valid_bit=0)
    with pytest.raises(ValueError, match="valid_bit"):
        M.check_warp(10, **one, dst_grids=[], S=8, valid_bit=3)
    with pytest.raises(ValueError, match="float32"):
        M.warp_cut(k["planes"].astype(np.float64), **ok)
    none = M.warp_cut(k["planes"], **{**ok, "dst_grids": np.zeros((0, 4))})
    assert none[0].shape == (0, 1, 8, 8) and none[1].shape == (0,) and none[3] is None
    none = M.warp_cut(k["planes"], **{**ok, "dst_grids": np.zeros((0, 4)), "labels": i8[:0], "num_classes": 8})
    assert none[3].shape == (0, 8, 8) and none[4].shape == (0,) and none[5].shape == (0, 8)


# ---- the identity with s1_chips.cut ----------------------------------------------------------------------------------------------------------
def exact_lattice():
    """A stack whose arithmetic is exact in float64 (integer coordinates, integer pixel sizes): three dates, a corner per date, two slices
    on the second, and label grids that are windows of the stack lattice -> (planes, the scene arguments, the stack grid, origins)."""
    grid = (600000.0, 4400000.0, 10.0, 10.0)
    corners = [(-3, -5), (20, 11), (20 + 30, 11), (7, -20)]
    sizes = [(70, 61), (40, 53), (45, 53), (66, 77)]
    rng = np.random.default_rng(3)
    planes = []
    for h, w in sizes:
        for _ in range(2):
            a = rng.gamma(2.0, 0.05, size=(h, w)).astype(np.float32).view(np.uint32)
            pick = rng.random((h, w)) < 0.2
            a[pick] = VR.SPECIAL[rng.integers(0, len(VR.SPECIAL), size=int(pick.sum()))]
            planes.append(a.view(np.float32).reshape(-1))
    starts = np.concatenate([[0], np.cumsum([p.size for p in planes])[:-1]]).astype(np.int64)
    scene = dict(starts=starts, scene_crs=[32636] * 4, scene_grid=[(grid[0] + 10.0 * c, grid[1] - 10.0 * r, 10.0, 10.0) for r, c in corners],
                 scene_size=sizes, date_scenes=[1, 2, 1])
    origins = [(0, 0), (-10, -12), (35, 20), (60, 50), (500, 500)]
    return np.concatenate(planes), scene, grid, origins


def test_windows_of_the_stack_lattice_give_the_chips_of_s1_chips_cut():
    planes, scene, grid, origins = exact_lattice()
    for size in (24, 65):
        want = s1_chips.cut(planes, **scene, dst_crs=32636, dst_grid=grid, origins=origins, chip_size=size, src_nodata=-32768.0)
        windows = [(grid[0] + 10.0 * c, grid[1] - 10.0 * r, 10.0, 10.0) for r, c in origins]
        got = M.warp_cut(planes, **scene, dst_crs=32636, dst_grids=windows, chip_size=size, src_nodata=-32768.0)
        assert all(VR.same_bits(g, w) for g, w in zip(got[:3], want)) and got[3] is None
        assert want[1][0] > 0 and want[1][4] == 0 and 0 < want[1][1] < want[1][0]


# ---- create_s1_raster_chips, file to file ------------------------------------------------------------------------------------------------------
def write_labels(root, dtype=np.int16):
    """Label rasters of 16 x 16 pixels on the lattice of test_cpu_s1_chips.write_stack (10 m, UTM 36; chip (x, y) of that file's lattice):
    (0, 0) and (1, 2) with classes, (2, 0) where every scene is NaN, (1, 0) all -1, one of 8 x 8 pixels, one far away, (1, 3) for another
    run's id, and (0, 2) moved by (3.3, -7.1) m -> (the records table, {name: (x, y)})."""
    os.makedirs(root, exist_ok=True)
    rng = np.random.default_rng(11)
    cells = {"label_a_20220525.tif": (0, 0), "label_b_20220525.tif": (1, 2), "label_nan_20220525.tif": (2, 0), "label_blank_20220525.tif": (1, 0),
             "label_small_20220525.tif": (0, 0), "label_far_20220525.tif": (500, 500), "label_other_20220525.tif": (1, 3),
             "mask_moved_20220525.tif": (0, 2)}
    for name, (x, y) in cells.items():
        side = 8 if "small" in name else S
        a = rng.integers(0, 4, size=(side, side)).astype(dtype)
        a[0, :3] = -1
        if "blank" in name:
            a[:] = -1
        dx, dy = (3.3, -7.1) if "moved" in name else (0.0, 0.0)
        tiff.write(os.path.join(root, name), a, _profile(32636, FX + 10.0 * S * x + dx, FY - 10.0 * S * y + dy))
    table = {"label_filename": list(cells), "date": ["2022-05-25"] * len(cells),
             "mgrs_tile_id": [None if "other" not in n else "S1A_IW_20220101T000000_000001_00000A_rtc" for n in cells]}
    return table, cells


KW = dict(chip_size=S, src_crs=32636, spatial_resolution=10.0, src_nodata=-32768.0)
SCENE_KW = dict(scene_crs=[32636] * 3, scene_grid=[(FX, FY, 10.0, 10.0), (FX, FY, 10.0, 10.0), (FX, FY - 320.0, 10.0, 10.0)],
                scene_size=[(64, 48), (40, 48), (32, 48)], date_scenes=[1, 2], dst_crs=32636, chip_size=S, src_nodata=-32768.0)


def test_create_s1_raster_chips_file_to_file(tmp_path):
    scenes, flat, starts, _ = write_stack(str(tmp_path / "in"))
    table, cells = write_labels(str(tmp_path / "labels"))
    out = str(tmp_path / "out")
    names, segs = M.create_s1_raster_chips(scenes, table, str(tmp_path / "labels"), out, masking_strategy="any", **KW)
    kept = ["label_a_20220525.tif", "label_b_20220525.tif", "mask_moved_20220525.tif"]
    stem = lambda n: os.path.splitext(n)[0] + "_" + TILE_ID + ".tif"  # noqa: E731
    assert segs == [stem(n) for n in kept] and names == [stem(n).replace("mask", "merged").replace("label", "chip") for n in kept]
    assert sorted(os.listdir(os.path.join(out, "chips"))) == sorted(names) and sorted(os.listdir(os.path.join(out, "seg_maps"))) == sorted(segs)
    stats = json.load(open(os.path.join(out, "s1_raster_chips_stats.json")))
    assert stats["records"] == 8 and stats["kept"] == 3
    assert stats["dropped"] == {"other_tile": 1, "existing": 0, "invalid_shape": 1, "outside_tile": 1, "no_valid_values": 1, "no_valid_labels": 1}
    assert open(os.path.join(out, "chips_dataset.csv")).read().split() == ["Input,Label"] + [f"chips/{c},seg_maps/{s}" for c, s in zip(names, segs)]
    hist = np.zeros(4, dtype=np.int64)
    for n, chip, seg in zip(kept, names, segs):
        x, y = cells[n]
        lab, lprof = tiff.read(os.path.join(str(tmp_path / "labels"), n))
        # snap=True: the lattice of multiples of 10 m, which for the moved raster is the cell its top-left corner lies in: (0, 2) again
        want = s1_chips.cut(flat, starts, **{k: v for k, v in SCENE_KW.items()}, dst_grid=(FX, FY, 10.0, 10.0), origins=[(y * S, x * S)])
        a, prof = tiff.read(os.path.join(out, "chips", chip))
        assert a.dtype == np.float32 and a.shape == (4, S, S) and VR.same_bits(a, want[0][0]) and want[1][0] > 0
        m, mprof = tiff.read(os.path.join(out, "seg_maps", seg))
        assert m.dtype == np.int8 and VR.same_bits(m[0], np.where((want[2][0] & 1) == 0, -1, lab[0]).astype(np.int8))
        for p in (prof, mprof):  # the georeferencing is the label raster's, moved or not
            assert p["tags"][33922] == lprof["tags"][33922] and p["tags"][33550] == lprof["tags"][33550] and p["tags"][34735] == lprof["tags"][34735]
        hist += np.bincount(m[m >= 0], minlength=4)
    assert stats["class_histogram"] == hist.tolist() and hist.min() > 0
    # again: every file exists, nothing is rewritten
    again = M.create_s1_raster_chips(scenes, table, str(tmp_path / "labels"), out, masking_strategy="any", **KW)
    assert again == (names, segs) and json.load(open(os.path.join(out, "s1_raster_chips_stats.json")))["dropped"]["existing"] == 3
    # snap=False: the moved raster's own grid; no qa_check: nothing is dropped for its values or labels, the labels are not masked
    out2 = str(tmp_path / "own")
    names2, segs2 = M.create_s1_raster_chips(scenes, table, str(tmp_path / "labels"), out2, snap=False, qa_check=False, tile_id=TILE_ID, **KW)
    assert len(names2) == 5 and json.load(open(os.path.join(out2, "s1_raster_chips_stats.json")))["dropped"]["no_valid_values"] == 0
    own = (FX + 3.3, FY - 10.0 * S * 2 - 7.1, 10.0, 10.0)
    want = M.warp_cut(flat, starts, **{k: v for k, v in SCENE_KW.items()}, dst_grids=[own])
    moved = tiff.read(os.path.join(out2, "chips", "merged_moved_20220525_" + TILE_ID + ".tif"))[0]
    snapped = tiff.read(os.path.join(out, "chips", "merged_moved_20220525_" + TILE_ID + ".tif"))[0]
    assert VR.same_bits(moved, want[0][0]) and not VR.same_bits(moved, snapped)
    lab = tiff.read(os.path.join(str(tmp_path / "labels"), "label_blank_20220525.tif"))[0]
    assert VR.same_bits(tiff.read(os.path.join(out2, "seg_maps", "label_blank_20220525_" + TILE_ID + ".tif"))[0], lab.astype(np.int8))
    # reg: float32 label maps, NaN -> -1, no histogram
    regs = str(tmp_path / "reg_labels")
    table_r, _ = write_labels(regs, np.float32)
    a = tiff.read(os.path.join(regs, "label_a_20220525.tif"))[0]
    a[0, 5, 5] = np.nan
    tiff.write(os.path.join(regs, "label_a_20220525.tif"), a[0], _profile(32636, FX, FY))
    out3 = str(tmp_path / "reg")
    _, segs3 = M.create_s1_raster_chips(scenes, table_r, regs, out3, task_type="reg", **KW)
    m = tiff.read(os.path.join(out3, "seg_maps", segs3[0]))[0]
    assert m.dtype == np.float32 and m[0, 5, 5] == -1 and "class_histogram" not in json.load(open(os.path.join(out3, "s1_raster_chips_stats.json")))
    for bad, what in ((dict(scenes=[]), "list of dates"), (dict(masking_strategy="all"), "masking_strategy"), (dict(task_type="cls"), "task_type"),
                      (dict(device="cpu"), "device"), (dict(bands=[]), "bands"), (dict(spatial_resolution=0), "spatial_resolution"),
                      (dict(scenes=[[["a_vv.tif", "a_vh.tif"]]]), "not a Sentinel-1 item name"), (dict(raster_path=None), "raster_path"),
                      (dict(is_bbox_feature=True), "bbox_feature_path"), (dict(src_crs=32637), "EPSG:32636")):
        with pytest.raises(ValueError, match=what):
            M.create_s1_raster_chips(**{**dict(scenes=scenes, records=table, raster_path=str(tmp_path / "labels"),
                                               output_directory=str(tmp_path / "bad")), **KW, **bad})


def test_create_s1_raster_chips_over_bounding_boxes(tmp_path):
    scenes, flat, starts, _ = write_stack(str(tmp_path / "in"))
    lon, lat = (float(v) for v in WR.to_lonlat(VR.U36, FX + 20.0, FY - 500.0))
    res = 0.0001
    boxes = str(tmp_path / "boxes.json")
    json.dump([[lon, lat, lon + 1.5 * S * res, lat + 0.5 * S * res]], open(boxes, "w"))  # whole chips from the lower left corner: 2 x 1
    out = str(tmp_path / "out")
    names, segs = M.create_s1_raster_chips(scenes, None, None, out, chip_size=S, spatial_resolution=res, src_nodata=-32768.0, is_bbox_feature=True,
                                           bbox_feature_path=boxes)
    assert names == [f"chip_x{x}_y0_20220525_{TILE_ID}.tif" for x in (0, 1)] and segs == [None, None]
    assert not os.path.exists(os.path.join(out, "seg_maps")) and open(os.path.join(out, "chips_dataset.csv")).read().splitlines()[0] == "Input"
    from instageo_amd import raster_chips

    for x, name in enumerate(names):
        a, prof = tiff.read(os.path.join(out, "chips", name))
        b = raster_chips.grid_polygons(json.load(open(boxes)), "20220525", S, res)[x]["bounds"]
        grid = raster_chips.snapped_grid(b, res)
        want = M.warp_cut(flat, starts, **{**SCENE_KW, "dst_crs": 4326}, dst_grids=[grid])
        assert a.dtype == np.float32 and VR.same_bits(a, want[0][0]) and want[1][0] > 0
        assert prof["tags"][33922][1][3:5] == grid[:2] and prof["tags"][34735] == crs.geokeys(4326)[34735]
    named = M.create_s1_raster_chips(scenes, None, None, str(tmp_path / "named"), chip_size=S, spatial_resolution=res, src_nodata=-32768.0,
                                     is_bbox_feature=True, bbox_feature_path=boxes, date="2022-01-01", tile_id="mine")[0]
    assert named[0] == "chip_x0_y0_2022-01-01_mine.tif"


# ---- the config section and the CLI ----------------------------------------------------------------------------------------------------------
def test_config_section_and_its_refusals():
    from instageo_amd import run
    from instageo_amd.config import DEFAULTS, load_config

    assert run.PREP_MODES["create_s1_raster_chips"] == "s1_raster_chips"
    assert set(DEFAULTS["s1_raster_chips"]) == set(M.CONFIG_KEYS) and len(M.CONFIG_KEYS) == 19
    cfg = load_config("config", [])
    opts = M.s1_raster_chips_options(cfg)  # nothing required outside the mode
    assert opts["scenes"] is None and opts["chip_size"] == 256 and opts["no_data_value"] == -1.0 and opts["bands"] == ["vv", "vh"]
    assert opts["snap"] is True and opts["qa_check"] is True and opts["task_type"] == "seg" and opts["src_crs"] == 4326
    with pytest.raises(ValueError, match="needs s1_raster_chips.scenes"):
        M.s1_raster_chips_options(load_config("config", ["mode=create_s1_raster_chips"]))
    base = ["mode=create_s1_raster_chips", "s1_raster_chips.scenes=[[[a_vv.tif,a_vh.tif]],[[b_vv.tif,b_vh.tif],[c_vv.tif,c_vh.tif]]]",
            "s1_raster_chips.output_directory=out"]
    full = base + ["s1_raster_chips.records_file=r.csv", "s1_raster_chips.raster_path=labels"]
    opts = M.s1_raster_chips_options(load_config("config", full + ["s1_raster_chips.chip_size=64", "s1_raster_chips.masking_strategy=any",
                                                                    "s1_raster_chips.task_type=reg", "s1_raster_chips.src_crs=3857",
                                                                    "s1_raster_chips.spatial_resolution=10", "s1_raster_chips.no_data_value=-9999",
                                                                    "s1_raster_chips.src_nodata=-32768", "s1_raster_chips.clip=[-40,10]",
                                                                    "s1_raster_chips.snap=false", "s1_raster_chips.qa_check=false",
                                                                    "s1_raster_chips.tile_id=mine", "s1_raster_chips.date=2022-05-25"]))
    assert opts == dict(scenes=[[["a_vv.tif", "a_vh.tif"]], [["b_vv.tif", "b_vh.tif"], ["c_vv.tif", "c_vh.tif"]]], records="r.csv", raster_path="labels",
                        output_directory="out", chip_size=64, bands=["vv", "vh"], masking_strategy="any", src_crs=3857, spatial_resolution=10.0,
                        qa_check=False, task_type="reg", is_bbox_feature=False, bbox_feature_path=None, date="2022-05-25", snap=False,
                        no_data_value=-9999.0, src_nodata=-32768.0, clip=(-40.0, 10.0), tile_id="mine")
    for ov, what in (("s1_raster_chips.chip_size=0", "chip_size"), ("s1_raster_chips.chip_size=40000", "chip_size"), ("s1_raster_chips.bands=[]", "bands"),
                     ("s1_raster_chips.masking_strategy=all", "masking_strategy"), ("s1_raster_chips.task_type=cls", "task_type"),
                     ("s1_raster_chips.src_crs=1234", "EPSG"), ("s1_raster_chips.spatial_resolution=0", "spatial_resolution"),
                     ("s1_raster_chips.no_data_value=.nan", "no_data_value"), ("s1_raster_chips.src_nodata=x", "src_nodata"),
                     ("s1_raster_chips.clip=[1,0]", "clip"), ("s1_raster_chips.scenes=a.tif", "scenes"), ("s1_raster_chips.bands=[vv]", "scenes"),
                     ("s1_raster_chips.snap=2", "snap"), ("s1_raster_chips.qa_check=3", "qa_check"), ("s1_raster_chips.is_bbox_feature=1", "is_bbox_feature"),
                     ("s1_raster_chips.is_bbox_feature=true", "needs s1_raster_chips.bbox_feature_path"),
                     ("s1_raster_chips.output_directory=None", "needs s1_raster_chips.scenes")):
        with pytest.raises(ValueError, match=what):
            M.s1_raster_chips_options(load_config("config", full + [ov]))
    with pytest.raises(ValueError, match="records_file and s1_raster_chips.raster_path"):
        M.s1_raster_chips_options(load_config("config", base))
    with pytest.raises(KeyError):
        load_config("config", ["s1_raster_chips.chipsize=3"])
    with pytest.raises(ValueError, match="unknown s1_raster_chips keys"):
        M.s1_raster_chips_options({"s1_raster_chips": {"chipsize": 3}})


def test_the_cli_prints_its_json_line(tmp_path, capsys):
    import pandas as pd

    scenes, _, _, _ = write_stack(str(tmp_path / "in"))
    table, _ = write_labels(str(tmp_path / "labels"))
    records = str(tmp_path / "records.csv")
    pd.DataFrame(table).to_csv(records, index=False)
    out = str(tmp_path / "out")
    text = "[" + ",".join("[" + ",".join("[" + ",".join(s) + "]" for s in d) + "]" for d in scenes) + "]"
    argv = [f"s1_raster_chips.scenes={text}", f"s1_raster_chips.chip_size={S}", f"s1_raster_chips.records_file={records}",
            f"s1_raster_chips.raster_path={tmp_path / 'labels'}", f"s1_raster_chips.output_directory={out}", "s1_raster_chips.src_nodata=-32768",
            "s1_raster_chips.src_crs=32636", "s1_raster_chips.spatial_resolution=10", "s1_raster_chips.masking_strategy=any"]
    assert M.main(argv) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == {"create_s1_raster_chips": {"chips": 3, "seg_maps": 3, "output_directory": out}}
    from instageo_amd import run

    assert run.main(["mode=create_s1_raster_chips"] + argv) == 0  # through run.py: every file exists and is listed again
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == line


# ---- polygon labels -> chips, speckle filter -> chips -------------------------------------------------------------------------------------------
def test_polygon_labels_feed_the_s1_raster_chips(tmp_path):
    """A GeoJSON of two flood polygons burned by create_polygon_labels on the 10 m lattice of the stack; its records.csv and rasters go
    into create_s1_raster_chips.  A pixel inside a polygon and inside a scene carries the polygon's value and the scene's bits."""
    scenes, flat, starts, _ = write_stack(str(tmp_path / "in"))
    at = lambda c, r: [FX + 10.0 * c, FY - 10.0 * r]  # noqa: E731
    quad = lambda c0, r0, c1, r1: [at(c0, r0), at(c1, r0), at(c1, r1), at(c0, r1), at(c0, r0)]  # noqa: E731
    path = PR.write_geojson(tmp_path / "flood.geojson", [({"kind": "water"}, [[quad(2.0, 1.0, 11.0, 9.0)]]), ({"kind": "flood"}, [[quad(18.0, 34.0, 30.0, 46.0)]])])
    lab_dir = str(tmp_path / "lab")
    made = polygon_labels.create_polygon_labels(path, lab_dir, crs=32636, src_crs=32636, spatial_resolution=10.0, chip_size=S, value_property="kind",
                                                class_map={"water": 1, "flood": 2}, date="2022-05-25")
    assert made == ["label_x0_y0_2022-05-25.tif", "label_x1_y2_2022-05-25.tif"]
    out = str(tmp_path / "out")
    names, segs = M.create_s1_raster_chips(scenes, os.path.join(lab_dir, "records.csv"), os.path.join(lab_dir, "labels"), out, **KW)
    assert names == [f"chip_x0_y0_2022-05-25_{TILE_ID}.tif", f"chip_x1_y2_2022-05-25_{TILE_ID}.tif"]
    first = flat[starts[0] : starts[0] + 64 * 48].reshape(64, 48)  # vv of the first date
    for (cx, cy), (row, col), value, chip, seg in (((0, 0), (4, 3), 1, names[0], segs[0]), ((1, 2), (40, 21), 2, names[1], segs[1])):
        a, m = tiff.read(os.path.join(out, "chips", chip))[0], tiff.read(os.path.join(out, "seg_maps", seg))[0]
        gx, gy = tiff.read(os.path.join(lab_dir, "labels", made[cx]))[1]["tags"][33922][1][3:5]  # the label grid starts at the polygons' bounds
        r, c = int((gy - (FY - 10.0 * row - 5.0)) // 10.0), int((FX + 10.0 * col + 5.0 - gx) // 10.0)
        assert 0 <= r < S and 0 <= c < S and first[row, col] == 0.5 and a[0, r, c].view(np.uint32) == first[row, col].view(np.uint32) and m[0, r, c] == value
        assert (m == 0).any()  # the background stays a class of its own


def test_filtered_db_scenes_are_accepted_as_scenes(tmp_path):
    scenes, _, _, _ = write_stack(str(tmp_path / "in"))
    table, _ = write_labels(str(tmp_path / "labels"))
    filtered = s1_filter.filter_s1(scenes, str(tmp_path / "db"), method="boxcar", window=3, scale="db", src_nodata=-32768.0)
    out = str(tmp_path / "out")
    names, segs = M.create_s1_raster_chips(filtered, table, str(tmp_path / "labels"), out, chip_size=S, src_crs=32636, spatial_resolution=10.0,
                                           no_data_value=-9999.0)
    assert len(names) == 3 and names[0].endswith(TILE_ID + ".tif")
    a = tiff.read(os.path.join(out, "chips", names[0]))[0]
    db = tiff.read(filtered[0][0][0])[0][0][:S, :S]
    assert VR.same_bits(a[0], np.where(np.isnan(db), np.float32(-9999.0), db)) and (a[0] < -1).any() and not (a == -1).all()


# ---- the entry point ---------------------------------------------------------------------------------------------------------------------------
def test_entry_point_exported_and_validated_without_gpu(built_lib):  # noqa: F811
    """IG_REQUIRE rejects bad arguments before any launch, and n = 0 returns before a pointer is looked at."""
    assert "ig_s1_chip_warp" in built_lib.declared_symbols()
    lib, err = built_lib.load(), built_lib.last_error
    one, odd, four = ctypes.c_void_p(4096), ctypes.c_void_p(4098), ctypes.c_void_p(4100)
    ok = dict(planes=one, starts=one, scene_crs=one, scene_grid=one, scene_size=one, N=4, first_bits=0b1011, dst_crs=one, dst_grids=one, n=1, T=3,
              C=2, S=256, no_data=-1.0, has_src_nodata=1, src_nodata=-32768.0, clip=0, clip_lo=0.0, clip_hi=0.0, labels=one, elem_size=1,
              valid_bit=2, K=8, chips=one, valid_values=one, validity=one, maps=one, valid_labels=one, hist=one, stream=None)

    def warp(**kw):
        return lib.ig_s1_chip_warp(*{**ok, **kw}.values())

    nan = float("nan")
    for kw, what in ((dict(n=-1), "n >= 0"), (dict(T=0), "dates"), (dict(T=33, N=32, first_bits=2**32 - 1), "dates"), (dict(C=0), "C >= 1"),
                     (dict(N=0), "scenes in all"), (dict(N=33), "scenes in all"), (dict(first_bits=0b1010), "at least one scene"),
                     (dict(first_bits=0b0011), "at least one scene"), (dict(N=2, first_bits=0b111), "at least one scene"),
                     (dict(S=0), "1 <= S <= 2^15"), (dict(S=2**15 + 1), "1 <= S <= 2^15"), (dict(no_data=nan), "no_data must not be NaN"),
                     (dict(src_nodata=nan), "src_nodata must not be NaN"), (dict(has_src_nodata=2), "has_src_nodata"), (dict(clip=2), "clip must be"),
                     (dict(clip=1, clip_lo=1.0, clip_hi=0.5), "clip_lo <= clip_hi"), (dict(clip=1, clip_lo=nan), "clip_lo <= clip_hi"),
                     (dict(elem_size=2), "elem_size"), (dict(valid_bit=3), "valid_bit"), (dict(K=129), "histogram cells"),
                     (dict(K=8, elem_size=4), "needs int8 labels"), (dict(S=2**15), "valid_values is int32"), (dict(n=2**31 - 1), "2^40"),
                     (dict(planes=None), "null pointer"), (dict(starts=None), "null pointer"), (dict(scene_crs=None), "null pointer"),
                     (dict(scene_grid=None), "null pointer"), (dict(scene_size=None), "null pointer"), (dict(dst_crs=None), "null pointer"),
                     (dict(dst_grids=None), "null pointer"), (dict(chips=None), "null pointer"), (dict(valid_values=None), "null pointer"),
                     (dict(maps=None), "maps, valid_labels"), (dict(valid_labels=None), "maps, valid_labels"), (dict(hist=None), "labels, hist"),
                     (dict(labels=None), "labels, hist"), (dict(planes=odd), "4-byte aligned"), (dict(chips=odd), "4-byte aligned"),
                     (dict(scene_size=odd), "4-byte aligned"), (dict(valid_values=odd), "4-byte aligned"), (dict(valid_labels=odd), "4-byte aligned"),
                     (dict(hist=odd), "4-byte aligned"), (dict(elem_size=4, K=0, labels=odd), "to their elements"),
                     (dict(elem_size=4, K=0, maps=odd), "to their elements"), (dict(starts=four), "8-byte aligned"), (dict(scene_crs=four), "8-byte aligned"),
                     (dict(scene_grid=four), "8-byte aligned"), (dict(dst_crs=four), "8-byte aligned"), (dict(dst_grids=four), "8-byte aligned")):
        assert warp(**kw) == -1 and what in err(), (kw, err())
    nothing = dict(planes=None, starts=None, scene_crs=None, scene_grid=None, scene_size=None, dst_crs=None, dst_grids=None, labels=None, chips=None,
                   valid_values=None, validity=None, maps=None, valid_labels=None, hist=None)
    assert warp(n=0, **nothing) == 0 and warp(N=32, T=32, first_bits=2**32 - 1, C=1, S=8, n=0) == 0
    with pytest.raises(built_lib.HipLibraryError, match="1 <= N <= 32 scenes in all"):
        built_lib.call("ig_s1_chip_warp", *{**ok, "N": 40}.values())


def test_prototype_is_declared_and_the_custom_op_follows_it():
    import re

    from instageo_amd import _lib, torch_ops

    text = open(os.path.join(ROOT, "include", "instageo_hip.h")).read()
    assert re.search(r"\bint ig_s1_chip_warp\(", text)
    assert "s1_raster_chips.hip" in open(os.path.join(PKG, "csrc", "Makefile")).read()
    s = torch_ops.register()["s1_chip_warp"]
    for piece in ("Tensor? planes", "Tensor? starts", "Tensor? scene_crs", "Tensor? scene_grid", "Tensor? scene_size", "int N", "int first_bits",
                  "Tensor? dst_crs", "Tensor? dst_grids", "float no_data", "float src_nodata", "Tensor? labels", "int valid_bit", "chips",
                  "valid_values", "validity", "maps", "valid_labels", "hist"):
        assert piece in s, (piece, s)
    assert "stream" not in s
    proto = _lib.parse_header()["ig_s1_chip_warp"][1]
    assert len(proto) == 30 and proto[6] == "unsigned" and proto[13] == "float"
