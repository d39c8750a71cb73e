"""Chips and label maps cut from HLS tiles, host side (no GPU): the Fmask decode, the numpy host path of instageo_amd/chips.py against the
sequential twin of the rule (tests/chips_reference.py) array for array, the label rule on hand-made points, the point geometry, create_chips
file to file, the argument checks of the two HIP entry points through the library, and the config keys of mode=create_chips."""
import ctypes
import itertools
import json
import os

import numpy as np
import pytest

import chips_reference as CR
from instageo_amd import chips, cog, crs, tiff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "instageo-e2e-geospatial-ml_amd")
X0, Y0, PX = 399960.0, 4500000.0, 30.0
TAGS = {33550: (12, (PX, PX, 0.0)), 33922: (12, (0.0, 0.0, 0.0, X0, Y0, 0.0)),
        34735: (3, (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 32613))}
PROFILE = {"tags": TAGS, "nodata": None}


@pytest.fixture(scope="module")
def built_lib():
    import subprocess

    from instageo_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j4"], check=True)
    return _lib


# ---- Fmask decode ----------------------------------------------------------------------------------------------------------------------------
def test_fmask_decode_reproduces_the_reference_table():
    v = CR.FMASK_TABLE["value"]
    assert [int(chips.decode_fmask_value(v, p)) for p in range(8)] == CR.FMASK_TABLE["bits"]
    assert [(v >> p) & 1 for p in range(8)] == CR.FMASK_TABLE["bits"]
    for v in range(256):
        for p in range(8):
            assert CR.decode_arithmetic(v, p) == (v >> p) & 1 == int(chips.decode_fmask_value(np.uint8(v), p))


def test_mask_bits_of_every_subset():
    names = list(CR.POSITIONS)
    assert chips.MASK_POSITIONS["HLS"] == CR.POSITIONS
    for k in range(len(names) + 1):
        for sub in itertools.combinations(names, k):
            assert chips.mask_bits(list(sub)) == sum(1 << CR.POSITIONS[s] for s in sub)
    assert chips.mask_bits([]) == 0 and chips.mask_bits(names) == 2 | 4 | 8 | 32
    with pytest.raises(ValueError, match="unknown mask type"):
        chips.mask_bits(["cloud", "snow"])
    with pytest.raises(ValueError, match="HLS only"):
        chips.mask_bits(["cloud"], data_source="S2")


# ---- host path == twin -----------------------------------------------------------------------------------------------------------------------
CUT_CASES = {
    "t3c2_70x75_s32": dict(T=3, C=2, H=70, W=75, S=32, origins=[(0, 0), (0, 32), (32, 0), (32, 32), (38, 43), (1, 3)], fully=(32, 0), clean=(0, 32)),
    "s64_130x131": dict(T=2, C=1, H=130, W=131, S=64, origins=[(0, 0), (64, 64), (66, 67)], fully=None, clean=None),
    "s65_130x131": dict(T=2, C=1, H=130, W=131, S=65, origins=[(0, 0), (65, 65), (65, 66), (3, 1)], fully=None, clean=None),
    # two block columns per chip (128 columns each), the second ragged, and nine block rows, the last ragged
    "s130_140x150": dict(T=1, C=2, H=140, W=150, S=130, origins=[(0, 0), (10, 20), (7, 3)], fully=None, clean=None),
    "t1c1": dict(T=1, C=1, H=40, W=41, S=17, origins=[(0, 0), (23, 24), (5, 7)], fully=None, clean=None),
}


def cut_case(name):
    k = CUT_CASES[name]
    tile, fmask = CR.make_tile(k["T"], k["C"], k["H"], k["W"], seed=len(name), fully_masked=k["fully"], untouched=k["clean"], S=k["S"])
    return k, tile, fmask


@pytest.mark.parametrize("name", list(CUT_CASES))
@pytest.mark.parametrize("strategy", ["each", "any"])
def test_cut_host_path_equals_the_twin(name, strategy):
    k, tile, fmask = cut_case(name)
    bits = chips.mask_bits(list(CR.POSITIONS))
    for fm, clip in ((fmask, None), (None, None), (fmask, (0, 10000)), (None, (100, 5000))):
        got = chips.cut(tile, fm, k["origins"], k["S"], dates=k["T"], mask=bits, strategy=strategy, clip=clip)
        want = CR.cut(tile, fm, k["origins"], k["S"], k["T"], bits, strategy, 0, clip)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and np.array_equal(g, w)
    if k["fully"] is not None:
        _, valid, plane = chips.cut(tile, fmask, k["origins"], k["S"], mask=bits, strategy=strategy)
        i, j = k["origins"].index(k["fully"]), k["origins"].index(k["clean"])
        assert valid[i] == 0 and not plane[i].any()
        assert np.array_equal(chips.cut(tile, fmask, [k["clean"]], k["S"], mask=bits, strategy=strategy)[0][0],
                              tile[:, k["clean"][0] : k["clean"][0] + k["S"], k["clean"][1] : k["clean"][1] + k["S"]])
        assert valid[j] > 0


def test_single_bits_and_nonzero_no_data():
    _, tile, fmask = cut_case("t3c2_70x75_s32")
    for name, pos in CR.POSITIONS.items():
        got = chips.cut(tile, fmask, [(38, 43)], 32, mask=[name], strategy="each", no_data_value=-9999)
        want = CR.cut(tile, fmask, [(38, 43)], 32, 3, 1 << pos, "each", -9999)
        assert all(np.array_equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("dtype,K", [(np.int16, 8), (np.float32, 0)])
@pytest.mark.parametrize("S,w,counts", [(32, 0, [0, 1, 7]), (32, 2, [5, 0, 9]), (64, 3, [300]), (65, 3, [40, 3])])
def test_label_host_path_equals_the_twin(dtype, K, S, w, counts):
    rng = np.random.default_rng(S + w)
    origins = [(3 * i, 5 * i) for i in range(len(counts))]
    ptr, pts, labels = CR.random_points(origins, S, counts, seed=S * 7 + w)
    labels = labels.astype(dtype) + (dtype(0.25) if dtype == np.float32 else dtype(0))
    validity = rng.integers(0, 4, size=(len(counts), S, S)).astype(np.uint8)
    for strat, bit in (("any", 1), ("each", 2), (None, 0)):
        got = chips.label_maps(origins, S, ptr, pts, labels, w, validity if strat else None, strat, "seg" if dtype == np.int16 else "reg", K)
        want = CR.label_maps(origins, S, ptr, pts, labels, w, validity, bit, K, dtype)
        assert got[0].dtype == dtype and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert (got[2] is None and want[2] is None) or np.array_equal(got[2], want[2])


# ---- the label rule by hand --------------------------------------------------------------------------------------------------------------------
def _maps(pts, labels, S=8, w=0, validity=None, task="seg", K=4, origin=(10, 20)):
    pts = np.array([(origin[0] + r, origin[1] + c, i) for r, c, i in pts], dtype=np.int32).reshape(-1, 3)
    return chips.label_maps([origin], S, [0, len(pts)], pts, np.asarray(labels), w, validity, "any", task, K)


def test_later_point_wins_where_windows_overlap():
    m, valid, hist = _maps([(3, 3, 0), (4, 4, 1)], [1, 2], w=1)  # 3 x 3 windows that share (3..4, 3..4)
    want = np.full((8, 8), -1, dtype=np.int16)
    want[2:5, 2:5] = 1
    want[3:6, 3:6] = 2
    assert np.array_equal(m[0], want) and valid[0] == 14 and hist[0].tolist() == [0, 5, 9, 0]
    # the order of the list does not matter: the original index decides
    m2, _, _ = _maps([(4, 4, 1), (3, 3, 0)], [1, 2], w=1)
    assert np.array_equal(m2[0], want)


def test_window_sizes_corner_clipping_and_two_points_in_one_pixel():
    m, valid, _ = _maps([(5, 5, 0)], [3], w=0)
    assert valid[0] == 1 and m[0, 5, 5] == 3 and (m[0] == -1).sum() == 63
    m, valid, _ = _maps([(5, 5, 0)], [3], w=2, S=16)
    assert valid[0] == 25 and (m[0, 3:8, 3:8] == 3).all()
    m, valid, _ = _maps([(0, 7, 0)], [2], w=2)  # the top right corner: the window is cut to 3 x 3
    assert valid[0] == 9 and (m[0, 0:3, 5:8] == 2).all()
    m, valid, hist = _maps([(2, 2, 0), (2, 2, 1)], [1, 3], w=0)
    assert m[0, 2, 2] == 3 and valid[0] == 1 and hist[0].tolist() == [0, 0, 0, 1]


def test_labels_outside_the_histogram_and_minus_one():
    m, valid, hist = _maps([(1, 1, 0), (2, 2, 1), (3, 3, 2), (4, 4, 3)], [-1, 9, 300, 0], K=4)
    assert m[0, 1, 1] == -1 and m[0, 2, 2] == 9 and m[0, 3, 3] == 300 and valid[0] == 3 and hist[0].tolist() == [1, 0, 0, 0]


def test_validity_bit_blanks_labels_and_reg_labels_are_copied_bit_for_bit():
    validity = np.full((1, 8, 8), 3, dtype=np.uint8)
    validity[0, 3, 3] = 2  # one band without data: `any` blanks it, `each` keeps it
    m, valid, _ = _maps([(3, 3, 0), (5, 5, 1)], [1, 1], validity=validity)
    assert m[0, 3, 3] == -1 and m[0, 5, 5] == 1 and valid[0] == 1
    pts = np.array([(13, 23, 0), (15, 25, 1)], dtype=np.int32)
    each = chips.label_maps([(10, 20)], 8, [0, 2], pts, np.array([1, 1]), 0, validity, "each", "seg", 2)
    assert each[0][0, 3, 3] == 1 and each[1][0] == 2
    odd = np.array([np.float32(0.1), np.uint32(0x7FC01234).view(np.float32), np.float32(-0.0)], dtype=np.float32)
    m, valid, hist = _maps([(1, 1, 0), (2, 2, 1), (3, 3, 2)], odd, task="reg", K=0)
    assert m.dtype == np.float32 and hist is None and valid[0] == 3
    assert [m[0, i, i].view(np.uint32) for i in (1, 2, 3)] == [v.view(np.uint32) for v in odd]
    assert m[0, 0, 0] == -1.0


# ---- point geometry ----------------------------------------------------------------------------------------------------------------------------
def test_lonlat_point_and_its_utm_twin_land_in_the_same_pixel():
    H, W = 100, 120
    ux = np.array([X0 + 37.4 * PX, X0 + 99.9 * PX, X0 + 0.6 * PX])
    uy = np.array([Y0 - 12.7 * PX, Y0 - 80.2 * PX, Y0 - 98.9 * PX])
    lon, lat = crs.transform(crs.from_epsg(32613), crs.from_epsg(4326), ux, uy)
    a = chips.locate_points(ux, uy, 32613, PROFILE, (H, W))
    b = chips.locate_points(lon, lat, 4326, PROFILE, (H, W))
    assert a[0].tolist() == b[0].tolist() == [0, 1, 2]
    assert a[1].tolist() == b[1].tolist() == [12, 80, 98] and a[2].tolist() == b[2].tolist() == [37, 99, 0]


def test_points_outside_the_tile_are_dropped_and_chips_beyond_the_grid_skipped():
    H, W, S = 40, 50, 16
    x = np.array([X0 - 5.0, X0 + 0.2 * PX, X0 + 0.5 * PX, X0 + 49.5 * PX, X0 + 49.8 * PX, X0 + 20.5 * PX, X0 + 20.5 * PX, X0 + 49.0 * PX])
    y = np.array([Y0 - 60.0, Y0 - 60.0, Y0 - 0.5 * PX, Y0 - 39.5 * PX, Y0 - 60.0, Y0 + 1.0, Y0 - 39.8 * PX, Y0 - 35.0 * PX])
    keep, rows, cols, tx, ty = chips.locate_points(x, y, 32613, PROFILE, (H, W))
    assert keep.tolist() == [2, 3, 7]  # the outer half pixel of the tile is outside its pixel-centre bounds
    assert rows.tolist() == [0, 39, 35] and cols.tolist() == [0, 49, 49]
    xy, beyond, ptr, pts = chips.group_points(rows, cols, tx, ty, keep, S, (H, W), (X0, Y0, PX, PX))
    assert xy.tolist() == [[0, 0]] and beyond == 1  # chip (3, 2) lies beyond W // S = 3, H // S = 2
    assert ptr.tolist() == [0, 1] and pts.tolist() == [[0, 0, 2]]


def test_a_point_in_the_half_pixel_fringe_selects_its_chip_and_paints_nothing():
    H, W, S = 64, 64, 16
    x = np.array([X0 + 16.2 * PX, X0 + 40.5 * PX])  # column 16: the first of chip x = 1, left of its centre
    y = np.array([Y0 - 20.5 * PX, Y0 - 40.5 * PX])
    keep, rows, cols, tx, ty = chips.locate_points(x, y, 32613, PROFILE, (H, W))
    xy, beyond, ptr, pts = chips.group_points(rows, cols, tx, ty, keep, S, (H, W), (X0, Y0, PX, PX))
    assert xy.tolist() == [[1, 1], [2, 2]] and beyond == 0
    assert ptr.tolist() == [0, 0, 1] and pts.tolist() == [[40, 40, 1]]


# ---- create_chips, file to file ------------------------------------------------------------------------------------------------------------------
STAMPS = ("2022145T072619", "2022161T072619")
BANDS = ("B02", "B03")


def _write_tile(folder, H=40, W=50, seed=3):
    os.makedirs(folder, exist_ok=True)
    T, C = len(STAMPS), len(BANDS)
    tile, fmask = CR.make_tile(T, C, H, W, seed, fully_masked=(16, 16), untouched=(0, 0), S=16)
    tile[tile < 0] = 1
    files, fmasks = [], []
    for t, stamp in enumerate(STAMPS):
        for c, band in enumerate(BANDS):
            p = os.path.join(folder, f"HLS.S30.T13TDE.{stamp}.v2.0.{band}.tif")
            if (t, c) == (1, 0):
                cog.write_cog(p, [tile[t * C + c][None]], PROFILE, blocksize=16, compress="deflate")  # a tiled deflate file
            else:
                tiff.write(p, tile[t * C + c], PROFILE, compress="deflate" if c else None)
            files.append(p)
        p = os.path.join(folder, f"HLS.S30.T13TDE.{stamp}.v2.0.Fmask.tif")
        tiff.write(p, fmask[t], PROFILE)
        fmasks.append(p)
    return tile, fmask, files, fmasks


def _points():
    # (column, row) in pixels -> chip (0,0): 2 points; (1,1): fully masked; (2,0): one point; (3,1): beyond the grid; (0,1): fringe only
    px = [(3.5, 4.5, 1), (10.5, 11.5, 2), (20.5, 20.5, 1), (40.5, 5.5, 0), (49.4, 20.5, 1), (0.7, 16.2, 2)]
    return {"x": [X0 + c * PX for c, r, _ in px], "y": [Y0 - r * PX for c, r, _ in px], "label": [v for _, _, v in px],
            "date": ["2022-05-25"] * len(px)}


def test_create_chips_end_to_end(tmp_path):
    from instageo_amd.dataloader import get_valid_filepaths

    tile, fmask, files, fmasks = _write_tile(str(tmp_path / "tiles"))
    out = str(tmp_path / "out")
    kw = dict(chip_size=16, mask_types=["cloud", "water"], masking_strategy="each", window_size=1, src_crs=32613)
    names, segs = chips.create_chips(files, fmasks, _points(), out, **kw)
    tid = "S30_T13TDE_2022145T072619"
    assert names == [f"chip_20220525_{tid}_0_0.tif", f"chip_20220525_{tid}_2_0.tif"]
    assert segs == [n.replace("chip_", "seg_map_") for n in names]
    bits = chips.mask_bits(kw["mask_types"])
    for name, seg, (x, y) in zip(names, segs, [(0, 0), (2, 0)]):
        a, prof = tiff.read(os.path.join(out, "chips", name))
        want, _, plane = CR.cut(tile, fmask, [(16 * y, 16 * x)], 16, 2, bits, "each")
        assert a.dtype == np.int16 and np.array_equal(a, want[0])
        assert prof["tags"][33922][1] == (0.0, 0.0, 0.0, X0 + 16 * x * PX, Y0 - 16 * y * PX, 0.0)
        assert prof["tags"][33550] == TAGS[33550] and prof["tags"][34735] == TAGS[34735]
        m, mprof = tiff.read(os.path.join(out, "seg_maps", seg))
        assert m.dtype == np.int16 and m.shape == (1, 16, 16) and mprof["tags"][33922] == prof["tags"][33922]
        assert ((m[0] != -1) <= (plane[0] & 1).astype(bool)).all() and (m[0] != -1).any()
    stats = json.load(open(os.path.join(out, "chips_stats.json")))
    assert stats["nominated"] == 5 and stats["kept"] == 2
    assert stats["dropped"] == {"out_of_bounds": 1, "existing": 0, "no_valid_values": 1, "no_valid_labels": 1}
    seg_all = np.stack([tiff.read(os.path.join(out, "seg_maps", s))[0][0] for s in segs])
    hist = [int((seg_all == k).sum()) for k in range(3)]
    assert stats["class_histogram"] == hist and sum(hist) == int((seg_all != -1).sum())
    present = {k: v for k, v in enumerate(hist) if v}
    assert stats["class_weights"] == pytest.approx([sum(hist) / (len(present) * v) if v else 0.0 for v in hist])
    pairs = get_valid_filepaths(os.path.join(out, "chips_dataset.csv"), out, no_data_value=0, ignore_index=-1)
    assert [(os.path.basename(a), os.path.basename(b)) for a, b in pairs] == list(zip(names, segs))
    # again: every file exists, nothing is rewritten
    before = {n: os.path.getmtime(os.path.join(out, "chips", n)) for n in names}
    names2, segs2 = chips.create_chips(files, fmasks, _points(), out, **kw)
    assert names2 == [] and segs2 == []
    stats2 = json.load(open(os.path.join(out, "chips_stats.json")))
    assert stats2["dropped"]["existing"] == 2 and stats2["kept"] == 0
    assert before == {n: os.path.getmtime(os.path.join(out, "chips", n)) for n in names}
    assert len(get_valid_filepaths(os.path.join(out, "chips_dataset.csv"), out, no_data_value=0, ignore_index=-1)) == 2


def test_a_chip_whose_labels_fall_on_masked_pixels_is_dropped_for_that_reason(tmp_path):
    tile, fmask, files, fmasks = _write_tile(str(tmp_path / "tiles"))
    r, c = np.argwhere((fmask[0, :16, 16:32] & 2) != 0)[0]  # a cloudy pixel of date 0 in chip (1, 0)
    pts = {"x": [X0 + (16 + c + 0.5) * PX], "y": [Y0 - (r + 0.5) * PX], "label": [1], "date": ["2022-05-25"]}
    names, segs = chips.create_chips(files, fmasks, pts, str(tmp_path / "out"), chip_size=16, mask_types=["cloud"], src_crs=32613)
    stats = json.load(open(tmp_path / "out" / "chips_stats.json"))
    assert names == [] and stats["dropped"]["no_valid_labels"] == 1 and stats["dropped"]["no_valid_values"] == 0


def test_create_chips_without_points_cuts_the_grid_as_uint16(tmp_path):
    tile, fmask, files, fmasks = _write_tile(str(tmp_path / "tiles"))
    tile2 = tile.copy()
    out = str(tmp_path / "out")
    names, segs = chips.create_chips(files, fmasks, None, out, chip_size=16, mask_types=["cloud", "water"], masking_strategy="any")
    tid = "S30_T13TDE_2022145T072619"
    grid = [(x, y) for x in range(3) for y in range(2) if (x, y) != (1, 1)]  # (1, 1) is masked on every date
    assert names == [f"chip_20220525_{tid}_{x}_{y}.tif" for x, y in grid] and segs == [None] * 5
    assert not os.path.exists(os.path.join(out, "seg_maps"))
    for name, (x, y) in zip(names, grid):
        a, prof = tiff.read(os.path.join(out, "chips", name))
        want = CR.cut(tile2, fmask, [(16 * y, 16 * x)], 16, 2, chips.mask_bits(["cloud", "water"]), "any", 0, (0, 10000))[0][0]
        assert a.dtype == np.uint16 and np.array_equal(a, want.astype(np.uint16)) and a.max() <= 10000
    assert open(os.path.join(out, "chips_dataset.csv")).read().splitlines()[0] == "Input"


# ---- argument checks ---------------------------------------------------------------------------------------------------------------------------
def test_host_checks_of_origins_and_point_lists():
    tile = np.zeros((2, 20, 30), dtype=np.int16)
    for bad in ([(-1, 0)], [(5, 0)], [(0, 15)]):
        with pytest.raises(ValueError, match="wholly inside"):
            chips.cut(tile, None, bad, 16)
    with pytest.raises(ValueError, match="does not fit"):
        chips.cut(tile, None, [(0, 0)], 21)
    with pytest.raises(ValueError, match="chip_size"):
        chips.cut(tile, None, [(0, 0)], 0)
    with pytest.raises(ValueError, match="dates"):
        chips.cut(tile, None, [(0, 0)], 4, dates=3)
    with pytest.raises(ValueError, match="fmask must be"):
        chips.cut(tile, np.zeros((2, 20, 29), dtype=np.uint8), [(0, 0)], 4)
    with pytest.raises(ValueError, match="masking_strategy"):
        chips.cut(tile, None, [(0, 0)], 4, strategy="all")
    with pytest.raises(ValueError, match="clip"):
        chips.cut(tile, None, [(0, 0)], 4, clip=(5, 1))
    with pytest.raises(ValueError, match="int16"):
        chips.cut(tile.astype(np.int32), None, [(0, 0)], 4)
    with pytest.raises(ValueError, match="valid_values is int32"):
        chips.check_cut((18, 11000, 11000), None, [(0, 0)], 11000, 3, 0, "each", 0, None)
    ok = dict(origins=[(0, 0), (8, 8)], S=8, ptr=[0, 1, 2], pts=[(1, 1, 0), (9, 9, 1)], P=2, w=0, K=2, task_type="seg", label_strategy="any")
    chips.check_labels(**ok)
    for change, what in ((dict(ptr=[0, 2, 1]), "ascending"), (dict(ptr=[0, 1]), "ascending"), (dict(ptr=[1, 1, 2]), "ascending"),
                         (dict(pts=[(1, 1, 0), (7, 9, 1)]), "outside the chip"), (dict(pts=[(1, 1, 0), (9, 16, 1)]), "outside the chip"),
                         (dict(pts=[(1, 1, 0), (9, 9, 2)]), "original index"), (dict(w=-1), "window_size"), (dict(K=257), "histogram"),
                         (dict(K=2, task_type="reg"), "histogram"), (dict(S=0), "chip_size"), (dict(label_strategy="all"), "label_strategy")):
        with pytest.raises(ValueError, match=what):
            chips.check_labels(**{**ok, **change})


def test_entry_points_exported_and_validated_without_gpu(built_lib):
    """IG_REQUIRE rejects bad arguments before any launch, and n = 0 returns before a pointer is looked at."""
    assert {"ig_chip_cut", "ig_chip_labels"} <= set(built_lib.declared_symbols())
    lib, err = built_lib.load(), built_lib.last_error
    one, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4097)
    ok = dict(tile=one, fmask=one, origins=one, n=1, T=3, C=6, H=3660, W=3660, S=256, mask_bits=46, strategy=0, no_data=0, clip=0, clip_lo=0,
              clip_hi=0, chips=one, valid_values=one, validity=one, stream=None)

    def cut(**kw):
        return lib.ig_chip_cut(*{**ok, **kw}.values())

    for kw, what in ((dict(n=-1), "n >= 0"), (dict(T=0), "dates"), (dict(T=33), "dates"), (dict(C=0), "C >= 1"), (dict(H=0), "H >= 1"),
                     (dict(S=0), "S >= 1"), (dict(S=3661), "does not fit"), (dict(H=11000, W=11000, S=11000), "valid_values is int32"), (dict(mask_bits=256), "mask_bits"), (dict(strategy=2), "strategy"),
                     (dict(no_data=40000), "no_data"), (dict(clip=2), "clip"), (dict(clip=1, clip_lo=5, clip_hi=1), "clip range"),
                     (dict(clip=1, clip_hi=40000), "clip range"), (dict(tile=None), "null pointer"), (dict(origins=None), "null pointer"),
                     (dict(chips=None), "null pointer"), (dict(valid_values=None), "null pointer"), (dict(tile=odd), "aligned"),
                     (dict(origins=ctypes.c_void_p(4098)), "aligned")):
        assert cut(**kw) == -1 and what in err(), (kw, err())
    assert cut(n=0, tile=None, origins=None, chips=None, valid_values=None) == 0
    okl = dict(origins=one, n=1, S=64, ptr=one, pts=one, labels=one, P=5, elem_size=2, w=1, validity=one, valid_bit=1, K=4, maps=one,
               valid_labels=one, hist=one, stream=None)

    def lab(**kw):
        return lib.ig_chip_labels(*{**okl, **kw}.values())

    for kw, what in ((dict(n=-1), "n >= 0"), (dict(S=0), "chip side"), (dict(elem_size=1), "elem_size"), (dict(w=-1), "window"),
                     (dict(w=(1 << 20) + 1), "window"), (dict(K=-1), "histogram"), (dict(K=257), "histogram"), (dict(K=2, elem_size=4), "int16 labels"),
                     (dict(P=-1), "points"), (dict(valid_bit=3), "valid_bit"), (dict(valid_bit=0), "validity plane"),
                     (dict(validity=None), "validity plane"), (dict(origins=None), "null pointer"), (dict(ptr=None), "null pointer"),
                     (dict(maps=None), "null pointer"), (dict(pts=None), "null pointer"), (dict(labels=None), "null pointer"),
                     (dict(hist=None), "null pointer"), (dict(ptr=ctypes.c_void_p(4098)), "aligned"), (dict(maps=odd), "aligned")):
        assert lab(**kw) == -1 and what in err(), (kw, err())
    assert lab(n=0, origins=None, ptr=None, maps=None, valid_labels=None) == 0
    with pytest.raises(built_lib.HipLibraryError, match="strategy must be 0 each or 1 any"):
        built_lib.call("ig_chip_cut", *{**ok, "strategy": 7}.values())


def test_prototypes_are_declared_and_custom_ops_follow_them():
    import re

    from instageo_amd import torch_ops

    text = open(os.path.join(ROOT, "include", "instageo_hip.h")).read()
    assert re.search(r"\bint ig_chip_cut\(", text) and re.search(r"\bint ig_chip_labels\(", text)
    assert "chips.hip" in open(os.path.join(PKG, "csrc", "Makefile")).read()
    raw = torch_ops.register()
    s = raw["chip_cut"]
    assert "Tensor? tile" in s and "Tensor? fmask" in s and "Tensor? origins" in s and "Tensor(a!)? chips" in s and "int mask_bits" in s and "stream" not in s
    s = raw["chip_labels"]
    assert "Tensor? pts" in s and "Tensor? labels" in s and "Tensor(a!)? maps" in s and "int valid_bit" in s and "int K" in s


def test_config_carries_the_chips_keys_and_other_modes_are_untouched(tmp_path, capsys):
    from instageo_amd.config import DEFAULTS, load_config

    assert set(DEFAULTS["chips"]) == set(chips.CONFIG_KEYS)
    d = DEFAULTS["chips"]
    assert (d["chip_size"], d["mask_types"], d["masking_strategy"], d["window_size"], d["task_type"], d["src_crs"]) == (256, [], "each", 0, "seg", 4326)
    assert d["tiles"] is d["fmasks"] is d["records_file"] is d["output_directory"] is None
    assert load_config("config", [])["mode"] == "train"
    opts = chips.chips_options(load_config("config", []))  # nothing required outside the mode
    assert opts["tile_files"] is None and opts["chip_size"] == 256
    with pytest.raises(ValueError, match="needs chips.tiles"):
        chips.chips_options(load_config("config", ["mode=create_chips"]))
    base = ["mode=create_chips", "chips.tiles=[a.tif,b.tif]", "chips.output_directory=out"]
    opts = chips.chips_options(load_config("config", base + ["chips.mask_types=[cloud,water]", "chips.fmasks=[f.tif]", "chips.window_size=2",
                                                             "chips.task_type=reg", "chips.records_file=p.csv", "chips.src_crs=32613"]))
    assert opts == dict(tile_files=["a.tif", "b.tif"], fmask_files=["f.tif"], points="p.csv", output_directory="out", chip_size=256,
                        mask_types=["cloud", "water"], masking_strategy="each", window_size=2, task_type="reg", src_crs=32613)
    for ov, what in (("chips.chip_size=0", "chip_size"), ("chips.mask_types=[snow]", "unknown mask type"), ("chips.masking_strategy=all", "masking_strategy"),
                     ("chips.window_size=-1", "window_size"), ("chips.task_type=cls", "task_type"), ("chips.src_crs=1234", "EPSG"),
                     ("chips.mask_types=[cloud]", "needs chips.fmasks")):
        with pytest.raises(ValueError, match=what):
            chips.chips_options(load_config("config", base + [ov]))
    with pytest.raises(KeyError):
        load_config("config", ["chips.chipsize=3"])
    # the mode end to end on the host path
    tile, fmask, files, fmasks = _write_tile(str(tmp_path / "tiles"))
    import pandas as pd

    pd.DataFrame(_points()).to_csv(tmp_path / "p.csv", index=False)
    cfg = load_config("config", ["mode=create_chips", f"chips.tiles=[{','.join(files)}]", f"chips.fmasks=[{','.join(fmasks)}]", "chips.chip_size=16",
                                 "chips.mask_types=[cloud,water]", f"chips.records_file={tmp_path / 'p.csv'}", "chips.src_crs=32613",
                                 "chips.window_size=1", f"chips.output_directory={tmp_path / 'out'}"])
    assert chips.run_from_config(cfg) == 0
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["create_chips"]["chips"] == 2
    assert len(os.listdir(tmp_path / "out" / "chips")) == 2 and len(os.listdir(tmp_path / "out" / "seg_maps")) == 2
