"""Cloud Optimized GeoTIFF output, host side (no GPU): the reference of the two overview rules (tests/overview_reference.py) on pyramids
worked out by hand, level_shapes, the numpy path of build_overviews against that reference, write_cog -> tiff.read(level=k) round trips,
validate_cog, the unchanged strip writer, seg_stats, the config keys and option checks, the header's statement of the rules, the argument
checks of the three HIP entry points and the generated custom ops."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

import overview_reference as OR
from instageo_amd import cog, tiff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "instageo-e2e-geospatial-ml_amd")
NAMES = ("ig_overview_mode", "ig_overview_mean", "ig_cog_tiles")
TAGS = {33550: (12, (30.0, 30.0, 0.0)), 33922: (12, (0.0, 0.0, 0.0, 399960.0, 4500000.0, 0.0)),
        34735: (3, (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 32613))}
NAN = np.float32(np.nan)


@pytest.fixture(scope="module")
def built_lib():
    import subprocess

    from instageo_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j4"], check=True)
    return _lib


# ---- reference ----------------------------------------------------------------------------------------------------------------------------
def test_reference_gives_the_pyramids_worked_out_by_hand():
    cm = np.array([[0, 1, 2, 2, -1, -1, 1],
                   [1, 0, 2, 1, -1, -1, -1],
                   [2, 2, -1, 0, 1, 0, 0]], dtype=np.int8)
    # (0,0): {0, 1, 1, 0} a tie -> 0; (0,1): 2 three times; (0,2): all fill -> fill; (0,3): 1 and a fill -> 1 (a single valid child);
    # second row has one child row: {2, 2} -> 2; {-1, 0} -> 0; {1, 0} tie -> 0; {0} -> 0
    l1, l2, l3 = OR.pyramid(cm, "mode", 3, -1)
    assert l1.tolist() == [[0, 2, -1, 1], [2, 0, 0, 0]] and l1.dtype == np.int8
    # {0, 2, 2, 0} tie -> 0; {-1, 1, 0, 0} -> 0
    assert l2.tolist() == [[0, 0]] and l3.tolist() == [[0]]
    # fill = a class value: the 2s are ignored and -1 is a value like any other ({1, -1} and {-1, 0} are ties -> -1)
    assert OR.pyramid(cm, "mode", 1, 2)[0].tolist() == [[0, 1, -1, -1], [2, -1, 0, 0]]
    # ties go to the smallest value as a signed number
    assert OR.mode_of([5, -128, 5, -128], -1) == -128 and OR.mode_of([7, 3, 9, 1], -1) == 1 and OR.mode_of([-1, -1], -1) == -1
    # a 1 x N raster: one row at every level
    row = np.array([[1, 1, 0, -1, -1, 2, 2]], dtype=np.int8)
    assert [l.tolist() for l in OR.pyramid(row, "mode", 3, -1)] == [[[1, 0, 2, 2]], [[0, 2]], [[0]]]
    f = np.array([[0.5, 0.25, NAN, NAN, 1.0], [0.125, NAN, NAN, NAN, 0.5]], dtype=np.float32)
    m1, m2, m3 = OR.pyramid(f, "mean", 3)
    assert m1.dtype == np.float32 and m1[0, :1].tolist() == [np.float32(0.875) / np.float32(3)] and np.isnan(m1[0, 1]) and m1[0, 2] == 0.75
    assert OR.bits(m1)[0, 1] == OR.NAN_BITS
    third = np.float32(0.875) / np.float32(3)  # a NaN child in a mean: {third, NaN} -> third, then (third + 0.75) / 2
    assert m2.tolist() == [[third, 0.75]] and m3.tolist() == [[np.float32(third + np.float32(0.75)) / np.float32(2)]]
    # the order of the sum is the children's row-major order: (a + b) + c in float32
    a, b, c = np.float32(1e8), np.float32(-1e8), np.float32(1.0)
    assert OR.mean_of([a, c, b, NAN]) == np.float32(np.float32(np.float32(a + c) + b) / np.float32(3)) == 0.0
    assert OR.mean_of([a, b, c, NAN]) == np.float32(1.0) / np.float32(3)


def test_level_shapes_auto_and_int():
    assert cog.level_shapes(4096, 4096) == [(2048, 2048), (1024, 1024), (512, 512), (256, 256)]
    assert cog.level_shapes(10980, 10980, "auto", 256) == [(5490, 5490), (2745, 2745), (1373, 1373), (687, 687), (344, 344), (172, 172)]
    assert cog.level_shapes(256, 256) == [] and cog.level_shapes(257, 3, "auto", 256) == [(129, 2)]
    assert cog.level_shapes(300, 260, "auto", 128) == [(150, 130), (75, 65)]
    assert cog.level_shapes(37, 67, 3) == [(19, 34), (10, 17), (5, 9)] and cog.level_shapes(37, 67, 0) == []
    assert cog.level_shapes(3, 5, 12) == [(2, 3), (1, 2), (1, 1)] and cog.level_shapes(1, 1, 6) == []  # stops at 1 x 1
    for bad in (-1, 13, "six", 2.0, True):
        with pytest.raises(ValueError, match="overview_levels"):
            cog.level_shapes(8, 8, bad)
    with pytest.raises(ValueError, match="at least one"):
        cog.level_shapes(0, 8)


@pytest.mark.parametrize("name", ["odd_37x67", "block_65x129", "deep_130x70"])
def test_numpy_path_equals_the_reference(name):
    H, W, levels = OR.CASES[name]
    cm, want = OR.mode_case(name)
    got = cog.build_overviews(cm, "mode", levels, -1)
    assert got[0] is not None and np.array_equal(got[0], cm) and len(got) == len(cog.level_shapes(H, W, levels)) + 1
    for g, w in zip(got[1:], want):
        assert g.dtype == np.int8 and np.array_equal(g, w)
    a, wantf = OR.mean_case(name, 3)
    gotf = cog.build_overviews(a, "mean", levels)
    for g, w in zip(gotf[1:], wantf):
        assert g.dtype == np.float32 and g.shape == w.shape and np.array_equal(OR.bits(g), OR.bits(w))
    counts = np.zeros(4, dtype=np.int64)
    cog.build_overviews(cm, "mode", 0, -1, ncls=3, counts=counts)
    assert np.array_equal(counts, OR.histogram(cm, 3, -1)) and counts.sum() == H * W
    with pytest.raises(ValueError, match="int8"):
        cog.build_overviews(a, "mode", 1)
    with pytest.raises(ValueError, match="float32"):
        cog.build_overviews(cm, "mean", 1)
    with pytest.raises(ValueError, match="kind"):
        cog.build_overviews(cm, "median", 1)


# ---- writer, reader, checker ------------------------------------------------------------------------------------------------------------------
def _levels(dtype, bands, H, W, n, seed=0):
    """Level 0 random, the others by plain decimation (the writer does not care where the levels come from)."""
    rng = np.random.default_rng(seed)
    if np.dtype(dtype).kind == "f":
        a = rng.random((bands, H, W)).astype(dtype)
        a[:, 3:9, 5:40] = np.nan
    else:
        info = np.iinfo(dtype)
        a = rng.integers(info.min, info.max + 1, size=(bands, H, W)).astype(dtype)
    out = [a]
    for _ in range(n):
        p = out[-1]
        p = np.pad(p, [(0, 0), (0, p.shape[1] % 2), (0, p.shape[2] % 2)], mode="edge")
        out.append(np.ascontiguousarray(p[:, ::2, ::2]))
    return out


@pytest.mark.parametrize("dtype,bands,block,compress,predictor", [
    ("int8", 1, 128, "deflate", None), ("int8", 3, 256, None, None), ("float32", 1, 256, "deflate", None), ("float32", 3, 128, None, None),
    ("int8", 1, 128, "deflate", 2), ("int16", 3, 128, None, 2), ("int16", 1, 256, "deflate", 2), ("uint8", 1, 128, "none", 1)])
def test_write_cog_round_trip(tmp_path, dtype, bands, block, compress, predictor):
    lv = _levels(dtype, bands, 300, 517, 3, seed=bands)
    nodata = None if dtype == "float32" else -1 if dtype != "uint8" else 255
    tags = {**TAGS, **({42113: (2, "nan")} if dtype == "float32" else {})}
    path = cog.write_cog(str(tmp_path / "a.tif"), lv, {"tags": tags, "nodata": nodata}, block, compress, predictor)
    assert cog.validate_cog(path) == [] and tiff.overview_count(path) == 3
    for k, want in enumerate(lv):
        got, prof = tiff.read(path, level=k)
        assert got.dtype == want.dtype and got.shape == want.shape
        assert np.array_equal(got.view(f"u{got.dtype.itemsize}"), want.view(f"u{want.dtype.itemsize}")), k
        assert repr(prof) == repr(tiff.read_profile(path, level=k)) and (prof["width"], prof["height"], prof["count"]) == (want.shape[2], want.shape[1], bands)
        assert (42113 in prof["tags"]) and ({t for t in prof["tags"] if t != 42113} == (set(TAGS) if k == 0 else set()))  # GDAL_NODATA on every IFD
    assert tiff.read(path)[1]["tags"] == {**tags, **({42113: (2, str(nodata))} if nodata is not None else {})}  # verbatim, as tiff.write
    if bands == 3:
        one, _ = tiff.read(path, bands=[2], level=1)
        assert np.array_equal(one[0].view("u1"), lv[1][2].view("u1"))
    # the layout: header, the IFDs in decreasing size, then the data from the smallest level to level 0
    buf = open(path, "rb").read()
    chain = tiff._ifd_chain(buf, "<", struct.unpack_from("<I", buf, 4)[0])
    assert chain[0] == 8 and chain == sorted(chain)
    ifds = [tiff._read_ifd(buf, "<", off) for off in chain]
    assert [t.get(254, (4, (0,)))[1][0] for t in ifds] == [0, 1, 1, 1] and all(t[322][1] == t[323][1] == (block,) for t in ifds)
    starts = [t[324][1][0] for t in ifds]
    assert starts == sorted(starts, reverse=True) and min(starts) > chain[-1]
    assert all(t[284][1][0] == (2 if bands > 1 else 1) and t[259][1][0] == (8 if compress == "deflate" else 1) for t in ifds)
    assert all((317 in t) == (predictor == 2) for t in ifds)
    # the same input gives the same bytes
    assert open(cog.write_cog(str(tmp_path / "b.tif"), lv, {"tags": tags, "nodata": nodata}, block, compress, predictor), "rb").read() == buf


def test_write_cog_refuses_what_it_cannot_write(tmp_path):
    lv = _levels("int8", 1, 40, 40, 2)
    p = str(tmp_path / "x.tif")
    with pytest.raises(tiff.TiffError, match="predictor"):
        cog.write_cog(p, _levels("float32", 1, 40, 40, 0), predictor=2)
    with pytest.raises(tiff.TiffError, match="predictor"):
        cog.write_cog(p, lv, predictor=3)
    with pytest.raises(tiff.TiffError, match="compression"):
        cog.write_cog(p, lv, compress="lzw")
    with pytest.raises(tiff.TiffError, match="multiple of 16"):
        cog.write_cog(p, lv, blocksize=100)
    with pytest.raises(tiff.TiffError, match="level 1 is"):
        cog.write_cog(p, [lv[0], lv[2]])
    with pytest.raises(tiff.TiffError, match="level 1 has"):
        cog.write_cog(p, [lv[0], lv[1].astype(np.int16)])
    with pytest.raises(tiff.TiffError, match="float64"):
        cog.write_cog(p, [np.zeros((4, 4))])
    with pytest.raises(tiff.TiffError, match="at least level 0"):
        cog.write_cog(p, [])
    assert not os.path.exists(p)


def test_validate_cog_names_the_violations(tmp_path):
    lv = _levels("int8", 1, 300, 517, 2)
    strip = str(tmp_path / "strip.tif")
    tiff.write(strip, lv[0], {"tags": TAGS}, compress="deflate")
    assert any("not tiled" in v for v in cog.validate_cog(strip))
    good = cog.write_cog(str(tmp_path / "good.tif"), lv, {"tags": TAGS}, 128)
    assert cog.validate_cog(good) == []
    # by hand: the two overviews change places in the IFD chain (0 -> 2 -> 1 -> end)
    buf = bytearray(open(good, "rb").read())
    chain = tiff._ifd_chain(bytes(buf), "<", 8)
    nxt = [off + 2 + 12 * struct.unpack_from("<H", buf, off)[0] for off in chain]
    struct.pack_into("<I", buf, nxt[0], chain[2]), struct.pack_into("<I", buf, nxt[2], chain[1]), struct.pack_into("<I", buf, nxt[1], 0)
    swapped = str(tmp_path / "swapped.tif")
    open(swapped, "wb").write(bytes(buf))
    bad = cog.validate_cog(swapped)
    assert any("does not follow" in v for v in bad) and any("does not lie before" in v for v in bad)
    assert tiff.read(swapped, level=1)[0].shape == lv[2].shape  # still a readable TIFF
    # an overview without its subfile type, and a block size that is no multiple of 16
    buf = bytearray(open(good, "rb").read())
    at = chain[1] + 2
    assert struct.unpack_from("<H", buf, at)[0] == 254
    struct.pack_into("<I", buf, at + 8, 0)
    open(swapped, "wb").write(bytes(buf))
    assert cog.validate_cog(swapped) == ["IFD 1: an overview without NewSubfileType = 1"]
    odd = cog.write_cog(str(tmp_path / "odd.tif"), lv, None, 128)
    buf = bytearray(open(odd, "rb").read())
    n = struct.unpack_from("<H", buf, 8)[0]
    for i in range(n):
        if struct.unpack_from("<H", buf, 10 + 12 * i)[0] == 322:
            struct.pack_into("<I", buf, 10 + 12 * i + 8, 120)
    open(odd, "wb").write(bytes(buf))
    assert any("no multiple of 16" in v for v in cog.validate_cog(odd))


def test_strip_files_read_as_before_and_have_no_overviews(tmp_path):
    gold = os.path.join(ROOT, "tests", "golden", "tiff", "chip_178_022.tif")
    arr, prof = tiff.read(gold)
    arr0, prof0 = tiff.read(gold, level=0)
    assert np.array_equal(arr, arr0) and prof == prof0 == tiff.read_profile(gold) == tiff.read_profile(gold, level=0)
    assert tiff.overview_count(gold) == 0
    a = np.arange(6 * 50 * 70, dtype=np.int16).reshape(6, 50, 70)
    p = str(tmp_path / "w.tif")
    tiff.write(p, a, {"tags": TAGS, "nodata": -9999}, compress="deflate")
    got, gp = tiff.read(p)
    assert np.array_equal(got, a) and gp["tags"] == {**TAGS, 42113: (2, "-9999")} and tiff.overview_count(p) == 0
    # the strip writer's layout: header, strips, values, one IFD at the end with no successor
    buf = open(p, "rb").read()
    ifd = struct.unpack_from("<I", buf, 4)[0]
    n = struct.unpack_from("<H", buf, ifd)[0]
    assert ifd + 2 + 12 * n + 4 == len(buf) and struct.unpack_from("<I", buf, ifd + 2 + 12 * n)[0] == 0 and 324 not in tiff._read_ifd(buf, "<", ifd)
    for level in (1, 2, -1):
        with pytest.raises(tiff.TiffError, match="level"):
            tiff.read(p, level=level)
        with pytest.raises(tiff.TiffError, match="level"):
            tiff.read_profile(p, level=level)
    c = cog.write_cog(str(tmp_path / "c.tif"), _levels("int8", 1, 40, 40, 2), None, 128)
    cut = str(tmp_path / "cut.tif")
    for n in (6, 9, 40):  # truncated in the header, in IFD 0 and before the next-IFD offset: TiffError, as read and read_profile raise
        open(cut, "wb").write(open(c, "rb").read()[:n])
        for fn in (tiff.overview_count, tiff.read, tiff.read_profile):
            with pytest.raises(tiff.TiffError, match="truncated or corrupt"):
                fn(cut)
    with pytest.raises(tiff.TiffError, match="level 3 is beyond"):
        tiff.read(c, level=3)


def test_convert_picks_the_rule_by_sample_type(tmp_path):
    cm, want = OR.mode_case("odd_37x67")
    src = str(tmp_path / "cm.tif")
    tiff.write(src, cm, {"tags": TAGS, "nodata": -1})
    dst = cog.convert(src, str(tmp_path / "cm_cog.tif"), levels=3, blocksize=128)
    assert cog.validate_cog(dst) == [] and tiff.overview_count(dst) == 3 and tiff.read(dst)[1]["tags"] == tiff.read(src)[1]["tags"]
    assert np.array_equal(tiff.read(dst)[0][0], cm) and all(np.array_equal(tiff.read(dst, level=k + 1)[0][0], want[k]) for k in range(3))
    a, wantf = OR.mean_case("odd_37x67", 3)
    tiff.write(src, a, {"tags": {**TAGS, 42113: (2, "nan")}})
    dst = cog.convert(src, str(tmp_path / "f_cog.tif"), levels=2, blocksize=128, compress=None)
    assert all(np.array_equal(OR.bits(tiff.read(dst, level=k + 1)[0]), OR.bits(wantf[k])) for k in range(2))
    tiff.write(src, np.zeros((4, 4), dtype=np.int16))
    with pytest.raises(ValueError, match="no overview rule"):
        cog.convert(src, str(tmp_path / "no.tif"))


def test_seg_stats_is_the_reference_dictionary():
    cm = np.array([[0, 0, 2, -1], [2, 2, 5, -1], [0, 100, -128, 2]], dtype=np.int8)
    want = {"valid_pixels": 7, "class_counts": {"0": 3, "2": 4}, "unique_values": 2}
    assert OR.seg_stats(cm, 3, -1) == want
    counts = cog.class_histogram(cm, 3, -1)
    assert counts.tolist() == [3, 0, 4, 5] and np.array_equal(counts, OR.histogram(cm, 3, -1)) and cog.seg_stats(counts) == want
    # what the reference computes with rasterio on the written file: masked read, bincount of the valid values, str keys, only n > 0
    valid = cm[(cm != -1) & (cm >= 0) & (cm < 3)]
    bc = np.bincount(valid, minlength=int(valid.max()) + 1)
    assert want == {"valid_pixels": int(valid.size), "class_counts": {str(i): int(c) for i, c in enumerate(bc) if c > 0},
                    "unique_values": int((bc > 0).sum())}
    assert cog.seg_stats(np.zeros(4, dtype=np.int64)) == {"valid_pixels": 0, "class_counts": {}, "unique_values": 0}
    assert cog.seg_stats(cog.class_histogram(cm, 6, 2)) == {"valid_pixels": 4, "class_counts": {"0": 3, "5": 1}, "unique_values": 2}


# ---- config and option checks ---------------------------------------------------------------------------------------------------------------
def test_config_carries_the_cog_keys_and_they_default_to_off():
    import inspect

    from instageo_amd import run
    from instageo_amd.config import DEFAULTS, load_config
    from instageo_amd.infer_utils import tile_inference

    t = DEFAULTS["test"]
    assert (t["cog"], t["cog_blocksize"], t["overview_levels"], t["cog_compress"]) == (False, 256, "auto", "deflate")
    off = dict(cog=False, cog_blocksize=256, overview_levels="auto", cog_compress="deflate")
    assert run.cog_options(load_config("config", [])) == off
    assert run.cog_options(load_config("config", ["mode=chip_inference"])) == off  # off: chip inference is not concerned
    cfg = load_config("sen1floods11", ["mode=tile_inference", "test.cog=true", "test.cog_blocksize=512", "test.overview_levels=6",
                                       "test.cog_compress=none"])
    assert run.cog_options(cfg) == dict(cog=True, cog_blocksize=512, overview_levels=6, cog_compress="none")
    p = inspect.signature(tile_inference).parameters
    assert (p["cog"].default, p["cog_blocksize"].default, p["overview_levels"].default, p["cog_compress"].default) == (False, 256, "auto", "deflate")
    with pytest.raises(ValueError, match="per-chip COGs are not produced.*cog.convert"):
        run.cog_options(load_config("config", ["mode=chip_inference", "test.cog=true"]))
    for ov, what in (("test.cog_blocksize=100", "cog_blocksize"), ("test.cog_blocksize=64", "cog_blocksize"), ("test.overview_levels=13", "overview_levels"),
                     ("test.overview_levels=-1", "overview_levels"), ("test.overview_levels=all", "overview_levels"), ("test.cog_compress=lzw", "cog_compress")):
        with pytest.raises(ValueError, match=what):
            run.cog_options(load_config("config", ["mode=tile_inference", ov]))
    with pytest.raises(KeyError):
        load_config("config", ["test.cogs=true"])


def test_tile_inference_checks_the_cog_options_before_any_work():
    from instageo_amd.infer_utils import tile_inference

    for kw, what in ((dict(cog_blocksize=200), "cog_blocksize"), (dict(overview_levels=40), "overview_levels"), (dict(cog_compress="lzw"), "cog_compress")):
        with pytest.raises(ValueError, match=what):
            tile_inference("/nonexistent/tile.tif", "/nonexistent/out", None, [0.0], [1.0], cog=True, **kw)
    assert not os.path.exists("/nonexistent")
    cog.check_cog_options(True, 128, 0, None)
    with pytest.raises(ValueError, match="cog.convert"):
        cog.check_cog_options(True, chip_mode=True)
    cog.check_cog_options(False, chip_mode=True)
    # more classes than the histogram (and an int8 class map) holds: refused up front, with the model in hand and nothing else touched
    from types import SimpleNamespace

    wide = SimpleNamespace(cfg=SimpleNamespace(num_classes=128))
    with pytest.raises(ValueError, match="at most 127 classes"):
        tile_inference("/nonexistent/tile.tif", "/nonexistent/out", wide, [0.0], [1.0], cog=True)
    cog.check_cog_options(True, ncls=127), cog.check_cog_options(False, ncls=128)
    assert not os.path.exists("/nonexistent")


# ---- header, library, custom ops ------------------------------------------------------------------------------------------------------------
def test_header_states_the_two_rules():
    text = open(os.path.join(ROOT, "include", "instageo_hip.h")).read()
    block = [c for c in re.findall(r"/\*.*?\*/", text, flags=re.S) if "ig_overview_mode:" in c]
    assert len(block) == 1
    block = " ".join(block[0].replace("\n *", " ").split())
    for phrase in ("H_k = ceil(H_{k-1} / 2)", "W_k = ceil(W_{k-1} / 2)", "(2r..2r+1, 2c..2c+1)", "1, 2 or 4 of them", "never from level 0",
                   "children equal to fill are ignored", "if none is left the result is fill", "ties go to the smallest value",
                   "does not depend on child order", "multiples of 2^levels", "no claim of equality with GDAL's MODE",
                   "those that are not NaN", "row-major child order", "IEEE round-to-nearest division", "0x7fc00000", "equal to numpy float32",
                   "origin at multiples of 64", "written exactly once", "1 <= levels <= 12", "1 <= ncls <= 127", "wrap-around arithmetic"):
        assert phrase in block, phrase
    parts = re.split(r"(?=\big_(?:overview|cog)_\w+: )", block)
    assert [p.split(":")[0] for p in parts[1:]] == list(NAMES)
    for n in NAMES:
        assert re.search(r"\bint %s\(" % n, text)
    doc = " ".join(cog.__doc__.split())
    for phrase in ("ties to the smallest value", "no claim of equality with GDAL's ``MODE``", "row-major child order", "never from level 0"):
        assert phrase in doc, phrase
    src = open(os.path.join(PKG, "csrc", "cog.hip")).read()
    assert "CB = 64" in src and "CMAXL = 6" in src and "__fdiv_rn" in src  # the block and the six levels the GPU cases are built on
    assert "cog.hip" in open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert "-ffast-math" not in open(os.path.join(PKG, "csrc", "Makefile")).read()


def test_entry_points_exported_and_validated_without_gpu(built_lib):
    """IG_REQUIRE rejects bad arguments before any launch, and empty calls return before a pointer is looked at (safe on a CPU-only box)."""
    assert set(NAMES) <= set(built_lib.declared_symbols())
    lib = built_lib.load()
    err = built_lib.last_error
    one, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)

    mode = lib.ig_overview_mode
    assert mode(None, 8, 8, -1, 3, 2, one, None, None) == -1 and "null pointer" in err()
    assert mode(one, 8, 8, -1, 3, 2, None, None, None) == -1 and "null pointer" in err()
    assert mode(one, 8, 8, -1, 3, 0, one, None, None) == -1 and "levels" in err()
    assert mode(one, 8, 8, -1, 3, 13, one, None, None) == -1 and "1 <= levels <= 12" in err()
    assert mode(one, 8, 8, 128, 3, 2, one, None, None) == -1 and "fill" in err()
    assert mode(one, 8, 8, -1, 0, 2, one, None, None) == -1 and "ncls" in err()
    assert mode(one, 8, 8, -1, 128, 2, one, None, None) == -1 and "ncls" in err()
    assert mode(one, 8, 8, -1, 3, 2, one, odd, None) == -1 and "aligned" in err()
    assert mode(one, 65536, 32768, -1, 3, 2, one, None, None) == -1 and "2^31" in err()
    assert mode(one, -1, 8, -1, 3, 2, one, None, None) == -1 and "H" in err()
    assert mode(None, 0, 8, -1, 3, 2, None, None, None) == 0 and mode(None, 8, 0, -1, 3, 2, None, None, None) == 0  # H * W = 0

    mean = lib.ig_overview_mean
    assert mean(None, 1, 8, 8, 2, one, None) == -1 and "null pointer" in err()
    assert mean(one, 1, 8, 8, 2, None, None) == -1 and "null pointer" in err()
    assert mean(ctypes.c_void_p(4098), 1, 8, 8, 2, one, None) == -1 and "aligned" in err()
    assert mean(one, 1, 8, 8, 0, one, None) == -1 and "levels" in err()
    assert mean(one, 1, 8, 8, 13, one, None) == -1 and "levels" in err()
    assert mean(one, -1, 8, 8, 2, one, None) == -1 and "bands" in err()
    assert mean(one, 65536, 8, 8, 2, one, None) == -1 and "bands" in err()
    assert mean(one, 1, 8, -1, 2, one, None) == -1 and "W" in err()
    assert mean(None, 0, 8, 8, 2, None, None) == 0 and mean(None, 2, 0, 8, 2, None, None) == 0

    tiles = lib.ig_cog_tiles
    assert tiles(None, 1, 8, 8, 1, 0, 128, 0, 1, one, None) == -1 and "null pointer" in err()
    assert tiles(one, 1, 8, 8, 1, 0, 128, 0, 1, None, None) == -1 and "null pointer" in err()
    assert tiles(one, 1, 8, 8, 3, 0, 128, 0, 1, one, None) == -1 and "elem_size" in err()
    assert tiles(one, 1, 8, 8, 8, 0, 128, 0, 1, one, None) == -1 and "elem_size" in err()
    assert tiles(one, 1, 8, 8, 4, 1, 128, 0, 2, one, None) == -1 and "integers only" in err()  # predictor 2 on floats
    assert tiles(one, 1, 8, 8, 2, 1, 128, 0, 1, one, None) == -1 and "floating point" in err()
    assert tiles(one, 1, 8, 8, 1, 0, 128, 0, 3, one, None) == -1 and "predictor" in err()
    assert tiles(one, 1, 8, 8, 1, 0, 100, 0, 1, one, None) == -1 and "tile" in err()
    assert tiles(one, 1, 8, 8, 1, 0, 0, 0, 1, one, None) == -1 and "tile" in err()
    assert tiles(one, 1, 8, 8, 1, 0, 128, 0, 1, odd, None) == -1 and "16-byte" in err()
    assert tiles(ctypes.c_void_p(4098), 1, 8, 8, 4, 0, 128, 0, 1, one, None) == -1 and "aligned" in err()
    assert tiles(one, -1, 8, 8, 1, 0, 128, 0, 1, one, None) == -1 and "bands" in err()
    assert tiles(one, 65536, 8, 8, 1, 0, 128, 0, 1, one, None) == -1 and "bands <= 65535" in err()
    assert tiles(one, 65535, 1, 2**31 - 1, 4, 0, 4096, 0, 1, one, None) == -1 and "2^40" in err()  # the largest product still fits a long
    assert tiles(None, 0, 8, 8, 1, 0, 128, 0, 1, None, None) == 0 and tiles(None, 1, 0, 8, 1, 0, 128, 0, 1, None, None) == 0
    with pytest.raises(built_lib.HipLibraryError, match="levels"):
        built_lib.call("ig_overview_mode", one, 8, 8, -1, 3, 99, one, None, None)


def test_generated_custom_ops_follow_the_header():
    from instageo_amd import torch_ops

    raw = torch_ops.register()
    assert {n[3:] for n in NAMES} <= set(raw)
    assert "Tensor? src" in raw["overview_mode"] and "Tensor(a!)? dst" in raw["overview_mode"] and "Tensor(b!)? counts" in raw["overview_mode"]
    assert "int fill" in raw["overview_mode"] and "int levels" in raw["overview_mean"] and "Tensor(a!)? dst" in raw["overview_mean"]
    assert "int elem_size" in raw["cog_tiles"] and "int pad" in raw["cog_tiles"] and "int predictor" in raw["cog_tiles"]
