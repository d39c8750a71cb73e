"""Map tiles without a GPU: the tile lattice against closed forms, the covering tiles, the zoom range and the level choice, the numpy host
path against the sequential twin (tests/maptiles_reference.py) for all three styles, the PNG writer, ``tilejson.json``, ``export`` on a
COG, and the imagery mosaic of ``merge_chips``.  Every comparison with the twin is exact; the twin reports no tie on these cases."""
import functools
import json
import math
import os

import numpy as np
import pytest

import maptiles_reference as MR
from instageo_amd import cog, crs, maptiles as M, tiff

EPSG = {"utm_north": 32636, "utm_south": 32736, "geographic": 4326, "web_mercator": 3857}


def profile_of(name, shape=(MR.H, MR.W), grid=None, dtype="int8", count=1):
    X0, Y0, sx, sy = grid or MR.SOURCES[name][1]
    tags = dict(crs.geokeys(EPSG[name]))
    tags[33550] = (12, (sx, sy, 0.0))
    tags[33922] = (12, (0.0, 0.0, 0.0, X0, Y0, 0.0))
    return {"width": shape[1], "height": shape[0], "count": count, "dtype": dtype, "nodata": None, "tags": tags}


@functools.lru_cache(maxsize=None)
def export_case(style, name="utm_north", tile=64):
    """-> (levels, profile, the XYZ tiles of the automatic zoom range, their levels, the twin's ties over all of them)."""
    levels = MR.levels_of(style)
    profile = profile_of(name)
    zmin, zmax = M.zoom_range(profile, (MR.H, MR.W), len(levels), tile)
    tiles = [t for z in range(zmin, zmax + 1) for t in M.covering_tiles(profile, (MR.H, MR.W), z)]
    lvls = M.choose_levels(profile, (MR.H, MR.W), tiles, len(levels), tile)
    system, grid = MR.SOURCES[name]
    ties = sum(MR.scaled_coords(system, grid, xyz_grid(*t, tile), tile, int(k))[2] for t, k in zip(tiles, lvls))
    return levels, profile, tiles, lvls, ties


def xyz_grid(z, x, y, tile):
    """The closed form, written independently of the product."""
    side = 2 * MR.ORIGIN / 2**z
    return (-MR.ORIGIN + x * side, MR.ORIGIN - y * side, side / tile, side / tile)


# ---- the lattice -------------------------------------------------------------------------------------------------------------------------
def test_tile_grid_and_bounds_against_closed_forms():
    assert M.ORIGIN == 20037508.342789244
    assert M.tile_grid(0, 0, 0, 256) == (-20037508.342789244, 20037508.342789244, 2 * 20037508.342789244 / 256, 2 * 20037508.342789244 / 256)
    w, s, e, n = M.tile_bounds(1, 1, 0)
    assert (w, e) == (0.0, 180.0) and s == 0.0 and abs(n - 85.0511287798066) < 1e-12
    assert M.tile_bounds(0, 0, 0)[0::2] == (-180.0, 180.0)
    for z, x, y, tile in ((3, 5, 2, 256), (11, 1217, 771, 64), (14, 9740, 6170, 512)):
        X0, Y0, sx, sy = M.tile_grid(z, x, y, tile)
        assert (X0, Y0, sx, sy) == xyz_grid(z, x, y, tile)
        kids = [M.tile_grid(z + 1, 2 * x + i, 2 * y + j, tile) for j in (0, 1) for i in (0, 1)]
        assert all(k[2] == sx / 2 and k[3] == sy / 2 for k in kids)
        # the children share the parent's lattice lines exactly: its origin, its far corner (the origin of tile x + 1, y + 1) and one
        # middle line each way, which lies half a tile from the origin
        assert kids[0][:2] == (X0, Y0) and M.tile_grid(z + 1, 2 * x + 2, 2 * y + 2, tile)[:2] == M.tile_grid(z, x + 1, y + 1, tile)[:2]
        assert kids[1][0] == kids[3][0] and kids[2][1] == kids[3][1] and kids[1][1] == Y0 and kids[2][0] == X0
        assert abs(kids[1][0] - (X0 + tile * sx / 2)) < 1e-8 and abs(kids[2][1] - (Y0 - tile * sy / 2)) < 1e-8
        b = M.tile_bounds(z, x, y)
        kb = [M.tile_bounds(z + 1, 2 * x + i, 2 * y + j) for j in (0, 1) for i in (0, 1)]
        assert kb[0][0] == b[0] and kb[0][3] == b[3] and kb[3][2] == b[2] and kb[3][1] == b[1] and kb[0][2] == kb[1][0] and kb[0][1] == kb[2][3]
    with pytest.raises(ValueError, match="no tile"):
        M.tile_grid(2, 4, 0)
    with pytest.raises(ValueError, match="multiple of 64"):
        M.check_tile_size(100)


def test_covering_tiles_of_a_raster_across_a_tile_corner():
    z = 12
    X0, Y0, s, _ = xyz_grid(z, 2435, 1542, 256)  # the raster straddles this tile's north-west corner
    prof = profile_of("web_mercator", (40, 50), (X0 - 20 * 38.2, Y0 + 15 * 38.2, 38.2, 38.2))
    assert M.covering_tiles(prof, (40, 50), z) == [(z, 2434, 1541), (z, 2435, 1541), (z, 2434, 1542), (z, 2435, 1542)]
    assert M.covering_tiles(prof, (40, 50), 0) == [(0, 0, 0)]
    inside = profile_of("web_mercator", (40, 50), (X0 + 100.0, Y0 - 100.0, 38.2, 38.2))
    assert M.covering_tiles(inside, (40, 50), z) == [(z, 2435, 1542)]
    across = profile_of("geographic", (100, 100), (179.9, 10.0, 0.01, 0.01))
    with pytest.raises(ValueError, match="antimeridian"):
        M.covering_tiles(across, (100, 100), 3)


@pytest.mark.parametrize("name,maxzoom", [("utm_north", 12), ("geographic", 12), ("web_mercator", 13)])
def test_zoom_range_and_level_choice(name, maxzoom):
    """A 30 m UTM and a 0.00027 degree raster at 40.6 degrees are about 39.5 m of web Mercator per pixel, and 2 pi R / 256 / 2^12 =
    38.22 m: zoom 12.  A 38.2 m web Mercator raster is just finer than that: zoom 13."""
    prof, shape = profile_of(name, (1000, 900)), (1000, 900)
    nlevels = 4
    assert M.zoom_range(prof, shape, nlevels) == (maxzoom - nlevels, maxzoom)
    assert M.zoom_range(prof, shape, nlevels, tile=512) == (maxzoom - 1 - nlevels, maxzoom - 1)
    assert M.zoom_range(prof, shape, nlevels, minzoom=3, maxzoom=5) == (3, 5)
    with pytest.raises(ValueError, match="map_tiles_minzoom"):
        M.zoom_range(prof, shape, nlevels, minzoom=9, maxzoom=5)
    with pytest.raises(ValueError, match="map_tiles_maxzoom"):
        M.zoom_range(prof, shape, nlevels, maxzoom=99)
    system, grid = crs.from_profile(prof), MR.SOURCES[name][1]
    for z in range(maxzoom - 5, maxzoom + 2):
        tiles = M.covering_tiles(prof, shape, z)
        lv = M.choose_levels(prof, shape, tiles, nlevels)
        assert ((lv >= 0) & (lv < nlevels)).all()
        for (zz, x, y), k in zip(tiles, lv):
            X0, Y0, s, _ = xyz_grid(zz, x, y, 256)
            cx, cy = X0 + 128 * s, Y0 - 128 * s
            xs, ys = crs.transform(M.WEBM, system, np.array([cx, cx + s, cx]), np.array([cy, cy, cy - s]))
            step = min(math.hypot((xs[1] - xs[0]) / grid[2], (ys[1] - ys[0]) / grid[3]), math.hypot((xs[2] - xs[0]) / grid[2], (ys[2] - ys[0]) / grid[3]))
            assert 2.0**k <= step * (1 + 1e-6) or k == 0  # never coarser than the tile
            assert k == nlevels - 1 or 2.0 ** (k + 1) > step  # and the coarsest such level
    if name == "web_mercator":  # 2 pi R / 256 / 2^10 = 152.9 m = 4.002 source pixels: level 2
        tiles = M.covering_tiles(prof, shape, 10)
        assert M.choose_levels(prof, shape, tiles, nlevels).tolist() == [2] * len(tiles)


# ---- the host path against the twin ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tile,style", MR.CASES)
def test_host_path_equals_the_twin(name, tile, style):
    want, opaque, ties = MR.twin(name, tile, style)
    assert ties == 0
    system, grid = MR.SOURCES[name]
    grids, lvls = MR.tile_cases(name, tile)
    a = MR.STYLE_ARGS[style]
    rgba, got = M._render_host(MR.levels_of(style), system, np.array(grid), np.array(grids), lvls, tile, style, a.get("lut"), a.get("ncolors", 0),
                               a.get("fill", -1), (MR.LO, MR.HI), a.get("order", (0, 1, 2)))
    assert np.array_equal(got, opaque) and np.array_equal(rgba, want)
    assert opaque[0] > 0 and (tile != 64 or opaque[5] == 0)


@pytest.mark.parametrize("style", ["palette", "ramp", "rgb"])
def test_render_of_xyz_tiles_equals_the_twin(style):
    levels, profile, tiles, lvls, ties = export_case(style)
    assert ties == 0 and len(tiles) >= 4 and set(lvls.tolist()) == {0, 1, 2}
    a = MR.STYLE_ARGS[style]
    system, grid = MR.SOURCES["utm_north"]
    want = MR.render(levels, system, grid, [xyz_grid(*t, 64) for t in tiles], lvls.tolist(), 64, style, **a)
    got = M.render(levels, profile, tiles, style, 64, a.get("lut"), a.get("ncolors"), a.get("fill", -1), (MR.LO, MR.HI), a.get("order", (0, 1, 2)))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and want[1].sum() > 0


def test_ramp_index_at_the_ends_and_default_tables():
    v = np.array([-np.inf, -1.0, 0.0, 0.5, 1.0, 2.0, np.inf, 0.1], dtype=np.float32)
    assert M.ramp_index(v, 0.0, 1.0).tolist() == [0, 0, 0, 128, 255, 255, 255, int(np.rint(np.float64(np.float32(0.1)) * 255))]
    assert M.ramp_index(np.array([1500.0], dtype=np.float32), 0.0, 3000.0).tolist() == [128]  # 127.5 rounds to even
    ramp = M.default_ramp()
    assert ramp.shape == (256, 4) and ramp.dtype == np.uint8 and (ramp[:, 3] == 255).all()
    assert [tuple(ramp[i, :3]) for i in (0, 255)] == [M.RAMP_ANCHORS[0], M.RAMP_ANCHORS[4]]
    lut = M.palette_lut(20)
    assert tuple(lut[17, :3]) == M.DEFAULT_PALETTE[1] and not lut[20:].any() and len(M.DEFAULT_PALETTE) == 16
    assert M.palette_lut(2, [[1, 2, 3], [4, 5, 6, 7]]).tolist()[:3] == [[1, 2, 3, 255], [4, 5, 6, 7], [0, 0, 0, 0]]
    with pytest.raises(ValueError, match="map_tiles_palette"):
        M.load_colors([[1, 2]])
    with pytest.raises(ValueError, match="map_tiles_palette"):
        M.load_colors([[1, 2, 256]])


# ---- PNG and TileJSON ----------------------------------------------------------------------------------------------------------------------
def test_png_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, size=(64, 64, 4), dtype=np.uint8)
    for level in (0, 6, 9):
        p = M.write_png(str(tmp_path / f"t{level}.png"), a, level)
        assert np.array_equal(M.read_png(p), a)
    raw = open(p, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n" and raw[12:16] == b"IHDR" and raw[-8:-4] == b"IEND"
    with pytest.raises(ValueError, match="map_tiles_png_level"):
        M.encode_png(a, 10)
    with pytest.raises(ValueError, match="h, w, 4"):
        M.encode_png(a[..., :3])
    open(p, "wb").write(raw[:-20])
    with pytest.raises(ValueError):
        M.read_png(p)


def test_png_is_read_by_pil(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    a = np.random.default_rng(4).integers(0, 256, size=(64, 128, 4), dtype=np.uint8)
    p = M.write_png(str(tmp_path / "t.png"), a)
    with Image.open(p) as im:
        assert im.mode == "RGBA" and im.size == (128, 64) and np.array_equal(np.asarray(im), a)


def _export(tmp_path, raster, profile=None, **kw):
    out = str(tmp_path / "tiles")
    written = M.export(raster, out, profile, **kw)
    files = sorted(os.path.relpath(os.path.join(r, n), out) for r, _, names in os.walk(out) for n in names)
    assert sorted(os.path.relpath(w, out) for w in written) == files
    return out, files, json.load(open(os.path.join(out, "tilejson.json")))


def test_export_writes_the_tiles_and_tilejson(tmp_path):
    levels, profile, tiles, lvls, ties = export_case("palette")
    out, files, doc = _export(tmp_path, levels, profile, tile=64, ncolors=MR.NCOLORS)
    zmin, zmax = M.zoom_range(profile, (MR.H, MR.W), 3, 64)
    assert doc["tilejson"] == "3.0.0" and doc["tiles"] == ["{z}/{x}/{y}.png"] and (doc["minzoom"], doc["maxzoom"]) == (zmin, zmax) == (11, 14)
    w, s, e, n = doc["bounds"]
    assert 33.9 < w < 34.0 < e < 34.1 and 40.5 < s < n < 40.7 and doc["center"] == [(w + e) / 2, (s + n) / 2, zmin]
    assert doc["colors"] == M.palette_lut(MR.NCOLORS)[: MR.NCOLORS].tolist() and "rescale" not in doc and doc["style"] == "palette"
    rgba, opaque = M.render(levels, profile, tiles, tile=64, ncolors=MR.NCOLORS)
    want = sorted(f"{z}/{x}/{y}.png" for (z, x, y), o in zip(tiles, opaque) if o > 0)
    assert [f for f in files if f.endswith(".png")] == want and 0 < len(want) <= len(tiles)
    for (z, x, y), px, o in zip(tiles, rgba, opaque):
        if o > 0:
            assert np.array_equal(M.read_png(os.path.join(out, str(z), str(x), f"{y}.png")), px)
    assert set(M.TIMINGS) == {"pyramid", "render", "readback", "png"}


def test_export_of_a_cog_uses_its_overviews(tmp_path, monkeypatch):
    a = MR.float_levels(1)[0]
    profile = profile_of("utm_north", dtype="float32")
    path = str(tmp_path / "reg.tif")
    cog.write_cog(path, cog.build_overviews(a, "mean", 2, blocksize=128), dict(profile, nodata=None), blocksize=128)
    assert tiff.overview_count(path) == 2
    monkeypatch.setattr(cog, "build_overviews", lambda *a, **k: pytest.fail("the overviews of the COG are to be used, not rebuilt"))
    out, files, doc = _export(tmp_path, path, tile=64, rescale=(0.0, 1.0))
    assert doc["rescale"] == [0.0, 1.0] and doc["style"] == "ramp" and "colors" not in doc
    levels = [a] + [lv for lv in MR.float_levels(1)[1:]]
    tiles = [tuple(int(v) for v in f[:-4].split("/")) for f in files if f.endswith(".png")]
    rgba, opaque = M.render(levels, profile, tiles, "ramp", 64, rescale=(0.0, 1.0))
    assert len(tiles) >= 4 and (opaque > 0).all()
    for t, px in zip(tiles, rgba):
        assert np.array_equal(M.read_png(os.path.join(out, *map(str, t[:2]), f"{t[2]}.png")), px)


def test_export_defaults_and_refusals(tmp_path):
    levels, profile = MR.float_levels(1), profile_of("utm_north", dtype="float32")
    out, files, doc = _export(tmp_path, levels[0], profile, tile=64, maxzoom=12, minzoom=12)
    finite = levels[0][np.isfinite(levels[0])]
    assert doc["rescale"] == [float(finite.min()), float(finite.max())] and (doc["minzoom"], doc["maxzoom"]) == (12, 12)
    with pytest.raises(ValueError, match="multiple of 64"):
        M.export(levels[0], str(tmp_path / "x"), profile, tile=96)
    with pytest.raises(ValueError, match="style"):
        M.export(levels[0], str(tmp_path / "x"), profile, style="palette")
    with pytest.raises(ValueError, match="map_tiles_rescale"):
        M.export(levels[0], str(tmp_path / "x"), profile, rescale=(2.0, 1.0), tile=64)
    with pytest.raises(ValueError, match="int8 class maps and float32"):
        M.export(levels[0].astype(np.int16), str(tmp_path / "x"), profile)
    with pytest.raises(ValueError, match="profile"):
        M.export(levels[0], str(tmp_path / "x"))


# ---- the imagery ---------------------------------------------------------------------------------------------------------------------------
def write_chips(root, size=32, step=16, bands=4, labels=False, nodata=-9999):
    """Four overlapping ``size`` x ``size`` int16 chips, ``step`` apart, every chip with data of its own (so the overlaps tell the rule
    ``last`` from any other) and a no-data hole in the overlap of all four; ``nodata``: the value of the hole and the file's NODATA tag,
    None: no tag and the hole holds 0.  With ``labels`` also label files and ``set.csv``.  -> (paths, the (3, H, W) float32 mosaic of
    bands 0..2 by rule last)."""
    rng = np.random.default_rng(5)
    X0, Y0 = MR.SOURCES["utm_north"][1][:2]
    side = size + step
    want = np.full((3, side, side), np.nan, dtype=np.float32)
    hole = nodata if nodata is not None else 0
    paths, rows = [], []
    for k, (r0, c0) in enumerate(((0, 0), (0, step), (step, 0), (step, step))):
        a = rng.integers(1, 3000, size=(bands, size, size)).astype(np.int16)
        lo, hi = step + 2, size - 2  # mosaic rows / columns of the hole, inside all four chips
        a[:, lo - r0 : hi - r0, lo - c0 : hi - c0] = hole
        if k == 1:
            a[:, :4, :4] = hole  # a hole of this chip alone where chip 0 lies below: chip 0 shows through
        prof = dict(profile_of("utm_north", (size, size), (X0 + 30.0 * c0, Y0 - 30.0 * r0, 30.0, 30.0), "int16", bands), nodata=nodata)
        p = os.path.join(str(root), f"chip_{k}.tif")
        tiff.write(p, a, prof)
        paths.append(p)
        v = a[:3].astype(np.float32)
        v[a[:3] == hole] = np.nan
        win = want[:, r0 : r0 + size, c0 : c0 + size]
        win[~np.isnan(v)] = v[~np.isnan(v)]
        if labels:
            tiff.write(os.path.join(str(root), f"lab_{k}.tif"), rng.integers(0, 2, (1, size, size)).astype(np.int16))
            rows.append(f"chip_{k}.tif,lab_{k}.tif")
    if labels:
        with open(os.path.join(str(root), "set.csv"), "w") as f:
            f.write("Input,Label\n" + "\n".join(rows) + "\n")
    return paths, want


@pytest.mark.parametrize("nodata", [-9999, None])
def test_merge_chips_of_four_overlapping_chips_with_a_hole(tmp_path, nodata):
    """The file's own NODATA tag, and without one the default of ``chips.*`` (0)."""
    paths, want = write_chips(tmp_path, nodata=nodata)
    X0, Y0 = MR.SOURCES["utm_north"][1][:2]
    out = str(tmp_path / "chips_merged.tif")
    levels, profile = M.merge_chips(paths, bands=(0, 1, 2), out_path=out, tile=64)
    assert levels[0].shape == (3, 48, 48) and np.array_equal(levels[0], want, equal_nan=True) and np.isnan(levels[0][:, 22, 22]).all()
    first = tiff.read(paths[0])[0][:3].astype(np.float32)
    second = tiff.read(paths[1])[0][:3].astype(np.float32)
    assert np.array_equal(levels[0][:, :4, 16:20], first[:, :4, 16:20]) and np.array_equal(levels[0][:, 8:12, 16:20], second[:, 8:12, :4])
    assert not np.array_equal(first[:, 8:12, 16:20], second[:, 8:12, :4])  # the overlap tells the chips apart: the later one won
    assert profile["count"] == 3 and M._source(profile)[1] == (X0, Y0, 30.0, 30.0)
    back, bp = tiff.read(out)
    assert back.dtype == np.float32 and np.array_equal(back, want, equal_nan=True) and cog.validate_cog(out) == []
    written = M.export(levels, str(tmp_path / "tiles_chips"), profile, tile=64, order=(2, 1, 0), rescale=(0.0, 3000.0))
    doc = json.load(open(written[-1]))
    assert doc["style"] == "rgb" and doc["rescale"] == [0.0, 3000.0] and len(written) >= 2
    px = M.read_png(written[0])
    assert set(np.unique(px[..., 3])) <= {0, 255} and (px[..., 3] == 255).any()
    with pytest.raises(ValueError, match="at least one chip"):
        M.merge_chips([])


# ---- the runner ----------------------------------------------------------------------------------------------------------------------------
def _cfg(*overrides):
    from instageo_amd.config import load_config

    return load_config("config", list(overrides))


def test_the_keys_are_off_by_default_and_refused_where_they_cannot_apply(tmp_path):
    from instageo_amd import run

    opts = run.map_tiles_options(_cfg("mode=tile_inference"))
    assert opts["on"] is False and opts["imagery"] is False
    assert opts["export"] == dict(tile=256, palette=None, rescale=None, png_level=6, minzoom="auto", maxzoom="auto")
    assert run.map_tiles_options(_cfg("mode=tile_inference", "test.map_tiles=true", "test.map_tiles_maxzoom=12"))["export"]["maxzoom"] == 12
    assert run.map_tiles_options(_cfg("mode=chip_inference", "test.mosaic=true", "test.map_tiles=true", "test.map_tiles_imagery=true"))["imagery"]
    for overrides, key in (
        (("mode=tile_inference", "test.map_tiles_size=100"), "map_tiles_size"),
        (("mode=tile_inference", "test.map_tiles_size=2048"), "map_tiles_size"),
        (("mode=tile_inference", "test.map_tiles=yes please"), "test.map_tiles "),
        (("mode=tile_inference", "test.map_tiles_minzoom=25"), "map_tiles_minzoom"),
        (("mode=tile_inference", "test.map_tiles_minzoom=9", "test.map_tiles_maxzoom=5"), "map_tiles_minzoom"),
        (("mode=tile_inference", "test.map_tiles_rescale=[3, 1]"), "map_tiles_rescale"),
        (("mode=tile_inference", "test.map_tiles=true", "test.map_tiles_rescale=[0, 1]"), "map_tiles_rescale"),
        (("mode=tile_inference", "test.map_tiles_png_level=12"), "map_tiles_png_level"),
        (("mode=train", "test.map_tiles=true"), "test.map_tiles needs mode"),
        (("mode=chip_inference", "test.map_tiles=true"), "test.mosaic=true"),
        (("mode=tile_inference", "test.map_tiles=true", "test.map_tiles_imagery=true"), "map_tiles_imagery"),
        (("mode=chip_inference", "test.mosaic=true", "test.map_tiles_imagery=true"), "map_tiles_imagery"),
        (("mode=map_tiles",), "test.input"),
    ):
        with pytest.raises(ValueError, match=key):
            run.map_tiles_options(_cfg(*overrides))
    bad = tmp_path / "bad.json"
    bad.write_text("[[1, 2]]")
    with pytest.raises(ValueError, match="map_tiles_palette"):
        run.map_tiles_options(_cfg("mode=tile_inference", f"test.map_tiles_palette={bad}"))


def test_mode_map_tiles_renders_an_existing_file_and_touches_nothing_else(tmp_path, capsys):
    from instageo_amd import run

    cm = MR.class_levels()[0]
    path = str(tmp_path / "prediction_x.tif")
    tiff.write(path, cm[None], dict(profile_of("utm_north"), nodata=-1))
    before = sorted(os.listdir(tmp_path))
    assert run.main(["mode=map_tiles", f"test.input={path}", "test.map_tiles_size=64", "test.map_tiles_maxzoom=13"]) == 0
    assert sorted(os.listdir(tmp_path)) == before + ["tiles_prediction_x"]
    doc = json.load(open(tmp_path / "tiles_prediction_x" / "tilejson.json"))
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["map_tiles"].endswith("tilejson.json")
    assert doc["style"] == "palette" and doc["maxzoom"] == 13 and doc["minzoom"] == 11 and len(doc["colors"]) == 10
    pngs = [os.path.join(r, n) for r, _, names in os.walk(tmp_path / "tiles_prediction_x") for n in names if n.endswith(".png")]
    assert pngs and all(M.read_png(p).shape == (64, 64, 4) for p in pngs)
