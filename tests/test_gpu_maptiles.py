"""Map tiles rendered on the device (-m gpu): ``ig_tile_render`` against the sequential twin (tests/maptiles_reference.py) for sources in
UTM north and south, EPSG:4326 and EPSG:3857 (the affine path), tiles of one and of 2 x 2 blocks inside, across each edge and outside the
source, one tile per level in one launch, all three styles, stores into a poisoned output from unaligned levels, invalid levels and grids,
no tiles, determinism, ``export`` and ``merge_chips`` on the device against the host path, file for file, and ``run.main`` through
``tile_inference`` and ``chip_inference`` with a mosaic, with the ``test.map_tiles*`` keys off and on.

Every case is one the twin reports free of ties (no pixel whose level-scaled u or v lies within 1e-6 of an integer: asserted before
anything is compared), so every comparison is exact equality on all bytes and all ``opaque`` counts."""
import json
import os

import numpy as np
import pytest
import torch

import maptiles_reference as MR
from instageo_amd import maptiles as M
from instageo_amd import ops
from test_cpu_maptiles import export_case

pytestmark = pytest.mark.gpu
POISON = (0xA5, 0xA5, 0xA5, 0x00)  # a pixel the kernel never stores: colour without alpha


def _dev_levels(levels, off=0):
    """The levels on the device; level 0 starts ``off`` bytes behind a 16-byte boundary."""
    out = []
    for k, lv in enumerate(levels):
        lv = np.ascontiguousarray(lv)
        pad = (off if k == 0 else 0) // lv.itemsize
        buf = torch.zeros(lv.size + pad, dtype=torch.from_numpy(lv).dtype, device="cuda")
        t = buf[pad:].view(lv.shape)
        t.copy_(torch.from_numpy(lv))
        out.append(t)
    return out


def _kw(style, fill=MR.FILL):
    a = MR.STYLE_ARGS[style]
    return dict(lut=a.get("lut"), ncolors=a.get("ncolors", 0), fill=fill if style == "palette" else -1, rescale=(MR.LO, MR.HI),
                order=a.get("order", (0, 1, 2)))


def _render(name, tile, style, fill=MR.FILL, off=0, out=None):
    system, grid = MR.SOURCES[name]
    grids, lvls = MR.tile_cases(name, tile)
    return ops.tile_render(_dev_levels(MR.levels_of(style), off), system, grid, grids, lvls, tile, style, out=out, **_kw(style, fill))


@pytest.mark.parametrize("name,tile,style", MR.CASES)
def test_tile_render_equals_the_twin(name, tile, style):
    want, opaque, ties = MR.twin(name, tile, style)
    assert ties == 0
    rgba, got = _render(name, tile, style)
    assert np.array_equal(got.cpu().numpy(), opaque) and np.array_equal(rgba.cpu().numpy(), want)
    if tile == 64:
        assert opaque[5] == 0 and not rgba[5].any() and opaque[0] > 0  # the tile wholly outside


def test_fill_that_is_a_class_is_transparent():
    want, opaque, ties = MR.twin("utm_north", 64, "palette", 2)
    assert ties == 0 and (opaque < MR.twin("utm_north", 64, "palette")[1])[[0, 6, 7]].all()
    rgba, got = _render("utm_north", 64, "palette", fill=2)
    assert np.array_equal(got.cpu().numpy(), opaque) and np.array_equal(rgba.cpu().numpy(), want)


@pytest.mark.parametrize("style,off", [("palette", 2), ("ramp", 4), ("rgb", 4)])
def test_every_pixel_is_stored_from_unaligned_levels(style, off):
    """rgba pre-filled with a pixel the kernel never writes; level 0 starts 2 bytes (int8) or one element (float32) off a 16-byte
    boundary."""
    for tile in (64, 128):
        want, opaque, ties = MR.twin("geographic" if style == "palette" else "utm_north", tile, style)
        assert ties == 0
        n = len(opaque)
        out = torch.tensor(POISON, dtype=torch.uint8, device="cuda").repeat(n, tile, tile, 1).contiguous()
        name = "geographic" if style == "palette" else "utm_north"
        system, grid = MR.SOURCES[name]
        grids, lvls = MR.tile_cases(name, tile)
        levels = _dev_levels(MR.levels_of(style), off)
        assert levels[0].data_ptr() % 16 == off
        rgba, got = ops.tile_render(levels, system, grid, grids, lvls, tile, style, out=out, **_kw(style))
        assert rgba is out
        poison = (rgba == torch.tensor(POISON, dtype=torch.uint8, device="cuda")).all(dim=-1)
        assert not poison.any()
        assert np.array_equal(got.cpu().numpy(), opaque) and np.array_equal(rgba.cpu().numpy(), want)


def test_invalid_levels_and_grids_give_transparent_tiles_and_no_tiles_nothing():
    system, grid = MR.SOURCES["utm_north"]
    good = MR.tile_cases("utm_north", 64)[0][0]
    grids = [good, good, good, (np.nan, good[1], good[2], good[3]), (good[0], good[1], 0.0, good[3]), (good[0], good[1], good[2], np.inf), good]
    lvls = [0, -1, MR.NLEVELS, 0, 0, 0, 0]
    levels = _dev_levels(MR.levels_of("palette"))
    out = torch.tensor(POISON, dtype=torch.uint8, device="cuda").repeat(len(grids), 64, 64, 1).contiguous()
    rgba, opaque = ops.tile_render(levels, system, grid, grids, lvls, 64, "palette", out=out, **_kw("palette"))
    want = MR.twin("utm_north", 64, "palette")
    assert opaque.tolist() == [want[1][0], 0, 0, 0, 0, 0, want[1][0]]
    assert not rgba[1:6].any() and np.array_equal(rgba[0].cpu().numpy(), want[0][0]) and torch.equal(rgba[0], rgba[6])
    # a source grid that is not positive: every tile transparent
    rgba, opaque = ops.tile_render(levels, system, (grid[0], grid[1], -30.0, 30.0), grids[:1], [0], 64, "palette", **_kw("palette"))
    assert opaque.tolist() == [0] and not rgba.any()
    rgba, opaque = ops.tile_render(levels, system, grid, np.zeros((0, 4)), [], 64, "palette", **_kw("palette"))
    assert tuple(rgba.shape) == (0, 64, 64, 4) and opaque.numel() == 0


def test_two_launches_give_the_same_bits():
    a = _render("utm_south", 64, "rgb")
    b = _render("utm_south", 64, "rgb")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_render_on_the_device_equals_the_host_path():
    """maptiles.render with the level choice of the host, true XYZ tiles."""
    levels, profile, tiles, lvls, ties = export_case("palette")
    assert ties == 0
    host = M.render(levels, profile, tiles, tile=64, ncolors=MR.NCOLORS)
    dev = M.render(_dev_levels(levels), profile, tiles, tile=64, ncolors=MR.NCOLORS)
    assert dev[0].is_cuda and np.array_equal(dev[0].cpu().numpy(), host[0]) and np.array_equal(dev[1].cpu().numpy(), host[1])
    assert host[1].sum() > 0


@pytest.mark.parametrize("style", ["palette", "ramp", "rgb"])
def test_export_on_the_device_writes_the_bytes_of_the_host_path(tmp_path, style):
    levels, profile, tiles, lvls, ties = export_case(style)
    assert ties == 0
    outs = {}
    for dev in (None, "cuda"):
        out = str(tmp_path / f"out_{dev}")
        M.export(levels, out, profile, tile=64, device=dev, order=MR.ORDER)
        outs[dev] = out
    seen = 0
    for root, _, names in os.walk(outs[None]):
        for n in names:
            pa = os.path.join(root, n)
            assert open(pa, "rb").read() == open(os.path.join(outs["cuda"], os.path.relpath(pa, outs[None])), "rb").read(), pa
            seen += 1
    assert seen >= 5 and seen == sum(len(f) for _, _, f in os.walk(outs["cuda"]))


def test_entry_point_with_no_tiles_touches_no_pointer():
    from instageo_amd import _lib

    for style, es, bands in ((0, 1, 1), (1, 4, 1), (2, 4, 3)):
        _lib.call("ig_tile_render", None, 3, es, bands, MR.H, MR.W, None, None, None, None, 0, 64, style, None, 5, -1, 0.0, 1.0, 0, 1, 2, None, None, None)
    with pytest.raises(_lib.HipLibraryError, match="tile must be a multiple of 64"):
        _lib.call("ig_tile_render", None, 3, 1, 1, MR.H, MR.W, None, None, None, None, 0, 96, 0, None, 5, -1, 0.0, 1.0, 0, 1, 2, None, None, None)


# ---- merge_chips and the runner --------------------------------------------------------------------------------------------------------------
from test_cpu_maptiles import write_chips  # noqa: E402


def _listing(folder):
    return sorted(os.path.relpath(os.path.join(r, n), folder) for r, _, names in os.walk(folder) for n in names)


def _same_files(a, b, names):
    for n in names:
        assert open(os.path.join(a, n), "rb").read() == open(os.path.join(b, n), "rb").read(), n


def test_merge_chips_on_the_device_equals_the_host_path(tmp_path):
    paths, want = write_chips(tmp_path, size=64, step=32)
    host = M.merge_chips(paths, out_path=str(tmp_path / "host.tif"), tile=64)
    dev = M.merge_chips(paths, device="cuda", out_path=str(tmp_path / "dev.tif"), tile=64)
    assert len(host[0]) == len(dev[0]) >= 2 and dev[1] == host[1]
    for h, d in zip(host[0], dev[0]):
        assert d.is_cuda and np.array_equal(d.cpu().numpy().view(np.uint32), np.ascontiguousarray(h).view(np.uint32))
    assert np.array_equal(host[0][0], want, equal_nan=True)
    assert open(tmp_path / "host.tif", "rb").read() == open(tmp_path / "dev.tif", "rb").read()


def _checkpoint(tmp_path, extra=()):
    from instageo_amd.config import load_config
    from instageo_amd.factory import create_model

    common = ["model.model_name=prithvi_eo_tiny", "model.load_pretrained_weights=False", "dataloader.constant_multiplier=0.0001",
              "train.batch_size=4"] + list(extra)
    mod = create_model(load_config("config", ["mode=train"] + common), device="cuda")
    ck = str(tmp_path / "ck.ckpt")
    torch.save({"state_dict": mod.checkpoint_state_dict()}, ck)
    return common + [f"checkpoint_path={ck}"]


# the grid of the runner's tile: that of the twin's UTM source moved by a few irrational-looking metres, checked to be free of ties
TILE_GRID = (MR.SOURCES["utm_north"][1][0] + 1.4142, MR.SOURCES["utm_north"][1][1] - 2.2361, 30.0, 30.0)


def _tile_file(path, H=260, W=260):
    from instageo_amd import crs, tiff

    rng = np.random.default_rng(6)
    arr = rng.integers(0, 10000, size=(6, H, W)).astype(np.int16)
    arr[:, 100:120, 200:230] = -9999
    x, y = TILE_GRID[:2]
    tags = {**crs.geokeys(32636), 33550: (12, (30.0, 30.0, 0.0)), 33922: (12, (0.0, 0.0, 0.0, x, y, 0.0))}
    tiff.write(str(path), arr, {"tags": tags, "nodata": -9999}, compress="deflate")


def test_run_py_tile_inference_with_and_without_map_tiles(tmp_path):
    """Without the keys the output folder holds what it held before; with ``test.map_tiles`` the same files, byte for byte, and
    ``tiles_<name>/`` beside them."""
    from instageo_amd import run, tiff

    common = _checkpoint(tmp_path)
    roots = {}
    for tag, extra in (("off", []), ("on", ["test.map_tiles=true", "test.map_tiles_size=64"])):
        root = tmp_path / tag
        os.makedirs(root)
        _tile_file(root / "tile_a.tif")
        assert run.main(["--output-dir", str(root / "out"), "mode=tile_inference", "test_filepath=tile_a.tif", f"root_dir={root}"] + common + extra) == 0
        roots[tag] = str(root / "predictions")
    assert _listing(roots["off"]) == ["prediction_tile_a.tif"]
    on = _listing(roots["on"])
    assert [f for f in on if not f.startswith("tiles_tile_a" + os.sep)] == ["prediction_tile_a.tif"]
    _same_files(roots["off"], roots["on"], ["prediction_tile_a.tif"])
    doc = json.load(open(os.path.join(roots["on"], "tiles_tile_a", "tilejson.json")))
    pred, prof = tiff.read(os.path.join(roots["on"], "prediction_tile_a.tif"))
    zmin, zmax = doc["minzoom"], doc["maxzoom"]
    assert doc["style"] == "palette" and doc["name"] == "tile_a" and "rescale" not in doc and len(doc["colors"]) == int(pred.max()) + 1
    pngs = [f for f in on if f.endswith(".png")]
    assert pngs and {int(f.split(os.sep)[1]) for f in pngs} == set(range(zmin, zmax + 1)) and len(on) == len(pngs) + 2
    # the tiles are those of the host path on the written file (a geometry the twin reports free of ties)
    from instageo_amd import cog
    from test_cpu_maptiles import xyz_grid

    nlevels = len(cog.level_shapes(260, 260, "auto", 64)) + 1
    every = [t for z in range(zmin, zmax + 1) for t in M.covering_tiles(prof, (260, 260), z)]
    lv = M.choose_levels(prof, (260, 260), every, nlevels, 64)
    assert M._source(prof)[1] == TILE_GRID
    assert sum(MR.scaled_coords(MR.U36, TILE_GRID, xyz_grid(*t, 64), 64, int(k))[2] for t, k in zip(every, lv)) == 0
    M.export(os.path.join(roots["on"], "prediction_tile_a.tif"), str(tmp_path / "host_tiles"), tile=64, name="tile_a")
    assert _listing(str(tmp_path / "host_tiles")) == [os.path.relpath(f, "tiles_tile_a") for f in on if f != "prediction_tile_a.tif"]
    _same_files(str(tmp_path / "host_tiles"), os.path.join(roots["on"], "tiles_tile_a"), _listing(str(tmp_path / "host_tiles")))


def test_run_py_tile_inference_of_a_regression_head_renders_the_ramp(tmp_path):
    from instageo_amd import run, tiff

    common = _checkpoint(tmp_path, ["is_reg_task=True"])
    _tile_file(tmp_path / "tile_a.tif")
    assert run.main(["--output-dir", str(tmp_path / "out"), "mode=tile_inference", "test_filepath=tile_a.tif", f"root_dir={tmp_path}",
                     "test.map_tiles=true", "test.map_tiles_size=64", "test.blend=gaussian", "test.stride=112", "test.cover_edges=true"] + common) == 0
    pdir = str(tmp_path / "predictions")
    files = _listing(pdir)
    assert [f for f in files if not f.startswith("tiles_tile_a" + os.sep)] == ["prediction_tile_a.tif"]
    pred = tiff.read(os.path.join(pdir, "prediction_tile_a.tif"))[0]
    assert pred.dtype == np.float32
    doc = json.load(open(os.path.join(pdir, "tiles_tile_a", "tilejson.json")))
    finite = pred[np.isfinite(pred)]
    assert doc["style"] == "ramp" and doc["rescale"] == [float(finite.min()), float(finite.max())] and "colors" not in doc
    assert any(f.endswith(".png") for f in files)


def test_run_py_chip_inference_mosaic_with_and_without_map_tiles_and_imagery(tmp_path):
    """``test.mosaic=true`` alone, with ``test.map_tiles`` and with ``test.map_tiles_imagery``: the earlier files keep their bytes;
    ``tiles_merged/``, then ``tiles_chips/`` and ``chips_merged.tif`` appear beside them."""
    from instageo_amd import run, tiff

    common = _checkpoint(tmp_path) + ["test.mosaic=true", "test.img_size=256", "dataloader.no_data_value=-9999",
                                      "dataloader.bands=[0,1,2,3,4,5]", "test.cog_blocksize=128"]
    roots = {}
    for tag, extra in (("off", []), ("tiles", ["test.map_tiles=true", "test.map_tiles_size=64"]),
                       ("imagery", ["test.map_tiles=true", "test.map_tiles_size=64", "test.map_tiles_imagery=true"])):
        root = tmp_path / tag
        os.makedirs(root)
        paths, want = write_chips(root, size=256, step=128, bands=6, labels=True)
        assert run.main(["--output-dir", str(root / "out"), "mode=chip_inference", "test_filepath=set.csv", f"root_dir={root}"] + common + extra) == 0
        roots[tag] = str(root / "predictions")
    off = _listing(roots["off"])
    assert "predictions_merged.tif" in off and not any(f.startswith("tiles_") or f.startswith("chips_merged") for f in off)
    tiles = _listing(roots["tiles"])
    assert [f for f in tiles if not f.startswith("tiles_merged" + os.sep)] == off
    _same_files(roots["off"], roots["tiles"], off)
    doc = json.load(open(os.path.join(roots["tiles"], "tiles_merged", "tilejson.json")))
    assert doc["style"] == "palette" and doc["name"] == "merged" and any(f.endswith(".png") for f in tiles)
    imagery = _listing(roots["imagery"])
    assert [f for f in imagery if not f.startswith("tiles_chips" + os.sep) and f != "chips_merged.tif"] == tiles
    _same_files(roots["tiles"], roots["imagery"], tiles)
    doc = json.load(open(os.path.join(roots["imagery"], "tiles_chips", "tilejson.json")))
    assert doc["style"] == "rgb" and doc["rescale"] == [0.0, 3000.0] and any(f.startswith("tiles_chips") and f.endswith(".png") for f in imagery)
    got = tiff.read(os.path.join(roots["imagery"], "chips_merged.tif"))[0]
    assert got.dtype == np.float32 and np.array_equal(got, want, equal_nan=True)
