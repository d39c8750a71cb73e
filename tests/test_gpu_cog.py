"""Overview pyramids and COG tiles on the device (-m gpu): ig_overview_mode, ig_overview_mean and ig_cog_tiles against the pixel-by-pixel
reference of tests/overview_reference.py, and tile inference with test.cog end to end.  Every comparison is exact: array_equal, and for
floats on the uint32 views, so NaN positions count.

The shapes (overview_reference.CASES) are the smallest that can break each stage of a kernel whose workgroup owns a 64 x 64 block and
emits six levels per launch: 1 x 1, 37 x 67 (odd at several levels, W no multiple of 16 or 64), 64 x 64 and 65 x 129 (a block boundary
plus one), 3 x 9000 (141 blocks in a row, the last one partial), 130 x 70 with 8 levels (the second launch on level 6) and 128 x 192
(multiples of 2^6: the mode rule commutes with the D4 maps).  Where W >= 128, columns 64..127 are all fill / NaN, so a whole block is
empty and its workgroup carries nothing but fill through every level (asserted on the inputs).  The float inputs hold no subnormals:
whether the device keeps or flushes them is not what these tests are about."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import overview_reference as OR  # noqa: E402
from instageo_amd import cog, ops, tiff  # noqa: E402
from instageo_amd.infer_utils import tile_inference  # noqa: E402
from instageo_amd.model import PrithviSeg  # noqa: E402
from oracle import prithvi_oracle as O  # noqa: E402

DEV = "cuda"
MEAN = [0.14245495, 0.13921481, 0.12434631, 0.31420089, 0.20743526, 0.12046503]
STD = [0.04036231, 0.04186983, 0.05267646, 0.0822221, 0.06834774, 0.05294205]
TAGS = {33550: (12, (30.0, 30.0, 0.0)), 33922: (12, (0.0, 0.0, 0.0, 399960.0, 4500000.0, 0.0)),
        34735: (3, (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 32613))}


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the shared arrays are read-only


def _same(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.shape, w.shape)
        if w.dtype == np.float32:
            assert np.array_equal(OR.bits(g), OR.bits(w)), (what, k + 1)
        else:
            assert np.array_equal(g, w), (what, k + 1)


# ---- class maps: the mode rule ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(OR.CASES))
def test_mode_pyramid_equals_the_reference(name):
    H, W, levels = OR.CASES[name]
    cm, want = OR.mode_case(name)  # three classes, fill -1, stray values 3 (= ncls), 100 and -128
    assert OR.empty_blocks(cm, -1) >= (1 if W >= 128 else 0) and (cm == 100).any() == (H * W > 100)  # whole blocks of fill; strays elsewhere
    counts = torch.zeros(4, dtype=torch.int64, device=DEV)
    got = ops.overview_mode(_dev(cm), levels, -1, 3, counts)
    _same(got, want, name)
    hist = OR.histogram(cm, 3, -1)
    print(f"{name}: {levels} levels, histogram {hist.tolist()}, level sizes {[tuple(g.shape) for g in got]}")
    assert np.array_equal(counts.cpu().numpy(), hist) and hist.sum() == H * W


def test_many_classes_fill_as_a_class_counts_accumulate_and_two_runs():
    name = "block_65x129"
    H, W, levels = OR.CASES[name]
    cm, want = OR.mode_case(name, 127, 5, (127, -128))  # 127 classes (the LDS table at its largest), fill = class value 5
    assert (cm[:64, 64:128] == 5).all() and OR.empty_blocks(cm, 5) == 2  # a full block (and the one-row block below it) of nothing but fill
    d = _dev(cm)
    counts = torch.zeros(128, dtype=torch.int64, device=DEV)
    a = ops.overview_mode(d, levels, 5, 127, counts)
    _same(a, want, name)
    once = counts.cpu().numpy().copy()
    assert np.array_equal(once, OR.histogram(cm, 127, 5)) and once[5] == 0 and once[127] >= (cm == 5).sum() > 0
    b = ops.overview_mode(d, levels, 5, 127, counts)  # accumulates over two calls; the levels come out with the same bits
    assert np.array_equal(counts.cpu().numpy(), 2 * once) and all(torch.equal(x, y) for x, y in zip(a, b))
    # without counts nothing is tallied, and a source that is not 16-byte aligned takes the byte path to the same result
    shifted = torch.empty(H * W + 1, dtype=torch.int8, device=DEV)[1:].view(H, W).copy_(d)
    _same(ops.overview_mode(shifted, levels, 5, 127), want, "unaligned")
    wide, want_wide = OR.mode_case("d4_128x192", 127, 5, (127, -128))  # W a multiple of 16: the 16-byte path, aligned and not
    dw = _dev(wide)
    _same(ops.overview_mode(dw, 6, 5, 127), want_wide, "vector")
    _same(ops.overview_mode(torch.empty(128 * 192 + 1, dtype=torch.int8, device=DEV)[1:].view(128, 192).copy_(dw), 6, 5, 127), want_wide, "shifted")


def test_mode_rule_commutes_with_the_d4_maps():
    cm, want = OR.mode_case("d4_128x192")
    maps = [lambda a, k=k, f=f: np.rot90(a[:, ::-1] if f else a, k) for f in (0, 1) for k in range(4)]
    for i, g in enumerate(maps):
        got = ops.overview_mode(_dev(np.ascontiguousarray(g(cm))), 6, -1, 3)
        _same(got, [np.ascontiguousarray(g(w)) for w in want], f"d4 map {i}")


# ---- float rasters: the mean rule ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(OR.CASES))
@pytest.mark.parametrize("bands", [1, 3])
@pytest.mark.parametrize("dyadic", [False, True])
def test_mean_pyramid_equals_the_reference(name, bands, dyadic):
    H, W, levels = OR.CASES[name]
    a, want = OR.mean_case(name, bands, dyadic)
    assert OR.empty_blocks(a) >= (1 if W >= 128 else 0)  # whole blocks of NaN
    d = _dev(a)
    got = ops.overview_mean(d, levels)
    _same(got, want, name)
    nan = sum(int(np.isnan(w).sum()) for w in want)
    print(f"{name} x {bands} {'dyadic' if dyadic else 'random'}: {levels} levels, {nan} NaN results, level sizes {[tuple(g.shape) for g in got]}")
    again = ops.overview_mean(d, levels)
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(got, again))


def test_mean_of_a_band_offset_that_is_not_16_byte_aligned():
    a, want = OR.mean_case("odd_37x67", 3)  # 37 * 67 floats per band: bands 1 and 2 start off a 16-byte boundary (scalar loads)
    _same(ops.overview_mean(_dev(a), 7), want, "odd pitch")
    b, want_b = OR.mean_case("d4_128x192", 3, True)  # W a multiple of 4 and aligned: the 16-byte path; shifted by one float: scalar again
    d = _dev(b)
    _same(ops.overview_mean(d, 6), want_b, "vector")
    _same(ops.overview_mean(torch.empty(d.numel() + 1, dtype=torch.float32, device=DEV)[1:].view(d.shape).copy_(d), 6), want_b, "shifted")


def test_build_overviews_on_the_device_equals_the_numpy_path():
    cm, _ = OR.mode_case("deep_130x70")
    a, _ = OR.mean_case("deep_130x70", 3)
    for levels, block in ((8, 256), ("auto", 16), (0, 256)):
        host, devl = cog.build_overviews(cm, "mode", levels, -1, block), cog.build_overviews(_dev(cm), "mode", levels, -1, block)
        _same(devl, host, f"mode {levels}")
        host, devl = cog.build_overviews(a, "mean", levels, blocksize=block), cog.build_overviews(_dev(a), "mean", levels, blocksize=block)
        _same(devl, host, f"mean {levels}")
    counts = torch.zeros(4, dtype=torch.int64, device=DEV)
    assert len(cog.build_overviews(_dev(cm), "mode", 0, -1, ncls=3, counts=counts)) == 1  # no level asked for: the histogram still comes
    assert np.array_equal(counts.cpu().numpy(), OR.histogram(cm, 3, -1))


# ---- tiles ----------------------------------------------------------------------------------------------------------------------------------
def _tiles_by_slicing(a, tile, pad, predictor):
    B, H, W = a.shape
    ny, nx = -(-H // tile), -(-W // tile)
    out = np.empty((B, ny, nx, tile, tile), dtype=a.dtype)
    for b in range(B):
        for ty in range(ny):
            for tx in range(nx):
                t = np.full((tile, tile), pad, dtype=a.dtype)
                blk = a[b, ty * tile : (ty + 1) * tile, tx * tile : (tx + 1) * tile]
                t[: blk.shape[0], : blk.shape[1]] = blk
                if predictor == 2:
                    u = t.view(f"u{a.dtype.itemsize}")
                    t = np.concatenate([u[:, :1], np.diff(u, axis=1)], axis=1).view(a.dtype)  # unsigned: wraps in the element's width
                out[b, ty, tx] = t
    return out


@pytest.mark.parametrize("H,W", [(37, 67), (130, 300)])
@pytest.mark.parametrize("dtype,pad", [("int8", -1), ("int16", -9999), ("int32", -7), ("float32", None)])
def test_cog_tiles_equal_numpy_slicing_and_padding(H, W, dtype, pad):
    rng = np.random.default_rng(H + len(dtype))
    if dtype == "float32":
        a = rng.random((2, H, W)).astype(np.float32)
        a[:, 5:20, 10:60] = np.nan
        padv, bits = np.uint32(OR.NAN_BITS).view(np.float32), OR.NAN_BITS
    else:
        info = np.iinfo(dtype)
        a = rng.integers(info.min, info.max + 1, size=(2, H, W)).astype(dtype)  # the extremes occur: differences wrap
        padv, bits = pad, int(np.array(pad, dtype=dtype).view(f"u{np.dtype(dtype).itemsize}"))
    for predictor in (1, 2) if dtype != "float32" else (1,):
        got = ops.cog_tiles(_dev(a), 128, bits, predictor).cpu().numpy()
        want = _tiles_by_slicing(a, 128, padv, predictor)
        u = f"u{a.dtype.itemsize}"
        assert got.shape == want.shape == (2, -(-H // 128), -(-W // 128), 128, 128) and np.array_equal(got.view(u), want.view(u)), predictor
        assert np.array_equal(cog._tiles_host(a, 128, bits, predictor), want.view(u))  # the writer's numpy twin
    if dtype == "float32":
        with pytest.raises(Exception, match="integers only"):
            ops.cog_tiles(_dev(a), 128, bits, 2)


def test_write_cog_from_device_levels_gives_the_bytes_of_the_host_path(tmp_path):
    cm, _ = OR.mode_case("deep_130x70")
    prof = {"tags": TAGS, "nodata": -1}
    for kw in (dict(compress="deflate", predictor=2), dict(compress=None)):
        h = cog.write_cog(str(tmp_path / "h.tif"), cog.build_overviews(cm, "mode", 3, -1), prof, 128, **kw)
        d = cog.write_cog(str(tmp_path / "d.tif"), cog.build_overviews(_dev(cm), "mode", 3, -1), prof, 128, **kw)
        assert open(h, "rb").read() == open(d, "rb").read() and cog.validate_cog(d) == []
    a, _ = OR.mean_case("deep_130x70", 3)
    h = cog.write_cog(str(tmp_path / "h.tif"), cog.build_overviews(a, "mean", 2), None, 128)
    d = cog.write_cog(str(tmp_path / "d.tif"), cog.build_overviews(_dev(a), "mean", 2), None, 128)
    assert open(h, "rb").read() == open(d, "rb").read()
    c = cog.convert(h, str(tmp_path / "c.tif"), levels=2, blocksize=128, device=DEV)
    assert open(c, "rb").read() == open(h, "rb").read()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def _tiny(ncls=2):
    net = PrithviSeg(temporal_step=1, num_classes=ncls, load_pretrained_weights=False, freeze_backbone=True, variant="prithvi_eo_tiny", device=DEV)
    net.load_state_dict(O.make_state_dict(O.make_config("prithvi_eo_tiny", 1, ncls), seed=11))
    return net


def _geotiff(path, H, W, seed):
    rng = np.random.default_rng(seed)
    arr = rng.integers(0, 10000, size=(6, H, W)).astype(np.int16)
    arr[:, 40:50, 60:90] = -9999
    tiff.write(str(path), arr, {"tags": TAGS, "nodata": -9999}, compress="deflate")


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("blend,H,W", [("nearest", 280, 280), ("gaussian", 260, 300)])
def test_tile_inference_writes_cogs_whose_level_0_is_the_strip_file(tmp_path, blend, H, W):
    net = _tiny()
    src = tmp_path / "chip_T13SDV.tif"
    _geotiff(src, H, W, 3)
    kw = dict(batch_size=16, constant_multiplier=1e-4, blend=blend, min_region=16)
    names = ["prediction_T13SDV.tif"]
    if blend != "nearest":
        kw.update(cover_edges=True, save_probabilities=True, save_uncertainty=True)
        names += ["probability_T13SDV.tif", "uncertainty_T13SDV.tif"]
    rest = (net, MEAN, STD, 1, 128, 76)
    tile_inference(str(src), str(tmp_path / "off"), *rest, **kw)
    out = tile_inference(str(src), str(tmp_path / "on"), *rest, cog=True, cog_blocksize=128, **kw)
    tile_inference(str(src), str(tmp_path / "again"), *rest, cog=True, cog_blocksize=128, **kw)
    assert sorted(os.listdir(tmp_path / "off")) == sorted(names) and os.path.basename(out) == names[0]
    assert sorted(os.listdir(tmp_path / "on")) == sorted(names + ["cogstats_T13SDV.json"]) == sorted(os.listdir(tmp_path / "again"))
    source_tags = {k: v for k, v in tiff.read_profile(str(src))["tags"].items() if k != 42113}
    n_levels = len(cog.level_shapes(H, W, "auto", 128))
    assert n_levels == 2
    for name in names:
        on, off = str(tmp_path / "on" / name), str(tmp_path / "off" / name)
        assert _bytes(on) == _bytes(tmp_path / "again" / name)  # two runs, the same bytes
        assert cog.validate_cog(on) == [] and cog.validate_cog(off) != [] and tiff.overview_count(on) == n_levels
        a0, p0 = tiff.read(on)
        b0, q0 = tiff.read(off)
        u = f"u{a0.dtype.itemsize}"
        assert a0.dtype == b0.dtype and np.array_equal(a0.view(u), b0.view(u))  # level 0: the pixels of the strip file, bit for bit
        assert repr(p0) == repr(q0) and {k: v for k, v in p0["tags"].items() if k != 42113} == source_tags  # the geo tags of IFD 0
        kind = "mode" if name.startswith("prediction") else "mean"
        want = OR.pyramid(a0, kind, n_levels, -1)
        for k, w in enumerate(want):
            g, pk = tiff.read(on, level=k + 1)
            assert g.shape == w.shape and np.array_equal(g.view(u), w.view(u)), (name, k + 1)
            assert set(pk["tags"]) == {42113} and repr(pk["nodata"]) == repr(p0["nodata"])
        print(f"{blend} {name}: level 0 {a0.shape}, overviews {[w.shape for w in want]}, {os.path.getsize(on)} bytes (strips: {os.path.getsize(off)})")
    pred = tiff.read(str(tmp_path / "on" / names[0]))[0][0]
    with open(tmp_path / "on" / "cogstats_T13SDV.json") as f:
        stats = json.load(f)
    assert stats == OR.seg_stats(pred, 2, -1) and stats["valid_pixels"] + int((pred == -1).sum()) == H * W and (pred == -1).sum() >= 300
    assert _bytes(tmp_path / "on" / "cogstats_T13SDV.json") == _bytes(tmp_path / "again" / "cogstats_T13SDV.json")
    with pytest.raises(ValueError, match="cog_blocksize"):
        tile_inference(str(src), str(tmp_path / "bad"), *rest, cog=True, cog_blocksize=100, **kw)
    assert not os.path.exists(tmp_path / "bad")
