"""Mosaic of per-chip predictions on the device (-m gpu): ig_mosaic_paste against the pixel-by-pixel reference of tests/mosaic_reference.py
on every case, rule and dtype, and chip inference -> merge_predictions end to end.  Every comparison is exact: array_equal, and for floats
on the uint32 views, so NaN positions and the sign of zero count.

The cases (mosaic_reference.CASES) are the smallest shapes at which a kernel whose workgroup owns a 64 x 64 block, whose threads own 16
pixels of a row and whose chip list goes through LDS in chunks can go wrong.  The canvas and the cover raster are exactly H x W and
pre-filled with a value no rule produces on these inputs, so a pixel the kernel did not write shows."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mosaic_reference as MR  # noqa: E402
import zonal_reference as ZR  # noqa: E402
from instageo_amd import cog, mosaic, ops, tiff  # noqa: E402
from instageo_amd import dataloader as DL  # noqa: E402
from instageo_amd.infer_utils import chip_inference  # noqa: E402
from instageo_amd.model import PrithviSeg  # noqa: E402
from oracle import prithvi_oracle as O  # noqa: E402

DEV = "cuda"
MEAN = [0.14245495, 0.13921481, 0.12434631, 0.31420089, 0.20743526, 0.12046503]
STD = [0.04036231, 0.04186983, 0.05267646, 0.0822221, 0.06834774, 0.05294205]
TAGS = {33550: (12, (30.0, 30.0, 0.0)), 33922: (12, (0.0, 0.0, 0.0, 399960.0, 4500000.0, 0.0)),
        34735: (3, (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 32613))}
POISON_I8 = 127  # the cases hold 0..126, -128 and fill (-1 or 5)
POISON_F32 = 0x7FC00001  # a NaN that is not the one the kernel writes


def _run(name, dtype, rule, cover, order=None):
    """ops.mosaic_paste on a case (``order``: the chips permuted) into poisoned tensors -> (canvas, cover or None) as arrays."""
    chips, rects, (H, W), fill = MR.case(name, dtype)
    order = list(range(len(chips))) if order is None else list(order)
    chips, rects = [chips[i] for i in order], np.array([rects[i] for i in order], dtype=np.int64)
    sizes = rects[:, 2] * rects[:, 3]
    packed = torch.from_numpy(np.concatenate([a.reshape(-1) for a in chips])).to(DEV)
    if dtype == "int8":
        out = torch.full((H, W), POISON_I8, dtype=torch.int8, device=DEV)
    else:
        out = torch.full((H, W), POISON_F32, dtype=torch.int32, device=DEV).view(torch.float32)
    want_cover = MR.expected(name, dtype, MR.RULES[dtype][0])[1]
    poison_c = next(v for v in range(254, 0, -1) if not (want_cover == v).any())
    cov = torch.full((H, W), poison_c, dtype=torch.uint8, device=DEV) if cover else None
    res = ops.mosaic_paste(packed, np.cumsum(sizes) - sizes, rects, *mosaic.bins(rects, H, W), (H, W), rule, fill, out=out, cover_out=cov)
    canvas, c = res if cover else (res, None)
    assert canvas is out and c is cov
    return canvas.cpu().numpy(), (c.cpu().numpy() if cover else None)


@pytest.mark.parametrize("cover", [False, True])
@pytest.mark.parametrize("name,dtype,rule", MR.all_cases())
def test_paste_equals_the_reference(name, dtype, rule, cover):
    want, want_cover = MR.expected(name, dtype, rule)
    got, got_cover = _run(name, dtype, rule, cover)
    if dtype == "int8":
        assert not (want == POISON_I8).any()
    else:
        assert not (MR.bits(want) == POISON_F32).any()
    bad = np.argwhere(MR.bits(got) != MR.bits(want)) if dtype == "float32" else np.argwhere(got != want)
    print(f"{name} {dtype} {rule}: canvas {want.shape}, {len(MR.case(name, dtype)[0])} chips, {len(bad)} pixels differ {bad[:4].tolist()}")
    assert MR.same(got, want)
    if cover:
        assert MR.same(got_cover, want_cover)
        if name == "stack":
            assert got_cover[MR.STACK_ALL] == 255


def test_two_runs_are_bit_identical_and_the_byte_path_equals_the_vector_path(monkeypatch):
    for name, dtype, rule in (("stack", "int8", "mode"), ("stack", "float32", "mean"), ("row", "int8", "last")):
        a, ca = _run(name, dtype, rule, True)
        b, cb = _run(name, dtype, rule, True)
        assert MR.same(a, b) and MR.same(ca, cb)
    # 64-column chips at 16-byte aligned places take the 16-byte loads; IG_MOSAIC_VEC=0 sends them through single elements
    rng = np.random.default_rng(3)
    for dtype in ("int8", "float32"):
        chips = [rng.integers(0, 3, size=(8, 64)).astype(np.int8) if dtype == "int8" else rng.random((8, 64)).astype(np.float32) for _ in range(3)]
        rects = [(0, 0, 8, 64), (4, 16, 8, 64), (2, 3, 8, 64)]  # the last one off the 16-column grid: never vector loads
        want = MR.reference(chips, rects, (16, 96), "last")[0]
        d = [torch.from_numpy(c).to(DEV) for c in chips]
        monkeypatch.setenv("IG_MOSAIC_VEC", "1")
        vec = mosaic.paste(d, rects, (16, 96), "last").cpu().numpy()
        monkeypatch.setenv("IG_MOSAIC_VEC", "0")
        one = mosaic.paste(d, rects, (16, 96), "last").cpu().numpy()
        assert MR.same(vec, want) and MR.same(one, want)


@pytest.mark.parametrize("name", ["corner", "stack"])
def test_mode_does_not_depend_on_the_order_of_the_chips(name):
    want, want_cover = MR.expected(name, "int8", "mode")
    n = len(MR.case(name)[0])
    for seed in (1, 2):
        got, cov = _run(name, "int8", "mode", True, order=np.random.default_rng(seed).permutation(n))
        assert MR.same(got, want) and MR.same(cov, want_cover)
    # last and first do depend on it: the reversed order swaps them
    rev = list(range(n))[::-1]
    assert MR.same(_run(name, "int8", "last", False, order=rev)[0], MR.expected(name, "int8", "first")[0])
    assert MR.same(_run(name, "int8", "first", False, order=rev)[0], MR.expected(name, "int8", "last")[0])


def test_paste_takes_device_tensors_and_empty_inputs():
    chips, rects, shape, fill = MR.case("overhang")
    d = [torch.from_numpy(np.array(c)).to(DEV) for c in chips]
    got, cov = mosaic.paste(d, rects, shape, "first", fill, cover=True)
    want, want_cover = MR.expected("overhang", "int8", "first")
    assert got.is_cuda and MR.same(got.cpu().numpy(), want) and MR.same(cov.cpu().numpy(), want_cover)
    # no chips: the canvas is fill / NaN and nothing is read
    none = ops.mosaic_paste(torch.empty(0, dtype=torch.int8, device=DEV), [], np.zeros((0, 4)), [0], [], (70, 130), "mode", 7, cover=True)
    assert (none[0] == 7).all() and (none[1] == 0).all() and tuple(none[0].shape) == (70, 130)
    nan = ops.mosaic_paste(torch.empty(0, dtype=torch.float32, device=DEV), [], np.zeros((0, 4)), [0], [], (3, 5), "mean")
    assert (nan.view(torch.int32) == MR.NAN_BITS).all()
    assert tuple(ops.mosaic_paste(torch.empty(0, dtype=torch.int8, device=DEV), [], np.zeros((0, 4)), [0], [], (0, 5)).shape) == (0, 5)
    # a chip that would be read beyond the packed buffer is refused before the launch
    with pytest.raises(ValueError, match="outside the packed buffer"):
        ops.mosaic_paste(torch.zeros(8, dtype=torch.int8, device=DEV), [0], [(0, 0, 3, 3)], *mosaic.bins([(0, 0, 3, 3)], 4, 4), (4, 4))
    with pytest.raises(ValueError, match="does not go with"):
        ops.mosaic_paste(torch.zeros(9, dtype=torch.float32, device=DEV), [0], [(0, 0, 3, 3)], *mosaic.bins([(0, 0, 3, 3)], 4, 4), (4, 4), "mode")


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------
def _sha(folder, names):
    return {n: hashlib.sha256(open(os.path.join(folder, n), "rb").read()).hexdigest() for n in names}


def test_chip_inference_then_merge_end_to_end(tmp_path):
    net = PrithviSeg(temporal_step=1, num_classes=2, load_pretrained_weights=False, freeze_backbone=True, variant="prithvi_eo_tiny", device=DEV)
    net.load_state_dict(O.make_state_dict(O.make_config("prithvi_eo_tiny", 1, 2), seed=11))
    rng = np.random.default_rng(4)
    x, y = 399960.0, 4500000.0
    names, rects, arrays = [], [], []
    os.makedirs(tmp_path / "chips")
    for name, (r, c) in (("20200101_r0c0", (0, 0)), ("20200101_r0c1", (0, 1)), ("20200101_r1c0", (1, 0)), ("20200101_r1c1", (1, 1)),
                         ("20200201_r0c1", (0, 1))):  # a 2 x 2 grid and a second date over one chip
        a = rng.integers(0, 10000, size=(6, 16, 16)).astype(np.int16)
        p = str(tmp_path / "chips" / f"chip_{name}.tif")
        tags = {**TAGS, 33922: (12, (0.0, 0.0, 0.0, x + 480.0 * c, y - 480.0 * r, 0.0))}
        tiff.write(p, a, {"tags": tags, "nodata": -9999})
        names.append(p), rects.append((16 * r, 16 * c, 16, 16)), arrays.append(a)
    ds = DL.ArrayChipDataset(arrays, [np.zeros((16, 16), dtype=np.float32)] * 5, MEAN, STD, 1, 1e-4, include_filenames=True, names=names, device=DEV)
    loader = [DL.infer_collate_fn([ds[i] for i in range(s, min(s + 3, 5))]) for s in (0, 3)]
    pred = [f"prediction_{os.path.basename(n)[5:]}" for n in names]
    plain, out = str(tmp_path / "plain"), str(tmp_path / "predictions")
    for folder in (plain, out):
        assert chip_inference(loader, folder, net, device="gpu") == {} and sorted(os.listdir(folder)) == sorted(pred)
    zpath = str(tmp_path / "zone.geojson")
    ring = [(10.0, 10.0), (22.0, 10.0), (22.0, 22.0), (10.0, 22.0), (10.0, 10.0)]  # one square over the seam, in pixels of the mosaic
    with open(zpath, "w") as f:
        json.dump({"type": "FeatureCollection", "features": [{"type": "Feature", "properties": {"name": "seam"}, "geometry": {
            "type": "Polygon", "coordinates": [[[x + 30.0 * px, y - 30.0 * py] for px, py in ring]]}}]}, f)
    written = mosaic.merge_predictions(out, out, num_classes=2, cog_blocksize=128, overview_levels=2, save_regions=True, save_polygons=True,
                                       zones=zpath, zone_id_property="name")
    products = ["regions_merged.csv", "polygons_merged.geojson", "zones_merged.csv", "predictions_merged.tif", "cogstats_merged.json"]
    assert written == [os.path.join(out, n) for n in products] and sorted(os.listdir(out)) == sorted(pred + products)
    assert _sha(out, pred) == _sha(plain, pred)  # the per-chip files are those of a run without the mosaic
    maps = [tiff.read(os.path.join(out, n))[0][0] for n in sorted(pred)]
    order = [sorted(pred).index(n) for n in pred]  # the chip index is the sorted name order
    want = MR.reference(maps, [rects[pred.index(n)] for n in sorted(pred)], (32, 32), "last", -1)[0]
    assert order == [0, 1, 2, 3, 4] and np.array_equal(want[:16, 16:], maps[4])  # the second date wins where it lies
    merged = os.path.join(out, "predictions_merged.tif")
    got, prof = tiff.read(merged)
    assert cog.validate_cog(merged) == [] and tiff.overview_count(merged) == 2 and got.dtype == np.int8 and np.array_equal(got[0], want)
    assert prof["tags"][33922] == TAGS[33922] and prof["tags"][34735] == TAGS[34735] and prof["tags"][42113] == (2, "-1")
    # device and host runs write the same bytes
    for tag, device in (("dev", "gpu"), ("host", "cpu")):
        mosaic.merge_predictions([os.path.join(out, n) for n in sorted(pred)], str(tmp_path / tag), num_classes=2, device=device,
                                 cog_blocksize=128, overview_levels=2, save_cover=True)
    files = sorted(os.listdir(tmp_path / "dev"))
    assert files == ["cogstats_merged.json", "cover_merged.tif", "predictions_merged.tif"] == sorted(os.listdir(tmp_path / "host"))
    assert _sha(str(tmp_path / "dev"), files) == _sha(str(tmp_path / "host"), files)
    assert open(tmp_path / "dev" / "predictions_merged.tif", "rb").read() == open(merged, "rb").read()
    twice = np.ones((32, 32), dtype=np.uint8)
    twice[:16, 16:] = 2
    assert np.array_equal(tiff.read(str(tmp_path / "dev" / "cover_merged.tif"))[0][0], twice)
    # the products describe the whole map: region areas sum to its valid pixels, the zone straddles all four chips
    import csv

    rows = list(csv.DictReader(open(os.path.join(out, "regions_merged.csv"))))
    assert sum(int(r["area"]) for r in rows) == int((want != -1).sum()) == 1024
    edges, edge_zone = ZR.edges_of([[ZR.rect(10, 10, 22, 22)]])
    counts = ZR.ref_counts(want, ZR.ref_masks(edges, edge_zone, 1, 32, 32), 2, -1)
    (zrow,) = list(csv.DictReader(open(os.path.join(out, "zones_merged.csv"))))
    assert zrow["id"] == "seam" and int(zrow["pixels"]) == 144 == int(counts.sum())
    assert [int(zrow["count_0"]), int(zrow["count_1"]), int(zrow["invalid"])] == counts[0].tolist()
    geo = json.load(open(os.path.join(out, "polygons_merged.geojson")))
    assert len(geo["features"]) == len(rows)
