"""The output path of chip and tile inference (-m gpu): every product of the class map asked for at once gives, file by file, the bytes of
the run that asks for it alone; region tables and rings built on shared labels equal those that label for themselves; a regression head
goes through the same tail.  Every check is equality of bytes, bits or integers.

The tiles are the smallest on which each path differs: 150 x 150 (square: the nearest-centre stitch) and 150 x 170 (blended, with an edge
column of windows), crop 128 at stride 22 (four and six overlapping windows), a 10 x 30 NODATA block, a sieve that changes the map."""
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from instageo_amd import cog, tiff, vectorize  # noqa: E402
from instageo_amd import dataloader as DL  # noqa: E402
from instageo_amd import postprocess as PP  # noqa: E402
from instageo_amd.infer_utils import chip_inference, tile_inference  # noqa: E402
from instageo_amd.model import PrithviSeg  # noqa: E402
from oracle import prithvi_oracle as O  # noqa: E402

DEV = "cuda"
MEAN = [0.14245495, 0.13921481, 0.12434631, 0.31420089, 0.20743526, 0.12046503]
STD = [0.04036231, 0.04186983, 0.05267646, 0.0822221, 0.06834774, 0.05294205]
TAGS = {33550: (12, (30.0, 30.0, 0.0)), 33922: (12, (0.0, 0.0, 0.0, 399960.0, 4500000.0, 0.0)),
        34735: (3, (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 32613))}
RASTERS = ("prediction", "probability", "uncertainty")


@functools.lru_cache(maxsize=None)
def _tiny(ncls=2):
    net = PrithviSeg(temporal_step=1, num_classes=ncls, load_pretrained_weights=False, freeze_backbone=True, variant="prithvi_eo_tiny", device=DEV)
    net.load_state_dict(O.make_state_dict(O.make_config("prithvi_eo_tiny", 1, ncls), seed=11))
    return net


def _geotiff(path, H, W, seed=3):
    rng = np.random.default_rng(seed)
    arr = rng.integers(0, 10000, size=(6, H, W)).astype(np.int16)
    arr[:, 40:50, 60:90] = -9999
    tiff.write(str(path), arr, {"tags": TAGS, "nodata": -9999}, compress="deflate")
    return str(path)


def _zones_file(path, to_map):
    """Three zones given in pixel coordinates and written through ``to_map``: a rectangle over the NODATA block, an off-lattice triangle
    and a rectangle with a hole."""
    pix = [("block", [[(50.0, 30.0), (100.0, 30.0), (100.0, 60.0), (50.0, 60.0)]]),
           ("tri", [[(10.3, 5.7), (140.9, 33.2), (70.1, 149.6)]]),
           ("holed", [[(5.0, 100.0), (60.0, 100.0), (60.0, 145.0), (5.0, 145.0)], [(20.0, 110.0), (40.0, 110.0), (40.0, 130.0), (20.0, 130.0)]])]
    feats = [{"type": "Feature", "properties": {"name": name},
              "geometry": {"type": "Polygon", "coordinates": [[list(to_map(x, y)) for x, y in r + r[:1]] for r in rings]}} for name, rings in pix]
    with open(path, "w") as f:
        json.dump({"type": "FeatureCollection", "features": feats}, f)
    return str(path)


def _files(folder):
    """{name: bytes} of a folder."""
    out = {}
    for name in sorted(os.listdir(folder)):
        with open(os.path.join(folder, name), "rb") as f:
            out[name] = f.read()
    return out


def _same_pixels(a_path, b_path):
    (a, _), (b, _) = tiff.read(str(a_path)), tiff.read(str(b_path))
    u = f"u{a.dtype.itemsize}"
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(u), b.view(u))


def _all_equal_each_alone(run, products):
    """``run(tag, **options)`` -> {name: bytes}.  The run with every product on holds, byte for byte, the files of the runs with one product
    each, and nothing else.  Returns the combined run's files."""
    both = run("all", **{k: v for kw in products.values() for k, v in kw.items()})
    union = {}
    for tag, kw in products.items():
        alone = run(tag, **kw)
        assert any(not n.startswith(RASTERS + ("cogstats",)) for n in alone), tag  # the option did write its product
        for name, data in alone.items():
            assert name in both and both[name] == data, (tag, name)
        union.update(alone)
    assert sorted(both) == sorted(union)
    return both


@pytest.mark.parametrize("blend,H,W", [("nearest", 150, 150), ("gaussian", 150, 170)])
def test_tile_products_asked_for_together_equal_each_product_alone(tmp_path, blend, H, W):
    net = _tiny()
    src = _geotiff(tmp_path / "chip_T13SDV.tif", H, W)
    zpath = _zones_file(tmp_path / "zones.geojson", lambda x, y: (399960.0 + 30.0 * x, 4500000.0 - 30.0 * y))
    kw = dict(batch_size=16, constant_multiplier=1e-4, blend=blend, min_region=16)
    rasters = ["prediction_T13SDV.tif"]
    if blend != "nearest":
        kw.update(cover_edges=True, save_probabilities=True, save_uncertainty=True, tta="flips")
        rasters += ["probability_T13SDV.tif", "uncertainty_T13SDV.tif"]
    products = {"regions": dict(save_regions=True), "polygons": dict(save_polygons=True), "zones": dict(zones=zpath, zone_id_property="name")}

    def run(tag, **options):
        tile_inference(src, str(tmp_path / tag), net, MEAN, STD, 1, 128, 22, **{**kw, **options})
        return _files(tmp_path / tag)

    both = _all_equal_each_alone(run, products)
    tables = ["polygons_T13SDV.geojson", "regions_T13SDV.csv", "zones_T13SDV.csv"]
    assert sorted(both) == sorted(rasters + tables)
    raw = run("raw", min_region=0)
    assert raw["prediction_T13SDV.tif"] != both["prediction_T13SDV.tif"]  # the sieve did change the map the products describe
    # the same as Cloud Optimized GeoTIFFs: the tables keep their bytes, level 0 of every raster holds the strip file's pixels, and the
    # rasters and the statistics are those of the run with cog alone
    alone = run("cog", cog=True, cog_blocksize=128)
    both_cog = _all_equal_each_alone(lambda tag, **o: run(tag + "_cog", cog=True, cog_blocksize=128, **o), products)
    assert sorted(alone) == sorted(rasters + ["cogstats_T13SDV.json"]) and sorted(both_cog) == sorted(rasters + tables + ["cogstats_T13SDV.json"])
    for name in tables:
        assert both_cog[name] == both[name], name
    for name in rasters + ["cogstats_T13SDV.json"]:
        assert both_cog[name] == alone[name], name
    for name in rasters:
        assert cog.validate_cog(str(tmp_path / "all_cog" / name)) == [] and both_cog[name] != both[name]
        assert _same_pixels(tmp_path / "all_cog" / name, tmp_path / "all" / name), name


def test_chip_products_asked_for_together_equal_each_product_alone(tmp_path):
    net = _tiny()
    ds = DL.SyntheticChipDataset(3, 1, 2, MEAN, STD, device=DEV)
    arr = DL.ArrayChipDataset([ds.raw(i)[0] for i in range(3)], [ds.raw(i)[1] for i in range(3)], MEAN, STD, 1, 1e-4,
                              include_filenames=True, names=[f"chip_{i}.tif" for i in range(3)], device=DEV)
    loader = [DL.infer_collate_fn([arr[i] for i in range(s, min(s + 2, 3))]) for s in range(0, 3, 2)]  # batches of 2 and 1
    zpath = _zones_file(tmp_path / "zones.geojson", lambda x, y: (x, y))  # in-memory chips: lattice coordinates
    products = {"regions": dict(save_regions=True), "polygons": dict(save_polygons=True), "zones": dict(zones=zpath, zone_id_property="name")}

    def run(tag, **options):
        assert chip_inference(loader, str(tmp_path / tag), net, device="gpu", connectivity=8, **{"min_region": 16, **options}) == {}
        return _files(tmp_path / tag)

    both = _all_equal_each_alone(run, products)
    assert sorted(both) == sorted(f"{kind}_{i}.{ext}" for i in range(3)
                                  for kind, ext in (("prediction", "tif"), ("regions", "csv"), ("polygons", "geojson"), ("zones", "csv")))
    raw = run("raw", min_region=0)
    assert any(raw[f"prediction_{i}.tif"] != both[f"prediction_{i}.tif"] for i in range(3))  # the sieve did change a map
    assert len({both[f"regions_{i}.csv"] for i in range(3)}) == 3  # every chip has its own table


@pytest.mark.parametrize("connectivity", [4, 8])
def test_tables_and_rings_on_shared_labels_equal_those_that_label_for_themselves(connectivity):
    cm = torch.from_numpy(np.random.default_rng(37).integers(0, 3, size=(3, 37, 53)).astype(np.int8))
    cm[:, 10:13, :] = -1
    cm = cm.to(DEV)
    labels = PP.label_regions(cm, connectivity, -1)
    assert labels.dtype == torch.int32 and labels.shape == cm.shape
    table, shared = PP.region_table(cm, connectivity, -1), PP.region_table(cm, connectivity, -1, labels=labels)
    assert list(shared) == list(table) == list(PP.TABLE_COLUMNS)
    for k in table:
        assert shared[k].dtype == table[k].dtype and np.array_equal(shared[k], table[k]), k
    rings, vertices = vectorize.region_rings(cm, connectivity, -1)
    rings_s, vertices_s = vectorize.region_rings(cm, connectivity, -1, labels=labels)
    assert rings_s.dtype == rings.dtype and np.array_equal(rings_s, rings)
    assert vertices_s.dtype == vertices.dtype and np.array_equal(vertices_s, vertices)
    assert len(table["root"]) > 100
    for i in range(3):  # the table's roots are the rings' labels: one labelling
        assert np.array_equal(table["root"][table["image"] == i], np.unique(rings[rings[:, 0] == i, 1]))


@pytest.mark.parametrize("as_cog", [False, True])
def test_regression_head_writes_one_float_raster(tmp_path, as_cog):
    net = _tiny(ncls=1)
    src = _geotiff(tmp_path / "chip_T13SDV.tif", 150, 170)
    kw = dict(batch_size=16, constant_multiplier=1e-4, blend="gaussian", cover_edges=True)
    strip = tile_inference(src, str(tmp_path / "strip"), net, MEAN, STD, 1, 128, 22, **kw)
    out = tile_inference(src, str(tmp_path / "out"), net, MEAN, STD, 1, 128, 22, cog=True, cog_blocksize=128, **kw) if as_cog else strip
    assert os.listdir(os.path.dirname(out)) == ["prediction_T13SDV.tif"] and os.path.basename(out) == "prediction_T13SDV.tif"
    value, profile = tiff.read(out)
    assert value.dtype == np.float32 and value.shape == (1, 150, 170) and profile["dtype"] == "float32"
    nan = np.isnan(value[0])
    assert nan[40:50, 60:90].all() and int(nan.sum()) == 300
    if as_cog:
        assert cog.validate_cog(out) == [] and cog.validate_cog(strip) != [] and _same_pixels(out, strip)
