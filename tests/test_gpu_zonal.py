"""Zonal statistics on the device (-m gpu): ig_zone_edge_rows, ig_zone_toggle and ig_zone_tally through instageo_amd.zonal against the
pixel-by-pixel reference of tests/zonal_reference.py, array for array; the round trip with the vectoriser; chip and tile inference end
to end.  Every check is exact integer equality.

The rasters (zonal_reference.cases) are the smallest that can break each stage: 37 x 67 (W no multiple of a wave), 3 x 9000 (a workgroup
scans ZCHUNK = 1024 columns in one step, zonal.hip: nine chunks, the last one partial, so the carry between chunks is exercised),
1 x 1, 70 zones on 24 x 40 (two passes, bit 63 and bit 0 of the second pass in use), ties on 8 x 8, 50 random zones on 19 x 23."""
import csv
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import zonal_reference as ZR  # noqa: E402
from instageo_amd import dataloader as DL  # noqa: E402
from instageo_amd import ops, tiff, vectorize, zonal  # noqa: E402
from instageo_amd import postprocess as PP  # noqa: E402
from instageo_amd.infer_utils import chip_inference, tile_inference  # noqa: E402
from instageo_amd.model import PrithviSeg  # noqa: E402
from oracle import prithvi_oracle as O  # noqa: E402

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN = [0.14245495, 0.13921481, 0.12434631, 0.31420089, 0.20743526, 0.12046503]
STD = [0.04036231, 0.04186983, 0.05267646, 0.0822221, 0.06834774, 0.05294205]
TAGS = {33550: (12, (30.0, 30.0, 0.0)), 33922: (12, (0.0, 0.0, 0.0, 399960.0, 4500000.0, 0.0)),
        34735: (3, (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 32613))}


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the shared arrays are read-only


@pytest.mark.parametrize("name", sorted(ZR.cases()))
def test_masks_and_counts_equal_the_reference(name):
    H, W, _ = ZR.cases()[name]
    edges, edge_zone, Z, masks = ZR.reference(name)
    planes = zonal.zone_masks(edges, edge_zone, Z, H, W, DEV)
    want = ZR.to_planes(masks)
    assert planes.dtype == torch.int64 and tuple(planes.shape) == want.shape == ((Z + 63) // 64, H, W)
    assert np.array_equal(planes.cpu().numpy(), want)
    # three classes; fill, and values that are no class (3 = ncls, 100, -7), land in the last column
    cm = ZR.class_map(len(name), H, W, 3, -1, extra=(3, 100, -7))
    counts = zonal.zone_counts(_dev(cm), edges, edge_zone, Z, 3, -1)
    want_c = ZR.ref_counts(cm, masks, 3, -1)
    print(f"{name}: {Z} zones, {len(edges)} edges, {int(masks.sum())} inside pixels, {int(want_c[:, 3].sum())} of them invalid")
    assert counts.dtype == np.int64 and counts.shape == (Z, 4) and np.array_equal(counts, want_c)
    assert np.array_equal(counts.sum(axis=1), masks.sum(axis=(1, 2)))


def test_fill_value_many_classes_accumulation_and_two_runs():
    H, W, _ = ZR.cases()["odd_37x67"]
    edges, edge_zone, Z, masks = ZR.reference("odd_37x67")
    cm = ZR.class_map(5, H, W, 127, fill=5, extra=(127, -128))  # 127 classes (the LDS table at its largest), fill = class value 5
    a = zonal.zone_counts(_dev(cm), edges, edge_zone, Z, 127, fill=5)
    assert np.array_equal(a, ZR.ref_counts(cm, masks, 127, 5)) and a[:, 5].sum() == 0 and a[:, 127].sum() > 0
    assert np.array_equal(a, zonal.zone_counts(_dev(cm), edges, edge_zone, Z, 127, fill=5))
    p1, p2 = (zonal.zone_masks(edges, edge_zone, Z, H, W, DEV) for _ in range(2))
    assert torch.equal(p1, p2)
    # the stages one by one: rows per edge, the toggles (an even number per row and zone inside the raster's columns or not at all),
    # counts accumulate over two calls, and write_mask = 0 leaves the toggles where they were
    e, bit = _dev(edges), _dev(edge_zone.astype(np.uint8))
    rows = ops.zone_edge_rows(e, H)
    yc = 256 * np.arange(H) + 128
    want_rows = ((edges[:, 1, None] <= yc) != (edges[:, 3, None] <= yc)).sum(axis=1)
    assert rows.dtype == torch.int32 and np.array_equal(rows.cpu().numpy(), want_rows)
    first = torch.cumsum(rows, 0, dtype=torch.int64).sub_(rows)
    canvas = torch.zeros((H, W), dtype=torch.int64, device=DEV)
    ops.zone_toggle(e, bit, first, canvas, int(want_rows.sum()))
    toggles = canvas.clone()
    assert int(toggles.ne(0).sum()) > 0
    cm3 = ZR.class_map(6, H, W, 3)
    counts = torch.zeros((64, 4), dtype=torch.int64, device=DEV)
    ops.zone_tally(canvas, _dev(cm3), counts, 3, -1)
    assert torch.equal(canvas, toggles)
    once = counts.cpu().numpy().copy()
    ops.zone_tally(canvas, _dev(cm3), counts, 3, -1, write_mask=True)
    assert np.array_equal(once[:Z], ZR.ref_counts(cm3, masks, 3)) and not once[Z:].any() and np.array_equal(counts.cpu().numpy(), 2 * once)
    assert np.array_equal(canvas.cpu().numpy(), ZR.to_planes(masks)[0])


def test_empty_calls_launch_nothing(monkeypatch):
    calls = []
    real = ops._call
    monkeypatch.setattr(ops, "_call", lambda name, *a, **k: (calls.append(name), real(name, *a, **k))[1])
    none = np.zeros((0, 4), dtype=np.int32), np.zeros(0, dtype=np.int32)
    cm = torch.zeros((5, 7), dtype=torch.int8, device=DEV)
    assert not zonal.zone_counts(cm, *none, 3, 2).any() and zonal.zone_counts(cm, *none, 0, 2).shape == (0, 3)  # E = 0, Z = 0
    assert not zonal.zone_masks(*none, 65, 5, 7, DEV).any() and zonal.zone_masks(*none, 0, 5, 7, DEV).shape == (0, 5, 7)
    e, z = ZR.edges_of([[ZR.rect(0, 0, 1, 1)]])
    assert zonal.zone_masks(e, z, 1, 0, 7, DEV).shape == (1, 0, 7)  # H * W = 0
    assert ops.zone_edge_rows(torch.zeros((0, 4), dtype=torch.int32, device=DEV), 5).shape == (0,)
    assert calls == []
    far = ZR.edges_of([[ZR.rect(0, 50, 4, 60)]])  # below the raster: rows are counted, nothing crosses, nothing else runs
    assert not zonal.zone_counts(cm, *far, 1, 2).any() and calls == ["ig_zone_edge_rows"]


# ---- round trip with the vectoriser --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [4, 8])
def test_polygons_of_the_vectoriser_hold_exactly_their_regions(tmp_path, connectivity):
    """region_rings -> write_geojson -> read_zones -> zone_counts: zone j holds area[j] pixels, all of class cls[j].  Without
    georeferencing, with the golden chip's profile (it carries no georeferencing tags: lattice coordinates again) and with a
    georeferenced profile, whose floats go through repr and back."""
    cm = ZR.class_map(2440, 24, 40, 3)
    d = _dev(cm)
    rings, vertices = vectorize.region_rings(d, connectivity, -1)
    table = PP.region_table(d, connectivity, -1)
    gold = tiff.read_profile(os.path.join(ROOT, "tests", "golden", "tiff", "chip_178_022.tif"))
    n = len(table["root"])
    want = np.zeros((n, 4), dtype=np.int64)
    want[np.arange(n), table["cls"]] = table["area"]
    assert n > 30 and (cm == -1).any() and want.sum() == (cm != -1).sum()
    for k, profile in enumerate((None, gold, {"tags": TAGS})):
        path = vectorize.write_geojson(str(tmp_path / f"p{k}.geojson"), rings, vertices, table, profile)
        zones = zonal.read_zones(path, "root")
        assert [z.id for z in zones] == table["root"].tolist()
        edges, edge_zone = zonal.zones_to_pixels(zones, profile)
        assert len(edges) == int(rings[:, 3].sum()) and (edges % 256 == 0).all()  # lattice corners, to the bit
        assert np.array_equal(zonal.zone_counts(d, edges, edge_zone, n, 3, -1), want), k


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


def _zones_file(path, to_map):
    """Five zones in pixel coordinates, written through ``to_map``: a rectangle over the NODATA block, an off-lattice triangle, a
    MultiPolygon with a hole, one that covers the tile and one beside it."""
    P = lambda ring: [list(to_map(x, y)) for x, y in ring + ring[:1]]  # noqa: E731  closed, as GeoJSON wants
    pix = [("block", [[[(50.0, 30.0), (100.0, 30.0), (100.0, 60.0), (50.0, 60.0)]]]),
           ("tri", [[[(10.3, 5.7), (140.9, 33.2), (70.1, 149.6)]]]),
           ("multi", [[[(5.0, 100.0), (60.0, 100.0), (60.0, 145.0), (5.0, 145.0)], [(20.0, 110.0), (40.0, 110.0), (40.0, 130.0), (20.0, 130.0)]],
                      [[(120.5, 80.5), (149.5, 80.5), (149.5, 120.5)]]]),
           ("all", [[[(-10.0, -10.0), (400.0, -10.0), (400.0, 400.0), (-10.0, 400.0)]]]),
           ("beside", [[[(-50.0, 10.0), (-5.0, 10.0), (-5.0, 90.0)]]])]
    feats = [{"type": "Feature", "properties": {"name": name, "rank": i},
              "geometry": {"type": "MultiPolygon", "coordinates": [[P(r) for r in poly] for poly in polys]} if len(polys) > 1 else
              {"type": "Polygon", "coordinates": [P(r) for r in polys[0]]}} for i, (name, polys) in enumerate(pix)]
    with open(path, "w") as f:
        json.dump({"type": "FeatureCollection", "features": feats}, f)
    # the reference's own quantisation of the same vertices: floor(v * 256 + 0.5) of the pixel coordinates the map values stand for
    quant = lambda x, y, inv: tuple(int(np.floor(v * 256 + 0.5)) for v in inv(*to_map(x, y)))  # noqa: E731
    return str(path), [name for name, _ in pix], lambda inv: [[[quant(x, y, inv) for x, y in r] for poly in polys for r in poly] for _, polys in pix]


def _csv(path):
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    return rows[0], rows[1:]


@pytest.mark.parametrize("blend,H,W", [("nearest", 150, 150), ("gaussian", 150, 170)])
def test_tile_inference_writes_the_zone_table_of_the_sieved_map(tmp_path, blend, H, W):
    net = _tiny()
    src = tmp_path / "chip_T13SDV.tif"
    _geotiff(src, H, W, 3)
    zpath, names, quantised = _zones_file(tmp_path / "zones.geojson", lambda x, y: (399960.0 + 30.0 * x, 4500000.0 - 30.0 * y))
    kw = dict(batch_size=16, constant_multiplier=1e-4, blend=blend, min_region=16)
    if blend != "nearest":
        kw.update(cover_edges=True)
    rest = (net, MEAN, STD, 1, 128, 22)
    tile_inference(str(src), str(tmp_path / "base"), *rest, **kw)
    tile_inference(str(src), str(tmp_path / "off"), *rest, zones=None, **kw)
    out = tile_inference(str(src), str(tmp_path / "on"), *rest, zones=zpath, zone_id_property="name", **kw)
    assert os.listdir(tmp_path / "base") == os.listdir(tmp_path / "off") == ["prediction_T13SDV.tif"]
    assert sorted(os.listdir(tmp_path / "on")) == ["prediction_T13SDV.tif", "zones_T13SDV.csv"] and os.path.basename(out) == "prediction_T13SDV.tif"
    assert _bytes(tmp_path / "base" / "prediction_T13SDV.tif") == _bytes(tmp_path / "off" / "prediction_T13SDV.tif") == _bytes(out)
    pred, _ = tiff.read(out)
    edges, edge_zone = ZR.edges_of(quantised(lambda x, y: ((x - 399960.0) / 30.0, (4500000.0 - y) / 30.0)))
    masks = ZR.ref_masks(edges, edge_zone, 5, H, W)
    want = ZR.ref_counts(pred[0], masks, 2, -1)
    head, rows = _csv(tmp_path / "on" / "zones_T13SDV.csv")
    print(f"end to end {blend}: counts {want.tolist()}")
    assert head == ["zone", "id", "pixels", "invalid", "count_0", "count_1", "area_map_0", "area_map_1"]
    assert [r[:2] for r in rows] == [[str(i), n] for i, n in enumerate(names)]
    assert [[int(v) for v in r[4:6]] + [int(r[3])] for r in rows] == want.tolist()
    assert [int(r[2]) for r in rows] == masks.sum(axis=(1, 2)).tolist() and [[float(v) for v in r[6:]] for r in rows] == (want[:, :2] * 900.0).tolist()
    assert want[0, 2] >= 300 and want[3].sum() == H * W and not want[4].any() and (want[:4, :2].sum(axis=1) > 0).all()  # NODATA block: 10 x 30 fill
    # the table is that of the written (sieved) map, and the sieve did change the map
    raw = tile_inference(str(src), str(tmp_path / "raw"), *rest, zones=zpath, **{**kw, "min_region": 0})
    assert _bytes(raw) != _bytes(out)
    assert [r[1] for r in _csv(tmp_path / "raw" / "zones_T13SDV.csv")[1]] == [str(i) for i in range(5)]  # no property: the feature index
    assert [[int(v) for v in r[4:6]] + [int(r[3])] for r in _csv(tmp_path / "raw" / "zones_T13SDV.csv")[1]] == ZR.ref_counts(tiff.read(raw)[0][0], masks, 2, -1).tolist()


def test_chip_inference_writes_one_zone_table_per_chip(tmp_path):
    net = _tiny()
    ds = DL.SyntheticChipDataset(3, 1, 2, MEAN, STD, device=DEV)
    arr = DL.ArrayChipDataset([ds.raw(i)[0] for i in range(3)], [ds.raw(i)[1] for i in range(3)], MEAN, STD, 1, 1e-4,
                              include_filenames=True, names=[f"chip_{i}.tif" for i in range(3)], device=DEV)
    loader = [DL.infer_collate_fn([arr[i] for i in range(s, min(s + 2, 3))]) for s in range(0, 3, 2)]  # batches of 2 and 1
    zpath, names, quantised = _zones_file(tmp_path / "zones.geojson", lambda x, y: (x, y))  # in-memory chips: lattice coordinates
    assert chip_inference(loader, str(tmp_path / "off"), net, device="gpu") == {}
    assert chip_inference(loader, str(tmp_path / "on"), net, device="gpu", zones=zpath, zone_id_property="rank") == {}
    assert sorted(os.listdir(tmp_path / "off")) == [f"prediction_{i}.tif" for i in range(3)]
    assert sorted(os.listdir(tmp_path / "on")) == [f"prediction_{i}.tif" for i in range(3)] + [f"zones_{i}.csv" for i in range(3)]
    edges, edge_zone = ZR.edges_of(quantised(lambda x, y: (x, y)))
    for i in range(3):
        assert _bytes(tmp_path / "off" / f"prediction_{i}.tif") == _bytes(tmp_path / "on" / f"prediction_{i}.tif")
        pred, _ = tiff.read(str(tmp_path / "on" / f"prediction_{i}.tif"))
        masks = ZR.ref_masks(edges, edge_zone, 5, *pred[0].shape)
        head, rows = _csv(tmp_path / "on" / f"zones_{i}.csv")
        assert head == ["zone", "id", "pixels", "invalid", "count_0", "count_1"] and [r[1] for r in rows] == [str(k) for k in range(5)]
        assert [[int(v) for v in r[4:6]] + [int(r[3])] for r in rows] == ZR.ref_counts(pred[0], masks, 2, -1).tolist()
