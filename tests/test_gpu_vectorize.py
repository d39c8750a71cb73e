"""Vectorisation on the device (-m gpu): ig_edge_mask, ig_edge_link, ig_ring_jump, ig_ring_sums and ig_ring_emit through
instageo_amd.vectorize.region_rings against the sequential tracer of tests/vector_reference.py, array for array, and against its two
rule-free checkers; then tile inference end to end.  Every check is exact integer equality.

The maps (vector_reference.cases) are the smallest that can break each stage.  A closed walk on the lattice has an even number of
edges, so "a ring of 2^k edges and one of 2^k + 1" is 2^6 and 2^6 + 2 here: at E = 2^6 the last of the ceil(log2 E) rounds is needed."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vector_reference as VR  # noqa: E402
from instageo_amd import ops  # noqa: E402
from instageo_amd import postprocess as PP  # noqa: E402
from instageo_amd import tiff, vectorize  # noqa: E402
from instageo_amd import dataloader as DL  # noqa: E402
from instageo_amd.infer_utils import chip_inference, tile_inference  # noqa: E402
from instageo_amd.model import PrithviSeg  # noqa: E402
from oracle import prithvi_oracle as O  # noqa: E402

DEV = "cuda"
MEAN = [0.14245495, 0.13921481, 0.12434631, 0.31420089, 0.20743526, 0.12046503]
STD = [0.04036231, 0.04186983, 0.05267646, 0.0822221, 0.06834774, 0.05294205]
TAGS = {33550: (12, (30.0, 30.0, 0.0)), 33922: (12, (0.0, 0.0, 0.0, 399960.0, 4500000.0, 0.0)),
        34735: (3, (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 32613))}


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the shared maps are read-only


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", sorted(VR.cases()))
def test_rings_equal_the_sequential_tracer(name, connectivity):
    cm = VR.cases()[name]
    rings, vertices = vectorize.region_rings(_dev(cm), connectivity)
    want_r, want_v = VR.reference(name, connectivity)
    assert rings.dtype == np.int64 and vertices.dtype == np.int32 and rings.shape == want_r.shape and vertices.shape == want_v.shape
    assert np.array_equal(rings, want_r) and np.array_equal(vertices, want_v)
    VR.check_areas(rings, vertices, cm, connectivity)
    VR.check_fill(rings, vertices, cm, connectivity)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_three_images_never_link_and_equal_the_single_image_runs(connectivity):
    cms = VR.cases()["blobs_33x31_x3"]
    rings, vertices = vectorize.region_rings(_dev(cms), connectivity)
    assert sorted(set(rings[:, 0].tolist())) == [0, 1, 2]
    for i, cm in enumerate(cms):
        one_r, one_v = vectorize.region_rings(_dev(cm), connectivity)
        sub_r, sub_v = vectorize.rings_of_image(rings, vertices, i)
        assert np.array_equal(sub_r, one_r) and np.array_equal(sub_v, one_v)


def test_fill_value_other_than_minus_one_and_an_empty_batch():
    cm = VR.cases()["blobs_37x53"]
    z = np.where(cm == -1, 0, cm + 1).astype(np.int8)  # classes 1.., fill 0
    rings, vertices = vectorize.region_rings(_dev(z), 4, fill=0)
    want_r, want_v = VR.reference("blobs_37x53", 4)
    want_r = want_r.copy()
    want_r[:, 2] += 1
    assert np.array_equal(rings, want_r) and np.array_equal(vertices, want_v)
    r0, v0 = vectorize.region_rings(torch.empty((0, 5, 7), dtype=torch.int8, device=DEV))
    assert r0.shape == (0, 6) and v0.shape == (0, 2) and r0.dtype == np.int64 and v0.dtype == np.int32


def test_the_spiral_needs_many_rounds_and_the_mask_counts_every_edge():
    """The stages one by one on the spiral: the mask's total is the edge count, the successor map is a permutation, and its two rings of
    several thousand edges keep the jumping going for ceil(log2 length) rounds (the early exit cannot fire before)."""
    cm = VR.cases()["spiral_96"]
    labels = ops.ccl_label(_dev(cm)[None], 4, -1)
    mask, total = ops.edge_mask(labels)
    E = int(total.item())
    m = mask.cpu().numpy()
    assert E == int((m >> 4).sum()) and np.array_equal(m >> 4, sum((m >> s) & 1 for s in range(4)))
    cnt = torch.bitwise_right_shift(mask.view(-1), 4)
    off = torch.cumsum(cnt, 0, dtype=torch.int32).sub_(cnt)
    succ, tail, flag = ops.edge_link(labels, mask, off.view(labels.shape), E)
    s = succ.cpu().numpy()
    assert np.array_equal(np.sort(s), np.arange(E))
    root = vectorize._jump(0, succ)
    lengths = np.bincount(root.cpu().numpy())
    lengths = lengths[lengths > 0]
    assert len(lengths) == 2 and lengths.sum() == E and lengths.min() > 4000
    rounds = []
    real = ops.ring_jump
    try:
        ops.ring_jump = lambda phase, *a, **k: (rounds.append(phase), real(phase, *a, **k))[1]
        vectorize.region_rings(_dev(cm), 4)
    finally:
        ops.ring_jump = real
    need = int(lengths.max() - 1).bit_length()  # ceil(log2 of the longest ring)
    assert need >= 13 and rounds.count(0) in (need, need + 1) and rounds.count(1) in (need, need + 1), (rounds, need)


def test_two_runs_are_bit_identical():
    cm = _dev(VR.cases()["noise_128"])
    for connectivity in (4, 8):
        a, b = vectorize.region_rings(cm, connectivity), vectorize.region_rings(cm, connectivity)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


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


@pytest.mark.parametrize("blend,H,W", [("nearest", 150, 150), ("gaussian", 150, 170)])
def test_tile_inference_writes_the_polygons_of_the_sieved_map(tmp_path, blend, H, W):
    net = _tiny()
    src = tmp_path / "chip_T13SDV.tif"
    _geotiff(src, H, W, 3)
    kw = dict(batch_size=16, constant_multiplier=1e-4, blend=blend, min_region=16, save_regions=True)
    if blend != "nearest":
        kw.update(cover_edges=True)
    rest = (net, MEAN, STD, 1, 128, 22)
    tile_inference(str(src), str(tmp_path / "base"), *rest, **kw)
    tile_inference(str(src), str(tmp_path / "off"), *rest, save_polygons=False, **kw)
    out = tile_inference(str(src), str(tmp_path / "on"), *rest, save_polygons=True, **kw)
    names = ["prediction_T13SDV.tif", "regions_T13SDV.csv"]
    assert sorted(os.listdir(tmp_path / "base")) == names and sorted(os.listdir(tmp_path / "off")) == names
    assert sorted(os.listdir(tmp_path / "on")) == ["polygons_T13SDV.geojson"] + names and os.path.basename(out) == names[0]
    for n in names:  # the key changes no other file, whether it is absent, off or on
        assert _bytes(tmp_path / "base" / n) == _bytes(tmp_path / "off" / n) == _bytes(tmp_path / "on" / n), n
    pred, _ = tiff.read(out)
    table = PP.region_table(_dev(pred[0]), 4, -1)
    doc = json.load(open(tmp_path / "on" / "polygons_T13SDV.geojson"))
    feats = doc["features"]
    print(f"end to end {blend}: {len(feats)} regions, {sum(len(f['geometry']['coordinates']) for f in feats)} rings")
    assert len(feats) == len(table["root"]) >= 1
    for j, f in enumerate(feats):  # the regions_*.csv rows: same regions, same areas
        p = f["properties"]
        assert (p["root"], p["cls"], p["area"], p["area_map"]) == (table["root"][j], table["cls"][j], table["area"][j], table["area"][j] * 900.0)
        twice = sum(sum(x1 * y2 - x2 * y1 for (x1, y1), (x2, y2) in zip(r, r[1:])) for r in f["geometry"]["coordinates"])
        assert twice == 2 * p["area_map"]  # 30 m pixels at integer metres: exact in float64; exterior counter-clockwise, holes clockwise
        assert all(r[0] == r[-1] for r in f["geometry"]["coordinates"])
    # the polygons are those of the written (sieved) map, in map coordinates
    rings, vertices = vectorize.region_rings(_dev(pred[0]), 4, -1)
    want_r, want_v = VR.ref_rings(pred[0], 4)
    assert np.array_equal(rings, want_r) and np.array_equal(vertices, want_v)
    assert sum(len(f["geometry"]["coordinates"]) for f in feats) == len(rings) >= 2  # the NODATA block is a hole at least
    first = feats[0]["geometry"]["coordinates"][0]
    v = vertices[: rings[0, 3]]
    assert first[0] == [399960.0 + 30.0 * v[0, 0], 4500000.0 - 30.0 * v[0, 1]] and first[1] == [399960.0 + 30.0 * v[-1, 0], 4500000.0 - 30.0 * v[-1, 1]]


def test_chip_inference_writes_one_polygon_file_per_chip(tmp_path):
    net = _tiny()
    ds = DL.SyntheticChipDataset(3, 1, 2, MEAN, STD, device=DEV)
    arr = DL.ArrayChipDataset([ds.raw(i)[0] for i in range(3)], [ds.raw(i)[1] for i in range(3)], MEAN, STD, 1, 1e-4,
                              include_filenames=True, names=[f"chip_{i}.tif" for i in range(3)], device=DEV)
    loader = [DL.infer_collate_fn([arr[i] for i in range(s, min(s + 2, 3))]) for s in range(0, 3, 2)]  # batches of 2 and 1
    assert chip_inference(loader, str(tmp_path / "off"), net, device="gpu", connectivity=8) == {}
    assert chip_inference(loader, str(tmp_path / "on"), net, device="gpu", connectivity=8, save_polygons=True) == {}
    assert sorted(os.listdir(tmp_path / "off")) == [f"prediction_{i}.tif" for i in range(3)]
    assert sorted(os.listdir(tmp_path / "on")) == [f"polygons_{i}.geojson" for i in range(3)] + [f"prediction_{i}.tif" for i in range(3)]
    for i in range(3):
        assert _bytes(tmp_path / "off" / f"prediction_{i}.tif") == _bytes(tmp_path / "on" / f"prediction_{i}.tif")
        pred, _ = tiff.read(str(tmp_path / "on" / f"prediction_{i}.tif"))
        rings, vertices = VR.ref_rings(pred[0], 8)
        vectorize.write_geojson(str(tmp_path / "want.geojson"), rings, vertices, PP.region_table(_dev(pred[0]), 8, -1), None)
        assert _bytes(tmp_path / "on" / f"polygons_{i}.geojson") == _bytes(tmp_path / "want.geojson")  # in-memory chips: lattice coordinates
