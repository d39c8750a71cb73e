"""Region post-processing on the device (-m gpu): ig_ccl_label, ig_region_area, ig_sieve_pass and ig_region_stats through
instageo_amd.postprocess against the host reference (tests/regions_reference.py).  Every check is exact integer equality."""
import csv
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import regions_reference as RR  # noqa: E402
from instageo_amd import postprocess as PP  # noqa: E402
from instageo_amd import tiff  # noqa: E402
from instageo_amd.infer_utils import tile_inference  # noqa: E402
from instageo_amd.model import PrithviSeg  # noqa: E402
from oracle import prithvi_oracle as O  # noqa: E402

DEV = "cuda"
MEAN = [0.14245495, 0.13921481, 0.12434631, 0.31420089, 0.20743526, 0.12046503]
STD = [0.04036231, 0.04186983, 0.05267646, 0.0822221, 0.06834774, 0.05294205]
TAGS = {33550: (12, (30.0, 30.0, 0.0)), 33922: (12, (0.0, 0.0, 0.0, 399960.0, 4500000.0, 0.0)),
        34735: (3, (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 32613))}
SHAPES = [(1, 1), (1, 300), (300, 1), (64, 64), (37, 53), (130, 257)]  # kernel tiles are 64 wide and 16 high


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _patterns(H, W):
    """The maps of one shape, stacked (n, H, W): blobs with 2 and 13 classes and 2 % fill, one class, all fill, checkerboard, stripes
    both ways, rings.  Read-only (shared between tests)."""
    maps = [RR.blobs(H, W, 2, 10 + H), RR.blobs(H, W, 13, 20 + W), np.full((H, W), 5, np.int8), np.full((H, W), -1, np.int8),
            RR.checkerboard(H, W), RR.stripes(H, W), RR.stripes(H, W, vertical=True), RR.rings(H, W)]
    out = np.stack(maps)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _ref_labels(H, W, connectivity):
    out = RR.ref_label_batch(_patterns(H, W), connectivity)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _blob_map(ncls):
    cm = RR.blobs(150, 170, ncls, 100 + ncls)
    cm.setflags(write=False)
    return cm


@functools.lru_cache(maxsize=None)
def _noisy_map():
    """13-class salt and pepper over blobs: peels one layer per pass."""
    rng = np.random.default_rng(77)
    cm = RR.blobs(90, 110, 13, 5).copy()
    salt = rng.random(cm.shape) < 0.5
    cm[salt] = rng.integers(0, 13, size=int(salt.sum()))
    cm.setflags(write=False)
    return cm


@functools.lru_cache(maxsize=None)
def _ref_sieve(key, min_region, connectivity, max_passes):
    cm = {"blob2": _blob_map(2), "blob13": _blob_map(13), "noisy": _noisy_map()}[key]
    return RR.ref_sieve(cm, min_region, connectivity, -1, max_passes)


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("H,W", SHAPES)
def test_labels_equal_the_reference_on_every_shape_and_pattern(H, W, connectivity):
    """All patterns of a shape in one call: n = 8 different maps per launch."""
    cms = _patterns(H, W)
    got = PP.label_regions(_dev(cms), connectivity)
    assert got.dtype == torch.int32 and got.shape == cms.shape
    ref = _ref_labels(H, W, connectivity)
    got = got.cpu().numpy()
    for i in range(len(cms)):
        assert np.array_equal(got[i], ref[i]), (i, int((got[i] != ref[i]).sum()))
    assert (got[3] == -1).all() and (got[2] == 0).all()  # all fill; one class: everything is pixel 0's region
    idx = np.arange(H * W).reshape(H, W)
    if connectivity == 4:
        assert np.array_equal(got[4], idx)  # checkerboard: every pixel its own region
    elif H > 1 and W > 1:
        assert np.array_equal(got[4], (idx // W + idx % W) & 1)  # two regions, rooted at pixels 0 and 1
    one = PP.label_regions(_dev(cms[0]), connectivity)  # the (H, W) form
    assert one.shape == (H, W) and np.array_equal(one.cpu().numpy(), ref[0])


def test_three_images_are_labelled_independently():
    cms = np.stack([RR.blobs(37, 53, 3, s) for s in (1, 2, 3)])
    for connectivity in (4, 8):
        got = PP.label_regions(_dev(cms), connectivity).cpu().numpy()
        assert np.array_equal(got, RR.ref_label_batch(cms, connectivity))
    assert not np.array_equal(got[0], got[1])


@pytest.mark.parametrize("connectivity", [4, 8])
def test_fill_zero_instead_of_minus_one(connectivity):
    cm = RR.blobs(130, 257, 4, 9, fill=0)
    assert cm.min() == 0 and -1 not in cm
    got = PP.label_regions(_dev(cm), connectivity, fill=0).cpu().numpy()
    assert np.array_equal(got == -1, cm == 0) and np.array_equal(got, RR.ref_label(cm, connectivity, fill=0))
    # with the default fill the zeros are a class like any other
    assert (PP.label_regions(_dev(cm), connectivity).cpu().numpy() >= 0).all()


@pytest.mark.parametrize("connectivity", [4, 8])
def test_serpentine_corridor_through_every_tile(connectivity):
    """One one-pixel component across 256 x 256: 4 x 16 tiles, long union chains."""
    cm = RR.serpentine(256)
    got = PP.label_regions(_dev(cm), connectivity).cpu().numpy()
    assert (got[cm == 1] == 0).all()
    assert np.array_equal(got, RR.ref_label(cm, connectivity))


@pytest.mark.parametrize("connectivity", [4, 8])
def test_many_workgroups_on_an_enlarged_map(connectivity):
    """A 64 x 96 random 13-class map enlarged 16 x to 1024 x 1536 (64 x 24 tiles): a block of 16 x 16 equal pixels per small pixel, so
    the components are those of the small map under 4 and under 8, and the root (y, x) moves to (16 y, 16 x)."""
    small = RR.noise(64, 96, 13, 4)
    ref = RR.ref_label(small, connectivity).astype(np.int64)
    big_root = (ref // 96) * 16 * 1536 + (ref % 96) * 16
    want = np.kron(big_root, np.ones((16, 16), dtype=np.int64))
    cm = np.kron(small, np.ones((16, 16), dtype=np.int8))
    got = PP.label_regions(_dev(cm), connectivity)
    assert torch.equal(got.long(), _dev(want))
    again = PP.label_regions(_dev(cm), connectivity)
    assert torch.equal(got, again)


def test_region_area_counts_pixels_at_roots():
    from instageo_amd import ops

    for H, W in ((37, 53), (130, 257)):
        lab = _dev(_ref_labels(H, W, 4))
        area = ops.region_area(lab).cpu().numpy()
        for i, l in enumerate(_ref_labels(H, W, 4)):
            assert np.array_equal(area[i].reshape(-1), RR.ref_area(l))
    big = torch.zeros((1024, 1536), dtype=torch.int32, device=DEV)  # one region of 1.5 M pixels
    a = ops.region_area(big)
    assert int(a[0, 0]) == 1024 * 1536 and int(a.sum()) == 1024 * 1536


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("min_region", [16, 64])
@pytest.mark.parametrize("key", ["blob2", "blob13"])
def test_sieve_on_blob_maps(key, min_region, connectivity):
    cm = _blob_map(2 if key == "blob2" else 13)
    ref, ref_info = _ref_sieve(key, min_region, connectivity, 8)
    got, info = PP.sieve_class_map(_dev(cm), min_region, connectivity, -1, 8)
    print(f"sieve {key} min_region={min_region} conn={connectivity}: {info}, reference {ref_info}")
    assert got.dtype == torch.int8 and np.array_equal(got.cpu().numpy(), ref) and info == ref_info
    assert info["changed"] > 0 and np.array_equal(got.cpu().numpy() == -1, cm == -1)  # fill never changes


def test_sieve_cap_bites_on_the_noisy_map():
    cm = _noisy_map()
    ref, ref_info = _ref_sieve("noisy", 16, 4, 3)
    got, info = PP.sieve_class_map(_dev(cm), 16, 4, -1, 3)
    print(f"noisy map, 3 passes: {info}, reference {ref_info}")
    assert ref_info["passes"] == 3 and ref_info["small_left"] > 0
    assert np.array_equal(got.cpu().numpy(), ref) and info == ref_info


def test_sieve_batch_equals_single_images():
    cms = np.stack([_blob_map(2), _blob_map(13)])
    got, info = PP.sieve_class_map(_dev(cms), 16, 4, -1, 8)
    refs = [_ref_sieve(k, 16, 4, 8) for k in ("blob2", "blob13")]
    assert np.array_equal(got[0].cpu().numpy(), refs[0][0]) and np.array_equal(got[1].cpu().numpy(), refs[1][0])
    assert info["small_left"] == refs[0][1]["small_left"] + refs[1][1]["small_left"]


def test_sieve_rings_one_layer_per_pass():
    r = RR.rings(21, 21)  # 10 rings + the centre, a class each; only the outer ring (80 px) is kept at min_region 78
    for max_passes in (12, 4):
        ref, ref_info = RR.ref_sieve(r, 78, 4, -1, max_passes)
        got, info = PP.sieve_class_map(_dev(r), 78, 4, -1, max_passes)
        assert np.array_equal(got.cpu().numpy(), ref) and info == ref_info
        assert info["passes"] == min(10, max_passes) and info["changed"] == info["passes"]
    assert (got.cpu().numpy()[5:16, 5:16] == r[5:16, 5:16]).all() and (got.cpu().numpy()[:5] == 0).all()  # 4 passes: rings 1 - 4 gone


def test_sieve_ties_fill_and_identity():
    def cm(rows):
        return np.array([[-1 if ch == "." else int(ch) for ch in r] for r in rows], dtype=np.int8)

    for rows, want in ((["1112333", "1112333"], 1), (["3332111", "3332111"], 3)):  # equal areas: the smaller label wins
        t = cm(rows)
        got, info = PP.sieve_class_map(_dev(t), 3, 4)
        assert (got.cpu().numpy()[:, 3] == want).all() and info == {"passes": 1, "changed": 1, "small_left": 0}
        assert np.array_equal(got.cpu().numpy(), RR.ref_sieve(t, 3, 4)[0])
    t = cm(["1121333", "1121333"])  # the larger kept neighbour wins; small neighbours do not count; both columns change in one pass
    got, info = PP.sieve_class_map(_dev(t), 3, 4)
    assert np.array_equal(got.cpu().numpy(), cm(["1113333", "1113333"])) and info == {"passes": 1, "changed": 2, "small_left": 0}
    e = cm(["00000", "0...0", "0.1.0", "0...0", "00000"])  # enclosed by fill: stays
    for connectivity in (4, 8):
        got, info = PP.sieve_class_map(_dev(e), 4, connectivity)
        assert np.array_equal(got.cpu().numpy(), e) and info == {"passes": 0, "changed": 0, "small_left": 1}
    b = _blob_map(13)
    for mr in (0, 1):
        got, info = PP.sieve_class_map(_dev(b), mr)
        assert np.array_equal(got.cpu().numpy(), b) and info == {"passes": 0, "changed": 0, "small_left": 0}
    src = _dev(b)
    PP.sieve_class_map(src, 64)
    assert np.array_equal(src.cpu().numpy(), b)  # the input is not written


def test_two_runs_are_bit_identical():
    cm = _dev(_noisy_map())
    a, ia = PP.sieve_class_map(cm, 16, 8, -1, 8)
    b, ib = PP.sieve_class_map(cm, 16, 8, -1, 8)
    assert torch.equal(a, b) and ia == ib
    assert torch.equal(PP.label_regions(cm, 8), PP.label_regions(cm, 8))


@pytest.mark.parametrize("connectivity", [4, 8])
def test_region_table_equals_the_reference(connectivity):
    cms = np.stack([_blob_map(2), _blob_map(13)])
    ref = RR.ref_table(cms, connectivity)
    got = PP.region_table(_dev(cms), connectivity)
    assert list(got) == list(PP.TABLE_COLUMNS)
    for k in PP.TABLE_COLUMNS:
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), k
    assert got["area"].sum() == (cms != -1).sum()
    one = PP.region_table(_dev(cms[1]), connectivity)
    sub = PP.table_of_image(got, 1)
    assert all(np.array_equal(one[k], sub[k]) for k in PP.TABLE_COLUMNS)
    empty = PP.region_table(_dev(np.full((5, 7), -1, np.int8)))
    assert all(len(v) == 0 for v in empty.values())


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
def test_tile_inference_writes_the_sieved_map_and_the_region_table(tmp_path, blend, H, W):
    net = _tiny()
    src = tmp_path / "chip_T13SDV.tif"
    _geotiff(src, H, W, 3)
    kw = dict(batch_size=16, constant_multiplier=1e-4, blend=blend)
    if blend != "nearest":
        kw.update(cover_edges=True, save_probabilities=True)
    args = (str(src),)
    rest = (net, MEAN, STD, 1, 128, 22)  # windows of 128 at stride 22: 2 x 2 on the square tile, 2 x 3 with the edge column on 150 x 170
    base = tile_inference(*args, str(tmp_path / "base"), *rest, **kw)
    zero = tile_inference(*args, str(tmp_path / "zero"), *rest, min_region=0, save_regions=False, **kw)
    out = tile_inference(*args, str(tmp_path / "sieved"), *rest, min_region=16, save_regions=True, **kw)
    names = ["prediction_T13SDV.tif", "regions_T13SDV.csv"] + (["probability_T13SDV.tif"] if blend != "nearest" else [])
    assert sorted(os.listdir(tmp_path / "sieved")) == sorted(names) and os.path.basename(out) == "prediction_T13SDV.tif"
    assert sorted(os.listdir(tmp_path / "base")) == sorted(n for n in names if n.endswith(".tif"))
    for n in os.listdir(tmp_path / "base"):  # the default call is byte-identical to min_region=0
        assert _bytes(tmp_path / "base" / n) == _bytes(tmp_path / "zero" / n), n
    if blend != "nearest":  # the probabilities describe the blend before the sieve
        assert _bytes(tmp_path / "base" / names[2]) == _bytes(tmp_path / "sieved" / names[2])
    raw, _ = tiff.read(base)
    pred, prof = tiff.read(out)
    assert pred.shape == (1, H, W) and pred.dtype == np.int8 and prof["tags"][33550][1] == (30.0, 30.0, 0.0)
    want, info = PP.sieve_class_map(_dev(raw[0]), 16, 4, -1, 8)
    print(f"end to end {blend}: {info}, {len(np.unique(raw[0]))} values in the raw map")
    assert np.array_equal(pred[0], want.cpu().numpy()) and (pred[0, 40:50, 60:90] == -1).all()
    table = PP.region_table(want, 4, -1)
    with open(tmp_path / "sieved" / "regions_T13SDV.csv", newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == list(PP.TABLE_COLUMNS) + ["x", "y", "area_map"] and len(rows) == 1 + len(table["root"])
    for i, r in enumerate(rows[1:]):
        assert [int(v) for v in r[:8]] == [int(table[k][i]) for k in PP.TABLE_COLUMNS[:8]]
        assert float(r[8]) == table["centroid_row"][i] and float(r[9]) == table["centroid_col"][i]
        assert float(r[10]) == 399960.0 + (table["centroid_col"][i] + 0.5) * 30.0
        assert float(r[11]) == 4500000.0 - (table["centroid_row"][i] + 0.5) * 30.0 and float(r[12]) == table["area"][i] * 900.0
