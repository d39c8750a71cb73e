"""Zonal statistics of float rasters on the device (-m gpu): ig_zone_value_tally and ig_zone_value_reduce through instageo_amd.zonal
against the numpy reference of tests/zonal_values_reference.py on the masks of tests/zonal_reference.py.

The rasters are those of zonal_reference.cases, the smallest that can break each stage: 37 x 67 (W no multiple of a wave), 3 x 9000 (nine
chunks of 1024 columns: the carry), 1 x 1, 70 zones on 24 x 40 (two passes, bit 63 and bit 0), ties on 8 x 8, 50 random zones on 19 x 23;
several of them hold zones without a pixel, so the empty-zone path is covered as they are.

Bounds.  Integer-valued data: counts, min, max and the sum are exact (integer sums below 2^53 are exact in any order) and the mean is one
division of that sum, compared at 2 ulp.  Offset data 2^23 + k: std to a relative 1e-9, between what merged triples reach on the CPU
(about 1e-11) and what the sum-of-squares formula loses (2.7e-4 and more), DESIGN.md 3.16.  General floats: |sum - ref| <= n 2^-52
sum|v|, the any-order float64 summation bound with a factor 2, the mean accordingly, std again 1e-9."""
import csv
import json
from functools import lru_cache

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import zonal_reference as ZR  # noqa: E402
import zonal_values_reference as VR  # noqa: E402
from instageo_amd import ops, tiff, zonal  # noqa: E402

DEV = "cuda"
CASES = sorted(ZR.cases())
INSIDE = {"odd_37x67": (11519, 0), "wide_3x9000": (77895, 0), "one_pixel": (3, 1), "seventy_24x40": (18555, 5), "ties_8x8": (161, 1),
          "random_19x23": (5636, 1)}  # inside pixels over all zones, zones without one
MAKERS = {"integer": VR.integer_raster, "offset": VR.offset_raster, "normal": VR.normal_raster}


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the shared arrays are read-only


@lru_cache(maxsize=None)
def _case(kind, name, B):
    """-> (raster, nodata, reference), computed once per (kind, case, bands) and left unchanged."""
    H, W, _ = ZR.cases()[name]
    raster = MAKERS[kind](len(name) + B, B, H, W)
    nodata = None if kind == "offset" else VR.NODATA
    ref = VR.reference(name, raster, nodata)
    raster.setflags(write=False)
    for a in ref:
        a.setflags(write=False)
    return raster, nodata, ref


def _run(name, raster, nodata):
    edges, edge_zone, Z, _ = ZR.reference(name)
    return zonal.zone_values(_dev(raster), edges, edge_zone, Z, nodata)


def _check_shapes_and_empties(got, ref):
    Z, B = ref.valid.shape
    assert got.pixels.dtype == np.int64 and got.pixels.shape == (Z,) and got.valid.dtype == np.int64 and got.valid.shape == (Z, B)
    assert np.array_equal(got.pixels, ref.pixels) and np.array_equal(got.valid, ref.valid)
    none = ref.valid == 0
    for k in ("sum", "mean", "std", "min", "max"):
        a = getattr(got, k)
        assert a.dtype == np.float64 and a.shape == (Z, B) and np.isnan(a[none]).all() and np.isfinite(a[~none]).all(), k
    return ~none


def _ulps(got, want):
    return np.abs(got - want) / np.spacing(np.abs(want))


@pytest.mark.parametrize("name", CASES)
def test_integer_rasters_are_exact(name):
    raster, nodata, ref = _case("integer", name, 3)
    got = _run(name, raster, nodata)
    has = _check_shapes_and_empties(got, ref)
    assert (int(ref.pixels.sum()), int((ref.pixels == 0).sum())) == INSIDE[name]
    print(f"{name}: {len(ref.pixels)} zones, {int(ref.pixels.sum())} inside pixels, {int((~has).all(axis=1).sum())} zones without a valid value, "
          f"max mean error {_ulps(got.mean[has], ref.mean[has]).max() if has.any() else 0:.2f} ulp")
    assert np.array_equal(got.min[has], ref.min[has]) and np.array_equal(got.max[has], ref.max[has])
    assert np.array_equal(np.rint(got.sum[has]), ref.sum[has])  # mean * valid rounds back to the integer
    assert (_ulps(got.mean[has], ref.mean[has]) <= 2).all()
    assert (np.abs(got.std[has] - ref.std[has]) <= 1e-9 * ref.std[has]).all()


@pytest.mark.parametrize("name", ["odd_37x67", "wide_3x9000"])
def test_offset_rasters_keep_their_std(name):
    raster, nodata, ref = _case("offset", name, 2)
    got = _run(name, raster, nodata)
    has = _check_shapes_and_empties(got, ref)
    rel = np.abs(got.std[has] - ref.std[has]) / np.where(ref.std[has] > 0, ref.std[has], 1.0)
    print(f"{name}: std of 2^23 + k, largest zone {int(ref.valid.max())} values: max relative error {rel.max():.3e}; "
          f"mean error {_ulps(got.mean[has], ref.mean[has]).max():.2f} ulp")
    assert ref.std[has].max() > 1.9  # the spread the offset must not swallow
    assert (np.abs(got.std[has] - ref.std[has]) <= 1e-9 * ref.std[has]).all()
    assert np.array_equal(np.rint(got.sum[has]), ref.sum[has]) and (_ulps(got.mean[has], ref.mean[has]) <= 2).all()
    assert np.array_equal(got.min[has], ref.min[has]) and np.array_equal(got.max[has], ref.max[has])


@pytest.mark.parametrize("name", CASES)
def test_general_floats_within_the_summation_bound(name):
    raster, nodata, ref = _case("normal", name, 2)
    got = _run(name, raster, nodata)
    has = _check_shapes_and_empties(got, ref)
    n, bound = ref.valid[has], ref.valid[has] * 2.0**-52 * ref.abs_sum[has]
    err = np.abs(got.sum[has] - ref.sum[has])
    rel = np.abs(got.std[has] - ref.std[has]) / np.where(ref.std[has] > 0, ref.std[has], 1.0)
    print(f"{name}: max sum error / bound {np.max(err / bound) if has.any() else 0:.3e}, max relative std error {rel.max() if has.any() else 0:.3e}")
    assert (err <= bound).all()
    assert (np.abs(got.mean[has] - ref.mean[has]) <= bound / n + 2 * np.spacing(np.abs(ref.mean[has]))).all()
    assert (np.abs(got.std[has] - ref.std[has]) <= 1e-9 * ref.std[has]).all()
    assert np.array_equal(got.min[has], ref.min[has]) and np.array_equal(got.max[has], ref.max[has])


def _bytes(values):
    return [np.ascontiguousarray(a).tobytes() for a in values]


def test_two_runs_band_groups_and_the_canvas():
    # two calls: the same bytes in every array, NaN cells included
    raster, nodata, _ = _case("normal", "seventy_24x40", 2)
    assert _bytes(_run("seventy_24x40", raster, nodata)) == _bytes(_run("seventy_24x40", raster, nodata))
    # 11 bands = a group of 8 and a group of 3: band for band the bytes of eleven single-band calls (two passes of zones)
    raster, nodata, ref = _case("normal", "seventy_24x40", 11)
    many = _run("seventy_24x40", raster, nodata)
    _check_shapes_and_empties(many, ref)
    for b in range(11):
        one = _run("seventy_24x40", raster[b], nodata)  # (H, W): a single band
        assert np.array_equal(one.pixels, many.pixels)
        for k in ("valid", "sum", "mean", "std", "min", "max"):
            assert getattr(one, k).shape == (70, 1) and getattr(one, k)[:, 0].tobytes() == np.ascontiguousarray(getattr(many, k)[:, b]).tobytes(), (k, b)
    # the op: the canvas of toggles is left as it was found, and two calls on it agree bit for bit
    H, W, _ = ZR.cases()["odd_37x67"]
    edges, edge_zone, Z, masks = ZR.reference("odd_37x67")
    raster, nodata, ref = _case("integer", "odd_37x67", 3)
    (p, canvas), = list(zonal._passes(edges, edge_zone, Z, H, W, DEV))
    toggles = canvas.clone()
    assert p == 0 and int(toggles.ne(0).sum()) > 0
    first = ops.zone_value_tally(canvas, _dev(raster), nodata)
    assert torch.equal(canvas, toggles)
    second = ops.zone_value_tally(canvas, _dev(raster), nodata)
    assert torch.equal(canvas, toggles)
    pixels, valid, stats = first
    assert pixels.dtype == torch.int64 and tuple(pixels.shape) == (64,) and tuple(valid.shape) == (64, 3) and tuple(stats.shape) == (64, 3, 4)
    assert stats.dtype == torch.float64 and all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(first, second))
    assert np.array_equal(pixels.cpu().numpy()[:Z], ref.pixels) and np.array_equal(valid.cpu().numpy()[:Z], ref.valid)
    # bits without a zone, and zones without a valid value: valid 0, mean = M2 = 0, min = +inf, max = -inf
    st, none = stats.cpu().numpy(), valid.cpu().numpy() == 0
    assert none[Z:].all() and int(pixels[Z:].sum()) == 0
    assert (st[none][:, :2] == 0).all() and np.isposinf(st[none][:, 2]).all() and np.isneginf(st[none][:, 3]).all()
    # the counting tally on the same canvas still finds the toggles
    counts = torch.zeros((64, 3), dtype=torch.int64, device=DEV)
    ops.zone_tally(canvas, torch.zeros((H, W), dtype=torch.int8, device=DEV), counts, 2, -1)
    assert np.array_equal(counts.cpu().numpy()[:Z, 0], ref.pixels)


@pytest.mark.parametrize("name", ["odd_37x67", "seventy_24x40"])
def test_consistent_with_the_counting_path(name):
    H, W, _ = ZR.cases()[name]
    edges, edge_zone, Z, masks = ZR.reference(name)
    # a float raster that holds the class ids of a class map, no-data = its fill value
    cm = ZR.class_map(len(name), H, W, 3, -1)
    counts = zonal.zone_counts(_dev(cm), edges, edge_zone, Z, 3, -1)
    got = zonal.zone_values(_dev(cm.astype(np.float32)), edges, edge_zone, Z, nodata=-1)
    assert np.array_equal(got.valid[:, 0], counts[:, :3].sum(axis=1)) and np.array_equal(got.pixels, counts.sum(axis=1))
    has = got.valid[:, 0] > 0
    assert np.array_equal(np.rint(got.sum[has, 0]), (counts[has, :3] * np.arange(3)).sum(axis=1))
    # with values that are no class (3 = ncls, 100, -7): the counting path files them with the fill, here they are values like any other
    cm = ZR.class_map(len(name), H, W, 3, -1, extra=(3, 100, -7))
    counts = zonal.zone_counts(_dev(cm), edges, edge_zone, Z, 3, -1)
    got = zonal.zone_values(_dev(cm.astype(np.float32)), edges, edge_zone, Z, nodata=-1)
    extra = np.array([(m & (cm != -1) & ((cm < 0) | (cm >= 3))).sum() for m in masks])
    assert extra.sum() > 0 and np.array_equal(got.valid[:, 0], counts[:, :3].sum(axis=1) + extra)
    assert np.array_equal(got.pixels, counts.sum(axis=1)) and np.array_equal(counts[:, 3] - extra, got.pixels - got.valid[:, 0])


TAGS = {33550: (12, (30.0, 30.0, 0.0)), 33922: (12, (0.0, 0.0, 0.0, 399960.0, 4500000.0, 0.0)),
        34735: (3, (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 32613))}


def test_mode_zonal_stats_end_to_end(tmp_path, capsys):
    H, W = 40, 56
    raster = VR.integer_raster(4056, 2, H, W)  # NaN, +Inf and -9999 among integer values
    path = str(tmp_path / "prediction_tile.tif")
    tiff.write(path, raster, {"tags": TAGS, "nodata": VR.NODATA})

    def ring(c0, r0, c1, r1):  # pixel corners -> map coordinates of the 30 m grid
        pts = [(c0, r0), (c1, r0), (c1, r1), (c0, r1), (c0, r0)]
        return [[399960.0 + 30.0 * c, 4500000.0 - 30.0 * r] for c, r in pts]

    feats = [("north", {"type": "Polygon", "coordinates": [ring(2.25, 1.5, 50.75, 17.5), ring(10, 5, 20, 11)]}),
             ("far", {"type": "Polygon", "coordinates": [ring(80, 5, 95, 30)]}),  # east of the raster
             ("south", {"type": "MultiPolygon", "coordinates": [[ring(-4, 20, 30.5, 45)], [ring(40, 25, 56, 40)]]})]
    zpath = str(tmp_path / "districts.geojson")
    with open(zpath, "w") as f:
        json.dump({"type": "FeatureCollection",
                   "features": [{"type": "Feature", "properties": {"name": n}, "geometry": g} for n, g in feats]}, f)
    profile = tiff.read_profile(path)
    zones = zonal.read_zones(zpath, "name")
    edges, edge_zone = zonal.zones_to_pixels(zones, profile)
    ref = VR.ref_values(raster, ZR.ref_masks(edges, edge_zone, 3, H, W), VR.NODATA)
    assert ref.pixels[0] > 0 and ref.pixels[1] == 0 and ref.pixels[2] > 0

    assert zonal.main([f"zonal_stats.raster={path}", f"zonal_stats.zones={zpath}", "zonal_stats.zone_id_property=name"]) == 0
    said = json.loads(capsys.readouterr().out.strip().splitlines()[-1])["zonal_stats"]
    out = str(tmp_path / "zonevalues_prediction_tile.csv")
    assert said == {"zones": 3, "bands": 2, "empty_zones": 1, "output": out}
    rows = list(csv.DictReader(open(out)))
    assert [r["id"] for r in rows] == ["north", "far", "south"] and [r["zone"] for r in rows] == ["0", "1", "2"]
    for z, r in enumerate(rows):
        assert int(r["pixels"]) == ref.pixels[z] and float(r["area_map"]) == ref.pixels[z] * 900.0
        for b in (0, 1):
            assert int(r[f"valid_{b}"]) == ref.valid[z, b]
            if ref.valid[z, b] == 0:
                assert all(r[f"{k}_{b}"] == "" for k in ("mean", "std", "min", "max", "sum"))
                continue
            assert float(r[f"min_{b}"]) == ref.min[z, b] and float(r[f"max_{b}"]) == ref.max[z, b]
            assert np.rint(float(r[f"sum_{b}"])) == ref.sum[z, b] and _ulps(float(r[f"mean_{b}"]), ref.mean[z, b]) <= 2
            assert abs(float(r[f"std_{b}"]) - ref.std[z, b]) <= 1e-9 * ref.std[z, b]
    assert int(rows[1]["valid_0"]) == 0 and int(rows[0]["valid_0"]) > 0

    # one band by its index, another output, the zones by their position: the cells of band 1 above, byte for byte
    sel = str(tmp_path / "band1.csv")
    assert zonal.main([f"zonal_stats.raster={path}", f"zonal_stats.zones={zpath}", "zonal_stats.bands=[1]", f"zonal_stats.output={sel}"]) == 0
    said = json.loads(capsys.readouterr().out.strip().splitlines()[-1])["zonal_stats"]
    assert said == {"zones": 3, "bands": 1, "empty_zones": 1, "output": sel}
    one = list(csv.DictReader(open(sel)))
    assert list(one[0]) == ["zone", "id", "pixels"] + [f"{k}_1" for k in ("valid", "mean", "std", "min", "max", "sum")] + ["area_map"]
    assert [r["id"] for r in one] == ["0", "1", "2"]
    for a, b in zip(one, rows):
        assert all(a[k] == b[k] for k in a if k != "id")
