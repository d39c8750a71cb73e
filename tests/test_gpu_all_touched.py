"""all_touched rasterisation on the device (-m gpu): ig_zone_touch_rows, ig_zone_touch and ig_zone_touch_merge through instageo_amd.zonal
and instageo_amd.polygon_labels against the numpy twin (which tests/test_cpu_all_touched.py holds against the Fraction reference), bit
for bit.

The canvases (all_touched_reference.cases) are the smallest that can break each stage: 5 x 7; 8 x 9 hand-built ties; 37 x 130 (W crosses
waves and the runs of 4 pixels, two near-horizontal edges longer than a wave); 3 x 1500 (the merge's carry across its chunk of 1024
columns; edges that span 1500 and 65 columns inside one row: the wave-wide path in 24 steps and in two); 65 zones on 9 x 70 (two passes,
bit 63, and a second pass that touches a pixel without crossing a centre line)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import all_touched_reference as AR  # noqa: E402
import polygon_labels_reference as PR  # noqa: E402
import zonal_reference as ZR  # noqa: E402
import zonal_values_reference as VR  # noqa: E402
from instageo_amd import ops, zonal  # noqa: E402
from instageo_amd import polygon_labels as P  # noqa: E402

DEV = "cuda"
CASES = sorted(AR.cases())


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the shared arrays are read-only


@pytest.mark.parametrize("name", CASES)
def test_touch_rows_equal_the_twin(name):
    H, W, _ = AR.cases()[name]
    edges = AR.reference(name)[0]
    far = np.array([[-900, -900, -10, -5], [10, 256 * H + 1, 900, 256 * H + 700], [5, 256, 700, 256]], dtype=np.int32)  # above, below, on a border
    e = np.concatenate([edges, far])
    for h in (H, 1):
        rows = ops.zone_touch_rows(_dev(e), h)
        assert rows.dtype == torch.int32 and np.array_equal(rows.cpu().numpy(), zonal.touch_rows(e, h)), h
    assert not ops.zone_touch_rows(_dev(far), H).any()


@pytest.mark.parametrize("name", CASES)
def test_masks_equal_the_twin_and_two_runs_agree(name):
    H, W, _ = AR.cases()[name]
    edges, edge_zone, Z, touched = AR.reference(name)
    want = AR.twin_masks(name)
    planes = zonal.zone_masks(edges, edge_zone, Z, H, W, DEV, all_touched=True)
    assert planes.dtype == torch.int64 and tuple(planes.shape) == ((Z + 63) // 64, H, W)
    assert torch.equal(planes.cpu(), torch.from_numpy(ZR.to_planes(want)))
    assert torch.equal(planes, zonal.zone_masks(edges, edge_zone, Z, H, W, DEV, all_touched=True))
    centre = zonal.zone_masks(edges, edge_zone, Z, H, W, DEV)
    assert torch.equal(centre, zonal.zone_masks(edges, edge_zone, Z, H, W, DEV, all_touched=False))  # off: the call without the argument
    assert torch.equal(planes & centre, centre) and int(want.sum()) > int(ZR.ref_masks(edges, edge_zone, Z, H, W).sum())
    print(f"{name}: {Z} zones, {len(edges)} edges, {int(want.sum())} pixels, {int(touched.sum())} of them touched")


def test_the_cases_reach_the_paths_they_claim():
    e, r, c0, c1 = zonal.touch_spans(AR.reference("wide_3x1500")[0], 3, 1500)
    n = c1 - c0 + 1
    assert (n == 1500).sum() >= 2 and (n == 65).sum() >= 1 and (n <= 4).sum() > 10 and ((c0 < 1024) & (c1 >= 1024)).any()
    n = np.subtract(*zonal.touch_spans(AR.reference("wave_37x130")[0], 37, 130)[:1:-1]) + 1
    assert (n == 130).any() and ((n > 4) & (n < 64)).any() and (n == 1).any()
    edges, edge_zone, Z, _ = AR.reference("zones65_9x70")
    last = edges[edge_zone == 64]
    yc = 256 * np.arange(9) + 128
    assert Z == 65 and not ((last[:, 1, None] <= yc) != (last[:, 3, None] <= yc)).any() and zonal.touch_rows(last, 9).sum() == 3
    assert AR.twin_masks("zones65_9x70")[64].sum() == 1 and AR.twin_masks("zones65_9x70")[63].any()


def test_the_merged_canvas_is_a_toggle_canvas():
    """Stage by stage on 3 x 1500: touch bits, the merge in place, and the masks ig_zone_tally writes from the merged canvas."""
    H, W, _ = AR.cases()["wide_3x1500"]
    edges, edge_zone, Z, touched = AR.reference("wide_3x1500")
    e, bit = _dev(edges), _dev(edge_zone.astype(np.uint8))
    rows = ops.zone_edge_rows(e, H)
    canvas = torch.zeros((H, W), dtype=torch.int64, device=DEV)
    ops.zone_toggle(e, bit, torch.cumsum(rows, 0, dtype=torch.int64).sub_(rows), canvas, int(rows.sum()))
    toggles = canvas.clone()
    trows = ops.zone_touch_rows(e, H)
    touch = torch.zeros((H, W), dtype=torch.int64, device=DEV)
    ops.zone_touch(e, bit, torch.cumsum(trows, 0, dtype=torch.int64).sub_(trows), touch, int(trows.sum()))
    assert np.array_equal(touch.cpu().numpy(), ZR.to_planes(np.array(touched))[0])
    kept = touch.clone()
    ops.zone_touch_merge(canvas, touch)
    assert torch.equal(touch, kept)  # only read
    inside = toggles.clone()
    ops.zone_tally(inside, None, None, write_mask=True)
    m = inside | touch  # prefix XOR | touch, in torch
    assert torch.equal(canvas[:, 0], m[:, 0]) and torch.equal(canvas[:, 1:], m[:, 1:] ^ m[:, :-1])
    merged = canvas.clone()
    counts = torch.zeros((64, 4), dtype=torch.int64, device=DEV)
    ops.zone_tally(canvas, _dev(ZR.class_map(7, H, W, 3)), counts, 3, -1, write_mask=True)
    assert torch.equal(canvas, m) and np.array_equal(counts.cpu().numpy()[:Z].sum(axis=1), AR.twin_masks("wide_3x1500").sum(axis=(1, 2)))
    again = toggles.clone()
    ops.zone_touch_merge(again, touch)
    assert torch.equal(again, merged)


@pytest.mark.parametrize("name", ["wave_37x130", "wide_3x1500", "zones65_9x70"])
def test_counts_values_and_quantiles_equal_the_host_on_the_twins_masks(name):
    H, W, _ = AR.cases()[name]
    edges, edge_zone, Z, _ = AR.reference(name)
    masks = AR.twin_masks(name)
    cm = ZR.class_map(len(name), H, W, 3, -1, extra=(3, 100, -7))
    counts = zonal.zone_counts(_dev(cm), edges, edge_zone, Z, 3, -1, all_touched=True)
    assert counts.dtype == np.int64 and np.array_equal(counts, ZR.ref_counts(cm, masks, 3, -1))
    assert np.array_equal(zonal.zone_counts(_dev(cm), edges, edge_zone, Z, 3, -1), ZR.ref_counts(cm, ZR.ref_masks(edges, edge_zone, Z, H, W), 3, -1))
    raster = VR.integer_raster(len(name), 2, H, W)  # integer-valued: the sums are exact
    got = zonal.zone_values(_dev(raster), edges, edge_zone, Z, VR.NODATA, all_touched=True)
    ref = VR.ref_values(raster, masks, VR.NODATA)
    has = ref.valid > 0
    assert np.array_equal(got.pixels, ref.pixels) and np.array_equal(got.pixels, masks.sum(axis=(1, 2))) and np.array_equal(got.valid, ref.valid)
    assert has.any() and np.isnan(got.mean[~has]).all()
    assert np.array_equal(got.min[has], ref.min[has]) and np.array_equal(got.max[has], ref.max[has])
    assert np.array_equal(np.rint(got.sum[has]), ref.sum[has])
    assert (np.abs(got.mean[has] - ref.mean[has]) <= 2 * np.spacing(np.abs(ref.mean[has]))).all()
    assert (np.abs(got.std[has] - ref.std[has]) <= 1e-9 * ref.std[has]).all()
    qs = [0, 25, 50, 90.5, 100]
    valid, values, pairs = zonal.zone_quantiles(_dev(raster), edges, edge_zone, Z, qs, VR.NODATA, pairs=True, all_touched=True)
    for z in range(Z):
        v, q, p = zonal.zone_quantiles_host(masks[z], raster, qs, VR.NODATA, pairs=True)
        assert np.array_equal(valid[z], v) and np.array_equal(values[z], q, equal_nan=True) and np.array_equal(pairs[z], p, equal_nan=True), z


@pytest.mark.parametrize("dtype", [np.int8, np.float32])
def test_burn_into_a_view_equals_the_host_path(dtype):
    """A 37 x 130 raster that is a view at (2, 3) of a 41 x 137 buffer (odd pitch, odd offset): the bytes of the host path, the buffer
    around it untouched, the same count of written pixels; and the flag off gives the bytes of the call without it."""
    H, W, zones = AR.cases()["wave_37x130"]
    values = PR.seg_values(len(zones), avoid=(77,)) if dtype == np.int8 else PR.reg_values(len(zones))
    items = PR.items_of(list(zip(values, zones)))
    init = 77 if dtype == np.int8 else np.float32(-7.25)
    out = {}
    for flag in (True, False, None):
        kw = {} if flag is None else dict(all_touched=flag)
        hs, ds = {}, {}
        host = P.burn_fixed(np.full((H, W), init, dtype=dtype), items, hs, **kw)
        buf = torch.full((41, 137), float(init), device=DEV).to(torch.int8 if dtype == np.int8 else torch.float32)
        dev = P.burn_fixed(buf[2 : 2 + H, 3 : 3 + W], items, ds, **kw)
        assert np.array_equal(dev.contiguous().cpu().numpy().view(f"u{host.itemsize}"), host.view(f"u{host.itemsize}")) and ds == hs
        frame = buf.clone()
        frame[2 : 2 + H, 3 : 3 + W] = float(init)
        assert bool((frame == float(init)).all())
        out[flag] = (host, hs)
    assert out[False][0].tobytes() == out[None][0].tobytes() and out[False][1] == out[None][1]
    full = AR.twin_masks("wave_37x130")
    want = np.full((H, W), init, dtype=dtype)
    for z, v in enumerate(values):
        want[full[z]] = v
    assert want.tobytes() == out[True][0].tobytes() and out[True][1]["pixels_written"] == int(full.any(axis=0).sum())
    assert out[True][1]["pixels_written"] > out[False][1]["pixels_written"]


def _parcels(tmp_path):
    """Parcels on a 30 m UTM 36N grid of 2 x 2 cells of 16 pixels: cells (0, 0), (0, 1) and (1, 0) hold parcels with pixel centres; cell
    (1, 1) holds one of 9 m x 9 m between the centres, which only all_touched burns."""
    at = lambda c, r: [399960.0 + 30.0 * c, 4500000.0 - 30.0 * r]  # noqa: E731
    quad = lambda c0, r0, c1, r1: [at(c0, r0), at(c1, r0), at(c1, r1), at(c0, r1), at(c0, r0)]  # noqa: E731
    day = "2022-06-01"
    feats = [({"crop": "maize", "day": day}, [[quad(0.0, 0.0, 12.5, 9.5)]]),
             ({"crop": "wheat", "day": day}, [[quad(10.25, 5.0, 27.0, 14.0), quad(20.0, 8.0, 23.0, 11.0)]]),
             ({"crop": "wheat", "day": day}, [[quad(20.6, 20.6, 20.9, 20.9)]]),
             ({"crop": "maize", "day": day}, [[quad(2.0, 18.0, 9.5, 30.25)]])]
    return PR.write_geojson(tmp_path / "parcels.geojson", feats)


def test_create_polygon_labels_on_the_device_writes_the_host_paths_bytes(tmp_path):
    path = _parcels(tmp_path)
    outs = []
    for device in (None, DEV):
        out = str(tmp_path / f"at_{len(outs)}")
        P.create_polygon_labels(path, out, date_property="day", device=device, all_touched=True, **PR.KW)
        outs.append(out)
    files = sorted(os.listdir(os.path.join(outs[0], "labels")))
    assert files == sorted(os.listdir(os.path.join(outs[1], "labels"))) and len(files) == 4 and "label_x1_y1_2022-06-01.tif" in files
    for rel in [os.path.join("labels", f) for f in files] + ["records.csv", "polygon_labels_stats.json"]:
        assert open(os.path.join(outs[0], rel), "rb").read() == open(os.path.join(outs[1], rel), "rb").read(), rel
    base = str(tmp_path / "base")
    P.create_polygon_labels(path, base, date_property="day", device=DEV, **PR.KW)
    off = str(tmp_path / "off")
    P.create_polygon_labels(path, off, date_property="day", device=DEV, all_touched=False, **PR.KW)
    for rel in [os.path.join("labels", f) for f in sorted(os.listdir(os.path.join(base, "labels")))] + ["records.csv", "polygon_labels_stats.json"]:
        assert open(os.path.join(base, rel), "rb").read() == open(os.path.join(off, rel), "rb").read(), rel
    assert len(os.listdir(os.path.join(base, "labels"))) == 3
