"""Polygon labels on the device (-m gpu): ig_burn_resolve and ig_label_cells against the pixel-by-pixel reference of
tests/polygon_labels_reference.py and numpy, every pixel of every buffer (row padding included), exactly; the device path of
instageo_amd/polygon_labels.py against its host path byte for byte; the round trip with the vectoriser.

Shapes are the smallest at which each launch can still go wrong: 5 x 1030 and 3 x 2051 (a workgroup scans 1024 columns in one step,
ZCHUNK of zone_canvas.h: the prefix carry crosses one and two chunk borders, and a wave border every 256 columns inside a chunk), pass rectangles at c0 = 0..3 under row pitches of 1030, 1031, 1033 and 1034
(every residue mod 4 of the row start and of the column offset: the packed 4-byte store of int8 pixels must stay inside words the thread
owns), all 64 bits, bit 63 alone, bit 0 alone, three passes, an empty pass; cells of 16 x 16 on 3 x 5 cells, K = 0, 2, 127, and S = 1."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import all_touched_reference as AR  # noqa: E402
import polygon_labels_reference as PR  # noqa: E402
import zonal_reference as ZR  # noqa: E402
from instageo_amd import ops, vectorize, warp, zonal  # noqa: E402
from instageo_amd import polygon_labels as P  # noqa: E402
from instageo_amd import postprocess as PP  # noqa: E402

DEV = "cuda"
POISON = {np.int8: 77, np.float32: np.float32(-7.25)}


def same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(got.view(f"u{got.itemsize}"), want.view(f"u{want.itemsize}"))


def values_of(n, dtype):
    return PR.seg_values(n, avoid=(77,)) if dtype == np.int8 else PR.reg_values(n)


def wide_zones(Hp, Wp, seed, n=64):
    """n <= 64 features on an Hp x Wp canvas.  Row 0 is dense (long runs across the chunk borders, a hole over them), row 1 sparse (slivers
    on and next to the borders, the first and the last column), row 2 holds a run from column 1024 to the border at 2048, a triangle cuts
    through all rows, and the rest are polygons a few pixels wide at random columns: rows with short runs."""
    zones = [[ZR.rect(5, 0, Wp - 10, 1)], [ZR.rect(-3, 0.25, Wp + 3, 0.75), ZR.rect(700, 0, 1500.5, 1)],
             [ZR.rect(1023, 1, 1025, 2)], [ZR.rect(0, 1, 1, 2)], [ZR.rect(Wp - 1, 1, Wp, 2)], [ZR.rect(1000, 1.25, 1030, 1.75)],
             [ZR.rect(1024, 2, min(Wp, 2048), 3)], [ZR.px((100.5, -1), (Wp - 20.25, Hp + 1), (600, -2))]]
    rng = np.random.default_rng(seed)
    for z in ZR.random_zones(seed, n - len(zones), Hp, Wp, spread=0.02):
        x = int(rng.integers(0, Wp)) * ZR.Q
        zones.append([[(x + (vx % (6 * ZR.Q)), vy) for vx, vy in z[0]]])
    return zones[:n]


def resolve(zones, values, Hp, Wp, H, W, pitch, r0, c0, dtype):
    """One pass through ig_zone_edge_rows / ig_zone_toggle on the pass canvas (zonal.toggle_canvas; where nothing crosses, an empty
    canvas) and ig_burn_resolve into a poisoned (H, pitch) buffer -> (the whole buffer, the counter)."""
    edges, owner = ZR.edges_of(zones)
    canvas = zonal.toggle_canvas(torch.from_numpy(edges).to(DEV), torch.from_numpy(owner.astype(np.uint8)).to(DEV), Hp, Wp)
    if canvas is None:
        canvas = torch.zeros((Hp, Wp), dtype=torch.int64, device=DEV)
    table = np.zeros(64, dtype=dtype)
    table[: len(values)] = values
    buf = torch.full((H, pitch), POISON[dtype], dtype=torch.int8 if dtype == np.int8 else torch.float32, device=DEV)
    written = torch.zeros(1, dtype=torch.int64, device=DEV)
    ops.burn_resolve(canvas, torch.from_numpy(table).to(DEV), buf[:, :W], r0, c0, written)
    return buf.cpu().numpy(), int(written.item())


def expect(zones, values, Hp, Wp, H, pitch, r0, c0, dtype):
    masks = PR.masks_of(list(zip(values, zones)), Hp, Wp)
    want = np.full((H, pitch), POISON[dtype], dtype=dtype)
    want[r0 : r0 + Hp, c0 : c0 + Wp] = PR.burn(want[r0 : r0 + Hp, c0 : c0 + Wp], list(zip(values, zones)), masks)
    return want, int(masks.any(axis=0).sum())


@pytest.fixture(scope="module")
def wide():
    """The zones and reference masks of the two wide canvases, computed once."""
    out = {}
    for Hp, Wp in ((5, 1030), (3, 2051)):
        zones = wide_zones(Hp, Wp, Wp)
        out[(Hp, Wp)] = zones, PR.masks_of([(0, z) for z in zones], Hp, Wp)
    return out


@pytest.mark.parametrize("dtype", [np.int8, np.float32])
@pytest.mark.parametrize("shape", [(5, 1030), (3, 2051)])
def test_resolve_across_chunk_borders(wide, shape, dtype):
    Hp, Wp = shape
    zones, masks = wide[shape]
    values = values_of(64, dtype)
    got, n = resolve(zones, values, Hp, Wp, Hp, Wp, Wp, 0, 0, dtype)
    want = PR.burn(np.full((Hp, Wp), POISON[dtype], dtype=dtype), list(zip(values, zones)), masks)
    per_row = masks.any(axis=0).sum(axis=1)
    print(f"{Hp} x {Wp}: {int(masks.any(axis=0).sum())} of {Hp * Wp} pixels written, per row {per_row.tolist()}")
    same(got, want)
    assert n == int(masks.any(axis=0).sum()) and 0 < n < Hp * Wp  # unwritten pixels exist and kept the poison
    assert (masks.sum(axis=0) > 1).any()  # pixels inside several features: the highest bit decides


@pytest.mark.parametrize("dtype", [np.int8, np.float32])
@pytest.mark.parametrize("pitch", [1030, 1031, 1033, 1034])
def test_pass_rectangles_at_every_offset_and_pitch(pitch, dtype):
    """A 3 x (1030 - c0 - 1) rectangle at (1, c0) of a 5 x 1030 raster in a buffer of row pitch `pitch`: sparse and dense rows."""
    H, W = 5, 1030
    for c0 in (0, 1, 2, 3):
        Hp, Wp = 3, W - c0 - 1
        zones = [[ZR.rect(0, 0, Wp, 1)], [ZR.rect(3, 1, 9, 2)], [ZR.rect(5, 1, 6, 3)], [ZR.rect(1019, 1, 1027, 2)], [ZR.rect(100, 2, 1026.5, 3)],
                 [ZR.px((7.25, 0), (400, 3), (90.5, 3))]] + ZR.random_zones(pitch + c0, 20, Hp, Wp, spread=0.02)
        values = values_of(len(zones), dtype)
        got, n = resolve(zones, values, Hp, Wp, H, W, pitch, 1, c0, dtype)
        want, count = expect(zones, values, Hp, Wp, H, pitch, 1, c0, dtype)
        same(got, want)
        assert n == count


@pytest.mark.parametrize("dtype", [np.int8, np.float32])
def test_every_bit_bit_63_alone_bit_0_alone_and_an_empty_canvas(dtype):
    Hp, Wp = 26, 27  # feature k covers a 4 x 4 block at (3 (k // 8), 3 (k % 8)): it overlaps its neighbours and owns pixels of its own
    zones = [[ZR.rect(3 * (k % 8), 3 * (k // 8), 3 * (k % 8) + 4, 3 * (k // 8) + 4)] for k in range(64)]
    values = values_of(64, dtype)
    got, n = resolve(zones, values, Hp, Wp, Hp, Wp, Wp, 0, 0, dtype)
    want, count = expect(zones, values, Hp, Wp, Hp, Wp, 0, 0, dtype)
    same(got, want)
    winners = {int(np.nonzero(m)[0].max()) for m in PR.masks_of(list(zip(values, zones)), Hp, Wp).reshape(64, -1).T if m.any()}
    assert n == count and winners == set(range(64))  # every bit decides somewhere
    outside = [[ZR.rect(-9, 1, -2, 4)]] * 63
    for z, vals in ((outside + [zones[5]], values), ([zones[5]], values[:1])):  # bit 63 alone, bit 0 alone
        got, n = resolve(z, vals, Hp, Wp, Hp, Wp, Wp, 0, 0, dtype)
        want, count = expect(z, vals, Hp, Wp, Hp, Wp, 0, 0, dtype)
        same(got, want)
        assert n == count > 0 and set(np.unique(got).tolist()) == {POISON[dtype].item() if dtype == np.float32 else 77, vals[len(z) - 1]}
    got, n = resolve(outside, values, Hp, Wp, Hp, Wp, Wp, 0, 0, dtype)  # nothing crosses: nothing is written
    assert n == 0 and (got == POISON[dtype]).all()


@pytest.fixture(scope="module")
def scratch_case():
    """The wide zones of a 5 x 2051 and of a 3 x 1030 pass, and the reference masks of the second under both rules (the centre rule of
    polygon_labels_reference; all_touched: OR the pixels all_touched_reference finds touched, feature by feature), computed once."""
    first, second = wide_zones(5, 2051, 2051), wide_zones(3, 1030, 1030)
    centre = PR.masks_of([(0, z) for z in second], 3, 1030)
    touched = np.stack([AR.touched(ZR.edges_of([z])[0], 3, 1030) for z in second])
    return first, second, {False: centre, True: centre | touched}


@pytest.mark.parametrize("all_touched", [False, True])
def test_toggle_canvas_in_reused_scratch_equals_fresh_memory_and_the_reference(scratch_case, all_touched):
    """A 5 x 2051 pass built in poisoned scratch, then a 3 x 1030 pass in the same scratch: what the first left behind (toggles across two
    chunk borders, touch bits) must not reach the second, whose rows start at other offsets of the buffer."""
    first, second, masks = scratch_case
    scratch = torch.full((5 * 2051,), -1, dtype=torch.int64, device=DEV)
    scratch2 = torch.full_like(scratch, -1)

    def build(zones, Hp, Wp, *bufs):
        edges, owner = ZR.edges_of(zones)
        return zonal.toggle_canvas(torch.from_numpy(edges).to(DEV), torch.from_numpy(owner.astype(np.uint8)).to(DEV), Hp, Wp, all_touched, *bufs)

    big = build(first, 5, 2051, scratch, scratch2)
    assert big.data_ptr() == scratch.data_ptr() and tuple(big.shape) == (5, 2051) and bool(big.any())
    got = build(second, 3, 1030, scratch, scratch2)
    fresh = build(second, 3, 1030)
    assert got.data_ptr() == scratch.data_ptr() and fresh.data_ptr() != scratch.data_ptr() and tuple(got.shape) == (3, 1030)
    assert torch.equal(got, fresh)
    assert bool((scratch[3 * 1030 :].view(-1) != 0).any())  # the rest of the first pass is still there: only the view was zeroed
    m = masks[all_touched]
    for dtype in (np.int8, np.float32):
        values = values_of(64, dtype)
        buf = torch.full((3, 1030), POISON[dtype], dtype=torch.int8 if dtype == np.int8 else torch.float32, device=DEV)
        written = torch.zeros(1, dtype=torch.int64, device=DEV)
        ops.burn_resolve(got, torch.from_numpy(np.asarray(values, dtype=dtype)).to(DEV), buf, 0, 0, written)
        same(buf.cpu().numpy(), PR.burn(np.full((3, 1030), POISON[dtype], dtype=dtype), list(zip(values, second)), m))
        assert int(written.item()) == int(m.any(axis=0).sum()) < 3 * 1030
    assert int(masks[True].sum()) > int(masks[False].sum())  # the two rules differ on these zones


# ---- the launches, as a contract ---------------------------------------------------------------------------------------------------------------
def launch_sequences():
    """The entry points launched, in order, by zone_counts, zone_values and burn_fixed with all_touched off and on, for 70 zones on a 5 x
    1030 raster: a first pass of 64 wide zones and a second of five zones above the raster and one smaller than a pixel between four
    centres, which crosses no centre line (off: the pass ends after ig_zone_edge_rows) and touches one pixel (on: it runs without
    ig_zone_toggle) -> {"<function>/<off | on>": [names]}."""
    H, W = 5, 1030
    zones = wide_zones(H, W, W) + [[ZR.rect(3 + k, -9, 8 + k, -2)] for k in range(5)] + [[ZR.rect(10.625, 2.625, 10.875, 2.875)]]
    edges, owner = ZR.edges_of(zones)
    items = PR.items_of([(1 + k % 5, z) for k, z in enumerate(zones)])
    cm = torch.from_numpy(ZR.class_map(7, H, W, 3)).to(DEV)
    raster = torch.from_numpy(np.random.default_rng(7).random((H, W), dtype=np.float32)).to(DEV)
    out, real = {}, ops._call
    for flag in (False, True):
        for name, run in (("zone_counts", lambda: zonal.zone_counts(cm, edges, owner, len(zones), 3, -1, all_touched=flag)),
                          ("zone_values", lambda: zonal.zone_values(raster, edges, owner, len(zones), all_touched=flag)),
                          ("burn_fixed", lambda: P.burn_fixed(torch.zeros((H, W), dtype=torch.int8, device=DEV), items, all_touched=flag))):
            calls = []
            ops._call = lambda entry, *a, **k: (calls.append(entry), real(entry, *a, **k))[1]
            try:
                run()
            finally:
                ops._call = real
            out[f"{name}/{'on' if flag else 'off'}"] = calls
    return out


def test_the_launch_sequences_are_those_recorded_before_the_shared_canvas_builder():
    """tests/golden/zone_launch_sequences.json holds what launch_sequences() returned on the commit before zonal.toggle_canvas existed (the
    same function, run there on the device): the names and the order of the launches are part of the contract."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zone_launch_sequences.json")) as f:
        want = json.load(f)
    got = launch_sequences()
    assert sorted(got) == sorted(want) and len(want) == 6
    for key in sorted(want):
        print(key, got[key])
        assert got[key] == want[key], key
    assert want["zone_counts/off"][-1] == "ig_zone_edge_rows" and "ig_zone_toggle" not in want["zone_counts/on"][-4:]  # the second pass


# ---- ig_label_cells ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [0, 2, 127])
def test_label_cells_equal_numpy(K):
    rng = np.random.default_rng(K)
    a = rng.integers(-3, 128, size=(48, 80)).astype(np.int8)
    a[:16, :16] = 1  # a uniform cell: every lane of a wave holds the same value
    a[16:32, 16:32] = -1  # a cell of ignore alone
    valid, hist = ops.label_cells(torch.from_numpy(a).to(DEV), 16, K, -1)
    want_v, want_h = P.label_cells(a, 16, K)
    assert valid.dtype == torch.int64 and np.array_equal(valid.cpu().numpy(), want_v) and want_v[1, 1] == 0 and want_v[0, 0] == 256
    if K:
        assert np.array_equal(hist.cpu().numpy(), want_h) and want_h.sum() < want_v.sum() and want_h[0, 0, 1] == 256
    else:
        assert hist is None
    again = ops.label_cells(torch.from_numpy(a).to(DEV), 16, K, -1)
    assert torch.equal(again[0], valid) and (K == 0 or torch.equal(again[1], hist))
    other = ops.label_cells(torch.from_numpy(a).to(DEV), 16, 0, 1)[0].cpu().numpy()  # another ignore value
    assert other[0, 0] == 0 and other.sum() == (a != 1).sum()


def test_label_cells_float32_one_pixel_cells_and_a_tall_cell():
    rng = np.random.default_rng(8)
    f = rng.random((48, 80)).astype(np.float32)
    f[rng.random((48, 80)) < 0.3] = np.nan
    valid, hist = ops.label_cells(torch.from_numpy(f).to(DEV), 16, 0)
    assert hist is None and np.array_equal(valid.cpu().numpy(), P.label_cells(f, 16)[0])
    a = rng.integers(-1, 4, size=(7, 9)).astype(np.int8)
    valid, hist = ops.label_cells(torch.from_numpy(a).to(DEV), 1, 3, -1)  # S = 1
    assert np.array_equal(valid.cpu().numpy(), (a != -1).astype(np.int64))
    assert np.array_equal(hist.cpu().numpy(), np.stack([a == k for k in range(3)], axis=2).astype(np.int64))
    tall = rng.integers(-1, 3, size=(130, 260)).astype(np.int8)  # S = 130: three row slabs of 64 per cell, the last one partial
    valid, hist = ops.label_cells(torch.from_numpy(tall).to(DEV), 130, 3, -1)
    want_v, want_h = P.label_cells(tall, 130, 3)
    assert np.array_equal(valid.cpu().numpy(), want_v) and np.array_equal(hist.cpu().numpy(), want_h)


# ---- the device path of the module ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.int8, np.float32])
@pytest.mark.parametrize("name", sorted(PR.cases()))
def test_device_burn_equals_host_burn_and_the_reference(name, dtype):
    H, W, zones, masks = PR.reference(name)
    feats = list(zip(values_of(len(zones), dtype), zones))
    items = PR.items_of(feats)
    init = POISON[dtype] if dtype == np.int8 else np.float32("nan")
    host_stats, dev_stats = {}, {}
    host = P.burn_fixed(np.full((H, W), init, dtype=dtype), items, host_stats)
    dev = P.burn_fixed(torch.from_numpy(np.full((H, W), init, dtype=dtype)).to(DEV), items, dev_stats)
    same(dev.cpu().numpy(), host)
    same(host, PR.burn(np.full((H, W), init, dtype=dtype), feats, masks))
    assert dev_stats == host_stats and dev_stats["pixels_written"] == PR.pixels_written(masks)
    again = P.burn_fixed(torch.from_numpy(np.full((H, W), init, dtype=dtype)).to(DEV), items)
    assert torch.equal(again.view(torch.uint8), dev.view(torch.uint8))  # two device runs: the same bits


def test_an_empty_pass_launches_nothing_and_later_passes_still_win():
    H, W, zones, masks = PR.reference("overlap130_24x40")
    outside = [[ZR.rect(-9, 1, -2, 4)]] * 64
    feats = list(zip(values_of(64 + len(zones), np.int8), outside + zones))
    calls, real = [], ops._call
    ops._call = lambda name, *a, **k: (calls.append(name), real(name, *a, **k))[1]
    try:
        stats = {}
        dev = P.burn_fixed(torch.full((H, W), 77, dtype=torch.int8, device=DEV), PR.items_of(feats), stats)
    finally:
        ops._call = real
    assert stats["passes"] == 3 and calls.count("ig_burn_resolve") == 3  # the first 64 features touch nothing: no launch for them
    same(dev.cpu().numpy(), PR.burn(np.full((H, W), 77, dtype=np.int8), feats[64:], masks))


def test_burn_with_a_labelled_area_on_the_device():
    H, W, zones, masks = PR.reference("seventy_24x40")
    feats = list(zip(values_of(len(zones), np.int8), zones))[9:14]
    area = PR.map_features([(0, [ZR.rect(2, 2, 30, 20)]), (0, [ZR.rect(25, 10, 45, 30), ZR.rect(28, 12, 33, 18)])], H)
    kw = dict(src_crs=3857, dtype="int8", background=5, labelled_area=area)
    host = P.burn(PR.map_features(feats, H), (H, W), (0.0, float(H), 1.0, 1.0), 3857, **kw)
    dev = P.burn(PR.map_features(feats, H), (H, W), (0.0, float(H), 1.0, 1.0), 3857, device=DEV, **kw)
    same(dev.cpu().numpy(), host)
    assert (host == -1).any() and (host == 5).any()


def test_create_polygon_labels_on_the_device_writes_the_host_paths_bytes(tmp_path):
    KW = PR.KW
    path, _ = PR.parcels(tmp_path)
    for task, extra in (("seg", {}), ("reg", dict(value_property=None, class_map=None, burn_value=2.5))):
        outs = []
        for device in (None, DEV, DEV):
            out = str(tmp_path / f"{task}_{len(outs)}")
            P.create_polygon_labels(path, out, date_property="day", task_type=task, device=device, **{**KW, **extra})
            outs.append(out)
        for other in outs[1:]:
            files = sorted(os.listdir(os.path.join(outs[0], "labels")))
            assert files == sorted(os.listdir(os.path.join(other, "labels"))) and len(files) == 3
            for rel in [os.path.join("labels", f) for f in files] + ["records.csv", "polygon_labels_stats.json"]:
                assert open(os.path.join(outs[0], rel), "rb").read() == open(os.path.join(other, rel), "rb").read(), rel


# ---- round trip with the vectoriser --------------------------------------------------------------------------------------------------------
def test_polygons_of_the_vectoriser_burn_back_to_the_class_map(tmp_path):
    from instageo_amd import crs

    cm = np.random.default_rng(96160).integers(0, 4, size=(96, 160)).astype(np.int8)
    cm[20:60, 30:90] = 2  # a large region with islands in it
    cm[30:40, 40:50] = np.random.default_rng(1).integers(0, 4, size=(10, 10))
    d = torch.from_numpy(cm).to(DEV)
    rings, vertices = vectorize.region_rings(d, 4, -1)
    table = PP.region_table(d, 4, -1)
    profile = {"tags": {33550: (12, (30.0, 30.0, 0.0)), 33922: (12, (0.0, 0.0, 0.0, 399960.0, 4500000.0, 0.0)), **crs.geokeys(32613)}}
    path = vectorize.write_geojson(str(tmp_path / "regions.geojson"), rings, vertices, table, profile)
    feats = P.read_features(path, value_property="cls")
    assert len(feats) == len(table["root"]) > 1000
    for device in (None, DEV):
        stats = {}
        got = P.burn(feats, cm.shape, warp.grid_of(profile), 32613, src_crs=32613, dtype="int8", background=-1, device=device, stats=stats)
        got = got if device is None else got.cpu().numpy()
        same(got, cm)
        assert stats["outside"] == 0 and stats["degenerate"] == 0 and stats["passes"] == -(-len(feats) // 64)
