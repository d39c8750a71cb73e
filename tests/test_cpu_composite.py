"""Temporal composites, host side (no GPU): the numpy host path of instageo_amd/composite.py against the sequential twin of the rule
(tests/composite_reference.py) bit for bit, the median against np.median, a hand-worked medoid, the ordering of the candidates,
create_composite file to file through the mode and into chips.create_chips, the config keys of mode=create_composite, the argument checks
of ``ig_composite`` through the library, and the custom op.  The rule is integer: every comparison is exact equality over every pixel."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import composite_reference as R
from instageo_amd import chips, crs, tiff
from instageo_amd import composite as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "instageo-e2e-geospatial-ml_amd")


@pytest.fixture(scope="module")
def built_lib():
    from instageo_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j4"], check=True)
    return _lib


def run_host(k, method, min_clear=1, with_fmask=True, mask=R.BITS):
    return K.composite(k["bands"][1:], k["starts"], k["fmasks"][1:] if with_fmask else None, k["fmask_starts"] if with_fmask else None,
                       k["step_ptr"], k["C"], (k["H"], k["W"]), mask, R.ND, min_clear, method)


# ---- host path == twin -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", R.METHODS)
@pytest.mark.parametrize("name", ["p36_c6", "p36_c1", "narrow_c6", "narrow_c1", "blocks_c1"])
def test_host_path_equals_the_twin(name, method):
    got, want = run_host(R.case(name), method), R.expected(name, method)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    assert [g.dtype for g in got] == [np.int16, np.uint8, np.uint8, np.int32]
    assert (got[3].sum(axis=1) == R.case(name)["H"] * R.case(name)["W"]).all()


def test_the_cases_cover_what_they_claim():
    k = R.case("p36_c6")
    comp, count, source, hist = R.expected("p36_c6", "medoid")
    assert (count == 0).any() and (comp[:, :, count[0] == 0][0] == R.ND).all() and (source[count == 0] == 255).all()
    assert (k["fmasks"] == 255).any() and set(np.diff(k["step_ptr"]).tolist()) == {0, 1, 2, 3, 4, 5, 8, 15, 16}
    assert (comp[-1] == R.ND).all() and not count[-1].any() and (source[-1] == 255).all() and hist[-1, 0] == 180  # the step with m = 0
    # the identical candidates 0 and 2 tie in the medoid: the earlier wins, never the later
    assert (source[3, 0, :12] != 2).all() and (source[3, 0, :12] == 0).any()
    near = R.expected("p36_c6", "nearest")
    assert not np.array_equal(near[0], comp) and np.array_equal(near[1], count)
    assert {-32768, 32767} <= set(np.unique(k["bands"]).tolist())


@pytest.mark.parametrize("name", ["p36_c6", "blocks_c1"])
def test_median_equals_numpy_where_the_count_is_odd(name):
    k = R.case(name)
    comp, count, _, _ = run_host(k, "median")
    C, HW = k["C"], k["H"] * k["W"]
    checked = 0
    for t in range(len(k["step_ptr"]) - 1):
        cand = range(k["step_ptr"][t], k["step_ptr"][t + 1])
        if not len(cand):
            continue
        v = np.stack([np.stack([k["bands"][1 + k["starts"][n * C + c] :][:HW] for c in range(C)]) for n in cand]).astype(np.float64)
        f = np.stack([k["fmasks"][1 + k["fmask_starts"][n] :][:HW] for n in cand])
        clear = ((f & R.BITS) == 0) & (v != R.ND).all(axis=1)
        v[~np.broadcast_to(clear[:, None, :], v.shape)] = np.nan
        odd = (count[t].reshape(-1) % 2) == 1
        med = np.nanmedian(v[:, :, odd], axis=0)
        assert np.array_equal(comp[t].reshape(C, HW)[:, odd], med.astype(np.int16))
        checked += int(odd.sum())
    assert checked > 50


def test_hand_worked_medoid_and_its_tie():
    # one pixel, C = 2, four candidates; candidate 1 is cloudy.  Clear values: (10, 100), (14, 90), (10, 100) -> lower medians (10, 100);
    # distances 0, 14, 0: candidates 0 and 3 tie, the earlier wins
    bands = np.array([10, 100, 0, 0, 14, 90, 10, 100], dtype=np.int16)
    fm = np.array([0, 2, 0, 0], dtype=np.uint8)
    args = (np.arange(8), fm, np.arange(4), [0, 4], 2, (1, 1))
    comp, count, source, hist = K.composite(bands, *args, ["cloud"], R.ND, 1, "medoid")
    assert comp.reshape(-1).tolist() == [10, 100] and count.item() == 3 and source.item() == 0 and hist[0, 3] == 1
    # moving the first candidate moves the median with it while it stays the middle value; once it is the largest the median is 14
    bands2 = np.array([12, 100, 0, 0, 14, 90, 10, 100], dtype=np.int16)  # medians (12, 100): distances 0, 12, 2
    assert K.composite(bands2, *args, ["cloud"], R.ND, 1, "medoid")[2].item() == 0
    bands3 = np.array([30, 100, 0, 0, 14, 90, 10, 100], dtype=np.int16)  # medians (14, 100): distances 16, 10, 4 -> candidate 3
    comp3, _, source3, _ = K.composite(bands3, *args, ["cloud"], R.ND, 1, "medoid")
    assert source3.item() == 3 and comp3.reshape(-1).tolist() == [10, 100]
    assert K.composite(bands3, *args, ["cloud"], R.ND, 1, "median")[0].reshape(-1).tolist() == [14, 100]  # not a spectrum that was observed
    assert K.composite(bands3, *args, ["cloud"], R.ND, 1, "nearest")[0].reshape(-1).tolist() == [30, 100]
    # the differences need more than 16 bits
    wide = np.array([-32768, 32767, 32767], dtype=np.int16)
    out = K.composite(wide, np.arange(3), None, None, [0, 3], 1, (1, 1), 0, R.ND, 1, "medoid")
    assert out[0].item() == 32767 and out[2].item() == 1


def test_candidates_are_ordered_by_distance_from_the_target_the_earlier_date_first_on_a_tie():
    assert K.order_candidates(["20220510", "20220520", "20220514", "20220516"], "2022-05-15") == [2, 3, 0, 1]
    assert K.order_candidates(["20220516", "20220514"], 20220515) == [1, 0]
    assert K.order_candidates(["20220514", "20220514", "20220513"], "20220514") == [0, 1, 2]
    with pytest.raises(ValueError, match="a date is"):
        K.order_candidates(["20220514"], "May")


def test_min_clear_and_steps_without_candidates():
    k = R.case("p36_c6")
    for method in R.METHODS:
        one, three = run_host(k, method), run_host(k, method, min_clear=3)
        assert all(np.array_equal(g, w) for g, w in zip(three, R.expected("p36_c6", method, 3)))
        assert np.array_equal(one[1], three[1]) and np.array_equal(one[3], three[3])  # the counts do not depend on min_clear
        few = three[1] < 3
        assert few.any() and (three[0].transpose(0, 2, 3, 1)[few] == R.ND).all() and (three[2][few] == 255).all()
        assert np.array_equal(one[0].transpose(0, 2, 3, 1)[~few], three[0].transpose(0, 2, 3, 1)[~few])
    nof = run_host(k, "medoid", with_fmask=False)
    assert all(np.array_equal(g, w) for g, w in zip(nof, R.expected("p36_c6", "medoid", 1, False))) and (nof[1] >= one[1]).all()
    empty = K.composite(np.zeros(0, dtype=np.int16), [], None, None, [0, 0, 0], 3, (2, 5), 0, -1, 1, "median")
    assert (empty[0] == -1).all() and empty[0].shape == (2, 3, 2, 5) and not empty[1].any() and (empty[2] == 255).all() and empty[3][:, 0].tolist() == [10, 10]


def test_host_checks():
    k = R.case("narrow_c1")
    ok = dict(bands=k["bands"][1:], starts=k["starts"], fmasks=k["fmasks"][1:], fmask_starts=k["fmask_starts"], step_ptr=k["step_ptr"],
              bands_per_scene=1, shape=(3, 7), mask=R.BITS, no_data_value=R.ND, min_clear=1, method="medoid")
    for change, what in ((dict(bands_per_scene=0), "bands"), (dict(bands_per_scene=2), "do not go with"), (dict(shape=(3, 7, 1)), "grid"),
                         (dict(shape=(2**16, 2**15)), "grid"), (dict(step_ptr=[0, 17]), "at most 16"), (dict(step_ptr=[1, 2]), "ascending"),
                         (dict(step_ptr=[0, 3, 2]), "ascending"), (dict(step_ptr=[0] * 34), "at most 32"), (dict(starts=k["starts"] + 10**6), "inside the packed"),
                         (dict(starts=-k["starts"] - 1), "inside the packed"), (dict(fmask_starts=k["fmask_starts"][:-1]), "Fmask planes"),
                         (dict(fmask_starts=k["fmask_starts"] + 10**6), "Fmask plane does not lie"), (dict(mask=256), "mask_bits"),
                         (dict(mask=["fog"]), "unknown mask type"), (dict(no_data_value=40000), "no_data"), (dict(min_clear=0), "min_clear"),
                         (dict(min_clear=17), "min_clear"), (dict(method="mean"), "method"), (dict(fmasks=None), "goes with an Fmask buffer"),
                         (dict(bands=k["bands"][1:].astype(np.int32)), "int16"), (dict(fmasks=k["fmasks"][1:].astype(np.int16)), "uint8")):
        with pytest.raises(ValueError, match=what):
            K.composite(**{**ok, **change})


# ---- the header, the entry point, the custom op -------------------------------------------------------------------------------------------------
def test_header_states_the_rule():
    text = open(os.path.join(ROOT, "include", "instageo_hip.h")).read()
    at = text.index("composite.hip")
    rule = " ".join(text[at : text.index("int ig_composite(", at)].replace("*", " ").split()).lower()
    for phrase in ("the rule", "lower median", "earliest in list order", "written exactly once", "fmask_n & mask_bits == 0", "differs from no_data",
                   "count < min_clear", "source = 255", "first clear candidate in list order", "floor((count - 1) / 2)", "255 (fill)",
                   "same bits for any launch geometry", "without touching a pointer"):
        assert phrase in rule, phrase
    assert "composite.hip" in open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert "include/instageo_hip.h" in open(os.path.join(PKG, "csrc", "composite.hip")).read()[:600]


def test_entry_point_exported_and_validated_without_gpu(built_lib):
    """IG_REQUIRE rejects bad arguments before any launch, and an empty problem returns before a pointer is looked at."""
    assert "ig_composite" in built_lib.declared_symbols()
    lib, err = built_lib.load(), built_lib.last_error
    one, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4097)
    ok = dict(bands=one, starts=one, fmasks=one, fmask_starts=one, step_ptr=one, T=3, N=20, max_m=16, C=6, H=3660, W=3660, mask_bits=14, no_data=-9999,
              min_clear=1, method=2, composite=one, count=one, source=one, hist=one, stream=None)

    def comp(**kw):
        return lib.ig_composite(*{**ok, **kw}.values())

    for kw, what in ((dict(max_m=17), "0 <= m <= 16"), (dict(max_m=-1), "0 <= m <= 16"), (dict(T=33), "0 <= T <= 32"), (dict(T=-1), "0 <= T <= 32"),
                     (dict(N=49), "do not go with"), (dict(N=-1), "do not go with"), (dict(C=0), "bands"), (dict(C=32768), "bands"),
                     (dict(no_data=32768), "no_data must fit int16"), (dict(no_data=-32769), "no_data must fit int16"),
                     (dict(min_clear=0), "min_clear"), (dict(min_clear=17), "min_clear"), (dict(method=3), "method"), (dict(method=-1), "method"),
                     (dict(mask_bits=256), "mask_bits"), (dict(H=-1), "H >= 0"), (dict(H=65536, W=32768), "2^31 - 1"),
                     (dict(T=32, N=32, C=32767, H=46340, W=46340), "2^40"),
                     (dict(bands=None), "null pointer"), (dict(starts=None), "null pointer"), (dict(step_ptr=None), "null pointer"),
                     (dict(composite=None), "null pointer"), (dict(count=None), "null pointer"), (dict(source=None), "null pointer"),
                     (dict(hist=None), "null pointer"), (dict(fmask_starts=None), "go together"), (dict(fmasks=None), "go together"),
                     (dict(bands=odd), "aligned"), (dict(composite=odd), "aligned"), (dict(step_ptr=ctypes.c_void_p(4098)), "aligned"),
                     (dict(hist=ctypes.c_void_p(4098)), "aligned"), (dict(starts=ctypes.c_void_p(4100)), "aligned"),
                     (dict(fmask_starts=ctypes.c_void_p(4100)), "aligned")):
        assert comp(**kw) == -1 and what in err(), (kw, err())
    none = dict(bands=None, starts=None, fmasks=None, fmask_starts=None, step_ptr=None, composite=None, count=None, source=None, hist=None)
    assert comp(H=0, **none) == 0 and comp(W=0, **none) == 0 and comp(T=0, N=0, **none) == 0
    with pytest.raises(built_lib.HipLibraryError, match="0 <= m <= 16"):
        built_lib.call("ig_composite", *{**ok, "max_m": 40}.values())


def test_prototype_is_declared_and_the_custom_op_follows_it():
    from instageo_amd import _lib, torch_ops

    s = torch_ops.register()["composite"]
    for piece in ("Tensor? bands", "Tensor? starts", "Tensor? fmasks", "Tensor? fmask_starts", "Tensor? step_ptr", "int T", "int N", "int max_m", "int C",
                  "int H", "int W", "int mask_bits", "int no_data", "int min_clear", "int method", "Tensor(a!)? composite", "Tensor(b!)? count",
                  "Tensor(c!)? source", "Tensor(d!)? hist"):
        assert piece in s, (piece, s)
    assert "stream" not in s
    proto = _lib.parse_header()["ig_composite"][1]
    assert len(proto) == 20 and proto[1] == "const long long*" and proto[15] == "short*"


# ---- the config section ----------------------------------------------------------------------------------------------------------------------
def test_config_carries_the_composite_keys_and_other_sections_are_untouched():
    from instageo_amd import raster_chips, run, s1_chips, s2_chips
    from instageo_amd.config import DEFAULTS, load_config

    assert set(DEFAULTS["composite"]) == set(K.CONFIG_KEYS)
    d = DEFAULTS["composite"]
    assert (d["method"], d["mask_types"], d["min_clear"], d["no_data"]) == ("medoid", ["cloud", "near_cloud_or_shadow", "cloud_shadow"], 1, -9999)
    assert all(d[k] is None for k in ("scenes", "fmasks", "dates", "output_directory", "device"))
    assert set(DEFAULTS["chips"]) == set(chips.CONFIG_KEYS) and set(DEFAULTS["s1_chips"]) == set(s1_chips.CONFIG_KEYS)
    assert set(DEFAULTS["s2_chips"]) == set(s2_chips.CONFIG_KEYS) and set(DEFAULTS["raster_chips"]) == set(raster_chips.CONFIG_KEYS)
    assert run.PREP_MODES["create_composite"] == "composite" and run.PREP_MODES["create_chips"] == "chips"
    cfg = load_config("config", [])
    opts = K.composite_options(cfg)  # nothing required outside the mode
    assert opts["scenes"] is None and opts["method"] == "medoid" and opts["min_clear"] == 1 and opts["no_data"] == -9999 and opts["device"] is None
    with pytest.raises(ValueError, match="needs composite.scenes"):
        K.composite_options(load_config("config", ["mode=create_composite"]))
    base = ["mode=create_composite", "composite.scenes=[[[a_B02.tif,a_B03.tif],[b_B02.tif,b_B03.tif]],[[c_B02.tif,c_B03.tif]]]",
            "composite.output_directory=out"]
    opts = K.composite_options(load_config("config", base + ["composite.fmasks=[[a_F.tif,b_F.tif],[c_F.tif]]", "composite.dates=[2022-05-25,20220610]",
                                                             "composite.method=nearest", "composite.mask_types=[cloud,water]", "composite.min_clear=2",
                                                             "composite.no_data=0", "composite.device=host"]))
    assert opts == dict(scenes=[[["a_B02.tif", "a_B03.tif"], ["b_B02.tif", "b_B03.tif"]], [["c_B02.tif", "c_B03.tif"]]], fmasks=[["a_F.tif", "b_F.tif"], ["c_F.tif"]],
                        output_directory="out", dates=["20220525", "20220610"], method="nearest", mask_types=["cloud", "water"], min_clear=2, no_data=0,
                        device="host")
    for ov, what in (("composite.method=mean", "method"), ("composite.mask_types=[fog]", "mask_types"), ("composite.min_clear=0", "min_clear"),
                     ("composite.min_clear=17", "min_clear"), ("composite.min_clear=1.5", "min_clear"), ("composite.no_data=40000", "no_data"),
                     ("composite.no_data=x", "no_data"), ("composite.device=cpu", "device"), ("composite.scenes=a.tif", "scenes"),
                     ("composite.scenes=[[a.tif]]", "scenes"), ("composite.scenes=[[[a.tif,b.tif],[c.tif]]]", "scenes"),
                     ("composite.fmasks=[[a_F.tif]]", "fmasks"), ("composite.fmasks=x.tif", "fmasks"), ("composite.dates=[2022-05-25]", "dates"),
                     ("composite.dates=[May,June]", "dates"), ("composite.output_directory=None", "needs composite.scenes")):
        with pytest.raises(ValueError, match=what):
            K.composite_options(load_config("config", base + [ov]))
    with pytest.raises(KeyError):
        load_config("config", ["composite.mincount=3"])
    with pytest.raises(ValueError, match="unknown composite keys"):
        K.composite_options({"composite": {"mincount": 3}})


# ---- file to file ------------------------------------------------------------------------------------------------------------------------------
TILE, H, W, X0, Y0 = "T36NXF", 40, 48, 600000.0, 400000.0
STAMPS = ("2022140T075611", "2022145T075621", "2022148T075609")  # May 20, 25, 28
BANDS = ("B02", "B03")


def _profile(x0=X0):
    return {"tags": {33550: (12, (30.0, 30.0, 0.0)), 33922: (12, (0.0, 0.0, 0.0, float(x0), Y0, 0.0)), **crs.geokeys(32636)}, "nodata": None}


def write_scenes(root):
    """Three tiny scenes of one tile: the rows 0..7 are cloudy in every scene (count 0), the rows 8..15 only in the scene nearest the target."""
    os.makedirs(root, exist_ok=True)
    rng = np.random.default_rng(5)
    scenes, fmasks, arrays, masks = [], [], [], []
    for i, stamp in enumerate(STAMPS):
        files, planes = [], []
        for b in BANDS:
            a = rng.integers(1, 3000, size=(H, W)).astype(np.int16)
            a[30:, 40:] = -9999  # the corner is fill in every scene
            files.append(os.path.join(root, f"HLS.{'SL'[i % 2]}30.{TILE}.{stamp}.v2.0.{b}.tif"))
            tiff.write(files[-1], a, _profile())
            planes.append(a)
        f = np.zeros((H, W), dtype=np.uint8)
        f[:8] = 2
        if i == 1:
            f[8:16] = 8
        f[30:, 40:] = 255
        fmasks.append(os.path.join(root, f"HLS.{'SL'[i % 2]}30.{TILE}.{stamp}.v2.0.Fmask.tif"))
        tiff.write(fmasks[-1], f, _profile())
        scenes.append(files), arrays.append(np.stack(planes)), masks.append(f)
    return scenes, fmasks, np.stack(arrays), np.stack(masks)


def test_create_composite_through_the_mode_and_into_create_chips(tmp_path):
    scenes, fmasks, arrays, masks = write_scenes(str(tmp_path / "in"))
    out = str(tmp_path / "out")
    text = "[[" + ",".join("[" + ",".join(s) + "]" for s in scenes) + "]]"
    argv = [sys.executable, "-m", "instageo_amd.run", "mode=create_composite", f"composite.scenes={text}", f"composite.fmasks=[[{','.join(fmasks)}]]",
            "composite.dates=[2022-05-26]", f"composite.output_directory={out}", "composite.device=host"]
    env = {**os.environ, "PYTHONPATH": PKG + os.pathsep + os.environ.get("PYTHONPATH", "")}
    res = subprocess.run(argv, capture_output=True, text=True, env=env, cwd=str(tmp_path))
    assert res.returncode == 0, res.stderr
    line = json.loads(res.stdout.strip().splitlines()[-1])
    tiles = [f"HLS.M30.{TILE}.2022146T000000.v2.0.{b}.tif" for b in BANDS]
    aux = [f"composite_{TILE}_2022146_count.tif", f"composite_{TILE}_2022146_source.tif"]
    assert sorted(os.listdir(out)) == sorted(tiles + aux + ["composite_stats.json"])
    # the order used: May 25 (1 day), May 28 (2 days), May 20 (6 days)
    order = [1, 2, 0]
    flat = np.ascontiguousarray(arrays[order]).reshape(-1)
    want = K.composite(flat, np.arange(6) * H * W, np.ascontiguousarray(masks[order]).reshape(-1), np.arange(3) * H * W, [0, 3], 2, (H, W),
                       K.MASK_TYPES, -9999, 1, "medoid")
    stats = json.load(open(os.path.join(out, "composite_stats.json")))
    step = stats["steps"][0]
    assert step["candidates"] == [[os.path.basename(f) for f in scenes[i]] for i in order] and step["date"] == "20220526"
    assert step["histogram"] == want[3][0].tolist() and step["tiles"] == tiles == stats["tiles"] and (step["count"], step["source"]) == tuple(aux)
    covered = float((want[1] >= 1).sum()) / (H * W)
    assert step["covered"] == covered and 0 < covered < 1
    assert (stats["method"], stats["min_clear"], stats["no_data"], stats["tile"]) == ("medoid", 1, -9999, TILE)
    assert line == {"create_composite": {"steps": 1, "files": 2, "covered": [covered], "output_directory": out}}
    from instageo_amd import prep

    for c, name in enumerate(tiles):
        a, prof = tiff.read(os.path.join(out, name))
        assert a.dtype == np.int16 and np.array_equal(a[0], want[0][0, c])
        assert prof["tags"][33922] == _profile()["tags"][33922] and prof["tags"][33550] == _profile()["tags"][33550]
        assert prof["tags"][34735] == crs.geokeys(32636)[34735]
        assert prep.hls_name(name) == ("M30", TILE, "2022146T000000") and prep.hls_date(name) == "20220526"
    count = tiff.read(os.path.join(out, aux[0]))[0][0]
    source = tiff.read(os.path.join(out, aux[1]))[0][0]
    assert count.dtype == np.uint8 and np.array_equal(count, want[1][0]) and np.array_equal(source, want[2][0])
    assert (count[:8] == 0).all() and (count[8:16, :40] == 2).all() and (count[16:30] == 3).all() and (count[30:, 40:] == 0).all()
    assert set(np.unique(source[8:16]).tolist()) <= {1, 2} and (source[count == 0] == 255).all()
    # the band files go into the chip creator as a tile without an Fmask: what is no-data in the chips is what no scene saw clear
    S = 8
    cells = [(x, y) for x in range(W // S) for y in range(H // S)]
    table = {"x": [X0 + (S * x + 3.5) * 30.0 for x, _ in cells], "y": [Y0 - (S * y + 3.5) * 30.0 for _, y in cells], "label": [1] * len(cells),
             "date": ["2022-05-26"] * len(cells)}
    names, segs = chips.create_chips([os.path.join(out, n) for n in tiles], None, table, str(tmp_path / "chips"), chip_size=S, src_crs=32636,
                                     no_data_value=-9999)
    alive = [(x, y) for x, y in cells if (count[S * y : S * y + S, S * x : S * x + S] > 0).any()]
    assert 0 < len(alive) < len(cells) and names == [f"chip_20220526_M30_{TILE}_2022146T000000_{x}_{y}.tif" for x, y in alive]
    for (x, y), n in zip(alive, names):
        a, _ = tiff.read(str(tmp_path / "chips" / "chips" / n))
        assert a.dtype == np.int16 and a.shape == (2, S, S)
        assert np.array_equal((a == -9999).any(axis=0), count[S * y : S * y + S, S * x : S * x + S] == 0)
        assert np.array_equal((a == -9999).all(axis=0), count[S * y : S * y + S, S * x : S * x + S] == 0)


def test_create_composite_checks_the_grid_and_its_arguments(tmp_path):
    scenes, fmasks, arrays, masks = write_scenes(str(tmp_path / "in"))
    out = str(tmp_path / "out")
    # dates=None: the date of the first scene, list order kept; no Fmask: only no_data decides
    written, stats = K.create_composite([scenes], None, out, method="nearest")
    assert written == [f"HLS.M30.{TILE}.2022140T000000.v2.0.{b}.tif" for b in BANDS]
    assert stats["steps"][0]["candidates"][0] == [os.path.basename(f) for f in scenes[0]]
    a = tiff.read(os.path.join(out, written[0]))[0][0]
    assert np.array_equal(a, arrays[0, 0]) and stats["steps"][0]["histogram"][3] == H * W - 80
    # two steps, the second without candidates
    written, stats = K.create_composite([scenes, []], [fmasks, []], str(tmp_path / "two"), dates=["20220526", "20220615"], method="median")
    assert len(written) == 4 and stats["steps"][1]["covered"] == 0.0 and stats["steps"][1]["histogram"][0] == H * W
    assert (tiff.read(os.path.join(str(tmp_path / "two"), written[2]))[0] == -9999).all()
    shifted = os.path.join(str(tmp_path / "in"), f"HLS.S30.{TILE}.2022150T075611.v2.0.B02.tif")
    tiff.write(shifted, arrays[0, 0], _profile(X0 + 30.0))
    small = os.path.join(str(tmp_path / "in"), f"HLS.S30.{TILE}.2022151T075611.v2.0.B02.tif")
    tiff.write(small, arrays[0, 0][:-1], _profile())
    other = os.path.join(str(tmp_path / "in"), f"HLS.S30.T36NYF.2022150T075611.v2.0.B03.tif")
    tiff.write(other, arrays[0, 1], _profile())
    for bad, what in ((dict(scenes=[[scenes[0], [shifted, scenes[1][1]]]]), "share one grid"), (dict(scenes=[[scenes[0], [small, scenes[1][1]]]]), "share one grid"),
                      (dict(scenes=[[scenes[0], [scenes[1][0], other]]]), "one MGRS tile"), (dict(method="mean"), "method"), (dict(mask_types=["fog"]), "mask type"),
                      (dict(device="cpu"), "device"), (dict(scenes=[]), "list of steps"), (dict(scenes=[[]]), "at least one scene"),
                      (dict(scenes=[scenes] * 33), "at most 32 steps"), (dict(scenes=[scenes * 6]), "at most 32 steps"), (dict(fmasks=[fmasks[:2]]), "nesting of scenes"),
                      (dict(dates=["20220526", "20220527"]), "one target date per step"), (dict(scenes=[scenes, []]), "give dates"),
                      (dict(min_clear=0), "min_clear"), (dict(no_data=10**6), "no_data")):
        with pytest.raises(ValueError, match=what):
            K.create_composite(**{**dict(scenes=[scenes], fmasks=None, output_directory=str(tmp_path / "bad")), **bad})
