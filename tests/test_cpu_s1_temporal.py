"""Multi-temporal Sentinel-1 speckle filtering without a GPU: the numpy path of instageo_amd/s1_temporal.py against the sequential twin of
the rule (tests/s1_temporal_reference.py) bit for bit, the one-date identity, the looks gain on homogeneous gamma speckle, the argument
checks, the config section, the entry point's refusals, and files -> files runs whose outputs ``s1_chips.scene_files`` takes."""
import ctypes
import json
import os

import numpy as np
import pytest

import s1_temporal_reference as R
from instageo_amd import crs, tiff
from instageo_amd import s1_temporal as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "instageo-e2e-geospatial-ml_amd")


@pytest.fixture(scope="module")
def built_lib():
    import subprocess

    from instageo_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j4"], check=True)
    return _lib


def run(k, h, with_snd, scale):
    return Q.temporal(k["planes"][1:], k["starts"], k["sizes"], k["group"], k["date"], k["offsets"], 2 * h + 1, R.SND if with_snd else None, scale)


# ---- host path == twin -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,with_snd", R.RUNS)
def test_host_path_equals_the_twin(h, with_snd):
    """Linear: byte for byte.  dB: both sides call numpy's log10, and the test allows the 1 float32 ulp two log10 implementations may differ
    by next to a rounding tie; the NaN patterns and the counts are equal."""
    k = R.stack()
    for scale in ("linear", "db"):
        out, counts = run(k, h, with_snd, scale)
        want, wcounts = R.expected(h, with_snd, scale)
        got = R.bits_of(out)
        assert out.dtype == np.float32 and counts.dtype == np.int32 and counts.shape == (len(R.STACK), 4)
        assert np.array_equal(counts, wcounts), (h, scale, counts.tolist(), wcounts.tolist())
        assert np.array_equal(got == R.QNAN, want == R.QNAN)
        if scale == "linear":
            assert np.array_equal(got, want), (h, int((got != want).sum()))
        else:
            assert R.ulps(got, want) <= 1
        pixels = np.array([H * W for H, W in k["sizes"]])
        assert (counts[:, 0] + counts[:, 1] <= pixels).all() and (counts[:, 3] <= counts[:, 0]).all()


def test_the_stack_covers_what_it_claims():
    k = R.stack()
    a = k["planes"][1:]
    assert np.isnan(a).any() and np.isinf(a).sum() >= 2 and (a == R.SND).any() and (a < 0).any() and (a == 0).sum() >= 81
    assert [g for g, *_ in R.STACK] == [0, 0, 0, 0, 1, 1, 1] and [d for _, d, *_ in R.STACK][:4] == [0, 1, 2, 1]
    _, _, _, _, _, T = Q.check_temporal(a.shape[0], k["starts"], k["sizes"], k["group"], k["date"], k["offsets"], 7, None, "linear")
    assert T.lattice.tolist() == [[42, 80], [65, 65]] and T.members.tolist() == [0, 1, 3, 2, 4, 5, 6] and T.member_ptr.tolist() == [0, 4, 7]
    assert T.tile_ptr.tolist() == [0, 4, 10] and T.place[3].tolist() == [10, 50, 1]
    # the zero patch gives m = 0 and a passthrough; the dB step drops pixels; somewhere one date alone contributes, elsewhere all three
    lin, cl = R.expected(1, True, "linear")
    at = int(k["starts"][0]) + 16 * 70 + 24  # the centre of the zero patch of plane 0
    assert lin[at] == 0 and cl[0, 2] >= 49 and R.expected(1, True, "db")[1][:4, 1].min() > 0 and (cl[:4, 3] > 0).all() and (cl[:4, 3] < cl[:4, 0]).all()
    # the second slice of date 1 decides where the first is absent or does not reach: dropping it changes plane 0 only there
    rest = [0, 1, 2, 4, 5, 6]
    pick = lambda v: [v[p] for p in rest]  # noqa: E731
    without = R.bits_of(Q.temporal(a, pick(k["starts"]), pick(k["sizes"]), pick(k["group"]), pick(k["date"]), pick(k["offsets"]), 3, R.SND)[0])
    p0, p1 = a[: 37 * 70].reshape(37, 70), a[int(k["starts"][1]) : int(k["starts"][1]) + 33 * 66].reshape(33, 66)
    changed = (without[: 37 * 70] != lin[: 37 * 70]).reshape(37, 70)
    assert changed.any() and not changed[:10].any() and not changed[:, :50].any()
    first = np.zeros((37, 70), dtype=bool)  # where the first slice of date 1 is present
    first[5:37, 3:69] = (np.isfinite(p1) & (p1 != R.SND))[:32]
    assert not (changed & first).any()


def test_small_integers_by_hand():
    """Two dates of 1 x 3, window 3: m of (2, 4, 6) is (3, 4, 5), m of (1, 1, 1) is 1: R = x / m + 1, c = 2."""
    a = np.array([2, 4, 6, 1, 1, 1], dtype=np.float32)
    out, counts = Q.temporal(a, [0, 3], [(1, 3), (1, 3)], [0, 0], [0, 1], [(0, 0), (0, 0)], 3)
    ratio = [(2 / 3 + 1) / 2, (4 / 4 + 1) / 2, (6 / 5 + 1) / 2]
    assert out.tolist() == [np.float32(3 * ratio[0]), np.float32(4 * ratio[1]), np.float32(5 * ratio[2])] + [np.float32(r) for r in ratio]
    assert counts.tolist() == [[3, 0, 0, 0], [3, 0, 0, 0]]
    # the second date absent in the middle: c = 1 there; a zero plane passes through and contributes nothing
    b = np.array([2, 4, 6, 1, np.nan, 1, 0, 0, 0], dtype=np.float32)
    out, counts = Q.temporal(b, [0, 3, 6], [(1, 3)] * 3, [0, 0, 0], [0, 1, 2], [(0, 0)] * 3, 3)
    assert out[1] == 4 and np.isnan(out[4]) and out[6:].tolist() == [0, 0, 0] and counts.tolist() == [[3, 0, 0, 1], [2, 0, 0, 0], [3, 0, 3, 1]]
    db, counts = Q.temporal(b, [0, 3, 6], [(1, 3)] * 3, [0, 0, 0], [0, 1, 2], [(0, 0)] * 3, 3, scale="db")
    assert db[1] == np.float32(10 * np.log10(4.0)) and np.isnan(db[6:]).all() and counts.tolist() == [[3, 0, 0, 1], [2, 0, 0, 0], [0, 3, 3, 0]]
    # two slices of one date: the first present one is taken, the order given decides; an offset places a plane on the lattice
    # (8, 4) has m = 6, (2, 6) has m = 4, the 1 x 1 plane of date 1 sits on column 1 with m = 4
    s = np.array([8, 4, 2, 6, 4], dtype=np.float32)
    one, _ = Q.temporal(s, [0, 2, 4], [(1, 2), (1, 2), (1, 1)], [0, 0, 0], [0, 0, 1], [(0, 0), (0, 0), (0, 1)], 3)
    two, _ = Q.temporal(s, [2, 0, 4], [(1, 2), (1, 2), (1, 1)], [0, 0, 0], [0, 0, 1], [(0, 0), (0, 0), (0, 1)], 3)
    a, b = (8 / 6) / 1, (4 / 6 + 4 / 4) / 2  # (8, 4) is tried first
    assert one.tolist() == [np.float32(v) for v in (6 * a, 6 * b, 4 * a, 4 * b, 4 * b)]
    a, b = (2 / 4) / 1, (6 / 4 + 4 / 4) / 2  # (2, 6) is tried first
    assert two.tolist() == [np.float32(v) for v in (6 * a, 6 * b, 4 * a, 4 * b, 4 * b)]


def test_one_date_returns_the_input_bits():
    """c = 1: y = m ((x / m) / 1); for gamma values in [1e-4, 10] (x / m) m in float64 rounds back to the float32 x."""
    rng = np.random.default_rng(5)
    a = np.clip(rng.gamma(R.LOOKS, 0.3 / R.LOOKS, size=70 * 131), 1e-4, 10.0).astype(np.float32)
    a[rng.random(a.shape) < 0.03] = np.nan
    for window in (3, 7, 15):
        out, counts = Q.temporal(a, [0, 70 * 66], [(70, 66), (70, 65)], [0, 1], [0, 0], [(0, 0), (3, 2)], window)
        present = ~np.isnan(a)
        assert np.array_equal(R.bits_of(out)[present], R.bits_of(a)[present]) and (R.bits_of(out)[~present] == R.QNAN).all()
        n = [int(present[: 70 * 66].sum()), int(present[70 * 66 :].sum())]
        assert counts.tolist() == [[n[0], 0, 0, n[0]], [n[1], 0, 0, n[1]]]


def test_looks_gain_on_homogeneous_gamma_speckle():
    """D = 4 dates of 96 x 96, L = 4.4, w = 7 (N = 49): the equivalent number of looks mean^2 / var of every date rises by at least
    0.8 D N / (D + N - 1) = 3.0 on the interior (16 pixels trimmed) and every date's mean is kept within 0.5 %."""
    planes, starts, sizes, group, date, offsets = R.gamma_stack(7)
    out, counts = Q.temporal(planes, starts, sizes, group, date, offsets, 7)
    assert counts.tolist() == [[96 * 96, 0, 0, 0]] * 4
    bound = 0.8 * 4 * 49 / (4 + 49 - 1)
    for d in range(4):
        x = planes[d * 9216 : (d + 1) * 9216].reshape(96, 96)[16:-16, 16:-16].astype(np.float64)
        y = out[d * 9216 : (d + 1) * 9216].reshape(96, 96)[16:-16, 16:-16].astype(np.float64)
        gain = (y.mean() ** 2 / y.var()) / (x.mean() ** 2 / x.var())
        print(f"date {d}: looks gain {gain:.2f} (bound {bound:.2f}), mean kept within {abs(y.mean() / x.mean() - 1):.4%}")
        assert gain >= bound and abs(y.mean() / x.mean() - 1) <= 0.005


def test_rows_at_a_time_changes_nothing(monkeypatch):
    k = R.stack()
    whole = run(k, 7, True, "db")
    monkeypatch.setattr(Q, "_ROWS", 5)
    parts = run(k, 7, True, "db")
    assert np.array_equal(R.bits_of(whole[0]), R.bits_of(parts[0])) and np.array_equal(whole[1], parts[1])


def test_host_checks():
    a = np.ones(24, dtype=np.float32)
    ok = dict(planes=a, starts=[0, 12], sizes=[(3, 4), (3, 4)], group=[0, 0], date=[0, 1], offsets=[(0, 0), (1, 2)])
    for kw, what in ((dict(window=2), "window"), (dict(window=17), "window"), (dict(window=True), "window"), (dict(scale="log"), "scale"),
                     (dict(src_nodata=float("nan")), "src_nodata"), (dict(sizes=[(3, 4), (3, 5)]), "inside the packed buffer"),
                     (dict(starts=[0, 6]), "overlap"), (dict(group=[0]), "group"), (dict(group=[0, -1]), "group"), (dict(group=[0, 0.5]), "group"),
                     (dict(date=[0, 1, 2]), "date"), (dict(date=[0, -1]), "date"), (dict(offsets=[(0, 0)]), "offsets"),
                     (dict(offsets=[(0, 0), (-1, 0)]), "offsets"), (dict(offsets=[(0, 0), (2**31 - 2, 0)]), "lattice"),
                     (dict(offsets=[(0, 0), (2**16, 2**16)]), "lattice"), (dict(planes=a.astype(np.float64)), "float32"), (dict(planes=a.reshape(2, 12)), "1-D")):
        with pytest.raises(ValueError, match=what):
            Q.temporal(**{**ok, **kw})
    out, counts = Q.temporal(a, [], [], [], [], [])
    assert out.shape == (24,) and counts.shape == (0, 4)
    out, counts = Q.temporal(**ok)
    assert (out == 1).all() and counts.tolist() == [[12, 0, 0, 8], [12, 0, 0, 8]]  # the lattice is 4 x 6; four pixels of each plane see both dates
    n = Q.MAX_MEMBERS + 1
    with pytest.raises(ValueError, match="at most 64 planes"):
        Q.temporal(np.ones(n, dtype=np.float32), np.arange(n), [(1, 1)] * n, [0] * n, [0] * n, [(0, 0)] * n)
    n = Q.MAX_DATES + 1
    with pytest.raises(ValueError, match="at most 32 dates"):
        Q.temporal(np.ones(n, dtype=np.float32), np.arange(n), [(1, 1)] * n, [7] * n, np.arange(n), [(0, 0)] * n)
    # group ids are names: any ints, any order; the tables put the groups in ascending order of their ids
    T = Q.check_temporal(24, [0, 12], [(3, 4), (3, 4)], [9, 2], [5, 5], [(0, 0), (0, 0)], 3, None, "db")[5]
    assert T.ids.tolist() == [2, 9] and T.members.tolist() == [1, 0] and T.lattice.tolist() == [[3, 4], [3, 4]] and T.tile_ptr.tolist() == [0, 1, 2]


# ---- the config section and the mode -----------------------------------------------------------------------------------------------------------
def test_config_carries_the_s1_temporal_keys():
    from instageo_amd import run as runner
    from instageo_amd.config import DEFAULTS, load_config

    assert runner.PREP_MODES["filter_s1_temporal"] == "s1_temporal" and runner.PREP_MODES["filter_s1"] == "s1_filter"
    assert set(DEFAULTS["s1_temporal"]) == set(Q.CONFIG_KEYS) == {"scenes", "output_directory", "bands", "window", "scale", "src_nodata"}
    opts = Q.s1_temporal_options(load_config("config", []))  # nothing required outside the mode
    assert opts == dict(scenes=None, output_directory=None, bands=["vv", "vh"], window=7, scale="linear", src_nodata=None)
    with pytest.raises(ValueError, match="needs s1_temporal.scenes"):
        Q.s1_temporal_options(load_config("config", ["mode=filter_s1_temporal"]))
    base = ["mode=filter_s1_temporal", "s1_temporal.scenes=[[[a_vv.tif,a_vh.tif]],[b_vv.tif,b_vh.tif]]", "s1_temporal.output_directory=out"]
    opts = Q.s1_temporal_options(load_config("config", base + ["s1_temporal.window=15", "s1_temporal.scale=db", "s1_temporal.src_nodata=-32768"]))
    assert opts == dict(scenes=[[["a_vv.tif", "a_vh.tif"]], ["b_vv.tif", "b_vh.tif"]], output_directory="out", bands=["vv", "vh"], window=15, scale="db",
                        src_nodata=-32768.0)
    one = Q.s1_temporal_options(load_config("config", ["mode=filter_s1_temporal", "s1_temporal.scenes=[[a_vv.tif],[b_vv.tif]]", "s1_temporal.bands=[vv]",
                                                       "s1_temporal.output_directory=out"]))
    assert one["bands"] == ["vv"] and one["scenes"] == [["a_vv.tif"], ["b_vv.tif"]]
    for ov, what in (("s1_temporal.window=4", "window"), ("s1_temporal.window=17", "window"), ("s1_temporal.window=big", "window"),
                     ("s1_temporal.scale=log", "scale"), ("s1_temporal.src_nodata=.nan", "src_nodata"), ("s1_temporal.src_nodata=x", "src_nodata"),
                     ("s1_temporal.scenes=[[a_vv.tif,3]]", "scenes"), ("s1_temporal.scenes=[[a_vv.tif]]", "scenes"), ("s1_temporal.scenes=[]", "scenes"),
                     ("s1_temporal.bands=[]", "bands"), ("s1_temporal.output_directory=None", "needs s1_temporal.scenes")):
        with pytest.raises(ValueError, match=what):
            Q.s1_temporal_options(load_config("config", base + [ov]))
    with pytest.raises(KeyError):
        load_config("config", ["s1_temporal.windows=3"])
    with pytest.raises(ValueError, match="unknown s1_temporal keys"):
        Q.s1_temporal_options({"s1_temporal": {"method": "lee"}})


# ---- files -> files --------------------------------------------------------------------------------------------------------------------------
FX, FY = 600000.0, 4400000.0
BANDS = ("vv", "vh")


def _write(root, name, a, x0, y0, res=10.0, tag=None):
    tags = {33550: (12, (res, res, 0.0)), 33922: (12, (0.0, 0.0, 0.0, x0, y0, 0.0)), **crs.geokeys(32636)}
    path = os.path.join(root, name)
    tiff.write(path, a, {"tags": tags, "nodata": tag})
    return path


def write_stack(root):
    """Three dates.  Lattice A (10 m at FX, FY; files tagged -32768): date 0 one scene of 32 x 48, date 1 two orbit slices (20 x 48 at the
    origin, then 24 x 40 at row 12, column 8: they overlap in rows 12..19), date 2 one scene.  Lattice B (20 m, no tag): dates 0 and 1.
    One scene of date 2 sits half a pixel east of lattice A.  -> (scenes [date][scene][band], {name: (array, (row0, col0))})."""
    os.makedirs(root, exist_ok=True)
    rng = np.random.default_rng(11)
    made = {}

    def scene(stamp, shape, x0, y0, res=10.0, tag=None, at=(0, 0)):
        files = []
        for band in BANDS:
            a = rng.gamma(4.4, 0.02, size=shape).astype(np.float32)
            a[rng.random(shape) < 0.06] = np.nan
            if tag is not None:
                a[rng.random(shape) < 0.05] = tag
            name = f"S1A_IW_GRDH_1SDV_{stamp}_{stamp[:9]}033128_043365_052DB0_rtc_{band}.tif"
            files.append(_write(root, name, a, x0, y0, res, tag))
            made[name] = (a, at)
        return files

    a0 = scene("20220501T033103", (32, 48), FX, FY, tag=-32768.0)
    b0 = scene("20220501T033203", (16, 24), FX, FY, res=20.0)
    a1a = scene("20220513T033103", (20, 48), FX, FY, tag=-32768.0)
    a1b = scene("20220513T033128", (24, 40), FX + 80.0, FY - 120.0, tag=-32768.0, at=(12, 8))
    b1 = scene("20220513T033203", (16, 24), FX, FY, res=20.0)
    a2 = scene("20220525T033103", (32, 48), FX, FY, tag=-32768.0)
    half = scene("20220525T033203", (32, 48), FX + 5.0, FY, tag=-32768.0)
    return [[a0, b0], [a1a, a1b, b1], [a2, half]], made


def _expected_files(made, window, scale):
    """What the files must hold: every group filtered on its own through the array interface, with the tagged no-data value absent."""
    names = list(made)
    want = {}
    for b, band in enumerate(BANDS):
        per = [n for n in names if n.endswith(f"_{band}.tif")]  # in the order given: a0, b0, a1a, a1b, b1, a2, half
        for members, dates in (((0, 2, 3, 5), (0, 1, 1, 2)), ((1, 4), (0, 1)), ((6,), (2,))):
            arrays = [np.where(made[per[m]][0] == -32768.0, np.float32(np.nan), made[per[m]][0]) for m in members]
            starts = np.concatenate([[0], np.cumsum([a.size for a in arrays])[:-1]])
            out, counts = Q.temporal(np.concatenate([a.reshape(-1) for a in arrays]), starts, [a.shape for a in arrays], [0] * len(members), list(dates),
                                     [made[per[m]][1] for m in members], window, None, scale)
            for i, m in enumerate(members):
                want[per[m]] = (out[int(starts[i]) : int(starts[i]) + arrays[i].size].reshape(arrays[i].shape), counts[i])
    return want


def test_files_to_files_groups_by_lattice_and_the_chip_creator_takes_them(tmp_path, capsys):
    from instageo_amd import run as runner
    from instageo_amd import s1_chips as V

    scenes, made = write_stack(str(tmp_path / "in"))
    out = str(tmp_path / "filtered")
    text = "[" + ",".join("[" + ",".join("[" + ",".join(s) + "]" for s in d) + "]" for d in scenes) + "]"
    assert runner.main(["mode=filter_s1_temporal", f"s1_temporal.scenes={text}", f"s1_temporal.output_directory={out}", "s1_temporal.window=5"]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])["filter_s1_temporal"]
    stats = json.load(open(os.path.join(out, "temporal_stats.json")))
    names = [os.path.basename(f) for d in scenes for s in d for f in s]
    assert sorted(os.listdir(out)) == sorted(names + ["temporal_stats.json"])
    assert (line["files"], line["groups"], line["alone"], line["output_directory"]) == (14, 6, 2, out)
    assert (stats["window"], stats["scale"], stats["src_nodata"], stats["bands"]) == (5, "linear", None, ["vv", "vh"])
    want = _expected_files(made, 5, "linear")
    for n in names:
        a, prof = tiff.read(os.path.join(out, n))
        src = tiff.read_profile(os.path.join(str(tmp_path / "in"), n))
        assert a.dtype == np.float32 and a.shape == (1,) + made[n][0].shape and np.isnan(prof["nodata"])
        assert np.array_equal(R.bits_of(a[0]), R.bits_of(want[n][0])), n
        assert all(prof["tags"][t] == src["tags"][t] for t in (33550, 33922, 34735))
        f = stats["files"][n]
        assert [f["present"], f["dropped"], f["passed"], f["single"]] == want[n][1].tolist() and f["pixels"] == made[n][0].size
        assert f["src_nodata"] == (None if "033203" in n and "20220525" not in n else -32768.0)
        assert V.tile_id_of(os.path.join(out, n)) == V.tile_id_of(n)
    # two lattices give two groups per band, the half-pixel-shifted scene a group of its own, reported alone and written with its input's bits
    groups = stats["groups"]
    assert [g["band"] for g in groups] == ["vv", "vh"] * 3 and [len(g["files"]) for g in groups] == [4, 4, 2, 2, 1, 1]
    assert [g["alone"] for g in groups] == [False] * 4 + [True] * 2 and groups[0]["dates"] == [0, 1, 1, 2] and groups[2]["dates"] == [0, 1]
    assert groups[0]["offsets"] == [[0, 0], [0, 0], [12, 8], [0, 0]] and groups[0]["files"] == [names[0], names[4], names[6], names[10]]
    assert groups[0]["lattice"] == {"grid": [FX, FY, 10.0, 10.0], "height": 36, "width": 48, "crs": list(tuple(crs.from_epsg(32636))[:5])}
    assert groups[2]["lattice"]["grid"] == [FX, FY, 20.0, 20.0] and groups[4]["lattice"]["grid"] == [FX + 5.0, FY, 10.0, 10.0]
    for n in names[-2:]:
        a, _ = tiff.read(os.path.join(out, n))
        x = made[n][0]
        keep = ~np.isnan(x) & (x != -32768.0)
        assert stats["files"][n]["alone"] and np.array_equal(R.bits_of(a[0])[keep], R.bits_of(x)[keep]) and np.isnan(a[0][~keep]).all()
        assert stats["files"][n]["single"] == stats["files"][n]["present"] == int(keep.sum())
    assert not any(stats["files"][n]["alone"] for n in names[:-2]) and stats["files"][names[4]]["group"] == 0 and stats["files"][names[4]]["date"] == 1
    # the overlapping slices of date 1 follow the first-present rule: the slices in the other order give other values in date 0
    swapped = [scenes[0], [scenes[1][1], scenes[1][0], scenes[1][2]], scenes[2]]
    Q.filter_s1_temporal(swapped, str(tmp_path / "swapped"), window=5)
    a, _ = tiff.read(os.path.join(out, names[0]))
    b, _ = tiff.read(os.path.join(str(tmp_path / "swapped"), names[0]))
    differ = R.bits_of(a[0]) != R.bits_of(b[0])
    assert differ[12:20, 8:].any() and not differ[:12].any() and not differ[20:].any() and not differ[:, :8].any()
    # the written nesting goes to create_s1_chips as it is; a flat date comes back flat; small batches and the dB scale
    written = Q.filter_s1_temporal(scenes, out, window=5)
    assert written == [[[os.path.join(out, os.path.basename(f)) for f in s] for s in d] for d in scenes]
    files, counts = V.scene_files(written, 2)
    assert counts == [2, 3, 2] and [os.path.basename(f) for f in files] == names
    flat = Q.filter_s1_temporal([scenes[0][0], scenes[2][0]], str(tmp_path / "flat"), window=5, scale="db")
    assert flat == [[os.path.join(str(tmp_path / "flat"), os.path.basename(f)) for f in s] for s in (scenes[0][0], scenes[2][0])]
    sd = json.load(open(os.path.join(str(tmp_path / "flat"), "temporal_stats.json")))
    assert sd["scale"] == "db" and [g["dates"] for g in sd["groups"]] == [[0, 1], [0, 1]] and V.scene_files(flat, 2)[1] == [1, 1]
    largest = 4 * (2 * 32 * 48 + 20 * 48 + 24 * 40)  # the bytes of a group on lattice A: one group per batch, each with one no-data value
    Q.filter_s1_temporal(scenes, str(tmp_path / "small"), window=5, max_bytes=largest)
    assert all(open(os.path.join(out, n), "rb").read() == open(os.path.join(str(tmp_path / "small"), n), "rb").read() for n in names)
    with pytest.raises(ValueError, match=rf"group 0 \(band vv, 4 files from .*\) holds {largest} bytes, more than max_bytes = {largest - 1}"):
        Q.filter_s1_temporal(scenes, str(tmp_path / "never"), window=5, max_bytes=largest - 1)
    assert not os.path.exists(str(tmp_path / "never"))


def test_filter_s1_temporal_refuses_to_replace_its_inputs(tmp_path):
    scenes, _ = write_stack(str(tmp_path / "in"))
    before = {f: open(f, "rb").read() for d in scenes for s in d for f in s}
    with pytest.raises(ValueError, match="replace an input"):
        Q.filter_s1_temporal(scenes, str(tmp_path / "in"))
    with pytest.raises(ValueError, match="replace an input"):
        Q.filter_s1_temporal(scenes, os.path.join(str(tmp_path / "in"), "..", "in"))
    with pytest.raises(ValueError, match="share a base name"):
        Q.filter_s1_temporal([scenes[0][0], scenes[0][0]], str(tmp_path / "out"))
    with pytest.raises(ValueError, match="scenes is a list"):
        Q.filter_s1_temporal([], str(tmp_path / "out"))
    with pytest.raises(ValueError, match="a scene is a list of 2 band files"):
        Q.filter_s1_temporal([[scenes[0][0][0]]], str(tmp_path / "out"))
    with pytest.raises(ValueError, match="device"):
        Q.filter_s1_temporal(scenes, str(tmp_path / "out"), device="cpu")
    with pytest.raises(ValueError, match="window"):
        Q.filter_s1_temporal(scenes, str(tmp_path / "out"), window=4)
    with pytest.raises(ValueError, match="max_bytes"):
        Q.filter_s1_temporal(scenes, str(tmp_path / "out"), max_bytes=0)
    assert all(open(f, "rb").read() == b for f, b in before.items()) and not os.path.exists(str(tmp_path / "out"))


# ---- the entry point ---------------------------------------------------------------------------------------------------------------------------
def test_entry_point_exported_and_validated_without_gpu(built_lib):
    """IG_REQUIRE rejects bad arguments before any launch, and N = 0 returns before a pointer is looked at."""
    assert "ig_s1_temporal" in built_lib.declared_symbols()
    lib, err = built_lib.load(), built_lib.last_error
    one, far, odd, off8 = ctypes.c_void_p(4096), ctypes.c_void_p(1 << 30), ctypes.c_void_p(4098), ctypes.c_void_p(4100)
    ok = dict(planes=one, starts=one, sizes=one, place=one, lattice=one, member_ptr=one, members=one, tile_ptr=one, N=3, G=2, M=3, total=1000, tiles=3,
              h=3, has_src_nodata=1, src_nodata=-32768.0, to_db=0, out=far, counts=one, stream=None)

    def call(**kw):
        return lib.ig_s1_temporal(*{**ok, **kw}.values())

    nan = float("nan")
    for kw, what in ((dict(h=0), "1..7"), (dict(h=8), "1..7"), (dict(src_nodata=nan), "src_nodata must not be NaN"), (dict(has_src_nodata=2), "has_src_nodata"),
                     (dict(to_db=2), "to_db"), (dict(N=-1), "N >= 0"), (dict(G=0), "groups"), (dict(G=4), "groups"), (dict(M=-1), "member lists"),
                     (dict(M=4), "member lists"), (dict(total=-1), "2^40"), (dict(total=2**40), "2^40"), (dict(tiles=-1), "workgroups"),
                     (dict(tiles=2**31), "workgroups"), (dict(planes=None), "null pointer"), (dict(starts=None), "null pointer"),
                     (dict(sizes=None), "null pointer"), (dict(place=None), "null pointer"), (dict(lattice=None), "null pointer"),
                     (dict(member_ptr=None), "null pointer"), (dict(members=None), "null pointer"), (dict(tile_ptr=None), "null pointer"),
                     (dict(out=None), "null pointer"), (dict(counts=None), "null pointer"), (dict(planes=odd), "4-byte"),
                     (dict(out=ctypes.c_void_p((1 << 30) + 2)), "4-byte"), (dict(sizes=odd), "4-byte"), (dict(place=odd), "4-byte"),
                     (dict(lattice=odd), "4-byte"), (dict(member_ptr=odd), "4-byte"), (dict(members=odd), "4-byte"), (dict(counts=odd), "4-byte"),
                     (dict(starts=off8), "8-byte"), (dict(tile_ptr=off8), "8-byte"), (dict(out=one), "overlap"),
                     (dict(out=ctypes.c_void_p(4096 + 3996)), "overlap"), (dict(out=ctypes.c_void_p(4096 - 3996)), "overlap")):
        assert call(**kw) == -1 and what in err(), (kw, err())
    assert call(N=0, G=0, M=0, planes=None, starts=None, sizes=None, place=None, lattice=None, member_ptr=None, members=None, tile_ptr=None, out=None,
                counts=None, has_src_nodata=0, src_nodata=nan) == 0
    assert call(tiles=0) == 0 and call(out=ctypes.c_void_p(4096 + 4000), tiles=0) == 0
    with pytest.raises(built_lib.HipLibraryError, match="1..7"):
        built_lib.call("ig_s1_temporal", *{**ok, "h": 9}.values())


def test_prototype_is_declared_and_the_custom_op_follows_it():
    import re

    from instageo_amd import _lib, torch_ops

    text = open(os.path.join(ROOT, "include", "instageo_hip.h")).read()
    assert re.search(r"\bint ig_s1_temporal\(", text) and "Ratio sum at lattice pixel x" in text
    assert "s1_temporal.hip" in open(os.path.join(PKG, "csrc", "Makefile")).read()
    s = torch_ops.register()["s1_temporal"]
    for piece in ("Tensor? planes", "Tensor? starts", "Tensor? sizes", "Tensor? place", "Tensor? lattice", "Tensor? member_ptr", "Tensor? members",
                  "Tensor? tile_ptr", "int N", "int G", "int M", "int total", "int tiles", "int h", "int has_src_nodata", "float src_nodata", "int to_db",
                  "Tensor(a!)? out", "Tensor(b!)? counts"):
        assert piece in s, (piece, s)
    assert "stream" not in s
    proto = _lib.parse_header()["ig_s1_temporal"][1]
    assert len(proto) == 20 and proto[11] == "long" and proto[15] == "float"
    assert Q.TILE_W == 64 and Q.TILE_H == 32 and "TW = 64, TH = 32" in open(os.path.join(PKG, "csrc", "s1_temporal.hip")).read()
    assert Q.MAX_DATES == 32 and Q.MAX_MEMBERS == 64
