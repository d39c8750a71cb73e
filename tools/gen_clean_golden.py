"""Records tests/golden/clean_reference.npz from the reference's own data cleaner.

    python tools/gen_clean_golden.py /path/to/reference/checkout [output.npz]

The reference's ``instageo/data/data_cleaner.py`` is imported from the given checkout and its ``should_drop_chip``,
``buffer_observation_pixels`` and ``limit_seg_map_to_observation_pixels`` run on rasters that live in memory: ``rasterio``, ``pyproj``,
``absl`` and ``mgrs`` are replaced by the small stand-ins below (an "opened file" is an array held in a dict, written files go back into
it; the transformer is the identity, so the ``limit`` map is in EPSG:4326).  Nothing of the reference is copied here and no test runs
this script: the tests read the recorded arrays."""
import importlib.util
import os
import sys
import types

import numpy as np

FILES = {}  # path -> {"array": (bands, H, W), "transform": (X0, Y0, sx, sy), "crs": 4326}


class _Dataset:
    def __init__(self, path, mode="r", **profile):
        self.path, self.mode = path, mode
        if mode == "r":
            self.rec = FILES[path]
        else:
            self.rec = {"array": None, "transform": profile.get("transform"), "crs": profile.get("crs")}
            FILES[path] = self.rec

    def read(self):
        return self.rec["array"].copy()

    def write(self, array):
        self.rec["array"] = np.array(array)

    @property
    def profile(self):
        return {"transform": self.rec["transform"], "crs": self.rec["crs"]}

    @property
    def crs(self):
        return self.rec["crs"]

    def index(self, x, y):
        X0, Y0, sx, sy = self.rec["transform"]
        return int(np.floor((Y0 - y) / sy)), int(np.floor((x - X0) / sx))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def _install_stand_ins():
    rasterio = types.ModuleType("rasterio")
    rasterio.open = lambda path, mode="r", **kw: _Dataset(path, mode, **kw)
    pyproj = types.ModuleType("pyproj")

    class Transformer:
        @staticmethod
        def from_crs(src, dst, always_xy=True):
            assert src == 4326 and dst == 4326, "the stand-in transformer is the identity"
            return Transformer()

        def transform(self, x, y):
            return np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)

    pyproj.Transformer = Transformer
    mgrs = types.ModuleType("mgrs")
    mgrs.MGRS = object
    absl = types.ModuleType("absl")

    class _Flags(types.ModuleType):
        FLAGS = types.SimpleNamespace()

        def __getattr__(self, name):  # DEFINE_*, mark_flag_as_required
            return lambda *a, **k: None

    absl.flags = _Flags("absl.flags")
    absl.app = types.SimpleNamespace(run=lambda main: None)
    absl.logging = types.SimpleNamespace(warning=lambda *a, **k: None, info=lambda *a, **k: None, error=lambda *a, **k: None)
    for name, mod in (("rasterio", rasterio), ("pyproj", pyproj), ("mgrs", mgrs), ("absl", absl), ("absl.flags", absl.flags)):
        sys.modules[name] = mod
    os.makedirs = lambda *a, **k: None  # the cleaned "files" stay in FILES


def main(argv):
    ref = argv[1]
    out = argv[2] if len(argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                                                     "clean_reference.npz")
    real_makedirs = os.makedirs
    _install_stand_ins()
    spec = importlib.util.spec_from_file_location("ref_data_cleaner", os.path.join(ref, "instageo", "data", "data_cleaner.py"))
    dc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dc)
    import pandas as pd

    rng = np.random.default_rng(2024)
    rec = {}
    shapes = [(48, 40), (17, 33), (40, 48), (9, 9), (31, 1), (25, 26)]
    windows = [1, 2, 3, 3, 2, 1]
    nd, ign = -9999, -1
    for k, ((H, W), w) in enumerate(zip(shapes, windows)):
        seg = np.full((H, W), ign, dtype=np.int16)
        src = rng.random((H, W)) < (0.04, 0.3, 0.08, 0.2, 0.3, 0.02)[k]
        src[0, 0] = src[H - 1, W - 1] = True
        seg[src] = rng.integers(0, 5, size=int(src.sum()))
        chip = rng.integers(1, 3000, size=(3, H, W)).astype(np.int16)
        one = rng.random((H, W)) < 0.25
        chip[rng.integers(0, 3), one] = nd
        every = rng.random((H, W)) < 0.15
        if k < 2:
            every |= src & (rng.random((H, W)) < 0.5)  # all-no-data pixels on sources
        every[H // 2, 0] = True
        chip[:, every] = nd
        FILES[f"/in/chip{k}.tif"] = {"array": chip, "transform": None, "crs": 4326}
        FILES[f"/in/seg{k}.tif"] = {"array": seg[None], "transform": None, "crs": 4326}
        path = dc.buffer_observation_pixels(f"/in/seg{k}.tif", f"/in/chip{k}.tif", w, nd, ign, f"/out{k}")
        rec[f"buf{k}_seg"], rec[f"buf{k}_chip"], rec[f"buf{k}_w"] = seg, chip, np.int64(w)
        rec[f"buf{k}_no_data"], rec[f"buf{k}_ignore"] = np.int64(nd), np.int64(ign)
        rec[f"buf{k}_out"] = FILES[path]["array"][0]
        for s in ("any", "all"):
            m = np.any(chip == nd, axis=0) if s == "any" else np.all(chip == nd, axis=0)
            ratio = float(m.sum() / float(m.size))
            thr = np.array([np.nextafter(ratio, -1.0), ratio, np.nextafter(ratio, 2.0)])
            rec[f"buf{k}_drop_{s}_thr"] = thr
            rec[f"buf{k}_drop_{s}"] = np.array([bool(dc.should_drop_chip(f"/in/chip{k}.tif", float(t), nd, s)) for t in thr])
    rec["n_buffer"] = np.int64(len(shapes))
    # limit: a 30 x 36 map in EPSG:4326 (0.001 degree pixels); duplicates, points outside, points of another tile / date
    H, W, X0, Y0, px = 30, 36, 10.0, 45.0, 0.001
    seg = rng.integers(0, 4, size=(H, W)).astype(np.int16)
    name = "seg_map_20200101_L30_T13SCS_2020001T173930_9_11.tif"
    FILES[f"/in/{name}"] = {"array": seg[None], "transform": (X0, Y0, px, px), "crs": 4326}
    cells = [(0, 0), (29, 35), (4, 7), (4, 7), (12, 3), (-2, 5), (30, 1), (3, 36), (3, -1), (20, 20)]
    xs = [X0 + (c + 0.3) * px for r, c in cells] + [X0 + 5.5 * px, X0 + 6.5 * px]
    ys = [Y0 - (r + 0.6) * px for r, c in cells] + [Y0 - 5.5 * px, Y0 - 6.5 * px]
    tiles = ["13SCS"] * len(cells) + ["13SCT", "13SCS"]
    dates = ["2020-01-01"] * len(cells) + ["2020-01-01", "2020-01-02"]
    obs = pd.DataFrame({"x": xs, "y": ys, "mgrs_tile_id": tiles, "date": dates})
    path = dc.limit_seg_map_to_observation_pixels(f"/in/{name}", obs, ign, "/lim")
    rec["lim_seg"], rec["lim_out"], rec["lim_ignore"] = seg, FILES[path]["array"][0].astype(np.int16), np.int64(ign)
    rec["lim_x"], rec["lim_y"], rec["lim_tile"], rec["lim_date"] = np.array(xs), np.array(ys), np.array(tiles), np.array(dates)
    rec["lim_scale"], rec["lim_tie"], rec["lim_name"] = np.array([px, px, 0.0]), np.array([0.0, 0.0, 0.0, X0, Y0, 0.0]), np.array(name)
    other = "seg_map_20200105_L30_T13SCS_2020005T173930_9_11.tif"
    FILES[f"/in/{other}"] = {"array": seg[None], "transform": (X0, Y0, px, px), "crs": 4326}
    rec["lim_none_name"] = np.array(other)
    rec["lim_none_returned_none"] = np.bool_(dc.limit_seg_map_to_observation_pixels(f"/in/{other}", obs, ign, "/lim") is None)
    real_makedirs(os.path.dirname(out), exist_ok=True)
    np.savez_compressed(out, **rec)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(sys.argv)
