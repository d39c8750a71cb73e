"""What the five chip-creation modes write, pinned file by file (no GPU): ``create_chips``, ``create_s2_chips``, ``create_s1_chips``,
``create_raster_chips`` and ``create_s2_raster_chips`` are driven through ``run_from_config`` on the host path over the tiny inputs the
``test_cpu_*chips.py`` files build, and everything they write and print is compared with ``tests/golden/chip_drivers_snapshot.json``.

Every mode runs with labels (``seg`` at S = 32, ``reg`` at S = 33) and in its bounding-box case (S = 33), on T = 2 dates (3 for the HLS
label rasters) under a mask; the Sentinel-1 builder's lattice of 64 x 48 pixels holds a single chip of side 33, so that mode runs at 16
and 32.  Every run is followed by a second one into the same folder after the first pair was deleted: one record is
fresh, the others take the ``existing`` branch.  The golden file records, per written ``.tif``, dtype, shape, the SHA-256 of the decoded
array, the no-data value and the sorted tags as ``tiff.read`` returns them; the rows of ``chips_dataset.csv``; the whole ``*_stats.json``;
and the JSON line the mode prints (the scratch folder replaced by ``<root>``).  It was written by ``python tools/chip_drivers_snapshot.py``
at the commit BEFORE the modes were moved onto the two drivers (``chips.create_from_points``, ``raster_chips.create_from_records``) and is
committed as that run left it: the test pins the behaviour of the code it replaced.  Do not regenerate it to make a change pass."""
import contextlib
import csv
import hashlib
import io
import json
import os

import numpy as np

import s2_chips_reference as SR
import test_cpu_chips as TC
import test_cpu_raster_chips as TR
import test_cpu_s1_chips as TV
import test_cpu_s2_chips as TS
import test_cpu_s2_raster_chips as TQ
import warp_reference as WR
from instageo_amd import chips, raster_chips, s1_chips, s2_chips, s2_raster_chips, tiff
from instageo_amd.config import load_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "chip_drivers_snapshot.json")
H, W = 70, 100  # the grid of the two point modes whose builders take a size: 2 x 3 complete chips of side 32 or 33
# (column, row, label) in pixels: chip (0, 0) three points, two of them with overlapping windows; chip (1, 1) and chip (2, 0) one each; chip
# (2, 1) only from its outer half-pixel fringe (it is nominated and not painted); one point right of the grid's last complete chip
POINTS = [(3.5, 4.5, 1), (10.5, 11.5, 2), (11.2, 12.4, 3), (40.5, 45.5, 1), (75.5, 5.5, 0), (66.7, 40.2, 2), (99.4, 20.5, 1)]


def _points(path, x0, y0, px):
    with open(path, "w") as f:
        f.write("x,y,label,date\n")
        for c, r, v in POINTS:
            f.write(f"{x0 + c * px!r},{y0 - r * px!r},{v},2022-05-25\n")
    return path


def _s2_tile(folder):
    """``test_cpu_s2_chips._write_tile`` on the H x W grid: two dates of a 10 m and a 20 m band under a 20 m SCL; cloud on both dates over
    10 m rows 34..63 of columns 34..63, and on the first date only at 10 m pixel (4, 76)."""
    os.makedirs(folder, exist_ok=True)
    files, scl_files = [], []
    for t, stamp in enumerate(TS.STAMPS):
        for c, (band, p) in enumerate(TS.BANDS):
            a = SR.band_plane(H * 10 // p, W * 10 // p, seed=7 * t + c)
            files.append(os.path.join(folder, f"T13TDE_{stamp}_{band}_{p}m.tif"))
            tiff.write(files[-1], a, {"tags": TS.tags_of(p), "nodata": None}, compress="deflate" if c else None)
        s = SR.scl_plane(H // 2, W // 2, seed=50 + t)
        s[17:32, 17:32] = 9
        s[2, 38] = 9 if t == 0 else 4
        scl_files.append(os.path.join(folder, f"T13TDE_{stamp}_SCL_20m.tif"))
        tiff.write(scl_files[-1], s, {"tags": TS.tags_of(20), "nodata": None})
    return files, scl_files


@contextlib.contextmanager
def _side(module, S):
    """The label rasters of ``module.write_granule`` at side ``S`` (the builder reads the module's ``S``)."""
    old, module.S = module.S, S
    try:
        yield
    finally:
        module.S = old


def _plain(v):
    if isinstance(v, (tuple, list)):
        return [_plain(x) for x in v]
    return v.item() if isinstance(v, np.generic) else v


def _record(path):
    if path.endswith(".tif"):
        a, prof = tiff.read(path)
        return {"dtype": a.dtype.name, "shape": list(a.shape), "sha256": hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest(),
                "nodata": _plain(prof["nodata"]), "tags": [[int(k), _plain(prof["tags"][k])] for k in sorted(prof["tags"])]}
    if path.endswith(".csv"):
        with open(path, newline="") as f:
            return {"rows": list(csv.reader(f))}
    with open(path) as f:
        return {"json": json.load(f)}


def _files(folder):
    out = {}
    for base, _, names in os.walk(folder):
        for n in names:
            p = os.path.join(base, n)
            out[os.path.relpath(p, folder).replace(os.sep, "/")] = _record(p)
    return dict(sorted(out.items()))


def _run(module, root, overrides):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        assert module.run_from_config(load_config("config", overrides)) == 0
    lines = buf.getvalue().strip().splitlines()
    assert len(lines) == 1
    return json.loads(lines[0].replace(root, "<root>"))


def _listing(files):
    return "[" + ",".join(files) + "]"


def snapshot(root):
    """Run the modes under ``root`` -> {case: {"line", "files", "again": {"line", "files"}}}."""
    root = os.path.abspath(root)
    snap = {}

    def case(name, module, section, overrides):
        out = os.path.join(root, "out", name)
        args = [f"mode=create_{section}"] + [f"{section}.{o}" for o in overrides] + [f"{section}.output_directory={out}"]
        line = _run(module, root, args)
        snap[name] = {"line": line, "files": _files(out)}
        kept = sorted(os.listdir(os.path.join(out, "chips")))
        assert len(kept) >= 2, (name, kept)
        os.remove(os.path.join(out, "chips", kept[0]))  # the first pair goes: it is cut again, the others exist
        if os.path.isdir(os.path.join(out, "seg_maps")):
            os.remove(os.path.join(out, "seg_maps", sorted(os.listdir(os.path.join(out, "seg_maps")))[0]))
        snap[name]["again"] = {"line": _run(module, root, args), "files": _files(out)}

    # HLS tiles, points
    _, _, files, fmasks = TC._write_tile(os.path.join(root, "hls"), H=H, W=W)
    pts = _points(os.path.join(root, "hls_points.csv"), TC.X0, TC.Y0, TC.PX)
    hls = [f"tiles={_listing(files)}", f"fmasks={_listing(fmasks)}", "mask_types=[cloud,water]"]
    case("chips_seg", chips, "chips", hls + [f"records_file={pts}", "src_crs=32613", "window_size=1", "chip_size=32"])
    case("chips_reg", chips, "chips", hls + [f"records_file={pts}", "src_crs=32613", "task_type=reg", "masking_strategy=any", "window_size=2", "chip_size=33"])
    case("chips_bbox", chips, "chips", hls + ["masking_strategy=any", "chip_size=33"])
    # Sentinel-2 tiles, points
    files, scl = _s2_tile(os.path.join(root, "s2"))
    pts = _points(os.path.join(root, "s2_points.csv"), TS.X0, TS.Y0, 10.0)
    s2 = [f"tiles={_listing(files)}", f"scl={_listing(scl)}", "mask_types=[cloud]", f"granule_id={TS.GRANULE}"]
    case("s2_chips_seg", s2_chips, "s2_chips", s2 + [f"records_file={pts}", "src_crs=32613", "window_size=1", "chip_size=32", "boa_offset=1000"])
    case("s2_chips_reg", s2_chips, "s2_chips", s2 + [f"records_file={pts}", "src_crs=32613", "task_type=reg", "masking_strategy=any", "window_size=2", "chip_size=33"])
    case("s2_chips_bbox", s2_chips, "s2_chips", s2 + ["masking_strategy=any", "chip_size=33", "valid_range=[0,10000]"])
    # Sentinel-1 scenes, points (the builder's 64 x 48 lattice: two complete chips of side 32 below one another; at 33 there is one, so
    # the bounding-box case runs at 32 and the reg case at 16 next to it)
    import pandas as pd

    scenes, _, _, table = TV.write_stack(os.path.join(root, "s1"))
    pts = os.path.join(root, "s1_points.csv")
    pd.DataFrame(table).to_csv(pts, index=False)
    text = "[" + ",".join("[" + ",".join(_listing(s) for s in d) + "]" for d in scenes) + "]"
    s1 = [f"scenes={text}", "src_nodata=-32768"]
    case("s1_chips_seg", s1_chips, "s1_chips", s1 + [f"records_file={pts}", "masking_strategy=any", "window_size=1", "chip_size=16"])
    case("s1_chips_reg", s1_chips, "s1_chips", s1 + [f"records_file={pts}", "task_type=reg", "chip_size=16", "clip=[0.0,0.4]"])
    case("s1_chips_bbox", s1_chips, "s1_chips", s1 + ["chip_size=32"])
    # HLS tiles, label rasters
    for name, S, task in (("raster_chips_seg", 32, "seg"), ("raster_chips_reg", 33, "reg")):
        with _side(TR, S):
            _, _, files, fmasks, records, rasters = TR.write_granule(os.path.join(root, name), task)
        hls = [f"tiles={_listing(files)}", f"fmasks={_listing(fmasks)}", "mask_types=[cloud,water]", f"spatial_resolution={TR.RES}", f"chip_size={S}"]
        more = ["task_type=reg", "qa_check=false", "snap=false"] if task == "reg" else []
        case(name, raster_chips, "raster_chips", hls + [f"records_file={records}", f"raster_path={rasters}"] + more)
    lon, lat = (float(v) for v in WR.to_lonlat(TR.RR.U36, TR.RR.X0 + TR.RR.PX * 4, TR.RR.Y0 - TR.RR.PX * 36))
    boxes = os.path.join(root, "hls_boxes.json")
    with open(boxes, "w") as f:
        json.dump([[lon, lat, lon + 2 * 33 * TR.RES - 1e-9, lat + 33 * TR.RES - 1e-9]], f)
    case("raster_chips_bbox", raster_chips, "raster_chips", hls[:4] + ["chip_size=33", "is_bbox_feature=true", f"bbox_feature_path={boxes}", "date=2022-06-08"])
    # Sentinel-2 tiles, label rasters
    for name, S in (("s2_raster_chips_seg", 32), ("s2_raster_chips_noqa", 33)):
        with _side(TQ, S):
            _, _, files, scl, records, rasters = TQ.write_granule(os.path.join(root, name))
        s2 = [f"tiles={_listing(files)}", f"scl={_listing(scl)}", "mask_types=[cloud]", f"spatial_resolution={TQ.RES}", f"chip_size={S}"]
        more = ["qa_check=false", "snap=false", "masking_strategy=any"] if name.endswith("noqa") else []
        case(name, s2_raster_chips, "s2_raster_chips", s2 + [f"records_file={records}", f"raster_path={rasters}"] + more)
    lon, lat = (float(v) for v in WR.to_lonlat(TQ.QR.U36, TQ.QR.X0 + 100.0, TQ.QR.Y0 - 600.0))
    boxes = os.path.join(root, "s2_boxes.json")
    with open(boxes, "w") as f:
        json.dump([[lon, lat, lon + 1.9 * 33 * TQ.RES, lat + 0.9 * 33 * TQ.RES]], f)
    case("s2_raster_chips_bbox", s2_raster_chips, "s2_raster_chips", s2[:4] + ["chip_size=33", "is_bbox_feature=true", f"records_file={boxes}"])
    return snap


def test_the_modes_write_what_they_wrote_before_the_two_drivers(tmp_path):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = json.loads(json.dumps(snapshot(str(tmp_path))))
    assert sorted(got) == sorted(want)
    for name in want:
        for w, g in ((want[name], got[name]), (want[name]["again"], got[name]["again"])):
            assert g["line"] == w["line"], name
            assert sorted(g["files"]) == sorted(w["files"]), name
            for path, rec in w["files"].items():
                assert g["files"][path] == rec, (name, path)
    # the cases do what they are meant to exercise: every mode keeps chips with and without labels, and the second run finds existing files
    for name, case in want.items():
        (mode, line), = case["line"].items()
        assert line["chips"] >= 2 and (line["seg_maps"] == 0) == name.endswith("bbox"), name
        stats = next(rec["json"] for path, rec in case["again"]["files"].items() if path.endswith("_stats.json"))
        assert stats["dropped"]["existing"] >= 1 and stats["kept"] == 1, name
