"""What the four dataset-preparation modes write, pinned file by file (no GPU): ``create_chips`` (points and bounding-box runs),
``create_raster_chips``, ``clean_chips`` and ``create_polygon_labels`` are driven through ``run_from_config`` on the host path over tiny
synthetic inputs built here, and everything they write and print is compared with ``tests/golden/prep_snapshot.json``.

The golden file records, per output file, the SHA-256 of the bytes (``.csv`` / ``.json``) or dtype, shape, the SHA-256 of the decoded
array and the sorted georeferencing tags as ``tiff.read`` returns them (``.tif``: independent of the zlib build), and the JSON line each
mode prints (the scratch folder replaced by ``<root>``).  It was written by ``python tests/test_cpu_prep_snapshot.py --write`` at the commit
BEFORE the modes were moved onto the shared host layer (``instageo_amd/prep.py``) and is committed as that run left it: the test pins the
behaviour of the code it replaced.  Do not regenerate it to make a change pass."""
import contextlib
import hashlib
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "instageo-e2e-geospatial-ml_amd"))

from instageo_amd import chips, clean, polygon_labels, raster_chips, tiff  # noqa: E402
from instageo_amd.config import load_config  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "prep_snapshot.json")
X0, Y0, PX, EPSG = 399960.0, 4500000.0, 30.0, 32613
H, W, S, T, C = 40, 48, 16, 2, 2
GEOKEYS = (3, (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, EPSG))
STAMPS = ("2022145T072619", "2022150T072619")


def _tags(x0=X0, y0=Y0):
    return {33550: (12, (PX, PX, 0.0)), 33922: (12, (0.0, 0.0, 0.0, x0, y0, 0.0)), 34735: GEOKEYS}


def _tile():
    """(T * C, H, W) int16 and (T, H, W) uint8 without a random generator: reflectances with scattered no-data zeros, one value above
    10000 and one negative; cloud over a corner of date 0, water over a stripe of date 1, chip (1, 1) cloudy on both dates."""
    b, r, c = np.meshgrid(np.arange(T * C), np.arange(H), np.arange(W), indexing="ij")
    tile = (1 + (37 * r + 101 * c + 1009 * b) % 9000).astype(np.int16)
    tile[(3 * r + 5 * c + b) % 11 == 0] = 0
    tile[:, 32:, 32:] = 0  # chip (2, 2) does not exist (H // S = 2); rows 32.. of columns 32.. are no-data
    tile[1, 3, 5], tile[2, 20, 40] = 12000, -7
    fmask = np.zeros((T, H, W), dtype=np.uint8)
    fmask[0, :6, :9] = 2  # cloud
    fmask[1, 8:11, :] = 32  # water
    fmask[:, 16:32, 16:32] = 2
    fmask[0, 25, 40] = 8  # cloud shadow: not among the mask types of the runs
    return tile, fmask


def _write_inputs(root):
    tile, fmask = _tile()
    os.makedirs(os.path.join(root, "tiles"))
    files, fmasks = [], []
    for t, stamp in enumerate(STAMPS):
        for c, band in enumerate(("B02", "B03")):
            files.append(os.path.join(root, "tiles", f"HLS.S30.T13TDE.{stamp}.v2.0.{band}.tif"))
            tiff.write(files[-1], tile[t * C + c], {"tags": _tags(), "nodata": -9999}, compress="deflate" if c else None)
        fmasks.append(os.path.join(root, "tiles", f"HLS.S30.T13TDE.{stamp}.v2.0.Fmask.tif"))
        tiff.write(fmasks[-1], fmask[t], {"tags": _tags(), "nodata": None})
    # (column, row) in pixels, label: two chips with several points, one point on a masked pixel, chip (1, 1) fully masked, a point below
    # the chip grid (row 35), one outside the tile, and one in the outer half-pixel fringe of chip (0, 1): it nominates, it does not paint
    px = [(3.5, 4.5, 1), (10.5, 11.5, 2), (12.2, 2.8, 0), (1.5, 1.5, 3), (20.5, 20.5, 1), (40.5, 5.5, 0), (45.1, 12.9, 2), (33.0, 9.5, 1),
          (47.4, 20.5, 1), (5.0, 16.2, 2), (20.5, 35.5, 1), (60.0, 5.0, 2)]
    with open(os.path.join(root, "points.csv"), "w") as f:
        f.write("x,y,label,date\n")
        for c, r, v in px:
            f.write(f"{X0 + c * PX!r},{Y0 - r * PX!r},{v},2022-05-25\n")
    # three label rasters on the tile's lattice: inside, half below the tile, far outside; a fourth record names another MGRS tile
    os.makedirs(os.path.join(root, "rasters"))
    r, c = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    for k, (r0, c0) in enumerate(((4, 8), (30, 28), (400, 900))):
        lab = ((r // 4 + c // 5 + k) % 3).astype(np.int8)
        lab[(r + 2 * c + k) % 13 == 0] = -1
        tiff.write(os.path.join(root, "rasters", f"label_x{k}_y0_20220525.tif"), lab, {"tags": _tags(X0 + c0 * PX, Y0 - r0 * PX), "nodata": -1})
    with open(os.path.join(root, "records.csv"), "w") as f:
        f.write("label_filename,date,mgrs_tile_id\n")
        for k in range(3):
            f.write(f"label_x{k}_y0_20220525.tif,2022-05-25,\n")
        f.write("label_x0_y0_20220525.tif,2022-05-25,T13TDF\n")
    # five features in the tile's map coordinates (pixels -> metres): a MultiPolygon with a hole, a triangle over it (the later feature
    # wins), a named class, one outside the grid, one degenerate (two distinct vertices)
    m = lambda ring: [[X0 + x * PX, Y0 - y * PX] for x, y in ring]  # noqa: E731
    box = lambda x0, y0, x1, y1: [(x0, y0), (x1, y0), (x1, y1), (x0, y1), (x0, y0)]  # noqa: E731
    feats = [("MultiPolygon", [[m(box(2.2, 1.7, 20.4, 14.1)), m(box(6.0, 4.0, 11.0, 9.0))], [m(box(33.3, 2.2, 46.9, 13.6))]], 1),
             ("Polygon", [m([(8.5, 2.5), (30.2, 7.5), (12.4, 15.9), (8.5, 2.5)])], 2),
             ("Polygon", [m(box(17.1, 18.3, 44.6, 30.8))], "maize"),
             ("Polygon", [m(box(100.0, 100.0, 120.0, 130.0))], 3),
             ("Polygon", [m([(5.0, 20.0), (9.0, 26.0), (5.0, 20.0)])], 1)]
    doc = {"type": "FeatureCollection", "features": [{"type": "Feature", "properties": {"cls": v, "name": f"field {i}"},
                                                      "geometry": {"type": kind, "coordinates": coords}} for i, (kind, coords, v) in enumerate(feats)]}
    with open(os.path.join(root, "fields.geojson"), "w") as f:
        json.dump(doc, f)
    return files, fmasks


def _plain(v):
    if isinstance(v, (tuple, list)):
        return [_plain(x) for x in v]
    return v.item() if isinstance(v, np.generic) else v


def _record(path):
    if path.endswith(".tif"):
        a, prof = tiff.read(path)
        return {"dtype": a.dtype.name, "shape": list(a.shape), "sha256": hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest(),
                "nodata": _plain(prof["nodata"]), "tags": [[int(k), _plain(prof["tags"][k])] for k in sorted(prof["tags"])]}
    with open(path, "rb") as f:
        return {"sha256": hashlib.sha256(f.read()).hexdigest()}


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


def snapshot(root):
    """Run the modes under ``root`` -> {case: {"line": the printed JSON, "files": {relative path: record}}}."""
    root = os.path.abspath(root)
    files, fmasks = _write_inputs(root)
    tiles = [f"chips.tiles=[{','.join(files)}]", f"chips.fmasks=[{','.join(fmasks)}]", "chips.chip_size=16", "chips.mask_types=[cloud,water]"]
    snap = {}

    def case(name, module, overrides, folder):
        line = _run(module, root, overrides)
        snap[name] = {"line": line, "files": _files(os.path.join(root, folder))}

    case("create_chips", chips, ["mode=create_chips"] + tiles + [f"chips.records_file={root}/points.csv", f"chips.src_crs={EPSG}",
                                                                  "chips.window_size=1", f"chips.output_directory={root}/points_out"], "points_out")
    case("create_chips_bbox", chips, ["mode=create_chips"] + tiles + ["chips.masking_strategy=any", f"chips.output_directory={root}/bbox_out"],
         "bbox_out")
    case("create_raster_chips", raster_chips,
         ["mode=create_raster_chips"] + [t.replace("chips.", "raster_chips.") for t in tiles] +
         [f"raster_chips.records_file={root}/records.csv", f"raster_chips.raster_path={root}/rasters", f"raster_chips.src_crs={EPSG}",
          "raster_chips.spatial_resolution=30.0", f"raster_chips.output_directory={root}/raster_out"], "raster_out")
    # the pairs of the first case, cleaned into a folder of their own beside them (their CSV's folder is the root of the relative paths);
    # the recorded folder holds the first case's files again: they are as they were
    case("clean_chips", clean,
         ["mode=clean_chips", f"clean.chips_dataset_csv={root}/points_out/chips_dataset.csv", f"clean.output_chips_dataset_csv={root}/points_out/cleaned.csv",
          "clean.drop_chips=true", "clean.no_data_value=0", "clean.no_data_threshold=0.5", "clean.clean_seg_maps=true", "clean.cleaning_method=buffer",
          "clean.window_size=1", f"clean.seg_map_output_dir={root}/points_out/cleaned_seg_maps"], "points_out")
    case("create_polygon_labels", polygon_labels,
         ["mode=create_polygon_labels", f"polygon_labels.features={root}/fields.geojson", f"polygon_labels.like={files[0]}",
          f"polygon_labels.src_crs={EPSG}", "polygon_labels.chip_size=16", "polygon_labels.value_property=cls", "polygon_labels.class_map={maize: 4}",
          "polygon_labels.date=20220525", "polygon_labels.mgrs_tile_id=T13TDE", f"polygon_labels.output_directory={root}/polygon_out"], "polygon_out")
    return snap


def test_the_modes_write_what_they_wrote_before_the_shared_host_layer(tmp_path):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = json.loads(json.dumps(snapshot(str(tmp_path))))
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name]["line"] == want[name]["line"], name
        assert sorted(got[name]["files"]) == sorted(want[name]["files"]), name
        for path, rec in want[name]["files"].items():
            assert got[name]["files"][path] == rec, (name, path)
    # the cases do what they are meant to exercise
    d = json.loads(json.dumps(want))
    assert d["create_chips"]["line"]["create_chips"]["chips"] >= 2 and d["create_chips_bbox"]["line"]["create_chips"]["seg_maps"] == 0
    assert d["create_raster_chips"]["line"]["create_raster_chips"]["chips"] >= 1
    assert d["clean_chips"]["line"]["clean_chips"]["rows_out"] >= 1
    assert d["create_polygon_labels"]["line"]["create_polygon_labels"]["features"] == {"read": 5, "outside": 1, "degenerate": 1}


if __name__ == "__main__":
    import tempfile

    if sys.argv[1:] != ["--write"]:
        raise SystemExit("usage: python tests/test_cpu_prep_snapshot.py --write   (at the commit whose behaviour is to be pinned)")
    with tempfile.TemporaryDirectory() as tmp:
        snap = snapshot(tmp)
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    with open(GOLDEN, "w") as f:
        json.dump(snap, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {GOLDEN}: " + ", ".join(f"{k}: {len(v['files'])} files" for k, v in snap.items()))
