"""The output options of chip and tile inference without a device: the options object and the two signatures it is built from cannot drift,
the option checks run in one fixed order before any file is touched, and shared labels are validated before any launch."""
import dataclasses
import inspect
import os
from types import SimpleNamespace

import pytest
import torch

from instageo_amd import postprocess, vectorize
from instageo_amd.infer_utils import OutputOptions, chip_inference, tile_inference

FIELDS = ("min_region", "connectivity", "sieve_passes", "save_regions", "save_polygons", "zones", "zone_id_property", "cog", "cog_blocksize",
          "overview_levels", "cog_compress")
TILE = ("/nonexistent/tile.tif", "/nonexistent/out")


def _loader():
    raise AssertionError("the loader must not be touched")
    yield


def test_options_are_the_output_keywords_of_both_signatures():
    fields = dataclasses.fields(OutputOptions)
    assert tuple(f.name for f in fields) == FIELDS and OutputOptions.__dataclass_params__.frozen
    tile, chip = inspect.signature(tile_inference).parameters, inspect.signature(chip_inference).parameters
    for f in fields:
        assert tile[f.name].default == f.default and type(tile[f.name].default) is type(f.default), f.name
        if f.name in chip:
            assert chip[f.name].default == f.default and type(chip[f.name].default) is type(f.default), f.name
    assert [f.name for f in fields if f.name in chip] == list(FIELDS[:7])  # chips: everything but the COG keys
    with pytest.raises(dataclasses.FrozenInstanceError):
        OutputOptions().min_region = 3


def test_the_first_check_that_objects_decides_the_error():
    reg = SimpleNamespace(cfg=SimpleNamespace(num_classes=1))
    wide = SimpleNamespace(cfg=SimpleNamespace(num_classes=128))
    # region options, polygons, zones, COG: in that order
    cases = [(dict(connectivity=5, cog_blocksize=100), None, "connectivity must be 4 or 8"),
             (dict(min_region=-1, zones="/nonexistent/z.geojson"), None, "min_region"),
             (dict(zones="/nonexistent/z.geojson", cog_blocksize=100), None, "is not a file"),
             (dict(cog_blocksize=100), None, "cog_blocksize"),
             (dict(save_regions=True, save_polygons=True, zones="/nonexistent/z.geojson"), reg, "min_region and save_regions need a class map"),
             (dict(save_polygons=True, zones="/nonexistent/z.geojson", cog_blocksize=100), reg, "save_polygons needs a class map"),
             (dict(zones="/nonexistent/z.geojson", cog_blocksize=100), reg, "zones needs a class map"),
             (dict(zones="/nonexistent/z.geojson", cog=True), wide, "is not a file"),
             (dict(cog=True), wide, "at most 127 classes")]
    for kw, model, what in cases:
        with pytest.raises(ValueError, match=what):
            OutputOptions(**kw).check(model)
        with pytest.raises(ValueError, match=what):
            tile_inference(*TILE, model, [0.0], [1.0], **kw)
        chip_kw = {k: v for k, v in kw.items() if not k.startswith("cog")}
        if chip_kw and not what.startswith(("cog", "at most")):
            with pytest.raises(ValueError, match=what):
                chip_inference(_loader(), TILE[1], model, **chip_kw)
    # without a model only the checks that need none can fire: what a regression head refuses passes, and the missing tile is met next
    for kw in (dict(save_regions=True, save_polygons=True, min_region=4), dict(cog=True)):
        OutputOptions(**kw).check(None)
        with pytest.raises(OSError):
            tile_inference(*TILE, None, [0.0], [1.0], **kw)
    with pytest.raises(ValueError, match="per-chip COGs are not produced"):
        OutputOptions(cog=True).check(None, chip_mode=True)
    OutputOptions().check(None, chip_mode=True), OutputOptions().check(reg), OutputOptions(cog=True).check(reg)
    # the temperature is looked at before the output options, the blend and tta options after them, the tile last
    with pytest.raises(ValueError, match="temperature"):
        tile_inference(*TILE, None, [0.0], [1.0], temperature=0.0, connectivity=5)
    with pytest.raises(ValueError, match="connectivity"):
        tile_inference(*TILE, None, [0.0], [1.0], blend="cubic", connectivity=5)
    with pytest.raises(ValueError, match="blend must be"):
        tile_inference(*TILE, None, [0.0], [1.0], blend="cubic")
    assert not os.path.exists("/nonexistent")


@pytest.mark.parametrize("fn", [postprocess.region_table, vectorize.region_rings])
def test_shared_labels_of_the_wrong_kind_are_refused_before_any_launch(fn):
    p = list(inspect.signature(fn).parameters.values())[-1]
    assert p.name == "labels" and p.default is None
    cm = torch.zeros((2, 5, 7), dtype=torch.int8)  # host tensors: a launch would fail with HipLibraryError, not ValueError
    for bad in (torch.zeros((2, 5, 7), dtype=torch.int64), torch.zeros((2, 5, 7), dtype=torch.int8), torch.zeros((5, 7), dtype=torch.int32),
                torch.zeros((2, 7, 5), dtype=torch.int32), torch.zeros((1, 2, 5, 7), dtype=torch.int32), [[0]]):
        with pytest.raises(ValueError, match="labels must be the int32 tensor"):
            fn(cm, 4, -1, labels=bad)
    with pytest.raises(ValueError, match="labels must be the int32 tensor"):
        fn(cm[0], 8, -1, torch.zeros((2, 5, 7), dtype=torch.int32))
