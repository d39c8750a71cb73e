"""The pixel picks of the five value kernels against the 50-digit truth of tests/golden/warp_pick_truth.npz (-m gpu).

``ig_warp``, ``ig_chip_warp`` (with its label maps), ``ig_s1_chip_warp``, ``ig_s2_chip_warp`` and ``ig_tile_render`` each compile their
own copy of csrc/warp_proj.h and then turn its result into a pixel pick; until now only ``ig_warp_coords`` stood on the independent truth
(tests/test_gpu_projection_truth.py).  Here every kernel warps, in ONE launch per case on the FULL destination grid, source rasters that
encode their own indices (tests/warp_pick_reference.py), and what arrives at the sampled pixels (corners, both sides of every 64 x 64
block seam, a seeded scatter) must name the pixel that the truth names.  The checks are those of tests/test_cpu_warp_picks.py, which holds
the twin and the host paths to them; this module only puts the kernels behind the same calls.  numpy, torch and the fixture: neither
mpmath nor the twin is needed.

ASSERTED, outside the tie zone (1e-6 m + 4 ulp from a pixel boundary; derived in tests/warp_pick_reference.py): the decoded (row, col)
EQUALS the true pick; inside / outside the raster matches the truth (fill, NaN, ``src_id`` 255, no-data, validity 0, label -1, alpha 0);
``src_id`` is the source whose raster holds the true pick under LAST and under FIRST.  Bilinear: |value - a (u - 1/2) - b (v - 1/2) - k|
within the derived bar wherever every source is whole or out of reach.  Map tiles: the ``rgb`` style with ``rescale`` = (0, 255) passes
integers 0 ... 126 through unchanged, so the decode is exact and the kernel is in.

MEASURED on an MI355X (104 tests, 2.6 s in all).  Nearest picks, every kernel and every case (ig_warp int8 and float32 under LAST and
FIRST, ig_chip_warp with its label maps, ig_s1_chip_warp, ig_s2_chip_warp at 10 m and at 20 m on six cases, ig_tile_render rgb on
wm_to_utm36): 250 of 250 samples compared, 0 in a tie zone, every decoded pixel equal to the true pick.  Bilinear, samples compared (the
rest lie in the clipped border of one of the two sources) and worst |value - truth| as a share of the bar, LAST / FIRST; the error is the
float32 rounding of the result (half an ulp of values up to 1500 is 6e-5), the coordinate part of the bar is 5e-7 and less:
  utm37_to_utm36_lat40p6 247 0.967 0.959 | utm37_to_utm36_lat80 248 0.965 0.967 | utm36_north_to_south_equator 249 0.777 0.777
  utm60_to_utm1_across_180 246 0.985 0.976 | wm_to_utm36 249 0.987 0.971 | utm36_to_wm 249 0.959 0.932
  geographic_to_utm36 246 0.982 0.982 | utm21s_to_geographic 247 0.981 0.981 | custom_tm_to_utm32 250 0.956 0.962
  utm36_same_system 248 0.930 0.930 | utm36_to_utm37_thin 249 0.960 0.984 | utm36_to_utm37_partly_outside 247 0.968 0.968
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_cpu_warp_picks as C  # noqa: E402
import warp_pick_reference as PR  # noqa: E402
from instageo_amd import ops, warp  # noqa: E402

DEV = "cuda"
FIX, NAMES = C.FIX, C.NAMES


class Device(C.Host):
    """The kernels behind the calls of the checks."""

    name = "device"
    put = staticmethod(lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV))
    get = staticmethod(lambda t: t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t))

    def warp(self, arrays, srcs, case, resampling, rule):
        systems, grids = [case["src_crs"]] * len(srcs), [s.grid for s in srcs]
        sizes = np.array([s.size for s in srcs], dtype=np.int64)
        n = sizes[:, 0] * sizes[:, 1]
        ptr, idx = warp.block_lists(case["dst_crs"], case["dst_grid"], case["shape"], systems, grids, sizes)
        return ops.warp(torch.cat([a.reshape(-1) for a in arrays]), np.cumsum(n) - n, systems, grids, sizes, ptr, idx, case["dst_crs"],
                        case["dst_grid"], case["shape"], resampling, rule, -1, src_id=True)

    def tiles(self, level, src, case, grids):
        return ops.tile_render([level], case["src_crs"], src.grid, grids, np.zeros(len(grids), dtype=np.int32), C.S, "rgb", rescale=(0.0, 255.0))


def test_fixture_is_the_one_the_cpu_tests_pinned():
    assert len(NAMES) == 12 and sum(len(c["rc"]) for c in FIX.values()) == 3000


@pytest.mark.parametrize("rule", C.RULES)
@pytest.mark.parametrize("dtype", [np.int8, np.float32], ids=["int8", "float32"])
@pytest.mark.parametrize("name", NAMES)
def test_warp_nearest(name, dtype, rule):
    C.check_warp_nearest(Device(), FIX[name], dtype, rule)


@pytest.mark.parametrize("rule", C.RULES)
@pytest.mark.parametrize("name", NAMES)
def test_warp_bilinear(name, rule):
    C.check_warp_bilinear(Device(), FIX[name], rule)


@pytest.mark.parametrize("name", NAMES)
def test_chip_warp_and_label_maps(name):
    C.check_chip_warp(Device(), FIX[name])


@pytest.mark.parametrize("name", NAMES)
def test_s1_chip_warp(name):
    C.check_s1_chip_warp(Device(), FIX[name])


@pytest.mark.parametrize("name", PR.S2_CASES)
def test_s2_chip_warp(name):
    C.check_s2_chip_warp(Device(), FIX[name])


@pytest.mark.parametrize("name", C.FROM_WEB_MERCATOR)
def test_tile_render(name):
    C.check_tiles(Device(), FIX[name])
