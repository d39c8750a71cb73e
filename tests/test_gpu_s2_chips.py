"""Sentinel-2 chips on the device (-m gpu): ``ig_s2_chip_cut`` against the sequential twin of the rule (tests/s2_chips_reference.py) over
planes of 10 m, 20 m and 60 m, a plane stored short, several dates and a downsampled grid, under every option set; a band buffer one
element off a 16-byte boundary; run-to-run determinism; and create_s2_chips on the device against the host path, file for file.  Every
comparison is ``torch.equal``: all outputs are integers or copies."""
import os

import numpy as np
import pytest
import torch

import s2_chips_reference as SR
from instageo_amd import s2_chips
from test_cpu_s2_chips import CHIP, CUT_PARAMS, GRANULE, _points, _write_tile, packed_case, run_cut

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(a).cuda()


def _same(got, want):
    for g, w in zip(got, want):
        w = torch.from_numpy(w)
        assert g.is_cuda and g.dtype == w.dtype and torch.equal(g.cpu(), w)


@pytest.mark.parametrize("name,S", CUT_PARAMS)
@pytest.mark.parametrize("option", list(SR.OPTIONS))
def test_s2_chip_cut_equals_the_twin(name, S, option):
    _, bands, scl = packed_case(name)
    _same(run_cut(name, S, option, bands, scl, xp=_dev), SR.twin(name, S, option))


@pytest.mark.parametrize("name", ["c6_10m", "sixty"])
def test_s2_chip_cut_on_a_band_buffer_one_element_off_a_16_byte_boundary(name):
    """The planes start 2 bytes after the allocation, so every row of every plane has another alignment than in the aligned runs; the SCL
    buffer starts one byte off."""
    k, planes, scls = SR.make_case(name)
    bands, starts, geom = SR.pack(planes, np.uint16, lead=1)
    scl, scl_starts, scl_geom = SR.pack(scls, np.uint8, lead=1)
    b, s = _dev(bands)[1:], _dev(scl)[1:]
    assert b.data_ptr() % 16 == 2 and s.data_ptr() % 16 == 1
    for option in ("each", "any_boa_nd7"):
        strategy, _, boa, rng, nd = SR.OPTIONS[option]
        got = s2_chips.cut(b, starts - 1, geom, s, scl_starts - 1, scl_geom, SR.SIZES[32], 32, k["grid"], dates=k["T"], class_bits=SR.CLASS_BITS,
                           strategy=strategy, no_data_value=nd, boa_offset=boa, valid_range=rng)
        _same(got, SR.twin(name, 32, option))


def test_s2_chip_cut_at_every_alignment_of_the_4_and_5_source_pixel_reads():
    """A 20 m band and a 20 m SCL under a 10 m grid: the 8 outputs of a segment come from 4 (even first column) or 5 (odd) source pixels,
    read as one 8-byte (band) or 4-byte (SCL) segment in the widest units the address allows.  The band buffer starts 0..3 elements and the
    SCL buffer 0..7 bytes into its allocation, so every alignment arm of both reads is taken; an arm that read nothing would leave the
    SCL mask empty or the band zero, which the comparison with the twin and the two assertions on the mask exclude."""
    grid, S, origins = (80, 80, 10), 32, [(3, 10), (6, 21)]  # both wholly inside: every segment takes the vector form
    planes = [(SR.band_plane(80, 80, seed=5), 10), (SR.band_plane(40, 40, seed=6), 20)]
    scls = [(SR.scl_plane(40, 40, seed=7), 20)]
    want = SR.cut(planes, scls, origins, S, grid, 1, SR.CLASS_BITS, "each")
    unmasked = SR.cut(planes, None, origins, S, grid, 1, SR.CLASS_BITS, "each")
    assert (want[0] != unmasked[0]).any() and (want[0] != 0).any()  # the mask removed some values and left others
    for lead in range(4):
        bands, starts, geom = SR.pack(planes, np.uint16, lead=lead)
        b = _dev(bands)[lead:]
        assert b.data_ptr() % 16 == 2 * lead
        for scl_lead in range(8):
            scl, scl_starts, scl_geom = SR.pack(scls, np.uint8, lead=scl_lead)
            s = _dev(scl)[scl_lead:]
            assert s.data_ptr() % 16 == scl_lead
            got = s2_chips.cut(b, starts - lead, geom, s, scl_starts - scl_lead, scl_geom, origins, S, grid, class_bits=SR.CLASS_BITS,
                               strategy="each")
            _same(got, want)
    chips = got[0].cpu().numpy()
    assert (chips != unmasked[0]).any() and (chips != 0).any()  # on the device output too


def test_two_runs_give_equal_outputs_and_a_window_masked_on_all_dates_has_no_valid_value():
    k, planes, scls = SR.make_case("t3c2", fully_masked=(64, 32), S=32)
    bands, starts, geom = SR.pack(planes, np.uint16)
    scl, ss, sg = SR.pack(scls, np.uint8)
    b, s = _dev(bands), _dev(scl)
    origins = [(64, 32), (0, 0), (7, 13)]
    for strategy in ("each", "any"):
        a1 = s2_chips.cut(b, starts, geom, s, ss, sg, origins, 32, k["grid"], class_bits=1 << 9, strategy=strategy)
        a2 = s2_chips.cut(b, starts, geom, s, ss, sg, origins, 32, k["grid"], class_bits=1 << 9, strategy=strategy)
        assert all(torch.equal(x.cpu(), y.cpu()) for x, y in zip(a1, a2))
        assert a1[1][0].item() == 0 and not a1[2][0].any().item() and a1[1][1].item() > 0
        _same(a1, SR.cut(planes, scls, origins, 32, k["grid"], 3, 1 << 9, strategy))


def test_create_s2_chips_on_the_device_writes_the_bytes_of_the_host_path(tmp_path):
    planes, scls, files, scl_files = _write_tile(str(tmp_path / "tiles"))
    outs = {}
    for dev in (None, "cuda"):
        out = str(tmp_path / f"out_{dev}")
        outs[dev] = (out, s2_chips.create_s2_chips(files, scl_files, _points(), out, device=dev, chip_size=CHIP, mask_types=["cloud"],
                                                   masking_strategy="each", window_size=1, src_crs=32613, granule_id=GRANULE, boa_offset=1000))
        out = str(tmp_path / f"grid_{dev}")
        outs[(dev, "grid")] = (out, s2_chips.create_s2_chips(files, scl_files, None, out, device=dev, chip_size=CHIP, mask_types=["cloud", "water"],
                                                             masking_strategy="any", valid_range=(0, 10000)))
    for a, b in ((outs[None], outs["cuda"]), (outs[(None, "grid")], outs[("cuda", "grid")])):
        assert a[1] == b[1] and len(a[1][0]) >= 2
        seen = 0
        for root, _, names in os.walk(a[0]):
            for n in names:
                pa = os.path.join(root, n)
                assert open(pa, "rb").read() == open(os.path.join(b[0], os.path.relpath(pa, a[0])), "rb").read(), n
                seen += 1
        assert seen >= len(a[1][0]) + 2  # the chips (and label maps), the CSV and the stats
    assert any(n.startswith("seg_map_") for n in os.listdir(os.path.join(outs["cuda"][0], "seg_maps")))
