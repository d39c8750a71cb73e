"""``ig_s1_temporal`` on the device against the sequential twin of the rule (tests/s1_temporal_reference.py) on one stack of two groups in
one launch: group 0 has three dates on a lattice of 42 x 80 (two tiles of 64 x 32 both ways, ragged: halos cross the seams), planes at
offsets, a second orbit slice of date 1 that overlaps the first, NaN holes, +-inf, src_nodata values, negative values and a 9 x 9 patch of
zeros (m = 0: a passthrough); group 1 has a 1 x 1 plane and planes one row / one column past a tile.  h = 1, 3 and 7, src_nodata given and
not.  The input buffer starts one element off, so a plane starts 4-byte but not 16-byte aligned.

The linear scale uses correctly rounded float64 operations only: bit for bit.  A dB output goes through log10 on either side, each within
about one float64 ulp of the exact value, so the float32 roundings can differ only next to a rounding tie: at most 1 float32 ulp, measured on
the int32 bit views, with equal absent / dropped patterns and counts."""
import numpy as np
import pytest
import torch

import s1_temporal_reference as R
from instageo_amd import s1_temporal as Q

pytestmark = pytest.mark.gpu
POISON = 0x5A5A5A5A


def on_device(k):
    planes = torch.from_numpy(k["planes"].copy()).cuda()[1:]
    assert planes.data_ptr() % 16 == 4
    return planes


def run(k, planes, h, with_snd, scale):
    return Q.temporal(planes, k["starts"], k["sizes"], k["group"], k["date"], k["offsets"], 2 * h + 1, R.SND if with_snd else None, scale)


@pytest.mark.parametrize("h,with_snd", R.RUNS)
def test_linear_equals_the_twin_bit_for_bit_and_db_within_one_ulp(h, with_snd):
    k = R.stack()
    planes = on_device(k)
    for scale in ("linear", "db"):
        out, counts = run(k, planes, h, with_snd, scale)
        assert out.is_cuda and counts.is_cuda and out.dtype == torch.float32 and counts.dtype == torch.int32 and counts.shape == (len(R.STACK), 4)
        got, (want, wcounts) = R.bits_of(out.cpu().numpy()), R.expected(h, with_snd, scale)
        assert np.array_equal(counts.cpu().numpy(), wcounts), (h, scale, counts.cpu().tolist(), wcounts.tolist())
        assert np.array_equal(got == R.QNAN, want == R.QNAN), (h, scale, "the absent / dropped pattern")
        worst = R.ulps(got, want)
        print(f"h={h} src_nodata={with_snd} {scale}: {int((got != want).sum())} of {got.size} differ, at most {worst} ulp")
        if scale == "linear":
            assert np.array_equal(got, want), (h, int((got != want).sum()), worst)
        else:
            assert worst <= 1, (h, worst)


def test_device_output_equals_the_host_path_and_runs_repeat():
    k = R.stack()
    planes = on_device(k)
    for h, with_snd in R.RUNS:
        host, hcounts = run(k, k["planes"][1:], h, with_snd, "linear")
        a, ca = run(k, planes, h, with_snd, "linear")
        b, cb = run(k, planes, h, with_snd, "linear")
        assert np.array_equal(R.bits_of(a.cpu().numpy()), R.bits_of(host)) and np.array_equal(ca.cpu().numpy(), hcounts)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(ca, cb)
        da, cda = run(k, planes, h, with_snd, "db")
        db, cdb = run(k, planes, h, with_snd, "db")
        assert torch.equal(da.view(torch.int32), db.view(torch.int32)) and torch.equal(cda, cdb)


def test_planes_permuted_in_the_buffer_with_gaps_give_the_same_bits_and_leave_the_gaps_alone():
    from instageo_amd import ops

    k = R.stack()
    flat = k["planes"][1:]
    order = [5, 1, 6, 0, 3, 4, 2]  # plane 1 stays ahead of plane 3, the second slice of its date
    pix = [H * W for H, W in k["sizes"]]
    gap, at, starts = 37, 5, {}
    for p in order:
        starts[p] = at
        at += pix[p] + gap
    buf = np.full(at, 777.0, dtype=np.float32)  # the gaps hold a present value: nothing may read it into a window
    for p in order:
        buf[starts[p] : starts[p] + pix[p]] = flat[int(k["starts"][p]) : int(k["starts"][p]) + pix[p]]
    pick = lambda v: [v[p] for p in order]  # noqa: E731
    out = torch.full((at,), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
    got, counts = ops.s1_temporal(torch.from_numpy(buf).cuda(), [starts[p] for p in order], pick(k["sizes"]), pick(k["group"]), pick(k["date"]),
                                  pick(k["offsets"]), 7, R.SND, "linear", out=out)
    got = R.bits_of(got.cpu().numpy())
    want, wcounts = R.expected(3, True, "linear")
    inside = np.zeros(at, dtype=bool)
    for i, p in enumerate(order):
        inside[starts[p] : starts[p] + pix[p]] = True
        assert np.array_equal(got[starts[p] : starts[p] + pix[p]], want[int(k["starts"][p]) : int(k["starts"][p]) + pix[p]]), p
        assert counts[i].cpu().tolist() == wcounts[p].tolist()
    assert (got[~inside] == POISON).all() and not (got[inside] == POISON).any()


def test_one_date_returns_the_input_bits():
    """c = 1 everywhere: y = m ((x / m) / 1), and (x / m) m in float64 rounds back to the float32 x for gamma values in [1e-4, 10]."""
    rng = np.random.default_rng(5)
    a = np.clip(rng.gamma(R.LOOKS, 0.3 / R.LOOKS, size=70 * 131), 1e-4, 10.0).astype(np.float32)
    a[rng.random(a.shape) < 0.03] = np.nan
    out, counts = Q.temporal(torch.from_numpy(a).cuda(), [0, 70 * 66], [(70, 66), (70, 65)], [0, 1], [0, 0], [(0, 0), (3, 2)], 7)
    got = R.bits_of(out.cpu().numpy())
    present = ~np.isnan(a)
    assert np.array_equal(got[present], R.bits_of(a)[present]) and (got[~present] == R.QNAN).all()
    n = [int(present[: 70 * 66].sum()), int(present[70 * 66 :].sum())]
    assert counts.cpu().tolist() == [[n[0], 0, 0, n[0]], [n[1], 0, 0, n[1]]]


def _raw(planes, st, ss, T, h, out, counts, place=None, members=None, tile_ptr=None, lattice=None):
    """The op itself on tables of the test's making: nothing checks them on the host."""
    from instageo_amd import torch_ops

    torch_ops.register()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    tp = T.tile_ptr if tile_ptr is None else tile_ptr
    N, G = st.shape[0], T.lattice.shape[0]
    torch.ops.instageo_mi355x.s1_temporal(planes, dev(st), dev(ss.reshape(-1)), dev((T.place if place is None else place).reshape(-1)),
                                          dev((T.lattice if lattice is None else lattice).reshape(-1)), dev(T.member_ptr),
                                          dev(T.members if members is None else members), dev(tp), N, G, N, planes.shape[0], int(tp[-1]), h, 1, R.SND, 0,
                                          out, counts)


def test_tables_the_wrapper_would_refuse_are_skipped_by_the_kernel():
    """The second fence: the tables are on the device, so the kernel does not trust them.  A skipped plane keeps the poison of ``out`` and
    its counts stay zero; the other planes are filtered as if it were not there (the host path on the stack without it)."""
    k = R.stack()
    planes = on_device(k)
    flat = k["planes"][1:]
    total, N, h = planes.shape[0], len(R.STACK), 3
    st, ss, _, _, _, T = Q.check_temporal(total, k["starts"], k["sizes"], k["group"], k["date"], k["offsets"], 7, R.SND, "linear")
    skip = 3  # the second slice of date 1
    lo, hi = int(st[skip]), int(st[skip]) + int(ss[skip, 0]) * int(ss[skip, 1])
    rest = [p for p in range(N) if p != skip]
    pick = lambda v: [v[p] for p in rest]  # noqa: E731
    want, wcounts = Q.temporal(flat, pick(k["starts"]), pick(k["sizes"]), pick(k["group"]), pick(k["date"]), pick(k["offsets"]), 7, R.SND)
    want = R.bits_of(want)

    def check(**broken):
        out = torch.full((total,), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
        counts = torch.zeros((N, 4), dtype=torch.int32, device="cuda")
        _raw(planes, st, ss, T, h, out, counts, **broken)
        got, c = R.bits_of(out.cpu().numpy()), counts.cpu().numpy()
        assert (got[lo:hi] == POISON).all() and np.array_equal(got[:lo], want[:lo]) and np.array_equal(got[hi:], want[hi:]), broken
        assert c[skip].tolist() == [0, 0, 0, 0] and np.array_equal(c[rest], wcounts), broken

    for row0, col0 in ((10, 51), (23, 50), (-1, 50), (10, -1)):  # one column or one row beyond the lattice of 42 x 80, negative offsets
        place = T.place.copy()
        place[skip, 0], place[skip, 1] = row0, col0
        check(place=place)
    place = T.place.copy()
    place[skip, 2] = -1  # a negative date
    check(place=place)
    at = int(np.nonzero(T.members == skip)[0][0])
    for bad in (N, 2**31 - 1, -1):  # a member entry that names no plane
        members = T.members.copy()
        members[at] = bad
        check(members=members)
    # a tile table with extra tiles: the workgroups beyond a lattice's own tiles find nothing to do; a lattice that is not positive: its
    # group is skipped whole
    more = T.tile_ptr.copy()
    more[1:] += 5
    more[2:] += 3
    full, fcounts = R.expected(h, True, "linear")
    out = torch.full((total,), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
    counts = torch.zeros((N, 4), dtype=torch.int32, device="cuda")
    _raw(planes, st, ss, T, h, out, counts, tile_ptr=more)
    assert np.array_equal(R.bits_of(out.cpu().numpy()), full) and np.array_equal(counts.cpu().numpy(), fcounts)
    lattice = T.lattice.copy()
    lattice[1] = (0, 65)
    out = torch.full((total,), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
    counts = torch.zeros((N, 4), dtype=torch.int32, device="cuda")
    _raw(planes, st, ss, T, h, out, counts, lattice=lattice)
    got, first = R.bits_of(out.cpu().numpy()), int(st[4])
    assert np.array_equal(got[:first], full[:first]) and (got[first:] == POISON).all() and counts.cpu().numpy()[4:].sum() == 0
