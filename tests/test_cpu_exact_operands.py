"""CPU checks of what tests/test_gpu_exact_parity.py stands on: the torch split reference equals an independent numpy bit-twiddling
round-to-nearest-even, the operand generators are exact (bf16 numbers, hi / lo that the reference split reproduces), and the exactness budget
(sum of |term| + |bias| + |residual| + |initial buffer| in units of the smallest term < 2^24) holds for every parametrised shape."""
import numpy as np
import pytest
import torch

import test_gpu_exact_parity as E

BF16 = torch.bfloat16


def np_rne_bf16(bits):
    """fp32 bit patterns (uint32) -> bf16 bit patterns (uint16), round to nearest even on the integer; NaNs are quieted."""
    b = bits.astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    nan = ((bits & 0x7F800000) == 0x7F800000) & ((bits & 0x007FFFFF) != 0)
    r[nan] = ((bits[nan] >> 16) | 0x40).astype(np.uint16)
    return r


def np_split(bits):
    hi = np_rne_bf16(bits)
    x = bits.view(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        res = (x - (hi.astype(np.uint32) << 16).view(np.float32)).astype(np.float32)  # exact: both are fp32 numbers within a bf16 ulp
    return hi, np_rne_bf16(res.view(np.uint32)), res


@pytest.mark.parametrize("vector", ["special", "subnormal"])
def test_torch_split_reference_equals_numpy_rne(vector):
    bits = E.special_fp32_bits() if vector == "special" else E.subnormal_fp32_bits()
    x = E.f32_from_bits(bits)
    assert np.array_equal(x.numpy().view(np.uint32), bits), "the bit patterns did not survive the trip into torch"
    hi, lo = E.split_ref(x)
    nhi, nlo, res = np_split(bits)
    fin = np.isfinite((nhi.astype(np.uint32) << 16).view(np.float32)) & np.isfinite(res)
    assert fin.sum() > 0.95 * bits.size
    assert np.array_equal(E.bits16(hi).numpy().view(np.uint16)[fin], nhi[fin]), "hi"
    assert np.array_equal(E.bits16(lo).numpy().view(np.uint16)[fin], nlo[fin]), "lo"
    # the residual hi + lo leaves is below 2^-16 of the value (two 8-bit roundings)
    m = E.merged_ref(hi, lo).double().numpy()[fin]
    xv = x.double().numpy()[fin]
    big = np.abs(xv) >= 2.0**-100
    assert (np.abs(m - xv)[big] <= np.abs(xv)[big] * 2.0**-16).all()


def test_special_vector_holds_what_the_issue_lists():
    bits = E.special_fp32_bits()
    sub = E.subnormal_fp32_bits()
    assert bits.size + 0 >= 65536 - 254 + 3000 and ((sub & 0x7F800000) == 0).all() and ((sub & 0x007FFFFF) != 0).all()
    assert ((bits & 0x7F800000) != 0).sum() + ((bits & 0x7FFFFFFF) == 0).sum() == bits.size, "a subnormal in the main vector"
    for v in (0x7F7FFFFF, 0x7F7F7FFF, 0x00800000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x80000000):
        assert (bits == v).any(), hex(v)
    for low in (0x7FFF, 0x8000, 0x8001, 0x0001, 0xFFFF):
        sel = bits[(bits & 0xFFFF) == low]
        assert sel.size >= 400 and ((sel >> 16) & 1).min() == 0 and ((sel >> 16) & 1).max() == 1 and (sel >> 31).min() == 0 and (sel >> 31).max() == 1
    # values whose lo is itself a tie: the residual has exactly nine significant bits with the last one set
    x = E.f32_from_bits(bits)
    hi, lo = E.split_ref(x)
    res = (x - hi.float())
    ok = torch.isfinite(res) & (res != 0)
    rb = res[ok].view(torch.int32) & 0x007FFFFF
    ties = ((rb & 0xFFFF) == 0x8000).sum().item()  # the 16 mantissa bits below the 7 kept ones: exactly one half
    assert ties >= 500, ties
    assert E.finite_split_values().numel() > 60000


def test_merge_pairs_are_not_split_outputs():
    hi, lo = E.merge_pairs()
    h, l = hi.float(), lo.float()
    assert torch.isfinite(h + l).all()
    s = (h + l)
    assert ((s == 0) | (s.abs() >= 2.0**-126)).all(), "a subnormal sum"
    assert ((h * l) < 0).sum() > 5000 and (l.abs() > h.abs() * 2.0**-8).sum() > 5000  # opposite signs; lo beyond half an ulp of hi


def _check_operand(pair, split):
    hi, lo = pair
    assert torch.equal(hi.to(BF16).double(), hi)
    if not split:
        assert lo is None
        return
    assert torch.equal(lo.to(BF16).double(), lo) and (hi != 0).all()
    v = (hi + lo).float()
    assert torch.equal(v.double(), hi + lo)
    rh, rl = E.split_ref(v)
    assert torch.equal(rh.double(), hi) and torch.equal(rl.double(), lo), "the reference split does not reproduce (hi, lo)"


@pytest.mark.parametrize("split", [False, True])
def test_generators_are_exact(split):
    for amp in (8, 4, 2, 1):
        for role in ("x", "w"):
            p = E.gen_operand((64, 96), 3, split, amp, role)
            _check_operand(p, split)
            step = (E.X_HI if role == "x" else E.W_HI)
            assert p[0].abs().max().item() == amp * step and torch.equal((p[0] / step).round(), p[0] / step)
    g = E.gen_grid((1000,), 5)
    assert torch.equal((g / E.U_PLAIN).round(), g / E.U_PLAIN) and g.abs().max().item() <= 4.0
    c = E.patch_grad_prep_case(9, 17, 12)
    assert torch.equal(c["dx"].float().double(), c["dx"])


def _terms_are_unit_multiples(acc, split):
    q = acc / E.units(split)
    assert torch.equal(q.round(), q)


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("route,M,N,K", E.LINEAR_FWD_CASES + E.LINEAR_SEAM_CASES)
def test_budget_linear(route, M, N, K, split):
    c = E.linear_case(M, N, K, split, bias=True, resid=True)
    E.assert_budget(c["mag"], split, "linear")
    _check_operand(c["x"], split), _check_operand(c["w"], split)
    _terms_are_unit_multiples(c["acc"], split)
    assert torch.equal(c["acc"].float().double(), c["acc"])


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("M,N,K", E.DGRAD_CASES + [c[1:4] for c in E.DGRAD_WT_CASES])
def test_budget_dgrad(M, N, K, split):
    c = E.dgrad_case(M, N, K, split)
    E.assert_budget(c["mag"], split, "dgrad")
    assert c["cs_exact"] or (split and M * N > 2**13), "column sums: exact for every plain case and the small split ones"
    if c["cs_exact"]:
        E.assert_budget(c["cs_mag"], split, "dgrad column sums")
        _terms_are_unit_multiples(c["cs"], split)
        assert torch.equal(c["cs"].float().double(), c["cs"])


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("M,N,K", E.WGRAD_CASES)
def test_budget_wgrad(M, N, K, split):
    c = E.wgrad_case(M, N, K, split, launches=2)
    E.assert_budget(c["mag"] + c["mag"] - c["dw0"].abs(), split, "wgrad, two launches")
    _terms_are_unit_multiples(c["acc"], split)


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("M,shapes", E.WGRAD_GROUP_CASES + [E.WGRAD_GROUP_FALLBACK])
def test_budget_wgrad_group(M, shapes, split):
    for gi, (N, K) in enumerate(shapes):
        c = E.wgrad_case(M, N, K, split, seed=7 * gi)
        E.assert_budget(c["mag"], split, "grouped wgrad")
        _check_operand(c["dy"], split), _check_operand(c["x"], split)


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("T,B,tpf,D,K", E.PATCH_EMBED_CASES)
def test_budget_patch_embed(T, B, tpf, D, K, split):
    c = E.patch_embed_case(T, B, tpf, D, K, split)
    E.assert_budget(c["mag"], split, "patch_embed")
    assert torch.equal(c["acc"].float().double(), c["acc"])


@pytest.mark.parametrize("case,split", E.CONV_PARAMS)
def test_budget_conv(case, split):
    name, kind, env, B, H, W, Cin, Cout, ks, _, routes = case
    c = E.conv_case(kind, B, H, W, Cin, Cout, split, ks)
    budgets = E.conv_budgets(c, name)
    assert max(budgets) < E.LIMIT
    for k in ("x", "w", "dy"):
        _check_operand(c[k], split)
    for k in ("y", "dx", "dw", "db"):
        _terms_are_unit_multiples(c[k], split)
        assert torch.equal(c[k].float().double(), c[k]), k
    assert c["y"].shape == (B, c["Ho"], c["Wo"], Cout) and c["dx"].shape == (B, H, W, Cin) and c["dw"].shape == (Cout, ks * ks, Cin)


def test_conv_reference_layout_matches_autograd():
    """The stored weight layout Wc[Cout][tap][Cin] and the three-term references against plain float64 autograd on hi + lo operands: the two
    differ by exactly the lo x lo products the engines omit."""
    import torch.nn.functional as F

    for kind, (B, H, W, Cin, Cout) in (("conv", (2, 5, 7, 8, 16)), ("convT", (1, 3, 4, 16, 8))):
        c = E.conv_case(kind, B, H, W, Cin, Cout, True)
        x = E._nchw(c["x"][0] + c["x"][1]).requires_grad_(True)
        w = E._w_torch(kind, c["w"][0] + c["w"][1], Cout, Cin, 3).requires_grad_(True)
        y = E._conv(kind, x, w)
        ll = E._conv(kind, E._nchw(c["x"][1]), E._w_torch(kind, c["w"][1], Cout, Cin, 3))
        assert torch.equal(E._nhwc((y - ll).detach() + c["bias"].view(1, -1, 1, 1)), c["y"])
        plain = E.conv_case(kind, B, H, W, Cin, Cout, False)
        xp = E._nchw(plain["x"][0]).requires_grad_(True)
        wp = E._w_torch(kind, plain["w"][0], Cout, Cin, 3).requires_grad_(True)
        gx, gw = torch.autograd.grad((E._conv(kind, xp, wp) * E._nchw(plain["dy"][0])).sum(), [xp, wp])
        assert torch.equal(E._nhwc(gx), plain["dx"])
        assert torch.equal(plain["dw0"] + E._w_stored(kind, gw, Cout, Cin, 3), plain["dw"])


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("M,C", E.COLSUM_CASES)
def test_budget_colsum(M, C, split):
    c = E.colsum_case(M, C, split)
    E.colsum_budget(c)
    assert torch.equal(c["acc"].float().double(), c["acc"])


@pytest.mark.parametrize("B,ntok,D", E.PGP_CASES)
def test_budget_patch_grad_prep(B, ntok, D):
    c = E.patch_grad_prep_case(B, ntok, D)
    E.patch_grad_prep_budget(c)
    assert torch.equal(c["dcls"].float().double(), c["dcls"]) and torch.equal(c["dbias"].float().double(), c["dbias"])
    if ntok > 1:  # the values exercise both halves: some lo parts are non-zero, some hi roundings are exact ties
        hi, lo = E.split_ref(c["rows"].float())
        assert (lo.float() != 0).any()


def test_pick_amp_follows_the_budget_rule():
    assert E.pick_amp(3072, False) == 8 and 64 * 3072 + 2048 < 2**24  # the plain generator at K <= 3072
    assert E.pick_amp(192, True) == 8 and E.pick_amp(768, True) == 4 and E.pick_amp(3072, True) == 2
