"""Attention at tile and chunk seams (-m gpu): every attention kernel family at the token counts on both sides of its tile, workgroup and
chunk boundaries, on inputs that turn a tail fault into an error of tens of per cent (tests/attention_reference.py: a last key that holds
half of every row, scores near -10 that a zero-filled row would swamp, a last query that dominates dk and dv), against float64 on the
operands the kernel sees.  Bars: the project's (test_attention_fwd_bwd / test_attention_generic_head_dim), in plain mode widened only
where the float64 emulation of the kernels' two bf16 roundings says so (attention_reference.PLAIN_BARS); dq, dk and dv are judged each
against its own third.  Every check prints error and bar (``-s``).

Geometry.  attention2.hip (head_dim 64): 32-key tiles, 32 queries per wave, 7 waves = 224 queries per workgroup, 224-key chunks; plain bf16
runs the single-pass backward up to N = 224 and the two-pass one above.  attention_g.hip (head_dim 80, or 64 with IG_ATTN_GENERIC=1):
16-row tiles, 4 waves per workgroup in the register kernels (split mode) and 8 in the LDS kernels (plain), 272-row chunks.
"""
import functools
import os

import pytest
import torch

import attention_reference as AR

pytestmark = pytest.mark.gpu

from instageo_amd import ops  # noqa: E402
from instageo_amd.ops import BT  # noqa: E402

DEV = "cuda"
SPLITS = [False, True]
ROUTES = {"tuned": 64, "generic80": 80, "generic64": 64}  # route -> head_dim; generic64 = head_dim 64 forced onto attention_g.hip
TUNED_NS = (31, 32, 63, 64, 65, 192, 193, 223, 226, 447, 448, 449, 672, 673, 785)
GENERIC_NS = (15, 17, 64, 65, 128, 129, 271, 272, 273, 544, 545, 817)
GENERIC_ALL_KINDS_NS = (15, 65, 129, 273, 545)
FORCED_NS = (17, 129, 273)
DQKV = ("dq", "dk", "dv")


def bt(x, split):
    b = BT.from_float(x.to(DEV), split)
    return b, b.float().double().cpu()  # (device tensor, exact value the kernel sees)


class _Route:
    """IG_ATTN_GENERIC for the launches inside (the switch is read at every call)."""

    def __init__(self, route):
        self.value = "1" if route == "generic64" else None

    def __enter__(self):
        self.old = os.environ.pop("IG_ATTN_GENERIC", None)
        if self.value:
            os.environ["IG_ATTN_GENERIC"] = self.value

    def __exit__(self, *exc):
        os.environ.pop("IG_ATTN_GENERIC", None)
        if self.old is not None:
            os.environ["IG_ATTN_GENERIC"] = self.old


def launch(route, qkv, dout, B, N, H, split, lse=True, dbias=None):
    """One forward and one backward: (out, lse, dqkv, forward kernel, backward kernel)."""
    hd = ROUTES[route]
    out = BT.zeros((B, N, H * hd), split, DEV)
    lse_t = torch.zeros(B, H, N, device=DEV) if lse else None
    with _Route(route):
        ops.attention_fwd(qkv, out, lse_t, B, N, H, hd=hd)
        kf = ops.last_kernel()
        if dout is None:
            return out, lse_t, None, kf, None
        dqkv = BT.zeros((B, N, 3 * H * hd), split, DEV)
        delta = torch.zeros(B * H * N, device=DEV)
        ops.attention_bwd(qkv, out, dout, lse_t, delta, dqkv, B, N, H, hd=hd, dbias=dbias)
        kb = ops.last_kernel()
    return out, lse_t, dqkv, kf, kb


@functools.lru_cache(maxsize=2)
def run(route, kind, N, split, B=AR.B, H=AR.H):
    """The kernels' five outputs and the float64 reference on the same operands, both on the host: one launch set and one reference per
    case, shared by the checks of its five outputs (which run back to back).  Asserts the kernel names, so that the sweep cannot silently
    change route."""
    hd = ROUTES[route]
    x, dy = AR.operands(kind, N, hd, B, H)
    qkv, qr = bt(x, split)
    dout, dor = bt(dy, split)
    out, lse, dqkv, kf, kb = launch(route, qkv, dout, B, N, H, split)
    expect_kernels(route, N, split, kf, kb)
    g = dqkv.float().double().cpu().reshape(B, N, 3, H * hd)
    got = dict(out=out.float().double().cpu(), lse=lse.double().cpu(), dq=g[:, :, 0], dk=g[:, :, 1], dv=g[:, :, 2])
    return got, AR.reference(qr, dor, H, hd)


def check(route, kind, N, split, what, B=AR.B, H=AR.H):
    got, ref = run(route, kind, N, split, B, H)
    assert torch.isfinite(got[what]).all(), f"{what}: non-finite kernel output"
    err, bar = AR.rel_err(got[what], ref[what]), AR.bar(kind, ROUTES[route], what, split)
    print(f"SEAM {route} {kind} N {N} B {B} H {H} {'split' if split else 'plain'} {what}: err {err:.3e} bar {bar:.3e} ratio {err / bar:.3g}")
    assert err <= bar, f"{route} {kind} N {N} {'split' if split else 'plain'} {what}: relative max error {err:.3e} > bar {bar:.3e}"


def expect_kernels(route, N, split, kf, kb):
    if route == "tuned":
        assert kf.startswith("attn2_fwd_kernel"), kf
        if not split and N <= 224:
            assert kb == "attn2_bwd_fused_kernel", kb
        else:
            assert "attn2_bwd_dq_kernel" in kb and "attn2_bwd_dkv_kernel" in kb, kb
    else:  # plain bf16: the LDS-staged kernels; split: the register / L2 kernels
        assert kf.startswith("attng_fwd_lds_kernel" if not split else "attng_fwd_kernel"), kf
        assert kb.startswith("attng_bwd_dkv_lds_kernel" if not split else "attng_bwd_dkv_kernel<"), kb
        assert ("lds" in kf) == ("lds" in kb) == (not split), (kf, kb)


def _sweep():
    cases = [("tuned", kind, N) for N in TUNED_NS for kind in AR.KINDS]
    cases += [("generic80", kind, N) for N in GENERIC_NS for kind in AR.KINDS if kind == "random" or N in GENERIC_ALL_KINDS_NS]
    cases += [("generic64", "random", N) for N in FORCED_NS]
    return cases


@pytest.mark.parametrize("what", AR.OUTPUTS)
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("route,kind,N", _sweep())
def test_seam_sweep(route, kind, N, split, what):
    """Forward and backward at every seam, one output per test (the five of a case share one launch set).  No case needs a pin: the
    largest error is 0.64 of its bar (tuned, ``negative``, N = 193, split out)."""
    check(route, kind, N, split, what)


@pytest.mark.parametrize("what", AR.OUTPUTS)
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("route,B,H,N", [("tuned", 3, 12, 33), ("generic80", 3, 16, 17)])
def test_head_and_batch_indexing(route, B, H, N, split, what):
    """Grid y / z and the [3][H][hd] stride beyond the H = 3, B = 2 of every other case."""
    check(route, "random", N, split, what, B, H)


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("route,N", [("tuned", 193), ("tuned", 226), ("tuned", 449), ("generic80", 273)])
def test_qkv_bias_gradient(route, N, split):
    """dbias += column sums of dqkv over the tokens, fused into the tuned backward kernels (K third identically zero) and one ig_colsum
    pass over C = 3 H 80 columns behind the generic ones; the buffer starts at 0.5."""
    hd, B, H = ROUTES[route], AR.B, AR.H
    x, dy = AR.operands("random", N, hd)
    qkv, qr = bt(x, split)
    dout, dor = bt(dy, split)
    ref = AR.reference(qr, dor, H, hd)
    bref = torch.stack([ref[w] for w in DQKV], 2).reshape(B * N, 3 * H * hd).sum(0)
    dbias = torch.full((3 * H * hd,), 0.5, device=DEV)
    _, _, dqkv, _, _ = launch(route, qkv, dout, B, N, H, split, dbias=dbias)
    _, _, plain_dqkv, _, _ = launch(route, qkv, dout, B, N, H, split)
    assert torch.equal(dqkv.hi, plain_dqkv.hi), "dqkv must not depend on the bias-gradient request"
    got = (dbias - 0.5).double().cpu()
    err, bar = AR.rel_err(got, bref), AR.bar("random", hd, "dbias", split)
    kpart = got[H * hd : 2 * H * hd].abs().max().item() / bref.abs().max().item()
    kbar = AR.PROJECT_BARS["dk"][1 if split else 0]
    print(f"SEAM {route} N {N} {'split' if split else 'plain'} dbias: err {err:.3e} bar {bar:.3e}; K third {kpart:.3e} bound {kbar:.1e}")
    assert err <= bar, f"qkv bias gradient: relative max error {err:.3e} > bar {bar:.3e}"
    if route == "tuned":
        assert kpart <= kbar, f"K third of the qkv bias gradient should vanish, got {kpart:.3e} of the largest entry"


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("route,N", [("tuned", 226), ("generic80", 273), ("generic64", 273)])
def test_inference_form_without_lse(route, N, split):
    """lse = NULL, the documented inference form: the same out, bit for bit."""
    hd = ROUTES[route]
    qkv, _ = bt(AR.operands("random", N, hd)[0], split)
    with_lse = launch(route, qkv, None, AR.B, N, AR.H, split)
    without = launch(route, qkv, None, AR.B, N, AR.H, split, lse=False)
    assert with_lse[3] == without[3], (with_lse[3], without[3])
    assert torch.equal(with_lse[0].hi, without[0].hi)
    assert not split or torch.equal(with_lse[0].lo, without[0].lo)
    assert with_lse[0].hi.float().abs().max().item() > 0


# one ragged multi-chunk N per kernel family (the single-pass backward is one chunk by construction: a ragged one)
@pytest.mark.parametrize("route,N,split,family", [
    ("tuned", 449, False, "attn2_fwd_kernel<false>, attn2_bwd_dq_kernel + attn2_bwd_dkv_kernel"),
    ("tuned", 449, True, "attn2_fwd_kernel<true>, split two-pass backward"),
    ("tuned", 193, False, "attn2_bwd_fused_kernel"),
    ("generic80", 545, False, "attng_*_lds_kernel"),
    ("generic80", 545, True, "attng register kernels"),
])
def test_repeated_launches_are_bit_identical(route, N, split, family):
    """The screen every LDS-DMA GEMM has: fresh zeroed outputs, four more launches, out, lse and dqkv (hi and lo) identical each time.
    (dbias accumulates with float atomics and is not screened.)"""
    hd = ROUTES[route]
    x, dy = AR.operands("random", N, hd)
    qkv, _ = bt(x, split)
    dout, _ = bt(dy, split)
    first = launch(route, qkv, dout, AR.B, N, AR.H, split)
    expect_kernels(route, N, split, first[3], first[4])
    for i in range(4):
        again = launch(route, qkv, dout, AR.B, N, AR.H, split)
        assert again[3:] == first[3:]
        assert torch.equal(again[1], first[1]), f"{family}: lse differs on launch {i + 2}"
        for a, b, name in ((again[0], first[0], "out"), (again[2], first[2], "dqkv")):
            assert torch.equal(a.hi, b.hi), f"{family}: {name} differs on launch {i + 2}"
            assert not split or torch.equal(a.lo, b.lo), f"{family}: {name} (lo) differs on launch {i + 2}"
