"""Value-range parity tests (-m gpu): normalisation, softmax-family, attention, GELU and input-normalisation kernels on
offset, extreme and degenerate inputs, where fp32 formulas that are exact on centred data lose precision.

Every case compares the kernel with a float64 restatement of the op on the operands the kernel actually sees (bf16, bf16x2
or fp32, as in test_gpu_ops.py), and measures PyTorch's own fp32 implementation of the op (CPU, same operands) against the
same float64 reference.  One accuracy bar applies to every check:

    max |kernel - f64|  <=  min(cap, max(4 * max |torch fp32 - f64|, floor))

* ``floor`` is the rounding of the output: one bf16 ulp (2^-7), one bf16x2 ulp (2^-15) or two fp32 ulps (2^-22) of the
  largest reference magnitude; integer-coded sums add their quantum (the 2^-28 fixed point of the loss partials).
* ``cap`` is the tolerance that test_gpu_ops.py applies to the same output at the same precision, where it has one: the bar
  is never looser than the existing test.  Where fp32 arithmetic itself misses the cap on a case (torch's own error is above
  it: a row offset of 1e3 sigma rounds the stored fp32 mean), the cap cannot apply and the 4x rule stands alone.
* GELU has no fp32 counterpart in the same form: its bar is the documented erf_fast bound (1.5e-7 absolute on erf, common.h)
  carried through, per element, plus the output rounding.

No case widens the bar by hand.  Each check prints its error, the bar and the fp32 error (``-s`` shows the table).
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from instageo_amd import dataloader as DL  # noqa: E402
from instageo_amd import ops  # noqa: E402
from instageo_amd.ops import BT  # noqa: E402

DEV = "cuda"
SPLITS = [False, True]
FLOOR_BF16, FLOOR_SPLIT, FLOOR_F32 = 2.0**-7, 2.0**-15, 2.0**-22
EPS = 1e-5


def bt(x, split):
    b = BT.from_float(x.to(DEV), split)
    return b, b.float().double().cpu()  # (device tensor, exact value the kernel sees)


def out_floor(split):
    return FLOOR_SPLIT if split else FLOOR_BF16


def out_cap(split):  # test_gpu_ops.tol_out: the existing bound on a bf16 / bf16x2 output
    return 2e-5 if split else 6e-3


def check(got, ref, t32, floor, what, cap=None, quantum=0.0):
    """The module's bar: kernel error <= min(cap, max(4 x fp32 error, floor)) (floor and cap relative to max |ref|)."""
    got, ref, t32 = got.double().cpu(), ref.double().cpu(), t32.double().cpu()
    assert got.shape == ref.shape == t32.shape, (what, got.shape, ref.shape, t32.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite kernel output"
    scale = ref.abs().max().item()
    err = (got - ref).abs().max().item()
    terr = (t32 - ref).abs().max().item()
    bar = max(4.0 * terr, floor * scale) + quantum
    if cap is not None and terr <= cap * scale:
        bar = min(bar, cap * scale + quantum)
    print(f"VR {what}: err {err:.3e} bar {bar:.3e} torch32 {terr:.3e} scale {scale:.3e} ratio {err / max(bar, 1e-300):.3g}")
    assert err <= bar, f"{what}: max err {err:.3e} > bar {bar:.3e} (fp32 torch {terr:.3e}, scale {scale:.3e})"


# ---------------------------------------------------------------------------------------------------------------------------------
# BatchNorm statistics
# ---------------------------------------------------------------------------------------------------------------------------------
BN_CASES = ["r0", "r1", "r8", "r64", "r512", "const", "tiny", "relu"]


def bn_values(case, M, C, seed):
    """[M, C] activations of one value case: per-channel mean / std = r (rN), a constant channel set, std near sqrt(eps), or
    ReLU'd (non-negative, positive mean) channels."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(M, C, generator=g)
    sig = 0.5 + 1.5 * torch.rand(C, generator=g)
    sign = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    if case[1:].isdigit():
        return z * sig + float(case[1:]) * sig * sign
    if case == "const":
        return (3.0 * torch.randn(C, generator=g)).expand(M, C).contiguous()
    if case == "tiny":
        return z * 3e-3 + 0.05 * sign
    assert case == "relu"
    return torch.relu(z * sig + 0.3 * sig)


def bn_torch(x, g, b, rm, rv, dy):
    """native_batch_norm (training) + ReLU and its backward in the dtype of ``x``: out, mean, rstd, running stats, dx, dgamma, dbeta."""
    x, g, b = x.clone().requires_grad_(True), g.clone().requires_grad_(True), b.clone().requires_grad_(True)
    out, mean, rstd = torch.ops.aten.native_batch_norm(x, g, b, rm, rv, True, 0.1, EPS)
    y = torch.relu(out)
    gx, gg, gb = torch.autograd.grad((y * dy).sum(), [x, g, b])
    return dict(y=y.detach(), mean=mean, rstd=rstd, rm=rm, rv=rv, dx=gx, dgamma=gg, dbeta=gb,
                scale=(g * rstd).detach(), shift=(b - mean * g * rstd).detach())


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("M,C", [(20000, 48), (2500, 192)])
@pytest.mark.parametrize("case", BN_CASES)
def test_bn_relu_value_ranges(case, M, C, split, det):
    """bn_relu_fwd (training: statistics pass + finalize + running update + apply), bn_stats and bn_relu_bwd, atomic and
    deterministic reductions."""
    x, xr = bt(bn_values(case, M, C, seed=11), split)
    gam = 1 + 0.1 * torch.randn(C, generator=torch.Generator().manual_seed(12))
    bet = 0.1 * torch.randn(C, generator=torch.Generator().manual_seed(13))
    dy, dyr = bt(torch.randn(M, C, generator=torch.Generator().manual_seed(14)), split)
    ref = bn_torch(xr, gam.double(), bet.double(), torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64), dyr)
    t32 = bn_torch(xr.float(), gam, bet, torch.zeros(C), torch.ones(C), dyr.float())
    flat = torch.zeros(4 * C + 8, device=DEV)
    try:
        if det:
            ops.set_deterministic(flat)
        rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        y = BT.empty((M, C), split, DEV)
        scale, shift, mean, rstd = (torch.empty(C, device=DEV) for _ in range(4))
        sums = torch.empty(2 * C, dtype=torch.float64, device=DEV)
        ops.bn_relu_fwd(x, gam.to(DEV), bet.to(DEV), rm, rv, y, scale, shift, mean, rstd, sums, M, C, True, True)
        got = dict(y=y.float(), mean=mean, rstd=rstd, rm=rm, rv=rv, scale=scale, shift=shift)
        for k in ("mean", "rstd", "scale", "shift"):
            check(got[k], ref[k], t32[k], FLOOR_F32, f"bn {k}")
        check(rm, ref["rm"], t32["rm"], FLOOR_F32, "bn running mean", cap=1e-5)
        check(rv, ref["rv"], t32["rv"], FLOOR_F32, "bn running var", cap=1e-5)
        check(y.float(), ref["y"], t32["y"], out_floor(split), "bn fwd", cap=out_cap(split))
        # statistics only (the consumer applies them): the same numbers
        rm2, rv2 = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        sc2, sh2, mean2, rstd2 = (torch.empty(C, device=DEV) for _ in range(4))
        sums2 = torch.empty_like(sums)
        ops.bn_stats(x, gam.to(DEV), bet.to(DEV), rm2, rv2, sc2, sh2, mean2, rstd2, sums2, M, C, True)
        check(mean2, ref["mean"], t32["mean"], FLOOR_F32, "bn_stats mean")
        check(rstd2, ref["rstd"], t32["rstd"], FLOOR_F32, "bn_stats rstd")
        if det:  # ordered partial folds: bit-identical from run to run
            assert torch.equal(sums2, sums) and torch.equal(rstd2, rstd) and torch.equal(rv2, rv)
        dx = BT.empty((M, C), split, DEV)
        dgam, dbet = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        bsums = torch.empty(2 * C, dtype=torch.float64, device=DEV)
        ops.bn_relu_bwd(x, dy, scale, shift, mean, rstd, dx, dgam, dbet, bsums, M, C)
        check(dx.float(), ref["dx"], t32["dx"], out_floor(split), "bn dx", cap=out_cap(split))
        check(dgam, ref["dgamma"], t32["dgamma"], FLOOR_F32, "bn dgamma", cap=3e-5)
        check(dbet, ref["dbeta"], t32["dbeta"], FLOOR_F32, "bn dbeta", cap=3e-5)
    finally:
        ops.set_deterministic(None)


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("ncls,C", [(2, 48), (13, 144)])
@pytest.mark.parametrize("case", ["r8", "r64", "r512", "relu"])
def test_classifier_bn_tail_value_ranges(case, ncls, C, split, det):
    """The fused training tail (bn_stats -> classifier_bn_fwd / classifier_bn_bwd) on offset activations."""
    B, H, W = 2, 24, 20
    HW, M = H * W, B * H * W
    x, xr = bt(bn_values(case, M, C, seed=21), split)
    gen = torch.Generator().manual_seed(22)
    gam, bet = 1 + 0.1 * torch.randn(C, generator=gen), 0.1 * torch.randn(C, generator=gen)
    w, cb = torch.randn(ncls, C, generator=gen) * C**-0.5, torch.randn(ncls, generator=gen)
    dl = torch.randn(B, ncls, H, W, generator=gen)

    def tail(xv, dt):
        xv = xv.to(dt).clone().requires_grad_(True)
        g_, b_, w_, c_ = (t.to(dt).clone().requires_grad_(True) for t in (gam, bet, w, cb))
        out, mean, rstd = torch.ops.aten.native_batch_norm(xv, g_, b_, torch.zeros(C, dtype=dt), torch.ones(C, dtype=dt), True, 0.1, EPS)
        lg = (torch.relu(out).view(B, HW, C) @ w_.t() + c_).permute(0, 2, 1).reshape(B, ncls, H, W)
        grads = torch.autograd.grad((lg * dl.to(dt)).sum(), [xv, g_, b_, w_, c_])
        return (lg.detach(), mean, rstd) + tuple(grads)

    ref, t32 = tail(xr, torch.float64), tail(xr.float(), torch.float32)
    nw = ncls * C
    flat = torch.zeros(nw + ncls + 2 * C + 8, device=DEV)
    dw, db = flat[:nw].view(ncls, C), flat[nw : nw + ncls]
    dgam, dbet = flat[nw + ncls : nw + ncls + C], flat[nw + ncls + C : nw + ncls + 2 * C]
    try:
        if det:
            ops.set_deterministic(flat)
        rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        scale, shift, mean, rstd = (torch.empty(C, device=DEV) for _ in range(4))
        sums = torch.empty(2 * C, dtype=torch.float64, device=DEV)
        ops.bn_stats(x, gam.to(DEV), bet.to(DEV), rm, rv, scale, shift, mean, rstd, sums, M, C, True)
        logits = torch.empty(B, ncls, H, W, device=DEV)
        ops.classifier_bn_fwd(x, scale, shift, w.to(DEV), cb.to(DEV), logits, B, HW, C, ncls)
        check(mean, ref[1], t32[1], FLOOR_F32, "tail mean")
        check(rstd, ref[2], t32[2], FLOOR_F32, "tail rstd")
        check(logits, ref[0], t32[0], FLOOR_F32, "tail logits", cap=3e-5)
        dx = BT.empty((M, C), split, DEV)
        ops.classifier_bn_bwd(dl.to(DEV), x, scale, shift, mean, rstd, w.to(DEV), dx, dw, db, dgam, dbet, sums, None, B, HW, C, ncls)
        ops.det_fold(0, flat.numel())
        check(dx.float(), ref[3], t32[3], out_floor(split), "tail dx", cap=out_cap(split))
        for got, i, nm in ((dgam, 4, "dgamma"), (dbet, 5, "dbeta"), (dw, 6, "dw"), (db, 7, "db")):
            check(got, ref[i], t32[i], FLOOR_F32, f"tail {nm}", cap=3e-5)
    finally:
        ops.set_deterministic(None)


def conv_offset_operands(source, ratio, B, H, W, C, gen):
    """Input, weights and bias of a 3 x 3 convolution whose outputs sit ``ratio`` standard deviations (about 1.3) off zero.
    source "bias": centred input, the offset in the bias.  source "input": bias ~ 0 and a DC input (every channel = D + noise, as
    the non-negative features the decode head convolves); the centre tap carries the DC (its weights sum to ~6 per output channel)
    and the eight others sum to zero over the input channels, so the zero padding does not move the border pixels."""
    x = torch.randn(B, H, W, C, generator=gen)
    w = torch.randn(C, 9, C, generator=gen) * (9 * C) ** -0.5
    bias = 0.1 * torch.randn(C, generator=gen)
    if source == "bias":
        bias += ratio * torch.where(torch.rand(C, generator=gen) < 0.5, -1.0, 1.0)
    else:
        w -= w.mean(2, keepdim=True)
        w[:, 4, :] = 0.125 + 0.02 * torch.randn(C, C, generator=gen)
        x += ratio * 1.3 / 6.0
    return x, w, bias


# The split-precision kernel still centres its statistics on the bias (conv_direct.hip, launch_direct_split): an output mean that comes
# from the input is an open finding there.
_SPLIT_INPUT_OFFSET = pytest.mark.xfail(strict=True, reason="split direct conv: statistics centred on the bias, not on the data")


def _conv_params():
    return [pytest.param(*shape, source, ratio, marks=[_SPLIT_INPUT_OFFSET] if shape[-1] and source == "input" and ratio >= 8 else [])
            for shape in [(48, 3, 40, 40, False), (48, 3, 21, 37, True), (96, 2, 40, 40, False)] for source in ("bias", "input")
            for ratio in (0, 8, 64, 512)]


@pytest.mark.parametrize("C,B,H,W,split,source,ratio", _conv_params())
def test_conv3x3_fused_statistics_value_ranges(C, B, H, W, split, source, ratio):
    """conv3x3_fwd_stats on the shapes where the direct kernels fuse the BatchNorm statistics, with the output mean ``ratio`` output
    standard deviations off zero, carried by the bias or coming from the input; bn_finalize from those sums against the statistics of
    the stored tensor."""
    gen = torch.Generator().manual_seed(31 + ratio)
    x0, w0, bias = conv_offset_operands(source, ratio, B, H, W, C, gen)
    x, xr = bt(x0, split)
    w, wr = bt(w0, split)
    gam, bet = 1 + 0.1 * torch.randn(C, generator=gen), 0.1 * torch.randn(C, generator=gen)
    y = BT.empty((B, H, W, C), split, DEV)
    sums = torch.full((2 * C,), -1.0, dtype=torch.float64, device=DEV)
    assert ops.conv3x3_fwd_stats(x, w, bias.to(DEV), y, sums, B, H, W, C, C)
    M = B * H * W
    yd = y.float().double().cpu().reshape(M, C)  # the statistics are those of the STORED outputs
    if ratio:  # the case is what it says: the channel means sit about ``ratio`` standard deviations off zero
        r = (yd.mean(0).abs() / yd.std(0)).median().item()
        assert 0.5 * ratio < r < 2 * ratio, r
    check(sums[:C], yd.sum(0), yd.float().sum(0), FLOOR_F32, "conv sum", cap=2e-6)
    check(sums[C:], (yd * yd).sum(0), (yd.float() * yd.float()).sum(0), FLOOR_F32, "conv sum of squares", cap=2e-6)
    sums2 = torch.empty_like(sums)
    ops.conv3x3_fwd_stats(x, w, bias.to(DEV), y, sums2, B, H, W, C, C)
    assert torch.equal(sums, sums2)  # ordered partial sums: bit-identical from run to run
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    scale, shift, mean, rstd = (torch.empty(C, device=DEV) for _ in range(4))
    ops.bn_finalize(sums, gam.to(DEV), bet.to(DEV), rm, rv, scale, shift, mean, rstd, M, C, True)
    ref = torch.ops.aten.native_batch_norm(yd, gam.double(), bet.double(), rmd := torch.zeros(C, dtype=torch.float64),
                                           rvd := torch.ones(C, dtype=torch.float64), True, 0.1, EPS)
    t32 = torch.ops.aten.native_batch_norm(yd.float(), gam, bet, rm32 := torch.zeros(C), rv32 := torch.ones(C), True, 0.1, EPS)
    check(mean, ref[1], t32[1], FLOOR_F32, "conv bn mean")
    check(rstd, ref[2], t32[2], FLOOR_F32, "conv bn rstd")
    check(rm, rmd, rm32, FLOOR_F32, "conv bn running mean", cap=2e-6)
    check(rv, rvd, rv32, FLOOR_F32, "conv bn running var", cap=2e-6)
    check(shift, bet.double() - ref[1] * gam.double() * ref[2], bet - t32[1] * gam * t32[2], FLOOR_F32, "conv bn shift")


# ---------------------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------------------------------------
def ln_values(case, M, D, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(M, D, generator=g)
    if case == "dc":  # row DC offsets up to 1e3 sigma
        return z + 1e3 * (2 * torch.rand(M, 1, generator=g) - 1)
    if case == "const":
        return (5 * torch.randn(M, 1, generator=g)).expand(M, D).contiguous()
    if case == "tiny":
        return 1.0 + 3e-3 * z
    assert case == "big"
    return 1e4 * z + 3e4 * torch.randn(M, 1, generator=g)


def ln_torch(x, g, b, dy, dx0):
    x, g, b = x.clone().requires_grad_(True), g.clone().requires_grad_(True), b.clone().requires_grad_(True)
    out, mean, rstd = torch.ops.aten.native_layer_norm(x, (x.shape[-1],), g, b, EPS)
    gx, gg, gb = torch.autograd.grad((out * dy).sum(), [x, g, b])
    return dict(out=out.detach(), mean=mean.reshape(-1), rstd=rstd.reshape(-1), dx=dx0 + gx, dgamma=gg, dbeta=gb)


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("D", [256, 768, 1024, 1280, 320])  # the four IG_LNB_EXACT widths and the generic kernel
@pytest.mark.parametrize("case", ["dc", "const", "tiny", "big"])
def test_layernorm_value_ranges(case, D, split):
    M = 197 * 2 + 3
    x = ln_values(case, M, D, seed=41)
    gen = torch.Generator().manual_seed(42)
    gam, bet = 1 + 0.1 * torch.randn(D, generator=gen), 0.1 * torch.randn(D, generator=gen)
    dy, dyr = bt(torch.randn(M, D, generator=gen), split)
    dx0 = torch.randn(M, D, generator=gen)
    ref = ln_torch(x.double(), gam.double(), bet.double(), dyr, dx0.double())
    t32 = ln_torch(x, gam, bet, dyr.float(), dx0)
    out = BT.empty((M, D), split, DEV)
    mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    ops.layernorm_fwd(x.to(DEV), gam.to(DEV), bet.to(DEV), out, mean, rstd, M, D)
    check(out.float(), ref["out"], t32["out"], out_floor(split), "ln fwd", cap=out_cap(split))
    check(mean, ref["mean"], t32["mean"], FLOOR_F32, "ln mean", cap=1e-5)
    check(rstd, ref["rstd"], t32["rstd"], FLOOR_F32, "ln rstd")
    dx = dx0.clone().to(DEV)
    dxb = BT.empty((M, D), split, DEV)
    dgam, dbet, dcol = (torch.zeros(D, device=DEV) for _ in range(3))
    ops.layernorm_bwd(dy, x.to(DEV), mean, rstd, gam.to(DEV), dx, True, dxb, dgam, dbet, dcol, M, D)
    check(dx, ref["dx"], t32["dx"], FLOOR_F32, "ln dx", cap=2e-5)
    check(dxb.float(), ref["dx"], t32["dx"], out_floor(split), "ln dx bf16", cap=out_cap(split))
    check(dgam, ref["dgamma"], t32["dgamma"], FLOOR_F32, "ln dgamma", cap=2e-5)
    check(dbet, ref["dbeta"], t32["dbeta"], FLOOR_F32, "ln dbeta", cap=2e-5)


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("case", ["dc", "big"])
def test_layernorm_feature_layout_value_ranges(case, split):
    B, G, D, T = 2, 9, 64, 3
    ntok = 1 + T * G
    M = B * ntok
    x = ln_values(case, M, D, seed=43)
    gen = torch.Generator().manual_seed(44)
    gam, bet = 1 + 0.1 * torch.randn(D, generator=gen), 0.1 * torch.randn(D, generator=gen)
    dy, dyr = bt(torch.randn(B, G, D * T, generator=gen), split)

    def feat(xv, dt):
        xv = xv.to(dt).clone().requires_grad_(True)
        ln = F.layer_norm(xv, (D,), gam.to(dt), bet.to(dt), EPS).reshape(B, ntok, D)
        f = ln[:, 1:, :].permute(0, 2, 1).reshape(B, D * T, G).permute(0, 2, 1)
        (gx,) = torch.autograd.grad((f * dyr.to(dt)).sum(), xv)
        return f.detach(), gx

    ref, t32 = feat(x, torch.float64), feat(x, torch.float32)
    out = BT.zeros((B, G, D * T), split, DEV)
    mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    ops.layernorm_fwd(x.to(DEV), gam.to(DEV), bet.to(DEV), out, mean, rstd, M, D, feat_T=T, feat_G=G, ntok=ntok)
    check(out.float(), ref[0], t32[0], out_floor(split), "ln feature layout", cap=out_cap(split))
    dx = torch.zeros(M, D, device=DEV)
    ops.layernorm_bwd(dy, x.to(DEV), mean, rstd, gam.to(DEV), dx, False, None, None, None, None, M, D, feat_T=T, feat_G=G, ntok=ntok)
    check(dx, ref[1], t32[1], FLOOR_F32, "ln feature layout bwd", cap=2e-5)


# ---------------------------------------------------------------------------------------------------------------------------------
# Attention
# ---------------------------------------------------------------------------------------------------------------------------------
def attn_values(case, B, N, H, hd, seed):
    """qkv [B, N, 3 H hd] with scores q.k / sqrt(hd) reaching the 100s: peaked rows, or near-uniform rows on a large common offset
    (every key = one shared vector + small noise)."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, N, H, hd, generator=g)
    v = torch.randn(B, N, H, hd, generator=g)
    if case == "peaked":
        q, k = q * 6.0, torch.randn(B, N, H, hd, generator=g) * 6.0
    else:
        q = q * 3.0
        k = 40.0 * torch.randn(B, 1, H, hd, generator=g) + 0.05 * torch.randn(B, N, H, hd, generator=g)
    return torch.stack([q, k, v], 2).reshape(B, N, 3 * H * hd)


def attn_torch(qkv, B, N, H, hd, dout):
    qkv = qkv.clone().requires_grad_(True)
    q, k, v = qkv.reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    s = (q * hd**-0.5) @ k.transpose(-2, -1)
    out = (s.softmax(-1) @ v).transpose(1, 2).reshape(B, N, H * hd)
    (g,) = torch.autograd.grad((out * dout).sum(), qkv)
    return out.detach(), torch.logsumexp(s, -1).detach(), g


# Open findings, pinned as strict xfails, one output per test (a fix turns its cases into XPASS, which fails the run until the mark
# goes; the kernels are deterministic, so a thin margin does not flip).  Keys: (case, split, output[, hd, N]).
_BF16_DS = "bf16 dS breaks the zero row sum of dS: the common key component (|k| ~ 40 sqrt(hd)) leaks into dq, 2-4x dq's own scale"
_SPLIT_EXP = ("split attention loses ~|score| fp32 ulps in the exp argument of P (scores in the 100s): 1.05-17x the bf16x2 bar; the "
              "backward recomputes P the same way")
FINDINGS = {("offset", False, "dq"): _BF16_DS}
FINDINGS.update({(case, True, what): _SPLIT_EXP for case in ("peaked", "offset") for what in ("lse", "out", "dq", "dk")})
FINDINGS.update({("offset", True, "dv"): _SPLIT_EXP, ("peaked", True, "dv", 64, 197): _SPLIT_EXP, ("peaked", True, "dv", 80, 589): _SPLIT_EXP})


def _attn_params(whats):
    out = []
    for case in ("peaked", "offset"):
        for hd in (64, 80):
            for N in (197, 589):
                for split in SPLITS:
                    for what in whats:
                        if what == "out_no_offset" and case != "offset":
                            continue
                        reason = FINDINGS.get((case, split, what), FINDINGS.get((case, split, what, hd, N)))
                        marks = [pytest.mark.xfail(strict=True, reason=reason)] if reason else []
                        out.append(pytest.param(case, hd, N, split, what, marks=marks))
    return out


@pytest.mark.parametrize("case,hd,N,split,what", _attn_params(("lse", "out", "out_no_offset")))
def test_attention_fwd_value_ranges(case, hd, N, split, what):
    B, H = 1, 2
    if what == "out_no_offset":  # the common score offset must not move the output: the same keys without it
        k0 = attn_values(case, B, N, H, hd, seed=51).reshape(B, N, 3, H, hd)
        k0[:, :, 1] -= k0[:, :, 1].mean(1, keepdim=True)
        qkv, qr = bt(k0.reshape(B, N, 3 * H * hd), split)
    else:
        qkv, qr = bt(attn_values(case, B, N, H, hd, seed=51), split)
        s = ((qr.reshape(B, N, 3, H, hd)[:, :, 0] * hd**-0.5).transpose(1, 2) @ qr.reshape(B, N, 3, H, hd)[:, :, 1].permute(0, 2, 3, 1))
        assert s.abs().max().item() > 100.0  # the scores do reach the 100s
    dor = torch.zeros(B, N, H * hd, dtype=torch.float64)
    ref = attn_torch(qr, B, N, H, hd, dor)
    t32 = attn_torch(qr.float(), B, N, H, hd, dor.float())
    out = BT.empty((B, N, H * hd), split, DEV)
    lse = torch.empty(B, H, N, device=DEV)
    ops.attention_fwd(qkv, out, lse, B, N, H, hd=hd)
    if what == "lse":
        check(lse, ref[1], t32[1], FLOOR_F32, "attn lse", cap=1e-5 if split else 2e-3)
    else:
        check(out.float(), ref[0], t32[0], out_floor(split), f"attn {what}", cap=3e-5 if split else 1e-2)


@pytest.mark.parametrize("case,hd,N,split,what", _attn_params(("dq", "dk", "dv")))
def test_attention_bwd_value_ranges(case, hd, N, split, what):
    B, H = 1, 2
    qkv, qr = bt(attn_values(case, B, N, H, hd, seed=51), split)
    dout, dor = bt(torch.randn(B, N, H * hd, generator=torch.Generator().manual_seed(52)), split)
    ref = attn_torch(qr, B, N, H, hd, dor)
    t32 = attn_torch(qr.float(), B, N, H, hd, dor.float())
    out = BT.empty((B, N, H * hd), split, DEV)
    lse = torch.empty(B, H, N, device=DEV)
    ops.attention_fwd(qkv, out, lse, B, N, H, hd=hd)
    dqkv = BT.empty((B, N, 3 * H * hd), split, DEV)
    delta = torch.empty(B * H * N, device=DEV)
    ops.attention_bwd(qkv, out, dout, lse, delta, dqkv, B, N, H, hd=hd)
    j = ("dq", "dk", "dv").index(what)
    g, gr, g32 = dqkv.float().double().cpu().reshape(B, N, 3, H * hd), ref[2].reshape(B, N, 3, H * hd), t32[2].reshape(B, N, 3, H * hd)
    check(g[:, :, j], gr[:, :, j], g32[:, :, j], out_floor(split), f"attn {what}", cap=1e-4 if split else 2e-2)


# ---------------------------------------------------------------------------------------------------------------------------------
# GELU epilogue of the GEMM engines
# ---------------------------------------------------------------------------------------------------------------------------------
ERF_BOUND = 1.5e-7 + 2.0**-22  # A-S 7.1.26 plus the fp32 rounding of its evaluation (common.h erf_fast)


def gelu_check(got, ref, bound, split, what):
    """Per element: ``bound`` + the rounding of the stored output (half a bf16 ulp, 2^-8 relative; bf16x2: 2^-16); as a whole: no looser
    than test_gpu_ops.py on the same output (tol_out)."""
    got, ref = got.double().cpu(), ref.double()
    lim = bound + (2.0**-16 if split else 2.0**-8) * ref.abs() + 1e-30
    err = (got - ref).abs()
    worst = (err / lim).max().item()
    cap = out_cap(split) * ref.abs().max().item()
    print(f"VR {what}: worst err / bound {worst:.3g}, max err {err.max().item():.3e} (cap {cap:.3e})")
    assert worst <= 1.0, f"{what}: {int((err > lim).sum())} elements above the bound (worst ratio {worst:.3g})"
    assert err.max().item() <= cap, f"{what}: max err {err.max().item():.3e} > {cap:.3e}"


def exact_operands(rows, cols, step, gen):
    """Integers in [-8, 8] times ``step`` (a power of two): bf16 values whose products and sums are exact in fp32 here."""
    return torch.randint(-8, 9, (rows, cols), generator=gen).float() * step


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("route", ["default", "gemm4", "gemm8"])
def test_gelu_epilogue_value_ranges(route, split, monkeypatch):
    """linear_fwd act=1 (with and without the saved gelu') and linear_dgrad mode 1 with pre-activations spanning [-12, 12] and past.
    The operands are multiples of 2^-3 / 2^-4 and the bias of 2^-7, so every partial sum of the pre-activation (|sum| < 2^8) is exact
    in fp32 in any order: the only error left is the GELU epilogue's, and the bar is the erf_fast bound carried through."""
    if route == "gemm4":
        monkeypatch.setenv("IG_GEMM4", "2")
    elif route == "gemm8":
        monkeypatch.setenv("IG_GEMM8", "2")
    M, N, K = 1000, 512, 256
    gen = torch.Generator().manual_seed(61)
    x0, w0 = exact_operands(M, K, 2.0**-3, gen), exact_operands(N, K, 2.0**-4, gen)
    x, xr = bt(x0, split)
    w, wr = bt(w0, split)
    assert torch.equal(xr, x0.double()) and torch.equal(wr, w0.double())  # the kernel sees them unrounded
    b = torch.round(torch.linspace(-12.0, 12.0, N) * 128) / 128
    pre_ref = xr @ wr.t() + b.double()
    assert pre_ref.min().item() < -12 and pre_ref.max().item() > 12
    y = BT.empty((M, N), split, DEV)
    pre = BT.empty((M, N), split, DEV)
    ops.linear_fwd(x, w, b.to(DEV), y, M, N, K, act=1, pre=pre)
    rr = pre_ref.clone().requires_grad_(True)
    gel = F.gelu(rr)
    (dref,) = torch.autograd.grad(gel.sum(), rr)
    gbound = 0.5 * pre_ref.abs() * ERF_BOUND
    gelu_check(y.float(), gel.detach(), gbound, split, f"{route} gelu")
    # gelu' = Phi(x) + x phi(x): the erf bound on Phi, and phi = exp2(-x^2 log2(e) / 2) off by ~x^2 / 2 ulps of its argument
    xpdf = (pre_ref * torch.exp(-0.5 * pre_ref**2) * (2 * math.pi) ** -0.5).abs()
    gelu_check(pre.float(), dref, 0.5 * ERF_BOUND + xpdf * (pre_ref**2 * 2.0**-24 + 2.0**-22), split, f"{route} saved gelu'")
    y2 = BT.empty((M, N), split, DEV)
    ops.linear_fwd(x, w, b.to(DEV), y2, M, N, K, act=1)
    gelu_check(y2.float(), gel.detach(), gbound, split, f"{route} gelu (no save)")
    # dgrad mode 1: dx[M, K] = (dy[M, N] @ w[N, K]) * pre[M, K], pre = the saved gelu' of a [M, K] activation (exact operands again:
    # the product by the stored factor is the only rounding before the output's)
    pk = BT.empty((M, K), split, DEV)
    xk = BT.empty((M, K), split, DEV)
    wk, _ = bt(exact_operands(K, K, 2.0**-4, gen), split)
    bk = torch.round(torch.linspace(-12.0, 12.0, K) * 128) / 128
    ops.linear_fwd(x, wk, bk.to(DEV), xk, M, K, K, act=1, pre=pk)
    dy, dyr = bt(exact_operands(M, N, 2.0**-3, gen), split)
    dx = BT.empty((M, K), split, DEV)
    ops.linear_dgrad(dy, w, dx, M, N, K, pre=pk)
    pkr = pk.float().double().cpu()  # the factor the kernel multiplies by
    dref2 = (dyr @ wr) * pkr
    check(dx.float(), dref2, (dyr.float() @ wr.float()) * pkr.float(), out_floor(split), f"{route} dgrad gelu'", cap=out_cap(split))


# ---------------------------------------------------------------------------------------------------------------------------------
# Softmax family: cross-entropy, distillation, probabilities, AUC histograms, argmax, blended windows
# ---------------------------------------------------------------------------------------------------------------------------------
SCALES = [1.0, 30.0, 300.0, 3000.0]
MARGINS = [0.0, 1e-3, 10.0, 50.0]


def confident_logits(B, ncls, H, W, scale, margin, seed):
    """Logits of magnitude ``scale`` whose top class leads the runner-up by ``margin`` (margin 0: an exact tie for the maximum).
    Returns (logits f32, top class = first maximum)."""
    g = torch.Generator().manual_seed(seed)
    z = (2 * torch.rand(B, ncls, H, W, generator=g) - 1) * scale
    top = torch.randint(0, ncls, (B, H, W), generator=g)
    other = (top + torch.randint(1, ncls, (B, H, W), generator=g)) % ncls
    zmax = z.max(1).values
    z.scatter_(1, other[:, None], zmax[:, None])
    z.scatter_(1, top[:, None], (zmax + margin)[:, None])
    z = z.float()
    return z, z.double().argmax(1)


def labels_for(kind, top, ncls, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "top":
        lab = top.clone()
    else:
        lab = torch.randint(0, ncls, top.shape, generator=g)
    lab[torch.rand(top.shape, generator=g) < 0.1] = -1
    return lab


def loss_quantum(npix):  # the loss partial of each workgroup passes through a 2^-28 fixed point
    return 2.0**-28 * math.ceil(npix / 64)


@pytest.mark.parametrize("labels_kind", ["top", "mixed"])
@pytest.mark.parametrize("margin", MARGINS)
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("ncls", [2, 7, 13])
def test_ce_loss_value_ranges(ncls, scale, margin, labels_kind):
    B, H, W = 2, 24, 36
    z, top = confident_logits(B, ncls, H, W, scale, margin, seed=71)
    lab = labels_for(labels_kind, top, ncls, seed=72)
    cw = torch.rand(ncls, generator=torch.Generator().manual_seed(73)) + 0.5
    mask = lab.ne(-1)

    def ce(zz):
        zz = zz.clone().requires_grad_(True)
        s = F.cross_entropy(zz, lab, weight=cw.to(zz.dtype), ignore_index=-1, reduction="sum")
        (g,) = torch.autograd.grad(s, zz)
        return s.detach(), g

    ref, t32 = ce(z.double()), ce(z)
    stats = torch.zeros(2, dtype=torch.float64, device=DEV)
    dlog = torch.empty_like(z, device=DEV)
    preds = torch.empty(B, H, W, dtype=torch.int64, device=DEV)
    p8 = torch.empty(B, H, W, dtype=torch.int8, device=DEV)
    conf = torch.zeros(ncls, ncls, dtype=torch.int64, device=DEV)
    ops.ce_loss(z.to(DEV), lab.to(DEV), cw.to(DEV), -1, stats, dlog, preds, p8, conf)
    assert stats[1].item() == mask.sum().item()
    check(stats[:1], ref[0].reshape(1), t32[0].reshape(1), FLOOR_F32, "ce loss sum", quantum=loss_quantum(B * H * W))
    check(dlog, ref[1], t32[1], FLOOR_F32, "ce dlogits", cap=2e-5)
    assert torch.equal(preds.cpu(), top) and torch.equal(p8.cpu().long(), top), "argmax: first maximum, as torch.argmax"
    assert torch.equal(ops.argmax_i8(z.to(DEV)).cpu().long(), top)
    from oracle import prithvi_oracle as O

    assert np.array_equal(conf.cpu().numpy(), O.confusion_matrix(lab.numpy(), top.numpy(), ncls, -1))


@pytest.mark.parametrize("margin", MARGINS)
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("ncls", [2, 7, 13])
def test_kd_loss_value_ranges(ncls, scale, margin):
    B, H, W = 2, 24, 36
    s, top = confident_logits(B, ncls, H, W, scale, margin, seed=81)
    t = (s.double() + torch.randn(s.shape, generator=torch.Generator().manual_seed(82)) * max(1.0, 0.01 * scale)).float()
    lab = labels_for("top", top, ncls, seed=83)
    mask = lab.ne(-1)

    def kd(ss, tt):
        ss = ss.clone().requires_grad_(True)
        kl = F.kl_div(F.log_softmax(ss, 1), F.softmax(tt, 1), reduction="none").sum(1)[mask].sum()
        (g,) = torch.autograd.grad(kl, ss)
        return kl.detach(), g

    ref, t32 = kd(s.double(), t.double()), kd(s, t)
    kl = torch.zeros(1, dtype=torch.float64, device=DEV)
    dlog = torch.zeros_like(s, device=DEV)
    ops.kd_loss(s.to(DEV), t.to(DEV), lab.to(DEV), -1, kl, dlog)
    check(kl, ref[0].reshape(1), t32[0].reshape(1), FLOOR_F32, "kd sum")
    check(dlog, ref[1], t32[1], FLOOR_F32, "kd dlogits")


@pytest.mark.parametrize("margin", MARGINS)
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("ncls", [2, 7, 13])
def test_softmax_prob_auc_argmax_value_ranges(ncls, scale, margin):
    from oracle import prithvi_oracle as O

    B, H, W = 2, 24, 36
    z, top = confident_logits(B, ncls, H, W, scale, margin, seed=91)
    p64, p32 = torch.softmax(z.double(), 1), torch.softmax(z, 1)
    for cls in (0, ncls - 1):
        check(ops.softmax_prob(z.to(DEV), cls), p64[:, cls], p32[:, cls], FLOOR_F32, f"softmax prob class {cls}", cap=1e-6)
    assert torch.equal(ops.argmax_i8(z.to(DEV)).cpu().long(), top), "argmax: first maximum, as torch.argmax"
    lab = labels_for("mixed", top, ncls, seed=92)
    nbins = 64
    hist = torch.zeros(2, ncls, nbins, dtype=torch.int64, device=DEV)
    ops.auc_update(z.to(DEV), lab.to(DEV), -1, hist, nbins)
    keep = lab.reshape(-1).ne(-1)
    probs = p64.permute(0, 2, 3, 1).reshape(-1, ncls)[keep]
    pos, neg = O.auc_histograms(lab.reshape(-1)[keep].numpy(), probs.numpy(), ncls, nbins)
    # a probability within the fp32 error bar of a bin edge may land in the neighbour bin: count those, nothing else may differ
    perr = max(4 * (p32 - p64).abs().max().item(), FLOOR_F32)
    xb = probs * (nbins - 1)
    near = int(((xb - xb.round()).abs() <= perr * (nbins - 1)).sum())
    diff = int(np.abs(hist[0].cpu().numpy() - pos).sum() + np.abs(hist[1].cpu().numpy() - neg).sum())
    print(f"VR auc: {diff} bin moves, {near} probabilities near an edge")
    assert diff <= 2 * near
    assert int(hist.sum()) == int(keep.sum()) * ncls


@pytest.mark.parametrize("margin", MARGINS)
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("ncls", [2, 7, 13])
def test_window_blend_value_ranges(ncls, scale, margin):
    """Blended windows on confident logits: the canvas against float64, and the class map the first maximum of the blend (an exact
    tie of the logits in every window blends to an exact tie)."""
    H, W, crop, stride = 70, 90, 32, 24
    tops, lefts = DL.window_grid(H, W, crop, stride, cover_edges=True)
    n = len(tops) * len(lefts)
    z, _ = confident_logits(n, ncls, crop, crop, scale, margin, seed=101)
    if margin == 0.0:  # classes 0 and 1 tie everywhere, above the others
        zt = z.max(1).values + scale
        z[:, 0], z[:, 1] = zt, zt
    wvec = ops.blend_weights(crop, "gaussian")
    td = torch.tensor(tops, dtype=torch.int32, device=DEV)
    ld = torch.tensor(lefts, dtype=torch.int32, device=DEV)
    acc, ws = torch.zeros((ncls, H, W), device=DEV), torch.zeros((H, W), device=DEV)
    ops.window_blend_accumulate(z.to(DEV), td, ld, 0, wvec.to(DEV), acc, ws, H)

    def host(dt):
        a, s = torch.zeros((ncls, H, W), dtype=dt), torch.zeros((H, W), dtype=dt)
        w2 = wvec.to(dt)[:, None] * wvec.to(dt)[None, :]
        for i in range(n):
            t, l = tops[i // len(lefts)], lefts[i % len(lefts)]
            a[:, t : t + crop, l : l + crop] += w2 * torch.softmax(z[i].to(dt), 0)
            s[t : t + crop, l : l + crop] += w2
        return a, s

    (a64, s64), (a32, s32) = host(torch.float64), host(torch.float32)
    check(acc, a64, a32, FLOOR_F32, "blend canvas", cap=1e-5)
    cmap, prob = ops.window_blend_finalize(acc, ws, probabilities=True)
    check(prob, a64 / s64, a32 / s32, FLOOR_F32, "blend probabilities")
    p = a64 / s64
    if margin == 0.0:
        assert bool((cmap.cpu() == 0).all()), "exact ties: the first maximum"
    else:
        top2 = p.topk(2, dim=0).values
        sure = (top2[0] - top2[1]) > 8 * max((a32 / s32 - p).abs().max().item(), FLOOR_F32)
        assert torch.equal(cmap.cpu().long()[sure], p.argmax(0)[sure])


# ---------------------------------------------------------------------------------------------------------------------------------
# Input normalisation
# ---------------------------------------------------------------------------------------------------------------------------------
MEAN = [0.14245495, 0.13921481, 0.12434631, 0.31420089, 0.20743526, 0.12046503]
STD = [0.04036231, 0.04186983, 0.05267646, 0.0822221, 0.06834774, 0.05294205]


def extreme_raw(shape, dtype, seed):
    """int16 extremes (-32768, 32767), NODATA -9999 and 0 among ordinary values; float32 adds values up to 1e7."""
    g = torch.Generator().manual_seed(seed)
    raw = torch.randint(0, 10000, shape, generator=g)
    pick = torch.randint(0, 6, shape, generator=g)
    specials = torch.tensor([-32768, 32767, -9999, 0, 1, -1])
    raw = torch.where(torch.rand(shape, generator=g) < 0.3, specials[pick], raw)
    if dtype == torch.int16:
        return raw.to(torch.int16)
    big = torch.where(torch.rand(shape, generator=g) < 0.5, 1.0, -1.0) * 10.0 ** torch.randint(4, 8, shape, generator=g).float()
    return torch.where(torch.rand(shape, generator=g) < 0.2, big, raw.float()).float()


def norm_refs(raw, mult, T):
    """(f64, fp32) normalisation of (..., T*C, H, W) -> (..., C, T, H, W): (x * mult - mean_c) / std_c."""
    C = len(MEAN)
    outs = []
    for dt in (torch.float64, torch.float32):
        x = raw.to(torch.float64) * (mult if mult is not None else 1.0)
        x = x.to(dt)
        sh = x.shape
        x = x.reshape(*sh[:-3], T, C, sh[-2], sh[-1])
        m = torch.tensor(MEAN, dtype=dt).view(C, 1, 1)
        s = torch.tensor(STD, dtype=dt).view(C, 1, 1)
        outs.append(((x - m) / s).transpose(-4, -3).contiguous())
    return outs


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("dtype", [torch.int16, torch.float32])
def test_input_normalisation_value_ranges(dtype, T):
    B, C, H, W = 2, len(MEAN), 40, 48
    mult = 1e-4 if dtype == torch.int16 else None
    raw = extreme_raw((B, T * C, H, W), dtype, seed=111 + T)
    m, s = torch.tensor(MEAN, device=DEV), torch.tensor(STD, device=DEV)
    out = ops.normalize_chips(raw.to(DEV), m, s, T, constant_multiplier=mult)
    r64, r32 = norm_refs(raw, mult, T)
    check(out, r64, r32, FLOOR_F32, "normalize_chips")
    im = 32
    params = torch.tensor([[0, 0, 0, 0], [5, 9, 1, 1]], dtype=torch.int32)
    out2, _ = ops.crop_flip_normalize(raw.to(DEV), params.to(DEV), m, s, T, im, mult)
    for b in range(B):
        top, left, hf, vf = params[b].tolist()
        sl = (slice(None), slice(None), slice(top, top + im), slice(left, left + im))
        c64, c32 = r64[b][sl], r32[b][sl]
        dims = ([-1] if hf else []) + ([-2] if vf else [])
        if dims:
            c64, c32 = c64.flip(dims), c32.flip(dims)
        check(out2[b], c64, c32, FLOOR_F32, f"crop_flip_normalize chip {b}")
    origins = torch.tensor([[0, 0], [H - im, W - im], [3, 7]], dtype=torch.int32)
    out3, _ = ops.normalize_windows(raw[0].to(DEV), origins.to(DEV), m, s, T, im, mult)
    for i, (t, l) in enumerate(origins.tolist()):
        sl = (slice(None), slice(None), slice(t, t + im), slice(l, l + im))
        check(out3[i], r64[0][sl], r32[0][sl], FLOOR_F32, f"normalize_windows window {i}")
