"""No launch reads what an earlier launch left in scratch (-m gpu).

The library keeps nine grow-only scratch buffers per (device, stream) (``IgScratchSlot``, csrc/common.h; ``ig_scratch2``, csrc/runtime.hip):
a fresh one is zero-filled, a grown one is never cleared again.  Every slot gets the same three steps on the current stream:

* probe: the entry point at a small shape that uses the slot, against the float64 restatement and the bar of the op's own test;
* dirty: the slot's users at a shape whose scratch footprint contains the probe's, on inputs that make every cell they write
  absorbing (NaN, or d2 = 0 for ``split_nearest``); the dirty launch's own output must show the poison;
* probe again, twice, into re-poisoned outputs: finite, inside the same bar, and bit-equal to the first probe.

Every probe also proves that it took the scratch path: by the kernel and grid the library noted (``ops.last_kernel`` / ``ops.last_grid``),
by the engine switch of the op's own test, or -- where the entry point has one path only -- by the dirty launch's poisoned output, which
reaches it through the scratch cells alone.  tests/scratch_cases.py lists the tests per slot.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import split_reference as SR  # noqa: E402
import test_gpu_calibration as TC  # noqa: E402
import test_gpu_seg_loss as TS  # noqa: E402
from instageo_amd import ops, split  # noqa: E402
from instageo_amd.ops import BT  # noqa: E402
from test_gpu_ops import bt, close, nhwc, rnd, tol_out  # noqa: E402

DEV = "cuda"
NAN = float("nan")
SPLITS = [False, True]


def cdiv(a, b):
    return -(-a // b)


def carry(probe, dirties, bits=True):
    """probe -> every dirty launch -> probe, probe.  ``probe()`` fills its outputs with a sentinel, runs, checks path and float64 bar
    and returns the output tensors; ``bits``: the repeats must equal the first run bit for bit."""
    first = [t.clone() for t in probe()]
    for d in dirties:
        d()
    for rep in range(2):
        again = probe()
        for i, (a, b) in enumerate(zip(first, again)):
            assert torch.isfinite(b.double()).all(), f"repeat {rep}, output {i}: not finite after the dirty launches"
            if bits:
                assert torch.equal(a, b), f"repeat {rep}, output {i}: differs from the first probe after the dirty launches"


def nan_bt(shape, split):
    return BT.from_float(torch.full(shape, NAN, device=DEV), split)


# ---------------------------------------------------------------------------------------------------------------- IG_SLOT_SPLITK
def splitk_v1_plan(rows, cols, tokens, Z=1):
    """(output tiles, K splits) of the 128-column engine behind the weight gradients (launch_gemm in csrc/gemm.hip, atomic epilogue)."""
    best = None
    for cand, eff in ((128, 100), (96, 80), (48, 50)):
        padded = cdiv(rows, cand) * cand * 100 // eff
        if best is None or padded < best[0]:
            best = (padded, cand)
    tiles = cdiv(rows, best[1]) * cdiv(cols, 128)
    nk = cdiv(tokens, 64)
    ks = max(1, min(512 // (tiles * Z), nk // 8))
    return tiles, cdiv(nk, cdiv(nk, ks))


def took_splitk(rows, cols, tokens, Z=1):
    tiles, ks = splitk_v1_plan(rows, cols, tokens, Z)
    k = ops.last_kernel()
    assert k.startswith("gemm_kernel<") and "EpAtomic" in k, k
    assert ks > 1 and ops.last_grid() == tiles * ks, (k, ops.last_grid(), tiles, ks)
    return ks


def linear_wgrad_probe(M, N, K, split, want_ks):
    dy, dyr = bt(rnd(M, N, seed=5), split)
    x, xr = bt(rnd(M, K, seed=7), split)
    ref = dyr.t() @ xr

    def probe():
        dw = torch.zeros(N, K, device=DEV)
        ops.linear_wgrad(dy, x, dw, M, N, K)
        assert took_splitk(N, K, M) == want_ks
        close(dw, ref, 3e-5 if split else 2e-5, what=f"wgrad {M}x{N}x{K}")
        return [dw]

    return probe


def linear_wgrad_dirty(M, N, K, split):
    dy, x = nan_bt((M, N), split), BT.from_float(torch.ones(M, K, device=DEV), split)

    def dirty():
        dw = torch.zeros(N, K, device=DEV)
        ops.linear_wgrad(dy, x, dw, M, N, K)
        took_splitk(N, K, M)
        assert torch.isnan(dw).all()

    return dirty


@pytest.mark.parametrize("split", SPLITS)
def test_splitk_linear_wgrad(split, monkeypatch):
    """ig_linear_wgrad on the split-K slabs of gemm.hip (IG_WGRAD8=0 keeps the 8-phase engine away): tile grids that overhang both
    dimensions of dW.  The suite's shapes with the token count raised to the smallest that splits (16 K-steps of 64)."""
    monkeypatch.setenv("IG_WGRAD8", "0")
    # small -> large -> small, two slabs -> four
    for M, N, K in [(1061, 768, 256), (1000, 64, 72), (1300, 256, 192)]:
        carry(linear_wgrad_probe(M, N, K, split, 2), [linear_wgrad_dirty(2100, 768, 256, split)])
    # large -> small -> large
    carry(linear_wgrad_probe(2100, 768, 256, split, 4), [linear_wgrad_dirty(1000, 64, 72, split), linear_wgrad_dirty(1300, 256, 192, split)])
    # the same dW, another split count: ks = 2 after ks = 4 and back
    carry(linear_wgrad_probe(1000, 64, 72, split, 2), [linear_wgrad_dirty(2100, 64, 72, split)])
    carry(linear_wgrad_probe(2100, 64, 72, split, 4), [linear_wgrad_dirty(1000, 64, 72, split)])


def conv_wgrad_case(kind, B, H, W, Cin, Cout, split):
    """kind "conv": Conv2d 3 x 3 pad 1; "convT": ConvTranspose2d k3 s2 p1 op1 (the tap slices Z = 9 of the split-K launch)."""
    x, xr = bt(nhwc(rnd(B, Cin, H, W, seed=30)), split)
    xin = xr.permute(0, 3, 1, 2).clone()
    if kind == "conv":
        wv = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
        ref = F.conv2d(xin, wv, None, padding=1)
        s = 1
    else:
        wv = torch.zeros(Cin, Cout, 3, 3, dtype=torch.float64, requires_grad=True)
        ref = F.conv_transpose2d(xin, wv, None, stride=2, padding=1, output_padding=1)
        s = 2
    dy, dyr = bt(nhwc(rnd(B, Cout, s * H, s * W, seed=33)), split)
    (gw,) = torch.autograd.grad((ref * dyr.permute(0, 3, 1, 2)).sum(), [wv])
    gw = (gw.permute(0, 2, 3, 1) if kind == "conv" else gw.permute(1, 2, 3, 0)).reshape(Cout, 9, Cin)
    fn = ops.conv3x3_wgrad if kind == "conv" else ops.convT_wgrad
    plan = (Cout, 9 * Cin, B * H * W, 1) if kind == "conv" else (Cout, Cin, B * H * W, 9)

    def probe():
        dw = torch.zeros(Cout, 9, Cin, device=DEV)
        fn(dy, x, dw, B, H, W, Cin, Cout)
        took_splitk(*plan)
        close(dw, gw, 3e-5, what=f"{kind} wgrad {Cin}->{Cout}")
        return [dw]

    def dirty():
        dw = torch.zeros(Cout, 9, Cin, device=DEV)
        fn(nan_bt(tuple(dy.shape), split), x, dw, B, H, W, Cin, Cout)
        took_splitk(*plan)
        assert torch.isnan(dw).all()

    return probe, dirty


@pytest.mark.parametrize("split", SPLITS)
def test_splitk_conv_wgrads(split, monkeypatch):
    """The gathered weight gradients on the same slabs: Conv2d 8 -> 136 (two 96-row tiles over 136 rows) and the ConvTranspose 48 -> 24,
    whose nine taps are the z slices of one launch; dirtied by a larger Conv2d gradient with four splits and by each other."""
    for k, v in (("IG_WGRAD8", "0"), ("IG_CONV_DIRECT", "0")):
        monkeypatch.setenv(k, v)
    conv_p, conv_d = conv_wgrad_case("conv", 2, 23, 25, 8, 136, split)
    convT_p, convT_d = conv_wgrad_case("convT", 2, 23, 23, 48, 24, split)
    _, big_d = conv_wgrad_case("conv", 2, 32, 32, 48, 96, split)
    carry(conv_p, [big_d, convT_d])
    carry(convT_p, [big_d, conv_d])


# ----------------------------------------------------------------------------------------------------------- IG_SLOT_WGRAD_SLABS
@pytest.mark.parametrize("arm", ["0", "1"])
@pytest.mark.parametrize("split", SPLITS)
def test_wgrad_slabs_grouped(split, arm, monkeypatch):
    """ig_linear_wgrad_group (gemm8w.hip: the 8-wave kernel with IG_GEMM4=0, the 4-wave one with 1), accumulate and overwrite: two small
    GEMMs over 197 tokens (a ragged second K-tile) after a group with more tiles, more token splits and NaN in every slab."""
    monkeypatch.setenv("IG_GEMM4", arm)
    want = f"gemm4w_kernel<{'true' if split else 'false'}>" if arm == "1" else f"gemm8w_kernel<{2 if split else 1},0,4,2>"
    M, shapes = 197, [(256, 256), (768, 256)]
    items, refs = [], []
    for gi, (N, K) in enumerate(shapes):
        dy, dyr = bt(rnd(M, N, seed=11 + gi), split)
        x, xr = bt(rnd(M, K, seed=31 + gi), split)
        items.append((dy, x, None, N, K))
        refs.append(dyr.t() @ xr)
    Md, dshapes = 1000, [(768, 768), (1024, 256), (256, 512)]
    ditems = [(nan_bt((Md, N), split), BT.from_float(torch.ones(Md, K, device=DEV), split), torch.zeros(N, K, device=DEV), N, K) for N, K in dshapes]
    grids = {}

    def probe_of(overwrite):
        def probe():
            its = [(dy, x, torch.full((N, K), NAN if overwrite else 0.5, device=DEV), N, K) for dy, x, _, N, K in items]
            ops.linear_wgrad_group(its, M, overwrite=overwrite)
            assert ops.last_kernel() == want, ops.last_kernel()
            grids["probe"] = ops.last_grid()
            for it, ref in zip(its, refs):
                close(it[2] - (0.0 if overwrite else 0.5), ref, 3e-5 if split else 2e-5, what=f"grouped wgrad {it[3]}x{it[4]}")
            return [it[2] for it in its]

        return probe

    def dirty():
        for it in ditems:
            it[2].zero_()
        ops.linear_wgrad_group(ditems, Md, overwrite=False)
        assert ops.last_kernel() == want, ops.last_kernel()
        grids["dirty"] = ops.last_grid()
        assert all(torch.isnan(it[2]).all() for it in ditems)

    for overwrite in (False, True):
        carry(probe_of(overwrite), [dirty])
    assert grids["dirty"] > grids["probe"] > 4, grids  # more workgroups than tiles: the tokens are split, more so in the dirty launch


# ----------------------------------------------------------------------------------------------------------- IG_SLOT_BN_PARTIALS
def bn_case(M, C, split):
    x, xr = bt(rnd(M, C, seed=34) * 1.5 + 0.3, split)
    g, b = 1 + 0.1 * rnd(C, seed=35), 0.1 * rnd(C, seed=36)
    dy, dyr = bt(rnd(M, C, seed=38), split)
    xd = xr.clone().requires_grad_(True)
    gd, bd = g.double().requires_grad_(True), b.double().requires_grad_(True)
    ref = F.relu(F.batch_norm(xd, torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64), gd, bd, True, 0.1, 1e-5))
    gx, gg, gb = torch.autograd.grad((ref * dyr).sum(), [xd, gd, bd])
    return dict(M=M, C=C, split=split, x=x, g=g.to(DEV), b=b.to(DEV), dy=dy, ref=ref.detach(), gx=gx, gg=gg, gb=gb)


def bn_fwd(c, x=None):
    M, C = c["M"], c["C"]
    y = BT.from_float(torch.full((M, C), -7.0, device=DEV), c["split"])
    st = [torch.full((C,), -7.0, device=DEV) for _ in range(4)]
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    sums = torch.full((2 * C,), -7.0, dtype=torch.float64, device=DEV)
    ops.bn_relu_fwd(x or c["x"], c["g"], c["b"], rm, rv, y, *st, sums, M, C, True, True)
    return y, st, sums


def bn_fwd_probe(c):
    def probe():
        y, st, sums = bn_fwd(c)
        close(y.float(), c["ref"], tol_out(c["split"]), what="bn fwd")
        c["stats"] = st
        return [y.hi, sums] + st

    return probe


def bn_bwd_probe(c, flat):
    M, C = c["M"], c["C"]

    def probe():
        flat.zero_()
        dgam, dbet = flat[:C], flat[C : 2 * C]
        dx = BT.from_float(torch.full((M, C), -7.0, device=DEV), c["split"])
        sums = torch.full((2 * C,), -7.0, dtype=torch.float64, device=DEV)
        ops.bn_relu_bwd(c["x"], c["dy"], *c["stats"], dx, dgam, dbet, sums, M, C)
        ops.det_fold(0, flat.numel())
        close(dx.float(), c["gx"], tol_out(c["split"]), what="bn dx")
        close(dgam, c["gg"], 3e-5, what="bn dgamma")
        close(dbet, c["gb"], 3e-5, what="bn dbeta")
        return [dx.hi, sums, dgam.clone(), dbet.clone()]

    return probe


def bn_dirty(M, C, backward):
    """NaN in every row and column: every partial of every workgroup is NaN (double in the forward, float in the backward)."""
    x = nan_bt((M, C), False)
    ones = torch.ones(C, device=DEV)
    live = BT.from_float(torch.ones(M, C, device=DEV), False) if backward else None  # x * scale + shift > 0: the ReLU lets the NaN of dy through

    def dirty():
        if backward:
            dx, dg, db = BT.empty((M, C), False, DEV), torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
            sums = torch.zeros(2 * C, dtype=torch.float64, device=DEV)
            ops.bn_relu_bwd(live, x, ones, ones, ones, ones, dx, dg, db, sums, M, C)
            assert torch.isnan(sums).all() and torch.isnan(dg).all()
        else:
            st = [torch.zeros(C, device=DEV) for _ in range(4)]
            sums = torch.zeros(2 * C, dtype=torch.float64, device=DEV)
            ops.bn_stats(x, ones, ones, torch.zeros(C, device=DEV), torch.ones(C, device=DEV), *st, sums, M, C, True)
            assert torch.isnan(sums).all() and torch.isnan(st[2]).all()

    return dirty


def conv_stats_case(B, H, W, poison):
    C = 48
    x, xr = bt(torch.full((B, H, W, C), NAN) if poison else rnd(B, H, W, C, seed=61), False)
    w, wr = bt(rnd(C, 9, C, seed=62, scale=(9 * C) ** -0.5), False)
    bias = rnd(C, seed=63)
    ref = None if poison else F.conv2d(xr.permute(0, 3, 1, 2), wr.view(C, 3, 3, C).permute(0, 3, 1, 2), bias.double(), padding=1).permute(0, 2, 3, 1)

    def run():
        y = BT.from_float(torch.full((B, H, W, C), -7.0, device=DEV), False)
        sums = torch.full((2 * C,), -1.0, dtype=torch.float64, device=DEV)
        assert ops.conv3x3_fwd_stats(x, w, bias.to(DEV), y, sums, B, H, W, C, C), "the fused statistics did not run"
        assert ops.last_kernel() == "conv3x3_direct_kernel<48,0>", ops.last_kernel()
        if poison:
            assert torch.isnan(sums).all()
            return []
        close(y.float(), ref, tol_out(False), what="conv fwd")
        yd = y.float().double().cpu().reshape(-1, C)
        close(sums[:C], yd.sum(0), 2e-6, what="sum")
        close(sums[C:], (yd * yd).sum(0), 2e-6, what="sum of squares")
        return [y.hi, sums]

    return run


def cls_bn_bwd_probe(B, HW, C, ncls, split, flat):
    M = B * HW
    H, W = HW // 28, 28
    x, xr = bt(rnd(M, C, seed=51) * 1.5 + 0.3, split)
    g, b = 1 + 0.1 * rnd(C, seed=52), 0.1 * rnd(C, seed=53)
    w, cb = rnd(ncls, C, seed=54, scale=C**-0.5), rnd(ncls, seed=55)
    xd = xr.clone().requires_grad_(True)
    gd, bd = g.double().requires_grad_(True), b.double().requires_grad_(True)
    wd, cbd = w.double().requires_grad_(True), cb.double().requires_grad_(True)
    act = F.relu(F.batch_norm(xd, torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64), gd, bd, True, 0.1, 1e-5))
    ref = (act.view(B, HW, C) @ wd.t() + cbd).permute(0, 2, 1).reshape(B, ncls, H, W)
    dl = rnd(B, ncls, H, W, seed=57)
    gx, gg, gb, gw, gcb = torch.autograd.grad((ref * dl.double()).sum(), [xd, gd, bd, wd, cbd])
    nw = ncls * C
    dld, wdev = dl.to(DEV), w.to(DEV)

    def probe():
        flat.zero_()
        dw, db, dgam, dbet = flat[:nw].view(ncls, C), flat[nw : nw + ncls], flat[nw + ncls : nw + ncls + C], flat[nw + ncls + C : nw + ncls + 2 * C]
        st = [torch.full((C,), -7.0, device=DEV) for _ in range(4)]
        sums = torch.full((2 * C,), -7.0, dtype=torch.float64, device=DEV)
        ops.bn_stats(x, g.to(DEV), b.to(DEV), torch.zeros(C, device=DEV), torch.ones(C, device=DEV), *st, sums, M, C, True)
        dx = BT.from_float(torch.full((M, C), -7.0, device=DEV), split)
        ops.classifier_bn_bwd(dld, x, *st, wdev, dx, dw, db, dgam, dbet, sums, None, B, HW, C, ncls)
        ops.det_fold(0, flat.numel())
        close(dx.float(), gx, tol_out(split), what="fused dx")
        close(dw, gw, 3e-5, what="fused dw")
        close(db, gcb, 3e-5, what="fused db")
        close(dgam, gg, 3e-5, what="fused dgamma")
        close(dbet, gb, 3e-5, what="fused dbeta")
        return [dx.hi, flat.clone(), sums]

    return probe


@pytest.mark.parametrize("split", SPLITS)
def test_bn_partials_double_float_and_conv_statistics(split):
    """One slot, four users, two element types: bn_relu_fwd (double partials) -> bn_relu_bwd (float) -> conv3x3_fwd_stats at 48 channels
    (double) -> classifier_bn_bwd (float), in the deterministic mode that sends the first, second and fourth through the slot.  Every
    probe follows NaN partials of the other width, written by more workgroups over more channels."""
    flat = torch.zeros(4096, device=DEV)
    try:
        ops.set_deterministic(flat)
        assert ops.deterministic()
        big_fwd = [bn_dirty(70000, 192, False), bn_dirty(70000, 24, False)]
        big_bwd = [bn_dirty(70000, 192, True), bn_dirty(70000, 24, True)]
        for M, C in [(769, 48), (2 * 28 * 28, 192)]:
            c = bn_case(M, C, split)
            carry(bn_fwd_probe(c), big_bwd + big_fwd)  # double partials over what was float and double NaN
            carry(bn_bwd_probe(c, flat), big_fwd)      # float partials over double NaN
        conv_dirty = conv_stats_case(30, 48, 48, True)
        carry(conv_stats_case(2, 23, 37, False), big_bwd)                                # double partials over float NaN
        carry(cls_bn_bwd_probe(2, 28 * 28, 48, 2, split, flat), [conv_dirty] + big_fwd)  # float partials over double NaN
        carry(cls_bn_bwd_probe(1, 28 * 28, 48, 6, split, flat), big_bwd)
    finally:
        ops.set_deterministic(None)


# --------------------------------------------------------------------------------------------------------- IG_SLOT_CONV8_WEIGHTS
def conv8_case(kind, B, H, W, Cin, Cout, split, poison=False):
    """kind: "fwd" / "dgrad" of Conv2d 3 x 3 pad 1, "convT" = ConvTranspose2d forward.  poison: NaN weights."""
    tw = kind == "convT"
    wt = torch.full((Cout, 9, Cin), NAN) if poison else rnd(Cout, 9, Cin, seed=27, scale=(9 * Cin) ** -0.5)
    w, wr = bt(wt, split)
    bias = rnd(Cout, seed=28)
    if kind == "dgrad":
        src, sr = bt(nhwc(rnd(B, Cout, H, W, seed=29)), split)
        out_shape, ref = (B, H, W, Cin), None
        if not poison:
            xin = torch.zeros(B, Cin, H, W, dtype=torch.float64, requires_grad=True)
            r = F.conv2d(xin, wr.reshape(Cout, 3, 3, Cin).permute(0, 3, 1, 2), None, padding=1)
            (ref,) = torch.autograd.grad((r * sr.permute(0, 3, 1, 2)).sum(), [xin])
    else:
        src, sr = bt(nhwc(rnd(B, Cin, H, W, seed=26)), split)
        out_shape, ref = ((B, 2 * H, 2 * W, Cout) if tw else (B, H, W, Cout)), None
        if not poison and tw:
            ref = F.conv_transpose2d(sr.permute(0, 3, 1, 2), wr.reshape(Cout, 3, 3, Cin).permute(3, 0, 1, 2), bias.double(), stride=2, padding=1, output_padding=1)
        elif not poison:
            ref = F.conv2d(sr.permute(0, 3, 1, 2), wr.reshape(Cout, 3, 3, Cin).permute(0, 3, 1, 2), bias.double(), padding=1)

    def run():
        y = BT.from_float(torch.full(out_shape, -7.0, device=DEV), split)
        if kind == "dgrad":
            ops.conv3x3_dgrad(src, w, y, B, H, W, Cin, Cout)
        elif tw:
            ops.convT_fwd(src, w, bias.to(DEV), y, B, H, W, Cin, Cout)
        else:
            ops.conv3x3_fwd(src, w, bias.to(DEV), y, B, H, W, Cin, Cout)
        assert ops.last_kernel().startswith(("conv8_kernel", "conv4_kernel")), ops.last_kernel()
        if poison:
            assert torch.isnan(y.float()).all()
            return []
        close(y.float(), nhwc(ref), tol_out(split), what=f"conv8 {kind} {Cin}->{Cout}")
        return [y.hi] + ([y.lo] if split else [])

    return run


@pytest.mark.parametrize("split", SPLITS)
def test_conv8_packed_weights_and_table(split, monkeypatch):
    """conv8.hip packs the weights (rows padded to whole 128-wide K-tiles) and their gather table into the slot on every call.  Channel
    counts that leave K-padding, after NaN weights with a larger Cin x Cout in the plain form and in the split form (hi + lo: the table
    sits at another offset of the buffer)."""
    monkeypatch.setenv("IG_CONV8", "2")
    monkeypatch.setenv("IG_CONV_DIRECT", "0")
    dirties = [conv8_case("fwd", 1, 8, 9, 256, 256, False, True), conv8_case("fwd", 1, 8, 9, 192, 320, True, True),
               conv8_case("dgrad", 1, 8, 9, 256, 256, False, True), conv8_case("convT", 1, 5, 6, 256, 256, split, True)]
    for kind, B, H, Cin, Cout in [("fwd", 3, 7, 8, 136), ("fwd", 1, 24, 144, 72), ("dgrad", 1, 24, 144, 72), ("fwd", 1, 12, 128, 256),
                                  ("dgrad", 2, 9, 128, 256), ("convT", 1, 7, 128, 256), ("convT", 1, 10, 144, 72)]:
        carry(conv8_case(kind, B, H, H + 3, Cin, Cout, split), dirties)


# ----------------------------------------------------------------------------------------------------------- IG_SLOT_LOSS_TOTALS
def loss_case(kind, B, H, W, poison=False, ignored=False):
    """kind "kd": ig_kd_loss (one total per workgroup), "mse": ig_mse_loss with the metric sums (ten), "kdmse": ig_kd_mse_loss (one).
    Bars: those of tests/test_gpu_pipeline.py (per-pixel loss to 1e-5 for the KL term, 1e-6 relative for the squared errors)."""
    g = torch.Generator(device=DEV).manual_seed(17 + B * H)
    ncls = 5
    if kind == "kd":
        s = torch.randn(B, ncls, H, W, device=DEV, generator=g)
        t = torch.randn(B, ncls, H, W, device=DEV, generator=g) * 1.5
        lab = torch.randint(-1, ncls, (B, H, W), device=DEV, generator=g)
        if ignored:
            lab.fill_(-1)
        if poison:
            s.fill_(NAN)
        valid = lab != -1
        n = int(valid.sum())
        pt, lpt, lps = F.softmax(t.double(), 1), F.log_softmax(t.double(), 1), F.log_softmax(s.double(), 1)
        ref = ((pt * (lpt - lps)).sum(1) * valid).sum().item() if not poison and n else 0.0

        def run():
            kl = torch.zeros(1, dtype=torch.float64, device=DEV)
            ops.kd_loss(s, t, lab, -1, kl, None)
            if poison:
                assert torch.isnan(kl).all()
            elif ignored:
                assert kl.item() == 0.0
            else:
                assert abs(kl.item() / n - ref / n) < 1e-5, (kl.item() / n, ref / n)
            return [kl]

        return run
    pred = torch.rand(B, 1, H, W, device=DEV, generator=g) * 2.0
    teach = torch.rand(B, 1, H, W, device=DEV, generator=g) * 2.0
    lab = torch.rand(B, H, W, device=DEV, generator=g) * 3.0
    lab[torch.rand(B, H, W, device=DEV, generator=g) < 0.2] = -1.0
    if ignored:
        lab.fill_(-1.0)
    if poison:
        pred.fill_(NAN)
    valid = lab != -1.0
    n = int(valid.sum())
    other = lab if kind == "mse" else teach[:, 0]
    ref = (((pred[:, 0].double() - other.double()) ** 2) * valid).sum().item() / max(n, 1) if not poison else 0.0

    def run():
        tot = torch.zeros(2 if kind == "mse" else 1, dtype=torch.float64, device=DEV)
        ms = torch.zeros(9, dtype=torch.float64, device=DEV)
        if kind == "mse":
            ops.mse_loss(pred, lab, -1.0, False, tot, None, ms, 0.05, 0.15, True)
        else:
            ops.kd_mse_loss(pred, teach, lab, -1.0, False, tot)
        if poison:
            assert torch.isnan(tot[0])
        elif ignored:
            assert tot[0].item() == 0.0 and not ms.any()
        else:
            assert kind != "mse" or int(tot[1].item()) == n
            assert abs(tot[0].item() / n - ref) < 1e-6 * max(1.0, ref), (tot[0].item() / n, ref)
        return [tot, ms]

    return run


def test_loss_totals_ticket_shared_by_three_entry_points():
    """ordered_grid_totals (pixel_logits.h): 1024 x 16 partials and one ticket shared by ig_kd_loss, ig_mse_loss and ig_kd_mse_loss.  The
    three alternate, on one workgroup (256 pixels) and on the 1024-workgroup cap (6 x 224 x 224 pixels), after NaN predictions on the
    cap's grid and an all-ignored launch.  The entry points have no other path: a NaN total can only come out of the partials."""
    small, big = (1, 16, 16), (6, 224, 224)
    kinds = ["kd", "mse", "kdmse"]
    for i, kind in enumerate(kinds):
        a, b = kinds[(i + 1) % 3], kinds[(i + 2) % 3]
        for shape, other in ((small, big), (big, small)):
            dirties = [loss_case(a, *big, poison=True), loss_case(b, *other, poison=True), loss_case(a, *other, ignored=True),
                       loss_case(b, *small, poison=True)]
            carry(loss_case(kind, *shape), dirties)


# ---------------------------------------------------------------------------------------- IG_SLOT_CE_ACC and IG_SLOT_REGION_SUMS
def seg_probe(shape, gamma, lam, with_dlogits, entry="seg"):
    """ig_ce_loss / ig_seg_loss against the float64 formulas and the bars of tests/test_gpu_seg_loss.py."""
    B, K, H, W = shape
    z, z64, lab, cw = TS.make_case(shape, "randn3", TS.label_variants(K)[0])
    ab, s = (0.3, 0.7), 1.0
    ref = TS.formulas(z64, lab, cw.double(), gamma, lam, ab[0], ab[1], s)
    t32 = TS.formulas(z64.float(), lab, cw, gamma, lam, ab[0], ab[1], s)
    q = TS.loss_quantum(B * H * W)

    def probe():
        if entry == "ce":
            stats = torch.zeros(2, dtype=torch.float64, device=DEV)
            dl = torch.full_like(z, NAN) if with_dlogits else None
            ops.ce_loss(z, lab, cw, TS.IGN, stats, dl)
            got = dict(stats=stats, dlogits=dl, parts=None)
        else:
            got = TS.run_kernel(z, lab, cw, gamma, lam, ab, s, want_dlogits=with_dlogits)
        tag = f"{entry} g{gamma:g} l{lam:g}"
        assert got["stats"][1].item() == ref[1].item()
        TS.check(got["stats"][:1], ref[0].reshape(1), t32[0].reshape(1), f"stats {tag}", "randn3", quantum=q)
        out = [got["stats"]]
        if got["parts"] is not None:
            TS.check(got["parts"], ref[2], t32[2], f"parts {tag}", "randn3", quantum=q)
            out.append(got["parts"])
        if with_dlogits:
            TS.check(got["dlogits"], ref[3], t32[3], f"dlogits {tag}", "randn3")
            out.append(got["dlogits"])
        return out

    return probe


def seg_dirty(lam, mode):
    """(8, 16, 64, 64) logits with NaN, +-Inf and 3e38 spread over every workgroup's pixels: the poison word rises and the totals leave the
    fixed-point sum.  mode "stats": the totals must not be finite; "ignored": an all-ignored batch; "nostats": stats = None."""
    B, K, H, W = 8, 16, 64, 64
    g = torch.Generator().manual_seed(9)
    z = torch.randn(B, K, H, W, generator=g) * 3
    z[:, 0::4, :, 0::4] = NAN
    z[:, 1::4, :, 1::4] = float("inf")
    z[:, 2::4, :, 2::4] = float("-inf")
    z[:, 3::4, :, 3::4] = 3e38
    z = z.to(DEV)
    lab = torch.randint(0, K, (B, H, W), generator=g).to(DEV)
    if mode == "ignored":
        lab.fill_(TS.IGN)

    def dirty():
        stats = None if mode == "nostats" else torch.zeros(2, dtype=torch.float64, device=DEV)
        dl = torch.empty_like(z)
        if lam is None:
            ops.ce_loss(z, lab, None, TS.IGN, stats, dl)
        else:
            ops.seg_loss(z, lab, None, TS.IGN, stats, dl, focal_gamma=2.0, region_weight=lam)
        if mode == "stats":
            assert not torch.isfinite(stats[0]), stats
            assert stats[1].item() == B * H * W
        elif mode == "ignored":
            assert stats[1].item() == 0

    return dirty


def test_ce_accumulators_and_region_sums():
    """ce_loss_kernel's (loss, count) accumulators, arrival counter and poison word, and the class sums and coefficients of the region
    term: ig_ce_loss and ig_seg_loss with and without the region term and with and without dlogits, after poisoned launches on 512
    workgroups, an all-ignored batch and a launch without stats.  Both entry points have one path (stats given -> the accumulators;
    region_weight > 0 -> the class sums): the dirty totals, NaN, reach their output through those cells alone."""
    dirties = [seg_dirty(None, "stats"), seg_dirty(1.0, "stats"), seg_dirty(1.0, "ignored"), seg_dirty(None, "ignored"), seg_dirty(1.0, "nostats"),
               seg_dirty(None, "nostats")]
    for shape in [(3, 2, 8, 12), (2, 13, 7, 9)]:
        carry(seg_probe(shape, 0.0, 0.0, True, entry="ce"), dirties)
        carry(seg_probe(shape, 0.0, 0.0, False, entry="ce"), dirties[:2])
        carry(seg_probe(shape, 2.0, 1.0, True), dirties)
        carry(seg_probe(shape, 0.0, 0.5, False), dirties[:3])
        carry(seg_probe(shape, 2.0, 0.0, True), dirties[1:3])


# ------------------------------------------------------------------------------------------------------------- IG_SLOT_CALIB_NLL
def test_calib_nll_partials():
    """ig_calib_nll_grid: 1 and 7 temperatures (the 4- and 8-column kernels) after 32 temperatures of NaN logits on 128 workgroups.  One
    path: the sums reach nll through the workgroup partials of the slot."""
    zd = torch.full((8, 5, 64, 64), NAN, device=DEV)
    labd = torch.zeros(8, 64, 64, dtype=torch.int64, device=DEV)

    def dirty():
        nll, count = TC.run_nll(zd, labd, TC.betas_of(32))
        assert torch.isnan(nll).all() and count.item() == labd.numel()

    for shape in [(3, 2, 8, 12), (2, 13, 7, 9)]:
        z, z64, lab = TC.make_case(shape, "randn3")
        for K in (1, 7):
            betas = TC.betas_of(K)
            ref, n_ref = TC.nll_torch(z64, lab, betas)
            t32, _ = TC.nll_torch(z64.float(), lab, betas)

            def probe():
                nll = torch.zeros(K, dtype=torch.float64, device=DEV)
                count = torch.zeros(1, dtype=torch.int64, device=DEV)
                TC.run_nll(z, lab, betas, nll, count)
                assert count.item() == n_ref > 0
                for k in range(K):
                    err = abs(nll[k].item() - ref[k].item())
                    bar = max(4.0 * abs(t32[k].double().item() - ref[k].item()), TC.FLOOR_F32 * abs(ref[k].item()))
                    assert err <= bar, f"K={K} k={k}: err {err:.3e} > bar {bar:.3e}"
                return [nll, count]

            carry(probe, [dirty])


# --------------------------------------------------------------------------------------------------------- IG_SLOT_SPLIT_NEAREST
def test_split_nearest_candidates():
    """ig_split_nearest: the per-range (d2, idx) candidates.  Dirty: 40 ranges x 3000 rows, every row of a present in every range of b,
    so every candidate cell holds d2 = 0 -- the value that wins any merge.  Probe: 5 and 3 ranges, fewer rows, against the numpy twin."""
    pts = SR.unit_points(64, 3)
    ad = torch.from_numpy(np.ascontiguousarray(pts[np.arange(3000) % 64])).cuda()
    bd = torch.from_numpy(np.ascontiguousarray(pts[np.arange(40 * 1024) % 64])).cuda()

    def dirty():
        d2, idx = ops.split_nearest(ad, bd)
        assert ops.last_kernel() == "split_nearest_kernel<4>+split_merge_kernel" and ops.last_grid() == 3 * 40, (ops.last_kernel(), ops.last_grid())
        assert not d2.any() and torch.equal(idx.cpu().long(), torch.arange(3000) % 64)

    for Na, Nb, ranges, ra in [(300, 4 * 1024 + 5, 5, 1), (1500, 3000, 3, 4)]:
        a, b = SR.nearest_case(Na, Nb, Na + Nb)
        want = split.nearest(a, b)
        a_d, b_d = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()

        def probe():
            d2, idx = ops.split_nearest(a_d, b_d)
            assert ops.last_kernel() == f"split_nearest_kernel<{ra}>+split_merge_kernel", ops.last_kernel()
            assert ops.last_grid() == cdiv(Na, 256 * ra) * ranges, ops.last_grid()
            assert torch.equal(d2.cpu(), torch.from_numpy(want[0].view(np.int64))) and torch.equal(idx.cpu(), torch.from_numpy(want[1]))
            return [d2, idx]

        carry(probe, [dirty])
