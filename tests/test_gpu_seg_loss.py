"""Focal + Dice / Tversky segmentation loss (-m gpu): ``ig_seg_loss`` against the formulas of DESIGN.md ("Focal and region losses")
evaluated in float64 torch in this file, and the modules that train on it.

Accuracy bar (the rule of test_gpu_value_ranges.py): max |kernel - f64| <= max(4 x max |the same formulas in fp32 torch on the
device - f64|, 2^-22 x max |f64|); the loss sums add the quantum of the 2^-28 fixed point their workgroup partials pass through.

Every check prints its error, the bar, the fp32 error and err / bar (``-s`` shows the table); each case ends with the worst ratios
of its input family.
"""
import itertools
import math
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from instageo_amd import ops  # noqa: E402
from instageo_amd.segmentation import (PrithviDistillationSegmentationModule, PrithviSegmentationModule, loss_spec,  # noqa: E402
                                       segmentation_loss)
from oracle import prithvi_oracle as O  # noqa: E402

DEV = "cuda"
IGN = -1
FLOOR_F32 = 2.0**-22
SHAPES = [(3, 2, 8, 12), (2, 13, 7, 9), (1, 16, 4, 4), (40, 5, 224, 224)]
FAMILIES = ["randn3", "confident", "offset"]
LABEL_DTYPES = [torch.int64, torch.int32, torch.float32]
GAMMAS, LAMBDAS, TVERSKY, SMOOTH = [0.0, 1.0, 2.0, 5.0], [0.0, 0.5, 1.0], [(0.5, 0.5), (0.3, 0.7)], [1.0, 0.0]
ALL_COMBOS = list(itertools.product(GAMMAS, LAMBDAS, TVERSKY, SMOOTH, [False, True]))
# the large shape: every value of every parameter at least once, region term on and off, not the whole product
BIG_COMBOS = [(0.0, 1.0, (0.5, 0.5), 1.0, False), (2.0, 0.0, (0.5, 0.5), 1.0, True), (2.0, 1.0, (0.3, 0.7), 0.0, True),
              (5.0, 0.5, (0.5, 0.5), 0.0, False), (1.0, 0.5, (0.3, 0.7), 1.0, True)]


def label_variants(K):
    """Two classes cannot have one absent AND one on a single pixel with anything left: those two label sets are separate there."""
    return ["single", "absent"] if K == 2 else ["both"]


def make_case(shape, family, variant=None):
    """(logits f32 [as the kernel sees them], logits f64 of the un-offset problem, labels int64, class weights), on the device.
    Labels: ~10 % ignore_index, a few out-of-range values (K and -5), class K - 1 absent, class 0 on exactly one pixel
    (K = 2: "single" = class 0 on one pixel and class 1 elsewhere, "absent" = class 0 everywhere and class 1 absent)."""
    B, K, H, W = shape
    g = torch.Generator().manual_seed(1000 * K + B)
    z = torch.randn(B, K, H, W, generator=g) * (30.0 if family == "confident" else 3.0)
    z = (z * 1024).round() / 1024  # multiples of 2^-10: z + 1000 is exact in fp32, so the offset case is the same problem
    z64 = z.double()
    if family == "offset":
        z = z + 1000.0
        assert torch.equal(z.double() - 1000.0, z64)
    lab = torch.randint(1, max(K - 1, 2), (B, H, W), generator=g)  # classes 1 .. K-2 (K = 2: class 1 only)
    if variant == "absent":
        lab.zero_()
    flat = lab.view(-1)
    n = flat.numel()
    perm = torch.randperm(n, generator=g)
    flat[perm[: n // 10]] = IGN
    flat[perm[n // 10]] = K
    flat[perm[n // 10 + 1]] = -5
    flat[perm[n // 10 + 2]] = K
    if variant != "absent":
        flat[perm[n // 10 + 3]] = 0  # the single pixel of class 0
    if family == "confident":
        # the label's class is the top class on ~80 % of the valid pixels (its logit and the largest one change places), so pt is
        # within 1e-6 of 1 on most pixels; on the rest the prediction is confidently wrong
        valid = (lab >= 0) & (lab < K)
        hit = valid & (torch.rand(B, H, W, generator=g) < 0.8)
        yi, ti = lab.clamp(0, K - 1)[:, None], z64.argmax(1, keepdim=True)
        zy, zt = z64.gather(1, yi), z64.gather(1, ti)
        z64 = z64.scatter(1, ti, torch.where(hit[:, None], zy, zt)).scatter(1, yi, torch.where(hit[:, None], zt, zy))
        z = z64.float()
        assert torch.equal(z.double(), z64)
    cw = torch.rand(K, generator=g) + 0.5
    return z.to(DEV), z64.to(DEV), lab.to(DEV), cw.to(DEV)


def formulas(z, y, w, gamma, lam, alpha, beta, s, pixel_on=True):
    """Section "Focal and region losses" of DESIGN.md in the dtype of ``z``: -> (stats[0], |V|, parts[2], dlogits), all un-normalised."""
    K = z.shape[1]
    T = z.dtype
    valid = (y != IGN) & (y >= 0) & (y < K)
    yc = y.clamp(0, K - 1)
    v = valid[:, None].to(T)
    oh = F.one_hot(yc, K).permute(0, 3, 1, 2).to(T) * v
    logp, p = F.log_softmax(z, 1), F.softmax(z, 1)
    pt, logpt = (p * oh).sum(1), (logp * oh).sum(1)
    wy = (w.to(T)[yc] if w is not None else torch.ones_like(pt)) * valid.to(T) * (1.0 if pixel_on else 0.0)
    omp = 1 - pt
    if gamma == 0:
        f, gf = torch.ones_like(pt), torch.ones_like(pt)
    else:
        f, gf = omp**gamma, omp ** (gamma - 1) * (omp - gamma * pt * logpt)
    pix = (wy * f * (-logpt)).sum()
    dl = (wy * gf)[:, None] * (p - oh) * v
    V = valid.sum().to(T)
    reg = torch.zeros((), dtype=T, device=z.device)
    if lam > 0:
        I, P, G = (p * oh).sum((0, 2, 3)), (p * v).sum((0, 2, 3)), oh.sum((0, 2, 3))
        present = G > 0
        Kp = present.sum().to(T)
        N, D = I + s, I + alpha * (P - I) + beta * (G - I) + s
        zero = torch.zeros_like(D)
        Lreg = torch.where(present, 1 - N / D, zero).sum() / Kp
        A = torch.where(present, -(D - N * (1 - alpha - beta)) / (Kp * D * D), zero)
        Bc = torch.where(present, N * alpha / (Kp * D * D), zero)
        gg = A[None, :, None, None] * oh + Bc[None, :, None, None]
        reg = V * lam * Lreg
        dl = dl + V * lam * (p * (gg - (p * gg).sum(1, keepdim=True)) * v)
    return pix + reg, V, torch.stack([pix, reg]), dl


def run_kernel(z, lab, cw, gamma, lam, ab, s, pixel_on=True, want_dlogits=True, confusion=True):
    B, K, H, W = z.shape
    out = dict(stats=torch.zeros(2, dtype=torch.float64, device=DEV), parts=torch.zeros(2, dtype=torch.float64, device=DEV),
               dlogits=torch.full_like(z, float("nan")) if want_dlogits else None,
               preds=torch.full((B, H, W), -7, dtype=torch.int64, device=DEV), preds_i8=torch.full((B, H, W), -7, dtype=torch.int8, device=DEV),
               confusion=torch.zeros(K, K, dtype=torch.int64, device=DEV) if confusion else None)
    ops.seg_loss(z, lab, cw, IGN, out["stats"], out["dlogits"], out["preds"], out["preds_i8"], out["confusion"], focal_gamma=gamma,
                 pixel_term=pixel_on, region_weight=lam, region_smooth=s, tversky=ab, parts=out["parts"])
    return out


WORST = {}


def check(got, ref, t32, what, family, quantum=0.0):
    got, ref, t32 = got.double(), ref.double(), t32.double()
    assert got.shape == ref.shape == t32.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(ref).all(), f"{what}: the float64 reference is not finite"
    assert torch.isfinite(got).all(), f"{what}: non-finite kernel output"
    scale = ref.abs().max().item()
    err = (got - ref).abs().max().item()
    terr = (t32 - ref).abs().max().item()
    bar = max(4.0 * terr, FLOOR_F32 * scale) + quantum
    ratio = err / max(bar, 1e-300)
    key = (family, what.split()[0])
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print(f"SL {family} {what}: err {err:.3e} bar {bar:.3e} torch32 {terr:.3e} scale {scale:.3e} ratio {ratio:.3g}")
    assert err <= bar, f"{family} {what}: max err {err:.3e} > bar {bar:.3e} (fp32 torch {terr:.3e}, scale {scale:.3e})"


def loss_quantum(npix):  # one rounding to the 2^-28 fixed point per workgroup partial (ce_loss_kernel): at most 1024 workgroups
    return 2.0**-28 * min(1024, math.ceil(npix / 256))


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_seg_loss_matches_float64_formulas(shape, family):
    for variant in label_variants(shape[1]):
        _check_formulas(shape, family, variant)
    print("SL worst ratios:", {k: f"{v:.3g}" for k, v in WORST.items() if k[0] == family})


def _check_formulas(shape, family, variant):
    B, K, H, W = shape
    z, z64, lab, cw = make_case(shape, family, variant)
    valid = (lab != IGN) & (lab >= 0) & (lab < K)
    top = z64.argmax(1)
    conf_ref = torch.bincount((lab[valid] * K + top[valid]).view(-1), minlength=K * K).view(K, K)
    assert variant == "single" or conf_ref[K - 1].sum() == 0  # one class absent
    assert variant == "absent" or conf_ref[0].sum() == 1  # one class with a single pixel
    z32 = z64.float()  # the fp32 yardstick works on the un-offset problem
    q = loss_quantum(B * H * W)
    combos = ALL_COMBOS if B * H * W < 10000 else BIG_COMBOS
    for i, (gamma, lam, ab, s, weighted) in enumerate(combos):
        if lam == 0 and (ab != TVERSKY[0] or s != SMOOTH[0]):
            continue  # the region parameters do not enter
        w = cw if weighted else None
        ref = formulas(z64, lab, w.double() if weighted else None, gamma, lam, ab[0], ab[1], s)
        t32 = formulas(z32, lab, w, gamma, lam, ab[0], ab[1], s)
        ldt = LABEL_DTYPES[i % 3]
        got = run_kernel(z, lab.to(ldt), w, gamma, lam, ab, s)
        tag = f"g{gamma:g} l{lam:g} ab{ab} s{s:g} w{int(weighted)} {str(ldt)[6:]}"
        assert got["stats"][1].item() == ref[1].item() == valid.sum().item(), tag
        check(got["stats"][:1], ref[0].reshape(1), t32[0].reshape(1), f"stats {tag}", family, quantum=q)
        check(got["parts"], ref[2], t32[2], f"parts {tag}", family, quantum=q)
        check(got["dlogits"], ref[3], t32[3], f"dlogits {tag}", family)
        if family == "confident":  # the same bar on the truly confident pixels alone, where (1 - pt)^gamma is ~0 and 1.f - pt is 0
            sure = (valid & (F.softmax(z64, 1).gather(1, lab.clamp(0, K - 1)[:, None])[:, 0] > 0.999))[:, None].expand_as(z64)
            assert sure.float().mean() > 0.25  # 0.31 (16 classes: the runner-up is often close) to 0.74 (2 classes) of all pixels
            check(got["dlogits"][sure], ref[3][sure], t32[3][sure], f"dlogits_sure {tag}", family)
        assert torch.equal(got["preds"], top) and torch.equal(got["preds_i8"].long(), top), tag
        assert torch.equal(got["confusion"], conf_ref), tag


@pytest.mark.parametrize("shape", SHAPES[:3], ids=lambda s: "x".join(map(str, s)))
def test_dice_alone_and_loss_only_launch(shape):
    """pixel_term = 0 (loss "dice"): the pixel term leaves loss and gradient, the count, argmax and confusion stay.  Without dlogits
    (validation): the same statistics, bit for bit, from the launch that only finalises the loss."""
    z, z64, lab, cw = make_case(shape, "randn3")
    ref = formulas(z64, lab, cw.double(), 0.0, 1.0, 0.3, 0.7, 1.0, pixel_on=False)
    t32 = formulas(z64.float(), lab, cw, 0.0, 1.0, 0.3, 0.7, 1.0, pixel_on=False)
    got = run_kernel(z, lab, cw, 0.0, 1.0, (0.3, 0.7), 1.0, pixel_on=False)
    full = run_kernel(z, lab, cw, 0.0, 1.0, (0.3, 0.7), 1.0)
    assert got["parts"][0].item() == 0.0 and got["stats"][1].item() == ref[1].item()
    check(got["stats"][:1], ref[0].reshape(1), t32[0].reshape(1), "stats dice", "randn3")
    check(got["dlogits"], ref[3], t32[3], "dlogits dice", "randn3")
    assert torch.equal(got["preds"], full["preds"]) and torch.equal(got["confusion"], full["confusion"])
    for pixel_on in (False, True):
        a = run_kernel(z, lab, cw, 2.0, 0.5, (0.5, 0.5), 1.0, pixel_on=pixel_on)
        b = run_kernel(z, lab, cw, 2.0, 0.5, (0.5, 0.5), 1.0, pixel_on=pixel_on, want_dlogits=False, confusion=False)
        assert torch.equal(a["stats"], b["stats"]) and torch.equal(a["parts"], b["parts"]) and torch.equal(a["preds"], b["preds"])


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gamma0_lambda0_is_ig_ce_loss_bit_for_bit(shape, weighted):
    B, K, H, W = shape
    for family in ("randn3", "confident"):
        z, _, lab, cw = make_case(shape, family)
        w = cw if weighted else None
        for ldt in LABEL_DTYPES:
            got = run_kernel(z, lab.to(ldt), w, 0.0, 0.0, (0.5, 0.5), 1.0)
            stats = torch.zeros(2, dtype=torch.float64, device=DEV)
            dlog = torch.full_like(z, float("nan"))
            preds = torch.empty(B, H, W, dtype=torch.int64, device=DEV)
            p8 = torch.empty(B, H, W, dtype=torch.int8, device=DEV)
            conf = torch.zeros(K, K, dtype=torch.int64, device=DEV)
            ops.ce_loss(z, lab.to(ldt), w, IGN, stats, dlog, preds, p8, conf)
            assert torch.equal(got["stats"], stats), (got["stats"], stats)
            assert torch.equal(got["dlogits"], dlog) and torch.equal(got["preds"], preds) and torch.equal(got["preds_i8"], p8)
            assert torch.equal(got["confusion"], conf)
            assert got["parts"][0].item() == stats[0].item() and got["parts"][1].item() == 0.0


def test_label_dtypes_agree_bit_for_bit():
    z, _, lab, cw = make_case(SHAPES[1], "randn3")
    outs = [run_kernel(z, lab.to(t), cw, 2.0, 1.0, (0.3, 0.7), 1.0) for t in LABEL_DTYPES]
    for o in outs[1:]:
        for k in ("stats", "parts", "dlogits", "preds", "confusion"):
            assert torch.equal(o[k], outs[0][k]), k


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[1]], ids=lambda s: "x".join(map(str, s)))
def test_all_labels_ignored(shape):
    B, K, H, W = shape
    z, _, lab, cw = make_case(shape, "randn3")
    for labels in (torch.full_like(lab, IGN), torch.full_like(lab, K + 3)):
        got = run_kernel(z, labels, cw, 2.0, 1.0, (0.5, 0.5), 1.0)
        torch.cuda.synchronize()
        assert got["stats"][1].item() == 0 and math.isnan((got["stats"][0] / got["stats"][1]).item())
        assert math.isnan(got["stats"][0].item())  # the region term of an empty selection is 0 / 0, as the formulas give
        assert torch.equal(got["dlogits"], torch.zeros_like(z))
        assert got["confusion"].sum().item() == 0 and torch.equal(got["preds"], z.argmax(1))


@pytest.mark.parametrize("shape", [SHAPES[3], SHAPES[2]], ids=lambda s: "x".join(map(str, s)))
def test_seg_loss_is_bit_reproducible(shape):
    z, _, lab, cw = make_case(shape, "randn3")
    runs = [run_kernel(z, lab, cw, 2.0, 1.0, (0.3, 0.7), 1.0) for _ in range(4)]
    for r in runs[1:]:
        for k in ("stats", "parts", "dlogits"):
            assert torch.equal(r[k], runs[0][k]), k


# ---------------------------------------------------------------------------------------------------------------------------------
# modules
# ---------------------------------------------------------------------------------------------------------------------------------
def _module(loss, precision, cls=PrithviSegmentationModule, **kw):
    m = cls(freeze_backbone=False, load_pretrained_weights=False, num_classes=3, model_name="prithvi_eo_tiny", class_weights=[1.0, 2.0, 0.5],
            ignore_index=IGN, learning_rate=1e-3, precision=precision, device=DEV, loss=loss, focal_gamma=2.0, region_weight=0.5,
            tversky=(0.3, 0.7), **kw)
    m.net.load_state_dict(O.make_state_dict(O.make_config("prithvi_eo_tiny", 1, 3), seed=11))
    m.net.cfg.drop_p = 0.0
    return m


def _batch():
    g = torch.Generator().manual_seed(21)
    x = torch.randn(2, 6, 1, 224, 224, generator=g).to(DEV)
    y = torch.randint(-1, 3, (2, 224, 224), generator=g).to(DEV)
    return x, y


@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
@pytest.mark.parametrize("loss", ["focal", "ce_dice", "focal_dice"])
def test_fused_step_equals_the_autograd_path(loss, precision):
    """fused_train_step against training_step + backward: the same loss, the same parameter gradients (the bounds of
    test_regression_lightning_style_steps); the loss itself against the float64 formulas on the module's own logits."""
    x, y = _batch()
    a, b = _module(loss, precision), _module(loss, precision)
    a.net.train()
    lval = a.training_step((x, y), 0)
    assert lval.dim() == 0 and lval.requires_grad and torch.isfinite(lval)
    lval.backward()
    got = {n: p.grad.clone() for n, p in a.net.named_parameters() if p.grad is not None}
    b.net.train()
    st = b.fused_train_step(x, y)
    assert abs((st[0] / st[1]).item() - lval.item()) < 1e-5 * max(1.0, lval.item())
    gb = b.net.store.grad
    for name in ("segmentation_head.5.weight", "prithvi_encoder.blocks.0.attn.qkv.weight", "prithvi_encoder.patch_embed.proj.weight"):
        ref = b.net.store.entries[name].api_view(gb)
        assert torch.allclose(got[name], ref, rtol=2e-3, atol=1e-6 + 2e-3 * float(ref.abs().max())), name
    with torch.no_grad():
        a.net.eval()
        logits = a.net(x)
        spec = loss_spec(loss, 2.0, 0.5, 1.0, (0.3, 0.7))
        ref = formulas(logits.double(), y, a._weights().double(), spec["focal_gamma"], spec["region_weight"], 0.3, 0.7, 1.0)
        v = a.validation_step((x, y), 0)
        assert abs(v.item() - (ref[0] / ref[1]).item()) < 1e-5 * max(1.0, v.item())
        sv = a.fused_eval_step(x, y, "val")
        assert abs((sv[0] / sv[1]).item() - v.item()) < 1e-6 * max(1.0, v.item())
    if loss.endswith("dice"):
        for step in ("train", "val"):
            assert {f"{step}_pixel_loss", f"{step}_dice_loss"} <= set(a.logged), a.logged.keys()
        assert abs(float(a.logged["val_pixel_loss"]) + float(a.logged["val_dice_loss"]) - v.item()) < 1e-5
        assert abs(float(b.logged["train_pixel_loss"]) + float(b.logged["train_dice_loss"]) - (st[0] / st[1]).item()) < 1e-5
    else:
        assert "train_dice_loss" not in a.logged and "train_dice_loss" not in b.logged


def test_ce_module_still_calls_ig_ce_loss(monkeypatch):
    calls = []
    monkeypatch.setattr(ops, "seg_loss", lambda *a, **k: calls.append("seg"))
    real = ops.ce_loss
    monkeypatch.setattr(ops, "ce_loss", lambda *a, **k: (calls.append("ce"), real(*a, **k))[1])
    m = _module("ce", "bf16")
    x, y = _batch()
    m.fused_train_step(x, y)
    m.fused_eval_step(x, y, "val")
    m.training_step((x, y), 0)
    assert calls == ["ce", "ce", "ce"] and m._loss_spec is None


def test_graphed_focal_dice_step_replays_bit_identically_and_learns():
    x, y = _batch()
    try:
        eager = _module("focal_dice", "bf16")
        eager.net.engine.deterministic = True
        s_eager = torch.stack([eager.fused_train_step(x, y).clone() for _ in range(3)])
        p_eager = eager.net.store.flat.clone()
        graphed = _module("focal_dice", "bf16")
        graphed.net.engine.deterministic = True
        run = graphed.make_graphed_train_step(x, y)
        s_graph = torch.stack([run(x, y).clone() for _ in range(3)])
        torch.cuda.synchronize()
        assert torch.equal(s_graph, s_eager), (s_graph, s_eager)
        assert torch.equal(graphed.net.store.flat, p_eager)
        losses = (s_eager[:, 0] / s_eager[:, 1]).tolist()
        assert losses[2] < losses[0], losses  # three steps on a fixed batch lower the loss
        assert abs(float(graphed.logged["train_pixel_loss"]) + float(graphed.logged["train_dice_loss"]) - losses[2]) < 1e-5
    finally:
        ops.set_deterministic(None)


def test_distillation_module_stacks_the_kl_term_on_focal_dice(tmp_path):
    x, y = _batch()
    teacher = _module("ce", "bf16")
    ck = os.path.join(tmp_path, "teacher.ckpt")
    torch.save({"state_dict": teacher.checkpoint_state_dict()}, ck)
    m = _module("focal_dice", "bf16", cls=PrithviDistillationSegmentationModule, teacher_ckpt_path=ck)
    st = m.fused_train_step(x, y)
    total = (st[0] / st[1]).item()
    parts = [m.logged["train_ce_loss"], m.logged["train_dice_loss"], m.logged["train_distill_loss"]]
    assert all(math.isfinite(float(p)) for p in parts) and float(parts[1]) > 0
    assert abs(total - sum(float(p) for p in parts)) < 1e-6 * max(1.0, abs(total)), (total, parts)
    with torch.no_grad():  # the pixel term named by train_ce_loss is the focal term, not the plain cross-entropy
        plain = _module("focal", "bf16", cls=PrithviDistillationSegmentationModule, teacher_ckpt_path=ck)
        plain.fused_train_step(x, y)
    assert abs(float(plain.logged["train_ce_loss"]) - float(parts[0])) < 1e-6 * max(1.0, float(parts[0]))
    m2 = _module("focal_dice", "bf16", cls=PrithviDistillationSegmentationModule, teacher_ckpt_path=ck)
    m2.net.train()
    loss = m2.training_step((x, y), 0)  # the autograd path gives the same total
    assert abs(loss.item() - total) < 1e-5 * max(1.0, abs(total))
