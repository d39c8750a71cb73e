"""Loss-kernel timings: ig_ce_loss (the yardstick) against ig_seg_loss -- focal only, region (Dice) only, both -- with and without
dlogits, at the two flagship head shapes (B = 432, K = 2 and B = 72, K = 13 at 224 x 224), next to the box's copy rate (the "copy"
line of tools/hbm_ceiling.py -- a 1 GiB torch copy_ -- measured again here, in this process, with this file's event timing) and, with --step, the chips/s of a fused train step with loss = ce against focal_dice.

    python tools/seg_loss_bench.py [--metrics] [--step] [--batch 432]

IG_HIP_LIB=<another build> runs the same timings on that build (same-box A/B of two builds: alternate the two in separate processes).

Each kernel variant is timed ROUNDS times, interleaved with the others (so drift hits all alike), each sample = REPS back-to-back launches
between two HIP events after a warm-up; the table gives the median and the min-max spread of the samples, the ratio to ce_loss's median,
and for the region variants the extra time against the bytes of the second pass at the copy rate.
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "instageo-e2e-geospatial-ml_amd"))
from instageo_amd import ops  # noqa: E402

DEV = "cuda"
ROUNDS, REPS = 9, 20


def sample(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / REPS * 1e3  # us


def copy_rate():
    x = torch.empty(256 * 1024 * 1024, dtype=torch.float32, device=DEV).normal_()
    y = torch.empty_like(x)
    for _ in range(3):
        y.copy_(x)
    return statistics.median(2 * x.numel() * 4 / (sample(lambda: y.copy_(x)) * 1e-6) for _ in range(5))  # B/s


def kernels(B, K, rate):
    g = torch.Generator().manual_seed(5)
    z = (torch.randn(B, K, 224, 224, generator=g) * 3).to(DEV)
    y = torch.randint(-1, K, (B, 224, 224), generator=g).to(DEV)
    cw = (torch.rand(K, generator=g) + 0.5).to(DEV)
    stats = torch.zeros(2, dtype=torch.float64, device=DEV)
    conf = torch.zeros(K, K, dtype=torch.int64, device=DEV)
    dl = torch.empty_like(z)
    variants = {}  # (name, with dlogits) -> launch
    for d in (dl, None):
        variants[("ce_loss", d is not None)] = lambda d=d: ops.ce_loss(z, y, cw, -1, stats, d, None, None, conf)
        for name, gamma, lam in (("seg_loss focal g=2 l=0", 2.0, 0.0), ("seg_loss dice g=0 l=1", 0.0, 1.0), ("seg_loss focal+dice g=2 l=1", 2.0, 1.0)):
            variants[(name, d is not None)] = lambda d=d, gamma=gamma, lam=lam: ops.seg_loss(
                z, y, cw, -1, stats, d, None, None, conf, focal_gamma=gamma, region_weight=lam)
    for fn in variants.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, fn in variants.items():
            t[k].append(sample(fn))
    med = {k: statistics.median(v) for k, v in t.items()}
    npx = B * 224 * 224
    pass2 = npx * (K * 4 + 8 + 2 * K * 4)  # second pass: logits + int64 labels read, dlogits read and written
    print(f"\nB = {B}, K = {K}, 224 x 224 ({npx * K * 4 / 2**20:.0f} MiB of logits), int64 labels; {ROUNDS} samples of {REPS} launches")
    print(f"{'variant':40s} {'median us':>10s} {'min':>8s} {'max':>8s} {'spread':>7s} {'/ ce':>6s}")
    for (name, wd), v in t.items():
        base = med[("ce_loss", wd)]
        m = med[(name, wd)]
        line = (f"{name + (' +dlogits' if wd else ' loss only'):40s} {m:10.1f} {min(v):8.1f} {max(v):8.1f} {(max(v) - min(v)) / m * 100:6.1f}% "
                f"{m / base:6.3f}")
        if "l=1" in name and wd:  # what the region term adds to the same pixel term without it
            extra = m - (base if "g=0" in name else med[("seg_loss focal g=2 l=0", wd)])
            bw = pass2 / (extra * 1e-6)
            line += f"   second pass {extra:7.1f} us for {pass2 / 2**20:.0f} MiB = {bw / 1e12:.2f} TB/s ({bw / rate * 100:.0f}% of copy)"
        print(line)


def metrics(B, K):
    """The other label-walking kernels of the family: distillation loss, AUC histograms, temperature grid, reliability histograms."""
    g = torch.Generator().manual_seed(7)
    z = (torch.randn(B, K, 224, 224, generator=g) * 3).to(DEV)
    zt = (torch.randn(B, K, 224, 224, generator=g) * 3).to(DEV)
    y = torch.randint(-1, K, (B, 224, 224), generator=g).to(DEV)
    kl = torch.zeros(1, dtype=torch.float64, device=DEV)
    dl = torch.zeros_like(z)
    auc = torch.zeros(2 * K * 100, dtype=torch.int64, device=DEV)
    nll = torch.zeros(9, dtype=torch.float64, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int64, device=DEV)
    rel = torch.zeros(K, 3, 15, dtype=torch.int64, device=DEV)
    variants = {"kd_loss +dlogits": lambda: ops.kd_loss(z, zt, y, -1, kl, dl),
                "auc_update 100 bins": lambda: ops.auc_update(z, y, -1, auc, 100),
                "calib_nll_grid K=9": lambda: ops.calib_nll_grid(z, y, -1, [0.5 + 0.125 * k for k in range(9)], nll, cnt),
                "reliability_update 15 bins": lambda: ops.reliability_update(z, y, -1, 1.0, rel)}
    for fn in variants.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, fn in variants.items():
            t[k].append(sample(fn))
    print(f"\nB = {B}, K = {K}, 224 x 224, int64 labels; {ROUNDS} samples of {REPS} launches")
    print(f"{'variant':40s} {'median us':>10s} {'min':>8s} {'max':>8s} {'spread':>7s}")
    for k, v in t.items():
        m = statistics.median(v)
        print(f"{k:40s} {m:10.1f} {min(v):8.1f} {max(v):8.1f} {(max(v) - min(v)) / m * 100:6.1f}%")


def step(B):
    from instageo_amd.segmentation import PrithviSegmentationModule

    g = torch.Generator().manual_seed(6)
    x = torch.randn(B, 6, 1, 224, 224, generator=g).to(DEV)
    y = torch.randint(-1, 2, (B, 224, 224), generator=g).to(DEV)
    stats = torch.zeros(2, dtype=torch.float64, device=DEV)
    t = {}
    for loss in ("ce", "focal_dice"):  # one module at a time: two sets of B = 432 workspaces need not fit together
        m = PrithviSegmentationModule(image_size=224, learning_rate=1e-4, freeze_backbone=False, load_pretrained_weights=False, num_classes=2,
                                      class_weights=[1, 3], ignore_index=-1, scheduler=False, model_name="prithvi_eo_v1_100",
                                      precision="bf16", device=DEV, loss=loss)
        for _ in range(3):
            m.fused_train_step(x, y, stats=stats)
        torch.cuda.synchronize()
        t[loss] = []
        for _ in range(5):
            t0 = time.perf_counter()
            for _ in range(4):
                m.fused_train_step(x, y, stats=stats)
            torch.cuda.synchronize()
            t[loss].append(B * 4 / (time.perf_counter() - t0))
        del m
        torch.cuda.empty_cache()
    print(f"\nfused_train_step, prithvi_eo_v1_100 bf16, B = {B}, K = 2: chips/s, 5 samples of 4 steps each")
    for k, v in t.items():
        print(f"  loss = {k:10s} median {statistics.median(v):8.1f}  min {min(v):8.1f}  max {max(v):8.1f}")
    print(f"  focal_dice / ce = {statistics.median(t['focal_dice']) / statistics.median(t['ce']):.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", action="store_true", help="also time the whole fused train step with loss = ce and focal_dice")
    ap.add_argument("--batch", type=int, default=432, help="batch of the --step leg")
    ap.add_argument("--metrics", action="store_true", help="also time ig_kd_loss, ig_auc_update, ig_calib_nll_grid and ig_reliability_update")
    args = ap.parse_args()
    print(torch.cuda.get_device_name(0))
    rate = copy_rate()
    print(f"copy rate (1 GiB read + 1 GiB write): {rate / 1e12:.2f} TB/s")
    kernels(432, 2, rate)
    kernels(72, 13, rate)
    if args.metrics:
        metrics(432, 2)
        metrics(72, 13)
    if args.step:
        step(args.batch)


if __name__ == "__main__":
    main()
