"""Float64 host formulas of the calibration kernels and of the temperature fit, for the tests.

Everything works on numpy arrays: logits (B, ncls, H, W), labels (B, H, W) integers.  A pixel is valid iff
``label != ignore_index and 0 <= label < ncls``."""
import math

import numpy as np

CONF_SCALE = float(2**24)


def valid_mask(labels, ignore_index, ncls):
    lab = np.asarray(labels).astype(np.int64)
    return (lab != ignore_index) & (lab >= 0) & (lab < ncls)


def _rows(logits, labels, ignore_index):
    """(z (n, ncls) float64, y (n,)) of the valid pixels, in pixel order."""
    z = np.asarray(logits, dtype=np.float64)
    B, K = z.shape[:2]
    z = np.moveaxis(z.reshape(B, K, -1), 1, 2).reshape(-1, K)
    lab = np.asarray(labels).astype(np.int64).reshape(-1)
    v = valid_mask(lab, ignore_index, K)
    return z[v], lab[v]


def nll_sums(logits, labels, ignore_index, betas):
    """-> (sum over valid pixels of logsumexp_c(beta z_c) - beta z_y for every beta, #valid)."""
    z, y = _rows(logits, labels, ignore_index)
    out = []
    for b in betas:
        a = float(b) * z
        m = a.max(1, keepdims=True)
        lse = m[:, 0] + np.log(np.exp(a - m).sum(1))
        out.append(float((lse - a[np.arange(len(y)), y]).sum()))
    return np.array(out), len(y)


def softmax_rows(z, beta=1.0):
    a = float(beta) * z
    e = np.exp(a - a.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def reliability(logits, labels, ignore_index, beta, nbins):
    """-> dict: hist int64 [ncls][3][nbins] (count, hits, confidence in 2^-24 units rounded per pixel), conf_sum float64 [ncls][nbins],
    and per valid pixel pred, bin, conf, second (the runner-up class) and gap (top probability - runner-up)."""
    z, y = _rows(logits, labels, ignore_index)
    K = z.shape[1]
    p = softmax_rows(z, beta)
    pred = z.argmax(1)  # the first maximum; beta > 0 keeps the order
    conf = p[np.arange(len(y)), pred]
    q = p.copy()
    q[np.arange(len(y)), pred] = -1.0
    second = q.argmax(1)
    gap = conf - q[np.arange(len(y)), second]
    b = np.minimum(nbins - 1, np.floor(conf * nbins).astype(np.int64))
    hist = np.zeros((K, 3, nbins), dtype=np.int64)
    conf_sum = np.zeros((K, nbins))
    np.add.at(hist[:, 0], (pred, b), 1)
    np.add.at(hist[:, 1], (pred, b), (pred == y).astype(np.int64))
    np.add.at(hist[:, 2], (pred, b), np.floor(conf * CONF_SCALE + 0.5).astype(np.int64))
    np.add.at(conf_sum, (pred, b), conf)
    return dict(hist=hist, conf_sum=conf_sum, pred=pred, bin=b, conf=conf, second=second, gap=gap, y=y)


def golden_section(f, lo, hi, tol=1e-10):
    """Minimiser of a unimodal f on [lo, hi]."""
    g = (math.sqrt(5.0) - 1.0) / 2.0
    a, b = lo, hi
    c, d = b - g * (b - a), a + g * (b - a)
    fc, fd = f(c), f(d)
    while b - a > tol:
        if fc < fd:
            b, d, fd = d, c, fc
            c = b - g * (b - a)
            fc = f(c)
        else:
            a, c, fc = c, d, fd
            d = a + g * (b - a)
            fd = f(d)
    return 0.5 * (a + b)


def best_ln_temperature(logits, labels, ignore_index, lo=math.log(1.0 / 64), hi=math.log(64.0)):
    """ln T minimising the cross-entropy of softmax(logits / T) (convex in 1 / T, unimodal in ln T)."""
    z, y = _rows(logits, labels, ignore_index)
    idx = np.arange(len(y))

    def f(ln_t):
        a = z * math.exp(-ln_t)
        m = a.max(1, keepdims=True)
        return float((m[:, 0] + np.log(np.exp(a - m).sum(1)) - a[idx, y]).sum())

    return golden_section(f, lo, hi)


def ece_from_pixels(conf, hit, nbins):
    """The textbook ECE / MCE straight from per-pixel confidences and hits (float64), for cross-checking the histogram arithmetic."""
    b = np.minimum(nbins - 1, np.floor(np.asarray(conf) * nbins).astype(np.int64))
    ece, mce, n = 0.0, 0.0, len(conf)
    for k in range(nbins):
        m = b == k
        if m.any():
            gap = abs(np.mean(np.asarray(hit)[m]) - np.mean(np.asarray(conf)[m]))
            ece += m.sum() / n * gap
            mce = max(mce, gap)
    return ece, mce
