"""Sequential twin of the compositing rule of include/instageo_hip.h (``ig_composite``), written pixel by pixel from the header's text with
plain Python integers: independent of the vectorised host path of instageo_amd/composite.py.  Also the packed test stacks both suites
share."""
import functools

import numpy as np

ND = -9999
CLOUD, NEAR, SHADOW, WATER = 1 << 1, 1 << 2, 1 << 3, 1 << 5
BITS = CLOUD | NEAR | SHADOW
METHODS = ("nearest", "median", "medoid")


def twin(bands, starts, fmasks, fmask_starts, step_ptr, C, H, W, bits, nd, min_clear, method):
    """-> (composite (T, C, H, W) int16, count (T, H, W) uint8, source (T, H, W) uint8, hist (T, 17) int32)."""
    T, HW = len(step_ptr) - 1, H * W
    comp = np.empty((T, C, HW), dtype=np.int16)
    count = np.empty((T, HW), dtype=np.uint8)
    source = np.empty((T, HW), dtype=np.uint8)
    hist = np.zeros((T, 17), dtype=np.int32)
    b = [int(x) for x in bands.tolist()]
    f = None if fmasks is None else [int(x) for x in fmasks.tolist()]
    for t in range(T):
        cand = list(range(int(step_ptr[t]), int(step_ptr[t + 1])))
        for p in range(HW):
            vals = [[b[int(starts[n * C + c]) + p] for c in range(C)] for n in cand]
            clear = []
            for i, n in enumerate(cand):
                ok = f is None or (f[int(fmask_starts[n]) + p] & bits) == 0
                clear.append(ok and all(x != nd for x in vals[i]))
            idx = [i for i in range(len(cand)) if clear[i]]
            cnt = len(idx)
            count[t, p] = cnt
            hist[t, cnt] += 1
            out, src = [nd] * C, 255
            if cnt >= min_clear:
                if method == "nearest":
                    src = idx[0]
                    out = vals[src]
                else:
                    med = [sorted(vals[i][c] for i in idx)[(cnt - 1) // 2] for c in range(C)]
                    if method == "median":
                        out = med
                    else:
                        best = None
                        for i in idx:  # ascending: a later candidate must be strictly better
                            d = sum(abs(vals[i][c] - med[c]) for c in range(C))
                            if best is None or d < best:
                                best, src = d, i
                        out = vals[src]
            comp[t, :, p] = out
            source[t, p] = src
    return comp.reshape(T, C, H, W), count.reshape(T, H, W), source.reshape(T, H, W), hist


# name -> (H, W, candidates per step, C).  5 x 36: an int16 pitch of 72 bytes, 8 mod 16; 3 x 7: narrower than one vector; 17 x 129: more
# than one workgroup (2193 pixels) and an odd plane size, so every second plane starts at an odd element; 2 x 3660: the real pitch.
CASES = {
    "p36_c6": (5, 36, (1, 2, 3, 4, 5, 8, 15, 16, 0), 6),
    "p36_c1": (5, 36, (16, 0, 1, 5, 2), 1),
    "narrow_c6": (3, 7, (3, 16, 0, 1), 6),
    "narrow_c1": (3, 7, (4, 2, 15), 1),
    "blocks_c6": (17, 129, (5, 16), 6),
    "blocks_c1": (17, 129, (8, 3, 0), 1),
    "pitch_c6": (2, 3660, (8,), 6),
    "pitch_c5": (2, 3660, (3,), 5),  # a band count the kernel does not keep in registers
}


@functools.lru_cache(maxsize=None)
def case(name):
    """A packed stack: the int16 buffer starts with one padding element (so `bands[1:]` is one element off alignment and the offsets are
    relative to it), planes in shuffled order with gaps of 0 or 1 elements.  Values from a small set (ties in the median), whole pixels
    where every candidate is masked, Fmask 255, no_data in a single band of an otherwise clear candidate, two identical candidates (a tie in
    the medoid) and -32768 next to 32767 (a 16-bit difference would overflow)."""
    H, W, counts, C = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    HW, N = H * W, sum(counts)
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    planes = rng.choice(np.array([-32768, -5, 0, 1, 2, 3, 7, 100, 101, 32767], dtype=np.int16), size=(N, C, HW))
    planes[rng.random((N, C, HW)) < 0.3] = 50  # many duplicates
    nd_at = rng.random((N, C, HW)) < 0.04
    planes[nd_at] = ND  # no_data in single bands
    fm = rng.choice(np.array([0, 0, 0, 0, WATER, CLOUD, NEAR, SHADOW, CLOUD | SHADOW, 64, 255], dtype=np.uint8), size=(N, HW))
    dead = rng.random(HW) < 0.1
    fm[:, dead] = rng.choice(np.array([CLOUD, 255], dtype=np.uint8), size=(N, int(dead.sum())))  # every candidate masked
    for t in range(len(counts)):
        if counts[t] >= 3:  # candidates 0 and 2 of the step identical and clear on a stretch of pixels; -32768 / 32767 beside each other
            a, b = int(ptr[t]), int(ptr[t]) + 2
            sl = slice(0, max(HW // 3, 1))
            planes[a, :, sl] = np.where(planes[a, :, sl] == ND, 7, planes[a, :, sl])
            planes[b, :, sl] = planes[a, :, sl]
            fm[a, sl] = fm[b, sl] = 0
            planes[a + 1, :, sl] = np.where(np.arange(C)[:, None] % 2 == 0, -32768, 32767).astype(np.int16)
            fm[a + 1, sl] = 0
    order = rng.permutation(N * C)
    gaps = rng.integers(0, 2, size=N * C)
    starts = np.zeros(N * C, dtype=np.int64)
    at = 0
    for k, g in zip(order, gaps):
        at += int(g)
        starts[k] = at
        at += HW
    buf = np.full(at + 1, 12345, dtype=np.int16)
    for k in range(N * C):
        buf[1 + starts[k] : 1 + starts[k] + HW] = planes[k // C, k % C]
    forder = rng.permutation(N)
    fstarts = np.zeros(N, dtype=np.int64)
    at = 0
    for k in forder:
        at += int(rng.integers(0, 2))
        fstarts[k] = at
        at += HW
    fbuf = np.full(at + 1, 77, dtype=np.uint8)
    for k in range(N):
        fbuf[1 + fstarts[k] : 1 + fstarts[k] + HW] = fm[k]
    for a in (buf, fbuf, starts, fstarts, ptr):
        a.setflags(write=False)
    return dict(bands=buf, starts=starts, fmasks=fbuf, fmask_starts=fstarts, step_ptr=ptr, C=C, H=H, W=W)


@functools.lru_cache(maxsize=None)
def expected(name, method, min_clear=1, with_fmask=True):
    k = case(name)
    out = twin(k["bands"][1:], k["starts"], k["fmasks"][1:] if with_fmask else None, k["fmask_starts"], k["step_ptr"], k["C"], k["H"], k["W"],
               BITS, ND, min_clear, method)
    for a in out:
        a.setflags(write=False)
    return out
