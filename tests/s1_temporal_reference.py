"""Sequential twin of the multi-temporal speckle rule of include/instageo_hip.h (``ig_s1_temporal``), written pixel by pixel from the header's
text with Python floats (IEEE float64, every operation rounded on its own): independent of the vectorised host path of
instageo_amd/s1_temporal.py.  ``log10`` is numpy's, the function the host path calls.  Also the packed test stacks both suites share, and
cached expectations."""
import functools
import math

import numpy as np

QNAN = 0x7FC00000
SND = -32768.0
LOOKS = 4.4


def _present(f, snd):
    return math.isfinite(f) and (snd is None or np.float32(f) != np.float32(snd))


def local_means(plane, H, W, h, snd):
    """-> per pixel of a plane (m, x) where the centre is present, else None.  m = A / n over the window clipped to the plane: per window
    row left to right over the present values from +0.0, then the rows top to bottom from +0.0."""
    x = [[float(v) for v in row] for row in plane.reshape(H, W).tolist()]
    ok = [[_present(v, snd) for v in row] for row in x]
    rows = {}

    def row_moment(i, c):
        if (i, c) not in rows:
            A, K = 0.0, 0
            for j in range(max(c - h, 0), min(c + h, W - 1) + 1):  # left to right
                if ok[i][j]:
                    A += x[i][j]
                    K += 1
            rows[(i, c)] = (A, K)
        return rows[(i, c)]

    means = []
    for r in range(H):
        line = []
        for c in range(W):
            if not ok[r][c]:
                line.append(None)
                continue
            A, n = 0.0, 0
            for i in range(max(r - h, 0), min(r + h, H - 1) + 1):  # top to bottom
                Ai, Ki = row_moment(i, c)
                A += Ai
                n += Ki
            line.append((A / float(n), x[r][c]))
        means.append(line)
    return means


def twin(planes, starts, sizes, group, date, offsets, h, snd, to_db, means=None):
    """-> (out as uint32 bit views with the layout of planes, elements outside every plane 0; counts (N, 4) int32).  ``means``: the
    planes' :func:`local_means` where they are at hand."""
    N = len(starts)
    out = np.zeros(planes.shape[0], dtype=np.uint32)
    counts = np.zeros((N, 4), dtype=np.int32)
    if means is None:
        means = [local_means(planes[int(at) : int(at) + H * W], H, W, h, snd) for at, (H, W) in zip(starts, sizes)]
    for g in sorted(set(int(v) for v in group)):
        mem = sorted((p for p in range(N) if int(group[p]) == g), key=lambda p: (int(date[p]), p))  # by date, then the order given
        Hg = max(int(offsets[p][0]) + sizes[p][0] for p in mem)
        Wg = max(int(offsets[p][1]) + sizes[p][1] for p in mem)
        for r in range(Hg):
            for c in range(Wg):
                R, cnt, taken = 0.0, 0, set()
                at = {}  # plane -> (m, x) of the planes that cover the pixel and are present there
                for p in mem:
                    pr, pc = r - int(offsets[p][0]), c - int(offsets[p][1])
                    if not (0 <= pr < sizes[p][0] and 0 <= pc < sizes[p][1]):
                        continue
                    v = means[p][pr][pc]
                    if v is not None:
                        at[p] = v
                        if int(date[p]) not in taken:  # the first present member of the date decides for it
                            taken.add(int(date[p]))
                            if v[0] > 0:
                                R += v[1] / v[0]
                                cnt += 1
                for p in mem:
                    pr, pc = r - int(offsets[p][0]), c - int(offsets[p][1])
                    if not (0 <= pr < sizes[p][0] and 0 <= pc < sizes[p][1]):
                        continue
                    k = int(starts[p]) + pr * sizes[p][1] + pc
                    if p not in at:
                        out[k] = QNAN
                        continue
                    m, x = at[p]
                    if m > 0 and cnt >= 1:
                        y = m * (R / float(cnt))
                    else:
                        y = x
                        counts[p, 2] += 1
                    if to_db:
                        if not y > 0:
                            counts[p, 1] += 1
                            out[k] = QNAN
                            continue
                        y = 10.0 * float(np.log10(np.float64(y)))
                    with np.errstate(over="ignore"):
                        out[k] = np.array([y], dtype=np.float64).astype(np.float32).view(np.uint32)[0]
                    counts[p, 0] += 1
                    counts[p, 3] += cnt == 1
    return out, counts


# ---- the stacks ----------------------------------------------------------------------------------------------------------------------------
# (group, date, (H, W), (row0, col0)) per plane, in the order of the buffer.  Group 0: three dates; the lattice is 42 x 80 (more than one tile
# of 64 columns x 32 rows both ways, ragged); date 1 has a second orbit slice, given after the first, that overlaps it and reaches past it.
# Group 1: a 1 x 1 plane alone on its date, a plane one row and one column past a tile (33 x 65) and one of 65 x 33 (two tiles and a row).
STACK = ((0, 0, (37, 70), (0, 0)), (0, 1, (33, 66), (5, 3)), (0, 2, (40, 65), (2, 0)), (0, 1, (20, 30), (10, 50)), (1, 0, (1, 1), (0, 0)),
         (1, 3, (33, 65), (0, 0)), (1, 4, (65, 33), (0, 0)))
RUNS = ((1, True), (3, False), (7, True))  # (h, src_nodata given): without it -32768 is a value, and most local means are negative


def _plane(rng, H, W, level):
    a = (level * rng.gamma(LOOKS, 1.0 / LOOKS, size=(H, W))).astype(np.float32)
    if H * W > 1:
        a[rng.random((H, W)) < 0.04] = SND
        a[rng.random((H, W)) < 0.04] = np.nan
        a[rng.random((H, W)) < 0.03] *= -1.0
        a[H - 1, W - 1] = np.inf
        a[0, W // 2] = -np.inf
        a[H // 2, 2 : W // 2] = np.nan  # a run of absent pixels wider than the smallest window
    return a


@functools.lru_cache(maxsize=None)
def stack():
    """-> {planes (with one leading element, so a view from element 1 starts 4-byte but not 16-byte aligned), starts, sizes, group, date,
    offsets}.  NaN holes, +-inf, src_nodata values and negative values everywhere; plane 0 holds a 9 x 9 patch of zeros (m = 0 at its
    centre for h <= 4, a passthrough) and plane 1 a patch of negatives (m < 0)."""
    rng = np.random.default_rng(2024)
    planes = [_plane(rng, H, W, 10.0 ** rng.uniform(-2, 1)) for _, _, (H, W), _ in STACK]
    planes[0][12:21, 20:29] = 0.0
    planes[1][20:27, 40:47] = -np.abs(planes[1][20:27, 40:47])
    starts = np.concatenate([[0], np.cumsum([p.size for p in planes])[:-1]]).astype(np.int64)
    flat = np.concatenate([np.zeros(1, dtype=np.float32)] + [p.reshape(-1) for p in planes])
    flat.setflags(write=False)
    starts.setflags(write=False)
    return {"planes": flat, "starts": starts, "sizes": [s for _, _, s, _ in STACK], "group": [g for g, _, _, _ in STACK],
            "date": [d for _, d, _, _ in STACK], "offsets": [o for _, _, _, o in STACK]}


@functools.lru_cache(maxsize=None)
def _means(h, with_snd):
    k = stack()
    flat = k["planes"][1:]
    return [local_means(flat[int(at) : int(at) + H * W], H, W, h, SND if with_snd else None) for at, (H, W) in zip(k["starts"], k["sizes"])]


@functools.lru_cache(maxsize=None)
def expected(h, with_snd, scale):
    """The twin's result on :func:`stack`, computed once: (bits uint32 with the layout of the planes, counts)."""
    k = stack()
    out, counts = twin(k["planes"][1:], k["starts"], k["sizes"], k["group"], k["date"], k["offsets"], h, SND if with_snd else None, scale == "db",
                       _means(h, with_snd))
    out.setflags(write=False)
    counts.setflags(write=False)
    return out, counts


def bits_of(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def ulps(got_bits, want_bits):
    """The largest difference of the int32 bit views over the elements that are finite on both sides (0 when there is none)."""
    g, w = got_bits.view(np.int32).astype(np.int64), want_bits.view(np.int32).astype(np.int64)
    fin = np.isfinite(got_bits.view(np.float32)) & np.isfinite(want_bits.view(np.float32))
    return int(np.abs(g - w)[fin].max()) if fin.any() else 0


def gamma_stack(seed, D=4, side=96, means=(0.02, 0.05, 0.11, 0.3, 0.07, 0.2, 0.9, 0.4)):
    """D homogeneous planes of side x side with gamma speckle of 4.4 looks and different means, on one lattice -> the arguments of a run."""
    rng = np.random.default_rng(seed)
    planes = np.concatenate([(means[d] * rng.gamma(LOOKS, 1.0 / LOOKS, size=side * side)).astype(np.float32) for d in range(D)])
    return planes, np.arange(D, dtype=np.int64) * side * side, [(side, side)] * D, [0] * D, list(range(D)), [(0, 0)] * D
