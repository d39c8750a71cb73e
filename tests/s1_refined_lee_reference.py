"""Sequential twin of the refined Lee rule of include/instageo_hip.h (``ig_s1_refined_lee``), written pixel by pixel from the header's
text with Python floats (IEEE float64, every operation rounded on its own): independent of the vectorised host path of
instageo_amd/s1_filter.py.  ``log10`` is numpy's, the function the host path calls.  The planes are the shared cases of
tests/s1_filter_reference.py; expectations are computed once and cached.

``trace`` (a dict, optional) counts what the rule did: ``homogeneous``, ``fallback``, ``mask_SE`` .. ``mask_N``, ``tie_gradient_d1`` ..
(the largest gradient was shared and the named one, the first in the order, won) and ``tie_half_d1`` .. (the two halves of the winning
pair were equally close to the centre mean and the first-named won)."""
import functools

import numpy as np

import s1_filter_reference as R

H3 = 3
PAIRS = ("d1", "d2", "h", "v")
HALVES = (("SE", "NW"), ("NE", "SW"), ("E", "W"), ("S", "N"))
IN_MASK = {"E": lambda dy, dx: dx >= 0, "W": lambda dy, dx: dx <= 0, "S": lambda dy, dx: dy >= 0, "N": lambda dy, dx: dy <= 0,
           "SE": lambda dy, dx: dx + dy >= 0, "NW": lambda dy, dx: dx + dy <= 0, "NE": lambda dy, dx: dx - dy >= 0,
           "SW": lambda dy, dx: dx - dy <= 0}


def _note(trace, key):
    if trace is not None:
        trace[key] = trace.get(key, 0) + 1


def _lee_terms(A, Q, n, s):
    m = A / n
    v = Q / n - m * m
    if v < 0:
        v = 0.0
    t = (m * m) * s
    vx = (v - t) / (1.0 + s)
    return m, v, vx


def plane_values(plane, H, W, looks, snd, trace=None):
    """-> per pixel y (a Python float), or None where the centre is absent."""
    x = [[float(v) for v in row] for row in plane.reshape(H, W).tolist()]
    ok = [[R._present(v, snd) for v in row] for row in x]
    s = 1.0 / float(np.float32(looks))
    means = {}

    def sub_mean(cr, cc):
        """The mean of the 3 x 3 window centred at (cr, cc), clipped to the plane; None when nothing in it is present."""
        if (cr, cc) not in means:
            A3, n3 = 0.0, 0
            for i in range(max(cr - 1, 0), min(cr + 1, H - 1) + 1):  # top to bottom
                Ar = 0.0
                for j in range(max(cc - 1, 0), min(cc + 1, W - 1) + 1):  # left to right
                    if ok[i][j]:
                        Ar += x[i][j]
                        n3 += 1
                A3 += Ar
            means[(cr, cc)] = A3 / n3 if n3 else None
        return means[(cr, cc)]

    ys = []
    for r in range(H):
        for c in range(W):
            if not ok[r][c]:
                ys.append(None)
                continue
            xc = x[r][c]
            # 1 the full window
            A, Q, n = 0.0, 0.0, 0
            for i in range(max(r - H3, 0), min(r + H3, H - 1) + 1):
                Ai, Qi, Ki = 0.0, 0.0, 0
                for j in range(max(c - H3, 0), min(c + H3, W - 1) + 1):
                    if ok[i][j]:
                        Ai += x[i][j]
                        Qi += x[i][j] * x[i][j]
                        Ki += 1
                A += Ai
                Q += Qi
                n += Ki
            m, v, vx = _lee_terms(A, Q, n, s)
            if not (v > 0 and vx > 0):
                _note(trace, "homogeneous")
                ys.append(m)
                continue
            # 2 the sub-window means
            M = [[sub_mean(r + 2 * (i - 1), c + 2 * (j - 1)) for j in range(3)] for i in range(3)]
            if any(M[i][j] is None for i in range(3) for j in range(3)):
                _note(trace, "fallback")
                ys.append(m + (vx / v) * (xc - m))
                continue
            # 3 the direction
            c0 = M[1][1]
            g = (abs((M[1][2] + M[2][1] + M[2][2]) - (M[0][0] + M[0][1] + M[1][0])),
                 abs((M[0][1] + M[0][2] + M[1][2]) - (M[1][0] + M[2][0] + M[2][1])),
                 abs((M[0][2] + M[1][2] + M[2][2]) - (M[0][0] + M[1][0] + M[2][0])),
                 abs((M[2][0] + M[2][1] + M[2][2]) - (M[0][0] + M[0][1] + M[0][2])))
            k = g.index(max(g))  # the first of the largest
            if g.count(g[k]) > 1:
                _note(trace, "tie_gradient_" + PAIRS[k])
            near, far = ((M[2][2], M[0][0]), (M[0][2], M[2][0]), (M[1][2], M[1][0]), (M[2][1], M[0][1]))[k]
            if abs(near - c0) == abs(far - c0):
                _note(trace, "tie_half_" + PAIRS[k])
            name = HALVES[k][0] if abs(near - c0) <= abs(far - c0) else HALVES[k][1]
            _note(trace, "mask_" + name)
            inside = IN_MASK[name]
            # 4 the half window
            A, Q, n = 0.0, 0.0, 0
            for dy in range(-3, 4):
                Ai, Qi = 0.0, 0.0
                i = r + dy
                if 0 <= i < H:
                    for dx in range(-3, 4):
                        j = c + dx
                        if 0 <= j < W and inside(dy, dx) and ok[i][j]:
                            Ai += x[i][j]
                            Qi += x[i][j] * x[i][j]
                            n += 1
                A += Ai
                Q += Qi
            m, v, vx = _lee_terms(A, Q, n, s)
            b = vx / v if v > 0 and vx > 0 else 0.0
            ys.append(m + b * (xc - m))
    return ys


def finish(ys, to_db):
    """-> (the uint32 bit views of the outputs, present, dropped) of one plane."""
    bits = np.full(len(ys), R.QNAN, dtype=np.uint32)
    present = dropped = 0
    for k, y in enumerate(ys):
        if y is None:
            continue
        if to_db:
            if not y > 0:
                dropped += 1
                continue
            y = 10.0 * float(np.log10(np.float64(y)))
        with np.errstate(over="ignore"):
            bits[k] = np.array([y], dtype=np.float64).astype(np.float32).view(np.uint32)[0]
        present += 1
    return bits, present, dropped


def twin(planes, starts, sizes, looks, snd, to_db, trace=None):
    """-> (out as uint32 bit views with the layout of planes, elements outside every plane 0; counts (N, 2) int32)."""
    out = np.zeros(planes.shape[0], dtype=np.uint32)
    counts = np.zeros((len(starts), 2), dtype=np.int32)
    for p, (at, (H, W)) in enumerate(zip(starts, sizes)):
        at = int(at)
        bits, counts[p, 0], counts[p, 1] = finish(plane_values(planes[at : at + H * W], H, W, looks, snd, trace), to_db)
        out[at : at + H * W] = bits
    return out, counts


@functools.lru_cache(maxsize=None)
def _values(name, positive, with_snd):
    """The y of every pixel of a shared case and the trace of the run, computed once."""
    k = R.case(name, positive)
    flat = k["planes"][1:]
    trace = {}
    ys = [plane_values(flat[int(at) : int(at) + H * W], H, W, R.LOOKS, R.SND if with_snd else None, trace) for at, (H, W) in zip(k["starts"], k["sizes"])]
    return ys, trace


def trace_of(name, positive, with_snd):
    return dict(_values(name, positive, with_snd)[1])


@functools.lru_cache(maxsize=None)
def expected(name, positive, with_snd, scale):
    """The twin's result for a shared case, computed once: (bits uint32 with the layout of the planes, counts)."""
    k = R.case(name, positive)
    out = np.zeros(k["planes"].shape[0] - 1, dtype=np.uint32)
    counts = np.zeros((len(k["sizes"]), 2), dtype=np.int32)
    for p, (ys, at, (H, W)) in enumerate(zip(_values(name, positive, with_snd)[0], k["starts"], k["sizes"])):
        out[int(at) : int(at) + H * W], counts[p, 0], counts[p, 1] = finish(ys, scale == "db")
    out.setflags(write=False)
    counts.setflags(write=False)
    return out, counts


# ---- noiseless steps: a plane of two levels split by a line -----------------------------------------------------------------------------
STEP_SIDE, STEP_LOW, STEP_HIGH, STEP_LOOKS = 24, 1.0, 16.0, 10000.0


@functools.lru_cache(maxsize=None)
def steps():
    """Every 24 x 24 plane of 1.0 and 16.0 split by a vertical line, a horizontal line or one of the two 45-degree staircases, at every
    offset that leaves both levels in the plane -> (names, planes packed, starts, sizes)."""
    n = STEP_SIDE
    r, c = np.mgrid[0:n, 0:n]
    names, planes = [], []
    for kind, field, offsets in (("vertical", c, range(1, n)), ("horizontal", r, range(1, n)), ("diagonal", r + c, range(1, 2 * n - 1)),
                                 ("antidiagonal", r - c, range(-(n - 2), n))):
        for k in offsets:
            names.append(f"{kind} {k}")
            planes.append(np.where(field >= k, STEP_HIGH, STEP_LOW).astype(np.float32).reshape(-1))
    flat = np.concatenate(planes)
    starts = np.arange(len(planes), dtype=np.int64) * n * n
    flat.setflags(write=False)
    return names, flat, starts, [(n, n)] * len(planes)
