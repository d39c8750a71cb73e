"""Host reference of the vectorisation (numpy + plain Python): a SEQUENTIAL tracer that walks every ring edge by edge with the linking
rule of include/instageo_hip.h, on breadth-first labels of its own -- no scan, no pointer jumping, no atomics -- and two checkers that
know nothing of the rule: ring areas against pixel counts, and an even-odd scanline fill of the rings against the region's pixels.
Used by test_cpu_vectorize.py and test_gpu_vectorize.py, which also share the test maps at the end."""
import functools
from collections import deque

import numpy as np

import regions_reference as RR

D = ((0, 1), (1, 0), (0, -1), (-1, 0))  # E, S, W, N as (dr, dc)


def bfs_label(cm, connectivity=4, fill=-1):
    """(H, W) int8 -> (H, W) int64: the smallest row-major index of the pixel's component (the first pixel a row-major scan meets), -1 at
    fill."""
    H, W = cm.shape
    lab = np.full((H, W), -1, dtype=np.int64)
    nb = D + (((-1, -1), (-1, 1), (1, -1), (1, 1)) if connectivity == 8 else ())
    for r0 in range(H):
        for c0 in range(W):
            if cm[r0, c0] == fill or lab[r0, c0] >= 0:
                continue
            me, root = cm[r0, c0], r0 * W + c0
            lab[r0, c0] = root
            todo = deque([(r0, c0)])
            while todo:
                r, c = todo.popleft()
                for dr, dc in nb:
                    rr, cc = r + dr, c + dc
                    if 0 <= rr < H and 0 <= cc < W and lab[rr, cc] < 0 and cm[rr, cc] == me:
                        lab[rr, cc] = root
                        todo.append((rr, cc))
    return lab


def shoelace2(v):
    """Twice the signed area of the polygon with vertices v (k, 2), closed implicitly."""
    x, y = v[:, 0].astype(np.int64), v[:, 1].astype(np.int64)
    return int((x * np.roll(y, -1) - np.roll(x, -1) * y).sum())


def _trace_image(cm, connectivity, fill):
    """-> [(label, cls, twice_area, root edge id within the image, vertices (k, 2))] of one image, unordered."""
    H, W = cm.shape
    lab = bfs_label(cm, connectivity, fill)

    def at(r, c):
        return int(lab[r, c]) if 0 <= r < H and 0 <= c < W else -1

    def live(r, c, s):
        dr, dc = D[(s + 3) % 4]
        return at(r, c) >= 0 and at(r + dr, c + dc) != at(r, c)

    seen = set()
    out = []
    for r0 in range(H):
        for c0 in range(W):
            for s0 in range(4):
                if (r0, c0, s0) in seen or not live(r0, c0, s0):
                    continue
                me = at(r0, c0)
                walk = []  # (heading, tail x, tail y), from the root edge (the scan meets a ring at its smallest edge id)
                r, c, s = r0, c0, s0
                while True:
                    assert live(r, c, s) and (r, c, s) not in seen, "the successor of a live edge is live and rings are disjoint"
                    seen.add((r, c, s))
                    walk.append((s, c + (s in (1, 2)), r + (s >= 2)))
                    left = (s + 3) % 4
                    ar, ac = r + D[s][0], c + D[s][1]
                    br, bc = ar + D[left][0], ac + D[left][1]
                    if at(br, bc) == me:
                        r, c, s = br, bc, left
                    elif at(ar, ac) == me:
                        r, c = ar, ac
                    else:
                        s = (s + 1) % 4
                    if (r, c, s) == (r0, c0, s0):
                        break
                v = np.array([(x, y) for k, (h, x, y) in enumerate(walk) if walk[k - 1][0] != h], dtype=np.int32)
                out.append((me, int(cm[r0, c0]), shoelace2(v), (r0 * W + c0) * 4 + s0, v))
    return out


def ref_rings(cms, connectivity=4, fill=-1):
    """(H, W) | (n, H, W) int8 -> (rings (R, 6) int64 [image, label, cls, n_vertices, twice_area, first], vertices (V, 2) int32), rows
    ordered by (image, label, hole, root edge): vectorize.region_rings' contract."""
    cms = np.asarray(cms)
    if cms.ndim == 2:
        cms = cms[None]
    rows, verts, first = [], [], 0
    for i, cm in enumerate(cms):
        for label, cls, a2, root, v in sorted(_trace_image(cm, connectivity, fill), key=lambda t: (t[0], t[2] < 0, t[3])):
            rows.append((i, label, cls, len(v), a2, first))
            verts.append(v)
            first += len(v)
    if not rows:
        return np.zeros((0, 6), dtype=np.int64), np.zeros((0, 2), dtype=np.int32)
    return np.array(rows, dtype=np.int64), np.concatenate(verts).astype(np.int32)


def _regions(rings):
    """{(image, label): [ring rows]} in row order."""
    out = {}
    for i, row in enumerate(rings):
        out.setdefault((int(row[0]), int(row[1])), []).append(i)
    return out


def check_areas(rings, vertices, cms, connectivity=4, fill=-1):
    """(a) every region of the maps has rings, exactly one of them positive; the shoelace sums of a region's rings (recomputed from the
    vertices) equal twice its pixel count, and the twice_area column holds them."""
    cms = np.asarray(cms)
    if cms.ndim == 2:
        cms = cms[None]
    regs = _regions(rings)
    want = {}
    for i, cm in enumerate(cms):
        lab = bfs_label(cm, connectivity, fill)
        roots, counts = np.unique(lab[lab >= 0], return_counts=True)
        want.update({(i, int(r)): int(k) for r, k in zip(roots, counts)})
    assert set(regs) == set(want), "the rings' regions are not the regions of the map"
    for key, idx in regs.items():
        areas = []
        for i in idx:
            a, k = int(rings[i, 5]), int(rings[i, 3])
            assert k >= 4
            areas.append(shoelace2(vertices[a:a + k]))
            assert areas[-1] == rings[i, 4] and areas[-1] != 0
        assert sum(a > 0 for a in areas) == 1 and areas[0] > 0, (key, areas)
        assert sum(areas) == 2 * want[key], (key, areas, want[key])
    assert int(rings[:, 3].sum()) == len(vertices) and (len(rings) == 0 or np.array_equal(rings[:, 5], np.cumsum(rings[:, 3]) - rings[:, 3]))


def check_fill(rings, vertices, cms, connectivity=4, fill=-1):
    """(b) an even-odd scanline fill of a region's rings reproduces exactly that region's pixels: a pixel (r, c) is inside iff an odd
    number of vertical ring edges at x <= c span its row."""
    cms = np.asarray(cms)
    if cms.ndim == 2:
        cms = cms[None]
    labs = [bfs_label(cm, connectivity, fill) for cm in cms]
    for (image, label), idx in _regions(rings).items():
        segs = []
        for i in idx:
            a, k = int(rings[i, 5]), int(rings[i, 3])
            v = vertices[a:a + k].astype(np.int64)
            w = np.roll(v, -1, axis=0)
            assert ((v[:, 0] == w[:, 0]) ^ (v[:, 1] == w[:, 1])).all(), "every ring edge is axis-parallel and not empty"
            vert = v[:, 0] == w[:, 0]
            segs.append(np.stack([v[vert, 0], np.minimum(v[vert, 1], w[vert, 1]), np.maximum(v[vert, 1], w[vert, 1])], axis=1))
        segs = np.concatenate(segs)
        x0, x1, y0, y1 = segs[:, 0].min(), segs[:, 0].max(), segs[:, 1].min(), segs[:, 2].max()
        cross = np.zeros((y1 - y0, x1 - x0 + 1), dtype=np.int64)
        for x, ya, yb in segs:
            cross[ya - y0:yb - y0, x - x0] += 1
        inside = (np.cumsum(cross, axis=1)[:, :-1] & 1).astype(bool)
        mine = labs[image] == label
        box = np.zeros_like(mine)
        box[y0:y1, x0:x1] = inside
        assert np.array_equal(box, mine), (image, label)


def is_simple(v):
    """No vertex of the ring is visited twice (a ring of axis-parallel unit-lattice edges that touches itself does so at a vertex)."""
    return len({(int(x), int(y)) for x, y in v}) == len(v)


# ---- test maps -------------------------------------------------------------------------------------------------------------------------
def _cm(rows):
    """'.' = fill (-1), digits = classes."""
    return np.array([[-1 if ch == "." else int(ch) for ch in r] for r in rows], dtype=np.int8)


def spiral(S):
    """A one-pixel-wide corridor of class 1 that winds inwards clockwise from (0, 0) between one-pixel walls of class 0: one region of
    class 1 and one of class 0, each with a single ring of several thousand edges at S = 96."""
    cm = np.zeros((S, S), dtype=np.int8)
    r, c, d = 0, 0, 0
    cm[0, 0] = 1

    def can(r, c, d):
        r1, c1, r2, c2 = r + D[d][0], c + D[d][1], r + 2 * D[d][0], c + 2 * D[d][1]
        if not (0 <= r1 < S and 0 <= c1 < S) or cm[r1, c1]:
            return False
        return not (0 <= r2 < S and 0 <= c2 < S) or cm[r2, c2] == 0

    while True:
        if not can(r, c, d):
            d = (d + 1) % 4
            if not can(r, c, d):
                return cm
        r, c = r + D[d][0], c + D[d][1]
        cm[r, c] = 1


def comb(H, W):
    cm = np.zeros((H, W), dtype=np.int8)
    cm[0, :] = 1
    cm[:, ::2] = 1
    return cm


def bar(length):
    """A 1 x length bar of class 2 in a frame of fill: the map's only ring has 2 * length + 2 edges."""
    cm = np.full((3, length + 2), -1, dtype=np.int8)
    cm[1, 1:-1] = 2
    return cm


def noise_with_fill(H, W, ncls, seed, fill_frac=0.1):
    rng = np.random.default_rng(seed)
    cm = rng.integers(0, ncls, size=(H, W)).astype(np.int8)
    cm[rng.random((H, W)) < fill_frac] = -1
    return cm


@functools.lru_cache(maxsize=None)
def cases():
    """{name: (H, W) | (n, H, W) int8}, read-only: the smallest maps that can break each stage (the mask kernel takes 4 pixels per thread
    and 1024 per workgroup)."""
    c = {
        "1x1": _cm(["3"]),
        "1x7": _cm(["0011.10"]),
        "7x1": _cm(["0011.10"]).T.copy(),
        "all_fill": np.full((4, 5), -1, dtype=np.int8),
        "checker_2x2": RR.checkerboard(2, 2),
        "checker_5x5": RR.checkerboard(5, 5),
        "ring_3x3": _cm(["111", "101", "111"]),
        "ring_3x3_fill_hole": _cm(["111", "1.1", "111"]),
        "hole_at_exterior_corner": _cm(["111", "101", "110"]),  # the diagonal pair (1, 2), (2, 1) is one component through the detour
        "diagonal_pair_alone": _cm(["0000", "0100", "0010", "0000"]),  # two regions under 4, one under 8
        "diagonal_pair_with_detour": _cm(["11111", "11011", "10111", "11111", "11111"]),  # two holes that meet at a corner
        "spiral_96": spiral(96),
        "comb": comb(9, 17),
        "blobs_65x17": RR.blobs(65, 17, 3, 1),
        "blobs_130x40": RR.blobs(130, 40, 4, 2),
        "blobs_37x53": RR.blobs(37, 53, 2, 3),
        "blobs_33x31_x3": np.stack([RR.blobs(33, 31, 3, 4), RR.noise(33, 31, 2, 5), RR.blobs(33, 31, 5, 6, fill_frac=0.2)]),
        "noise_128": noise_with_fill(128, 128, 3, 7),
        "bar_64_edges": bar(31),  # E = the ring's edges = 2^6: the last of the ceil(log2 E) rounds is needed
        "bar_66_edges": bar(32),  # a closed lattice walk has an even number of edges: 2^6 + 2 is the next ring after 2^6
    }
    for v in c.values():
        v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def reference(name, connectivity):
    rings, vertices = ref_rings(cases()[name], connectivity)
    rings.setflags(write=False)
    vertices.setflags(write=False)
    return rings, vertices
