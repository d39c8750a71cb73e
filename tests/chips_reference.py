"""Sequential twin of the chip-cutting rule of include/instageo_hip.h: one Python loop per pixel, written from the rule alone and sharing
nothing with instageo_amd/chips.py.  It is the oracle of the numpy host path and of the kernels (ig_chip_cut, ig_chip_labels); the cases
both test files use are built here too."""
import numpy as np

POSITIONS = {"cloud": 1, "near_cloud_or_shadow": 2, "cloud_shadow": 3, "water": 5}
# the reference's own table for decode_fmask_value: value 100, positions 0..7
FMASK_TABLE = {"value": 100, "bits": [0, 0, 1, 0, 0, 1, 1, 0]}


def decode_arithmetic(v: int, p: int) -> int:
    """The reference's arithmetic form: quotient = v // 2^p; quotient - (quotient // 2) * 2."""
    q = v // (2 ** p)
    return q - (q // 2) * 2


def cut(tile, fmask, origins, S, T, bits, strategy, nd=0, clip=None):
    """-> (chips (n, TC, S, S) int16, valid_values (n,) int32, validity (n, S, S) uint8)."""
    TC, H, W = tile.shape
    C = TC // T
    n = len(origins)
    chips = np.zeros((n, TC, S, S), dtype=np.int16)
    valid = np.zeros(n, dtype=np.int32)
    plane = np.zeros((n, S, S), dtype=np.uint8)
    for i, (r0, c0) in enumerate(origins):
        assert 0 <= r0 <= H - S and 0 <= c0 <= W - S
        for r in range(S):
            for c in range(S):
                masked = [fmask is not None and (int(fmask[t, r0 + r, c0 + c]) & bits) != 0 for t in range(T)]
                anyone = any(masked)
                nvalid = 0
                for b in range(TC):
                    v = int(tile[b, r0 + r, c0 + c])
                    if (strategy == "each" and masked[b // C]) or (strategy == "any" and anyone):
                        v = nd
                    if clip is not None:
                        v = min(max(v, clip[0]), clip[1])
                    chips[i, b, r, c] = v
                    nvalid += v != nd
                valid[i] += nvalid
                plane[i, r, c] = (1 if nvalid == TC else 0) | (2 if nvalid > 0 else 0)
    return chips, valid, plane


def label_maps(origins, S, ptr, pts, labels, w, validity, bit, K, dtype):
    """-> (maps (n, S, S) dtype, valid_labels (n,) int32, hist (n, K) int32 or None).  pts rows: (row, col, original index)."""
    n = len(origins)
    maps = np.full((n, S, S), -1, dtype=dtype)
    valid = np.zeros(n, dtype=np.int32)
    hist = np.zeros((n, K), dtype=np.int32) if K else None
    minus = np.array(-1, dtype=dtype)
    for i, (r0, c0) in enumerate(origins):
        mine = [tuple(int(v) for v in p) for p in pts[ptr[i] : ptr[i + 1]]]
        for r in range(S):
            for c in range(S):
                winner = -1
                for row, col, idx in mine:
                    if abs(r - (row - r0)) <= w and abs(c - (col - c0)) <= w and idx > winner:
                        winner = idx
                if winner < 0:
                    continue
                if bit and not (int(validity[i, r, c]) & bit):
                    continue
                maps[i, r, c] = labels[winner]
                if maps[i, r, c] != minus:
                    valid[i] += 1
                    if K and 0 <= int(maps[i, r, c]) < K:
                        hist[i, int(maps[i, r, c])] += 1
    return maps, valid, hist


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------
def make_tile(T, C, H, W, seed, fully_masked=None, untouched=None, S=32):
    """A tile with zeros (no data) sprinkled in, and an Fmask in which each of the four bits occurs alone, together with others and on only
    one date; ``fully_masked`` / ``untouched``: (row0, col0) of S x S windows that are masked on every date / on none."""
    rng = np.random.default_rng(seed)
    tile = rng.integers(-50, 12000, size=(T * C, H, W)).astype(np.int16)
    tile[rng.random(tile.shape) < 0.15] = 0
    tile[:, :3, :5] = 0  # a patch with no data in any band
    choices = np.array([0, 0, 0, 1, 64, 2, 4, 8, 32, 2 | 8, 4 | 32, 2 | 4 | 8 | 32, 255, 16], dtype=np.uint8)  # bits 0, 4, 6: never asked for
    fmask = choices[rng.integers(0, len(choices), size=(T, H, W))]
    if T > 1:
        fmask[1:, H // 2 :, : W // 3] = 0  # masked on date 0 only
        fmask[0, H // 2 :, : W // 3] = 2
    if fully_masked is not None:
        r, c = fully_masked
        fmask[:, r : r + S, c : c + S] = 2 | 32
    if untouched is not None:
        r, c = untouched
        fmask[:, r : r + S, c : c + S] = 1 | 16 | 64
    return tile, fmask


def random_points(origins, S, counts, seed, P=None, label_values=(-1, 0, 1, 2, 3, 7, 300)):
    """``counts[i]`` points inside chip i -> (ptr, pts (m, 3) int32 in stable original order per chip, labels (P,) int16).  The original
    indices are a random subset of range(P), so they are neither dense nor grouped by chip."""
    rng = np.random.default_rng(seed)
    m = int(sum(counts))
    P = P or 2 * m + 3
    idx = np.sort(rng.choice(P, size=m, replace=False))
    owner = rng.permutation(np.repeat(np.arange(len(origins)), counts))  # chip of the k-th index
    rows, ptr = [], [0]
    for i, (r0, c0) in enumerate(origins):
        for k in np.nonzero(owner == i)[0]:
            rows.append((r0 + int(rng.integers(0, S)), c0 + int(rng.integers(0, S)), int(idx[k])))
        ptr.append(len(rows))
    labels = np.array(label_values, dtype=np.int16)[rng.integers(0, len(label_values), size=P)]
    return np.array(ptr, dtype=np.int32), np.array(rows, dtype=np.int32).reshape(-1, 3), labels
