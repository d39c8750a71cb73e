"""Bit-exact parity tests (-m gpu) on exactly representable operands.

Part A pins the conversion layer (``ig_split_bf16`` / ``ig_merge_bf16`` and the ``store4_split`` users) against a reference that is computed with
torch on the CPU and never touches the library.  Part B runs every linear-algebra entry point, on every engine route, on operands that are small
integers times a power of two: every product and every partial sum is then exact in fp32 in ANY accumulation order, the fp32 accumulator is
known exactly, and the stored output must equal RNE(exact) bit for bit.  Tolerances are zero.

The exactness is a CONDITION, not a measurement: for every output element the sum of |term| (+ |bias| + |residual| + |initial buffer|), in units
of the smallest term, must stay below 2^24.  ``budget`` of every case is asserted before the kernel runs and by tests/test_cpu_exact_operands.py
for every parametrised shape.  Operands are uploaded as bf16 bit patterns and outputs are read back as bit patterns: ``BT.from_float`` and
``BT.float`` are not part of the measuring stick here.

The split (bf16x3) mode forms hi*hi + hi*lo + lo*hi and omits lo*lo in every engine (common.h, gemm.hip seg_a / seg_b, conv_direct.hip,
gemm8w.hip): the split reference is the float64 sum of exactly those products.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from instageo_amd import ops  # noqa: E402
from instageo_amd.ops import BT  # noqa: E402

DEV = "cuda"
BF16 = torch.bfloat16
LIMIT = float(2**24)


# =====================================================================================================================================
# The reference of part A: torch on the CPU only
# =====================================================================================================================================
def split_ref(x32):
    """(hi, lo) bf16 of an fp32 CPU tensor: hi = RNE(x), lo = RNE(x - hi)."""
    assert x32.dtype == torch.float32 and not x32.is_cuda
    hi = x32.to(BF16)
    lo = (x32 - hi.float()).to(BF16)
    return hi, lo


def merged_ref(hi, lo):
    return hi.float() + lo.float()


def bits16(t):
    return t.contiguous().view(torch.int16)


def f32_from_bits(bits_u32):
    return torch.from_numpy(np.ascontiguousarray(bits_u32, dtype=np.uint32).view(np.float32).copy())


def _uppers():
    """A few hundred upper halves (positive) spread over the normal exponent range, even and odd last bits."""
    ups = []
    for e in list(range(1, 255, 6)) + [254]:
        for m in (0x00, 0x01, 0x02, 0x40, 0x41, 0x7E, 0x7F):
            ups.append((e << 7) | m)
    return np.array(sorted(set(ups)), dtype=np.uint32)


def special_fp32_bits():
    """The fp32 bit patterns of part A (normal, zero and non-finite inputs; the subnormals are ``subnormal_fp32_bits``)."""
    pats = np.arange(65536, dtype=np.uint32)
    exp = (pats >> 7) & 0xFF
    keep = ~((exp == 0) & ((pats & 0x7F) != 0))  # bf16 subnormals widen to fp32 subnormals: the other vector
    out = [pats[keep] << 16]
    ups = _uppers()
    for low in (0x7FFF, 0x8000, 0x8001, 0x0001, 0xFFFF):
        for sign in (0, 0x80000000):
            out.append((ups << 16) | np.uint32(low) | np.uint32(sign))
    # lo itself a tie: the residual has nine significant bits, the ninth set (kept last bit even / odd), hi rounding down and up
    mid = ups[(ups >> 7) >= 40]  # keep the residual (2^-16 of the value at the smallest) a normal number
    for low in (0x4040, 0x40C0, 0x2020, 0x2060, 0x0101, 0x0103, 0xBFC0, 0xBF40, 0xDFE0, 0xDFA0, 0xFEFF, 0xFEFD):
        for sign in (0, 0x80000000):
            out.append((mid << 16) | np.uint32(low) | np.uint32(sign))
    out.append(np.array([0x7F7FFFFF, 0xFF7FFFFF,   # the largest finite fp32
                         0x7F7F7FFF, 0xFF7F7FFF,   # the largest value that still rounds to a finite bf16
                         0x7F7F8000, 0xFF7F8000,   # the tie above it: rounds to infinity
                         0x00800000, 0x80800000,   # the smallest normal fp32
                         0x00800001, 0x00FFFFFF,
                         0x7F800000, 0xFF800000,   # +-inf
                         0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0xFFBFFFFF], dtype=np.uint32))  # NaNs
    return np.concatenate(out).astype(np.uint32)


def subnormal_fp32_bits():
    pats = np.arange(65536, dtype=np.uint32)
    exp = (pats >> 7) & 0xFF
    sub = pats[(exp == 0) & ((pats & 0x7F) != 0)] << 16
    extra = np.array([0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00010000, 0x00018000, 0x00400000, 0x007F8000, 0x007FFFFF], dtype=np.uint32)
    return np.concatenate([sub, extra, extra | np.uint32(0x80000000)]).astype(np.uint32)


def finite_split_values():
    """The inputs of ``special_fp32_bits`` whose reference (hi, lo) are finite and whose residual is not subnormal, in a fixed shuffled order."""
    x = f32_from_bits(special_fp32_bits())
    hi, lo = split_ref(x)
    res = (x - hi.float()).abs()
    ok = torch.isfinite(hi.float()) & torch.isfinite(lo.float()) & ((res == 0) | (res >= 2.0**-126)) & ((x == 0) | (x.abs() >= 2.0**-126))
    x = x[ok]
    g = torch.Generator().manual_seed(7)
    return x[torch.randperm(x.numel(), generator=g)]


SPLIT_LENGTHS = [1, 2, 3, 7, 8, 9, 255, 257, 16384 * 256 + 5]  # the last: the grid-stride loop (16384 blocks of TPB = 256) takes a second trip


# =====================================================================================================================================
# Exact operand generators of part B (imported by tests/test_cpu_exact_operands.py)
# =====================================================================================================================================
X_HI, X_LO = 2.0**-3, 2.0**-13   # the "activation" operand: i 2^-3 + e 2^-13
W_HI, W_LO = 2.0**-4, 2.0**-14   # the "weight" operand:     j 2^-4 + f 2^-14
U_PLAIN = X_HI * W_HI            # smallest plain product: 2^-7; bias, residual and initial buffers are multiples of it
U_SPLIT = X_HI * W_LO            # smallest split product: 2^-17 (= X_LO * W_HI)


def _ints(shape, seed, lo, hi, nonzero=False):
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(lo, hi + 1, tuple(shape), generator=g)
    if nonzero:  # 0 -> +-1 (hi = 0 would make the torch split put the small part into hi)
        alt = torch.randint(0, 2, tuple(shape), generator=g) * 2 - 1
        v = torch.where(v == 0, alt, v)
    return v.double()


def pick_amp(kred, split):
    """Largest integer range [-amp, amp] of the hi parts for a reduction of ``kred`` terms: plain operands always take 8 (64 units a term);
    split operands (unit 2^-17: a term is amp^2 2^10 + 6 amp units) narrow it so that kred terms + 2^21 units of bias / residual / initial
    buffer (each at most 4 = 2^19 units) stay below 2^24."""
    if not split:
        return 8
    for amp in (8, 4, 2, 1):
        if kred * (amp * amp * 1024 + 6 * amp) + 2**21 < 2**24:
            return amp
    raise AssertionError(f"no exact split operands for a reduction of {kred}")


def gen_operand(shape, seed, split, amp, role):
    """(hi, lo) float64 CPU tensors (lo None when plain) of role 'x' (i 2^-3 [+ e 2^-13]) or 'w' (j 2^-4 [+ f 2^-14])."""
    sh, sl = (X_HI, X_LO) if role == "x" else (W_HI, W_LO)
    hi = _ints(shape, seed, -amp, amp, nonzero=split) * sh
    if not split:
        return hi, None
    lo = _ints(shape, seed + 100003, -3, 3) * sl
    # Just below a power of two the bf16 spacing halves: |hi| = one step with lo = three small steps of the OTHER sign lies past the midpoint
    # to the next bf16 number, so hi + lo would not split back into (hi, lo).  Those lo take the sign of hi.
    past = (hi.abs() == sh) & (lo.abs() == 3 * sl) & (hi * lo < 0)
    return hi, torch.where(past, -lo, lo)


def gen_grid(shape, seed, maxabs=4.0):
    """Multiples of 2^-7 in [-maxabs, maxabs] (bias, residual, initial accumulation buffers), float64."""
    n = int(maxabs / U_PLAIN)
    return _ints(shape, seed, -n, n) * U_PLAIN


def tri(f, a, b):
    """The products a split engine forms: f(a_hi, b_hi) + f(a_hi, b_lo) + f(a_lo, b_hi); plain: f(a_hi, b_hi)."""
    r = f(a[0], b[0])
    if a[1] is not None:
        r = r + f(a[0], b[1]) + f(a[1], b[0])
    return r


def tri_abs(f, a, b):
    ab = lambda t: (t[0].abs(), None if t[1] is None else t[1].abs())  # noqa: E731
    return tri(f, ab(a), ab(b))


def units(split):
    return U_SPLIT if split else U_PLAIN


def assert_budget(mag, split, what, unit=None):
    """``mag``: per output element, the sum of |term| + |bias| + |residual| + |initial value| (float64); ``unit``: the smallest addend
    (default: the smallest product of the mode)."""
    b = float(mag.max().item()) / (unit or units(split)) if mag.numel() else 0.0
    assert b < LIMIT, f"{what}: exactness budget {b:.0f} units >= 2^24"
    return b


# ---- linear forms -----------------------------------------------------------------------------------------------------------------
def linear_case(M, N, K, split, bias=True, resid=False, seed=0):
    """y[M][N] = x[M][K] @ w[N][K]^T (+ bias) (+ resid): operands, the exact accumulator and its budget."""
    amp = pick_amp(K, split)
    x = gen_operand((M, K), 11 + seed, split, amp, "x")
    w = gen_operand((N, K), 12 + seed, split, amp, "w")
    b = gen_grid((N,), 13 + seed) if bias else None
    r = gen_grid((M, N), 14 + seed) if resid else None
    mm = lambda a, c: a @ c.t()  # noqa: E731
    acc, mag = tri(mm, x, w), tri_abs(mm, x, w)
    if bias:
        acc, mag = acc + b, mag + b.abs()
    if resid:
        acc, mag = acc + r, mag + r.abs()
    return dict(x=x, w=w, bias=b, resid=r, acc=acc, mag=mag, split=split)


def dgrad_case(M, N, K, split, seed=0):
    """dx[M][K] = dy[M][N] @ w[N][K] (reduction over N) and the column sums of dx on top of an initial buffer."""
    amp = pick_amp(N, split)
    if split and M * N <= 2**13:  # the column sums reduce over M as well: small problems narrow the range for them, larger ones check dx only
        while amp > 1 and M * N * (amp * amp * 1024 + 6 * amp) + 2**21 >= 2**24:
            amp //= 2
    dy = gen_operand((M, N), 21 + seed, split, amp, "x")
    w = gen_operand((N, K), 22 + seed, split, amp, "w")
    cs0 = gen_grid((K,), 23 + seed)
    mm = lambda a, c: a @ c  # noqa: E731
    acc, mag = tri(mm, dy, w), tri_abs(mm, dy, w)
    cs_mag = cs0.abs() + mag.sum(0)
    cs_exact = float(cs_mag.max().item()) / units(split) < LIMIT  # plain operands: always (asserted); split: only the small problems
    return dict(dy=dy, w=w, acc=acc, mag=mag, cs0=cs0, cs=cs0 + acc.sum(0), cs_mag=cs_mag, cs_exact=cs_exact, split=split)


def wgrad_case(M, N, K, split, seed=0, launches=1):
    """dw[N][K] = dw0 + dy[M][N]^T @ x[M][K] (reduction over the M tokens); ``launches``: accumulating launches the budget must cover."""
    amp = pick_amp(launches * M, split)
    dy = gen_operand((M, N), 31 + seed, split, amp, "x")
    x = gen_operand((M, K), 32 + seed, split, amp, "w")
    dw0 = gen_grid((N, K), 33 + seed)
    mm = lambda a, c: a.t() @ c  # noqa: E731
    prod, pmag = tri(mm, dy, x), tri_abs(mm, dy, x)
    return dict(dy=dy, x=x, dw0=dw0, prod=prod, acc=dw0 + prod, mag=dw0.abs() + pmag, split=split)


# ---- convolutions (NHWC activations, weights Wc[Cout][taps][Cin]) ---------------------------------------------------------------------
def _nchw(t):
    return None if t is None else t.permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _w_torch(kind, w, Cout, Cin, ks):
    if w is None:
        return None
    w4 = w.reshape(Cout, ks, ks, Cin)
    return (w4.permute(0, 3, 1, 2) if kind == "conv" else w4.permute(3, 0, 1, 2)).contiguous()


def _w_stored(kind, wt, Cout, Cin, ks):
    return (wt.permute(0, 2, 3, 1) if kind == "conv" else wt.permute(1, 2, 3, 0)).reshape(Cout, ks * ks, Cin).contiguous()


def _conv(kind, x, w):
    if kind == "conv":
        return F.conv2d(x, w, None, padding=1)
    return F.conv_transpose2d(x, w, None, stride=2, padding=1, output_padding=1)


def conv_case(kind, B, H, W, Cin, Cout, split, ks=3, seed=0):
    """Forward (+ bias), data gradient, weight gradient (on an initial buffer) and bias gradient of nn.Conv2d(ks, padding=1) ('conv') or
    nn.ConvTranspose2d(3, stride 2, padding 1, output_padding 1) ('convT'), each as the float64 sum of the products the engines form."""
    taps = ks * ks
    if kind == "conv":
        Ho, Wo = H + 3 - ks, W + 3 - ks
    else:
        assert ks == 3
        Ho, Wo = 2 * H, 2 * W
    npix_out = B * Ho * Wo
    amp_f = pick_amp(taps * Cin, split)               # forward: at most taps * Cin terms
    amp_d = pick_amp(taps * Cout, split)              # data gradient: at most taps * Cout terms
    amp_w = pick_amp(2 * npix_out, split)             # weight gradient: at most one term per output pixel, of twice the size (see dy below)
    amp_x, amp_wt, amp_dy = min(amp_f, amp_w), min(amp_f, amp_d), min(amp_d, amp_w)
    x = gen_operand((B, H, W, Cin), 41 + seed, split, amp_x, "x")
    w = gen_operand((Cout, taps, Cin), 42 + seed, split, amp_wt, "w")
    # dy multiplies w in the data gradient (role x there) and x in the weight gradient: x is generated with the 'x' scales too, so the smallest
    # weight-gradient term is X_HI * X_LO = 2^-16 >= U_SPLIT and every term stays a multiple of the unit
    dy = gen_operand((B, Ho, Wo, Cout), 43 + seed, split, amp_dy, "x")
    bias = gen_grid((Cout,), 44 + seed)
    dw0 = gen_grid((Cout, taps, Cin), 45 + seed)
    db0 = gen_grid((Cout,), 46 + seed)
    xs = (_nchw(x[0]), _nchw(x[1]))
    ws = (_w_torch(kind, w[0], Cout, Cin, ks), _w_torch(kind, w[1], Cout, Cin, ks))
    dys = (_nchw(dy[0]), _nchw(dy[1]))
    xshape, wshape = xs[0].shape, ws[0].shape

    def fwd(a, c):
        return _conv(kind, a, c)

    def gx(d, c):
        x0 = torch.zeros(xshape, dtype=torch.float64, requires_grad=True)
        return torch.autograd.grad((_conv(kind, x0, c) * d).sum(), x0)[0]

    def gw(d, a):
        w0 = torch.zeros(wshape, dtype=torch.float64, requires_grad=True)
        return torch.autograd.grad((_conv(kind, a, w0) * d).sum(), w0)[0]

    bshape = (1, -1, 1, 1)
    y = _nhwc(tri(fwd, xs, ws) + bias.view(bshape))
    y_mag = _nhwc(tri_abs(fwd, xs, ws) + bias.abs().view(bshape))
    dx, dx_mag = _nhwc(tri(gx, dys, ws)), _nhwc(tri_abs(gx, dys, ws))
    dw = dw0 + _w_stored(kind, tri(gw, dys, xs), Cout, Cin, ks)
    dw_mag = dw0.abs() + _w_stored(kind, tri_abs(gw, dys, xs), Cout, Cin, ks)
    dyv = dy[0] if dy[1] is None else dy[0] + dy[1]
    db = db0 + dyv.sum((0, 1, 2))
    db_mag = db0.abs() + (dy[0].abs() if dy[1] is None else dy[0].abs() + dy[1].abs()).sum((0, 1, 2))
    return dict(x=x, w=w, dy=dy, bias=bias, dw0=dw0, db0=db0, y=y, y_mag=y_mag, dx=dx, dx_mag=dx_mag, dw=dw, dw_mag=dw_mag, db=db, db_mag=db_mag,
                split=split, Ho=Ho, Wo=Wo)


def conv_budgets(c, what):
    s = c["split"]
    return [assert_budget(c["y_mag"], s, what + " fwd"), assert_budget(c["dx_mag"], s, what + " dgrad"),
            assert_budget(c["dw_mag"], s, what + " wgrad"),
            assert_budget(c["db_mag"], s, what + " dbias", X_LO if s else U_PLAIN)]  # sums of dy itself: addends are multiples of 2^-13 / of 2^-7


def colsum_case(M, C, split, seed=0):
    x = gen_operand((M, C), 51 + seed, split, 8, "x")
    out0 = gen_grid((C,), 52 + seed)
    v = x[0] if x[1] is None else x[0] + x[1]
    mag = out0.abs() + (x[0].abs() if x[1] is None else x[0].abs() + x[1].abs()).sum(0)
    return dict(x=x, out0=out0, acc=out0 + v.sum(0), mag=mag, split=split)


def colsum_budget(c):
    b = float(c["mag"].max().item()) / (X_LO if c["split"] else X_HI)
    assert b < LIMIT, f"colsum: exactness budget {b:.0f} units >= 2^24"
    return b


PGP_UNIT = 2.0**-10


def patch_grad_prep_case(B, ntok, D, seed=0):
    """dx f32 [B][ntok][D] = k 2^-10 with |k| <= kmax, kmax the largest power of two (<= 2^15) that keeps B * ntok * kmax + 2^10 below 2^24:
    up to 16 significant bits, so hi / lo are non-trivial (exact ties included) while the fp32 column sums stay exact."""
    kmax = 2**15
    while B * ntok * kmax + 2**10 >= 2**24:
        kmax //= 2
    dx = _ints((B, ntok, D), 61 + seed, -kmax, kmax) * PGP_UNIT
    dcls0, dbias0 = gen_grid((D,), 62 + seed, 1.0), gen_grid((D,), 63 + seed, 1.0)
    dcls = dcls0 + dx[:, 0].sum(0)
    dbias = dbias0 + dx[:, 1:].sum((0, 1))
    mag = torch.maximum(dcls0.abs() + dx[:, 0].abs().sum(0), dbias0.abs() + dx[:, 1:].abs().sum((0, 1)))
    return dict(dx=dx, dcls0=dcls0, dbias0=dbias0, dcls=dcls, dbias=dbias, mag=mag, rows=dx[:, 1:].reshape(B * (ntok - 1), D))


def patch_grad_prep_budget(c):
    b = float(c["mag"].max().item()) / PGP_UNIT
    assert b < LIMIT, f"patch_grad_prep: exactness budget {b:.0f} units >= 2^24"
    return b


# ---- the parametrised shapes (dispatch conditions read from gemm.hip / gemm8.hip / gemm4.hip / gemm8w.hip / conv8.hip / conv_direct.hip) -------
# route -> (environment, kernel-name prefix plain, kernel-name prefix split)
LINEAR_ROUTES = {
    # no switch: shapes with N, K multiples of 128 take the 128 x 128 instance of gemm8.hip (fewer than 128 tiles of 256 x 256) ...
    "default8": ({}, "gemm8_kernel<0,1,0,false,false,2,2,2>", "gemm8_kernel<0,2,0,false,true,2,2,2>"),
    # ... every other shape the generic engine of gemm.hip (128-row tiles, K-step 64 or 32)
    "generic": ({}, "gemm_kernel<", "gemm_kernel<"),
    "gemm8": ({"IG_GEMM8": "2", "IG_GEMM4": "0"}, "gemm8_kernel<0,1,0,false,false,4>", "gemm8_kernel<0,2,0,false,true,4>"),
    "gemm4": ({"IG_GEMM8": "2", "IG_GEMM4": "2"}, "gemm4_kernel<0,0,false>", "gemm4_kernel<0,0,false,2>"),
}
LINEAR_FWD_CASES = [
    # 128-row tiles: M one below / at / one above; N = 384: three column tiles; K = 128: the smallest legal, 256, and the plain budget's edge
    ("default8", 127, 128, 128), ("default8", 128, 128, 128), ("default8", 129, 384, 256), ("default8", 130, 128, 3072),
    # generic: K = 8 (smallest legal), 72 = one K-tile + 8, N with a partial last tile, M around the tile height
    ("generic", 77, 40, 8), ("generic", 127, 136, 72), ("generic", 128, 200, 72), ("generic", 129, 136, 136), ("generic", 300, 256, 192),
    # 256 x 256 tiles: M one below / at / one above; K = 128 (two K-tiles: the smallest), 192 is not legal there -> 256, 384
    ("gemm8", 255, 256, 128), ("gemm8", 256, 256, 128), ("gemm8", 257, 512, 256), ("gemm8", 300, 256, 384),
    # 4-wave engine: K >= 256, a multiple of 128
    ("gemm4", 255, 256, 256), ("gemm4", 256, 256, 256), ("gemm4", 257, 512, 384), ("gemm4", 300, 256, 3072),
]
# persistent seam: 33 x 4 = 132 tiles of 256 x 256 (ragged last row tile) on 72 workgroups (IG_RESERVED_STRICT=1 with 127 reserved CUs: two rounds)
LINEAR_SEAM_CASES = [("gemm8", 8348, 1024, 128), ("gemm4", 8348, 1024, 256)]
DGRAD_CASES = [(77, 40, 8), (127, 136, 72), (128, 128, 72), (129, 200, 136), (130, 256, 128)]
DGRAD_WT_CASES = [  # (IG_GEMM8, M, N, K, prefix plain, prefix split): the GEMM is M x K with reduction N
    ("1", 127, 128, 128, "gemm8_kernel<0,1,0,false,false,2,2,2>", "gemm8_kernel<0,2,0,false,true,2,2,2>"),
    ("1", 129, 256, 384, "gemm8_kernel<0,1,0,false,false,2,2,2>", "gemm8_kernel<0,2,0,false,true,2,2,2>"),
    ("1", 333, 192, 64, "gemm_kernel<", "gemm_kernel<"),
    ("1", 128, 72, 40, "gemm_kernel<", "gemm_kernel<"),
    ("2", 255, 128, 256, "gemm8_kernel<0,1,0,false,false,4>", "gemm8_kernel<0,2,0,false,true,4>"),
    ("2", 257, 384, 512, "gemm8_kernel<0,1,0,false,false,4>", "gemm8_kernel<0,2,0,false,true,4>"),
]
WGRAD_CASES = [(1, 256, 256), (127, 256, 256), (128, 256, 512), (129, 512, 256), (130, 40, 72), (64, 192, 64), (500, 40, 72), (8, 8, 8)]
WGRAD_GROUP_CASES = [(127, [(256, 256)]), (128, [(256, 256), (512, 256)]), (129, [(256, 512)]), (197, [(256, 256), (768, 256)]), (257, [(512, 512)])]
WGRAD_GROUP_FALLBACK = (130, [(192, 64), (256, 256), (40, 72)])
PATCH_EMBED_CASES = [(1, 2, 9, 40, 72), (3, 2, 9, 40, 72), (1, 3, 43, 136, 8), (3, 1, 43, 64, 200)]  # (T, B, tokens per frame, D, K)

CONV_OFF = {"IG_CONV8": "0", "IG_CONV_DIRECT": "0", "IG_WGRAD8_CONV": "0"}
CONV8_ON = {"IG_CONV8": "2", "IG_CONV_DIRECT": "0", "IG_GEMM4": "0", "IG_WGRAD8_CONV": "0"}
CONV4_ON = {"IG_CONV8": "2", "IG_CONV_DIRECT": "0", "IG_GEMM4": "2", "IG_WGRAD8_CONV": "0"}
WG8_ON = {"IG_CONV8": "0", "IG_CONV_DIRECT": "0", "IG_WGRAD8_CONV": "2"}
# (id, kind, env, B, H, W, Cin, Cout, ks, splits, routes): routes = {op: (prefix plain, prefix split)}; an op without an entry is not run
CONV_CASES = [
    # the gather GEMM of gemm.hip (every engine switched off): smallest channels, ragged maps, more than one 128-row tile
    ("generic-8-8", "conv", CONV_OFF, 2, 5, 7, 8, 8, 3, (False, True), dict(fwd=("gemm_kernel<",) * 2, dgrad=("gemm_kernel<",) * 2, wgrad=("gemm",) * 2)),
    ("generic-16-40", "conv", CONV_OFF, 1, 13, 10, 16, 40, 3, (False, True), dict(fwd=("gemm_kernel<",) * 2, dgrad=("gemm_kernel<",) * 2, wgrad=("gemm",) * 2)),
    ("generic-T-16-8", "convT", CONV_OFF, 2, 3, 4, 16, 8, 3, (False, True), dict(fwd=("gemm_kernel<",) * 2, dgrad=("gemm_kernel<",) * 2, wgrad=("gemm",) * 2)),
    ("generic-T-24-40", "convT", CONV_OFF, 1, 5, 7, 24, 40, 3, (False, True), dict(fwd=("gemm_kernel<",) * 2, dgrad=("gemm_kernel<",) * 2, wgrad=("gemm",) * 2)),
    ("k5", "conv", {}, 1, 6, 7, 16, 8, 5, (False, True), dict(fwd=("gemm_kernel<",) * 2, dgrad=("gemm_kernel<",) * 2, wgrad=("gemm",) * 2)),
    ("k5-ragged", "conv", {}, 2, 9, 11, 24, 40, 5, (False, True), dict(fwd=("gemm_kernel<",) * 2, dgrad=("gemm_kernel<",) * 2, wgrad=("gemm",) * 2)),
    ("k7", "conv", {}, 1, 7, 8, 16, 8, 7, (False, True), dict(fwd=("gemm_kernel<",) * 2, dgrad=("gemm_kernel<",) * 2, wgrad=("gemm",) * 2)),
    ("k7-ragged", "conv", {}, 2, 9, 12, 8, 24, 7, (False, True), dict(fwd=("gemm_kernel<",) * 2, dgrad=("gemm_kernel<",) * 2, wgrad=("gemm",) * 2)),
    # conv8.hip forced: 256-row tiles, B H W = 255 / 256 / 257; Cout = 192: two column tiles on the 128-wide instance or one 192-wide
    ("conv8-255", "conv", CONV8_ON, 1, 15, 17, 64, 128, 3, (False, True), dict(fwd=("conv8_kernel<",) * 2, dgrad=("conv8_kernel<",) * 2)),
    ("conv8-256", "conv", CONV8_ON, 1, 16, 16, 64, 128, 3, (False, True), dict(fwd=("conv8_kernel<",) * 2, dgrad=("conv8_kernel<",) * 2)),
    ("conv8-257", "conv", CONV8_ON, 1, 1, 257, 64, 192, 3, (False, True), dict(fwd=("conv8_kernel<",) * 2, dgrad=("conv8_kernel<",) * 2)),
    ("conv8-k16", "conv", CONV8_ON, 2, 9, 11, 16, 128, 3, (False, True), dict(fwd=("conv8_kernel<",) * 2)),  # K = 144: padded to two K-tiles
    ("conv8-T-255", "convT", CONV8_ON, 1, 15, 17, 64, 128, 3, (False, True), dict(fwd=("conv8_kernel<",) * 2, dgrad=("conv8_kernel<",) * 2)),
    ("conv8-T-257", "convT", CONV8_ON, 1, 1, 257, 128, 128, 3, (False, True), dict(fwd=("conv8_kernel<",) * 2, dgrad=("conv8_kernel<",) * 2)),
    # conv4_kernel (IG_GEMM4=2): widths that tile by 96 / 192, at least four K-tiles
    ("conv4-96", "conv", CONV4_ON, 1, 15, 17, 96, 96, 3, (False, True), dict(fwd=("conv4_kernel<3",) * 2, dgrad=("conv4_kernel<3",) * 2)),
    ("conv4-192", "conv", CONV4_ON, 1, 1, 257, 32, 192, 3, (False, True), dict(fwd=("conv4_kernel<6",) * 2)),
    ("conv4-T", "convT", CONV4_ON, 1, 9, 15, 192, 96, 3, (False, True), dict(fwd=("conv4_kernel<3",) * 2, dgrad=("conv4_kernel<6",) * 2)),
    # the direct kernels of conv_direct.hip (no switch): 48 and 96 channels, 96 -> 48 ConvTranspose; split operands: the 48-channel forward /
    # data gradient have a kernel of their own, the weight gradients run three launches of the plain kernel
    ("direct48-tiny", "conv", {}, 1, 1, 3, 48, 48, 3, (False, True),
     dict(fwd=("conv3x3_direct_kernel<48", "conv3x3_direct_split_kernel<48>"), dgrad=("conv3x3_direct_kernel<48", "conv3x3_direct_split_kernel<48>"),
          wgrad=("conv3x3_wgrad_dma_kernel<48",) * 2)),
    ("direct48", "conv", {}, 2, 17, 19, 48, 48, 3, (False, True),
     dict(fwd=("conv3x3_direct_kernel<48", "conv3x3_direct_split_kernel<48>"), dgrad=("conv3x3_direct_kernel<48", "conv3x3_direct_split_kernel<48>"),
          wgrad=("conv3x3_wgrad_dma_kernel<48",) * 2)),
    ("direct96", "conv", {}, 2, 17, 19, 96, 96, 3, (False,), dict(fwd=("conv3x3_direct",) * 2, dgrad=("conv3x3_direct",) * 2, wgrad=("conv3x3_wgrad_dma_kernel<96",) * 2)),
    ("direct96-tiny", "conv", {}, 1, 3, 1, 96, 96, 3, (False,), dict(fwd=("conv3x3_direct",) * 2, dgrad=("conv3x3_direct",) * 2, wgrad=("conv3x3_wgrad_dma_kernel<96",) * 2)),
    ("directT", "convT", {}, 2, 9, 11, 96, 48, 3, (False,),
     dict(fwd=("convT_direct_dma_kernel<96,48>",) * 2, dgrad=("convT_dgrad_direct_kernel<96,48>",) * 2, wgrad=("convT_wgrad_dma_kernel<96,48>",) * 2)),
    ("directT-tiny", "convT", {}, 1, 1, 1, 96, 48, 3, (False,),
     dict(fwd=("convT_direct_dma_kernel<96,48>",) * 2, dgrad=("convT_dgrad_direct_kernel<96,48>",) * 2, wgrad=("convT_wgrad_dma_kernel<96,48>",) * 2)),
    # gemm8w.hip forced for the convolution weight gradients: token counts around one pair of 64-token K-tiles
    ("wgrad8-127", "conv", WG8_ON, 1, 1, 127, 32, 64, 3, (False, True), dict(wgrad=("gemm8w_kernel<",) * 2)),
    ("wgrad8-128", "conv", WG8_ON, 1, 8, 16, 32, 64, 3, (False, True), dict(wgrad=("gemm8w_kernel<",) * 2)),
    ("wgrad8-129", "conv", WG8_ON, 1, 3, 43, 48, 200, 3, (False, True), dict(wgrad=("gemm8w_kernel<",) * 2)),
    ("wgrad8-T-33", "convT", WG8_ON, 1, 3, 11, 64, 32, 3, (False, True), dict(wgrad=("gemm8w_kernel<",) * 2)),
    ("wgrad8-T-130", "convT", WG8_ON, 2, 5, 13, 200, 24, 3, (False, True), dict(wgrad=("gemm8w_kernel<",) * 2)),
]
CONV_PARAMS = [pytest.param(c, s, id=f"{c[0]}-{'split' if s else 'plain'}") for c in CONV_CASES for s in c[9]]

COLSUM_CASES = [(M, C) for C in (8, 1024, 1032) for M in (1, 31, 32, 33, 100, 1000)]  # 32 rows a chunk at these sizes
PGP_CASES = [(B, ntok, 12) for B in (1, 8, 9, 65) for ntok in (1, 2, 16, 17, 197)] + [(9, 17, 1028)]  # D = 1028: 257 float4 columns > TPB


# =====================================================================================================================================
# Device helpers
# =====================================================================================================================================
def to_bt(pair, split=None):
    """Upload (hi, lo) float64 CPU tensors as bf16 bit patterns; every value must be a bf16 number."""
    hi, lo = pair
    b = BT.empty(tuple(hi.shape), lo is not None, DEV)
    for dst, src in ((b.hi, hi), (b.lo, lo)):
        if src is not None:
            h = src.to(BF16)
            assert torch.equal(h.double(), src), "operand is not exactly representable in bf16"
            dst.copy_(h)
    return b


def f32_dev(t):
    f = t.float()
    assert torch.equal(f.double(), t), "value is not exactly representable in fp32"
    return f.to(DEV).contiguous()


def run(fn, *a, **k):
    """Call an entry point and return the kernel it launched last."""
    from instageo_amd import _lib

    _lib.load().ig_note_reset()
    fn(*a, **k)
    return ops.last_kernel()


def _fail(what, route, got, want):
    diff = (got != want).flatten().nonzero().flatten()
    g, w = got.flatten(), want.flatten()
    first = [(int(i), g[i].item(), w[i].item()) for i in diff[:6]]
    return f"{what} [{route}]: {diff.numel()} of {g.numel()} elements differ; first (index, got, want): {first}"


def check_bits(got_bf16, want_bf16, what, route):
    got, want = bits16(got_bf16.cpu()), bits16(want_bf16)
    if not torch.equal(got, want):
        raise AssertionError(_fail(what, route, got_bf16.cpu().float(), want_bf16.float()) + f" (bits: {_fail(what, route, got, want)})")


def check_bt(out, acc, what, route):
    """bf16 output == RNE(acc); split output == the part-A reference applied to the fp32 value of acc."""
    a32 = acc.float()
    assert torch.equal(a32.double(), acc), f"{what}: the reference accumulator is not an fp32 number"
    hi, lo = split_ref(a32)
    check_bits(out.hi, hi, what + " hi", route)
    if out.lo is not None:
        check_bits(out.lo, lo, what + " lo", route)


def check_f32(got, acc, what, route):
    a32 = acc.float()
    assert torch.equal(a32.double(), acc), f"{what}: the reference is not an fp32 number"
    g = got.cpu()
    if not torch.equal(g, a32):
        raise AssertionError(_fail(what, route, g, a32))


def want_route(route, prefix, what):
    print(f"{what}: {route}")
    assert route.startswith(prefix), f"{what}: expected a kernel named {prefix}..., ran {route!r}"


def setenv(monkeypatch, env):
    for k in ("IG_GEMM8", "IG_GEMM4", "IG_CONV8", "IG_CONV_DIRECT", "IG_WGRAD8_CONV", "IG_WGRAD8", "IG_G8_PAIR", "IG_RESERVED_STRICT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# =====================================================================================================================================
# A. The conversion layer
# =====================================================================================================================================
def _split_dev(x32, split):
    n = x32.numel()
    out = BT.empty((n,), split, DEV)
    out.hi.view(torch.int16).fill_(0x7F7F)  # not a value any input here rounds to by accident of a stale buffer
    if split:
        out.lo.view(torch.int16).fill_(0x7F7F)
    ops.split_bf16(x32.to(DEV), out)
    return out


def _merge_dev(hi, lo):
    b = BT(hi.to(DEV).contiguous(), None if lo is None else lo.to(DEV).contiguous())
    return b.float().cpu()


def test_split_special_values():
    x = f32_from_bits(special_fp32_bits())
    hi_ref, lo_ref = split_ref(x)
    res = (x - hi_ref.float()).abs()
    sub = (res != 0) & (res < 2.0**-126)  # a subnormal residual: test_split_subnormals
    fin = torch.isfinite(hi_ref.float()) & torch.isfinite(lo_ref.float()) & ~sub
    out = _split_dev(x, True)
    hi, lo = out.hi.cpu(), out.lo.cpu()
    check_bits(hi[fin], hi_ref[fin], "split hi", "ig_split_bf16")
    check_bits(lo[fin], lo_ref[fin], "split lo", "ig_split_bf16")
    plain = _split_dev(x, False)
    check_bits(plain.hi.cpu()[fin], hi_ref[fin], "split hi (lo = None)", "ig_split_bf16")
    merged = out.float().cpu()
    assert torch.equal(merged[fin].view(torch.int32), merged_ref(hi_ref, lo_ref)[fin].view(torch.int32)), "merge of the split halves"
    # all bf16 patterns: unchanged, lo = +0, the sign of -0 kept in hi
    nb = 65536 - 2 * 127
    assert torch.equal(bits16(hi[:nb][fin[:nb]]), (x[:nb][fin[:nb]].view(torch.int32) >> 16).to(torch.int16)), "a bf16 number did not round-trip"
    assert (bits16(lo[:nb][fin[:nb]]) == 0).all(), "lo of a bf16 number is not +0"
    # non-finite results: hi keeps the class, the merged value is non-finite
    nf = ~torch.isfinite(hi_ref.float())
    assert torch.equal(torch.isnan(hi.float()[nf]), torch.isnan(hi_ref.float()[nf])) and torch.equal(torch.isinf(hi.float()[nf]), torch.isinf(hi_ref.float()[nf]))
    assert torch.equal(torch.signbit(hi.float()[nf & ~torch.isnan(hi_ref.float())]), torch.signbit(hi_ref.float()[nf & ~torch.isnan(hi_ref.float())]))
    assert torch.equal(torch.isnan(plain.hi.cpu().float()[nf]), torch.isnan(hi_ref.float()[nf]))
    assert not torch.isfinite(merged[nf]).any(), "a non-finite input merged to a finite value"


def test_split_subnormals():
    """fp32 subnormal inputs and subnormal residuals of small normal inputs: torch keeps them, and so must the kernels."""
    x = f32_from_bits(subnormal_fp32_bits())
    small = f32_from_bits(special_fp32_bits())
    h, _ = split_ref(small)
    r = (small - h.float()).abs()
    x = torch.cat([x, small[(r != 0) & (r < 2.0**-126)]])
    hi_ref, lo_ref = split_ref(x)
    out = _split_dev(x, True)
    check_bits(out.hi, hi_ref, "split hi (subnormal)", "ig_split_bf16")
    check_bits(out.lo, lo_ref, "split lo (subnormal)", "ig_split_bf16")
    assert torch.equal(out.float().cpu().view(torch.int32), merged_ref(hi_ref, lo_ref).view(torch.int32)), "merge (subnormal)"


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("n", SPLIT_LENGTHS)
def test_split_merge_lengths(n, split):
    base = finite_split_values()
    x = base.repeat((n + base.numel() - 1) // base.numel())[:n].contiguous()
    hi_ref, lo_ref = split_ref(x)
    pad = 64  # a guard band behind the n elements: a tail handled as a wider unit would write into it
    out = BT.empty((n + pad,), split, DEV)
    out.hi.view(torch.int16).fill_(0x1234)
    if split:
        out.lo.view(torch.int16).fill_(0x1234)
    ops.split_bf16(x.to(DEV), BT(out.hi[:n], None if not split else out.lo[:n]))
    check_bits(out.hi[:n], hi_ref, f"split hi, n = {n}", "ig_split_bf16")
    assert (bits16(out.hi[n:].cpu()) == 0x1234).all(), "split wrote past n (hi)"
    if split:
        check_bits(out.lo[:n], lo_ref, f"split lo, n = {n}", "ig_split_bf16")
        assert (bits16(out.lo[n:].cpu()) == 0x1234).all(), "split wrote past n (lo)"
    dst = torch.full((n + pad,), 7.0, device=DEV)
    from instageo_amd import _lib

    _lib.call("ig_merge_bf16", out.hi.data_ptr(), out.lo.data_ptr() if split else None, dst.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
    want = merged_ref(hi_ref, lo_ref) if split else hi_ref.float()
    assert torch.equal(dst[:n].cpu().view(torch.int32), want.view(torch.int32)), f"merge, n = {n}"
    assert (dst[n:] == 7.0).all(), "merge wrote past n"


def merge_pairs():
    """(hi, lo) bf16 pairs no split would produce: random signs, lo from far below to sixteen times hi (so lo beyond half an ulp of hi, opposite
    signs, cancellation to zero), zeros on either side; exponents kept where every fp32 sum is zero or normal."""
    g = torch.Generator().manual_seed(5)
    n = 20000
    e_hi = torch.randint(-60, 61, (n,), generator=g)
    m = lambda: torch.randint(128, 256, (n,), generator=g).double() / 128.0  # noqa: E731
    s = lambda: (torch.randint(0, 2, (n,), generator=g) * 2 - 1).double()  # noqa: E731
    hi = s() * m() * torch.pow(2.0, e_hi.double())
    lo = s() * m() * torch.pow(2.0, (e_hi + torch.randint(-20, 5, (n,), generator=g)).double())
    lo[:500] = -hi[:500]                  # exact cancellation
    lo[500:1000] = -hi[500:1000] * 0.5    # opposite sign, far beyond half an ulp
    lo[1000:1100] = 0.0
    hi[1100:1200] = 0.0
    lo[1200:1250] = -0.0
    hi, lo = hi.to(BF16), lo.to(BF16)
    return hi, lo


def test_merge_hand_built_pairs():
    hi, lo = merge_pairs()
    got = _merge_dev(hi, lo)
    want = hi.float() + lo.float()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), _fail("merge", "ig_merge_bf16", got, want)
    got = _merge_dev(hi, None)
    assert torch.equal(got.view(torch.int32), hi.float().view(torch.int32)), "merge with lo = None"


@pytest.mark.parametrize("B,ntok,D", PGP_CASES)
def test_patch_grad_prep(B, ntok, D):
    """store4_split through ig_patch_grad_prep, bit for bit against the torch split of the same fp32 values; dcls / dbias accumulate exactly.
    B = 1, 8 | 9 | 65: the three batch-group rules of the launcher; ntok = 1: no patch rows at all; 16 / 17: one and two token chunks."""
    c = patch_grad_prep_case(B, ntok, D)
    patch_grad_prep_budget(c)
    dx = f32_dev(c["dx"])
    rows = B * (ntok - 1)
    want_hi, want_lo = split_ref(c["rows"].float())
    for split in (False, True):
        out = BT.empty((rows + 1, D), split, DEV)  # one spare row: never empty, and a guard behind the last row
        out.hi.view(torch.int16).fill_(0x1234)
        if split:
            out.lo.view(torch.int16).fill_(0x1234)
        dcls, dbias = f32_dev(c["dcls0"]), f32_dev(c["dbias0"])
        ops.patch_grad_prep(dx, out, dcls, dbias, B, ntok, D)
        check_bits(out.hi[:rows], want_hi, "patch_grad_prep hi", "ig_patch_grad_prep")
        if split:
            check_bits(out.lo[:rows], want_lo, "patch_grad_prep lo", "ig_patch_grad_prep")
            assert (bits16(out.lo[rows:].cpu()) == 0x1234).all()
        assert (bits16(out.hi[rows:].cpu()) == 0x1234).all(), "patch_grad_prep wrote past its rows"
        check_f32(dcls, c["dcls"], "patch_grad_prep dcls", "ig_patch_grad_prep")
        check_f32(dbias, c["dbias"], "patch_grad_prep dbias", "ig_patch_grad_prep")


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("n", [12, 4096 + 8])
def test_adamw_shadow_is_the_split_of_the_parameter(n, split):
    """store4_split through the AdamW shadow: shadow bits == split(p) of the p the kernel wrote."""
    g = torch.Generator().manual_seed(3)
    p = (torch.randn(n, generator=g) * torch.pow(2.0, torch.randint(-12, 6, (n,), generator=g).float())).to(DEV)
    grad, m, v = torch.randn(n, generator=g).to(DEV), (0.1 * torch.randn(n, generator=g)).to(DEV), torch.rand(n, generator=g).to(DEV)
    hyper = torch.zeros(16, device=DEV)
    hyper[:5] = torch.tensor([1e-3, 0.9, 0.999, 1e-8, 1e-2])
    hyper[11], hyper[12] = 1 - 0.9, 1 - 0.999
    shadow = BT.empty((n,), split, DEV)
    ops.adamw_advance(hyper)
    ops.adamw_step(p, grad, m, v, shadow, hyper, n)
    hi, lo = split_ref(p.cpu())
    check_bits(shadow.hi, hi, "adamw shadow hi", "ig_adamw_step")
    if split:
        check_bits(shadow.lo, lo, "adamw shadow lo", "ig_adamw_step")


# =====================================================================================================================================
# B. Exact-arithmetic parity
# =====================================================================================================================================
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("route,M,N,K", LINEAR_FWD_CASES)
def test_linear_fwd_and_residual(route, M, N, K, split, monkeypatch):
    env, pre_plain, pre_split = LINEAR_ROUTES[route]
    prefix = pre_split if split else pre_plain
    c = linear_case(M, N, K, split, bias=True, resid=True)
    assert_budget(c["mag"], split, f"linear {M}x{N}x{K}")
    setenv(monkeypatch, env)
    x, w = to_bt(c["x"]), to_bt(c["w"])
    bias, resid = f32_dev(c["bias"]), f32_dev(c["resid"])
    y = BT.zeros((M, N), split, DEV)
    r = run(ops.linear_fwd, x, w, bias, y, M, N, K, act=0)
    want_route(r, prefix, f"linear_fwd {M}x{N}x{K} {'split' if split else 'plain'}")
    check_bt(y, c["acc"] - c["resid"], "linear_fwd + bias", r)
    r = run(ops.linear_fwd, x, w, None, y, M, N, K, act=0)
    want_route(r, prefix, "linear_fwd, no bias")
    check_bt(y, c["acc"] - c["resid"] - c["bias"], "linear_fwd, no bias", r)
    out = torch.full((M, N), 3.0, device=DEV)
    r = run(ops.linear_residual_fwd, x, w, bias, resid, out, M, N, K)
    kind1 = prefix.replace("gemm8_kernel<0,", "gemm8_kernel<1,").replace(",true,", ",false,").replace("gemm4_kernel<0,", "gemm4_kernel<1,")
    want_route(r, kind1, "linear_residual_fwd")
    check_f32(out, c["acc"], "linear_residual_fwd", r)
    r = run(ops.linear_residual_fwd, x, w, None, resid, resid, M, N, K)  # in place, no bias
    check_f32(resid, c["acc"] - c["bias"], "linear_residual_fwd in place, no bias", r)


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("route,M,N,K", LINEAR_SEAM_CASES)
def test_linear_persistent_seam(route, M, N, K, split, monkeypatch):
    """More tiles than workgroups: with 127 CUs reserved (strictly) the persistent kernels launch fewer workgroups than the 132 tiles, so the tile
    hand-over inside a workgroup (accumulator re-initialisation, pipeline drain and refill) is exercised at a modest shape."""
    env, pre_plain, pre_split = LINEAR_ROUTES[route]
    c = linear_case(M, N, K, split, bias=True, resid=True)
    assert_budget(c["mag"], split, f"linear seam {M}x{N}x{K}")
    setenv(monkeypatch, dict(env, IG_RESERVED_STRICT="1"))
    from instageo_amd import _lib

    x, w, bias, resid = to_bt(c["x"]), to_bt(c["w"]), f32_dev(c["bias"]), f32_dev(c["resid"])
    y = BT.zeros((M, N), split, DEV)
    out = torch.zeros((M, N), device=DEV)
    try:
        ops.set_reserved_cus(127)
        r = run(ops.linear_fwd, x, w, bias, y, M, N, K, act=0)
        grid = _lib.load().ig_last_grid()
        want_route(r, pre_split if split else pre_plain, f"linear_fwd seam {M}x{N}x{K}")
        assert 0 < grid < ((M + 255) // 256) * (N // 256), f"grid {grid}: no workgroup walks two tiles"
        r2 = run(ops.linear_residual_fwd, x, w, bias, resid, out, M, N, K)
    finally:
        ops.set_reserved_cus(0)
    check_bt(y, c["acc"] - c["resid"], "linear_fwd across the tile seam", r)
    check_f32(out, c["acc"], "linear_residual_fwd across the tile seam", r2)


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("M,N,K", DGRAD_CASES)
def test_linear_dgrad(M, N, K, split, monkeypatch):
    c = dgrad_case(M, N, K, split)
    assert_budget(c["mag"], split, f"dgrad {M}x{N}x{K}")
    assert c["cs_exact"] or split, "the column sums of every plain case are exact"
    setenv(monkeypatch, {})
    dy, w = to_bt(c["dy"]), to_bt(c["w"])
    dx = BT.zeros((M, K), split, DEV)
    r = run(ops.linear_dgrad, dy, w, dx, M, N, K)
    want_route(r, "gemm", f"linear_dgrad {M}x{N}x{K}")
    check_bt(dx, c["acc"], "linear_dgrad", r)
    dx = BT.zeros((M, K), split, DEV)
    cs = f32_dev(c["cs0"])
    r = run(ops.linear_dgrad, dy, w, dx, M, N, K, colsum=cs)
    want_route(r, "gemm2_kernel<", f"linear_dgrad + colsum {M}x{N}x{K}")  # the fused column sums live in the 256 x 128 engine
    check_bt(dx, c["acc"], "linear_dgrad (+ colsum)", r)
    if c["cs_exact"]:
        assert_budget(c["cs_mag"], split, f"dgrad column sums {M}x{N}x{K}")
        check_f32(cs, c["cs"], "linear_dgrad column sums", r)


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("force,M,N,K,pre_plain,pre_split", DGRAD_WT_CASES)
def test_linear_dgrad_wt(force, M, N, K, pre_plain, pre_split, split, monkeypatch):
    c = dgrad_case(M, N, K, split)
    assert_budget(c["mag"], split, f"dgrad_wt {M}x{N}x{K}")
    setenv(monkeypatch, {"IG_GEMM8": force, "IG_GEMM4": "0"})
    dy = to_bt(c["dy"])
    wt = to_bt((c["w"][0].t().contiguous(), None if c["w"][1] is None else c["w"][1].t().contiguous()))
    dx = BT.zeros((M, K), split, DEV)
    r = run(ops.linear_dgrad, dy, None, dx, M, N, K, wt=wt)
    want_route(r, pre_split if split else pre_plain, f"linear_dgrad_wt {M}x{N}x{K} IG_GEMM8={force}")
    check_bt(dx, c["acc"], "linear_dgrad_wt", r)


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("M,N,K", WGRAD_CASES)
def test_linear_wgrad(M, N, K, split, monkeypatch):
    c = wgrad_case(M, N, K, split, launches=2)
    assert_budget(c["mag"] + c["mag"] - c["dw0"].abs(), split, f"wgrad {M}x{N}x{K}")  # two accumulating launches
    setenv(monkeypatch, {})
    dy, x = to_bt(c["dy"]), to_bt(c["x"])
    dw = f32_dev(c["dw0"])
    r = run(ops.linear_wgrad, dy, x, dw, M, N, K)
    want_route(r, "gemm4w_kernel<" if (N % 256 == 0 and K % 256 == 0) else "gemm", f"linear_wgrad {M}x{N}x{K}")
    check_f32(dw, c["acc"], "linear_wgrad (+=)", r)
    r = run(ops.linear_wgrad, dy, x, dw, M, N, K)
    check_f32(dw, c["acc"] + c["prod"], "linear_wgrad, second accumulation", r)


def _group_items(M, shapes, split, flat=None):
    cases = [wgrad_case(M, N, K, split, seed=7 * gi) for gi, (N, K) in enumerate(shapes)]
    items, off = [], 0
    for c, (N, K) in zip(cases, shapes):
        if flat is None:
            dw = f32_dev(c["dw0"])
        else:
            dw = flat[off : off + N * K].view(N, K)
            dw.copy_(f32_dev(c["dw0"]))
            off += N * K
        items.append((to_bt(c["dy"]), to_bt(c["x"]), dw, N, K))
    return cases, items


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("arm", ["0", "1"])
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("M,shapes", WGRAD_GROUP_CASES)
def test_linear_wgrad_group(M, shapes, split, arm, det, monkeypatch):
    """Both kernels of the grouped weight gradients (IG_GEMM4 = 0: gemm8w_kernel, 1: gemm4w_kernel), accumulate and overwrite forms, with the
    deterministic-reduction mode off and on."""
    setenv(monkeypatch, {"IG_GEMM4": arm})
    flat = torch.zeros(sum(n * k for n, k in shapes), device=DEV) if det else None
    cases, items = _group_items(M, shapes, split, flat)
    for c in cases:
        assert_budget(c["mag"], split, f"grouped wgrad M = {M}")
    want = f"gemm4w_kernel<{'true' if split else 'false'}>" if arm == "1" else f"gemm8w_kernel<{2 if split else 1},0,4,2>"
    try:
        if det:
            ops.set_deterministic(flat)
        r = run(ops.linear_wgrad_group, items, M)
        if det:
            ops.det_fold(0, flat.numel())
        want_route(r, want, f"linear_wgrad_group M = {M} {shapes}")
        for c, it in zip(cases, items):
            check_f32(it[2], c["acc"], f"grouped wgrad {it[3]}x{it[4]} (+=)", r)
        for it in items:
            it[2].fill_(float("nan"))
        r = run(ops.linear_wgrad_group, items, M, overwrite=True)
        if det:
            ops.det_fold(0, flat.numel())
        want_route(r, want, "linear_wgrad_group, overwrite")
        for c, it in zip(cases, items):
            check_f32(it[2], c["prod"], f"grouped wgrad {it[3]}x{it[4]} (overwrite)", r)
    finally:
        if det:
            ops.set_deterministic(None)


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("split", [False, True])
def test_linear_wgrad_group_fallback_shapes(split, det, monkeypatch):
    """A group with shapes the 8-phase engine does not cover runs one ig_linear_wgrad per GEMM (atomic split-K epilogues of gemm.hip)."""
    M, shapes = WGRAD_GROUP_FALLBACK
    setenv(monkeypatch, {})
    flat = torch.zeros(sum(n * k for n, k in shapes), device=DEV) if det else None
    cases, items = _group_items(M, shapes, split, flat)
    for c in cases:
        assert_budget(c["mag"], split, "grouped wgrad fallback")
    try:
        if det:
            ops.set_deterministic(flat)
        r = run(ops.linear_wgrad_group, items, M)
        if det:
            ops.det_fold(0, flat.numel())
        want_route(r, "gemm", "linear_wgrad_group fallback")
        assert not r.startswith(("gemm8w", "gemm4w")), r  # the last GEMM of the group (40 x 72) is not a gemm8w shape
        for c, it in zip(cases, items):
            check_f32(it[2], c["acc"], f"grouped wgrad fallback {it[3]}x{it[4]} (+=)", r)
        for it in items:
            it[2].fill_(float("nan"))
        r = run(ops.linear_wgrad_group, items, M, overwrite=True)
        if det:
            ops.det_fold(0, flat.numel())
        for c, it in zip(cases, items):
            check_f32(it[2], c["prod"], f"grouped wgrad fallback {it[3]}x{it[4]} (overwrite)", r)
    finally:
        if det:
            ops.set_deterministic(None)


def patch_embed_case(T, B, tpf, D, K, split):
    tpc = T * tpf
    c = linear_case(B * tpc, D, K, split, bias=True, resid=False, seed=5)
    pos = gen_grid((1 + tpc, D), 71)
    acc = (c["acc"].reshape(B, tpc, D) + pos[1:]).contiguous()
    mag = c["mag"].reshape(B, tpc, D) + pos[1:].abs()
    return dict(c, pos=pos, acc=acc, mag=mag, tpc=tpc)


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("T,B,tpf,D,K", PATCH_EMBED_CASES)
def test_patch_embed_fwd(T, B, tpf, D, K, split, monkeypatch):
    c = patch_embed_case(T, B, tpf, D, K, split)
    assert_budget(c["mag"], split, "patch_embed")
    setenv(monkeypatch, {})
    tpc = c["tpc"]
    x = torch.full((B, 1 + tpc, D), 5.0, device=DEV)
    r = run(ops.patch_embed_fwd, to_bt(c["x"]), to_bt(c["w"]), f32_dev(c["bias"]), f32_dev(c["pos"]), x, B, tpc, D, K)
    want_route(r, "gemm", f"patch_embed_fwd T = {T}")
    check_f32(x[:, 1:].contiguous(), c["acc"], "patch_embed_fwd", r)
    assert (x[:, 0] == 5.0).all(), "patch_embed_fwd touched the cls rows"


@pytest.mark.parametrize("case,split", CONV_PARAMS)
def test_conv_routes(case, split, monkeypatch):
    """Forward (+ bias; dropout p = 0, no BatchNorm fold), data gradient, weight gradient (+= on an initial buffer) and bias gradient of the
    3 x 3 / k x k convolutions and the ConvTranspose on every engine route."""
    name, kind, env, B, H, W, Cin, Cout, ks, _, routes = case
    c = conv_case(kind, B, H, W, Cin, Cout, split, ks)
    conv_budgets(c, name)
    setenv(monkeypatch, env)
    si = 1 if split else 0
    Ho, Wo = c["Ho"], c["Wo"]
    x, w, dy = to_bt(c["x"]), to_bt(c["w"]), to_bt(c["dy"])
    if "fwd" in routes:
        y = BT.zeros((B, Ho, Wo, Cout), split, DEV)
        if kind == "convT":
            r = run(ops.convT_fwd, x, w, f32_dev(c["bias"]), y, B, H, W, Cin, Cout)
        else:
            r = run(ops.conv_fwd, x, w, f32_dev(c["bias"]), y, B, H, W, Cin, Cout, ks)
        want_route(r, routes["fwd"][si], f"{name} fwd")
        check_bt(y, c["y"], f"{name} fwd", r)
    if "dgrad" in routes:
        dx = BT.zeros((B, H, W, Cin), split, DEV)
        if kind == "convT":
            r = run(ops.convT_dgrad, dy, w, dx, B, H, W, Cin, Cout)
        else:
            r = run(ops.conv_dgrad, dy, w, dx, B, H, W, Cin, Cout, ks)
        want_route(r, routes["dgrad"][si], f"{name} dgrad")
        check_bt(dx, c["dx"], f"{name} dgrad", r)
    if "wgrad" in routes:
        dw, db = f32_dev(c["dw0"]), f32_dev(c["db0"])
        from instageo_amd import _lib

        _lib.load().ig_note_reset()
        if kind == "convT":
            ops.convT_wgrad(dy, x, dw, B, H, W, Cin, Cout, dbias=db)
        else:
            ops.conv_wgrad(dy, x, dw, B, H, W, Cin, Cout, ks, dbias=db)
        r = ops.last_kernel()
        want_route(r, routes["wgrad"][si], f"{name} wgrad")
        check_f32(dw, c["dw"], f"{name} wgrad (+=)", r)
        check_f32(db, c["db"], f"{name} bias gradient (+=)", r)


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("M,C", COLSUM_CASES)
def test_colsum(M, C, split):
    c = colsum_case(M, C, split)
    colsum_budget(c)
    out = f32_dev(c["out0"])
    ops.colsum(to_bt(c["x"]), out, M, C)
    check_f32(out, c["acc"], f"colsum {M}x{C}", "ig_colsum")


def ulp32(v):
    """Spacing of fp32 numbers at |v| (float64 tensor)."""
    v = v.abs().clamp_min(2.0**-126)
    return torch.pow(2.0, torch.floor(torch.log2(v)) - 23)


@pytest.mark.parametrize("C", [1, 48, 257])
def test_bn_eval_affine(C):
    """scale = gamma * rsqrt(var + eps), shift = beta - mean * scale.  The only check here that is not exact: rsqrt is not.  scale against float64
    within 2 fp32 ulps; shift against the float64 value of beta - mean * (the scale the kernel stored): that is two fp32 roundings (the
    product and the difference, or one for a fused multiply-add), at most 1/2 ulp of the product + 1/2 ulp of the result, so within the same
    2 ulps taken at the larger of the two magnitudes."""
    g = torch.Generator().manual_seed(C)
    gamma, beta = 0.5 + torch.rand(C, generator=g), torch.randn(C, generator=g)
    mean, var = torch.randn(C, generator=g), 0.05 + 4 * torch.rand(C, generator=g)
    scale, shift = torch.full((C,), 9.0, device=DEV), torch.full((C,), 9.0, device=DEV)
    eps = 1e-5
    ops.bn_eval_affine(gamma.to(DEV), beta.to(DEV), mean.to(DEV), var.to(DEV), scale, shift, C, eps)
    eps32 = float(np.float32(eps))
    sc_ref = gamma.double() / torch.sqrt(var.double() + eps32)
    sc, sh = scale.cpu().double(), shift.cpu().double()
    err = ((sc - sc_ref).abs() / ulp32(sc_ref)).max().item()
    print(f"bn_eval_affine C = {C}: scale error {err:.3f} ulp")
    assert err <= 2.0, f"scale: {err} ulp"
    prod = mean.double() * sc
    sh_ref = beta.double() - prod
    err = ((sh - sh_ref).abs() / ulp32(torch.maximum(prod.abs(), sh_ref.abs()))).max().item()
    print(f"bn_eval_affine C = {C}: shift error {err:.3f} ulp")
    assert err <= 2.0, f"shift: {err} ulp"
