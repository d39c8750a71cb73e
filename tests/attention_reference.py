"""Attention at tile and chunk seams: inputs that amplify a tail fault, the float64 reference, float64 emulations of the classic tail
faults and of the plain-bf16 kernels' two rounding points, and the accuracy bars of tests/test_cpu_attention_seams.py and
tests/test_gpu_attention_seams.py.  Plain torch on the CPU: nothing here is shared with instageo_amd.

Layout as in csrc/attention.hip: qkv [B, N, 3, H, hd] (flattened to [B, N, 3 H hd]), out and dout [B, N, H hd], lse [B, H, N].

Input kinds (``operands``), each built so that one kind of tail fault moves an output by tens of per cent instead of the fraction of a
per cent it moves i.i.d. normal inputs (u = the unit vector with every component hd^-1/2):

* ``random``     i.i.d. normal qkv and dout, what test_gpu_ops.py runs.
* ``lastkey``    q = sqrt(hd) u + 0.05 noise, k = 0.05 noise, k[N-1] = ln(N-1) u, v[N-1] = 4: every key but the last scores ~0, the
                 last ln(N-1), so the last key holds about half of every row's weight.  Counting it twice or dropping it moves out.
* ``negative``   q = C_Q sqrt(hd) u + 0.2 noise, k = -C_K u + 0.2 noise: every real score is about -C_Q C_K = -10 (-6 to -14), so a
                 phantom key with score 0 (a zero-filled or unmasked row) takes 95 % of every row at N = 800 and more below.  The offset
                 is no larger because fp32 arithmetic itself loses ~|score| sqrt(hd) ulps in the exp argument (_SPLIT_EXP in
                 test_gpu_value_ranges.py): at -20 torch's fp32 is already 4e-6 off in out, above a tenth of the split bar.
* ``lastquery``  ``random`` with dout[N-1] x 8: the last query dominates dk and dv, so counting it twice in the key-owner pass shows.

Bars.  Every bar is a relative max error against the largest reference value of that output (dq, dk and dv each against its own third).
PROJECT_BARS are the numbers of test_attention_fwd_bwd / test_attention_generic_head_dim.  ``lastkey`` and ``negative`` give the keys a
common component by construction, and the suite already records (test_gpu_value_ranges.py, _BF16_DS) that the bf16 rounding of dS leaks
such a component into dq.  ``emulate_bf16`` is the float64 evaluation with P and dS rounded to bf16 before the second products (the
kernels' rounding points: csrc/attention2.hip, "P^T as the B operand of the next product"); where four times its error (the margin for
fp32 accumulation order on top of the two roundings) exceeds the project bar, the plain-mode bar of that output is four times the
emulation's error.  PLAIN_BARS holds the measured errors (maximum over EMULATION_NS; ``python tests/attention_reference.py`` prints the
table, test_cpu_attention_seams.py checks it).  The split-mode bars are the project's, unchanged.  No bar comes from a kernel's output.
"""
import functools
import math

import torch

KINDS = ("random", "lastkey", "negative", "lastquery")
OUTPUTS = ("out", "lse", "dq", "dk", "dv")
B, H = 2, 3
C_Q, C_K = 5.0, 2.0

# relative max error against the largest reference value: {output: (plain bf16, split bf16x3)}
PROJECT_BARS = {"out": (1e-2, 3e-5), "lse": (2e-3, 1e-5), "dq": (2e-2, 1e-4), "dk": (2e-2, 1e-4), "dv": (2e-2, 1e-4), "dbias": (6e-3, 2e-5)}

# token counts the emulation is measured at: one per side of every seam class of both kernel files (a tile, a workgroup, a chunk, two)
EMULATION_NS = (33, 193, 226, 273, 449, 545)

# (kind, hd): {output: (measured relative max error of emulate_bf16 against the float64 reference, maximum over EMULATION_NS; the plain-mode
# bar that follows: max(project bar, 4 x error))}.  lse has no rounding point before it: its error is zero and its bar the project's.
PLAIN_BARS = {
    ("random", 64): {"out": (2.424e-03, 1.000e-02), "lse": (0.000e+00, 2.000e-03), "dq": (2.399e-03, 2.000e-02), "dk": (2.597e-03, 2.000e-02), "dv": (1.969e-03, 2.000e-02)},
    ("random", 80): {"out": (2.401e-03, 1.000e-02), "lse": (0.000e+00, 2.000e-03), "dq": (2.622e-03, 2.000e-02), "dk": (2.495e-03, 2.000e-02), "dv": (2.615e-03, 2.000e-02)},
    ("lastkey", 64): {"out": (3.633e-03, 1.453e-02), "lse": (0.000e+00, 2.000e-03), "dq": (2.676e-03, 2.000e-02), "dk": (2.064e-03, 2.000e-02), "dv": (1.907e-03, 2.000e-02)},
    ("lastkey", 80): {"out": (3.645e-03, 1.457e-02), "lse": (0.000e+00, 2.000e-03), "dq": (3.481e-03, 2.000e-02), "dk": (3.379e-03, 2.000e-02), "dv": (2.337e-03, 2.000e-02)},
    ("negative", 64): {"out": (3.548e-03, 1.419e-02), "lse": (0.000e+00, 2.000e-03), "dq": (3.908e-03, 2.000e-02), "dk": (2.586e-03, 2.000e-02), "dv": (2.204e-03, 2.000e-02)},
    ("negative", 80): {"out": (3.029e-03, 1.211e-02), "lse": (0.000e+00, 2.000e-03), "dq": (4.395e-03, 2.000e-02), "dk": (2.236e-03, 2.000e-02), "dv": (2.721e-03, 2.000e-02)},
    ("lastquery", 64): {"out": (2.133e-03, 1.000e-02), "lse": (0.000e+00, 2.000e-03), "dq": (2.800e-03, 2.000e-02), "dk": (3.234e-03, 2.000e-02), "dv": (3.087e-03, 2.000e-02)},
    ("lastquery", 80): {"out": (2.754e-03, 1.101e-02), "lse": (0.000e+00, 2.000e-03), "dq": (2.269e-03, 2.000e-02), "dk": (3.226e-03, 2.000e-02), "dv": (2.980e-03, 2.000e-02)},
}


def bar(kind, hd, what, split):
    """The bar of output ``what`` on inputs of ``kind``: the project's, or in plain mode 4 x the emulation's error where that is larger."""
    plain, tight = PROJECT_BARS[what]
    if split:
        return tight
    return PLAIN_BARS[(kind, hd)][what][1] if what in OUTPUTS else plain


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def operands(kind, N, hd, B=B, H=H):
    """(qkv [B, N, 3 H hd], dout [B, N, H hd]) in fp32, before the rounding to what the kernel sees."""
    assert kind in KINDS and (N >= 2 or kind in ("random", "lastquery"))
    g = torch.Generator().manual_seed(1000 * KINDS.index(kind) + 7 * N + hd)
    q, k, v = (torch.randn(B, N, H, hd, generator=g) for _ in range(3))
    dout = torch.randn(B, N, H * hd, generator=g)
    u = hd**-0.5
    if kind == "lastkey":
        q = 0.05 * q + hd**0.5 * u
        k = 0.05 * k
        k[:, N - 1] = math.log(N - 1) * u
        v[:, N - 1] = 4.0
    elif kind == "negative":
        q = 0.2 * q + C_Q * hd**0.5 * u
        k = 0.2 * k - C_K * u
    elif kind == "lastquery":
        dout[:, N - 1] *= 8.0
    return torch.stack([q, k, v], 2).reshape(B, N, 3 * H * hd).contiguous(), dout


def round_bf16(x, split=False):
    """float64 value of ``x`` rounded to bf16 (round to nearest even), or to bf16 hi + bf16 lo of the remainder (split)."""
    x = x.float()
    hi = x.to(torch.bfloat16).float()
    if split:
        hi = hi + (x - hi).to(torch.bfloat16).float()
    return hi.double()


def rounded_operands(kind, N, hd, split, B=B, H=H):
    """The operands as the kernel sees them (float64), by the CPU restatement of the rounding."""
    qkv, dout = operands(kind, N, hd, B, H)
    return round_bf16(qkv, split), round_bf16(dout, split)


def unpack(qkv, dout, H, hd):
    """q, k, v, dout as [B, H, N, hd]."""
    Bn, N = qkv.shape[:2]
    q, k, v = qkv.reshape(Bn, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    return q, k, v, dout.reshape(Bn, N, H, hd).transpose(1, 2)


def _tokens_first(x):  # [B, H, N, hd] -> [B, N, H hd]
    return x.transpose(1, 2).reshape(x.shape[0], x.shape[2], -1)


# ---------------------------------------------------------------------------------------------------------------------------------
# reference (attn_torch of test_gpu_value_ranges.py, with keys and queries that may differ in number) and the fault emulations
# ---------------------------------------------------------------------------------------------------------------------------------
def _attention(q, k, v, do):
    """softmax(q k^T / sqrt(hd)) v and its gradients in the dtype of the arguments: q, do [B, H, Nq, hd], k, v [B, H, Nk, hd]."""
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    s = (q * q.shape[-1] ** -0.5) @ k.transpose(-2, -1)
    out = s.softmax(-1) @ v
    dq, dk, dv = torch.autograd.grad((out * do).sum(), [q, k, v])
    return dict(out=out.detach(), lse=torch.logsumexp(s, -1).detach(), dq=dq, dk=dk, dv=dv)


def _packed(r, N):
    """Kernel layouts of the first N rows: out, dq, dk, dv [B, N, H hd], lse [B, H, N]."""
    return {k: (t[:, :, :N] if k == "lse" else _tokens_first(t[:, :, :N])) for k, t in r.items()}


def reference(qkv, dout, H, hd):
    """out, lse, dq, dk, dv of the operands as given (float64 operands: the reference; fp32 operands: torch's own fp32)."""
    q, k, v, do = unpack(qkv, dout, H, hd)
    return _packed(_attention(q, k, v, do), qkv.shape[1])


def _extra(t, row):  # t with one more row along the token axis
    return torch.cat([t, row], 2)


def fault_duplicated_last_key(qkv, dout, H, hd):
    """The last key (and its value) counted twice."""
    q, k, v, do = unpack(qkv, dout, H, hd)
    return _packed(_attention(q, _extra(k, k[:, :, -1:]), _extra(v, v[:, :, -1:]), do), qkv.shape[1])


def fault_appended_zero_key(qkv, dout, H, hd):
    """One key past the end read as a zero row (score 0, value 0): a zero-filled or unmasked tail row."""
    q, k, v, do = unpack(qkv, dout, H, hd)
    z = torch.zeros_like(k[:, :, -1:])
    return _packed(_attention(q, _extra(k, z), _extra(v, z), do), qkv.shape[1])


def fault_dropped_last_key(qkv, dout, H, hd):
    """The last key never visited: its dk and dv stay zero."""
    q, k, v, do = unpack(qkv, dout, H, hd)
    r = _attention(q, k[:, :, :-1], v[:, :, :-1], do)
    z = torch.zeros_like(k[:, :, -1:])
    r["dk"], r["dv"] = _extra(r["dk"], z), _extra(r["dv"], z)
    return _packed(r, qkv.shape[1])


def fault_duplicated_last_query(qkv, dout, H, hd):
    """The last query counted twice in the key-owner (dK / dV) pass; out, lse and dq are those of the reference."""
    q, k, v, do = unpack(qkv, dout, H, hd)
    r = _attention(q, k, v, do)
    twice = _attention(_extra(q, q[:, :, -1:]), k, v, _extra(do, do[:, :, -1:]))
    r["dk"], r["dv"] = twice["dk"], twice["dv"]
    return _packed(r, qkv.shape[1])


FAULTS = {"duplicated last key": fault_duplicated_last_key, "appended zero key": fault_appended_zero_key,
          "dropped last key": fault_dropped_last_key, "duplicated last query": fault_duplicated_last_query}
# the faults each kind answers for: it moves at least one output by 5 x that output's plain bar
RESPONSIBLE = {"lastkey": ("duplicated last key", "dropped last key"), "negative": ("appended zero key",),
               "lastquery": ("duplicated last query",)}


def emulate_bf16(qkv, dout, H, hd):
    """float64 with the plain-bf16 kernels' two roundings: P to bf16 before P v and P^T dO, dS = P o (dP - delta) (from the unrounded P)
    to bf16 before dS k and dS^T q.  Row sums, lse and delta stay exact."""
    q, k, v, do = unpack(qkv, dout, H, hd)
    scale = hd**-0.5
    s = (q * scale) @ k.transpose(-2, -1)
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    pb = round_bf16(p)
    out = pb @ v
    delta = ((p @ v) * do).sum(-1, keepdim=True)
    dsb = round_bf16(p * (do @ v.transpose(-2, -1) - delta))
    r = dict(out=out, lse=lse, dq=(dsb @ k) * scale, dk=(dsb.transpose(-2, -1) @ q) * scale, dv=pb.transpose(-2, -1) @ do)
    return _packed(r, qkv.shape[1])


def rel_err(got, ref):
    """max |got - ref| / max |ref|."""
    return (got.double() - ref.double()).abs().max().item() / (ref.double().abs().max().item() + 1e-300)


@functools.lru_cache(maxsize=None)
def emulation_error(kind, hd, N):
    """{output: relative max error of emulate_bf16 against the reference} on the plain-bf16 operands."""
    qkv, dout = rounded_operands(kind, N, hd, False)
    ref, emu = reference(qkv, dout, H, hd), emulate_bf16(qkv, dout, H, hd)
    return {what: rel_err(emu[what], ref[what]) for what in OUTPUTS}


def measure_emulation():
    """The errors of PLAIN_BARS as measured now: the maximum over EMULATION_NS."""
    return {(kind, hd): {what: max(emulation_error(kind, hd, N)[what] for N in EMULATION_NS) for what in OUTPUTS}
            for kind in KINDS for hd in (64, 80)}


if __name__ == "__main__":
    print("measured = {")
    for key, row in measure_emulation().items():
        print(f"    {key!r}: {{" + ", ".join(f'"{w}": {e:.3e}' for w, e in row.items()) + "},")
    print("}")
