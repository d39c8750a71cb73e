"""Self-check of tests/attention_reference.py on the CPU (no GPU): the reference is accurate far inside every bar, every input kind
moves an output far past its bar under the tail fault it answers for, and the committed table of emulation errors and plain-mode bars
is what the emulation measures.  ``-s`` shows the fault-sensitivity table."""
import functools

import pytest

import attention_reference as AR

NS = (33, 193, 226, 273)
HDS = (64, 80)


@functools.lru_cache(maxsize=None)
def case(kind, hd, N, split=False):
    qkv, dout = AR.rounded_operands(kind, N, hd, split)
    return qkv, dout, AR.reference(qkv, dout, AR.H, hd)


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("kind", AR.KINDS)
def test_fp32_torch_is_within_a_tenth_of_every_bar(kind, hd, N, split):
    qkv, dout, ref = case(kind, hd, N, split)
    t32 = AR.reference(qkv.float(), dout.float(), AR.H, hd)
    for what in AR.OUTPUTS:
        err, bar = AR.rel_err(t32[what], ref[what]), AR.bar(kind, hd, what, split)
        assert err <= 0.1 * bar, f"{kind} hd {hd} N {N} {what}: fp32 torch is {err:.3e} off float64, bar {bar:.3e}"


def sensitivity(kind, hd, N, fault):
    """{output: error of the faulty evaluation / plain bar of that output}."""
    qkv, dout, ref = case(kind, hd, N)
    bad = AR.FAULTS[fault](qkv, dout, AR.H, hd)
    return {what: AR.rel_err(bad[what], ref[what]) / AR.bar(kind, hd, what, False) for what in AR.OUTPUTS}


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("kind,fault", [(kind, fault) for kind, faults in AR.RESPONSIBLE.items() for fault in faults])
def test_each_kind_exposes_the_fault_it_answers_for(kind, fault, hd, N):
    ratio = sensitivity(kind, hd, N, fault)
    print(f"SEAM {kind:9s} {fault:21s} hd {hd} N {N:3d}  error / plain bar: " + "  ".join(f"{w} {r:8.1f}" for w, r in ratio.items()))
    assert max(ratio.values()) >= 5.0, f"{fault} on {kind} inputs moves no output by 5 x its plain bar: {ratio}"


@pytest.mark.parametrize("hd", HDS)
def test_random_inputs_hide_a_phantom_key(hd):
    """The gap the tail-amplifying kinds close: on i.i.d. normal inputs at N = 193 a zero row counted as a key stays under the plain out bar."""
    ratio = sensitivity("random", hd, 193, "appended zero key")
    print(f"SEAM random    appended zero key     hd {hd} N 193  error / plain bar: " + "  ".join(f"{w} {r:8.2f}" for w, r in ratio.items()))
    assert ratio["out"] < 1.0, ratio


def test_the_bars_table_is_what_the_emulation_measures():
    """Every (kind, hd, output) is listed; the error is the emulation's (to the table's four digits; a BLAS may reorder a sum) and
    no bar is looser than max(project bar, 4 x the emulation's error)."""
    measured = AR.measure_emulation()
    assert set(AR.PLAIN_BARS) == {(kind, hd) for kind in AR.KINDS for hd in HDS}
    for key, row in AR.PLAIN_BARS.items():
        assert tuple(row) == AR.OUTPUTS
        for what, (err, bar) in row.items():
            project = AR.PROJECT_BARS[what][0]
            assert abs(err - measured[key][what]) <= 2e-3 * err + 1e-12, f"{key} {what}: table {err:.3e}, measured {measured[key][what]:.3e}"
            assert project <= bar <= max(project, 4.0 * err), f"{key} {what}: bar {bar:.3e} against project {project:.3e} and 4 x {err:.3e}"
            print(f"SEAM bars {key[0]:9s} hd {key[1]} {what:3s}  emulation {err:.3e}  project {project:.1e}  bar {bar:.3e}")
