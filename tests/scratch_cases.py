"""The table of the scratch-carry-over tests: every slot of ``IgScratchSlot`` (csrc/common.h) -> the tests of
tests/test_gpu_scratch_carryover.py that run probe -> dirty -> probe on it.  tests/test_cpu_scratch_slots.py checks the table against the
enum and against the test file, so a new slot cannot arrive untested.  Nothing here imports torch."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON_H = os.path.join(ROOT, "instageo-e2e-geospatial-ml_amd", "csrc", "common.h")
GPU_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_scratch_carryover.py")

SLOT_TESTS = {
    "IG_SLOT_BN_PARTIALS": ["test_bn_partials_double_float_and_conv_statistics"],
    "IG_SLOT_CONV8_WEIGHTS": ["test_conv8_packed_weights_and_table"],
    "IG_SLOT_LOSS_TOTALS": ["test_loss_totals_ticket_shared_by_three_entry_points"],
    "IG_SLOT_CE_ACC": ["test_ce_accumulators_and_region_sums"],
    "IG_SLOT_WGRAD_SLABS": ["test_wgrad_slabs_grouped"],
    "IG_SLOT_SPLITK": ["test_splitk_linear_wgrad", "test_splitk_conv_wgrads"],
    "IG_SLOT_REGION_SUMS": ["test_ce_accumulators_and_region_sums"],
    "IG_SLOT_CALIB_NLL": ["test_calib_nll_partials"],
    "IG_SLOT_SPLIT_NEAREST": ["test_split_nearest_candidates"],
}


def enum_slots(path=COMMON_H):
    """[(name, value)] of ``enum IgScratchSlot`` without its count member, in file order."""
    with open(path) as f:
        text = f.read()
    m = re.search(r"enum\s+IgScratchSlot\s*\{(.*?)\}", text, re.S)
    assert m, "enum IgScratchSlot not found in common.h"
    body = re.sub(r"//[^\n]*", "", m.group(1))
    out = []
    for name, val in re.findall(r"(\w+)\s*=\s*(\d+)", body):
        out.append((name, int(val)))
    count = [v for n, v in out if n == "IG_SCRATCH_SLOTS"]
    assert count, "IG_SCRATCH_SLOTS not found"
    return [(n, v) for n, v in out if n != "IG_SCRATCH_SLOTS"], count[0]


def gpu_test_names(path=GPU_FILE):
    with open(path) as f:
        return set(re.findall(r"^def (test_\w+)\(", f.read(), re.M))
