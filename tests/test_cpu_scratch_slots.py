"""Every scratch slot of the library (``IgScratchSlot``, csrc/common.h) has a carry-over test: the table of tests/scratch_cases.py names
every member of the enum, and every test it names exists in tests/test_gpu_scratch_carryover.py."""
import scratch_cases as SC


def test_the_enum_is_dense_and_counted():
    slots, count = SC.enum_slots()
    assert [v for _, v in slots] == list(range(count)) and count == len(slots) >= 9


def test_every_slot_has_a_carryover_test():
    slots, _ = SC.enum_slots()
    names = [n for n, _ in slots]
    assert sorted(SC.SLOT_TESTS) == sorted(names), (set(names) ^ set(SC.SLOT_TESTS))
    have = SC.gpu_test_names()
    for slot, tests in SC.SLOT_TESTS.items():
        assert tests, f"{slot}: no test named"
        for t in tests:
            assert t in have, f"{slot}: {t} is not in test_gpu_scratch_carryover.py"


def test_every_carryover_test_is_in_the_table():
    named = {t for ts in SC.SLOT_TESTS.values() for t in ts}
    assert SC.gpu_test_names() == named
