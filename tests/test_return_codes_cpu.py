"""Which return code wins (no GPU): every launching entry point of libswmhd.so with one argument defect, with every pair of defects,
and the empty calls that return before any launch, against tests/golden/return_codes.json -- the answers of the library before its
argument checks and flag decoding were gathered in csrc/api_args.hpp (tests/return_code_cases.py: the cases and the recorder).  The
ABI tests pin single defects; which code answers two defects at once is the order of the checks, and that order is behaviour."""
import pytest
import torch

import return_code_cases as RC

# With a device a library that wrongly accepted a defect case would launch on host pointers.
pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="the cases pass host pointers: only without a device")

ENTRIES = RC.entries()


@pytest.fixture(scope="module")
def golden():
    return RC.load_golden()


def test_every_launching_entry_point_has_cases(swmhd, golden):
    launching = {s for s in swmhd._lib.EXPORTS if s.endswith(("_f64", "_f32"))} | {"swmhd_tendency_launch_geometry"}
    assert launching == {sym for _, sym, _, _ in ENTRIES}
    assert set(golden) == {key for key, _, _, _ in ENTRIES}


@pytest.mark.parametrize("entry", ENTRIES, ids=[e[0] for e in ENTRIES])
def test_return_codes_are_the_recorded_ones(swmhd, golden, entry):
    key, _sym, name, _sfx = entry
    cases = RC.cases(name)
    want = golden[key]
    assert len(want) == len(cases), "the golden file was recorded for another list of cases"
    got = RC.run(swmhd._lib.lib(), entry)
    wrong = [f"{label}: {g}, recorded {w}" for (_, label, _), g, w in zip(cases, got, want) if g != w]
    assert not wrong, f"{len(wrong)} of {len(cases)} cases:\n" + "\n".join(wrong[:20])
