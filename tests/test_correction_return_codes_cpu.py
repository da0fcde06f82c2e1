"""Which return code wins (no GPU) for the four per-stage correction launches: all sixteen entry points of _lib.CORIOLIS_EXPORTS,
DIFFUSION_EXPORTS, BIHARMONIC_EXPORTS and RELAXATION_EXPORTS with one argument defect, with every pair of defects, and the empty calls
that return before any launch, against tests/golden/correction_return_codes.json -- the answers of the library before the checks these
calls share were gathered in shared helpers (tests/correction_return_code_cases.py: the cases and the recorder).  Their ABI tests pin
single defects; which code answers two defects at once is the order of the checks, and that order is behaviour."""
import pytest
import torch

import correction_return_code_cases as CRC

# With a device a library that wrongly accepted a defect case would launch on host pointers.
pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="the cases pass host pointers: only without a device")

ENTRIES = CRC.entries()


@pytest.fixture(scope="module")
def golden():
    return CRC.load_golden()


def test_every_entry_point_has_cases(swmhd, golden):
    assert CRC.launching(swmhd._lib) == {sym for _, sym, _, _ in ENTRIES} and len(ENTRIES) == 16
    assert set(golden) == {key for key, _, _, _ in ENTRIES}


@pytest.mark.parametrize("entry", ENTRIES, ids=[e[0] for e in ENTRIES])
def test_return_codes_are_the_recorded_ones(swmhd, golden, entry):
    key, sym, name, sfx = entry
    cases = CRC.cases(name)
    want = golden[key]
    assert len(want) == len(cases) > 500, "the golden file was recorded for another list of cases"
    assert {"0", "1", "3", "L"} <= set(want) and ("2" in want) == ("relaxation" not in name)      # every answer these calls have is in the matrix
    L = swmhd._lib.lib()
    assert CRC.call(L, sym, name, sfx, {}) == CRC.NO_DEVICE     # the baseline gets past every check: it reaches HIP (no device)
    got = CRC.run(L, entry)
    wrong = [f"{label}: {g}, recorded {w}" for (_, label, _), g, w in zip(cases, got, want) if g != w]
    assert not wrong, f"{len(wrong)} of {len(cases)} cases:\n" + "\n".join(wrong[:20])
