"""Which return code wins (no GPU) for the derived frames, the zonal spectra and the 2-D spectra: every launching entry point of
_lib.DERIVED_EXPORTS, SPECTRA_EXPORTS and SPECTRA2D_EXPORTS with one argument defect, with every pair of defects, and the empty calls
that return before any launch, against tests/golden/frame_return_codes.json -- the answers of the library before the checks these
calls share with the output frames were gathered in csrc/api_args.hpp (tests/frame_return_code_cases.py: the cases and the recorder).
Their ABI tests pin single defects; which code answers two defects at once is the order of the checks, and that order is behaviour."""
import pytest
import torch

import frame_return_code_cases as FRC

# With a device a library that wrongly accepted a defect case would launch on host pointers.
pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="the cases pass host pointers: only without a device")

ENTRIES = FRC.entries()


@pytest.fixture(scope="module")
def golden():
    return FRC.load_golden()


def test_every_launching_entry_point_has_cases(swmhd, golden):
    assert FRC.launching(swmhd._lib) == {sym for _, sym, _, _ in ENTRIES}
    assert set(golden) == {key for key, _, _, _ in ENTRIES}


@pytest.mark.parametrize("entry", ENTRIES, ids=[e[0] for e in ENTRIES])
def test_return_codes_are_the_recorded_ones(swmhd, golden, entry):
    key, sym, name, sfx = entry
    cases = FRC.cases(name)
    want = golden[key]
    assert len(want) == len(cases) > 100, "the golden file was recorded for another list of cases"
    assert {"1", "2"} <= set(want) and ("3" in want) == ("derived" not in name)      # every answer these calls have is in the matrix
    L = swmhd._lib.lib()
    assert FRC.call(L, sym, name, sfx, {}) == -100          # the baseline gets past every check: it reaches HIP (no device)
    got = FRC.run(L, entry)
    wrong = [f"{label}: {g}, recorded {w}" for (_, label, _), g, w in zip(cases, got, want) if g != w]
    assert not wrong, f"{len(wrong)} of {len(cases)} cases:\n" + "\n".join(wrong[:20])
