"""The Python host layer makes the calls into libswmhd.so that it made before its paths were folded into shared helpers: every entry
point, in order, with every argument and with each buffer in the role it had (host_call_cases: the scenarios, the recorder and how
tests/golden/host_calls.json was recorded)."""
import json

import pytest

import host_call_cases as HC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return HC.load_golden()


def test_golden_covers_the_scenarios(golden):
    assert sorted(golden) == sorted(HC.SCENARIOS)


def test_arguments_that_leave_no_correction_change_no_call(swmhd, golden):
    """closure= with all coefficients 0, forcing={} and coriolis=FPlane(f): argument by argument the calls of the model built without
    them, now and in the recording."""
    given, plain = (json.loads(json.dumps(HC.run(swmhd, name))) for name in ("H_absent_given", "H_absent_plain"))
    assert given == plain
    assert golden["H_absent_given"] == golden["H_absent_plain"]


@pytest.mark.parametrize("name", sorted(HC.SCENARIOS))
def test_host_calls_are_the_recorded_ones(swmhd, golden, name):
    got = json.loads(json.dumps(HC.run(swmhd, name)))
    want = golden[name]
    assert [label for label, _ in got] == [label for label, _ in want]
    for (label, calls), (_, recorded) in zip(got, want):
        for k, (a, b) in enumerate(zip(calls, recorded)):
            assert a == b, f"{name}, {label}, call {k}"
        assert len(calls) == len(recorded), f"{name}, {label}: {[c[0] for c in calls]} != {[c[0] for c in recorded]}"
    assert got == want
