"""Every call form of the tracer stage kernel k_tracers_tile at ragged shapes, walls included: its fast periodic body (fast), the fast
Bounded body (wall) and the strict Bounded body (wall-strict), each call against the reference of tests/tracer_stage_cases.py (pinned
on the CPU by tests/test_tracer_stage_cases_cpu.py).  Periodic strict stays with tests/test_tracers_gpu.py::test_strict_stage_matrix.

One test = one (path, shape, topology, formulation, precision, halo mode) of tracer_stage_cases.matrix(); over all rows and over rows
[2, Ny - 3) it makes the 23 calls of tracer_stage_cases.calls() through swmhd_tracers_rk3_* -- the 19 of stage_cases.calls() with
K = 3 distinct tracers and operands, S2g again with K = 1 and K = 8 -- on pitched parents (stride_y = Nx + 2 H + 5), and asserts per
call: every written output finite and, on the fast paths, within the header's tolerance of the float64 oracle and a longdouble update
over the rows of the call (max-norm), per tracer -- on wall-strict bitwise the oracle's tendency and substep in the precision of the
call; every output the call must not write (Gn with store_G = 0, Gn of the anchor second stage although store_G = 1, W under an
aliased Gn), every halo, every pad column and every row outside the range bitwise as before; the inputs and the operand bitwise
unchanged.  Halo mode "wrap": the WRAP flag of every periodic direction with NaN in those halos of q1, q2, h and every c; "filled":
no WRAP flag.  Bounded directions always hold the boundary conditions in their halos.  A form the path refuses
(SWMHD_GM_IS_PREV_STATE everywhere, SWMHD_RK3_ANCHOR with a Bounded direction or SWMHD_STRICT) returns SWMHD_ENOTSUP and leaves every
buffer of the call bitwise untouched.  A Bounded case also asserts that its oracle reference differs from the periodic one inside
the wall buffers and nowhere else, per tracer.  The tiles each shape is there for are asserted from tracer_tiles' arithmetic.

Achieved error / bound ratios: profiles/tracer_stage_matrix/ (tools/stage_matrix_report.py --tracers)."""
import pytest

import tracer_stage_cases as TS

pytestmark = pytest.mark.gpu
CASES = list(TS.matrix())


@pytest.mark.parametrize("path,Nx,Ny,topo,form,dtype,wrap", CASES, ids=[TS.case_id(*c) for c in CASES])
def test_tracer_stage_matrix(swmhd, oracle, path, Nx, Ny, topo, form, dtype, wrap):
    failures = TS.run_cases(swmhd, oracle, path, Nx, Ny, topo, form, dtype, wrap)
    assert not failures, "\n".join(failures)
