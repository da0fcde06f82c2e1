"""Every stage variant of the LDS-tiled tendency kernel k_tendency_tile at ragged shapes, walls included: its fast 64 x 4 and 64 x 8
bodies (tile4, tile8), the strict 64 x 8 body (strict) and the fast and strict wall bodies (wall, wall-strict), each call against
the reference of tests/stage_cases.py (pinned on the CPU by tests/test_stage_cases_cpu.py).

One test = one (path, shape, formulation x forcing, precision, WRAP flags, topology) of stage_cases.tile_matrix(); it makes all 19
calls of stage_cases.calls() through the C-ABI with the flags of its path and asserts per call what tests/test_stage_matrix_gpu.py
asserts of the marching kernels: every written output finite and, on the fast paths, within the header's tolerance of the float64
oracle and a longdouble substep over the whole row range (max-norm) -- on the strict paths bitwise the oracle's tendencies and
substep in the precision of the call; every output the call must not write (Gn of the anchor second stage with store_G = 1
included), every output halo and every row outside [j_begin, j_end) bitwise as before; the inputs bitwise unchanged; with a WRAP
flag the halos of that direction of all four inputs are NaN on entry.  The strict and wall paths refuse the previous-state and anchor
forms: SWMHD_ENOTSUP and every buffer of the call bitwise untouched.  A Bounded case also asserts that its oracle reference differs
from the periodic one inside the wall buffers and nowhere else.  The layout each shape is there for (tile columns, tile rows, rows
of a tile) is asserted from swmhd_tendency_launch_geometry; for the wall kernel, which the query does not model, from
stage_cases.wall_tiles.

Achieved error / bound ratios: profiles/stage_matrix/ (tools/stage_matrix_report.py --tile)."""
import os

import pytest

import stage_cases as SC

pytestmark = pytest.mark.gpu
CASES = list(SC.tile_matrix())
KNOBS = ("SWMHD_ENS_RY", "SWMHD_ENS_MAP", "SWMHD_T_NT", "SWMHD_T_LY")


@pytest.mark.parametrize("path,Nx,Ny,rows,form,lor,dtype,flags,topo", CASES, ids=[SC.tile_case_id(*c) for c in CASES])
def test_tile_stage_matrix(swmhd, oracle, path, Nx, Ny, rows, form, lor, dtype, flags, topo):
    assert not any(os.environ.get(k) for k in KNOBS), "layout knobs set: the planner's default is not what runs"
    nrows = Ny if rows is None else rows[1] - rows[0]
    print(SC.check_layout(swmhd._lib, Nx, nrows, form, dtype, flags, path=path))
    failures = SC.run_cases(swmhd, oracle, Nx, Ny, rows, form, lor, dtype, flags, path=path, topo=topo)
    assert not failures, "\n".join(failures)
