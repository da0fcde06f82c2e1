"""Every stage variant of the ensemble instantiations of the LDS-tiled tendency kernel, k_tendency_tile<..., ENS = true, PAR = false |
true>, member by member at ragged shapes: the scalar entry points swmhd_ensemble_tendencies_rk3_* on 64 x 4 tiles (ens4), on 64 x 8
tiles with members above 0.33 Mcell (ens8) and strict (ens-strict), and the per-member-parameter entry points
swmhd_ensemble_tendencies_rk3_params_* fast and strict (par4, par-strict), each call against the reference of tests/stage_cases.py
(pinned on the CPU by tests/test_stage_cases_cpu.py, which also shows that the check catches swapped members, a shared operand, a
shared row of the parameter table and a write into a gap or the row padding).

One test = one (path, shape, members, layout, formulation x forcing, precision, WRAP flags) of stage_cases.ens_matrix(); it makes the
18 calls of stage_cases.ens_calls() (there is no ensemble form of T) on 1, 3 or 5 members -- 2 on ens8 -- that share no field, operand
included, in pitched family buffers (stride_y = Nx + 2 H + 5, stride_m = (Ny + 2 H) stride_y + 37; one case dense), and asserts per
call and member what tests/test_tile_stage_matrix_gpu.py asserts of a single grid: every written output finite and within the header's
tolerance of that member's float64 oracle and longdouble substep -- on the strict paths bitwise the oracle's tendencies and substep in
the precision of the call, with the member's g, f and dt on the par paths; every output the call must not write, every output halo,
the row padding and the member gaps of every output family, every input and operand bitwise as before; with a WRAP flag the halos of
that direction of every member's inputs NaN on entry.  On ens4 every member is also bitwise the same call made through
swmhd_tendencies_rk3_* with SWMHD_TILE_KERNEL on the member alone (the header's promise for fast members below ~0.33 Mcell).  The
previous-state forms are refused on every path and the anchor forms on the strict ones: SWMHD_ENOTSUP and every buffer bitwise
untouched.  The layout each shape is there for is asserted from swmhd_tendency_launch_geometry for a single grid of the member's
shape, which is the ensemble's plan, and from swmhd_ensemble_launch_geometry, which also gives the member mapping and the grid.

Achieved error / bound ratios: profiles/stage_matrix/ (tools/stage_matrix_report.py --ensemble)."""
import json
import os
import subprocess
import sys

import pytest

import stage_cases as SC

pytestmark = pytest.mark.gpu
CASES = list(SC.ens_matrix())
KNOBS = ("SWMHD_ENS_RY", "SWMHD_ENS_MAP", "SWMHD_T_NT", "SWMHD_T_LY")


@pytest.mark.parametrize("path,Nx,Ny,members,form,lor,dtype,flags,dense", CASES, ids=[SC.ens_case_id(*c) for c in CASES])
def test_ensemble_stage_matrix(swmhd, oracle, path, Nx, Ny, members, form, lor, dtype, flags, dense):
    assert not any(os.environ.get(k) for k in KNOBS), "layout knobs set: the planner's default is not what runs"
    line = SC.check_ens_layout(swmhd._lib, path, Nx, Ny, members, form, dtype, flags)
    print(line)
    assert f"grid {SC.ens_workgroups(path, Nx, Ny, members)} x 1" in line
    failures = SC.run_ens_cases(swmhd, oracle, path, Nx, Ny, members, form, lor, dtype, flags, dense)
    assert not failures, "\n".join(failures)


def test_forced_layouts(swmhd, tmp_path):
    """The two layouts the ensemble launcher makes only under its read-once knobs, in fresh child processes (stage_cases.ENS_FORCED):
    the member in blockIdx.y (SWMHD_ENS_MAP=2 on ens4 and par-strict) and 64 x 8 fast tiles at small shapes (SWMHD_ENS_RY=2 on ens4 and par4:
    one-row and one-column last tiles of that body), at 65 x 9 and 129 x 31 with 3 pitched members for (1, 1) and (0, 2) in fp64 and
    fp32, with WRAP_X | WRAP_Y.  Each child makes all calls with the assertions of test_ensemble_stage_matrix (under
    SWMHD_ENS_RY=2 without the bitwise single-grid comparison, which it only reports) and stops at its first failure; the second child
    starts only if the first passed.  That the knob took effect is read back from the library in the child
    (swmhd_ensemble_launch_geometry: blockIdx.y with a grid of tiles x members, or tile rows of 8) and asserted again here."""
    for name, cfg in SC.ENS_FORCED.items():
        env = {k: v for k, v in os.environ.items() if k not in KNOBS}
        env.update(cfg["env"])
        out = tmp_path / f"{name}.json"
        r = subprocess.run([sys.executable, SC.__file__, name, str(out)], env=env, capture_output=True, text=True, timeout=300)
        res = json.load(open(out)) if out.exists() else None
        assert r.returncode == 0 and res and res["ok"], (name, res and res["failed"], r.stdout[-3000:], r.stderr[-3000:])
        print(name, json.dumps(res["layouts"], indent=1), json.dumps(res["worst"], sort_keys=True), json.dumps(res["observed"]))
        assert res["env"] == cfg["env"] and len(res["layouts"]) == len(SC.ens_forced_cases(name))
        fast = [line for cid, line in res["layouts"].items() if cid.startswith(("ens4", "par4"))]
        assert fast and all((" tile rows of 8" in line and "forced from 4" in line) if cfg["ty"] == 8 else " tile rows of 4" in line for line in fast)
        want = "member in blockIdx.y, grid" if cfg["member_map"] == 2 else "member in blockIdx.x, grid"
        assert all(want in line and (cfg["member_map"] == 1 or line.endswith(f" x {SC.ENS_FORCED_MEMBERS}")) for line in res["layouts"].values())
