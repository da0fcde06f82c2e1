"""Every stage variant of the row-marching tendency kernels (k_tendency_vi_march, k_tendency_cons_march, k_tendency_vi_march_pk) at
ragged shapes, each call against the float64 oracle and a longdouble substep (tests/stage_cases.py, pinned on the CPU by
tests/test_stage_cases_cpu.py).

One test = one (shape, formulation x forcing, precision, WRAP flags); it makes all 19 calls of stage_cases.calls() -- the ten call forms
T, S1g, S1n, S2g, S3n, P2g, P3n, A1, A2, A2a with the RK3 coefficients and with a generic pair -- through the C-ABI with
SWMHD_MARCH_KERNEL, and asserts per call: every written output finite and within the header's tolerance over the whole row range
(max-norm); every output the call must not write, every output halo and every row outside [j_begin, j_end) bitwise as before; the
inputs bitwise unchanged; with a WRAP flag the halos of that direction of all four inputs are NaN on entry.  The layout each shape is
there for is asserted from swmhd_tendency_launch_geometry.  SWMHD_MARCH_KERNEL puts grids of a few thousand cells on these kernels,
where segments have their minimum of 6 rows: a 31-row grid has six segments, the last of one row.

Achieved error / bound ratios: profiles/stage_matrix/ (tools/stage_matrix_report.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import stage_cases as SC

pytestmark = pytest.mark.gpu
CASES = list(SC.matrix())


@pytest.mark.parametrize("Nx,Ny,rows,form,lor,dtype,flags", CASES, ids=[SC.case_id(*c) for c in CASES])
def test_stage_matrix(swmhd, oracle, Nx, Ny, rows, form, lor, dtype, flags):
    # (the fold of a last strip is inferred from the geometry, the query does not report it: the environment must not switch it off)
    assert SC.fold_enabled(), "SWMHD_T_FOLD=0 in the environment: the folded layouts of the matrix would not be exercised"
    assert not os.environ.get("SWMHD_T_NT") and not os.environ.get("SWMHD_T_LY"), "layout knobs set: the default chooser is not what runs"
    nrows = Ny if rows is None else rows[1] - rows[0]
    print(SC.check_layout(swmhd._lib, Nx, nrows, form, dtype, flags))
    failures = SC.run_cases(swmhd, oracle, Nx, Ny, rows, form, lor, dtype, flags)
    assert not failures, "\n".join(failures)


def test_forced_layouts(swmhd, tmp_path):
    """Layouts the default chooser never makes, through its read-once knobs in fresh child processes (stage_cases.FORCED): 128-lane
    strips with a one-column last strip (SWMHD_T_NT=128 at 123 and 489 columns), and segments of 13 rows on a 33-row grid
    (SWMHD_T_LY=13: 13 + 13 + 7) at 2501 and 600 columns.  Each child runs all calls for (1, 1) and (0, 2) in fp64 and fp32 with the
    assertions of test_stage_matrix and stops at its first failure; the second child starts only if the first passed."""
    for name, cfg in SC.FORCED.items():
        env = {k: v for k, v in os.environ.items() if k not in ("SWMHD_T_NT", "SWMHD_T_LY", "SWMHD_T_FOLD")}
        env.update(cfg["env"])
        out = tmp_path / f"{name}.json"
        r = subprocess.run([sys.executable, SC.__file__, name, str(out)], env=env, capture_output=True, text=True, timeout=300)
        res = json.load(open(out)) if out.exists() else None
        assert r.returncode == 0 and res and res["ok"], (name, res and res["failed"], r.stdout[-3000:], r.stderr[-3000:])
        print(name, json.dumps(res["layouts"], indent=1), json.dumps(res["worst"], sort_keys=True))
        assert len(res["layouts"]) == 2 * 2 * 2 * len(cfg["shapes"])
