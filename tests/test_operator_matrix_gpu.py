"""The call matrix of the Lorentz operator kernels: every compiled path of swmhd_lorentz_jacobian_rows_* / swmhd_lorentz_divergence_rows_*
(tests/operator_cases.py: march, tile, strict, wall, wall-strict) through ctypes on the C ABI, one column and one row below, at and above
its workgroup and at two workgroups and one more, in fp64 and fp32, with the minimal halo and a contiguous pitch and with a deeper,
unequal halo and a padded odd pitch, over all rows, the inner rows and an empty range; on the marching kernels also the twelve phases of
their LDS row rings.  The reference is pinned on the CPU by tests/test_operator_cases_cpu.py.

One test = one (path, form, precision, layout [, topology]).  Per call: it returns 0; every written value is finite; strict paths are
bitwise the oracle in the precision of the call; fast paths keep max|got - oracle64| <= tol max|oracle64| per component over the rows
written (tol = 1e-13 | 2e-5, include/swmhd.h; oracle64: the fp64 oracle on the exactly widened inputs); every other element of Fx and Fy
-- halos, pad columns, rows outside the range -- is bitwise the sentinel; A and h are bitwise unchanged, the NaN beyond the stencil reach
included; wall paths differ from the periodic result on the rows written (no non-empty range of the matrix excludes every wall-affected
cell: test_operator_cases_cpu.py).  What each shape lands on is asserted on the CPU (tests/launch_plan_check.cpp).

Achieved error / bound ratios: profiles/operator_matrix/ (tools/stage_matrix_report.py --operators)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import operator_cases as OC

pytestmark = pytest.mark.gpu
CASES = list(OC.matrix())
# SWMHD_OP_LY (read once per process): segments of 5 and of 13 rows on the 21-row sweep grid -- 5 + 5 + 5 + 5 + 1 and 13 + 8 rows
# over all rows, 5 + 4 and 9 in the sweep -- which the default chooser (8 rows on a small grid) never makes
FORCED_LY = (5, 13)


def run_case(S, O, path, form, dtype, lay, topo, calls=None, worst=None, stop_at_first=False):
    """All calls of one case (operator_cases.calls, or `calls`); the failure texts of operator_cases.check_call, each with its call."""
    import torch
    L = S._lib
    cfg = OC.PATHS[path]
    rows_fn = getattr(L.lib(), f"swmhd_lorentz_{form}_rows_{OC.SFX[dtype]}")
    dx, dy = OC.spacing(dtype)
    failures, dev = [], {}
    for Nx, Ny, rows, tag in OC.calls(path, form) if calls is None else calls:
        c = OC.case(form, dtype, Nx, Ny, lay)
        if (Nx, Ny) not in dev:
            dev = {(Nx, Ny): (torch.from_numpy(c.A).cuda(), torch.from_numpy(c.h).cuda())}
        A_d, h_d = dev[Nx, Ny]
        F_d = torch.from_numpy(c.outputs()).cuda()
        args = [A_d.data_ptr(), h_d.data_ptr(), F_d[0].data_ptr(), F_d[1].data_ptr(), Nx, Ny, c.Hx, c.Hy, c.sy, dx, dy]
        args += list(topo) if form == "divergence" else []
        rc = rows_fn(*args, rows[0], rows[1], cfg["flags"], None)
        torch.cuda.synchronize()
        where = f"{Nx} x {Ny} rows [{rows[0]}, {rows[1]}){' ' + tag if tag else ''}"
        if rc != 0:
            fails = [f"returned {rc}"]
        else:
            fails = OC.check_call(c, O, path, topo, rows, F_d.cpu().numpy(), A_d.cpu().numpy(), h_d.cpu().numpy(), worst)
        failures += [f"{where}: {m}" for m in fails]
        if failures and stop_at_first:
            break
    return failures


@pytest.mark.parametrize("path,form,dtype,lay,topo", CASES, ids=[OC.case_id(*c) for c in CASES])
def test_operator_matrix(swmhd, oracle, path, form, dtype, lay, topo):
    assert not os.environ.get("SWMHD_OP_LY"), "SWMHD_OP_LY set: the default segments are not what runs"
    failures = run_case(swmhd, oracle, path, form, dtype, lay, topo)
    assert not failures, "\n".join(failures)


def forced_calls(form):
    Nx, Ny = OC.sweep_shape(form)
    return [(Nx, Ny, (0, Ny), "forced")] + [(Nx, Ny, r, "forced sweep") for r in OC.sweep_ranges()]


def forced_main(ly, out_path):
    """Child process: the march path of both forms, precisions and layouts on the sweep grid, all rows and the twelve-j0 sweep, with
    SWMHD_OP_LY = ly set by the parent.  Writes {"ok", "failed", "cases", "worst"}; stops at the first failure."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import swmhd_amd as S
    from oracle import oracle as O
    assert os.environ.get("SWMHD_OP_LY") == str(ly), "SWMHD_OP_LY must be set in the environment of this process"
    worst, failures, ncases = {}, [], 0
    for form in OC.FORMS:
        for dtype in OC.DTYPES:
            for lay in OC.LAYOUTS:
                if failures:
                    break
                ncases += 1
                cid = OC.case_id("march", form, dtype, lay, (OC.P, OC.P))
                failures = [f"{cid} {m}" for m in run_case(S, O, "march", form, dtype, lay, (OC.P, OC.P), forced_calls(form), worst, True)]
    with open(out_path, "w") as fh:
        json.dump({"ok": not failures, "failed": failures, "cases": ncases, "worst": worst}, fh, indent=1, sort_keys=True)
    return 1 if failures else 0


def test_forced_layouts(swmhd, tmp_path):
    """Segments the default chooser never makes, through its read-once knob in fresh child processes, one at a time: SWMHD_OP_LY=5 and
    =13, both forms, precisions and layouts on (W + 1, 21) with the all-rows range and the twelve-j0 sweep, with the assertions of
    test_operator_matrix.  A child stops at its first failure; the second starts only if the first passed.  (That the knob gives these
    segments is asserted by tests/launch_plan_check.cpp in a process of its own.)"""
    for ly in FORCED_LY:
        env = {k: v for k, v in os.environ.items() if k != "SWMHD_OP_LY"}
        env["SWMHD_OP_LY"] = str(ly)
        out = tmp_path / f"ly{ly}.json"
        r = subprocess.run([sys.executable, os.path.abspath(__file__), str(ly), str(out)], env=env, capture_output=True, text=True, timeout=300)
        res = json.load(open(out)) if out.exists() else None
        assert r.returncode == 0 and res and res["ok"], (ly, res and res["failed"], r.stdout[-3000:], r.stderr[-3000:])
        print(ly, json.dumps(res["worst"], sort_keys=True))
        assert res["cases"] == 2 * 2 * 2


if __name__ == "__main__":
    sys.exit(forced_main(int(sys.argv[1]), sys.argv[2]))
