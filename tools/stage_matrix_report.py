"""Largest achieved error / allowed error of the stage matrix (tests/stage_cases.py: the calls of tests/test_stage_matrix_gpu.py) per
kernel family (vi, cons, packed) x precision x call form, on the current GPU.  Prints the table and writes it as JSON:

    python tools/stage_matrix_report.py [out.json]        (default: profiles/stage_matrix/achieved.json)

A ratio of 1 would be a call at its bound (include/swmhd.h: 1e-12 / 1e-4 of max(max|G|, S) per tendency, carried into the new state).

The same for the tile matrix (the calls of tests/test_tile_stage_matrix_gpu.py) per tile path (tile4, tile8, strict, wall,
wall-strict) x precision x call form, with the number of cases per path and the wall time of the whole matrix in this process:

    python tools/stage_matrix_report.py --tile [out.json] (default: profiles/stage_matrix/achieved_tile.json)

And for the ensemble matrix (the calls of tests/test_ensemble_stage_matrix_gpu.py) per ensemble path (ens4, ens8, ens-strict, par4,
par-strict) x precision x call form, over all members, with the observation the test does not assert: in how many calls of par4 and
ens8 every member happened to be bitwise the single-grid call on the member alone (the header promises that for ens4 only):

    python tools/stage_matrix_report.py --ensemble [out.json] (default: profiles/stage_matrix/achieved_ensemble.json)

And for the tracer stage matrix (the calls of tests/test_tracer_stage_matrix_gpu.py, tests/tracer_stage_cases.py) per path (fast,
wall, wall-strict) x precision x call form, with the call in which the worst ratio of every path and precision occurred:

    python tools/stage_matrix_report.py --tracers [out.json] (default: profiles/tracer_stage_matrix/achieved.json)

And for the call matrix of the Lorentz operator kernels (the calls of tests/test_operator_matrix_gpu.py, tests/operator_cases.py) per path
(march, tile, wall) x form x precision -- max|got - oracle64| / (tol max|oracle64|) over the rows written, tol = 1e-13 | 2e-5 -- with
the forced segment lengths SWMHD_OP_LY = 5 and 13 in child processes of their own (march-ly5, march-ly13):

    python tools/stage_matrix_report.py --operators [out.json] (default: profiles/operator_matrix/achieved.json)

The strict paths are compared bitwise: their ratio is 0 (every written cell equal to the oracle's) or inf."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import stage_cases as SC      # noqa: E402


def main(out_path):
    import torch
    import swmhd_amd as S
    from oracle import oracle as O
    worst, layouts, failures, ncases = {}, {}, [], 0
    for case in SC.matrix():
        Nx, Ny, rows, form, lor, dtype, flags = case
        ncases += 1
        nrows = Ny if rows is None else rows[1] - rows[0]
        prec = "f64" if dtype == SC.DTYPES[0] else "f32"
        layouts[f"{Nx} x {nrows} rows {SC.family(Nx, form, dtype, flags)}/{prec}"] = SC.check_layout(S._lib, Nx, nrows, form, dtype, flags)
        failures += [f"{SC.case_id(*case)} {m}" for m in SC.run_cases(S, O, *case, worst=worst)]
    rec = {"device": torch.cuda.get_device_name(0), "kernel_source_hash": S._lib.source_hash(), "cases": ncases,
           "calls_per_case": len(SC.calls()), "failures": failures,
           "max_error_over_bound": {k: float(f"{v:.3g}") for k, v in sorted(worst.items())}, "layouts": layouts}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps(rec["max_error_over_bound"], indent=1))
    print(f"{ncases} cases x {len(SC.calls())} calls, {len(failures)} failures -> {out_path}")
    return 1 if failures else 0


def main_tile(out_path):
    import torch
    import swmhd_amd as S
    from oracle import oracle as O
    worst, layouts, failures, ncases, refusals = {}, {}, [], {}, 0
    t0 = time.perf_counter()
    for case in SC.tile_matrix():
        path, Nx, Ny, rows, form, lor, dtype, flags, topo = case
        ncases[path] = ncases.get(path, 0) + 1
        refusals += sum(1 for v, _ in SC.calls() if v in SC.PATHS[path]["refused"])
        nrows = Ny if rows is None else rows[1] - rows[0]
        layouts[f"{Nx} x {nrows} rows {path}"] = SC.check_layout(S._lib, Nx, nrows, form, dtype, flags, path=path)
        failures += [f"{SC.tile_case_id(*case)} {m}" for m in SC.run_cases(S, O, Nx, Ny, rows, form, lor, dtype, flags, worst=worst,
                                                                          path=path, topo=topo)]
    seconds = time.perf_counter() - t0
    rec = {"device": torch.cuda.get_device_name(0), "kernel_source_hash": S._lib.source_hash(), "cases": sum(ncases.values()),
           "cases_per_path": ncases, "calls_per_case": len(SC.calls()), "refused_calls": refusals, "seconds": float(f"{seconds:.1f}"),
           "failures": failures, "max_error_over_bound": {k: float(f"{v:.3g}") for k, v in sorted(worst.items())}, "layouts": layouts}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps(rec["max_error_over_bound"], indent=1))
    print(f"{rec['cases']} cases x {len(SC.calls())} calls ({refusals} of them refusals) in {seconds:.1f} s, {len(failures)} failures -> {out_path}")
    return 1 if failures else 0


def main_ensemble(out_path):
    import torch
    import swmhd_amd as S
    from oracle import oracle as O
    worst, layouts, failures, ncases, refusals, observed, workgroups = {}, {}, [], {}, 0, {}, {}
    t0 = time.perf_counter()
    for case in SC.ens_matrix():
        path, Nx, Ny, members, form, lor, dtype, flags, dense = case
        ncases[path] = ncases.get(path, 0) + 1
        refusals += sum(1 for v, _ in SC.ens_calls() if v in SC.ENS_PATHS[path]["refused"])
        layouts[f"{Nx} x {Ny} x {members} members {path}"] = SC.check_ens_layout(S._lib, path, Nx, Ny, members, form, dtype, flags)
        workgroups.setdefault(path, set()).add(SC.ens_workgroups(path, Nx, Ny, members))
        single = {"ens4": "assert", "par4": "observe", "ens8": "observe"}.get(path)
        failures += [f"{SC.ens_case_id(*case)} {m}" for m in SC.run_ens_cases(S, O, *case, worst=worst, single=single, observed=observed)]
    seconds = time.perf_counter() - t0
    rec = {"device": torch.cuda.get_device_name(0), "kernel_source_hash": S._lib.source_hash(), "cases": sum(ncases.values()),
           "cases_per_path": ncases, "calls_per_case": len(SC.ens_calls()), "refused_calls": refusals, "seconds": float(f"{seconds:.1f}"),
           "workgroups_per_launch": {k: sorted(v) for k, v in workgroups.items()}, "failures": failures,
           "max_error_over_bound": {k: float(f"{v:.3g}") for k, v in sorted(worst.items())},
           "calls_bitwise_the_single_grid_call": {k: {"bitwise": v[0], "calls": v[1]} for k, v in sorted(observed.items())}, "layouts": layouts}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps(rec["max_error_over_bound"], indent=1))
    print(json.dumps(rec["calls_bitwise_the_single_grid_call"], indent=1))
    print(f"{rec['cases']} cases x {len(SC.ens_calls())} calls ({refusals} of them refusals) in {seconds:.1f} s, {len(failures)} failures -> {out_path}")
    return 1 if failures else 0


def main_tracers(out_path):
    import torch
    import swmhd_amd as S
    from oracle import oracle as O
    import tracer_stage_cases as TS
    worst, layouts, failures, ncases, refusals, ncalls = {}, {}, [], {}, 0, 0
    t0 = time.perf_counter()
    for case in TS.matrix():
        path, Nx, Ny, topo, form, dtype, wrap = case
        ncases[path] = ncases.get(path, 0) + 1
        for rows in TS.row_ranges(Ny):
            ncalls += len(TS.calls())
            refusals += sum(1 for v, _, _ in TS.calls() if v in TS.PATHS[path]["refused"])
            nrows = Ny if rows is None else rows[1] - rows[0]
            layouts[f"{Nx} x {nrows} rows"] = TS.check_layout(Nx, Ny, rows)
        failures += [f"{TS.case_id(*case)} {m}" for m in TS.run_cases(S, O, *case, worst=worst)]
    seconds = time.perf_counter() - t0
    # the worst ratio per path and precision, with the call it occurred in
    per_path = {}
    for key, (ratio, where) in worst.items():
        pp = key.rsplit("/", 1)[0]
        if ratio >= per_path.get(pp, (-1.0, ""))[0]:
            per_path[pp] = (ratio, where)
    rec = {"device": torch.cuda.get_device_name(0), "kernel_source_hash": S._lib.source_hash(), "cases": sum(ncases.values()),
           "cases_per_path": ncases, "calls": ncalls, "refused_calls": refusals, "seconds": float(f"{seconds:.1f}"), "failures": failures,
           "max_error_over_bound": {k: float(f"{v[0]:.3g}") for k, v in sorted(worst.items())},
           "worst_per_path_and_precision": {k: {"ratio": float(f"{v[0]:.3g}"), "call": v[1]} for k, v in sorted(per_path.items())},
           "layouts": layouts}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps(rec["max_error_over_bound"], indent=1))
    print(json.dumps(rec["worst_per_path_and_precision"], indent=1))
    print(f"{rec['cases']} cases, {ncalls} calls ({refusals} of them refusals) in {seconds:.1f} s, {len(failures)} failures -> {out_path}")
    return 1 if failures else 0


def main_operators(out_path):
    import subprocess
    import tempfile
    import torch
    import swmhd_amd as S
    from oracle import oracle as O
    import operator_cases as OC
    import test_operator_matrix_gpu as TM
    worst, failures, ncases, ncalls = {}, [], {}, 0
    t0 = time.perf_counter()
    for case in OC.matrix():
        path, form = case[:2]
        ncases[path] = ncases.get(path, 0) + 1
        ncalls += len(OC.calls(path, form))
        failures += [f"{OC.case_id(*case)} {m}" for m in TM.run_case(S, O, *case, worst=worst)]
    seconds = time.perf_counter() - t0
    for path, cfg in OC.PATHS.items():      # strict paths: bitwise, 0 or inf
        for form in cfg["forms"] if cfg["strict"] else ():
            for dtype in OC.DTYPES:
                bad = any(f.startswith(f"{path}-{form}-{OC.SFX[dtype]}-") and "bitwise" in f for f in failures)
                worst[f"{path}/{form}/{OC.SFX[dtype]}"] = float("inf") if bad else 0.0
    forced = {}
    for ly in TM.FORCED_LY:                 # one child at a time; the second only if the first passed
        env = {k: v for k, v in os.environ.items() if k != "SWMHD_OP_LY"}
        env["SWMHD_OP_LY"] = str(ly)
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, "forced.json")
            r = subprocess.run([sys.executable, TM.__file__, str(ly), out], env=env, capture_output=True, text=True, timeout=300)
            res = json.load(open(out)) if os.path.exists(out) else {"ok": False, "failed": [r.stderr[-1000:]], "worst": {}}
        forced[f"SWMHD_OP_LY={ly}"] = {"cases": res.get("cases"), "calls_per_case": len(TM.forced_calls("jacobian"))}
        worst.update({k.replace("march/", f"march-ly{ly}/"): v for k, v in res["worst"].items()})
        failures += [f"SWMHD_OP_LY={ly} {m}" for m in res["failed"]]
        if not res["ok"]:
            break
    rec = {"device": torch.cuda.get_device_name(0), "kernel_source_hash": S._lib.source_hash(), "cases": sum(ncases.values()),
           "cases_per_path": ncases, "calls": ncalls, "seconds": float(f"{seconds:.1f}"), "forced_layouts": forced, "failures": failures,
           "tolerance": {OC.SFX[t]: OC.TOL[t] for t in OC.DTYPES},
           "max_error_over_bound": {k: float(f"{v:.3g}") for k, v in sorted(worst.items())}}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps(rec["max_error_over_bound"], indent=1))
    print(f"{rec['cases']} cases, {ncalls} calls in {seconds:.1f} s, {len(failures)} failures -> {out_path}")
    return 1 if failures else 0


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] == "--operators":
        sys.exit(main_operators(args[1] if len(args) > 1 else os.path.join(ROOT, "profiles", "operator_matrix", "achieved.json")))
    if args and args[0] == "--tracers":
        sys.exit(main_tracers(args[1] if len(args) > 1 else os.path.join(ROOT, "profiles", "tracer_stage_matrix", "achieved.json")))
    if args and args[0] == "--ensemble":
        sys.exit(main_ensemble(args[1] if len(args) > 1 else os.path.join(ROOT, "profiles", "stage_matrix", "achieved_ensemble.json")))
    if args and args[0] == "--tile":
        sys.exit(main_tile(args[1] if len(args) > 1 else os.path.join(ROOT, "profiles", "stage_matrix", "achieved_tile.json")))
    sys.exit(main(args[0] if args else os.path.join(ROOT, "profiles", "stage_matrix", "achieved.json")))
