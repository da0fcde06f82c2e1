#!/usr/bin/env python3
"""Throughput of Bounded ensembles (swmhd_amd.BoundedShallowWaterEnsemble) against one Bounded ShallowWaterModel with graph replay.

    python tools/time_ensemble_bounded.py [--out profiles/ensemble_bounded/time_ensemble_bounded.json] [--trace]

The workload is the reference's commented channel experiment as a sweep (examples/run_swmhd.py --channel): topology (Periodic,
Bounded, Flat) on [-5, 5]^2, A = g y with GradientBoundaryCondition(g) on A north and south, one gradient g per member (spread over
-0.01 .. -0.1), h = 1 and the reference's vortex.  One process, one box; rows timed as tools/time_ensemble.py times them (graph replay,
two RK3 steps per replay, HIP events, median of three repeats).  Single-model rows: one Bounded ShallowWaterModel of the same size,
formulation and precision, graph replay, in the same process just before.  Speed-up = B x (single-model us/step) / (ensemble us/step).
--trace runs a short fixed set for `rocprofv3 --kernel-trace --stats`; summarise it with
`python tools/time_ensemble.py --summarize-trace DIR --out ...`."""
import argparse, json, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import swmhd_amd as S  # noqa: E402
from swmhd_amd import _lib, configs  # noqa: E402
from time_ensemble import FORMS, DTYPES, timed, nsteps, box  # noqa: E402


def grid(N):
    return S.RectilinearGrid(size=(N, N), x=(-5, 5), y=(-5, 5), topology=("Periodic", "Bounded", "Flat"))


def gradients(members):
    return list(np.linspace(-0.01, -0.1, members)) if members > 1 else [-0.05]


def channel_bcs(gr):
    return {"A": S.FieldBoundaryConditions(north=S.GradientBoundaryCondition(float(gr)), south=S.GradientBoundaryCondition(float(gr)))}


def setup(obj, grads):
    n1, n2 = obj.names[:2]
    A = [(lambda X, Y, gr=float(gr): gr * Y) for gr in grads]
    obj.set(**{n1: lambda X, Y: 5 * Y * np.exp(-(X ** 2 + Y ** 2)), n2: lambda X, Y: -5 * X * np.exp(-(X ** 2 + Y ** 2)),
               "h": lambda X, Y: np.ones_like(X), "A": A if hasattr(obj, "members") else A[0]})


def run_single(N, form, dt_name):
    m = S.ShallowWaterModel(grid(N), configs.G, configs.F, formulation=FORMS[form], dtype=DTYPES[dt_name],
                            boundary_conditions=channel_bcs(-0.05))
    setup(m, [-0.05])
    dt = 0.01 * 64 / N
    m.time_step(dt)
    m.capture_graph(dt)
    us, reps = timed(lambda n: m.time_steps(n, dt), 1000)
    ok = bool(torch.isfinite(m.solution["h"].data).all())
    return dict(kind="single", topology="PB", N=N, form=form, dtype=dt_name, members=1, us_per_step=us, repeats_us=reps,
                gcell_steps_per_s=N * N / us / 1e3, finite=ok)


def run_ensemble(N, B, form, dt_name):
    grads = gradients(B)
    e = S.BoundedShallowWaterEnsemble(grid(N), B, configs.G, configs.F, formulation=FORMS[form], dtype=DTYPES[dt_name],
                                      boundary_conditions=[channel_bcs(g) for g in grads])
    setup(e, grads)
    dt = 0.01 * 64 / N
    e.time_step(dt)
    e.capture_graph(dt)
    us, reps = timed(lambda n: e.time_steps(n, dt), nsteps(B * N * N))
    ok = bool(all(torch.isfinite(t).all() for t in e.fields))
    del e
    torch.cuda.empty_cache()
    return dict(kind="ensemble", topology="PB", N=N, form=form, dtype=dt_name, members=B, us_per_step=us, repeats_us=reps,
                gcell_steps_per_s=B * N * N / us / 1e3, finite=ok)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="JSON file for the results")
    ap.add_argument("--trace", action="store_true", help="short fixed set for a rocprofv3 kernel trace")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    if a.trace:
        run_single(64, "vi", "f64")
        for B in (1, 256):
            run_ensemble(64, B, "vi", "f64")
        run_ensemble(128, 256, "vi", "f64")
        return
    singles = {}
    for N in (64, 128):
        for form in ("vi", "cons"):
            for dt_name in ("f64", "f32"):
                s = singles[(N, form, dt_name)] = run_single(N, form, dt_name)
                print(f"single PB {form:4s} {dt_name} N={N:4d}: {s['us_per_step']:8.1f} us/step  {s['gcell_steps_per_s']:7.3f} Gcell-steps/s",
                      flush=True)
    rows = []
    for form in ("vi", "cons"):
        for dt_name in ("f64", "f32"):
            for N, B in [(64, 1), (64, 16), (64, 256), (64, 1024), (128, 64), (128, 256)]:
                r = run_ensemble(N, B, form, dt_name)
                r["speedup_vs_one_after_another"] = B * singles[(N, form, dt_name)]["us_per_step"] / r["us_per_step"]
                rows.append(r)
                print(f"ensemble PB {form:4s} {dt_name} N={N:4d} B={B:5d}: {r['us_per_step']:9.1f} us/step  "
                      f"{r['gcell_steps_per_s']:7.2f} Gcell-steps/s  x{r['speedup_vs_one_after_another']:6.1f} vs one after another  "
                      f"finite={r['finite']}", flush=True)
    res = dict(tool="tools/time_ensemble_bounded.py", kernel_source_hash=_lib.source_hash(), device=torch.cuda.get_device_name(0),
               box=box(), singles=list(singles.values()), rows=rows)
    r256 = [r for r in rows if r["N"] == 64 and r["members"] == 256 and r["form"] == "vi" and r["dtype"] == "f64"][0]
    r1 = [r for r in rows if r["N"] == 64 and r["members"] == 1 and r["form"] == "vi" and r["dtype"] == "f64"][0]
    base = singles[(64, "vi", "f64")]
    res["bar"] = dict(speedup_256x64_vi_f64_vs_single_64_graph=r256["speedup_vs_one_after_another"], required=10.0,
                      members1_slowdown_vs_single=r1["us_per_step"] / base["us_per_step"] - 1.0)
    print(json.dumps(res["bar"]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
