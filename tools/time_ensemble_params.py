#!/usr/bin/env python3
"""What per-member parameters cost: the per-member path (swmhd_ensemble_step_rk3_params, the PAR kernels) against the uniform path
(swmhd_ensemble_step_rk3) of the same binary, at 256 x 64^2 with graph replay.

    python tools/time_ensemble_params.py [--out profiles/ensemble_params/time_ensemble_params.json]

One process, one box, one GPU call.  For both formulations in fp64 and fp32: two ensembles from the same state, one constructed with
scalars (g, f) and stepped with a scalar dt, one with sequences of equal entries -- the same parameters in every row of the table, so
the arithmetic is the same work and only the way g, f and dt reach the kernel differs.  The two are timed alternately, A / B / A
(uniform, per-member, uniform), each a HIP-event time over the same number of graph-replayed steps, median of three repeats.  The
yardstick is the uniform path in the same call: `spread` is |A1 - A2| / mean(A1, A2), `difference` is B / mean(A1, A2) - 1."""
import argparse, json, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import swmhd_amd as S  # noqa: E402
from swmhd_amd import _lib, configs  # noqa: E402
from time_ensemble import DTYPES, FORMS, box, grid, nsteps, setup, timed  # noqa: E402

N, B, DT = 64, 256, 0.01


def make(form, dt_name, per_member):
    g, f, dt = (([configs.G] * B, [configs.F] * B, [DT] * B) if per_member else (configs.G, configs.F, DT))
    e = S.ShallowWaterEnsemble(grid(N), B, g, f, formulation=FORMS[form], dtype=DTYPES[dt_name])
    setup(e, N, B)
    e.time_step(dt)
    e.capture_graph(dt)
    assert (e.parameters is not None) == per_member
    return e, dt


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="JSON file for the results")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    n = nsteps(B * N * N)
    rows = []
    for dt_name in ("f64", "f32"):
        for form in ("vi", "cons"):
            (uni, dt_u), (par, dt_p) = make(form, dt_name, False), make(form, dt_name, True)
            a1, a1_reps = timed(lambda k: uni.time_steps(k, dt_u), n)
            b1, b1_reps = timed(lambda k: par.time_steps(k, dt_p), n)
            a2, a2_reps = timed(lambda k: uni.time_steps(k, dt_u), n)
            uni.synchronize(); par.synchronize()
            ok = bool(all(torch.isfinite(t).all() for t in uni.fields + par.fields))
            mean_a = 0.5 * (a1 + a2)
            r = dict(N=N, members=B, form=form, dtype=dt_name, steps_per_timing=n, uniform_us_per_step=[a1, a2], per_member_us_per_step=b1,
                     repeats_us=dict(uniform_first=a1_reps, per_member=b1_reps, uniform_second=a2_reps),
                     spread=abs(a1 - a2) / mean_a, difference=b1 / mean_a - 1.0, gcell_steps_per_s_uniform=B * N * N / mean_a / 1e3,
                     gcell_steps_per_s_per_member=B * N * N / b1 / 1e3, finite=ok)
            rows.append(r)
            print(f"{form:4s} {dt_name} {B} x {N}^2: uniform {a1:8.2f} / {a2:8.2f} us/step (spread {r['spread'] * 100:5.2f} %)  per-member {b1:8.2f} "
                  f"us/step ({r['difference'] * 100:+5.2f} %)  finite={ok}", flush=True)
            del uni, par
            torch.cuda.empty_cache()
    res = dict(tool="tools/time_ensemble_params.py", kernel_source_hash=_lib.source_hash(), device=torch.cuda.get_device_name(0), box=box(),
               rows=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
