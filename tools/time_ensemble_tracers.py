#!/usr/bin/env python3
"""What passive tracers cost on an ensemble (ShallowWaterEnsemble(tracers=...): swmhd_ensemble_tendencies_rk3 + swmhd_ensemble_tracers_rk3
per stage, six launches per step) at the reference's sweep sizes, 256 x 64^2 and 64 x 128^2, with graph replay.

    python tools/time_ensemble_tracers.py [--out profiles/ensemble_tracers/time_ensemble_tracers.json]

One process, one box, one GPU call.  For every (size, formulation, precision): the ensemble without tracers (the native driver, three
launches per step), the ensembles with K = 1, 4 and 8 tracers, and the ensemble without tracers again -- A / B / B / B / A, each a
HIP-event time over the same number of graph-replayed steps, median of three repeats after a warm-up of the same length.  `spread` is
|A1 - A2| / mean(A1, A2): what the box does to the same work within the call.  Then single ShallowWaterModel(tracers=...) runs of one
member with the same K, graph-replayed: `vs_models_one_after_another` = members x (single us/step) / (ensemble us/step).

Unless --no-bitwise is given it also steps a fast 4-member ensemble with 3 tracers for two steps beside four fast single models from the same
data and records whether every member's tracers are bitwise the single model's (the ensemble instantiation of the tile kernel against
the single-grid one; scalar dt)."""
import argparse, json, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import swmhd_amd as S  # noqa: E402
from swmhd_amd import _lib, configs  # noqa: E402
from time_ensemble import DTYPES, FORMS, box, grid, nsteps, setup, timed  # noqa: E402

SIZES = ((64, 256), (128, 64))
KS = (1, 4, 8)
NAMES = tuple(f"c{k}" for k in range(8))


def dye(k):
    return lambda X, Y: np.tanh((1 + 0.25 * k) * Y) + 0.1 * k


def make_ensemble(N, B, form, dt_name, K):
    e = S.ShallowWaterEnsemble(grid(N), B, configs.G, configs.F, formulation=FORMS[form], dtype=DTYPES[dt_name], tracers=NAMES[:K])
    setup(e, N, B)
    if K:
        e.set(**{n: dye(k) for k, n in enumerate(NAMES[:K])})
    dt = 0.01 * 64 / N
    e.time_step(dt)
    e.capture_graph(dt)
    return e, dt


def make_model(N, form, dt_name, K, amp=0.1):
    m = S.ShallowWaterModel(grid(N), configs.G, configs.F, formulation=FORMS[form], dtype=DTYPES[dt_name], tracers=NAMES[:K])
    n1, n2 = m.names[:2]
    m.set(**{n1: lambda X, Y: 5 * Y * np.exp(-(X ** 2 + Y ** 2)), n2: lambda X, Y: -5 * X * np.exp(-(X ** 2 + Y ** 2)),
             "h": lambda X, Y: np.ones_like(X), "A": configs.two_gaussians(amp)})
    if K:
        m.set(**{n: dye(k) for k, n in enumerate(NAMES[:K])})
    return m


def finite(e):
    return bool(all(torch.isfinite(t).all() for t in list(e.fields) + list(e.tracers.values())))


def bitwise(N, form, dt_name, B=4, K=3, steps=2):
    """Members of a fast ensemble with tracers against fast single models from the same data: (members whose tracers are bitwise equal,
    members whose state is, largest tracer difference relative to max|c|)."""
    dt = 0.01 * 64 / N
    e = S.ShallowWaterEnsemble(grid(N), B, configs.G, configs.F, formulation=FORMS[form], dtype=DTYPES[dt_name], tracers=NAMES[:K])
    setup(e, N, B)
    e.set(**{n: dye(k) for k, n in enumerate(NAMES[:K])})
    amps = np.linspace(0.1, 0.5, B)
    for _ in range(steps):
        e.time_step(dt)
    e.synchronize()
    same_tr = same_st = 0
    worst = 0.0
    for m in range(B):
        one = make_model(N, form, dt_name, K, float(amps[m]))
        for _ in range(steps):
            one.time_step(dt)
        one.synchronize()
        tr = [(one.tracers[n].data, e.tracers[n][m]) for n in NAMES[:K]]
        same_tr += all(torch.equal(a, b) for a, b in tr)
        same_st += all(torch.equal(f.data, t[m]) for f, t in zip(one.fields, e.fields))
        worst = max([worst] + [float((a - b).abs().max() / a.abs().max()) for a, b in tr])
    return dict(N=N, form=form, dtype=dt_name, members=B, K=K, steps=steps, members_with_bitwise_tracers=same_tr,
                members_with_bitwise_state=same_st, largest_tracer_difference_rel=worst)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="JSON file for the results")
    ap.add_argument("--no-bitwise", action="store_true", help="skip the bitwise comparison with single models")
    ap.add_argument("--forms", default="vi,cons")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    rows, bits = [], []
    for N, B in SIZES:
        n = nsteps(B * N * N)
        for dt_name in ("f64", "f32"):
            for form in a.forms.split(","):
                plain, dt = make_ensemble(N, B, form, dt_name, 0)
                a1, a1_reps = timed(lambda k: plain.time_steps(k, dt), n)
                with_k = {}
                for K in KS:
                    e, _ = make_ensemble(N, B, form, dt_name, K)
                    us, reps = timed(lambda k: e.time_steps(k, dt), n)
                    e.synchronize()
                    with_k[K] = (us, reps, finite(e))
                    del e
                    torch.cuda.empty_cache()
                a2, a2_reps = timed(lambda k: plain.time_steps(k, dt), n)
                del plain
                torch.cuda.empty_cache()
                mean_a = 0.5 * (a1 + a2)
                for K in KS:
                    m = make_model(N, form, dt_name, K)
                    m.time_step(dt)
                    m.capture_graph(dt)
                    single, single_reps = timed(lambda k: m.time_steps(k, dt), 1000)
                    us, reps, ok = with_k[K]
                    r = dict(N=N, members=B, form=form, dtype=dt_name, K=K, steps_per_timing=n, us_per_step=us, repeats_us=reps,
                             without_tracers_us_per_step=[a1, a2], without_tracers_repeats_us=[a1_reps, a2_reps],
                             spread=abs(a1 - a2) / mean_a, ratio_to_without_tracers=us / mean_a,
                             single_model_us_per_step=single, single_model_repeats_us=single_reps,
                             vs_models_one_after_another=B * single / us, gcell_steps_per_s=B * N * N / us / 1e3, finite=ok)
                    rows.append(r)
                    print(f"{form:4s} {dt_name} {B:3d} x {N:3d}^2 K={K}: {us:9.2f} us/step  x{r['ratio_to_without_tracers']:5.2f} of no tracers "
                          f"({a1:8.2f} / {a2:8.2f} us, spread {r['spread'] * 100:5.2f} %)  single {single:7.2f} us/step -> "
                          f"x{r['vs_models_one_after_another']:6.1f} vs one after another  finite={ok}", flush=True)
                if not a.no_bitwise:
                    bits.append(bitwise(N, form, dt_name))
                    print("bitwise", json.dumps(bits[-1]), flush=True)
    res = dict(tool="tools/time_ensemble_tracers.py", kernel_source_hash=_lib.source_hash(), device=torch.cuda.get_device_name(0), box=box(),
               rows=rows, bitwise=bits)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
