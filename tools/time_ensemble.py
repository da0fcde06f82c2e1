#!/usr/bin/env python3
"""Throughput of ensembles (swmhd_amd.ShallowWaterEnsemble) on the reference's grid sizes against one ShallowWaterModel with graph replay.

    python tools/time_ensemble.py [--out profiles/ensemble/time_ensemble.json] [--variants] [--trace]

One process, one box.  Every row: a ShallowWaterEnsemble of B members of N^2 (graph replay, two RK3 steps per replay), timed with HIP
events over a fixed number of steps, median of three repeats; the single-model rows are ShallowWaterModels of one member, graph replay,
timed the same way in the same process.  Speed-up = B x (single-model us/step of that N, formulation and precision) / (ensemble us/step):
what the ensemble gains over running its members one after another.  --variants repeats a subset in child processes with the launch
knobs of the ensemble stage (SWMHD_ENS_MAP = 2: member in blockIdx.y instead of folded into blockIdx.x; SWMHD_ENS_RY = 2: 64 x 8
tiles instead of 64 x 4), each child timing the default launch beside it.  --trace runs a short fixed set for
`rocprofv3 --kernel-trace --stats` (kernel times come from that separate run, not from this tool)."""
import argparse, json, os, statistics, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import swmhd_amd as S  # noqa: E402
from swmhd_amd import _lib, configs  # noqa: E402

FORMS = {"vi": "VectorInvariant", "cons": "Conservative"}
DTYPES = {"f64": torch.float64, "f32": torch.float32}


def setup(obj, N, members):
    """The reference's vortex with two Gaussians of A; the amplitude of A spread over the members (its own sweep)."""
    n1, n2 = obj.names[:2]
    u0 = lambda X, Y: 5 * Y * np.exp(-(X ** 2 + Y ** 2))
    v0 = lambda X, Y: -5 * X * np.exp(-(X ** 2 + Y ** 2))
    amps = np.linspace(0.1, 0.5, members) if members > 1 else [0.1]
    A = [configs.two_gaussians(float(a)) for a in amps]
    obj.set(**{n1: u0, n2: v0, "h": lambda X, Y: np.ones_like(X), "A": A})


def timed(step, n, reps=3):
    """us per step: median over `reps` of HIP-event time of n steps (graph replays), after a warm-up of the same length."""
    step(n)
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step(n)
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / n)
    return statistics.median(us), us


def nsteps(cells):
    n = int(1.3e9 / cells)
    return max(20, min(1000, n - n % 2))


def grid(N):
    return S.RectilinearGrid(size=(N, N), x=(-5, 5), y=(-5, 5))


def run_single(N, form, dt_name):
    m = S.ShallowWaterModel(grid(N), configs.G, configs.F, formulation=FORMS[form], dtype=DTYPES[dt_name])
    n1, n2 = m.names[:2]
    m.set(**{n1: lambda X, Y: 5 * Y * np.exp(-(X ** 2 + Y ** 2)), n2: lambda X, Y: -5 * X * np.exp(-(X ** 2 + Y ** 2)),
             "h": lambda X, Y: np.ones_like(X), "A": configs.two_gaussians(0.1)})
    dt = 0.01 * 64 / N
    m.time_step(dt)
    m.capture_graph(dt)
    us, reps = timed(lambda n: m.time_steps(n, dt), 1000)
    ok = bool(torch.isfinite(m.solution["h"].data).all())
    return dict(kind="single", N=N, form=form, dtype=dt_name, members=1, us_per_step=us, repeats_us=reps,
                gcell_steps_per_s=N * N / us / 1e3, finite=ok)


def run_ensemble(N, B, form, dt_name):
    e = S.ShallowWaterEnsemble(grid(N), B, configs.G, configs.F, formulation=FORMS[form], dtype=DTYPES[dt_name])
    setup(e, N, B)
    dt = 0.01 * 64 / N
    e.time_step(dt)
    e.capture_graph(dt)
    us, reps = timed(lambda n: e.time_steps(n, dt), nsteps(B * N * N))
    ok = bool(all(torch.isfinite(t).all() for t in e.fields))
    del e
    torch.cuda.empty_cache()
    return dict(kind="ensemble", N=N, form=form, dtype=dt_name, members=B, us_per_step=us, repeats_us=reps,
                gcell_steps_per_s=B * N * N / us / 1e3, finite=ok)


def table(configs_, singles):
    rows = []
    for N, B, form, dt_name in configs_:
        r = run_ensemble(N, B, form, dt_name)
        s = singles[(N, form, dt_name)]
        r["speedup_vs_one_after_another"] = B * s["us_per_step"] / r["us_per_step"]
        r["gcell_ratio_vs_single_64_graph"] = r["gcell_steps_per_s"] / singles[(64, "vi", "f64")]["gcell_steps_per_s"]
        rows.append(r)
        print(f"{form:4s} {dt_name} N={N:4d} B={B:5d}: {r['us_per_step']:9.1f} us/step  {r['gcell_steps_per_s']:7.2f} Gcell-steps/s  "
              f"x{r['speedup_vs_one_after_another']:6.1f} vs one after another  finite={r['finite']}", flush=True)
    return rows


def box():
    try:
        from bench import box_probe
        return box_probe(torch, _lib)
    except Exception as ex:      # (the probe is a record of the box, not part of the measurement)
        return {"error": repr(ex)}


def summarize_trace(raw, out):
    """Per (kernel, workgroups) of a `rocprofv3 --kernel-trace --stats -f csv` run of --trace: dispatches and their duration."""
    import csv, glob, re
    files = glob.glob(os.path.join(raw, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit(f"no *kernel_trace.csv under {raw}")
    groups = {}
    for fn in files:
        for r in csv.DictReader(open(fn)):
            name = r["Kernel_Name"]
            m = re.search(r"(k_\w+)<([^()]*)>", name)
            short = f"{m.group(1)}<{m.group(2)}>" if m else name[:80]
            wg = 1
            for d in "XYZ":
                wg *= max(1, int(r[f"Grid_Size_{d}"]) // max(1, int(r[f"Workgroup_Size_{d}"])))
            groups.setdefault((short, wg), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    rows = [dict(kernel=k, workgroups=wg, dispatches=len(v), median_us=statistics.median(v), mean_us=statistics.mean(v), min_us=min(v))
            for (k, wg), v in sorted(groups.items(), key=lambda kv: (kv[0][0], kv[0][1]))]
    res = dict(tool="tools/time_ensemble.py --trace under rocprofv3 --kernel-trace --stats -f csv", kernel_source_hash=_lib.source_hash(),
               rows=rows)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    for r in rows:
        print(f"{r['kernel'][:70]:70s} wg={r['workgroups']:7d} n={r['dispatches']:6d} median {r['median_us']:8.1f} us")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--summarize-trace", metavar="DIR", default=None, help="summarise the kernel trace of a --trace run under DIR into --out")
    ap.add_argument("--out", default=None, help="JSON file for the results")
    ap.add_argument("--variants", action="store_true", help="also time the member-mapping and tile-height alternatives (child processes)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--trace", action="store_true", help="short fixed set for a rocprofv3 kernel trace")
    a = ap.parse_args()
    if a.summarize_trace:
        return summarize_trace(a.summarize_trace, a.out)
    torch.cuda.set_device(0)
    if a.trace:
        run_single(64, "vi", "f64")
        for B in (1, 256, 1024):
            run_ensemble(64, B, "vi", "f64")
        run_ensemble(128, 256, "vi", "f64")
        return
    singles = {}
    want = [(N, f, d) for N in (64, 128) for f in ("vi", "cons") for d in ("f64",)] + [(64, "vi", "f32")]
    if a.child:
        want = [(64, "vi", "f64"), (128, "vi", "f64")]
    for key in want:
        singles[key] = run_single(*key)
        s = singles[key]
        print(f"single {key}: {s['us_per_step']:8.1f} us/step  {s['gcell_steps_per_s']:7.3f} Gcell-steps/s", flush=True)
    if a.child:
        rows = table([(N, B, "vi", "f64") for N in (64, 128) for B in (256, 1024)], singles)
        print("CHILD_JSON " + json.dumps(rows))
        return
    cfg = [(N, B, f, "f64") for f in ("vi", "cons") for N in (64, 128) for B in (1, 16, 64, 256, 1024)] + [(64, 256, "vi", "f32")]
    rows = table(cfg, singles)
    b = box()
    res = dict(tool="tools/time_ensemble.py", kernel_source_hash=_lib.source_hash(), device=torch.cuda.get_device_name(0), box=b,
               singles=list(singles.values()), rows=rows)
    base = singles[(64, "vi", "f64")]
    r256 = [r for r in rows if r["N"] == 64 and r["members"] == 256 and r["form"] == "vi" and r["dtype"] == "f64"][0]
    r1 = [r for r in rows if r["N"] == 64 and r["members"] == 1 and r["form"] == "vi" and r["dtype"] == "f64"][0]
    res["bar"] = dict(ratio_256x64_vi_f64_vs_single_64_graph=r256["gcell_steps_per_s"] / base["gcell_steps_per_s"], required=10.0,
                      members1_slowdown_vs_single=r1["us_per_step"] / base["us_per_step"] - 1.0, members1_allowed=0.10)
    print(json.dumps(res["bar"]))
    if a.variants:
        res["variants"] = {}
        for name, env in (("default", {}), ("member_in_blockIdx_y", {"SWMHD_ENS_MAP": "2"}), ("tile_64x8_RY2", {"SWMHD_ENS_RY": "2"}),
                          ("blockIdx_y_and_RY2", {"SWMHD_ENS_MAP": "2", "SWMHD_ENS_RY": "2"})):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env={**os.environ, **env}, capture_output=True,
                               text=True, timeout=900)
            line = [l for l in r.stdout.splitlines() if l.startswith("CHILD_JSON ")]
            if r.returncode != 0 or not line:
                print(f"variant {name} failed: rc {r.returncode}\n{r.stderr[-2000:]}", file=sys.stderr)
                sys.exit(1)
            res["variants"][name] = dict(env=env, rows=json.loads(line[0][len("CHILD_JSON "):]))
            print(f"variant {name}: " + ", ".join(f"N={x['N']} B={x['members']} {x['us_per_step']:.1f} us" for x in res["variants"][name]["rows"]),
                  flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
