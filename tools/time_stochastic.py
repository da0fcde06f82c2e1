#!/usr/bin/env python3
"""Timings of the StochasticForcing (swmhd_stochastic_rk3_*, k_stochastic; swmhd_stochastic_coefficients_*): its launch alone beside
the two floors measured on the same box in the same run, and the step with it beside the step without forcing and with a drag.

    python tools/time_stochastic.py [--out profiles/stochastic] [--size 4096] [--rounds 3] [--reps 10] [--groups ...]

Every group runs in a fresh process of its own; inside it the variants alternate over `--rounds` rounds, each round timing `--reps`
steps or launches between two HIP events after a warm-up of the same call.  The JSON keeps every round; the figures quoted are medians.

launch_f64, _f32     the correction launch alone at N x N through the ABI, two fields (the vortical pair), random tables, M = 24, 94,
                     220 modes, without and with acc; beside it
                       the FMA floor: 2 M FMA per cell and field = 2 M N² fields / 64 wave-instructions over all SIMDs (4 per compute
                       unit) at the nanoseconds per fp64 wave-instruction swmhd_probe_fp64_issue reports in the same rounds (for
                       fp32 the same price: a lane-wide fp32 FMA issues no slower);
                       the copy floor: 16 B (fp64; 8 B fp32) per cell and field for new, twice that with acc, at the rate
                       swmhd_probe_copy reports in the same rounds;
                     and the fraction of the LARGER floor the launch reaches (floor / time).
step_f64, step_f32   ShallowWaterModel.time_steps at N x N on the 2π square, vector invariant, fast: no forcing (the parent's step: the
                     native step driver), drag on u and v, and the vortical pair at k_f = 8, 32, 64 with dk = 1 (M = 24, 94, 220 at
                     4096²).  ms per step and the ratios to the step without forcing and to the step with drag.
ensemble             256 members of 64 x 64, fp64, graph-replayed: no forcing, drag, and the pair at k_f = 8 (M = 24).
Writes time_stochastic.json into --out.  Needs a GPU."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GROUPS = ("launch_f64", "launch_f32", "step_f64", "step_f32", "ensemble")
DT = 1e-4
MODES = (24, 94, 220)


def event_ms(fn, reps):
    import torch
    from swmhd_amd import _lib
    fn()
    torch.cuda.synchronize()
    e0, e1 = _lib.TimingEvent(), _lib.TimingEvent()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def init(np, m):
    n1, n2 = m.names[:2]
    m.set(**{n1: lambda X, Y: 0.1 * np.sin(Y), n2: lambda X, Y: -0.1 * np.sin(X), "h": lambda X, Y: 1.0 + 0.05 * np.cos(X) * np.cos(Y),
             "A": lambda X, Y: 0.1 * np.sin(X) * np.sin(Y)})
    return m


def group_launch(sfx, N, rounds, reps):
    import numpy as np
    import torch
    import swmhd_amd as S
    from swmhd_amd import _lib
    dtype = torch.float64 if sfx == "f64" else torch.float32
    esz = 8 if sfx == "f64" else 4
    g = S.RectilinearGrid(size=(N, N), x=(0, 2 * np.pi), y=(0, 2 * np.pi))
    K = 2
    mk = lambda: [S.Field(g, dtype=dtype) for _ in range(K)]
    old, new, acc = mk(), mk(), mk()
    for f in new + acc:
        f.data.normal_()
    L, P = _lib.lib(), _lib.ptr_array
    fn = getattr(L, f"swmhd_stochastic_rk3_{sfx}")
    stream = torch.cuda.current_stream().cuda_stream
    Px = g.parent_shape[1]
    cases, keep = {}, []
    for M in MODES:
        xt = [torch.rand((2 * M, Px), dtype=dtype, device="cuda") * 2 - 1 for _ in range(K)]
        yt = [torch.rand((2 * M, N), dtype=dtype, device="cuda") * 2 - 1 for _ in range(K)]
        cf = [torch.randn(2 * M, dtype=dtype, device="cuda") * 1e-3 for _ in range(K)]
        keep += xt + yt + cf
        mid = (P([c.data_ptr() for c in cf]), P([x.data_ptr() + g.Hx * esz for x in xt]), P([y.data_ptr() for y in yt]),
               (ctypes.c_int * K)(*[M] * K), K, Px, N)
        for with_acc in (False, True):
            def go(mid=mid, with_acc=with_acc):
                for _ in range(reps):
                    rc = fn(P([f.ptr for f in old]), P([f.ptr for f in new]), P([f.ptr for f in acc]) if with_acc else None, *mid,
                            g.Nx, g.Ny, g.Hx, g.Hy, old[0].stride_y, 1e-6, 1e-6, 0, g.Ny, _lib.WRAP_X | _lib.WRAP_Y, stream)
                    _lib.check(rc, "swmhd_stochastic_rk3")
            cases[f"M{M}" + ("_acc" if with_acc else "")] = (go, M, with_acc)
    nbytes = 2 * K * esz * N * N
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    scratch = torch.zeros(8, dtype=torch.float64, device="cuda")
    gbs, ns = ctypes.c_float(), ctypes.c_float()
    res = {k: [] for k in cases}
    res["probe_copy_gbs"], res["probe_fp64_ns"] = [], []
    for _ in range(rounds):
        for k, (go, _, _) in cases.items():
            res[k].append(event_ms(go, reps))
        _lib.check(L.swmhd_probe_copy(dst.data_ptr(), src.data_ptr(), src.numel(), reps, ctypes.byref(gbs), stream), "swmhd_probe_copy")
        _lib.check(L.swmhd_probe_fp64_issue(scratch.data_ptr(), ctypes.byref(ns), stream), "swmhd_probe_fp64_issue")
        res["probe_copy_gbs"].append(gbs.value)
        res["probe_fp64_ns"].append(ns.value)
    torch.cuda.synchronize()
    assert all(torch.isfinite(f.data).all().item() for f in new + acc)
    out = {f"{k}_ms": v for k, v in res.items() if k in cases}
    out["probe_copy_gbs"], out["probe_fp64_ns"] = res["probe_copy_gbs"], res["probe_fp64_ns"]
    out["simds"] = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    out["wave_instructions"] = {k: 2 * M * K * N * N // 64 for k, (_, M, _) in cases.items()}
    out["bytes"] = {k: (4 if a else 2) * K * esz * N * N for k, (_, _, a) in cases.items()}
    return out


def group_step(sfx, N, rounds, reps):
    import numpy as np
    import torch
    import swmhd_amd as S
    dtype = torch.float64 if sfx == "f64" else torch.float32
    g = S.RectilinearGrid(size=(N, N), x=(0, 2 * np.pi), y=(0, 2 * np.pi))
    variants = {"none": None, "drag": {"u": S.Relaxation(0.1), "v": S.Relaxation(0.1)}}
    modes = {}
    for kf in (8.0, 32.0, 64.0):
        if kf + 0.5 >= N / 2:
            continue
        s = S.StochasticForcing(1e-3, kf, 1.0, seed=1)
        variants[f"stir_kf{int(kf)}"] = {"u": s, "v": s}
        modes[f"stir_kf{int(kf)}"] = len(S.forcing_modes(g, kf, 1.0))
    ms = {k: init(np, S.ShallowWaterModel(g, 9.81, 1.0, dtype=dtype, forcing=f)) for k, f in variants.items()}
    res = {k: [] for k in ms}
    for _ in range(rounds):
        for k, m in ms.items():
            res[k].append(event_ms(lambda: m.time_steps(reps, DT), reps))
    for m in ms.values():
        m.synchronize()
        assert all(torch.isfinite(f.data).all().item() for f in m.fields)
    out = {f"{k}_ms": v for k, v in res.items()}
    out["modes"] = modes
    return out


def group_ensemble(rounds, reps):
    import numpy as np
    import torch
    import swmhd_amd as S
    B, N = 256, 64
    g = S.RectilinearGrid(size=(N, N), x=(0, 2 * np.pi), y=(0, 2 * np.pi))
    s = S.StochasticForcing(list(np.geomspace(1e-4, 1e-2, B)), 8.0, 1.0, seed=1)
    variants = {"none": None, "drag": {"u": S.Relaxation(0.1), "v": S.Relaxation(0.1)}, "stir_kf8": {"u": s, "v": s}}
    es = {k: init(np, S.ShallowWaterEnsemble(g, B, 9.81, 1.0, forcing=f)).capture_graph(1e-3) for k, f in variants.items()}
    res = {k: [] for k in es}
    n = 2 * max(reps // 2, 1)
    for _ in range(rounds):
        for k, e in es.items():
            res[k].append(event_ms(lambda: e.time_steps(n, 1e-3), n))
    for e in es.values():
        e.synchronize()
        assert all(torch.isfinite(t).all().item() for t in e.fields)
    out = {f"{k}_ms": v for k, v in res.items()}
    out["modes"] = {"stir_kf8": len(S.forcing_modes(g, 8.0, 1.0))}
    return out


def worker(a):
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_stochastic.py needs a GPU")
    kind, _, sfx = a.worker.partition("_")
    if kind == "step":
        out = group_step(sfx, a.size, a.rounds, a.reps)
    elif kind == "launch":
        out = group_launch(sfx, a.size, a.rounds, a.reps)
    else:
        out = group_ensemble(a.rounds, a.reps)
    print("RESULT " + json.dumps(out), flush=True)


def med(xs):
    return statistics.median(xs)


def summarise(groups):
    s = {}
    for sfx in ("f64", "f32"):
        la = groups.get(f"launch_{sfx}")
        if la:
            copy, ns = med(la["probe_copy_gbs"]) / 1e3, med(la["probe_fp64_ns"])
            d = dict(probe_copy_TBps=copy, probe_fp64_ns_per_wave_instruction=ns, simds=la["simds"])
            for k, b in la["bytes"].items():
                ms = med(la[f"{k}_ms"])
                fma = la["wave_instructions"][k] / la["simds"] * ns * 1e-6
                cp = b / (copy * 1e12) * 1e3
                d[k] = dict(ms=ms, fma_floor_ms=fma, copy_floor_ms=cp, larger_floor="fma" if fma >= cp else "copy",
                            fraction_of_larger_floor=max(fma, cp) / ms)
            s[f"launch_{sfx}"] = d
        st = groups.get(f"step_{sfx}")
        if st:
            m = {k[:-3]: med(v) for k, v in st.items() if k.endswith("_ms")}
            s[f"step_{sfx}"] = dict(ms=m, modes=st["modes"], over_none={k: v / m["none"] for k, v in m.items()},
                                    over_drag={k: v / m["drag"] for k, v in m.items()})
    en = groups.get("ensemble")
    if en:
        m = {k[:-3]: med(v) for k, v in en.items() if k.endswith("_ms")}
        s["ensemble_256x64x64_f64_graph"] = dict(ms=m, modes=en["modes"], over_none={k: v / m["none"] for k, v in m.items()},
                                                 over_drag={k: v / m["drag"] for k, v in m.items()})
    return s


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/stochastic")
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--groups", default=",".join(GROUPS))
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    from swmhd_amd import _lib
    groups = {}
    for grp in a.groups.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", grp, "--size", str(a.size), "--rounds", str(a.rounds), "--reps", str(a.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.exit(f"{grp}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        groups[grp] = json.loads(line[0][7:])
        print(f"{grp}: " + ", ".join(f"{k} {med(v):.4g}" for k, v in groups[grp].items() if isinstance(v, list)), flush=True)
    out = dict(size=a.size, rounds=a.rounds, reps=a.reps, source_hash=_lib.source_hash(), groups=groups, summary=summarise(groups))
    try:
        import torch
        out["device"] = torch.cuda.get_device_name(0)
    except Exception:
        pass
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "time_stochastic.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out["summary"], indent=1))


if __name__ == "__main__":
    main()
