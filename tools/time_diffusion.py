#!/usr/bin/env python3
"""Timings of the ScalarDiffusivity closure (swmhd_diffusion_rk3_*, k_diffusion): the step with and without it, and its launch alone.

    python tools/time_diffusion.py [--out profiles/diffusion] [--size 4096] [--processes 2] [--rounds 3] [--reps 10]

Every group below runs in fresh processes of its own (`--processes` of them, one after the other, alternating over the groups as
profiles/rk3_anchor/ alternated its two trees); inside a process the variants of the group alternate over `--rounds` rounds, each round
timing `--reps` steps or launches between two HIP events after a warm-up of the same call.  The JSON keeps every round of every process;
the figures quoted are medians over all of them.

step_f64, step_f32   ShallowWaterModel.time_steps at N x N, periodic, vector invariant, fast: no closure (the parent's step: the
                     native step driver), nu only (u, v), nu + eta (u, v, A), 4 tracers without a closure, nu + eta + kappa on 4
                     tracers.  ms per step and the ratio to the step without a closure and the same tracers.
ensemble             256 members of 64 x 64, fp64, graph-replayed (capture_graph + time_steps): no closure, nu, nu + eta with
                     per-member values.  ms per step of all members.
launch_f64, _f32     the diffusion launch alone at N x N through the ABI, wrapped reads: nfields = 1, 3, 7 without acc (24 B per cell
                     and field in fp64: 8 read of old, 8 + 8 of new) and 3 with acc (40 B), the TB/s that byte count implies, and the
                     box's own copy rate in the same rounds (swmhd_probe_copy over as many bytes as the 3-field launch moves).
Writes time_diffusion.json into --out.  Needs a GPU."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GROUPS = ("step_f64", "step_f32", "ensemble", "launch_f64", "launch_f32")
NU, ETA, KAPPA = 1e-3, 2e-3, 5e-4
DT = 1e-4


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


def init(S, np, m, tracers):
    n1, n2 = m.names[:2]
    m.set(**{n1: lambda X, Y: Y * np.exp(-(X ** 2 + Y ** 2)), n2: lambda X, Y: -X * np.exp(-(X ** 2 + Y ** 2)),
             "h": lambda X, Y: 1.0 + 0.1 * np.exp(-(X ** 2 + Y ** 2)),
             "A": lambda X, Y: 0.1 * np.exp(-((X - 0.5) ** 2 + Y ** 2)) - 0.1 * np.exp(-((X + 0.5) ** 2 + Y ** 2))})
    if tracers:
        m.set(**{n: (lambda X, Y, k=k: np.tanh((1 + k) * Y)) for k, n in enumerate(tracers)})
    return m


def group_step(sfx, N, rounds, reps):
    import numpy as np
    import torch
    import swmhd_amd as S
    dtype = torch.float64 if sfx == "f64" else torch.float32
    tr4 = tuple(f"c{k}" for k in range(4))
    variants = {"none": ((), None), "nu": ((), S.ScalarDiffusivity(nu=NU)), "nu_eta": ((), S.ScalarDiffusivity(nu=NU, kappa=ETA)),
                "tr4": (tr4, None), "nu_eta_tr4": (tr4, S.ScalarDiffusivity(nu=NU, kappa={"A": ETA, **{n: KAPPA for n in tr4}}))}
    g = S.RectilinearGrid(size=(N, N), x=(-5, 5), y=(-5, 5))
    ms = {k: init(S, np, S.ShallowWaterModel(g, 9.81, 1.0, dtype=dtype, tracers=t, closure=c), t) for k, (t, c) in variants.items()}
    res = {k: [] for k in ms}
    for _ in range(rounds):
        for k, m in ms.items():
            res[k].append(event_ms(lambda: m.time_steps(reps, DT), reps))
    for m in ms.values():
        m.synchronize()
        assert all(torch.isfinite(f.data).all().item() for f in m.fields)
    return {f"{k}_ms": v for k, v in res.items()}


def group_ensemble(rounds, reps):
    import numpy as np
    import torch
    import swmhd_amd as S
    B, N = 256, 64
    g = S.RectilinearGrid(size=(N, N), x=(-5, 5), y=(-5, 5))
    sweep = lambda lo, hi: list(np.geomspace(lo, hi, B))
    variants = {"none": None, "nu": S.ScalarDiffusivity(nu=sweep(1e-4, 1e-2)),
                "nu_eta": S.ScalarDiffusivity(nu=sweep(1e-4, 1e-2), kappa=sweep(1e-2, 1e-4))}
    es = {}
    for k, c in variants.items():
        e = init(S, np, S.ShallowWaterEnsemble(g, B, 9.81, 1.0, closure=c), ())
        es[k] = e.capture_graph(1e-3)
    res = {k: [] for k in es}
    n = 2 * max(reps // 2, 1)
    for _ in range(rounds):
        for k, e in es.items():
            res[k].append(event_ms(lambda: e.time_steps(n, 1e-3), n))
    for e in es.values():
        e.synchronize()
        assert all(torch.isfinite(t).all().item() for t in e.fields)
    return {f"{k}_ms": v for k, v in res.items()}


def group_launch(sfx, N, rounds, reps):
    import torch
    import swmhd_amd as S
    from swmhd_amd import _lib
    dtype = torch.float64 if sfx == "f64" else torch.float32
    esz = 8 if sfx == "f64" else 4
    g = S.RectilinearGrid(size=(N, N), x=(-5, 5), y=(-5, 5))
    K = 7
    mk = lambda: [S.Field(g, dtype=dtype) for _ in range(K)]
    old, new, acc = mk(), mk(), mk()
    for f in old + new + acc:
        f.data.normal_()
    L, P = _lib.lib(), _lib.ptr_array
    fn = getattr(L, f"swmhd_diffusion_rk3_{sfx}")
    ft = ctypes.c_double if sfx == "f64" else ctypes.c_float
    coef = ctypes.cast((ft * K)(*[1e-3 * (k + 1) for k in range(K)]), ctypes.c_void_p)
    stream = torch.cuda.current_stream().cuda_stream

    def launch(n, with_acc):
        def go():
            for _ in range(reps):
                rc = fn(P([f.ptr for f in old[:n]]), P([f.ptr for f in new[:n]]), P([f.ptr for f in acc[:n]]) if with_acc else None, coef, n,
                        g.Nx, g.Ny, g.Hx, g.Hy, old[0].stride_y, g.dx, g.dy, 1e-6, 1e-6, 0, g.Ny, _lib.WRAP_X | _lib.WRAP_Y, stream)
                _lib.check(rc, "swmhd_diffusion_rk3")
        return go
    cases = {"n1": (1, False), "n3": (3, False), "n7": (7, False), "n3_acc": (3, True)}
    nbytes = 3 * 3 * esz * N * N
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    rate = ctypes.c_float()
    res = {k: [] for k in cases}
    res["probe_copy_gbs"] = []
    for _ in range(rounds):
        for k, (n, with_acc) in cases.items():
            res[k].append(event_ms(launch(n, with_acc), reps))
        _lib.check(L.swmhd_probe_copy(dst.data_ptr(), src.data_ptr(), src.numel(), reps, ctypes.byref(rate), stream), "swmhd_probe_copy")
        res["probe_copy_gbs"].append(rate.value)
    torch.cuda.synchronize()
    out = {f"{k}_ms": v for k, v in res.items() if k in cases}
    out["probe_copy_gbs"] = res["probe_copy_gbs"]
    out["bytes"] = {k: (5 if with_acc else 3) * n * esz * N * N for k, (n, with_acc) in cases.items()}
    return out


def worker(a):
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_diffusion.py needs a GPU")
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


def summarise(groups, N):
    s = {}
    for sfx in ("f64", "f32"):
        st = groups.get(f"step_{sfx}")
        if st:
            m = {k[:-3]: med(v) for k, v in st.items()}
            s[f"step_{sfx}"] = dict(ms=m, nu_over_none=m["nu"] / m["none"], nu_eta_over_none=m["nu_eta"] / m["none"],
                                    nu_eta_tr4_over_tr4=m["nu_eta_tr4"] / m["tr4"])
        la = groups.get(f"launch_{sfx}")
        if la:
            copy = med(la["probe_copy_gbs"]) / 1e3
            d = dict(probe_copy_TBps=copy)
            for k, b in la["bytes"].items():
                ms = med(la[f"{k}_ms"])
                d[k] = dict(ms=ms, bytes=b, TBps=b / (ms * 1e-3) / 1e12, fraction_of_copy=b / (ms * 1e-3) / 1e12 / copy)
            s[f"launch_{sfx}"] = d
    en = groups.get("ensemble")
    if en:
        m = {k[:-3]: med(v) for k, v in en.items()}
        s["ensemble_256x64x64_f64_graph"] = dict(ms=m, nu_over_none=m["nu"] / m["none"], nu_eta_over_none=m["nu_eta"] / m["none"])
    return s


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/diffusion")
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--processes", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--groups", default=",".join(GROUPS))
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    from swmhd_amd import _lib
    groups = {}
    for p in range(a.processes):
        for grp in a.groups.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", grp, "--size", str(a.size), "--rounds", str(a.rounds),
                   "--reps", str(a.reps)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                sys.exit(f"{grp}, process {p}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            got = json.loads(line[0][7:])
            print(f"process {p} {grp}: " + ", ".join(f"{k} {med(v):.4g}" for k, v in got.items() if isinstance(v, list)), flush=True)
            have = groups.setdefault(grp, {})
            for k, v in got.items():
                if isinstance(v, list):
                    have.setdefault(k, []).extend(v)
                else:
                    have[k] = v
    out = dict(size=a.size, processes=a.processes, rounds=a.rounds, reps=a.reps, source_hash=_lib.source_hash(), groups=groups,
               summary=summarise(groups, a.size))
    try:
        import torch
        out["device"] = torch.cuda.get_device_name(0)
    except Exception:
        pass
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "time_diffusion.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out["summary"], indent=1))


if __name__ == "__main__":
    main()
