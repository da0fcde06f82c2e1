#!/usr/bin/env python3
"""Timings of the BetaPlane Coriolis launch (swmhd_coriolis_rk3_*, k_coriolis): the step with and without it, and its launch alone.

    python tools/time_coriolis.py [--out profiles/coriolis] [--size 4096] [--processes 2] [--rounds 3] [--reps 10]

Every group below runs in fresh processes of its own (`--processes` of them, one after the other, alternating over the groups, as
tools/time_diffusion.py does); inside a process the variants of the group alternate over `--rounds` rounds, each round timing `--reps`
steps or launches between two HIP events after a warm-up of the same call.  The JSON keeps every round of every process; the figures
quoted are medians over all of them.

step_f64, step_f32   ShallowWaterModel.time_steps at N x N, periodic, vector invariant, fast: FPlane (the parent's step: the native
                     step driver), FPlane stepped stage by stage (time_step: what the host path alone costs), BetaPlane.  ms per step
                     and the ratios to the FPlane step.
ensemble             256 members of 64 x 64, fp64, graph-replayed (capture_graph + time_steps): FPlane, BetaPlane with per-member beta.
                     ms per step of all members.
launch_f64, _f32     the Coriolis launch alone at N x N through the ABI, wrapped reads: without acc (48 B per cell in fp64: 8 + 8
                     read of old, (8 + 8) x 2 of new) and with acc (80 B), the TB/s that byte count implies; the diffusion launch of two
                     fields with acc (the same 80 B) and the box's own copy rate (swmhd_probe_copy over as many bytes) in the same
                     rounds of the same process.
Writes time_coriolis.json into --out.  Needs a GPU."""
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
F0, BETA = 1.0, 0.2
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


def init(np, m):
    n1, n2 = m.names[:2]
    m.set(**{n1: lambda X, Y: Y * np.exp(-(X ** 2 + Y ** 2)), n2: lambda X, Y: -X * np.exp(-(X ** 2 + Y ** 2)),
             "h": lambda X, Y: 1.0 + 0.1 * np.exp(-(X ** 2 + Y ** 2)),
             "A": lambda X, Y: 0.1 * np.exp(-((X - 0.5) ** 2 + Y ** 2)) - 0.1 * np.exp(-((X + 0.5) ** 2 + Y ** 2))})
    return m


def group_step(sfx, N, rounds, reps):
    import numpy as np
    import torch
    import swmhd_amd as S
    dtype = torch.float64 if sfx == "f64" else torch.float32
    g = S.RectilinearGrid(size=(N, N), x=(-5, 5), y=(-5, 5))
    variants = {"fplane": S.FPlane(F0), "fplane_staged": S.FPlane(F0), "beta": S.BetaPlane(F0, BETA)}
    ms = {k: init(np, S.ShallowWaterModel(g, 9.81, dtype=dtype, coriolis=c)) for k, c in variants.items()}

    def steps(k, m):
        if k == "fplane_staged":
            return lambda: [m.time_step(DT) for _ in range(reps)]
        return lambda: m.time_steps(reps, DT)
    res = {k: [] for k in ms}
    for _ in range(rounds):
        for k, m in ms.items():
            res[k].append(event_ms(steps(k, m), reps))
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
    variants = {"fplane": S.FPlane(F0), "beta": S.BetaPlane(F0, list(np.linspace(0.0, 0.5, B)))}
    es = {}
    for k, c in variants.items():
        e = init(np, S.ShallowWaterEnsemble(g, B, 9.81, coriolis=c))
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
    mk = lambda: [S.Field(g, dtype=dtype) for _ in range(2)]
    old, new, acc = mk(), mk(), mk()
    for f in old + new + acc:
        f.data.normal_()
    table = torch.linspace(0.5, 1.5, 2 * N, dtype=dtype, device="cuda")
    L, P = _lib.lib(), _lib.ptr_array
    cor = getattr(L, f"swmhd_coriolis_rk3_{sfx}")
    dif = getattr(L, f"swmhd_diffusion_rk3_{sfx}")
    ft = ctypes.c_double if sfx == "f64" else ctypes.c_float
    coef = ctypes.cast((ft * 2)(1e-3, 2e-3), ctypes.c_void_p)
    stream = torch.cuda.current_stream().cuda_stream
    wrap = _lib.WRAP_X | _lib.WRAP_Y

    def coriolis(with_acc):
        def go():
            for _ in range(reps):
                rc = cor(old[0].ptr, old[1].ptr, new[0].ptr, new[1].ptr, acc[0].ptr if with_acc else None, acc[1].ptr if with_acc else None,
                         table.data_ptr(), g.Nx, g.Ny, g.Hx, g.Hy, old[0].stride_y, 1e-6, 1e-6, 0, g.Ny, wrap, stream)
                _lib.check(rc, "swmhd_coriolis_rk3")
        return go

    def diffusion():
        for _ in range(reps):
            rc = dif(P([f.ptr for f in old]), P([f.ptr for f in new]), P([f.ptr for f in acc]), coef, 2, g.Nx, g.Ny, g.Hx, g.Hy,
                     old[0].stride_y, g.dx, g.dy, 1e-6, 1e-6, 0, g.Ny, wrap, stream)
            _lib.check(rc, "swmhd_diffusion_rk3")
    cases = {"coriolis": coriolis(False), "coriolis_acc": coriolis(True), "diffusion_n2_acc": diffusion}
    cells = N * N
    nbytes = {"coriolis": 6 * esz * cells, "coriolis_acc": 10 * esz * cells, "diffusion_n2_acc": 10 * esz * cells}
    src = torch.empty(nbytes["coriolis_acc"] // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    rate = ctypes.c_float()
    res = {k: [] for k in cases}
    res["probe_copy_gbs"] = []
    for _ in range(rounds):
        for k, fn in cases.items():
            res[k].append(event_ms(fn, reps))
        _lib.check(L.swmhd_probe_copy(dst.data_ptr(), src.data_ptr(), src.numel(), reps, ctypes.byref(rate), stream), "swmhd_probe_copy")
        res["probe_copy_gbs"].append(rate.value)
    torch.cuda.synchronize()
    out = {f"{k}_ms": v for k, v in res.items() if k in cases}
    out["probe_copy_gbs"] = res["probe_copy_gbs"]
    out["bytes"] = nbytes
    return out


def worker(a):
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_coriolis.py needs a GPU")
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
        st = groups.get(f"step_{sfx}")
        if st:
            m = {k[:-3]: med(v) for k, v in st.items()}
            s[f"step_{sfx}"] = dict(ms=m, beta_over_fplane=m["beta"] / m["fplane"], beta_over_fplane_staged=m["beta"] / m["fplane_staged"])
        la = groups.get(f"launch_{sfx}")
        if la:
            copy = med(la["probe_copy_gbs"]) / 1e3
            d = dict(probe_copy_TBps=copy)
            for k, b in la["bytes"].items():
                ms = med(la[f"{k}_ms"])
                d[k] = dict(ms=ms, bytes=b, TBps=b / (ms * 1e-3) / 1e12, fraction_of_copy=b / (ms * 1e-3) / 1e12 / copy)
            d["coriolis_acc_over_diffusion_n2_acc"] = d["coriolis_acc"]["ms"] / d["diffusion_n2_acc"]["ms"]
            s[f"launch_{sfx}"] = d
    en = groups.get("ensemble")
    if en:
        m = {k[:-3]: med(v) for k, v in en.items()}
        s["ensemble_256x64x64_f64_graph"] = dict(ms=m, beta_over_fplane=m["beta"] / m["fplane"])
    return s


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/coriolis")
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
               summary=summarise(groups))
    try:
        import torch
        out["device"] = torch.cuda.get_device_name(0)
    except Exception:
        pass
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "time_coriolis.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out["summary"], indent=1))


if __name__ == "__main__":
    main()
