#!/usr/bin/env python3
"""Timings of the Relaxation forcing (swmhd_relaxation_rk3_*, k_relaxation): the step with and without it, and its launch alone beside
the diffusion launch of the same field count and the box's own copy rate.

    python tools/time_relaxation.py [--out profiles/relaxation] [--size 4096] [--processes 2] [--rounds 3] [--reps 10]

Every group below runs in fresh processes of its own (`--processes` of them, one after the other, alternating over the groups, as
tools/time_diffusion.py does); inside a process the variants of the group alternate over `--rounds` rounds, each round timing `--reps`
steps or launches between two HIP events after a warm-up of the same call.  The JSON keeps every round of every process; the figures
quoted are medians over all of them.

step_f64, step_f32   ShallowWaterModel.time_steps at N x N, periodic, vector invariant, fast: no forcing (the parent's step: the native
                     step driver), drag on u and v, and four fields (u, v, h, A) each with a mask and a target array.  ms per step and
                     the ratio to the step without forcing.
ensemble             256 members of 64 x 64, fp64, graph-replayed (capture_graph + time_steps): no forcing, per-member drag on u and
                     v, and drag plus h towards a shared h_eq(x, y).  ms per step of all members.
launch_f64, _f32     the relaxation launch alone at N x N through the ABI: drag on two fields without arrays (24 B per cell and field
                     in fp64: 8 read of old, 8 + 8 of new), h with a target array (32 B), four fields each with a mask and a target
                     (40 B), the same four with acc (56 B); beside each the diffusion launch of the same field count (24 B, with acc
                     40 B), the TB/s the byte counts imply, and the box's own copy rate in the same rounds (swmhd_probe_copy over as
                     many bytes as the two-field drag launch moves).
Writes time_relaxation.json into --out.  Needs a GPU."""
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
    mask = lambda x, y: np.exp(-(y / 2.0) ** 2) + 0 * x
    target = lambda x, y: 0.1 * np.cos(x) * np.sin(y)
    h_eq = lambda x, y: 1.0 + 0.05 * np.cos(x) * np.sin(y)
    four = {n: S.Relaxation(0.5, mask=mask, target=h_eq if n == "h" else target) for n in ("u", "v", "h", "A")}
    variants = {"none": None, "drag": {"u": S.Relaxation(0.1), "v": S.Relaxation(0.1)}, "four_mask_target": four}
    g = S.RectilinearGrid(size=(N, N), x=(-5, 5), y=(-5, 5))
    ms = {k: init(np, S.ShallowWaterModel(g, 9.81, 1.0, dtype=dtype, forcing=f)) for k, f in variants.items()}
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
    sweep = list(np.geomspace(1e-2, 1.0, B))
    drag = {"u": S.Relaxation(sweep), "v": S.Relaxation(sweep)}
    variants = {"none": None, "drag": drag,
                "drag_h_target": {**drag, "h": S.Relaxation(0.5, target=lambda x, y: 1.0 + 0.05 * np.cos(x) * np.sin(y))}}
    es = {}
    for k, f in variants.items():
        e = init(np, S.ShallowWaterEnsemble(g, B, 9.81, 1.0, forcing=f))
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
    K = 4
    mk = lambda: [S.Field(g, dtype=dtype) for _ in range(K)]
    old, new, acc, mask, target = mk(), mk(), mk(), mk(), mk()
    for f in old + new + acc + mask + target:
        f.data.normal_()
    L, P = _lib.lib(), _lib.ptr_array
    relax = getattr(L, f"swmhd_relaxation_rk3_{sfx}")
    diff = getattr(L, f"swmhd_diffusion_rk3_{sfx}")
    ft = ctypes.c_double if sfx == "f64" else ctypes.c_float
    vals = lambda v: ctypes.cast((ft * K)(*[v * (k + 1) for k in range(K)]), ctypes.c_void_p)
    rate, tval, coef = vals(0.1), vals(0.0), vals(1e-3)
    stream = torch.cuda.current_stream().cuda_stream
    ptrs = lambda fs, n, on: P([f.ptr for f in fs[:n]]) if on else None

    def launch_relax(n, m, t, a):
        def go():
            for _ in range(reps):
                rc = relax(ptrs(old, n, True), ptrs(new, n, True), ptrs(acc, n, a), ptrs(mask, n, m), ptrs(target, n, t), rate, tval, n,
                           g.Nx, g.Ny, g.Hx, g.Hy, old[0].stride_y, 1e-6, 1e-6, 0, g.Ny, _lib.WRAP_X | _lib.WRAP_Y, stream)
                _lib.check(rc, "swmhd_relaxation_rk3")
        return go

    def launch_diff(n, a):
        def go():
            for _ in range(reps):
                rc = diff(ptrs(old, n, True), ptrs(new, n, True), ptrs(acc, n, a), coef, n, g.Nx, g.Ny, g.Hx, g.Hy, old[0].stride_y,
                          g.dx, g.dy, 1e-6, 1e-6, 0, g.Ny, _lib.WRAP_X | _lib.WRAP_Y, stream)
                _lib.check(rc, "swmhd_diffusion_rk3")
        return go
    # name: (launch, streams of 8 B (fp64) per cell and field, fields)
    cases = {"drag_n2": (launch_relax(2, False, False, False), 3, 2), "h_target_n1": (launch_relax(1, False, True, False), 4, 1),
             "mask_target_n4": (launch_relax(4, True, True, False), 5, 4), "mask_target_acc_n4": (launch_relax(4, True, True, True), 7, 4),
             "diffusion_n1": (launch_diff(1, False), 3, 1), "diffusion_n2": (launch_diff(2, False), 3, 2),
             "diffusion_n4": (launch_diff(4, False), 3, 4), "diffusion_acc_n4": (launch_diff(4, True), 5, 4)}
    nbytes = 3 * 2 * esz * N * N
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    gbs = ctypes.c_float()
    res = {k: [] for k in cases}
    res["probe_copy_gbs"] = []
    for _ in range(rounds):
        for k, (go, _, _) in cases.items():
            res[k].append(event_ms(go, reps))
        _lib.check(L.swmhd_probe_copy(dst.data_ptr(), src.data_ptr(), src.numel(), reps, ctypes.byref(gbs), stream), "swmhd_probe_copy")
        res["probe_copy_gbs"].append(gbs.value)
    torch.cuda.synchronize()
    out = {f"{k}_ms": v for k, v in res.items() if k in cases}
    out["probe_copy_gbs"] = res["probe_copy_gbs"]
    out["bytes"] = {k: streams * n * esz * N * N for k, (_, streams, n) in cases.items()}
    out["streams"] = {k: streams for k, (_, streams, _) in cases.items()}
    return out


def worker(a):
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_relaxation.py needs a GPU")
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
            s[f"step_{sfx}"] = dict(ms=m, drag_over_none=m["drag"] / m["none"], four_mask_target_over_none=m["four_mask_target"] / m["none"])
        la = groups.get(f"launch_{sfx}")
        if la:
            copy = med(la["probe_copy_gbs"]) / 1e3
            d = dict(probe_copy_TBps=copy)
            for k, b in la["bytes"].items():
                ms = med(la[f"{k}_ms"])
                d[k] = dict(ms=ms, bytes=b, streams=la["streams"][k], TBps=b / (ms * 1e-3) / 1e12, fraction_of_copy=b / (ms * 1e-3) / 1e12 / copy)
            s[f"launch_{sfx}"] = d
    en = groups.get("ensemble")
    if en:
        m = {k[:-3]: med(v) for k, v in en.items()}
        s["ensemble_256x64x64_f64_graph"] = dict(ms=m, drag_over_none=m["drag"] / m["none"], drag_h_target_over_none=m["drag_h_target"] / m["none"])
    return s


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/relaxation")
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
    with open(os.path.join(a.out, "time_relaxation.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out["summary"], indent=1))


if __name__ == "__main__":
    main()
