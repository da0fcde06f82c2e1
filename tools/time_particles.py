#!/usr/bin/env python3
"""Timings of the Lagrangian particles (swmhd_particles_rk3_*, k_particles): the step with particles beside the step without and the
step of the parent commit, the launch alone beside the box's own copy rate, and a graph-replayed ensemble.

    python tools/time_particles.py [--out profiles/particles] [--size 4096] [--processes 2] [--rounds 3] [--reps 10] [--parent DIR]

Every group below runs in fresh processes of its own (`--processes` of them, one after the other, alternating over the groups, as
tools/time_source.py does); inside a process the variants of the group alternate over `--rounds` rounds, each round timing `--reps`
steps or launches between two HIP events after a warm-up of the same call.  The JSON keeps every round of every process; the figures
quoted are medians over all of them.

step_f64, step_f32   ShallowWaterModel.time_steps at N x N, periodic, fast: no particles (the native step driver), and P = 2^20 and
                     P = 2^24 particles, each seeded as a row-major lattice and SCRAMBLED: the same lattice points in a random order,
                     the incoherent limit that a long stirred run tends to (stirring 4096^2 until the lattice is mixed takes an eddy
                     turnover, thousands of steps; the permutation is its end state and costs nothing).  ms per step, the ratio to the
                     step without, and the added ms per step.
alone_f64, _f32      the step without particles again, in processes that hold this one model and nothing else: what the parent's step
                     is compared with (in the step_* processes three models and up to 2^24 particles share the device).
parent_f64, _f32     the same from the package under --parent (a built tree of the parent commit), in processes of its own between
                     the others; skipped without --parent.
launch_f64, _f32     the particle launch alone on the model's state (LagrangianParticles.launch: stage 1, zeta = 0, and stage 2), for the
                     same four particle sets, with a frozen flow (dt = 0, so a set stays as seeded): ns per particle, the bytes the
                     launch asks for (8 gathers of the element size, 32 B of x, y read and written, 16 B of G- written and, at stage 2,
                     16 B of it read: 112 / 128 B in fp64) as TB/s, and that as a fraction of the box's own copy rate in the same rounds
                     (swmhd_probe_copy).
ensemble_f64, _f32   ShallowWaterEnsemble of 256 members of 64^2, graph-replayed: without particles and with P = 4096 per member.
Writes time_particles.json into --out.  Needs a GPU."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = ("step_f64", "step_f32", "alone_f64", "alone_f32", "parent_f64", "parent_f32", "launch_f64", "launch_f32", "ensemble_f64", "ensemble_f32")
DT = 1e-4
COUNTS = (20, 24)


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


def lattice(np, log2p, L=10.0):
    """2^log2p cell-centred points of [-L/2, L/2]^2 in row-major order, and the same points in a random order"""
    n = 1 << (log2p // 2)
    pts = -L / 2 + (np.arange(n) + 0.5) * (L / n)
    X, Y = np.meshgrid(pts, pts)
    x, y = X.ravel(), Y.ravel()
    perm = np.random.default_rng(log2p).permutation(x.size)
    return (x, y), (x[perm], y[perm])


def group_step(sfx, N, rounds, reps, only=None):
    import numpy as np
    import torch
    import swmhd_amd as S
    dtype = torch.float64 if sfx == "f64" else torch.float32
    g = S.RectilinearGrid(size=(N, N), x=(-5, 5), y=(-5, 5))
    if only:      # "alone" or "parent": one model without particles and nothing else in the process
        ms = {f"{only}_none": (init(np, S.ShallowWaterModel(g, 9.81, 1.0, dtype=dtype)), None)}
    else:
        ms = {"none": (init(np, S.ShallowWaterModel(g, 9.81, 1.0, dtype=dtype)), None)}
        for lp in COUNTS:
            seeded, scrambled = lattice(np, lp)
            m = init(np, S.ShallowWaterModel(g, 9.81, 1.0, dtype=dtype, particles=S.LagrangianParticles(*seeded)))
            ms[f"p{lp}_lattice"] = (m, seeded)
            ms[f"p{lp}_scrambled"] = (m, scrambled)
    res = {k: [] for k in ms}
    for _ in range(rounds):
        for k, (m, xy) in ms.items():
            if xy is not None:
                m.particles.set(x=xy[0], y=xy[1])      # (a few steps of dt = 1e-4 move a particle by far less than a cell)
            res[k].append(event_ms(lambda: m.time_steps(reps, DT), reps))
    for m, _ in ms.values():
        m.synchronize()
        assert all(torch.isfinite(f.data).all().item() for f in m.fields)
        p = getattr(m, "particles", None)      # (the parent's model has no such attribute)
        assert p is None or torch.isfinite(p.x).all().item()
    return {f"{k}_ms": v for k, v in res.items()}


def group_launch(sfx, N, rounds, reps):
    import numpy as np
    import torch
    import swmhd_amd as S
    from swmhd_amd import _lib
    dtype = torch.float64 if sfx == "f64" else torch.float32
    esz = 8 if sfx == "f64" else 4
    g = S.RectilinearGrid(size=(N, N), x=(-5, 5), y=(-5, 5))
    cases, sets = {}, {}
    for lp in COUNTS:
        seeded, scrambled = lattice(np, lp)
        m = init(np, S.ShallowWaterModel(g, 9.81, 1.0, dtype=dtype, particles=S.LagrangianParticles(*seeded)))
        m.particles._gx.zero_(); m.particles._gy.zero_()
        for name, xy in (("lattice", seeded), ("scrambled", scrambled)):
            for stage in (0, 1):
                cases[f"p{lp}_{name}_stage{stage + 1}"] = (m, stage, 1 << lp)
                sets[f"p{lp}_{name}_stage{stage + 1}"] = xy

    def go(m, stage):
        def run():
            for _ in range(reps):
                m.particles.launch(m, 0.0, stage)      # dt = 0: the set stays as seeded, the traffic is that of any dt
        return run
    L = _lib.lib()
    nbytes = (8 * esz + 64) << COUNTS[-1]
    a_, b_ = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda"), torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    gbs = ctypes.c_float()
    stream = torch.cuda.current_stream().cuda_stream
    res = {k: [] for k in cases}
    res["probe_copy_gbs"] = []
    for _ in range(rounds):
        for k, (m, stage, _) in cases.items():
            m.particles.set(x=sets[k][0], y=sets[k][1])
            res[k].append(event_ms(go(m, stage), reps))
        _lib.check(L.swmhd_probe_copy(b_.data_ptr(), a_.data_ptr(), a_.numel(), reps, ctypes.byref(gbs), stream), "swmhd_probe_copy")
        res["probe_copy_gbs"].append(gbs.value)
    torch.cuda.synchronize()
    out = {f"{k}_ms": v for k, v in res.items() if k in cases}
    out["probe_copy_gbs"] = res["probe_copy_gbs"]
    out["particles"] = {k: P for k, (_, _, P) in cases.items()}
    out["bytes_per_particle"] = {k: 8 * esz + 32 + 16 + (16 if stage else 0) for k, (_, stage, _) in cases.items()}
    return out


def group_ensemble(sfx, rounds, reps):
    import numpy as np
    import torch
    import swmhd_amd as S
    dtype = torch.float64 if sfx == "f64" else torch.float32
    g = S.RectilinearGrid(size=(64, 64), x=(-5, 5), y=(-5, 5))
    B, dt = 256, 1e-3
    (x, y), _ = lattice(np, 12)
    ens = {"none": S.ShallowWaterEnsemble(g, B, dtype=dtype), "p4096": S.ShallowWaterEnsemble(g, B, dtype=dtype, particles=S.LagrangianParticles(x, y))}
    for e in ens.values():
        init(np, e)
        e.capture_graph(dt)
    res = {k: [] for k in ens}
    for _ in range(rounds):
        for k, e in ens.items():
            res[k].append(event_ms(lambda: e.time_steps(2 * reps, dt), 2 * reps))
    for e in ens.values():
        e.synchronize()
        assert all(torch.isfinite(t).all().item() for t in e.fields)
    return {f"{k}_ms": v for k, v in res.items()}


def worker(a):
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_particles.py needs a GPU")
    kind, _, sfx = a.worker.partition("_")
    if kind in ("step", "alone", "parent"):
        out = group_step(sfx, a.size, a.rounds, a.reps, None if kind == "step" else kind)
    elif kind == "launch":
        out = group_launch(sfx, a.size, a.rounds, a.reps)
    else:
        out = group_ensemble(sfx, a.rounds, a.reps)
    print("RESULT " + json.dumps(out), flush=True)


def med(xs):
    return statistics.median(xs)


def summarise(groups):
    s = {}
    for sfx in ("f64", "f32"):
        st = groups.get(f"step_{sfx}")
        if st:
            m = {k[:-3]: med(v) for k, v in st.items()}
            d = dict(ms=m, over_none={k: v / m["none"] for k, v in m.items() if k != "none"},
                     added_ms={k: v - m["none"] for k, v in m.items() if k != "none"})
            al, pa = groups.get(f"alone_{sfx}"), groups.get(f"parent_{sfx}")
            if al:
                d.update(alone_none_ms=med(al["alone_none_ms"]))
            if al and pa:
                p = med(pa["parent_none_ms"])
                d.update(parent_none_ms=p, alone_none_over_parent=d["alone_none_ms"] / p)
            s[f"step_{sfx}"] = d
        la = groups.get(f"launch_{sfx}")
        if la:
            copy = med(la["probe_copy_gbs"]) / 1e3
            d = dict(probe_copy_TBps=copy)
            for k, P in la["particles"].items():
                ms = med(la[f"{k}_ms"])
                b = la["bytes_per_particle"][k] * P
                d[k] = dict(ms=ms, ns_per_particle=ms * 1e6 / P, bytes=b, TBps=b / (ms * 1e-3) / 1e12, fraction_of_copy=b / (ms * 1e-3) / 1e12 / copy)
            s[f"launch_{sfx}"] = d
        en = groups.get(f"ensemble_{sfx}")
        if en:
            m = {k[:-3]: med(v) for k, v in en.items()}
            s[f"ensemble_{sfx}"] = dict(ms=m, p4096_over_none=m["p4096"] / m["none"])
    return s


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/particles")
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--processes", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--groups", default=",".join(GROUPS))
    ap.add_argument("--parent", default=None, help="root of a built tree of the parent commit, for the parent_* groups")
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    sys.path.insert(0, ROOT)
    from swmhd_amd import _lib
    groups = {}
    for p in range(a.processes):
        for grp in a.groups.split(","):
            if grp.startswith("parent") and not a.parent:
                continue
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", grp, "--size", str(a.size), "--rounds", str(a.rounds),
                   "--reps", str(a.reps), "--root", a.parent if grp.startswith("parent") else ROOT]
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
    out = dict(size=a.size, processes=a.processes, rounds=a.rounds, reps=a.reps, source_hash=_lib.source_hash(), parent=bool(a.parent),
               groups=groups, summary=summarise(groups))
    try:
        import torch
        out["device"] = torch.cuda.get_device_name(0)
    except Exception:
        pass
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "time_particles.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out["summary"], indent=1))


if __name__ == "__main__":
    main()
