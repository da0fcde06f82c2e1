#!/usr/bin/env python3
"""Timings of the static sources (swmhd_source_rk3_*, k_source): the step over a bottom beside the step without one and the step of
the parent commit, and the launch alone beside the relaxation launch of the same byte count and the box's own copy rate.

    python tools/time_source.py [--out profiles/source] [--size 4096] [--processes 2] [--rounds 3] [--reps 10] [--parent DIR]

Every group below runs in fresh processes of its own (`--processes` of them, one after the other, alternating over the groups, as
tools/time_relaxation.py does); inside a process the variants of the group alternate over `--rounds` rounds, each round timing `--reps`
steps or launches between two HIP events after a warm-up of the same call.  The JSON keeps every round of every process; the figures
quoted are medians over all of them.

step_f64, step_f32   ShallowWaterModel.time_steps at N x N, periodic, fast: no bathymetry (the native step driver), and a Gaussian hill
                     in the vector-invariant (two plain fields) and the conservative formulation (two weighted fields, h going along).
                     ms per step and the ratio to the step without.
parent_f64, _f32     the same step without bathymetry from the package under --parent (a built tree of the parent commit), in
                     processes of its own between the others; skipped without --parent.
launch_f64, _f32     the source launch alone at N x N through the ABI: two plain fields (24 B per cell and field in fp64: 8 read of S,
                     8 + 8 of new), an x-face and a y-face field (32 B: + 8 of h), the two weighted with acc (48 B), two plain with acc
                     (40 B); beside them the relaxation launch of the same bytes -- drag on two fields (24 B), two fields with a target
                     array (32 B), with a mask, a target and acc (56 B) -- the TB/s the byte counts imply, and the box's own copy rate in
                     the same rounds (swmhd_probe_copy over as many bytes as the two-field plain launch moves).
Writes time_source.json into --out.  Needs a GPU."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = ("step_f64", "step_f32", "parent_f64", "parent_f32", "launch_f64", "launch_f32")
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


def init(np, m, bump=None):
    n1, n2 = m.names[:2]
    h = (lambda X, Y: 1.0 + 0.1 * np.exp(-(X ** 2 + Y ** 2))) if bump is None else (lambda X, Y: 1.0 - bump(X, Y))
    m.set(**{n1: lambda X, Y: Y * np.exp(-(X ** 2 + Y ** 2)), n2: lambda X, Y: -X * np.exp(-(X ** 2 + Y ** 2)), "h": h,
             "A": lambda X, Y: 0.1 * np.exp(-((X - 0.5) ** 2 + Y ** 2)) - 0.1 * np.exp(-((X + 0.5) ** 2 + Y ** 2))})
    return m


def group_step(sfx, N, rounds, reps, parent):
    import numpy as np
    import torch
    import swmhd_amd as S
    dtype = torch.float64 if sfx == "f64" else torch.float32
    g = S.RectilinearGrid(size=(N, N), x=(-5, 5), y=(-5, 5))
    bump = lambda x, y: 0.3 * np.exp(-(x ** 2 + y ** 2) / 2.25)
    if parent:
        ms = {"parent_none": init(np, S.ShallowWaterModel(g, 9.81, 1.0, dtype=dtype))}
    else:
        ms = {"none": init(np, S.ShallowWaterModel(g, 9.81, 1.0, dtype=dtype)),
              "bathymetry": init(np, S.ShallowWaterModel(g, 9.81, 1.0, dtype=dtype, bathymetry=bump), bump),
              "none_conservative": init(np, S.ShallowWaterModel(g, 9.81, 1.0, dtype=dtype, formulation=S.ConservativeFormulation)),
              "bathymetry_conservative": init(np, S.ShallowWaterModel(g, 9.81, 1.0, dtype=dtype, formulation=S.ConservativeFormulation,
                                                                      bathymetry=bump), bump)}
    res = {k: [] for k in ms}
    for _ in range(rounds):
        for k, m in ms.items():
            res[k].append(event_ms(lambda: m.time_steps(reps, DT), reps))
    for m in ms.values():
        m.synchronize()
        assert all(torch.isfinite(f.data).all().item() for f in m.fields)
    return {f"{k}_ms": v for k, v in res.items()}


def group_launch(sfx, N, rounds, reps):
    import torch
    import swmhd_amd as S
    from swmhd_amd import _lib
    dtype = torch.float64 if sfx == "f64" else torch.float32
    esz = 8 if sfx == "f64" else 4
    g = S.RectilinearGrid(size=(N, N), x=(-5, 5), y=(-5, 5))
    K = 3
    mk = lambda: [S.Field(g, dtype=dtype) for _ in range(K)]
    old, new, acc, src, mask = mk(), mk(), mk(), mk(), mk()
    for f in old + new + acc + src + mask:
        f.data.normal_()
    L, P = _lib.lib(), _lib.ptr_array
    source = getattr(L, f"swmhd_source_rk3_{sfx}")
    relax = getattr(L, f"swmhd_relaxation_rk3_{sfx}")
    ft = ctypes.c_double if sfx == "f64" else ctypes.c_float
    vals = lambda v: ctypes.cast((ft * K)(*[v * (k + 1) for k in range(K)]), ctypes.c_void_p)
    rate, tval = vals(0.1), vals(0.0)
    stream = torch.cuda.current_stream().cuda_stream
    ptrs = lambda fs, n, on: P([f.ptr for f in fs[:n]]) if on else None
    wrap = _lib.WRAP_X | _lib.WRAP_Y

    def launch_source(kinds, thick, a):
        n = len(kinds)
        k = (ctypes.c_int * n)(*kinds)
        sp = P([src[j].ptr if (thick < 0 or j != thick) else None for j in range(n)])

        def go():
            for _ in range(reps):
                rc = source(ptrs(old, n, True), ptrs(new, n, True), ptrs(acc, n, a), sp, k, n, thick, g.Nx, g.Ny, g.Hx, g.Hy, old[0].stride_y,
                            1e-6, 1e-6, 0, g.Ny, wrap, stream)
                _lib.check(rc, "swmhd_source_rk3")
        return go

    def launch_relax(n, m, t, a):
        def go():
            for _ in range(reps):
                rc = relax(ptrs(old, n, True), ptrs(new, n, True), ptrs(acc, n, a), ptrs(mask, n, m), ptrs(src, n, t), rate, tval, n,
                           g.Nx, g.Ny, g.Hx, g.Hy, old[0].stride_y, 1e-6, 1e-6, 0, g.Ny, wrap, stream)
                _lib.check(rc, "swmhd_relaxation_rk3")
        return go
    # name: (launch, streams of 8 B (fp64) per cell and field, fields that move bytes)
    cases = {"plain_n2": (launch_source([0, 0], -1, False), 3, 2), "weighted_n2": (launch_source([1, 2, 0], 2, False), 4, 2),
             "plain_acc_n2": (launch_source([0, 0], -1, True), 5, 2), "weighted_acc_n2": (launch_source([1, 2, 0], 2, True), 6, 2),
             "relaxation_drag_n2": (launch_relax(2, False, False, False), 3, 2), "relaxation_target_n2": (launch_relax(2, False, True, False), 4, 2),
             "relaxation_acc_n2": (launch_relax(2, False, False, True), 5, 2), "relaxation_target_acc_n2": (launch_relax(2, False, True, True), 6, 2)}
    nbytes = 3 * 2 * esz * N * N
    a_, b_ = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda"), torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    gbs = ctypes.c_float()
    res = {k: [] for k in cases}
    res["probe_copy_gbs"] = []
    for _ in range(rounds):
        for k, (go, _, _) in cases.items():
            res[k].append(event_ms(go, reps))
        _lib.check(L.swmhd_probe_copy(b_.data_ptr(), a_.data_ptr(), a_.numel(), reps, ctypes.byref(gbs), stream), "swmhd_probe_copy")
        res["probe_copy_gbs"].append(gbs.value)
    torch.cuda.synchronize()
    out = {f"{k}_ms": v for k, v in res.items() if k in cases}
    out["probe_copy_gbs"] = res["probe_copy_gbs"]
    out["bytes"] = {k: streams * n * esz * N * N for k, (_, streams, n) in cases.items()}
    out["streams"] = {k: streams for k, (_, streams, _) in cases.items()}
    return out


def worker(a):
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_source.py needs a GPU")
    kind, _, sfx = a.worker.partition("_")
    if kind in ("step", "parent"):
        out = group_step(sfx, a.size, a.rounds, a.reps, kind == "parent")
    else:
        out = group_launch(sfx, a.size, a.rounds, a.reps)
    print("RESULT " + json.dumps(out), flush=True)


def med(xs):
    return statistics.median(xs)


def summarise(groups):
    s = {}
    for sfx in ("f64", "f32"):
        st = groups.get(f"step_{sfx}")
        if st:
            m = {k[:-3]: med(v) for k, v in st.items()}
            d = dict(ms=m, bathymetry_over_none=m["bathymetry"] / m["none"],
                     bathymetry_conservative_over_none_conservative=m["bathymetry_conservative"] / m["none_conservative"])
            pa = groups.get(f"parent_{sfx}")
            if pa:
                p = med(pa["parent_none_ms"])
                d.update(parent_none_ms=p, none_over_parent=m["none"] / p, bathymetry_over_parent=m["bathymetry"] / p)
            s[f"step_{sfx}"] = d
        la = groups.get(f"launch_{sfx}")
        if la:
            copy = med(la["probe_copy_gbs"]) / 1e3
            d = dict(probe_copy_TBps=copy)
            for k, b in la["bytes"].items():
                ms = med(la[f"{k}_ms"])
                d[k] = dict(ms=ms, bytes=b, streams=la["streams"][k], TBps=b / (ms * 1e-3) / 1e12, fraction_of_copy=b / (ms * 1e-3) / 1e12 / copy)
            for mine, theirs in (("plain_n2", "relaxation_drag_n2"), ("weighted_n2", "relaxation_target_n2"), ("plain_acc_n2", "relaxation_acc_n2"),
                                 ("weighted_acc_n2", "relaxation_target_acc_n2")):
                d[f"{mine}_over_{theirs}"] = d[mine]["ms"] / d[theirs]["ms"]
            s[f"launch_{sfx}"] = d
    return s


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/source")
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
    with open(os.path.join(a.out, "time_source.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out["summary"], indent=1))


if __name__ == "__main__":
    main()
