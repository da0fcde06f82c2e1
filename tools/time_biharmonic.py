#!/usr/bin/env python3
"""Timings of the ScalarBiharmonicDiffusivity closure (swmhd_biharmonic_rk3_*, k_biharmonic) next to the Laplacian closure's: the launch
alone, the step with and without it, and the graph-replayed ensemble.

    python tools/time_biharmonic.py [--out profiles/biharmonic] [--size 4096] [--processes 2] [--rounds 3] [--reps 10]

The method is tools/time_diffusion.py's (its event_ms and init are used): every group runs in fresh processes of its own
(`--processes` of them, alternating over the groups); inside a process the variants of the group alternate over `--rounds` rounds, each
round timing `--reps` steps or launches between two HIP events after a warm-up of the same call.  The JSON keeps every round of every
process; the figures quoted are medians over all of them.

launch_f64, _f32     at N x N through the ABI, wrapped reads, the biharmonic launch and, alternating with it on the same box and the same
                     parents, the Laplacian launch of the same call: (u, v) and (u, v, A), without and with acc.  Bytes per cell and
                     field in fp64: 8 x 20/16 read of old and 8 + 8 of new, 26 (42 with acc) against the Laplacian's 8 x 18/16 + 16 = 25
                     (41); the TB/s those counts imply, and the box's own copy rate in the same rounds (swmhd_probe_copy over as many
                     bytes as the 3-field launch moves).
step_f64, step_f32   ShallowWaterModel.time_steps at N x N, periodic, vector invariant, fast: no closure (the native step driver),
                     ScalarDiffusivity(nu, eta), ScalarBiharmonicDiffusivity(nu4, eta4), and the tuple of both.  ms per step and the
                     ratios to the step without a closure and to the step with ScalarDiffusivity.
ensemble             256 members of 64 x 64, fp64, graph-replayed (capture_graph + time_steps): no closure, ScalarDiffusivity and
                     ScalarBiharmonicDiffusivity with per-member nu.  ms per step of all members.
Writes time_biharmonic.json into --out.  Needs a GPU."""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_diffusion import event_ms, init, med      # noqa: E402

GROUPS = ("launch_f64", "launch_f32", "step_f64", "step_f32", "ensemble")
NU, ETA = 1e-3, 2e-3
DT = 1e-4


def hyper(N, extent, dt, share):
    """A biharmonic coefficient at `share` of RK3's limit for the grid-scale mode: dt c (8/dx²)² = 2.51 share."""
    dx = extent / N
    return 2.51 * share / (dt * (8.0 / dx ** 2) ** 2)


def group_step(sfx, N, rounds, reps):
    import numpy as np
    import torch
    import swmhd_amd as S
    dtype = torch.float64 if sfx == "f64" else torch.float32
    nu4, eta4 = hyper(N, 10.0, DT, 0.05), hyper(N, 10.0, DT, 0.1)
    lap, bih = S.ScalarDiffusivity(nu=NU, kappa=ETA), S.ScalarBiharmonicDiffusivity(nu=nu4, kappa=eta4)
    variants = {"none": None, "laplacian": lap, "biharmonic": bih, "both": (lap, bih)}
    g = S.RectilinearGrid(size=(N, N), x=(-5, 5), y=(-5, 5))
    ms = {k: init(S, np, S.ShallowWaterModel(g, 9.81, 1.0, dtype=dtype, closure=c), ()) for k, c in variants.items()}
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
    B, N, dt = 256, 64, 1e-3
    g = S.RectilinearGrid(size=(N, N), x=(-5, 5), y=(-5, 5))
    top = hyper(N, 10.0, dt, 0.1)
    variants = {"none": None, "laplacian": S.ScalarDiffusivity(nu=list(np.geomspace(1e-4, 1e-2, B))),
                "biharmonic": S.ScalarBiharmonicDiffusivity(nu=list(np.geomspace(top / 100, top, B)))}
    es = {}
    for k, c in variants.items():
        e = init(S, np, S.ShallowWaterEnsemble(g, B, 9.81, 1.0, closure=c), ())
        es[k] = e.capture_graph(dt)
    res = {k: [] for k in es}
    n = 2 * max(reps // 2, 1)
    for _ in range(rounds):
        for k, e in es.items():
            res[k].append(event_ms(lambda: e.time_steps(n, dt), n))
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
    K = 3
    mk = lambda: [S.Field(g, dtype=dtype) for _ in range(K)]
    old, new, acc = mk(), mk(), mk()
    for f in old + new + acc:
        f.data.normal_()
    L, P = _lib.lib(), _lib.ptr_array
    ft = ctypes.c_double if sfx == "f64" else ctypes.c_float
    coef = ctypes.cast((ft * K)(*[1e-3 * (k + 1) for k in range(K)]), ctypes.c_void_p)
    stream = torch.cuda.current_stream().cuda_stream

    def launch(op, n, with_acc):
        fn = getattr(L, f"swmhd_{op}_rk3_{sfx}")

        def go():
            for _ in range(reps):      # (a, w tiny: the parents stay finite over every repetition)
                rc = fn(P([f.ptr for f in old[:n]]), P([f.ptr for f in new[:n]]), P([f.ptr for f in acc[:n]]) if with_acc else None, coef, n,
                        g.Nx, g.Ny, g.Hx, g.Hy, old[0].stride_y, g.dx, g.dy, 1e-30, 1e-30, 0, g.Ny, _lib.WRAP_X | _lib.WRAP_Y, stream)
                _lib.check(rc, f"swmhd_{op}_rk3")
        return go
    cases = {f"{op}_n{n}{'_acc' if with_acc else ''}": (op, n, with_acc)
             for n in (2, 3) for with_acc in (False, True) for op in ("biharmonic", "diffusion")}
    nbytes = 3 * 3 * esz * N * N
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    rate = ctypes.c_float()
    res = {k: [] for k in cases}
    res["probe_copy_gbs"] = []
    for _ in range(rounds):
        for k, c in cases.items():
            res[k].append(event_ms(launch(*c), reps))
        _lib.check(L.swmhd_probe_copy(dst.data_ptr(), src.data_ptr(), src.numel(), reps, ctypes.byref(rate), stream), "swmhd_probe_copy")
        res["probe_copy_gbs"].append(rate.value)
    torch.cuda.synchronize()
    assert all(torch.isfinite(f.data).all().item() for f in new + acc)
    out = {f"{k}_ms": v for k, v in res.items() if k in cases}
    out["probe_copy_gbs"] = res["probe_copy_gbs"]
    # old: 16 rows of a wave segment and the rows around them, 2 a side (biharmonic) or 1 (Laplacian); new and acc: read and written
    out["bytes"] = {k: int(((20 if op == "biharmonic" else 18) / 16 + (4 if with_acc else 2)) * n * esz * N * N)
                    for k, (op, n, with_acc) in cases.items()}
    return out


def worker(a):
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_biharmonic.py needs a GPU")
    kind, _, sfx = a.worker.partition("_")
    if kind == "step":
        out = group_step(sfx, a.size, a.rounds, a.reps)
    elif kind == "launch":
        out = group_launch(sfx, a.size, a.rounds, a.reps)
    else:
        out = group_ensemble(a.rounds, a.reps)
    print("RESULT " + json.dumps(out), flush=True)


def summarise(groups):
    s = {}
    for sfx in ("f64", "f32"):
        la = groups.get(f"launch_{sfx}")
        if la:
            copy = med(la["probe_copy_gbs"]) / 1e3
            d = dict(probe_copy_TBps=copy)
            for k, b in la["bytes"].items():
                ms = med(la[f"{k}_ms"])
                d[k] = dict(ms=ms, bytes=b, TBps=b / (ms * 1e-3) / 1e12, fraction_of_copy=b / (ms * 1e-3) / 1e12 / copy)
            for k in [k for k in la["bytes"] if k.startswith("biharmonic")]:
                other = k.replace("biharmonic", "diffusion")
                d[k]["over_laplacian_launch"] = d[k]["ms"] / d[other]["ms"]
                d[k]["bytes_over_laplacian"] = d[k]["bytes"] / d[other]["bytes"]
            s[f"launch_{sfx}"] = d
        st = groups.get(f"step_{sfx}")
        if st:
            m = {k[:-3]: med(v) for k, v in st.items()}
            s[f"step_{sfx}"] = dict(ms=m, laplacian_over_none=m["laplacian"] / m["none"], biharmonic_over_none=m["biharmonic"] / m["none"],
                                    biharmonic_over_laplacian=m["biharmonic"] / m["laplacian"], both_over_none=m["both"] / m["none"])
    en = groups.get("ensemble")
    if en:
        m = {k[:-3]: med(v) for k, v in en.items()}
        s["ensemble_256x64x64_f64_graph"] = dict(ms=m, laplacian_over_none=m["laplacian"] / m["none"],
                                                 biharmonic_over_none=m["biharmonic"] / m["none"],
                                                 biharmonic_over_laplacian=m["biharmonic"] / m["laplacian"])
    return s


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/biharmonic")
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
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
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
    with open(os.path.join(a.out, "time_biharmonic.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out["summary"], indent=1))


if __name__ == "__main__":
    main()
