#!/usr/bin/env python3
"""Timings of the passive-tracer stage (swmhd_tracers_rk3_*, k_tracers_tile) and of the full step with tracers, one process,
alternating rounds.

    python tools/time_tracers.py [--out profiles/tracers] [--size 4096] [--rounds 5] [--reps 10] [--dtypes f64,f32]

For each precision, on an N x N periodic vector-invariant fast model:
stage     the tracer stage alone for K = 1, 4, 8 in the anchor form of a second RK3 stage (reads q1, q2, h once and, per tracer, c and W;
          writes cnew: (3 + 3 K) elements per cell, 24 + 24 K B in fp64), by HIP events over `reps` launches, and the implied TB/s;
          the main fused stage (second stage, anchor form, 12 elements per cell) and the box's one-shot copy rate (swmhd_probe_copy)
          in the same rounds.
step      ShallowWaterModel.time_step with K = 0, 1, 4, 8 tracers (K = 0 through the same Python-driven stages), ms per step and the
          cost relative to K = 0.
Writes time_tracers.json into --out.  Needs a GPU."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import swmhd_amd as S  # noqa: E402
from swmhd_amd import _lib  # noqa: E402

KS = (1, 4, 8)
DTYPES = {"f64": torch.float64, "f32": torch.float32}


def event_ms(fn, reps):
    fn()
    e0, e1 = _lib.TimingEvent(), _lib.TimingEvent()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    return e0.elapsed_time(e1) / reps


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), rounds=list(xs))


def model(N, dtype, K):
    g = S.RectilinearGrid(size=(N, N), x=(-5, 5), y=(-5, 5))
    m = S.ShallowWaterModel(g, 9.81, 1.0, dtype=dtype, tracers=tuple(f"c{k}" for k in range(K)))
    n1, n2 = m.names[:2]
    m.set(**{n1: lambda X, Y: Y * np.exp(-(X ** 2 + Y ** 2)), n2: lambda X, Y: -X * np.exp(-(X ** 2 + Y ** 2)),
             "h": lambda X, Y: 1.0 + 0.1 * np.exp(-(X ** 2 + Y ** 2)),
             "A": lambda X, Y: 0.1 * np.exp(-((X - 0.5) ** 2 + Y ** 2)) - 0.1 * np.exp(-((X + 0.5) ** 2 + Y ** 2))})
    m.set(**{f"c{k}": (lambda X, Y, k=k: np.tanh((1 + k) * Y)) for k in range(K)})
    return m


def time_stage(N, dtype, rounds, reps, dt=1e-4):
    m = model(N, dtype, max(KS))
    m.time_step(dt)                    # every buffer holds a sane field (W in G-, the alternate sets)
    m.synchronize()
    g, L, P = m.grid, m._L, _lib.ptr_array
    esz = 8 if dtype == torch.float64 else 4
    q = m._raw_fields
    names = m.tracer_names
    tr = getattr(L, f"swmhd_tracers_rk3_{m.sfx}")
    flags = _lib.WRAP_X | _lib.WRAP_Y | _lib.RK3_ANCHOR

    def tracer_stage(K):
        rc = tr(q[0].ptr, q[1].ptr, q[2].ptr, P([m._tr[n].ptr for n in names[:K]]), P([m._tr_alt[n].ptr for n in names[:K]]),
                P([f.ptr for f in m._tGn[:K]]), P([f.ptr for f in m._tGm[:K]]), K, g.Nx, g.Ny, g.Hx, g.Hy, q[0].stride_y, g.dx, g.dy,
                m.form_code, dt, 5.0 / 12.0, 0.0, 0, 0, g.Ny, flags, torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "swmhd_tracers_rk3")
    nbytes = 12 * esz * N * N
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    rate = ctypes.c_float()
    res = {f"tracers_K{K}_ms": [] for K in KS}
    res.update(main_stage_ms=[], probe_copy_gbs=[])
    for _ in range(rounds):
        for K in KS:
            res[f"tracers_K{K}_ms"].append(event_ms(lambda: tracer_stage(K), reps))
        res["main_stage_ms"].append(event_ms(lambda: m._stage_fused(dt, 1), reps))
        _lib.check(L.swmhd_probe_copy(dst.data_ptr(), src.data_ptr(), src.numel(), reps, ctypes.byref(rate),
                                      torch.cuda.current_stream().cuda_stream), "swmhd_probe_copy")
        res["probe_copy_gbs"].append(rate.value)
    torch.cuda.synchronize()
    out = {k: spread(v) for k, v in res.items()}
    for K in KS:
        b = (3 + 3 * K) * esz * N * N
        out[f"tracers_K{K}_bytes_per_cell"] = (3 + 3 * K) * esz
        out[f"tracers_K{K}_TBps"] = b / (out[f"tracers_K{K}_ms"]["median"] * 1e-3) / 1e12
        out[f"tracers_K{K}_ms_per_tracer"] = out[f"tracers_K{K}_ms"]["median"] / K
    out["main_stage_bytes_per_cell"] = 12 * esz
    out["main_stage_TBps"] = nbytes / (out["main_stage_ms"]["median"] * 1e-3) / 1e12
    out["probe_copy_TBps"] = out["probe_copy_gbs"]["median"] / 1e3
    del m
    torch.cuda.empty_cache()
    return out


def time_step(N, dtype, rounds, reps, dt=1e-4):
    ms = {K: model(N, dtype, K) for K in (0,) + KS}
    for m in ms.values():
        m.time_step(dt)
    torch.cuda.synchronize()
    res = {K: [] for K in ms}
    for _ in range(rounds):
        for K, m in ms.items():
            res[K].append(event_ms(lambda: m.time_step(dt), reps))
    torch.cuda.synchronize()
    out = {f"step_K{K}_ms": spread(v) for K, v in res.items()}
    base = out["step_K0_ms"]["median"]
    for K in KS:
        out[f"step_K{K}_over_K0"] = out[f"step_K{K}_ms"]["median"] / base
    for m in ms.values():
        assert all(torch.isfinite(f.data).all().item() for f in m._tr.values())
    ms.clear()
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/tracers")
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--dtypes", default="f64,f32")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_tracers.py needs a GPU")
    out = dict(device=torch.cuda.get_device_name(0), size=a.size, rounds=a.rounds, reps=a.reps, source_hash=_lib.source_hash(),
               tile=[64, 16])
    for sfx in a.dtypes.split(","):
        out[sfx] = dict(stage=time_stage(a.size, DTYPES[sfx], a.rounds, a.reps), step=time_step(a.size, DTYPES[sfx], a.rounds, a.reps))
        st, sp = out[sfx]["stage"], out[sfx]["step"]
        print(f"{sfx}: tracer stage " + ", ".join(f"K={K}: {st[f'tracers_K{K}_ms']['median']:.3f} ms ({st[f'tracers_K{K}_TBps']:.2f} TB/s)" for K in KS)
              + f"; main stage {st['main_stage_ms']['median']:.3f} ms ({st['main_stage_TBps']:.2f} TB/s); copy {st['probe_copy_TBps']:.2f} TB/s", flush=True)
        print(f"{sfx}: step " + ", ".join(f"K={K}: {sp[f'step_K{K}_ms']['median']:.3f} ms" for K in (0,) + KS)
              + "; relative to K=0: " + ", ".join(f"{sp[f'step_K{K}_over_K0']:.2f}" for K in KS), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "time_tracers.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
