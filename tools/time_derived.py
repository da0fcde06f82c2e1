#!/usr/bin/env python3
"""Timings of the derived frames (swmhd_derived_fields_*, ShallowWaterModel.derived_fields), one process, alternating rounds.

    python tools/time_derived.py [--out profiles/derived_fields] [--rounds 5] [--only single,ensemble]

single    4096^2 vector-invariant fp64, periodic, float32 frames.
ensemble  256 x 64^2 vector-invariant fp64, periodic, float32 frames (all members in one launch).
For each: derived_fields of every single field and of all four; in the same rounds output_fields of (u, v, A, s) -- the same access
shape with fewer rows in flight -- and swmhd_probe_copy (the one-shot copy of as many bytes as the all-four call moves).
Times are CALL times: HIP events around as many back-to-back calls of the Python method as fill a window of about 40 ms (counted from a
short trial), so a call shorter than its host enqueue is timed at the host's pace; the host time of the enqueue loop per call is
recorded beside every figure (`*_host_enqueue_ms`) to tell the two apart.  The frame buffers are allocated once, outside the timed
calls.
Bytes: what each path must move at least, from the shapes: every fp64 parent a mask touches is read once (the rows y - 1 and y + 1 a
thread reads are its neighbours' own rows) and every float32 field is written once.  Vector-invariant:
    vorticity            reads u, v       16 B + 4 B written per cell
    divergence           reads u, v       16 B + 4 B
    current              reads A           8 B + 4 B
    potential_vorticity  reads u, v, h    24 B + 4 B
    all four             reads u, v, h, A 32 B + 16 B
    output_fields(u, v, A, s)  reads u, v, A   24 B + 16 B
(the conservative form reads h for every velocity as well).  Rates are those bytes over the median call time, and are reported as a
fraction of the copy rate and of output_fields' rate of the same rounds.  Writes time_derived.json into --out."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import swmhd_amd as S  # noqa: E402
from swmhd_amd import _lib  # noqa: E402

ALL = tuple(_lib.DRV_BITS)
FRAME = ("u", "v", "A", "s")
# (parents read, bytes read per cell, bytes written per cell): vector-invariant fp64 parents, float32 frames
TRAFFIC = {"vorticity": ("u v", 16, 4), "divergence": ("u v", 16, 4), "current": ("A", 8, 4), "potential_vorticity": ("u v h", 24, 4),
           "all_four": ("u v h A", 32, 16), "output_fields_uvAs": ("u v A", 24, 16)}
WINDOW_MS = 40.0    # every timed window lasts about this long: a window of a millisecond measures the clock and the scheduler


def event_ms(fn, reps):
    """(device ms per call between two events around `reps` calls, host ms per call the enqueue loop took)"""
    fn()
    torch.cuda.synchronize()
    e0, e1 = _lib.TimingEvent(), _lib.TimingEvent()
    e0.record()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    host = time.perf_counter() - t0
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, host * 1e3 / reps


def calls_per_window(fn):
    """how many calls fill WINDOW_MS, from a short trial (which also warms the shape up)"""
    return max(5, int(WINDOW_MS / event_ms(fn, 5)[0]) + 1)


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), rounds=list(xs))


def vortex(m, amp=0.1):
    u0 = lambda X, Y: Y * np.exp(-(X ** 2 + Y ** 2))
    v0 = lambda X, Y: -X * np.exp(-(X ** 2 + Y ** 2))
    gauss = lambda a: (lambda X, Y: a * np.exp(-((X - 0.5) ** 2 + Y ** 2)) - a * np.exp(-((X + 0.5) ** 2 + Y ** 2)))
    members = getattr(m, "members", None)
    A0 = gauss(amp) if members is None else [gauss(amp * (1 + k / members)) for k in range(members)]
    n1, n2 = m.names[:2]
    m.set(**{n1: u0, n2: v0, "h": lambda X, Y: 1.0 + 0.05 * np.exp(-(X ** 2 + Y ** 2)), "A": A0})
    return m


def measure(m, rounds):
    g, B = m.grid, getattr(m, "members", None) or 1
    lead = (B,) if getattr(m, "members", None) is not None else ()
    cells = B * g.Nx * g.Ny
    buf = {n: torch.empty(lead + (k, g.Ny, g.Nx), dtype=torch.float32, device="cuda") for n, k in (("one", 1), ("four", 4), ("frame", 4))}
    paths = {n: (lambda n=n: m.derived_fields((n,), out=buf["one"])) for n in ALL}
    paths["all_four"] = lambda: m.derived_fields(ALL, out=buf["four"])
    paths["output_fields_uvAs"] = lambda: m.output_fields(FRAME, out=buf["frame"])
    # the single-field calls are bitwise the fields of the all-four call
    m.derived_fields(ALL, out=buf["four"])
    same = all(bool(torch.equal(m.derived_fields((n,), out=buf["one"]).select(-3, 0), buf["four"].select(-3, k))) for k, n in enumerate(ALL))
    copy_bytes = sum(TRAFFIC["all_four"][1:]) * cells
    src = torch.empty(copy_bytes // 2 // 16 * 16, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    rate = ctypes.c_float()
    reps = {k: calls_per_window(fn) for k, fn in paths.items()}
    ms = {k: [] for k in paths}
    host = {k: [] for k in paths}
    copy = []
    for _ in range(rounds):
        for k, fn in paths.items():
            dev_ms, host_ms = event_ms(fn, reps[k])
            ms[k].append(dev_ms)
            host[k].append(host_ms)
        _lib.check(_lib.lib().swmhd_probe_copy(dst.data_ptr(), src.data_ptr(), src.numel(), max(reps["all_four"], 5), ctypes.byref(rate),
                                               torch.cuda.current_stream().cuda_stream), "swmhd_probe_copy")
        copy.append(rate.value)
    copy_gbs = statistics.median(copy)
    out = dict(cells=cells, window_ms=WINDOW_MS, calls_per_window=reps, single_field_calls_are_bitwise_the_fields_of_all_four=same,
               probe_copy_bytes=2 * src.numel(), probe_copy_gbs=spread(copy), paths={})
    gbs = {}
    for k in paths:
        parents, rd, wr = TRAFFIC[k]
        med = statistics.median(ms[k])
        gbs[k] = (rd + wr) * cells / (med * 1e-3) / 1e9
        out["paths"][k] = dict(parents_read=parents, bytes_read_per_cell=rd, bytes_written_per_cell=wr, us=spread([x * 1e3 for x in ms[k]]),
                               host_enqueue_us=spread([x * 1e3 for x in host[k]]), gbs=gbs[k], fraction_of_one_shot_copy=gbs[k] / copy_gbs)
    for k in paths:
        out["paths"][k]["fraction_of_output_fields_rate"] = gbs[k] / gbs["output_fields_uvAs"]
    return out


def time_single(rounds, N=4096):
    g = S.RectilinearGrid(size=(N, N), x=(-5, 5), y=(-5, 5))
    m = vortex(S.ShallowWaterModel(g, 9.81, 1.0))
    m.time_step(1e-4)
    m.synchronize()
    return dict(size=N, **measure(m, rounds))


def time_ensemble(rounds, B=256, N=64):
    g = S.RectilinearGrid(size=(N, N), x=(-5, 5), y=(-5, 5))
    ens = vortex(S.ShallowWaterEnsemble(g, B, 9.81, 1.0))
    ens.time_steps(2, 0.01)
    ens.synchronize()
    return dict(members=B, size=N, **measure(ens, rounds))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/derived_fields")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default="single,ensemble")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_derived.py measures on the GPU only"
    res = dict(device=torch.cuda.get_device_name(0), source_hash=_lib.source_hash(), rounds=a.rounds)
    for name, fn in (("single", time_single), ("ensemble", time_ensemble)):
        if name in a.only.split(","):
            res[name] = fn(a.rounds)
            print(name, json.dumps(res[name]), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "time_derived.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
