#!/usr/bin/env python3
"""Timings of the output frames and the writer (swmhd_output_fields_*, swmhd_amd.FieldTimeSeries), one process, alternating rounds.

    python tools/time_output.py [--out profiles/output_writer] [--rounds 5] [--only kernel,run,ensemble]

kernel    4096^2 vector-invariant fp64, default frame (u, v, A, s) -> float32: 24 B read (u, v, A; this mask does not touch h, and the
          second row of v a thread reads is its neighbour's first) + 16 B written per cell.  Kernel time by HIP
          events over `reps` launches; against the same frame made with what the library offered before on the device (torch slices of
          the parents, .to(float32), the torch expression for s), against swmhd_probe_copy (one-shot copy) and torch's copy of the
          same number of bytes, all in alternating rounds of this process.
run       64^2 to t = 30 (3000 steps, graph replay): wall time with no output, with FieldTimeSeries at 0.1 (301 frames), and with the
          checkpoint path (time_steps(10) + save_checkpoint per frame).
ensemble  256 x 64^2: one frame of all members in one launch against 256 member(m) round trips to the host.
Writes time_output.json into --out."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import swmhd_amd as S  # noqa: E402
from swmhd_amd import _lib  # noqa: E402


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


def vortex(m, amp=0.1):
    u0 = lambda X, Y: Y * np.exp(-(X ** 2 + Y ** 2))
    v0 = lambda X, Y: -X * np.exp(-(X ** 2 + Y ** 2))
    gauss = lambda a: (lambda X, Y: a * np.exp(-((X - 0.5) ** 2 + Y ** 2)) - a * np.exp(-((X + 0.5) ** 2 + Y ** 2)))
    members = getattr(m, "members", None)
    A0 = gauss(amp) if members is None else [gauss(amp * (1 + k / members)) for k in range(members)]
    n1, n2 = m.names[:2]
    m.set(**{n1: u0, n2: v0, "h": lambda X, Y: np.ones_like(X), "A": A0})
    return m


def torch_frame(m, out):
    """The default frame from the parents with torch alone (halos must be current)."""
    g = m.grid
    u, v, _, A = (f.data for f in m._raw_fields)
    I = lambda a, di, dj: a[g.Hy + dj:g.Hy + dj + g.Ny, g.Hx + di:g.Hx + di + g.Nx]
    out[0].copy_(I(u, 0, 0))
    out[1].copy_(I(v, 0, 0))
    out[2].copy_(I(A, 0, 0))
    v2 = 0.5 * (0.5 * (I(v, -1, 0) ** 2 + I(v, 0, 0) ** 2) + 0.5 * (I(v, -1, 1) ** 2 + I(v, 0, 1) ** 2))
    out[3].copy_(torch.sqrt(I(u, 0, 0) ** 2 + v2))


def time_kernel(rounds, N=4096, reps=20):
    g = S.RectilinearGrid(size=(N, N), x=(-5, 5), y=(-5, 5))
    m = vortex(S.ShallowWaterModel(g, 9.81, 1.0))
    m.time_step(1e-4)
    m.synchronize()                              # halos current for the torch path (its fill is not counted)
    out = torch.empty((4, N, N), dtype=torch.float32, device="cuda")
    ref = torch.empty_like(out)
    m.output_fields(out=out)
    torch_frame(m, ref)
    torch.cuda.synchronize()
    max_diff = float((out - ref).abs().max())
    nbytes = 40 * N * N                          # 24 B read (u, v, A) + 16 B written per cell
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    rate = ctypes.c_float()
    res = dict(kernel_ms=[], torch_ms=[], probe_copy_gbs=[], torch_copy_gbs=[])
    for _ in range(rounds):
        res["kernel_ms"].append(event_ms(lambda: m.output_fields(out=out), reps))
        res["torch_ms"].append(event_ms(lambda: torch_frame(m, ref), max(reps // 4, 2)))
        _lib.check(_lib.lib().swmhd_probe_copy(dst.data_ptr(), src.data_ptr(), src.numel(), reps, ctypes.byref(rate), torch.cuda.current_stream().cuda_stream),
                   "swmhd_probe_copy")
        res["probe_copy_gbs"].append(rate.value)
        res["torch_copy_gbs"].append(nbytes / (event_ms(lambda: dst.copy_(src), reps) * 1e-3) / 1e9)
    k = statistics.median(res["kernel_ms"])
    return dict(size=N, bytes_per_frame=nbytes, reps=reps, max_abs_diff_to_torch_frame=max_diff,
                kernel_ms=spread(res["kernel_ms"]), torch_frame_ms=spread(res["torch_ms"]),
                kernel_gbs=nbytes / (k * 1e-3) / 1e9, probe_copy_gbs=spread(res["probe_copy_gbs"]), torch_copy_gbs=spread(res["torch_copy_gbs"]),
                fraction_of_one_shot_copy=nbytes / (k * 1e-3) / 1e9 / statistics.median(res["probe_copy_gbs"]),
                fraction_of_torch_copy=nbytes / (k * 1e-3) / 1e9 / statistics.median(res["torch_copy_gbs"]),
                torch_over_kernel=statistics.median(res["torch_ms"]) / k)


def time_run(rounds, N=64, dt=0.01, stop=30.0):
    g = S.RectilinearGrid(size=(N, N), x=(-5, 5), y=(-5, 5))
    nsteps, every = int(round(stop / dt)), 10

    def fresh():
        m = vortex(S.ShallowWaterModel(g, 9.81, 1.0))
        m.capture_graph(dt)
        m.time_steps(20, dt)
        m.synchronize()
        m.clock_time, m.iteration = 0.0, 0
        return m

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def plain(m):
        for _ in range(nsteps // every):
            m.time_steps(every, dt)

    def writer(m):
        series = S.FieldTimeSeries(m, schedule=S.TimeInterval(0.1), capacity=nsteps // every + 1)
        S.run(m, dt, stop_iteration=nsteps, writers=[series])

    def checkpoints(m, d):
        m.save_checkpoint(os.path.join(d, "f0"))
        for k in range(nsteps // every):
            m.time_steps(every, dt)
            m.save_checkpoint(os.path.join(d, "f"))    # (overwritten: the cost is the synchronisation, the copies and the file)

    res = dict(no_output_s=[], writer_s=[], checkpoint_s=[])
    with tempfile.TemporaryDirectory() as d:
        for _ in range(rounds):
            res["no_output_s"].append(wall(lambda m=fresh(): plain(m)))
            res["writer_s"].append(wall(lambda m=fresh(): writer(m)))
            res["checkpoint_s"].append(wall(lambda m=fresh(): checkpoints(m, d)))
    out = {k: spread(v) for k, v in res.items()}
    out.update(size=N, steps=nsteps, frames=nsteps // every + 1,
               writer_over_no_output=out["writer_s"]["median"] / out["no_output_s"]["median"],
               checkpoint_over_writer=out["checkpoint_s"]["median"] / out["writer_s"]["median"])
    return out


def time_ensemble(rounds, B=256, N=64):
    g = S.RectilinearGrid(size=(N, N), x=(-5, 5), y=(-5, 5))
    ens = vortex(S.ShallowWaterEnsemble(g, B, 9.81, 1.0))
    ens.time_steps(2, 0.01)
    out = torch.empty((B, 4, N, N), dtype=torch.float32, device="cuda")
    res = dict(frame_ms=[], members_s=[])

    def members():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(B):
            [f.numpy() for f in ens.member(k).fields]
        return time.perf_counter() - t0
    for _ in range(rounds):
        res["frame_ms"].append(event_ms(lambda: ens.output_fields(out=out), 50))
        res["members_s"].append(members())
    return dict(members=B, size=N, frame_ms=spread(res["frame_ms"]), member_round_trips_s=spread(res["members_s"]),
                round_trips_over_frame=statistics.median(res["members_s"]) * 1e3 / statistics.median(res["frame_ms"]))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/output_writer")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default="kernel,run,ensemble")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_output.py measures on the GPU only"
    res = dict(device=torch.cuda.get_device_name(0), source_hash=_lib.source_hash(), rounds=a.rounds)
    for name, fn in (("kernel", time_kernel), ("run", time_run), ("ensemble", time_ensemble)):
        if name in a.only.split(","):
            res[name] = fn(a.rounds)
            print(name, json.dumps(res[name]), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "time_output.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
