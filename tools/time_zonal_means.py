#!/usr/bin/env python3
"""Timings of the zonal means (swmhd_zonal_means_*, ShallowWaterModel.zonal_means) against what the library offered before for the
same numbers, one process, alternating rounds.

    python tools/time_zonal_means.py [--out profiles/zonal_means] [--rounds 5] [--only single,ensemble]

single    4096^2 vector-invariant fp64, periodic.
ensemble  256 x 64^2 vector-invariant fp64, periodic (16 384 rows, one wave each).
For each: one zonal_means call of the default names (u, v, A) and one of all fourteen, against
    frames   output_fields(names, array_type=torch.float64) followed by torch.mean(dim=-1): the default names directly; for all fourteen
             the frame of the seven fields, the seven products formed from it with torch (x and y periodic, torch.roll for the
             neighbours) and the means of both.
Times are CALL times: HIP events around as many back-to-back calls of the Python method as fill a window of about 40 ms (counted from a
short trial), so a call shorter than its host enqueue is timed at the host's pace; the host time of the enqueue loop per call is
recorded beside every figure (`*_host_enqueue_ms`) to tell the two apart.  The frame buffers are allocated once, outside the timed
calls.  Bytes: what each path must move at least, from the shapes -- the zonal kernel reads every parent its mask touches once and writes Ny doubles per profile; the frame path writes the frame, reads it
back for the mean, and the products add a write and a read each.  Also recorded: the largest difference between the two paths in
units of the bound of tests/zonal_cases.py (D(Nx) 2^-53 mean|term|, the row sums taken from the frame path).
Writes time_zonal_means.json into --out."""
import argparse
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

FRAME = ("u", "v", "h", "A", "s", "B_x", "B_y")
ALL = tuple(_lib.ZM_BITS)
DEFAULT = ("u", "v", "A")


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


def frames_default(m, frame):
    m.output_fields(DEFAULT, out=frame)
    return frame.mean(dim=-1)


def frames_all(m, frame):
    """All fourteen from the float64 frame of the seven fields (x and y periodic)."""
    m.output_fields(FRAME, out=frame)
    u, v, h, A, s, bx, by = frame.unbind(-3)
    west = lambda a: torch.roll(a, 1, -1)
    north = lambda a: torch.roll(a, -1, -2)
    xy = lambda a: 0.5 * (0.5 * (west(a) + a) + 0.5 * (west(north(a)) + north(a)))
    second = torch.stack([u * u, v * v, u * xy(v), bx * bx, by * by, by * xy(bx), v * (0.5 * (torch.roll(A, 1, -2) + A))], dim=-3)
    return torch.cat([frame.mean(dim=-1), second.mean(dim=-1)], dim=-2), second


def depth(Nx):
    terms0 = 4 * (Nx // 256) + min(4, Nx % 256)
    return terms0 - 1 + (min(64, -(-Nx // 4)) - 1).bit_length()


def measure(m, rounds):
    g, B = m.grid, getattr(m, "members", None) or 1
    lead = (B,) if getattr(m, "members", None) is not None else ()
    cells = B * g.Nx * g.Ny
    f3 = torch.empty(lead + (3, g.Ny, g.Nx), dtype=torch.float64, device="cuda")
    f7 = torch.empty(lead + (7, g.Ny, g.Nx), dtype=torch.float64, device="cuda")
    o3 = torch.empty(lead + (3, g.Ny), dtype=torch.float64, device="cuda")
    o14 = torch.empty(lead + (14, g.Ny), dtype=torch.float64, device="cuda")
    # agreement of the two paths, in units of the tests' bound
    m.zonal_means(ALL, out=o14)
    ref, second = frames_all(m, f7)
    sumabs = torch.cat([f7.abs().sum(dim=-1), second.abs().sum(dim=-1)], dim=-2)
    bound = depth(g.Nx) * 2.0 ** -53 * sumabs / g.Nx + 2.0 ** -53 * ref.abs()
    worst = float(((o14 - ref).abs() / bound.clamp_min(1e-300)).max())
    del second
    m.zonal_means(DEFAULT, out=o3)
    same3 = bool(torch.equal(o3, o14.index_select(-2, torch.tensor([0, 1, 3], device="cuda"))))
    paths = dict(zonal_default=lambda: m.zonal_means(DEFAULT, out=o3), frames_default=lambda: frames_default(m, f3),
                 zonal_all=lambda: m.zonal_means(ALL, out=o14), frames_all=lambda: frames_all(m, f7))
    reps = {k: calls_per_window(fn) for k, fn in paths.items()}
    res = {k + "_ms": [] for k in paths}
    host = {k + "_host_enqueue_ms": [] for k in paths}
    for _ in range(rounds):
        for k, fn in paths.items():
            dev_ms, host_ms = event_ms(fn, reps[k])
            res[k + "_ms"].append(dev_ms)
            host[k + "_host_enqueue_ms"].append(host_ms)
    out = {k: spread(v) for k, v in {**res, **host}.items()}
    med = lambda k: out[k]["median"]
    # least bytes per cell, vector-invariant fp64: the parents a mask touches, once each; frame path: the frame kernel's reads, the
    # frame written and read back, and for the seven products one write and one read each (their operands come from the frame again:
    # not counted)
    bytes_cell = dict(zonal_default=24, frames_default=24 + 24 + 24, zonal_all=32, frames_all=32 + 56 + 56 + 56 + 56)
    out.update(cells=cells, calls_per_window=reps, window_ms=WINDOW_MS, bytes_per_cell=bytes_cell,
               zonal_default_gbs=bytes_cell["zonal_default"] * cells / (med("zonal_default_ms") * 1e-3) / 1e9,
               zonal_all_gbs=bytes_cell["zonal_all"] * cells / (med("zonal_all_ms") * 1e-3) / 1e9,
               frames_over_zonal_default=med("frames_default_ms") / med("zonal_default_ms"),
               frames_over_zonal_all=med("frames_all_ms") / med("zonal_all_ms"),
               frame_buffer_bytes=dict(default=f3.numel() * 8, all=2 * f7.numel() * 8), profile_bytes=dict(default=o3.numel() * 8, all=o14.numel() * 8),
               largest_difference_over_bound=worst, default_is_bitwise_the_rows_of_all=same3)
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
    ap.add_argument("--out", default="profiles/zonal_means")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default="single,ensemble")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_zonal_means.py measures on the GPU only"
    res = dict(device=torch.cuda.get_device_name(0), source_hash=_lib.source_hash(), rounds=a.rounds)
    for name, fn in (("single", time_single), ("ensemble", time_ensemble)):
        if name in a.only.split(","):
            res[name] = fn(a.rounds)
            print(name, json.dumps(res[name]), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "time_zonal_means.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
