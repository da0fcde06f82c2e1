#!/usr/bin/env python3
"""Timings of the zonal spectra (swmhd_zonal_spectra_*, ShallowWaterModel.zonal_spectra) against two yardsticks, one process, alternating
rounds.

    python tools/time_zonal_spectra.py [--out profiles/zonal_spectra] [--rounds 5] [--only single,ensemble]

single    4096^2 vector-invariant fp64, periodic: one field (u), (u, v, A), all seven.
ensemble  256 x 64^2 vector-invariant fp64, periodic: (u, v, A), all seven.
For each list of names, in the same process and alternating within a round:
    spectra  one zonal_spectra call (two launches: the row FFT in LDS with its per-workgroup sums, and the sum over workgroups)
    means    (a) zonal_means of the same names: the one-pass reader of the same rows, the floor
    torch    (b) what a user does without this call: output_fields(names, array_type=torch.float64), torch.fft.rfft along x, abs^2,
             the one-sided weights, the mean over rows -- where the installed torch provides rfft on this device (recorded if not)
Times are CALL times: HIP events around as many back-to-back calls of the Python method as fill a window of about 40 ms (counted from a
short trial); the host time of the enqueue loop per call is recorded beside every figure (`*_host_enqueue_ms`).  Output, frame and
workspace buffers are allocated once, outside the timed calls.  Also recorded: the largest difference between `spectra` and `torch` in
units of the mean square of the field, and the LDS bytes the transform moves per row (launch_plan.hpp / spectra.hip: per butterfly two
16-byte reads, one 16-byte twiddle read and two 16-byte writes; the row written once and the untangling pass reading two 16-byte
elements and a twiddle per mode).
Writes time_zonal_spectra.json into --out."""
import argparse
import json
import math
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


def torch_route(m, names, frame, weights):
    m.output_fields(names, out=frame)
    f = torch.fft.rfft(frame, dim=-1)
    p = (f.real * f.real + f.imag * f.imag) * weights
    return p.mean(dim=-2)


def lds_bytes_per_row(Nx):
    """LDS bytes one row moves in pass 1: the row written (8 Nx), log2(Nx) - 1 stages of Nx/4 butterflies at 80 B, Nx/2 + 1 modes of the
    untangling pass at 48 B"""
    L = int(math.log2(Nx))
    return 8 * Nx + (L - 1) * (Nx // 4) * 80 + (Nx // 2 + 1) * 48


def measure(m, lists, rounds):
    g, B = m.grid, getattr(m, "members", None) or 1
    lead = (B,) if getattr(m, "members", None) is not None else ()
    nk = g.Nx // 2 + 1
    weights = torch.full((nk,), 2.0 / g.Nx ** 2, dtype=torch.float64, device="cuda")
    weights[0] = weights[-1] = 1.0 / g.Nx ** 2
    have_rfft = True
    try:
        torch.fft.rfft(torch.zeros((2, g.Nx), dtype=torch.float64, device="cuda"), dim=-1)
        torch.cuda.synchronize()
    except Exception as e:      # noqa: BLE001 -- whatever the installed torch answers where it has no FFT for this device
        have_rfft = repr(e)
    out = dict(cells=B * g.Nx * g.Ny, rows=B * g.Ny, lds_bytes_per_row=lds_bytes_per_row(g.Nx), torch_rfft=have_rfft, window_ms=WINDOW_MS)
    for names in lists:
        key = "+".join(names)
        n = len(names)
        o = torch.empty(lead + (n, nk), dtype=torch.float64, device="cuda")
        zo = torch.empty(lead + (n, g.Ny), dtype=torch.float64, device="cuda")
        frame = torch.empty(lead + (n, g.Ny, g.Nx), dtype=torch.float64, device="cuda")
        paths = dict(spectra=lambda: m.zonal_spectra(names, out=o), means=lambda: m.zonal_means(names, out=zo))
        res = {}
        if have_rfft is True:
            paths["torch"] = lambda: torch_route(m, names, frame, weights)
            m.zonal_spectra(names, out=o)
            ref = torch_route(m, names, frame, weights)
            ms = (frame * frame).mean(dim=(-1, -2)).unsqueeze(-1)
            res["largest_difference_over_mean_square"] = float(((o - ref).abs() / ms).max())
            res["parseval_defect_over_mean_square"] = float(((o.sum(dim=-1, keepdim=True) - ms).abs() / ms).max())
        reps = {k: calls_per_window(fn) for k, fn in paths.items()}
        dev = {k: [] for k in paths}
        host = {k: [] for k in paths}
        for _ in range(rounds):
            for k, fn in paths.items():
                d, h = event_ms(fn, reps[k])
                dev[k].append(d)
                host[k].append(h)
        for k in paths:
            res[k + "_ms"] = spread(dev[k])
            res[k + "_host_enqueue_ms"] = spread(host[k])
        med = lambda k: res[k + "_ms"]["median"]
        res.update(calls_per_window=reps, spectra_over_means=med("spectra") / med("means"),
                   lds_gbs=n * B * g.Ny * lds_bytes_per_row(g.Nx) / (med("spectra") * 1e-3) / 1e9,
                   workspace_bytes=8 * int(_lib.lib().swmhd_zonal_spectra_workspace(g.Nx, g.Ny, n, B)), frame_buffer_bytes=frame.numel() * 8)
        if "torch" in paths:
            res["torch_over_spectra"] = med("torch") / med("spectra")
        out[key] = res
        print(key, json.dumps(res), flush=True)
        del frame
    return out


def time_single(rounds, N=4096):
    g = S.RectilinearGrid(size=(N, N), x=(-5, 5), y=(-5, 5))
    m = vortex(S.ShallowWaterModel(g, 9.81, 1.0))
    m.time_step(1e-4)
    m.synchronize()
    return dict(size=N, **measure(m, (("u",), ("u", "v", "A"), FRAME), rounds))


def time_ensemble(rounds, B=256, N=64):
    g = S.RectilinearGrid(size=(N, N), x=(-5, 5), y=(-5, 5))
    ens = vortex(S.ShallowWaterEnsemble(g, B, 9.81, 1.0))
    ens.time_steps(2, 0.01)
    ens.synchronize()
    return dict(members=B, size=N, **measure(ens, (("u", "v", "A"), FRAME), rounds))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/zonal_spectra")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default="single,ensemble")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_zonal_spectra.py measures on the GPU only"
    res = dict(device=torch.cuda.get_device_name(0), source_hash=_lib.source_hash(), rounds=a.rounds)
    for name, fn in (("single", time_single), ("ensemble", time_ensemble)):
        if name in a.only.split(","):
            res[name] = fn(a.rounds)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "time_zonal_spectra.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
