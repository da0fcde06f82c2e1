#!/usr/bin/env python3
"""Timings of the 2-D and isotropic spectra (swmhd_spectra2d_*, ShallowWaterModel.isotropic_spectra / power_spectra_2d), one process,
alternating rounds.

    python tools/time_spectra2d.py [--out profiles/spectra2d] [--rounds 5] [--only single,ensemble]

single    4096^2 vector-invariant fp64, periodic: one field (u) and (u, v, A).
ensemble  256 x 64^2 vector-invariant fp64, periodic: (u, v, A).
For each list of names, in the same process and alternating within a round:
    isotropic  one isotropic_spectra call (three launches: rows with the transposed store, columns with the shell partials, shells)
    plane      one power_spectra_2d call (two launches: rows, columns with the store of out_2d)
    both       the C call with out_shell and out_2d (three launches)
    zonal      zonal_spectra of the same names: the row half of the work without the transposed store
    copy       swmhd_probe_copy over as many bytes as the three passes of `isotropic` imply: the box's own copy rate
Times are CALL times, measured as tools/time_zonal_spectra.py measures them (HIP events around as many back-to-back calls as fill a
window of about 40 ms; the host time of the enqueue loop per call beside every figure).  Buffers are allocated outside the timed calls.
Also recorded, per list: the traffic the passes imply in bytes per cell -- pass 1 reads the parents of the fields (8 B per cell and
parent read) and writes 16 (Nx/2 + 1) / Nx; pass 2 reads those and writes 8 (Nx/2 + 1) / Nx of out_2d and 8 (Nx/2 + 1) NS / (Nx Ny) of
partials; pass 3 reads the partials -- the rate that traffic and the call time give, its share of the copy rate, the LDS bytes a
workgroup may take on the device and the plan's R.  The kernels' own shares of a call are read from a kernel trace of this tool
(profiles/spectra2d/README.md says how).
Writes time_spectra2d.json into --out."""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import swmhd_amd as S  # noqa: E402
from swmhd_amd import _lib, spectra2d  # noqa: E402
from swmhd_amd.fields import _stream_ptr  # noqa: E402
from time_zonal_spectra import WINDOW_MS, calls_per_window, event_ms, spread, vortex  # noqa: E402

# parents a vector-invariant frame field reads (u: q1; v: q2; A: A; ...): 8 B per cell each, counted once per field
PARENTS = {"u": 1, "v": 1, "h": 1, "A": 1, "s": 2, "B_x": 2, "B_y": 2}


def traffic_bytes_per_cell(names, Nx, Ny, NS, shells=True, plane=False):
    half = (Nx // 2 + 1) / Nx
    per = {"pass1_read": 8.0 * sum(PARENTS[n] for n in names), "pass1_write_transposed": 16.0 * half * len(names),
           "pass2_read": 16.0 * half * len(names), "pass2_write_out_2d": 8.0 * half * len(names) if plane else 0.0,
           "pass2_write_partials": 8.0 * half * NS / Ny * len(names) if shells else 0.0,
           "pass3_read": 8.0 * half * NS / Ny * len(names) if shells else 0.0}
    per["total"] = sum(per.values())
    return per


def c_call_both(m, names, E, P2, ws):
    """the C call with both outputs, for one run of names in mask order"""
    g = m.grid
    _, wx, wy = spectra2d.metric(g)
    which = sum(_lib.ZS_BITS[n] for n in names)
    ens = getattr(m, "members", None) is not None
    if ens:
        q = m._state
        ptrs, sy = [t.data_ptr() for t in q], q[0].stride(1)
        rc = getattr(m._L, f"swmhd_ensemble_spectra2d_{m.sfx}")(*ptrs, m.members, m.stride_m, g.Nx, g.Ny, g.Hx, g.Hy, sy, g.dx, g.dy, m.form_code, which, wx, wy,
                                                               ws.data_ptr(), E.data_ptr(), E.stride(-2), E.stride(0), P2.data_ptr(), P2.stride(-2),
                                                               P2.stride(-3), P2.stride(0), m._rwrap, _stream_ptr())
    else:
        q = m._raw_fields
        ptrs, sy = [f.ptr for f in q], q[0].stride_y
        rc = getattr(m._L, f"swmhd_spectra2d_{m.sfx}")(*ptrs, g.Nx, g.Ny, g.Hx, g.Hy, sy, g.dx, g.dy, m.form_code, which, wx, wy, ws.data_ptr(), E.data_ptr(),
                                                      E.stride(-2), P2.data_ptr(), P2.stride(-2), P2.stride(-3), m._rwrap, _stream_ptr())
    _lib.check(rc, "swmhd_spectra2d")


def measure(m, lists, rounds):
    g, B = m.grid, getattr(m, "members", None) or 1
    lead = (B,) if getattr(m, "members", None) is not None else ()
    nkx, NS = g.Nx // 2 + 1, spectra2d.shells(g)
    cells = B * g.Nx * g.Ny
    out = dict(cells=cells, shells=NS, window_ms=WINDOW_MS)
    L = _lib.lib()
    for names in lists:
        key = "+".join(names)
        n = len(names)
        E = torch.empty(lead + (n, NS), dtype=torch.float64, device="cuda")
        P2 = torch.empty(lead + (n, nkx, g.Ny), dtype=torch.float64, device="cuda")
        Z = torch.empty(lead + (n, nkx), dtype=torch.float64, device="cuda")
        m.isotropic_spectra(names, out=E)          # (allocates the cached workspace)
        ws = m._spectra2d_ws
        traffic = {k: traffic_bytes_per_cell(names, g.Nx, g.Ny, NS, shells=k != "plane", plane=k != "isotropic") for k in ("isotropic", "plane", "both")}
        nbytes = int(traffic["isotropic"]["total"] * cells / 2) // 16 * 16      # a copy moves every byte twice: read and write
        src = torch.zeros((nbytes // 8,), dtype=torch.float64, device="cuda")
        dst = torch.empty_like(src)
        rate = ctypes.c_float(0)
        paths = dict(isotropic=lambda: m.isotropic_spectra(names, out=E), plane=lambda: m.power_spectra_2d(names, out=P2),
                     both=lambda: c_call_both(m, names, E, P2, ws), zonal=lambda: m.zonal_spectra(names, out=Z))
        res = {}
        ms = (m.output_fields(names, array_type=torch.float64) ** 2).mean(dim=(-1, -2))
        res["parseval_defect_over_mean_square"] = float(((E.sum(dim=-1) - ms).abs() / ms).max())
        m.power_spectra_2d(names, out=P2)
        res["plane_parseval_defect_over_mean_square"] = float(((P2.sum(dim=(-1, -2)) - ms).abs() / ms).max())
        reps = {k: calls_per_window(fn) for k, fn in paths.items()}
        dev, host, copy = {k: [] for k in paths}, {k: [] for k in paths}, []
        for _ in range(rounds):
            for k, fn in paths.items():
                d, h = event_ms(fn, reps[k])
                dev[k].append(d)
                host[k].append(h)
            _lib.check(L.swmhd_probe_copy(dst.data_ptr(), src.data_ptr(), nbytes, 10, ctypes.byref(rate), torch.cuda.current_stream().cuda_stream),
                       "swmhd_probe_copy")
            copy.append(rate.value)
        torch.cuda.synchronize()
        for k in paths:
            res[k + "_ms"] = spread(dev[k])
            res[k + "_host_enqueue_ms"] = spread(host[k])
        med = lambda k: res[k + "_ms"]["median"]
        res["probe_copy_gbs"] = spread(copy)
        res["traffic_bytes_per_cell"] = traffic
        for k in ("isotropic", "plane", "both"):
            gbs = traffic[k]["total"] * cells / (med(k) * 1e-3) / 1e9
            res[k + "_implied_gbs"] = gbs
            res[k + "_share_of_copy_rate"] = gbs / res["probe_copy_gbs"]["median"]
        res.update(calls_per_window=reps, isotropic_over_zonal=med("isotropic") / med("zonal"), plane_over_zonal=med("plane") / med("zonal"),
                   workspace_bytes=8 * int(L.swmhd_spectra2d_workspace(g.Nx, g.Ny, n, B, *spectra2d.metric(g)[1:])))
        out[key] = res
        print(key, json.dumps(res), flush=True)
        del src, dst, P2
    return out


def time_single(rounds, N=4096):
    g = S.RectilinearGrid(size=(N, N), x=(-5, 5), y=(-5, 5))
    m = vortex(S.ShallowWaterModel(g, 9.81, 1.0))
    m.time_step(1e-4)
    m.synchronize()
    return dict(size=N, **measure(m, (("u",), ("u", "v", "A")), rounds))


def time_ensemble(rounds, B=256, N=64):
    g = S.RectilinearGrid(size=(N, N), x=(-5, 5), y=(-5, 5))
    ens = vortex(S.ShallowWaterEnsemble(g, B, 9.81, 1.0))
    ens.time_steps(2, 0.01)
    ens.synchronize()
    return dict(members=B, size=N, **measure(ens, (("u", "v", "A"),), rounds))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/spectra2d")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default="single,ensemble")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_spectra2d.py measures on the GPU only"
    props = torch.cuda.get_device_properties(0)
    res = dict(device=torch.cuda.get_device_name(0), source_hash=_lib.source_hash(), rounds=a.rounds,
               lds_bytes_per_workgroup=getattr(props, "shared_memory_per_block_optin", None) or getattr(props, "shared_memory_per_block", None))
    for name, fn in (("single", time_single), ("ensemble", time_ensemble)):
        if name in a.only.split(","):
            res[name] = fn(a.rounds)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "time_spectra2d.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
