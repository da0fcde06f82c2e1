"""RK3 step time of the reference's channel -- (Periodic, Bounded), A = g y with GradientBoundaryCondition(g) north and south on A
(SWMHD_example.jl:18-22, divergence_sw_mhd.jl:17-21,34) -- on y-slabs, beside the single-domain Bounded model, in ONE process on one GPU:

    single   ShallowWaterModel on the whole grid (fused G- stage + boundary-condition fill per stage, stages driven from Python)
    chain1   the chain driver swmhd_ring_step_rk3_bc on a ring of ONE over RCCL (SlabDecomposition(force_ring=True, periodic=False)):
             both walls in the one slab, nothing exchanged -- what a chain costs over the single model when there is no neighbour
    loop2    two slabs of the loopback transport (swmhd_ring_create_loopback), each driven from its own thread: a CORRECTNESS vehicle,
             not a scaling figure -- both slabs share one chip, so their step time is at best that of the whole grid

fp64, both formulations, 4096 x 512 and 4096 x 4096 (or the sizes given).  Configurations alternate within a round; the median of
`rounds` rounds is printed.  Usage: python tools/time_channel_slabs.py [rounds] [NxN ...]"""
import os
import socket
import sys
import threading
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import swmhd_amd as S                 # noqa: E402
from swmhd_amd import configs         # noqa: E402

GA, DT, WARM, STEPS = -0.05, 1e-4, 5, 20
TOPO = ("Periodic", "Bounded", "Flat")


def _set(m):
    n1, n2 = m.names[:2]
    A0 = configs.two_gaussians(0.1)
    m.set(**{n1: lambda X, Y: 0 * X, n2: lambda X, Y: 0 * X, "h": lambda X, Y: np.ones_like(X), "A": lambda X, Y: A0(X, Y) + GA * Y})


def _bcs():
    return {"A": S.FieldBoundaryConditions(north=S.GradientBoundaryCondition(GA), south=S.GradientBoundaryCondition(GA))}


def _timed(m):
    m.time_steps(WARM, DT)
    m.synchronize()
    t0 = time.perf_counter()
    m.time_steps(STEPS, DT)
    m.synchronize()
    return (time.perf_counter() - t0) / STEPS


def single(Nx, Ny, form):
    g = S.RectilinearGrid(size=(Nx, Ny), x=(-5, 5), y=(-5, 5), topology=TOPO)
    m = S.ShallowWaterModel(g, formulation=form, boundary_conditions=_bcs())
    _set(m)
    return _timed(m)


def chain1(Nx, Ny, form):
    dec = S.SlabDecomposition(Ny, 1, 0, force_ring=True, periodic=False)
    g = dec.local_grid(S.RectilinearGrid, Nx, x=(-5, 5), y=(-5, 5), halo=dec.ring_halo(), topology=TOPO)
    m = S.ShallowWaterModel(g, formulation=form, decomp=dec, boundary_conditions=_bcs())
    assert m._ring is not None, "no native ring (RCCL)"
    _set(m)
    el = _timed(m)
    m.close()
    return el


def loop2(Nx, Ny, form, world=2):
    rings = S.loopback_rings(world, 120.0)
    bar = threading.Barrier(world)
    el, errs = [0.0] * world, []

    def work(r):
        try:
            torch.cuda.set_device(0)
            with torch.cuda.stream(torch.cuda.Stream()):
                dec = S.SlabDecomposition(Ny, world, r, periodic=False)
                g = dec.local_grid(S.RectilinearGrid, Nx, x=(-5, 5), y=(-5, 5), halo=dec.ring_halo(), topology=TOPO)
                m = S.ShallowWaterModel(g, formulation=form, decomp=dec, ring=rings[r], boundary_conditions=_bcs())
                _set(m)
                m.time_steps(WARM, DT)
                m.synchronize()
                bar.wait()
                t0 = time.perf_counter()
                m.time_steps(STEPS, DT)
                m.synchronize()
                el[r] = (time.perf_counter() - t0) / STEPS
                bar.wait()
                m.close()
        except Exception as e:        # noqa: BLE001
            errs.append(repr(e))
            bar.abort()

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join() for t in th]
    if errs:
        raise RuntimeError(errs)
    return max(el)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    sizes = [tuple(int(v) for v in a.split("x")) for a in sys.argv[2:]] or [(4096, 512), (4096, 4096)]
    import torch.distributed as dist
    torch.cuda.set_device(0)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        print(f"# {torch.cuda.get_device_name(0)}, fp64, {STEPS} timed steps after {WARM}, median of {rounds} alternating rounds; "
              "loop2 = two loopback slabs on ONE chip (correctness vehicle, not a scaling figure)", flush=True)
        for Nx, Ny in sizes:
            for form in ("VectorInvariant", "Conservative"):
                t = {"single": [], "chain1": [], "loop2": []}
                for _ in range(rounds):
                    t["single"].append(single(Nx, Ny, form))
                    t["chain1"].append(chain1(Nx, Ny, form))
                    t["loop2"].append(loop2(Nx, Ny, form))
                med = {k: float(np.median(v)) for k, v in t.items()}
                print(f"{form[:4]} {Nx}x{Ny}: single {med['single'] * 1e3:7.3f} ms/step   chain1 {med['chain1'] * 1e3:7.3f} "
                      f"({(med['chain1'] / med['single'] - 1) * 100:+5.1f} %)   loop2 {med['loop2'] * 1e3:7.3f}   "
                      f"spread single {min(t['single']) * 1e3:.3f}-{max(t['single']) * 1e3:.3f} chain1 "
                      f"{min(t['chain1']) * 1e3:.3f}-{max(t['chain1']) * 1e3:.3f}", flush=True)
    finally:
        torch.cuda.synchronize()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
