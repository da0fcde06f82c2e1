"""Bounded grids on y-slabs: the chain (SlabDecomposition(..., periodic=False), swmhd_ring_step_rk3_bc, SWMHD_OPEN_SOUTH / _NORTH,
swmhd_fill_halo_walls) and Bounded-x slabs of a periodic-y ring.

A Bounded-y grid cut into y-slabs is a chain, not a ring: rank 0 holds the south wall, the last rank the north wall, and every other
side is a cut whose halo rows come from the neighbour.  The reference's channel experiment -- (Periodic, Bounded), A = g y with
GradientBoundaryCondition(g) north and south on A (SWMHD_example.jl:18-22, divergence_sw_mhd.jl:17-21,34) -- is cut exactly across
its Bounded direction.  What the single-domain Bounded model computes must come out: bit for bit with the strict kernels (every row
is the same arithmetic, whoever computes it), within the fast tolerance of tests/test_bounded_gpu.py otherwise.  The slabs run on the
loopback transport (several rings in one process on one GPU, tests/test_loopback_gpu.py), on a ring of one over RCCL, and on the
torch p2p path (two processes over gloo)."""
import ctypes
import os
import socket
import sys
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 0.002
GA = -0.05           # the reference's commented gradient on A
TOPO = {"PB": ("Periodic", "Bounded"), "BB": ("Bounded", "Bounded"), "BP": ("Bounded", "Periodic")}


def _ics(form, topo):
    """the usual vortex; with a Bounded y the channel's A = g y on top of it"""
    from test_model_oracle import hf, uf, vf, Af
    A = (lambda X, Y: Af(X, Y) + GA * Y) if TOPO[topo][1] == "Bounded" else Af
    if form == "VectorInvariant":
        return dict(u=uf, v=vf, h=hf, A=A)
    return dict(uh=lambda X, Y: hf(X, Y) * uf(X, Y), vh=lambda X, Y: hf(X, Y) * vf(X, Y), h=hf, A=A)


def _bcs(S, topo):
    if TOPO[topo][1] != "Bounded":
        return None
    return {"A": S.FieldBoundaryConditions(north=S.GradientBoundaryCondition(GA), south=S.GradientBoundaryCondition(GA))}


def _run(m, plan, dt):
    for n in plan:
        m.time_step(dt) if n == 1 else m.time_steps(n, dt)
    m.synchronize()


def _single(S, form, topo, Nx, Ny, strict, dtype, plan, dt=DT, L=None):
    from test_model_oracle import Lx, Ly
    Lx, Ly = L or (Lx, Ly)
    g = S.RectilinearGrid(size=(Nx, Ny), x=(0, Lx), y=(0, Ly), topology=(*TOPO[topo], "Flat"))
    m = S.ShallowWaterModel(g, 9.81, 1.0, formulation=form, strict=strict, dtype=dtype, boundary_conditions=_bcs(S, topo))
    m.set(**_ics(form, topo))
    _run(m, plan, dt)
    return np.stack([f.numpy()[g.interior] for f in m.fields]), m


def _slabs(S, form, topo, Nx, Ny_local, world, strict, dtype, plan, dt=DT, L=None, keep=False):
    """every slab in its own thread + stream on the loopback transport; the global interior assembled from the slabs, the slabs'
    parents, and (keep=True) their diagnostics"""
    from test_model_oracle import Lx, Ly
    Lx, Ly = L or (Lx, Ly)
    rings = S.loopback_rings(world, 60.0)
    out, diags, hys, errs = [None] * world, [None] * world, [3] * world, []
    chain = TOPO[topo][1] == "Bounded"

    def work(r):
        try:
            torch.cuda.set_device(0)
            with torch.cuda.stream(torch.cuda.Stream()):
                dec = S.SlabDecomposition(Ny_local * world, world, r, periodic=not chain)
                g = dec.local_grid(S.RectilinearGrid, Nx, x=(0, Lx), y=(0, Ly), halo=dec.ring_halo(), topology=(*TOPO[topo], "Flat"))
                m = S.ShallowWaterModel(g, 9.81, 1.0, formulation=form, strict=strict, dtype=dtype, decomp=dec, ring=rings[r],
                                        boundary_conditions=_bcs(S, topo))
                m.set(**_ics(form, topo))
                _run(m, plan, dt)
                out[r] = np.stack([f.numpy() for f in m.fields])
                hys[r] = g.Hy
                if keep:
                    ws = torch.empty(S._lib.DIAG_WORKSPACE, dtype=torch.float64, device="cuda")
                    d = torch.empty(S._lib.DIAG_NOUT, dtype=torch.float64, device="cuda")
                    q = m.fields
                    rc = getattr(S._lib.lib(), f"swmhd_diagnostics_{m.sfx}")(
                        q[0].ptr, q[1].ptr, q[2].ptr, q[3].ptr, g.Nx, g.Ny, g.Hx, g.Hy, q[0].stride_y, g.dx, g.dy, m.g, 1.0,
                        m.form_code, 0, g.Ny, ws.data_ptr(), d.data_ptr(), S.fields._stream_ptr())
                    S._lib.check(rc, "swmhd_diagnostics")
                    diags[r] = d.cpu().numpy()
                m.close()
        except Exception as e:          # noqa: BLE001 -- reported by the main thread
            errs.append((r, repr(e)))

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errs, errs
    glob = np.concatenate([p[:, hy:hy + Ny_local, 3:3 + Nx] for p, hy in zip(out, hys)], axis=1)
    return glob, out, diags


CASES = [("PB", 2, 12), ("PB", 3, 33), ("PB", 2, 64), ("BB", 3, 12), ("BB", 2, 33), ("BP", 2, 33), ("BP", 3, 12)]


@pytest.mark.parametrize("topo,world,Ny_local", CASES)
@pytest.mark.parametrize("form", ["VectorInvariant", "Conservative"])
def test_strict_slabs_are_the_single_bounded_domain_bitwise(swmhd, topo, world, Ny_local, form):
    plan = (1, 2, 1)          # time_step and time_steps mixed: the exchange stays in flight between C calls
    want, _ = _single(swmhd, form, topo, 64, Ny_local * world, True, torch.float64, plan)
    got, parents, _ = _slabs(swmhd, form, topo, 64, Ny_local, world, True, torch.float64, plan)
    assert np.isfinite(got).all() and np.array_equal(got, want), np.abs(got - want).max()
    if TOPO[topo][1] == "Bounded":   # the cut sides end with the neighbours' edge rows; the walls are each slab's own
        for r in range(world - 1):
            assert np.array_equal(parents[r][:, Ny_local + 3:, 3:-3], parents[r + 1][:, 3:6, 3:-3])
            assert np.array_equal(parents[r + 1][:, :3, 3:-3], parents[r][:, Ny_local:Ny_local + 3, 3:-3])


@pytest.mark.parametrize("topo", ["PB", "BB"])
@pytest.mark.parametrize("form", ["VectorInvariant", "Conservative"])
def test_strict_fp32_slabs_bitwise(swmhd, topo, form):
    plan = (2, 1)
    want, _ = _single(swmhd, form, topo, 64, 66, True, torch.float32, plan)
    got, _, _ = _slabs(swmhd, form, topo, 64, 33, 2, True, torch.float32, plan)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("topo,dtype", [("PB", torch.float64), ("BB", torch.float64), ("BP", torch.float64), ("PB", torch.float32)])
@pytest.mark.parametrize("form", ["VectorInvariant", "Conservative"])
def test_fast_slabs_50_steps_within_tolerance_and_deterministic(swmhd, topo, dtype, form):
    plan = (1, 24, 25)
    want, _ = _single(swmhd, form, topo, 96, 99, False, dtype, plan)
    a, _, _ = _slabs(swmhd, form, topo, 96, 33, 3, False, dtype, plan)
    b, _, _ = _slabs(swmhd, form, topo, 96, 33, 3, False, dtype, plan)
    assert np.array_equal(a, b), "two runs of the same slabs differ: a race between the streams"
    tol = 1e-12 if dtype == torch.float64 else 1e-4      # the fast bars of tests/test_bounded_gpu.py
    scale = np.maximum(np.abs(want).max(axis=(1, 2), keepdims=True), 1.0)
    assert np.isfinite(a).all() and (np.abs(a - want) / scale).max() <= tol, (np.abs(a - want) / scale).max(axis=(1, 2))


@pytest.mark.parametrize("form", ["VectorInvariant", "Conservative"])
def test_fast_slabs_on_the_hybrid_launch(swmhd, form):
    """2 slabs of 1024 x 512 (0.52 Mcell each, above the hybrid threshold): row-marching kernel plus a wall frame on the wall side only,
    against the strict single domain (1024 x 1024 on the tile kernel) within the fast tolerance."""
    plan = (1, 2)
    L, dt = (2 * np.pi, 2 * np.pi), 2e-4
    want, _ = _single(swmhd, form, "PB", 1024, 1024, True, torch.float64, plan, dt=dt, L=L)
    got, _, _ = _slabs(swmhd, form, "PB", 1024, 512, 2, False, torch.float64, plan, dt=dt, L=L)
    scale = np.maximum(np.abs(want).max(axis=(1, 2), keepdims=True), 1.0)
    assert np.isfinite(got).all() and (np.abs(got - want) / scale).max() <= 1e-11, (np.abs(got - want) / scale).max(axis=(1, 2))


def test_diagnostics_summed_over_the_slabs_are_the_single_domain(swmhd):
    _, m = _single(swmhd, "VectorInvariant", "PB", 64, 66, True, torch.float64, (2,))
    d = m.diagnostics()
    _, _, diags = _slabs(swmhd, "VectorInvariant", "PB", 64, 22, 3, True, torch.float64, (2,), keep=True)
    ke, me, pe = (sum(x[k] for x in diags) for k in range(3))
    for got, key in ((ke, "kinetic_energy"), (me, "magnetic_energy"), (pe, "potential_energy")):
        assert abs(got - d[key]) <= 1e-12 * abs(d[key]), key
    assert max(x[3] for x in diags) == d["max_abs_u"] and max(x[4] for x in diags) == d["max_abs_v"]
    assert max(x[5] for x in diags) == d["max_abs_A"] and min(x[6] for x in diags) == d["min_h"]


# ---- entry-point level ------------------------------------------------------------------------------------------------------
def _bc_state(S, O, Nx, Ny, form, dtype, seed):
    """a Bounded-y state with filled halos (the oracle's fill), as device parents"""
    from test_bounded_oracle import state, fill_all, P, B
    q = fill_all(O, state(Nx, Ny, seed, form), Nx, Ny, (P, B), gradA=(None, None, GA, GA), dx=0.1, dy=0.1)
    return [torch.from_numpy(a.astype(dtype)).cuda() for a in q]


@pytest.mark.parametrize("Nx,Ny", [(64, 48), (1024, 768)])
@pytest.mark.parametrize("form,lor", [(1, 1), (0, 2)])
def test_open_flags_give_the_rows_of_the_whole_domain(swmhd, oracle, Nx, Ny, form, lor):
    """swmhd_tendencies_rk3 on the bottom half with BOUNDED_Y | OPEN_NORTH and on the top half with BOUNDED_Y | OPEN_SOUTH (halo rows
    cut from the whole parent) == the rows of the whole-domain call: bitwise in strict builds; fast builds (above 0.33 Mcell per slab
    the hybrid launch with a one-sided frame) within the fast tolerance of the whole-domain fast call."""
    S, B = swmhd, swmhd._lib
    L = B.lib()
    H, h = 3, Ny // 2
    q = _bc_state(S, oracle, Nx, Ny, form, np.float64, 5)
    sy = Nx + 2 * H
    f = L.swmhd_tendencies_rk3_f64
    ptrs = lambda ts: B.ptr_array([t.data_ptr() for t in ts])
    for strict in (True, False):
        base = B.BOUNDED_Y | (B.STRICT if strict else 0)
        qn = [torch.zeros_like(a) for a in q]
        Gn = [torch.zeros_like(a) for a in q]
        B.check(f(ptrs(q), ptrs(qn), ptrs(Gn), None, Nx, Ny, H, H, sy, 0.1, 0.1, 9.81, 1.0, form, lor, 1e-3, 8 / 15, 0.0, 1, 0, Ny,
                  base, None), "whole")
        for lo, flag in ((0, B.OPEN_NORTH), (h, B.OPEN_SOUTH)):
            qs = [a[lo:lo + h + 2 * H].contiguous() for a in q]
            qns = [torch.zeros_like(a) for a in qs]
            Gs = [torch.zeros_like(a) for a in qs]
            B.check(f(ptrs(qs), ptrs(qns), ptrs(Gs), None, Nx, h, H, H, sy, 0.1, 0.1, 9.81, 1.0, form, lor, 1e-3, 8 / 15, 0.0, 1, 0, h,
                      base | flag, None), "slab")
            torch.cuda.synchronize()
            for w, s in zip(list(Gn) + list(qn), list(Gs) + list(qns)):
                w = w[lo + H:lo + H + h, H:H + Nx].cpu().numpy(); s = s[H:H + h, H:H + Nx].cpu().numpy()
                if strict:
                    assert np.array_equal(w, s), (lo, np.abs(w - s).max())
                else:
                    assert np.abs(w - s).max() <= 1e-12 * max(np.abs(w).max(), 1.0), (lo, np.abs(w - s).max())


@pytest.mark.parametrize("sfx,dtype", [("f64", np.float64), ("f32", np.float32)])
def test_fill_halo_walls(swmhd, sfx, dtype):
    S, B = swmhd, swmhd._lib
    L = B.lib()
    Nx, Ny, H = 37, 21, 3
    sy = Nx + 2 * H
    rng = np.random.default_rng(3)
    base = [rng.standard_normal((Ny + 2 * H, sy)).astype(dtype) for _ in range(4)]
    ct = ctypes.c_double if sfx == "f64" else ctypes.c_float
    grads = (ct * 16)(*([float("nan")] * 14 + [GA, 0.125]))
    ptrs = lambda ts: B.ptr_array([t.data_ptr() for t in ts])
    for tx in (B.PERIODIC, B.BOUNDED):
        a = [torch.from_numpy(x.copy()).cuda() for x in base]
        b = [torch.from_numpy(x.copy()).cuda() for x in base]
        B.check(getattr(L, f"swmhd_fill_halo_{sfx}")(ptrs(a), 4, Nx, Ny, H, H, sy, tx, B.BOUNDED, 1, 2, grads, 0.1, 0.12, None), "fill")
        B.check(getattr(L, f"swmhd_fill_halo_walls_{sfx}")(ptrs(b), 4, Nx, Ny, H, H, sy, tx, 3, 1, 2, grads, 0.1, 0.12, None), "walls")
        torch.cuda.synchronize()
        for x, y in zip(a, b):
            assert np.array_equal(x.cpu().numpy(), y.cpu().numpy())
        # south wall only: the north halo rows keep their sentinel, the rest is the full fill's
        c = [torch.from_numpy(x.copy()).cuda() for x in base]
        for t in c:
            t[Ny + H:] = float("nan")
        B.check(getattr(L, f"swmhd_fill_halo_walls_{sfx}")(ptrs(c), 4, Nx, Ny, H, H, sy, tx, 1, 1, 2, grads, 0.1, 0.12, None), "walls")
        torch.cuda.synchronize()
        for x, y in zip(a, c):
            x, y = x.cpu().numpy(), y.cpu().numpy()
            assert np.isnan(y[Ny + H:]).all()
            assert np.array_equal(x[:Ny + H], y[:Ny + H])


# ---- a chain of one over RCCL -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rccl_world_of_one():
    import torch.distributed as dist
    if dist.is_initialized():
        pytest.skip("a process group already exists in this process")
    torch.cuda.set_device(0)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    yield dist
    torch.cuda.synchronize()
    dist.destroy_process_group()


@pytest.mark.parametrize("form", ["VectorInvariant", "Conservative"])
def test_chain_of_one_over_rccl_is_the_single_bounded_model_bitwise(rccl_world_of_one, swmhd, form):
    S = swmhd
    from test_model_oracle import Lx, Ly
    plan = (1, 3, 1)
    want, _ = _single(S, form, "PB", 96, 64, True, torch.float64, plan)
    dec = S.SlabDecomposition(64, 1, 0, force_ring=True, periodic=False)
    g = dec.local_grid(S.RectilinearGrid, 96, x=(0, Lx), y=(0, Ly), halo=dec.ring_halo(), topology=(*TOPO["PB"], "Flat"))
    m = S.ShallowWaterModel(g, 9.81, 1.0, formulation=form, strict=True, decomp=dec, boundary_conditions=_bcs(S, "PB"))
    assert m._ring is not None, "the native ring was not created"
    m.set(**_ics(form, "PB"))
    _run(m, plan, DT)
    got = np.stack([f.numpy()[g.interior] for f in m.fields])
    m.close()
    assert np.array_equal(got, want)


# ---- the torch p2p path: two ranks share the GPU over gloo ----------------------------------------------------------------------
def _p2p_worker(rank, world, port, form, out):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import swmhd_amd as S
        from test_model_oracle import Lx, Ly
        dec = S.SlabDecomposition(64, world, rank, periodic=False)
        g = dec.local_grid(S.RectilinearGrid, 64, x=(0, Lx), y=(0, Ly), halo=dec.ring_halo(), topology=(*TOPO["PB"], "Flat"))
        m = S.ShallowWaterModel(g, 9.81, 1.0, formulation=form, strict=True, decomp=dec, boundary_conditions=_bcs(S, "PB"))
        assert m._ring is None
        m.set(**_ics(form, "PB"))
        _run(m, (1, 2), DT)
        d = m.diagnostics()
        np.save(os.path.join(out, f"rank{rank}.npy"), np.stack([f.numpy()[g.interior] for f in m.fields]))
        if rank == 0:
            np.save(os.path.join(out, "diag.npy"), np.array([d["kinetic_energy"], d["magnetic_energy"], d["potential_energy"],
                                                               d["max_abs_u"], d["max_abs_v"], d["max_abs_A"], d["min_h"]]))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("form", ["VectorInvariant", "Conservative"])
def test_torch_p2p_chain_over_gloo_is_the_single_domain_bitwise(swmhd, tmp_path, form):
    import torch.multiprocessing as mp
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    mp.spawn(_p2p_worker, args=(2, port, form, str(tmp_path)), nprocs=2, join=True)
    want, m = _single(swmhd, form, "PB", 64, 64, True, torch.float64, (1, 2))
    got = np.concatenate([np.load(tmp_path / f"rank{r}.npy") for r in range(2)], axis=1)
    assert np.array_equal(got, want), np.abs(got - want).max()
    d, w = np.load(tmp_path / "diag.npy"), m.diagnostics()
    for k, key in enumerate(("kinetic_energy", "magnetic_energy", "potential_energy")):
        assert abs(d[k] - w[key]) <= 1e-12 * abs(w[key]), key
    assert (d[3], d[4], d[5], d[6]) == (w["max_abs_u"], w["max_abs_v"], w["max_abs_A"], w["min_h"])
