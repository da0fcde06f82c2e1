"""CPU tests (no GPU) of Bounded grids on y-slabs: the chain decomposition's bookkeeping (SlabDecomposition(..., periodic=False)), the
chain halo exchange over gloo (2 and 3 ranks: cut sides receive the neighbour's edge rows, wall sides are left alone), and the argument
checks of the new C entry points (swmhd_ring_step_rk3_bc_*, swmhd_fill_halo_walls_*, SWMHD_OPEN_SOUTH / _NORTH), every one of which
returns before any HIP call."""
import ctypes
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("world", [1, 2, 3])
def test_chain_bookkeeping(swmhd, world):
    S = swmhd
    for r in range(world):
        d = S.SlabDecomposition(12 * world, world, r, periodic=False)
        assert (d.Ny_local, d.j_offset, d.periodic) == (12, 12 * r, False)
        assert d.south == (None if r == 0 else r - 1) and d.north == (None if r == world - 1 else r + 1)
        assert d.ring_halo() == (3, 3)
        assert d.walls_y() == (1 if r == 0 else 0) | (2 if r == world - 1 else 0)
        assert d.cuts() == (0 if r == 0 else 1) | (0 if r == world - 1 else 2)
        assert d.ring == (world > 1)
        p = S.SlabDecomposition(48 * world, world, r)      # the ring is unchanged
        assert (p.south, p.north, p.periodic, p.walls_y(), p.cuts()) == ((r - 1) % world, (r + 1) % world, True, 0, 3)
        assert p.ring_halo() == ((3, 9) if world > 1 else (3, 3))
    assert S.SlabDecomposition(12, 1, 0, force_ring=True, periodic=False).ring


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _exchange_worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from swmhd_amd import SlabDecomposition, exchange_y_halos
        Ny, H, W = 5, 3, 7
        glob = np.arange(world * Ny * W, dtype=np.float64).reshape(world * Ny, W) + 1.0
        res = {}
        for periodic in (False, True):
            dec = SlabDecomposition(world * Ny, world, rank, periodic=periodic)
            p = np.full((Ny + 2 * H, W), np.nan)
            p[H:H + Ny] = glob[rank * Ny:(rank + 1) * Ny]
            exchange_y_halos([torch.from_numpy(p)], Ny, H, dec)
            res[periodic] = p
        np.save(os.path.join(out, f"rank{rank}.npy"), np.stack([res[False], res[True]]))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_chain_exchange_over_gloo(tmp_path, world):
    mp.spawn(_exchange_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    Ny, H, W = 5, 3, 7
    glob = np.arange(world * Ny * W, dtype=np.float64).reshape(world * Ny, W) + 1.0
    for r in range(world):
        chain, ring = np.load(tmp_path / f"rank{r}.npy")
        assert np.array_equal(chain[H:H + Ny], glob[r * Ny:(r + 1) * Ny])
        # cut sides: the neighbour's edge rows; wall sides: the NaN sentinel, bit for bit
        if r > 0:
            assert np.array_equal(chain[:H], glob[r * Ny - H:r * Ny])
        else:
            assert np.isnan(chain[:H]).all()
        if r < world - 1:
            assert np.array_equal(chain[Ny + H:], glob[(r + 1) * Ny:(r + 1) * Ny + H])
        else:
            assert np.isnan(chain[Ny + H:]).all()
        # the periodic decomposition still wraps
        ext = np.concatenate([glob[-H:], glob, glob[:H]])
        assert np.array_equal(ring, ext[r * Ny:(r + 1) * Ny + 2 * H])


# ---- argument checks of the new entry points: all before any HIP call (libswmhd.so loads without a GPU) ---------------------------
FLOAT = {"f64": ctypes.c_double, "f32": ctypes.c_float}
Nx = Ny = 8
H, SY = 3, 14


def _bufs(sfx):
    buf = (FLOAT[sfx] * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    return buf, p, (ctypes.c_void_p * 4)(p, p, p, p)


def test_new_symbols_are_exported(swmhd):
    L = swmhd._lib.lib()
    for sfx in ("f64", "f32"):
        for name in ("ring_step_rk3_bc", "ring_exchange_y_sides", "fill_halo_walls"):
            assert hasattr(L, f"swmhd_{name}_{sfx}")
    assert (swmhd._lib.OPEN_SOUTH, swmhd._lib.OPEN_NORTH) == (4096, 8192)
    assert L.swmhd_version() == 300


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_ring_step_bc_refusals(swmhd, sfx):
    B = swmhd._lib
    L = B.lib()
    _b1, p, arr = _bufs(sfx)
    _b2, _p2, alt = _bufs(sfx)
    _b3, _p3, ga = _bufs(sfx)
    _b4, _p4, gb = _bufs(sfx)
    step = getattr(L, f"swmhd_ring_step_rk3_bc_{sfx}")
    ring = ctypes.c_void_p(None)

    def call(flags, r=ring):
        return step(r, arr, alt, ga, gb, Nx, Ny, H, H, SY, 0.1, 0.1, 9.81, 1.0, 1, 1, 1e-3, 1, None, flags, None, None)

    assert call(B.BOUNDED_Y) == 1                                                              # NULL ring
    assert call(B.BOUNDED_X | B.STRICT) == 1                                                   # NULL ring
    assert call(0) == 1                                                                        # no Bounded flag
    assert call(B.STRICT | B.WRAP_X) == 1
    assert call(B.BOUNDED_Y | B.OPEN_NORTH) == 1                                               # the chain decides its walls
    assert call(B.BOUNDED_Y | B.WRAP_Y) == 1
    assert call(B.BOUNDED_X | B.WRAP_X) == 1
    assert call(B.BOUNDED_Y | (1 << 20)) == 1                                                  # unknown flag
    assert call(B.BOUNDED_Y | B.RK3_ANCHOR) == 3
    assert call(B.BOUNDED_Y | B.GM_IS_PREV_STATE) == 3
    assert call(B.BOUNDED_X | B.MARCH_KERNEL) == 3
    # the periodic driver keeps the periodic slabs and points Bounded ones to the _bc call
    ring_step = getattr(L, f"swmhd_ring_step_rk3_{sfx}")
    fake = ctypes.c_void_p(1)    # never dereferenced: the flag check comes first
    for fl in (B.BOUNDED_X, B.BOUNDED_Y):
        assert ring_step(fake, arr, alt, ga, gb, Nx, Ny, H, H, SY, 0.1, 0.1, 9.81, 1.0, 1, 1, 1e-3, 1, fl, None, None) == 3
    ex = getattr(L, f"swmhd_ring_exchange_y_sides_{sfx}")
    assert ex(ring, arr, 4, Nx, Ny, H, H, SY, 3, None) == 1                                    # NULL ring
    assert ex(fake, arr, 4, Nx, Ny, H, H, SY, 4, None) == 1                                    # unknown side


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_slab_drivers_check_everything_before_touching_the_ring(swmhd, sfx):
    """both slab drivers check every stage argument, and return on nsteps == 0, before any HIP call and any read of the ring"""
    B = swmhd._lib
    L = B.lib()
    _b1, p, arr = _bufs(sfx)
    _b2, _p2, alt = _bufs(sfx)
    _b3, _p3, ga = _bufs(sfx)
    _b4, _p4, gb = _bufs(sfx)
    ring_step = getattr(L, f"swmhd_ring_step_rk3_{sfx}")
    ring_step_bc = getattr(L, f"swmhd_ring_step_rk3_bc_{sfx}")
    fake = ctypes.c_void_p(1)    # never dereferenced
    for strict in (0, B.STRICT):
        def step(form=1, lorentz=1, q_alt=alt, nsteps=1, Hx=H, flags=0):
            return ring_step(fake, arr, q_alt, ga, gb, Nx, Ny, Hx, H, Nx + 2 * Hx, 0.1, 0.1, 9.81, 1.0, form, lorentz, 1e-3, nsteps,
                             strict | flags, None, None)

        assert step(form=7) == 1                                   # unknown formulation
        assert step(form=B.CONSERVATIVE, lorentz=B.LORENTZ_JACOBIAN) == 1
        assert step(q_alt=arr) == 1                                # the new state aliases the state read through halos
        assert step(Hx=Nx + 1) == 2                                # the x fill's halo check (x halos in memory)
        assert step(Hx=Nx + 1, flags=B.WRAP_X) == 2                # the stage's own (x wrapped on read)
        for fl in (0, B.WRAP_X):
            alt_flag = ctypes.c_int(7)
            assert ring_step(fake, arr, alt, ga, gb, Nx, Ny, H, H, SY, 0.1, 0.1, 9.81, 1.0, 1, 1, 1e-3, 0, strict | fl,
                             ctypes.byref(alt_flag), None) == 0
            assert alt_flag.value == 0
        for fl in (B.BOUNDED_X, B.BOUNDED_Y, B.BOUNDED_X | B.BOUNDED_Y):
            alt_flag = ctypes.c_int(7)
            assert ring_step_bc(fake, arr, alt, ga, gb, Nx, Ny, H, H, SY, 0.1, 0.1, 9.81, 1.0, 1, 1, 1e-3, 0, None, strict | fl,
                                ctypes.byref(alt_flag), None) == 0
            assert alt_flag.value == 0
            assert ring_step_bc(fake, arr, arr, ga, gb, Nx, Ny, H, H, SY, 0.1, 0.1, 9.81, 1.0, 1, 1, 1e-3, 1, None, strict | fl,
                                None, None) == 1


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_open_flags_and_wall_fill_refusals(swmhd, sfx):
    B = swmhd._lib
    L = B.lib()
    _b1, p, arr = _bufs(sfx)
    _b2, _p2, alt = _bufs(sfx)
    _b3, _p3, gn = _bufs(sfx)
    t = getattr(L, f"swmhd_tendencies_rk3_{sfx}")

    def tend(flags):
        return t(arr, alt, gn, None, Nx, Ny, H, H, SY, 0.1, 0.1, 9.81, 1.0, 1, 1, 1e-3, 8 / 15, 0.0, 1, 0, Ny, flags, None)

    for open_ in (B.OPEN_SOUTH, B.OPEN_NORTH, B.OPEN_SOUTH | B.OPEN_NORTH):
        assert tend(open_) == 1                          # OPEN_* without BOUNDED_Y
        assert tend(open_ | B.BOUNDED_X) == 1
        assert tend(open_ | B.BOUNDED_Y | B.RK3_ANCHOR) == 3
        assert tend(open_ | B.BOUNDED_Y | B.MARCH_KERNEL) == 3
        assert tend(open_ | B.BOUNDED_Y | B.WRAP_Y) == 1
    tp = getattr(L, f"swmhd_tendencies_{sfx}")
    assert tp(p, p, p, p, p, p, p, p, Nx, Ny, H, H, SY, 0.1, 0.1, 9.81, 1.0, 1, 1, 0, Ny, B.OPEN_NORTH, None) == 1
    fw = getattr(L, f"swmhd_fill_halo_walls_{sfx}")
    for walls in (4, 8, -1):
        assert fw(arr, 4, Nx, Ny, H, H, SY, B.BOUNDED, walls, 1, 2, None, 0.1, 0.1, None) == 1   # unknown walls_y bits
    assert fw(arr, 4, Nx, Ny, H, H, SY, 2, 3, 1, 2, None, 0.1, 0.1, None) == 1                  # unknown topology code
    assert fw(None, 4, Nx, Ny, H, H, SY, B.BOUNDED, 3, 1, 2, None, 0.1, 0.1, None) == 1
    assert fw(arr, 4, Nx, Ny, H, 0, SY, B.BOUNDED, 1, 1, 2, None, 0.1, 0.1, None) == 2          # a wall needs a halo line


def test_model_refusals_before_touching_a_device(swmhd):
    """the decomposition checks of ShallowWaterModel come before its fields are allocated"""
    S = swmhd
    gb = S.RectilinearGrid(size=(16, 16), x=(0, 1), y=(0, 1), topology=("Periodic", "Bounded", "Flat"))
    gp = S.RectilinearGrid(size=(16, 16), x=(0, 1), y=(0, 1))
    with pytest.raises(S._lib.SwmhdError, match="chain"):
        S.ShallowWaterModel(gb, decomp=S.SlabDecomposition(16, 1, 0, force_ring=True), device="cpu")
    with pytest.raises(S._lib.SwmhdError, match="Bounded y"):
        S.ShallowWaterModel(gp, decomp=S.SlabDecomposition(16, 1, 0, periodic=False), device="cpu")
