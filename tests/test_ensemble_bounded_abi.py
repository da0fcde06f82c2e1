"""CPU tests (no GPU) of the Bounded ensemble entry points (swmhd_ensemble_fill_halo_*, swmhd_ensemble_step_rk3_bc_*): exported, and
every argument error is returned before any HIP call; BoundedShallowWaterEnsemble refuses what it does not support before touching a
device."""
import ctypes

import pytest

FLOAT = {"f64": ctypes.c_double, "f32": ctypes.c_float}
Nx = Ny = 8
H, SY = 3, 14
SM = (Ny + 2 * H) * SY


def _bufs(sfx):
    buf = (FLOAT[sfx] * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    return buf, p, (ctypes.c_void_p * 4)(p, p, p, p)


def test_bounded_ensemble_symbols_are_exported(swmhd):
    L = swmhd._lib.lib()
    for sfx in ("f64", "f32"):
        for name in ("fill_halo", "step_rk3_bc"):
            assert hasattr(L, f"swmhd_ensemble_{name}_{sfx}")
            assert f"swmhd_ensemble_{name}_{sfx}" in swmhd._lib.EXPORTS
    assert swmhd.BoundedShallowWaterEnsemble is not None
    assert L.swmhd_version() == 300


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_bounded_step_refusals(swmhd, sfx):
    B = swmhd._lib
    L = B.lib()
    _buf, p, arr = _bufs(sfx)
    _buf2, _p2, alt = _bufs(sfx)
    _buf3, p3, _arr3 = _bufs(sfx)
    s = getattr(L, f"swmhd_ensemble_step_rk3_bc_{sfx}")

    def step(members=2, stride_m=SM, q=arr, flags=B.BOUNDED_Y | B.WRAP_X, nsteps=1, Hx=H, Hy=H, grad=p3, form=1, lor=1):
        return s(q, alt, arr, arr, members, stride_m, Nx, Ny, Hx, Hy, SY, 1.0, 1.0, 9.81, 1.0, form, lor, 0.01, nsteps, grad, flags,
                 None, None)
    assert step(members=0) == 1                          # members out of range
    assert step(members=-1) == 1
    assert step(members=B.ENSEMBLE_MAX_MEMBERS + 1) == 1
    assert step(stride_m=SM - 1) == 1                     # members would overlap
    assert step(q=None) == 1                              # null pointer arrays
    assert step(q=(ctypes.c_void_p * 4)(p, None, p, p)) == 1
    assert step(nsteps=-1) == 1
    for fl in (8, 128, 1 << 20):                          # unknown flags
        assert step(flags=B.BOUNDED_Y | fl) == 1, fl
    for fl in (B.MARCH_KERNEL, B.GM_IS_PREV_STATE, B.LEAVE_ROOM, B.RK3_ANCHOR):
        assert step(flags=B.BOUNDED_Y | fl) == 3, fl      # SWMHD_ENOTSUP
    assert step(flags=0) == 1                             # no Bounded direction: the periodic driver's job
    assert step(flags=B.WRAP_X | B.WRAP_Y) == 1
    assert step(flags=B.BOUNDED_Y | B.WRAP_Y) == 1        # WRAP on a Bounded direction
    assert step(flags=B.BOUNDED_X | B.WRAP_X) == 1
    assert step(flags=B.BOUNDED_X | B.BOUNDED_Y | B.WRAP_X) == 1
    assert step(Hx=2) == 2                                # the stencil needs halo 3 (SWMHD_EHALO)
    assert step(Hy=0, stride_m=Ny * SY) == 2              # a Bounded direction with halo 0
    assert step(form=1, lor=2) == 1                       # forcing that does not go with the formulation
    # the periodic ensemble calls keep refusing Bounded directions
    ps = getattr(L, f"swmhd_ensemble_step_rk3_{sfx}")
    assert ps(arr, alt, arr, arr, 2, SM, Nx, Ny, H, H, SY, 1.0, 1.0, 9.81, 1.0, 1, 1, 0.01, 1, B.BOUNDED_Y, None, None) == 3
    ph = getattr(L, f"swmhd_ensemble_fill_halo_periodic_{sfx}")
    assert ph(arr, 4, 0, SM, Nx, Ny, H, H, SY, 3, None) == 1


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_bounded_fill_halo_refusals(swmhd, sfx):
    B = swmhd._lib
    L = B.lib()
    _buf, p, arr = _bufs(sfx)
    h = getattr(L, f"swmhd_ensemble_fill_halo_{sfx}")

    def fill(f=arr, nf=4, members=2, stride_m=SM, Nx=Nx, Hx=H, Hy=H, sy=SY, tx=B.PERIODIC, ty=B.BOUNDED, dx=1.0):
        return h(f, nf, members, stride_m, Nx, Ny, Hx, Hy, sy, tx, ty, 1, 2, p, dx, 1.0, None)
    assert fill(members=0) == 1
    assert fill(members=B.ENSEMBLE_MAX_MEMBERS + 1) == 1
    assert fill(stride_m=SM - 1) == 1
    assert fill(f=None) == 1
    assert fill(f=(ctypes.c_void_p * 4)(p, p, None, p)) == 1
    assert fill(nf=0) == 1                                # nf outside 1..4
    assert fill(nf=5) == 1
    assert fill(tx=2) == 1                                # unknown topology
    assert fill(Hy=0, stride_m=Ny * SY) == 2              # Bounded with halo 0
    assert fill(tx=B.BOUNDED, Hx=0, sy=Nx) == 2
    assert fill(Nx=2, sy=8) == 2                          # halo deeper than the grid
    assert fill(sy=Nx + 2 * H - 1) == 1                   # row stride < Nx + 2Hx
    assert fill(dx=0.0) == 1                              # spacing


def test_bounded_step_accepts_4096_members_without_a_device(swmhd):
    """With nsteps = 0 the Bounded step driver validates and enqueues nothing, so no device is needed."""
    B = swmhd._lib
    L = B.lib()
    _buf, p, arr = _bufs("f64")
    _buf2, _p2, alt = _bufs("f64")
    for members, stride, flags in ((4096, SM, B.BOUNDED_Y | B.WRAP_X), (B.ENSEMBLE_MAX_MEMBERS, SM, B.BOUNDED_X | B.BOUNDED_Y),
                                   (3, SM + 17, B.BOUNDED_X | B.WRAP_Y | B.STRICT | B.TILE_KERNEL)):
        rc = L.swmhd_ensemble_step_rk3_bc_f64(arr, alt, arr, arr, members, stride, Nx, Ny, H, H, SY, 1.0, 1.0, 9.81, 1.0, 1, 1, 0.01, 0,
                                              None, flags, None, None)
        assert rc == 0, (members, stride, flags, rc)


def test_bounded_ensemble_class_refusals(swmhd):
    S = swmhd
    chan = S.RectilinearGrid(size=(16, 16), x=(0, 1), y=(0, 1), topology=("Periodic", "Bounded", "Flat"))
    bc = {"A": S.FieldBoundaryConditions(north=S.GradientBoundaryCondition(-0.05))}
    with pytest.raises(S._lib.SwmhdError):
        S.BoundedShallowWaterEnsemble(chan, 4, device="cpu", boundary_conditions=bc)          # no CPU fallback
    with pytest.raises(S._lib.SwmhdError):
        S.BoundedShallowWaterEnsemble(chan, 4, decomp=S.SlabDecomposition(16, 2, 0))
    slab = S.RectilinearGrid(size=(16, 8), x=(0, 1), y=(0, 1), j_offset=8, Ny_global=16, topology=("Periodic", "Bounded", "Flat"))
    with pytest.raises(S._lib.SwmhdError):
        S.BoundedShallowWaterEnsemble(slab, 4)
    with pytest.raises(S._lib.SwmhdError):                                                    # a condition on a Periodic side
        S.BoundedShallowWaterEnsemble(chan, 2, boundary_conditions={"A": S.FieldBoundaryConditions(west=S.GradientBoundaryCondition(0.1))})
    with pytest.raises(S._lib.SwmhdError):                                                    # ... of one member of a list
        S.BoundedShallowWaterEnsemble(chan, 2, boundary_conditions=[bc, {"h": S.FieldBoundaryConditions(east=S.GradientBoundaryCondition(0.1))}])
    with pytest.raises(S._lib.SwmhdError):                                                    # a list of the wrong length
        S.BoundedShallowWaterEnsemble(chan, 3, boundary_conditions=[bc, bc])
    with pytest.raises(S._lib.SwmhdError):                                                    # a field the formulation does not have
        S.BoundedShallowWaterEnsemble(chan, 2, formulation="Conservative", boundary_conditions={"u": bc["A"]})
    periodic = S.RectilinearGrid(size=(16, 16), x=(0, 1), y=(0, 1))
    with pytest.raises(S._lib.SwmhdError):                                                    # (Periodic, Periodic): ShallowWaterEnsemble
        S.BoundedShallowWaterEnsemble(periodic, 2)
    with pytest.raises(S._lib.SwmhdError):                                                    # ShallowWaterEnsemble still refuses Bounded
        S.ShallowWaterEnsemble(chan, 2)
