"""CPU tests (no GPU) of the ensemble entry points (swmhd_ensemble_*): exported, and every argument error is returned before any HIP
call; ShallowWaterEnsemble refuses what it does not support before touching a device."""
import ctypes

import pytest

FLOAT = {"f64": ctypes.c_double, "f32": ctypes.c_float}


def _bufs(sfx):
    buf = (FLOAT[sfx] * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    return buf, p, (ctypes.c_void_p * 4)(p, p, p, p)


def test_ensemble_symbols_are_exported(swmhd):
    L = swmhd._lib.lib()
    for sfx in ("f64", "f32"):
        for name in ("tendencies_rk3", "step_rk3", "fill_halo_periodic", "diagnostics"):
            assert hasattr(L, f"swmhd_ensemble_{name}_{sfx}")
            assert f"swmhd_ensemble_{name}_{sfx}" in swmhd._lib.EXPORTS
    assert swmhd._lib.ensemble_diag_workspace(3, 64, 64) == 3 * 7 * 16
    assert swmhd._lib.ensemble_diag_workspace(2, 1024, 1024) == 2 * 7 * 1024


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_ensemble_tendencies_refusals(swmhd, sfx):
    B = swmhd._lib
    L = B.lib()
    _buf, p, arr = _bufs(sfx)
    # a distinct qnew set (aliasing q is refused on its own)
    buf2 = (FLOAT[sfx] * 64)()
    p2 = ctypes.cast(buf2, ctypes.c_void_p)
    alt = (ctypes.c_void_p * 4)(p2, p2, p2, p2)
    t = getattr(L, f"swmhd_ensemble_tendencies_rk3_{sfx}")
    Nx = Ny = 8
    H, sy = 3, 14
    sm = (Ny + 2 * H) * sy

    def call(members=2, stride_m=sm, q=arr, qnew=alt, Gn=arr, Gm=None, Nx=Nx, Ny=Ny, Hx=H, Hy=H, sy=sy, form=1, lor=1, flags=0):
        return t(q, qnew, Gn, Gm, members, stride_m, Nx, Ny, Hx, Hy, sy, 1.0, 1.0, 9.81, 1.0, form, lor, 0.01, 8 / 15, 0.0, 1, flags, None)
    assert call(members=0) == 1                       # members < 1
    assert call(members=-3) == 1
    assert call(members=B.ENSEMBLE_MAX_MEMBERS + 1) == 1
    assert call(stride_m=sm - 1) == 1                  # members would overlap
    assert call(q=None) == 1                           # null pointer arrays
    assert call(qnew=(ctypes.c_void_p * 4)(p2, None, p2, p2)) == 1   # a null field
    assert call(qnew=arr) == 1                         # qnew aliases q
    assert call(flags=8) == 1                          # unknown flags
    assert call(flags=128) == 1
    assert call(flags=1 << 20) == 1
    assert call(sy=Nx + 2 * H - 1, stride_m=10 ** 6) == 1   # row stride < Nx + 2Hx
    assert call(Nx=0) == 1                              # extents
    assert call(Hx=2) == 2                              # WENO5 needs halo 3 (SWMHD_EHALO)
    assert call(form=1, lor=2) == 1                     # forcing that does not go with the formulation
    for fl in (B.BOUNDED_X, B.BOUNDED_Y, B.MARCH_KERNEL, B.GM_IS_PREV_STATE, B.LEAVE_ROOM):
        assert call(flags=fl) == 3, fl                   # SWMHD_ENOTSUP
    assert call(flags=B.RK3_ANCHOR | B.STRICT) == 3     # anchor form: fast builds only, as for one grid


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_ensemble_step_halo_diagnostics_refusals(swmhd, sfx):
    B = swmhd._lib
    L = B.lib()
    _buf, p, arr = _bufs(sfx)
    Nx = Ny = 8
    H, sy = 3, 14
    sm = (Ny + 2 * H) * sy
    s = getattr(L, f"swmhd_ensemble_step_rk3_{sfx}")
    _buf2, _p2, alt = _bufs(sfx)

    def step(members=2, stride_m=sm, q=arr, flags=B.WRAP_X | B.WRAP_Y, nsteps=1, Hx=H):
        return s(q, alt, arr, arr, members, stride_m, Nx, Ny, Hx, H, sy, 1.0, 1.0, 9.81, 1.0, 1, 1, 0.01, nsteps, flags, None, None)
    assert step(members=0) == 1
    assert step(stride_m=sm - 1) == 1
    assert step(q=None) == 1
    assert step(nsteps=-1) == 1
    assert step(flags=8) == 1
    assert step(Hx=2) == 2
    for fl in (B.BOUNDED_X, B.BOUNDED_Y, B.MARCH_KERNEL, B.GM_IS_PREV_STATE, B.LEAVE_ROOM):
        assert step(flags=fl) == 3, fl
    h = getattr(L, f"swmhd_ensemble_fill_halo_periodic_{sfx}")
    assert h(arr, 4, 0, sm, Nx, Ny, H, H, sy, 3, None) == 1             # members < 1
    assert h(arr, 4, 2, sm - 1, Nx, Ny, H, H, sy, 3, None) == 1         # stride_m too small
    assert h(arr, 5, 2, sm, Nx, Ny, H, H, sy, 3, None) == 1             # more than 4 fields
    assert h(None, 4, 2, sm, Nx, Ny, H, H, sy, 3, None) == 1            # null array
    assert h(arr, 4, 2, sm, Nx, Ny, H, H, sy, 4, None) == 1             # unknown `which`
    assert h(arr, 4, 2, sm, 2, Ny, H, H, 8, 3, None) == 2               # Nx < Hx
    d = getattr(L, f"swmhd_ensemble_diagnostics_{sfx}")

    def diag(members=2, stride_m=sm, ws=p, out=p, form=1, Hx=H):
        return d(p, p, p, p, members, stride_m, Nx, Ny, Hx, H, sy, 1.0, 1.0, 9.81, 1.0, form, ws, out, None)
    assert diag(members=0) == 1
    assert diag(members=B.ENSEMBLE_MAX_MEMBERS + 1) == 1
    assert diag(stride_m=sm - 1) == 1
    assert diag(ws=None) == 1
    assert diag(out=None) == 1
    assert diag(form=5) == 1
    assert diag(Hx=0) == 2


def test_ensemble_accepts_4096_members_and_pitched_strides(swmhd):
    """Validation passes for a large ensemble: with nsteps = 0 the step driver enqueues nothing, so no device is needed."""
    B = swmhd._lib
    L = B.lib()
    _buf, p, arr = _bufs("f64")
    sm = (8 + 6) * 14
    for members, stride in ((4096, sm), (B.ENSEMBLE_MAX_MEMBERS, sm), (3, sm + 17)):
        rc = L.swmhd_ensemble_step_rk3_f64(arr, arr, arr, arr, members, stride, 8, 8, 3, 3, 14, 1.0, 1.0, 9.81, 1.0, 1, 1, 0.01, 0,
                                           B.WRAP_X | B.WRAP_Y, None, None)
        assert rc == 0, (members, stride, rc)


def test_ensemble_class_refusals(swmhd):
    import torch
    S = swmhd
    bounded = S.RectilinearGrid(size=(16, 16), x=(0, 1), y=(0, 1), topology=("Periodic", "Bounded", "Flat"))
    with pytest.raises(S._lib.SwmhdError):
        S.ShallowWaterEnsemble(bounded, 4)
    with pytest.raises(S._lib.SwmhdError):
        S.ShallowWaterEnsemble(S.RectilinearGrid(size=(16, 16), x=(0, 1), y=(0, 1), topology=("Bounded", "Periodic", "Flat")), 4)
    g = S.RectilinearGrid(size=(16, 16), x=(0, 1), y=(0, 1))
    with pytest.raises(S._lib.SwmhdError):
        S.ShallowWaterEnsemble(g, 4, device="cpu")             # no CPU fallback
    with pytest.raises(S._lib.SwmhdError):
        S.ShallowWaterEnsemble(g, 4, decomp=S.SlabDecomposition(16, 2, 0))
    slab = S.RectilinearGrid(size=(16, 8), x=(0, 1), y=(0, 1), j_offset=8, Ny_global=16)
    with pytest.raises(S._lib.SwmhdError):
        S.ShallowWaterEnsemble(slab, 4)
    with pytest.raises(S._lib.SwmhdError):
        S.ShallowWaterEnsemble(g, 0, device="cpu")
    with pytest.raises(S._lib.SwmhdError):
        S.ShallowWaterEnsemble(g, 2, dtype=torch.float16)
