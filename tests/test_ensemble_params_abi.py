"""CPU tests (no GPU) of the per-member-parameter ensemble entry points (swmhd_ensemble_*_params): exported, declared, and every
argument error is returned before any HIP call, exactly as by the scalar counterpart; the ensemble classes refuse sequences of the
wrong length, run() with a per-member dt, and clock_time once the members' clocks differ -- all before touching a device."""
import ctypes

import numpy as np
import pytest

FLOAT = {"f64": ctypes.c_double, "f32": ctypes.c_float}
NAMES = ("tendencies_rk3_params", "step_rk3_params", "step_rk3_bc_params", "diagnostics_params")
Nx = Ny = 8
H, SY = 3, 14
SM = (Ny + 2 * H) * SY


def _bufs(sfx):
    buf = (FLOAT[sfx] * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    return buf, p, (ctypes.c_void_p * 4)(p, p, p, p)


def test_params_symbols_are_exported(swmhd):
    L = swmhd._lib.lib()
    for sfx in ("f64", "f32"):
        for name in NAMES:
            assert hasattr(L, f"swmhd_ensemble_{name}_{sfx}")
            assert f"swmhd_ensemble_{name}_{sfx}" in swmhd._lib.EXPORTS
    assert swmhd._lib.ENSEMBLE_NPARAMS == 3
    assert L.swmhd_version() == 300


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_params_tendencies_refusals(swmhd, sfx):
    B = swmhd._lib
    L = B.lib()
    _buf, p, arr = _bufs(sfx)
    _buf2, p2, alt = _bufs(sfx)
    t = getattr(L, f"swmhd_ensemble_tendencies_rk3_params_{sfx}")

    def call(members=2, stride_m=SM, q=arr, qnew=alt, params=p, Hx=H, sy=SY, form=1, lor=1, flags=0):
        return t(q, qnew, arr, None, members, stride_m, Nx, Ny, Hx, H, sy, 1.0, 1.0, params, form, lor, 8 / 15, 0.0, 1, flags, None)
    assert call(params=None) == 1                      # no table
    assert call(members=0) == 1
    assert call(members=B.ENSEMBLE_MAX_MEMBERS + 1) == 1
    assert call(stride_m=SM - 1) == 1                  # members would overlap
    assert call(q=None) == 1
    assert call(qnew=arr) == 1                         # qnew aliases q
    assert call(flags=8) == 1                          # unknown flags
    assert call(sy=Nx + 2 * H - 1, stride_m=10 ** 6) == 1
    assert call(Hx=2) == 2                             # SWMHD_EHALO
    assert call(form=1, lor=2) == 1
    for fl in (B.BOUNDED_X, B.BOUNDED_Y, B.MARCH_KERNEL, B.GM_IS_PREV_STATE, B.LEAVE_ROOM):
        assert call(flags=fl) == 3, fl                  # SWMHD_ENOTSUP, as the scalar call
    assert call(flags=B.RK3_ANCHOR | B.STRICT) == 3


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_params_step_and_diagnostics_refusals(swmhd, sfx):
    B = swmhd._lib
    L = B.lib()
    _buf, p, arr = _bufs(sfx)
    _buf2, _p2, alt = _bufs(sfx)
    s = getattr(L, f"swmhd_ensemble_step_rk3_params_{sfx}")

    def step(members=2, stride_m=SM, q=arr, params=p, flags=B.WRAP_X | B.WRAP_Y, nsteps=1, Hx=H):
        return s(q, alt, arr, arr, members, stride_m, Nx, Ny, Hx, H, SY, 1.0, 1.0, params, 1, 1, nsteps, flags, None, None)
    assert step(params=None) == 1
    assert step(params=None, nsteps=0) == 1            # the table is checked even when nothing would be enqueued
    assert step(members=0) == 1
    assert step(members=B.ENSEMBLE_MAX_MEMBERS + 1) == 1
    assert step(stride_m=SM - 1) == 1
    assert step(q=None) == 1
    assert step(nsteps=-1) == 1
    assert step(flags=8) == 1
    assert step(Hx=2) == 2
    for fl in (B.BOUNDED_X, B.BOUNDED_Y, B.MARCH_KERNEL, B.GM_IS_PREV_STATE, B.LEAVE_ROOM):
        assert step(flags=fl) == 3, fl
    assert step(nsteps=0) == 0                          # nothing enqueued: no device needed

    bc = getattr(L, f"swmhd_ensemble_step_rk3_bc_params_{sfx}")

    def stepbc(members=2, stride_m=SM, params=p, flags=B.BOUNDED_Y | B.WRAP_X, nsteps=1, grad=None):
        return bc(arr, alt, arr, arr, members, stride_m, Nx, Ny, H, H, SY, 1.0, 1.0, params, 1, 1, nsteps, grad, flags, None, None)
    assert stepbc(params=None) == 1
    assert stepbc(members=0) == 1
    assert stepbc(stride_m=SM - 1) == 1
    assert stepbc(flags=B.WRAP_X | B.WRAP_Y) == 1       # no Bounded direction: the periodic driver's job
    assert stepbc(flags=0, nsteps=0) == 1
    assert stepbc(flags=B.BOUNDED_Y | B.WRAP_Y) == 1    # Bounded or wrapped, not both
    for fl in (B.MARCH_KERNEL, B.GM_IS_PREV_STATE, B.LEAVE_ROOM, B.RK3_ANCHOR):
        assert stepbc(flags=B.BOUNDED_Y | fl) == 3, fl
    assert stepbc(nsteps=-1) == 1
    assert stepbc(nsteps=0) == 0
    assert stepbc(flags=B.BOUNDED_X | B.BOUNDED_Y | B.STRICT, nsteps=0, grad=p) == 0

    d = getattr(L, f"swmhd_ensemble_diagnostics_params_{sfx}")

    def diag(members=2, stride_m=SM, params=p, ws=p, out=p, form=1, Hx=H):
        return d(p, p, p, p, members, stride_m, Nx, Ny, Hx, H, SY, 1.0, 1.0, params, 1.0, form, ws, out, None)
    assert diag(params=None) == 1
    assert diag(members=0) == 1
    assert diag(members=B.ENSEMBLE_MAX_MEMBERS + 1) == 1
    assert diag(stride_m=SM - 1) == 1
    assert diag(ws=None) == 1
    assert diag(out=None) == 1
    assert diag(form=5) == 1
    assert diag(Hx=0) == 2


def test_params_accept_65535_members_and_pitched_strides(swmhd):
    B = swmhd._lib
    L = B.lib()
    for sfx in ("f64", "f32"):
        _buf, p, arr = _bufs(sfx)
        for members, stride in ((4096, SM), (B.ENSEMBLE_MAX_MEMBERS, SM), (3, SM + 17)):
            rc = getattr(L, f"swmhd_ensemble_step_rk3_params_{sfx}")(arr, arr, arr, arr, members, stride, Nx, Ny, H, H, SY, 1.0, 1.0, p, 1, 1, 0,
                                                                    B.WRAP_X | B.WRAP_Y, None, None)
            assert rc == 0, (sfx, members, stride, rc)
            rc = getattr(L, f"swmhd_ensemble_step_rk3_bc_params_{sfx}")(arr, arr, arr, arr, members, stride, Nx, Ny, H, H, SY, 1.0, 1.0, p, 0, 2,
                                                                       0, None, B.BOUNDED_X, None, None)
            assert rc == 0, (sfx, members, stride, rc)


def test_wrong_length_sequences_are_refused_before_any_device(swmhd):
    S = swmhd
    g = S.RectilinearGrid(size=(16, 16), x=(0, 1), y=(0, 1))
    gb = S.RectilinearGrid(size=(16, 16), x=(0, 1), y=(0, 1), topology=("Periodic", "Bounded", "Flat"))
    for cls, grid in ((S.ShallowWaterEnsemble, g), (S.BoundedShallowWaterEnsemble, gb)):
        for kw in (dict(gravitational_acceleration=[9.81, 1.0, 2.0]), dict(coriolis_f=(1.0,)), dict(coriolis_f=np.ones(5)),
                   dict(gravitational_acceleration=np.ones((4, 1)))):
            with pytest.raises(S._lib.SwmhdError):
                cls(grid, 4, device="cuda", **kw)
    from swmhd_amd.ensemble import per_member_values
    vals, seq = per_member_values(2.5, 3, "dt")
    assert not seq and vals.tolist() == [2.5] * 3
    vals, seq = per_member_values([0.01, 0.005, 0.01], 3, "dt")
    assert seq and vals.dtype == np.float64 and vals.tolist() == [0.01, 0.005, 0.01]
    for bad in ([0.01, 0.02], np.ones(4), []):
        with pytest.raises(S._lib.SwmhdError):
            per_member_values(bad, 3, "dt")


class _HostEnsemble:
    """The clock bookkeeping of ShallowWaterEnsemble without its device tensors."""

    def __new__(cls, S, members):
        e = object.__new__(S.ShallowWaterEnsemble)
        e.members = members
        e.clock_times = np.zeros(members)
        e.clock_time, e.iteration = 0.0, 0
        e.parameters = None
        return e


def test_clock_time_raises_once_the_clocks_differ(swmhd):
    S = swmhd
    e = _HostEnsemble(S, 3)
    e._advance_clock(2, 0.01, None)                              # scalar dt on the scalar entry points
    assert e.clock_time == 2 * 0.01 and e.clock_times.tolist() == [0.02] * 3
    same = np.full(3, 0.005)
    e._advance_clock(1, same, same)                              # a per-member dt with equal entries keeps one clock
    assert e.clock_time == 0.02 + 0.005 and np.array_equal(e.clock_times, np.full(3, e.clock_time))
    dts = np.array([0.01, 0.005, 0.0025])
    t0 = e.clock_time
    e._advance_clock(4, dts, dts)
    assert np.allclose(e.clock_times, t0 + 4 * dts, rtol=0, atol=1e-15)
    with pytest.raises(S._lib.SwmhdError):
        e.clock_time
    e._advance_clock(1, 0.01, None)                              # a later uniform step does not bring them back together
    with pytest.raises(S._lib.SwmhdError):
        e.clock_time
    assert np.allclose(e.clock_times, t0 + 4 * dts + 0.01, rtol=0, atol=1e-15)
    e.clock_time = 1.5                                           # setting the clock (a restored checkpoint) sets every member's
    assert e.clock_time == 1.5 and e.clock_times.tolist() == [1.5] * 3


def test_run_refuses_a_per_member_dt(swmhd):
    S = swmhd
    e = _HostEnsemble(S, 3)
    for dt in ([0.01, 0.01, 0.005], (0.01, 0.01, 0.01), np.array([0.01, 0.02, 0.03])):
        with pytest.raises(S._lib.SwmhdError, match="per-member dt"):
            S.run(e, dt, stop_iteration=4)
    assert e.iteration == 0
