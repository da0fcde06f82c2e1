"""CPU tests (no GPU) of the ensemble tracer entry points (swmhd_ensemble_tracers_rk3_*, swmhd_ensemble_tracers_rk3_params_*):
exported and declared, every argument error is returned with its code before any HIP call (the pattern of tests/test_tracers_abi.py),
ShallowWaterEnsemble(tracers=...) refuses bad names and BoundedShallowWaterEnsemble refuses tracers, both before they touch a device."""
import ctypes
import os
import re

import pytest

FLOAT = {"f64": ctypes.c_double, "f32": ctypes.c_float}
Nx = Ny = 8
H, SY = 3, 14
SM = (Ny + 2 * H) * SY
EINVAL, EHALO, ENOTSUP = 1, 2, 3


def _bufs(sfx, n=8):
    buf = (FLOAT[sfx] * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    return buf, p, (ctypes.c_void_p * n)(*[ctypes.addressof(buf) + 8 * k for k in range(n)])     # entry 0 is p


def test_ensemble_tracer_symbols_are_exported_and_declared(swmhd):
    L = swmhd._lib.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "swmhd.h")).read()
    for sfx in ("f64", "f32"):
        for name in ("ensemble_tracers_rk3", "ensemble_tracers_rk3_params"):
            sym = f"swmhd_{name}_{sfx}"
            assert hasattr(L, sym)
            assert sym in swmhd._lib.EXPORTS
            assert re.search(rf"^int {sym}\(", header, flags=re.M), sym
            f = getattr(L, sym)
            assert f.restype is ctypes.c_int and len(f.argtypes) == 24, sym
    # the table takes the place of dt
    assert L.swmhd_ensemble_tracers_rk3_f64.argtypes[18] is ctypes.c_double
    assert L.swmhd_ensemble_tracers_rk3_params_f64.argtypes[18] is ctypes.c_void_p
    assert L.swmhd_version() == 300


def _caller(swmhd, sfx, par):
    B = swmhd._lib
    L = B.lib()
    keep = [_bufs(sfx) for _ in range(3)]
    (_b0, p, arr), (_b1, p1, alt), (_b2, p2, gn) = keep
    t = getattr(L, f"swmhd_ensemble_tracers_rk3_{'params_' if par else ''}{sfx}")

    def call(q1=p, h=p, c=arr, cnew=alt, Gn=gn, Gm=None, K=2, members=2, stride_m=SM, nx=Nx, ny=Ny, Hx=H, Hy=H, sy=SY, dx=1.0, form=1,
             params=p, store=1, flags=0):
        return t(q1, p, h, c, cnew, Gn, Gm, K, members, stride_m, nx, ny, Hx, Hy, sy, dx, 1.0, form, params if par else 0.01, 8 / 15, 0.0,
                 store, flags, None)
    return call, keep


@pytest.mark.parametrize("par", [False, True])
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_ensemble_tracer_refusals(swmhd, sfx, par):
    """Every refusal of the header's list returns its code; no call here reaches a launch (there is no device to launch on)."""
    B = swmhd._lib
    call, keep = _caller(swmhd, sfx, par)
    p, p1, p2 = keep[0][1], keep[1][1], keep[2][1]
    arr = keep[0][2]
    # what swmhd_tracers_rk3 refuses
    assert call(q1=None) == EINVAL
    assert call(h=None) == EINVAL
    assert call(c=None) == EINVAL
    assert call(Gn=None) == EINVAL
    assert call(c=(ctypes.c_void_p * 2)(p, None)) == EINVAL            # a null entry
    assert call(cnew=(ctypes.c_void_p * 2)(p1, None)) == EINVAL
    assert call(Gm=(ctypes.c_void_p * 2)(p2, None)) == EINVAL
    assert call(K=0) == EINVAL
    assert call(K=B.MAX_TRACERS + 1) == EINVAL
    assert call(nx=0) == EINVAL
    assert call(ny=0) == EINVAL
    assert call(sy=Nx + 2 * H - 1, stride_m=10 ** 6) == EINVAL             # pitch
    assert call(dx=0.0) == EINVAL
    assert call(form=2) == EINVAL
    assert call(cnew=arr) == EINVAL                                       # cnew aliases c
    assert call(cnew=(ctypes.c_void_p * 2)(p1, p)) == EINVAL            # cnew[1] aliases c[0]
    assert call(flags=8) == EINVAL                                        # unknown flags
    assert call(flags=1 << 20) == EINVAL
    assert call(cnew=None, store=0) == EINVAL                             # tendencies only: they must be stored
    assert call(cnew=None, flags=B.RK3_ANCHOR) == EINVAL                  # the anchor form is a form of the update
    assert call(flags=B.BOUNDED_X | B.WRAP_X) == EINVAL
    assert call(nx=2, flags=B.WRAP_X) == EINVAL                           # wrap with N < H
    assert call(ny=2, flags=B.WRAP_Y) == EINVAL
    # the ensemble's own
    assert call(members=0) == EINVAL
    assert call(members=-1) == EINVAL
    assert call(members=B.ENSEMBLE_MAX_MEMBERS + 1) == EINVAL
    assert call(stride_m=SM - 1) == EINVAL                                # members would overlap
    assert call(stride_m=0) == EINVAL
    if par:
        assert call(params=None) == EINVAL                                # no table
        assert call(params=None, flags=B.MARCH_KERNEL) == EINVAL
    assert call(Hx=2) == EHALO
    assert call(Hy=2, stride_m=10 ** 6) == EHALO
    for fl in (B.BOUNDED_X, B.BOUNDED_Y, B.BOUNDED_X | B.BOUNDED_Y | B.STRICT, B.MARCH_KERNEL, B.GM_IS_PREV_STATE, B.OPEN_SOUTH, B.OPEN_NORTH,
               B.OPEN_SOUTH | B.BOUNDED_Y, B.OPEN_NORTH | B.BOUNDED_Y, B.LEAVE_ROOM):
        assert call(flags=fl) == ENOTSUP, fl
    assert call(flags=B.RK3_ANCHOR | B.STRICT) == ENOTSUP
    # an argument error outranks an unsupported flag, and both outrank the halo depth, as in swmhd_tracers_rk3
    assert call(members=0, flags=B.MARCH_KERNEL) == EINVAL
    assert call(Hx=2, flags=B.LEAVE_ROOM) == ENOTSUP


def test_ensemble_constructor_refusals_before_any_device(swmhd):
    S = swmhd
    g = S.RectilinearGrid(size=(16, 16), x=(0, 1), y=(0, 1))
    bad = [("c", 3), ("c", "c"), ("c", ""), tuple(f"t{k}" for k in range(9))] + [("c", n) for n in ("u", "v", "uh", "vh", "h", "A", "s", "B_x", "B_y")]
    for names in bad:
        with pytest.raises(S._lib.SwmhdError, match="tracers"):
            S.ShallowWaterEnsemble(g, 3, tracers=names, device="cuda")


def test_bounded_ensemble_refuses_tracers_before_any_device(swmhd):
    S = swmhd
    for topo in (("Periodic", "Bounded", "Flat"), ("Bounded", "Periodic", "Flat"), ("Bounded", "Bounded", "Flat")):
        gb = S.RectilinearGrid(size=(16, 16), x=(0, 1), y=(0, 1), topology=topo)
        for names in (("c",), "dye", ("c", "d")):
            with pytest.raises(S._lib.SwmhdError, match="SWMHD_ENOTSUP"):
                S.BoundedShallowWaterEnsemble(gb, 3, tracers=names, device="cuda")
        with pytest.raises(S._lib.SwmhdError, match="tracers"):               # a bad name is a bad name there too
            S.BoundedShallowWaterEnsemble(gb, 3, tracers=("u",), device="cuda")
