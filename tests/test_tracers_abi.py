"""CPU tests (no GPU) of the passive-tracer entry points (swmhd_tracers_rk3_*): exported and declared, every argument error is
returned with its code before any HIP call, and ShallowWaterModel(tracers=...) refuses bad names and unsupported combinations before
it touches a device."""
import ctypes

import pytest

FLOAT = {"f64": ctypes.c_double, "f32": ctypes.c_float}
Nx = Ny = 8
H, SY = 3, 14


def _bufs(sfx, n=8):
    buf = (FLOAT[sfx] * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    return buf, p, (ctypes.c_void_p * n)(*[ctypes.addressof(buf) + 8 * k for k in range(n)])     # entry 0 is p


def test_tracer_symbols_are_exported(swmhd):
    L = swmhd._lib.lib()
    for sfx in ("f64", "f32"):
        assert hasattr(L, f"swmhd_tracers_rk3_{sfx}")
        assert f"swmhd_tracers_rk3_{sfx}" in swmhd._lib.EXPORTS
    assert swmhd._lib.MAX_TRACERS == 8
    import os, re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "swmhd.h")).read()
    assert re.search(r"^#define SWMHD_MAX_TRACERS 8$", header, flags=re.M)
    assert L.swmhd_version() == 300


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_tracer_refusals(swmhd, sfx):
    B = swmhd._lib
    L = B.lib()
    _b0, p, arr = _bufs(sfx)
    _b1, p1, alt = _bufs(sfx)
    _b2, p2, gn = _bufs(sfx)
    t = getattr(L, f"swmhd_tracers_rk3_{sfx}")

    def call(q1=p, h=p, c=arr, cnew=alt, Gn=gn, Gm=None, K=2, nx=Nx, ny=Ny, Hx=H, Hy=H, sy=SY, dx=1.0, form=1, store=1, j0=0, j1=Ny, flags=0):
        return t(q1, p, h, c, cnew, Gn, Gm, K, nx, ny, Hx, Hy, sy, dx, 1.0, form, 0.01, 8 / 15, 0.0, store, j0, j1, flags, None)
    EINVAL, EHALO, ENOTSUP = 1, 2, 3
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
    assert call(sy=Nx + 2 * H - 1) == EINVAL                              # pitch
    assert call(dx=0.0) == EINVAL
    assert call(j0=-1) == EINVAL
    assert call(j1=Ny + 1) == EINVAL
    assert call(j0=5, j1=4) == EINVAL
    assert call(form=2) == EINVAL
    assert call(cnew=arr) == EINVAL                                       # cnew aliases c
    assert call(cnew=(ctypes.c_void_p * 2)(p1, p)) == EINVAL            # cnew[1] aliases c[0]
    assert call(flags=8) == EINVAL                                        # unknown flags
    assert call(flags=1 << 20) == EINVAL
    assert call(cnew=None, store=0) == EINVAL                             # tendencies only: they must be stored
    assert call(flags=B.BOUNDED_X | B.WRAP_X) == EINVAL
    assert call(nx=2, sy=SY, flags=B.WRAP_X) == EINVAL                    # wrap with N < H
    assert call(ny=2, j1=2, flags=B.WRAP_Y) == EINVAL
    assert call(Hx=2) == EHALO
    assert call(Hy=2) == EHALO
    for fl in (B.MARCH_KERNEL, B.GM_IS_PREV_STATE, B.OPEN_SOUTH | B.BOUNDED_Y, B.OPEN_NORTH | B.BOUNDED_Y, B.LEAVE_ROOM):
        assert call(flags=fl) == ENOTSUP, fl
    assert call(flags=B.RK3_ANCHOR | B.STRICT) == ENOTSUP
    assert call(flags=B.RK3_ANCHOR | B.BOUNDED_X) == ENOTSUP
    assert call(flags=B.RK3_ANCHOR | B.BOUNDED_Y) == ENOTSUP
    # accepted, and nothing to enqueue: an empty row range, with every accepted flag
    for fl in (0, B.STRICT, B.TILE_KERNEL, B.WRAP_X | B.WRAP_Y, B.BOUNDED_X | B.BOUNDED_Y | B.STRICT, B.RK3_ANCHOR | B.WRAP_X | B.WRAP_Y):
        assert call(j0=3, j1=3, flags=fl) == 0, fl
    assert call(j0=3, j1=3, K=B.MAX_TRACERS) == 0
    assert call(j0=3, j1=3, cnew=None) == 0                               # tendencies only


def test_constructor_refusals_before_any_device(swmhd):
    S = swmhd
    g = S.RectilinearGrid(size=(16, 16), x=(0, 1), y=(0, 1))
    bad = [("c", 3), ("c", "c"), ("c", ""), tuple(f"t{k}" for k in range(9))] + [("c", n) for n in ("u", "v", "uh", "vh", "h", "A", "s", "B_x", "B_y")]
    for names in bad:
        with pytest.raises(S._lib.SwmhdError, match="tracers"):
            S.ShallowWaterModel(g, tracers=names, device="cuda")
    with pytest.raises(S._lib.SwmhdError, match="SWMHD_ENOTSUP"):
        S.ShallowWaterModel(g, tracers=("c",), fused=False)
    with pytest.raises(S._lib.SwmhdError, match="SWMHD_ENOTSUP"):
        S.ShallowWaterModel(g, tracers=("c",), ring=ctypes.c_void_p(1))
    with pytest.raises(S._lib.SwmhdError, match="SWMHD_ENOTSUP"):
        S.ShallowWaterModel(S.RectilinearGrid(size=(16, 8), x=(0, 1), y=(0, 1), j_offset=0, Ny_global=16), tracers=("c",),
                            decomp=S.SlabDecomposition(16, 2, 0))
    from swmhd_amd.model import tracer_names
    assert tracer_names(("c", "d")) == ("c", "d") and tracer_names("dye") == ("dye",) and tracer_names(()) == ()
    assert len(tracer_names(tuple(f"t{k}" for k in range(8)))) == 8
