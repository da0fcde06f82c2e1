"""CPU tests (no GPU) of the ScalarBiharmonicDiffusivity closure's C ABI: the entry points of include/swmhd_biharmonic.h are exported and
declared, every argument error comes back with its code, in the order of the diffusion calls and before any HIP call, a halo of 1 is
refused without the WRAP flag of its direction, and the Makefile builds the kernel twice."""
import ctypes
import os
import re

import pytest

FLOAT = {"f64": ctypes.c_double, "f32": ctypes.c_float}
Nx = Ny = 8
H, SY = 3, 14
EINVAL, EHALO, ENOTSUP = 1, 2, 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bufs(sfx, n=11):
    buf = (FLOAT[sfx] * 64)()
    return buf, (ctypes.c_void_p * n)(*[ctypes.addressof(buf) + 8 * k for k in range(n)])


def test_biharmonic_symbols_are_exported(swmhd):
    B = swmhd._lib
    L = B.lib()
    assert B.BIHARMONIC_EXPORTS == [f"swmhd_{n}_{s}" for s in ("f64", "f32") for n in ("biharmonic_rk3", "ensemble_biharmonic_rk3")]
    header = open(os.path.join(ROOT, "include", "swmhd_biharmonic.h")).read()
    for name in B.BIHARMONIC_EXPORTS:
        assert hasattr(L, name)
        assert re.search(rf"^int {name}\(", header, flags=re.M), name
    assert sorted(re.findall(r"^int (swmhd_\w+)\(", header, flags=re.M)) == sorted(B.BIHARMONIC_EXPORTS)
    assert '#include "swmhd_biharmonic.h"' in open(os.path.join(ROOT, "include", "swmhd.h")).read()
    assert L.swmhd_version() == 300          # symbols added, none changed
    others = B.EXPORTS + B.ZONAL_EXPORTS + B.DERIVED_EXPORTS + B.SPECTRA_EXPORTS + B.SPECTRA2D_EXPORTS + B.DIFFUSION_EXPORTS + B.CORIOLIS_EXPORTS
    assert not set(B.BIHARMONIC_EXPORTS) & set(others)
    # the argument lists are those of the four diffusion calls
    diffusion = open(os.path.join(ROOT, "include", "swmhd_diffusion.h")).read()

    def prototypes(text, word):
        protos = re.findall(r"^int swmhd_\w+\([^;]*;", text, flags=re.M)
        return sorted(re.sub(r"\s+", " ", p.replace(word, "X")) for p in protos)
    assert prototypes(header, "biharmonic") == prototypes(diffusion, "diffusion")
    for name in B.BIHARMONIC_EXPORTS:
        assert getattr(L, name).argtypes == getattr(L, name.replace("biharmonic", "diffusion")).argtypes


def test_makefile_builds_the_kernel_twice():
    mk = open(os.path.join(ROOT, "swmhd_amd", "csrc", "Makefile")).read()
    hdrs = re.search(r"^HDRS\s*:=(.*)$", mk, flags=re.M).group(1)
    assert "../../include/swmhd_biharmonic.h" in hdrs.split()
    objs = " ".join(re.findall(r"^OBJS\s*[:+]=(.*)$", mk, flags=re.M)).split()
    assert "biharmonic_fast.o" in objs and "biharmonic_strict.o" in objs
    fast = re.search(r"^(.*): %_fast\.o: %\.hip", mk, flags=re.M).group(1).split()
    strict = re.search(r"^(.*): %_strict\.o: %\.hip", mk, flags=re.M).group(1).split()
    assert "biharmonic_fast.o" in fast and "diffusion_fast.o" in fast and "coriolis_fast.o" in fast
    assert "biharmonic_strict.o" in strict and "diffusion_strict.o" in strict and "coriolis_strict.o" in strict
    assert os.path.exists(os.path.join(ROOT, "swmhd_amd", "csrc", "biharmonic.hip"))


@pytest.mark.parametrize("ens", [False, True], ids=["single", "ensemble"])
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_biharmonic_return_codes(swmhd, sfx, ens):
    """No device is touched: every call here returns before the first HIP call (an error, an empty row range, or coefficients that are
    all 0).  Order: where a call has an error of one class and one of a later class, the earlier one comes back."""
    B = swmhd._lib
    L = B.lib()
    _o, old = _bufs(sfx)
    _n, new = _bufs(sfx)
    _a, acc = _bufs(sfx)
    ft = FLOAT[sfx]
    good = (ft * 11)(*[1e-6] * 11)
    fn = getattr(L, f"swmhd_{'ensemble_' if ens else ''}biharmonic_rk3_{sfx}")
    V = ctypes.c_void_p

    def call(old=old, new=new, acc=acc, coef=good, n=2, members=2, stride_m=(Ny + 2 * H) * SY, nx=Nx, ny=Ny, Hx=H, Hy=H, sy=SY, dx=1.0,
             dy=1.0, params=None, a=0.01, w=1.0, j0=0, j1=Ny, flags=0):
        coef = ctypes.cast(coef, V) if coef is not None else None
        if ens:
            return fn(old, new, acc, coef, n, members, stride_m, nx, ny, Hx, Hy, sy, dx, dy, params, a, w, j0, j1, flags, None)
        return fn(old, new, acc, coef, n, nx, ny, Hx, Hy, sy, dx, dy, a, w, j0, j1, flags, None)

    def coefs(*v):
        return (ft * len(v))(*v)
    # null pointers
    assert call(old=None) == EINVAL
    assert call(new=None) == EINVAL
    assert call(coef=None) == EINVAL
    assert call(old=(V * 2)(old[0], None)) == EINVAL
    assert call(new=(V * 2)(new[0], None)) == EINVAL
    # nfields
    assert call(n=0) == EINVAL
    assert call(n=B.DIFFUSION_MAX_FIELDS + 1) == EINVAL
    # extents, pitch, spacing, rows
    assert call(nx=0) == EINVAL
    assert call(ny=0) == EINVAL
    assert call(Hx=-1) == EINVAL
    assert call(sy=Nx + 2 * H - 1) == EINVAL
    assert call(dx=0.0) == EINVAL
    assert call(dy=-1.0) == EINVAL
    assert call(dx=float("nan")) == EINVAL
    assert call(j0=-1) == EINVAL
    assert call(j1=Ny + 1) == EINVAL
    assert call(j0=5, j1=4) == EINVAL
    # aliasing: new or acc on any old, an output twice
    assert call(new=old) == EINVAL
    assert call(new=(V * 2)(new[0], old[0])) == EINVAL
    assert call(acc=old) == EINVAL
    assert call(acc=(V * 2)(acc[0], old[0])) == EINVAL
    assert call(acc=new) == EINVAL
    assert call(new=(V * 2)(new[0], new[0])) == EINVAL
    # unknown flags
    assert call(flags=8) == EINVAL
    assert call(flags=1 << 20) == EINVAL
    # a or w not finite
    assert call(a=float("inf")) == EINVAL
    assert call(w=float("nan")) == EINVAL
    if ens:
        assert call(members=0) == EINVAL
        assert call(members=B.ENSEMBLE_MAX_MEMBERS + 1) == EINVAL
        assert call(stride_m=(Ny + 2 * H) * SY - 1) == EINVAL
    else:   # host coefficients: finite and not negative
        assert call(coef=coefs(1e-6, -1e-9)) == EINVAL
        assert call(coef=coefs(float("nan"), 1e-6)) == EINVAL
        assert call(coef=coefs(1e-6, float("inf"))) == EINVAL
    # known flags this family does not take
    for fl in (B.BOUNDED_X, B.BOUNDED_Y, B.BOUNDED_X | B.BOUNDED_Y, B.MARCH_KERNEL, B.TILE_KERNEL, B.GM_IS_PREV_STATE, B.OPEN_SOUTH,
               B.OPEN_NORTH | B.BOUNDED_Y, B.LEAVE_ROOM):
        assert call(flags=fl) == ENOTSUP, fl
    # a halo of depth >= 2 unless that direction is wrapped
    for h in (0, 1):
        assert call(Hx=h, sy=SY) == EHALO
        assert call(Hy=h) == EHALO
        assert call(Hx=h, flags=B.WRAP_Y) == EHALO
        assert call(Hy=h, flags=B.WRAP_X) == EHALO
        assert call(Hx=h, Hy=h, j0=3, j1=3, flags=B.WRAP_X | B.WRAP_Y) == 0
        assert call(Hx=h, j0=3, j1=3, flags=B.WRAP_X) == 0
        assert call(Hy=h, j0=3, j1=3, flags=B.WRAP_Y) == 0
    assert call(Hx=2, Hy=2, j0=3, j1=3) == 0
    # the order: EINVAL before ENOTSUP before EHALO; the ensemble's own errors before everything
    assert call(flags=B.BOUNDED_X, a=float("inf")) == EINVAL
    assert call(flags=B.BOUNDED_X | 8) == EINVAL
    assert call(flags=B.BOUNDED_X, Hx=1) == ENOTSUP
    assert call(Hx=1, new=old) == EINVAL
    assert call(Hx=1, j0=5, j1=4) == EINVAL
    if ens:
        assert call(members=0, flags=B.BOUNDED_X, Hx=1) == EINVAL
    else:
        assert call(coef=coefs(-1.0, 1e-6), flags=B.LEAVE_ROOM) == EINVAL
        assert call(coef=coefs(0.0, 0.0), Hx=1) == EHALO          # the halo check precedes the look at what there is to do
    # accepted, nothing to enqueue: an empty row range with every accepted flag, the widest list, no acc, null entries of acc
    for fl in (0, B.STRICT, B.WRAP_X | B.WRAP_Y, B.STRICT | B.WRAP_X, B.RK3_ANCHOR | B.WRAP_X | B.WRAP_Y, B.RK3_ANCHOR | B.STRICT):
        assert call(j0=3, j1=3, flags=fl) == 0, fl
    assert call(j0=0, j1=0, n=B.DIFFUSION_MAX_FIELDS) == 0
    assert call(j0=Ny, j1=Ny, acc=None) == 0
    assert call(j0=3, j1=3, acc=(V * 2)(None, acc[1])) == 0
    if not ens:   # coefficients that are all 0: nothing to enqueue for any rows
        assert call(coef=coefs(0.0, 0.0)) == 0
        assert call(coef=coefs(-0.0, 0.0), acc=None) == 0
        assert call(coef=coefs(0.0, 0.0), Hx=1, Hy=1, flags=B.WRAP_X | B.WRAP_Y) == 0


@pytest.mark.parametrize("ens", [False, True], ids=["single", "ensemble"])
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_diffusion_codes_are_what_they_were(swmhd, sfx, ens):
    """The Laplacian calls share their checks with the new ones: a halo of 1 is still enough for them, 0 still is not."""
    B = swmhd._lib
    L = B.lib()
    _o, old = _bufs(sfx)
    _n, new = _bufs(sfx)
    good = (FLOAT[sfx] * 11)(*[1e-3] * 11)
    fn = getattr(L, f"swmhd_{'ensemble_' if ens else ''}diffusion_rk3_{sfx}")

    def call(Hx=H, Hy=H, flags=0, j0=3, j1=3):
        head = (old, new, None, ctypes.cast(good, ctypes.c_void_p), 2)
        tail = (Nx, Ny, Hx, Hy, SY, 1.0, 1.0) + ((None,) if ens else ()) + (0.01, 1.0, j0, j1, flags, None)
        return fn(*head, *((2, (Ny + 2 * H) * SY) if ens else ()), *tail)
    assert call(Hx=1, Hy=1) == 0
    assert call(Hx=0) == EHALO and call(Hy=0) == EHALO
    assert call(Hx=0, Hy=0, flags=B.WRAP_X | B.WRAP_Y) == 0
