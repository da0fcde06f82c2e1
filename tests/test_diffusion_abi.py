"""CPU tests (no GPU) of the ScalarDiffusivity closure: the entry points of include/swmhd_diffusion.h are exported and declared, every
argument error comes back with its code before any HIP call, and the Python classes refuse what they do not support before anything
is allocated."""
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


def test_diffusion_symbols_are_exported(swmhd):
    B = swmhd._lib
    L = B.lib()
    assert B.DIFFUSION_EXPORTS == [f"swmhd_{n}_{s}" for s in ("f64", "f32") for n in ("diffusion_rk3", "ensemble_diffusion_rk3")]
    header = open(os.path.join(ROOT, "include", "swmhd_diffusion.h")).read()
    for name in B.DIFFUSION_EXPORTS:
        assert hasattr(L, name)
        assert re.search(rf"^int {name}\(", header, flags=re.M), name
    assert sorted(re.findall(r"^int (swmhd_\w+)\(", header, flags=re.M)) == sorted(B.DIFFUSION_EXPORTS)
    assert '#include "swmhd_diffusion.h"' in open(os.path.join(ROOT, "include", "swmhd.h")).read()
    assert re.search(r"^#define SWMHD_DIFFUSION_MAX_FIELDS 11$", header, flags=re.M) and B.DIFFUSION_MAX_FIELDS == 11 == 3 + B.MAX_TRACERS
    assert re.search(rf"^#define SWMHD_DIFFUSION_TILE_ROWS {B.DIFFUSION_TILE_ROWS}$", header, flags=re.M)
    assert L.swmhd_version() == 300          # symbols added, none changed
    assert not set(B.DIFFUSION_EXPORTS) & set(B.EXPORTS)


@pytest.mark.parametrize("ens", [False, True], ids=["single", "ensemble"])
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_diffusion_return_codes(swmhd, sfx, ens):
    B = swmhd._lib
    L = B.lib()
    _o, old = _bufs(sfx)
    _n, new = _bufs(sfx)
    _a, acc = _bufs(sfx)
    ft = FLOAT[sfx]
    good = (ft * 11)(*[0.01] * 11)
    fn = getattr(L, f"swmhd_{'ensemble_' if ens else ''}diffusion_rk3_{sfx}")
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
        assert call(coef=coefs(0.01, -1e-9)) == EINVAL
        assert call(coef=coefs(float("nan"), 0.01)) == EINVAL
        assert call(coef=coefs(0.01, float("inf"))) == EINVAL
    # known flags this family does not take
    for fl in (B.BOUNDED_X, B.BOUNDED_Y, B.BOUNDED_X | B.BOUNDED_Y, B.MARCH_KERNEL, B.TILE_KERNEL, B.GM_IS_PREV_STATE, B.OPEN_SOUTH,
               B.OPEN_NORTH | B.BOUNDED_Y, B.LEAVE_ROOM):
        assert call(flags=fl) == ENOTSUP, fl
    # a halo of depth >= 1 unless that direction is wrapped
    assert call(Hx=0, sy=SY) == EHALO
    assert call(Hy=0) == EHALO
    assert call(Hx=0, flags=B.WRAP_Y) == EHALO
    assert call(Hy=0, flags=B.WRAP_X) == EHALO
    # accepted, nothing to enqueue: an empty row range with every accepted flag, the widest list, no acc, null entries of acc
    for fl in (0, B.STRICT, B.WRAP_X | B.WRAP_Y, B.STRICT | B.WRAP_X, B.RK3_ANCHOR | B.WRAP_X | B.WRAP_Y, B.RK3_ANCHOR | B.STRICT):
        assert call(j0=3, j1=3, flags=fl) == 0, fl
    assert call(j0=3, j1=3, Hx=0, Hy=0, flags=B.WRAP_X | B.WRAP_Y) == 0
    assert call(j0=0, j1=0, n=B.DIFFUSION_MAX_FIELDS) == 0
    assert call(j0=Ny, j1=Ny, acc=None) == 0
    assert call(j0=3, j1=3, acc=(V * 2)(None, acc[1])) == 0
    if not ens:   # coefficients that are all 0: nothing to enqueue for any rows
        assert call(coef=coefs(0.0, 0.0)) == 0
        assert call(coef=coefs(-0.0, 0.0), acc=None) == 0


def test_scalar_diffusivity_values(swmhd):
    S = swmhd
    E = S._lib.SwmhdError
    names = ("u", "v", "h", "A")
    c = S.ScalarDiffusivity(nu=1e-3, kappa=2e-3)
    assert c.coefficients(names, ("c", "d")) == {"u": 1e-3, "v": 1e-3, "h": 0.0, "A": 2e-3, "c": 2e-3, "d": 2e-3}
    c = S.ScalarDiffusivity(kappa={"A": 3e-3, "d": 1e-3})
    assert c.coefficients(names, ("c", "d")) == {"u": 0.0, "v": 0.0, "h": 0.0, "A": 3e-3, "c": 0.0, "d": 1e-3}
    assert S.ScalarDiffusivity().coefficients(names) == {"u": 0.0, "v": 0.0, "h": 0.0, "A": 0.0}
    for bad in ({"B": 1e-3}, {"u": 1e-3}, {"h": 1e-3}, {"c": 1e-3}):
        with pytest.raises(E, match="kappa names"):
            S.ScalarDiffusivity(kappa=bad).coefficients(names, ("d",))
    for kw in (dict(nu=-1.0), dict(nu=float("nan")), dict(kappa=float("inf")), dict(kappa={"A": -1e-3}), dict(kappa={3: 1e-3}),
               dict(nu=[[1.0]])):
        with pytest.raises(E, match="ScalarDiffusivity"):
            S.ScalarDiffusivity(**kw)
    g = S.RectilinearGrid(size=(16, 8), x=(0, 1.6), y=(0, 0.4))
    c = S.ScalarDiffusivity(nu=1e-3, kappa={"A": 4e-3})
    assert c.max_stable_dt(g) == pytest.approx(2.51 / (4 * 4e-3 * (1 / 0.1 ** 2 + 1 / 0.05 ** 2)), rel=1e-12)
    assert S.ScalarDiffusivity().max_stable_dt(g) == float("inf")
    m = S.ScalarDiffusivity(nu=[1e-3, 2e-3], kappa={"A": [0.0, 5e-3], "c": 1e-3}).for_member(1)
    assert (m.nu, m.kappa) == (2e-3, {"A": 5e-3, "c": 1e-3})
    assert S.ScalarDiffusivity(nu=[1e-3, 2e-3]).max_stable_dt(g) == S.ScalarDiffusivity(nu=2e-3).max_stable_dt(g)


def test_constructor_refusals_before_any_device(swmhd, monkeypatch):
    S = swmhd
    E = S._lib.SwmhdError
    import swmhd_amd.ensemble as ens_mod
    import swmhd_amd.model as model_mod

    def no_allocation(*a, **k):
        raise AssertionError("allocated before the refusal")
    monkeypatch.setattr(model_mod, "Field", no_allocation)
    monkeypatch.setattr(ens_mod.torch, "zeros", no_allocation)
    g = S.RectilinearGrid(size=(16, 16), x=(0, 1), y=(0, 1))
    c = S.ScalarDiffusivity(nu=1e-3, kappa=1e-3)
    for topo in (("Bounded", "Periodic", "Flat"), ("Periodic", "Bounded", "Flat"), ("Bounded", "Bounded", "Flat")):
        gb = S.RectilinearGrid(size=(16, 16), x=(0, 1), y=(0, 1), topology=topo)
        with pytest.raises(E, match="SWMHD_ENOTSUP"):
            S.ShallowWaterModel(gb, closure=c)
        with pytest.raises(E, match="SWMHD_ENOTSUP"):
            S.BoundedShallowWaterEnsemble(gb, 2, closure=c)
        with pytest.raises(E, match="SWMHD_ENOTSUP"):
            S.ShallowWaterEnsemble(gb, 2, closure=c)
    with pytest.raises(E, match="SWMHD_ENOTSUP"):
        S.ShallowWaterModel(g, closure=c, fused=False)
    with pytest.raises(E, match="SWMHD_ENOTSUP"):
        S.ShallowWaterModel(g, closure=c, ring=ctypes.c_void_p(1))
    with pytest.raises(E, match="SWMHD_ENOTSUP"):
        S.ShallowWaterModel(S.RectilinearGrid(size=(16, 8), x=(0, 1), y=(0, 1), j_offset=0, Ny_global=16), closure=c,
                            decomp=S.SlabDecomposition(16, 2, 0))
    for cls, args in ((S.ShallowWaterModel, (g,)), (S.ShallowWaterEnsemble, (g, 2))):
        with pytest.raises(E, match="SWMHD_ENOTSUP.*conservative viscous stress"):
            cls(*args, formulation=S.ConservativeFormulation, closure=c)
        with pytest.raises(E, match="kappa names"):
            cls(*args, closure=S.ScalarDiffusivity(kappa={"c": 1e-3}))
        with pytest.raises(E, match="kappa names"):
            cls(*args, tracers=("d",), closure=S.ScalarDiffusivity(kappa={"A": 1e-3, "c": 1e-3}))
        with pytest.raises(E, match="closure"):
            cls(*args, closure=1e-3)
    with pytest.raises(E, match="SWMHD_ENOTSUP"):
        S.ShallowWaterEnsemble(g, 2, formulation=S.ConservativeFormulation, closure=S.ScalarDiffusivity(nu=[0.0, 1e-3]))
    with pytest.raises(E, match="closure coefficient of A"):
        S.ShallowWaterEnsemble(g, 3, closure=S.ScalarDiffusivity(kappa=[1e-3, 2e-3]))
