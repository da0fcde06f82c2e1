"""CPU tests (no GPU) of the Relaxation forcing: the entry points of include/swmhd_relaxation.h are exported and declared, every
argument error comes back with its code, in the documented order, before any HIP call, and the Python classes refuse what they do not
support before anything is allocated."""
import ctypes
import os
import re

import numpy as np
import pytest

FLOAT = {"f64": ctypes.c_double, "f32": ctypes.c_float}
Nx = Ny = 8
H, SY = 3, 14
EINVAL, EHALO, ENOTSUP = 1, 2, 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEMBER = (Ny + 2 * H) * SY


def _bufs(sfx, n=12):
    buf = (FLOAT[sfx] * 64)()
    return buf, (ctypes.c_void_p * n)(*[ctypes.addressof(buf) + 8 * k for k in range(n)])


def test_relaxation_symbols_are_exported(swmhd):
    B = swmhd._lib
    L = B.lib()
    assert B.RELAXATION_EXPORTS == [f"swmhd_{n}_{s}" for s in ("f64", "f32") for n in ("relaxation_rk3", "ensemble_relaxation_rk3")]
    header = open(os.path.join(ROOT, "include", "swmhd_relaxation.h")).read()
    for name in B.RELAXATION_EXPORTS:
        assert hasattr(L, name)
        assert re.search(rf"^int {name}\(", header, flags=re.M), name
    assert sorted(re.findall(r"^int (swmhd_\w+)\(", header, flags=re.M)) == sorted(B.RELAXATION_EXPORTS)
    assert '#include "swmhd_relaxation.h"' in open(os.path.join(ROOT, "include", "swmhd.h")).read()
    assert re.search(r"^#define SWMHD_RELAXATION_MAX_FIELDS 12$", header, flags=re.M) and B.RELAXATION_MAX_FIELDS == 12 == 4 + B.MAX_TRACERS
    assert re.search(rf"^#define SWMHD_RELAXATION_TILE_ROWS {B.RELAXATION_TILE_ROWS}$", header, flags=re.M)
    assert L.swmhd_version() == 300          # symbols added, none changed
    others = (B.EXPORTS, B.ZONAL_EXPORTS, B.DERIVED_EXPORTS, B.SPECTRA_EXPORTS, B.SPECTRA2D_EXPORTS, B.DIFFUSION_EXPORTS,
              B.BIHARMONIC_EXPORTS, B.CORIOLIS_EXPORTS)
    assert not any(set(B.RELAXATION_EXPORTS) & set(o) for o in others)
    # the header states the formula, the bytes, the checks and their order
    for words in ("p        = rate_k mask_k[i,j]", "Bytes per cell, field and stage (fp64)", "Checks, in this order", "4 eps |a| S"):
        assert words in header, words


@pytest.mark.parametrize("ens", [False, True], ids=["single", "ensemble"])
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_relaxation_return_codes(swmhd, sfx, ens):
    B = swmhd._lib
    L = B.lib()
    _o, old = _bufs(sfx)
    _n, new = _bufs(sfx)
    _a, acc = _bufs(sfx)
    _m, mask = _bufs(sfx)
    _t, target = _bufs(sfx)
    ft = FLOAT[sfx]
    good = (ft * 12)(*[0.01] * 12)
    zeros = (ft * 12)(*[0.0] * 12)
    fn = getattr(L, f"swmhd_{'ensemble_' if ens else ''}relaxation_rk3_{sfx}")
    V = ctypes.c_void_p

    def call(old=old, new=new, acc=acc, mask=mask, target=target, rate=good, tval=zeros, n=2, members=2, stride_m=MEMBER, mask_sm=0,
             target_sm=MEMBER, nx=Nx, ny=Ny, Hx=H, Hy=H, sy=SY, params=None, a=0.01, w=1.0, j0=0, j1=Ny, flags=0):
        rate = ctypes.cast(rate, V) if rate is not None else None
        tval = ctypes.cast(tval, V) if tval is not None else None
        if ens:
            return fn(old, new, acc, mask, target, rate, tval, n, members, stride_m, mask_sm, target_sm, nx, ny, Hx, Hy, sy, params, a, w,
                      j0, j1, flags, None)
        return fn(old, new, acc, mask, target, rate, tval, n, nx, ny, Hx, Hy, sy, a, w, j0, j1, flags, None)

    def vals(*v):
        return (ft * len(v))(*v)
    # null pointers
    assert call(old=None) == EINVAL
    assert call(new=None) == EINVAL
    assert call(rate=None) == EINVAL
    assert call(tval=None) == EINVAL
    # nfields
    assert call(n=0) == EINVAL
    assert call(n=B.RELAXATION_MAX_FIELDS + 1) == EINVAL
    # extents, pitch, rows
    assert call(nx=0) == EINVAL
    assert call(ny=0) == EINVAL
    assert call(Hx=-1) == EINVAL
    assert call(Hy=-1) == EINVAL
    assert call(sy=Nx + 2 * H - 1) == EINVAL
    assert call(j0=-1) == EINVAL
    assert call(j1=Ny + 1) == EINVAL
    assert call(j0=5, j1=4) == EINVAL
    # unknown flags; Bounded and wrapped at once
    assert call(flags=8) == EINVAL
    assert call(flags=1 << 20) == EINVAL
    assert call(flags=B.BOUNDED_X | B.WRAP_X) == EINVAL
    assert call(flags=B.BOUNDED_Y | B.WRAP_Y | B.STRICT) == EINVAL
    # null entries of old and new
    assert call(old=(V * 2)(old[0], None)) == EINVAL
    assert call(new=(V * 2)(new[0], None)) == EINVAL
    # aliasing: an output on any input (old, mask, target), an output twice
    assert call(new=old) == EINVAL
    assert call(new=(V * 2)(new[0], old[0])) == EINVAL
    assert call(new=(V * 2)(new[0], mask[0])) == EINVAL
    assert call(new=(V * 2)(target[1], new[1])) == EINVAL
    assert call(acc=old) == EINVAL
    assert call(acc=(V * 2)(acc[0], old[0])) == EINVAL
    assert call(acc=(V * 2)(mask[1], acc[1])) == EINVAL
    assert call(acc=(V * 2)(acc[0], target[0])) == EINVAL
    assert call(acc=new) == EINVAL
    assert call(new=(V * 2)(new[0], new[0])) == EINVAL
    assert call(acc=(V * 2)(acc[0], acc[0])) == EINVAL
    assert call(acc=(V * 2)(new[1], acc[1])) == EINVAL
    # a or w not finite
    assert call(a=float("inf")) == EINVAL
    assert call(w=float("nan")) == EINVAL
    if ens:
        assert call(members=0) == EINVAL
        assert call(members=B.ENSEMBLE_MAX_MEMBERS + 1) == EINVAL
        assert call(stride_m=MEMBER - 1) == EINVAL
        assert call(stride_m=0) == EINVAL
        # a member stride of the masks or the targets: 0 (shared) or a whole parent
        assert call(mask_sm=MEMBER - 1) == EINVAL
        assert call(mask_sm=1) == EINVAL
        assert call(target_sm=-MEMBER) == EINVAL
        assert call(target_sm=MEMBER - 1) == EINVAL
        # the ensemble's own errors come first: before a null pointer, before an unsupported flag
        assert call(members=0, flags=B.TILE_KERNEL) == EINVAL
        # the device tables are not looked at
        assert call(rate=vals(-1.0, float("nan")), tval=vals(float("inf"), 0.0), j0=3, j1=3) == 0
    else:   # host values: rates finite and not negative, scalar targets finite
        assert call(rate=vals(0.01, -1e-9)) == EINVAL
        assert call(rate=vals(float("nan"), 0.01)) == EINVAL
        assert call(rate=vals(0.01, float("inf"))) == EINVAL
        assert call(tval=vals(float("nan"), 0.0)) == EINVAL
        assert call(tval=vals(0.0, float("-inf"))) == EINVAL
    # known flags this family does not take; an argument error beside one of them comes first
    for fl in (B.MARCH_KERNEL, B.TILE_KERNEL, B.GM_IS_PREV_STATE, B.OPEN_SOUTH, B.OPEN_NORTH | B.BOUNDED_Y, B.LEAVE_ROOM):
        assert call(flags=fl) == ENOTSUP, fl
        assert call(flags=fl, n=0) == EINVAL
        assert call(flags=fl, a=float("nan")) == EINVAL
        assert call(flags=fl, j0=3, j1=3) == ENOTSUP          # before "nothing to enqueue"
    # there is no SWMHD_EHALO: no halo at all is accepted, wrapped or not
    assert call(j0=3, j1=3, Hx=0, Hy=0, sy=Nx) == 0
    assert call(j0=3, j1=3, Hx=0, Hy=0, sy=Nx, flags=B.BOUNDED_X | B.BOUNDED_Y) == 0
    # accepted, nothing to enqueue: an empty row range with every accepted flag, the widest list, no acc / mask / target, null entries
    for fl in (0, B.STRICT, B.WRAP_X | B.WRAP_Y, B.STRICT | B.WRAP_X, B.RK3_ANCHOR | B.WRAP_X | B.WRAP_Y, B.RK3_ANCHOR | B.STRICT,
               B.BOUNDED_X, B.BOUNDED_Y | B.WRAP_X, B.BOUNDED_X | B.BOUNDED_Y | B.STRICT):
        assert call(j0=3, j1=3, flags=fl) == 0, fl
    assert call(j0=0, j1=0, n=B.RELAXATION_MAX_FIELDS) == 0
    assert call(j0=Ny, j1=Ny, acc=None, mask=None, target=None) == 0
    assert call(j0=3, j1=3, acc=(V * 2)(None, acc[1]), mask=(V * 2)(mask[0], None), target=(V * 2)(None, None)) == 0
    assert call(j0=3, j1=3, mask=(V * 2)(mask[0], mask[0]), target=(V * 2)(mask[0], target[0])) == 0      # inputs may be shared
    if not ens:   # rates that are all 0: nothing to enqueue for any rows
        assert call(rate=vals(0.0, 0.0)) == 0
        assert call(rate=vals(-0.0, 0.0), acc=None) == 0


def test_relaxation_values(swmhd):
    S = swmhd
    E = S._lib.SwmhdError
    g = S.RectilinearGrid(size=(16, 8), x=(0, 1.6), y=(0, 0.4))
    r = S.Relaxation(0.5)
    assert (r.rate, r.mask, r.target) == (0.5, None, 0.0) and not r.per_member
    assert r.max_stable_dt() == pytest.approx(2.51 / 0.5, rel=1e-15)
    assert S.Relaxation(0.0).max_stable_dt() == float("inf")
    m = np.linspace(0, 2, 16 * 8).reshape(8, 16)
    assert S.Relaxation(0.5, mask=m).max_stable_dt() == pytest.approx(2.51 / (0.5 * 2.0), rel=1e-15)
    assert S.Relaxation([0.1, 0.4], mask=m).max_stable_dt() == pytest.approx(2.51 / (0.4 * 2.0), rel=1e-15)
    sponge = lambda x, y: 3.0 * np.exp(-(y / 0.1) ** 2) + 0 * x
    rs = S.Relaxation(0.5, mask=sponge)
    assert rs.max_stable_dt(g, (S.Center, S.Face)) == pytest.approx(2.51 / 1.5, rel=1e-15)      # a face node stands at y = 0
    with pytest.raises(E, match="needs the grid"):
        rs.max_stable_dt()
    # callables: the grid's own nodes at the location, x (1, Nx) and y (Ny, 1)
    seen = {}

    def target(x, y):
        seen["shapes"] = (x.shape, y.shape)
        return x + 10 * y
    mask_h, t_h = S.Relaxation(0.5, mask=sponge, target=target).evaluate(g, (S.Face, S.Center), "u")
    assert seen["shapes"] == ((1, 16), (8, 1)) and mask_h.shape == t_h.shape == (8, 16)
    assert np.array_equal(t_h, g.xf[3:19][None, :] + 10 * g.yc[3:11][:, None])
    assert np.array_equal(S.Relaxation(0.5, target=target).evaluate(g, (S.Center, S.Face), "v")[1], g.xc[3:19][None, :] + 10 * g.yf[3:11][:, None])
    assert S.Relaxation(0.5, target=lambda x, y: 2.0).evaluate(g, (S.Center, S.Center), "h")[1].shape == (8, 16)      # broadcast
    for kw in (dict(rate=-1.0), dict(rate=float("nan")), dict(rate=float("inf")), dict(rate=[[1.0]]), dict(rate=0.1, target=float("nan")),
               dict(rate=0.1, mask=np.full((8, 16), np.inf)), dict(rate=0.1, mask=1.0), dict(rate=0.1, mask="x"), dict(rate=0.1, target="x"),
               dict(rate=lambda x, y: 1.0)):
        with pytest.raises(E, match="Relaxation"):
            S.Relaxation(**kw)
    with pytest.raises(E, match="not finite"):
        S.Relaxation(0.1, target=lambda x, y: np.where(x > 0.5, np.inf, 1.0) + 0 * y).evaluate(g, (S.Face, S.Center), "u")
    with pytest.raises(E, match="shape"):
        S.Relaxation(0.1, mask=np.ones((16, 8))).evaluate(g, (S.Center, S.Center), "h")
    with pytest.raises(E, match="belong to an ensemble"):
        S.Relaxation([0.1, 0.2]).evaluate(g, (S.Center, S.Center), "h")
    # members
    pm = S.Relaxation([0.1, 0.2], mask=np.stack([m, 2 * m]), target=[1.0, 2.0])
    assert pm.per_member
    one = pm.for_member(1)
    assert one.rate == 0.2 and one.target == 2.0 and np.array_equal(one.mask, 2 * m) and not one.per_member
    mk, tg = pm.evaluate(g, (S.Center, S.Center), "h", members=2)
    assert mk.shape == (2, 8, 16) and np.array_equal(tg, [1.0, 2.0])
    with pytest.raises(E, match=r"expected \(8, 16\) or \(3, 8, 16\)"):
        pm.evaluate(g, (S.Center, S.Center), "h", members=3)


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
    drag = {"u": S.Relaxation(0.1), "v": S.Relaxation(0.1)}
    for topo in (("Bounded", "Periodic", "Flat"), ("Periodic", "Bounded", "Flat"), ("Bounded", "Bounded", "Flat")):
        gb = S.RectilinearGrid(size=(16, 16), x=(0, 1), y=(0, 1), topology=topo)
        with pytest.raises(E, match="SWMHD_ENOTSUP"):
            S.BoundedShallowWaterEnsemble(gb, 2, forcing=drag)
        with pytest.raises(E, match="SWMHD_ENOTSUP"):
            S.ShallowWaterEnsemble(gb, 2, forcing=drag)
    with pytest.raises(E, match="SWMHD_ENOTSUP"):
        S.ShallowWaterModel(g, forcing=drag, fused=False)
    with pytest.raises(E, match="SWMHD_ENOTSUP"):
        S.ShallowWaterModel(g, forcing=drag, ring=ctypes.c_void_p(1))
    with pytest.raises(E, match="SWMHD_ENOTSUP"):
        S.ShallowWaterModel(S.RectilinearGrid(size=(16, 8), x=(0, 1), y=(0, 1), j_offset=0, Ny_global=16), forcing=drag,
                            decomp=S.SlabDecomposition(16, 2, 0))
    for cls, args in ((S.ShallowWaterModel, (g,)), (S.ShallowWaterEnsemble, (g, 2))):
        with pytest.raises(E, match="prognostic field is 'uh'"):
            cls(*args, formulation=S.ConservativeFormulation, forcing=drag)
        with pytest.raises(E, match="prognostic field is 'v'"):
            cls(*args, forcing={"vh": S.Relaxation(0.1)})
        with pytest.raises(E, match="prognostic fields are"):
            cls(*args, forcing={"c": S.Relaxation(0.1)})
        with pytest.raises(E, match="prognostic fields are"):
            cls(*args, tracers=("d",), forcing={"B_x": S.Relaxation(0.1)})
        with pytest.raises(E, match="a Relaxation"):
            cls(*args, forcing={"u": 0.1})
        with pytest.raises(E, match="forcing: a dict"):
            cls(*args, forcing=S.Relaxation(0.1))
        with pytest.raises(E, match="shape"):
            cls(*args, forcing={"h": S.Relaxation(0.1, target=np.ones((4, 4)))})
        with pytest.raises(E, match="not finite"):
            cls(*args, forcing={"h": S.Relaxation(0.1, mask=lambda x, y: np.where(y > 0.5, np.nan, 1.0) + 0 * x)})
    with pytest.raises(E, match="belong to an ensemble"):
        S.ShallowWaterModel(g, forcing={"u": S.Relaxation([0.1, 0.2])})
    with pytest.raises(E, match="2 rates for 3 members"):
        S.ShallowWaterEnsemble(g, 3, forcing={"u": S.Relaxation([0.1, 0.2])})
    with pytest.raises(E, match="2 targets for 3 members"):
        S.ShallowWaterEnsemble(g, 3, forcing={"h": S.Relaxation(0.1, target=[1.0, 2.0])})
