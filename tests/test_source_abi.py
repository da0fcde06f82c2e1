"""CPU tests (no GPU) of the static sources (bathymetry, Source): the entry points of include/swmhd_source.h are exported and declared,
every argument error comes back with its code, in the documented order, before any HIP call, and the Python classes refuse what they do
not support before anything is allocated."""
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


def test_source_symbols_are_exported(swmhd):
    B = swmhd._lib
    L = B.lib()
    assert B.SOURCE_EXPORTS == [f"swmhd_{n}_{s}" for s in ("f64", "f32") for n in ("source_rk3", "ensemble_source_rk3")]
    header = open(os.path.join(ROOT, "include", "swmhd_source.h")).read()
    for name in B.SOURCE_EXPORTS:
        assert hasattr(L, name)
        assert re.search(rf"^int {name}\(", header, flags=re.M), name
    assert sorted(re.findall(r"^int (swmhd_\w+)\(", header, flags=re.M)) == sorted(B.SOURCE_EXPORTS)
    assert '#include "swmhd_source.h"' in open(os.path.join(ROOT, "include", "swmhd.h")).read()
    assert re.search(r"^#define SWMHD_SOURCE_MAX_FIELDS 12$", header, flags=re.M) and B.SOURCE_MAX_FIELDS == 12 == 4 + B.MAX_TRACERS
    assert re.search(rf"^#define SWMHD_SOURCE_TILE_ROWS {B.SOURCE_TILE_ROWS}$", header, flags=re.M)
    for k, name in enumerate(("PLAIN", "X_FACE", "Y_FACE")):
        assert re.search(rf"^#define SWMHD_SOURCE_{name} {k}$", header, flags=re.M) and getattr(B, f"SOURCE_{name}") == k
    assert L.swmhd_version() == 300          # symbols added, none changed
    others = (B.EXPORTS, B.ZONAL_EXPORTS, B.DERIVED_EXPORTS, B.SPECTRA_EXPORTS, B.SPECTRA2D_EXPORTS, B.DIFFUSION_EXPORTS,
              B.BIHARMONIC_EXPORTS, B.CORIOLIS_EXPORTS, B.RELAXATION_EXPORTS, B.STOCHASTIC_EXPORTS)
    assert not any(set(B.SOURCE_EXPORTS) & set(o) for o in others)
    # the header states the formula, the bytes, the checks and their order, the bound and the decision on the conservative term
    for words in ("D = ((h_old[i-1,j] + h_old[i,j]) / 2) S_k[i,j]", "D = ((h_old[i,j-1] + h_old[i,j]) / 2) S_k[i,j]",
                  "Bytes per cell, field and stage (fp64)", "Checks, in this order", "eps |ref| + ((1 + eps/2)^n - 1) |a| M",
                  "INTERPOLATED form is a decision"):
        assert words in header, words


@pytest.mark.parametrize("ens", [False, True], ids=["single", "ensemble"])
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_source_return_codes(swmhd, sfx, ens):
    B = swmhd._lib
    L = B.lib()
    _o, old = _bufs(sfx)
    _n, new = _bufs(sfx)
    _a, acc = _bufs(sfx)
    _s, src = _bufs(sfx)
    fn = getattr(L, f"swmhd_{'ensemble_' if ens else ''}source_rk3_{sfx}")
    V = ctypes.c_void_p
    kinds = lambda *v: (ctypes.c_int * len(v))(*v)
    plain, mixed = kinds(*[0] * 12), kinds(1, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)

    def call(old=old, new=new, acc=acc, src=src, kind=plain, n=3, thick=-1, members=2, stride_m=MEMBER, src_sm=0, nx=Nx, ny=Ny, Hx=H, Hy=H,
             sy=SY, params=None, a=0.01, w=1.0, j0=0, j1=Ny, flags=0):
        if ens:
            return fn(old, new, acc, src, kind, n, thick, members, stride_m, src_sm, nx, ny, Hx, Hy, sy, params, a, w, j0, j1, flags, None)
        return fn(old, new, acc, src, kind, n, thick, nx, ny, Hx, Hy, sy, a, w, j0, j1, flags, None)

    # null pointers
    assert call(old=None) == EINVAL
    assert call(new=None) == EINVAL
    assert call(src=None) == EINVAL
    assert call(kind=None) == EINVAL
    # nfields
    assert call(n=0) == EINVAL
    assert call(n=B.SOURCE_MAX_FIELDS + 1) == EINVAL
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
    assert call(old=(V * 3)(old[0], None, old[2])) == EINVAL
    assert call(new=(V * 3)(new[0], new[1], None)) == EINVAL
    # aliasing: an output on any input (old, source), an output twice
    assert call(new=old) == EINVAL
    assert call(new=(V * 3)(new[0], old[0], new[2])) == EINVAL
    assert call(new=(V * 3)(new[0], new[1], src[0])) == EINVAL
    assert call(acc=old) == EINVAL
    assert call(acc=(V * 3)(acc[0], None, old[0])) == EINVAL
    assert call(acc=(V * 3)(src[1], acc[1], None)) == EINVAL
    assert call(acc=new) == EINVAL
    assert call(new=(V * 3)(new[0], new[0], new[2])) == EINVAL
    assert call(acc=(V * 3)(acc[0], acc[0], None)) == EINVAL
    assert call(acc=(V * 3)(new[1], acc[1], None)) == EINVAL
    # a or w not finite
    assert call(a=float("inf")) == EINVAL
    assert call(w=float("nan")) == EINVAL
    # kinds and the thickness
    assert call(kind=kinds(0, 3, 0)) == EINVAL
    assert call(kind=kinds(-1, 0, 0)) == EINVAL
    assert call(kind=kinds(0, 0, 7), src=(V * 3)(src[0], src[1], None)) == EINVAL       # (a kind is checked with or without a source)
    assert call(thick=-2) == EINVAL
    assert call(thick=3) == EINVAL
    assert call(kind=mixed, thick=-1) == EINVAL                                            # a kind needs the thickness
    assert call(kind=kinds(0, 2, 0), thick=-1) == EINVAL
    if ens:
        assert call(members=0) == EINVAL
        assert call(members=B.ENSEMBLE_MAX_MEMBERS + 1) == EINVAL
        assert call(stride_m=MEMBER - 1) == EINVAL
        assert call(stride_m=0) == EINVAL
        # the member stride of the sources: 0 (shared) or a whole parent
        assert call(src_sm=MEMBER - 1) == EINVAL
        assert call(src_sm=1) == EINVAL
        assert call(src_sm=-MEMBER) == EINVAL
        assert call(members=0, flags=B.TILE_KERNEL) == EINVAL
        assert call(src_sm=MEMBER, j0=3, j1=3) == 0
    # known flags this family does not take; an argument error beside one of them comes first
    for fl in (B.MARCH_KERNEL, B.TILE_KERNEL, B.GM_IS_PREV_STATE, B.OPEN_SOUTH, B.OPEN_NORTH | B.BOUNDED_Y, B.LEAVE_ROOM):
        assert call(flags=fl) == ENOTSUP, fl
        assert call(flags=fl, n=0) == EINVAL
        assert call(flags=fl, a=float("nan")) == EINVAL
        assert call(flags=fl, kind=mixed, thick=-1) == EINVAL
        assert call(flags=fl, j0=3, j1=3) == ENOTSUP          # before "nothing to enqueue"
        assert call(flags=fl, kind=mixed, thick=2, Hx=0, Hy=0, sy=Nx) == ENOTSUP      # before SWMHD_EHALO
    # SWMHD_EHALO: a weighted field reads the thickness one cell west or south -- the periodic image, else a halo cell
    weighted = dict(kind=mixed, thick=2, j0=3, j1=3)
    assert call(**weighted, Hx=0, Hy=0, sy=Nx) == EHALO
    assert call(**weighted, Hx=0, Hy=1, sy=Nx, flags=B.WRAP_Y) == EHALO
    assert call(**weighted, Hx=1, Hy=0, sy=Nx + 2, flags=B.WRAP_X) == EHALO
    assert call(**weighted, Hx=0, Hy=0, sy=Nx, flags=B.BOUNDED_X | B.BOUNDED_Y) == EHALO
    assert call(**weighted, Hx=0, Hy=0, sy=Nx, flags=B.WRAP_X | B.WRAP_Y) == 0
    assert call(**weighted, Hx=0, Hy=1, sy=Nx, flags=B.WRAP_X) == 0
    assert call(**weighted, Hx=1, Hy=1, sy=Nx + 2) == 0
    # the weighted fields without a source do not count; plain fields accept no halo at all
    assert call(kind=mixed, thick=2, src=(V * 3)(None, None, src[2]), j0=3, j1=3, Hx=0, Hy=0, sy=Nx) == 0
    assert call(kind=mixed, thick=-1, src=(V * 3)(None, None, src[2]), j0=3, j1=3) == 0
    assert call(j0=3, j1=3, Hx=0, Hy=0, sy=Nx) == 0
    # accepted, nothing to enqueue: an empty row range with every accepted flag, the widest list, no acc, null entries
    for fl in (0, B.STRICT, B.WRAP_X | B.WRAP_Y, B.STRICT | B.WRAP_X, B.RK3_ANCHOR | B.WRAP_X | B.WRAP_Y, B.RK3_ANCHOR | B.STRICT,
               B.BOUNDED_X, B.BOUNDED_Y | B.WRAP_X, B.BOUNDED_X | B.BOUNDED_Y | B.STRICT):
        assert call(j0=3, j1=3, flags=fl) == 0, fl
        assert call(j0=3, j1=3, flags=fl, kind=mixed, thick=2) == 0, fl
    assert call(j0=0, j1=0, n=B.SOURCE_MAX_FIELDS) == 0
    assert call(j0=Ny, j1=Ny, acc=None) == 0
    assert call(j0=3, j1=3, acc=(V * 3)(None, acc[1], None), src=(V * 3)(src[0], None, src[0])) == 0      # a source may be shared
    # sources that are all NULL: nothing to enqueue for any rows
    assert call(src=(V * 3)(None, None, None)) == 0
    assert call(src=(V * 3)(None, None, None), kind=mixed, thick=2, acc=None) == 0


def test_source_values(swmhd):
    S = swmhd
    E = S._lib.SwmhdError
    g = S.RectilinearGrid(size=(16, 8), x=(0, 1.6), y=(0, 0.4))
    assert S.Source(0.5).value == 0.5 and not S.Source(0.5).per_member and "0.5" in repr(S.Source(0.5))
    seen = {}

    def force(x, y):
        seen["shapes"] = (x.shape, y.shape)
        return x + 10 * y
    F = S.Source(force).evaluate(g, (S.Face, S.Center), "u")
    assert seen["shapes"] == ((1, 16), (8, 1)) and F.shape == (8, 16)
    assert np.array_equal(F, g.xf[3:19][None, :] + 10 * g.yc[3:11][:, None])
    assert np.array_equal(S.Source(force).evaluate(g, (S.Center, S.Face), "v"), g.xc[3:19][None, :] + 10 * g.yf[3:11][:, None])
    assert np.array_equal(S.Source(lambda x, y: 2.0).evaluate(g, (S.Center, S.Center), "h"), np.full((8, 16), 2.0))
    assert np.array_equal(S.Source(0.25).evaluate(g, (S.Center, S.Center), "h"), np.full((8, 16), 0.25))
    for v in (float("nan"), float("inf"), "x", np.zeros((1, 1, 1, 1)), np.full((8, 16), np.nan)):
        with pytest.raises(E, match="Source"):
            S.Source(v)
    with pytest.raises(E, match="not finite"):
        S.Source(lambda x, y: np.where(x > 0.5, np.inf, 1.0) + 0 * y).evaluate(g, (S.Face, S.Center), "u")
    with pytest.raises(E, match="shape"):
        S.Source(np.ones((16, 8))).evaluate(g, (S.Center, S.Center), "h")
    with pytest.raises(E, match="shape"):
        S.Source(lambda x, y: np.ones((3, 3))).evaluate(g, (S.Center, S.Center), "h")
    with pytest.raises(E, match="belong to an ensemble"):
        S.Source([0.1, 0.2]).evaluate(g, (S.Center, S.Center), "h")
    pm = S.Source([0.1, 0.2])
    assert pm.per_member and pm.for_member(1).value == 0.2 and not pm.for_member(1).per_member
    assert np.array_equal(pm.evaluate(g, (S.Center, S.Center), "h", members=2)[1], np.full((8, 16), 0.2))
    with pytest.raises(E, match="2 sources for 3 members"):
        pm.evaluate(g, (S.Center, S.Center), "h", members=3)
    arr = np.arange(2 * 8 * 16, dtype=float).reshape(2, 8, 16)
    assert np.array_equal(S.Source(arr).for_member(1).value, arr[1])
    with pytest.raises(E, match=r"expected \(8, 16\) or \(3, 8, 16\)"):
        S.Source(arr).evaluate(g, (S.Center, S.Center), "h", members=3)
    shared = S.Source(force)
    assert shared.for_member(1) is shared


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
    hill = lambda x, y: 0.1 * np.exp(-((x - 0.5) ** 2 + (y - 0.5) ** 2) / 0.02)
    push = {"u": S.Source(0.1)}
    for kw in (dict(bathymetry=hill), dict(forcing=push)):
        for topo in (("Bounded", "Periodic", "Flat"), ("Periodic", "Bounded", "Flat"), ("Bounded", "Bounded", "Flat")):
            gb = S.RectilinearGrid(size=(16, 16), x=(0, 1), y=(0, 1), topology=topo)
            with pytest.raises(E, match="SWMHD_ENOTSUP"):
                S.BoundedShallowWaterEnsemble(gb, 2, **kw)
            with pytest.raises(E, match="SWMHD_ENOTSUP"):
                S.ShallowWaterEnsemble(gb, 2, **kw)
        with pytest.raises(E, match="SWMHD_ENOTSUP"):
            S.ShallowWaterModel(g, fused=False, **kw)
        with pytest.raises(E, match="SWMHD_ENOTSUP"):
            S.ShallowWaterModel(g, ring=ctypes.c_void_p(1), **kw)
        with pytest.raises(E, match="SWMHD_ENOTSUP"):
            S.ShallowWaterModel(S.RectilinearGrid(size=(16, 8), x=(0, 1), y=(0, 1), j_offset=0, Ny_global=16), decomp=S.SlabDecomposition(16, 2, 0), **kw)
    with pytest.raises(E, match="bathymetry on a Bounded ensemble"):
        S.BoundedShallowWaterEnsemble(S.RectilinearGrid(size=(16, 16), x=(0, 1), y=(0, 1), topology=("Periodic", "Bounded", "Flat")), 2, bathymetry=hill)
    with pytest.raises(E, match="bathymetry needs the fused stage kernel"):
        S.ShallowWaterModel(g, bathymetry=hill, fused=False)
    for cls, args in ((S.ShallowWaterModel, (g,)), (S.ShallowWaterEnsemble, (g, 2))):
        with pytest.raises(E, match="prognostic field is 'uh'"):
            cls(*args, formulation=S.ConservativeFormulation, forcing=push)
        with pytest.raises(E, match="prognostic fields are"):
            cls(*args, forcing={"c": S.Source(0.1)})
        with pytest.raises(E, match="a Relaxation, a StochasticForcing, a Source or a tuple with at most one of each"):
            cls(*args, forcing={"u": (S.Source(0.1), S.Source(0.2))})
        with pytest.raises(E, match="at most one of each, not float"):
            cls(*args, forcing={"u": (S.Source(0.1), 0.2)})
        with pytest.raises(E, match="shape"):
            cls(*args, forcing={"h": S.Source(np.ones((4, 4)))})
        with pytest.raises(E, match="not finite"):
            cls(*args, forcing={"h": S.Source(lambda x, y: np.where(y > 0.5, np.nan, 1.0) + 0 * x)})
        with pytest.raises(E, match="bathymetry.*shape"):
            cls(*args, bathymetry=np.ones((4, 4)))
        with pytest.raises(E, match="bathymetry.*shape"):
            cls(*args, bathymetry=lambda x, y: np.ones((3, 3)))
        with pytest.raises(E, match="bathymetry = str"):
            cls(*args, bathymetry="flat")
        with pytest.raises(E, match="bathymetry has values that are not finite"):
            cls(*args, bathymetry=lambda x, y: np.where(y > 0.5, np.inf, 1.0) + 0 * x)
    with pytest.raises(E, match="belong to an ensemble"):
        S.ShallowWaterModel(g, forcing={"u": S.Source([0.1, 0.2])})
    with pytest.raises(E, match="bathymetry.*shape"):
        S.ShallowWaterModel(g, bathymetry=np.zeros((2, 16, 16)))
    with pytest.raises(E, match="2 sources for 3 members"):
        S.ShallowWaterEnsemble(g, 3, forcing={"u": S.Source([0.1, 0.2])})
    with pytest.raises(E, match=r"bathymetry.*\(16, 16\) or \(3, 16, 16\)"):
        S.ShallowWaterEnsemble(g, 3, bathymetry=np.zeros((2, 16, 16)))
