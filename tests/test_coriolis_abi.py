"""CPU tests (no GPU) of the BetaPlane Coriolis: the entry points of include/swmhd_coriolis.h are exported and declared, every argument
error comes back with its code before any HIP call, the Python classes refuse what they do not support before anything is allocated,
and coriolis=None / FPlane change nothing in what a model calls."""
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


def test_coriolis_symbols_are_exported(swmhd):
    B = swmhd._lib
    L = B.lib()
    assert B.CORIOLIS_EXPORTS == [f"swmhd_{n}_{s}" for s in ("f64", "f32") for n in ("coriolis_rk3", "ensemble_coriolis_rk3")]
    header = open(os.path.join(ROOT, "include", "swmhd_coriolis.h")).read()
    for name in B.CORIOLIS_EXPORTS:
        assert hasattr(L, name)
        assert re.search(rf"^int {name}\(", header, flags=re.M), name
    assert sorted(re.findall(r"^int (swmhd_\w+)\(", header, flags=re.M)) == sorted(B.CORIOLIS_EXPORTS)
    assert '#include "swmhd_coriolis.h"' in open(os.path.join(ROOT, "include", "swmhd.h")).read()
    assert "swmhd_coriolis.h" in open(os.path.join(ROOT, "swmhd_amd", "csrc", "Makefile")).read()
    assert re.search(rf"^#define SWMHD_CORIOLIS_TILE_ROWS {B.CORIOLIS_TILE_ROWS}$", header, flags=re.M)
    assert L.swmhd_version() == 300          # symbols added, none changed
    assert re.search(r"^#define SWMHD_VERSION 300$", open(os.path.join(ROOT, "include", "swmhd.h")).read(), flags=re.M)
    others = B.EXPORTS + B.ZONAL_EXPORTS + B.DERIVED_EXPORTS + B.SPECTRA_EXPORTS + B.DIFFUSION_EXPORTS
    assert not set(B.CORIOLIS_EXPORTS) & set(others)
    for name in ("FPlane", "BetaPlane", "CoriolisProfile"):
        assert name in swmhd.__all__ and hasattr(swmhd, name)


@pytest.mark.parametrize("ens", [False, True], ids=["single", "ensemble"])
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_coriolis_return_codes(swmhd, sfx, ens):
    """Every code, in the order the header states the checks; host memory stands in for the device pointers: no check reads it."""
    B = swmhd._lib
    L = B.lib()
    buf = (FLOAT[sfx] * 64)()
    at = lambda k: ctypes.c_void_p(ctypes.addressof(buf) + 16 * k)
    q1, q2, n1, n2, a1, a2, tab = (at(k) for k in range(7))
    fn = getattr(L, f"swmhd_{'ensemble_' if ens else ''}coriolis_rk3_{sfx}")

    def call(q1=q1, q2=q2, n1=n1, n2=n2, a1=a1, a2=a2, frow=tab, members=2, stride_m=(Ny + 2 * H) * SY, nx=Nx, ny=Ny, Hx=H, Hy=H, sy=SY,
             params=None, a=0.01, w=1.0, j0=3, j1=3, flags=0):
        if ens:
            return fn(q1, q2, n1, n2, a1, a2, frow, members, stride_m, nx, ny, Hx, Hy, sy, params, a, w, j0, j1, flags, None)
        return fn(q1, q2, n1, n2, a1, a2, frow, nx, ny, Hx, Hy, sy, a, w, j0, j1, flags, None)

    # null parents or a null table
    for name in ("q1", "q2", "n1", "n2", "frow"):
        assert call(**{name: None}) == EINVAL, name
    # one acc without the other
    assert call(a1=None) == EINVAL
    assert call(a2=None) == EINVAL
    # extents, pitch, rows
    assert call(nx=0) == EINVAL
    assert call(ny=0) == EINVAL
    assert call(Hx=-1) == EINVAL
    assert call(Hy=-1) == EINVAL
    assert call(sy=Nx + 2 * H - 1) == EINVAL
    assert call(j0=-1) == EINVAL
    assert call(j1=Ny + 1) == EINVAL
    assert call(j0=5, j1=4) == EINVAL
    # unknown flag bits; both flags of one direction
    assert call(flags=8) == EINVAL
    assert call(flags=1 << 20) == EINVAL
    assert call(flags=B.BOUNDED_X | B.WRAP_X) == EINVAL
    assert call(flags=B.BOUNDED_Y | B.WRAP_Y | B.WRAP_X) == EINVAL
    # an output equal to an input or to another output
    assert call(n1=q1) == EINVAL
    assert call(n2=q1) == EINVAL
    assert call(n1=q2) == EINVAL
    assert call(a1=q1) == EINVAL
    assert call(a2=q2) == EINVAL
    assert call(n2=n1) == EINVAL
    assert call(a1=n1) == EINVAL
    assert call(a2=n2) == EINVAL
    assert call(a2=a1) == EINVAL
    # a or w not finite
    assert call(a=float("inf")) == EINVAL
    assert call(a=float("nan")) == EINVAL
    assert call(w=float("nan")) == EINVAL
    assert call(w=float("-inf")) == EINVAL
    if ens:
        assert call(members=0) == EINVAL
        assert call(members=B.ENSEMBLE_MAX_MEMBERS + 1) == EINVAL
        assert call(stride_m=(Ny + 2 * H) * SY - 1) == EINVAL
    # the order: an argument error comes before ENOTSUP, ENOTSUP before EHALO
    assert call(a=float("nan"), flags=B.MARCH_KERNEL, Hx=0) == EINVAL
    assert call(flags=B.MARCH_KERNEL, Hx=0) == ENOTSUP
    # known flags this family does not take
    for fl in (B.MARCH_KERNEL, B.TILE_KERNEL, B.GM_IS_PREV_STATE, B.OPEN_SOUTH, B.OPEN_NORTH | B.BOUNDED_Y, B.LEAVE_ROOM):
        assert call(flags=fl) == ENOTSUP, fl
    # a halo of depth >= 1 unless that direction is wrapped
    assert call(Hx=0) == EHALO
    assert call(Hy=0) == EHALO
    assert call(Hx=0, flags=B.WRAP_Y) == EHALO
    assert call(Hy=0, flags=B.WRAP_X) == EHALO
    assert call(Hx=0, flags=B.BOUNDED_X) == EHALO
    # accepted, nothing to enqueue: an empty row range with every accepted flag, with and without acc
    for fl in (0, B.STRICT, B.WRAP_X | B.WRAP_Y, B.STRICT | B.WRAP_X, B.RK3_ANCHOR | B.WRAP_X | B.WRAP_Y, B.RK3_ANCHOR | B.STRICT,
               B.BOUNDED_X, B.BOUNDED_Y | B.WRAP_X, B.BOUNDED_X | B.BOUNDED_Y | B.STRICT):
        assert call(flags=fl) == 0, fl
        assert call(flags=fl, a1=None, a2=None) == 0, fl
    assert call(Hx=0, Hy=0, flags=B.WRAP_X | B.WRAP_Y) == 0
    assert call(j0=0, j1=0) == 0
    assert call(j0=Ny, j1=Ny) == 0
    if ens:
        assert call(params=at(8)) == 0
        assert call(members=B.ENSEMBLE_MAX_MEMBERS, stride_m=1 << 20) == 0


def test_coriolis_classes(swmhd):
    S = swmhd
    E = S._lib.SwmhdError
    from swmhd_amd.coriolis import check_coriolis, row_table
    g = S.RectilinearGrid(size=(4, 3), x=(0, 1), y=(1.0, 4.0))
    for kw in (dict(f0=float("nan")), dict(beta=float("inf")), dict(f0=[[1.0]]), dict(f0=[1.0, 2.0], beta=[1.0, 2.0, 3.0])):
        with pytest.raises(E, match="BetaPlane"):
            S.BetaPlane(**kw)
    with pytest.raises(E, match="FPlane"):
        S.FPlane(float("nan"))
    with pytest.raises(E, match="callable"):
        S.CoriolisProfile(1.0)
    with pytest.raises(E, match="not finite"):
        S.CoriolisProfile(lambda y: np.where(y > 2.0, np.inf, y)).rows(g)
    assert "BetaPlane(f0=1.0, beta=2.0)" == repr(S.BetaPlane(1.0, 2.0))
    # None and FPlane: the scalar of the stage kernels and no table; with coriolis= given, coriolis_f must be left at its default
    assert check_coriolis(None, 0.7, 1.0) == (0.7, None)
    assert check_coriolis(S.FPlane(0.7), 1.0, 1.0) == (0.7, None)
    f, prof = check_coriolis(S.BetaPlane(0.7, 0.1), 1.0, 1.0)
    assert f == 0.0 and isinstance(prof, S.BetaPlane)
    for c in (S.FPlane(0.7), S.BetaPlane(0.7, 0.1)):
        with pytest.raises(E, match="coriolis_f"):
            check_coriolis(c, 0.5, 1.0)
        with pytest.raises(E, match="coriolis_f"):
            check_coriolis(c, [1.0, 1.0], 1.0)
    with pytest.raises(E, match="coriolis"):
        check_coriolis(0.7, 1.0, 1.0)
    # the tables
    t = row_table(S.BetaPlane(0.5, 2.0), g)
    assert t.shape == (2, 3) and np.array_equal(t[0], 0.5 + 2.0 * np.array([1.5, 2.5, 3.5])) and np.array_equal(t[1], 0.5 + 2.0 * np.array([1.0, 2.0, 3.0]))
    t3 = row_table(S.BetaPlane(0.5, [2.0, 0.0, -1.0]), g, 3)
    assert t3.shape == (3, 2, 3) and np.array_equal(t3[0], t) and np.all(t3[1] == 0.5) and np.array_equal(t3[2, 1], 0.5 - np.array([1.0, 2.0, 3.0]))
    assert np.array_equal(row_table(S.BetaPlane(0.5, 2.0), g, 2), np.stack([t, t]))
    with pytest.raises(E, match="members"):
        row_table(S.BetaPlane([0.5, 0.6], 2.0), g, 3)
    with pytest.raises(E, match="ensemble"):
        row_table(S.BetaPlane([0.5, 0.6], 2.0), g)


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
    b = S.BetaPlane(1.0, 0.5)
    for topo in (("Bounded", "Periodic", "Flat"), ("Periodic", "Bounded", "Flat"), ("Bounded", "Bounded", "Flat")):
        gb = S.RectilinearGrid(size=(16, 16), x=(0, 1), y=(0, 1), topology=topo)
        with pytest.raises(E, match="SWMHD_ENOTSUP"):
            S.BoundedShallowWaterEnsemble(gb, 2, coriolis=b)
        with pytest.raises(E, match="SWMHD_ENOTSUP"):
            S.ShallowWaterEnsemble(gb, 2, coriolis=b)
        with pytest.raises(AssertionError, match="allocated"):      # a Bounded MODEL is supported: it gets as far as its fields
            S.ShallowWaterModel(gb, coriolis=b)
    with pytest.raises(E, match="SWMHD_ENOTSUP"):
        S.ShallowWaterModel(g, coriolis=b, fused=False)
    with pytest.raises(E, match="SWMHD_ENOTSUP"):
        S.ShallowWaterModel(g, coriolis=b, ring=ctypes.c_void_p(1))
    with pytest.raises(E, match="SWMHD_ENOTSUP"):
        S.ShallowWaterModel(S.RectilinearGrid(size=(16, 8), x=(0, 1), y=(0, 1), j_offset=0, Ny_global=16), coriolis=b,
                            decomp=S.SlabDecomposition(16, 2, 0))
    for cls, args in ((S.ShallowWaterModel, (g,)), (S.ShallowWaterEnsemble, (g, 2)), (S.BoundedShallowWaterEnsemble, (g, 2))):
        with pytest.raises(E, match="coriolis_f"):
            cls(*args, coriolis_f=0.5, coriolis=b)
        with pytest.raises(E, match="coriolis_f"):
            cls(*args, coriolis_f=0.5, coriolis=S.FPlane(0.5))
        with pytest.raises(E, match="coriolis"):
            cls(*args, coriolis=0.5)
    with pytest.raises(E, match="ensemble"):
        S.ShallowWaterModel(g, coriolis=S.BetaPlane(1.0, [0.5, 0.6]))
    with pytest.raises(E, match="ensemble"):
        S.ShallowWaterModel(g, coriolis=S.FPlane([0.5, 0.6]))
    with pytest.raises(E, match="members"):
        S.ShallowWaterEnsemble(g, 3, coriolis=S.BetaPlane(1.0, [0.5, 0.6]))
    with pytest.raises(E, match="not finite"):
        S.ShallowWaterModel(g, coriolis=S.CoriolisProfile(lambda y: np.full_like(y, np.nan)))


class _Entry:
    """A recording entry of a model's _corrections."""

    def __init__(self, name):
        self.name = name

    def launch(self, o, dt, stage):
        assert o._state == "state"          # before the swaps
        o.log.append(self.name)


class _Stub:
    """What finish_stage touches of a model, with the tracer stage and the entries of _corrections recording their calls."""

    def __init__(self, coriolis, diffusion, tracers):
        self.log = []
        self._coriolis, self._diffusion = coriolis, diffusion
        self._corrections = ([_Entry("coriolis")] if coriolis is not None else []) + ([_Entry("diffusion")] if diffusion is not None else [])
        self._tr, self._tr_alt, self._tGn, self._tGm = ({"c": 1} if tracers else {}), {}, [], []
        self._state, self._alt, self.Gn, self.Gm = "state", "alt", "Gn", "Gm"

    def _tracer_stage(self, dt, stage):
        self.log.append("tracers")


def test_none_and_fplane_leave_the_stage_as_it_was(swmhd):
    """finish_stage launches the Coriolis correction only where the constructor kept a parameter that varies with y -- after the
    tracers, before the closure, before the swaps -- and the constructors keep none for None and FPlane (check_coriolis, above).  The
    list the constructors build has its four kinds in the order of the launches."""
    import types

    import torch
    from swmhd_amd.corrections import correction_list
    from swmhd_amd.shared import finish_stage
    for tracers in (False, True):
        for diffusion in (None, {"A": 1e-3}):
            plain = _Stub(None, diffusion, tracers)
            finish_stage(plain, 1e-3, 0)
            assert "coriolis" not in plain.log
            beta = _Stub(object(), diffusion, tracers)
            finish_stage(beta, 1e-3, 0)
            assert beta.log == (["tracers"] if tracers else []) + ["coriolis"] + (["diffusion"] if diffusion else [])
            assert [x for x in beta.log if x != "coriolis"] == plain.log
            assert (beta._state, beta._alt, beta.Gn, beta.Gm) == ("alt", "state", "Gm", "Gn")
    # what correction_list reads of a model with all four kinds (host tensors stand in for the device tables: nothing is launched)
    g = swmhd.RectilinearGrid(size=(8, 8), x=(0, 1), y=(0, 1))
    o = types.SimpleNamespace(grid=g, names=("u", "v", "h", "A"), tracer_names=("c",), sfx="f64", _coriolis=object(),
                              coriolis_rows=torch.zeros(2, 8, dtype=torch.float64), _diffusion={"u": 1e-3, "A": 2e-3},
                              _biharmonic={"c": 1e-6}, _relaxation=[("h", 0.5, None, 1.0), ("c", 0.1, torch.zeros(14, 14, dtype=torch.float64), 0.0)])
    built = correction_list(o, 14)
    assert [c.stem for c in built] == ["coriolis", "diffusion", "biharmonic", "relaxation"]
    assert [c.names for c in built] == [("u", "v"), ("u", "A"), ("c",), ("h", "c")]
    o._coriolis = o._diffusion = o._biharmonic = o._relaxation = None
    assert correction_list(o, 14) == []


def test_potential_vorticity_is_refused_under_f_of_y(swmhd):
    S = swmhd
    E = S._lib.SwmhdError
    from swmhd_amd.derived import check_coriolis_names

    class M:
        pass
    m = M()
    m._coriolis = m.coriolis = S.BetaPlane(1.0, 0.5)
    with pytest.raises(E, match="SWMHD_ENOTSUP"):
        check_coriolis_names(m, ("vorticity", "potential_vorticity"))
    check_coriolis_names(m, ("vorticity", "divergence", "current"))
    m._coriolis = None
    check_coriolis_names(m, ("potential_vorticity",))
    with pytest.raises(E, match="SWMHD_ENOTSUP"):
        m._coriolis = S.BetaPlane(1.0, 0.5)
        m.tracer_names = ()
        S.FieldTimeSeries(m, names=("u", "potential_vorticity"), capacity=2)
