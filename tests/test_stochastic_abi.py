"""CPU tests (no GPU) of the StochasticForcing: the entry points of include/swmhd_stochastic.h are exported and declared, every argument
error comes back with its code before any HIP call, and the Python classes refuse what they do not support before anything is
allocated."""
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
V = ctypes.c_void_p


def _bufs(ct, n=12):
    buf = (ct * 64)()
    return buf, (V * n)(*[ctypes.addressof(buf) + 8 * k for k in range(n)])


def _ints(*v):
    return (ctypes.c_int * len(v))(*v)


def test_stochastic_symbols_are_exported(swmhd):
    B = swmhd._lib
    L = B.lib()
    assert B.STOCHASTIC_EXPORTS == [f"swmhd_{n}_{s}" for s in ("f64", "f32") for n in (
        "stochastic_coefficients", "ensemble_stochastic_coefficients", "stochastic_rk3", "ensemble_stochastic_rk3")]
    header = open(os.path.join(ROOT, "include", "swmhd_stochastic.h")).read()
    for name in B.STOCHASTIC_EXPORTS:
        assert hasattr(L, name)
        assert re.search(rf"^int {name}\(", header, flags=re.M), name
    assert sorted(re.findall(r"^int (swmhd_\w+)\(", header, flags=re.M)) == sorted(B.STOCHASTIC_EXPORTS)
    assert '#include "swmhd_stochastic.h"' in open(os.path.join(ROOT, "include", "swmhd.h")).read()
    for name, value in (("MAX_FIELDS", B.STOCHASTIC_MAX_FIELDS), ("MAX_MODES", B.STOCHASTIC_MAX_MODES), ("TILE_ROWS", B.STOCHASTIC_TILE_ROWS),
                        ("MODE_CHUNK", B.STOCHASTIC_MODE_CHUNK)):
        assert re.search(rf"^#define SWMHD_STOCHASTIC_{name} {value}$", header, flags=re.M), name
    assert (B.STOCHASTIC_MAX_FIELDS, B.STOCHASTIC_MAX_MODES) == (12, 256)
    assert L.swmhd_version() == 300          # symbols added, none changed
    others = (B.EXPORTS, B.ZONAL_EXPORTS, B.DERIVED_EXPORTS, B.SPECTRA_EXPORTS, B.SPECTRA2D_EXPORTS, B.DIFFUSION_EXPORTS,
              B.BIHARMONIC_EXPORTS, B.CORIOLIS_EXPORTS, B.RELAXATION_EXPORTS)
    assert not any(set(B.STOCHASTIC_EXPORTS) & set(o) for o in others)
    # the header states the formulas, the generator with its known answers, the bytes and flops, the checks and the fast bound
    for words in ("R = P*cy[m][j] + Q*sy[m][j]", "Philox4x32-10", "6627e8d5 e169c58d bc57ac4c 9b00dbd8", "408f276d 41c83b0e a20bc7c6 6d5451fd",
                  "d16cfe09 94fdcceb 5001e420 24126ea1", "Bytes per cell, field and stage (fp64)", "Flops per cell and field",
                  "Checks, in this order", "(M + 3) eps |a| S"):
        assert words in header, words


@pytest.mark.parametrize("ens", [False, True], ids=["single", "ensemble"])
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_stochastic_rk3_return_codes(swmhd, sfx, ens):
    B = swmhd._lib
    L = B.lib()
    ft = FLOAT[sfx]
    _o, old = _bufs(ft)
    _n, new = _bufs(ft)
    _a, acc = _bufs(ft)
    _c, coef = _bufs(ft)
    _x, xtab = _bufs(ft)
    _y, ytab = _bufs(ft)
    _p, params = _bufs(ft)
    fn = getattr(L, f"swmhd_{'ensemble_' if ens else ''}stochastic_rk3_{sfx}")

    def call(old=old, new=new, acc=acc, coef=coef, xtab=xtab, ytab=ytab, nmodes=_ints(3, 1), n=2, xp=Nx, yp=Ny, members=2, stride_m=MEMBER,
             coef_sm=16, nx=Nx, ny=Ny, Hx=H, Hy=H, sy=SY, params=None, a=0.01, w=1.0, j0=0, j1=Ny, flags=0):
        if ens:
            return fn(old, new, acc, coef, xtab, ytab, nmodes, n, xp, yp, members, stride_m, coef_sm, nx, ny, Hx, Hy, sy, params, a, w, j0, j1,
                      flags, None)
        return fn(old, new, acc, coef, xtab, ytab, nmodes, n, xp, yp, nx, ny, Hx, Hy, sy, a, w, j0, j1, flags, None)

    # relaxation_common's checks: null pointers, nfields, extents, pitch, rows, flags, entries, aliasing, a and w
    assert call(old=None) == EINVAL
    assert call(new=None) == EINVAL
    assert call(n=0) == EINVAL
    assert call(n=B.STOCHASTIC_MAX_FIELDS + 1) == EINVAL
    assert call(nx=0) == EINVAL
    assert call(ny=0) == EINVAL
    assert call(Hx=-1) == EINVAL
    assert call(Hy=-1) == EINVAL
    assert call(sy=Nx + 2 * H - 1) == EINVAL
    assert call(j0=-1) == EINVAL
    assert call(j1=Ny + 1) == EINVAL
    assert call(j0=5, j1=4) == EINVAL
    assert call(flags=8) == EINVAL
    assert call(flags=1 << 20) == EINVAL
    assert call(flags=B.BOUNDED_X | B.WRAP_X) == EINVAL
    assert call(flags=B.BOUNDED_Y | B.WRAP_Y | B.STRICT) == EINVAL
    assert call(old=(V * 2)(old[0], None)) == EINVAL
    assert call(new=(V * 2)(new[0], None)) == EINVAL
    assert call(new=old) == EINVAL
    assert call(acc=(V * 2)(acc[0], old[0])) == EINVAL
    assert call(acc=new) == EINVAL
    assert call(new=(V * 2)(new[0], new[0])) == EINVAL
    assert call(a=float("inf")) == EINVAL
    assert call(w=float("nan")) == EINVAL
    # the tables: null lists, mode counts, null or misaligned entries of a field with modes, pitches
    assert call(coef=None) == EINVAL
    assert call(xtab=None) == EINVAL
    assert call(ytab=None) == EINVAL
    assert call(nmodes=None) == EINVAL
    assert call(nmodes=_ints(3, -1)) == EINVAL
    assert call(nmodes=_ints(B.STOCHASTIC_MAX_MODES + 1, 1)) == EINVAL
    for which in ("coef", "xtab", "ytab"):
        good = dict(coef=coef, xtab=xtab, ytab=ytab)[which]
        assert call(**{which: (V * 2)(good[0], None)}) == EINVAL, which
        assert call(**{which: (V * 2)(good[0] + 2, good[1])}) == EINVAL, which      # not a multiple of the element size
        assert call(**{which: (V * 2)(good[0], None)}, nmodes=_ints(3, 0), j0=3, j1=3) == 0      # a field without modes brings no tables
    assert call(xp=Nx - 1) == EINVAL
    assert call(yp=Ny - 1) == EINVAL
    if ens:
        assert call(members=0) == EINVAL
        assert call(members=B.ENSEMBLE_MAX_MEMBERS + 1) == EINVAL
        assert call(stride_m=MEMBER - 1) == EINVAL
        assert call(coef_sm=5) == EINVAL               # < 2 x 3 modes
        assert call(members=0, flags=B.TILE_KERNEL) == EINVAL
        # a per-member dt: the amplitude carries 1 / sqrt(dt)
        assert call(params=params[0]) == ENOTSUP
        assert call(params=params[0], j0=3, j1=3) == ENOTSUP
        assert call(params=params[0], n=0) == EINVAL
    for fl in (B.MARCH_KERNEL, B.TILE_KERNEL, B.GM_IS_PREV_STATE, B.OPEN_SOUTH, B.OPEN_NORTH | B.BOUNDED_Y, B.LEAVE_ROOM):
        assert call(flags=fl) == ENOTSUP, fl
        assert call(flags=fl, n=0) == EINVAL
        assert call(flags=fl, nmodes=_ints(3, 257)) == EINVAL
        assert call(flags=fl, j0=3, j1=3) == ENOTSUP          # before "nothing to enqueue"
    # there is no SWMHD_EHALO; accepted, nothing to enqueue: an empty row range, mode counts that are all 0 for any rows
    assert call(j0=3, j1=3, Hx=0, Hy=0, sy=Nx) == 0
    for fl in (0, B.STRICT, B.WRAP_X | B.WRAP_Y, B.RK3_ANCHOR | B.WRAP_X | B.WRAP_Y, B.BOUNDED_X | B.BOUNDED_Y | B.STRICT):
        assert call(j0=3, j1=3, flags=fl) == 0, fl
    assert call(j0=0, j1=0, n=B.STOCHASTIC_MAX_FIELDS, nmodes=_ints(*[1] * 12)) == 0
    assert call(j0=Ny, j1=Ny, acc=None) == 0
    assert call(nmodes=_ints(0, 0)) == 0
    assert call(nmodes=_ints(0, 0), coef=(V * 2)(None, None), xtab=(V * 2)(None, None), ytab=(V * 2)(None, None), acc=None) == 0


@pytest.mark.parametrize("ens", [False, True], ids=["single", "ensemble"])
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_stochastic_coefficients_return_codes(swmhd, sfx, ens):
    """Every defect is an argument error, answered before any HIP call (a valid call launches: the GPU tests make those)."""
    B = swmhd._lib
    L = B.lib()
    _k, counter = _bufs(ctypes.c_uint64)
    _c, coef = _bufs(FLOAT[sfx])
    _a, amp = _bufs(ctypes.c_double)
    _x, ktx = _bufs(ctypes.c_double)
    _y, kty = _bufs(ctypes.c_double)
    _s, subs = _bufs(ctypes.c_uint32)
    fn = getattr(L, f"swmhd_{'ensemble_' if ens else ''}stochastic_coefficients_{sfx}")

    def call(counter=counter[0], coef=coef, amp=amp, ktx=ktx, kty=kty, nmodes=_ints(3, 2), kind=_ints(1, 0), n=2, members=2, coef_sm=16,
             amp_sm=0, seed=5, sub=7, subs=subs[0], sdt=10.0):
        if ens:
            return fn(counter, coef, amp, ktx, kty, nmodes, kind, n, members, coef_sm, amp_sm, seed, subs, sdt, None)
        return fn(counter, coef, amp, ktx, kty, nmodes, kind, n, seed, sub, sdt, None)
    assert call(counter=None) == EINVAL
    assert call(counter=counter[0] + 4) == EINVAL           # not 8-byte aligned
    assert call(coef=None) == EINVAL
    assert call(amp=None) == EINVAL
    assert call(nmodes=None) == EINVAL
    assert call(kind=None) == EINVAL
    assert call(n=0) == EINVAL
    assert call(n=B.STOCHASTIC_MAX_FIELDS + 1) == EINVAL
    assert call(nmodes=_ints(0, 2)) == EINVAL
    assert call(nmodes=_ints(3, B.STOCHASTIC_MAX_MODES + 1)) == EINVAL
    assert call(kind=_ints(1, 2)) == EINVAL
    assert call(kind=_ints(-1, 0)) == EINVAL
    assert call(coef=(V * 2)(coef[0], None)) == EINVAL
    assert call(coef=(V * 2)(coef[0] + 1, coef[1])) == EINVAL
    assert call(amp=(V * 2)(None, amp[1])) == EINVAL
    assert call(amp=(V * 2)(amp[0] + 4, amp[1])) == EINVAL
    assert call(ktx=None) == EINVAL                          # group 0 is a pair
    assert call(kty=None) == EINVAL
    assert call(ktx=(V * 2)(None, ktx[1])) == EINVAL
    assert call(kty=(V * 2)(kty[0] + 4, None)) == EINVAL
    for sdt in (0.0, -1.0, float("nan"), float("inf")):
        assert call(sdt=sdt) == EINVAL
    if ens:
        assert call(members=0) == EINVAL
        assert call(members=B.ENSEMBLE_MAX_MEMBERS + 1) == EINVAL
        assert call(subs=None) == EINVAL
        assert call(coef_sm=11) == EINVAL                    # the pair writes 4 x 3 values
        assert call(amp_sm=2) == EINVAL                      # neither 0 nor >= 3 modes
        assert call(amp_sm=-3) == EINVAL


def test_stochastic_values(swmhd):
    S = swmhd
    E = S._lib.SwmhdError
    s = S.StochasticForcing(0.5, 8, 1.0, seed=2 ** 64 - 1, stream=2 ** 32 - 1)
    assert (s.rate, s.k_f, s.dk, s.seed, s.stream) == (0.5, 8.0, 1.0, 2 ** 64 - 1, 2 ** 32 - 1)
    one = S.StochasticForcing([0.1, 0.0, 0.3], 8, 1, seed=3, stream=5).for_member(2)
    assert (one.rate, one.seed, one.stream) == (0.3, 3, 7)
    assert s.for_member(1).stream == 0                       # mod 2^32
    for kw in (dict(rate=-1.0), dict(rate=float("nan")), dict(rate=[[1.0]]), dict(rate=lambda x: 1.0), dict(k_f=0.0), dict(k_f=float("inf")),
               dict(dk=-1.0), dict(dk="x"), dict(seed=-1), dict(seed=2 ** 64), dict(seed=1.5), dict(stream=2 ** 32), dict(stream=-1)):
        with pytest.raises(E, match="StochasticForcing"):
            S.StochasticForcing(**{**dict(rate=0.1, k_f=8.0, dk=1.0), **kw})


def test_constructor_refusals_before_any_device(swmhd, monkeypatch):
    S = swmhd
    E = S._lib.SwmhdError
    import swmhd_amd.ensemble as ens_mod
    import swmhd_amd.model as model_mod

    def no_allocation(*a, **k):
        raise AssertionError("allocated before the refusal")
    monkeypatch.setattr(model_mod, "Field", no_allocation)
    monkeypatch.setattr(ens_mod.torch, "zeros", no_allocation)
    TP = 2 * np.pi
    g = S.RectilinearGrid(size=(16, 16), x=(0, TP), y=(0, TP))
    s = S.StochasticForcing(0.1, 4.0, 1.0)
    stir = {"u": s, "v": s}
    # any Bounded direction
    for topo in (("Bounded", "Periodic", "Flat"), ("Periodic", "Bounded", "Flat"), ("Bounded", "Bounded", "Flat")):
        gb = S.RectilinearGrid(size=(16, 16), x=(0, TP), y=(0, TP), topology=topo)
        with pytest.raises(E, match="SWMHD_ENOTSUP"):
            S.ShallowWaterModel(gb, forcing=stir)
        with pytest.raises(E, match="SWMHD_ENOTSUP"):
            S.ShallowWaterModel(gb, forcing={"A": s})
        with pytest.raises(E, match="SWMHD_ENOTSUP"):
            S.BoundedShallowWaterEnsemble(gb, 2, forcing=stir)
        with pytest.raises(E, match="SWMHD_ENOTSUP"):
            S.ShallowWaterEnsemble(gb, 2, forcing=stir)
    # fused=False, ring=, several slab ranks
    with pytest.raises(E, match="SWMHD_ENOTSUP"):
        S.ShallowWaterModel(g, forcing=stir, fused=False)
    with pytest.raises(E, match="SWMHD_ENOTSUP"):
        S.ShallowWaterModel(g, forcing=stir, ring=ctypes.c_void_p(1))
    with pytest.raises(E, match="SWMHD_ENOTSUP"):
        S.ShallowWaterModel(S.RectilinearGrid(size=(16, 8), x=(0, TP), y=(0, TP), j_offset=0, Ny_global=16), forcing=stir,
                            decomp=S.SlabDecomposition(16, 2, 0))
    for cls, args in ((S.ShallowWaterModel, (g,)), (S.ShallowWaterEnsemble, (g, 2))):
        # the vortical kind on uh, vh
        with pytest.raises(E, match="SWMHD_ENOTSUP"):
            cls(*args, formulation=S.ConservativeFormulation, forcing={"uh": s, "vh": s})
        # one momentum name without the other, or two objects
        with pytest.raises(E, match="one name without the other"):
            cls(*args, forcing={"u": s})
        with pytest.raises(E, match="SAME object"):
            cls(*args, forcing={"u": s, "v": S.StochasticForcing(0.1, 4.0, 1.0)})
        with pytest.raises(E, match="share one seed"):
            cls(*args, forcing={"u": s, "v": s, "A": S.StochasticForcing(0.1, 4.0, 1.0, seed=1)})
        # the wrong type still says what a value may be
        with pytest.raises(E, match="a Relaxation"):
            cls(*args, forcing={"u": 0.1})
        with pytest.raises(E, match="a Relaxation"):
            cls(*args, forcing={"u": (s, 0.1)})
        with pytest.raises(E, match="at most one of each"):
            cls(*args, forcing={"A": (s, s)})
        with pytest.raises(E, match="at most one of each"):
            cls(*args, forcing={"A": (S.Relaxation(0.1), S.Relaxation(0.2), s)})
        # the ring of modes: empty, or more than SWMHD_STOCHASTIC_MAX_MODES
        with pytest.raises(E, match="0 modes"):
            cls(*args, forcing={"A": S.StochasticForcing(0.1, 40.0, 1.0)})
        with pytest.raises(E, match="modes in the ring"):
            cls(S.RectilinearGrid(size=(64, 64), x=(0, TP), y=(0, TP)), *args[1:], forcing={"A": S.StochasticForcing(0.1, 20.0, 8.0)})
    with pytest.raises(E, match="belong to an ensemble"):
        S.ShallowWaterModel(g, forcing={"A": S.StochasticForcing([0.1, 0.2], 4.0, 1.0)})
    with pytest.raises(E, match="2 rates for 3 members"):
        S.ShallowWaterEnsemble(g, 3, forcing={"A": S.StochasticForcing([0.1, 0.2], 4.0, 1.0)})
