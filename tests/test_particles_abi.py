"""CPU tests (no GPU) of the Lagrangian particles: the entry points of include/swmhd_particles.h are exported and declared, every
argument error comes back with its code before any HIP call, in the documented order, and the Python classes refuse what they do not
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
V = ctypes.c_void_p


def _ptrs(n):
    buf = (ctypes.c_double * 64)()
    return buf, [ctypes.addressof(buf) + 8 * k for k in range(n)]


def test_particle_symbols_are_exported(swmhd):
    B = swmhd._lib
    L = B.lib()
    assert B.PARTICLES_EXPORTS == [f"swmhd_{n}_{s}" for s in ("f64", "f32")
                                   for n in ("particles_rk3", "ensemble_particles_rk3", "particles_sample", "ensemble_particles_sample")]
    header = open(os.path.join(ROOT, "include", "swmhd_particles.h")).read()
    for name in B.PARTICLES_EXPORTS:
        assert hasattr(L, name)
        assert re.search(rf"^int {name}\(", header, flags=re.M), name
    assert sorted(re.findall(r"^int (swmhd_\w+)\(", header, flags=re.M)) == sorted(B.PARTICLES_EXPORTS)
    assert '#include "swmhd_particles.h"' in open(os.path.join(ROOT, "include", "swmhd.h")).read()
    assert re.search(rf"^#define SWMHD_PARTICLES_BLOCK {B.PARTICLES_BLOCK}$", header, flags=re.M)
    assert re.search(r"^#define SWMHD_PARTICLES_MAX_FIELDS 12$", header, flags=re.M) and B.PARTICLES_MAX_FIELDS == 12 == 4 + B.MAX_TRACERS
    assert re.search(r"^#define SWMHD_PARTICLES_CENTER_X 1$", header, flags=re.M) and re.search(r"^#define SWMHD_PARTICLES_CENTER_Y 2$", header, flags=re.M)
    assert (B.PARTICLES_CENTER_X, B.PARTICLES_CENTER_Y) == (1, 2)
    assert L.swmhd_version() == 300          # symbols added, none changed
    for other in (B.EXPORTS, B.SOURCE_EXPORTS, B.STOCHASTIC_EXPORTS):
        assert not set(B.PARTICLES_EXPORTS) & set(other)


@pytest.mark.parametrize("ens", [False, True], ids=["single", "ensemble"])
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_particles_rk3_return_codes(swmhd, sfx, ens):
    B = swmhd._lib
    L = B.lib()
    _keep, (q1, q2, h, x, y, gx, gy, par) = _ptrs(8)
    fn = getattr(L, f"swmhd_{'ensemble_' if ens else ''}particles_rk3_{sfx}")
    nan, inf = float("nan"), float("inf")

    def call(q1=q1, q2=q2, h=h, x=x, y=y, gx=gx, gy=gy, P=5, members=2, stride_m=(Ny + 2 * H) * SY, nx=Nx, ny=Ny, Hx=H, Hy=H, sy=SY,
             x0=0.0, y0=0.0, dx=0.5, dy=0.25, form=B.VECTOR_INVARIANT, params=None, dt=0.01, gamma=0.5, zeta=-0.25, flags=0):
        if ens:
            return fn(q1, q2, h, x, y, gx, gy, P, members, stride_m, nx, ny, Hx, Hy, sy, x0, y0, dx, dy, form, params, dt, gamma, zeta, flags, None)
        return fn(q1, q2, h, x, y, gx, gy, P, nx, ny, Hx, Hy, sy, x0, y0, dx, dy, form, dt, gamma, zeta, flags, None)
    # null pointers; two of the particle arrays the same
    for name in ("q1", "q2", "x", "y", "gx", "gy"):
        assert call(**{name: None}) == EINVAL, name
    assert call(y=x) == EINVAL and call(gx=x) == EINVAL and call(gy=gx) == EINVAL and call(gy=y) == EINVAL
    # extents, pitch, spacing, origin
    assert call(nx=0) == EINVAL
    assert call(ny=-1) == EINVAL
    assert call(Hx=-1) == EINVAL
    assert call(sy=Nx + 2 * H - 1) == EINVAL
    for bad in (0.0, -1.0, nan, inf):
        assert call(dx=bad) == EINVAL and call(dy=bad) == EINVAL, bad
    for bad in (nan, inf, -inf):
        assert call(x0=bad) == EINVAL and call(y0=bad) == EINVAL, bad
    # unknown flags; a direction Bounded and wrapped
    assert call(flags=8) == EINVAL
    assert call(flags=1 << 20) == EINVAL
    assert call(flags=B.BOUNDED_X | B.WRAP_X) == EINVAL
    assert call(flags=B.BOUNDED_Y | B.WRAP_Y | B.WRAP_X) == EINVAL
    # the count, the stage's scalars, the formulation, h for the conservative form
    assert call(P=-1) == EINVAL
    for name in ("dt", "gamma", "zeta"):
        assert call(**{name: nan}) == EINVAL and call(**{name: inf}) == EINVAL, name
    assert call(form=2) == EINVAL and call(form=-1) == EINVAL
    assert call(form=B.CONSERVATIVE, h=None) == EINVAL
    if ens:
        assert call(members=0) == EINVAL
        assert call(members=B.ENSEMBLE_MAX_MEMBERS + 1) == EINVAL
        assert call(stride_m=(Ny + 2 * H) * SY - 1) == EINVAL
    # EINVAL comes before the other answers
    assert call(P=-1, flags=B.TILE_KERNEL) == EINVAL
    assert call(gamma=nan, Hx=0, sy=SY) == EINVAL
    # known flags this family does not take
    for fl in (B.MARCH_KERNEL, B.TILE_KERNEL, B.GM_IS_PREV_STATE, B.OPEN_SOUTH, B.OPEN_NORTH | B.BOUNDED_Y, B.LEAVE_ROOM, B.RK3_ANCHOR,
               B.RK3_ANCHOR | B.WRAP_X | B.WRAP_Y):
        assert call(flags=fl) == ENOTSUP, fl
    assert call(flags=B.RK3_ANCHOR, Hx=0) == ENOTSUP          # ENOTSUP before EHALO
    # a filled halo of depth >= 1 unless that direction is wrapped
    assert call(Hx=0) == EHALO
    assert call(Hy=0) == EHALO
    assert call(Hx=0, flags=B.WRAP_Y) == EHALO
    assert call(Hy=0, flags=B.WRAP_X) == EHALO
    assert call(Hy=0, flags=B.BOUNDED_Y | B.WRAP_X) == EHALO
    assert call(Hx=0, P=0) == EHALO                           # before "nothing to do"
    # accepted, nothing to enqueue: P == 0 with every accepted flag; h may be NULL for the vector-invariant form
    for fl in (0, B.STRICT, B.WRAP_X | B.WRAP_Y, B.STRICT | B.WRAP_X, B.BOUNDED_X, B.BOUNDED_Y | B.WRAP_X, B.BOUNDED_X | B.BOUNDED_Y | B.STRICT):
        assert call(P=0, flags=fl) == 0, fl
    assert call(P=0, Hx=0, Hy=0, flags=B.WRAP_X | B.WRAP_Y) == 0
    assert call(P=0, h=None) == 0
    assert call(P=0, form=B.CONSERVATIVE) == 0
    assert call(P=0, zeta=0.0, gamma=0.0, dt=0.0) == 0
    if ens:
        assert call(P=0, params=par) == 0
    # 2^31 workgroups or more: refused before any HIP call, with the negated HIP error of an invalid configuration (9)
    assert call(P=B.PARTICLES_BLOCK << 31) == -9
    assert call(P=(B.PARTICLES_BLOCK << 31) - B.PARTICLES_BLOCK + 1) == -9
    if ens:
        assert call(P=B.PARTICLES_BLOCK << 30, members=2) == -9


@pytest.mark.parametrize("ens", [False, True], ids=["single", "ensemble"])
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_particles_sample_return_codes(swmhd, sfx, ens):
    B = swmhd._lib
    L = B.lib()
    _keep, ptrs = _ptrs(16)
    x, y, out = ptrs[13:16]
    fields = (V * 12)(*ptrs[:12])
    loc = (ctypes.c_int * 12)(*([0, 1, 2, 3] * 3))
    fn = getattr(L, f"swmhd_{'ensemble_' if ens else ''}particles_sample_{sfx}")
    nan, inf = float("nan"), float("inf")

    def call(fields=fields, loc=loc, n=3, x=x, y=y, out=out, P=5, members=2, stride_m=(Ny + 2 * H) * SY, nx=Nx, ny=Ny, Hx=H, Hy=H, sy=SY,
             x0=0.0, y0=0.0, dx=0.5, dy=0.25, flags=0):
        if ens:
            return fn(fields, loc, n, x, y, out, P, members, stride_m, nx, ny, Hx, Hy, sy, x0, y0, dx, dy, flags, None)
        return fn(fields, loc, n, x, y, out, P, nx, ny, Hx, Hy, sy, x0, y0, dx, dy, flags, None)
    for name in ("fields", "loc", "x", "y", "out"):
        assert call(**{name: None}) == EINVAL, name
    assert call(n=0) == EINVAL and call(n=B.PARTICLES_MAX_FIELDS + 1) == EINVAL
    assert call(fields=(V * 3)(ptrs[0], None, ptrs[2])) == EINVAL
    assert call(loc=(ctypes.c_int * 3)(0, 4, 1)) == EINVAL and call(loc=(ctypes.c_int * 3)(-1, 0, 1)) == EINVAL
    assert call(out=x) == EINVAL and call(out=y) == EINVAL
    assert call(nx=0) == EINVAL and call(Hy=-1) == EINVAL and call(sy=Nx + 2 * H - 1) == EINVAL
    for bad in (0.0, -1.0, nan, inf):
        assert call(dx=bad) == EINVAL and call(dy=bad) == EINVAL, bad
    assert call(x0=nan) == EINVAL and call(y0=inf) == EINVAL
    assert call(flags=8) == EINVAL and call(flags=B.BOUNDED_X | B.WRAP_X) == EINVAL
    assert call(P=-1) == EINVAL
    if ens:
        assert call(members=0) == EINVAL
        assert call(members=B.ENSEMBLE_MAX_MEMBERS + 1) == EINVAL
        assert call(stride_m=(Ny + 2 * H) * SY - 1) == EINVAL
    assert call(P=-1, flags=B.MARCH_KERNEL) == EINVAL
    for fl in (B.MARCH_KERNEL, B.TILE_KERNEL, B.GM_IS_PREV_STATE, B.OPEN_SOUTH, B.OPEN_NORTH, B.LEAVE_ROOM, B.RK3_ANCHOR):
        assert call(flags=fl) == ENOTSUP, fl
    assert call(flags=B.LEAVE_ROOM, Hy=0) == ENOTSUP
    assert call(Hx=0) == EHALO and call(Hy=0) == EHALO
    assert call(Hx=0, flags=B.WRAP_Y) == EHALO and call(Hy=0, flags=B.WRAP_X) == EHALO
    assert call(Hy=0, P=0) == EHALO
    for fl in (0, B.STRICT, B.WRAP_X | B.WRAP_Y, B.BOUNDED_X | B.BOUNDED_Y, B.BOUNDED_Y | B.WRAP_X):
        assert call(P=0, flags=fl) == 0, fl
    assert call(P=0, n=B.PARTICLES_MAX_FIELDS) == 0
    assert call(P=0, Hx=0, Hy=0, flags=B.WRAP_X | B.WRAP_Y) == 0
    assert call(P=B.PARTICLES_BLOCK << 31) == -9


def test_lagrangian_particles_values(swmhd):
    S = swmhd
    E = S._lib.SwmhdError
    from swmhd_amd.particles import fold_periodic
    for bad in (([0.0, 1.0], [0.0]), (0.5, 0.5), (np.zeros((2, 2, 2)), np.zeros((2, 2, 2)))):
        with pytest.raises(E, match="LagrangianParticles"):
            S.LagrangianParticles(*bad)
    p = S.LagrangianParticles([0.1, 0.2, 0.3], [0.0, 0.5, 1.0], tracked_fields="A")
    assert p.P == 3 and p.tracked_fields == ("A",)
    g = S.RectilinearGrid(size=(8, 4), x=(-1.0, 1.0), y=(0.0, 2.0))
    x = np.array([-1.0, 0.25, 1.0, 1.5, -3.25, 7.0, np.nan, 1e300])
    got = fold_periodic(x, -1.0, 8 * g.dx)
    np.testing.assert_array_equal(got[:6], [-1.0, 0.25, -1.0, -0.5, 0.75, -1.0])
    assert np.isnan(got[6]) and -1.0 <= got[7] <= 1.0
    xs, ys = S.LagrangianParticles(x[:6], np.zeros(6)).check(g, ("u", "v", "h", "A"), ())
    np.testing.assert_array_equal(xs, got[:6])
    xs, _ = S.LagrangianParticles([0.5, 1.5], [0.0, 0.0]).check(g, ("u", "v", "h", "A"), (), members=3)
    assert xs.shape == (3, 2) and np.array_equal(xs[2], [0.5, -0.5])
    with pytest.raises(E, match=r"\(P,\) or \(3, P\)"):
        S.LagrangianParticles(np.zeros((2, 4)), np.zeros((2, 4))).check(g, ("u", "v", "h", "A"), (), members=3)
    with pytest.raises(E, match="one array of P"):
        S.LagrangianParticles(np.zeros((2, 4)), np.zeros((2, 4))).check(g, ("u", "v", "h", "A"), ())
    with pytest.raises(E, match="tracked field 'c'"):
        S.LagrangianParticles([0.0], [0.0], tracked_fields=("A", "c")).check(g, ("u", "v", "h", "A"), ("d",))


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
    P = lambda **kw: S.LagrangianParticles([0.25, 0.5], [0.5, 0.75], **kw)
    with pytest.raises(E, match="SWMHD_ENOTSUP"):
        S.ShallowWaterModel(g, particles=P(), fused=False)
    with pytest.raises(E, match="SWMHD_ENOTSUP"):
        S.ShallowWaterModel(g, particles=P(), ring=ctypes.c_void_p(1))
    with pytest.raises(E, match="SWMHD_ENOTSUP"):
        S.ShallowWaterModel(S.RectilinearGrid(size=(16, 8), x=(0, 1), y=(0, 1), j_offset=0, Ny_global=16), particles=P(),
                            decomp=S.SlabDecomposition(16, 2, 0))
    for topo in (("Bounded", "Periodic", "Flat"), ("Periodic", "Bounded", "Flat"), ("Bounded", "Bounded", "Flat")):
        gb = S.RectilinearGrid(size=(16, 16), x=(0, 1), y=(0, 1), topology=topo)
        with pytest.raises(E, match="SWMHD_ENOTSUP"):
            S.BoundedShallowWaterEnsemble(gb, 2, particles=P())
        with pytest.raises(E, match="SWMHD_ENOTSUP"):
            S.ShallowWaterEnsemble(gb, 2, particles=P())
        # initial positions outside a Bounded domain
        bad = S.LagrangianParticles([0.5, 1.25], [0.5, 0.5]) if topo[0] == "Bounded" else S.LagrangianParticles([0.5, 0.5], [-0.01, 0.5])
        with pytest.raises(E, match="outside the Bounded domain"):
            S.ShallowWaterModel(gb, particles=bad)
        with pytest.raises(E, match="outside the Bounded domain"):
            S.ShallowWaterModel(gb, particles=S.LagrangianParticles([0.5, np.nan], [np.nan, 0.5]))
    for cls, args in ((S.ShallowWaterModel, (g,)), (S.ShallowWaterEnsemble, (g, 2))):
        with pytest.raises(E, match="particles: a LagrangianParticles"):
            cls(*args, particles=([0.5], [0.5]))
        with pytest.raises(E, match="tracked field 'c'"):
            cls(*args, particles=P(tracked_fields=("c",)))
        with pytest.raises(E, match="tracked field 'u'"):
            cls(*args, formulation=S.ConservativeFormulation, particles=P(tracked_fields=("u",)))
    with pytest.raises(E, match="one array of P"):
        S.ShallowWaterModel(g, particles=S.LagrangianParticles(np.zeros((2, 3)), np.zeros((2, 3))))
    with pytest.raises(E, match=r"\(P,\) or \(2, P\)"):
        S.ShallowWaterEnsemble(g, 2, particles=S.LagrangianParticles(np.zeros((3, 3)), np.zeros((3, 3))))
