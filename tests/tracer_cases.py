"""Reference of the passive tracers (swmhd_tracers_rk3_* in include/swmhd.h, ShallowWaterModel(tracers=...)) and the cases the tracer
tests run.  numpy + the CPU oracle only.

The oracle has no tracer list, but its tendency of A with the forcing switched off is the tendency of ANY centre field put in the A
slot: tracer_tendency.  RefModel steps (q1, q2, h, A) and the tracers with that call, numpy's U + dt (gamma Gn + zeta G-) in the
precision of the fields, and oracle.fill_halo*; tests/test_tracer_cases_cpu.py pins it bitwise to oracle.time_step before a GPU test
relies on it."""
import numpy as np

import helpers as Hh

H = 3
P, B = 0, 1
GRAV, FCOR = Hh.G, Hh.F
GAMMA = (8.0 / 15.0, 5.0 / 12.0, 3.0 / 4.0)
ZETA = (0.0, -17.0 / 60.0, -5.0 / 12.0)
FORMS = [(1, 1), (0, 2)]            # (formulation, the forcing the reference runs it with)
FORM_NAME = {0: "Conservative", 1: "VectorInvariant"}
# (Nx, Ny, topology): the grids the reference stepper is pinned on and the model tests run
PERIODIC_GRIDS = [(20, 12, (P, P)), (7, 9, (P, P))]
BOUNDED_GRIDS = [(13, 10, (P, B)), (13, 10, (B, P)), (13, 10, (B, B))]
DX, DY = 0.11, 0.13
SENTINEL = -555.5                   # exact in fp32
# the tracer kernel's tile (launch_plan.hpp TRACER_TILE_X / _Y): the stage matrix straddles it
TX, TY = 64, 16
STAGE_SHAPES = [(3, 3), (7, 9), (TX - 1, TY - 1), (TX, TY), (TX + 1, TY + 1), (2 * TX + 1, 9), (3, TY + 1), (2 * TX + 1, TY),
                (TX, 3), (7, TY - 1)]      # diagonal of Nx x Ny plus corners


def grad_A(topo):
    """The gradient condition of the Bounded cases: -0.05 on the south and north side of A where y is Bounded."""
    return (None, None, -0.05, -0.05) if topo[1] == B else None


def fill(O, a, Nx, Ny, topo, face=(False, False), grad=None, dx=DX, dy=DY):
    if topo == (P, P):
        return O.fill_halo_periodic(a, Nx, Ny, H, H)
    return O.fill_halo(a, Nx, Ny, H, H, topo=topo, face=face, grad=grad, dx=dx, dy=dy)


def state(Nx, Ny, form, seed, dtype=np.float64, rough=True):
    """(q1, q2, h, A) parents, halos unfilled: rough random fields as stage_cases.random_fields makes them, or smooth ones."""
    shp = (Ny + 2 * H, Nx + 2 * H)
    r = [np.random.default_rng([seed, k]) for k in range(4)]
    if rough:
        u, v = 0.5 * r[0].standard_normal(shp), 0.5 * r[1].standard_normal(shp)
        h = 1.0 + 0.3 * r[2].random(shp)
        A = r[3].standard_normal(shp)
    else:
        y, x = np.meshgrid(np.arange(shp[0]) * (2 * np.pi / Ny), np.arange(shp[1]) * (2 * np.pi / Nx), indexing="ij")
        u, v = 0.5 * np.cos(x + 0.4) * np.sin(2 * y) + 0.3, -0.4 * np.sin(2 * x) * np.cos(y + 0.2) - 0.2
        h = 1.0 + 0.2 * np.sin(x) * np.cos(y)
        A = 0.3 * np.sin(x + 0.1) * np.sin(y - 0.5)
    q1, q2 = (u, v) if form == 1 else (h * u, h * v)
    return [np.ascontiguousarray(a.astype(dtype)) for a in (q1, q2, h, A)]


def tracer_fields(Nx, Ny, K, seed, dtype=np.float64, rough=True):
    """K distinct tracer parents, halos unfilled: tanh(y) + noise with a different offset, slope and noise stream each."""
    shp = (Ny + 2 * H, Nx + 2 * H)
    y = ((np.arange(shp[0]) - H + 0.5) / Ny - 0.5).reshape(-1, 1) * np.ones(shp)
    out = []
    for k in range(K):
        noise = np.random.default_rng([seed, 100 + k]).standard_normal(shp)
        out.append(np.ascontiguousarray((np.tanh((3 + k) * y) + 0.1 * k + (0.3 if rough else 0.0) * noise).astype(dtype)))
    return out


def fill_state(O, q, Nx, Ny, topo, gradA=None, dx=DX, dy=DY):
    faces = ((True, False), (False, True), (False, False), (False, False))
    for k, a in enumerate(q):
        fill(O, a, Nx, Ny, topo, faces[k], gradA if k == 3 else None, dx, dy)
    return q


def tracer_tendency(O, q, c, Nx, Ny, dx, dy, form, topo=(P, P), nthreads=1):
    """The oracle's tendency of the centre field c advected by (q1, q2, h): its G_A with c in the A slot and no forcing (parent)."""
    return O.tendencies(q[0], q[1], q[2], c, Nx, Ny, H, H, dx, dy, form, O.LORENTZ_NONE, GRAV, FCOR, nthreads=nthreads, topo=topo)[3]


def substep(U, Gn, Gm, Nx, Ny, dt, gamma, zeta, first):
    """rk3_substep! on the interior, in the precision of U (the oracle's expression order): a new parent, halos as U's."""
    t = U.dtype.type
    dt, gamma, zeta = t(dt), t(gamma), t(zeta)
    out = U.copy()
    I = (slice(H, H + Ny), slice(H, H + Nx))
    if first:
        out[I] = U[I] + dt * gamma * Gn[I]
    else:
        out[I] = U[I] + dt * (gamma * Gn[I] + zeta * Gm[I])
    return out


class RefModel:
    """(q1, q2, h, A) and a list of tracers stepped by RK3 as ShallowWaterModel steps them.  q and the tracers are halo-filled parents
    (copied); tgrads[k] = (w, e, s, n) gradient values of tracer k on Bounded sides (None: no flux)."""

    def __init__(self, O, q, tracers, Nx, Ny, form, lor, topo=(P, P), gradA=None, tgrads=None, dx=DX, dy=DY):
        self.O, self.Nx, self.Ny, self.form, self.lor, self.topo, self.gradA, self.dx, self.dy = O, Nx, Ny, form, lor, topo, gradA, dx, dy
        self.q = [a.copy() for a in q]
        self.tr = [a.copy() for a in tracers]
        self.tgrads = list(tgrads) if tgrads is not None else [None] * len(self.tr)
        self.Gm = self.tGm = None

    def step(self, dt):
        O, Nx, Ny = self.O, self.Nx, self.Ny
        for s in range(3):
            G = O.tendencies(*self.q, Nx, Ny, H, H, self.dx, self.dy, self.form, self.lor, GRAV, FCOR, topo=self.topo)
            tG = [tracer_tendency(O, self.q, c, Nx, Ny, self.dx, self.dy, self.form, self.topo) for c in self.tr]
            new = [substep(U, g, self.Gm[k] if s else None, Nx, Ny, dt, GAMMA[s], ZETA[s], s == 0) for k, (U, g) in enumerate(zip(self.q, G))]
            self.tr = [fill(O, substep(c, g, self.tGm[k] if s else None, Nx, Ny, dt, GAMMA[s], ZETA[s], s == 0), Nx, Ny, self.topo,
                            grad=self.tgrads[k], dx=self.dx, dy=self.dy) for k, (c, g) in enumerate(zip(self.tr, tG))]
            self.q = fill_state(O, new, Nx, Ny, self.topo, self.gradA, self.dx, self.dy)
            self.Gm, self.tGm = G, tG
        return self
