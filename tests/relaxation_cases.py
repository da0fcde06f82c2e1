"""Reference of the Relaxation forcing (swmhd_relaxation_rk3_* in include/swmhd_relaxation.h, ShallowWaterModel(forcing=...)) and the
cases its tests run.  numpy + the CPU oracle only.

Oceananigans is not on this machine: the pin is the written formula, restated here.
    p = rate mask (no mask: p = rate),  d = target - phi,  D = p d                                                     (relax_strict)
in the precision of the field, one rounding per operation, in that order -- Oceananigans' rate * mask * (target - phi) evaluated left to
right; relax_exact is the same value in longdouble with the scale S of its rounding error.  The engine adds D to what the stage kernels
wrote: new += a D, acc += w D (correct).  RefModel steps the state and the tracers as tests/tracer_cases.RefModel does -- oracle
tendencies, numpy update, oracle halo fill, Periodic and Bounded directions -- and puts the forcing in by that correction ("classic",
the engine's strict schedule and its schedule on Bounded grids; "anchor", its fast periodic schedule in numpy), after the corrections
of a y-dependent Coriolis parameter and of the two closures where those are on, in the engine's launch order."""
import numpy as np

import biharmonic_cases as BC
import coriolis_cases as CC
import diffusion_cases as DC
import tracer_cases as T

H = T.H
GAMMA, ZETA = T.GAMMA, T.ZETA
ANCHOR_WEIGHT = 0.25
DX, DY = T.DX, T.DY
SENTINEL = T.SENTINEL
MAX_FIELDS = 12                     # SWMHD_RELAXATION_MAX_FIELDS

# ---- the stage matrix: the geometry of the strip-march launches, read from strip_cases -------------------------------------------------
from strip_cases import TILE_ROWS, row_ranges, wave_columns      # noqa: F401,E402
from strip_cases import stage_shapes as strip_stage_shapes      # noqa: E402

# wave segments of exactly 2 and 4 rows: the two-buffer march (csrc/strip_device.inc strip_pipeline) ends in its even tail without a
# steady trip, and after exactly one
SHORT_SHAPES = [(3, 2), (3, 4)]


def stage_shapes(itemsize, aligned):
    return strip_stage_shapes(itemsize, aligned) + SHORT_SHAPES


# the six kinds of a field: (has a mask array, target "zero" (the default 0) | "scalar" | "array")
FIELD_KINDS = [(m, t) for m in (False, True) for t in ("zero", "scalar", "array")]
NFIELDS = (1, 4, MAX_FIELDS)


def kind_of(k):
    """The kind of field k of a call of the stage matrix: the six kinds in turn, so that 4 fields hold four of them and 12 all, twice."""
    return FIELD_KINDS[(k + 2) % 6]      # (one field: kind 2, a scalar target without a mask -- h towards H_eq; field 1 has both arrays)


# ---- the term -------------------------------------------------------------------------------------------------------------------------
def relax_strict(old, rate, mask, target):
    """D on the cells of `old`, in its precision and the strict operation order.  mask: None or an array; target: a scalar or an array."""
    t = old.dtype.type
    p = t(rate) * mask if mask is not None else t(rate)
    d = (target if isinstance(target, np.ndarray) else t(target)) - old
    return p * d


def relax_exact(old, rate, mask, target):
    """(D, S) in longdouble from the values ROUNDED to the precision of `old` (what the kernel is given):
    S = |rate| |mask| (|t| + |old|)."""
    t, L = old.dtype.type, np.longdouble
    r = L(t(rate))
    m = mask.astype(L) if mask is not None else L(1)
    tt = target.astype(L) if isinstance(target, np.ndarray) else L(t(target))
    o = old.astype(L)
    return r * m * (tt - o), abs(r) * np.abs(m) * (np.abs(tt) + np.abs(o))


# Fast tolerance, derived (include/swmhd_relaxation.h).  The kernel's expression is the strict one; a fast object may fuse a D + new.
# D: the product rate mask, the difference t - old and their product, three roundings of at most eps/2 relative to partial results that S
# bounds: |D - D_exact| <= ((1 + eps/2)^3 - 1) S <= 2 eps S.  new = new_0 + a D: the rounding of a D where it is not fused and the
# rounding of the result (eps/2 |ref|): five roundings, ((1 + eps/2)^5 - 1) |a| S <= 4 eps |a| S -- the chain of coriolis_cases.
D_ROUNDINGS = 2
UPDATE_ROUNDINGS = 4


def correct(out, D, a):
    """out + a D in the precision of out, the product rounded before the sum (strict order)."""
    t = out.dtype.type
    return out + t(a) * D


def fast_bound_D(S, eps):
    """|D - D_exact| <= 2 eps S."""
    return D_ROUNDINGS * eps * S


def fast_bound(ref, a, S, eps):
    """|got - ref| <= eps |ref| + 4 eps |a| S for ref = out_0 + a D_exact (longdouble)."""
    return eps * np.abs(ref) + abs(np.longdouble(a)) * UPDATE_ROUNDINGS * eps * S


# ---- the reference stepper -------------------------------------------------------------------------------------------------------------
class RefModel:
    """(q1, q2, h, A) and tracers through RK3 with a forcing.  relax: one entry per field of the 4 + K, None or (rate, mask, target) with
    mask None or an interior array (Ny, Nx) and target a scalar or such an array, in the precision of the fields.  mode: "classic" |
    "anchor" (module docstring).  topo: Periodic and Bounded directions, filled by tracer_cases.fill / fill_state; q and tracers are
    halo-filled parents.  Optional, Periodic grids only, applied BEFORE the forcing in the engine's launch order: rows = (fc, ff) of a
    y-dependent Coriolis parameter (the oracle then runs with f = 0), coef and coef4 the Laplacian and the biharmonic coefficients of the
    4 + K fields."""

    def __init__(self, O, q, tracers, relax, Nx, Ny, form, lor, mode="classic", topo=(T.P, T.P), gradA=None, dx=DX, dy=DY, rows=None,
                 coef=None, coef4=None, grav=T.GRAV, fcor=T.FCOR):
        n = 4 + len(tracers)
        assert len(relax) == n
        self.O, self.Nx, self.Ny, self.form, self.lor, self.mode, self.dx, self.dy = O, Nx, Ny, form, lor, mode, dx, dy
        self.topo, self.gradA, self.grav, self.fcor = topo, gradA, grav, fcor
        self.q = [a.copy() for a in q]
        self.tr = [a.copy() for a in tracers]
        self.relax = list(relax)
        self.rows = rows
        self.coef = list(coef) if coef is not None else [0.0] * n
        self.coef4 = list(coef4) if coef4 is not None else [0.0] * n
        periodic = topo == (T.P, T.P)
        assert mode in ("classic", "anchor") and (mode == "classic" or periodic)      # (the engine runs Bounded grids in the classic form)
        assert periodic or (rows is None and not any(self.coef) and not any(self.coef4))
        self.Gm = None
        self.I = (slice(H, H + Ny), slice(H, H + Nx))

    def _D(self, U):
        """Per field, the correction terms of the current state in the launch order: Coriolis, Laplacian, biharmonic, relaxation."""
        Nx, Ny, I = self.Nx, self.Ny, self.I
        out = [[] for _ in U]
        if self.rows is not None:
            t = U[0].dtype.type
            P1, P2 = (DC.pad1(f, Nx, Ny, H, H, False, False) for f in U[:2])
            for k, d in enumerate(CC.coriolis_strict(P1, P2, np.asarray(self.rows[0], dtype=t), np.asarray(self.rows[1], dtype=t))):
                out[k].append(d)
        for k, f in enumerate(U):
            if self.coef[k] != 0:
                out[k].append(DC.laplacian_strict(DC.pad1(f, Nx, Ny, H, H, False, False), self.coef[k], self.dx, self.dy))
            if self.coef4[k] != 0:
                out[k].append(BC.biharmonic_strict(BC.pad2(f, Nx, Ny, H, H, False, False), self.coef4[k], self.dx, self.dy))
            if self.relax[k] is not None and self.relax[k][0] != 0:
                out[k].append(relax_strict(f[I], *self.relax[k]))
        return out

    def step(self, dt):
        O, Nx, Ny, I = self.O, self.Nx, self.Ny, self.I
        for s in range(3):
            U = self.q + self.tr
            f = 0.0 if self.rows is not None else self.fcor
            G = list(O.tendencies(*self.q, Nx, Ny, H, H, self.dx, self.dy, self.form, self.lor, self.grav, f, topo=self.topo))
            G += [T.tracer_tendency(O, self.q, c, Nx, Ny, self.dx, self.dy, self.form, self.topo) for c in self.tr]
            D = self._D(U)
            if self.mode == "classic":         # the stage kernels' update, then per launch new += dt gamma D and, in storing stages, Gn += D
                new = [T.substep(u, g, self.Gm[k] if s else None, Nx, Ny, dt, GAMMA[s], ZETA[s], s == 0) for k, (u, g) in enumerate(zip(U, G))]
                for n, g, ds in zip(new, G, D):
                    for d in ds:
                        n[I] = correct(n[I], d, dt * GAMMA[s])
                        if s < 2:
                            g[I] = correct(g[I], d, 1.0)
            else:                              # anchor: U1 = U0 + dt g1 G0, W = U0 + (dt/4) G0, U2 = W + dt g2 G1, U3 = W + dt g3 G2
                new = []
                for k, (u, g, ds) in enumerate(zip(U, G, D)):
                    t = u.dtype.type
                    base = u if s == 0 else self.Gm[k]
                    n = u.copy()
                    n[I] = base[I] + t(dt * GAMMA[s]) * g[I]
                    if s == 0:
                        w = u.copy()
                        w[I] = u[I] + t(dt * ANCHOR_WEIGHT) * g[I]
                    for d in ds:
                        n[I] = correct(n[I], d, dt * GAMMA[s])
                        if s == 0:
                            w[I] = correct(w[I], d, dt * ANCHOR_WEIGHT)
                    new.append(n)
                    G[k] = w if s == 0 else self.Gm[k]     # W travels where G- does
            self.q = T.fill_state(O, new[:4], Nx, Ny, self.topo, self.gradA, self.dx, self.dy)
            self.tr = [T.fill(O, c, Nx, Ny, self.topo, dx=self.dx, dy=self.dy) for c in new[4:]]
            self.Gm = G
        return self


# ---- the RK3 property ------------------------------------------------------------------------------------------------------------------
# f = 0, A = 0, uniform h, uniform u = u0, v = 0 on an 8 x 8 periodic grid: every advective tendency is a difference of equal values
# and exactly zero, so drag r on u makes every step u <- P(-r dt) u with P(z) = 1 + z + z²/2 + z³/6, the RK3 polynomial.  Likewise
# (h - H_eq) under Relaxation(r, target=H_eq) on h with u = v = 0.
DECAY_NX, DECAY_NY, DECAY_STEPS = 8, 8, 20
DECAY_RATE, DECAY_DT = 0.5, 0.05
DECAY_U0, DECAY_H = 0.3, 1.0                # the drag case: u = u0, h = 1
DECAY_H0, DECAY_HEQ = 1.25, 1.0             # the thermal case: h = h0 relaxing to H_eq
# max |x_20 / x_0 - P(z)^20| / P(z)^20 of RefModel("classic") in float64 against the longdouble value, x = u (drag) and x = h - H_eq
# (thermal), as tests/test_relaxation_cases_cpu.py computes and prints them: rounding of 60 stages of a scalar map (the thermal case
# also rounds h - H_eq near 1).  The margin of every decay test -- strict and fast, reference and device -- is ten times this, the
# margin diffusion_cases uses for its eigenmode; the fast schedule gets nothing on top of it.
DECAY_REFERENCE_DEVIATION = {"drag": 2.671e-16, "thermal": 1.982e-15}
DECAY_MARGIN = {k: 10 * v for k, v in DECAY_REFERENCE_DEVIATION.items()}


def decay_polynomial(steps=DECAY_STEPS):
    """P(z)^steps in longdouble, z = -(rate dt) with both as float64 values."""
    L = np.longdouble
    z = -L(DECAY_RATE) * L(DECAY_DT)
    return (1 + z + z * z / 2 + z ** 3 / 6) ** steps


def decay_case(which, dtype=np.float64):
    """(q, relax): the parents (u, v, h, A) of the drag or the thermal case (uniform fields: their halos are filled) and RefModel's
    relax list."""
    shp = (DECAY_NY + 2 * H, DECAY_NX + 2 * H)
    if which == "drag":
        q = [np.full(shp, DECAY_U0), np.zeros(shp), np.full(shp, DECAY_H), np.zeros(shp)]
        relax = [(DECAY_RATE, None, 0.0), None, None, None]
    else:
        q = [np.zeros(shp), np.zeros(shp), np.full(shp, DECAY_H0), np.zeros(shp)]
        relax = [None, None, (DECAY_RATE, None, DECAY_HEQ), None]
    return [np.ascontiguousarray(a.astype(dtype)) for a in q], relax


def decay_deviation(which, field, steps=DECAY_STEPS):
    """max |x_n / x_0 - P^n| / P^n over the interior of `field` (u or h after `steps` steps), in longdouble."""
    L = np.longdouble
    I = (slice(H, H + DECAY_NY), slice(H, H + DECAY_NX))
    x = field[I].astype(L)
    ratio = x / L(DECAY_U0) if which == "drag" else (x - L(DECAY_HEQ)) / (L(DECAY_H0) - L(DECAY_HEQ))
    Pn = decay_polynomial(steps)
    return float(np.abs(ratio - Pn).max() / Pn)

