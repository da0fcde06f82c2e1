"""Reference of the BetaPlane Coriolis launch (swmhd_coriolis_rk3_* in include/swmhd_coriolis.h, ShallowWaterModel(coriolis=...)) and
the cases its tests run.  numpy + the CPU oracle only.

The pin is the written formula, in the order of the oracle's own Coriolis term (oracle/sw_rhs.inc: vbar, ubar):
    vbar = ((q2[i-1,j] + q2[i,j]) / 2 + (q2[i-1,j+1] + q2[i,j+1]) / 2) / 2        D1 =   fc[j] vbar
    ubar = ((q1[i,j-1] + q1[i+1,j-1]) / 2 + (q1[i,j] + q1[i+1,j]) / 2) / 2        D2 = -(ff[j] ubar)                  (coriolis_strict)
in the precision of the fields, one rounding per operation; coriolis_exact is the same value in longdouble with the scale S = the mean
of the four absolute values.  The engine runs its stage kernels with f = 0 and adds D to what they wrote: new += a D, acc += w D
(diffusion_cases.correct).  RefModel steps the state as tests/tracer_cases.RefModel does -- oracle tendencies with fcor = 0, numpy
update, oracle halo fill, Periodic and Bounded -- and puts the term in by that correction ("classic", the engine's strict schedule;
"anchor", its fast schedule in numpy) or by adding D to the tendency before the update ("tendency": what Oceananigans does).
tests/test_coriolis_cases_cpu.py holds the three against each other and against the oracle's own scalar f."""
import numpy as np

import diffusion_cases as DC
import tracer_cases as T

H = T.H
GAMMA, ZETA = T.GAMMA, T.ZETA
ANCHOR_WEIGHT = 0.25
DX, DY = T.DX, T.DY
SENTINEL = T.SENTINEL
pad1, correct = DC.pad1, DC.correct

# ---- the stage matrix -----------------------------------------------------------------------------------------------------------------
from strip_cases import TILE_ROWS, row_ranges, stage_shapes, wave_columns      # noqa: F401  (shared with the other strip-march launch)


def row_values(Ny, dtype, seed=0):
    """(fc, ff): a distinct value for every row and for its face, as the call receives them (rounded to dtype)."""
    j = np.arange(Ny)
    fc = 0.7 + 0.031 * (j + 0.5) + 0.003 * seed
    ff = 0.7 + 0.031 * j + 0.003 * seed
    return fc.astype(dtype), ff.astype(dtype)


# ---- the operator ---------------------------------------------------------------------------------------------------------------------
def _corners(P1, P2):
    """The four values of vbar (q2: west and centre of row j, west and centre of row j + 1) and of ubar (q1: centre and east of row
    j - 1, centre and east of row j) on the cells of pad1's arrays."""
    v = (P2[1:-1, :-2], P2[1:-1, 1:-1], P2[2:, :-2], P2[2:, 1:-1])
    u = (P1[:-2, 1:-1], P1[:-2, 2:], P1[1:-1, 1:-1], P1[1:-1, 2:])
    return v, u


def coriolis_strict(P1, P2, fc, ff):
    """(D1, D2) on the cells of pad1's arrays of q1, q2, in their precision and the strict operation order."""
    t = P1.dtype.type
    two = t(2)
    fc, ff = np.asarray(fc, dtype=t)[:, None], np.asarray(ff, dtype=t)[:, None]
    v, u = _corners(P1, P2)
    vbar = ((v[0] + v[1]) / two + (v[2] + v[3]) / two) / two
    ubar = ((u[0] + u[1]) / two + (u[2] + u[3]) / two) / two
    return fc * vbar, -(ff * ubar)


def coriolis_fast_order(P1, P2, fc, ff):
    """(D1, D2) in the operation order of the fast build, 0.25 ((. + .) + (. + .)), unfused, in the precision of the fields."""
    t = P1.dtype.type
    q = t(0.25)
    fc, ff = np.asarray(fc, dtype=t)[:, None], np.asarray(ff, dtype=t)[:, None]
    v, u = _corners(P1, P2)
    return fc * (q * ((v[0] + v[1]) + (v[2] + v[3]))), -(ff * (q * ((u[0] + u[1]) + (u[2] + u[3]))))


def coriolis_exact(P1, P2, fc, ff):
    """((D1, |fc| S1), (D2, |ff| S2)) in longdouble from the values of fc, ff ROUNDED to the precision of the fields (what the kernel
    is given): S = (|.| + |.| + |.| + |.|) / 4 of the four values."""
    t, L = P1.dtype.type, np.longdouble
    fc, ff = np.asarray(fc, dtype=t).astype(L)[:, None], np.asarray(ff, dtype=t).astype(L)[:, None]
    v, u = _corners(P1.astype(L), P2.astype(L))
    D1, S1 = fc * (v[0] + v[1] + v[2] + v[3]) / 4, np.abs(fc) * (abs(v[0]) + abs(v[1]) + abs(v[2]) + abs(v[3])) / 4
    D2, S2 = -(ff * (u[0] + u[1] + u[2] + u[3]) / 4), np.abs(ff) * (abs(u[0]) + abs(u[1]) + abs(u[2]) + abs(u[3])) / 4
    return (D1, S1), (D2, S2)


# Fast tolerance, derived (include/swmhd_coriolis.h).  Every one of the four values goes through three roundings of at most eps/2 each
# before D stands: the sum of its pair, the sum of the two pairs, the product with f (the factors 1/2 and 1/4 are exact): in both
# operation orders |D - D_exact| <= ((1 + eps/2)^3 - 1) |f| S <= 2 eps |f| S.
# new = new_0 + a D: the rounding of a D where it is not fused and the rounding of the result:
# |new - ref| <= (eps/2) |ref| + ((1 + eps/2)^5 - 1) |a| |f| S, inside eps |ref| + 4 eps |a| |f| S, the bound held here.
D_ROUNDINGS = 2
UPDATE_ROUNDINGS = 4


def fast_bound_D(fS, eps):
    """|D - D_exact| <= 2 eps |f| S (fS: the second entry of a pair of coriolis_exact)."""
    return D_ROUNDINGS * eps * fS


def fast_bound(ref, a, fS, eps):
    """|got - ref| <= eps |ref| + 4 eps |a| |f| S for ref = out_0 + a D_exact (longdouble)."""
    return eps * np.abs(ref) + abs(np.longdouble(a)) * UPDATE_ROUNDINGS * eps * fS


# ---- the reference stepper -------------------------------------------------------------------------------------------------------------
# Measured by tests/test_coriolis_cases_cpu.py (it prints them), float64, one RK3 step of the smooth 20 x 12 and 13 x 10 states:
# the largest deviation between the modes "classic" / "anchor" and "tendency", in eps max |U| over both formulations and the Periodic
# and (Periodic, Bounded) grids; the bound of the test is 8 times that.
MODES_MEASURED_EPS = 1.93
MODES_BOUND_EPS = 8 * MODES_MEASURED_EPS
# the same for BetaPlane(f0, 0) in "tendency" mode against the unchanged oracle stepped with fcor = f0
FPLANE_MEASURED_EPS = 0.68
FPLANE_BOUND_EPS = 8 * FPLANE_MEASURED_EPS


class RefModel:
    """(q1, q2, h, A) through RK3 under f(y): fc, ff = f at the centres and at the south faces of the Ny rows, as the engine's table
    holds them (rounded to the precision of the fields).  mode: "classic" | "anchor" | "tendency" (module docstring).  topo: Periodic and
    Bounded directions, filled by tracer_cases.fill_state; q are halo-filled parents.  coef (optional, Periodic grids): the
    ScalarDiffusivity coefficients of the four fields, applied AFTER the Coriolis correction as the engine orders its launches."""

    def __init__(self, O, q, fc, ff, Nx, Ny, form, lor, mode="classic", topo=(T.P, T.P), gradA=None, dx=DX, dy=DY, coef=None, grav=T.GRAV):
        self.O, self.Nx, self.Ny, self.form, self.lor, self.mode, self.dx, self.dy = O, Nx, Ny, form, lor, mode, dx, dy
        self.topo, self.gradA, self.grav = topo, gradA, grav
        self.q = [a.copy() for a in q]
        t = q[0].dtype.type
        self.fc, self.ff = np.asarray(fc, dtype=t), np.asarray(ff, dtype=t)
        self.coef = list(coef) if coef is not None else [0.0] * 4
        assert mode != "anchor" or topo == (T.P, T.P)       # (the engine runs Bounded grids in the classic form)
        assert not any(self.coef) or (topo == (T.P, T.P) and mode == "classic")
        self.Gm = None
        self.I = (slice(H, H + Ny), slice(H, H + Nx))
        self.skip_stage = None      # (step, stage) whose correction is left out: a test of what the launch may touch

    def _D(self):
        """[D1, D2, None, None] of the current state, then the closure's D per field (or None)."""
        Nx, Ny = self.Nx, self.Ny
        P1, P2 = (pad1(f, Nx, Ny, H, H, False, False) for f in self.q[:2])
        C = list(coriolis_strict(P1, P2, self.fc, self.ff)) + [None, None]
        K = [DC.laplacian_strict(pad1(f, Nx, Ny, H, H, False, False), c, self.dx, self.dy) if c != 0 else None for f, c in zip(self.q, self.coef)]
        return C, K

    def step(self, dt, index=0):
        O, Nx, Ny, I = self.O, self.Nx, self.Ny, self.I
        for s in range(3):
            U = self.q
            G = list(O.tendencies(*U, Nx, Ny, H, H, self.dx, self.dy, self.form, self.lor, self.grav, 0.0, topo=self.topo))
            C, K = self._D()
            if self.skip_stage == (index, s):
                C = [None] * 4
            if self.mode == "tendency":        # Oceananigans: D is part of the tendency
                for g, d in zip(G, C):
                    if d is not None:
                        g[I] = g[I] + d
                new = [T.substep(u, g, self.Gm[k] if s else None, Nx, Ny, dt, GAMMA[s], ZETA[s], s == 0) for k, (u, g) in enumerate(zip(U, G))]
            elif self.mode == "classic":       # the stage kernel's update, then new += dt gamma D and, in storing stages, Gn += D
                new = [T.substep(u, g, self.Gm[k] if s else None, Nx, Ny, dt, GAMMA[s], ZETA[s], s == 0) for k, (u, g) in enumerate(zip(U, G))]
                for D in (C, K):               # the launch order: Coriolis, then the closure
                    for n, g, d in zip(new, G, D):
                        if d is not None:
                            n[I] = correct(n[I], d, dt * GAMMA[s])
                            if s < 2:
                                g[I] = correct(g[I], d, 1.0)
            else:                              # anchor: U1 = U0 + dt g1 G0, W = U0 + (dt/4) G0, U2 = W + dt g2 G1, U3 = W + dt g3 G2
                new = []
                for k, (u, g, d) in enumerate(zip(U, G, C)):
                    t = u.dtype.type
                    base = u if s == 0 else self.Gm[k]
                    n = u.copy()
                    n[I] = base[I] + t(dt * GAMMA[s]) * g[I]
                    if s == 0:
                        w = u.copy()
                        w[I] = u[I] + t(dt * ANCHOR_WEIGHT) * g[I]
                    if d is not None:
                        n[I] = correct(n[I], d, dt * GAMMA[s])
                        if s == 0:
                            w[I] = correct(w[I], d, dt * ANCHOR_WEIGHT)
                    new.append(n)
                    G[k] = w if s == 0 else self.Gm[k]     # W travels where G- does
            self.q = T.fill_state(O, new, Nx, Ny, self.topo, self.gradA, self.dx, self.dy)
            self.Gm = G
        return self


# ---- Rossby-wave propagation ------------------------------------------------------------------------------------------------------------
# A (Periodic, Bounded) channel 32 x 16 with y in (5, 7): f = f0 + beta y with f0 = 4, beta = 1, so f = 10 in mid-channel, a grid whose
# y[0] != 0: an origin error moves f by half its value.  h = 1 + eta, eta = eta0 cos(k x) sin(l (y - y_south)), l = pi / Ly (v = 0 at the
# walls), u, v in geostrophic balance with the mid-channel f.  Quasi-geostrophic theory: the wave moves WESTWARD with
#     c = -beta / (k^2 + l^2 + f_mid^2 / (g H)).
# The phase is that of the projection of h - 1 on exp(i k x) sin(l (y - y_south)); its speed is the least-squares slope over the run.
ROSSBY_NX, ROSSBY_NY = 32, 16
ROSSBY_X, ROSSBY_Y = (0.0, 4.0), (5.0, 7.0)
ROSSBY_F0, ROSSBY_BETA = 4.0, 1.0
ROSSBY_ETA0, ROSSBY_DT, ROSSBY_STEPS, ROSSBY_EVERY = 1e-3, 0.02, 150, 5
# |c_measured / c_theory - 1| of RefModel("tendency") in float64, as tests/test_coriolis_cases_cpu.py computes and prints it: the
# discretisation on 32 x 16 cells, the O(beta Ly / f) terms quasi-geostrophy drops and the inertia-gravity waves the unbalanced part
# of the start radiates.  The margin of the test is twice this.
ROSSBY_REFERENCE_DEVIATION = 0.0029
ROSSBY_MARGIN = 2 * ROSSBY_REFERENCE_DEVIATION


def rossby_theory(grav=T.GRAV, depth=1.0):
    k = 2 * np.pi / (ROSSBY_X[1] - ROSSBY_X[0])
    l = np.pi / (ROSSBY_Y[1] - ROSSBY_Y[0])
    f_mid = ROSSBY_F0 + ROSSBY_BETA * 0.5 * (ROSSBY_Y[0] + ROSSBY_Y[1])
    return k, l, f_mid, -ROSSBY_BETA / (k * k + l * l + f_mid * f_mid / (grav * depth))


def rossby_state(xc, xf, yc, yf, grav=T.GRAV):
    """(u, v, h, A) parents (halos unfilled) on the node coordinates of the grid, halos included."""
    k, l, f_mid, _ = rossby_theory(grav)
    y0 = ROSSBY_Y[0]
    eta = lambda x, y: ROSSBY_ETA0 * np.cos(k * x)[None, :] * np.sin(l * (y - y0))[:, None]
    u = -(grav / f_mid) * ROSSBY_ETA0 * l * np.cos(k * xf)[None, :] * np.cos(l * (yc - y0))[:, None]       # -g/f d eta/dy at (Face, Center)
    v = -(grav / f_mid) * ROSSBY_ETA0 * k * np.sin(k * xc)[None, :] * np.sin(l * (yf - y0))[:, None]       # +g/f d eta/dx at (Center, Face)
    h = 1.0 + eta(xc, yc)
    return [np.ascontiguousarray(a) for a in (u, v, h, np.zeros_like(h))]


def rossby_phase(h, xc, yc):
    """The phase phi of the mode eta ~ cos(k x - phi) sin(l (y - y_south)) in the interior of the parent h."""
    k, l, _, _ = rossby_theory()
    I = (slice(H, H + ROSSBY_NY), slice(H, H + ROSSBY_NX))
    x, y = xc[H:H + ROSSBY_NX], yc[H:H + ROSSBY_NY]
    z = ((h[I] - 1.0) * np.sin(l * (y - ROSSBY_Y[0]))[:, None] * np.exp(1j * k * x)[None, :]).sum()
    return np.angle(z)
