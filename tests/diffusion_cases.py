"""Reference of the ScalarDiffusivity closure (swmhd_diffusion_rk3_* in include/swmhd_diffusion.h, ShallowWaterModel(closure=...)) and
the cases its tests run.  numpy + the CPU oracle only.

Oceananigans is not on this machine: the pin is the written formula, restated here.
    Fx_i = c ((phi_i - phi_{i-1}) / dx),  Fy_j likewise,  D = (Fx_{i+1} - Fx_i) / dx + (Fy_{j+1} - Fy_j) / dy        (laplacian_strict)
in the precision of the field, one rounding per operation; laplacian_exact is the same value in longdouble with the scale S of its
rounding error.  The engine adds D to what the stage kernels wrote: new += a D, acc += w D (correct).  RefModel steps the state and the
tracers as tests/tracer_cases.RefModel does -- oracle tendencies, numpy update, oracle halo fill -- and puts the closure in by that
correction ("classic", the engine's strict schedule; "anchor", its fast schedule in numpy) or by adding D to the tendency before the
update ("tendency": what Oceananigans does).  tests/test_diffusion_cases_cpu.py holds the three against each other."""
import numpy as np

import tracer_cases as T

H = T.H
GAMMA, ZETA = T.GAMMA, T.ZETA
ANCHOR_WEIGHT = 0.25
DX, DY = T.DX, T.DY
SENTINEL = T.SENTINEL

# ---- the stage matrix -----------------------------------------------------------------------------------------------------------------
from strip_cases import TILE_ROWS, row_ranges, stage_shapes, wave_columns      # noqa: F401  (shared with the other strip-march launch)


# ---- the operator ---------------------------------------------------------------------------------------------------------------------
def pad1(parent, Nx, Ny, Hx, Hy, wrap_x, wrap_y):
    """The interior of `parent` with the one cell around it that the operator reads: (Ny + 2, Nx + 2).  Wrapped directions take the
    periodic image (x mod Nx, y mod Ny) of the INTERIOR, the others the halo cell."""
    rows = np.arange(-1, Ny + 1)
    cols = np.arange(-1, Nx + 1)
    rows = Hy + (rows % Ny if wrap_y else rows)
    cols = Hx + (cols % Nx if wrap_x else cols)
    return parent[np.ix_(rows, cols)]


def _parts(P):
    return P[1:-1, 1:-1], P[1:-1, :-2], P[1:-1, 2:], P[:-2, 1:-1], P[2:, 1:-1]      # centre, west, east, south, north


def laplacian_strict(P, c, dx, dy):
    """D on the cells of pad1's array, in its precision and the strict operation order."""
    t = P.dtype.type
    c, dx, dy = t(c), t(dx), t(dy)
    C, W, E, S, N = _parts(P)
    Fxw, Fxe = c * ((C - W) / dx), c * ((E - C) / dx)
    Fys, Fyn = c * ((C - S) / dy), c * ((N - C) / dy)
    return (Fxe - Fxw) / dx + (Fyn - Fys) / dy


def laplacian_exact(P, c, dx, dy):
    """(D, S) in longdouble from the values of c, dx, dy ROUNDED to the precision of P (what the kernel is given):
    S = |c|/dx² (|e| + 2|phi| + |w|) + |c|/dy² (|n| + 2|phi| + |s|)."""
    t, L = P.dtype.type, np.longdouble
    c, dx, dy = L(t(c)), L(t(dx)), L(t(dy))
    C, W, E, S, N = (a.astype(L) for a in _parts(P))
    D = c / (dx * dx) * (E - 2 * C + W) + c / (dy * dy) * (N - 2 * C + S)
    scale = abs(c) / (dx * dx) * (abs(E) + 2 * abs(C) + abs(W)) + abs(c) / (dy * dy) * (abs(N) + 2 * abs(C) + abs(S))
    return D, scale


# Fast tolerance, derived (include/swmhd_diffusion.h).  The kernel's expression is (c rdx2)((e + w) - 2 phi) + (c rdy2)((n + s) - 2 phi)
# with rdx2 = 1 / (dx dx): three roundings in c rdx2 (the product dx dx, the quotient, the product with c), one in e + w, one in the
# difference (2 phi is exact; fused or not), one in the product, one in the last sum (fused or not): seven, each at most eps/2 relative to
# a partial result that S bounds: |D - D_exact| <= 8 eps S, the count of eight (two in c/dx², one multiply, five in the sum) of a
# plain evaluation, stands.
# new = new_0 + a D: one rounding of the result (eps |ref|), and a times the error of D, the rounding of a D where it is not fused (eps |a|
# S) and second-order terms: 10 eps |a| S in all.
UPDATE_ROUNDINGS = 10


def correct(out, D, a):
    """out + a D in the precision of out, the product rounded before the sum (strict order)."""
    t = out.dtype.type
    return out + t(a) * D


def fast_bound(ref, a, scale, eps):
    """|got - ref| <= eps |ref| + |a| 10 eps S for ref = out_0 + a D_exact (longdouble)."""
    return eps * np.abs(ref) + abs(np.longdouble(a)) * UPDATE_ROUNDINGS * eps * scale


# ---- the reference stepper -------------------------------------------------------------------------------------------------------------
class RefModel:
    """(q1, q2, h, A) and tracers through RK3 with the closure: coef = the coefficient of every one of the 4 + K fields (0: not diffused;
    h's must be 0).  mode: "classic" | "anchor" | "tendency" (module docstring).  Periodic grids; q and tracers are halo-filled parents."""

    def __init__(self, O, q, tracers, coef, Nx, Ny, form, lor, mode="classic", dx=DX, dy=DY):
        assert len(coef) == 4 + len(tracers) and coef[2] == 0
        self.O, self.Nx, self.Ny, self.form, self.lor, self.mode, self.dx, self.dy = O, Nx, Ny, form, lor, mode, dx, dy
        self.q = [a.copy() for a in q]
        self.tr = [a.copy() for a in tracers]
        self.coef = list(coef)
        self.Gm = None
        self.I = (slice(H, H + Ny), slice(H, H + Nx))

    def _D(self, f, c):
        return laplacian_strict(pad1(f, self.Nx, self.Ny, H, H, False, False), c, self.dx, self.dy)

    def step(self, dt):
        O, Nx, Ny, I = self.O, self.Nx, self.Ny, self.I
        for s in range(3):
            U = self.q + self.tr
            G = list(O.tendencies(*self.q, Nx, Ny, H, H, self.dx, self.dy, self.form, self.lor, T.GRAV, T.FCOR))
            G += [T.tracer_tendency(O, self.q, c, Nx, Ny, self.dx, self.dy, self.form) for c in self.tr]
            D = [self._D(f, c) if c != 0 else None for f, c in zip(U, self.coef)]
            if self.mode == "tendency":        # Oceananigans: D is part of the tendency
                for g, d in zip(G, D):
                    if d is not None:
                        g[I] = g[I] + d
                new = [T.substep(u, g, self.Gm[k] if s else None, Nx, Ny, dt, GAMMA[s], ZETA[s], s == 0) for k, (u, g) in enumerate(zip(U, G))]
            elif self.mode == "classic":       # the stage kernels' update, then new += dt gamma D and, in storing stages, Gn += D
                new = [T.substep(u, g, self.Gm[k] if s else None, Nx, Ny, dt, GAMMA[s], ZETA[s], s == 0) for k, (u, g) in enumerate(zip(U, G))]
                for n, g, d in zip(new, G, D):
                    if d is not None:
                        n[I] = correct(n[I], d, dt * GAMMA[s])
                        if s < 2:
                            g[I] = correct(g[I], d, 1.0)
            else:                              # anchor: U1 = U0 + dt g1 G0, W = U0 + (dt/4) G0, U2 = W + dt g2 G1, U3 = W + dt g3 G2
                new = []
                for k, (u, g, d) in enumerate(zip(U, G, D)):
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
            self.q = T.fill_state(O, new[:4], Nx, Ny, (T.P, T.P), None, self.dx, self.dy)
            self.tr = [T.fill(O, c, Nx, Ny, (T.P, T.P)) for c in new[4:]]
            self.Gm = G
        return self


# ---- pure decay -----------------------------------------------------------------------------------------------------------------------
# A = sin(kx) sin(ly) at the centres of a 16 x 12 grid on u = v = 0, h = 1, no forcing: the advective tendency is exactly 0 and the field
# is an eigenvector of the 5-point operator, so every RK3 step multiplies it by R(z) = 1 + z + z²/2 + z³/6, z = -dt c lambda,
# lambda = (4/dx²) sin²(k dx/2) + (4/dy²) sin²(l dy/2).
DECAY_NX, DECAY_NY, DECAY_STEPS = 16, 12, 20
DECAY_C, DECAY_DT = 0.01, 0.05
DECAY_MODES = (2, 1)                # waves along x and along y
# max |A_20 - R(z)^20 A_0| / (R(z)^20 max |A_0|) of RefModel("classic") in float64, as tests/test_diffusion_cases_cpu.py computes and
# prints it: rounding of 60 stages of an exactly diagonal map.  The margin of every decay test is ten times this.
DECAY_REFERENCE_DEVIATION = 2.839e-15
DECAY_MARGIN = 10 * DECAY_REFERENCE_DEVIATION


def decay_case(dtype=np.float64):
    """(q, z, R): the halo-filled parents (u, v, h, A) of the decay case (fill them with oracle.fill_halo_periodic), z and R(z)."""
    Nx, Ny = DECAY_NX, DECAY_NY
    k, l = 2 * np.pi * DECAY_MODES[0] / (Nx * DX), 2 * np.pi * DECAY_MODES[1] / (Ny * DY)
    x = (np.arange(-H, Nx + H) + 0.5) * DX
    y = (np.arange(-H, Ny + H) + 0.5) * DY
    A = np.sin(l * y)[:, None] * np.sin(k * x)[None, :]
    shp = A.shape
    q = [np.zeros(shp), np.zeros(shp), np.ones(shp), A]
    lam = 4 / DX ** 2 * np.sin(k * DX / 2) ** 2 + 4 / DY ** 2 * np.sin(l * DY / 2) ** 2
    z = -DECAY_DT * DECAY_C * lam
    return [np.ascontiguousarray(a.astype(dtype)) for a in q], z, 1 + z + z * z / 2 + z ** 3 / 6


def decay_fast_bound(eps, steps=DECAY_STEPS):
    """What the fast kernel may add to the relative deviation after `steps` steps: per stage eps |A| + dt gamma 10 eps S with
    S <= c (4/dx² + 4/dy²) max |A|, summed over the 3 stages of every step against max |A| = 1 of the start (later stages are smaller,
    and the stage maps 1 + gamma z, ... of a decaying mode do not amplify an error), divided by R^steps by the caller."""
    S = DECAY_C * (4 / DX ** 2 + 4 / DY ** 2)
    return steps * sum(eps + DECAY_DT * g * UPDATE_ROUNDINGS * eps * S for g in GAMMA)
