"""Reference of the ScalarBiharmonicDiffusivity closure (swmhd_biharmonic_rk3_* in include/swmhd_biharmonic.h,
ShallowWaterModel(closure=...)) and the cases its tests run.  numpy + the CPU oracle only.

Oceananigans is not on this machine: the pin is the written formula, restated here.
    L = ((phi_e - phi) / dx - (phi - phi_w) / dx) / dx + ((phi_n - phi) / dy - (phi - phi_s) / dy) / dy     at the cell and its four neighbours
    Fx_i = c ((L_i - L_{i-1}) / dx),  Fy_j likewise,  D = -((Fx_{i+1} - Fx_i) / dx + (Fy_{j+1} - Fy_j) / dy)                 (biharmonic_strict)
in the precision of the field, one rounding per operation; biharmonic_exact is the same value in longdouble with the scale S of its
rounding error.  The engine adds D to what the stage kernels wrote, after the Laplacian closure's correction where there is one:
new += a D, acc += w D (correct).  RefModel steps the state and the tracers as diffusion_cases.RefModel does and takes both closures at
once, each by its own correction in the engine's order ("classic", "anchor") or both added to the tendency ("tendency")."""
import numpy as np

import diffusion_cases as DC
import tracer_cases as T
from strip_cases import TILE_ROWS, row_ranges, stage_shapes as strip_stage_shapes, wave_columns      # noqa: F401

H = T.H
GAMMA, ZETA = T.GAMMA, T.ZETA
ANCHOR_WEIGHT = DC.ANCHOR_WEIGHT
DX, DY = T.DX, T.DY
SENTINEL = T.SENTINEL

# ---- the stage matrix -----------------------------------------------------------------------------------------------------------------
# the shapes of the strip-march launches, and the widths and heights at which a wrap of radius 2 folds more than once or meets itself
NARROW_SHAPES = [(4, 1), (1, 4), (5, 2), (2, 5)]


def stage_shapes(itemsize, aligned):
    return strip_stage_shapes(itemsize, aligned) + NARROW_SHAPES


# ---- the operator ---------------------------------------------------------------------------------------------------------------------
def pad2(parent, Nx, Ny, Hx, Hy, wrap_x, wrap_y):
    """The interior of `parent` with the two cells around it: (Ny + 4, Nx + 4).  Wrapped directions take the periodic image
    (x mod Nx, y mod Ny; a true modulus) of the INTERIOR, the others the halo cell.  (The operator reads the diamond only: of the 2 x 2
    corner blocks just the inner cell.)"""
    rows = np.arange(-2, Ny + 2)
    cols = np.arange(-2, Nx + 2)
    rows = Hy + (rows % Ny if wrap_y else rows)
    cols = Hx + (cols % Nx if wrap_x else cols)
    return parent[np.ix_(rows, cols)]


def reach(Nx, Ny, Hx, Hy, shape, wrap_x, wrap_y, rows):
    """Boolean mask over a parent of `shape`: the cells the call over `rows` = (j0, j1) may read -- the 13-cell diamonds of its cells."""
    m = np.zeros(shape, dtype=bool)
    j0, j1 = rows
    if j1 <= j0:
        return m
    y, x = np.meshgrid(np.arange(j0, j1), np.arange(Nx), indexing="ij")
    for oy in range(-2, 3):
        for ox in range(-2 + abs(oy), 3 - abs(oy)):
            yy, xx = y + oy, x + ox
            m[Hy + (yy % Ny if wrap_y else yy), Hx + (xx % Nx if wrap_x else xx)] = True
    return m


def _lap_strict(P, dx, dy):
    C, W, E, S, N = DC._parts(P)
    return ((E - C) / dx - (C - W) / dx) / dx + ((N - C) / dy - (C - S) / dy) / dy


def biharmonic_strict(P, c, dx, dy):
    """D on the interior cells of pad2's array, in its precision and the strict operation order."""
    t = P.dtype.type
    c, dx, dy = t(c), t(dx), t(dy)
    with np.errstate(invalid="ignore"):
        C, W, E, S, N = DC._parts(_lap_strict(P, dx, dy))      # (L of a corner cell, made of cells outside the diamond, is not used)
        Fxw, Fxe = c * ((C - W) / dx), c * ((E - C) / dx)
        Fys, Fyn = c * ((C - S) / dy), c * ((N - C) / dy)
        return -((Fxe - Fxw) / dx + (Fyn - Fys) / dy)


def biharmonic_exact(P, c, dx, dy):
    """(D, S) in longdouble from the values of c, dx, dy ROUNDED to the precision of P (what the kernel is given):
    S = c Labs(Labs(|phi|)), Labs(psi) = (psi_e + 2 psi + psi_w) / dx² + (psi_n + 2 psi + psi_s) / dy²."""
    t, L = P.dtype.type, np.longdouble
    c, dx, dy = L(t(c)), L(t(dx)), L(t(dy))

    def lap(Q, sign):
        C, W, E, S, N = DC._parts(Q)
        return (E + sign * 2 * C + W) / (dx * dx) + (N + sign * 2 * C + S) / (dy * dy)
    with np.errstate(invalid="ignore"):
        Q = P.astype(L)
        return -c * lap(lap(Q, -1), -1), abs(c) * lap(lap(np.abs(Q), 1), 1)


# Fast tolerance, derived (include/swmhd_biharmonic.h).  The kernel's expression is the composed one,
#   L = rdx2 ((e + w) - 2 phi) + rdy2 ((n + s) - 2 phi),  D = (-(c rdx2)) ((L_e + L_w) - 2 L) + (-(c rdy2)) ((L_n + L_s) - 2 L).
# L: six roundings (two in rdx2, the sum, the difference, the product, the last sum; fused or not), each at most eps/2 relative to a partial
# result that Labs(|phi|) bounds: 3 eps Labs(|phi|), which the outer operator turns into at most 3 eps S.  D: seven roundings of its own
# (three in c rdx2, the sum, the difference, the product, the last sum) relative to partial results that c Labs(|L|) <= S (1 + 3 eps)
# bounds: 3.5 eps S.  Together 6.5 eps S to first order: |D - D_exact| <= 8 eps S.
# new = new_0 + a D: one rounding of the result (eps |ref|), a times the error of D, the rounding of a D where it is not fused and
# second-order terms: 10 eps |a| S in all.
D_ROUNDINGS = 8
UPDATE_ROUNDINGS = 10


def correct(out, D, a):
    """out + a D in the precision of out, the product rounded before the sum (strict order)."""
    return DC.correct(out, D, a)


def fast_bound(ref, a, scale, eps):
    """|got - ref| <= eps |ref| + |a| 10 eps S for ref = out_0 + a D_exact (longdouble)."""
    return eps * np.abs(ref) + abs(np.longdouble(a)) * UPDATE_ROUNDINGS * eps * scale


# ---- the reference stepper -------------------------------------------------------------------------------------------------------------
class RefModel(DC.RefModel):
    """diffusion_cases.RefModel with both closures: coef the Laplacian coefficient and coef4 the biharmonic one of every one of the 4 + K
    fields (0: none; h's must be 0).  Per stage the Laplacian correction comes first, then the biharmonic one: the engine's order."""

    def __init__(self, O, q, tracers, coef, coef4, Nx, Ny, form, lor, mode="classic", dx=DX, dy=DY):
        super().__init__(O, q, tracers, coef, Nx, Ny, form, lor, mode, dx, dy)
        assert len(coef4) == 4 + len(tracers) and coef4[2] == 0
        self.coef4 = list(coef4)

    def _D4(self, f, c):
        return biharmonic_strict(pad2(f, self.Nx, self.Ny, H, H, False, False), c, self.dx, self.dy)

    def step(self, dt):
        O, Nx, Ny, I = self.O, self.Nx, self.Ny, self.I
        for s in range(3):
            U = self.q + self.tr
            G = list(O.tendencies(*self.q, Nx, Ny, H, H, self.dx, self.dy, self.form, self.lor, T.GRAV, T.FCOR))
            G += [T.tracer_tendency(O, self.q, c, Nx, Ny, self.dx, self.dy, self.form) for c in self.tr]
            D = [[self._D(f, c) if c != 0 else None, self._D4(f, c4) if c4 != 0 else None] for f, c, c4 in zip(U, self.coef, self.coef4)]
            if self.mode == "tendency":        # Oceananigans: every D is part of the tendency
                for g, ds in zip(G, D):
                    for d in ds:
                        if d is not None:
                            g[I] = g[I] + d
                new = [T.substep(u, g, self.Gm[k] if s else None, Nx, Ny, dt, GAMMA[s], ZETA[s], s == 0) for k, (u, g) in enumerate(zip(U, G))]
            elif self.mode == "classic":       # the stage kernels' update, then per closure new += dt gamma D and, in storing stages, Gn += D
                new = [T.substep(u, g, self.Gm[k] if s else None, Nx, Ny, dt, GAMMA[s], ZETA[s], s == 0) for k, (u, g) in enumerate(zip(U, G))]
                for n, g, ds in zip(new, G, D):
                    for d in ds:
                        if d is not None:
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
# The decay case of diffusion_cases: A = sin(kx) sin(ly) on the 16 x 12 grid, u = v = 0, h = 1, no forcing.  The field is an eigenvector
# of the 13-point operator with the eigenvalue -c lambda², lambda the 5-point Laplacian's, so every RK3 step multiplies it by R(z),
# z = -dt c lambda².  The grid-scale mode has lambda_max = 4/dx² + 4/dy² and must stay inside RK3's interval, dt c lambda_max² < 2.51,
# or rounding noise would grow; (lambda / lambda_max)² = 0.0128 here, which caps |z| of the mode at 0.032: c is chosen for |z| = 0.029
# (dt c lambda_max² = 2.25), and 20 steps take the mode to 0.56 of its start.
DECAY_NX, DECAY_NY, DECAY_STEPS = DC.DECAY_NX, DC.DECAY_NY, DC.DECAY_STEPS
DECAY_C, DECAY_DT = 1.4e-4, DC.DECAY_DT
DECAY_MODES = DC.DECAY_MODES
# max |A_20 - R(z)^20 A_0| / (R(z)^20 max |A_0|) of RefModel("classic") in float64, as tests/test_biharmonic_cases_cpu.py computes and
# prints it on the CPU.  The margin of every decay test is ten times this.
DECAY_REFERENCE_DEVIATION = 1.997e-15
DECAY_MARGIN = 10 * DECAY_REFERENCE_DEVIATION
LAMBDA_MAX = 4 / DX ** 2 + 4 / DY ** 2


def decay_case(dtype=np.float64):
    """(q, z, R): the halo-filled parents (u, v, h, A) of the decay case (fill them with oracle.fill_halo_periodic), z and R(z)."""
    q, z1, _ = DC.decay_case(dtype)
    lam = -z1 / (DC.DECAY_DT * DC.DECAY_C)
    z = -DECAY_DT * DECAY_C * lam * lam
    return q, z, 1 + z + z * z / 2 + z ** 3 / 6


def decay_fast_bound(eps, steps=DECAY_STEPS):
    """What the fast kernel may add to the relative deviation after `steps` steps: per stage eps |A| + dt gamma 10 eps S with
    S <= c lambda_max² max |A|, summed over the 3 stages of every step against max |A| = 1 of the start (later stages are smaller, and the
    stage maps of a decaying mode do not amplify an error), divided by R^steps by the caller."""
    S = DECAY_C * LAMBDA_MAX ** 2
    return steps * sum(eps + DECAY_DT * g * UPDATE_ROUNDINGS * eps * S for g in GAMMA)
