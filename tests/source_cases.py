"""Reference of the static sources -- bathymetry and steady body forces (swmhd_source_rk3_* in include/swmhd_source.h,
ShallowWaterModel(bathymetry=..., forcing={...: Source(...)})) -- and the cases its tests run.  numpy + the CPU oracle only.

Oceananigans is not on this machine: the pin is the written formula, restated here.
    kind 0: D = S            kind 1: D = ((h[i-1,j] + h[i,j]) / 2) S            kind 2: D = ((h[i,j-1] + h[i,j]) / 2) S      (source_strict)
in the precision of the field, one rounding per operation, in that order; (x + y) / 2 is the oracle's interpolation
(oracle/sw_rhs.inc).  source_exact is the same value in longdouble with the scale M of its rounding error.  The engine adds D to what
the launches before it wrote: new += a D, acc += w D (relaxation_cases.correct).  host_source restates what the host hands over as S:
    S_u = F_u - g ((b[i,j] - b[i-1,j]) / dx),   S_v = F_v - g ((b[i,j] - b[i,j-1]) / dy)
in float64, b wrapped in a Periodic direction, 0 on the wall line of a Bounded one, rounded once to the precision of the model.
RefModel is stochastic_cases.RefModel (so relaxation_cases.RefModel with every other correction) with the source put in after the
relaxation and before the stochastic term, the engine's launch order."""
import numpy as np

import relaxation_cases as RC
import stochastic_cases as STC
import tracer_cases as T

H = T.H
DX, DY = T.DX, T.DY
SENTINEL = T.SENTINEL
MAX_FIELDS = 12                     # SWMHD_SOURCE_MAX_FIELDS
PLAIN, X_FACE, Y_FACE = 0, 1, 2     # SWMHD_SOURCE_PLAIN, _X_FACE, _Y_FACE
correct = RC.correct

# ---- the stage matrix: the geometry of the strip-march launches, read from strip_cases -------------------------------------------------
from strip_cases import TILE_ROWS, row_ranges, wave_columns      # noqa: F401,E402
import strip_cases as _SC      # noqa: E402

NFIELDS = (1, 4, MAX_FIELDS)
WRAPS = ((True, True), (True, False), (False, True), (False, False))      # (wrap x, wrap y): both, each alone, neither (filled halos)


def stage_shapes(itemsize, aligned):
    """Nx in {1, 2, 3, 63, 64, 65, 129} and Ny in {1, 2, 5, 67} (67 crosses the 64-row tile: its last wave segment starts with a freshly
    loaded carried h row, as every 16-row segment does), each value at least once, and the three shapes of strip_cases around the
    width of one wave and the height of one tile."""
    return [(1, 1), (2, 2), (3, 5), (63, 67), (64, 5), (65, 2), (129, 67)] + _SC.stage_shapes(itemsize, aligned)[-3:]


def kind_of(k):
    """The kind of field k of a call of the stage matrix: 0, 1, 2 in turn starting at 1, so that one field is an x face, four fields
    hold all three and twelve each four times."""
    return (k + 1) % 3


# ---- the term -------------------------------------------------------------------------------------------------------------------------
def neighbour(hp, Nx, Ny, kind, wrapx=False, wrapy=False, Hx=H, Hy=H):
    """The thickness one cell west (kind 1) or south (kind 2) of every interior cell of the parent hp: the periodic image in a wrapped
    direction, else the halo cell."""
    h = hp[Hy:Hy + Ny, Hx:Hx + Nx]
    if kind == X_FACE:
        return np.roll(h, 1, axis=1) if wrapx else hp[Hy:Hy + Ny, Hx - 1:Hx + Nx - 1]
    return np.roll(h, 1, axis=0) if wrapy else hp[Hy - 1:Hy + Ny - 1, Hx:Hx + Nx]


def source_strict(S, kind, h=None, other=None):
    """D on the cells of S, in its precision and the strict operation order.  h, other: the thickness at the cells and one cell west or
    south of them (neighbour), for kind 1 and 2."""
    if kind == PLAIN:
        return S
    t = S.dtype.type
    return ((other + h) / t(2)) * S


def source_exact(S, kind, h=None, other=None):
    """(D, M) in longdouble from the values the kernel is given: M = |S| (kind 0), ((|other| + |h|) / 2) |S| (kind 1, 2)."""
    L = np.longdouble
    s = S.astype(L)
    if kind == PLAIN:
        return s, np.abs(s)
    return ((other.astype(L) + h.astype(L)) / 2) * s, ((np.abs(other.astype(L)) + np.abs(h.astype(L))) / 2) * np.abs(s)


# Fast tolerance, derived (include/swmhd_source.h).  The kernel's expression is the strict one; a fast object may fuse a D + new.
# kind 0: D is a load and has no rounding; new = new_0 + a D rounds a D (where not fused) and the sum: 2 roundings.
# kind 1, 2: the sum other + h (the halving is exact) and the product with S, then the update: 4 roundings, 3 where fused.
# With ref = new_0 + a D_exact, n roundings of at most eps/2 each: |new - ref| <= (eps/2) |ref| + ((1 + eps/2)^(n-1) - 1) (1 + eps/2) |a| M
# <= eps |ref| + ((1 + eps/2)^n - 1) |a| M, which is what the tests hold the fast result to.
ROUNDINGS = {PLAIN: 2, X_FACE: 4, Y_FACE: 4}


def fast_bound(ref, a, M, eps, kind):
    """|got - ref| <= eps |ref| + ((1 + eps/2)^n - 1) |a| M for ref = out_0 + a D_exact (longdouble), n = ROUNDINGS[kind]."""
    L = np.longdouble
    return L(eps) * np.abs(ref) + ((1 + L(eps) / 2) ** ROUNDINGS[kind] - 1) * abs(L(a)) * M


# ---- what the host hands over ------------------------------------------------------------------------------------------------------------
def host_source(b, F, g, spacing, axis, periodic, dtype):
    """S of the momentum-like field of direction `axis` (1: x, 0: y) from the bottom b (Ny, Nx) at the centres, in float64 in the written
    order, rounded once to dtype.  F: the body force there (an array or 0.0)."""
    d = (b - np.roll(b, 1, axis=axis)) / np.float64(spacing)
    if not periodic:
        if axis == 1:
            d[:, 0] = 0.0
        else:
            d[0, :] = 0.0
    return (F - np.float64(g) * d).astype(dtype)


# ---- the reference stepper -------------------------------------------------------------------------------------------------------------
class RefModel(STC.RefModel):
    """stochastic_cases.RefModel with the static sources: source is one entry per field of the 4 + K, None or (kind, S) with S an
    interior array (Ny, Nx) in the precision of the fields.  The thickness is field 2 of the state the stage started from, halos
    filled.  weight: how a kind 1 / 2 source is weighted -- "face" (the engine's interpolated thickness) or "cell" (h[i,j]: the
    un-interpolated variant, for the lake-at-rest test only)."""

    def __init__(self, *a, source=None, weight="face", **kw):
        super().__init__(*a, **kw)
        self.source, self.weight = source, weight

    def source_terms(self, U):
        Nx, Ny, I = self.Nx, self.Ny, self.I
        out = {}
        for k, s in enumerate(self.source or ()):
            if s is None:
                continue
            kind, S = s
            if kind == PLAIN:
                out[k] = source_strict(S, kind)
            elif self.weight == "cell":
                out[k] = U[2][I] * S
            else:
                out[k] = source_strict(S, kind, U[2][I], neighbour(U[2], Nx, Ny, kind))
        return out

    def _D(self, U):
        out = RC.RefModel._D(self, U)
        for k, d in self.source_terms(U).items():
            out[k].append(d)
        if self._F:
            for k, F in self._F.items():
                out[k].append(F)
        return out


# ---- the lake at rest ------------------------------------------------------------------------------------------------------------------
# h + b constant, no flow, A = 0: the pressure force of the stage and the bathymetry term cancel to rounding in the interpolated form, for
# both formulations.  Two grids: (Periodic, Periodic) with a 2-D bottom, and a (Periodic, Bounded) channel.
LAKE_NX, LAKE_NY, LAKE_STEPS, LAKE_DT = 13, 11, 20, 2e-3
LAKE_H, LAKE_G = 1.0, 9.81
LAKE_TOPOS = {"periodic": (T.P, T.P), "channel": (T.P, T.B)}
LAKE_RESIDUAL_EPS = 32              # the residual tendency at rest: <= 32 eps g H^2 / min(dx, dy), the measured 16.5 .. 19 eps with margin


def lake_bottom(Nx=LAKE_NX, Ny=LAKE_NY, dx=DX, dy=DY, topo=(T.P, T.P)):
    """b at the cell centres: a Gaussian hill plus a sine in x, times a cosine in y (a full period: periodic and, in the channel, an even
    mirror at the walls), up to 0.35 H."""
    x = (np.arange(Nx) + 0.5) * dx
    y = (np.arange(Ny) + 0.5) * dy
    Lx, Ly = Nx * dx, Ny * dy
    X, Y = x[None, :], y[:, None]
    return (0.25 * np.exp(-((X - 0.45 * Lx) / (0.2 * Lx)) ** 2 - ((Y - 0.55 * Ly) / (0.25 * Ly)) ** 2)
            + 0.1 * np.sin(2 * np.pi * X / Lx) * np.cos(2 * np.pi * Y / Ly))


def lake_state(O, b, topo, dtype):
    """(q1, q2, h, A) parents of the lake at rest over b: h = H - b rounded to dtype, everything else 0, halos filled."""
    Ny, Nx = b.shape
    shp = (Ny + 2 * H, Nx + 2 * H)
    q = [np.zeros(shp, dtype=dtype) for _ in range(4)]
    q[2][H:H + Ny, H:H + Nx] = (LAKE_H - b).astype(dtype)
    return T.fill_state(O, q, Nx, Ny, topo, None, DX, DY)


def lake_sources(b, topo, form, dtype, g=LAKE_G):
    """RefModel's source list of the bathymetry b alone: S_u, S_v as the host builds them, kind 0 (vector-invariant) or 1, 2."""
    Su = host_source(b, 0.0, g, DX, 1, topo[0] == T.P, dtype)
    Sv = host_source(b, 0.0, g, DY, 0, topo[1] == T.P, dtype)
    kinds = (PLAIN, PLAIN) if form == 1 else (X_FACE, Y_FACE)
    return [(kinds[0], Su), (kinds[1], Sv), None, None]


def lake_bound(dtype):
    return LAKE_RESIDUAL_EPS * float(np.finfo(dtype).eps) * LAKE_G * LAKE_H ** 2 / min(DX, DY)


# max(|u|, |v|) (vector-invariant) or max(|uh|, |vh|) (conservative) of RefModel("classic") after LAKE_STEPS steps of LAKE_DT from the
# lake at rest, as tests/test_source_cases_cpu.py computes and prints it: the rounding residual of the balance, integrated.  The device
# is held to ten times this (LAKE_MARGIN), the margin relaxation_cases uses; it covers the fast build's fusion and schedule.
LAKE_REFERENCE_DRIFT = {
    ("periodic", 1, "f64"): 6.928e-16, ("periodic", 0, "f64"): 7.980e-16, ("channel", 1, "f64"): 6.928e-16, ("channel", 0, "f64"): 7.980e-16,
    ("periodic", 1, "f32"): 3.632e-07, ("periodic", 0, "f32"): 4.138e-07, ("channel", 1, "f32"): 3.632e-07, ("channel", 0, "f32"): 4.138e-07,
}
LAKE_MARGIN = {k: 10 * v for k, v in LAKE_REFERENCE_DRIFT.items()}
# without the bathymetry the same h is far from rest: the velocity must reach this multiple of the margin
LAKE_UNBALANCED_FACTOR = {"f64": 1e6, "f32": 1e3}


def lake_drift(q, Nx=LAKE_NX, Ny=LAKE_NY):
    I = (slice(H, H + Ny), slice(H, H + Nx))
    return float(max(np.abs(q[0][I]).max(), np.abs(q[1][I]).max()))


# ---- the RK3 property ------------------------------------------------------------------------------------------------------------------
# A uniform tracer c under Relaxation(r) and Source(F0), zero velocity, uniform h, A = 0: every advective tendency is exactly zero and
# c' = F0 - r c, so with c_0 = 0 every step maps the distance to F0 / r by R(-r dt): c_n = (F0 / r)(1 - R(-r dt)^n), R = decay_polynomial's.
RK3_NX, RK3_NY, RK3_STEPS = RC.DECAY_NX, RC.DECAY_NY, RC.DECAY_STEPS
RK3_RATE, RK3_DT, RK3_F0 = RC.DECAY_RATE, RC.DECAY_DT, 0.3
# max |c_20 - c_exact| / c_exact of RefModel("classic") in float64 against the longdouble value (test_source_cases_cpu.py prints it)
RK3_REFERENCE_DEVIATION = 7.645e-16
RK3_MARGIN = 10 * RK3_REFERENCE_DEVIATION


def rk3_exact(steps=RK3_STEPS):
    """c_n in longdouble from the float64 values of r, dt and F0."""
    L = np.longdouble
    return (L(RK3_F0) / L(RK3_RATE)) * (1 - RC.decay_polynomial(steps))


def rk3_deviation(c, steps=RK3_STEPS):
    I = (slice(H, H + RK3_NY), slice(H, H + RK3_NX))
    want = rk3_exact(steps)
    return float(np.abs(c[I].astype(np.longdouble) - want).max() / want)
