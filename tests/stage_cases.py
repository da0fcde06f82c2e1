"""Reference of ONE call of the fused tendency entry points (swmhd_tendencies_*, swmhd_tendencies_rk3_* in include/swmhd.h) and the
matrices of calls made through every kernel path of those entry points (PATHS):
    march        the row-marching kernels (k_tendency_vi_march, k_tendency_cons_march, k_tendency_vi_march_pk): matrix(), run by
                 tests/test_stage_matrix_gpu.py, its forced-layout child processes and tools/stage_matrix_report.py
    tile4, tile8, strict, wall, wall-strict
                 the LDS-tiled kernel k_tendency_tile in its fast 64 x 4 and 64 x 8 bodies, the strict 64 x 8 body and the fast and
                 strict wall bodies (Bounded directions): tile_matrix(), run by tests/test_tile_stage_matrix_gpu.py and
                 tools/stage_matrix_report.py --tile
    ens4, ens8, ens-strict, par4, par-strict
                 the ensemble instantiations of k_tendency_tile behind swmhd_ensemble_tendencies_rk3_* and, with a device table of
                 (g, f, dt) per member, swmhd_ensemble_tendencies_rk3_params_*: ens_matrix(), every member a StageData of its own in
                 pitched family buffers, run by tests/test_ensemble_stage_matrix_gpu.py, its forced-layout child processes and
                 tools/stage_matrix_report.py --ensemble (last section of this file)

Fast paths: the tendencies G come from the CPU oracle in float64 (fp32 inputs widened exactly); the substep is evaluated in
np.longdouble from the formulas of the header.  Strict paths: G is the oracle's in the precision of the call and the substep is
tracer_cases.substep (the oracle's expression order in that precision); both are compared bitwise.  Bounded paths: the oracle with
topo=..., on inputs whose halos hold the boundary conditions (tracer_cases.fill_state, a gradient condition on A where y is Bounded).
The strict and wall paths implement T, S1g, S1n, S2g, S3n only; for the other forms the header promises SWMHD_ENOTSUP, which is
asserted together with "nothing was written".  The reference part (reference_stage, reference_stage_strict, stage_bounds, StageData)
is numpy only; run_stage / check_case need a GPU.

Variants, at the level of the call (which compiled stage MODE a call lands on is launch_plan.hpp's business, pinned by
tests/launch_plan_check.cpp):
    T          swmhd_tendencies                                   Gn = G
    S1g / S1n  first stage (Gm == NULL), store_G 1 / 0            qnew = q + dt gamma G                       Gn = G iff store_G
    S2g / S3n  stage with Gm, store_G 1 / 0                       qnew = q + dt (gamma G + zeta Gm)           Gn = G iff store_G
    P2g / P3n  SWMHD_GM_IS_PREV_STATE, store_G 1 / 0              qnew = q + dt gamma G + zeta' (q - Uprev)   Gn = G iff store_G
               (Gm is passed as the buffers of qnew, which hold Uprev on entry)
    A1         SWMHD_RK3_ANCHOR, Gm == NULL                       qnew = q + dt gamma G                       Gn = W = q + dt zeta G
    A2 / A2a   SWMHD_RK3_ANCHOR with Gm = W                       qnew = W + dt gamma G                       Gn not written
               (A2: Gn is a buffer of its own; A2a: Gn aliases Gm)

Tolerances (all from include/swmhd.h and the tests that precede this one, none fitted to what the kernels give):
    tendencies  max|dG| <= tol * max(max|G|, S), tol = 1e-12 (fp64, rough random fields) / 1e-4 (fp32), S = helpers.term_scales
    new state   max|dqnew| <= dt c (tendency bound) + 4 eps max|operands of the update|: c is the weight G enters with -- |gamma|, and
                |gamma| + |zeta| for the stages that also add zeta Gm -- and 4 eps is the rounding allowance of
                test_second_stage_with_the_previous_state_as_operand.  The operands are the addends of the update (q or W, dt gamma G,
                dt zeta Gm or zeta' (q - Uprev)); the maximum also runs over the result, which is no operand: that is the precedent
                of the test named above (4 eps max|result|), and the result is at most the sum of the addends.  W: the same with zeta.
"""
import json
import os
import sys

import numpy as np

import helpers as Hh
import tracer_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 3                               # halo width in x and y
DX, DY = 0.11, 0.13                 # dx != dy
GRAV, FCOR = Hh.G, Hh.F
SENTINEL = -555.5                   # exact in fp32
KEEP = "must keep its sentinel"
FORM = {0: "Conservative", 1: "VectorInvariant"}
FORMS = [(1, 1), (1, 0), (0, 2), (0, 0)]      # (formulation, lorentz)
DTYPES = [np.float64, np.float32]
TOL = {np.dtype(np.float64): 1e-12, np.dtype(np.float32): 1e-4}
MARCH_KERNEL, WRAP_X, WRAP_Y, GM_IS_PREV_STATE, RK3_ANCHOR = 4, 16, 32, 1024, 2048      # include/swmhd.h
STRICT, TILE_KERNEL, BOUNDED_X, BOUNDED_Y, ENOTSUP = 1, 2, 256, 512, 3                  # include/swmhd.h
P, B = TC.P, TC.B                   # topology codes
NTHREADS = max(1, min(len(os.sched_getaffinity(0)), 8))

# variant: fused substep, operand (None | "Gm" | "Uprev" | "W"), store_G, anchor form, Gn aliases the operand
VARIANTS = {
    "T": dict(fused=False, operand=None, store_G=1, anchor=False, alias=False),
    "S1g": dict(fused=True, operand=None, store_G=1, anchor=False, alias=False),
    "S1n": dict(fused=True, operand=None, store_G=0, anchor=False, alias=False),
    "S2g": dict(fused=True, operand="Gm", store_G=1, anchor=False, alias=False),
    "S3n": dict(fused=True, operand="Gm", store_G=0, anchor=False, alias=False),
    "P2g": dict(fused=True, operand="Uprev", store_G=1, anchor=False, alias=False),
    "P3n": dict(fused=True, operand="Uprev", store_G=0, anchor=False, alias=False),
    "A1": dict(fused=True, operand=None, store_G=0, anchor=True, alias=False),
    "A2": dict(fused=True, operand="W", store_G=1, anchor=True, alias=False),     # (store_G is ignored in anchor form: Gn stays)
    "A2a": dict(fused=True, operand="W", store_G=0, anchor=True, alias=True),
}
# (gamma, zeta) as the call receives them.  "rk3": Oceananigans' values, stage by stage; for P* zeta' = zeta / gamma-, for A1 the weight of
# W.  "generic": one pair without the identities gamma1 + zeta2 = 1/4 and zeta3 = -gamma2 that could hide a wrong operand -- also
# passed where the header says zeta is unused (first stages, A2), which must then ignore it.
_G1, _G2, _G3, _Z2, _Z3 = 8.0 / 15.0, 5.0 / 12.0, 3.0 / 4.0, -17.0 / 60.0, -5.0 / 12.0
COEFFS = {
    "rk3": {"T": (0.0, 0.0), "S1g": (_G1, 0.0), "S1n": (_G1, 0.0), "S2g": (_G2, _Z2), "S3n": (_G3, _Z3), "P2g": (_G2, _Z2 / _G1),
            "P3n": (_G3, _Z3 / _G2), "A1": (_G1, 0.25), "A2": (_G2, 0.0), "A2a": (_G3, 0.0)},
    "generic": {v: (0.37, -0.21) for v in VARIANTS if v != "T"},
}


def calls():
    """Every (variant, coefficient set) of the matrix; T has no coefficients and runs once."""
    return [(v, c) for v in VARIANTS for c in COEFFS if v in COEFFS[c]]


# Kernel paths.  flags: what selects the path (a wall path adds SWMHD_BOUNDED_* from the topology of its StageData); strict: compared
# bitwise; wall: a Bounded direction; ty: rows of a tile (None: not a tile kernel); refused: the call forms the path answers with
# SWMHD_ENOTSUP (SWMHD_GM_IS_PREV_STATE and SWMHD_RK3_ANCHOR are fast and periodic only).
FAST_ONLY = ("P2g", "P3n", "A1", "A2", "A2a")
PATHS = {
    "march": dict(flags=MARCH_KERNEL, strict=False, wall=False, ty=None, refused=()),
    "tile4": dict(flags=TILE_KERNEL, strict=False, wall=False, ty=4, refused=()),
    "tile8": dict(flags=TILE_KERNEL, strict=False, wall=False, ty=8, refused=()),
    "strict": dict(flags=STRICT, strict=True, wall=False, ty=8, refused=FAST_ONLY),
    "wall": dict(flags=TILE_KERNEL, strict=False, wall=True, ty=8, refused=FAST_ONLY),
    "wall-strict": dict(flags=STRICT, strict=True, wall=True, ty=8, refused=FAST_ONLY),
}


def topo_flags(topo):
    return (BOUNDED_X if topo[0] == B else 0) | (BOUNDED_Y if topo[1] == B else 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs and the oracle's tendencies, once per (shape, formulation, forcing, precision)
# ---------------------------------------------------------------------------------------------------------------------------------
def random_fields(Nx, Ny, form, dtype, seed):
    """(q, aux): the state as test_model_gpu.random_state makes it (rough random fields, halos periodic-filled), each field from a
    stream of its own, and four independent fields of the same make for Gm / W / Uprev whose halos hold the sentinel."""
    shp = (Ny + 2 * H, Nx + 2 * H)
    out = []
    for base in (0, 4):
        r = [np.random.default_rng([seed, base + k]) for k in range(4)]
        u, v = 0.5 * r[0].standard_normal(shp), 0.5 * r[1].standard_normal(shp)
        h = 1.0 + 0.3 * r[2].random(shp)
        A = r[3].standard_normal(shp)
        q1, q2 = (u, v) if form == 1 else (h * u, h * v)
        out.append([np.ascontiguousarray(Hh.fill_halo_periodic(a, Nx, Ny, H, H).astype(dtype)) for a in (q1, q2, h, A)])
    q, aux = out
    for a in aux:
        keep = Hh.interior(a, Nx, Ny, H, H).copy()
        a[...] = SENTINEL
        Hh.interior(a, Nx, Ny, H, H)[...] = keep
    return q, aux


class StageData:
    """Inputs of one (shape, formulation, forcing, precision, topology) and the oracle's float64 tendencies of them.  With a Bounded
    direction the halos of q hold the boundary conditions (tracer_cases.fill_state in the precision of the call: impenetrable walls,
    no-flux mirrors, the gradient condition tracer_cases.grad_A on A where y is Bounded) and the oracle runs with that topology;
    wall_failures then says whether its result differs from the periodic one inside the wall buffers and nowhere else."""

    # defaults of a subclass that builds its own (periodic) inputs without this constructor (tests/test_weno_arith_gpu.py)
    topo, wall_failures, _G_strict = (P, P), (), None

    def __init__(self, oracle, Nx, Ny, form, lor, dtype, seed=None, topo=(P, P), grav=None, fcor=None):
        self.Nx, self.Ny, self.form, self.lor, self.dtype, self.topo = Nx, Ny, form, lor, np.dtype(dtype), tuple(topo)
        seed = 1000 * Nx + Ny if seed is None else seed
        self.q, self.aux = random_fields(Nx, Ny, form, dtype, seed)
        # spacings and constants as the call receives them (c_float rounds 0.11, 0.13 and 9.81); grav, fcor: the g and f of a member of
        # an ensemble with per-member parameters (None: the constants of every other case)
        own = grav is not None or fcor is not None
        self.dx, self.dy, self.grav, self.fcor = (float(self.dtype.type(x)) for x in (DX, DY, GRAV if grav is None else grav,
                                                                                      FCOR if fcor is None else fcor))
        kw = {}
        if self.topo != (P, P):
            TC.fill_state(oracle, self.q, Nx, Ny, self.topo, TC.grad_A(self.topo), self.dx, self.dy)
            kw = dict(topo=self.topo)
        q64 = [a.astype(np.float64) for a in self.q]                      # exact widening
        G = oracle.tendencies(*q64, Nx, Ny, H, H, self.dx, self.dy, form, lor, self.grav, self.fcor, nthreads=NTHREADS, **kw)
        self.G = [Hh.interior(g, Nx, Ny, H, H).copy() for g in G]
        force = 0.0
        if lor:
            w = (oracle.lorentz_jacobian(q64[3], q64[2], Nx, Ny, H, H, self.dx, self.dy, nthreads=NTHREADS) if lor == 1 else
                 oracle.lorentz_divergence(q64[3], q64[2], Nx, Ny, H, H, self.dx, self.dy, nthreads=NTHREADS, **kw))
            force = max(float(np.abs(Hh.interior(x, Nx, Ny, H, H)).max()) for x in w)
        # (the S of a member with its own g and f is formed with them: a smaller g must not keep the bound of 9.81)
        own = dict(g=self.grav, f=abs(self.fcor)) if own else {}
        self.scales = [float(s) for s in Hh.term_scales(FORM[form], q64, self.dx, self.dy, force, **own)]
        self.Gmax = [float(np.abs(g).max()) for g in self.G]
        self.Umax = [float(np.abs(Hh.interior(a, Nx, Ny, H, H)).max()) for a in q64]
        self._oracle, self._G_strict = oracle, None
        self.wall_failures = wall_buffer_failures(oracle, self, q64) if self.topo != (P, P) else []

    def G_strict(self):
        """The oracle's tendencies in the precision of the call (parents): what a strict call must give bit for bit."""
        if self._G_strict is None:
            kw = dict(topo=self.topo) if self.topo != (P, P) else {}
            self._G_strict = self._oracle.tendencies(*self.q, self.Nx, self.Ny, H, H, self.dx, self.dy, self.form, self.lor, self.grav,
                                                     self.fcor, nthreads=NTHREADS, **kw)
        return self._G_strict

    def dt(self, gamma):
        """dt with dt |gamma| max|G| = max|U| (maxima over the four fields): one stage has no stability limit, and an increment of the
        size of the state makes qnew as sharp a witness of G as Gn is.  Rounded to the precision of the call."""
        if gamma == 0.0:
            return 0.0
        return float(self.dtype.type(max(self.Umax) / (abs(gamma) * max(self.Gmax))))


def reference_stage(oracle, q, operand, variant, coeffs, Nx, Ny, dx, dy, form, lor, dt, rows=None, G=None):
    """Expected interior rows [j0, j1) of every output of one call: {"qnew": 4 arrays | None (the call has none), "Gn": 4 arrays | KEEP}.
    q: halo-filled parents in the precision of the call; operand: the parents of Gm / W / Uprev (None: first-stage forms);
    coeffs: (gamma, zeta) as passed; G: the oracle's float64 interior tendencies if the caller has them already."""
    v = VARIANTS[variant]
    j0, j1 = (0, Ny) if rows is None else rows
    dtype = q[0].dtype
    if G is None:
        q64 = [a.astype(np.float64) for a in q]
        G = [Hh.interior(g, Nx, Ny, H, H) for g in oracle.tendencies(*q64, Nx, Ny, H, H, dx, dy, form, lor, float(dtype.type(GRAV)),
                                                                        float(dtype.type(FCOR)), nthreads=NTHREADS)]
    G = [np.asarray(g[j0:j1], dtype=np.float64) for g in G]
    if not v["fused"]:
        return {"qnew": None, "Gn": G}
    LD = np.longdouble
    cut = lambda a: Hh.interior(a, Nx, Ny, H, H)[j0:j1].astype(LD)
    gam, zet, dtl = (LD(dtype.type(x)) for x in (coeffs[0], coeffs[1], dt))     # the values the kernel receives
    U, Gl = [cut(a) for a in q], [g.astype(LD) for g in G]
    Op = [cut(a) for a in operand] if v["operand"] else None
    if v["anchor"] and Op is None:
        return {"qnew": [u + dtl * gam * g for u, g in zip(U, Gl)], "Gn": [u + dtl * zet * g for u, g in zip(U, Gl)]}
    if v["anchor"]:
        return {"qnew": [w + dtl * gam * g for w, g in zip(Op, Gl)], "Gn": KEEP}
    if Op is None:
        qnew = [u + dtl * gam * g for u, g in zip(U, Gl)]
    elif v["operand"] == "Uprev":
        qnew = [u + dtl * gam * g + zet * (u - p) for u, g, p in zip(U, Gl, Op)]
    else:
        qnew = [u + dtl * (gam * g + zet * m) for u, g, m in zip(U, Gl, Op)]
    return {"qnew": qnew, "Gn": G if v["store_G"] else KEEP}


def reference_stage_strict(data, variant, coeffs, dt, rows=None):
    """reference_stage for a strict call, to be compared bitwise: Gn is the oracle's tendency in the precision of the call, qnew is
    tracer_cases.substep (U + dt gamma G | U + dt (gamma G + zeta Gm), each operation rounded to that precision in the oracle's
    order) of the parents.  The call forms of the strict paths only (no previous-state operand, no anchor)."""
    v = VARIANTS[variant]
    assert not v["anchor"] and v["operand"] in (None, "Gm"), variant
    Nx, Ny = data.Nx, data.Ny
    j0, j1 = (0, Ny) if rows is None else rows
    cut = lambda a: Hh.interior(a, Nx, Ny, H, H)[j0:j1]
    G = data.G_strict()
    if not v["fused"]:
        return {"qnew": None, "Gn": [cut(g) for g in G]}
    Gm = data.aux if v["operand"] else [None] * 4
    qnew = [cut(TC.substep(U, g, m, Nx, Ny, dt, coeffs[0], coeffs[1], m is None)) for U, g, m in zip(data.q, G, Gm)]
    return {"qnew": qnew, "Gn": [cut(g) for g in G] if v["store_G"] else KEEP}


WALL_DEPTH = 7      # cells from a wall beyond which the Bounded tendencies are the periodic ones (test_bounded_oracle: the boundary
                    # buffers are 2 interpolation points deep, the widest stencil reaches 3 cells, +1 for the flux differences, +3
                    # for the divergence forcing's face quantities)


def wall_buffers(Nx, Ny, topo):
    """{"west" | "east" | "south" | "north": boolean mask of the interior cells within WALL_DEPTH of that wall}, Bounded sides only."""
    y, x = np.meshgrid(np.arange(Ny), np.arange(Nx), indexing="ij")
    out = {}
    if topo[0] == B:
        out["west"], out["east"] = x < WALL_DEPTH, x >= Nx - WALL_DEPTH
    if topo[1] == B:
        out["south"], out["north"] = y < WALL_DEPTH, y >= Ny - WALL_DEPTH
    return out


def wall_buffer_failures(oracle, data, q64):
    """The Bounded reference of `data` against the periodic one of the same interior (halos periodic-filled instead): it must differ
    inside the buffer of every wall and equal it bit for bit outside all of them.  A matrix whose reference never took a wall branch
    fails here.  Returns one line per violation."""
    Nx, Ny = data.Nx, data.Ny
    qp = [oracle.fill_halo_periodic(a.copy(), Nx, Ny, H, H) for a in q64]
    Gp = [Hh.interior(g, Nx, Ny, H, H) for g in oracle.tendencies(*qp, Nx, Ny, H, H, data.dx, data.dy, data.form, data.lor, data.grav,
                                                                    data.fcor, nthreads=NTHREADS)]
    differs = np.zeros((Ny, Nx), dtype=bool)
    for gb, gp in zip(data.G, Gp):
        differs |= gb != gp
    buffers = wall_buffers(Nx, Ny, data.topo)
    near = np.zeros((Ny, Nx), dtype=bool)
    fails = []
    for side, mask in buffers.items():
        near |= mask
        if not (differs & mask).any():
            fails.append(f"the Bounded reference equals the periodic one in the whole {side} wall buffer")
    if (differs & ~near).any():
        fails.append(f"the Bounded reference differs from the periodic one in {int((differs & ~near).sum())} cells outside the wall buffers")
    return fails


def stage_bounds(data, q, operand, variant, coeffs, dt, ref, rows=None):
    """Allowed max-norm error of each written output, per field: {"qnew": [4] | None, "Gn": [4] | None} (module docstring)."""
    v = VARIANTS[variant]
    j0, j1 = (0, data.Ny) if rows is None else rows
    eps = float(np.finfo(data.dtype).eps)
    gam, zet = (abs(float(data.dtype.type(x))) for x in coeffs)
    tb = [TOL[data.dtype] * max(gm, s) for gm, s in zip(data.Gmax, data.scales)]
    if not v["fused"]:
        return {"qnew": None, "Gn": tb}
    cut = lambda a: Hh.interior(a, data.Nx, data.Ny, H, H)[j0:j1].astype(np.float64)
    amax = lambda a: float(np.abs(a).max())
    out = {"qnew": [], "Gn": None}
    for f in range(4):
        U = cut(q[f])
        terms = [amax(ref["qnew"][f]), dt * gam * data.Gmax[f]]
        weight = gam
        if v["operand"] == "W":
            terms.append(amax(cut(operand[f])))
        else:
            terms.append(amax(U))
        if v["operand"] == "Gm":
            terms.append(dt * zet * amax(cut(operand[f])))
            weight = gam + zet
        if v["operand"] == "Uprev":
            terms.append(zet * amax(U - cut(operand[f])))
        out["qnew"].append(dt * weight * tb[f] + 4 * eps * max(terms))
    if v["anchor"] and v["operand"] is None:      # W through the G pointers
        out["Gn"] = [dt * zet * tb[f] + 4 * eps * max(amax(cut(q[f])), dt * zet * data.Gmax[f], amax(ref["Gn"][f])) for f in range(4)]
    elif ref["Gn"] is not KEEP:
        out["Gn"] = tb
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# layouts: what each width and row count of the matrix is there for, asserted against swmhd_tendency_launch_geometry
# ---------------------------------------------------------------------------------------------------------------------------------
TXO = {256: 250, 128: 122}          # output columns of a strip
PACKED_TXO = 504
# Nx: (lanes, strips, output columns of the last strip) of the default chooser for both formulations and precisions (unpacked)
LAYOUTS = {
    250: (256, 1, 250),     # one strip, exactly full
    2501: (256, 11, 1),     # last strip of ONE column (the smallest such width that keeps 256 lanes: at 251 ... 2251 the chooser
                            # takes 128-lane strips); folds in the fp64 vector-invariant kernel
    372: (256, 2, 122),     # the widest last strip that folds
    373: (256, 2, 123),     # does not fold
    500: (256, 2, 250),     # two full strips
    100: (128, 1, 100),     # one partial 128-lane strip
    251: (128, 3, 7),       # 128-lane strips with a 7-column tail (what the chooser makes of 250 + 1)
    366: (128, 3, 122),     # three exactly full strips
    600: (128, 5, 112),     # five strips, 112-column tail
    3: (128, 1, 3),         # Nx = Hx, the smallest width WRAP allows
    7: (128, 1, 7),
}
PACKED_WIDTHS = {8: (1, 8), 504: (1, 504), 506: (2, 2), 1000: (2, 496)}     # strips, output columns of the last strip
ROWS = {3: (1, 3), 25: (5, 1), 31: (6, 1), 33: (6, 3), 24: (4, 6)}           # launch rows: (segments of 6 rows, rows of the last one)
PARTIAL = (5, 29)                   # j_begin = 5, j_end = Ny - 4 on Ny = 33


def is_packed(Nx, form, dtype, flags):
    return np.dtype(dtype) == np.float32 and form == 1 and bool(flags & WRAP_X) and Nx % 2 == 0 and Nx >= 8


def family(Nx, form, dtype, flags, path="march"):
    """Key of the achieved-ratio tables: the marching kernel family, or the tile path."""
    if path != "march":
        return path
    return "packed" if is_packed(Nx, form, dtype, flags) else ("vi" if form == 1 else "cons")


def fold_enabled():
    """The environment lets the launcher fold (launch_plan.hpp tendency_fold_enabled: SWMHD_T_FOLD unset or non-zero)."""
    e = os.environ.get("SWMHD_T_FOLD")
    try:
        return e is None or int(e.strip() or 0) != 0
    except ValueError:
        return False          # atoi of a non-number is 0


def folds(Nx, form, dtype, geo):
    """The launch folds its last strip.  INFERRED, not queried: swmhd_tendency_launch_geometry does not report the fold, so this
    restates launch_plan.hpp (fp64 vector-invariant, 256 lanes, more than one strip, tail <= 122, SWMHD_T_FOLD not 0).  With
    SWMHD_T_FOLD=0 in the environment nothing folds: fold_enabled() is what the GPU module asserts before it relies on this."""
    if not fold_enabled():
        return False
    return (form == 1 and np.dtype(dtype) == np.float64 and geo["kind"] == 2 and geo["threads"] == 256 and geo["nstrips"] > 1
            and Nx - (geo["nstrips"] - 1) * TXO[256] <= 122)


TILE_X = 64                         # columns of a tile (common.hpp TILE_X)
TILE_MIN_CELLS_RY2 = 330000         # launch_plan.hpp SW_MARCH_MIN_CELLS: forced onto the tile kernel, launches of that many cells keep 64 x 8 tiles


def tiles(n, t):
    """(tiles, cells of the last one) of n cells cut into tiles of t."""
    nt = -(-n // t)
    return nt, n - (nt - 1) * t


def wall_tiles(Nx, nrows):
    """(tile columns, tile rows, rows of a tile) of a Bounded launch.  INFERRED, not queried: swmhd_tendency_launch_geometry does not
    model the topology, so this restates launch_plan.hpp plan_tendency (pinned by tests/launch_plan_check.cpp): a Bounded grid runs on
    the wall kernel, 64 x 8 tiles over every row of the range, unless it is a fast launch of SW_MARCH_MIN_CELLS cells or more, at least
    256 columns and 48 rows that does NOT force the tile kernel -- then the marching kernel runs first and the wall kernel only
    overwrites a frame.  The wall paths force the tile kernel (SWMHD_TILE_KERNEL, or SWMHD_STRICT, which has no other), and their shapes
    also lie below every one of those thresholds, which is what this asserts."""
    assert Nx * nrows < TILE_MIN_CELLS_RY2 and (Nx < 4 * TILE_X or nrows < 48), (Nx, nrows)
    return tiles(Nx, TILE_X)[0], tiles(nrows, 8)[0], 8


def check_tile_layout(L, path, Nx, nrows, form, dtype, flags):
    """check_layout of the tile paths: kind 1, ceil(Nx / 64) tile columns, and the tile height the path is there for (4 rows for
    tile4, 8 for tile8 and strict) from the planner's own answer for SWMHD_TILE_KERNEL (| SWMHD_STRICT) and the rows of the launch;
    the wall paths take the height from wall_tiles."""
    p = PATHS[path]
    q = TILE_KERNEL | (STRICT if p["strict"] else 0) | (flags & (WRAP_X | WRAP_Y))
    geo = L.tendency_launch_geometry(Nx, nrows, form, np.dtype(dtype).itemsize, q)
    ntx, lastx = tiles(Nx, TILE_X)
    assert (geo["kind"], geo["nstrips"]) == (1, ntx), (path, Nx, nrows, geo)
    if p["wall"]:
        wx, nty, ty = wall_tiles(Nx, nrows)
        assert wx == ntx
        note = " (wall kernel: inferred)"
    else:
        ty, nty, note = p["ty"], tiles(nrows, p["ty"])[0], ""
        assert (geo["rows_per_segment"], geo["nseg"]) == (ty, nty), (path, Nx, nrows, geo)
    lasty = tiles(nrows, ty)[1]
    return f"kind 1, {ntx} tile columns, last {lastx} wide, {nty} tile rows of {ty}, last {lasty}{note}"


def check_layout(L, Nx, nrows, form, dtype, flags, lanes=None, LY=6, layouts=LAYOUTS, path="march"):
    """Assert that the launch of Nx x nrows has the layout the matrix wants from this shape; returns a one-line description."""
    if path != "march":
        return check_tile_layout(L, path, Nx, nrows, form, dtype, flags)
    elem = np.dtype(dtype).itemsize
    geo = L.tendency_launch_geometry(Nx, nrows, form, elem, MARCH_KERNEL | (flags & (WRAP_X | WRAP_Y)))
    if is_packed(Nx, form, dtype, flags):
        strips = -(-Nx // PACKED_TXO)
        assert (geo["kind"], geo["threads"], geo["nstrips"]) == (3, 256, strips), (Nx, geo)
        if Nx in PACKED_WIDTHS:
            assert PACKED_WIDTHS[Nx] == (strips, Nx - (strips - 1) * PACKED_TXO), (Nx, geo)
        tail = Nx - (strips - 1) * PACKED_TXO
    else:
        want = layouts[Nx] if lanes is None else (lanes, -(-Nx // TXO[lanes]), Nx - (-(-Nx // TXO[lanes]) - 1) * TXO[lanes])
        tail = Nx - (geo["nstrips"] - 1) * TXO[geo["threads"]]
        assert (geo["kind"], geo["threads"], geo["nstrips"], tail) == (2,) + want, (Nx, geo, want)
    nseg, last = -(-nrows // LY), nrows - (-(-nrows // LY) - 1) * LY
    assert (geo["rows_per_segment"], geo["nseg"]) == (LY, nseg), (nrows, geo)
    if LY == 6:
        assert ROWS[nrows] == (nseg, last), (nrows, geo)
    fold = folds(Nx, form, dtype, geo)
    return (f"kind {geo['kind']}, {geo['threads']} lanes, {geo['nstrips']} strips, last strip {tail} columns"
            f"{' (folded)' if fold else ''}, {nseg} segments of {LY} rows, last {last}")


def shape_groups():
    """(Nx, Ny, rows | None, [flags], packed-only) of the matrix: every width with Ny = 31; every Ny with the widths 2501, 372, 600
    and (packed) 506; one partial row range; WRAP_X alone and WRAP_Y alone once per kernel family.  2501 stands where 251 was meant
    as the 256-lane width with a one-column last strip (at 251 the chooser takes three 128-lane strips); 251 itself runs at Ny = 31
    only, as a 128-lane class with a 7-column tail."""
    XY = WRAP_X | WRAP_Y
    out = [(Nx, 31, None, [0, XY, WRAP_X, WRAP_Y] if Nx == 372 else [0, XY], False) for Nx in LAYOUTS]
    out += [(Nx, Ny, None, [0, XY], False) for Nx in (2501, 372, 600) for Ny in (3, 25, 33)]
    out += [(372, 33, PARTIAL, [0, XY], False)]
    out += [(Nx, 31, None, [XY, WRAP_X], True) for Nx in PACKED_WIDTHS]
    out += [(506, Ny, None, [XY], True) for Ny in (3, 25, 33)]
    out += [(506, 33, PARTIAL, [XY], True)]
    return out


def matrix():
    """Every (Nx, Ny, rows, form, lor, dtype, flags) of the matrix, grouped so that consecutive entries share their StageData."""
    for Nx, Ny, rows, flagsets, packed_only in shape_groups():
        for form, lor in FORMS:
            for dtype in DTYPES:
                if packed_only and not (form == 1 and dtype == np.float32):
                    continue
                for flags in flagsets:
                    yield Nx, Ny, rows, form, lor, dtype, flags


def case_id(Nx, Ny, rows, form, lor, dtype, flags):
    wrap = {0: "nowrap", WRAP_X: "wrapX", WRAP_Y: "wrapY", WRAP_X | WRAP_Y: "wrapXY"}[flags]
    return (f"{Nx}x{Ny}{'' if rows is None else f'-rows{rows[0]}to{rows[1]}'}-{'vi' if form == 1 else 'cons'}-lor{lor}-"
            f"{'f64' if dtype == np.float64 else 'f32'}-{wrap}")


# ---------------------------------------------------------------------------------------------------------------------------------
# the tile matrix: the smallest shapes at which a 64-wide tile of 4 or 8 rows can go wrong
# ---------------------------------------------------------------------------------------------------------------------------------
TILE_WIDTHS = (3, 7, 63, 64, 65, 129)     # Nx = Hx (every tile cell beyond x = 2 is a wrapped or clamped load); 7; below, at and above
                                          # one tile; three tile columns, the last of one column
TILE_ROWS = (3, 4, 5, 8, 9, 31)           # below, at and above one 4-row tile; at and above one 8-row tile; 8 | 4 tile rows, last of 3 | 7
TILE8_SHAPE = (2579, 129)                 # 332 691 cells: 41 tile columns, the last 19 wide; 17 tile rows of 8, the last of one row
WALL_SHAPES = [(65, 9), (67, 11), (64, 8), (7, 8), (129, 31)]     # a tile edge 1 and 3 cells from the east / north wall (inside its
                                          # boundary buffer, at its start), on the wall, the buffers of opposite walls meet, several tiles a side
WALL_TOPOS = [(P, B), (B, P), (B, B)]
WALL_FORMS = [(1, 1), (0, 2), (0, 0)]     # the divergence forcing has wall branches of its own


def tile_shape_groups():
    """(Nx, Ny, rows | None, [flags]) of the periodic tile paths tile4 and strict: every width at Ny = 9 (65 also with WRAP_X alone and
    WRAP_Y alone); every row count at the widths 65 and 129; the partial row range at 129 x 33."""
    XY = WRAP_X | WRAP_Y
    out = [(Nx, 9, None, [0, XY, WRAP_X, WRAP_Y] if Nx == 65 else [0, XY]) for Nx in TILE_WIDTHS]
    out += [(Nx, Ny, None, [0, XY]) for Nx in (65, 129) for Ny in TILE_ROWS if Ny != 9]
    out += [(129, 33, PARTIAL, [0, XY])]
    return out


def wall_shape_groups():
    """(Nx, Ny, rows | None, topology, [flags]) of the wall paths: WRAP in the periodic direction of (P, B) and of (B, P) once, at 65 x 9."""
    out = []
    for Nx, Ny, rows in [(Nx, Ny, None) for Nx, Ny in WALL_SHAPES] + [(129, 33, PARTIAL)]:
        for topo in WALL_TOPOS:
            wrap = {(P, B): [WRAP_X], (B, P): [WRAP_Y]}.get(topo, []) if (Nx, Ny) == (65, 9) else []
            out.append((Nx, Ny, rows, topo, [0] + wrap))
    return out


def tile_matrix():
    """Every (path, Nx, Ny, rows, form, lor, dtype, flags, topology) of the tile matrix, grouped so that consecutive entries share
    their StageData.  tile8 runs whole row ranges only: the planner counts the rows of the launch, a partial range of TILE8_SHAPE
    would fall back to 64 x 4 tiles."""
    for Nx, Ny, rows, flagsets in tile_shape_groups():
        for form, lor in FORMS:
            for dtype in DTYPES:
                for path in ("tile4", "strict"):
                    for flags in flagsets:
                        yield path, Nx, Ny, rows, form, lor, dtype, flags, (P, P)
    for form, lor in FORMS:
        for dtype in DTYPES:
            for flags in (0, WRAP_X | WRAP_Y):
                yield ("tile8",) + TILE8_SHAPE + (None, form, lor, dtype, flags, (P, P))
    for Nx, Ny, rows, topo, flagsets in wall_shape_groups():
        for form, lor in WALL_FORMS:
            for dtype in DTYPES:
                for path in ("wall", "wall-strict"):
                    for flags in flagsets:
                        yield path, Nx, Ny, rows, form, lor, dtype, flags, topo


def tile_case_id(path, Nx, Ny, rows, form, lor, dtype, flags, topo=(P, P)):
    t = "" if tuple(topo) == (P, P) else "-" + "".join("PB"[d] for d in topo)
    return f"{path}{t}-{case_id(Nx, Ny, rows, form, lor, dtype, flags)}"


_DATA = {}


def stage_data(oracle, Nx, Ny, form, lor, dtype, topo=(P, P)):
    """StageData of a shape, computed once (the oracle is not called per case); only the latest width is kept."""
    key = (Nx, Ny, form, lor, np.dtype(dtype).name, tuple(topo))
    if key not in _DATA:
        for k in [k for k in _DATA if k[:2] != (Nx, Ny)]:
            del _DATA[k]
        _DATA[key] = StageData(oracle, Nx, Ny, form, lor, dtype, topo=topo)
    return _DATA[key]


# ---------------------------------------------------------------------------------------------------------------------------------
# one call on the GPU, and its comparison
# ---------------------------------------------------------------------------------------------------------------------------------
def _same_bits(a, b):
    u = np.uint64 if a.dtype.itemsize == 8 else np.uint32
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(u), np.ascontiguousarray(b).view(u))


def run_stage(S, data, variant, cset, flags=0, rows=None, path="march", expect_rc=0, dt=None):
    """One call through the C-ABI with the flags of `path` (SWMHD_MARCH_KERNEL by default; the Bounded flags of data.topo) | flags.
    Inputs: data.q with NaN in the halos of every wrapped direction; the operand data.aux (sentinel halos).  Every output buffer starts
    as the sentinel (qnew of P*: as Uprev).  The return code must be expect_rc.  Returns the parents before and after:
    {"q": (before, after), "operand": ..., "qnew": ..., "Gn": ...} (None where the call has no such buffer).  dt: the time step of the
    call where it is not data.dt(gamma) (a member of an ensemble that steps at the ensemble's dt)."""
    import torch
    L = S._lib
    v = VARIANTS[variant]
    Nx, Ny = data.Nx, data.Ny
    j0, j1 = (0, Ny) if rows is None else rows
    gam, zet = COEFFS[cset][variant]
    dt = data.dt(gam) if dt is None else dt
    sfx = "f64" if data.dtype == np.float64 else "f32"
    q_in = [a.copy() for a in data.q]
    for a in q_in:
        Hh.poison_halo(a, Nx, Ny, H, H, x=bool(flags & WRAP_X), y=bool(flags & WRAP_Y))
    sent = np.full_like(data.q[0], SENTINEL)
    dev = lambda arrs: [torch.from_numpy(a).cuda() for a in arrs]
    PA = lambda ts: L.ptr_array([t.data_ptr() for t in ts])
    tq = dev(q_in)
    before = {"q": q_in, "operand": None, "qnew": None, "Gn": [sent] * 4}
    top = tnew = None
    if v["operand"]:
        top, before["operand"] = dev(data.aux), data.aux
    if v["fused"]:
        if v["operand"] == "Uprev":
            tnew, before["qnew"] = top, data.aux       # the new state goes into the buffers that hold the previous one
        else:
            tnew, before["qnew"] = dev([sent] * 4), [sent] * 4
    if v["alias"]:
        tGn, before["Gn"] = top, data.aux
    else:
        tGn = dev([sent] * 4)
    assert PATHS[path]["wall"] == (data.topo != (P, P)), (path, data.topo)
    fl = PATHS[path]["flags"] | topo_flags(data.topo) | flags | (GM_IS_PREV_STATE if v["operand"] == "Uprev" else 0) | (RK3_ANCHOR if v["anchor"] else 0)
    sy = Nx + 2 * H
    if not v["fused"]:
        rc = getattr(L.lib(), f"swmhd_tendencies_{sfx}")(*[t.data_ptr() for t in tq], *[t.data_ptr() for t in tGn], Nx, Ny, H, H, sy,
                                                           data.dx, data.dy, data.grav, data.fcor, data.form, data.lor, j0, j1, fl, None)
    else:
        rc = getattr(L.lib(), f"swmhd_tendencies_rk3_{sfx}")(PA(tq), PA(tnew), PA(tGn), PA(top) if top is not None else None, Nx, Ny, H, H, sy,
                                                               data.dx, data.dy, data.grav, data.fcor, data.form, data.lor, dt, gam, zet, v["store_G"], j0, j1,
                                                               fl, None)
    if expect_rc == 0:
        L.check(rc, f"{variant}/{cset}")
    assert rc == expect_rc, f"{variant}/{cset}: rc={rc}, expected {expect_rc}"
    torch.cuda.synchronize()
    host = lambda ts: None if ts is None else [t.cpu().numpy() for t in ts]
    after = {"q": host(tq), "operand": host(top), "qnew": host(tnew), "Gn": host(tGn)}
    return {k: (before[k], after[k]) for k in before}


def check_refusal(S, data, variant, cset, flags=0, rows=None, path="strict"):
    """A call form the path does not implement: the call must return SWMHD_ENOTSUP and leave every buffer it was given bitwise as it
    was (the refusal precedes the first launch).  Returns the failures."""
    try:
        out = run_stage(S, data, variant, cset, flags, rows, path=path, expect_rc=ENOTSUP)
    except AssertionError as e:
        return [str(e)]
    fails = []
    for name, (before, after) in out.items():
        for f in range(4 if after is not None else 0):
            if not _same_bits(before[f], after[f]):
                fails.append(f"refused call changed {name}[{f}] in {int((before[f] != after[f]).sum())} cells")
    return fails


def check_case(S, oracle, data, variant, cset, flags=0, rows=None, path="march"):
    """run_stage against reference_stage: (failures, ratios).  failures: one line per violated assertion (empty: the case passes);
    ratios: {"qnew" | "Gn": largest error / bound over the four fields} of the outputs the call writes.  Strict paths are compared
    bitwise with reference_stage_strict (ratio 0: every written cell equal; inf otherwise); a form the path refuses: check_refusal."""
    v = VARIANTS[variant]
    if variant in PATHS[path]["refused"]:
        return check_refusal(S, data, variant, cset, flags, rows, path), {}
    Nx, Ny = data.Nx, data.Ny
    j0, j1 = (0, Ny) if rows is None else rows
    coeffs = COEFFS[cset][variant]
    dt = data.dt(coeffs[0])
    operand = data.aux if v["operand"] else None
    if PATHS[path]["strict"]:
        ref, bounds = reference_stage_strict(data, variant, coeffs, dt, rows=rows), None
    else:
        ref = reference_stage(oracle, data.q, operand, variant, coeffs, Nx, Ny, data.dx, data.dy, data.form, data.lor, dt, rows=rows, G=data.G)
        bounds = stage_bounds(data, data.q, operand, variant, coeffs, dt, ref, rows=rows)
    out = run_stage(S, data, variant, cset, flags, rows, path=path)
    fails, ratios = [], {}
    # 3. inputs bitwise unchanged (Uprev of P* is the qnew buffer; the aliased Gn of A2a is the operand W)
    for f in range(4):
        if not _same_bits(*[x[f] for x in out["q"]]):
            fails.append(f"input field {f} was changed")
        if v["operand"] and v["operand"] != "Uprev" and not _same_bits(*[x[f] for x in out["operand"]]):
            fails.append(f"operand {v['operand']} field {f} was changed")
    for name in ("qnew", "Gn"):
        if out[name][1] is None or (name == "Gn" and v["alias"]):
            continue
        for f in range(4):
            b, a = out[name][0][f], out[name][1][f]
            if ref[name] is KEEP:
                # 2. an output the call must not write: bitwise its sentinel everywhere
                if not _same_bits(a, b):
                    fails.append(f"{name}[{f}] must keep its sentinel: {int((a != b).sum())} cells written")
                continue
            # 2. halos and rows outside [j_begin, j_end): bitwise what they held
            a_out, b_out = a.copy(), b.copy()
            a_out[H + j0:H + j1, H:H + Nx] = 0
            b_out[H + j0:H + j1, H:H + Nx] = 0
            if not _same_bits(a_out, b_out):
                fails.append(f"{name}[{f}]: {int((a_out != b_out).sum())} cells written outside rows [{j0}, {j1}) of the interior")
            # 1. finite and within tolerance over the whole range, max-norm
            got = a[H + j0:H + j1, H:H + Nx].astype(np.longdouble)
            if not np.isfinite(got).all():
                fails.append(f"{name}[{f}]: {int((~np.isfinite(got)).sum())} non-finite cells")
                ratios[name] = float("inf")
                continue
            if bounds is None:      # strict: every written cell equal to the reference in the precision of the call
                same = a[H + j0:H + j1, H:H + Nx] == ref[name][f]
                ratios[name] = max(ratios.get(name, 0.0), 0.0 if same.all() else float("inf"))
                if not same.all():
                    fails.append(f"{name}[{f}]: {int((~same).sum())} cells differ from the oracle's, max |difference| "
                                 f"{float(np.abs(got - ref[name][f]).max()):.3e}")
                continue
            err, bound = float(np.abs(got - ref[name][f]).max()), bounds[name][f]
            ratios[name] = max(ratios.get(name, 0.0), err / bound)
            if not err <= bound:
                fails.append(f"{name}[{f}]: max error {err:.3e} > bound {bound:.3e}")
    return fails, ratios


def run_cases(S, oracle, Nx, Ny, rows, form, lor, dtype, flags, worst=None, stop_at_first=False, path="march", topo=(P, P)):
    """All variants and coefficient sets of one matrix entry.  Returns the failures, each prefixed with its call; `worst` collects
    the largest error / bound ratio per (family | path, precision, variant).  A Bounded entry also fails if its reference never took
    a wall branch (StageData.wall_failures)."""
    data = stage_data(oracle, Nx, Ny, form, lor, dtype, topo)
    fam, prec = family(Nx, form, dtype, flags, path), ("f64" if np.dtype(dtype) == np.float64 else "f32")
    cid = case_id(Nx, Ny, rows, form, lor, dtype, flags) if path == "march" else tile_case_id(path, Nx, Ny, rows, form, lor, dtype, flags, topo)
    failures = [f"reference: {m}" for m in data.wall_failures]
    for variant, cset in calls():
        fails, ratios = check_case(S, oracle, data, variant, cset, flags, rows, path)
        refused = "refused (SWMHD_ENOTSUP), nothing written" if variant in PATHS[path]["refused"] and not fails else ""
        print(f"  {cid} {variant}/{cset}: {refused}"
              + ", ".join(f"{k} {r:.3g}" for k, r in ratios.items()) + (f"  FAILED: {fails}" if fails else ""))
        if worst is not None and ratios:
            key = f"{fam}/{prec}/{variant}"
            worst[key] = max(worst.get(key, 0.0), max(ratios.values()))
        failures += [f"{variant}/{cset}: {m}" for m in fails]
        if failures and stop_at_first:
            break
    return failures


# ---------------------------------------------------------------------------------------------------------------------------------
# forced layouts: the chooser's read-once knobs, in a child process of their own (test_stage_matrix_gpu.test_forced_layouts)
# ---------------------------------------------------------------------------------------------------------------------------------
FORCED = {
    # 128-lane strips with a one-column tail: 123 = 122 + 1, 489 = 4 x 122 + 1
    "nt128": dict(env={"SWMHD_T_NT": "128"}, shapes=[(123, 31), (489, 31)], lanes=128, LY=6),
    # segments longer than 6 rows on a small grid: 33 rows = 13 + 13 + 7 (an odd count: the folded workgroup's second half of the fp64
    # vector-invariant kernel owns no rows at 2501), default strips
    "ly13": dict(env={"SWMHD_T_LY": "13"}, shapes=[(2501, 33), (600, 33)], lanes=None, LY=13),
}


def forced_main(name, out_path):
    """Child process: all variants for (1, 1) and (0, 2) in fp64 and fp32, without and with WRAP_X | WRAP_Y, under the knob `name`
    (set by the parent in the environment).  Writes {"ok", "failed", "layouts", "worst"} and exits non-zero at the first failure."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import swmhd_amd as S
    from oracle import oracle as O
    cfg = FORCED[name]
    for k, val in cfg["env"].items():
        assert os.environ.get(k) == val, f"{k} must be {val} in the environment of this process"
    worst, layouts, failures = {}, {}, []
    for Nx, Ny in cfg["shapes"]:
        for form, lor in ((1, 1), (0, 2)):
            for dtype in DTYPES:
                for flags in (0, WRAP_X | WRAP_Y):
                    cid = case_id(Nx, Ny, None, form, lor, dtype, flags)
                    layouts[cid] = check_layout(S._lib, Nx, Ny, form, dtype, flags, lanes=cfg["lanes"], LY=cfg["LY"])
                    failures = run_cases(S, O, Nx, Ny, None, form, lor, dtype, flags, worst=worst, stop_at_first=True)
                    if failures:
                        break
                if failures:
                    break
            if failures:
                break
        if failures:
            break
    with open(out_path, "w") as fh:
        json.dump({"ok": not failures, "failed": [f"{cid} {m}" for m in failures], "layouts": layouts, "worst": worst}, fh, indent=1,
                  sort_keys=True)
    return 1 if failures else 0


# ---------------------------------------------------------------------------------------------------------------------------------
# the ensemble matrix: k_tendency_tile<..., ENS = true, PAR = false | true> through swmhd_ensemble_tendencies_rk3[_params]_*, member
# by member against the single-grid reference above (numpy only down to run_ens_stage)
# ---------------------------------------------------------------------------------------------------------------------------------
# Ensemble paths.  par: the *_params entry points (a device table of (g, f, dt) per member); ty: rows of a tile -- that of a single
# model of the member's size; refused: SWMHD_GM_IS_PREV_STATE everywhere, the anchor forms where SWMHD_STRICT refuses them for a single
# grid ("semantics ... as there").  There is no ensemble form of T.
NO_PREV_STATE = ("P2g", "P3n")
ENS_PATHS = {
    "ens4": dict(flags=TILE_KERNEL, strict=False, par=False, ty=4, refused=NO_PREV_STATE),
    "ens8": dict(flags=TILE_KERNEL, strict=False, par=False, ty=8, refused=NO_PREV_STATE),
    "ens-strict": dict(flags=STRICT, strict=True, par=False, ty=8, refused=FAST_ONLY),
    "par4": dict(flags=TILE_KERNEL, strict=False, par=True, ty=4, refused=NO_PREV_STATE),
    "par-strict": dict(flags=STRICT, strict=True, par=True, ty=8, refused=FAST_ONLY),
}
ENS_PAD, ENS_GAP = 5, 37            # columns after every row and elements after every member of a pitched family (ensemble_tracer_cases)
# members per shape: with 64 x 4 | 64 x 8 tiles the launches have 15 | 10, 18 | 12, 9 | 6, 4 | 2 and 72 | 36 workgroups -- none but
# 72 a multiple of 8, below and above 8 on both tile heights (xcd_remap deals ntiles * members blocks over 8 XCDs)
ENS_SHAPES = {(3, 9): 5, (65, 9): 3, (129, 9): 1, (65, 5): 1, (129, 31): 3}
ENS_DENSE_SHAPE = (65, 9)           # also run dense: stride_y = Nx + 2 H, stride_m = (Ny + 2 H) stride_y, with WRAP_X | WRAP_Y
ENS8_MEMBERS = 2
# g and f of member m of a par* path (rounded to the precision of the call by StageData): pairwise distinct, two f negative; dt is the
# member's own StageData.dt
PAR_G = (9.81, 1.0, 4.0, 20.0, 2.5)
PAR_F = (1.0, -0.5, 2.0, 0.25, -1.5)


def ens_calls():
    return [(v, c) for v, c in calls() if v != "T"]


def ens_matrix():
    """Every (path, Nx, Ny, members, form, lor, dtype, flags, dense) of the ensemble matrix, grouped so that consecutive entries share
    their members' StageData."""
    XY = WRAP_X | WRAP_Y
    for (Nx, Ny), members in ENS_SHAPES.items():
        layouts = [(0, False), (XY, False)] + ([(WRAP_X, False), (WRAP_Y, False), (XY, True)] if (Nx, Ny) == ENS_DENSE_SHAPE else [])
        for form, lor in FORMS:
            for dtype in DTYPES:
                for path in ("ens4", "ens-strict", "par4", "par-strict"):
                    for flags, dense in layouts:
                        yield path, Nx, Ny, members, form, lor, dtype, flags, dense
    for form, lor in FORMS:
        for dtype in DTYPES:
            for flags in (0, XY):
                yield ("ens8",) + TILE8_SHAPE + (ENS8_MEMBERS, form, lor, dtype, flags, False)


def ens_case_id(path, Nx, Ny, members, form, lor, dtype, flags, dense):
    return f"{path}-m{members}-{'dense' if dense else 'pitched'}-{case_id(Nx, Ny, None, form, lor, dtype, flags)}"


def ens_workgroups(path, Nx, Ny, members, ty=None):
    """Workgroups of the launch: tile columns x tile rows x members."""
    return tiles(Nx, TILE_X)[0] * tiles(Ny, ty or ENS_PATHS[path]["ty"])[0] * members


def ens_layout(Nx, Ny, dense):
    """(stride_y, stride_m) of a family."""
    sy = Nx + 2 * H + (0 if dense else ENS_PAD)
    return sy, (Ny + 2 * H) * sy + (0 if dense else ENS_GAP)


def ens_view(flat, m, Nx, Ny, dense):
    """Member m's parent inside a flat family buffer (a view)."""
    sy, sm = ens_layout(Nx, Ny, dense)
    return flat[m * sm:m * sm + (Ny + 2 * H) * sy].reshape(Ny + 2 * H, sy)[:, :Nx + 2 * H]


def ens_pack(parents, Nx, Ny, dense, fill):
    """One flat family buffer: member m's parent from parents[m], `fill` in the row padding and the member gaps."""
    flat = np.full(len(parents) * ens_layout(Nx, Ny, dense)[1], fill, dtype=parents[0].dtype)
    for m, a in enumerate(parents):
        ens_view(flat, m, Nx, Ny, dense)[...] = a
    return flat


_REGIONS = {}
INTERIOR, HALO, PADDING, GAP = 0, 1, 2, 3
REGION_NAME = {HALO: "halo", PADDING: "row padding", GAP: "member gap"}


def ens_regions(Nx, Ny, members, dense):
    """What every element of a family buffer is: INTERIOR | HALO | PADDING | GAP."""
    key = (Nx, Ny, members, dense)
    if key not in _REGIONS:
        _REGIONS.clear()
        sy, sm = ens_layout(Nx, Ny, dense)
        reg = np.full(members * sm, GAP, dtype=np.int8)
        for m in range(members):
            reg[m * sm:m * sm + (Ny + 2 * H) * sy] = PADDING
            v = ens_view(reg, m, Nx, Ny, dense)
            v[...] = HALO
            Hh.interior(v, Nx, Ny, H, H)[...] = INTERIOR
        _REGIONS[key] = reg
    return _REGIONS[key]


_ENS_DATA = {}


def ens_members(oracle, Nx, Ny, members, form, lor, dtype, par, row=None):
    """The members of a case: one StageData each, from a seed of its own (no two members share a field, the operand aux included);
    with par, member m carries (PAR_G[m], PAR_F[m]).  row: form every member's reference with that row of the table instead (what a
    kernel that read one row for all members would compute).  Computed once per shape and shared: do not modify."""
    out = []
    for m in range(members):
        r = m if row is None else row
        key = (Nx, Ny, form, lor, np.dtype(dtype).name, m, r if par else None)
        if key not in _ENS_DATA:
            for k in [k for k in _ENS_DATA if k[:2] != (Nx, Ny)]:
                del _ENS_DATA[k]
            kw = dict(grav=PAR_G[r], fcor=PAR_F[r]) if par else {}
            _ENS_DATA[key] = StageData(oracle, Nx, Ny, form, lor, dtype, seed=1000 * Nx + Ny + 7919 * (m + 1), **kw)
            _ENS_DATA[key]._ens_ref = {}
        out.append(_ENS_DATA[key])
    return out


def ens_dts(members, variant, cset, par):
    """dt of every member: its own StageData.dt with a table, member 0's for all where the call has one dt."""
    gam = COEFFS[cset][variant][0]
    return [d.dt(gam) for d in members] if par else [members[0].dt(gam)] * len(members)


def ens_expected(oracle, members, variant, cset, dts, strict):
    """[(reference, bounds | None)] per member: reference_stage + stage_bounds of that member with its dt, or reference_stage_strict
    (whose G is the oracle's with the member's g and f).  Kept per member for the other layouts of the shape (small shapes only)."""
    v, coeffs, out = VARIANTS[variant], COEFFS[cset][variant], []
    for d, dt in zip(members, dts):
        key = (variant, cset, dt, strict)
        if key not in d._ens_ref:
            operand = d.aux if v["operand"] else None
            if strict:
                ref, bounds = reference_stage_strict(d, variant, coeffs, dt), None
            else:
                ref = reference_stage(oracle, d.q, operand, variant, coeffs, d.Nx, d.Ny, d.dx, d.dy, d.form, d.lor, dt, G=d.G)
                bounds = stage_bounds(d, d.q, operand, variant, coeffs, dt, ref)
            if d.Nx * d.Ny > 20000:
                out.append((ref, bounds))
                continue
            d._ens_ref[key] = (ref, bounds)
        out.append(d._ens_ref[key])
    return out


def ens_buffers(members, variant, flags, dense):
    """The host buffers of one call, {"q", "operand", "qnew", "Gn"}: lists of 4 flat family buffers (None: the call has none).  Inputs:
    every member's q with NaN in the halos of every wrapped direction, its own operand aux (sentinel halos), NaN in the row padding
    and the member gaps.  Outputs: the sentinel everywhere.  qnew of P* IS the operand (it holds Uprev), Gn of A2a IS the operand."""
    v, d0 = VARIANTS[variant], members[0]
    Nx, Ny = d0.Nx, d0.Ny
    qs = []
    for d in members:
        q_in = [a.copy() for a in d.q]
        for a in q_in:
            Hh.poison_halo(a, Nx, Ny, H, H, x=bool(flags & WRAP_X), y=bool(flags & WRAP_Y))
        qs.append(q_in)
    sent = np.full_like(d0.q[0], SENTINEL)
    fam = lambda per_member, fill: [ens_pack([p[f] for p in per_member], Nx, Ny, dense, fill) for f in range(4)]
    out = {"q": fam(qs, np.nan), "operand": None, "qnew": None, "Gn": None}
    if v["operand"]:
        out["operand"] = fam([d.aux for d in members], np.nan)
    out["qnew"] = out["operand"] if v["operand"] == "Uprev" else fam([[sent] * 4] * len(members), SENTINEL)
    out["Gn"] = out["operand"] if v["alias"] else fam([[sent] * 4] * len(members), SENTINEL)
    return out


def ens_copy(bufs):
    """A deep copy of ens_buffers' result that keeps its aliases."""
    out = {k: None if bufs[k] is None else [a.copy() for a in bufs[k]] for k in ("q", "operand")}
    for k in ("qnew", "Gn"):
        out[k] = out["operand"] if bufs[k] is bufs["operand"] and bufs[k] is not None else [a.copy() for a in bufs[k]]
    return out


def ens_fabricate(members, variant, dense, before, expected):
    """What a correct kernel leaves behind, built from `expected` (rounded to the precision of the call) on a copy of `before`: for the
    CPU pin of check_ens_outputs, which then spoils it."""
    after, d0 = ens_copy(before), members[0]
    for m, (ref, _) in enumerate(expected):
        for name in ("qnew", "Gn"):
            if ref[name] is None or ref[name] is KEEP:
                continue
            for f in range(4):
                Hh.interior(ens_view(after[name][f], m, d0.Nx, d0.Ny, dense), d0.Nx, d0.Ny, H, H)[...] = ref[name][f].astype(d0.dtype)
    return after


def check_ens_refusal(before, after):
    """A refused call left every buffer bitwise as it was: the failures."""
    fails = []
    for name in ("q", "operand", "qnew", "Gn"):
        for f in range(4 if before[name] is not None else 0):
            if not _same_bits(before[name][f], after[name][f]):
                fails.append(f"refused call changed {name}[{f}]")
    return fails


def check_ens_outputs(members, variant, flags, dense, before, after, expected, singles=None):
    """check_case for every member of an ensemble call: (failures, ratios).  before / after: ens_buffers and what the call made of them;
    expected: ens_expected; singles: per member {"qnew", "Gn"} parents of the same call made on the member alone, to be equal bit for bit.
      1. every written output finite and within its member's bounds (bounds None: bitwise its member's strict reference)
      2. an output with KEEP, every halo, the row padding and the member gaps of every output family, every input and operand: bitwise
         as before
      3. with a WRAP flag the halos of that direction of all four inputs of every member are NaN on entry"""
    v, d0 = VARIANTS[variant], members[0]
    Nx, Ny, M = d0.Nx, d0.Ny, len(members)
    reg = ens_regions(Nx, Ny, M, dense)
    fails, ratios = [], {}
    for f in range(4):
        if not _same_bits(before["q"][f], after["q"][f]):
            fails.append(f"input field {f} was changed")
        if v["operand"] and v["operand"] != "Uprev" and not _same_bits(before["operand"][f], after["operand"][f]):
            fails.append(f"operand {v['operand']} field {f} was changed")
        for m in range(M):
            a = ens_view(before["q"][f], m, Nx, Ny, dense)
            if (flags & WRAP_X and not (np.isnan(a[:, :H]).all() and np.isnan(a[:, H + Nx:]).all())) or \
               (flags & WRAP_Y and not (np.isnan(a[:H]).all() and np.isnan(a[H + Ny:]).all())):
                fails.append(f"member {m} input field {f}: the halos of a wrapped direction are not NaN on entry")
    for name in ("qnew", "Gn"):
        if after[name] is None or (name == "Gn" and v["alias"]):
            continue
        for f in range(4):
            b, a = before[name][f], after[name][f]
            if expected[0][0][name] is KEEP:
                if not _same_bits(a, b):
                    fails.append(f"{name}[{f}] must keep its sentinel: {int((a != b).sum())} cells written")
                continue
            changed = (a.view(np.uint8).reshape(a.size, -1) != b.view(np.uint8).reshape(b.size, -1)).any(axis=1)
            for r, what in REGION_NAME.items():
                n = int((changed & (reg == r)).sum())
                if n:
                    fails.append(f"{name}[{f}]: {n} cells of the {what} written")
            for m, (ref, bounds) in enumerate(expected):
                got_t = Hh.interior(ens_view(a, m, Nx, Ny, dense), Nx, Ny, H, H)
                got = got_t.astype(np.longdouble)
                if not np.isfinite(got).all():
                    fails.append(f"member {m} {name}[{f}]: {int((~np.isfinite(got)).sum())} non-finite cells")
                    ratios[name] = float("inf")
                    continue
                if singles is not None:
                    alone = Hh.interior(singles[m][name][f], Nx, Ny, H, H)
                    if not _same_bits(np.ascontiguousarray(got_t), np.ascontiguousarray(alone)):
                        fails.append(f"member {m} {name}[{f}]: {int((got_t != alone).sum())} cells differ from the single-grid call on the member alone")
                if bounds is None:      # strict: the bits of the oracle's (a -0 for a +0 is a difference)
                    want = np.ascontiguousarray(ref[name][f])
                    u = np.uint64 if want.dtype.itemsize == 8 else np.uint32
                    same = (np.ascontiguousarray(got_t).view(u) == want.view(u)) if want.dtype == got_t.dtype else np.zeros(want.shape, bool)
                    ratios[name] = max(ratios.get(name, 0.0), 0.0 if same.all() else float("inf"))
                    if not same.all():
                        fails.append(f"member {m} {name}[{f}]: {int((~same).sum())} cells differ from the oracle's, max |difference| "
                                     f"{float(np.abs(got - ref[name][f]).max()):.3e}")
                    continue
                err, bound = float(np.abs(got - ref[name][f]).max()), bounds[name][f]
                ratios[name] = max(ratios.get(name, 0.0), err / bound)
                if not err <= bound:
                    fails.append(f"member {m} {name}[{f}]: max error {err:.3e} > bound {bound:.3e}")
    return fails, ratios


def check_ens_layout(L, path, Nx, Ny, members, form, dtype, flags, ty=None, member_map=1):
    """The layout the case is there for, as check_tile_layout: tile columns, tile rows and rows of a tile from the planner's answer
    for a single grid of the member's shape (swmhd_tendency_launch_geometry) -- the ensemble's plan by the header -- and the
    ensemble launch itself from swmhd_ensemble_launch_geometry, which reads the launcher's knobs: the same tiles, the member mapping
    (1: folded into blockIdx.x, 2: blockIdx.y) and the grid.  ty | member_map: what a SWMHD_ENS_RY | SWMHD_ENS_MAP child forces; the
    ensemble query must then report the forced layout, not the default."""
    p = ENS_PATHS[path]
    q = TILE_KERNEL | (STRICT if p["strict"] else 0) | (flags & (WRAP_X | WRAP_Y))
    elem = np.dtype(dtype).itemsize
    geo = L.tendency_launch_geometry(Nx, Ny, form, elem, q)
    ntx, lastx = tiles(Nx, TILE_X)
    assert (geo["kind"], geo["nstrips"]) == (1, ntx), (path, Nx, Ny, geo)
    assert (geo["rows_per_segment"], geo["nseg"]) == (p["ty"], tiles(Ny, p["ty"])[0]), (path, Nx, Ny, geo)
    ty = ty or p["ty"]
    nty, lasty = tiles(Ny, ty)
    ens = L.ensemble_launch_geometry(Nx, Ny, form, members, elem, q)
    grid = (ntx * nty * members, 1) if member_map == 1 else (ntx * nty, members)
    want = dict(kind=1, threads=256, tile_columns=ntx, tile_rows=nty, rows_per_tile=ty, member_map=member_map, grid_x=grid[0], grid_y=grid[1])
    assert ens == want, (path, Nx, Ny, members, ens, want)
    note = f" (forced from {p['ty']})" if ty != p["ty"] else ""
    return (f"kind 1, {ntx} tile columns, last {lastx} wide, {nty} tile rows of {ty}, last {lasty}{note}, "
            f"member in blockIdx.{'xy'[member_map - 1]}, grid {grid[0]} x {grid[1]}")


def run_ens_stage(S, members, variant, cset, flags, dense, path, before, dts, expect_rc=0):
    """One call of swmhd_ensemble_tendencies_rk3[_params]_* on copies of `before` on the device; returns what they hold afterwards
    (ens_buffers' structure).  The return code must be expect_rc."""
    import torch
    L, p, v, d0 = S._lib, ENS_PATHS[path], VARIANTS[variant], members[0]
    Nx, Ny, M = d0.Nx, d0.Ny, len(members)
    sy, sm = ens_layout(Nx, Ny, dense)
    gam, zet = COEFFS[cset][variant]
    sfx = "f64" if d0.dtype == np.float64 else "f32"
    dev = lambda arrs: None if arrs is None else [torch.from_numpy(a).cuda() for a in arrs]
    PA = lambda ts: L.ptr_array([t.data_ptr() for t in ts])
    t = {"q": dev(before["q"]), "operand": dev(before["operand"])}
    for k in ("qnew", "Gn"):
        t[k] = t["operand"] if before[k] is before["operand"] and before[k] is not None else dev(before[k])
    fl = p["flags"] | flags | (GM_IS_PREV_STATE if v["operand"] == "Uprev" else 0) | (RK3_ANCHOR if v["anchor"] else 0)
    gm = PA(t["operand"]) if t["operand"] is not None else None
    head = (PA(t["q"]), PA(t["qnew"]), PA(t["Gn"]), gm, M, sm, Nx, Ny, H, H, sy, d0.dx, d0.dy)
    if p["par"]:
        table = torch.from_numpy(np.array([[d.grav, d.fcor, dt] for d, dt in zip(members, dts)], dtype=d0.dtype)).cuda()
        rc = getattr(L.lib(), f"swmhd_ensemble_tendencies_rk3_params_{sfx}")(*head, table.data_ptr(), d0.form, d0.lor, gam, zet, v["store_G"], fl, None)
    else:
        assert len(set(dts)) == 1 and len({(d.grav, d.fcor) for d in members}) == 1
        rc = getattr(L.lib(), f"swmhd_ensemble_tendencies_rk3_{sfx}")(*head, d0.grav, d0.fcor, d0.form, d0.lor, dts[0], gam, zet, v["store_G"], fl, None)
    if expect_rc == 0:
        L.check(rc, f"{variant}/{cset}")
    assert rc == expect_rc, f"{variant}/{cset}: rc={rc}, expected {expect_rc}"
    torch.cuda.synchronize()
    return {k: None if t[k] is None else [x.cpu().numpy() for x in t[k]] for k in t}


def ens_singles(S, members, variant, cset, flags, dts):
    """The same call through swmhd_tendencies_rk3_* with SWMHD_TILE_KERNEL on every member alone, as a dense copy with the member's
    g, f and dt: [{"qnew", "Gn"}] parents afterwards."""
    out = []
    for d, dt in zip(members, dts):
        r = run_stage(S, d, variant, cset, flags, None, path="tile4", dt=dt)
        out.append({k: r[k][1] for k in ("qnew", "Gn")})
    return out


def check_ens_case(S, oracle, members, variant, cset, flags, dense, path, single=None):
    """One call of an ensemble case: (failures, ratios, observed).  single: "assert" -- every member bitwise the single-grid call on
    the member alone (the header's promise for fast members below ~0.33 Mcell without a table); "observe" -- only report whether that
    holds, as observed["bitwise_single"]."""
    p = ENS_PATHS[path]
    dts = ens_dts(members, variant, cset, p["par"])
    before = ens_buffers(members, variant, flags, dense)
    if variant in p["refused"]:
        try:
            after = run_ens_stage(S, members, variant, cset, flags, dense, path, before, dts, expect_rc=ENOTSUP)
        except AssertionError as e:
            return [str(e)], {}, {}
        return check_ens_refusal(before, after), {}, {}
    expected = ens_expected(oracle, members, variant, cset, dts, p["strict"])
    after = run_ens_stage(S, members, variant, cset, flags, dense, path, before, dts)
    singles = ens_singles(S, members, variant, cset, flags, dts) if single else None
    fails, ratios = check_ens_outputs(members, variant, flags, dense, before, after, expected, singles if single == "assert" else None)
    observed = {}
    if single == "observe":
        lines, _ = check_ens_outputs(members, variant, flags, dense, before, after, expected, singles)
        observed["bitwise_single"] = not any("single-grid call" in m for m in lines)
    return fails, ratios, observed


def run_ens_cases(S, oracle, path, Nx, Ny, members, form, lor, dtype, flags, dense, worst=None, stop_at_first=False, single="default",
                  observed=None):
    """All call forms and coefficient sets of one entry of the ensemble matrix: the failures, each prefixed with its call.  single:
    "default" asserts the bitwise single-grid promise on ens4 and nowhere else; observed: {path/precision: [calls bitwise the
    single-grid call, calls]} filled where single is "observe"."""
    if single == "default":
        single = "assert" if path == "ens4" else None
    data = ens_members(oracle, Nx, Ny, members, form, lor, dtype, ENS_PATHS[path]["par"])
    prec = "f64" if np.dtype(dtype) == np.float64 else "f32"
    cid = ens_case_id(path, Nx, Ny, members, form, lor, dtype, flags, dense)
    failures = []
    for variant, cset in ens_calls():
        fails, ratios, obs = check_ens_case(S, oracle, data, variant, cset, flags, dense, path, single)
        refused = "refused (SWMHD_ENOTSUP), nothing written" if variant in ENS_PATHS[path]["refused"] and not fails else ""
        print(f"  {cid} {variant}/{cset}: {refused}" + ", ".join(f"{k} {r:.3g}" for k, r in ratios.items())
              + (f", bitwise the single-grid call: {obs['bitwise_single']}" if obs else "") + (f"  FAILED: {fails}" if fails else ""))
        if worst is not None and ratios:
            key = f"{path}/{prec}/{variant}"
            worst[key] = max(worst.get(key, 0.0), max(ratios.values()))
        if observed is not None and obs:
            n = observed.setdefault(f"{path}/{prec}", [0, 0])
            n[0] += int(obs["bitwise_single"]); n[1] += 1
        failures += [f"{variant}/{cset}: {m}" for m in fails]
        if failures and stop_at_first:
            break
    return failures


# The ensemble launcher's read-once knobs, each in a child process of its own (test_ensemble_stage_matrix_gpu.test_forced_layouts).
# ty | member_map: the tile height of the fast paths | the member mapping under the knob, which the child reads back from the library
# (swmhd_ensemble_launch_geometry in check_ens_layout): a knob the launcher did not take would fail there.
ENS_FORCED = {
    # the member in blockIdx.y: a 2-D grid of ntiles x members workgroups; the scalar fast and the table strict path between them run
    # the member decoding with and without a table, in the fast and the strict object
    "ens-map2": dict(env={"SWMHD_ENS_MAP": "2"}, paths=("ens4", "par-strict"), ty=None, member_map=2),
    # 64 x 8 fast tiles at small shapes: last tiles of one row (9 rows) and one column (65, 129 columns) of that body; no bitwise
    # promise against the single grid's 64 x 4 tiles
    "ens-ry2": dict(env={"SWMHD_ENS_RY": "2"}, paths=("ens4", "par4"), ty=8, member_map=1),
}
ENS_FORCED_SHAPES = [(65, 9), (129, 31)]
ENS_FORCED_MEMBERS = 3


def ens_forced_cases(name):
    cfg = ENS_FORCED[name]
    return [(path, Nx, Ny, ENS_FORCED_MEMBERS, form, lor, dtype, flags, False) for Nx, Ny in ENS_FORCED_SHAPES for form, lor in ((1, 1), (0, 2))
            for dtype in DTYPES for path in cfg["paths"] for flags in (WRAP_X | WRAP_Y,)]


def ens_forced_main(name, out_path):
    """Child process: ens_forced_cases(name) under the knob `name` (set by the parent in the environment).  Writes {"ok", "failed",
    "layouts", "worst", "observed"} and exits non-zero at the first failure."""
    assert "swmhd_amd" not in sys.modules, "the knobs are read once: the library must not have been used in this process"
    cfg = ENS_FORCED[name]
    for k, val in cfg["env"].items():
        assert os.environ.get(k) == val, f"{k} must be {val} in the environment of this process"
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import swmhd_amd as S
    from oracle import oracle as O
    worst, layouts, failures, observed = {}, {}, [], {}
    for case in ens_forced_cases(name):
        path, Nx, Ny, members, form, lor, dtype, flags, dense = case
        cid = ens_case_id(*case)
        layouts[cid] = check_ens_layout(S._lib, path, Nx, Ny, members, form, dtype, flags, ty=cfg["ty"], member_map=cfg["member_map"])
        single = "default" if cfg["ty"] is None else ("observe" if path == "ens4" else None)
        failures = run_ens_cases(S, O, *case, worst=worst, stop_at_first=True, single=single, observed=observed)
        if failures:
            break
    with open(out_path, "w") as fh:
        json.dump({"ok": not failures, "failed": [f"{cid} {m}" for m in failures], "layouts": layouts, "worst": worst, "observed": observed,
                   "env": cfg["env"]}, fh, indent=1, sort_keys=True)
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit((ens_forced_main if sys.argv[1] in ENS_FORCED else forced_main)(sys.argv[1], sys.argv[2]))
