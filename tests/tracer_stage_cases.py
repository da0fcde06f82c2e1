"""Reference of ONE call of the tracer stage entry points (swmhd_tracers_rk3_* in include/swmhd.h, k_tracers_tile) and the matrix of
calls made through its fast periodic, fast wall and strict wall instantiations (PATHS):
    fast         no flags, periodic: k_tracers_tile<T, FORM, BND = false> of the fast object, every call form of the header
    wall         SWMHD_BOUNDED_* from the topology: the fast BND = true body (wall orders of the reconstructions, reciprocals of the wall
                 face depths in the conservative form)
    wall-strict  SWMHD_STRICT | SWMHD_BOUNDED_*: the strict BND = true body, compared bitwise
(periodic strict stays with tests/test_tracers_gpu.py::test_strict_stage_matrix).  Run by tests/test_tracer_stage_matrix_gpu.py and
tools/stage_matrix_report.py --tracers; pinned on the CPU by tests/test_tracer_stage_cases_cpu.py.

The call forms, coefficient sets, sentinel conventions, wall buffers and the formula of the bounds are those of tests/stage_cases.py
(VARIANTS, COEFFS, KEEP, wall_buffers, stage_bounds), here for K centre fields instead of the four prognostic ones:
    T          cnew == NULL, store_G = 1                          Gn = G
    S1g / S1n  Gm == NULL, store_G 1 / 0                          cnew = c + dt gamma G                       Gn = G iff store_G
    S2g / S3n  with Gm, store_G 1 / 0                             cnew = c + dt (gamma G + zeta Gm)           Gn = G iff store_G
    P2g / P3n  SWMHD_GM_IS_PREV_STATE                             refused everywhere: SWMHD_ENOTSUP, nothing written
    A1         SWMHD_RK3_ANCHOR, Gm == NULL                       cnew = c + dt gamma G                       Gn = W = c + dt zeta G
    A2 / A2a   SWMHD_RK3_ANCHOR with Gm = W                       cnew = W + dt gamma G                       Gn not written
               (A2: Gn is a buffer of its own and store_G = 1; A2a: Gn aliases Gm) -- refused with a Bounded direction or SWMHD_STRICT

Reference: G is tracer_cases.tracer_tendency (the oracle's tendency of A with the tracer in the A slot and no forcing) with the
topology of the case.  Fast paths: G in float64 on inputs widened exactly, the update in np.longdouble from the header's formulas.
wall-strict: G and tracer_cases.substep in the precision of the call, compared bitwise.  Bounded directions: the halos of q1, q2, h
and every c hold the boundary conditions (tracer_cases.fill_state; the gradient condition tracer_cases.grad_A on tracer 0 where y is
Bounded, no flux on the others); periodic directions run once with the WRAP flag and NaN in those halos and once with filled halos.

Bounds of the fast paths (include/swmhd.h and stage_cases, none fitted to what the kernel gives):
    tendencies  max|dG| <= tol max(max|G|, S), tol = 1e-12 (fp64, rough fields) / 1e-4 (fp32), S = helpers.term_scales(...)[3] with c in the
                A slot
    cnew, W     dt weight (tendency bound) + 4 eps max|addends and result|, per tracer: weight = |gamma| (S1g, S1n, A1, A2, A2a),
                |gamma| + |zeta| (S2g, S3n), |zeta| (W)
The reference part is numpy and the CPU oracle only; run_call needs a GPU."""
import ctypes

import numpy as np

import helpers as Hh
import stage_cases as SC
import tracer_cases as TC

H = TC.H
P, B = TC.P, TC.B
TX, TY = TC.TX, TC.TY
PAD = 5                             # stride_y = Nx + 2 H + PAD
KMAX = 8                            # SWMHD_MAX_TRACERS
K_DEFAULT = 3
SENTINEL, KEEP = SC.SENTINEL, SC.KEEP
DTYPES = SC.DTYPES
FORMULATIONS = (1, 0)
NO_PREV_STATE = ("P2g", "P3n")
PATHS = {
    "fast": dict(flags=0, strict=False, wall=False, refused=NO_PREV_STATE),
    "wall": dict(flags=0, strict=False, wall=True, refused=SC.FAST_ONLY),
    "wall-strict": dict(flags=SC.STRICT, strict=True, wall=True, refused=SC.FAST_ONLY),
}
# the wall shapes, built from the tracer tile as stage_cases.WALL_SHAPES is from the 64 x 8 tile: a tile edge 1 and 3 cells inside the
# east / north wall buffer, exactly at the wall, a grid narrower than two buffers, several tiles a side
WALL_SHAPES = [(TX + 1, TY + 1), (TX + 3, TY + 3), (TX, TY), (7, 8), (2 * TX + 1, 2 * TY - 1)]
WALL_TOPOS = SC.WALL_TOPOS
# (tile columns, columns of the last one, tile rows, rows of the last one) each shape exists for, over all rows
TILES = {
    (3, 3): (1, 3, 1, 3), (7, 9): (1, 7, 1, 9), (63, 15): (1, 63, 1, 15), (64, 16): (1, 64, 1, 16), (65, 17): (2, 1, 2, 1),
    (129, 9): (3, 1, 1, 9), (3, 17): (1, 3, 2, 1), (129, 16): (3, 1, 1, 16), (64, 3): (1, 64, 1, 3), (7, 15): (1, 7, 1, 15),
    (67, 19): (2, 3, 2, 3), (7, 8): (1, 7, 1, 8), (129, 31): (3, 1, 2, 15),
}
# Ny: (tile rows, rows of the last one) of rows [2, Ny - 3), which start off a tile multiple (and inside the south wall buffer)
PARTIAL_TILE_ROWS = {8: (1, 3), 9: (1, 4), 15: (1, 10), 16: (1, 11), 17: (1, 12), 19: (1, 14), 31: (2, 10)}


def calls():
    """Every (variant, coefficient set, K) of a case: stage_cases.calls() with K = 3 tracers, and S2g again with K = 1 and K = 8."""
    out = [(v, c, K_DEFAULT) for v, c in SC.calls()]
    return out + [("S2g", c, K) for c in SC.COEFFS for K in (1, KMAX)]


def row_ranges(Ny):
    """All rows, and [2, Ny - 3) where that is not empty."""
    return [None] + ([(2, Ny - 3)] if Ny - 3 > 2 else [])


def wrap_flags(topo, wrap):
    """The WRAP flag of every periodic direction (wrap), or none."""
    if not wrap:
        return 0
    return (SC.WRAP_X if topo[0] == P else 0) | (SC.WRAP_Y if topo[1] == P else 0)


def matrix():
    """Every (path, Nx, Ny, topology, formulation, dtype, wrap) of the matrix, grouped so that consecutive entries share their
    TracerStageData.  A (B, B) grid has no direction to wrap and runs with filled halos only."""
    for Nx, Ny in TC.STAGE_SHAPES:
        for form in FORMULATIONS:
            for dtype in DTYPES:
                for wrap in (True, False):
                    yield "fast", Nx, Ny, (P, P), form, dtype, wrap
    for Nx, Ny in WALL_SHAPES:
        for topo in WALL_TOPOS:
            for form in FORMULATIONS:
                for dtype in DTYPES:
                    for path in ("wall", "wall-strict"):
                        for wrap in ((True, False) if P in topo else (False,)):
                            yield path, Nx, Ny, topo, form, dtype, wrap


def case_id(path, Nx, Ny, topo, form, dtype, wrap):
    t = "" if tuple(topo) == (P, P) else "-" + "".join("PB"[d] for d in topo)
    return (f"{path}{t}-{Nx}x{Ny}-{'vi' if form == 1 else 'cons'}-{'f64' if np.dtype(dtype) == np.float64 else 'f32'}-"
            f"{'wrap' if wrap else 'filled'}")


def tracer_tiles(Nx, nrows):
    """(tile columns, columns of the last one, tile rows, rows of the last one): launch_plan.hpp tracer_tiles, restated from TX, TY."""
    return SC.tiles(Nx, TX) + SC.tiles(nrows, TY)


def check_layout(Nx, Ny, rows=None):
    """Assert that Nx x Ny (rows: a row range) has the tiles it exists for; returns a one-line description."""
    if rows is None:
        got = tracer_tiles(Nx, Ny)
        assert got == TILES[Nx, Ny], (Nx, Ny, got)
    else:
        assert rows == (2, Ny - 3) and rows[0] % TY, rows
        got = tracer_tiles(Nx, rows[1] - rows[0])
        assert got == TILES[Nx, Ny][:2] + PARTIAL_TILE_ROWS[Ny], (Nx, Ny, rows, got)
    return f"{got[0]} tile columns of {TX}, last {got[1]} wide, {got[2]} tile rows of {TY}, last {got[3]}"


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs and the oracle's tendencies, once per (shape, formulation, precision, topology)
# ---------------------------------------------------------------------------------------------------------------------------------
class TracerStageData:
    """(q1, q2, h), KMAX distinct tracers and KMAX distinct operands (Gm | W: random interiors, the sentinel in the halos, as
    test_tracers_gpu.StageInputs.Gm) of one case, halos filled for its topology, and the oracle's float64 tendency of every tracer.
    wall_failures: stage_cases.wall_buffer_failures restated for one centre field, per tracer (Bounded cases)."""

    def __init__(self, oracle, Nx, Ny, form, dtype, topo=(P, P), seed=None):
        self.Nx, self.Ny, self.form, self.dtype, self.topo = Nx, Ny, form, np.dtype(dtype), tuple(topo)
        seed = 1000 * Nx + Ny if seed is None else seed
        t = self.dtype.type
        self.dx, self.dy = float(t(TC.DX)), float(t(TC.DY))      # as the call receives them
        q = TC.state(Nx, Ny, form, seed, t)
        c = TC.tracer_fields(Nx, Ny, KMAX, seed, t)
        if self.topo == (P, P):
            q = [Hh.fill_halo_periodic(a, Nx, Ny, H, H) for a in q]
            c = [Hh.fill_halo_periodic(a, Nx, Ny, H, H) for a in c]
        else:
            gA = TC.grad_A(self.topo)
            TC.fill_state(oracle, q, Nx, Ny, self.topo, gA, self.dx, self.dy)
            for k, a in enumerate(c):
                TC.fill(oracle, a, Nx, Ny, self.topo, grad=gA if k == 0 else None, dx=self.dx, dy=self.dy)
        self.q, self.c = [np.ascontiguousarray(a) for a in q[:3]], [np.ascontiguousarray(a) for a in c]
        self.Gm = []
        for k in range(KMAX):
            a = np.full(self.q[0].shape, SENTINEL, dtype=t)
            Hh.interior(a, Nx, Ny, H, H)[...] = np.random.default_rng([seed, 200 + k]).standard_normal((Ny, Nx))
            self.Gm.append(a)
        self._oracle, self._G_strict, self._ref = oracle, None, {}
        q64, c64 = [a.astype(np.float64) for a in self.q], [a.astype(np.float64) for a in self.c]      # exact widening
        tend = lambda qq, cc, tp: Hh.interior(TC.tracer_tendency(oracle, qq, cc, Nx, Ny, self.dx, self.dy, form, tp, SC.NTHREADS),
                                              Nx, Ny, H, H).copy()
        self.G = [tend(q64, a, self.topo) for a in c64]
        self.scales = [float(Hh.term_scales(TC.FORM_NAME[form], q64 + [a], self.dx, self.dy, 0.0)[3]) for a in c64]
        self.Gmax = [float(np.abs(g).max()) for g in self.G]
        self.cmax = [float(np.abs(Hh.interior(a, Nx, Ny, H, H)).max()) for a in c64]
        self.G_periodic, self.wall_failures = None, []
        if self.topo != (P, P):
            qp = [oracle.fill_halo_periodic(a.copy(), Nx, Ny, H, H) for a in q64]
            self.G_periodic = [tend(qp, oracle.fill_halo_periodic(a.copy(), Nx, Ny, H, H), (P, P)) for a in c64]
            self.wall_failures = wall_buffer_failures(self.G, self.G_periodic, Nx, Ny, self.topo)

    def G_strict(self):
        """The oracle's tendencies in the precision of the call (parents): what a strict call must give bit for bit."""
        if self._G_strict is None:
            self._G_strict = [TC.tracer_tendency(self._oracle, self.q, a, self.Nx, self.Ny, self.dx, self.dy, self.form, self.topo,
                                                 SC.NTHREADS) for a in self.c]
        return self._G_strict

    def dt(self, gamma):
        """stage_cases.StageData.dt over the tracers: dt |gamma| max|G| = max|c|, rounded to the precision of the call."""
        if gamma == 0.0:
            return 0.0
        return float(self.dtype.type(max(self.cmax) / (abs(gamma) * max(self.Gmax))))


def wall_buffer_failures(G, G_periodic, Nx, Ny, topo):
    """stage_cases.wall_buffer_failures for centre fields: per tracer, the Bounded tendency must differ from the periodic one of the
    same interior inside the buffer of every wall and equal it bit for bit outside all of them.  One line per violation."""
    buffers = SC.wall_buffers(Nx, Ny, topo)
    near = np.zeros((Ny, Nx), dtype=bool)
    for mask in buffers.values():
        near |= mask
    fails = []
    for k, (gb, gp) in enumerate(zip(G, G_periodic)):
        differs = gb != gp
        for side, mask in buffers.items():
            if not (differs & mask).any():
                fails.append(f"tracer {k}: the Bounded reference equals the periodic one in the whole {side} wall buffer")
        if (differs & ~near).any():
            fails.append(f"tracer {k}: the Bounded reference differs from the periodic one in {int((differs & ~near).sum())} cells "
                         "outside the wall buffers")
    return fails


_DATA = {}


def stage_data(oracle, Nx, Ny, form, dtype, topo=(P, P)):
    """TracerStageData of a case, computed once; only the latest shape is kept.  Shared: do not modify."""
    key = (Nx, Ny, form, np.dtype(dtype).name, tuple(topo))
    if key not in _DATA:
        for k in [k for k in _DATA if k[:2] != (Nx, Ny)]:
            del _DATA[k]
        _DATA[key] = TracerStageData(oracle, Nx, Ny, form, dtype, topo)
    return _DATA[key]


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference of one call and its bounds
# ---------------------------------------------------------------------------------------------------------------------------------
def _rows(data, rows):
    return (0, data.Ny) if rows is None else rows


def _cut(data, a, rows):
    j0, j1 = _rows(data, rows)
    return Hh.interior(a, data.Nx, data.Ny, H, H)[j0:j1]


def reference_call(data, variant, coeffs, dt, K, rows=None, G=None):
    """Expected interior rows of every output of one fast call: {"cnew": K arrays | None (the call has none), "Gn": K arrays | KEEP}.
    coeffs: (gamma, zeta) as passed; G: interior tendencies to use instead of the oracle's float64 ones (widened exactly)."""
    v = SC.VARIANTS[variant]
    j0, j1 = _rows(data, rows)
    G = [np.asarray((data.G if G is None else G)[k][j0:j1], dtype=np.float64) for k in range(K)]
    if not v["fused"]:
        return {"cnew": None, "Gn": G}
    LD = np.longdouble
    gam, zet, dtl = (LD(data.dtype.type(x)) for x in (coeffs[0], coeffs[1], dt))      # the values the kernel receives
    C = [_cut(data, data.c[k], rows).astype(LD) for k in range(K)]
    Gl = [g.astype(LD) for g in G]
    Op = [_cut(data, data.Gm[k], rows).astype(LD) for k in range(K)] if v["operand"] else None
    if v["anchor"] and Op is None:
        return {"cnew": [c + dtl * gam * g for c, g in zip(C, Gl)], "Gn": [c + dtl * zet * g for c, g in zip(C, Gl)]}
    if v["anchor"]:
        return {"cnew": [w + dtl * gam * g for w, g in zip(Op, Gl)], "Gn": KEEP}
    if Op is None:
        cnew = [c + dtl * gam * g for c, g in zip(C, Gl)]
    else:
        assert v["operand"] == "Gm", variant
        cnew = [c + dtl * (gam * g + zet * m) for c, g, m in zip(C, Gl, Op)]
    return {"cnew": cnew, "Gn": G if v["store_G"] else KEEP}


def reference_call_strict(data, variant, coeffs, dt, K, rows=None):
    """reference_call of a strict call, to be compared bitwise: the oracle's tendency and tracer_cases.substep in the precision of
    the call.  The call forms of the strict paths only."""
    v = SC.VARIANTS[variant]
    assert not v["anchor"] and v["operand"] in (None, "Gm"), variant
    G = data.G_strict()[:K]
    if not v["fused"]:
        return {"cnew": None, "Gn": [_cut(data, g, rows) for g in G]}
    cnew = [_cut(data, TC.substep(data.c[k], G[k], data.Gm[k] if v["operand"] else None, data.Nx, data.Ny, dt, coeffs[0], coeffs[1],
                                  v["operand"] is None), rows) for k in range(K)]
    return {"cnew": cnew, "Gn": [_cut(data, g, rows) for g in G] if v["store_G"] else KEEP}


def call_bounds(data, variant, coeffs, dt, K, ref, rows=None):
    """Allowed max-norm error of each written output, per tracer: {"cnew": [K] | None, "Gn": [K] | None} -- the expression of
    stage_cases.stage_bounds with the tracer in the place of the field (pinned against it by the CPU tests)."""
    v = SC.VARIANTS[variant]
    eps = float(np.finfo(data.dtype).eps)
    gam, zet = (abs(float(data.dtype.type(x))) for x in coeffs)
    tb = [SC.TOL[data.dtype] * max(data.Gmax[k], data.scales[k]) for k in range(K)]
    if not v["fused"]:
        return {"cnew": None, "Gn": tb}
    amax = lambda a: float(np.abs(a).max())
    cut = lambda a: _cut(data, a, rows).astype(np.float64)
    out = {"cnew": [], "Gn": None}
    for k in range(K):
        terms = [amax(ref["cnew"][k]), dt * gam * data.Gmax[k], amax(cut(data.Gm[k] if v["operand"] == "W" else data.c[k]))]
        weight = gam
        if v["operand"] == "Gm":
            terms.append(dt * zet * amax(cut(data.Gm[k])))
            weight = gam + zet
        out["cnew"].append(dt * weight * tb[k] + 4 * eps * max(terms))
    if v["anchor"] and v["operand"] is None:      # W through the G pointers
        out["Gn"] = [dt * zet * tb[k] + 4 * eps * max(amax(cut(data.c[k])), dt * zet * data.Gmax[k], amax(ref["Gn"][k])) for k in range(K)]
    elif ref["Gn"] is not KEEP:
        out["Gn"] = tb
    return out


def expected_call(data, path, variant, cset, K, rows=None):
    """(reference, bounds | None (strict: bitwise)) of one call that the path does not refuse, kept for the other halo mode of the case."""
    key = (path, variant, cset, K, rows)
    if key not in data._ref:
        coeffs = SC.COEFFS[cset][variant]
        dt = data.dt(coeffs[0])
        if PATHS[path]["strict"]:
            data._ref[key] = (reference_call_strict(data, variant, coeffs, dt, K, rows), None)
        else:
            ref = reference_call(data, variant, coeffs, dt, K, rows)
            data._ref[key] = (ref, call_bounds(data, variant, coeffs, dt, K, ref, rows))
    return data._ref[key]


# ---------------------------------------------------------------------------------------------------------------------------------
# the buffers of one call, and their comparison (numpy only)
# ---------------------------------------------------------------------------------------------------------------------------------
def pitched(a, pad):
    """Parent a with PAD more columns that hold `pad`."""
    out = np.full((a.shape[0], a.shape[1] + PAD), pad, dtype=a.dtype)
    out[:, :a.shape[1]] = a
    return out


def call_buffers(data, variant, K, wrap):
    """The pitched host buffers of one call: {"q": [3], "c": [K], "Gm": [K] | None, "cnew": [K] | None, "Gn": [K]}.  Inputs: NaN in the
    pad columns and, with wrap, in the halos of every periodic direction of q1, q2, h and c; the operand's halos hold the sentinel.
    Outputs: the sentinel everywhere.  Gn of A2a IS Gm."""
    v = SC.VARIANTS[variant]
    wx, wy = bool(wrap) and data.topo[0] == P, bool(wrap) and data.topo[1] == P
    poison = lambda a: Hh.poison_halo(a.copy(), data.Nx, data.Ny, H, H, x=wx, y=wy) if (wx or wy) else a
    sent = lambda: [pitched(np.full_like(data.q[0], SENTINEL), SENTINEL) for _ in range(K)]
    out = {"q": [pitched(poison(a), np.nan) for a in data.q], "c": [pitched(poison(a), np.nan) for a in data.c[:K]],
           "Gm": [pitched(a, np.nan) for a in data.Gm[:K]] if v["operand"] else None, "cnew": sent() if v["fused"] else None}
    out["Gn"] = out["Gm"] if v["alias"] else sent()
    return out


def copy_buffers(bufs):
    """A deep copy of call_buffers' result that keeps its alias."""
    out = {k: None if bufs[k] is None else [a.copy() for a in bufs[k]] for k in ("q", "c", "Gm", "cnew")}
    out["Gn"] = out["Gm"] if bufs["Gn"] is bufs["Gm"] else [a.copy() for a in bufs["Gn"]]
    return out


def fabricate(data, K, rows, before, ref):
    """What a correct kernel leaves behind, built from the reference (rounded to the precision of the call) on a copy of `before`:
    for the CPU pin of check_outputs, which then spoils it."""
    after = copy_buffers(before)
    j0, j1 = _rows(data, rows)
    for name in ("cnew", "Gn"):
        if ref[name] is None or ref[name] is KEEP:
            continue
        for k in range(K):
            after[name][k][H + j0:H + j1, H:H + data.Nx] = np.asarray(ref[name][k]).astype(data.dtype)
    return after


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def check_refusal(before, after):
    """A refused call left every buffer it was given bitwise as it was: the failures."""
    fails = []
    for name in ("q", "c", "Gm", "cnew", "Gn"):
        for k in range(len(before[name]) if before[name] is not None else 0):
            if not _same_bits(before[name][k], after[name][k]):
                fails.append(f"refused call changed {name}[{k}]")
    return fails


def check_outputs(data, variant, K, rows, wrap, before, after, ref, bounds):
    """One call against its reference: (failures, ratios).  before / after: call_buffers and what the call made of them.
      1. every written output finite and within its tracer's bound over the rows of the call, max-norm (bounds None: bitwise the strict
         reference); ratios: {"cnew" | "Gn": largest error / bound over the tracers} (strict: 0 or inf)
      2. an output with KEEP, every halo, every pad column and every row outside the range of every output, every input and the
         operand: bitwise as before
      3. with wrap, the halos of every periodic direction of q1, q2, h and every c are NaN on entry"""
    v = SC.VARIANTS[variant]
    Nx, Ny = data.Nx, data.Ny
    j0, j1 = _rows(data, rows)
    fails, ratios = [], {}
    for name in ("q", "c") + (("Gm",) if v["operand"] else ()):
        for k, (b, a) in enumerate(zip(before[name], after[name])):
            if not _same_bits(a, b):
                fails.append(f"{'operand ' + v['operand'] if name == 'Gm' else 'input ' + name}[{k}] was changed")
    if wrap:
        for name in ("q", "c"):
            for k, b in enumerate(before[name]):
                p = b[:, :Nx + 2 * H]
                if (data.topo[0] == P and not (np.isnan(p[:, :H]).all() and np.isnan(p[:, H + Nx:]).all())) or \
                   (data.topo[1] == P and not (np.isnan(p[:H]).all() and np.isnan(p[H + Ny:]).all())):
                    fails.append(f"input {name}[{k}]: the halos of a wrapped direction are not NaN on entry")
    region = np.full(before["q"][0].shape, 1, dtype=np.int8)         # 0 rows of the call, 1 halo, 2 pad column, 3 interior row outside
    region[H:H + Ny, H:H + Nx] = 3
    region[H + j0:H + j1, H:H + Nx] = 0
    region[:, Nx + 2 * H:] = 2
    where = {1: "halo", 2: "pad columns", 3: f"interior outside rows [{j0}, {j1})"}
    for name in ("cnew", "Gn"):
        if after[name] is None or (name == "Gn" and v["alias"]):
            continue
        for k in range(K):
            b, a = before[name][k], after[name][k]
            if ref[name] is KEEP:
                if not _same_bits(a, b):
                    fails.append(f"{name}[{k}] must keep its sentinel: {int((_bits(a) != _bits(b)).sum())} cells written")
                continue
            changed = _bits(a) != _bits(b)
            for r, what in where.items():
                n = int((changed & (region == r)).sum())
                if n:
                    fails.append(f"{name}[{k}]: {n} cells of the {what} written")
            got_t = a[H + j0:H + j1, H:H + Nx]
            got = got_t.astype(np.longdouble)
            if not np.isfinite(got).all():
                fails.append(f"{name}[{k}]: {int((~np.isfinite(got)).sum())} non-finite cells")
                ratios[name] = float("inf")
                continue
            if bounds is None:      # strict: the bits of the oracle's
                want = np.ascontiguousarray(ref[name][k])
                same = (_bits(got_t) == _bits(want)) if want.dtype == got_t.dtype else np.zeros(want.shape, bool)
                ratios[name] = max(ratios.get(name, 0.0), 0.0 if same.all() else float("inf"))
                if not same.all():
                    fails.append(f"{name}[{k}]: {int((~same).sum())} cells differ from the oracle's, max |difference| "
                                 f"{float(np.abs(got - want).max()):.3e}")
                continue
            err, bound = float(np.abs(got - ref[name][k]).max()), bounds[name][k]
            ratios[name] = max(ratios.get(name, 0.0), err / bound)
            if not err <= bound:
                fails.append(f"{name}[{k}]: max error {err:.3e} > bound {bound:.3e}")
    return fails, ratios


# ---------------------------------------------------------------------------------------------------------------------------------
# one call on the GPU
# ---------------------------------------------------------------------------------------------------------------------------------
def run_call(S, data, path, variant, cset, K, rows, wrap, before, expect_rc=0):
    """One call of swmhd_tracers_rk3_* on device copies of `before` with the flags of `path`, the Bounded flags of data.topo, the WRAP
    flags of `wrap` and those of the call form; returns what the buffers hold afterwards (call_buffers' structure).  The return code
    must be expect_rc."""
    import torch
    L, v = S._lib, SC.VARIANTS[variant]
    assert PATHS[path]["wall"] == (data.topo != (P, P)), (path, data.topo)
    j0, j1 = _rows(data, rows)
    gam, zet = SC.COEFFS[cset][variant]
    dt = data.dt(gam)
    dev = lambda arrs: None if arrs is None else [torch.from_numpy(a).cuda() for a in arrs]
    t = {k: dev(before[k]) for k in ("q", "c", "Gm", "cnew")}
    t["Gn"] = t["Gm"] if before["Gn"] is before["Gm"] else dev(before["Gn"])
    PA = lambda ts: None if ts is None else (ctypes.c_void_p * len(ts))(*[x.data_ptr() for x in ts])
    fl = (PATHS[path]["flags"] | SC.topo_flags(data.topo) | wrap_flags(data.topo, wrap)
          | (SC.GM_IS_PREV_STATE if v["operand"] == "Uprev" else 0) | (SC.RK3_ANCHOR if v["anchor"] else 0))
    sfx = "f64" if data.dtype == np.float64 else "f32"
    rc = getattr(L.lib(), f"swmhd_tracers_rk3_{sfx}")(t["q"][0].data_ptr(), t["q"][1].data_ptr(), t["q"][2].data_ptr(), PA(t["c"]), PA(t["cnew"]),
                                                       PA(t["Gn"]), PA(t["Gm"]), K, data.Nx, data.Ny, H, H, data.Nx + 2 * H + PAD, data.dx, data.dy,
                                                       data.form, dt, gam, zet, v["store_G"], j0, j1, fl, None)
    if expect_rc == 0:
        L.check(rc, f"{variant}/{cset}")
    assert rc == expect_rc, f"{variant}/{cset}: rc={rc}, expected {expect_rc}"
    torch.cuda.synchronize()
    return {k: None if t[k] is None else [x.cpu().numpy() for x in t[k]] for k in t}


def check_call(S, data, path, variant, cset, K, rows, wrap):
    """run_call against its reference: (failures, ratios); a form the path refuses: SWMHD_ENOTSUP and nothing written."""
    before = call_buffers(data, variant, K, wrap)
    if variant in PATHS[path]["refused"]:
        try:
            after = run_call(S, data, path, variant, cset, K, rows, wrap, before, expect_rc=SC.ENOTSUP)
        except AssertionError as e:
            return [str(e)], {}
        return check_refusal(before, after), {}
    ref, bounds = expected_call(data, path, variant, cset, K, rows)
    after = run_call(S, data, path, variant, cset, K, rows, wrap, before)
    return check_outputs(data, variant, K, rows, wrap, before, after, ref, bounds)


def run_cases(S, oracle, path, Nx, Ny, topo, form, dtype, wrap, worst=None):
    """All calls of one matrix entry over all its row ranges.  Returns the failures, each prefixed with its call; `worst` collects the
    largest error / bound ratio and the call it occurred in per (path, precision, variant).  A Bounded entry also fails if its
    reference never took a wall branch (TracerStageData.wall_failures)."""
    data = stage_data(oracle, Nx, Ny, form, dtype, topo)
    prec = "f64" if np.dtype(dtype) == np.float64 else "f32"
    cid = case_id(path, Nx, Ny, topo, form, dtype, wrap)
    failures = [f"reference: {m}" for m in data.wall_failures]
    for rows in row_ranges(Ny):
        print(f"  {cid} rows {rows or 'all'}: {check_layout(Nx, Ny, rows)}")
        for variant, cset, K in calls():
            fails, ratios = check_call(S, data, path, variant, cset, K, rows, wrap)
            call = f"{variant}/{cset}/K{K}/rows {'all' if rows is None else f'{rows[0]}..{rows[1]}'}"
            refused = "refused (SWMHD_ENOTSUP), nothing written" if variant in PATHS[path]["refused"] and not fails else ""
            print(f"  {cid} {call}: {refused}" + ", ".join(f"{k} {r:.3g}" for k, r in ratios.items()) + (f"  FAILED: {fails}" if fails else ""))
            if worst is not None and ratios:
                key = f"{path}/{prec}/{variant}"
                if max(ratios.values()) >= worst.get(key, (-1.0, ""))[0]:
                    worst[key] = (max(ratios.values()), f"{cid} {call}")
            failures += [f"{call}: {m}" for m in fails]
    return failures
