"""The call matrix of the Lorentz operator kernels (swmhd_lorentz_*_rows_* in include/swmhd.h: k_lorentz_jacobian, k_lorentz_divergence
and the two marching kernels of lorentz_march_kernels.inc) and its reference.  numpy + the CPU oracle only.

The reference is the oracle's own operator (oracle.lorentz_jacobian / lorentz_divergence: the reference's functions restated) on the
inputs of the call; tests/test_operator_cases_cpu.py pins what the GPU matrix (tests/test_operator_matrix_gpu.py) relies on: the stencil
reach the header states, and that on every input of the matrix the oracle's own fp32 arithmetic stays far inside the fast tolerance.

A path is a compiled kernel family, chosen by flags and topology; one workgroup of it writes W columns x R rows:
    march        SWMHD_MARCH_KERNEL   both forms, periodic    252 x 8 | 250 x 8   (OP_MARCH_NT - 2 XH lanes, segments of OP_MARCH_LY_MIN rows)
    tile         SWMHD_TILE_KERNEL    both forms              64 x 16 | 64 x 8    (TILE_X x OP_JAC_TILE_Y | OP_DIV_TILE_Y)
    strict       SWMHD_STRICT         both forms              the same tiles
    wall         as tile,   topology (B, B), (B, P), (P, B)   divergence form, 64 x 8
    wall-strict  as strict, the same topologies
(the constants are launch_plan.hpp's; tests/launch_plan_check.cpp asserts what every shape of the matrix lands on)."""
import numpy as np

import helpers as Hh

# ---- constants of swmhd_amd/csrc/launch_plan.hpp, named once -----------------------------------------------------------------------------
OP_MARCH_NT, OP_MARCH_LY_MIN = 256, 8
TILE_X, OP_JAC_TILE_Y, OP_DIV_TILE_Y = 64, 16, 8
REACH = {"jacobian": (2, 1), "divergence": (3, 3)}      # stencil reach of (A, h), include/swmhd.h; the first is XH of the marching kernel
RING_PERIOD = 12                                         # LDS row rings of the marching kernels: jo & 3, jo & 1, jo % 3
# ---- flags and codes of include/swmhd.h -----------------------------------------------------------------------------------------------
STRICT, TILE_KERNEL, MARCH_KERNEL = 1, 2, 4
P, B = 0, 1
TOPO_NAME = {P: "P", B: "B"}

FORMS = ("jacobian", "divergence")
DTYPES = (np.float64, np.float32)
SFX = {np.float64: "f64", np.float32: "f32"}
TOL = {np.float64: 1e-13, np.float32: 2e-5}             # the header's fast tolerance: 450 eps64, 168 eps32
SENTINEL = -777.25
DX, DY = 0.37, 0.41
WALLS = [(B, B), (B, P), (P, B)]
PATHS = {
    "march": dict(flags=MARCH_KERNEL, strict=False, forms=FORMS, topos=[(P, P)]),
    "tile": dict(flags=TILE_KERNEL, strict=False, forms=FORMS, topos=[(P, P)]),
    "strict": dict(flags=STRICT, strict=True, forms=FORMS, topos=[(P, P)]),
    "wall": dict(flags=TILE_KERNEL, strict=False, forms=("divergence",), topos=WALLS),
    "wall-strict": dict(flags=STRICT, strict=True, forms=("divergence",), topos=WALLS),
}
LAYOUTS = ("minimal", "deep")
# a quarter of the fast budget of fp32, in eps32: what the oracle's own fp32 arithmetic may use of it on an input of the matrix
CONDITIONING_CAP_EPS32 = 42


def workgroup(path, form):
    """(W, R): output columns x rows of one workgroup of the path."""
    if path == "march":
        return OP_MARCH_NT - 2 * REACH[form][0], OP_MARCH_LY_MIN
    return TILE_X, OP_JAC_TILE_Y if form == "jacobian" else OP_DIV_TILE_Y


def shapes(path, form):
    W, R = workgroup(path, form)
    tiny = [(4, 3), (7, 9)] if path.startswith("wall") else [(1, 1), (2, 3), (5, 4)]
    extra = [] if path == "march" else [(129, 9)]
    return tiny + [(W - 1, R - 1), (W, R), (W + 1, R + 1), (2 * W + 1, 2 * R + 1)] + extra


def row_ranges(Ny):
    return [(0, Ny), (1, max(Ny - 1, 1)), (min(2, Ny), min(2, Ny))]      # all rows, the inner rows, an empty range


def sweep_shape(form):
    """The grid of the phase sweep of the marching kernels: two strips, the second one column wide; 21 rows."""
    return workgroup("march", form)[0] + 1, 21


def sweep_ranges():
    """[j0, j0 + 9) for every J0 mod 12: a full segment of 8 rows and a segment of one row, which starts at J0 + 8."""
    return [(j0, j0 + OP_MARCH_LY_MIN + 1) for j0 in range(RING_PERIOD)]


def layout(name, form, Nx):
    """(Hx, Hy, stride_y)"""
    if name == "minimal":
        r = REACH[form][0]
        return r, r, Nx + 2 * r
    return 5, 4, (Nx + 2 * 5 + 5) | 1


def seed(Nx, Ny):
    return 1000 * Nx + Ny


def spacing(dtype):
    """(dx, dy) as the call receives them, as Python floats: rounded to the precision of the call."""
    return float(dtype(DX)), float(dtype(DY))


def ring(Nx, Ny, Hx, Hy):
    """Ring number of every cell of a compact parent: 0 in the interior, k for a halo cell k cells outside it (the larger of x and y)."""
    x = np.arange(-Hx, Nx + Hx)
    y = np.arange(-Hy, Ny + Hy)
    ox = np.maximum(np.maximum(-x, x - (Nx - 1)), 0)
    oy = np.maximum(np.maximum(-y, y - (Ny - 1)), 0)
    return np.maximum(oy[:, None], ox[None, :])


def poisoned(A, h, Nx, Ny, Hx, Hy, form, closer=(0, 0)):
    """Copies of compact parents with NaN in every halo cell beyond the reach of the form (closer: that many rings earlier for A, h)."""
    k = ring(Nx, Ny, Hx, Hy)
    A, h = A.copy(), h.copy()
    A[k > REACH[form][0] - closer[0]] = np.nan
    h[k > REACH[form][1] - closer[1]] = np.nan
    return A, h


def run_oracle(O, form, A, h, Nx, Ny, Hx, Hy, topo=(P, P)):
    """(Fx, Fy) of compact parents in their precision, with the spacing rounded to it."""
    dx, dy = spacing(A.dtype.type)
    if form == "jacobian":
        assert topo == (P, P)
        return O.lorentz_jacobian(A, h, Nx, Ny, Hx, Hy, dx, dy)
    return O.lorentz_divergence(A, h, Nx, Ny, Hx, Hy, dx, dy, topo=topo)


class Case:
    """The parents of one (form, precision, shape, layout) as the call receives them, and the references of its topologies.
    A, h: (Ny + 2 Hy, stride_y), random interior and random halos up to the reach of the form, NaN beyond it and in the pad columns.
    clean: the compact parents without any NaN (what the oracle is given).  want(O, topo): the oracle's (Fx, Fy) in the precision of
    the call; want64(O, topo): the fp64 oracle on the exactly widened inputs -- compact arrays, computed once and left unchanged."""

    def __init__(self, form, dtype, Nx, Ny, lay):
        self.form, self.dtype, self.Nx, self.Ny, self.lay = form, dtype, Nx, Ny, lay
        self.Hx, self.Hy, self.sy = layout(lay, form, Nx)
        Hx, Hy = self.Hx, self.Hy
        self.clean = Hh.random_case(Nx, Ny, Hx, Hy, seed(Nx, Ny), dtype, periodic=False)
        self.A, self.h = (np.full((Ny + 2 * Hy, self.sy), np.nan, dtype=dtype) for _ in range(2))
        for dst, src in zip((self.A, self.h), poisoned(*self.clean, Nx, Ny, Hx, Hy, form)):
            dst[:, :Nx + 2 * Hx] = src
        self.I = (slice(Hy, Hy + Ny), slice(Hx, Hx + Nx))
        self._want, self._want64 = {}, {}

    def want(self, O, topo=(P, P)):
        if topo not in self._want:
            self._want[topo] = [f[self.I] for f in run_oracle(O, self.form, *self.clean, self.Nx, self.Ny, self.Hx, self.Hy, topo)]
        return self._want[topo]

    def want64(self, O, topo=(P, P)):
        if self.dtype == np.float64:
            return self.want(O, topo)
        if topo not in self._want64:
            wide = [a.astype(np.float64) for a in self.clean]
            self._want64[topo] = [f[self.I] for f in run_oracle(O, self.form, *wide, self.Nx, self.Ny, self.Hx, self.Hy, topo)]
        return self._want64[topo]

    def outputs(self):
        return np.full((2, self.Ny + 2 * self.Hy, self.sy), SENTINEL, dtype=self.dtype)


_cases = {}


def case(form, dtype, Nx, Ny, lay):
    """One Case per (form, precision, shape, layout) of the process: the paths share their inputs and references."""
    key = (form, dtype, Nx, Ny, lay)
    if key not in _cases:
        _cases[key] = Case(*key)
    return _cases[key]


def matrix():
    """(path, form, dtype, layout, topo): one pytest case each."""
    for path, cfg in PATHS.items():
        for form in cfg["forms"]:
            for dtype in DTYPES:
                for lay in LAYOUTS:
                    for topo in cfg["topos"]:
                        yield path, form, dtype, lay, topo


def case_id(path, form, dtype, lay, topo):
    walls = "" if topo == (P, P) else "-" + TOPO_NAME[topo[0]] + TOPO_NAME[topo[1]]
    return f"{path}-{form}-{SFX[dtype]}-{lay}{walls}"


def calls(path, form):
    """(Nx, Ny, (j0, j1), tag) of one pytest case, in order: every shape with its three row ranges, then on the march path the sweep."""
    out = [(Nx, Ny, r, "") for Nx, Ny in shapes(path, form) for r in row_ranges(Ny)]
    if path == "march":
        out += [(*sweep_shape(form), r, "sweep") for r in sweep_ranges()]
    return out


def inputs():
    """(form, dtype, Nx, Ny, layout, topos) of every distinct input of the matrix with the topologies it is run under."""
    seen = {}
    for path, form, dtype, lay, topo in matrix():
        for Nx, Ny, _, _ in calls(path, form):
            seen.setdefault((form, dtype, Nx, Ny, lay), set()).add(topo)
    return [(*k, sorted(v)) for k, v in seen.items()]


def written(rows, Hy, Hx, Nx):
    return (slice(Hy + rows[0], Hy + rows[1]), slice(Hx, Hx + Nx))


def check_call(c, O, path, topo, rows, got, A_after, h_after, worst=None):
    """The assertions of one call as a list of failure texts.  got: (2, Ny + 2 Hy, sy) -- Fx, Fy after the call on c.outputs();
    A_after, h_after: the inputs after it.  worst[(path, form, precision)] collects the largest achieved / allowed error of fast paths."""
    cfg, t, (j0, j1) = PATHS[path], c.dtype, rows
    u = np.uint64 if t == np.float64 else np.uint32
    fails = []
    R = written(rows, c.Hy, c.Hx, c.Nx)
    keep = np.ones(got[0].shape, dtype=bool)
    keep[R] = False
    for k, name in enumerate(("Fx", "Fy")):
        if not np.array_equal(got[k][keep].view(u), np.full(int(keep.sum()), SENTINEL, dtype=t).view(u)):
            n = int((got[k][keep].view(u) != np.array(SENTINEL, dtype=t).view(u)).sum())
            fails.append(f"{name}: {n} cells outside rows [{j0}, {j1}) x [0, Nx) are not the sentinel")
        if j1 <= j0:
            continue
        g = got[k][R]
        if not np.all(np.isfinite(g)):
            fails.append(f"{name}: {int((~np.isfinite(g)).sum())} written values are not finite")
            continue
        if cfg["strict"]:
            w = c.want(O, topo)[k][j0:j1]
            if not np.array_equal(g.view(u), w.view(u)):
                fails.append(f"{name}: {int((g.view(u) != w.view(u)).sum())} written values are not bitwise the oracle's")
        else:
            w = c.want64(O, topo)[k][j0:j1]
            err, scale = np.abs(g.astype(np.float64) - w).max(), np.abs(w).max()
            ratio = err / (TOL[t] * scale) if scale > 0 else np.inf
            if worst is not None:
                key = f"{path}/{c.form}/{SFX[t]}"
                worst[key] = max(worst.get(key, 0.0), float(ratio))
            if not err <= TOL[t] * scale:
                fails.append(f"{name}: max|got - oracle64| = {err:.3e} > {TOL[t]:g} x max|oracle64| = {TOL[t] * scale:.3e}")
        if topo != (P, P) and np.array_equal(c.want(O, topo)[k][j0:j1], c.want(O)[k][j0:j1]):
            fails.append(f"{name}: the oracle's wall result is its periodic result on these rows: no wall branch is exercised")
    for name, after, before in (("A", A_after, c.A), ("h", h_after, c.h)):
        if not np.array_equal(after.view(u), before.view(u)):
            fails.append(f"{name} was changed by the call")
    return fails
