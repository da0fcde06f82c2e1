"""GPU tests of the ScalarBiharmonicDiffusivity closure: the kernel through the ABI (swmhd_biharmonic_rk3_*,
swmhd_ensemble_biharmonic_rk3_*) and ShallowWaterModel / ShallowWaterEnsemble(closure=...).

References: tests/biharmonic_cases.py (the written formula in numpy, pinned on the CPU by test_biharmonic_cases_cpu.py).  Strict results
are compared bitwise; fast results are held to the derived bound |got - ref| <= eps |ref| + 10 eps |a| S against the longdouble value.
Every parent of `old` holds NaN in every cell outside the 13-cell diamonds of the cells the call computes: the halo from depth 3 on,
the halo corner cells the diamond skips, the halo of a wrapped direction, the rows beyond two rows around the row range, the pad columns.
The kernel's workgroup is the Laplacian launch's: 64 rows (four waves of 16) of a strip of 64 lanes x 16 bytes where every parent of the
call has the same 16-byte phase and the pitches keep it, and of 64 elements otherwise; the stage matrix runs both paths, each one
column and one row below, at and above its tile, and the widths and heights 1, 2, 4, 5 at which a wrap of radius 2 folds twice."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import biharmonic_cases as BC
import diffusion_cases as DC
import tracer_cases as TC
from host_call_cases import Transcript

pytestmark = pytest.mark.gpu
NPDT = {"f64": np.float64, "f32": np.float32}
A_STAGE = 0.013 * 0.37              # a = dt gamma of the stage matrix: no RK3 identity that could hide a wrong operand
DT_STAGE = 0.013
NF = 11
H = 3
WRAPS = {"wrapped": (True, True), "wrap-x": (True, False), "wrap-y": (False, True), "halos": (False, False)}


class Case:
    """NF parents of old, new and acc of one (shape, pitch, precision, wrap), halo 3: each set ONE array (NF, Ny + 6, sy), so that with
    sy a multiple of four all parents share their 16-byte phase.  old: random in the interior and in the whole halo; old_for(rows)
    puts NaN wherever the call over `rows` must not read.  new, acc: random interior, the sentinel everywhere else."""

    def __init__(self, Nx, Ny, sy, t, wrap, seed):
        self.Nx, self.Ny, self.Hx, self.Hy, self.sy, self.t, self.wrap = Nx, Ny, H, H, sy, t, wrap
        rng = np.random.default_rng([seed, Nx, Ny])
        shp = (NF, Ny + 2 * H, sy)
        self.I = (slice(None), slice(H, H + Ny), slice(H, H + Nx))
        self.old = np.full(shp, BC.SENTINEL, dtype=t)
        self.old[:, :, :Nx + 2 * H] = rng.standard_normal((NF, Ny + 2 * H, Nx + 2 * H))
        self.new, self.acc = np.full(shp, BC.SENTINEL, dtype=t), np.full(shp, BC.SENTINEL, dtype=t)
        self.new[self.I] = rng.standard_normal((NF, Ny, Nx))
        self.acc[self.I] = rng.standard_normal((NF, Ny, Nx))
        self.coef = [float(t(0.013 * (k + 1) + 0.001 * k * k)) for k in range(NF)]      # distinct, as the call receives them
        self.dx, self.dy = float(t(BC.DX)), float(t(BC.DY))
        self.pad = [BC.pad2(self.old[k, :, :Nx + 2 * H], Nx, Ny, H, H, wrap[0], wrap[1]) for k in range(NF)]
        self._strict, self._exact = {}, {}

    def old_for(self, rows):
        mask = BC.reach(self.Nx, self.Ny, H, H, self.old.shape[1:], self.wrap[0], self.wrap[1], rows)
        return np.where(mask[None], self.old, self.t(np.nan))

    def strict(self, k):
        if k not in self._strict:
            self._strict[k] = BC.biharmonic_strict(self.pad[k], self.coef[k], self.dx, self.dy)
        return self._strict[k]

    def exact(self, k):
        if k not in self._exact:
            self._exact[k] = BC.biharmonic_exact(self.pad[k], self.coef[k], self.dx, self.dy)
        return self._exact[k]


def ptrs(tensor, n):
    step = tensor.stride(0) * tensor.element_size()
    return (ctypes.c_void_p * n)(*[tensor.data_ptr() + k * step for k in range(n)])


def wrap_flags(L, wrap):
    return (L.WRAP_X if wrap[0] else 0) | (L.WRAP_Y if wrap[1] else 0)


def check_outputs(c, got, start, ks, zero, scalar, rows, strict, tag):
    """got, start: (NF, rows, sy) arrays of new or acc after and before the launch; scalar = a or w as the call received it."""
    t, (j0, j1) = c.t, rows
    eps = np.finfo(t).eps
    want = start.copy()
    R = (slice(H + j0, H + j1), slice(H, H + c.Nx))
    for k in ks:
        if k == zero:
            continue
        if strict:
            want[k][R] = BC.correct(start[k][R], c.strict(k)[j0:j1], scalar)
        else:
            E, S = c.exact(k)
            ref = start[k][R].astype(np.longdouble) + np.longdouble(t(scalar)) * E[j0:j1]
            err = np.abs(got[k][R].astype(np.longdouble) - ref)
            bound = BC.fast_bound(ref, t(scalar), S[j0:j1], eps)
            assert np.all(err <= bound), (tag, k, float((err / bound).max()))
            want[k][R] = got[k][R]
    # bitwise: the strict values, and everything the launch must not touch (halos, pad columns, rows outside, the coef == 0 field,
    # the fields beyond the list)
    u = np.uint64 if t == np.float64 else np.uint32
    assert np.array_equal(got.view(u), want.view(u)), tag


@pytest.mark.parametrize("pitch", ["aligned", "odd"])
@pytest.mark.parametrize("wrap", list(WRAPS))
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_stage_matrix(swmhd, sfx, strict, wrap, pitch):
    """Shapes x row ranges {all, [1, Ny - 1), empty} x nfields in {1, 3, 11} (distinct coefficients, the middle one 0 and its old all
    NaN) x {no acc, every acc with w = 1, acc with null entries and w = dt / 4}.  Each wrap flag alone, both, none: an unwrapped
    direction reads its random halo of depth 2, the diagonal cells included.  aligned: stride_y a multiple of four elements (the
    16-byte path); odd: an odd stride_y (one element per lane)."""
    L = swmhd._lib
    t = NPDT[sfx]
    wr = WRAPS[wrap]
    fn = getattr(L.lib(), f"swmhd_biharmonic_rk3_{sfx}")
    flags = (L.STRICT if strict else 0) | wrap_flags(L, wr)
    a = float(t(A_STAGE))
    for Nx, Ny in BC.stage_shapes(np.dtype(t).itemsize, pitch == "aligned"):
        sy = (Nx + 2 * H + 1 + 3) // 4 * 4 if pitch == "aligned" else (Nx + 2 * H + 5) | 1
        c = Case(Nx, Ny, sy, t, wr, 5)
        for rows in BC.row_ranges(Ny):
            old_h = c.old_for(rows)
            old_d = torch.from_numpy(old_h).cuda()
            for n in (1, 3, NF):
                zero = n // 2 if n > 1 else -1
                old_n = old_d
                if zero >= 0:
                    old_n = old_d.clone()
                    old_n[zero] = float("nan")
                coef = ((ctypes.c_double if sfx == "f64" else ctypes.c_float) * n)(*[0.0 if k == zero else c.coef[k] for k in range(n)])
                for w, holes in ((None, ()), (1.0, ()), (float(t(DT_STAGE / 4)), (0, n - 2))):
                    new_d, acc_d = torch.from_numpy(c.new).cuda(), torch.from_numpy(c.acc).cuda()
                    acc_p = ptrs(acc_d, n) if w is not None else None
                    with_acc = [k for k in range(n) if k not in holes] if w is not None else []
                    for k in holes:
                        if 0 <= k < n:
                            acc_p[k] = None
                    rc = fn(ptrs(old_n, n), ptrs(new_d, n), acc_p, ctypes.cast(coef, ctypes.c_void_p), n,
                            Nx, Ny, H, H, sy, c.dx, c.dy, a, w if w is not None else 0.0, rows[0], rows[1], flags, None)
                    L.check(rc, "swmhd_biharmonic_rk3")
                    torch.cuda.synchronize()
                    tag = (Nx, Ny, n, w, rows)
                    check_outputs(c, new_d.cpu().numpy(), c.new, range(n), zero, a, rows, strict, ("new",) + tag)
                    check_outputs(c, acc_d.cpu().numpy(), c.acc, with_acc, zero, w, rows, strict, ("acc",) + tag)
            assert np.array_equal(old_d.cpu().numpy().view(np.uint8), old_h.view(np.uint8))      # old is only read


def test_parents_of_different_phase(swmhd):
    """Parents whose 16-byte phases differ (new one element further into its allocation than old) take the one-element path whatever
    the pitch."""
    L = swmhd._lib
    t, Nx, Ny = np.float64, 129, 17
    sy = 136
    c = Case(Nx, Ny, sy, t, (True, False), 9)
    n = 3
    old_d, acc_d = torch.from_numpy(c.old_for((0, Ny))).cuda(), torch.from_numpy(c.acc).cuda()
    flat = torch.full((c.new.size + 1,), BC.SENTINEL, dtype=torch.float64, device="cuda")
    flat[1:].copy_(torch.from_numpy(c.new).reshape(-1))
    new_p = (ctypes.c_void_p * n)(*[flat.data_ptr() + 8 + k * c.new[0].size * 8 for k in range(n)])
    coef = (ctypes.c_double * n)(*c.coef[:n])
    a, w = float(A_STAGE), 1.0
    for strict in (True, False):
        flat[1:].copy_(torch.from_numpy(c.new).reshape(-1))
        acc_d.copy_(torch.from_numpy(c.acc))
        rc = L.lib().swmhd_biharmonic_rk3_f64(ptrs(old_d, n), new_p, ptrs(acc_d, n), ctypes.cast(coef, ctypes.c_void_p), n, Nx, Ny, H, H, sy,
                                              c.dx, c.dy, a, w, 0, Ny, (L.STRICT if strict else 0) | L.WRAP_X, None)
        L.check(rc, "swmhd_biharmonic_rk3")
        torch.cuda.synchronize()
        assert flat[0].item() == BC.SENTINEL
        check_outputs(c, flat[1:].cpu().numpy().reshape(c.new.shape), c.new, range(n), -1, a, (0, Ny), strict, "new")
        check_outputs(c, acc_d.cpu().numpy(), c.acc, range(n), -1, w, (0, Ny), strict, "acc")


# ----------------------------------------------------------------------------------------------------------------------------------
# ensembles through the ABI
# ----------------------------------------------------------------------------------------------------------------------------------
ENS_GEOMETRIES = {
    # one strip, one row block; the 16-byte path (stride_y and stride_m multiples of four): 9 workgroups
    "one-tile": dict(Nx={"f64": 65, "f32": 65}, Ny=17, sy={"f64": 72, "f32": 72}, gap=8, vec=True),
    # an odd stride_m: one element per lane, two strips of 64 columns, two row blocks: 36 workgroups
    "elem-2x2": dict(Nx={"f64": 65, "f32": 65}, Ny=65, sy={"f64": 72, "f32": 72}, gap=9, vec=False),
    # a width and a height at which the wrap folds twice
    "narrow": dict(Nx={"f64": 2, "f32": 1}, Ny=2, sy={"f64": 8, "f32": 8}, gap=4, vec=True),
}


@pytest.mark.parametrize("name", list(ENS_GEOMETRIES))
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_ensemble_members_are_single_grid_calls(swmhd, sfx, name):
    """Three members that share nothing, stride_m pitched with the sentinel in the gap; per-member coefficients (zeros among them) in
    the device table; dt: one for all (params NULL; w = 1), and per member from the (g, f, dt) table, with w = 1 (the stored tendency)
    and with SWMHD_RK3_ANCHOR (w = 1/4 of each member's dt).  Rows: all, and [1, Ny - 1).  Strict: member m is bitwise the single-grid
    call with coef[m], a = dt_m gamma formed in the element type as the kernel forms it, and its w.  Fast: member m is held to the
    derived bound of the single-grid stage matrix -- not bitwise to the fast single-grid call: two instantiations need not contract
    alike."""
    L = swmhd._lib
    t = NPDT[sfx]
    geo = ENS_GEOMETRIES[name]
    members, n = 3, 3
    Nx, Ny = geo["Nx"][sfx], geo["Ny"]
    sy = geo["sy"][sfx]
    size = (Ny + 2 * H) * sy
    stride_m = size + geo["gap"]
    V = 16 // np.dtype(t).itemsize
    assert (sy % V == 0 and stride_m % V == 0) == geo["vec"]
    ft = ctypes.c_double if sfx == "f64" else ctypes.c_float
    wr = (True, True)
    cases = [Case(Nx, Ny, sy, t, wr, 20 + m) for m in range(members)]
    table = np.array([[0.011 * (m + 1) + 0.002 * k if (m + k) % 4 != 1 else 0.0 for k in range(n)] for m in range(members)], dtype=t)
    for m, c in enumerate(cases):      # the references of check_outputs take the member's coefficients of the table
        c.coef[:n] = [float(x) for x in table[m]]
    dts = np.array([0.013 * (1 + 0.5 * m) for m in range(members)], dtype=t)
    gamma = t(0.37)
    params = np.stack([np.full(members, 9.81), np.ones(members), dts], axis=1).astype(t)
    single = getattr(L.lib(), f"swmhd_biharmonic_rk3_{sfx}")
    ens = getattr(L.lib(), f"swmhd_ensemble_biharmonic_rk3_{sfx}")
    u = np.uint64 if sfx == "f64" else np.uint32
    quarter = t(0.25)

    def pack(arrs):        # (n, members * stride_m): field k of member m at [k, m * stride_m:]
        out = np.full((n, members * stride_m), BC.SENTINEL, dtype=t)
        for m, a in enumerate(arrs):
            out[:, m * stride_m:m * stride_m + size] = a[:n].reshape(n, size)
        return torch.from_numpy(out).cuda()

    for strict in (True, False):
        flags = (L.STRICT if strict else 0) | L.WRAP_X | L.WRAP_Y
        for rows in ((0, Ny), (1, max(Ny - 1, 1))):
            olds = [c.old_for(rows) for c in cases]
            for par, w, anchor in ((False, 1.0, False), (True, 1.0, False), (True, float(quarter), True)):
                old_d, new_d, acc_d = pack(olds), pack([c.new for c in cases]), pack([c.acc for c in cases])
                tab_d, par_d = torch.from_numpy(table).cuda(), torch.from_numpy(params).cuda()
                rc = ens(ptrs(old_d, n), ptrs(new_d, n), ptrs(acc_d, n), tab_d.data_ptr(), n, members, stride_m, Nx, Ny, H, H, sy, cases[0].dx,
                         cases[0].dy, par_d.data_ptr() if par else None, float(gamma) if par else float(dts[0] * gamma), w, rows[0], rows[1],
                         flags | (L.RK3_ANCHOR if anchor else 0), None)
                L.check(rc, "swmhd_ensemble_biharmonic_rk3")
                torch.cuda.synchronize()
                got_new, got_acc = new_d.cpu().numpy(), acc_d.cpu().numpy()
                for m in range(members):
                    tag = (name, strict, rows, par, anchor, m)
                    c = cases[m]
                    a_m = float((dts[m] if par else dts[0]) * gamma)
                    w_m = float(dts[m] * quarter) if anchor else w
                    lo = m * stride_m
                    mine = [g[:, lo:lo + size] for g in (got_new, got_acc)]
                    assert np.all(got_new[:, lo + size:lo + stride_m] == BC.SENTINEL) and np.all(got_acc[:, lo + size:lo + stride_m] == BC.SENTINEL), tag
                    k0 = [k for k in range(n) if table[m, k] == 0]
                    assert len(k0) <= 1
                    if strict:
                        o_d, n_d, a_d = torch.from_numpy(olds[m]).cuda(), torch.from_numpy(c.new).cuda(), torch.from_numpy(c.acc).cuda()
                        coef = (ft * n)(*[float(x) for x in table[m]])
                        rc = single(ptrs(o_d, n), ptrs(n_d, n), ptrs(a_d, n), ctypes.cast(coef, ctypes.c_void_p), n, Nx, Ny, H, H, sy, c.dx, c.dy,
                                    a_m, w_m, rows[0], rows[1], flags, None)
                        L.check(rc, "swmhd_biharmonic_rk3")
                        torch.cuda.synchronize()
                        one_new, one_acc = n_d.cpu().numpy()[:n].reshape(n, size), a_d.cpu().numpy()[:n].reshape(n, size)
                        assert np.array_equal(mine[0].view(u), one_new.view(u)), tag
                        assert np.array_equal(mine[1].view(u), one_acc.view(u)), tag
                        for k in k0:        # a zero of the device table: that field of that member is untouched
                            assert np.array_equal(one_new[k].view(u), c.new[k].reshape(-1).view(u))
                    for got, start, scalar, what in ((mine[0], c.new, a_m, "new"), (mine[1], c.acc, w_m, "acc")):
                        full = start.copy()
                        full[:n] = got.reshape(n, Ny + 2 * H, sy)
                        check_outputs(c, full, start, range(n), k0[0] if k0 else -1, scalar, rows, strict, (what,) + tag)


# ----------------------------------------------------------------------------------------------------------------------------------
# whole runs: 24 x 20 periodic, 3 steps
# ----------------------------------------------------------------------------------------------------------------------------------
NX, NY, DT, STEPS = 24, 20, 2e-3, 3
NU4, ETA4, KAPPA4_C = 2e-5, 3e-5, 1e-5
ETA = 5e-3
DXG, DYG = (TC.DX * NX) / NX, (TC.DY * NY) / NY        # the spacings as RectilinearGrid forms them from the extents
# name -> (closure factory, Laplacian coefficients, biharmonic coefficients) of (u, v, h, A, c)
CLOSURES = {
    "nu": (lambda S: S.ScalarBiharmonicDiffusivity(nu=NU4), [0.0] * 5, [NU4, NU4, 0.0, 0.0, 0.0]),
    "kappa": (lambda S: S.ScalarBiharmonicDiffusivity(kappa={"A": ETA4, "c": KAPPA4_C}), [0.0] * 5, [0.0, 0.0, 0.0, ETA4, KAPPA4_C]),
    "tuple": (lambda S: (S.ScalarDiffusivity(kappa={"A": ETA}), S.ScalarBiharmonicDiffusivity(nu=NU4)),
              [0.0, 0.0, 0.0, ETA, 0.0], [NU4, NU4, 0.0, 0.0, 0.0]),
}
_reference = {}


def _start(O):
    q = TC.fill_state(O, TC.state(NX, NY, 1, 11, rough=False), NX, NY, (TC.P, TC.P))
    c = TC.fill(O, TC.tracer_fields(NX, NY, 1, 11, rough=False)[0], NX, NY, (TC.P, TC.P))
    return q, c


def _model(S, O, closure, strict=True, absent=False):
    g = S.RectilinearGrid(size=(NX, NY), x=(0, TC.DX * NX), y=(0, TC.DY * NY))
    assert g.dx == DXG and g.dy == DYG
    q, c = _start(O)
    kw = {} if absent else {"closure": closure}
    m = S.ShallowWaterModel(g, TC.GRAV, TC.FCOR, strict=strict, tracers=("c",), **kw)
    for f, a in zip(m.fields, q):
        f.data.copy_(torch.from_numpy(a))
    m.tracers["c"].data.copy_(torch.from_numpy(c))
    return m


def _ref(O, name, mode):
    """The reference stepper after STEPS steps, computed once per (closure, mode) and left unchanged."""
    if (name, mode) not in _reference:
        q, c = _start(O)
        r = BC.RefModel(O, q, [c], CLOSURES[name][1], CLOSURES[name][2], NX, NY, 1, 1, mode, DXG, DYG)
        for _ in range(STEPS):
            r.step(DT)
        _reference[(name, mode)] = r
    return _reference[(name, mode)]


def _fields(m):
    return m.fields + [m.tracers["c"]]


@pytest.mark.parametrize("how", ["eager", "graph"])
@pytest.mark.parametrize("name", list(CLOSURES))
def test_strict_runs_are_the_reference(swmhd, oracle, name, how):
    """Strict model, 3 steps: every field bitwise RefModel("classic"), halos included -- hyperviscosity alone, hyperdiffusivity of A
    and a tracer, and the tuple of Laplacian resistivity with hyperviscosity, whose launches run in the stated order.  graph: captured
    and replayed (one eager step, then a replay of two), bitwise the same."""
    S, O = swmhd, oracle
    m = _model(S, O, CLOSURES[name][0](S))
    assert (m._diffusion is not None) == (name == "tuple") and set(m._biharmonic) == {n for n, c in zip(("u", "v", "h", "A", "c"), CLOSURES[name][2]) if c}
    assert DT * max(CLOSURES[name][2]) * BC.LAMBDA_MAX ** 2 < 2.51
    if how == "eager":
        for _ in range(STEPS):
            m.time_step(DT)
    else:
        m.capture_graph(DT)
        m.time_steps(STEPS, DT)
    m.synchronize()
    assert m.iteration == STEPS
    ref = _ref(O, name, "classic")
    for f, a in zip(_fields(m), ref.q + ref.tr):
        assert np.array_equal(f.numpy(), a)
    # and the closure has moved its fields by far more than rounding
    q, c = _start(O)
    plain = DC.RefModel(O, q, [c], CLOSURES[name][1], NX, NY, 1, 1, "classic", DXG, DYG)
    for _ in range(STEPS):
        plain.step(DT)
    moved = [k for k, c4 in enumerate(CLOSURES[name][2]) if c4]
    for k in moved:
        a, b = (plain.q + plain.tr)[k], (ref.q + ref.tr)[k]
        assert np.abs(a - b).max() > 1e4 * np.finfo(np.float64).eps * np.abs(b).max()


def run_fast_allowance(eps, cmax, steps=STEPS):
    """What the fast biharmonic kernel may add to max |field| over a run, relative to it: per stage eps |U| + dt gamma 10 eps S with
    S <= c lambda_max² max |U| (composed over the stages as biharmonic_cases.decay_fast_bound does; dt c lambda_max² << 1 here, so the
    stage maps do not amplify)."""
    return steps * sum(eps + DT * g * BC.UPDATE_ROUNDINGS * eps * cmax * BC.LAMBDA_MAX ** 2 for g in BC.GAMMA)


@pytest.mark.parametrize("name", list(CLOSURES))
def test_fast_runs_follow_the_anchor_reference(swmhd, oracle, name):
    """Fast model (anchor form), same run, against RefModel("anchor"): within the project's fast tolerance of whole runs for the stage
    kernels, 1e-12 max |field| (tests/test_model_gpu.py, tests/test_diffusion_gpu.py), plus the derived allowance of the biharmonic
    launch."""
    S, O = swmhd, oracle
    m = _model(S, O, CLOSURES[name][0](S), strict=False)
    m.time_steps(STEPS, DT)
    m.synchronize()
    ref = _ref(O, name, "anchor")
    tol = 1e-12 + run_fast_allowance(np.finfo(np.float64).eps, max(CLOSURES[name][2]))
    for nm, f, a in zip(list(m.names) + ["c"], _fields(m), ref.q + ref.tr):
        err = np.abs(f.numpy() - a).max() / np.abs(a).max()
        print(f"fast vs anchor reference, {name}, {nm}: {err:.3e} (tolerance {tol:.3e})")
        assert err <= tol


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
def test_without_coefficients_nothing_changes(swmhd, oracle, strict):
    """A model with an all-zero ScalarBiharmonicDiffusivity, alone or in a tuple: the ctypes calls of time_step and time_steps, argument
    by argument, and the state are those of a model built without the argument; and next to a ScalarDiffusivity those of that closure
    alone."""
    S, O = swmhd, oracle
    B = S.ScalarBiharmonicDiffusivity
    lap = S.ScalarDiffusivity(kappa={"A": ETA})

    def run(**kw):
        m = _model(S, O, **kw)
        tr = Transcript()
        tr.watch(m)
        tr.do("time_step", m.time_step, DT)
        tr.do("time_steps", m.time_steps, 3, DT)
        m.synchronize()
        return tr.blocks, [f.numpy() for f in _fields(m)]
    base = run(closure=None, strict=strict, absent=True)
    for closure in (B(), B(nu=0.0, kappa={"A": 0.0}), (B(),), ()):
        got = run(closure=closure, strict=strict)
        assert got[0] == base[0]
        assert all(np.array_equal(x, y) for x, y in zip(got[1], base[1]))
    names = [c[0] for _, calls in base[0] for c in calls]
    assert names and not any("biharmonic" in n or "diffusion" in n for n in names)
    alone = run(closure=lap, strict=strict)
    for closure in ((lap, B()), (B(kappa=0.0), lap)):
        got = run(closure=closure, strict=strict)
        assert got[0] == alone[0]
        assert all(np.array_equal(x, y) for x, y in zip(got[1], alone[1]))
    names = [c[0] for _, calls in alone[0] for c in calls]
    assert any("diffusion" in n for n in names) and not any("biharmonic" in n for n in names)


def test_scalar_diffusivity_alone_is_what_it_was(swmhd, oracle):
    """A model with ScalarDiffusivity alone goes through the unchanged path: bitwise diffusion_cases.RefModel."""
    S, O = swmhd, oracle
    m = _model(S, O, S.ScalarDiffusivity(nu=3e-3, kappa={"A": ETA, "c": 2e-3}))
    assert m._biharmonic is None
    for _ in range(STEPS):
        m.time_step(DT)
    m.synchronize()
    q, c = _start(O)
    ref = DC.RefModel(O, q, [c], [3e-3, 3e-3, 0.0, ETA, 2e-3], NX, NY, 1, 1, "classic", DXG, DYG)
    for _ in range(STEPS):
        ref.step(DT)
    for f, a in zip(_fields(m), ref.q + ref.tr):
        assert np.array_equal(f.numpy(), a)


def test_the_launch_order_of_a_stage(swmhd, oracle):
    """tendencies, tracers, the Laplacian closure, the biharmonic closure: the order that decides the last bits; an operand in storing
    stages only."""
    S, O = swmhd, oracle
    for strict in (True, False):
        m = _model(S, O, (S.ScalarBiharmonicDiffusivity(nu=NU4, kappa={"c": KAPPA4_C}), S.ScalarDiffusivity(kappa={"A": ETA})), strict=strict)
        tr = Transcript()
        tr.watch(m)
        tr.do("step", m.time_steps, 2, DT)
        names = [c[0] for c in tr.blocks[0][1]]
        assert names == ["swmhd_tendencies_rk3_f64", "swmhd_tracers_rk3_f64", "swmhd_diffusion_rk3_f64", "swmhd_biharmonic_rk3_f64"] * 6, names
        calls = [c for c in tr.blocks[0][1] if c[0] == "swmhd_biharmonic_rk3_f64"]
        assert [c[5] for c in calls] == [3] * 6          # u, v, c
        assert [c[3] != "null" for c in calls] == ([True, True, False] if strict else [True, False, False]) * 2
        m.synchronize()


# ---- ensembles ----------------------------------------------------------------------------------------------------------------------
def _ensemble(S, O, strict, dts=None):
    B = 3
    g = S.RectilinearGrid(size=(NX, NY), x=(0, TC.DX * NX), y=(0, TC.DY * NY))
    closure = (S.ScalarBiharmonicDiffusivity(nu=[NU4, 0.0, 2 * NU4], kappa={"A": [ETA4, 2 * ETA4, 0.0], "c": KAPPA4_C}),
               S.ScalarDiffusivity(kappa={"A": [0.0, ETA, ETA]}))
    e = S.ShallowWaterEnsemble(g, B, TC.GRAV, [1.0, 0.5, 2.0] if dts is not None else TC.FCOR, strict=strict, tracers=("c",), closure=closure,
                               member_stride=(NY + 6) * (NX + 6) + 10)
    q, c = _start(O)
    for t_, a in zip(e._state + [e._tr["c"]], q + [c]):
        for m in range(B):
            t_[m].copy_(torch.from_numpy(a * (1.0 + 0.1 * m)))
    return e, closure


@pytest.mark.parametrize("per_member_dt", [False, True], ids=["dt", "dts"])
def test_ensemble_members_are_models(swmhd, oracle, per_member_dt):
    """Strict ensemble of three members with per-member nu4 and eta4 (zeros among them) next to a per-member Laplacian eta, under a
    scalar or per-member dt, 3 steps: member m is bitwise ShallowWaterModel(closure=that member's tuple) stepped alone, and the device
    table holds a zero entry.  The fast ensemble (anchor form; with per-member dt the kernel forms dt_m / 4) stays within the fast
    tolerance of whole runs plus the derived allowance of the launch for the largest coefficient."""
    S, O = swmhd, oracle
    dts = [DT, 1.5 * DT, 0.5 * DT] if per_member_dt else None
    dt = dts if per_member_dt else DT
    e, closure = _ensemble(S, O, True, dts)
    assert e.biharmonic_coefficients.shape == (3, 4) and (e.biharmonic_coefficients == 0).any().item()
    assert e.diffusion_coefficients.shape == (3, 1)
    start = [[t_[m].clone() for t_ in e._state + [e._tr["c"]]] for m in range(3)]
    e.time_steps(STEPS, dt)
    e.synchronize()
    one = e.member(1)
    assert isinstance(one.closure, tuple) and one.closure[0].nu == 0.0 and one.closure[0].kappa == {"A": 2 * ETA4, "c": KAPPA4_C}
    assert one.closure[1].kappa == {"A": ETA}
    for m in range(3):
        alone = e._member_model(m)
        assert alone.closure[0].nu == closure[0].nu[m]
        for f, a in zip(alone._raw_fields + [alone._tr["c"]], start[m]):
            f.data.copy_(a)
        for _ in range(STEPS):
            alone.time_step(dts[m] if per_member_dt else DT)
        alone.synchronize()
        for f, t_ in zip(_fields(alone), e.fields + [e.tracers["c"]]):
            assert torch.equal(f.data, t_[m]), m
    fast, _ = _ensemble(S, O, False, dts)
    fast.time_steps(STEPS, dt)
    fast.synchronize()
    tol = 1e-12 + run_fast_allowance(np.finfo(np.float64).eps, 2 * ETA4)
    for a, b in zip(fast.fields + [fast.tracers["c"]], e.fields + [e.tracers["c"]]):
        assert ((a - b).abs().amax() <= tol * b.abs().amax()).item()


def test_ensemble_graph_replay_and_no_closure_calls(swmhd, oracle):
    S, O = swmhd, oracle
    e, _ = _ensemble(S, O, False)
    g, _ = _ensemble(S, O, False)
    e.time_steps(5, DT)
    g.capture_graph(DT)
    g.time_steps(5, DT)
    e.synchronize(); g.synchronize()
    for a, b in zip(e.fields + [e.tracers["c"]], g.fields + [g.tracers["c"]]):
        assert torch.equal(a, b)
    logs = []
    for kw in ({}, {"closure": S.ScalarBiharmonicDiffusivity()}, {"closure": (S.ScalarBiharmonicDiffusivity(nu=[0.0, 0.0]),)}):
        p = S.ShallowWaterEnsemble(e.grid, 2, **kw)
        tr = Transcript()
        tr.watch(p)
        tr.do("steps", p.time_steps, 2, DT)
        p.synchronize()
        logs.append(tr.blocks)
    assert logs[0] == logs[1] == logs[2] and [c[0] for c in logs[0][0][1]] == ["swmhd_ensemble_step_rk3_f64"]


# ---- decay --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
def test_decay_of_an_eigenmode_on_the_device(swmhd, oracle, strict):
    """A = sin(kx) sin(ly) on a fluid at rest, 16 x 12, 20 steps: A_20 = R(z)^20 A_0, z = -dt c lambda², within the margin the CPU
    reference sets (ten times its own deviation, biharmonic_cases.DECAY_MARGIN); the fast run adds the derived per-stage bound of the
    kernel."""
    S, O = swmhd, oracle
    q, z, R = BC.decay_case()
    Nx, Ny = BC.DECAY_NX, BC.DECAY_NY
    q = [O.fill_halo_periodic(a, Nx, Ny, BC.H, BC.H) for a in q]
    g = S.RectilinearGrid(size=(Nx, Ny), x=(0, BC.DX * Nx), y=(0, BC.DY * Ny))
    closure = S.ScalarBiharmonicDiffusivity(kappa={"A": BC.DECAY_C})
    assert BC.DECAY_DT < closure.max_stable_dt(g)
    m = S.ShallowWaterModel(g, TC.GRAV, TC.FCOR, lorentz_forcing=False, strict=strict, closure=closure)
    for f, a in zip(m.fields, q):
        f.data.copy_(torch.from_numpy(a))
    for _ in range(BC.DECAY_STEPS):
        m.time_step(BC.DECAY_DT)
    m.synchronize()
    I = g.interior
    Rn = R ** BC.DECAY_STEPS
    dev = np.abs(m.solution["A"].numpy()[I] - Rn * q[3][I]).max() / (Rn * np.abs(q[3][I]).max())
    margin = BC.DECAY_MARGIN + (0.0 if strict else BC.decay_fast_bound(np.finfo(np.float64).eps) / Rn)
    print(f"decay on the device ({'strict' if strict else 'fast'}): relative deviation {dev:.3e}, margin {margin:.3e}")
    assert dev <= margin
    assert not m.solution["u"].numpy()[I].any() and not m.solution["v"].numpy()[I].any() and (m.solution["h"].numpy()[I] == 1.0).all()


# ---- the example --------------------------------------------------------------------------------------------------------------------
def test_example_runs_with_hyperviscosity(tmp_path):
    """examples/run_swmhd.py --hyperviscosity --hyperdiffusivity next to --diffusivity on 64^2 for a few steps: the progress lines, the
    dump and its fields exist and are finite."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "examples", "run_swmhd.py"), "--size", "64", "--stop-time", "0.1", "--every", "5",
           "--dump-every", "0.1", "--out", str(tmp_path), "--hyperviscosity", "1e-7", "--hyperdiffusivity", "1e-7", "--diffusivity", "1e-3"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "ScalarBiharmonicDiffusivity" in r.stdout and "ScalarDiffusivity(" in r.stdout
    assert len([l for l in r.stdout.splitlines() if l.startswith("Time:")]) >= 2
    z = np.load(os.path.join(str(tmp_path), "fields_0000010.npz"))
    for n in ("u", "v", "h", "A"):
        assert np.isfinite(z[n]).all()
