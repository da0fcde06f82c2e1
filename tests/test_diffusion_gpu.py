"""GPU tests of the ScalarDiffusivity closure: the kernel through the ABI (swmhd_diffusion_rk3_*, swmhd_ensemble_diffusion_rk3_*) and
ShallowWaterModel / ShallowWaterEnsemble(closure=...).

References: tests/diffusion_cases.py (the written formula in numpy, pinned on the CPU by test_diffusion_cases_cpu.py).  Strict results
are compared bitwise; fast results are held to the derived bound |got - ref| <= eps |ref| + 10 eps |a| S against the longdouble value.
The kernel's workgroup covers SWMHD_DIFFUSION_TILE_ROWS = 64 rows (four waves of 16) of a strip of 64 lanes x 16 bytes (128 doubles, 256
floats) where every parent of the call has the same 16-byte phase and the pitches keep it, and of 64 elements otherwise: the stage
matrix runs both paths, each one column and one row below, at and above its tile."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import diffusion_cases as DC
import tracer_cases as TC
from host_call_cases import Transcript

pytestmark = pytest.mark.gpu
NPDT = {"f64": np.float64, "f32": np.float32}
A_STAGE = 0.013 * 0.37              # a = dt gamma of the stage matrix: no RK3 identity that could hide a wrong operand
DT_STAGE = 0.013
NF = 11


class Case:
    """NF parents of old, new and acc of one (shape, halo, pitch, precision): each set ONE array (NF, Ny + 2 Hy, sy), so that with
    sy a multiple of four all parents share their 16-byte phase.  old: random interior; halo NaN (wrapped) or random (read as it is);
    pad columns the sentinel.  new, acc: random interior, the sentinel everywhere else."""

    def __init__(self, Nx, Ny, Hx, Hy, sy, t, wrap, seed):
        self.Nx, self.Ny, self.Hx, self.Hy, self.sy, self.t, self.wrap = Nx, Ny, Hx, Hy, sy, t, wrap
        rng = np.random.default_rng([seed, Nx, Ny])
        shp = (NF, Ny + 2 * Hy, sy)
        self.I = (slice(None), slice(Hy, Hy + Ny), slice(Hx, Hx + Nx))
        self.old = np.full(shp, DC.SENTINEL, dtype=t)
        self.old[:, :, :Nx + 2 * Hx] = np.nan if wrap else rng.standard_normal((NF, Ny + 2 * Hy, Nx + 2 * Hx))
        self.old[self.I] = rng.standard_normal((NF, Ny, Nx))
        self.new, self.acc = np.full(shp, DC.SENTINEL, dtype=t), np.full(shp, DC.SENTINEL, dtype=t)
        self.new[self.I] = rng.standard_normal((NF, Ny, Nx))
        self.acc[self.I] = rng.standard_normal((NF, Ny, Nx))
        self.coef = [float(t(0.013 * (k + 1) + 0.001 * k * k)) for k in range(NF)]      # distinct, as the call receives them
        self.dx, self.dy = float(t(DC.DX)), float(t(DC.DY))
        self.pad = [DC.pad1(self.old[k, :, :Nx + 2 * Hx], Nx, Ny, Hx, Hy, wrap, wrap) for k in range(NF)]
        self._strict, self._exact = {}, {}

    def strict(self, k):
        if k not in self._strict:
            self._strict[k] = DC.laplacian_strict(self.pad[k], self.coef[k], self.dx, self.dy)
        return self._strict[k]

    def exact(self, k):
        if k not in self._exact:
            self._exact[k] = DC.laplacian_exact(self.pad[k], self.coef[k], self.dx, self.dy)
        return self._exact[k]


def ptrs(tensor, n):
    step = tensor.stride(0) * tensor.element_size()
    return (ctypes.c_void_p * n)(*[tensor.data_ptr() + k * step for k in range(n)])


def check_outputs(c, got, start, ks, zero, scalar, rows, strict, tag):
    """got, start: (NF, rows, sy) arrays of new or acc after and before the launch; scalar = a or w as the call received it."""
    t, (j0, j1) = c.t, rows
    eps = np.finfo(t).eps
    want = start.copy()
    R = (slice(c.Hy + j0, c.Hy + j1), slice(c.Hx, c.Hx + c.Nx))
    for k in ks:
        if k == zero:
            continue
        if strict:
            want[k][R] = DC.correct(start[k][R], c.strict(k)[j0:j1], scalar)
        else:
            E, S = c.exact(k)
            ref = start[k][R].astype(np.longdouble) + np.longdouble(t(scalar)) * E[j0:j1]
            err = np.abs(got[k][R].astype(np.longdouble) - ref)
            assert np.all(err <= DC.fast_bound(ref, t(scalar), S[j0:j1], eps)), (tag, k, float((err / (eps * (np.abs(ref) + S[j0:j1]))).max()))
            want[k][R] = got[k][R]
    # bitwise: the strict values, and everything the launch must not touch (halos, pad columns, rows outside, the coef == 0 field,
    # the fields beyond the list)
    u = np.uint64 if t == np.float64 else np.uint32
    assert np.array_equal(got.view(u), want.view(u)), tag


@pytest.mark.parametrize("pitch", ["aligned", "odd"])
@pytest.mark.parametrize("wrap", [True, False], ids=["wrapped", "halos"])
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_stage_matrix(swmhd, sfx, strict, wrap, pitch):
    """Shapes x nfields in {1, 3, 11} (distinct coefficients, the middle one 0) x {no acc, w = 1, w = dt / 4} x row ranges {all, [1, Ny -
    1), empty}.  wrapped: SWMHD_WRAP_X | _Y with NaN in every halo (Hx = Hy = 3); halos: random halos of depth Hx = 2, Hy = 1, read
    as they are.  aligned: stride_y a multiple of four elements (the 16-byte path); odd: an odd stride_y (one element per lane)."""
    L = swmhd._lib
    t = NPDT[sfx]
    Hx, Hy = (3, 3) if wrap else (2, 1)
    fn = getattr(L.lib(), f"swmhd_diffusion_rk3_{sfx}")
    flags = (L.STRICT if strict else 0) | ((L.WRAP_X | L.WRAP_Y) if wrap else 0)
    a = float(t(A_STAGE))
    for Nx, Ny in DC.stage_shapes(np.dtype(t).itemsize, pitch == "aligned"):
        sy = (Nx + 2 * Hx + 1 + 3) // 4 * 4 if pitch == "aligned" else (Nx + 2 * Hx + 5) | 1
        c = Case(Nx, Ny, Hx, Hy, sy, t, wrap, 5)
        old_d = torch.from_numpy(c.old).cuda()
        for n in (1, 3, NF):
            zero = n // 2 if n > 1 else -1
            coef = ((ctypes.c_double if sfx == "f64" else ctypes.c_float) * n)(*[0.0 if k == zero else c.coef[k] for k in range(n)])
            for w in (None, 1.0, float(t(DT_STAGE / 4))):
                for rows in DC.row_ranges(Ny):
                    new_d, acc_d = torch.from_numpy(c.new).cuda(), torch.from_numpy(c.acc).cuda()
                    rc = fn(ptrs(old_d, n), ptrs(new_d, n), ptrs(acc_d, n) if w is not None else None, ctypes.cast(coef, ctypes.c_void_p), n,
                            Nx, Ny, Hx, Hy, sy, c.dx, c.dy, a, w if w is not None else 0.0, rows[0], rows[1], flags, None)
                    L.check(rc, "swmhd_diffusion_rk3")
                    torch.cuda.synchronize()
                    tag = (Nx, Ny, n, w, rows)
                    check_outputs(c, new_d.cpu().numpy(), c.new, range(n), zero, a, rows, strict, ("new",) + tag)
                    check_outputs(c, acc_d.cpu().numpy(), c.acc, range(n) if w is not None else [], zero, w, rows, strict, ("acc",) + tag)
        assert np.array_equal(old_d.cpu().numpy().view(np.uint8), c.old.view(np.uint8))      # old is only read


def test_parents_of_different_phase_and_null_acc_entries(swmhd):
    """Parents whose 16-byte phases differ (new one element further into its allocation than old) take the one-element path whatever
    the pitch; acc entries may be null one by one."""
    L = swmhd._lib
    t, Nx, Ny, Hx, Hy = np.float64, 129, 17, 3, 3
    sy = 136
    c = Case(Nx, Ny, Hx, Hy, sy, t, True, 9)
    n = 3
    old_d, acc_d = torch.from_numpy(c.old).cuda(), torch.from_numpy(c.acc).cuda()
    flat = torch.full((c.new.size + 1,), DC.SENTINEL, dtype=torch.float64, device="cuda")
    flat[1:].copy_(torch.from_numpy(c.new).reshape(-1))
    new_p = (ctypes.c_void_p * n)(*[flat.data_ptr() + 8 + k * c.new[0].size * 8 for k in range(n)])
    acc_p = ptrs(acc_d, n)
    acc_p[1] = None
    coef = (ctypes.c_double * n)(*c.coef[:n])
    a, w = float(A_STAGE), 1.0
    rc = L.lib().swmhd_diffusion_rk3_f64(ptrs(old_d, n), new_p, acc_p, ctypes.cast(coef, ctypes.c_void_p), n, Nx, Ny, Hx, Hy, sy, c.dx, c.dy,
                                         a, w, 0, Ny, L.STRICT | L.WRAP_X | L.WRAP_Y, None)
    L.check(rc, "swmhd_diffusion_rk3")
    torch.cuda.synchronize()
    assert flat[0].item() == DC.SENTINEL
    check_outputs(c, flat[1:].cpu().numpy().reshape(c.new.shape), c.new, range(n), -1, a, (0, Ny), True, "new")
    check_outputs(c, acc_d.cpu().numpy(), c.acc, [0, 2], -1, w, (0, Ny), True, "acc")


# ----------------------------------------------------------------------------------------------------------------------------------
# ensembles through the ABI
# ----------------------------------------------------------------------------------------------------------------------------------
# (Nx by precision, Ny, stride_y by precision, elements added to stride_m): the launch of three members and three fields has
# 9 x strips x row blocks workgroups
ENS_GEOMETRIES = {
    # one strip, one row block; the 16-byte path (stride_y and stride_m multiples of four): 9 workgroups
    "one-tile": dict(Nx={"f64": 65, "f32": 65}, Ny=17, sy={"f64": 72, "f32": 72}, gap=8, vec=True),
    # the 16-byte path with two strips (128 doubles | 256 floats each) and two row blocks of 64 rows: 36 workgroups, no multiple of 8
    "vec-2x2": dict(Nx={"f64": 129, "f32": 257}, Ny=65, sy={"f64": 136, "f32": 264}, gap=8, vec=True),
    # an odd stride_m: one element per lane, two strips of 64 columns, two row blocks: 36 workgroups
    "elem-2x2": dict(Nx={"f64": 65, "f32": 65}, Ny=65, sy={"f64": 72, "f32": 72}, gap=9, vec=False),
}


@pytest.mark.parametrize("members", [1, 3])
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_ensemble_members_are_single_grid_calls(swmhd, sfx, members):
    """Three fields, stride_m pitched with the sentinel in the gap; per-member coefficients (one of them 0) in the device table; dt: one
    for all (params NULL; w = 1), and per member from the (g, f, dt) table, with w = 1 (the stored tendency) and with SWMHD_RK3_ANCHOR
    (w = 1/4 of each member's dt).  Geometries (ENS_GEOMETRIES): 65 x 17, one tile per member and field; two strips x two row blocks on
    the 16-byte path and on the one-element path (an odd stride_m), where the kernel's decode of blockIdx into (member, field, tile)
    has more than one tile to tell apart.  Rows: all, and [1, Ny - 1), where rows 0 and Ny - 1 of every member stay bitwise what they
    were.  Strict: member m is bitwise the single-grid call with coef[m], a = dt_m gamma formed in the element type as the kernel
    forms it, and its w.  Fast: member m is held to the derived bound of the single-grid stage matrix (check_outputs, against the
    longdouble value with the coefficients of the table as rounded to the precision of the call) -- not bitwise to the fast
    single-grid call: two instantiations need not contract alike.  Then (strict) a member full of NaN leaves the others bitwise what
    they were."""
    L = swmhd._lib
    t = NPDT[sfx]
    for name, geo in ENS_GEOMETRIES.items():
        for strict in (True, False):
            _ensemble_abi_case(L, sfx, t, members, name, geo, strict)


def _ensemble_abi_case(L, sfx, t, members, name, geo, strict):
    Nx, Ny, Hx, Hy, n = geo["Nx"][sfx], geo["Ny"], 3, 3, 3
    sy = geo["sy"][sfx]
    size = (Ny + 2 * Hy) * sy
    stride_m = size + geo["gap"]
    V = 16 // np.dtype(t).itemsize
    assert (sy % V == 0 and stride_m % V == 0) == geo["vec"]
    ft = ctypes.c_double if sfx == "f64" else ctypes.c_float
    cases = [Case(Nx, Ny, Hx, Hy, sy, t, True, 20 + m) for m in range(members)]
    table = np.array([[0.011 * (m + 1) + 0.002 * k if (m + k) % 4 != 1 else 0.0 for k in range(n)] for m in range(members)], dtype=t)
    for m, c in enumerate(cases):      # the references of check_outputs take the member's coefficients of the table
        c.coef[:n] = [float(x) for x in table[m]]
    dts = np.array([0.013 * (1 + 0.5 * m) for m in range(members)], dtype=t)
    gamma = t(0.37)
    params = np.stack([np.full(members, 9.81), np.ones(members), dts], axis=1).astype(t)
    single = getattr(L.lib(), f"swmhd_diffusion_rk3_{sfx}")
    ens = getattr(L.lib(), f"swmhd_ensemble_diffusion_rk3_{sfx}")
    flags = (L.STRICT if strict else 0) | L.WRAP_X | L.WRAP_Y

    def pack(arrs):        # (n, members * stride_m): field k of member m at [k, m * stride_m:]
        out = np.full((n, members * stride_m), DC.SENTINEL, dtype=t)
        for m, a in enumerate(arrs):
            out[:, m * stride_m:m * stride_m + size] = a[:n].reshape(n, size)
        return torch.from_numpy(out).cuda()

    def run_ensemble(olds, par, w, anchor, rows):
        old_d, new_d, acc_d = pack(olds), pack([c.new for c in cases]), pack([c.acc for c in cases])
        tab_d, par_d = torch.from_numpy(table).cuda(), torch.from_numpy(params).cuda()
        rc = ens(ptrs(old_d, n), ptrs(new_d, n), ptrs(acc_d, n), tab_d.data_ptr(), n, members, stride_m, Nx, Ny, Hx, Hy, sy, cases[0].dx,
                 cases[0].dy, par_d.data_ptr() if par else None, float(gamma) if par else float(dts[0] * gamma), w, rows[0], rows[1],
                 flags | (L.RK3_ANCHOR if anchor else 0), None)
        L.check(rc, "swmhd_ensemble_diffusion_rk3")
        torch.cuda.synchronize()
        return new_d.cpu().numpy(), acc_d.cpu().numpy()

    def run_single(m, a, w, rows):
        c = cases[m]
        old_d, new_d, acc_d = torch.from_numpy(c.old).cuda(), torch.from_numpy(c.new).cuda(), torch.from_numpy(c.acc).cuda()
        coef = (ft * n)(*[float(x) for x in table[m]])
        rc = single(ptrs(old_d, n), ptrs(new_d, n), ptrs(acc_d, n), ctypes.cast(coef, ctypes.c_void_p), n, Nx, Ny, Hx, Hy, sy, c.dx, c.dy,
                    a, w, rows[0], rows[1], flags, None)
        L.check(rc, "swmhd_diffusion_rk3")
        torch.cuda.synchronize()
        return new_d.cpu().numpy()[:n].reshape(n, size), acc_d.cpu().numpy()[:n].reshape(n, size)

    u = np.uint64 if sfx == "f64" else np.uint32
    quarter = t(0.25)
    outer = [Hy, Hy + Ny - 1]      # parent rows of the rows 0 and Ny - 1
    for rows in ((0, Ny), (1, Ny - 1)):
        for par, w, anchor in ((False, 1.0, False), (True, 1.0, False), (True, float(quarter), True)):
            got_new, got_acc = run_ensemble([c.old for c in cases], par, w, anchor, rows)
            for m in range(members):
                tag = (name, strict, rows, par, anchor, m)
                a_m = float((dts[m] if par else dts[0]) * gamma)
                w_m = float(dts[m] * quarter) if anchor else w
                lo = m * stride_m
                mine = [g[:, lo:lo + size] for g in (got_new, got_acc)]
                assert np.all(got_new[:, lo + size:lo + stride_m] == DC.SENTINEL) and np.all(got_acc[:, lo + size:lo + stride_m] == DC.SENTINEL), tag
                k0 = [k for k in range(n) if table[m, k] == 0]
                if strict:
                    one_new, one_acc = run_single(m, a_m, w_m, rows)
                    assert np.array_equal(mine[0].view(u), one_new.view(u)), tag
                    assert np.array_equal(mine[1].view(u), one_acc.view(u)), tag
                    for k in k0:        # a zero of the device table: that field of that member is untouched
                        assert np.array_equal(one_new[k].view(u), cases[m].new[k].reshape(-1).view(u))
                else:
                    for got, start, scalar, what in ((mine[0], cases[m].new, a_m, "new"), (mine[1], cases[m].acc, w_m, "acc")):
                        full = start.copy()
                        full[:n] = got.reshape(n, Ny + 2 * Hy, sy)
                        check_outputs(cases[m], full, start, range(n), k0[0] if k0 else -1, scalar, rows, False, (what,) + tag)
                if rows[0] > 0:         # rows 0 and Ny - 1 of every member and field: bitwise what they were
                    for got, start in ((mine[0], cases[m].new), (mine[1], cases[m].acc)):
                        assert np.array_equal(got.reshape(n, Ny + 2 * Hy, sy)[:, outer].view(u), start[:n][:, outer].view(u)), tag
    if members > 1 and strict:
        clean = run_ensemble([c.old for c in cases], True, 1.0, False, (0, Ny))
        olds = [c.old for c in cases]
        olds[1] = np.full_like(olds[1], np.nan)
        bad = run_ensemble(olds, True, 1.0, False, (0, Ny))
        for x, y in zip(clean, bad):
            for m in (0, 2):
                assert np.array_equal(x[:, m * stride_m:(m + 1) * stride_m].view(u), y[:, m * stride_m:(m + 1) * stride_m].view(u))
        I1 = bad[0][:, stride_m:stride_m + size].reshape(n, Ny + 2 * Hy, sy)[:, Hy:Hy + Ny, Hx:Hx + Nx]
        assert all(np.isnan(I1[k]).all() for k in range(n) if table[1, k] != 0)


# ----------------------------------------------------------------------------------------------------------------------------------
# whole runs
# ----------------------------------------------------------------------------------------------------------------------------------
DT, STEPS = 2e-3, 10
NU, ETA, KAPPA_D = 3e-3, 5e-3, 2e-3
RUN_GRIDS = [(48, 40), (64, 64)]
_reference = {}


def _closure(S, form):
    """nu only with the vector-invariant formulation; c gets A's coefficient, d its own."""
    return S.ScalarDiffusivity(nu=NU if form == 1 else 0.0, kappa={"A": ETA, "c": ETA, "d": KAPPA_D})


def _start(O, Nx, Ny, form):
    q = TC.fill_state(O, TC.state(Nx, Ny, form, 11, rough=False), Nx, Ny, (TC.P, TC.P))
    d = TC.fill(O, TC.tracer_fields(Nx, Ny, 2, 11, rough=False)[1], Nx, Ny, (TC.P, TC.P))
    return q, d


def _model(S, O, Nx, Ny, form, strict=True, closure="default", lorentz=True, tracers=("c", "d")):
    g = S.RectilinearGrid(size=(Nx, Ny), x=(0, TC.DX * Nx), y=(0, TC.DY * Ny))
    q, d = _start(O, Nx, Ny, form)
    kw = {} if closure == "absent" else {"closure": _closure(S, form) if closure == "default" else closure}
    m = S.ShallowWaterModel(g, TC.GRAV, TC.FCOR, formulation=TC.FORM_NAME[form], strict=strict, lorentz_forcing=lorentz, tracers=tracers, **kw)
    for f, a in zip(m.fields, q):
        f.data.copy_(torch.from_numpy(a))
    if tracers:
        m.tracers["c"].data.copy_(torch.from_numpy(q[3]))
        m.tracers["d"].data.copy_(torch.from_numpy(d))
    return m


def _ref(O, Nx, Ny, form, lor):
    """The reference stepper after STEPS steps, computed once per (grid, formulation) and left unchanged."""
    key = (Nx, Ny, form)
    if key not in _reference:
        q, d = _start(O, Nx, Ny, form)
        nu = NU if form == 1 else 0.0
        dx, dy = (TC.DX * Nx) / Nx, (TC.DY * Ny) / Ny        # the spacings as RectilinearGrid forms them from the extents
        r = DC.RefModel(O, q, [q[3], d], [nu, nu, 0.0, ETA, ETA, KAPPA_D], Nx, Ny, form, lor, "classic", dx, dy)
        for _ in range(STEPS):
            r.step(DT)
        _reference[key] = r
    return _reference[key]


@pytest.mark.parametrize("how", ["eager", "graph", "checkpoint"])
@pytest.mark.parametrize("form,lor", TC.FORMS)
@pytest.mark.parametrize("Nx,Ny", RUN_GRIDS)
def test_strict_runs_are_the_reference(swmhd, oracle, tmp_path, Nx, Ny, form, lor, how):
    """Strict model with nu (vector invariant), eta on A and c, another kappa on d, 10 steps: every field bitwise the reference stepper,
    halos included -- stepped eagerly; through capture_graph with time_steps(5) twice, so that the second call starts on swapped roles
    (one eager step, then replays); and across a save_checkpoint / load_checkpoint at step 5."""
    S, O = swmhd, oracle
    m = _model(S, O, Nx, Ny, form)
    assert m.grid.dx == (TC.DX * Nx) / Nx and m.grid.dy == (TC.DY * Ny) / Ny
    ref = _ref(O, Nx, Ny, form, lor)
    if how == "eager":
        for _ in range(STEPS):
            m.time_step(DT)
    elif how == "graph":
        m.capture_graph(DT)
        m.time_steps(5, DT)
        m.time_steps(5, DT)
    else:
        m.time_steps(5, DT)
        path = str(tmp_path / "ck.npz")
        m.save_checkpoint(path)
        m = _model(S, O, Nx, Ny, form)
        m.tracers["d"].data.zero_()
        m.load_checkpoint(path)
        m.time_steps(5, DT)
    m.synchronize()
    assert m.iteration == STEPS
    for f, a in zip(m.fields, ref.q):
        assert np.array_equal(f.numpy(), a)
    assert np.array_equal(m.tracers["c"].numpy(), ref.tr[0]) and np.array_equal(m.tracers["d"].numpy(), ref.tr[1])


@pytest.mark.parametrize("form,lor", TC.FORMS)
@pytest.mark.parametrize("Nx,Ny", RUN_GRIDS)
def test_fast_runs_follow_the_strict_run(swmhd, oracle, Nx, Ny, form, lor):
    """Fast model (anchor form), same run: within the project's fast tolerance of whole runs, 1e-12 max |field| (tests/test_model_gpu.py),
    of the strict result; and the closure has moved A by far more than that."""
    S, O = swmhd, oracle
    m = _model(S, O, Nx, Ny, form, strict=False)
    plain = _model(S, O, Nx, Ny, form, strict=False, closure=None)
    m.time_steps(STEPS, DT)
    plain.time_steps(STEPS, DT)
    m.synchronize(); plain.synchronize()
    ref = _ref(O, Nx, Ny, form, lor)
    for name, f, a in zip(list(m.names) + ["c", "d"], m.fields + [m.tracers["c"], m.tracers["d"]], ref.q + ref.tr):
        err = np.abs(f.numpy() - a).max() / np.abs(a).max()
        print(f"fast vs strict {Nx}x{Ny} form {form} {name}: {err:.3e}")
        assert err <= 1e-12
    assert np.abs(plain.solution["A"].numpy() - ref.q[3]).max() > 1e-6 * np.abs(ref.q[3]).max()


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
def test_without_coefficients_nothing_changes(swmhd, oracle, strict):
    """closure=None and ScalarDiffusivity() (nu = kappa = 0): the ctypes calls of time_step and time_steps, argument by argument, and
    the state are those of a model built without the argument."""
    S, O = swmhd, oracle
    out = []
    for closure in ("absent", None, S.ScalarDiffusivity(), S.ScalarDiffusivity(nu=0.0, kappa={"A": 0.0})):
        for tracers in ((), ("c", "d")):
            m = _model(S, O, 48, 40, 1, strict=strict, closure=closure, tracers=tracers)
            tr = Transcript()
            tr.watch(m)
            tr.do("time_step", m.time_step, DT)
            tr.do("time_steps", m.time_steps, 3, DT)
            m.synchronize()
            out.append((bool(tracers), tr.blocks, [f.numpy() for f in m.fields]))
    for with_tracers in (False, True):
        same = [o for o in out if o[0] == with_tracers]
        assert len(same) == 4
        for o in same[1:]:
            assert o[1] == same[0][1]
            assert all(np.array_equal(x, y) for x, y in zip(o[2], same[0][2]))
    names = [c[0] for _, calls in out[0][1] for c in calls]
    assert not any("diffusion" in n for n in names) and names


def test_the_closure_adds_one_launch_per_stage(swmhd, oracle):
    S, O = swmhd, oracle
    for strict in (True, False):
        m = _model(S, O, 48, 40, 1, strict=strict)
        tr = Transcript()
        tr.watch(m)
        tr.do("step", m.time_steps, 2, DT)
        names = [c[0] for c in tr.blocks[0][1]]
        assert names == ["swmhd_tendencies_rk3_f64", "swmhd_tracers_rk3_f64", "swmhd_diffusion_rk3_f64"] * 6, names
        calls = [c for c in tr.blocks[0][1] if c[0] == "swmhd_diffusion_rk3_f64"]
        # u, v, A, c, d; an operand in storing stages only: stages 0, 1 (classic) or stage 0 (anchor)
        assert [c[5] for c in calls] == [5] * 6
        assert [c[3] != "null" for c in calls] == ([True, True, False] if strict else [True, False, False]) * 2
        m.synchronize()


@pytest.mark.parametrize("form,lor", TC.FORMS)
def test_a_tracer_with_the_coefficient_of_A_stays_A(swmhd, oracle, form, lor):
    """lorentz_forcing=False, kappa["c"] = kappa["A"], c := A: c stays bitwise A, halos included (strict)."""
    S, O = swmhd, oracle
    m = _model(S, O, 48, 40, form, lorentz=False)
    for _ in range(STEPS):
        m.time_step(DT)
    m.synchronize()
    assert np.array_equal(m.tracers["c"].numpy(), m.solution["A"].numpy())
    assert not np.array_equal(m.tracers["d"].numpy(), m.solution["A"].numpy())


def test_tendency_events_with_a_closure(swmhd, oracle):
    S, O = swmhd, oracle
    m = _model(S, O, 48, 40, 1)
    plain = _model(S, O, 48, 40, 1)
    m.tendency_events = []
    m.time_steps(2, DT)
    plain.time_steps(2, DT)
    m.synchronize(); plain.synchronize()
    assert len(m.tendency_events) == 6 and all(e0.elapsed_time(e1) >= 0 for e0, e1, _ in m.tendency_events)
    assert all(np.array_equal(a.numpy(), b.numpy()) for a, b in zip(m.fields, plain.fields))


# ---- ensembles ----------------------------------------------------------------------------------------------------------------------
def _ensemble(S, O, strict, dts=None):
    Nx, Ny, B = 48, 40, 3
    g = S.RectilinearGrid(size=(Nx, Ny), x=(0, TC.DX * Nx), y=(0, TC.DY * Ny))
    closure = S.ScalarDiffusivity(nu=[NU, 0.0, 2 * NU], kappa={"A": [ETA, 2 * ETA, 0.0], "c": KAPPA_D})
    e = S.ShallowWaterEnsemble(g, B, TC.GRAV, [1.0, 0.5, 2.0] if dts is not None else TC.FCOR, strict=strict, tracers=("c",), closure=closure,
                               member_stride=(Ny + 6) * (Nx + 6) + 10)
    q, d = _start(O, Nx, Ny, 1)
    for t_, a in zip(e._state + [e._tr["c"]], q + [d]):
        for m in range(B):
            t_[m].copy_(torch.from_numpy(a * (1.0 + 0.1 * m)))
    return e, closure


@pytest.mark.parametrize("per_member_dt", [False, True], ids=["dt", "dts"])
def test_ensemble_members_are_models(swmhd, oracle, per_member_dt):
    """Strict ensemble of three members with per-member nu and eta (zeros among them) and a scalar or per-member dt, 4 steps: member m
    is bitwise ShallowWaterModel(closure=that member's) stepped alone, and member(1) taken after 2 steps and stepped 2 more alone is
    bitwise member 1 of the ensemble.  The fast ensemble (anchor form; with per-member dt the kernel forms dt_m / 4) stays within 1e-12."""
    S, O = swmhd, oracle
    dts = [DT, 1.5 * DT, 0.5 * DT] if per_member_dt else None
    dt = dts if per_member_dt else DT
    e, closure = _ensemble(S, O, True, dts)
    start = [[t_[m].clone() for t_ in e._state + [e._tr["c"]]] for m in range(3)]
    e.time_steps(2, dt)
    one = e.member(1)
    assert one.closure.nu == 0.0 and one.closure.kappa == {"A": 2 * ETA, "c": KAPPA_D}
    e.time_steps(2, dt)
    one.time_steps(2, dts[1] if per_member_dt else DT)
    e.synchronize(); one.synchronize()
    for f, t_ in zip(one.fields + [one.tracers["c"]], e.fields + [e.tracers["c"]]):
        assert torch.equal(f.data, t_[1])
    for m in range(3):
        alone = e._member_model(m)
        assert alone.closure.nu == closure.nu[m]
        for f, a in zip(alone._raw_fields + [alone._tr["c"]], start[m]):
            f.data.copy_(a)
        for _ in range(4):
            alone.time_step(dts[m] if per_member_dt else DT)
        alone.synchronize()
        for f, t_ in zip(alone.fields + [alone.tracers["c"]], e.fields + [e.tracers["c"]]):
            assert torch.equal(f.data, t_[m]), m
    fast, _ = _ensemble(S, O, False, dts)
    fast.time_steps(4, dt)
    fast.synchronize()
    for a, b in zip(fast.fields + [fast.tracers["c"]], e.fields + [e.tracers["c"]]):
        assert ((a - b).abs().amax() <= 1e-12 * b.abs().amax()).item()


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
    grid = e.grid
    logs = []
    for kw in ({}, {"closure": None}, {"closure": S.ScalarDiffusivity()}):
        p = S.ShallowWaterEnsemble(grid, 2, **kw)
        tr = Transcript()
        tr.watch(p)
        tr.do("steps", p.time_steps, 2, DT)
        p.synchronize()
        logs.append(tr.blocks)
    assert logs[0] == logs[1] == logs[2] and [c[0] for c in logs[0][0][1]] == ["swmhd_ensemble_step_rk3_f64"]


# ---- decay --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
def test_decay_of_an_eigenmode_on_the_device(swmhd, oracle, strict):
    """A = sin(kx) sin(ly) on a fluid at rest, 16 x 12, 20 steps: A_20 = R(z)^20 A_0 within the margin the CPU reference sets (ten
    times its own deviation, diffusion_cases.DECAY_MARGIN); the fast run adds the derived per-stage bound of the kernel."""
    S, O = swmhd, oracle
    q, z, R = DC.decay_case()
    Nx, Ny = DC.DECAY_NX, DC.DECAY_NY
    q = [O.fill_halo_periodic(a, Nx, Ny, DC.H, DC.H) for a in q]
    g = S.RectilinearGrid(size=(Nx, Ny), x=(0, DC.DX * Nx), y=(0, DC.DY * Ny))
    m = S.ShallowWaterModel(g, TC.GRAV, TC.FCOR, lorentz_forcing=False, strict=strict, closure=S.ScalarDiffusivity(kappa={"A": DC.DECAY_C}))
    for f, a in zip(m.fields, q):
        f.data.copy_(torch.from_numpy(a))
    for _ in range(DC.DECAY_STEPS):
        m.time_step(DC.DECAY_DT)
    m.synchronize()
    I = g.interior
    Rn = R ** DC.DECAY_STEPS
    dev = np.abs(m.solution["A"].numpy()[I] - Rn * q[3][I]).max() / (Rn * np.abs(q[3][I]).max())
    margin = DC.DECAY_MARGIN + (0.0 if strict else DC.decay_fast_bound(np.finfo(np.float64).eps) / Rn)
    print(f"decay on the device ({'strict' if strict else 'fast'}): relative deviation {dev:.3e}, margin {margin:.3e}")
    assert dev <= margin
    assert not m.solution["u"].numpy()[I].any() and not m.solution["v"].numpy()[I].any() and (m.solution["h"].numpy()[I] == 1.0).all()


# ---- the example --------------------------------------------------------------------------------------------------------------------
def test_example_runs_with_a_closure(tmp_path):
    """examples/run_swmhd.py --viscosity 1e-3 --diffusivity 1e-3 on 64^2 for a few steps: the progress lines, the dump and its fields
    exist and are finite."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "examples", "run_swmhd.py"), "--size", "64", "--stop-time", "0.1", "--every", "5",
           "--dump-every", "0.1", "--out", str(tmp_path), "--viscosity", "1e-3", "--diffusivity", "1e-3"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "ScalarDiffusivity" in r.stdout
    assert len([l for l in r.stdout.splitlines() if l.startswith("Time:")]) >= 2
    z = np.load(os.path.join(str(tmp_path), "fields_0000010.npz"))
    for n in ("u", "v", "h", "A"):
        assert np.isfinite(z[n]).all()
