"""GPU tests of the BetaPlane Coriolis: the kernel through the ABI (swmhd_coriolis_rk3_*, swmhd_ensemble_coriolis_rk3_*) and
ShallowWaterModel / ShallowWaterEnsemble(coriolis=...).

References: tests/coriolis_cases.py (the written formula in numpy, pinned on the CPU by test_coriolis_cases_cpu.py).  Strict results are
compared bitwise; fast results are held to the derived bound |got - ref| <= eps |ref| + 4 eps |a| |f| S against the longdouble value.
The kernel's workgroup covers SWMHD_CORIOLIS_TILE_ROWS = 64 rows (four waves of 16) of a strip of 64 lanes x 16 bytes (128 doubles, 256
floats) where all six parents have the same 16-byte phase and the pitches keep it, and of 64 elements otherwise: the stage matrix runs
both paths, each one column and one row below, at and above its tile."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import coriolis_cases as CC
import tracer_cases as TC
from host_call_cases import Transcript

pytestmark = pytest.mark.gpu
NPDT = {"f64": np.float64, "f32": np.float32}
A_STAGE = 0.013 * 0.37              # a = dt gamma of the stage matrix: no RK3 identity that could hide a wrong operand
DT_STAGE = 0.013
NARR = 6                            # q1, q2 old; q1, q2 new; q1, q2 acc


class Case:
    """The parents of one (shape, halo, pitch, precision): `old`, `new`, `acc` are each ONE array (2, Ny + 2 Hy, sy) -- q1 then q2 --
    so that with sy a multiple of four all parents share their 16-byte phase.  old: random interior; halo NaN (wrapped) or random (read
    as it is); pad columns the sentinel.  new, acc: random interior, the sentinel everywhere else.  fc, ff: distinct for every row."""

    def __init__(self, Nx, Ny, Hx, Hy, sy, t, wrap, seed):
        self.Nx, self.Ny, self.Hx, self.Hy, self.sy, self.t, self.wrap = Nx, Ny, Hx, Hy, sy, t, wrap
        rng = np.random.default_rng([seed, Nx, Ny])
        shp = (2, Ny + 2 * Hy, sy)
        self.I = (slice(None), slice(Hy, Hy + Ny), slice(Hx, Hx + Nx))
        self.old = np.full(shp, CC.SENTINEL, dtype=t)
        self.old[:, :, :Nx + 2 * Hx] = np.nan if wrap else rng.standard_normal((2, Ny + 2 * Hy, Nx + 2 * Hx))
        self.old[self.I] = rng.standard_normal((2, Ny, Nx))
        self.new, self.acc = np.full(shp, CC.SENTINEL, dtype=t), np.full(shp, CC.SENTINEL, dtype=t)
        self.new[self.I] = rng.standard_normal((2, Ny, Nx))
        self.acc[self.I] = rng.standard_normal((2, Ny, Nx))
        self.fc, self.ff = CC.row_values(Ny, t, seed)
        self.table = np.concatenate([self.fc, self.ff])
        P1, P2 = (CC.pad1(self.old[k, :, :Nx + 2 * Hx], Nx, Ny, Hx, Hy, wrap, wrap) for k in range(2))
        self.strict = CC.coriolis_strict(P1, P2, self.fc, self.ff)
        self.exact = CC.coriolis_exact(P1, P2, self.fc, self.ff)


def ptr(tensor, k):
    return tensor.data_ptr() + k * tensor.stride(0) * tensor.element_size()


def check_outputs(c, got, start, given, scalar, rows, strict, tag):
    """got, start: (2, rows, sy) arrays of new or acc after and before the launch; scalar = a or w as the call received it;
    given = False: the call had no acc, nothing may have changed."""
    t, (j0, j1) = c.t, rows
    eps = np.finfo(t).eps
    want = start.copy()
    R = (slice(c.Hy + j0, c.Hy + j1), slice(c.Hx, c.Hx + c.Nx))
    for k in range(2) if given else ():
        if strict:
            want[k][R] = CC.correct(start[k][R], c.strict[k][j0:j1], scalar)
        else:
            E, fS = c.exact[k]
            ref = start[k][R].astype(np.longdouble) + np.longdouble(t(scalar)) * E[j0:j1]
            err = np.abs(got[k][R].astype(np.longdouble) - ref)
            bound = CC.fast_bound(ref, t(scalar), fS[j0:j1], eps)
            assert np.all(err <= bound), (tag, k, float((err / bound).max()))
            want[k][R] = got[k][R]
    # bitwise: the strict values, and everything the launch must not touch (halos, pad columns, rows outside)
    u = np.uint64 if t == np.float64 else np.uint32
    assert np.array_equal(got.view(u), want.view(u)), tag


def launch(L, sfx, c, old_d, new_d, acc_d, tab_d, a, w, rows, flags):
    fn = getattr(L.lib(), f"swmhd_coriolis_rk3_{sfx}")
    acc = (ptr(acc_d, 0), ptr(acc_d, 1)) if w is not None else (None, None)
    rc = fn(ptr(old_d, 0), ptr(old_d, 1), ptr(new_d, 0), ptr(new_d, 1), acc[0], acc[1], tab_d.data_ptr(), c.Nx, c.Ny, c.Hx, c.Hy, c.sy,
            a, w if w is not None else 0.0, rows[0], rows[1], flags, None)
    L.check(rc, "swmhd_coriolis_rk3")
    torch.cuda.synchronize()


@pytest.mark.parametrize("pitch", ["aligned", "odd"])
@pytest.mark.parametrize("wrap", [True, False], ids=["wrapped", "halos"])
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_stage_matrix(swmhd, sfx, strict, wrap, pitch):
    """Shapes x {no acc, w = 1, w = dt / 4} x row ranges {all, [1, Ny - 1), empty}.  wrapped: SWMHD_WRAP_X | _Y with NaN in every halo
    (Hx = Hy = 3); halos: random halos of depth Hx = 2, Hy = 1, read as they are.  aligned: stride_y a multiple of four elements (the
    16-byte path); odd: an odd stride_y (one element per lane).  Every row has its own fc and ff."""
    L = swmhd._lib
    t = NPDT[sfx]
    Hx, Hy = (3, 3) if wrap else (2, 1)
    flags = (L.STRICT if strict else 0) | ((L.WRAP_X | L.WRAP_Y) if wrap else 0)
    a = float(t(A_STAGE))
    for Nx, Ny in CC.stage_shapes(np.dtype(t).itemsize, pitch == "aligned"):
        sy = (Nx + 2 * Hx + 1 + 3) // 4 * 4 if pitch == "aligned" else (Nx + 2 * Hx + 5) | 1
        c = Case(Nx, Ny, Hx, Hy, sy, t, wrap, 5)
        old_d, tab_d = torch.from_numpy(c.old).cuda(), torch.from_numpy(c.table).cuda()
        for w in (None, 1.0, float(t(DT_STAGE / 4))):
            for rows in CC.row_ranges(Ny):
                new_d, acc_d = torch.from_numpy(c.new).cuda(), torch.from_numpy(c.acc).cuda()
                launch(L, sfx, c, old_d, new_d, acc_d, tab_d, a, w, rows, flags)
                tag = (Nx, Ny, w, rows)
                check_outputs(c, new_d.cpu().numpy(), c.new, True, a, rows, strict, ("new",) + tag)
                check_outputs(c, acc_d.cpu().numpy(), c.acc, w is not None, w, rows, strict, ("acc",) + tag)
        assert np.array_equal(old_d.cpu().numpy().view(np.uint8), c.old.view(np.uint8))      # old is only read
        assert np.array_equal(tab_d.cpu().numpy().view(np.uint8), c.table.view(np.uint8))


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_parents_of_different_phase_take_the_element_path(swmhd, sfx):
    """q1_new one element further into its allocation than the other parents: the phases differ, the call takes one element per lane
    whatever the pitch, and the results are bitwise those of the call with equal phases (strict and fast)."""
    L = swmhd._lib
    t = NPDT[sfx]
    Nx, Ny, Hx, Hy, sy = 129, 17, 3, 3, 136
    c = Case(Nx, Ny, Hx, Hy, sy, t, True, 9)
    fn = getattr(L.lib(), f"swmhd_coriolis_rk3_{sfx}")
    a, w = float(t(A_STAGE)), 1.0
    old_d, tab_d = torch.from_numpy(c.old).cuda(), torch.from_numpy(c.table).cuda()
    size = c.new[0].size
    for strict in (True, False):
        flags = (L.STRICT if strict else 0) | L.WRAP_X | L.WRAP_Y
        new_d, acc_d = torch.from_numpy(c.new).cuda(), torch.from_numpy(c.acc).cuda()
        launch(L, sfx, c, old_d, new_d, acc_d, tab_d, a, w, (0, Ny), flags)
        flat = torch.full((size + 1,), CC.SENTINEL, dtype=new_d.dtype, device="cuda")
        flat[1:].copy_(torch.from_numpy(c.new[0]).reshape(-1))
        new2_d, acc2_d = torch.from_numpy(c.new).cuda(), torch.from_numpy(c.acc).cuda()
        rc = fn(ptr(old_d, 0), ptr(old_d, 1), flat.data_ptr() + flat.element_size(), ptr(new2_d, 1), ptr(acc2_d, 0), ptr(acc2_d, 1),
                tab_d.data_ptr(), Nx, Ny, Hx, Hy, sy, a, w, 0, Ny, flags, None)
        L.check(rc, "swmhd_coriolis_rk3")
        torch.cuda.synchronize()
        assert flat[0].item() == CC.SENTINEL
        assert torch.equal(flat[1:].reshape(new_d[0].shape), new_d[0]) and torch.equal(new2_d[1], new_d[1]) and torch.equal(acc2_d, acc_d)
        if strict:
            check_outputs(c, new_d.cpu().numpy(), c.new, True, a, (0, Ny), True, "new")
            check_outputs(c, acc_d.cpu().numpy(), c.acc, True, w, (0, Ny), True, "acc")


# ----------------------------------------------------------------------------------------------------------------------------------
# ensembles through the ABI
# ----------------------------------------------------------------------------------------------------------------------------------
# (Nx by precision, Ny, stride_y by precision, elements added to stride_m): the launch of three members has 3 x strips x row blocks
# workgroups
ENS_GEOMETRIES = {
    # one strip, one row block; the 16-byte path (stride_y and stride_m multiples of four): 3 workgroups
    "one-tile": dict(Nx={"f64": 65, "f32": 65}, Ny=17, sy={"f64": 72, "f32": 72}, gap=8, vec=True),
    # the 16-byte path with two strips (128 doubles | 256 floats each) and two row blocks of 64 rows: 12 workgroups, no multiple of 8
    "vec-2x2": dict(Nx={"f64": 129, "f32": 257}, Ny=65, sy={"f64": 136, "f32": 264}, gap=8, vec=True),
    # an odd stride_m: one element per lane, two strips of 64 columns, two row blocks: 12 workgroups
    "elem-2x2": dict(Nx={"f64": 65, "f32": 65}, Ny=65, sy={"f64": 72, "f32": 72}, gap=9, vec=False),
}


@pytest.mark.parametrize("members", [1, 3])
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_ensemble_members_are_single_grid_calls(swmhd, sfx, members):
    """stride_m pitched with the sentinel in the gap; a table of rows per member; dt: one for all (params NULL; w = 1), and per member
    from the (g, f, dt) table, with w = 1 (the stored tendency) and with SWMHD_RK3_ANCHOR (w = 1/4 of each member's dt).  Geometries
    (ENS_GEOMETRIES): 65 x 17, one tile per member; two strips x two row blocks on the 16-byte path and on the one-element path (an
    odd stride_m), where the kernel's decode of blockIdx into (member, tile) has more than one tile to tell apart.  Rows: all, and
    [1, Ny - 1), where rows 0 and Ny - 1 of every member stay bitwise what they were.  Strict: member m is bitwise the single-grid
    call with its table, a = dt_m gamma formed in the element type as the kernel forms it, and its w.  Fast: member m is held to the
    derived bound of the single-grid stage matrix (check_outputs, against the longdouble value with fc, ff as rounded to the precision
    of the call) -- not bitwise to the fast single-grid call: two instantiations need not contract alike.  Then (strict) a member
    full of NaN stays NaN and leaves the others bitwise what they were."""
    L = swmhd._lib
    t = NPDT[sfx]
    for name, geo in ENS_GEOMETRIES.items():
        for strict in (True, False):
            _ensemble_abi_case(L, sfx, t, members, name, geo, strict)


def _ensemble_abi_case(L, sfx, t, members, name, geo, strict):
    Nx, Ny, Hx, Hy = geo["Nx"][sfx], geo["Ny"], 3, 3
    sy = geo["sy"][sfx]
    size = (Ny + 2 * Hy) * sy
    stride_m = size + geo["gap"]
    V = 16 // np.dtype(t).itemsize
    assert (sy % V == 0 and stride_m % V == 0) == geo["vec"]
    cases = [Case(Nx, Ny, Hx, Hy, sy, t, True, 20 + m) for m in range(members)]
    tables = np.stack([c.table for c in cases])
    dts = np.array([0.013 * (1 + 0.5 * m) for m in range(members)], dtype=t)
    gamma = t(0.37)
    params = np.stack([np.full(members, 9.81), np.zeros(members), dts], axis=1).astype(t)
    ens = getattr(L.lib(), f"swmhd_ensemble_coriolis_rk3_{sfx}")
    flags = (L.STRICT if strict else 0) | L.WRAP_X | L.WRAP_Y

    def pack(arrs):        # (2, members * stride_m): field k of member m at [k, m * stride_m:]
        out = np.full((2, members * stride_m), CC.SENTINEL, dtype=t)
        for m, a in enumerate(arrs):
            out[:, m * stride_m:m * stride_m + size] = a.reshape(2, size)
        return torch.from_numpy(out).cuda()

    def run_ensemble(olds, par, w, anchor, rows):
        old_d, new_d, acc_d = pack(olds), pack([c.new for c in cases]), pack([c.acc for c in cases])
        tab_d, par_d = torch.from_numpy(tables).cuda(), torch.from_numpy(params).cuda()
        rc = ens(ptr(old_d, 0), ptr(old_d, 1), ptr(new_d, 0), ptr(new_d, 1), ptr(acc_d, 0), ptr(acc_d, 1), tab_d.data_ptr(), members,
                 stride_m, Nx, Ny, Hx, Hy, sy, par_d.data_ptr() if par else None, float(gamma) if par else float(dts[0] * gamma), w,
                 rows[0], rows[1], flags | (L.RK3_ANCHOR if anchor else 0), None)
        L.check(rc, "swmhd_ensemble_coriolis_rk3")
        torch.cuda.synchronize()
        return new_d.cpu().numpy(), acc_d.cpu().numpy()

    def run_single(m, a, w, rows):
        c = cases[m]
        old_d, new_d, acc_d = torch.from_numpy(c.old).cuda(), torch.from_numpy(c.new).cuda(), torch.from_numpy(c.acc).cuda()
        launch(L, sfx, c, old_d, new_d, acc_d, torch.from_numpy(c.table).cuda(), a, w, rows, flags)
        return new_d.cpu().numpy().reshape(2, size), acc_d.cpu().numpy().reshape(2, size)

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
                assert np.all(got_new[:, lo + size:lo + stride_m] == CC.SENTINEL) and np.all(got_acc[:, lo + size:lo + stride_m] == CC.SENTINEL), tag
                if strict:
                    one_new, one_acc = run_single(m, a_m, w_m, rows)
                    assert np.array_equal(mine[0].view(u), one_new.view(u)), tag
                    assert np.array_equal(mine[1].view(u), one_acc.view(u)), tag
                else:
                    for got, start, scalar, what in ((mine[0], cases[m].new, a_m, "new"), (mine[1], cases[m].acc, w_m, "acc")):
                        check_outputs(cases[m], got.reshape(2, Ny + 2 * Hy, sy), start, True, scalar, rows, False, (what,) + tag)
                if rows[0] > 0:         # rows 0 and Ny - 1 of every member: bitwise what they were
                    for got, start in ((mine[0], cases[m].new), (mine[1], cases[m].acc)):
                        assert np.array_equal(got.reshape(2, Ny + 2 * Hy, sy)[:, outer].view(u), start[:, outer].view(u)), tag
    if members > 1 and strict:
        clean = run_ensemble([c.old for c in cases], True, 1.0, False, (0, Ny))
        olds = [c.old for c in cases]
        olds[1] = np.full_like(olds[1], np.nan)
        bad = run_ensemble(olds, True, 1.0, False, (0, Ny))
        for x, y in zip(clean, bad):
            for m in (0, 2):
                assert np.array_equal(x[:, m * stride_m:(m + 1) * stride_m].view(u), y[:, m * stride_m:(m + 1) * stride_m].view(u))
        I1 = bad[0][:, stride_m:stride_m + size].reshape(2, Ny + 2 * Hy, sy)[:, Hy:Hy + Ny, Hx:Hx + Nx]
        assert np.isnan(I1).all()


# ----------------------------------------------------------------------------------------------------------------------------------
# whole runs
# ----------------------------------------------------------------------------------------------------------------------------------
DT, STEPS = 2e-3, 10
F0, BETA, Y0 = 1.0, 0.9, 0.35       # f = F0 + BETA y on a grid whose y starts at Y0
NU, ETA = 3e-3, 5e-3
RUN_GRIDS = [(48, 40), (64, 64)]
TOPOS = [(TC.P, TC.P), (TC.P, TC.B)]
_reference = {}


def _grid(S, Nx, Ny, topo):
    names = {TC.P: "Periodic", TC.B: "Bounded"}
    return S.RectilinearGrid(size=(Nx, Ny), x=(0, TC.DX * Nx), y=(Y0, Y0 + TC.DY * Ny), topology=(names[topo[0]], names[topo[1]], "Flat"))


def _bcs(S, topo):
    if topo[1] != TC.B:
        return None
    return {"A": S.FieldBoundaryConditions(north=S.GradientBoundaryCondition(-0.05), south=S.GradientBoundaryCondition(-0.05))}


def _start(S, O, Nx, Ny, form, topo):
    g = _grid(S, Nx, Ny, topo)
    return TC.fill_state(O, TC.state(Nx, Ny, form, 11, rough=False), Nx, Ny, topo, TC.grad_A(topo), g.dx, g.dy)


def _model(S, O, Nx, Ny, form, topo=(TC.P, TC.P), strict=True, coriolis="beta", closure=None, **kw):
    g = _grid(S, Nx, Ny, topo)
    if coriolis == "beta":
        kw["coriolis"] = S.BetaPlane(F0, BETA)
    elif coriolis != "absent":
        kw["coriolis"] = coriolis
    m = S.ShallowWaterModel(g, TC.GRAV, formulation=TC.FORM_NAME[form], strict=strict, boundary_conditions=_bcs(S, topo), closure=closure, **kw)
    for f, a in zip(m.fields, _start(S, O, Nx, Ny, form, topo)):
        f.data.copy_(torch.from_numpy(a))
    return m


def _ref(S, O, Nx, Ny, form, lor, topo, coef=None):
    """The reference stepper after STEPS steps, computed once per case and left unchanged."""
    key = (Nx, Ny, form, topo, coef)
    if key not in _reference:
        g = _grid(S, Nx, Ny, topo)
        fc, ff = S.BetaPlane(F0, BETA).rows(g)
        r = CC.RefModel(O, _start(S, O, Nx, Ny, form, topo), fc, ff, Nx, Ny, form, lor, "classic", topo, TC.grad_A(topo), g.dx, g.dy, coef)
        for n in range(STEPS):
            r.step(DT, n)
        _reference[key] = r
    return _reference[key]


@pytest.mark.parametrize("how", ["eager", "graph"])
@pytest.mark.parametrize("topo", TOPOS, ids=["periodic", "channel"])
@pytest.mark.parametrize("form,lor", TC.FORMS)
@pytest.mark.parametrize("Nx,Ny", RUN_GRIDS)
def test_strict_runs_are_the_reference(swmhd, oracle, Nx, Ny, form, lor, topo, how):
    """Strict model under BetaPlane(F0, BETA) on a grid whose y starts at Y0, 10 steps: every field bitwise the reference stepper, halos
    included -- stepped eagerly, and through capture_graph with time_steps(5) twice, so that the second call starts on swapped roles
    (one eager step, then replays)."""
    S, O = swmhd, oracle
    m = _model(S, O, Nx, Ny, form, topo)
    assert m.f == 0.0 and tuple(m.coriolis_rows.shape) == (2, Ny)
    ref = _ref(S, O, Nx, Ny, form, lor, topo)
    if how == "eager":
        for _ in range(STEPS):
            m.time_step(DT)
    else:
        m.capture_graph(DT)
        m.time_steps(5, DT)
        m.time_steps(5, DT)
    m.synchronize()
    assert m.iteration == STEPS
    for f, a in zip(m.fields, ref.q):
        assert np.array_equal(f.numpy(), a)


@pytest.mark.parametrize("form,lor", TC.FORMS)
@pytest.mark.parametrize("Nx,Ny", RUN_GRIDS)
def test_fast_runs_follow_the_strict_run(swmhd, oracle, Nx, Ny, form, lor):
    """Fast model (anchor form), same periodic run: within the project's fast tolerance of whole runs, 1e-12 max |field|, of the strict
    result; and beta has moved u by far more than that against the f-plane of the same f0."""
    S, O = swmhd, oracle
    m = _model(S, O, Nx, Ny, form, strict=False)
    plain = _model(S, O, Nx, Ny, form, strict=False, coriolis=S.FPlane(F0))
    m.time_steps(STEPS, DT)
    plain.time_steps(STEPS, DT)
    m.synchronize(); plain.synchronize()
    ref = _ref(S, O, Nx, Ny, form, lor, (TC.P, TC.P))
    for name, f, a in zip(m.names, m.fields, ref.q):
        err = np.abs(f.numpy() - a).max() / np.abs(a).max()
        print(f"fast vs strict {Nx}x{Ny} form {form} {name}: {err:.3e}")
        assert err <= 1e-12
    assert np.abs(plain.fields[0].numpy() - ref.q[0]).max() > 1e-6 * np.abs(ref.q[0]).max()


def test_with_a_closure_the_launch_order_is_the_reference(swmhd, oracle):
    """closure= and coriolis= together (periodic, vector invariant, strict): bitwise the reference that corrects with the Coriolis term
    first and the closure's second, and not the one in the other order."""
    S, O = swmhd, oracle
    Nx, Ny = 48, 40
    m = _model(S, O, Nx, Ny, 1, closure=S.ScalarDiffusivity(nu=NU, kappa={"A": ETA}))
    for _ in range(STEPS):
        m.time_step(DT)
    m.synchronize()
    ref = _ref(S, O, Nx, Ny, 1, 1, (TC.P, TC.P), (NU, NU, 0.0, ETA))
    for f, a in zip(m.fields, ref.q):
        assert np.array_equal(f.numpy(), a)
    assert not np.array_equal(ref.q[0], _ref(S, O, Nx, Ny, 1, 1, (TC.P, TC.P)).q[0])


@pytest.mark.parametrize("topo", TOPOS, ids=["periodic", "channel"])
def test_the_launch_touches_the_two_momentum_fields_only(swmhd, oracle, topo):
    """One stage with the launch and one without it: h, A and their stored tendencies are bit-identical buffers, halos included, and
    the two momentum-like fields differ."""
    S, O = swmhd, oracle
    from swmhd_amd.shared import finish_stage
    out = []
    for skip in (False, True):
        m = _model(S, O, 48, 40, 1, topo)
        if skip:
            m._corrections = [c for c in m._corrections if c.stem != "coriolis"]
        m._stage_fused(DT, 0)
        finish_stage(m, DT, 0)
        torch.cuda.synchronize()
        out.append([f.data.clone() for f in m._raw_fields + m.Gm])
    with_, without = out
    for k in (2, 3, 6, 7):
        assert torch.equal(with_[k].view(torch.int64), without[k].view(torch.int64)), k
    for k in (0, 1, 4, 5):
        assert not torch.equal(with_[k], without[k]), k


def test_betaplane_adds_one_launch_per_stage_and_fplane_none(swmhd, oracle):
    S, O = swmhd, oracle
    logs = {}
    for key, coriolis, kw in (("absent", "absent", dict(coriolis_f=F0)), ("none", None, dict(coriolis_f=F0)), ("fplane", S.FPlane(F0), {}),
                              ("beta", "beta", {})):
        for strict in (True, False):
            m = _model(S, O, 48, 40, 1, strict=strict, coriolis=coriolis, **kw)
            tr = Transcript()
            tr.watch(m)
            tr.do("time_step", m.time_step, DT)
            tr.do("time_steps", m.time_steps, 3, DT)
            m.synchronize()
            logs[key, strict] = (tr.blocks, [f.numpy() for f in m.fields])
    for strict in (True, False):
        base = logs["absent", strict]
        for key in ("none", "fplane"):       # argument by argument the calls of a model built without coriolis=, and its state
            assert logs[key, strict][0] == base[0]
            assert all(np.array_equal(x, y) for x, y in zip(logs[key, strict][1], base[1]))
        assert not any("coriolis" in c[0] for _, calls in base[0] for c in calls)
        names = [c[0] for _, calls in logs["beta", strict][0] for c in calls]
        assert names == ["swmhd_tendencies_rk3_f64", "swmhd_coriolis_rk3_f64"] * 12, names
        calls = [c for _, cs in logs["beta", strict][0] for c in cs if c[0] == "swmhd_coriolis_rk3_f64"]
        # an operand in storing stages only: stages 0, 1 (classic) or stage 0 (anchor)
        assert [c[5] != "null" for c in calls] == ([True, True, False] if strict else [True, False, False]) * 4
        stages = [c for _, cs in logs["beta", strict][0] for c in cs if c[0] == "swmhd_tendencies_rk3_f64"]
        assert all(c[13] == float(0.0).hex() for c in stages)       # the stage kernels run with f = 0


def test_potential_vorticity_is_refused_and_vorticity_is_not(swmhd, oracle):
    S, O = swmhd, oracle
    m = _model(S, O, 48, 40, 1)
    with pytest.raises(S._lib.SwmhdError, match="SWMHD_ENOTSUP"):
        m.derived_fields(("potential_vorticity",))
    with pytest.raises(S._lib.SwmhdError, match="SWMHD_ENOTSUP"):
        S.FieldTimeSeries(m, names=("u", "potential_vorticity"), capacity=2)
    z = m.derived_fields(("vorticity",))
    torch.cuda.synchronize()
    assert torch.isfinite(z).all()
    p = _model(S, O, 48, 40, 1, coriolis=S.FPlane(F0)).derived_fields(("potential_vorticity",))
    torch.cuda.synchronize()
    assert torch.isfinite(p).all()


# ---- ensembles ----------------------------------------------------------------------------------------------------------------------
F0S, BETAS = [1.0, 0.5, 2.0], [0.9, 0.0, -1.5]


def _ensemble(S, O, strict, **kw):
    Nx, Ny, B = 48, 40, 3
    g = _grid(S, Nx, Ny, (TC.P, TC.P))
    e = S.ShallowWaterEnsemble(g, B, TC.GRAV, strict=strict, coriolis=S.BetaPlane(F0S, BETAS), member_stride=(Ny + 6) * (Nx + 6) + 10, **kw)
    q = _start(S, O, Nx, Ny, 1, (TC.P, TC.P))
    for t_, a in zip(e._state, q):
        for m in range(B):
            t_[m].copy_(torch.from_numpy(a * (1.0 + 0.1 * m)))
    return e


@pytest.mark.parametrize("per_member_dt", [False, True], ids=["dt", "dts"])
def test_ensemble_members_are_models(swmhd, oracle, per_member_dt):
    """Strict ensemble of three members with per-member f0 and beta (a zero among them) and a scalar or per-member dt, 4 steps: member m
    is bitwise ShallowWaterModel(coriolis=that member's) stepped alone, and member(1) taken after 2 steps and stepped 2 more alone is
    bitwise member 1 of the ensemble.  The fast ensemble (anchor form; with per-member dt the kernel forms dt_m / 4) stays within 1e-12."""
    S, O = swmhd, oracle
    dts = [DT, 1.5 * DT, 0.5 * DT] if per_member_dt else None
    dt = dts if per_member_dt else DT
    e = _ensemble(S, O, True)
    assert tuple(e.coriolis_rows.shape) == (3, 2, 40) and not np.any(e.f_values)
    start = [[t_[m].clone() for t_ in e._state] for m in range(3)]
    e.time_steps(2, dt)
    one = e.member(1)
    assert (one.coriolis.f0, one.coriolis.beta) == (0.5, 0.0) and one.f == 0.0
    e.time_steps(2, dt)
    one.time_steps(2, dts[1] if per_member_dt else DT)
    e.synchronize(); one.synchronize()
    for f, t_ in zip(one.fields, e.fields):
        assert torch.equal(f.data, t_[1])
    for m in range(3):
        alone = e._member_model(m)
        assert (alone.coriolis.f0, alone.coriolis.beta) == (F0S[m], BETAS[m])
        for f, a in zip(alone._raw_fields, start[m]):
            f.data.copy_(a)
        for _ in range(4):
            alone.time_step(dts[m] if per_member_dt else DT)
        alone.synchronize()
        for f, t_ in zip(alone.fields, e.fields):
            assert torch.equal(f.data, t_[m]), m
    fast = _ensemble(S, O, False)
    fast.time_steps(4, dt)
    fast.synchronize()
    for a, b in zip(fast.fields, e.fields):
        assert ((a - b).abs().amax() <= 1e-12 * b.abs().amax()).item()


def test_ensemble_graph_replay_and_fplane_calls(swmhd, oracle):
    S, O = swmhd, oracle
    e = _ensemble(S, O, False)
    g = _ensemble(S, O, False)
    e.time_steps(5, DT)
    g.capture_graph(DT)
    g.time_steps(5, DT)
    e.synchronize(); g.synchronize()
    for a, b in zip(e.fields, g.fields):
        assert torch.equal(a, b)
    grid = e.grid
    logs = []
    for kw in (dict(coriolis_f=[0.5, 0.7]), dict(coriolis=S.FPlane([0.5, 0.7]))):
        p = S.ShallowWaterEnsemble(grid, 2, **kw)
        tr = Transcript()
        tr.watch(p)
        tr.do("steps", p.time_steps, 2, DT)
        p.synchronize()
        logs.append([[c[0]] + c[5:] for c in tr.blocks[0][1]])      # (without the buffers and the table: other allocations)
    assert logs[0] == logs[1] and [c[0] for c in logs[0]] == ["swmhd_ensemble_step_rk3_params_f64"]


# ---- the example --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [(), ("--channel", "--gradients", "-0.05", "--coriolis", "2")], ids=["periodic", "channel"])
def test_example_runs_with_beta(tmp_path, extra):
    """examples/run_swmhd.py --beta 0.5 on 64^2 for a few steps, periodic and as one Bounded channel model: the progress lines, the dump
    and its fields exist and are finite."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "examples", "run_swmhd.py"), "--size", "64", "--stop-time", "0.1", "--every", "5",
           "--dump-every", "0.1", "--out", str(tmp_path), "--beta", "0.5", *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "BetaPlane" in r.stdout
    assert len([l for l in r.stdout.splitlines() if l.startswith("Time:")]) >= 2
    z = np.load(os.path.join(str(tmp_path), "fields_0000010.npz"))
    for n in ("u", "v", "h", "A"):
        assert np.isfinite(z[n]).all()
