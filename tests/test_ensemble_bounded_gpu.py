"""GPU tests of Bounded ensembles (BoundedShallowWaterEnsemble, swmhd_ensemble_fill_halo_*, swmhd_ensemble_step_rk3_bc_*): every
member, with its own boundary conditions, computes what the same grid computes alone -- the boundary-condition fill bitwise against the
oracle (f64) and the single-grid fill (f32), strict members bitwise against the oracle's Bounded time_step and a strict
ShallowWaterModel, fast members within the fast tolerance of a fast ShallowWaterModel (bitwise equality is not promised: the tendencies of the ensemble
instantiation of the wall kernel are reassociated on their own) -- member by member independent,
graph-replayable, handed over to a ShallowWaterModel mid-run, with per-member diagnostics; and the example runs the reference's
commented channel experiment as a sweep over the gradient of A."""
import csv
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_bounded_oracle import state, fill_all, LOC, G, F, P, B

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORM = {0: "Conservative", 1: "VectorInvariant"}
TOPO = {P: "Periodic", B: "Bounded"}
DT = 2e-3
# per-member GradientBoundaryCondition values of A (west, east, south, north; None = default) on a (Periodic, Bounded) grid
GRADS_PB = [(None, None, -0.05, -0.05), (None, None, 0.125, -0.02), None, (None, None, None, 0.3)]


def grid_for(S, Nx, Ny, topo, dx=0.1, dy=0.12):
    return S.RectilinearGrid(size=(Nx, Ny), x=(0, dx * Nx), y=(0, dy * Ny), topology=(TOPO[topo[0]], TOPO[topo[1]], "Flat"))


def bcs_for(S, grad):
    if grad is None:
        return None
    sides = {k: S.GradientBoundaryCondition(v) for k, v in zip(("west", "east", "south", "north"), grad) if v is not None}
    return {"A": S.FieldBoundaryConditions(**sides)}


def member_states(O, Nx, Ny, topo, form, grads, seed, dx, dy, dtype=np.float64):
    """One filled state per member (the oracle's fill with that member's gradients of A)."""
    return [[np.ascontiguousarray(a.astype(dtype)) for a in fill_all(O, state(Nx, Ny, seed + 13 * m, form), Nx, Ny, topo, gradA=gr, dx=dx, dy=dy)]
            for m, gr in enumerate(grads)]


def make_ensemble(S, g, form, states, grads, strict, dtype=torch.float64, **kw):
    e = S.BoundedShallowWaterEnsemble(g, len(states), G, F, formulation=FORM[form], dtype=dtype, strict=strict,
                                      boundary_conditions=[bcs_for(S, gr) for gr in grads], **kw)
    e.set(**{n: np.stack([st[k] for st in states]) for k, n in enumerate(e.names)})
    return e


def make_model(S, g, form, q, grad, strict, dtype=torch.float64):
    m = S.ShallowWaterModel(g, G, F, formulation=FORM[form], dtype=dtype, strict=strict, boundary_conditions=bcs_for(S, grad))
    for f, a in zip(m._raw_fields, q):
        f.data.copy_(torch.from_numpy(a))
    m.update_state()
    return m


def member_arrays(e, m):
    return [t[m].cpu().numpy() for t in e.fields]


def bitwise(a, b):
    return np.array_equal(a, b, equal_nan=True)


def close(want, got, dtype):
    """The fast tolerance between two fast runs of the same state: 1e-12 (fp64) / 1e-5 (fp32) of max(max|want|, 1)."""
    tol = 1e-12 if dtype in (torch.float64, np.float64) else 1e-5
    return np.abs(want.astype(np.float64) - got.astype(np.float64)).max() <= tol * max(np.abs(want).max(), 1.0)


@pytest.mark.parametrize("topo", [(P, B), (B, P), (B, B)])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_fill_halo_per_member(swmhd, oracle, topo, dtype):
    """swmhd_ensemble_fill_halo on pitched members with a per-member table: f64 == the oracle's fill, f32 == swmhd_fill_halo_f32 on the
    member alone, halos included; the gaps between members are not touched."""
    S, O = swmhd, oracle
    L = S._lib.lib()
    Nx, Ny, Bm = 37, 21, 3
    g = grid_for(S, Nx, Ny, topo)
    Py, Px = g.parent_shape
    sm = Py * Px + 29
    sfx = "f64" if dtype == np.float64 else "f32"
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    rng = np.random.default_rng(5)
    # gradients on the Bounded sides only: A differs per member, h gets one on member 1, member 2 keeps the defaults
    table = np.full((Bm, 4, 4), np.nan)
    for m in range(2):
        for side in range(4):
            if topo[side // 2] == B:
                table[m, 3, side] = rng.uniform(-0.2, 0.2)
    if topo[1] == B:
        table[1, 2, 3] = 0.07
    base = [[rng.standard_normal((Py, Px)).astype(dtype) for _ in range(4)] for _ in range(Bm)]
    flat = [torch.full((Bm * sm,), 777.0, dtype=tdt, device="cuda") for _ in range(4)]
    for k in range(4):
        for m in range(Bm):
            flat[k][m * sm:m * sm + Py * Px].copy_(torch.from_numpy(base[m][k].ravel()))
    gt = torch.from_numpy(table).to(tdt).cuda()
    ptrs = S._lib.ptr_array([t.data_ptr() for t in flat])
    rc = getattr(L, f"swmhd_ensemble_fill_halo_{sfx}")(ptrs, 4, Bm, sm, Nx, Ny, 3, 3, Px, topo[0], topo[1], 0b0001, 0b0010,
                                                      gt.data_ptr(), g.dx, g.dy, None)
    assert rc == 0
    torch.cuda.synchronize()
    for k in range(4):
        got = flat[k].cpu().numpy()
        for m in range(Bm):
            mine = got[m * sm:m * sm + Py * Px].reshape(Py, Px)
            assert bool((got[m * sm + Py * Px:(m + 1) * sm] == 777.0).all()), "a gap between members was written"
            if dtype == np.float64:
                grad = [None if np.isnan(v) else float(v) for v in table[m, k]]
                want = O.fill_halo(base[m][k].copy(), Nx, Ny, 3, 3, topo=topo, face=LOC[k], grad=grad, dx=g.dx, dy=g.dy)
            else:
                one = [torch.from_numpy(base[m][j].copy()).cuda() for j in range(4)]
                vals = (ctypes.c_float * 16)(*[float(v) for v in table[m].ravel()])
                assert L.swmhd_fill_halo_f32(S._lib.ptr_array([t.data_ptr() for t in one]), 4, Nx, Ny, 3, 3, Px, topo[0], topo[1],
                                             0b0001, 0b0010, vals, g.dx, g.dy, None) == 0
                want = one[k].cpu().numpy()
            assert bitwise(want, mine), (m, k, topo)


@pytest.mark.parametrize("form", [1, 0])
@pytest.mark.parametrize("topo,grads", [((P, B), GRADS_PB[:3]), ((B, B), [None] * 3), ((B, P), [None] * 3)])
def test_strict_members_equal_oracle(swmhd, oracle, form, topo, grads):
    """3 RK3 steps at 48 x 40: every strict member == the oracle's Bounded time_step with that member's gradients, halos included."""
    S, O = swmhd, oracle
    Nx, Ny = 48, 40
    g = grid_for(S, Nx, Ny, topo, 0.1, 0.1)
    states = member_states(O, Nx, Ny, topo, form, grads, 9, g.dx, g.dy)
    e = make_ensemble(S, g, form, states, grads, strict=True)
    e.time_steps(3, DT)
    e.synchronize()
    for m, (q, gr) in enumerate(zip(states, grads)):
        qo = [a.copy() for a in q]
        for _ in range(3):
            O.time_step(*qo, Nx, Ny, 3, 3, g.dx, g.dy, DT, form, 2 - form, G, F, nthreads=8, topo=topo, gradA=gr)
        model = make_model(S, g, form, q, gr, strict=True)
        model.time_steps(3, DT)
        model.synchronize()
        for w, s, a in zip(qo, model.fields, member_arrays(e, m)):
            assert bitwise(w, a), f"member {m}: strict Bounded ensemble != oracle by {np.abs(w - a).max()}"
            assert bitwise(s.numpy(), a), f"member {m}: strict Bounded ensemble != strict model"


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("form", [1, 0])
@pytest.mark.parametrize("shape", [(48, 40), (100, 37)])
def test_fast_members_match_single_model(swmhd, oracle, form, shape, dtype):
    """Fast members below the marching threshold (the single Bounded model's 64 x 8 wall tiles): within the fast tolerance of a fast
    ShallowWaterModel with that member's boundary conditions; f64 also within 1e-12 of the oracle."""
    S, O = swmhd, oracle
    Nx, Ny = shape
    topo = (P, B)
    npt = np.float64 if dtype == torch.float64 else np.float32
    g = grid_for(S, Nx, Ny, topo)
    states = member_states(O, Nx, Ny, topo, form, GRADS_PB, 23, g.dx, g.dy, npt)
    e = make_ensemble(S, g, form, states, GRADS_PB, strict=False, dtype=dtype)
    e.time_steps(3, DT)
    e.synchronize()
    for m, (q, gr) in enumerate(zip(states, GRADS_PB)):
        model = make_model(S, g, form, q, gr, strict=False, dtype=dtype)
        model.time_steps(3, DT)
        model.synchronize()
        got = member_arrays(e, m)
        for s, a in zip(model.fields, got):
            assert close(s.numpy(), a, dtype), f"member {m}: fast Bounded ensemble off the fast model by {np.abs(s.numpy() - a).max()}"
        if dtype == torch.float64:
            qo = [a.copy() for a in q]
            for _ in range(3):
                O.time_step(*qo, Nx, Ny, 3, 3, g.dx, g.dy, DT, form, 2 - form, G, F, nthreads=8, topo=topo, gradA=gr)
            for w, a in zip(qo, got):
                assert np.abs(w - a).max() <= 1e-12 * max(np.abs(w).max(), 1.0)


@pytest.mark.parametrize("form", [1, 0])
def test_large_members_within_tolerance_of_single_model(swmhd, oracle, form):
    """640 x 560 members (above the marching threshold): the ensemble runs the wall kernel on every tile, the single model the hybrid
    marching + wall-frame launch; within 1e-12 of each other."""
    S, O = swmhd, oracle
    Nx, Ny = 640, 560
    topo = (P, B)
    grads = GRADS_PB[:2]
    g = grid_for(S, Nx, Ny, topo)
    states = member_states(O, Nx, Ny, topo, form, grads, 3, g.dx, g.dy)
    e = make_ensemble(S, g, form, states, grads, strict=False)
    e.time_steps(3, DT)
    e.synchronize()
    for m, (q, gr) in enumerate(zip(states, grads)):
        model = make_model(S, g, form, q, gr, strict=False)
        model.time_steps(3, DT)
        model.synchronize()
        for s, a in zip(model.fields, member_arrays(e, m)):
            s = s.numpy()
            assert np.abs(s - a).max() <= 1e-12 * max(np.abs(s).max(), 1.0), f"member {m} off by {np.abs(s - a).max()}"


@pytest.mark.parametrize("form", [1, 0])
def test_a_nan_member_leaves_the_others_alone(swmhd, oracle, form):
    S = swmhd
    Nx, Ny, topo = 64, 40, (P, B)
    g = grid_for(S, Nx, Ny, topo)
    states = member_states(oracle, Nx, Ny, topo, form, GRADS_PB, 5, g.dx, g.dy)
    clean = make_ensemble(S, g, form, states, GRADS_PB, strict=False)
    bad = [[a.copy() for a in st] for st in states]
    bad[2][2][10, 20] = np.nan
    dirty = make_ensemble(S, g, form, bad, GRADS_PB, strict=False)
    for e in (clean, dirty):
        e.time_steps(5, DT)
        e.synchronize()
    assert np.isnan(member_arrays(dirty, 2)[2]).any()
    for m in (0, 1, 3):
        for a, b in zip(member_arrays(clean, m), member_arrays(dirty, m)):
            assert bitwise(a, b), f"member {m} changed by a NaN in member 2"


@pytest.mark.parametrize("form", [1, 0])
def test_graph_replay_equals_eager(swmhd, oracle, form):
    S = swmhd
    Nx, Ny, topo = 64, 64, (P, B)
    g = grid_for(S, Nx, Ny, topo)
    grads = GRADS_PB[:3]
    states = member_states(oracle, Nx, Ny, topo, form, grads, 9, g.dx, g.dy)
    eager = make_ensemble(S, g, form, states, grads, strict=False)
    graph = make_ensemble(S, g, form, states, grads, strict=False)
    graph.capture_graph(DT)
    for n in (7, 2, 5):                     # odd counts leave the roles swapped; the next call restores them
        graph.time_steps(n, DT)
        for _ in range(n):
            eager.time_step(DT)
        graph.synchronize(); eager.synchronize()
        assert graph.iteration == eager.iteration and abs(graph.clock_time - eager.clock_time) < 1e-12
        for m in range(3):
            for a, b in zip(member_arrays(graph, m), member_arrays(eager, m)):
                assert bitwise(a, b)


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_member_handover_continues(swmhd, oracle, dtype, strict):
    """4 ensemble steps == 2 ensemble steps, member(m), 2 steps of that ShallowWaterModel (its boundary conditions included): bitwise in
    strict builds, within the fast tolerance in fast ones."""
    S = swmhd
    Nx, Ny, topo, form = 48, 40, (P, B), 1
    npt = np.float64 if dtype == torch.float64 else np.float32
    g = grid_for(S, Nx, Ny, topo)
    states = member_states(oracle, Nx, Ny, topo, form, GRADS_PB, 41, g.dx, g.dy, npt)
    four = make_ensemble(S, g, form, states, GRADS_PB, strict=strict, dtype=dtype)
    two = make_ensemble(S, g, form, states, GRADS_PB, strict=strict, dtype=dtype)
    four.time_steps(4, DT)
    two.time_steps(2, DT)
    for m in range(len(states)):
        model = two.member(m)
        assert model.boundary_conditions == (bcs_for(S, GRADS_PB[m]) or {})
        model.time_steps(2, DT)
        model.synchronize()
        assert model.iteration == 4
        for s, a in zip(model.fields, member_arrays(four, m)):
            assert bitwise(s.numpy(), a) if strict else close(s.numpy(), a, dtype), m


def _diag_equal(d1, d2):
    return all(d1[k] == d2[k] or (math.isnan(d1[k]) and math.isnan(d2[k])) for k in d2)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("form,topo", [(1, (P, B)), (0, (B, B))])
def test_diagnostics_bitwise_per_member(swmhd, oracle, form, topo, dtype):
    S = swmhd
    Nx, Ny = 64, 48
    npt = np.float64 if dtype == torch.float64 else np.float32
    g = grid_for(S, Nx, Ny, topo)
    grads = GRADS_PB if topo == (P, B) else [None] * 3
    states = member_states(oracle, Nx, Ny, topo, form, grads, 31, g.dx, g.dy, npt)
    e = make_ensemble(S, g, form, states, grads, strict=False, dtype=dtype)
    e.time_steps(2, DT)
    into = torch.full((len(states), 7), -1.0, dtype=torch.float64, device="cuda")
    e.diagnostics_into(into, h_ref=1.1)
    into = into.cpu().tolist()
    got = e.diagnostics(h_ref=1.1)
    keys = ("kinetic_energy", "magnetic_energy", "potential_energy", "max_abs_u", "max_abs_v", "max_abs_A", "min_h")
    for m in range(len(states)):
        want = e.member(m).diagnostics(h_ref=1.1)
        assert _diag_equal(dict(zip(keys, into[m])), {k: want[k] for k in keys}), m
        assert _diag_equal(got[m], want), m


def test_example_runs_a_channel_gradient_sweep(tmp_path):
    ex = os.path.join(ROOT, "examples", "run_swmhd.py")
    csvf = tmp_path / "channel.csv"
    grads = (-0.01, -0.05, -0.1)
    r = subprocess.run([sys.executable, ex, "--channel", "--gradients", ",".join(str(x) for x in grads), "--size", "64", "--stop-time", "0.5",
                        "--every", "25", "--energies", str(csvf)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(csvf) as f:
        rows = list(csv.DictReader(f))
    assert list(rows[0].keys())[0] == "member"
    assert {row["member"] for row in rows} == {"0", "1", "2"}
    for m in range(len(grads)):
        mine = [row for row in rows if row["member"] == str(m)]
        assert [float(row["time"]) for row in mine] == pytest.approx([0.0, 0.25, 0.5])
        assert all(math.isfinite(float(row[k])) for row in mine for k in ("kinetic", "magnetic", "potential", "total"))
    # the imposed field B_x = -g / h: the magnetic energy grows with the gradient squared
    me = [float([row for row in rows if row["member"] == str(m)][0]["magnetic"]) for m in range(len(grads))]
    assert me[0] < me[1] < me[2]


# ---------------------------------------------------------------------------------------------------------------------------------
# the wall body of the ensemble kernel (BND + ENS has no stage entry point: it runs under swmhd_ensemble_step_rk3_bc* only) at the
# shapes of the single grid's wall matrix
# ---------------------------------------------------------------------------------------------------------------------------------
import stage_cases as SC      # noqa: E402

PAD, GAP, FILL = 5, 37, 777.0
# distinct GradientBoundaryCondition values of A per member (west, east, south, north), cut to the Bounded sides of a topology
WALL_GRADS = [(0.03, -0.04, -0.05, -0.05), (-0.11, 0.1, 0.125, -0.02), (0.2, 0.07, -0.3, 0.3)]


def wall_grads(topo):
    return [tuple(v if topo[k // 2] == B else None for k, v in enumerate(gr)) for gr in WALL_GRADS]


def step_pitched_members(S, Nx, Ny, topo, form, states, grads, dtype, strict, dx, dy, dt, params=None):
    """ONE RK3 step of swmhd_ensemble_step_rk3_bc_* (params: rows (g, f, dt) -> swmhd_ensemble_step_rk3_bc_params_*) through the C-ABI
    on members pitched in rows and between members (stride_y = Nx + 6 + 5, stride_m = (Ny + 6) stride_y + 37), all four buffer
    families prefilled with FILL.  Asserts that the row padding and the member gaps of all 16 buffers still hold FILL and returns every
    member's four parents."""
    L, M = S._lib, len(states)
    sy = Nx + 6 + PAD
    sm = (Ny + 6) * sy + GAP
    sfx, tdt = ("f64", torch.float64) if dtype == np.float64 else ("f32", torch.float32)
    outside = np.ones(M * sm, dtype=bool)
    view = lambda flat, m: flat[m * sm:m * sm + (Ny + 6) * sy].reshape(Ny + 6, sy)[:, :Nx + 6]
    for m in range(M):
        view(outside, m)[...] = False
    fams = []
    for fam in range(4):
        flats = [np.full(M * sm, FILL, dtype=dtype) for _ in range(4)]
        if fam == 0:
            for k in range(4):
                for m in range(M):
                    view(flats[k], m)[...] = states[m][k]
        fams.append([torch.from_numpy(a).cuda() for a in flats])
    table = np.full((M, 4, 4), np.nan)
    for m, gr in enumerate(grads):
        table[m, 3] = [np.nan if v is None else v for v in (gr or (None,) * 4)]
    gt = torch.from_numpy(table).to(tdt).cuda()
    flags = (L.STRICT if strict else 0) | (L.BOUNDED_X if topo[0] == B else 0) | (L.BOUNDED_Y if topo[1] == B else 0)
    swapped = ctypes.c_int(-1)
    head = [L.ptr_array([t.data_ptr() for t in ts]) for ts in fams] + [M, sm, Nx, Ny, 3, 3, sy, dx, dy]
    if params is None:
        rc = getattr(L.lib(), f"swmhd_ensemble_step_rk3_bc_{sfx}")(*head, G, F, form, 2 - form, dt, 1, gt.data_ptr(), flags, ctypes.byref(swapped), None)
    else:
        pt = torch.from_numpy(np.asarray(params, dtype=np.float64)).to(tdt).cuda()
        rc = getattr(L.lib(), f"swmhd_ensemble_step_rk3_bc_params_{sfx}")(*head, pt.data_ptr(), form, 2 - form, 1, gt.data_ptr(), flags,
                                                                          ctypes.byref(swapped), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert swapped.value in (0, 1)
    host = [[t.cpu().numpy() for t in ts] for ts in fams]
    for fam in host:
        for a in fam:
            assert bool((a[outside] == FILL).all()), "row padding or a gap between members was written"
    return [[view(a, m).copy() for a in host[swapped.value]] for m in range(M)]


def check_wall_shape(S, O, shape, topo, form, dtype, strict, params=None):
    """One step of 3 pitched members with distinct states and distinct gradients of A: strict members bitwise the oracle's time_step
    with that member's gradients (and (g, f, dt)), fast members within the fast tolerance of a fast single Bounded model of the member."""
    Nx, Ny = shape
    g = grid_for(S, Nx, Ny, topo)
    grads = wall_grads(topo)
    states = member_states(O, Nx, Ny, topo, form, grads, 100 * Nx + Ny, g.dx, g.dy, dtype)
    assert all(not np.array_equal(states[i][k], states[j][k]) for k in range(4) for i in range(3) for j in range(i))
    got = step_pitched_members(S, Nx, Ny, topo, form, states, grads, dtype, strict, g.dx, g.dy, DT, params)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    for m, (q, gr) in enumerate(zip(states, grads)):
        gm, fm, dtm = (G, F, DT) if params is None else params[m]
        if strict:
            want = [a.copy() for a in q]
            O.time_step(*want, Nx, Ny, 3, 3, g.dx, g.dy, dtm, form, 2 - form, gm, fm, nthreads=4, topo=topo, gradA=gr)
            for k, (w, a) in enumerate(zip(want, got[m])):
                assert bitwise(w, a), f"member {m} field {k}: strict != oracle by {np.abs(w.astype(np.float64) - a).max()} with (g, f, dt) = {gm, fm, dtm}"
        else:
            model = S.ShallowWaterModel(g, gm, fm, formulation=FORM[form], dtype=tdt, strict=False, boundary_conditions=bcs_for(S, gr))
            for f, a in zip(model._raw_fields, q):
                f.data.copy_(torch.from_numpy(a))
            model.update_state()
            model.time_step(dtm)
            model.synchronize()
            for k, (s, a) in enumerate(zip(model.fields, got[m])):
                err = np.abs(s.numpy().astype(np.float64) - a).max()
                print(f"member {m} field {k}: fast ensemble - fast model = {err:.3e}, bitwise: {bitwise(s.numpy(), a)}")
                assert close(s.numpy(), a, dtype), f"member {m} field {k}: fast ensemble off the fast model by {err}"


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("form", [1, 0], ids=["vi", "cons"])
@pytest.mark.parametrize("topo", SC.WALL_TOPOS, ids=["PB", "BP", "BB"])
@pytest.mark.parametrize("shape", SC.WALL_SHAPES, ids=[f"{a}x{b}" for a, b in SC.WALL_SHAPES])
def test_wall_shapes_on_pitched_members(swmhd, oracle, shape, topo, form, dtype, strict):
    """The wall body of the ensemble kernel at the shapes of the single grid's wall matrix (a tile edge 1 and 3 cells from a wall, on
    it, both walls in one tile, several tiles a side), one RK3 step on every Bounded topology."""
    check_wall_shape(swmhd, oracle, shape, topo, form, dtype, strict)
