"""GPU tests of per-member parameters in ensembles (gravitational_acceleration, coriolis_f and dt as sequences;
swmhd_ensemble_*_params): every member computes what the same grid computes alone with that member's (g, f, dt) -- strict members
bitwise against the oracle's time_step and a strict ShallowWaterModel, fast members within the fast tolerance of a fast
ShallowWaterModel -- under both member mappings and tile heights, on pitched members, with a NaN parameter in one member, through graph
replays, with per-member diagnostics and member handover; a table of equal rows reproduces the scalar call; the example sweeps f and dt.

Five members: 0 carries the defaults, 0 and 3 repeat g and dt (a table read with stride 1 instead of 3 would not survive that)."""
import csv
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

import helpers as Hh
from test_bounded_oracle import state, P, B
import stage_cases as SC
from test_ensemble_bounded_gpu import GRADS_PB, bcs_for, bitwise, check_wall_shape, close, grid_for, member_arrays, member_states

pytestmark = pytest.mark.gpu
FORM = {0: "Conservative", 1: "VectorInvariant"}
GS = [9.81, 1.0, 4.0, 9.81, 20.0]
FS = [1.0, 0.0, -0.5, 2.0, 1.0]
DTS = [0.01, 0.005, 0.0025, 0.01, 0.002]
NM = 5
PP = (P, P)
GRADS = {PP: [None] * NM,
         (P, B): GRADS_PB + [(None, None, 0.02, None)],
         (B, B): [(0.03, -0.04, -0.05, -0.05), None, (None, 0.1, None, 0.3), (None, None, 0.125, -0.02), (0.2, None, None, None)]}
NPT = {torch.float64: np.float64, torch.float32: np.float32}


def periodic_states(Nx, Ny, form, seed, dtype=np.float64):
    return [[np.ascontiguousarray(Hh.fill_halo_periodic(a, Nx, Ny, 3, 3).astype(dtype)) for a in state(Nx, Ny, seed + 13 * m, form)]
            for m in range(NM)]


def states_for(O, g, topo, form, seed, dtype=np.float64):
    if topo == PP:
        return periodic_states(g.Nx, g.Ny, form, seed, dtype)
    return member_states(O, g.Nx, g.Ny, topo, form, GRADS[topo], seed, g.dx, g.dy, dtype)


def make_ensemble(S, g, topo, form, states, strict, dtype=torch.float64, gs=GS, fs=FS, **kw):
    if topo == PP:
        e = S.ShallowWaterEnsemble(g, len(states), gs, fs, formulation=FORM[form], dtype=dtype, strict=strict, **kw)
    else:
        e = S.BoundedShallowWaterEnsemble(g, len(states), gs, fs, formulation=FORM[form], dtype=dtype, strict=strict,
                                          boundary_conditions=[bcs_for(S, gr) for gr in GRADS[topo]], **kw)
    e.set(**{n: np.stack([st[k] for st in states]) for k, n in enumerate(e.names)})
    return e


def make_model(S, g, topo, form, q, m, strict, dtype=torch.float64):
    """The single model of member m: its g and f, and its boundary conditions."""
    model = S.ShallowWaterModel(g, GS[m], FS[m], formulation=FORM[form], dtype=dtype, strict=strict, boundary_conditions=bcs_for(S, GRADS[topo][m]))
    for f, a in zip(model._raw_fields, q):
        f.data.copy_(torch.from_numpy(a))
    model.update_state()
    return model


_ORACLE = {}


def oracle_steps(O, g, topo, form, seed, nsteps=3):
    """(states, oracle results after nsteps with every member's own g, f, dt): computed once per case, never modified."""
    key = (g.Nx, g.Ny, topo, form, seed, nsteps)
    if key not in _ORACLE:
        states = states_for(O, g, topo, form, seed)
        want = []
        for m, q in enumerate(states):
            qo = [a.copy() for a in q]
            for _ in range(nsteps):
                O.time_step(*qo, g.Nx, g.Ny, 3, 3, g.dx, g.dy, DTS[m], form, 2 - form, GS[m], FS[m], nthreads=8, topo=topo, gradA=GRADS[topo][m])
            want.append(qo)
        _ORACLE[key] = (states, want)
    return _ORACLE[key]


def check_strict(S, O, g, topo, form, seed):
    states, want = oracle_steps(O, g, topo, form, seed)
    e = make_ensemble(S, g, topo, form, states, strict=True)
    assert e.parameters is not None and tuple(e.parameters.shape) == (NM, 3) and e.parameters.dtype == torch.float64
    e.time_steps(3, DTS)
    e.synchronize()
    assert np.array_equal(e.parameters.cpu().numpy(), np.stack([GS, FS, DTS], axis=1))
    for m, q in enumerate(states):
        model = make_model(S, g, topo, form, q, m, strict=True)
        model.time_steps(3, DTS[m])
        model.synchronize()
        for w, s, a in zip(want[m], model.fields, member_arrays(e, m)):
            assert bitwise(w, a), f"member {m}: strict ensemble != oracle with (g, f, dt) = {GS[m], FS[m], DTS[m]} by {np.abs(w - a).max()}"
            assert bitwise(s.numpy(), a), f"member {m}: strict ensemble != strict model"


@pytest.mark.parametrize("form", [1, 0])
@pytest.mark.parametrize("shape", [(48, 48), (100, 37)])
def test_strict_periodic_members_equal_oracle(swmhd, oracle, form, shape):
    check_strict(swmhd, oracle, grid_for(swmhd, *shape, PP), PP, form, 11)


@pytest.mark.parametrize("form", [1, 0])
@pytest.mark.parametrize("topo", [(P, B), (B, B)])
def test_strict_bounded_members_equal_oracle(swmhd, oracle, form, topo):
    """Per-member gradients combined with per-member parameters."""
    check_strict(swmhd, oracle, grid_for(swmhd, 48, 40, topo), topo, form, 9)


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("form", [1, 0], ids=["vi", "cons"])
@pytest.mark.parametrize("topo", SC.WALL_TOPOS, ids=["PB", "BP", "BB"])
@pytest.mark.parametrize("shape", SC.WALL_SHAPES, ids=[f"{a}x{b}" for a, b in SC.WALL_SHAPES])
def test_wall_shapes_on_pitched_members_with_their_own_parameters(swmhd, oracle, shape, topo, form, dtype, strict):
    """The wall body of the PAR ensemble kernel at the shapes of the single grid's wall matrix: one RK3 step of 3 pitched members with
    distinct states, gradients and (g, f, dt) (one f negative) -- strict bitwise the oracle's time_step with the member's gradients and
    parameters, fast within the fast tolerance of a fast single Bounded model with them; row padding and gaps untouched."""
    check_wall_shape(swmhd, oracle, shape, topo, form, dtype, strict, params=list(zip(GS, FS, DTS))[:3])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("form", [1, 0])
@pytest.mark.parametrize("shape,topo", [((48, 48), PP), ((100, 37), PP), ((48, 40), (P, B)), ((48, 40), (B, B))])
def test_fast_members_match_single_fast_model(swmhd, oracle, form, shape, topo, dtype):
    S = swmhd
    g = grid_for(S, *shape, topo)
    states = states_for(oracle, g, topo, form, 23, NPT[dtype])
    e = make_ensemble(S, g, topo, form, states, strict=False, dtype=dtype)
    assert e.parameters.dtype == dtype
    e.time_steps(3, DTS)
    e.synchronize()
    for m, q in enumerate(states):
        model = make_model(S, g, topo, form, q, m, strict=False, dtype=dtype)
        model.time_steps(3, DTS[m])
        model.synchronize()
        for s, a in zip(model.fields, member_arrays(e, m)):
            err = np.abs(s.numpy().astype(np.float64) - a).max()
            print(f"member {m}: fast ensemble - fast model = {err:.3e} of {np.abs(s.numpy()).max():.3e}")
            assert close(s.numpy(), a, dtype), f"member {m}: fast ensemble off the fast model by {err}"


def _child(out):
    """Run in a fresh process (SWMHD_ENS_MAP / SWMHD_ENS_RY are read once): strict (100, 37) x 5, both formulations, 3 steps."""
    import swmhd_amd as S
    res = {}
    g = grid_for(S, 100, 37, PP)
    for form in (1, 0):
        e = make_ensemble(S, g, PP, form, periodic_states(100, 37, form, 11), strict=True)
        e.time_steps(3, DTS)
        e.synchronize()
        for m in range(NM):
            for k, a in enumerate(member_arrays(e, m)):
                res[f"f{form}_m{m}_{k}"] = a
    np.savez(out, **res)


@pytest.mark.parametrize("knob", [{"SWMHD_ENS_MAP": "2"}, {"SWMHD_ENS_RY": "1"}], ids=["member-in-blockIdx.y", "64x4-tiles"])
def test_member_mapping_and_tile_height(swmhd, oracle, tmp_path, knob):
    """The member index under the other mapping (member = blockIdx.y) and the other tile height: still every member's own parameters."""
    out = str(tmp_path / "child.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("SWMHD_ENS_MAP", "SWMHD_ENS_RY")}
    env.update(knob)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out)
    g = grid_for(swmhd, 100, 37, PP)
    for form in (1, 0):
        _states, want = oracle_steps(oracle, g, PP, form, 11)
        for m in range(NM):
            for k, w in enumerate(want[m]):
                assert bitwise(w, got[f"f{form}_m{m}_{k}"]), f"{knob}: member {m} field {k} != oracle with its own (g, f, dt)"


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
def test_pitched_members_leave_the_gaps_alone(swmhd, strict):
    S = swmhd
    Nx, Ny = 48, 36
    g = grid_for(S, Nx, Ny, PP)
    states = periodic_states(Nx, Ny, 1, 3)
    Py, Px = g.parent_shape
    sm = Py * Px + 17
    e = make_ensemble(S, g, PP, 1, states, strict=strict, member_stride=sm)
    assert e.stride_m == sm
    flats = [t.as_strided((NM * sm,), (1,)) for t in e._state + e._alt + e.Gn + e.Gm]
    gaps = torch.cat([torch.arange(m * sm + Py * Px, (m + 1) * sm) for m in range(NM)]).cuda()
    for fl in flats:
        fl[gaps] = 12345.0
    ref = make_ensemble(S, g, PP, 1, states, strict=strict)
    for x in (e, ref):
        x.time_steps(4, DTS)
        x.synchronize()
    for fl in flats:
        assert bool((fl[gaps] == 12345.0).all()), "a gap between members was written"
    for m in range(NM):
        for a, b in zip(member_arrays(e, m), member_arrays(ref, m)):
            assert bitwise(a, b), m


@pytest.mark.parametrize("column", [0, 1, 2], ids=["g", "f", "dt"])
@pytest.mark.parametrize("topo", [PP, (P, B)])
def test_a_nan_parameter_poisons_its_member_only(swmhd, oracle, topo, column):
    S = swmhd
    g = grid_for(S, 64, 40, topo)
    states = states_for(oracle, g, topo, 1, 5)
    par = [list(GS), list(FS), list(DTS)]
    clean = make_ensemble(S, g, topo, 1, states, strict=False)
    par[column][2] = float("nan")
    dirty = make_ensemble(S, g, topo, 1, states, strict=False, gs=par[0], fs=par[1])
    clean.time_steps(3, DTS)
    dirty.time_steps(3, par[2])
    clean.synchronize(); dirty.synchronize()
    assert any(np.isnan(a).any() for a in member_arrays(dirty, 2))
    for m in (0, 1, 3, 4):
        for a, b in zip(member_arrays(clean, m), member_arrays(dirty, m)):
            assert bitwise(a, b), f"member {m} changed by a NaN parameter of member 2"


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("form,topo", [(1, PP), (0, PP), (1, (P, B)), (0, (B, B))])
def test_uniform_table_equals_scalar_call(swmhd, oracle, form, topo, dtype, strict):
    """All rows (9.81, 1, 0.01): strict is bitwise the scalar ensemble call, fast is within the fast bound of it."""
    S = swmhd
    g = grid_for(S, 100, 37, topo)
    states = states_for(oracle, g, topo, form, 7, NPT[dtype])
    scalar = make_ensemble(S, g, topo, form, states, strict=strict, dtype=dtype, gs=9.81, fs=1.0)
    table = make_ensemble(S, g, topo, form, states, strict=strict, dtype=dtype, gs=[9.81] * NM, fs=[1.0] * NM)
    assert scalar.parameters is None and table.parameters is not None
    scalar.time_steps(3, 0.01)
    table.time_steps(3, [0.01] * NM)
    scalar.synchronize(); table.synchronize()
    assert table.clock_time == scalar.clock_time and table.clock_times.tolist() == [scalar.clock_time] * NM
    for m in range(NM):
        for a, b in zip(member_arrays(scalar, m), member_arrays(table, m)):
            assert bitwise(a, b) if strict else close(a, b, dtype), f"member {m}: off by {np.abs(a.astype(np.float64) - b).max()}"


@pytest.mark.parametrize("topo", [PP, (P, B)])
def test_graph_replay_equals_eager(swmhd, oracle, topo):
    S = swmhd
    g = grid_for(S, 64, 64, topo)
    states = states_for(oracle, g, topo, 1, 9)
    eager = make_ensemble(S, g, topo, 1, states, strict=False)
    graph = make_ensemble(S, g, topo, 1, states, strict=False)
    graph.capture_graph(list(DTS))
    assert graph.iteration == 0 and graph.clock_times.tolist() == [0.0] * NM and graph.clock_time == 0.0
    graph.time_steps(6, np.array(DTS))          # another object with the captured values: replays
    assert graph._graph is not None and graph._graph_dt == tuple(DTS)
    for _ in range(6):
        eager.time_step(DTS)
    graph.synchronize(); eager.synchronize()
    assert graph.iteration == eager.iteration == 6
    assert np.allclose(graph.clock_times, 6 * np.array(DTS), rtol=0, atol=1e-12)
    assert np.allclose(graph.clock_times, eager.clock_times, rtol=0, atol=1e-12)
    with pytest.raises(S._lib.SwmhdError):
        graph.clock_time
    for m in range(NM):
        for a, b in zip(member_arrays(graph, m), member_arrays(eager, m)):
            assert bitwise(a, b), m
    # a graph steps with what the table holds when it runs: time_steps puts the captured dt back after a step with another one
    graph.time_step(0.001); eager.time_step(0.001)
    graph.time_steps(3, DTS)
    for _ in range(3):
        eager.time_step(DTS)
    graph.synchronize(); eager.synchronize()
    for m in range(NM):
        for a, b in zip(member_arrays(graph, m), member_arrays(eager, m)):
            assert bitwise(a, b), m


def _diag_equal(d1, d2):
    return all(d1[k] == d2[k] or (math.isnan(d1[k]) and math.isnan(d2[k])) for k in d2)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", [(64, 64), (100, 37)])
def test_diagnostics_use_each_members_g(swmhd, shape, dtype):
    S = swmhd
    g = grid_for(S, *shape, PP)
    states = periodic_states(*shape, 0, 31, NPT[dtype])
    e = make_ensemble(S, g, PP, 0, states, strict=False, dtype=dtype)
    e.time_steps(2, DTS)
    into = torch.full((NM, 7), -1.0, dtype=torch.float64, device="cuda")
    e.diagnostics_into(into, h_ref=1.1)
    into = into.cpu().tolist()
    got = e.diagnostics(h_ref=1.1)
    keys = ("kinetic_energy", "magnetic_energy", "potential_energy", "max_abs_u", "max_abs_v", "max_abs_A", "min_h")
    for m in range(NM):
        model = e.member(m)
        assert model.g == GS[m]
        want = model.diagnostics(h_ref=1.1)          # swmhd_diagnostics_* on that member alone with its g
        assert _diag_equal(dict(zip(keys, into[m])), {k: want[k] for k in keys}), m
        assert _diag_equal(got[m], want), m
    assert got[0]["potential_energy"] != got[1]["potential_energy"]


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
@pytest.mark.parametrize("topo", [PP, (P, B)])
def test_member_handover_continues(swmhd, oracle, topo, strict):
    """4 ensemble steps == 2 ensemble steps, member(m), 2 steps of that ShallowWaterModel with the member's g, f and dt."""
    S = swmhd
    g = grid_for(S, 48, 40, topo)
    states = states_for(oracle, g, topo, 1, 41)
    four = make_ensemble(S, g, topo, 1, states, strict=strict)
    two = make_ensemble(S, g, topo, 1, states, strict=strict)
    four.time_steps(4, DTS)
    two.time_steps(2, DTS)
    for m in range(NM):
        model = two.member(m)
        assert model.g == GS[m] and model.f == FS[m] and model.iteration == 2
        assert model.clock_time == two.clock_times[m] == pytest.approx(2 * DTS[m], abs=1e-15)
        model.time_steps(2, DTS[m])
        model.synchronize()
        for s, a in zip(model.fields, member_arrays(four, m)):
            assert bitwise(s.numpy(), a) if strict else close(s.numpy(), a, torch.float64), m


def test_run_and_frames_with_per_member_g_and_f(swmhd):
    """run() and FieldTimeSeries under a scalar dt: the same steps as time_steps; a per-member dt is refused before any step."""
    S = swmhd
    g = grid_for(S, 64, 40, PP)
    states = periodic_states(64, 40, 1, 3)
    a, b = (make_ensemble(S, g, PP, 1, states, strict=False) for _ in range(2))
    series = S.FieldTimeSeries(a, schedule=S.IterationInterval(2), capacity=4)
    S.run(a, 0.005, stop_iteration=4, writers=[series])
    b.time_steps(4, 0.005)
    a.synchronize(); b.synchronize()
    assert len(series) == 3 and series.times == pytest.approx([0.0, 0.01, 0.02]) and a.clock_time == b.clock_time
    for m in range(NM):
        for x, y in zip(member_arrays(a, m), member_arrays(b, m)):
            assert bitwise(x, y)
    with pytest.raises(S._lib.SwmhdError):
        S.run(a, DTS, stop_iteration=8)
    assert a.iteration == 4
    a.time_step(DTS)
    with pytest.raises(S._lib.SwmhdError):
        a.clock_time
    with pytest.raises(S._lib.SwmhdError):
        series.write()                              # a frame's time is the common clock


def test_example_sweeps_coriolis_and_dt(tmp_path):
    ex = os.path.join(ROOT, "examples", "run_swmhd.py")
    csvf = tmp_path / "sweep.csv"
    fs, dts = (0.0, 1.0, 2.0), (0.01, 0.01, 0.005)
    r = subprocess.run([sys.executable, ex, "--coriolis", "0,1,2", "--dts", "0.01,0.01,0.005", "--size", "64", "--stop-time", "0.2",
                        "--every", "10", "--energies", str(csvf)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(csvf) as f:
        rows = list(csv.DictReader(f))
    assert list(rows[0].keys())[:5] == ["member", "g", "f", "dt", "time"]
    assert {row["member"] for row in rows} == {"0", "1", "2"}
    for m in range(3):
        mine = [row for row in rows if row["member"] == str(m)]
        assert all(float(row["g"]) == 9.81 and float(row["f"]) == fs[m] and float(row["dt"]) == dts[m] for row in mine)
        assert [float(row["time"]) for row in mine] == pytest.approx([n * dts[m] for n in (0, 10, 20)], abs=1e-12)
        assert all(math.isfinite(float(row[k])) for row in mine for k in ("kinetic", "magnetic", "potential", "total"))
    first = {m: [row for row in rows if row["member"] == str(m)][1] for m in range(3)}
    assert first[0]["kinetic"] != first[1]["kinetic"]      # same dt, another f


if __name__ == "__main__":
    _child(sys.argv[1])
