"""GPU tests of ensembles (ShallowWaterEnsemble, swmhd_ensemble_*): every member of an ensemble computes what the same grid computes
alone -- bitwise against the strict oracle and a strict ShallowWaterModel, bitwise against a fast ShallowWaterModel (same tile shape,
same kernel body), member by member independent, graph-replayable, with per-member diagnostics bitwise equal to the single model's --
and the reference's own sweep (two A amplitudes at 64^2) reproduces its energy plots as one ensemble."""
import csv
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import plot_cases as P
from test_model_gpu import FORM, make_model, random_state
from test_model_oracle import G, F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DX, DY, DT = 0.11, 0.13, 0.002


def make_ensemble(S, Nx, Ny, form, states, strict, dtype=torch.float64, **kw):
    g = S.RectilinearGrid(size=(Nx, Ny), x=(0, DX * Nx), y=(0, DY * Ny), halo=(3, 3))
    e = S.ShallowWaterEnsemble(g, len(states), G, F, formulation=FORM[form], dtype=dtype, strict=strict, **kw)
    e.set(**{n: np.stack([st[k] for st in states]) for k, n in enumerate(e.names)})
    return e


def states_for(Nx, Ny, form, B, seed, dtype=np.float64):
    return [random_state(Nx, Ny, 3, seed + 17 * m, form, dtype) for m in range(B)]


def member_arrays(e, m):
    return [t[m].cpu().numpy() for t in e.fields]


def bitwise(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("form", [1, 0])
@pytest.mark.parametrize("shape", [(48, 48), (100, 37)])
def test_strict_members_equal_oracle_and_single_model(swmhd, oracle, form, shape):
    Nx, Ny = shape
    states = states_for(Nx, Ny, form, 5, 11)
    e = make_ensemble(swmhd, Nx, Ny, form, states, strict=True)
    e.time_steps(3, DT)
    e.synchronize()
    for m, q in enumerate(states):
        qo = [a.copy() for a in q]
        for _ in range(3):
            oracle.time_step(*qo, Nx, Ny, 3, 3, DX, DY, DT, form, 2 - form, G, F)
        model = make_model(swmhd, Nx, Ny, form, 2 - form, q, DX, DY, strict=True)
        model.time_steps(3, DT)
        model.synchronize()
        got = member_arrays(e, m)
        for w, s, a in zip(qo, model.fields, got):
            assert bitwise(w, a), f"member {m}: strict ensemble != oracle by {np.abs(w - a).max()}"
            assert bitwise(s.numpy(), a), f"member {m}: strict ensemble != strict model"


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("form", [1, 0])
@pytest.mark.parametrize("shape", [(48, 48), (100, 37)])
def test_fast_members_equal_single_model(swmhd, oracle, form, shape, dtype):
    Nx, Ny = shape
    npt = np.float64 if dtype == torch.float64 else np.float32
    states = states_for(Nx, Ny, form, 5, 23, npt)
    e = make_ensemble(swmhd, Nx, Ny, form, states, strict=False, dtype=dtype)
    e.time_steps(3, DT)
    e.synchronize()
    for m, q in enumerate(states):
        model = make_model(swmhd, Nx, Ny, form, 2 - form, q, DX, DY, strict=False, dtype=dtype)
        model.time_steps(3, DT)
        model.synchronize()
        got = member_arrays(e, m)
        for s, a in zip(model.fields, got):
            assert bitwise(s.numpy(), a), f"member {m}: fast ensemble != fast model by {np.abs(s.numpy() - a).max()}"
        if dtype == torch.float64:
            qo = [a.copy() for a in q]
            for _ in range(3):
                oracle.time_step(*qo, Nx, Ny, 3, 3, DX, DY, DT, form, 2 - form, G, F)
            for w, a in zip(qo, got):
                assert np.abs(w - a).max() <= 1e-12 * np.abs(w).max()


@pytest.mark.parametrize("form", [1, 0])
def test_a_nan_member_leaves_the_others_alone(swmhd, form):
    Nx, Ny = 64, 40
    states = states_for(Nx, Ny, form, 4, 5)
    clean = make_ensemble(swmhd, Nx, Ny, form, states, strict=False)
    bad = [[a.copy() for a in st] for st in states]
    bad[2][2][10, 20] = np.nan
    dirty = make_ensemble(swmhd, Nx, Ny, form, bad, strict=False)
    for e in (clean, dirty):
        e.time_steps(5, DT)
        e.synchronize()
    assert np.isnan(member_arrays(dirty, 2)[2]).any()
    for m in (0, 1, 3):
        for a, b in zip(member_arrays(clean, m), member_arrays(dirty, m)):
            assert bitwise(a, b), f"member {m} changed by a NaN in member 2"


@pytest.mark.parametrize("fuse_halo", [True, False], ids=["wrap", "halo-fill"])
def test_pitched_members_leave_the_gaps_alone(swmhd, fuse_halo):
    Nx, Ny, B = 48, 36, 3
    states = states_for(Nx, Ny, 1, B, 3)
    Py, Px = Ny + 6, Nx + 6
    sm = Py * Px + 37
    e = make_ensemble(swmhd, Nx, Ny, 1, states, strict=False, member_stride=sm, fuse_halo=fuse_halo)
    assert e.stride_m == sm
    bufs = e._state + e._alt + e.Gn + e.Gm
    flats = [t.as_strided((B * sm,), (1,)) for t in bufs]
    gaps = torch.cat([torch.arange(m * sm + Py * Px, (m + 1) * sm) for m in range(B)]).cuda()
    for fl in flats:
        fl[gaps] = 12345.0
    ref = make_ensemble(swmhd, Nx, Ny, 1, states, strict=False, fuse_halo=fuse_halo)
    for x in (e, ref):
        x.time_steps(10, DT)
        x.synchronize()
    for fl in flats:
        assert bool((fl[gaps] == 12345.0).all()), "a gap between members was written"
    for m in range(B):
        for a, b in zip(member_arrays(e, m), member_arrays(ref, m)):
            assert bitwise(a, b)


@pytest.mark.parametrize("form", [1, 0])
def test_graph_replay_equals_eager(swmhd, form):
    Nx, Ny = 64, 64
    states = states_for(Nx, Ny, form, 3, 9)
    eager = make_ensemble(swmhd, Nx, Ny, form, states, strict=False)
    graph = make_ensemble(swmhd, Nx, Ny, form, states, strict=False)
    graph.capture_graph(DT)
    for n in (4, 3, 1, 5):                  # odd counts leave the roles swapped; the next call restores them
        graph.time_steps(n, DT)
        for _ in range(n):
            eager.time_step(DT)
        graph.synchronize(); eager.synchronize()
        assert graph.iteration == eager.iteration and abs(graph.clock_time - eager.clock_time) < 1e-12
        for m in range(3):
            for a, b in zip(member_arrays(graph, m), member_arrays(eager, m)):
                assert bitwise(a, b)
    # one member with graph replay == the single model with graph replay
    one = make_ensemble(swmhd, Nx, Ny, form, states[:1], strict=False)
    model = make_model(swmhd, Nx, Ny, form, 2 - form, states[0], DX, DY, strict=False)
    one.capture_graph(DT); model.capture_graph(DT)
    one.time_steps(7, DT); model.time_steps(7, DT)
    one.synchronize(); model.synchronize()
    for a, s in zip(member_arrays(one, 0), model.fields):
        assert bitwise(a, s.numpy())


def _diag_equal(d1, d2):
    return all(d1[k] == d2[k] or (math.isnan(d1[k]) and math.isnan(d2[k])) for k in d2)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("form,shape", [(1, (64, 64)), (0, (100, 37)), (1, (520, 512))])
def test_diagnostics_bitwise_per_member(swmhd, form, shape, dtype):
    """520 x 512 = 266240 cells: every partial block of the single-grid launch owns cells; the smaller grids leave most empty."""
    Nx, Ny = shape
    B = 3 if Nx < 512 else 2
    npt = np.float64 if dtype == torch.float64 else np.float32
    states = states_for(Nx, Ny, form, B, 31, npt)
    states[-1][2][7, 9] = np.nan                     # a NaN member: its min h / energies are NaN like the single model's
    e = make_ensemble(swmhd, Nx, Ny, form, states, strict=False, dtype=dtype)
    e.time_steps(2, DT)
    got = e.diagnostics(h_ref=1.1)
    into = torch.full((B, 7), -1.0, dtype=torch.float64, device="cuda")
    e.diagnostics_into(into, h_ref=1.1)
    into = into.cpu().tolist()
    keys = ("kinetic_energy", "magnetic_energy", "potential_energy", "max_abs_u", "max_abs_v", "max_abs_A", "min_h")
    for m in range(B):
        want = e.member(m).diagnostics(h_ref=1.1)
        assert _diag_equal(got[m], want), (m, got[m], want)
        assert _diag_equal(dict(zip(keys, into[m])), {k: want[k] for k in keys}), m


def test_1024_members_of_64x64(swmhd):
    """4.2 Mcell in one launch per stage: the reference's set-up (vortex, two Gaussians of A, dt = 0.01) with 1024 amplitudes of A."""
    S = swmhd
    N, B, dt = 64, 1024, 0.01
    g = S.RectilinearGrid(size=(N, N), x=(-P.L / 2, P.L / 2), y=(-P.L / 2, P.L / 2))
    amps = np.linspace(0.05, 0.6, B)
    ic = dict(u=lambda X, Y: 5 * Y * np.exp(-(X ** 2 + Y ** 2)), v=lambda X, Y: -5 * X * np.exp(-(X ** 2 + Y ** 2)),
              h=lambda X, Y: np.ones_like(X))
    e = S.ShallowWaterEnsemble(g, B, G, F)
    e.set(**ic, A=[P.two_gaussians(a) for a in amps])
    e.time_steps(20, dt)
    e.synchronize()
    for t in e.fields:
        assert bool(torch.isfinite(t).all())
    # at 64^2 per member the launch uses the single model's 64 x 4 tile (RY = 1): bitwise
    for m in (0, 511, 1023):
        model = S.ShallowWaterModel(g, G, F)
        model.set(**ic, A=P.two_gaussians(amps[m]))
        model.time_steps(20, dt)
        model.synchronize()
        for a, s in zip(member_arrays(e, m), model.fields):
            assert bitwise(a, s.numpy()), m


@pytest.mark.parametrize("formdir", ["jacobian_formulation", "divergence_formulation"])
def test_reference_sweep_as_one_ensemble(swmhd, formdir):
    """The reference's two-Gaussian runs at 64^2 (A amplitude 0.1 and 0.5) as a 2-member ensemble, energies recorded into a device
    tensor every model time unit without a host sync, against the digitised plots with the bar of test_reference_plots.py."""
    S = swmhd
    keys = [f"{formdir}/64x64_two_Gaussians_low_B", f"{formdir}/64x64_two_Gaussians_high_B"]
    R = P.readings()
    form, N, _ = P.parse(keys[0])
    g = S.RectilinearGrid(size=(N, N), x=(-P.L / 2, P.L / 2), y=(-P.L / 2, P.L / 2))
    e = S.ShallowWaterEnsemble(g, 2, P.G, P.F, formulation="VectorInvariant" if form == 1 else "Conservative")
    zero = lambda X, Y: np.zeros_like(X)
    n1, n2 = e.names[:2]
    e.set(**{n1: zero, n2: zero, "h": lambda X, Y: np.ones_like(X), "A": [P.ICS[P.parse(k)[2]]["A"] for k in keys]})
    nsamp = int(round(1.0 / P.DT))
    t_end = max(R[k]["times"][-1] for k in keys)
    nrec = int(round(t_end)) + 1
    rec = torch.empty((nrec, 2, 7), dtype=torch.float64, device="cuda")
    e.capture_graph(P.DT)
    e.diagnostics_into(rec[0])
    for k in range(1, nrec):
        e.time_steps(nsamp, P.DT)
        e.diagnostics_into(rec[k])
    rec = rec.cpu().numpy()
    for m, key in enumerate(keys):
        n = int(round(R[key]["times"][-1])) + 1
        tot = rec[:n, m, 0] + rec[:n, m, 1] + rec[:n, m, 2]
        series = dict(times=[float(t) for t in range(n)], kinetic=list(rec[:n, m, 0]), magnetic=list(rec[:n, m, 1]),
                      potential=list(rec[:n, m, 2]), total=list(tot), error_x100=list(np.abs(tot - tot[0]) * 100))
        c = P.compare(series, R[key], slack=3.0)
        bad = {p: w for p, w in c.items() if w[0] > 1.0}
        assert not bad, f"{key}: (ratio, t, run, plot, tol) {bad}"


def test_example_runs_an_amplitude_sweep(tmp_path):
    ex = os.path.join(ROOT, "examples", "run_swmhd.py")
    common = ["--ic", "gaussians", "--size", "64", "--stop-time", "0.5", "--every", "25"]
    csvf = tmp_path / "ens.csv"
    r = subprocess.run([sys.executable, ex, "--amps", "0.1,0.5", *common, "--energies", str(csvf)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(csvf) as f:
        rows = list(csv.DictReader(f))
    assert {row["member"] for row in rows} == {"0", "1"}
    for m, amp in enumerate((0.1, 0.5)):
        mine = [row for row in rows if row["member"] == str(m)]
        assert len(mine) == 3 and abs(float(mine[-1]["time"]) - 0.5) < 1e-9
        assert all(math.isfinite(float(row[k])) for row in mine for k in ("kinetic", "magnetic", "potential", "total"))
        single = tmp_path / f"single{m}.csv"
        r1 = subprocess.run([sys.executable, ex, "--amp", str(amp), *common, "--energies", str(single)], capture_output=True, text=True, timeout=600)
        assert r1.returncode == 0, r1.stderr[-2000:]
        with open(single) as f:
            ref = list(csv.DictReader(f))
        assert float(mine[0]["magnetic"]) == float(ref[0]["magnetic"])
