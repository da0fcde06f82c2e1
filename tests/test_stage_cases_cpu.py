"""Pins of tests/stage_cases.py, the reference of the stage matrix (tests/test_stage_matrix_gpu.py), on the CPU: its substep formulas
composed into a whole RK3 step reproduce the oracle's time_step in all three operand forms, it marks the outputs a call must not write,
its time step keeps the new state a sharp witness of the tendencies, and every width and row count of the matrix has the layout it is
there for (the launch planner is host code: swmhd_tendency_launch_geometry answers without a GPU, with the 256 compute units of an
MI355X).  No test here needs a GPU; the layout test needs the BUILT libswmhd.so (the `swmhd` fixture: build() first), the others only
the CPU oracle."""
import numpy as np
import pytest

import helpers as Hh
import stage_cases as SC

Nx, Ny, H = 40, 33, SC.H
G1, G2, G3, Z2, Z3 = SC._G1, SC._G2, SC._G3, SC._Z2, SC._Z3


def _parent(oracle, interior, like):
    """float64 parent of an interior, halos periodic-filled by the oracle."""
    a = np.zeros_like(like)
    Hh.interior(a, Nx, Ny, H, H)[...] = np.asarray(interior, dtype=np.float64)
    return oracle.fill_halo_periodic(a, Nx, Ny, H, H)


def _embed(interior, like):
    a = np.full_like(like, SC.SENTINEL)
    Hh.interior(a, Nx, Ny, H, H)[...] = np.asarray(interior, dtype=np.float64)
    return a


@pytest.mark.parametrize("form,lor", [(1, 1), (0, 2)])
def test_composed_stages_reproduce_the_oracle_time_step(oracle, form, lor):
    """Three stages of reference_stage with oracle.fill_halo_periodic between them against oracle.time_step on a 40 x 33 grid: the
    classic G- form, the anchor form and the previous-state form (second stage) give the oracle's step.  Bound: the longdouble substep
    is rounded once to double where the oracle rounds every operation (3 per stage, each at most half an ulp of the largest operand
    <= max|U|), and a difference d in U1 or U2 re-enters through dt |dG/dU| d < d at this dt: 16 eps max|U| for the three stages."""
    q, _ = SC.random_fields(Nx, Ny, form, np.float64, 11)
    dt = 1e-4
    want = [a.copy() for a in q]
    oracle.time_step(*want, Nx, Ny, H, H, SC.DX, SC.DY, dt, form, lor, SC.GRAV, SC.FCOR)
    stage = lambda state, op, variant, coeffs: SC.reference_stage(oracle, state, op, variant, coeffs, Nx, Ny, SC.DX, SC.DY, form, lor, dt)
    P = lambda xs: [_parent(oracle, x, q[0]) for x in xs]
    E = lambda xs: [_embed(x, q[0]) for x in xs]
    # classic: S1g, S2g, S3n
    s1 = stage(q, None, "S1g", (G1, 0.0))
    s2 = stage(P(s1["qnew"]), E(s1["Gn"]), "S2g", (G2, Z2))
    s3 = stage(P(s2["qnew"]), E(s2["Gn"]), "S3n", (G3, Z3))
    assert s3["Gn"] is SC.KEEP
    # anchor: A1, A2 (gamma2), A2 (gamma3) with the same W
    a1 = stage(q, None, "A1", (G1, 0.25))
    a2 = stage(P(a1["qnew"]), E(a1["Gn"]), "A2", (G2, 0.0))
    a3 = stage(P(a2["qnew"]), E(a1["Gn"]), "A2a", (G3, 0.0))
    assert a2["Gn"] is SC.KEEP and a3["Gn"] is SC.KEEP
    # previous state: S1n stores no G; P2g gets U0 and zeta2 / gamma1; the last stage is classic on P2g's G
    p1 = stage(q, None, "S1n", (G1, 0.0))
    assert p1["Gn"] is SC.KEEP
    p2 = stage(P(p1["qnew"]), E([Hh.interior(a, Nx, Ny, H, H) for a in q]), "P2g", (G2, Z2 / G1))
    p3 = stage(P(p2["qnew"]), E(p2["Gn"]), "S3n", (G3, Z3))
    eps = np.finfo(np.float64).eps
    for f in range(4):
        w = Hh.interior(want[f], Nx, Ny, H, H)
        for name, got in (("classic", s3), ("anchor", a3), ("previous state", p3)):
            err = float(np.abs(got["qnew"][f] - w).max())
            print(name, f, err / (eps * np.abs(w).max()))
            assert err <= 16 * eps * np.abs(w).max(), (name, f, err)
        assert p2["Gn"][f].dtype == np.float64 and np.array_equal(p2["Gn"][f], s2["Gn"][f])      # same U1, same tendencies


def test_markers_coefficients_and_rows(oracle):
    """What a call must not write is marked; T has no new state; a row range cuts every output; coefficients reach the reference in
    the precision of the call; the two P* forms and the generic pair are distinguishable from their classic neighbours."""
    assert len(SC.calls()) == 2 * (len(SC.VARIANTS) - 1) + 1 == 19
    data = SC.StageData(oracle, Nx, Ny, 1, 1, np.float32, seed=5)
    for variant, cset in SC.calls():
        v, coeffs = SC.VARIANTS[variant], SC.COEFFS[cset][variant]
        dt = data.dt(coeffs[0])
        ref = SC.reference_stage(oracle, data.q, data.aux if v["operand"] else None, variant, coeffs, Nx, Ny, data.dx, data.dy, 1, 1, dt,
                                 rows=SC.PARTIAL, G=data.G)
        assert (ref["qnew"] is None) == (variant == "T")
        assert (ref["Gn"] is SC.KEEP) == (variant in ("S1n", "S3n", "P3n", "A2", "A2a"))
        for out in (ref["qnew"], ref["Gn"]):
            if out is not None and out is not SC.KEEP:
                assert all(a.shape == (SC.PARTIAL[1] - SC.PARTIAL[0], Nx) for a in out)
        b = SC.stage_bounds(data, data.q, data.aux if v["operand"] else None, variant, coeffs, dt, ref, rows=SC.PARTIAL)
        assert (b["Gn"] is None) == (ref["Gn"] is SC.KEEP) and (b["qnew"] is None) == (ref["qnew"] is None)
        if variant != "T":
            # the time step makes the increment of every field at least 1 % of the field (and at most its size): an error in G beyond
            # its tolerance then shows in qnew above the 4 eps rounding allowance
            assert dt == float(np.float32(dt)) and dt > 0
            for f in range(4):
                inc = dt * abs(coeffs[0]) * data.Gmax[f]
                assert 1e-2 * data.Umax[f] <= inc <= 1.01 * max(data.Umax), (variant, f, inc)
                assert dt * abs(coeffs[0]) * SC.TOL[data.dtype] * data.scales[f] >= 4 * np.finfo(np.float32).eps * data.Umax[f]
    # the generic zeta of a first stage is ignored, as the header says of Gm == NULL
    a = SC.reference_stage(oracle, data.q, None, "S1g", (0.37, -0.21), Nx, Ny, data.dx, data.dy, 1, 1, 1e-3, G=data.G)
    b = SC.reference_stage(oracle, data.q, None, "S1g", (0.37, 0.0), Nx, Ny, data.dx, data.dy, 1, 1, 1e-3, G=data.G)
    assert all(np.array_equal(x, y) for x, y in zip(a["qnew"], b["qnew"]))
    # fp32 coefficients are the rounded ones
    g32 = np.longdouble(np.float32(0.37))
    U = Hh.interior(data.q[0], Nx, Ny, H, H).astype(np.longdouble)
    assert np.array_equal(a["qnew"][0], U + np.longdouble(np.float32(1e-3)) * g32 * data.G[0].astype(np.longdouble))


def test_poison_halo():
    a = np.arange(7.0 * 9).reshape(9, 7).copy()
    b = Hh.poison_halo(a.copy(), 3, 5, 2, 2, x=True, y=False)
    assert np.isnan(b[:, :2]).all() and np.isnan(b[:, 5:]).all() and np.array_equal(b[:, 2:5], a[:, 2:5])
    c = Hh.poison_halo(a.copy(), 3, 5, 2, 2, x=False, y=True)
    assert np.isnan(c[:2]).all() and np.isnan(c[7:]).all() and np.array_equal(c[2:7], a[2:7])
    d = Hh.poison_halo(a.copy(), 3, 5, 2, 2)
    assert np.array_equal(d[2:7, 2:5], a[2:7, 2:5]) and np.isnan(d).sum() == a.size - 15


def test_every_shape_of_the_matrix_has_its_layout(swmhd):
    """The widths and row counts of the matrix hit the layouts they were chosen for, by the launch planner's own answer: exactly full,
    folding, just not folding and one-column last strips of 256 lanes; partial, full and ragged 128-lane strips; the packed-fp32
    strips; 1, 5 and 6 segments of 6 rows with last segments of 3, 1, 1 and 3 rows.  (The GPU test asserts the same on the device.)
    Which launches fold is inferred from those answers (stage_cases.folds), the query does not say; so the environment must allow it."""
    assert SC.fold_enabled(), "SWMHD_T_FOLD=0 in the environment: the folded layouts of the matrix would not be exercised"
    L = swmhd._lib
    seen, folded = set(), set()
    for Nx, Ny, rows, form, lor, dtype, flags in SC.matrix():
        nrows = Ny if rows is None else rows[1] - rows[0]
        line = SC.check_layout(L, Nx, nrows, form, dtype, flags)
        geo = L.tendency_launch_geometry(Nx, nrows, form, np.dtype(dtype).itemsize, SC.MARCH_KERNEL | flags)
        seen.add((geo["kind"], geo["threads"], Nx, nrows))
        if "folded" in line:
            folded.add((Nx, geo["nseg"]))
    assert {(2501, 1), (2501, 5), (2501, 6), (372, 1), (372, 5), (372, 6), (372, 4)} <= folded and not any(Nx == 373 for Nx, _ in folded)
    for Nx, (lanes, _, _) in SC.LAYOUTS.items():
        assert (2, lanes, Nx, 31) in seen
    for Nx in SC.PACKED_WIDTHS:
        assert (3, 256, Nx, 31) in seen
    for nrows in (3, 25, 31, 33, 24):
        assert any(s[3] == nrows for s in seen)
