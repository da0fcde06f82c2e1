"""CPU tests of the operator matrix's reference (tests/operator_cases.py), before any GPU run: the oracle reads nothing beyond the
stencil reach the header states, on every input of the matrix under all four topologies, and does read up to it; every input is one
on which the oracle's own fp32 arithmetic stays within a quarter of the fast tolerance, row by row; and every wall case differs from
the periodic result on every non-empty row range."""
import numpy as np
import pytest

import operator_cases as OC

TOPOS = [(OC.P, OC.P)] + OC.WALLS
EPS32 = float(np.finfo(np.float32).eps)


def test_constants_and_shapes():
    assert OC.workgroup("march", "jacobian") == (252, 8) and OC.workgroup("march", "divergence") == (250, 8)
    assert OC.workgroup("tile", "jacobian") == OC.workgroup("strict", "jacobian") == (64, 16)
    assert OC.workgroup("tile", "divergence") == OC.workgroup("wall", "divergence") == OC.workgroup("wall-strict", "divergence") == (64, 8)
    assert OC.shapes("march", "divergence") == [(1, 1), (2, 3), (5, 4), (249, 7), (250, 8), (251, 9), (501, 17)]
    assert OC.shapes("march", "jacobian")[-1] == (505, 17)
    assert OC.shapes("tile", "jacobian") == [(1, 1), (2, 3), (5, 4), (63, 15), (64, 16), (65, 17), (129, 33), (129, 9)]
    assert OC.shapes("wall", "divergence") == [(4, 3), (7, 9), (63, 7), (64, 8), (65, 9), (129, 17), (129, 9)]
    assert OC.sweep_shape("jacobian") == (253, 21) and OC.sweep_shape("divergence") == (251, 21)
    sweep = OC.sweep_ranges()
    assert sorted(j0 % 12 for j0, _ in sweep) == list(range(12)) and all(j1 - j0 == 9 and j1 <= 21 for j0, j1 in sweep)
    # the one-row second segment starts at J0 + 8: with the first segments every phase occurs twice over
    assert sorted((j0 + 8) % 12 for j0, _ in sweep) == list(range(12))
    assert OC.row_ranges(1) == [(0, 1), (1, 1), (1, 1)] and OC.row_ranges(9) == [(0, 9), (1, 8), (2, 2)]
    assert OC.layout("minimal", "jacobian", 7) == (2, 2, 11) and OC.layout("minimal", "divergence", 7) == (3, 3, 13)
    assert OC.layout("deep", "divergence", 7) == (5, 4, 23) and OC.layout("deep", "jacobian", 250) == (5, 4, 265)
    # the tolerances in units of eps, as the conditioning cap is derived from them
    assert abs(OC.TOL[np.float32] / EPS32 - 168) < 0.5 and abs(OC.TOL[np.float64] / np.finfo(np.float64).eps - 450) < 0.5
    assert OC.CONDITIONING_CAP_EPS32 * 4 == 168
    ids = [OC.case_id(*c) for c in OC.matrix()]
    assert len(ids) == len(set(ids)) == 3 * 8 + 2 * 12
    k = OC.ring(3, 2, 2, 1)
    assert k.tolist() == [[2, 1, 1, 1, 1, 1, 2], [2, 1, 0, 0, 0, 1, 2], [2, 1, 0, 0, 0, 1, 2], [2, 1, 1, 1, 1, 1, 2]]


def test_case_parents_are_poisoned_beyond_the_reach():
    c = OC.case("jacobian", np.float32, 5, 4, "deep")
    assert (c.Hx, c.Hy, c.sy) == (5, 4, 21) and c.A.shape == (12, 21) and c.A.dtype == np.float32
    k = OC.ring(5, 4, 5, 4)
    assert np.all(np.isnan(c.A[:, 15:])) and np.all(np.isnan(c.h[:, 15:]))                     # pad columns
    assert np.array_equal(np.isnan(c.A[:, :15]), k > 2) and np.array_equal(np.isnan(c.h[:, :15]), k > 1)
    assert np.array_equal(c.A[:, :15][k <= 2], c.clean[0][k <= 2]) and not np.any(np.isnan(c.clean[0]))
    d = OC.case("divergence", np.float64, 5, 4, "minimal")
    assert not np.any(np.isnan(d.A)) and not np.any(np.isnan(d.h)) and d.sy == 11               # the halo is the reach: nothing beyond
    assert np.all(c.outputs() == OC.SENTINEL) and c.outputs().shape == (2, 12, 21)
    # inputs are those of helpers.random_case with seed 1000 Nx + Ny
    import helpers as Hh
    A, h = Hh.random_case(5, 4, 5, 4, 5004, np.float32, periodic=False)
    assert np.array_equal(A, c.clean[0]) and np.array_equal(h, c.clean[1])


INPUTS = OC.inputs()


def test_reach_is_the_headers_and_tight(oracle):
    """Every input of the matrix, all four topologies for the divergence form: the oracle on the NaN-poisoned parents is finite on the
    interior and bitwise its result on the parents without NaN; with the last ring of the reach of A or of h poisoned as well, a NaN
    reaches the interior under every topology that has a Periodic direction."""
    u = {np.float64: np.uint64, np.float32: np.uint32}
    n, loose = 0, []
    for form, dtype, Nx, Ny, lay, _ in INPUTS:
        c = OC.case(form, dtype, Nx, Ny, lay)
        args = (Nx, Ny, c.Hx, c.Hy)
        for topo in TOPOS if form == "divergence" else TOPOS[:1]:
            want = c.want(oracle, topo)
            A, h = (a[:, :Nx + 2 * c.Hx].copy() for a in (c.A, c.h))
            got = [f[c.I] for f in OC.run_oracle(oracle, form, A, h, *args, topo)]
            for w, g in zip(want, got):
                assert np.all(np.isfinite(g)), (form, dtype, Nx, Ny, lay, topo)
                assert np.array_equal(w.view(u[dtype]), g.view(u[dtype])), (form, dtype, Nx, Ny, lay, topo)
            for closer in ((1, 0), (0, 1)):
                A, h = OC.poisoned(*c.clean, *args, form, closer)
                bad = OC.run_oracle(oracle, form, A, h, *args, topo)
                if not any(np.isnan(f[c.I]).any() for f in bad):
                    loose.append((form, OC.SFX[dtype], Nx, Ny, lay, topo, closer))
            n += 1
    print(f"{n} (input, topology) pairs; not tight: {loose}")
    # (Bounded, Bounded) is the exception: with a wall on every side the reference's wall branches replace the widest interpolants, and
    # ring 3 is mostly not read at all.  Every topology with a Periodic direction reads the full reach.
    assert not [l for l in loose if l[5] != (OC.B, OC.B)], loose


def test_every_fp32_input_is_well_conditioned_row_by_row(oracle):
    """No case is skipped.  For every fp32 input, every topology it is run under and every single row: the fp32 oracle lies within
    42 eps32 of the fp64 oracle on the exactly widened inputs, relative to that row's max|F| > 0 -- a quarter of the fast budget of
    168 eps32.  (The fp64 inputs are the same fields to 6e-8.  The tiny shapes run under the periodic topology only: on a 1 x 1
    (Bounded, Bounded) grid Fx is exactly 0.)"""
    worst = (0.0, None)
    for form, dtype, Nx, Ny, lay, topos in INPUTS:
        if dtype != np.float32:
            continue
        c = OC.case(form, dtype, Nx, Ny, lay)
        for topo in topos:
            for k, (w32, w64) in enumerate(zip(c.want(oracle, topo), c.want64(oracle, topo))):
                assert w64.dtype == np.float64 and w32.dtype == np.float32
                scale = np.abs(w64).max(axis=1)
                assert np.all(scale > 0), (form, Nx, Ny, lay, topo, k)
                ratio = np.abs(w32.astype(np.float64) - w64).max(axis=1) / (EPS32 * scale)
                if ratio.max() > worst[0]:
                    worst = (float(ratio.max()), (form, Nx, Ny, lay, topo, "Fx Fy".split()[k], int(ratio.argmax())))
                assert np.all(ratio <= OC.CONDITIONING_CAP_EPS32), (form, Nx, Ny, lay, topo, k, float(ratio.max()))
    print(f"largest row error of the fp32 oracle: {worst[0]:.1f} eps32 of the row's max|F| at {worst[1]}")


def test_every_wall_call_differs_from_the_periodic_result(oracle):
    """The inequality the GPU matrix asserts per wall call holds for the oracle itself: on every non-empty row range of every wall
    shape, layout, precision and topology both components differ from the periodic result."""
    for path in ("wall", "wall-strict"):
        for _, form, dtype, lay, topo in (m for m in OC.matrix() if m[0] == path):
            for Nx, Ny, (j0, j1), _ in OC.calls(path, form):
                c = OC.case(form, dtype, Nx, Ny, lay)
                for w, p in zip(c.want(oracle, topo), c.want(oracle)):
                    assert j1 == j0 or not np.array_equal(w[j0:j1], p[j0:j1]), (dtype, lay, topo, Nx, Ny, j0, j1)


@pytest.mark.parametrize("dtype", OC.DTYPES)
def test_check_call_sees_what_it_must(oracle, dtype):
    """check_call on made-up results: the oracle's own values pass; one stray store, one wrong row, a NaN, a changed input fail."""
    c = OC.case("divergence", dtype, 7, 9, "deep")
    topo, rows = (OC.B, OC.P), (1, 8)
    good = c.outputs()
    R = OC.written(rows, c.Hy, c.Hx, c.Nx)
    for k in range(2):
        good[k][R] = c.want(oracle, topo)[k][1:8]
    for path in ("wall", "wall-strict"):
        assert OC.check_call(c, oracle, path, topo, rows, good, c.A, c.h) == []
        stray = good.copy()
        stray[1, c.Hy, c.Hx + 2] = 0.5          # row 0 is outside the range
        assert any("sentinel" in m for m in OC.check_call(c, oracle, path, topo, rows, stray, c.A, c.h))
        pad = good.copy()
        pad[0, c.Hy + 3, c.sy - 1] = 0.5
        assert any("sentinel" in m for m in OC.check_call(c, oracle, path, topo, rows, pad, c.A, c.h))
        off = good.copy()
        off[0][R] = c.want(oracle, topo)[0][0:7]
        assert OC.check_call(c, oracle, path, topo, rows, off, c.A, c.h)
        nan = good.copy()
        nan[1, c.Hy + 4, c.Hx] = np.nan
        assert any("finite" in m for m in OC.check_call(c, oracle, path, topo, rows, nan, c.A, c.h))
        A2 = c.A.copy()
        A2[0, 0] = 1.0                           # a NaN of the poison replaced
        assert any("A was changed" in m for m in OC.check_call(c, oracle, path, topo, rows, good, A2, c.h))
    assert OC.check_call(c, oracle, "wall", topo, (2, 2), c.outputs(), c.A, c.h) == []
    worst = {}
    OC.check_call(c, oracle, "wall", topo, rows, good, c.A, c.h, worst)
    assert list(worst) == [f"wall/divergence/{OC.SFX[dtype]}"] and worst[f"wall/divergence/{OC.SFX[dtype]}"] <= 0.25
