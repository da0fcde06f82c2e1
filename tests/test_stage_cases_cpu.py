"""Pins of tests/stage_cases.py, the reference of the stage matrices (tests/test_stage_matrix_gpu.py,
tests/test_tile_stage_matrix_gpu.py), on the CPU: its substep formulas composed into a whole RK3 step reproduce the oracle's time_step
in all three operand forms, it marks the outputs a call must not write, its time step keeps the new state a sharp witness of the
tendencies, and every width and row count of the matrix has the layout it is there for (the launch planner is host code:
swmhd_tendency_launch_geometry answers without a GPU, with the 256 compute units of an MI355X).  Of the tile matrix: its shapes have
the ragged last tiles they were chosen for and the tile height of their path by the planner's answer, the strict reference composed
into a step is the oracle's time_step bit for bit, and the Bounded reference differs from the periodic one exactly inside the wall
buffers.  No test here needs a GPU; the layout tests need the BUILT libswmhd.so (the `swmhd` fixture: build() first), the others only
the CPU oracle."""
import numpy as np
import pytest

import helpers as Hh
import stage_cases as SC
import tracer_cases as TC

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


# ---------------------------------------------------------------------------------------------------------------------------------
# the tile matrix
# ---------------------------------------------------------------------------------------------------------------------------------
def _last(n, t):
    return n - (-(-n // t) - 1) * t


def test_the_tile_matrix_has_its_ragged_classes():
    """Last tile column and last tile row of every shape, computed here for both tile heights: one-column and one-row last tiles
    (4- and 8-row tiles), exactly full and nearly full ones, a one-tile-wide domain of Nx = Hx, a row range that starts off a tile
    multiple, the single-direction WRAP flags and the wall shapes whose three-cell boundary buffers straddle, end on and miss a tile
    edge; every path, form and precision the matrix promises."""
    cases = list(SC.tile_matrix())
    assert len({SC.tile_case_id(*c) for c in cases}) == len(cases)
    by_path = {p: [c for c in cases if c[0] == p] for p in SC.PATHS if p != "march"}
    assert all(by_path.values())
    XY = SC.WRAP_X | SC.WRAP_Y
    for path in ("tile4", "strict"):
        cs = by_path[path]
        shapes = {(Nx, Ny if rows is None else rows[1] - rows[0]) for _, Nx, Ny, rows, *_ in cs}
        assert {Nx for Nx, n in shapes if n == 9} == {3, 7, 63, 64, 65, 129}
        for W in (65, 129):
            assert {n for Nx, n in shapes if Nx == W} >= {3, 4, 5, 8, 9, 31}
        assert {_last(Nx, 64) for Nx, _ in shapes} == {3, 7, 63, 64, 1}                 # last tile column
        assert sum(1 for Nx, _ in shapes if -(-Nx // 64) == 3 and _last(Nx, 64) == 1)   # three tile columns, the last of one
        assert {_last(n, 4) for _, n in shapes} == {1, 3, 4} and {5, 9} <= {n for _, n in shapes if _last(n, 4) == 1}
        assert {_last(n, 8) for _, n in shapes} == {1, 3, 4, 5, 7, 8} and 9 in {n for _, n in shapes if _last(n, 8) == 1}
        assert any(rows == SC.PARTIAL and Ny == 33 and Nx == 129 and rows[0] % 8 and rows[0] % 4 for _, Nx, Ny, rows, *_ in cs)
        for c in cs:
            assert c[8] == (SC.P, SC.P)
        groups = {}
        for _, Nx, Ny, rows, form, lor, dtype, flags, _t in cs:
            groups.setdefault((Nx, Ny, rows), set()).add((form, lor, np.dtype(dtype).name, flags))
        for shape, g in groups.items():
            want = {0, XY} | ({SC.WRAP_X, SC.WRAP_Y} if shape == (65, 9, None) else set())
            assert g == {(f, l, d, w) for f, l in SC.FORMS for d in ("float64", "float32") for w in want}, shape
    t8 = by_path["tile8"]
    assert {(c[1], c[2], c[3]) for c in t8} == {(2579, 129, None)} and 2579 * 129 >= 330000 > 2579 * 127
    assert (-(-2579 // 64), _last(2579, 64), -(-129 // 8), _last(129, 8)) == (41, 19, 17, 1)
    assert {(c[4], c[5], np.dtype(c[6]).name, c[7]) for c in t8} == {(f, l, d, w) for f, l in SC.FORMS for d in ("float64", "float32") for w in (0, XY)}
    for path in ("wall", "wall-strict"):
        cs = by_path[path]
        for topo in SC.WALL_TOPOS:
            mine = [c for c in cs if c[8] == topo]
            assert {(c[1], c[2], c[3]) for c in mine} == {(65, 9, None), (67, 11, None), (64, 8, None), (7, 8, None), (129, 31, None),
                                                          (129, 33, SC.PARTIAL)}
            assert {(c[4], c[5]) for c in mine} == {(1, 1), (0, 2), (0, 0)} and {np.dtype(c[6]).name for c in mine} == {"float64", "float32"}
            wrapped = {(c[1], c[2], c[7]) for c in mine if c[7]}
            assert wrapped == {(SC.P, SC.B): {(65, 9, SC.WRAP_X)}, (SC.B, SC.P): {(65, 9, SC.WRAP_Y)}, (SC.B, SC.B): set()}[topo]
        # last tile column | row of 1 and 3 cells (a tile edge 1 and 3 cells from the east | north wall: inside its boundary buffer and at
        # its start), a full last tile (the buffer ends on the edge), one partial tile shared by both walls, several tiles a side
        assert [_last(Nx, 64) for Nx, _ in SC.WALL_SHAPES] == [1, 3, 64, 7, 1] and [-(-Nx // 64) for Nx, _ in SC.WALL_SHAPES] == [2, 2, 1, 1, 3]
        assert [_last(Ny, 8) for _, Ny in SC.WALL_SHAPES] == [1, 3, 8, 8, 7] and [-(-Ny // 8) for _, Ny in SC.WALL_SHAPES] == [2, 2, 1, 1, 4]
    # every path makes all 19 calls; the strict and wall paths are refused the five fast-only forms
    assert all(SC.PATHS[p]["refused"] == (() if p in ("march", "tile4", "tile8") else ("P2g", "P3n", "A1", "A2", "A2a")) for p in SC.PATHS)


def test_every_shape_of_the_tile_matrix_has_its_layout(swmhd):
    """The planner's own answer (swmhd_tendency_launch_geometry with SWMHD_TILE_KERNEL and the rows of the launch) puts every tile4
    shape on 64 x 4 tiles and the tile8 shape, just above the threshold, on 64 x 8; strict launches have 64 x 8 tiles at every size;
    the wall shapes lie below the hybrid thresholds (stage_cases.wall_tiles, inferred).  A partial row range of the tile8 shape would
    fall back to 64 x 4 tiles, which is why that path runs whole ranges only.  (The GPU test asserts the same on the device.)"""
    L = swmhd._lib
    heights = {}
    for path, Nx, Ny, rows, form, lor, dtype, flags, topo in SC.tile_matrix():
        nrows = Ny if rows is None else rows[1] - rows[0]
        line = SC.check_layout(L, Nx, nrows, form, dtype, flags, path=path)
        geo = L.tendency_launch_geometry(Nx, nrows, form, np.dtype(dtype).itemsize, SC.TILE_KERNEL | (SC.STRICT if SC.PATHS[path]["strict"] else 0) | flags)
        heights.setdefault(path, set()).add(geo["rows_per_segment"])
        assert f"{-(-Nx // 64)} tile columns, last {_last(Nx, 64)} wide" in line
        if path in ("tile4", "wall", "wall-strict"):
            assert Nx * nrows < 330000
    assert heights["tile4"] == {4} and heights["tile8"] == {8} and heights["strict"] == {8} and heights["wall-strict"] == {8}
    assert heights["wall"] == {4}        # what the query, which knows no topology, says of these sizes: the wall kernel's 8 rows are inferred
    Nx, Ny = SC.TILE8_SHAPE
    for form in (0, 1):
        for elem in (4, 8):
            assert L.tendency_launch_geometry(Nx, Ny - 2, form, elem, SC.TILE_KERNEL)["rows_per_segment"] == 4
            assert L.tendency_launch_geometry(Nx, SC.PARTIAL[1] - SC.PARTIAL[0], form, elem, SC.TILE_KERNEL)["rows_per_segment"] == 4
            assert L.tendency_launch_geometry(Nx, Ny, form, elem, SC.TILE_KERNEL)["rows_per_segment"] == 8


@pytest.mark.parametrize("topo", [(SC.P, SC.P), (SC.P, SC.B), (SC.B, SC.B)])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("form,lor", [(1, 1), (0, 2)])
def test_composed_strict_stages_are_the_oracle_time_step(oracle, form, lor, dtype, topo):
    """S1g, S2g and S3n of reference_stage_strict with the oracle's halo fills between them against oracle.time_step on a 40 x 33 grid,
    bit for bit in the precision of the call: the strict reference restates neither the tendencies nor the substep differently from
    the oracle, for periodic and Bounded grids (with the gradient condition on A)."""
    data = SC.StageData(oracle, Nx, Ny, form, lor, dtype, seed=13, topo=topo)
    dt = float(np.dtype(dtype).type(1e-4))
    want = [a.copy() for a in data.q]
    oracle.time_step(*want, Nx, Ny, H, H, data.dx, data.dy, dt, form, lor, data.grav, data.fcor, topo=topo, gradA=TC.grad_A(topo))

    def embed(interior):
        a = np.full_like(data.q[0], SC.SENTINEL)
        Hh.interior(a, Nx, Ny, H, H)[...] = interior
        return a
    for variant, coeffs in (("S1g", (G1, 0.0)), ("S2g", (G2, Z2)), ("S3n", (G3, Z3))):
        ref = SC.reference_stage_strict(data, variant, coeffs, dt)
        assert all(a.dtype == np.dtype(dtype) for a in ref["qnew"])
        if ref["Gn"] is not SC.KEEP:
            data.aux = [embed(g) for g in ref["Gn"]]
        data.q = TC.fill_state(oracle, [embed(x) for x in ref["qnew"]], Nx, Ny, topo, TC.grad_A(topo), data.dx, data.dy)
        data._G_strict = None
    assert ref["Gn"] is SC.KEEP
    for got, w in zip(data.q, want):
        assert np.array_equal(Hh.interior(got, Nx, Ny, H, H), Hh.interior(w, Nx, Ny, H, H))
    # a row range cuts every output, and T has no new state
    part = SC.reference_stage_strict(data, "T", (0.0, 0.0), 0.0, rows=SC.PARTIAL)
    assert part["qnew"] is None and all(g.shape == (SC.PARTIAL[1] - SC.PARTIAL[0], Nx) for g in part["Gn"])


@pytest.mark.parametrize("form,lor", SC.WALL_FORMS)
def test_the_bounded_reference_differs_exactly_inside_the_wall_buffers(oracle, form, lor):
    """Every Bounded shape and topology of the tile matrix: the oracle's Bounded tendencies of the boundary-condition-filled inputs
    differ from the periodic ones of the same interior inside the buffer of every wall (7 cells: test_bounded_oracle) and are equal bit
    for bit outside.  Control: a reference that took no wall branch -- the periodic oracle -- is caught."""
    for Nx_, Ny_, rows, topo, _flags in SC.wall_shape_groups():
        for dtype in SC.DTYPES:
            data = SC.StageData(oracle, Nx_, Ny_, form, lor, dtype, topo=topo)
            assert data.wall_failures == [], (Nx_, Ny_, topo, dtype, data.wall_failures)
            assert all(np.isfinite(g).all() for g in data.G)
            buffers = SC.wall_buffers(Nx_, Ny_, topo)
            assert set(buffers) == ({"west", "east"} if topo[0] == SC.B else set()) | ({"south", "north"} if topo[1] == SC.B else set())
            q64 = [a.astype(np.float64) for a in data.q]
            qp = [oracle.fill_halo_periodic(a.copy(), Nx_, Ny_, H, H) for a in q64]
            data.G = [Hh.interior(g, Nx_, Ny_, H, H).copy() for g in oracle.tendencies(*qp, Nx_, Ny_, H, H, data.dx, data.dy, form, lor, data.grav, data.fcor)]
            assert len(SC.wall_buffer_failures(oracle, data, q64)) == len(buffers)
    far = SC.wall_buffers(129, 31, (SC.B, SC.B))
    assert far["west"].sum() == far["east"].sum() == 7 * 31 and far["south"].sum() == far["north"].sum() == 7 * 129
    assert not (far["west"] | far["east"] | far["south"] | far["north"])[7:24, 7:122].any()
