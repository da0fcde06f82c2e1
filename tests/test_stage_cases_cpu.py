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


# ---------------------------------------------------------------------------------------------------------------------------------
# the ensemble matrix
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_ensemble_matrix_has_its_paths_shapes_and_workgroup_counts():
    """Every (formulation x forcing, precision) on every ensemble path; the shapes the matrix is there for with flags 0 and
    WRAP_X | WRAP_Y, the single-direction flags once at 65 x 9, one dense layout beside the pitched ones; 1, 3 or 5 members, chosen so
    that the launches of both tile heights have workgroup counts that are no multiple of 8, below and above 8; ids that name path,
    members, layout, shape and flags; the call forms every path refuses."""
    cases = list(SC.ens_matrix())
    ids = [SC.ens_case_id(*c) for c in cases]
    assert len(set(ids)) == len(ids)
    assert "ens4-m3-pitched-65x9-vi-lor1-f64-wrapXY" in ids and "par-strict-m3-dense-65x9-cons-lor2-f32-wrapXY" in ids
    assert "ens8-m2-pitched-2579x129-cons-lor0-f32-nowrap" in ids
    XY = SC.WRAP_X | SC.WRAP_Y
    every = {(f, l, d) for f, l in SC.FORMS for d in ("float64", "float32")}
    for path in SC.ENS_PATHS:
        mine = [c for c in cases if c[0] == path]
        assert {(c[4], c[5], np.dtype(c[6]).name) for c in mine} == every, path
        groups = {}
        for _, Nx_, Ny_, members, form, lor, dtype, flags, dense in mine:
            groups.setdefault((Nx_, Ny_, members), set()).add((form, lor, np.dtype(dtype).name, flags, dense))
        if path == "ens8":
            assert set(groups) == {SC.TILE8_SHAPE + (2,)}
            assert groups[SC.TILE8_SHAPE + (2,)] == {e + (w, False) for e in every for w in (0, XY)}
            # four families of four fields of both members, pitched, in fp64: under 50 MB a family group
            assert 4 * 2 * SC.ens_layout(*SC.TILE8_SHAPE, False)[1] * 8 < 50e6
            continue
        assert set(groups) == {(3, 9, 5), (65, 9, 3), (129, 9, 1), (65, 5, 1), (129, 31, 3)}
        for (Nx_, Ny_, members), g in groups.items():
            lay = {(0, False), (XY, False)} | ({(SC.WRAP_X, False), (SC.WRAP_Y, False), (XY, True)} if (Nx_, Ny_) == (65, 9) else set())
            assert g == {e + l for e in every for l in lay}, (path, Nx_, Ny_)
            assert members in (1, 3, 5)
        counts = {SC.ens_workgroups(path, *k) for k in groups}
        odd = {n for n in counts if n % 8}
        assert any(n < 8 for n in odd) and any(n > 8 for n in odd), (path, counts)
        assert counts == ({15, 18, 9, 4, 72} if SC.ENS_PATHS[path]["ty"] == 4 else {10, 12, 6, 2, 36})
    # widths: Nx = Hx, a last tile of one column behind one and behind two full tiles; rows: last tile rows of one row (4- and 8-row
    # tiles at 9 and 5 | 9 rows) and of 3 | 7 rows
    assert [_last(Nx_, 64) for Nx_, _ in SC.ENS_SHAPES] == [3, 1, 1, 1, 1] and [_last(n, 4) for _, n in SC.ENS_SHAPES] == [1, 1, 1, 1, 3]
    assert [_last(n, 8) for _, n in SC.ENS_SHAPES] == [1, 1, 1, 5, 7]
    assert SC.ens_layout(65, 9, False) == (65 + 6 + 5, 15 * 76 + 37) and SC.ens_layout(65, 9, True) == (71, 15 * 71)
    assert SC.ens_workgroups("ens8", *SC.TILE8_SHAPE, 2) == 41 * 17 * 2 and (41 * 17 * 2) % 8
    # T has no ensemble form; the previous-state forms are refused everywhere, the anchor forms by the strict paths
    assert len(SC.ens_calls()) == 18 and all(v != "T" for v, _ in SC.ens_calls())
    for path, p in SC.ENS_PATHS.items():
        assert p["refused"] == (("P2g", "P3n", "A1", "A2", "A2a") if p["strict"] else ("P2g", "P3n")), path
    # the forced-layout children: 65 x 9 and 129 x 31 with 3 members, (1, 1) and (0, 2), both precisions
    for name, cfg in SC.ENS_FORCED.items():
        fc = SC.ens_forced_cases(name)
        assert {(c[1], c[2], c[3]) for c in fc} == {(65, 9, 3), (129, 31, 3)} and {c[0] for c in fc} == set(cfg["paths"])
        assert {(c[4], c[5], np.dtype(c[6]).name) for c in fc} == {(1, 1, "float64"), (1, 1, "float32"), (0, 2, "float64"), (0, 2, "float32")}
    # with 64 x 8 tiles forced: one-row and one-column last tiles of that body
    assert (_last(9, 8), _last(65, 64), _last(129, 64)) == (1, 1, 1)


def test_every_shape_of_the_ensemble_matrix_has_its_layout(swmhd):
    """The planner's answer for a single grid of the member's shape: 64 x 4 tiles on ens4 and par4, 64 x 8 on ens8 and the strict paths."""
    heights = {}
    for path, Nx_, Ny_, members, form, lor, dtype, flags, dense in SC.ens_matrix():
        line = SC.check_ens_layout(swmhd._lib, path, Nx_, Ny_, members, form, dtype, flags)
        assert f"member in blockIdx.x, grid {SC.ens_workgroups(path, Nx_, Ny_, members)} x 1" in line
        heights.setdefault(path, set()).add(int(line.split(" tile rows of ")[1].split(",")[0]))
        assert f"{-(-Nx_ // 64)} tile columns, last {_last(Nx_, 64)} wide" in line
    assert heights == {"ens4": {4}, "par4": {4}, "ens8": {8}, "ens-strict": {8}, "par-strict": {8}}
    # without the knobs in the environment the library reports the default layout: a forced one is not accepted
    for forced in (dict(ty=8), dict(member_map=2)):
        with pytest.raises(AssertionError):
            SC.check_ens_layout(swmhd._lib, "ens4", 65, 9, 3, 1, np.float64, 0, **forced)


def test_the_ensemble_knobs_are_read_back(swmhd):
    """swmhd_ensemble_launch_geometry in fresh processes (the knobs are read once): SWMHD_ENS_MAP=2 puts the member in blockIdx.y,
    SWMHD_ENS_RY=2 gives fast periodic members 64 x 8 tiles and leaves Bounded members alone; bad arguments are refused."""
    import json
    import os
    import subprocess
    import sys
    code = ("import json, sys; sys.path.insert(0, sys.argv[1]); import swmhd_amd as S; L = S._lib; "
            "print(json.dumps([L.ensemble_launch_geometry(129, 31, 1, 3, 8, L.TILE_KERNEL), L.ensemble_launch_geometry(129, 31, 1, 3, 8, L.BOUNDED_Y)]))")
    got = {}
    for name, env in (("default", {}), ("map2", {"SWMHD_ENS_MAP": "2"}), ("ry2", {"SWMHD_ENS_RY": "2"}), ("ry1", {"SWMHD_ENS_RY": "1"})):
        e = {k: v for k, v in os.environ.items() if k not in ("SWMHD_ENS_MAP", "SWMHD_ENS_RY")}
        e.update(env)
        r = subprocess.run([sys.executable, "-c", code, SC.ROOT], env=e, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        got[name] = json.loads(r.stdout)
    base = dict(kind=1, threads=256, tile_columns=3, tile_rows=8, rows_per_tile=4, member_map=1, grid_x=72, grid_y=1)
    wall = dict(base, tile_rows=4, rows_per_tile=8, grid_x=36)
    assert got["default"] == [base, wall] == got["ry1"]
    assert got["map2"] == [dict(base, member_map=2, grid_x=24, grid_y=3), dict(wall, member_map=2, grid_x=12, grid_y=3)]
    assert got["ry2"] == [wall, wall]
    f, out = swmhd._lib.lib().swmhd_ensemble_launch_geometry, (__import__("ctypes").c_int * 8)()
    assert f(129, 31, 1, 8, 0, 3, out) == 0 and f(129, 31, 1, 8, 0, 0, out) == 1 and f(129, 31, 1, 8, 0, 65536, out) == 1
    assert f(129, 31, 1, 8, swmhd._lib.MARCH_KERNEL, 3, out) == 1 and f(129, 31, 1, 8, swmhd._lib.BOUNDED_X | swmhd._lib.WRAP_X, 3, out) == 1
    assert f(129, 31, 1, 6, 0, 3, out) == 1 and f(129, 31, 2, 8, 0, 3, out) == 1 and f(129, 31, 1, 8, 0, 3, None) == 1


def test_the_default_stage_data_is_unchanged_by_the_member_arguments(oracle):
    """grav = fcor = None is the StageData every other matrix uses, bit for bit: the same fields, constants, tendencies, scales and dt;
    a member with its own g and f differs in its tendencies and forms its scales with them."""
    a = SC.StageData(oracle, 20, 9, 1, 1, np.float32, seed=3)
    b = SC.StageData(oracle, 20, 9, 1, 1, np.float32, seed=3, grav=None, fcor=None)
    assert (a.grav, a.fcor) == (float(np.float32(SC.GRAV)), float(np.float32(SC.FCOR))) == (b.grav, b.fcor)
    for x, y in zip(a.q + a.aux + a.G, b.q + b.aux + b.G):
        assert SC._same_bits(x, y)
    assert a.scales == b.scales and a.Gmax == b.Gmax and a.dt(0.37) == b.dt(0.37)
    c = SC.StageData(oracle, 20, 9, 1, 1, np.float32, seed=3, grav=1.0, fcor=-0.5)
    assert (c.grav, c.fcor) == (1.0, -0.5) and all(SC._same_bits(x, y) for x, y in zip(a.q, c.q))
    assert not np.array_equal(a.G[0], c.G[0]) and c.scales[0] <= a.scales[0]
    q64 = [x.astype(np.float64) for x in a.q]
    assert Hh.term_scales("VectorInvariant", q64, a.dx, a.dy, 0.0, g=1.0, f=0.5)[0] < Hh.term_scales("VectorInvariant", q64, a.dx, a.dy, 0.0)[0]
    assert Hh.term_scales("Conservative", q64, a.dx, a.dy, 0.0, g=Hh.G, f=Hh.F) == Hh.term_scales("Conservative", q64, a.dx, a.dy, 0.0)


def _ens_case(oracle, path, variant, cset, Nx_=65, Ny_=9, members=3, form=1, lor=1, dtype=np.float64, flags=SC.WRAP_X, dense=False):
    data = SC.ens_members(oracle, Nx_, Ny_, members, form, lor, dtype, SC.ENS_PATHS[path]["par"])
    dts = SC.ens_dts(data, variant, cset, SC.ENS_PATHS[path]["par"])
    before = SC.ens_buffers(data, variant, flags, dense)
    expected = SC.ens_expected(oracle, data, variant, cset, dts, SC.ENS_PATHS[path]["strict"])
    return data, dts, before, expected


def test_ensemble_members_are_distinct_and_their_buffers_poisoned(oracle):
    """No two members share a field or an operand; par members have pairwise distinct g and f (two f negative) and their own dt;
    inputs hold NaN in the row padding, the member gaps and the halos of a wrapped direction, outputs the sentinel everywhere."""
    data, dts, before, _ = _ens_case(oracle, "par4", "S2g", "generic")
    fields = [a for d in data for a in d.q + d.aux]
    assert all(not np.array_equal(fields[i], fields[j]) for i in range(len(fields)) for j in range(i))
    for dtype in SC.DTYPES:
        g, f = [float(dtype(x)) for x in SC.PAR_G], [float(dtype(x)) for x in SC.PAR_F]
        assert len(set(g)) == len(set(f)) == 5 and sum(x < 0 for x in f) == 2
    assert [(d.grav, d.fcor) for d in data] == list(zip(SC.PAR_G, SC.PAR_F))[:3] and len(set(dts)) == 3
    shared = SC.ens_dts(SC.ens_members(oracle, 65, 9, 3, 1, 1, np.float64, False), "S2g", "generic", False)
    assert len(set(shared)) == 1
    reg = SC.ens_regions(65, 9, 3, False)
    assert {int((reg == r).sum()) for r in (SC.GAP,)} == {3 * 37} and int((reg == SC.PADDING).sum()) == 3 * 15 * 5
    assert int((reg == SC.INTERIOR).sum()) == 3 * 65 * 9
    for f in range(4):
        assert np.isnan(before["q"][f][reg >= SC.PADDING]).all() and np.isnan(before["operand"][f][reg >= SC.PADDING]).all()
        assert (before["operand"][f][reg == SC.HALO] == SC.SENTINEL).all() and np.isfinite(before["q"][f][reg == SC.INTERIOR]).all()
        assert (before["qnew"][f] == SC.SENTINEL).all() and (before["Gn"][f] == SC.SENTINEL).all()
        for m in range(3):
            a = SC.ens_view(before["q"][f], m, 65, 9, False)
            assert np.isnan(a[:, :H]).all() and np.isnan(a[:, H + 65:]).all() and np.isfinite(a[:, H:H + 65]).all()
    # the aliases of the call forms

    b = SC.ens_buffers(data, "A2a", 0, True)
    assert b["Gn"] is b["operand"] and SC.ens_copy(b)["Gn"] is not b["Gn"] and len(b["q"][0]) == 3 * 15 * 71
    c = SC.ens_copy(b)
    assert c["Gn"] is c["operand"]


@pytest.mark.parametrize("strict", [False, True], ids=["fast", "strict"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_a_table_of_equal_rows_is_the_scalar_reference(oracle, strict, dtype):
    """Members formed with one row of the parameter table (that of member 0) and one dt: their reference is bitwise the reference of
    the scalar call's members, in both the fast and the strict form."""
    scalar = SC.ens_members(oracle, 20, 9, 3, 0, 2, dtype, False)
    table = SC.ens_members(oracle, 20, 9, 3, 0, 2, dtype, True, row=0)
    assert all((d.grav, d.fcor) == (scalar[0].grav, scalar[0].fcor) for d in table)
    for variant, cset in (("S1g", "rk3"), ("S2g", "generic")):
        dts = SC.ens_dts(scalar, variant, cset, False)
        for (ra, ba), (rb, bb) in zip(SC.ens_expected(oracle, scalar, variant, cset, dts, strict), SC.ens_expected(oracle, table, variant, cset, dts, strict)):
            for name in ("qnew", "Gn"):
                assert all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(ra[name], rb[name]))     # (no NaN, no -0 in these)
            assert strict or all(abs(x - y) <= 1e-6 * x for x, y in zip(ba["qnew"] + ba["Gn"], bb["qnew"] + bb["Gn"]))


@pytest.mark.parametrize("path", ["ens4", "ens-strict", "par4", "par-strict"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_the_ensemble_check_catches_the_errors_it_exists_for(oracle, path, dtype):
    """check_ens_outputs on fabricated "kernel outputs" built from the reference: the faithful one passes; two members' qnew swapped,
    member 0's Gm used for every member, member 0's (g, f, dt) used for every member (par paths), one cell written in a member gap, one
    in the row padding, one in a halo and a written Gn that had to keep its sentinel each give at least one failure line.  No kernel
    runs."""
    par, strict = SC.ENS_PATHS[path]["par"], SC.ENS_PATHS[path]["strict"]
    for variant, cset in (("S2g", "generic"), ("S3n", "rk3"), ("S1g", "rk3")):
        data, dts, before, expected = _ens_case(oracle, path, variant, cset, dtype=dtype)
        check = lambda after, exp=expected: SC.check_ens_outputs(data, variant, SC.WRAP_X, False, before, after, exp)[0]
        good = SC.ens_fabricate(data, variant, False, before, expected)
        assert check(good) == [], (variant, check(good))
        assert check(before), "a kernel that wrote nothing passes"
        # two members' qnew swapped
        bad = SC.ens_copy(good)
        for f in range(4):
            x, y = SC.ens_view(bad["qnew"][f], 0, 65, 9, False), SC.ens_view(bad["qnew"][f], 2, 65, 9, False)
            keep = x.copy(); x[...] = y; y[...] = keep
        assert any("member 0 qnew" in m for m in check(bad)) and any("member 2 qnew" in m for m in check(bad))
        if SC.VARIANTS[variant]["operand"]:
            # member 0's Gm for every member: the reference of members whose operand is member 0's
            import copy
            wrong = [copy.copy(d) for d in data]
            for d in wrong:
                d.aux, d._ens_ref = data[0].aux, {}
            bad = SC.ens_fabricate(data, variant, False, before, SC.ens_expected(oracle, wrong, variant, cset, dts, strict))
            lines = check(bad)
            assert any("member 1 qnew" in m for m in lines) and any("member 2 qnew" in m for m in lines) and not any("member 0" in m for m in lines)
        if par:
            # member 0's row of the table for every member
            wrong = SC.ens_members(oracle, 65, 9, 3, 1, 1, dtype, True, row=0)
            bad = SC.ens_fabricate(data, variant, False, before, SC.ens_expected(oracle, wrong, variant, cset, [dts[0]] * 3, strict))
            lines = check(bad)
            assert any("member 1" in m for m in lines) and any("member 2" in m for m in lines) and not any("member 0" in m for m in lines)
            # ... and only its dt, or only its g and f
            bad = SC.ens_fabricate(data, variant, False, before, SC.ens_expected(oracle, data, variant, cset, [dts[0]] * 3, strict))
            assert any("member 1 qnew" in m for m in check(bad))
            bad = SC.ens_fabricate(data, variant, False, before, SC.ens_expected(oracle, wrong, variant, cset, dts, strict))
            assert any("member 2" in m for m in check(bad))
        # one cell outside the interiors
        reg = SC.ens_regions(65, 9, 3, False)
        for region, what in ((SC.GAP, "member gap"), (SC.PADDING, "row padding"), (SC.HALO, "halo")):
            bad = SC.ens_copy(good)
            bad["qnew"][1][np.flatnonzero(reg == region)[-1]] = 1.0
            assert check(bad) == [f"qnew[1]: 1 cells of the {what} written"]
        # an input or an operand changed, an output that had to stay
        bad = SC.ens_copy(good)
        bad["q"][2][np.flatnonzero(reg == SC.GAP)[0]] = 0.0
        assert check(bad) == ["input field 2 was changed"]
        if variant == "S3n":
            bad = SC.ens_copy(good)
            bad["Gn"][0][np.flatnonzero(reg == SC.INTERIOR)[5]] = 0.0
            assert check(bad) == ["Gn[0] must keep its sentinel: 1 cells written"]
        # the bitwise single-grid promise: a last-bit difference in one cell of one member
        singles = [{k: [SC.ens_view(a, m, 65, 9, False).copy() for a in good[k]] for k in ("qnew", "Gn")} for m in range(3)]
        assert SC.check_ens_outputs(data, variant, SC.WRAP_X, False, before, good, expected, singles)[0] == []
        cell = Hh.interior(singles[1]["qnew"][3], 65, 9, H, H)
        cell[4, 64] = np.nextafter(cell[4, 64], dtype(np.inf))
        lines = SC.check_ens_outputs(data, variant, SC.WRAP_X, False, before, good, expected, singles)[0]
        assert lines == ["member 1 qnew[3]: 1 cells differ from the single-grid call on the member alone"]
    # a refused call that wrote something; inputs whose wrapped halos were not poisoned
    data, dts, before, expected = _ens_case(oracle, path, "S1g", "rk3", dtype=dtype)
    after = SC.ens_copy(before)
    assert SC.check_ens_refusal(before, after) == []
    after["Gn"][3][0] = 2.0
    assert SC.check_ens_refusal(before, after) == ["refused call changed Gn[3]"]
    unpoisoned = SC.ens_buffers(data, "S1g", 0, False)
    lines = SC.check_ens_outputs(data, "S1g", SC.WRAP_X, False, unpoisoned, SC.ens_fabricate(data, "S1g", False, unpoisoned, expected), expected)[0]
    assert len(lines) == 12 and all("not NaN on entry" in m for m in lines)
