"""Pins of tests/tracer_stage_cases.py, the reference of the tracer stage matrix (tests/test_tracer_stage_matrix_gpu.py), on the CPU:
the case list, the tiles every shape exists for, the longdouble update against tracer_cases.substep, the bounds against
stage_cases.stage_bounds, the wall-buffer condition of every Bounded case, and the checker itself on fabricated kernel outputs -- the
reference with one defect each.  No test here needs a GPU; all of them need the CPU oracle."""
import types

import numpy as np
import pytest

import helpers as Hh
import stage_cases as SC
import tracer_cases as TC
import tracer_stage_cases as TS

H, P, B = TS.H, TS.P, TS.B
PERIODIC = ["3x3", "7x9", "63x15", "64x16", "65x17", "129x9", "3x17", "129x16", "64x3", "7x15"]
WALLS = ["65x17", "67x19", "64x16", "7x8", "129x31"]


def test_the_case_list():
    """280 cases: the ten periodic shapes on the fast path with and without WRAP, the five wall shapes on both wall paths over three
    topologies (no WRAP run where both directions are Bounded), both formulations and precisions everywhere; 23 calls per row range."""
    cases = list(TS.matrix())
    ids = [TS.case_id(*c) for c in cases]
    want = {f"fast-{s}-{f}-{p}-{w}" for s in PERIODIC for f in ("vi", "cons") for p in ("f64", "f32") for w in ("wrap", "filled")}
    want |= {f"{path}-{t}-{s}-{f}-{p}-{w}" for path in ("wall", "wall-strict") for t in ("PB", "BP", "BB") for s in WALLS
             for f in ("vi", "cons") for p in ("f64", "f32") for w in (("filled",) if t == "BB" else ("wrap", "filled"))}
    assert len(ids) == len(set(ids)) == 280 and set(ids) == want
    assert [f"{Nx}x{Ny}" for Nx, Ny in TC.STAGE_SHAPES] == PERIODIC and [f"{Nx}x{Ny}" for Nx, Ny in TS.WALL_SHAPES] == WALLS
    assert TS.WALL_SHAPES == [(TS.TX + 1, TS.TY + 1), (TS.TX + 3, TS.TY + 3), (TS.TX, TS.TY), (7, 8), (2 * TS.TX + 1, 2 * TS.TY - 1)]
    assert all(Nx <= 129 and Ny <= 33 for _, Nx, Ny, *_ in cases)
    calls = TS.calls()
    assert len(calls) == 23 and calls[:19] == [(v, c, 3) for v, c in SC.calls()]
    assert calls[19:] == [("S2g", "rk3", 1), ("S2g", "rk3", 8), ("S2g", "generic", 1), ("S2g", "generic", 8)]
    assert {p: TS.PATHS[p]["refused"] for p in TS.PATHS} == {"fast": ("P2g", "P3n"), "wall": ("P2g", "P3n", "A1", "A2", "A2a"),
                                                             "wall-strict": ("P2g", "P3n", "A1", "A2", "A2a")}
    assert TS.row_ranges(3) == [None] and TS.row_ranges(5) == [None] and TS.row_ranges(6) == [None, (2, 3)] and TS.row_ranges(31) == [None, (2, 28)]
    assert TS.wrap_flags((P, B), True) == SC.WRAP_X and TS.wrap_flags((B, P), True) == SC.WRAP_Y and TS.wrap_flags((B, B), True) == 0
    assert TS.wrap_flags((P, P), True) == SC.WRAP_X | SC.WRAP_Y and TS.wrap_flags((P, P), False) == 0


def test_every_shape_has_the_tiles_it_exists_for():
    """tracer_tiles' arithmetic (launch_plan.hpp, restated from TX, TY = 64, 16): one partial tile, one exactly full tile, last tiles
    of one column and of one row behind one and two full ones; the wall shapes put a tile edge 1 and 3 cells inside the east and north
    wall buffers and on the wall; the row range [2, Ny - 3) starts off a tile multiple, inside the south wall buffer."""
    assert (TS.TX, TS.TY) == (64, 16)
    for _, Nx, Ny, *_ in TS.matrix():
        for rows in TS.row_ranges(Ny):
            line = TS.check_layout(Nx, Ny, rows)
            assert f"{-(-Nx // 64)} tile columns of 64" in line
            if rows is not None:
                assert 0 < rows[0] < SC.WALL_DEPTH and rows[1] > rows[0]
    assert [TS.tracer_tiles(Nx, Ny) for Nx, Ny in TS.WALL_SHAPES] == [(2, 1, 2, 1), (2, 3, 2, 3), (1, 64, 1, 16), (1, 7, 1, 8), (3, 1, 2, 15)]
    assert {TS.tracer_tiles(Nx, Ny)[1] for Nx, Ny in TC.STAGE_SHAPES} == {3, 7, 63, 64, 1}
    assert {TS.tracer_tiles(Nx, Ny)[3] for Nx, Ny in TC.STAGE_SHAPES} == {3, 9, 15, 16, 1}
    assert TS.tracer_tiles(129, 26) == (3, 1, 2, 10)
    with pytest.raises(AssertionError):
        TS.check_layout(65, 17, (0, 16))


@pytest.mark.parametrize("dtype", TS.DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("topo", [(P, P), (B, B)], ids=["PP", "BB"])
def test_the_longdouble_update_is_substep_within_one_eps(oracle, topo, dtype):
    """reference_call's update, given the tendency of the precision of the call, against tracer_cases.substep (the oracle's
    expression order, every operation rounded to that precision): within 1 eps of the precision of the largest addend or result, for
    every fused call form that has a classic counterpart; the anchor forms restate the header: cnew of A1 is that of S1, W is the
    first-stage update with zeta for gamma, cnew of A2 is the first-stage update of W."""
    data = TS.TracerStageData(oracle, 65, 17, 0, dtype, topo)
    eps = float(np.finfo(dtype).eps)
    Gs = data.G_strict()
    Gint = [Hh.interior(g, 65, 17, H, H) for g in Gs]
    K = 3
    for variant, cset, _ in TS.calls()[:19]:
        v, coeffs = SC.VARIANTS[variant], SC.COEFFS[cset][variant]
        if not v["fused"] or v["operand"] == "Uprev":
            continue
        dt = data.dt(coeffs[0])
        for rows in (None, (2, 14)):
            ref = TS.reference_call(data, variant, coeffs, dt, K, rows, G=Gint)
            cut = lambda a: TS._cut(data, a, rows)
            for k in range(K):
                base = data.Gm[k] if v["operand"] == "W" else data.c[k]
                classic = v["operand"] == "Gm"
                want = TC.substep(base, Gs[k], data.Gm[k] if classic else None, 65, 17, dt, coeffs[0], coeffs[1], not classic)
                scale = max(np.abs(cut(base)).max(), np.abs(cut(want)).max(), dt * abs(coeffs[0]) * np.abs(cut(Gs[k])).max(),
                            dt * abs(coeffs[1]) * np.abs(cut(data.Gm[k])).max() if classic else 0.0)
                err = float(np.abs(ref["cnew"][k] - cut(want).astype(np.longdouble)).max())
                print(variant, cset, rows, k, err / (eps * scale))
                assert ref["cnew"][k].shape == cut(want).shape and err <= eps * scale, (variant, cset, k, err / (eps * scale))
                if variant == "A1":
                    w = TC.substep(data.c[k], Gs[k], None, 65, 17, dt, coeffs[1], 0.0, True)
                    sw = max(np.abs(cut(data.c[k])).max(), np.abs(cut(w)).max())
                    assert float(np.abs(ref["Gn"][k] - cut(w).astype(np.longdouble)).max()) <= eps * sw
            assert (ref["Gn"] is TS.KEEP) == (variant in ("S1n", "S3n", "A2", "A2a"))
    # a strict reference is substep itself, the tendency the oracle's in the precision of the call, and T has no new state
    s = TS.reference_call_strict(data, "S2g", (0.37, -0.21), 1e-3, K, (2, 14))
    assert all(a.dtype == np.dtype(dtype) and a.shape == (12, 65) for a in s["cnew"] + s["Gn"])
    assert np.array_equal(s["cnew"][1], TC.substep(data.c[1], Gs[1], data.Gm[1], 65, 17, 1e-3, 0.37, -0.21, False)[H + 2:H + 14, H:H + 65])
    t = TS.reference_call_strict(data, "T", (0.0, 0.0), 0.0, K)
    assert t["cnew"] is None and np.array_equal(t["Gn"][2], Gint[2])


def test_the_bounds_are_those_of_stage_bounds(oracle):
    """call_bounds with four tracers against stage_cases.stage_bounds on a stand-in whose four fields are those tracers: the same
    numbers for every call form the tracer call has, over all rows and over a row range; the time step keeps cnew a sharp witness of G."""
    data = TS.TracerStageData(oracle, 65, 17, 1, np.float32, (P, B))
    K = 4
    shim = types.SimpleNamespace(Nx=65, Ny=17, dtype=data.dtype, Gmax=data.Gmax[:K], scales=data.scales[:K])
    for variant, cset in SC.calls():
        v, coeffs = SC.VARIANTS[variant], SC.COEFFS[cset][variant]
        if v["operand"] == "Uprev":
            continue
        dt = data.dt(coeffs[0])
        for rows in (None, (2, 14)):
            ref = TS.reference_call(data, variant, coeffs, dt, K, rows)
            got = TS.call_bounds(data, variant, coeffs, dt, K, ref, rows)
            want = SC.stage_bounds(shim, data.c[:K], data.Gm[:K] if v["operand"] else None, variant, coeffs, dt,
                                   {"qnew": ref["cnew"], "Gn": ref["Gn"]}, rows=rows)
            assert got["cnew"] == want["qnew"] and got["Gn"] == want["Gn"], (variant, cset, rows)
        if variant != "T":
            inc = dt * abs(coeffs[0]) * max(data.Gmax)
            assert dt == float(np.float32(dt)) and 0.99 * max(data.cmax) <= inc <= 1.01 * max(data.cmax)
    assert data.dt(0.0) == 0.0
    tb = [SC.TOL[data.dtype] * max(g, s) for g, s in zip(data.Gmax, data.scales)]
    assert TS.call_bounds(data, "T", (0.0, 0.0), 0.0, 3, TS.reference_call(data, "T", (0.0, 0.0), 0.0, 3)) == {"cnew": None, "Gn": tb[:3]}
    q64 = [a.astype(np.float64) for a in data.q]
    assert data.scales[5] == Hh.term_scales("VectorInvariant", q64 + [data.c[5].astype(np.float64)], data.dx, data.dy, 0.0)[3]


@pytest.mark.parametrize("form", TS.FORMULATIONS, ids=["vi", "cons"])
def test_the_bounded_reference_differs_exactly_inside_the_wall_buffers(oracle, form):
    """Every wall shape, topology and precision: the Bounded tendency of every tracer differs from the periodic one of the same interior
    inside the buffer of every wall and equals it bit for bit outside all of them (at 7 x 8 the buffers cover the grid: that half is
    vacuous).  Control: a reference that took no wall branch -- the periodic one -- is caught in every buffer of every tracer.  The
    halos hold the boundary conditions: the gradient condition on tracer 0 where y is Bounded, no flux on the others."""
    for Nx, Ny in TS.WALL_SHAPES:
        for topo in TS.WALL_TOPOS:
            for dtype in TS.DTYPES:
                data = TS.TracerStageData(oracle, Nx, Ny, form, dtype, topo)
                assert data.wall_failures == [], (Nx, Ny, topo, dtype, data.wall_failures)
                assert all(np.isfinite(g).all() for g in data.G) and len(data.G) == TS.KMAX
                buffers = SC.wall_buffers(Nx, Ny, topo)
                caught = TS.wall_buffer_failures(data.G_periodic, data.G_periodic, Nx, Ny, topo)
                assert len(caught) == len(buffers) * TS.KMAX
                covered = np.logical_or.reduce(list(buffers.values())).all()
                assert covered == ((Nx, Ny) == (7, 8)), (Nx, Ny, topo)
                if topo[1] == B:
                    c0, c1 = data.c[0].astype(np.float64), data.c[1].astype(np.float64)
                    assert np.allclose(c0[H - 1, H:H + Nx] - c0[H, H:H + Nx], 0.05 * data.dy, rtol=0, atol=1e-6)
                    assert np.array_equal(c1[H - 1, H:H + Nx], c1[H, H:H + Nx])
    # a difference outside the buffers is the other violation
    data = TS.TracerStageData(oracle, 129, 31, form, np.float64, (B, B))
    spoiled = [g.copy() for g in data.G]
    spoiled[2][15, 64] += 1.0
    assert TS.wall_buffer_failures(spoiled, data.G_periodic, 129, 31, (B, B)) == [
        "tracer 2: the Bounded reference differs from the periodic one in 1 cells outside the wall buffers"]


def test_distinct_tracers_and_operands_and_poisoned_buffers(oracle):
    """No two tracers, operands or tendencies of a case are equal; the buffers of a call hold NaN in the pad columns of the inputs
    and in the halos of every wrapped direction, the sentinel in the operand's halos and everywhere in the outputs; Gn of A2a is Gm."""
    data = TS.TracerStageData(oracle, 65, 17, 1, np.float32, (P, B))
    fields = data.c + data.Gm
    assert all(not np.array_equal(fields[i], fields[j]) for i in range(len(fields)) for j in range(i))
    assert all(not np.array_equal(data.G[i], data.G[j]) for i in range(8) for j in range(i))
    b = TS.call_buffers(data, "S2g", 3, True)
    assert [len(b[k]) for k in ("q", "c", "Gm", "cnew", "Gn")] == [3, 3, 3, 3, 3] and b["q"][0].shape == (23, 71 + 5)
    for a in b["q"] + b["c"]:
        assert np.isnan(a[:, 71:]).all() and np.isnan(a[:, :H]).all() and np.isnan(a[:, H + 65:71]).all() and np.isfinite(a[:, H:H + 65]).all()
    for a in b["Gm"]:
        assert np.isnan(a[:, 71:]).all() and (a[:H, :71] == TS.SENTINEL).all() and np.isfinite(a[H:H + 17, H:H + 65]).all()
    assert all((a == TS.SENTINEL).all() for a in b["cnew"] + b["Gn"])
    filled = TS.call_buffers(data, "T", 8, False)
    assert filled["cnew"] is None and filled["Gm"] is None and len(filled["Gn"]) == 8 and all(np.isfinite(a[:, :71]).all() for a in filled["c"])
    al = TS.call_buffers(data, "A2a", 3, False)
    assert al["Gn"] is al["Gm"] and TS.copy_buffers(al)["Gn"] is not al["Gn"]
    cp = TS.copy_buffers(al)
    assert cp["Gn"] is cp["Gm"]


CHECKED = [("fast", (P, P)), ("wall", (P, B)), ("wall", (B, B)), ("wall-strict", (B, P))]


@pytest.mark.parametrize("path,topo", CHECKED, ids=[f"{p}-{''.join('PB'[d] for d in t)}" for p, t in CHECKED])
@pytest.mark.parametrize("dtype", TS.DTYPES, ids=["f64", "f32"])
def test_the_checker_catches_the_errors_it_exists_for(oracle, path, topo, dtype):
    """check_outputs on fabricated "kernel outputs": the reference itself passes; the reference with one defect -- one cell off by twice
    its bound, two tracers swapped, the operand of another tracer, zeta applied where it must be ignored, the periodic result on a
    Bounded grid, a write into a halo, a pad column or a row outside the range, Gn written with store_G = 0, W overwritten under A2a,
    a kernel that wrote nothing -- gives at least one failure line; so does a refused call that wrote cnew.  No kernel runs."""
    Nx, Ny, K = 65, 17, 3
    data = TS.TracerStageData(oracle, Nx, Ny, 0, dtype, topo)
    strict, wrap = TS.PATHS[path]["strict"], P in topo
    t = np.dtype(dtype).type

    def case(variant, cset, rows, K=K):
        before = TS.call_buffers(data, variant, K, wrap)
        ref, bounds = TS.expected_call(data, path, variant, cset, K, rows)
        good = TS.fabricate(data, K, rows, before, ref)
        check = lambda after: TS.check_outputs(data, variant, K, rows, wrap, before, after, ref, bounds)
        return before, ref, bounds, good, check

    for variant, cset, Kc in TS.calls():
        if variant in TS.PATHS[path]["refused"]:
            continue
        for rows in TS.row_ranges(Ny):
            before, ref, bounds, good, check = case(variant, cset, rows, Kc)
            fails, ratios = check(good)
            assert fails == [], (variant, cset, rows, fails)
            # (rounding the longdouble reference to the precision of the call costs half an ulp, far inside every bound)
            assert all(r <= 0.2 for r in ratios.values()) and set(ratios) == {n for n in ("cnew", "Gn") if ref[n] is not None and ref[n] is not TS.KEEP}
            assert check(before)[0], "a kernel that wrote nothing passes"
    j0, j1 = 2, Ny - 3
    for rows in (None, (j0, j1)):
        r0 = 0 if rows is None else j0
        # one cell off by twice its bound (strict: by one ulp)
        for variant, name in (("S2g", "cnew"), ("S2g", "Gn"), ("T", "Gn"), ("S1n", "cnew")):
            before, ref, bounds, good, check = case(variant, "generic" if variant != "T" else "rk3", rows)
            bad = TS.copy_buffers(good)
            cell = bad[name][1][H + r0 + 3:, H + 64:]
            cell[0, 0] = np.nextafter(cell[0, 0], t(np.inf)) if strict else t(np.longdouble(ref[name][1][3, 64]) + 2 * bounds[name][1])
            lines = check(bad)[0]
            assert len(lines) == 1 and lines[0].startswith(f"{name}[1]: "), lines
        # tracers 0 and 1 swapped; the operand of tracer k + 1 used for tracer k
        before, ref, bounds, good, check = case("S2g", "generic", rows)
        bad = TS.copy_buffers(good)
        bad["cnew"][0], bad["cnew"][1] = bad["cnew"][1], bad["cnew"][0]
        lines = check(bad)[0]
        assert any(m.startswith("cnew[0]") for m in lines) and any(m.startswith("cnew[1]") for m in lines) and not any("cnew[2]" in m for m in lines)
        rolled = TS.TracerStageData.__new__(TS.TracerStageData)
        rolled.__dict__.update(data.__dict__)
        rolled.Gm, rolled._ref = data.Gm[1:] + data.Gm[:1], {}
        wrong = TS.expected_call(rolled, path, "S2g", "generic", K, rows)[0]
        lines = check(TS.fabricate(data, K, rows, before, wrong))[0]
        assert [m.split(":")[0] for m in lines] == ["cnew[0]", "cnew[1]", "cnew[2]"], lines
        # Gm[0] read for every tracer
        rolled.Gm, rolled._ref = [data.Gm[0]] * TS.KMAX, {}
        wrong = TS.expected_call(rolled, path, "S2g", "generic", K, rows)[0]
        assert [m.split(":")[0] for m in check(TS.fabricate(data, K, rows, before, wrong))[0]] == ["cnew[1]", "cnew[2]"]
        # zeta applied where the header says it is unused: a first stage that adds dt zeta G
        before, ref, bounds, good, check = case("S1g", "generic", rows)
        gam, zet = SC.COEFFS["generic"]["S1g"]
        if strict:
            wrong = TS.reference_call_strict(data, "S1g", (gam + zet, 0.0), data.dt(gam), K, rows)
        else:
            wrong = TS.reference_call(data, "S1g", (gam + zet, 0.0), data.dt(gam), K, rows)
        lines = check(TS.fabricate(data, K, rows, before, wrong))[0]
        assert [m.split(":")[0] for m in lines] == ["cnew[0]", "cnew[1]", "cnew[2]"], lines
        if path == "fast":
            before, ref, bounds, good, check = case("A2", "generic", rows)
            wrong = TS.reference_call(data, "A2", (gam + zet, 0.0), data.dt(gam), K, rows)
            assert len(check(TS.fabricate(data, K, rows, before, wrong))[0]) == 3
            # ... W overwritten under A2a (through the aliased Gn), Gn of A2 written although the anchor form stores no G
            before, ref, bounds, good, check = case("A2a", "rk3", rows)
            bad = TS.copy_buffers(good)
            bad["Gn"][2][H + r0, H] = 0.0
            assert check(bad)[0] == ["operand W[2] was changed"]
            before, ref, bounds, good, check = case("A2", "rk3", rows)
            bad = TS.copy_buffers(good)
            bad["Gn"][0][H + r0, H] = 0.0
            assert check(bad)[0] == ["Gn[0] must keep its sentinel: 1 cells written"]
        # the periodic result submitted for a wall case
        if topo != (P, P):
            per = TS.TracerStageData.__new__(TS.TracerStageData)
            per.__dict__.update(data.__dict__)
            per._ref = {}
            if strict:
                qp = [oracle.fill_halo_periodic(a.copy(), Nx, Ny, H, H) for a in data.q]
                per._G_strict = [TC.tracer_tendency(oracle, qp, oracle.fill_halo_periodic(a.copy(), Nx, Ny, H, H), Nx, Ny, data.dx, data.dy, 0)
                                 for a in data.c]
            else:
                per.G = data.G_periodic
            for variant in ("T", "S2g", "S1n"):
                before, ref, bounds, good, check = case(variant, "rk3", rows)
                wrong = TS.expected_call(per, path, variant, "rk3", K, rows)[0]
                lines = check(TS.fabricate(data, K, rows, before, wrong))[0]
                assert len(lines) == 3 * sum(1 for n in ("cnew", "Gn") if ref[n] is not None and ref[n] is not TS.KEEP), (variant, lines)
        # a write into a halo, a pad column, a row outside the range; Gn written with store_G = 0; an input changed
        before, ref, bounds, good, check = case("S3n", "rk3", rows)
        for (j, i), what in (((H - 1, H + 5), "halo"), ((H + Ny, H + 5), "halo"), ((H + r0, H + Nx), "halo"), ((H + r0, H - 1), "halo"),
                             ((H + r0, Nx + 2 * H), "pad columns"), ((H + r0 + 1, Nx + 2 * H + TS.PAD - 1), "pad columns")):
            bad = TS.copy_buffers(good)
            bad["cnew"][1][j, i] = 1.0
            assert check(bad)[0] == [f"cnew[1]: 1 cells of the {what} written"], (j, i)
        if rows is not None:
            for j in (H + j0 - 1, H + j1, H, H + Ny - 1):
                bad = TS.copy_buffers(good)
                bad["cnew"][2][j, H + 7] = 1.0
                assert check(bad)[0] == [f"cnew[2]: 1 cells of the interior outside rows [{j0}, {j1}) written"], j
        bad = TS.copy_buffers(good)
        bad["Gn"][0][H + r0, H + 1] = ref["cnew"][0][0, 1]
        assert check(bad)[0] == ["Gn[0] must keep its sentinel: 1 cells written"]
        bad = TS.copy_buffers(good)
        bad["c"][1][0, 0] = 0.0
        bad["q"][2][H, H] = 0.0
        bad["Gm"][0][H, Nx + 2 * H] = 0.0
        assert check(bad)[0] == ["input q[2] was changed", "input c[1] was changed", "operand Gm[0] was changed"]
    # a refused call that wrote cnew; inputs whose wrapped halos were not poisoned
    before = TS.call_buffers(data, "P2g", K, wrap)
    after = TS.copy_buffers(before)
    assert TS.check_refusal(before, after) == []
    after["cnew"][1][H + 4, H + 4] = 2.0
    assert TS.check_refusal(before, after) == ["refused call changed cnew[1]"]
    if wrap:
        unpoisoned = TS.call_buffers(data, "S1g", K, False)
        ref, bounds = TS.expected_call(data, path, "S1g", "rk3", K, None)
        lines = TS.check_outputs(data, "S1g", K, None, True, unpoisoned, TS.fabricate(data, K, None, unpoisoned, ref), ref, bounds)[0]
        assert len(lines) == 6 and all("not NaN on entry" in m for m in lines)
