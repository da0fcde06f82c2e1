"""Pins of tests/diag_cases.py, the reference and case list of the diagnostics matrix (tests/test_diag_matrix_gpu.py), on the CPU: the
longdouble reference agrees with the independent restatement plot_cases.np_diagnostics wherever that applies, it propagates NaN the
way the kernel is asked to, its inputs are poisoned outside the stencil's footprint, and the list really holds the edges of the kernel's
structure (256 threads, 1024 blocks, 262 144 cells per trip).  No test here needs a GPU or the built library."""
import numpy as np
import pytest

import diag_cases as DC
import plot_cases as PC

CASES = DC.cases()


def test_longdouble_is_wider_than_double():
    """The tolerance of the matrix leaves the reference no share of the error: its terms must carry more than 53 bits."""
    assert np.finfo(np.longdouble).nmant >= 63


@pytest.mark.parametrize("c", [c for c in CASES if c.nonfinite is None and c.rows is None and np.dtype(c.dtype) == np.float64 and c.Hx == c.Hy],
                         ids=DC.case_id)
def test_reference_agrees_with_the_numpy_restatement(c):
    """plot_cases.np_diagnostics covers the whole row range, float64, Hx == Hy and g = 9.81.  It rounds every operation to double and
    sums pairwise: at most the 16 roundings per cell and a summation depth below D, so the matrix's own bound applies.  Extrema: equal."""
    assert PC.G == DC.GRAV
    q = DC.inputs(c)
    want, sumabs = DC.expected(c)
    got = PC.np_diagnostics(*q, c.Nx, c.Ny, DC.DX, DC.DY, c.form, href=DC.HREF, Hh=c.Hx)
    fails, ratio = DC.compare([got[k] for k in DC.NAMES], want, sumabs, DC.ncell_of(c))
    print(DC.case_id(c), "error / bound", ratio)
    assert not fails, fails


def test_the_list_holds_the_edges():
    ids = [DC.case_id(c) for c in CASES]
    assert len(set(ids)) == len(ids) == len(set(CASES))
    n = [DC.ncell_of(c) for c in CASES]
    assert any(0 < x < DC.NT for x in n)
    assert any(x in (DC.NT - 1, DC.NT, DC.NT + 1) for x in n) and {255, 256, 257} <= set(n)
    assert any(DC.TRIP < x < 2 * DC.TRIP and x % DC.NT for x in n)
    assert any(x >= 2 * DC.TRIP for x in n)
    assert any(x >= 2 * DC.TRIP and c.rows is not None and c.rows[0] > 0 for x, c in zip(n, CASES))
    rows = [c for c in CASES if c.rows is not None]
    assert any(c.rows[0] > 0 and c.rows[1] > c.rows[0] for c in rows) and any(c.rows[1] < c.Ny and c.rows[1] > c.rows[0] for c in rows)
    assert any(0 < c.rows[0] < c.rows[1] < c.Ny for c in rows)                               # a strict sub-range
    assert any(c.rows == (0, 1) and c.Ny > 1 for c in rows) and any(c.rows == (c.Ny - 1, c.Ny) and c.Ny > 1 for c in rows)
    for empty in ("first", "last", "inside"):
        assert any(c.rows[0] == c.rows[1] and {"first": c.rows[0] == 0, "last": c.rows[0] == c.Ny, "inside": 0 < c.rows[0] < c.Ny}[empty]
                   for c in rows)
    assert any(c.Hx != c.Hy for c in CASES) and any((c.Hx, c.Hy) == (1, 1) for c in CASES) and any(c.pitch for c in CASES)
    assert any(c.pitch and c.Hx != c.Hy and c.rows is not None for c in CASES)
    for form in (0, 1):
        for kind in (("u", "nan"), ("A", "nan"), ("h", "nan"), ("u", "inf")):
            assert any(c.nonfinite == kind and c.form == form for c in CASES), (form, kind)
        for dtype in (np.float64, np.float32):
            for shape in DC.SHAPES:
                assert any((c.Nx, c.Ny, c.form) == shape + (form,) and np.dtype(c.dtype) == dtype and c.rows is None for c in CASES)
    # the non-finite cell of a case lies inside its rows; at 513 x 512 only a second trip reaches it
    for c in CASES:
        if c.nonfinite is not None:
            x, y = DC.nonfinite_cell(c)
            j0, j1 = DC.rows_of(c)
            assert 0 <= x < c.Nx and j0 <= y < j1
            if c.Nx * c.Ny > DC.TRIP:
                assert (y - j0) * c.Nx + x >= DC.TRIP
    # ensembles: the three shapes, a per-member-g case whose three g differ, non-finite members
    E = DC.ensemble_cases()
    assert {(e[0], e[1]) for e in E} == set(DC.ENSEMBLE_SHAPES) and len(set(DC.ENSEMBLE_G)) == 3 == DC.ENSEMBLE_MEMBERS
    assert any(e[4] for e in E) and any(e[5] is not None for e in E)
    assert all(-(-Nx * Ny // DC.NT) < DC.NB for Nx, Ny in DC.ENSEMBLE_SHAPES[:2])      # the identity-fold path (nb < 1024)


def test_no_case_is_left_out():
    """The GPU module parametrizes exactly this list, without skip or xfail marks (its own source is the witness: importing it needs
    no GPU)."""
    import test_diag_matrix_gpu as T
    assert T.CASES == CASES and len(T.CASES) == len(CASES) == 124
    assert T.ENSEMBLE_CASES == DC.ensemble_cases() and len(T.ENSEMBLE_CASES) == 11
    src = open(T.__file__).read()
    assert "skip" not in src and "xfail" not in src


def test_inputs_are_poisoned_outside_the_ring():
    c = DC.Case(37, 21, 2, 5, True, (5, 17), 1, np.float32, None)
    for a in DC.inputs(c):
        assert a.shape == (21 + 10, 37 + 4 + DC.PAD) and a.dtype == np.float32 and not a.flags.writeable
        ring = a[5 + 4:5 + 18, 1:2 + 38]
        assert np.isfinite(ring).all() and np.isnan(a).sum() == a.size - ring.size
    h = DC.inputs(c)[2]
    assert np.nanmin(h) >= 1.0 and np.nanmax(h) <= 1.3 + 1e-6
    e = DC.Case(5, 4, 1, 1, False, (2, 2), 1, np.float64, None)
    assert all(np.isnan(a).all() for a in DC.inputs(e))
    # halo (1, 1), whole range, no pitch: the ring is the whole parent
    assert all(np.isfinite(a).all() for a in DC.inputs(DC.Case(5, 4, 1, 1, False, None, 1, np.float64, None)))


def test_empty_range_and_row_additivity():
    """j0 == j1: sums 0, maxima 0, min_h 1e300.  Sub-ranges: the energies of [0, 9) and [9, 21) add up to the whole range's (to the
    reference's own 2^-100) and the extrema combine -- on un-poisoned inputs, so that the three calls see the same data."""
    out, sumabs = DC.expected(DC.Case(37, 21, 3, 3, False, (9, 9), 0, np.float32, None))
    assert [float(v) for v in out] == list(DC.EMPTY) and [float(s) for s in sumabs] == [0.0] * 3
    q = DC._random_parents(37, 21, 3, 3, 43)
    ref = lambda j0, j1: DC.reference(*q, 37, 21, 3, 3, DC.DX, DC.DY, DC.GRAV, DC.HREF, 0, j0, j1, np.float64)[0]
    whole, lo, hi = ref(0, 21), ref(0, 9), ref(9, 21)
    for k in range(3):
        assert abs(whole[k] - (lo[k] + hi[k])) <= 2.0 ** -60 * whole[k]
    for k in (3, 4, 5):
        assert whole[k] == max(lo[k], hi[k])
    assert whole[6] == min(lo[6], hi[6])


def test_fp32_scalars_are_the_rounded_ones():
    """The fp32 entry point receives dx, dy, g, h_ref as floats: the reference of an fp32 case uses their roundings, which moves ME
    (dx, dy), PE (g, h_ref) and every energy (dx dy) well beyond the matrix's bound."""
    c = DC.Case(37, 21, 3, 3, False, None, 1, np.float32, None)
    q = DC.inputs(c)
    want, sumabs = DC.expected(c)
    f32 = lambda x: float(np.float32(x))
    same, _ = DC.reference(*q, 37, 21, 3, 3, f32(DC.DX), f32(DC.DY), f32(DC.GRAV), f32(DC.HREF), 1, 0, 21, np.float64)
    assert all(a == b for a, b in zip(want, same))
    unrounded, _ = DC.reference(*q, 37, 21, 3, 3, DC.DX, DC.DY, DC.GRAV, DC.HREF, 1, 0, 21, np.float64)
    for k in range(3):
        assert abs(unrounded[k] - want[k]) > 100 * DC.energy_bound(37 * 21, sumabs[k])


@pytest.mark.parametrize("form", [1, 0])
def test_nan_propagates_as_in_the_reference_callback(form):
    """maximum(abs, u), maximum(abs, A), minimum(h) of Julia propagate NaN (SWMHD_example.jl:47-65).  NaN in u: KE and max|u| are NaN;
    max|A|, min h, ME and PE stay bitwise the clean case's.  NaN in A: ME and max|A| only.  NaN in h: all energies and min h, and the
    conservative form's velocities (uh / h).  +Inf in u: KE and max|u| are +Inf."""
    base = DC.Case(37, 21, 3, 3, False, None, form, np.float64, None)
    clean, _ = DC.expected(base)
    assert all(np.isfinite(float(v)) for v in clean)
    changed = {("u", "nan"): {0, 3}, ("A", "nan"): {1, 5}, ("h", "nan"): {0, 1, 2, 6} | ({3, 4} if form == 0 else set()), ("u", "inf"): {0, 3}}
    for kind, idx in changed.items():
        out, _ = DC.expected(base._replace(nonfinite=kind))
        for k in range(DC.NQ):
            if k in idx:
                assert np.isnan(out[k]) if kind[1] == "nan" else out[k] == np.inf, (kind, DC.NAMES[k], out[k])
            else:
                assert DC.same_bits(out[k], clean[k]) and out[k] == clean[k], (kind, DC.NAMES[k])


def test_compare_rejects_what_it_should():
    c = DC.Case(37, 21, 3, 3, False, None, 1, np.float64, None)
    want, sumabs = DC.expected(c)
    good = [np.float64(v) for v in want]
    assert DC.compare(good, want, sumabs, 777) == ([], DC.compare(good, want, sumabs, 777)[1])
    assert DC.compare(good, want, sumabs, 777)[1] <= 1.0 / (DC.R_CELL + DC.depth(777))           # one rounding of the exact value
    for k in range(DC.NQ):
        bad = list(good)
        bad[k] = good[k] * (1 + 2.0 ** -45) if k < 3 else np.nextafter(good[k], 0)
        assert len(DC.compare(bad, want, sumabs, 777)[0]) == 1
        bad[k] = np.nan
        assert len(DC.compare(bad, want, sumabs, 777)[0]) == 1
    nan_want, nan_abs = DC.expected(c._replace(nonfinite=("u", "nan")))
    assert len(DC.compare(good, nan_want, nan_abs, 777)[0]) == 2        # finite KE and max|u| where NaN is due: today's fmax / fmin
    assert DC.depth(1) == 22 and DC.depth(DC.TRIP) == 22 and DC.depth(DC.TRIP + 1) == 23 and DC.depth(1024 * 520) == 24
