"""CPU tests (no GPU) that pin what tests/test_output_matrix_gpu.py relies on in tests/output_cases.py: the reach tables are what the
restatement reads, the restatement is bit for bit a second, scalar statement of the header's formulas, `images` is the periodic
gather, and the sign of zero of B_x, B_y is the written order's.  Every comparison is bitwise."""
import math

import numpy as np
import pytest

import helpers as Hh
import output_cases as OC

WRAPS = (0, OC.WRAP_X, OC.WRAP_Y, OC.WRAP_X | OC.WRAP_Y)
DX, DY = 0.1, 0.12


def _parents(Nx, Ny, Hx, Hy, seed):
    rng = np.random.default_rng(seed)
    shape = (Ny + 2 * Hy, Nx + 2 * Hx)
    return [rng.standard_normal(shape), rng.standard_normal(shape), 1.0 + 0.3 * rng.random(shape), rng.standard_normal(shape)]


# ---- the tables themselves ------------------------------------------------------------------------------------------------------------
def test_case_lists():
    assert OC.SHAPES == ((1, 1), (2, 3), (4, 1), (5, 2), (7, 9), (64, 2), (65, 3), (1025, 2)) and OC.HALOS == ((1, 1), (3, 2))
    assert sorted(Nx % 4 for Nx, _ in OC.SHAPES) == [0, 0, 1, 1, 1, 1, 2, 3]
    assert list(OC.ALL_MASKS) == list(range(1, 128)) and OC.ALL == 127
    assert set(OC.MASKS) == {1, 2, 4, 8, 16, 32, 64, 127, 1 | 2 | 8 | 16, 32 | 64, 2 | 32} and len(OC.MASKS) == 11
    assert OC.mask_names(1 | 2 | 8 | 16) == ("u", "v", "A", "s") and OC.mask_names(127) == OC.NAMES
    assert OC.ROW_RANGES(9) == ((0, 9), (1, 9), (0, 1), (1, 1)) and OC.ROW_RANGES(1) == ((0, 1), (1, 1))
    assert all(j0 <= j1 <= Ny for _, Ny in OC.SHAPES for j0, j1 in OC.ROW_RANGES(Ny))
    assert all(any(j0 == j1 for j0, j1 in OC.ROW_RANGES(Ny)) for _, Ny in OC.SHAPES)


def test_reach_tables():
    """The examples the tables are described by, and REACH as the union of FIELD_REACH over the fields."""
    assert OC.REACH[1]["q1"] == {(0, 0)} and OC.REACH[0]["q1"] == {(0, 0)}
    assert OC.REACH[0]["h"] == {(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (0, 0)}       # west column on rows j-1 .. j+1, south, north, itself
    assert OC.REACH[1]["h"] == OC.REACH[1]["A"] == OC.REACH[0]["A"] == {(0, 0), (-1, 0), (0, -1)}
    assert OC.REACH[1]["q2"] == OC.REACH[0]["q2"] == {(0, 0), (-1, 0), (-1, 1), (0, 1)}
    for form in (1, 0):
        assert set(OC.FIELD_REACH[form]) == set(OC.NAMES)
        for p in OC.PARENTS:
            assert OC.REACH[form][p] == set().union(*(OC.FIELD_REACH[form][n].get(p, set()) for n in OC.NAMES))
            assert all(di <= 0 for di, _ in OC.REACH[form][p]), "nothing reads east of its cell"


@pytest.mark.parametrize("Hx,Hy", OC.HALOS)
@pytest.mark.parametrize("Nx,Ny", OC.SHAPES[:-1] + ((7, 5),))
def test_keep_mask_never_holds_the_east_side(Nx, Ny, Hx, Hy):
    for form in (1, 0):
        for p in OC.PARENTS:
            for wrap in WRAPS:
                keep = OC.keep_mask(Nx, Ny, Hx, Hy, form, p, wrap)
                assert keep.shape == (Ny + 2 * Hy, Nx + 2 * Hx) and not keep[Hy:Hy + Ny, Hx:Hx + Nx].any()
                assert not keep[:, Hx + Nx:].any(), "the east column and the two east corners are never read"
                if wrap & OC.WRAP_X:
                    assert not keep[:, :Hx].any()
                if wrap & OC.WRAP_Y:
                    assert not keep[:Hy].any() and not keep[Hy + Ny:].any()
                ring = np.zeros_like(keep)
                ring[Hy - 1:Hy + Ny + 1, Hx - 1:Hx + Nx + 1] = True
                assert not (keep & ~ring).any(), "the reach is one cell"


# ---- REACH is what the restatement reads --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wrap", WRAPS, ids=["nowrap", "wrapx", "wrapy", "wrapxy"])
@pytest.mark.parametrize("form", [1, 0], ids=["vi", "cons"])
def test_reach_is_what_the_restatement_reads(form, wrap):
    """7 x 5, halo (3, 2): one NaN in each padded cell of each parent in turn.  The frame has a NaN exactly if the cell is in keep_mask
    or in the interior, and field by field the NaN cells are those FIELD_REACH predicts.  (With a wrap flag the parents go through
    `images` first, as the GPU tests hand them to the restatement.)"""
    Nx, Ny, Hx, Hy = 7, 5, 3, 2
    q = _parents(Nx, Ny, Hx, Hy, 7)
    clean = OC.np_output_fields(*OC.images(q, Nx, Ny, Hx, Hy, wrap), Nx, Ny, Hx, Hy, DX, DY, form)
    assert np.isfinite(clean).all()
    interior = np.zeros(q[0].shape, dtype=bool)
    interior[Hy:Hy + Ny, Hx:Hx + Nx] = True
    for k, p in enumerate(OC.PARENTS):
        keep = OC.keep_mask(Nx, Ny, Hx, Hy, form, p, wrap)
        for jp in range(Ny + 2 * Hy):
            for ip in range(Nx + 2 * Hx):
                bad = [a.copy() for a in q]
                bad[k][jp, ip] = np.nan
                got = OC.np_output_fields(*OC.images(bad, Nx, Ny, Hx, Hy, wrap), Nx, Ny, Hx, Hy, DX, DY, form)
                nan = np.isnan(got)
                assert nan.any() == bool(keep[jp, ip] or interior[jp, ip]), (p, jp, ip)
                for f, n in enumerate(OC.NAMES):
                    want = OC.reached_cells(Nx, Ny, form, n, p, (jp - Hy, ip - Hx), wrap)
                    assert np.array_equal(nan[f], want), (p, n, jp, ip)
                Hh.same_bits(got[~nan], clean[~nan], "the cells that do not read it")


# ---- an independent second statement -----------------------------------------------------------------------------------------------------
def _scalar_frames(q1, q2, h, A, Nx, Ny, Hx, Hy, dx, dy, form, rows):
    """The seven fields cell by cell in Python floats (IEEE double), written from the formulas of csrc/frame_device.inc:5-12."""
    at = lambda a, i, j: float(a[Hy + j, Hx + i])
    U = lambda i, j: at(q1, i, j) if form == 1 else at(q1, i, j) / (0.5 * (at(h, i - 1, j) + at(h, i, j)))
    V = lambda i, j: at(q2, i, j) if form == 1 else at(q2, i, j) / (0.5 * (at(h, i, j - 1) + at(h, i, j)))
    sq = lambda x: x * x
    j0, j1 = rows
    out = np.empty((7, j1 - j0, Nx))
    for j in range(j0, j1):
        for i in range(Nx):
            out[0, j - j0, i] = U(i, j)
            out[1, j - j0, i] = V(i, j)
            out[2, j - j0, i] = at(h, i, j)
            out[3, j - j0, i] = at(A, i, j)
            mean = 0.5 * (0.5 * (sq(V(i - 1, j)) + sq(V(i, j))) + 0.5 * (sq(V(i - 1, j + 1)) + sq(V(i, j + 1))))
            out[4, j - j0, i] = math.sqrt(sq(U(i, j)) + mean)
            out[5, j - j0, i] = -((at(A, i, j) - at(A, i, j - 1)) / dy) / (0.5 * (at(h, i, j - 1) + at(h, i, j)))
            out[6, j - j0, i] = ((at(A, i, j) - at(A, i - 1, j)) / dx) / (0.5 * (at(h, i - 1, j) + at(h, i, j)))
    return out


@pytest.mark.parametrize("Hx,Hy", OC.HALOS)
@pytest.mark.parametrize("Nx,Ny", [(5, 2), (7, 9)])
@pytest.mark.parametrize("form", [1, 0], ids=["vi", "cons"])
def test_restatement_is_the_scalar_loop_bitwise(form, Nx, Ny, Hx, Hy):
    for dtype in (np.float64, np.float32):               # fp32 parents and spacings as an fp32 call hands them over
        q = [a.astype(dtype) for a in _parents(Nx, Ny, Hx, Hy, 3 * Nx + Ny)]
        dx, dy = float(dtype(DX)), float(dtype(DY))
        for rows in OC.ROW_RANGES(Ny):
            got = OC.np_output_fields(*q, Nx, Ny, Hx, Hy, dx, dy, form, rows=rows)
            Hh.same_bits(got, _scalar_frames(*q, Nx, Ny, Hx, Hy, dx, dy, form, rows), f"{Nx}x{Ny} form {form} rows {rows}")
        for which in OC.MASKS:
            names = OC.mask_names(which)
            sel = [OC.NAMES.index(n) for n in names]
            Hh.same_bits(OC.np_output_fields(*q, Nx, Ny, Hx, Hy, dx, dy, form, names=names),
                         OC.np_output_fields(*q, Nx, Ny, Hx, Hy, dx, dy, form)[sel], f"mask {which}")


def test_errstate_changes_no_result():
    """NaN and Inf parents raise no warning (warnings are errors here) and give what the unguarded arithmetic gives."""
    import warnings
    Nx, Ny, Hx, Hy = 7, 9, 3, 2
    q = _parents(Nx, Ny, Hx, Hy, 21)
    q[2][Hy + 3, Hx + 4] = np.inf
    q[0][Hy + 1, Hx + 1] = np.nan
    q[3][Hy + 5, Hx + 2] = -np.inf                         # (Inf - Inf in B_x, B_y of the cells around)
    for form in (1, 0):
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            got = OC.np_output_fields(*q, Nx, Ny, Hx, Hy, DX, DY, form)
        with np.errstate(all="ignore"):
            want = _scalar_frames(*q, Nx, Ny, Hx, Hy, DX, DY, form, (0, Ny))
        Hh.same_bits(got, want, f"non-finite parents, form {form}")
        assert np.isnan(got).any() and np.isinf(got).any()


# ---- images ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hx,Hy", OC.HALOS)
@pytest.mark.parametrize("Nx,Ny", OC.SHAPES[:-1])
def test_images_is_wrap_parents_or_a_mod_gather(Nx, Ny, Hx, Hy):
    q = _parents(Nx, Ny, Hx, Hy, 5)
    for a in q:
        Hh.poison_halo(a, Nx, Ny, Hx, Hy)
    for wrap in WRAPS:
        wx, wy = bool(wrap & OC.WRAP_X), bool(wrap & OC.WRAP_Y)
        got = OC.images(q, Nx, Ny, Hx, Hy, wrap)
        if Nx >= Hx and Ny >= Hy:
            for a, b in zip(got, OC.wrap_parents(q, Nx, Ny, Hx, Hy, wx, wy)):
                Hh.same_bits(a, b, f"images vs wrap_parents {Nx}x{Ny} wrap {wrap}")
        for a, src in zip(got, q):                         # the direct gather, cell by cell
            want = np.empty_like(src)
            for jp in range(Ny + 2 * Hy):
                for ip in range(Nx + 2 * Hx):
                    js = (jp - Hy) % Ny + Hy if wy else jp
                    is_ = (ip - Hx) % Nx + Hx if wx else ip
                    want[jp, ip] = src[js, is_]
            Hh.same_bits(a, want, f"images vs mod gather {Nx}x{Ny} wrap {wrap}")
            if wx and wy:
                assert np.isfinite(a).all()
    assert any(Nx < hx for hx, _ in OC.HALOS for Nx, _ in OC.SHAPES) and any(Ny < hy for _, hy in OC.HALOS for _, Ny in OC.SHAPES)


# ---- the sign of zero -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [1, 0], ids=["vi", "cons"])
def test_constant_A_gives_minus_zero_B_x_and_plus_zero_B_y(form):
    """B_x = -((A - A) / dy) / h = -(+0) / h = -0.0 wherever h > 0; B_y = ((A - A) / dx) / h = +0.0; same_bits tells them apart."""
    Nx, Ny, Hx, Hy = 5, 2, 3, 2
    q = _parents(Nx, Ny, Hx, Hy, 9)
    q[3][:] = 0.75
    assert (q[2] > 0).all()
    bx, by = OC.np_output_fields(*q, Nx, Ny, Hx, Hy, DX, DY, form, names=("B_x", "B_y"))
    assert (bx == 0).all() and np.signbit(bx).all()
    assert (by == 0).all() and not np.signbit(by).any()
    Hh.same_bits(bx, np.full((Ny, Nx), -0.0), "B_x")
    Hh.same_bits(by, np.zeros((Ny, Nx)), "B_y")
    with pytest.raises(AssertionError):
        Hh.same_bits(bx, np.zeros((Ny, Nx)), "-0.0 is not 0.0")
    with pytest.raises(AssertionError):
        Hh.same_bits(np.array([1.0, np.nan]), np.array([np.nan, 1.0]), "NaN in another place")
    Hh.same_bits(np.array([1.0, np.nan], dtype=np.float32), np.array([1.0, np.nan]), "NaN in the same place")
