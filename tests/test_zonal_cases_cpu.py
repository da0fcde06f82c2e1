"""CPU tests (no GPU) of the reference of the zonal means (tests/zonal_cases.py): the yardstick of tests/test_zonal_means_gpu.py is pinned
here against a per-cell loop in pure Python, against np.mean of the float64 frame, and on fields that are constant in x."""
import math
from fractions import Fraction

import numpy as np
import pytest

import output_cases as OC
import zonal_cases as ZC

LD = np.longdouble


def _loop_terms(q1, q2, h, A, Nx, Ny, Hx, Hy, dx, dy, form, j0, j1):
    """The fourteen terms of every cell, one Python float operation at a time, in the order the header documents."""
    q1, q2, h, A = (np.asarray(a, dtype=np.float64).tolist() for a in (q1, q2, h, A))
    at = lambda a, i, j: a[Hy + j][Hx + i]
    U = lambda i, j: at(q1, i, j) if form == 1 else at(q1, i, j) / (0.5 * (at(h, i - 1, j) + at(h, i, j)))
    V = lambda i, j: at(q2, i, j) if form == 1 else at(q2, i, j) / (0.5 * (at(h, i, j - 1) + at(h, i, j)))
    BX = lambda i, j: -((at(A, i, j) - at(A, i, j - 1)) / dy) / (0.5 * (at(h, i, j - 1) + at(h, i, j)))
    BY = lambda i, j: ((at(A, i, j) - at(A, i - 1, j)) / dx) / (0.5 * (at(h, i - 1, j) + at(h, i, j)))
    out = np.empty((len(ZC.NAMES), j1 - j0, Nx))
    for j in range(j0, j1):
        for i in range(Nx):
            u, v, bx, by = U(i, j), V(i, j), BX(i, j), BY(i, j)
            g00, g10, g01, g11 = V(i - 1, j), V(i, j), V(i - 1, j + 1), V(i, j + 1)
            out[:, j - j0, i] = [
                u, v, at(h, i, j), at(A, i, j),
                math.sqrt(u * u + 0.5 * (0.5 * (g00 * g00 + g10 * g10) + 0.5 * (g01 * g01 + g11 * g11))),
                bx, by, u * u, v * v,
                u * (0.5 * (0.5 * (g00 + g10) + 0.5 * (g01 + g11))),
                bx * bx, by * by,
                by * (0.5 * (0.5 * (BX(i - 1, j) + BX(i, j)) + 0.5 * (BX(i - 1, j + 1) + BX(i, j + 1)))),
                v * (0.5 * (at(A, i, j - 1) + at(A, i, j)))]
    return out


@pytest.mark.parametrize("form", [1, 0])
@pytest.mark.parametrize("dtype", [ZC.F64, ZC.F32])
def test_reference_equals_a_per_cell_loop(form, dtype):
    """7 x 5 cells, halo (2, 3), rows (1, 4): terms bitwise those of the loop; means the exact rational mean, rounded once to longdouble."""
    Nx, Ny, Hx, Hy, rows = 7, 5, 2, 3, (1, 4)
    c = ZC.Case(Nx, Ny, Hx, Hy, True, rows, form, dtype, ZC.ALL, 0)
    q = ZC.inputs(c)
    dx, dy = ZC.spacing(dtype)
    terms = ZC.np_terms(*q, Nx, Ny, Hx, Hy, dx, dy, form, rows=rows)
    loop = _loop_terms(*q, Nx, Ny, Hx, Hy, dx, dy, form, *rows)
    assert np.isfinite(terms).all() and np.array_equal(terms, loop)
    want, sumabs = ZC.expected(c)
    assert want.shape == (14, 3) and want.dtype == LD
    for k in range(14):
        for r in range(3):
            exact = sum(Fraction(float(t)) for t in loop[k, r]) / Nx
            assert abs(Fraction(float(want[k, r])) - exact) <= abs(exact) * Fraction(1, 2 ** 52), (k, r)     # (want itself: one longdouble rounding)
            assert float(sumabs[k, r]) == pytest.approx(float(np.abs(loop[k, r]).sum()), rel=1e-14)
    # a sub-mask is the rows of the whole, in bit order
    sub = ZC.reference(q, Nx, Ny, Hx, Hy, dx, dy, form, rows, ZC.SPARSE)[0]
    assert np.array_equal(sub, want[[0, 4, 13]])


@pytest.mark.parametrize("Nx", [1, 5, 64, 257, 513])
def test_first_moment_is_the_mean_of_the_float64_frame(Nx):
    """np.mean sums pairwise in blocks: its error is far inside D(Nx) roundings for Nx > 1 and, like the kernel's, zero for Nx = 1."""
    Ny, H = 4, 3
    c = ZC.Case(Nx, Ny, H, H, False, None, 0, ZC.F64, ZC.ALL, 0)
    q = ZC.inputs(c)
    want, sumabs = ZC.expected(c)
    frame = OC.np_output_fields(*q, Nx, Ny, H, H, ZC.DX, ZC.DY, 0)
    assert np.array_equal(frame, ZC.np_terms(*q, Nx, Ny, H, H, ZC.DX, ZC.DY, 0, names=OC.NAMES))
    fails, ratio = ZC.compare(frame.mean(axis=-1), want[:7], sumabs[:7], Nx)
    print(f"Nx = {Nx}: np.mean within {ratio:.3f} of the bound")
    assert not fails, fails[:5]
    if Nx == 1:
        assert ZC.depth(1) == 0 and np.array_equal(frame[..., 0], want[:7].astype(np.float64))


def test_bound_is_tight_enough_to_catch_a_lost_term():
    """Dropping the last cell of a row, or averaging over Nx + 1, is far outside the bound."""
    Nx, Ny, H = 257, 2, 3
    c = ZC.Case(Nx, Ny, H, H, False, None, 1, ZC.F64, ZC.ALL, 0)
    terms = ZC.np_terms(*ZC.inputs(c), Nx, Ny, H, H, ZC.DX, ZC.DY, 1)
    want, sumabs = ZC.expected(c)
    assert len(ZC.compare(terms[..., :-1].sum(axis=-1) / Nx, want, sumabs, Nx)[0]) == want.size
    assert len(ZC.compare(terms.sum(axis=-1) / (Nx + 1), want, sumabs, Nx)[0]) == want.size
    assert not ZC.compare(want.astype(np.float64), want, sumabs, Nx)[0]


@pytest.mark.parametrize("form", [1, 0])
def test_a_field_constant_in_x_returns_that_constant(form):
    """Every term of a row is the same double t; the exact mean is t, and so is the reference."""
    Nx, Ny, H = 37, 3, 2
    rng = np.random.default_rng(3)
    col = lambda lo, hi: np.repeat(lo + (hi - lo) * rng.random((Ny + 2 * H, 1)), Nx + 2 * H, axis=1)
    q = [col(-1, 1), col(-1, 1), col(1.0, 1.3), col(-1, 1)]
    terms = ZC.np_terms(*q, Nx, Ny, H, H, ZC.DX, ZC.DY, form)
    assert np.array_equal(terms, np.repeat(terms[..., :1], Nx, axis=-1))
    want, _ = ZC.reference(q, Nx, Ny, H, H, ZC.DX, ZC.DY, form, (0, Ny), ZC.ALL)
    assert np.array_equal(want.astype(np.float64), terms[..., 0]) and np.array_equal(want, terms[..., 0].astype(LD))
    assert np.array_equal(terms[6], np.zeros((Ny, Nx)))        # B_y = dA/dx / h


def test_inputs_are_nan_outside_the_ring():
    for c in ZC.cases():
        j0, j1 = ZC.rows_of(c)
        q = ZC.inputs(c)
        keep = ZC.keep_mask(q[0].shape, c.Nx, c.Ny, c.Hx, c.Hy, j0, j1, c.wrap)
        assert q[0].shape == (c.Ny + 2 * c.Hy, ZC.stride_y(c)) and q[0].dtype == c.dtype
        for a in q:
            assert np.isnan(a[~keep]).all() and np.isfinite(a[keep]).all()
        if c.wrap & ZC.WRAP_X:
            assert not keep[:, :c.Hx].any() and not keep[:, c.Hx + c.Nx:].any()
        if c.wrap & ZC.WRAP_Y:
            assert not keep[:c.Hy].any() and not keep[c.Hy + c.Ny:].any()
        want, sumabs = ZC.expected(c)
        assert want.shape == (bin(c.which).count("1"), j1 - j0) and np.isfinite(want.astype(np.float64)).all()


def test_case_list_covers_what_the_kernel_can_get_wrong():
    cs = ZC.cases()
    assert len({ZC.case_id(c) for c in cs}) == len(cs)
    assert {c.Nx for c in cs} >= set(ZC.NXS) and {c.Ny for c in cs} >= set(ZC.NYS)
    assert {c.which for c in cs} >= set(ZC.BITS.values()) | {ZC.ALL, ZC.SPARSE}
    assert {c.form for c in cs} == {0, 1} and {np.dtype(c.dtype) for c in cs} == {np.dtype("f8"), np.dtype("f4")}
    assert any(c.pitch for c in cs) and any(c.Hx != c.Hy for c in cs) and any((c.Hx, c.Hy) == (1, 1) for c in cs)
    assert {(2, 5), (0, 0), (3, 4)} <= {c.rows for c in cs if c.rows}
    assert any(c.Nx == c.Hx and c.wrap & ZC.WRAP_X for c in cs) and any(c.Ny == 1 and c.wrap & ZC.WRAP_Y for c in cs)
    assert ZC.NAMES[:7] == OC.NAMES and [ZC.BITS[n] for n in OC.NAMES] == [1, 2, 4, 8, 16, 32, 64] and ZC.ALL == 16383
