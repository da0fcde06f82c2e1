"""Reference of ONE call of the zonal-mean entry points (swmhd_zonal_means_*, swmhd_ensemble_zonal_means_* in include/swmhd_zonal.h) and the
list of calls that tests/test_zonal_means_gpu.py runs through k_zonal_means (swmhd_amd/csrc/zonal.hip).  numpy only: no GPU, no torch.
Pinned on the CPU by tests/test_zonal_cases_cpu.py.

Reference.  The per-cell terms in IEEE double, in the operation order the header documents: the seven frame fields from
output_cases.np_output_fields, the seven products restated here.  Each row is summed exactly (diag_cases._exact_sum: math.fsum,
carried as a double-double) and divided by Nx in longdouble.

Bound.  |got - want| <= D(Nx) 2^-53 sum_i |term_i| / Nx  +  2^-53 |want|   (the rounding of the quotient).
D is the number of additions on the longest path from a term to the row sum in the kernel's tree, read off zonal.hip:
  * one wave64 per row; lane l owns the 4-cell chunks l, l + 64, l + 128, ...: TRIP = 256 cells per trip of the wave;
  * a lane adds its terms one after the other in x order, starting from 0.0 (the first addition is exact).  Lane 0 owns the most:
    terms0 = 4 floor(Nx / 256) + min(4, Nx mod 256), hence terms0 - 1 rounded additions;
  * a butterfly over lane distances 32, 16, .., 1 adds the 64 lane sums.  A level whose partner has no term adds 0.0, exactly; the
    levels that round are the bits of (lanes with terms - 1): ceil(log2(min(64, ceil(Nx / 4)))).
  D(Nx) = terms0 - 1 + levels.  D(1) = 0: the mean of one cell is the term.  launch_plan.hpp states the same function (zonal_depth);
  tests/test_zonal_plan_cpu.py compares the two.  An addition rounds by at most u / (1 + u) of its result, u = 2^-53, which is what makes
  D u sum|term| a bound without higher-order terms (Jeannerod & Rump 2013, "Improved error bounds for inner products in floating-point
  arithmetic", for sums along any tree of that height).  No slack factor.

Inputs.  Random fields with h in [1, 1.3]; every parent element outside the one-cell ring of the requested rows -- deeper halo cells,
pitch padding, rows beyond the range -- is NaN, so a read outside the stencil's footprint shows in the profile.  With SWMHD_WRAP_X /
_Y the halo of that direction is NaN too, and the ring holds the periodic images instead (row Ny - 1 for row -1, ...).

Shapes.  Nx: 1, 3 (below one vector chunk; = Hx: one period as wide as the halo), 4, 5 (one chunk, a ragged second), 63 / 64 / 65 (a
ragged 16th chunk, 16 lanes, a 17th), 255 / 256 / 257 (both sides of one wave trip: the kernel's trip is 256 cells, the issue's values
stand) and 513 (two trips and one cell of a third: only lane 0 makes it).  Ny: 1, 2, 7 (one wave of a workgroup, two, a second
workgroup of three)."""
import functools
from collections import namedtuple

import numpy as np

import diag_cases as DC
import output_cases as OC

LD = np.longdouble
WAVE, VEC = 64, 4
TRIP = WAVE * VEC
DX, DY = 0.11, 0.13                     # dx != dy; neither is a float32, so the fp32 rounding of each matters
PAD = 5
WRAP_X, WRAP_Y = 16, 32
NAMES = OC.NAMES + ("uu", "vv", "uv", "B_xB_x", "B_yB_y", "B_xB_y", "vA")
BITS = {n: 1 << k for k, n in enumerate(NAMES)}
ALL = (1 << len(NAMES)) - 1
F64, F32 = np.float64, np.float32


def depth(Nx):
    """D of the bound (module docstring)."""
    terms0 = VEC * (Nx // TRIP) + min(VEC, Nx % TRIP)
    lanes = min(WAVE, -(-Nx // VEC))
    return terms0 - 1 + (lanes - 1).bit_length()


def names_of(which):
    return tuple(n for n in NAMES if which & BITS[n])


def np_terms(q1, q2, h, A, Nx, Ny, Hx, Hy, dx, dy, form, names=NAMES, rows=None):
    """(len(names), rows, Nx) float64: the per-cell terms at indices 1..Nx x rows [j0, j1) from halo-padded parents (halos as given).
    form 1 = vector-invariant (q = u, v), 0 = conservative (q = uh, vh)."""
    j0, j1 = (0, Ny) if rows is None else rows
    q1, q2, h, A = (np.asarray(a, dtype=np.float64) for a in (q1, q2, h, A))
    dx, dy = np.float64(dx), np.float64(dy)
    S = lambda a, di, dj: a[Hy + j0 + dj:Hy + j1 + dj, Hx + di:Hx + di + Nx]
    U = lambda di, dj: S(q1, di, dj) if form == 1 else S(q1, di, dj) / (0.5 * (S(h, di - 1, dj) + S(h, di, dj)))
    V = lambda di, dj: S(q2, di, dj) if form == 1 else S(q2, di, dj) / (0.5 * (S(h, di, dj - 1) + S(h, di, dj)))
    BX = lambda di, dj: -((S(A, di, dj) - S(A, di, dj - 1)) / dy) / (0.5 * (S(h, di, dj - 1) + S(h, di, dj)))
    BY = lambda di, dj: ((S(A, di, dj) - S(A, di - 1, dj)) / dx) / (0.5 * (S(h, di - 1, dj) + S(h, di, dj)))

    def term(n):
        if n in OC.NAMES:
            return OC.np_output_fields(q1, q2, h, A, Nx, Ny, Hx, Hy, dx, dy, form, names=(n,), rows=(j0, j1))[0]
        if n == "uu":
            return U(0, 0) * U(0, 0)
        if n == "vv":
            return V(0, 0) * V(0, 0)
        if n == "uv":
            return U(0, 0) * (0.5 * (0.5 * (V(-1, 0) + V(0, 0)) + 0.5 * (V(-1, 1) + V(0, 1))))
        if n == "B_xB_x":
            return BX(0, 0) * BX(0, 0)
        if n == "B_yB_y":
            return BY(0, 0) * BY(0, 0)
        if n == "B_xB_y":
            return BY(0, 0) * (0.5 * (0.5 * (BX(-1, 0) + BX(0, 0)) + 0.5 * (BX(-1, 1) + BX(0, 1))))
        if n == "vA":
            return V(0, 0) * (0.5 * (S(A, 0, -1) + S(A, 0, 0)))
        raise KeyError(n)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        return np.stack([np.array(term(n), dtype=np.float64) for n in names]).reshape(len(names), j1 - j0, Nx)


def means_of_terms(terms):
    """(want, sumabs): the exact row means of terms (..., Nx) as longdouble, and sum_i |term_i| of every row."""
    lead, Nx = terms.shape[:-1], terms.shape[-1]
    flat = terms.reshape(-1, Nx)
    want, sumabs = np.empty(len(flat), dtype=LD), np.empty(len(flat), dtype=LD)
    for r, t in enumerate(flat):
        want[r] = DC._exact_sum(t.astype(LD)) / LD(Nx)
        sumabs[r] = DC._exact_sum(np.abs(t).astype(LD))
    return want.reshape(lead), sumabs.reshape(lead)


def bound(Nx, sumabs, want):
    """|got - want| <= D(Nx) 2^-53 sum|term| / Nx + 2^-53 |want| (module docstring), as a float64 array."""
    u = LD(2.0) ** -53
    with np.errstate(invalid="ignore"):
        return (LD(depth(Nx)) * u * sumabs / LD(Nx) + u * np.abs(want)).astype(np.float64)


def compare(got, want, sumabs, Nx):
    """got (float64 profiles of the kernel) against means_of_terms(): (failures, ratio) -- one line per violated entry and the largest
    |error| / bound over the finite entries (0.0 where the bound is 0 and the entry exact).  A non-finite reference entry (a NaN in
    the stencil) must be non-finite in the kernel's profile too."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    b = bound(Nx, sumabs, want)
    fails, ratio = [], 0.0
    for idx in np.ndindex(*want.shape):
        g, w = got[idx], want[idx]
        if not np.isfinite(w):
            if np.isfinite(g):
                fails.append(f"{idx}: got {g!r}, want {float(w)!r}")
            continue
        err = float(abs(LD(g) - w)) if np.isfinite(g) else float("inf")
        if b[idx] > 0:
            ratio = max(ratio, err / b[idx])
        if not err <= b[idx]:
            fails.append(f"{idx}: got {g!r}, want {float(w)!r}: error {err:.3e} > bound {b[idx]:.3e}")
    return fails, ratio


# rows: None = all rows, else (j0, j1); pitch: stride_y = Nx + 2 Hx + 5; wrap: SWMHD_WRAP_X | SWMHD_WRAP_Y bits
Case = namedtuple("Case", "Nx Ny Hx Hy pitch rows form dtype which wrap")


def stride_y(c):
    return c.Nx + 2 * c.Hx + (PAD if c.pitch else 0)


def rows_of(c):
    return (0, c.Ny) if c.rows is None else c.rows


def case_id(c):
    j0, j1 = rows_of(c)
    mask = "all" if c.which == ALL else "+".join(names_of(c.which))
    return (f"{c.Nx}x{c.Ny}-H{c.Hx}{c.Hy}{'-pitch' if c.pitch else ''}{'' if c.rows is None else f'-rows{j0}to{j1}'}-"
            f"{'vi' if c.form == 1 else 'cons'}-{'f64' if np.dtype(c.dtype) == np.float64 else 'f32'}-{mask}"
            f"{'-wrapx' if c.wrap & WRAP_X else ''}{'-wrapy' if c.wrap & WRAP_Y else ''}")


NXS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 513)
NYS = (1, 2, 7)
SPARSE = BITS["u"] | BITS["s"] | BITS["vA"]      # a non-contiguous mask


def cases():
    """The case list: plain data."""
    out = []
    # every Nx x Ny, all profiles, Hx != Hy: both formulations in fp64, and fp32 alternating between them
    for Nx in NXS:
        for k, Ny in enumerate(NYS):
            out.append(Case(Nx, Ny, 3, 4, False, None, 1, F64, ALL, 0))
            out.append(Case(Nx, Ny, 3, 4, False, None, 0, F64, ALL, 0))
            out.append(Case(Nx, Ny, 3, 4, False, None, k % 2, F32, ALL, 0))
    # each single-bit mask and the non-contiguous one, both formulations, on a ragged shape of two workgroups; the minimal halo
    for form in (1, 0):
        for n in NAMES:
            out.append(Case(65, 7, 1, 1, False, None, form, F64, BITS[n], 0))
        out.append(Case(65, 7, 3, 4, False, None, form, F64, SPARSE, 0))
        out.append(Case(65, 7, 3, 4, False, None, form, F32, SPARSE, 0))
    # row ranges: a strict sub-range, single rows at both ends and inside, empty ranges; pitched strides
    for rows in ((0, 7), (2, 5), (0, 1), (6, 7), (3, 4), (0, 0), (7, 7), (4, 4)):
        out.append(Case(257, 7, 3, 4, False, rows, 1, F64, ALL, 0))
        out.append(Case(5, 7, 3, 4, True, rows, 0, F32, ALL, 0))
    for Nx in (1, 5, 65, 257, 513):
        out.append(Case(Nx, 7, 3, 4, True, None, 0, F64, ALL, 0))
        out.append(Case(Nx, 2, 4, 3, True, (1, 2), 1, F32, SPARSE, 0))
    # WRAP flags on NaN halos: Nx = Hx (one period as wide as the halo), Ny = 1 (row -1, 0 and 1 are the same row), each flag alone
    for Nx, Ny in ((3, 1), (3, 7), (5, 2), (65, 1), (257, 7), (513, 2)):
        for form, dtype in ((1, F64), (0, F64), (0, F32)):
            out.append(Case(Nx, Ny, 3, 4, False, None, form, dtype, ALL, WRAP_X | WRAP_Y))
    for wrap in (WRAP_X, WRAP_Y):
        out.append(Case(65, 7, 3, 4, True, None, 0, F64, ALL, wrap))
        out.append(Case(65, 7, 3, 4, False, (2, 5), 1, F64, ALL, wrap))
        out.append(Case(3, 1, 3, 4, False, None, 0, F32, ALL, wrap))
    for rows in ((0, 3), (5, 7), (0, 0)):
        out.append(Case(65, 7, 3, 4, True, rows, 0, F64, ALL, WRAP_X | WRAP_Y))
    return out


def keep_mask(shape, Nx, Ny, Hx, Hy, j0, j1, wrap=0):
    """True on the one-cell ring of rows [j0, j1): rows j0 - 1 .. j1, columns -1 .. Nx (0-based interior indices), with the periodic
    image in place of the halo cell in a wrapped direction; an empty range has no ring."""
    keep = np.zeros(shape, dtype=bool)
    if j1 <= j0:
        return keep
    rows = [(j % Ny) if (wrap & WRAP_Y) else j for j in range(j0 - 1, j1 + 1)]
    cols = [(i % Nx) if (wrap & WRAP_X) else i for i in range(-1, Nx + 1)]
    keep[np.ix_([Hy + j for j in rows], [Hx + i for i in cols])] = True
    return keep


def _parents(Nx, Ny, Hx, Hy, sy, dtype, j0, j1, wrap, member=0):
    q = [np.ascontiguousarray(a.astype(dtype)) for a in DC._random_parents(Nx, Ny, Hx, Hy, sy, member=member)]
    keep = keep_mask(q[0].shape, Nx, Ny, Hx, Hy, j0, j1, wrap)
    for a in q:
        a[~keep] = np.nan
        a.setflags(write=False)
    return tuple(q)


@functools.lru_cache(maxsize=8)
def inputs(c):
    """The four parents (q1, q2, h, A) of a case in its precision, shape (Ny + 2 Hy, stride_y).  Do not modify them."""
    j0, j1 = rows_of(c)
    return _parents(c.Nx, c.Ny, c.Hx, c.Hy, stride_y(c), c.dtype, j0, j1, c.wrap)


def wrap_ring(parents, Nx, Ny, Hx, Hy, wrap):
    """float64 copies of the parents with the one-cell halo ring of the wrapped directions replaced by the periodic images (x first,
    so the corners hold the diagonal image): what a WRAP call reads, as plain halos."""
    out = []
    for a in parents:
        a = np.array(a, dtype=np.float64)
        if wrap & WRAP_X:
            a[:, Hx - 1], a[:, Hx + Nx] = a[:, Hx + Nx - 1].copy(), a[:, Hx].copy()
        if wrap & WRAP_Y:
            a[Hy - 1, :], a[Hy + Ny, :] = a[Hy + Ny - 1, :].copy(), a[Hy, :].copy()
        out.append(a)
    return out


def spacing(dtype):
    """dx, dy as the ABI receives them (rounded to float32 for the fp32 entry point)"""
    t = np.dtype(dtype).type
    return float(t(DX)), float(t(DY))


def reference(parents, Nx, Ny, Hx, Hy, dx, dy, form, rows, which, wrap=0):
    """(want, sumabs) of one call: longdouble arrays (popcount(which), j1 - j0)."""
    names = names_of(which)
    j0, j1 = rows
    if j1 == j0:
        z = np.zeros((len(names), 0), dtype=LD)
        return z, z
    q = wrap_ring(parents, Nx, Ny, Hx, Hy, wrap)
    return means_of_terms(np_terms(*q, Nx, Ny, Hx, Hy, dx, dy, form, names, rows))


@functools.lru_cache(maxsize=None)
def expected(c):
    """reference() of a case's inputs with this module's dx, dy (cached: a few numbers per case)."""
    dx, dy = spacing(c.dtype)
    return reference(inputs(c), c.Nx, c.Ny, c.Hx, c.Hy, dx, dy, c.form, rows_of(c), c.which, c.wrap)


def same_bits(a, b):
    """Two float64 arrays are the same values bit for bit, NaN equal to NaN (the payload of a NaN is not pinned)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.int64), b[~nan].view(np.int64)))


# ensembles: 3 members of one shape, halo (3, 4), each with data of its own; dense (stride_m = the parent) and pitched (a gap of NaN)
ENSEMBLE_MEMBERS = 3
ENSEMBLE_GAP = 11


def ensemble_cases():
    """(Nx, Ny, form, dtype, pitched, rows | None, which, wrap)"""
    out = []
    for Nx, Ny in ((5, 2), (65, 7), (257, 1)):
        out.append((Nx, Ny, 1, F64, False, None, ALL, 0))
        out.append((Nx, Ny, 0, F32, True, None, ALL, 0))
    out.append((65, 7, 0, F64, True, (2, 5), SPARSE, 0))
    out.append((65, 7, 1, F64, True, None, ALL, WRAP_X | WRAP_Y))
    out.append((64, 64, 0, F64, False, None, ALL, WRAP_X | WRAP_Y))      # the members of a sweep: 64 x 64
    return out


def ensemble_case_id(e):
    Nx, Ny, form, dtype, pitched, rows, which, wrap = e
    return (f"{Nx}x{Ny}-{'vi' if form == 1 else 'cons'}-{'f64' if np.dtype(dtype) == np.float64 else 'f32'}{'-pitched' if pitched else ''}"
            f"{'' if rows is None else f'-rows{rows[0]}to{rows[1]}'}-{'all' if which == ALL else '+'.join(names_of(which))}{'-wrap' if wrap else ''}")


ENS_HX, ENS_HY = 3, 4


@functools.lru_cache(maxsize=8)
def ensemble_member_inputs(Nx, Ny, dtype, m, rows, wrap):
    """Parents of member m: shape (Ny + 2 ENS_HY, Nx + 2 ENS_HX), NaN outside the ring."""
    j0, j1 = (0, Ny) if rows is None else rows
    return _parents(Nx, Ny, ENS_HX, ENS_HY, Nx + 2 * ENS_HX, dtype, j0, j1, wrap, member=m)
