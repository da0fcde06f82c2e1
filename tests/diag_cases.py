"""Reference of ONE call of the diagnostics entry points (swmhd_diagnostics_*, swmhd_ensemble_diagnostics_* in include/swmhd.h) and the
list of calls that tests/test_diag_matrix_gpu.py runs through k_diag_partial / k_diag_final (swmhd_amd/csrc/diagnostics.hip).  numpy
only: no GPU, no torch.  Pinned on the CPU by tests/test_diag_cases_cpu.py.

The reference evaluates the per-cell terms of the header of diagnostics.hip in np.longdouble from the inputs widened exactly, with
dx, dy, g, h_ref as the call receives them (rounded to float32 for the fp32 entry point), and sums them exactly (math.fsum over the
double-double split of every term).  The extrema are taken with np.max / np.min, which propagate NaN like the maximum / minimum of
the reference's progress callback (SWMHD_example.jl:47-65), and are evaluated in DOUBLE: |u|, |A| and h are exact, and the conservative
form's uh / (1/2 (h- + h)) is one correctly rounded division of an exactly halved, once rounded sum -- the kernel's value bit for bit.

Structure of the kernel the shapes are chosen for: NT = 256 threads per block, NB = 1024 blocks, so TRIP = 262 144 cells per trip of
the grid-stride loop; cell e of a call is (x, y) = (e % Nx, j0 + e // Nx).

Inputs: random fields with h in [1, 1.3]; every parent element outside the +-1 ring of the requested rows -- deeper halo cells, pitch
padding, rows beyond the range -- is NaN, so a read outside the stencil's footprint shows in the sums."""
import functools
import math
from collections import namedtuple

import numpy as np

NT, NB, NQ = 256, 1024, 7
TRIP = NT * NB
DX, DY, GRAV, HREF = 0.11, 0.13, 9.81, 1.1       # dx != dy; none of them is a float32, so the fp32 rounding of each one matters
NAMES = ("kinetic_energy", "magnetic_energy", "potential_energy", "max_abs_u", "max_abs_v", "max_abs_A", "min_h")
EMPTY = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1e300)    # what an empty row range returns: the identity element of the fold
LD = np.longdouble

# Roundings of the longest per-cell expression of k_diag_partial, the magnetic energy: a face value B = ((A - A') * rd) / (0.5 * (h' + h))
# has 5 (the difference, rd = 1 / d, the product, the sum of h, the quotient; the halving is exact); its square doubles that relative
# error and rounds once (11); then c00^2 + c10^2, the sum of the two halved pairs, b^2 + (...), Z(0) + Z(1) and the product with
# 0.5 h (5 more; every halving is exact): 16.  All addends are squares times positive h, so the relative errors do not amplify.  The
# kinetic energy has 8 (form 0: 1 / h included), the potential energy 3.  Doubled for FMA contraction (-ffp-contract=fast).
R_CELL = 2 * 16


def depth(ncell):
    """D of the tolerance: serial trips of a thread + 8 tree levels (256 threads) + 4 serial partials per thread of the final fold + 8
    tree levels + 1 for the scale dx dy."""
    return -(-ncell // TRIP) + 8 + 4 + 8 + 1


def energy_bound(ncell, sumabs):
    """|got - want| <= (R + D) 2^-53 sum|term| (terms scaled by dx dy)."""
    return float((R_CELL + depth(ncell)) * 2.0 ** -53 * float(sumabs))


# rows: None = all rows, else (j0, j1); nonfinite: None or (field name, value name); pitch: stride_y = Nx + 2 Hx + 5
Case = namedtuple("Case", "Nx Ny Hx Hy pitch rows form dtype nonfinite")
NONFINITE = {"nan": np.nan, "inf": np.inf}
FIELD = {"u": 0, "v": 1, "h": 2, "A": 3}
PAD = 5


def stride_y(c):
    return c.Nx + 2 * c.Hx + (PAD if c.pitch else 0)


def rows_of(c):
    return (0, c.Ny) if c.rows is None else c.rows


def ncell_of(c):
    j0, j1 = rows_of(c)
    return c.Nx * (j1 - j0)


def case_id(c):
    j0, j1 = rows_of(c)
    return (f"{c.Nx}x{c.Ny}-H{c.Hx}{c.Hy}{'-pitch' if c.pitch else ''}{'' if c.rows is None else f'-rows{j0}to{j1}'}-"
            f"{'vi' if c.form == 1 else 'cons'}-{'f64' if np.dtype(c.dtype) == np.float64 else 'f32'}"
            f"{'' if c.nonfinite is None else '-' + c.nonfinite[1] + '_in_' + c.nonfinite[0]}")


SHAPES = [(1, 1), (5, 4), (255, 1), (256, 1), (257, 1),     # one cell; a few; below, at and above one block
          (37, 21), (200, 75),
          (513, 512),        # 512 cells beyond one trip: only the threads of two blocks make a second trip
          (1030, 255),       # 506 cells beyond one trip, no multiple of 256: the last block of the second trip is ragged
          (1024, 520)]       # two full trips and 8192 cells of a third
REDUCED = [(5, 4), (257, 1), (37, 21), (513, 512)]
F64, F32 = np.float64, np.float32


def cases():
    """The case list: plain data."""
    out = []
    # every shape, both formulations, both precisions: whole range, halo (3, 3)
    for Nx, Ny in SHAPES:
        for form in (1, 0):
            for dtype in (F64, F32):
                out.append(Case(Nx, Ny, 3, 3, False, None, form, dtype, None))
    # halos: (1, 1) is the documented minimum (the ring is the whole parent), (2, 5) has Hx != Hy; then a pitched stride_y
    for Nx, Ny in REDUCED:
        for Hx, Hy in ((1, 1), (2, 5)):
            for form, dtype in ((1, F64), (0, F32)):
                out.append(Case(Nx, Ny, Hx, Hy, False, None, form, dtype, None))
        for form, dtype in ((0, F64), (1, F32)):
            out.append(Case(Nx, Ny, 3, 3, True, None, form, dtype, None))
    out.append(Case(37, 21, 2, 5, True, None, 1, F64, None))
    out.append(Case(37, 21, 1, 1, True, None, 0, F32, None))
    # row ranges: a strict sub-range, single rows at both ends, empty ranges at both ends and inside
    for Nx, Ny, Hx, Hy, pitch, ranges in (
            (5, 4, 1, 1, False, [(1, 3), (0, 1), (3, 4), (0, 0), (4, 4), (2, 2)]),
            (37, 21, 3, 3, False, [(5, 17), (0, 1), (20, 21), (0, 0), (21, 21), (9, 9)]),
            (37, 21, 2, 5, True, [(5, 17), (0, 1), (20, 21), (7, 7)]),
            (257, 1, 3, 3, False, [(0, 0), (1, 1)]),
            (513, 512, 3, 3, False, [(0, 1), (511, 512), (300, 300)]),
            (1024, 520, 2, 5, True, [(2, 519)])):          # 517 rows: two full trips and more, from a row that is not the first
        for rows in ranges:
            for form, dtype in ((1, F64), (0, F32)):
                out.append(Case(Nx, Ny, Hx, Hy, pitch, rows, form, dtype, None))
    # non-finite cells: one NaN in u, A, h in turn and one +Inf in u, both formulations; fp32; a NaN only a second trip reaches
    for form in (1, 0):
        for nf in (("u", "nan"), ("A", "nan"), ("h", "nan"), ("u", "inf")):
            out.append(Case(37, 21, 3, 3, False, None, form, F64, nf))
        out.append(Case(37, 21, 3, 3, False, None, form, F32, ("u", "nan")))
        out.append(Case(37, 21, 2, 5, True, (5, 17), form, F32, ("h", "nan")))
    out.append(Case(513, 512, 3, 3, False, None, 1, F64, ("v", "nan")))
    out.append(Case(513, 512, 3, 3, False, None, 0, F64, ("h", "nan")))
    return out


def nonfinite_cell(c):
    """(x, y) of the non-finite cell: inside the requested rows, away from their edges where the range allows; at 513 x 512 cell
    513 * 511 + 256 > TRIP, which only the second trip of one thread reaches."""
    j0, j1 = rows_of(c)
    if c.Nx * (j1 - j0) > TRIP:
        return c.Nx // 2, j1 - 1
    return c.Nx // 2, (j0 + j1) // 2


def clean(c):
    return c._replace(nonfinite=None)


def _random_parents(Nx, Ny, Hx, Hy, sy, member=0):
    shape = (Ny + 2 * Hy, sy)
    r = [np.random.default_rng([Nx, Ny, Hx, Hy, sy, member, k]) for k in range(4)]
    return [0.5 * r[0].standard_normal(shape), 0.5 * r[1].standard_normal(shape), 1.0 + 0.3 * r[2].random(shape), r[3].standard_normal(shape)]


def poison_outside_ring(a, Nx, Ny, Hx, Hy, j0, j1):
    """NaN in every parent element outside rows j0 - 1 .. j1 and columns -1 .. Nx (0-based interior indices), in place; an empty range
    has no ring."""
    keep = np.zeros(a.shape, dtype=bool)
    if j1 > j0:
        keep[Hy + j0 - 1:Hy + j1 + 1, Hx - 1:Hx + Nx + 1] = True
    a[~keep] = np.nan
    return a


@functools.lru_cache(maxsize=4)
def inputs(c):
    """The four parents (q1, q2, h, A) of a case in its precision, shape (Ny + 2 Hy, stride_y).  Do not modify them."""
    j0, j1 = rows_of(c)
    q = [np.ascontiguousarray(a.astype(c.dtype)) for a in _random_parents(c.Nx, c.Ny, c.Hx, c.Hy, stride_y(c))]
    for a in q:
        poison_outside_ring(a, c.Nx, c.Ny, c.Hx, c.Hy, j0, j1)
    if c.nonfinite is not None:
        x, y = nonfinite_cell(c)
        q[FIELD[c.nonfinite[0]]][c.Hy + y, c.Hx + x] = NONFINITE[c.nonfinite[1]]
    for a in q:
        a.setflags(write=False)
    return tuple(q)


def _exact_sum(t):
    """Sum of a longdouble array: exact (math.fsum of the double-double split of every term), returned as a longdouble to ~2^-106 of
    the sum; NaN / Inf terms: the plain sum, which propagates them."""
    t = np.ravel(t)
    if not np.isfinite(t).all():
        with np.errstate(invalid="ignore", over="ignore"):
            return LD(t.sum())
    hi = t.astype(np.float64)
    lo = (t - hi.astype(LD)).astype(np.float64)
    parts = hi.tolist() + lo.tolist()
    s = math.fsum(parts)
    return LD(s) + LD(math.fsum(parts + [-s]))


def reference(q1, q2, h, A, Nx, Ny, Hx, Hy, dx, dy, g, h_ref, form, j0, j1, dtype):
    """(out, sumabs): the 7 outputs of swmhd_diagnostics over rows [j0, j1) -- the three energies as longdouble, the four extrema as
    float64 -- and sum|term| of each energy (scaled by dx dy like the energies).  q1 .. A: parents of shape (Ny + 2 Hy, stride_y)."""
    t = np.dtype(dtype).type
    dx, dy, g, h_ref = (LD(t(x)) for x in (dx, dy, g, h_ref))      # as the ABI receives them
    if j0 == j1:
        return [LD(v) for v in EMPTY[:3]] + [np.float64(v) for v in EMPTY[3:]], [LD(0)] * 3
    W64 = lambda a, di, dj: a[Hy + j0 + dj:Hy + j1 + dj, Hx + di:Hx + di + Nx].astype(np.float64)      # exact widening
    S = lambda a, di, dj: W64(a, di, dj).astype(LD)
    half = LD(0.5)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        hc = S(h, 0, 0)
        Wf = lambda di: S(q1, di, 0) ** 2 + half * (half * (S(q2, di - 1, 0) ** 2 + S(q2, di, 0) ** 2) + half * (S(q2, di - 1, 1) ** 2 + S(q2, di, 1) ** 2))
        wbar = half * (Wf(0) + Wf(1))
        ke = half * (1 / hc) * wbar if form == 0 else half * hc * wbar
        BX = lambda di, dj: -((S(A, di, dj) - S(A, di, dj - 1)) / dy) / (half * (S(h, di, dj - 1) + S(h, di, dj)))
        BY = lambda di, dj: ((S(A, di, dj) - S(A, di - 1, dj)) / dx) / (half * (S(h, di - 1, dj) + S(h, di, dj)))
        Z = lambda dj: BX(0, dj) ** 2 + half * (half * (BY(0, dj - 1) ** 2 + BY(1, dj - 1) ** 2) + half * (BY(0, dj) ** 2 + BY(1, dj) ** 2))
        me = half * hc * (half * (Z(0) + Z(1)))
        pe = half * g * (hc - h_ref) ** 2
        cell = dx * dy
        energies = [_exact_sum(e) * cell for e in (ke, me, pe)]
        sumabs = [_exact_sum(np.abs(e)) * cell for e in (ke, me, pe)]
        # extrema: in double, as the kernel forms them
        h64 = W64(h, 0, 0)
        uw, vs = W64(q1, 0, 0), W64(q2, 0, 0)
        if form == 0:      # u = uh / h at uh's faces (divergence_sw_mhd.jl:45-47)
            uw, vs = uw / (0.5 * (W64(h, -1, 0) + h64)), vs / (0.5 * (W64(h, 0, -1) + h64))
        extrema = [np.max(np.abs(uw)), np.max(np.abs(vs)), np.max(np.abs(W64(A, 0, 0))), np.min(h64)]
    return energies + [np.float64(v) for v in extrema], sumabs


@functools.lru_cache(maxsize=None)
def expected(c):
    """reference() of a case's inputs with this module's dx, dy, g, h_ref (cached: a few numbers per case)."""
    j0, j1 = rows_of(c)
    return reference(*inputs(c), c.Nx, c.Ny, c.Hx, c.Hy, DX, DY, GRAV, HREF, c.form, j0, j1, c.dtype)


def same_bits(a, b):
    """Two doubles are the same value bit for bit, or both NaN (the payload of a NaN is not pinned)."""
    a, b = np.float64(a), np.float64(b)
    return bool((np.isnan(a) and np.isnan(b)) or a.tobytes() == b.tobytes())


def compare(got, want, sumabs, ncell):
    """got (7 doubles of the kernel) against reference(): (failures, ratio) -- one line per violated assertion, and the largest
    |error| / bound over the finite energies (0.0 if none)."""
    fails, ratio = [], 0.0
    for k in range(3):
        w, g = want[k], np.float64(got[k])
        if not np.isfinite(w):
            if not same_bits(g, np.float64(w)):
                fails.append(f"{NAMES[k]}: got {g!r}, want {w!r}")
            continue
        bound = energy_bound(ncell, sumabs[k])
        err = float(abs(LD(g) - w)) if np.isfinite(g) else float("inf")
        if bound > 0:
            ratio = max(ratio, err / bound)
        if not err <= bound:
            fails.append(f"{NAMES[k]}: got {g!r}, want {float(w)!r}: error {err:.3e} > bound {bound:.3e}")
    for k in range(3, NQ):
        if not same_bits(got[k], want[k]):
            fails.append(f"{NAMES[k]}: got {np.float64(got[k])!r}, want {want[k]!r} (must be equal bit for bit)")
    return fails, ratio


# ensembles: 3 members of one shape, halo (3, 3), each with data of its own, at a stride_m that leaves a gap of NaN between them
ENSEMBLE_SHAPES = [(257, 1), (37, 21), (513, 512)]
ENSEMBLE_MEMBERS = 3
ENSEMBLE_GAP = 11                   # elements of NaN between two members
ENSEMBLE_G = (9.81, 3.7, 24.79)     # per-member g of the _params case


def ensemble_cases():
    """(Nx, Ny, form, dtype, params, nonfinite member | None): every shape in both precisions, one of them with per-member g, one
    with a non-finite member."""
    out = []
    for Nx, Ny in ENSEMBLE_SHAPES:
        out.append((Nx, Ny, 1, F64, False, None))
        out.append((Nx, Ny, 0, F32, False, None))
    out.append((37, 21, 0, F64, True, None))
    out.append((37, 21, 1, F32, True, None))
    out.append((37, 21, 1, F64, False, 1))
    out.append((257, 1, 0, F32, False, 0))
    out.append((513, 512, 0, F64, False, 2))
    return out


def ensemble_case_id(e):
    Nx, Ny, form, dtype, params, bad = e
    return (f"{Nx}x{Ny}-{'vi' if form == 1 else 'cons'}-{'f64' if np.dtype(dtype) == np.float64 else 'f32'}"
            f"{'-params' if params else ''}{'' if bad is None else f'-member{bad}_nonfinite'}")


@functools.lru_cache(maxsize=8)
def ensemble_member_inputs(Nx, Ny, dtype, m, nonfinite):
    """Parents of member m: shape (Ny + 6, Nx + 6), poisoned outside the ring; nonfinite: NaN in h at the middle cell."""
    sy = Nx + 6
    q = [np.ascontiguousarray(a.astype(dtype)) for a in _random_parents(Nx, Ny, 3, 3, sy, member=m)]
    for a in q:
        poison_outside_ring(a, Nx, Ny, 3, 3, 0, Ny)
    if nonfinite:
        q[2][3 + Ny // 2, 3 + Nx // 2] = np.nan
    return tuple(q)
