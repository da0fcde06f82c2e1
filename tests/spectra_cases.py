"""Reference of ONE call of the zonal-spectrum entry points (swmhd_zonal_spectra_*, swmhd_ensemble_zonal_spectra_* in
include/swmhd_spectra.h) and the list of calls that tests/test_zonal_spectra_gpu.py runs through k_spectra_rows / k_spectra_sum
(swmhd_amd/csrc/spectra.hip).  numpy only: no GPU, no torch.  Pinned on the CPU by tests/test_spectra_cases_cpu.py.

Reference.  The frame values in IEEE double from output_cases.np_output_fields (bitwise the float64 frame, so bitwise the input of the
kernel's transform), then a DFT of every row in np.longdouble: the direct O(N^2) sum for Nx <= 256, a longdouble radix-2 FFT above,
pinned to the direct one at Nx <= 256.
    F^_j[k] = (1/Nx) sum_i F(i,j) exp(-2 pi i k (i-1)/Nx),   p_j[k] = c_k |F^_j[k]|^2,  c_k = 1 at k = 0 and k = Nx/2, else 2,
    P[k] = mean over the rows of p_j[k],  k = 0 .. Nx/2.

Bound.  Per row, with S_j = sum over all Nx modes of |F^_j[k]|^2 (the row's mean square) and eps = eta log2(Nx) 2^-53:
    |got_j[k] - p_j[k]| <= c_k (2 |F^_j[k]| eps sqrt(S_j) + eps^2 S_j).
The bound of P[k] is the mean of the row bounds, plus D_rows 2^-53 P[k] for the row summation (all terms are >= 0, so sum|term| is the
sum), plus 2^-53 P[k] for the rounding of the quotient.  This is the normwise FFT bound (Higham, Accuracy and Stability of Numerical
Algorithms, 2nd ed., Thm 24.2) applied per mode: |error of mode k| <= ||error||_2 <= eps ||F^||_2 = eps sqrt(S).

eta = ETA = 9.66, derived from the kernel's butterfly and twiddle source (the same derivation stands in include/swmhd_spectra.h), u = 2^-53:
  * a stage whose computed factor is off by at most eta_b u in every 2x2 block perturbs the result normwise by eta_b u; L stages by
    L eta_b u to first order (the proof of Thm 24.2);
  * the kernel's radix-2 decimation-in-frequency butterfly is y0 = a + b, y1 = (a - b) w: the subtraction rounds once per component
    (u), the complex product -- four multiplications, two additions, no contraction -- by sqrt(2) gamma_2 (Higham Lemma 3.5), and the
    stored twiddle is off by mu: eta_b u = mu + gamma_4 (sqrt(2) + mu), Higham's radix-2 constant;
  * twiddles come from sincospi of the exact fraction 2k/Nx, k < Nx/4 (the other quarter is -i times these: a swap and a sign, exact);
    sincospi is accurate to 2 ulp per component = 4u relative, hence mu = 4u and eta_b = 4 + 4 sqrt(2) = 9.657 -> 9.66;
  * the transform is a half-length complex one (log2 Nx - 1 stages) whose last two stages have the twiddles 1 and -i only (exact
    products: u each), followed by the untangling pass, which is two stages: sums and differences (u; the halving is exact) and
    E + w O (product, then sum: eta_b u);
  * the scaling by 1/Nx is exact; re^2 + im^2 rounds three times on positive terms: 2u of p_j[k], which is 1u in eps as |F^[k]| <= sqrt(S);
  * in all eps / u <= (log2 Nx - 2) eta_b + 4 (Nx >= 8) and eta_b + 3 (Nx = 4): at most log2(Nx) eta_b, with 2 eta_b - 4 = 15 u left
    over, thirteen orders above the second-order terms.  No slack factor.
RFFT_ETA = 5.66 is the same constant with exact twiddles (mu = 0): what numpy.fft.rfft in double is held to on the CPU, to show that the
bound is not wrong in the tight direction.

D_rows (depth): pass 1 gives W = min(rows, 256) partial spectra, workgroup w adding its rows w, w + W, ... one after the other from 0.0
(ceil(rows/W) - 1 rounded additions); pass 2 adds them with 16 lanes, lane g taking the partials g, g + 16, ... the same way
(ceil(W/16) - 1), then a tree of ceil(log2(min(16, W))) levels that round.  launch_plan.hpp states the same function (spectra_depth);
tests/test_spectra_plan_cpu.py compares the two.

Inputs.  zonal_cases' parents: random fields with h in [1, 1.3], every parent element outside the one-cell ring of the requested rows
NaN; with a WRAP flag the halo of that direction is NaN too and the ring holds the periodic images."""
import functools
from collections import namedtuple

import numpy as np

import output_cases as OC
import zonal_cases as ZC

LD = np.longdouble
ETA = 9.66
RFFT_ETA = 5.66
WMAX, P2_G = 256, 16
MIN_LOG2, MAX_LOG2 = 2, 12
DIRECT_MAX = 256
NAMES = OC.NAMES
BITS = {n: 1 << k for k, n in enumerate(NAMES)}
ALL = 127
WRAP_X, WRAP_Y = ZC.WRAP_X, ZC.WRAP_Y
F64, F32 = np.float64, np.float32
DX, DY, PAD = ZC.DX, ZC.DY, ZC.PAD
U53 = LD(2.0) ** -53


def names_of(which):
    return tuple(n for n in NAMES if which & BITS[n])


def plan_W(rows):
    return min(rows, WMAX)


def depth(rows):
    """D_rows of the bound (module docstring)."""
    if rows <= 0:
        return 0
    W = plan_W(rows)
    return (-(-rows // W) - 1) + (-(-W // P2_G) - 1) + (min(W, P2_G) - 1).bit_length()


def workspace(Nx, rows, nfields, members):
    """doubles of workspace a call needs: swmhd_zonal_spectra_workspace"""
    if min(Nx, rows, nfields, members) <= 0:
        return 0
    return plan_W(rows) * nfields * members * (Nx // 2 + 1)


PI = 4 * np.arctan(LD(1))


@functools.lru_cache(maxsize=None)
def _roots(N):
    """exp(-2 pi i k / N), k = 0 .. N-1, as (cos, -sin) longdouble arrays, from the first octant by symmetry"""
    c, s = np.empty(N, dtype=LD), np.empty(N, dtype=LD)
    for i in range(N):
        o, r = divmod(8 * i, N)              # octant and remainder: angle = (o + r/N) pi/4
        a = LD(r) / LD(N) * PI / LD(4)
        if o % 2 == 1:
            a = PI / LD(4) - a
        ca, sa = np.cos(a), np.sin(a)
        cc, ss = [(ca, sa), (sa, ca), (-sa, ca), (-ca, sa), (-ca, -sa), (-sa, -ca), (sa, -ca), (ca, -sa)][o]
        c[i], s[i] = cc, ss
    return c, -s


def dft_direct(x):
    """(re, im) longdouble (..., N): sum_i x[i] exp(-2 pi i k i / N), the O(N^2) sum"""
    x = np.asarray(x, dtype=LD)
    N = x.shape[-1]
    c, ms = _roots(N)
    idx = (np.arange(N)[:, None] * np.arange(N)[None, :]) % N      # [k, i]
    return x @ c[idx].T, x @ ms[idx].T


def fft_ld(x):
    """(re, im) longdouble (..., N), N = 2^p: recursive radix-2 decimation in time in longdouble"""
    x = np.asarray(x, dtype=LD)
    N = x.shape[-1]
    c, ms = _roots(N)

    def rec(re, im, n):
        if n == 1:
            return re, im
        er, ei = rec(re[..., 0::2], im[..., 0::2], n // 2)
        orr, oi = rec(re[..., 1::2], im[..., 1::2], n // 2)
        wr, wi = c[::N // n][:n // 2], ms[::N // n][:n // 2]
        tr, ti = orr * wr - oi * wi, orr * wi + oi * wr
        return np.concatenate([er + tr, er - tr], axis=-1), np.concatenate([ei + ti, ei - ti], axis=-1)
    return rec(x, np.zeros_like(x), N)


def row_modes(frames):
    """F^ of every row: (re, im) longdouble (..., Nx), all Nx modes, scaled by 1/Nx"""
    Nx = frames.shape[-1]
    re, im = dft_direct(frames) if Nx <= DIRECT_MAX else fft_ld(frames)
    return re / LD(Nx), im / LD(Nx)


def spectrum_of_frames(frames, eta=ETA):
    """frames (..., rows, Nx) float64 -> (want, bound): P[k] and its bound as longdouble (..., Nx/2 + 1).  A row with a non-finite value
    makes the whole spectrum non-finite."""
    frames = np.asarray(frames, dtype=np.float64)
    rows, Nx = frames.shape[-2:]
    half = Nx // 2
    with np.errstate(invalid="ignore", over="ignore"):
        re, im = row_modes(frames)
        mag2 = re * re + im * im
        S = mag2.sum(axis=-1, keepdims=True)
        ck = np.full(half + 1, 2, dtype=LD)
        ck[0] = ck[half] = 1
        p = ck * mag2[..., :half + 1]
        eps = LD(eta) * LD(int(np.log2(Nx))) * U53
        rowb = ck * (2 * np.sqrt(mag2[..., :half + 1]) * eps * np.sqrt(S) + eps * eps * S)
        want = p.sum(axis=-2) / LD(rows)
        bound = rowb.sum(axis=-2) / LD(rows) + LD(depth(rows)) * U53 * want + U53 * want
    return want, bound


def compare(got, want, bound):
    """got (float64 spectra of the kernel) against spectrum_of_frames(): (failures, ratio)"""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    fails, ratio = [], 0.0
    for idx in np.ndindex(*want.shape):
        g, w, b = got[idx], want[idx], bound[idx]
        if not np.isfinite(w):
            if np.isfinite(g):
                fails.append(f"{idx}: got {g!r}, want {float(w)!r}")
            continue
        err = float(abs(LD(g) - w)) if np.isfinite(g) else float("inf")
        if b > 0:
            ratio = max(ratio, err / float(b))
        if not err <= b:
            fails.append(f"{idx}: got {g!r}, want {float(w)!r}: error {err:.3e} > bound {float(b):.3e}")
    return fails, ratio


same_bits = ZC.same_bits

# rows: None = all rows, else (j0, j1); pitch: stride_y = Nx + 2 Hx + 5; wrap: SWMHD_WRAP_X | SWMHD_WRAP_Y bits
Case = namedtuple("Case", "Nx Ny Hx Hy pitch rows form dtype which wrap")
stride_y, rows_of = ZC.stride_y, ZC.rows_of


def case_id(c):
    j0, j1 = rows_of(c)
    mask = "all" if c.which == ALL else "+".join(names_of(c.which))
    return (f"{c.Nx}x{c.Ny}-H{c.Hx}{c.Hy}{'-pitch' if c.pitch else ''}{'' if c.rows is None else f'-rows{j0}to{j1}'}-"
            f"{'vi' if c.form == 1 else 'cons'}-{'f64' if np.dtype(c.dtype) == np.float64 else 'f32'}-{mask}"
            f"{'-wrapx' if c.wrap & WRAP_X else ''}{'-wrapy' if c.wrap & WRAP_Y else ''}")


NXS = tuple(1 << p for p in range(MIN_LOG2, MAX_LOG2 + 1))
NYS = (1, 2, 7)
W_ROWS = (WMAX - 1, WMAX, WMAX + 1, 2 * WMAX + 1)
SPARSE = BITS["u"] | BITS["s"] | BITS["B_y"]


def cases():
    """The case list: plain data.  Every log2 Nx from 2 to 12 with 1, 2 and 7 rows; formulation, precision and mask rotate through the
    sizes so that every size sees both formulations and both precisions; the full mask at the small sizes."""
    out = []
    for p, Nx in enumerate(NXS):
        for k, Ny in enumerate(NYS):
            small = Nx <= 256
            out.append(Case(Nx, Ny, 3, 4, False, None, (p + k) % 2, F64, ALL if small else (BITS["u"] | BITS["B_x"], BITS["s"], BITS["v"] | BITS["B_y"])[k], 0))
            out.append(Case(Nx, Ny, 3, 4, bool(k % 2), None, (p + k + 1) % 2, F32, ALL if Nx <= 64 else (BITS["s"], BITS["A"] | BITS["B_y"], BITS["u"])[k], 0))
    # each single-bit mask and a non-contiguous one, both formulations, minimal halo, two sizes (odd and even log2)
    for form in (1, 0):
        for Nx in (8, 64):
            for n in NAMES:
                out.append(Case(Nx, 7, 1, 1, False, None, form, F64, BITS[n], 0))
            out.append(Case(Nx, 7, 3, 4, True, None, form, F64, SPARSE, 0))
    # row counts around W and 2W at Nx = 8 and 64: every workgroup count and a second and third trip of workgroup 0
    for Nx in (8, 64):
        for rows in W_ROWS:
            out.append(Case(Nx, rows, 1, 1, False, None, 1 if Nx == 8 else 0, F64, BITS["u"] if Nx == 64 else BITS["B_x"] | BITS["h"], 0))
    # one odd row count at Nx = 4096
    out.append(Case(4096, 5, 3, 4, True, None, 0, F64, BITS["v"], 0))
    # row sub-ranges (and empty ones), pitched strides
    for rows in ((0, 7), (2, 5), (0, 1), (6, 7), (3, 4), (0, 0), (7, 7), (4, 4)):
        out.append(Case(32, 7, 3, 4, False, rows, 1, F64, ALL, 0))
        out.append(Case(16, 7, 3, 4, True, rows, 0, F32, ALL, 0))
    # WRAP flags on NaN halos: Ny = 1 (rows -1, 0 and 1 are the same row), each flag alone
    for Nx, Ny in ((4, 1), (4, 7), (8, 2), (64, 1), (256, 7), (512, 2)):
        for form, dtype in ((1, F64), (0, F64), (0, F32)):
            out.append(Case(Nx, Ny, 3, 4, False, None, form, dtype, ALL, WRAP_X | WRAP_Y))
    for wrap in (WRAP_X, WRAP_Y):
        out.append(Case(64, 7, 3, 4, True, None, 0, F64, ALL, wrap))
        out.append(Case(64, 7, 3, 4, False, (2, 5), 1, F64, ALL, wrap))
        out.append(Case(4, 1, 3, 4, False, None, 0, F32, ALL, wrap))
    return out


@functools.lru_cache(maxsize=8)
def inputs(c):
    """The four parents (q1, q2, h, A) of a case in its precision, shape (Ny + 2 Hy, stride_y).  Do not modify them."""
    j0, j1 = rows_of(c)
    return ZC._parents(c.Nx, c.Ny, c.Hx, c.Hy, stride_y(c), c.dtype, j0, j1, c.wrap)


spacing = ZC.spacing


def frames_of(parents, Nx, Ny, Hx, Hy, dx, dy, form, rows, which, wrap=0):
    """(popcount(which), j1 - j0, Nx) float64: the frame values a call transforms"""
    q = ZC.wrap_ring(parents, Nx, Ny, Hx, Hy, wrap)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        return OC.np_output_fields(*q, Nx, Ny, Hx, Hy, dx, dy, form, names=names_of(which), rows=rows)


def reference(parents, Nx, Ny, Hx, Hy, dx, dy, form, rows, which, wrap=0, eta=ETA):
    """(want, bound) of one call: longdouble arrays (popcount(which), Nx/2 + 1); an empty row range: shape (popcount, 0)."""
    if rows[1] == rows[0]:
        z = np.zeros((len(names_of(which)), 0), dtype=LD)
        return z, z
    return spectrum_of_frames(frames_of(parents, Nx, Ny, Hx, Hy, dx, dy, form, rows, which, wrap), eta)


@functools.lru_cache(maxsize=None)
def expected(c):
    dx, dy = spacing(c.dtype)
    return reference(inputs(c), c.Nx, c.Ny, c.Hx, c.Hy, dx, dy, c.form, rows_of(c), c.which, c.wrap)


# ensembles: 3 members of one shape, halo (3, 4), each with data of its own; dense and pitched (a gap of NaN between members)
ENSEMBLE_MEMBERS, ENSEMBLE_GAP = ZC.ENSEMBLE_MEMBERS, ZC.ENSEMBLE_GAP
ENS_HX, ENS_HY = ZC.ENS_HX, ZC.ENS_HY
ensemble_member_inputs = ZC.ensemble_member_inputs


def ensemble_cases():
    """(Nx, Ny, form, dtype, pitched, rows | None, which, wrap)"""
    return [(8, 2, 1, F64, False, None, ALL, 0), (8, 2, 0, F32, True, None, ALL, 0), (64, 7, 1, F64, True, None, ALL, 0),
            (256, 1, 0, F32, True, None, ALL, 0), (64, 7, 0, F64, True, (2, 5), SPARSE, 0), (64, 7, 1, F64, True, None, ALL, WRAP_X | WRAP_Y),
            (64, 64, 0, F64, False, None, ALL, WRAP_X | WRAP_Y), (1024, 3, 1, F64, True, None, SPARSE, 0)]


def ensemble_case_id(e):
    Nx, Ny, form, dtype, pitched, rows, which, wrap = e
    return (f"{Nx}x{Ny}-{'vi' if form == 1 else 'cons'}-{'f64' if np.dtype(dtype) == np.float64 else 'f32'}{'-pitched' if pitched else ''}"
            f"{'' if rows is None else f'-rows{rows[0]}to{rows[1]}'}-{'all' if which == ALL else '+'.join(names_of(which))}{'-wrap' if wrap else ''}")
