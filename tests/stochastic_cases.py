"""Reference of the StochasticForcing (swmhd_stochastic_coefficients_* and swmhd_stochastic_rk3_* in include/swmhd_stochastic.h,
ShallowWaterModel(forcing={"u": s, "v": s, "A": s})) and the cases its tests run.  numpy and Python integers only (RefModel: + the CPU
oracle, through relaxation_cases.RefModel).

The pin is the written formula, restated here independently of swmhd_amd/stochastic.py:
    Philox4x32-10 -> two uniforms of 53 bits -> P = c (2 u1 - 1), Q = c (2 u2 - 1), c = amp0 / sqrt(dt)                  (coefficients)
    F = sum over m ascending of cx R + sx T,  R = P cy + Q sy,  T = Q cy - P sy                                          (synth_strict)
in double for the coefficients (cast to the element type at the end) and in the element type for the synthesis, one rounding per
operation.  synth_exact is the same value in longdouble with the scale S of its rounding error.  RefModel appends the term LAST to the
corrections of relaxation_cases.RefModel and counts steps: the coefficients are renewed once per step and held over its stages."""
import numpy as np

import relaxation_cases as RC

H = RC.H
MAX_MODES, MAX_FIELDS, MODE_CHUNK, TILE_ROWS = 256, 12, 4, 64
SCALAR, PAIR = 0, 1
M32 = 0xffffffff

# ---- Philox4x32-10 ---------------------------------------------------------------------------------------------------------------------
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((M32,) * 4, (M32,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox4x32_10(counter, key):
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def u53(hi, lo):
    """((hi >> 5) 2^26 + (lo >> 6)) 2^-53 as a float64: exact."""
    return np.float64(((hi >> 5) << 26) + (lo >> 6)) * np.float64(2.0 ** -53)


def draw(seed, stream, n, group, m):
    """(2 u1 - 1, 2 u2 - 1) of mode m of draw group `group` at step counter n (a Python integer, taken mod 2^64)."""
    n &= (1 << 64) - 1
    w = philox4x32_10((n & M32, n >> 32, (m + 65536 * group) & M32, stream & M32), (seed & M32, (seed >> 32) & M32))
    return np.float64(2.0) * u53(w[0], w[1]) - np.float64(1.0), np.float64(2.0) * u53(w[2], w[3]) - np.float64(1.0)


# ---- modes, wavenumbers, tables --------------------------------------------------------------------------------------------------------
MODE_COUNTS = [((64, 64), 8.0, 24), ((4096, 4096), 32.0, 94), ((4096, 4096), 64.0, 220), ((16, 12), 3.0, 8), ((5, 3), 1.0, 1)]   # 2π square, dk = 1


def forcing_modes(Nx, Ny, Lx, Ly, k_f, dk):
    out = []
    nxs = np.arange(0, Nx // 2)                      # 0 <= nx < Nx/2, |ny| < Ny/2 with the integer quotients
    nys = np.arange(-(Ny // 2) + 1, Ny // 2)
    for nx in nxs:
        k = np.hypot(2.0 * np.pi * nx / Lx, 2.0 * np.pi * nys / Ly)
        for ny in nys[(k >= k_f - dk / 2) & (k < k_f + dk / 2) & ((nx > 0) | (nys > 0))]:
            out.append((int(nx), int(ny)))
    return np.asarray(out, dtype=np.int64).reshape(-1, 2)


def wavenumbers(modes, Lx, Ly):
    return 2.0 * np.pi * modes[:, 0] / Lx, 2.0 * np.pi * modes[:, 1] / Ly


def modified(modes, Lx, Ly, dx, dy):
    kx, ky = wavenumbers(modes, Lx, Ly)
    return np.sin(kx * dx / 2) / (dx / 2), np.sin(ky * dy / 2) / (dy / 2)


def amp0(modes, rate, pair, Lx, Ly, dx, dy):
    a = np.full(len(modes), np.sqrt(6.0 * rate / len(modes)))
    return a / np.hypot(*modified(modes, Lx, Ly, dx, dy)) if pair else a


def nodes(N, d, face, x0=0.0):
    ii = np.arange(N)
    return x0 + ii * d if face else x0 + (ii + 0.5) * d


def tables(k, x, dtype):
    """(cos, sin)(k_m x_i) as (M, N) arrays, formed in float64 and rounded to `dtype`."""
    arg = k[:, None] * x[None, :]
    return np.cos(arg).astype(dtype), np.sin(arg).astype(dtype)


# ---- the coefficients ------------------------------------------------------------------------------------------------------------------
def coefficients(kind, amp, ktx, kty, seed, stream, n, group, sdt, dtype):
    """The coefficient pairs of one draw group at step counter n: SCALAR -> [(P, Q)], PAIR -> [(Pu, Qu), (Pv, Qv)], arrays (M,) of
    `dtype`; all arithmetic in float64, one rounding per operation, the cast last."""
    M = len(amp)
    x = np.empty(M)
    y = np.empty(M)
    for m in range(M):
        x[m], y[m] = draw(seed, stream, n, group, m)
    c = amp * np.float64(sdt)
    P, Q = c * x, c * y
    if kind == SCALAR:
        return [(P.astype(dtype), Q.astype(dtype))]
    return [((-(kty * Q)).astype(dtype), (kty * P).astype(dtype)), ((ktx * Q).astype(dtype), (-(ktx * P)).astype(dtype))]


# ---- the synthesis ---------------------------------------------------------------------------------------------------------------------
def synth_strict(cx, sx, cy, sy, P, Q):
    """F (Ny, Nx) in the precision of the tables, the strict operation order, m ascending."""
    F = np.zeros((cy.shape[1], cx.shape[1]), dtype=cx.dtype)
    for m in range(len(P)):
        R = P[m] * cy[m] + Q[m] * sy[m]
        T = Q[m] * cy[m] - P[m] * sy[m]
        F = F + cx[m][None, :] * R[:, None]
        F = F + sx[m][None, :] * T[:, None]
    return F


def synth_exact(cx, sx, cy, sy, P, Q):
    """(F, S) in longdouble from the values the kernel is given; S = 2 sum (|P| + |Q|)."""
    L = np.longdouble
    F = np.zeros((cy.shape[1], cx.shape[1]), dtype=L)
    for m in range(len(P)):
        p, q = L(P[m]), L(Q[m])
        R = p * cy[m].astype(L) + q * sy[m].astype(L)
        T = q * cy[m].astype(L) - p * sy[m].astype(L)
        F += cx[m].astype(L)[None, :] * R[:, None] + sx[m].astype(L)[None, :] * T[:, None]
    return F, 2 * (np.abs(np.asarray(P, dtype=L)).sum() + np.abs(np.asarray(Q, dtype=L)).sum())


# Fast tolerance, derived (include/swmhd_stochastic.h).  Tables of magnitude <= 1: S bounds the sum of the magnitudes of the 2 M terms
# cx R and sx T.  With u = eps/2, a term carries at most three roundings of its own (two inside R or T for each addend: its product and
# the sum; one for the product with cx or sx) and at most 2 M of the running sum; a F and the final sum add two:
#     |new - ref| <= u |ref| + ((1 + u)^(2 M + 5) - 1) |a| S,
# and (1 + u)^(2 M + 5) - 1 <= (2 M + 6) u = (M + 3) eps for M <= 256 in either precision ((2 M + 5) u <= 3.1e-5).  An FMA removes roundings.
def fast_constant(M):
    return M + 3


def correct(out, F, a):
    t = out.dtype.type
    return out + t(a) * F


def fast_bound(ref, a, S, eps, M):
    """|got - ref| <= eps |ref| + (M + 3) eps |a| S for ref = out_0 + a F_exact (longdouble)."""
    return eps * np.abs(ref) + fast_constant(M) * eps * abs(np.longdouble(a)) * S


# ---- the stage matrix of the C ABI test ------------------------------------------------------------------------------------------------
SHAPES = [(5, 3), (16, 12), (66, 17), (130, 65), (257, 4)]
MODE_COUNT_CASES = [1, MODE_CHUNK - 1, MODE_CHUNK, MODE_CHUNK + 1, MAX_MODES]
NFIELDS = (1, 3, MAX_FIELDS)


# ---- the reference stepper -------------------------------------------------------------------------------------------------------------
class RefModel(RC.RefModel):
    """relaxation_cases.RefModel with the stochastic term appended LAST to the corrections of every field.  stir: dict(seed, stream, Lx,
    Ly, groups=[(kind, field indices, k_f, dk, rate)]) with the groups in field order -- PAIR on fields (0, 1), SCALAR on one field
    index of the 4 + K.  The step counter starts at `counter` and advances once per step; the coefficients are those of the counter at
    the start of the step in all three stages."""

    def __init__(self, *a, stir=None, counter=0, **kw):
        super().__init__(*a, **kw)
        self.stir, self.counter, self._F = stir, counter, None
        if stir is not None:
            Lx, Ly, dx, dy, Nx, Ny = stir["Lx"], stir["Ly"], self.dx, self.dy, self.Nx, self.Ny
            dtype = self.q[0].dtype
            face = {0: (True, False), 1: (False, True)}
            self._groups = []
            for kind, idx, k_f, dk, rate in stir["groups"]:
                modes = forcing_modes(Nx, Ny, Lx, Ly, k_f, dk)
                kx, ky = wavenumbers(modes, Lx, Ly)
                ktx, kty = modified(modes, Lx, Ly, dx, dy)
                tabs = []
                for k in idx:
                    fx, fy = face.get(k, (False, False))
                    tabs.append(tables(kx, nodes(Nx, dx, fx), dtype) + tables(ky, nodes(Ny, dy, fy), dtype))
                self._groups.append((kind, idx, amp0(modes, rate, kind == PAIR, Lx, Ly, dx, dy), ktx, kty, tabs))

    def _draw(self, dt):
        dtype = self.q[0].dtype
        sdt = 1.0 / np.sqrt(np.float64(dt))
        self._F = {}
        for g, (kind, idx, amp, ktx, kty, tabs) in enumerate(self._groups):
            pairs = coefficients(kind, amp, ktx, kty, self.stir["seed"], self.stir["stream"], self.counter, g, sdt, dtype)
            for k, (P, Q), (cx, sx, cy, sy) in zip(idx, pairs, tabs):
                self._F[k] = synth_strict(cx, sx, cy, sy, P, Q)

    def _D(self, U):
        out = super()._D(U)
        if self._F:
            for k, F in self._F.items():
                out[k].append(F)
        return out

    def step(self, dt):
        if self.stir is not None:
            self._draw(dt)
        super().step(dt)
        self.counter += 1
        return self


# ---- the injected band (CPU test: recorded here; GPU spectra test: compared with it) -----------------------------------------------------
BAND_N, BAND_STEPS, BAND_DT, BAND_RATE, BAND_KF, BAND_DK, BAND_SEED = 16, 6, 1e-3, 1e-6, 4.0, 1.0, 7
BAND_L = 2 * np.pi
# the fraction of the isotropic power of (u, v) outside the shells the ring covers, +-1 shell, that RefModel gives after BAND_STEPS steps
# from rest (tests/test_stochastic_cases_cpu.py computes and prints it; it must stay <= 1e-6)
BAND_REFERENCE_FRACTION = 8.915e-14


def band_shells():
    """The isotropic shells (integers, shell width 1 on the 2π square) the ring covers, +-1."""
    lo, hi = int(np.floor(BAND_KF - BAND_DK / 2 + 0.5)) - 1, int(np.floor(BAND_KF + BAND_DK / 2 + 0.5)) + 1
    return lo, hi


def out_of_band_fraction(shell_power):
    """shell_power (nfields, NS): 1 - (the power in band_shells()) / (all power), summed over the fields."""
    lo, hi = band_shells()
    p = np.asarray(shell_power, dtype=np.float64)
    return float(1.0 - p[:, lo:hi + 1].sum() / p.sum())


def isotropic_power(f):
    """Shell sums of |FFT|^2 / N^4 of an interior array (N, N) on the 2π square: shell = floor(|k| + 1/2)."""
    N = f.shape[0]
    P2 = np.abs(np.fft.fft2(f)) ** 2 / float(N) ** 4
    k = np.fft.fftfreq(N, 1.0 / N)
    shell = np.floor(np.hypot(k[None, :], k[:, None]) + 0.5).astype(int)
    return np.bincount(shell.ravel(), weights=P2.ravel())
