"""Reference of ONE call of the 2-D / isotropic spectrum entry points (swmhd_spectra2d_*, swmhd_ensemble_spectra2d_* in
include/swmhd_spectra2d.h) and the list of calls that tests/test_spectra2d_gpu.py runs through k_s2d_rows / k_s2d_cols / k_s2d_shells
(swmhd_amd/csrc/spectra2d.hip).  numpy only: no GPU, no torch.  Pinned on the CPU by tests/test_spectra2d_cases_cpu.py.

Reference.  The frame values in IEEE double from output_cases.np_output_fields (bitwise the float64 frame, so bitwise the input of the
kernel's transform); the rows through spectra_cases.row_modes in np.longdouble; the columns through the same longdouble transforms,
applied to the real and to the imaginary parts of the row modes; the shells by the statements of the header in float64:
    F^[kx,ky] = 1/(Nx Ny) sum_ij F(i,j) exp(-2 pi i (kx (i-1)/Nx + ky (j-1)/Ny)),   kx = 0 .. Nx/2, ky = 0 .. Ny-1
    P2[kx,ky] = c_kx |F^[kx,ky]|^2,  c_kx = 1 at kx = 0 and Nx/2, else 2
    my = ky (ky <= Ny/2) | ky - Ny;  r2 = wx * float(kx*kx) + wy * float(my*my);  shell = int(floor(sqrt(r2) + 0.5))
    E[s] = sum of P2 over the modes of shell s,  s = 0 .. NS-1,  NS = shell(Nx/2, Ny/2) + 1

Bound, per mode.  With S = the sum of |F^|^2 over all Nx Ny modes (= sum of P2) and eps2 = eta (log2 Nx + log2 Ny) 2^-53, eta = 9.66
(spectra_cases.ETA: the butterfly of the column pass is the row pass's statement, so the constant carries over):
    |got - P2[kx,ky]| <= c_kx (2 |F^[kx,ky]| eps2 sqrt(S) + eps2^2 S).
This is the normwise bound of spectra_cases composed over the two directions: the column transform is unitary up to its exact scale,
so it carries the norm of the row error and adds its own (include/swmhd_spectra2d.h has the derivation).
Bound, per shell: the sum of its modes' bounds plus gamma_(n_s - 1) E[s], n_s the mode count of the shell, gamma_n = n u / (1 - n u):
all terms are >= 0, so this holds for any order of summation.
RFFT_ETA = 5.66 (exact twiddles) is what numpy.fft.rfft2 is held to on the CPU.

Inputs: zonal_cases' parents of the whole grid: random fields with h in [1, 1.3], every parent element outside the one-cell ring of the
interior NaN; with a WRAP flag the halo of that direction is NaN too and the ring holds the periodic images."""
import functools
from collections import namedtuple

import numpy as np

import output_cases as OC
import spectra_cases as SC
import zonal_cases as ZC

LD = SC.LD
ETA, RFFT_ETA = SC.ETA, SC.RFFT_ETA
NAMES, BITS, ALL, SPARSE = SC.NAMES, SC.BITS, SC.ALL, SC.SPARSE
WRAP_X, WRAP_Y = SC.WRAP_X, SC.WRAP_Y
F64, F32 = SC.F64, SC.F32
DX, DY = SC.DX, SC.DY
U53 = SC.U53
MIN_LOG2, MAX_LOG2 = SC.MIN_LOG2, SC.MAX_LOG2
P2_G, P2_K, RMAX, UNITS_SMALL, SMALL = 16, 16, 16, 4, 256
names_of, same_bits, spacing = SC.names_of, SC.same_bits, SC.spacing
METRICS = ((1.0, 1.0), (1.0, 0.25), (0.36, 1.0))
SIZES = ((4, 4), (4, 8), (8, 4), (64, 4), (4, 64), (64, 64), (256, 512), (512, 256), (4096, 4), (4, 4096))


def shell_index(Nx, Ny, wx, wy):
    """int64 (Nx/2 + 1, Ny): the shell of every mode of the half-plane, by the header's statement in IEEE double"""
    mx = np.arange(Nx // 2 + 1, dtype=np.int64)[:, None]
    ky = np.arange(Ny, dtype=np.int64)[None, :]
    my = np.where(ky <= Ny // 2, ky, ky - Ny)
    a = np.float64(wx) * (mx * mx).astype(np.float64)
    b = np.float64(wy) * (my * my).astype(np.float64)
    r2 = a + b
    return np.floor(np.sqrt(r2) + 0.5).astype(np.int64)


def shells(Nx, Ny, wx, wy):
    """NS: swmhd_spectra2d_shells"""
    a = np.float64(wx) * np.float64((Nx // 2) ** 2)
    b = np.float64(wy) * np.float64((Ny // 2) ** 2)
    return int(np.floor(np.sqrt(a + b) + 0.5)) + 1


def ckx(Nx):
    c = np.full(Nx // 2 + 1, 2, dtype=np.int64)
    c[0] = c[Nx // 2] = 1
    return c


def counts(Nx, Ny, wx, wy):
    """int64 (NS,): modes of the full Nx x Ny plane per shell (a half-plane entry with 0 < kx < Nx/2 counts twice)"""
    sh = shell_index(Nx, Ny, wx, wy)
    w = np.broadcast_to(ckx(Nx)[:, None], sh.shape)
    return np.bincount(sh.ravel(), weights=w.ravel(), minlength=shells(Nx, Ny, wx, wy)).astype(np.int64)


def workspace(Nx, Ny, nfields, members, wx, wy):
    """doubles of workspace a call needs: swmhd_spectra2d_workspace"""
    if min(Nx, Ny, nfields, members) <= 0:
        return 0
    nkx = Nx // 2 + 1
    return (2 * nkx * Ny + nkx * shells(Nx, Ny, wx, wy)) * nfields * members


def plan_R(Nx, Ny, lds_limit=160 * 1024):
    """(R, pad, lds1) of pass 1: launch_plan.hpp spectra2d_plan"""
    budget = min(lds_limit, 80 * 1024)
    R = min(RMAX, Ny)
    while True:
        pad = 2 if R > 2 else 0
        lds = R * 8 * (Nx + pad) + 4 * Nx
        if lds <= budget or R == 1:
            return R, pad, lds
        R //= 2


def half_plane(frames):
    """frames (..., Ny, Nx) float64 -> (re, im) longdouble (..., Nx/2 + 1, Ny): F^[kx, ky]"""
    Nx = frames.shape[-1]
    re, im = SC.row_modes(frames)
    re, im = np.swapaxes(re[..., :Nx // 2 + 1], -1, -2), np.swapaxes(im[..., :Nx // 2 + 1], -1, -2)
    rr, ri = SC.row_modes(re)          # the column transform of the real parts (with its 1/Ny) ...
    ir, ii = SC.row_modes(im)          # ... and of the imaginary parts: T(re + i im) = T(re) + i T(im)
    return rr - ii, ri + ir


def shell_sums(p2, sh, NS):
    """p2 (..., nkx, Ny) -> (..., NS): sums over the shells, in the array's precision"""
    flat = p2.reshape(p2.shape[:-2] + (-1,))
    out = np.zeros(p2.shape[:-2] + (NS,), dtype=p2.dtype)
    order = np.argsort(sh.ravel(), kind="stable")
    s_sorted = sh.ravel()[order]
    starts = np.searchsorted(s_sorted, np.arange(NS + 1))
    srt = flat[..., order]
    for s in range(NS):
        if starts[s + 1] > starts[s]:
            out[..., s] = srt[..., starts[s]:starts[s + 1]].sum(axis=-1)
    return out


def spectra_of_frames(frames, wx, wy, eta=ETA):
    """frames (..., Ny, Nx) float64 -> (P2, P2 bound, E, E bound) as longdouble (..., Nx/2+1, Ny) and (..., NS).  A non-finite value
    in a frame makes all of its P2 and E non-finite."""
    frames = np.asarray(frames, dtype=np.float64)
    Ny, Nx = frames.shape[-2:]
    with np.errstate(invalid="ignore", over="ignore"):
        re, im = half_plane(frames)
        mag2 = re * re + im * im
        c = ckx(Nx).astype(LD)[:, None]
        p2 = c * mag2
        S = p2.sum(axis=(-1, -2), keepdims=True)
        eps = LD(eta) * LD(int(np.log2(Nx)) + int(np.log2(Ny))) * U53
        pb = c * (2 * np.sqrt(mag2) * eps * np.sqrt(S) + eps * eps * S)
        sh, NS = shell_index(Nx, Ny, wx, wy), shells(Nx, Ny, wx, wy)
        E, Eb = shell_sums(p2, sh, NS), shell_sums(pb, sh, NS)
        n = np.maximum(counts(Nx, Ny, wx, wy) - 1, 0).astype(LD)
        Eb = Eb + n * U53 / (1 - n * U53) * E
    return p2, pb, E, Eb


def compare(got, want, bound):
    """got (float64, the kernel's) against a reference and its bound: (failures, largest error / bound).  Where the reference is not
    finite the kernel's value must not be either."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    fin = np.isfinite(want)
    fails = [f"{tuple(i)}: got {got[tuple(i)]!r}, want non-finite" for i in np.argwhere(~fin & np.isfinite(got))[:8]]
    with np.errstate(invalid="ignore"):
        err = np.abs(got.astype(LD) - want)
    err = np.where(np.isfinite(got), err, LD(np.inf))
    bad = fin & ~(err <= bound)
    for i in np.argwhere(bad)[:8]:
        i = tuple(i)
        fails.append(f"{i}: got {got[i]!r}, want {float(want[i])!r}: error {float(err[i]):.3e} > bound {float(bound[i]):.3e}")
    pos = fin & (bound > 0)
    ratio = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    return fails, ratio


# pitch: stride_y = Nx + 2 Hx + 5; wrap: SWMHD_WRAP_X | SWMHD_WRAP_Y bits; outs: "shell", "2d" or "both"
Case = namedtuple("Case", "Nx Ny Hx Hy pitch form dtype which wrap wx wy outs")
OUTS = ("both", "shell", "2d")


def stride_y(c):
    return c.Nx + 2 * c.Hx + (ZC.PAD if c.pitch else 0)


def case_id(c):
    mask = "all" if c.which == ALL else "+".join(names_of(c.which))
    return (f"{c.Nx}x{c.Ny}-H{c.Hx}{c.Hy}{'-pitch' if c.pitch else ''}-{'vi' if c.form == 1 else 'cons'}-"
            f"{'f64' if np.dtype(c.dtype) == np.float64 else 'f32'}-{mask}{'-wrapx' if c.wrap & WRAP_X else ''}{'-wrapy' if c.wrap & WRAP_Y else ''}"
            f"-w{c.wx:g},{c.wy:g}-{c.outs}")


def cases():
    """The case list: plain data.  Every size sees both formulations and both precisions, rotating as spectra_cases.cases() does; the
    full mask at the small sizes; the metrics and the outputs asked for rotate through the sizes."""
    out = []
    pairs = (BITS["u"] | BITS["B_x"], BITS["s"] | BITS["A"], BITS["v"] | BITS["B_y"])
    for p, (Nx, Ny) in enumerate(SIZES):
        small = Nx * Ny <= 64 * 64
        (wx, wy), (wx2, wy2) = METRICS[p % 3], METRICS[(p + 1) % 3]
        out.append(Case(Nx, Ny, 3, 4, False, p % 2, F64, ALL if small else pairs[p % 3], 0, wx, wy, OUTS[p % 3]))
        out.append(Case(Nx, Ny, 3, 4, bool(p % 2), (p + 1) % 2, F32, ALL if Nx * Ny <= 256 else pairs[(p + 1) % 3], 0, wx2, wy2, OUTS[(p + 1) % 3]))
    # every metric and every choice of outputs at a small size and across both switch-overs
    for Nx, Ny in ((8, 4), (64, 64)):
        for k, (wx, wy) in enumerate(METRICS):
            for j, outs in enumerate(OUTS):
                out.append(Case(Nx, Ny, 1, 1, bool(j % 2), (k + j) % 2, F64, SPARSE, 0, wx, wy, outs))
    for k, (wx, wy) in enumerate(METRICS):
        out.append(Case(512, 256, 3, 4, True, k % 2, F64, BITS["s"], 0, wx, wy, "both"))
        out.append(Case(256, 512, 3, 4, True, (k + 1) % 2, F64, BITS["B_y"], 0, wx, wy, "both"))
    # each single-bit mask, both formulations, minimal halo
    for form in (1, 0):
        for n in NAMES:
            out.append(Case(8, 4, 1, 1, False, form, F64, BITS[n], 0, 1.0, 1.0, "both"))
    # WRAP flags on NaN halos: both, and each alone
    for Nx, Ny in ((4, 4), (8, 4), (64, 64), (4, 512)):
        for form, dtype in ((1, F64), (0, F64), (0, F32)):
            out.append(Case(Nx, Ny, 3, 4, False, form, dtype, ALL if Ny <= 64 else SPARSE, WRAP_X | WRAP_Y, 1.0, 0.25, "both"))
    for wrap in (WRAP_X, WRAP_Y):
        out.append(Case(64, 4, 3, 4, True, 0, F64, ALL, wrap, 0.36, 1.0, "both"))
        out.append(Case(4, 4, 3, 4, False, 1, F32, ALL, wrap, 1.0, 1.0, "shell"))
    return out


@functools.lru_cache(maxsize=8)
def inputs(c):
    """The four parents (q1, q2, h, A) of a case in its precision, shape (Ny + 2 Hy, stride_y).  Do not modify them."""
    return ZC._parents(c.Nx, c.Ny, c.Hx, c.Hy, stride_y(c), c.dtype, 0, c.Ny, c.wrap)


def frames_of(parents, Nx, Ny, Hx, Hy, dx, dy, form, which, wrap=0):
    """(popcount(which), Ny, Nx) float64: the frame values a call transforms"""
    return SC.frames_of(parents, Nx, Ny, Hx, Hy, dx, dy, form, (0, Ny), which, wrap)


def reference(parents, Nx, Ny, Hx, Hy, dx, dy, form, which, wx, wy, wrap=0, eta=ETA):
    """(P2, P2 bound, E, E bound) of one call"""
    return spectra_of_frames(frames_of(parents, Nx, Ny, Hx, Hy, dx, dy, form, which, wrap), wx, wy, eta)


@functools.lru_cache(maxsize=None)
def expected(c):
    dx, dy = spacing(c.dtype)
    return reference(inputs(c), c.Nx, c.Ny, c.Hx, c.Hy, dx, dy, c.form, c.which, c.wx, c.wy, c.wrap)


# ensembles: 3 members of one shape, halo (3, 4), each with data of its own; dense and pitched (a gap of NaN between members)
ENSEMBLE_MEMBERS, ENSEMBLE_GAP = ZC.ENSEMBLE_MEMBERS, ZC.ENSEMBLE_GAP
ENS_HX, ENS_HY = ZC.ENS_HX, ZC.ENS_HY


def ensemble_member_inputs(Nx, Ny, dtype, m, wrap):
    return ZC.ensemble_member_inputs(Nx, Ny, dtype, m, None, wrap)


def ensemble_cases():
    """(Nx, Ny, form, dtype, pitched, which, wrap, wx, wy, outs)"""
    return [(8, 4, 1, F64, False, ALL, 0, 1.0, 1.0, "both"), (8, 4, 0, F32, True, ALL, 0, 1.0, 0.25, "both"),
            (64, 64, 1, F64, True, SPARSE, WRAP_X | WRAP_Y, 1.0, 1.0, "both"), (4, 512, 0, F64, True, BITS["A"], 0, 0.36, 1.0, "shell"),
            (512, 4, 1, F32, False, BITS["u"] | BITS["s"], 0, 1.0, 0.25, "2d")]


def ensemble_case_id(e):
    Nx, Ny, form, dtype, pitched, which, wrap, wx, wy, outs = e
    return (f"{Nx}x{Ny}-{'vi' if form == 1 else 'cons'}-{'f64' if np.dtype(dtype) == np.float64 else 'f32'}{'-pitched' if pitched else ''}"
            f"-{'all' if which == ALL else '+'.join(names_of(which))}{'-wrap' if wrap else ''}-w{wx:g},{wy:g}-{outs}")
