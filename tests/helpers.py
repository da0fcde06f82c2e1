"""Shared input builders for the tests (numpy, host side)."""
import numpy as np


def coords(N, L, H, lo=None):
    """Cell-centre and face coordinates including H halo nodes, extended linearly (Oceananigans grid.xᶜᵃᵃ/xᶠᵃᵃ)."""
    lo = -L / 2 if lo is None else lo
    d = L / N
    k = np.arange(-H, N + H)
    return lo + (k + 0.5) * d, lo + k * d, d


def fill_halo_periodic(a, Nx, Ny, Hx, Hy):
    """numpy reference of the periodic halo fill (x first, then y over the padded width)."""
    a = a.copy()
    a[:, :Hx] = a[:, Nx:Nx + Hx]
    a[:, Nx + Hx:] = a[:, Hx:2 * Hx]
    a[:Hy, :] = a[Ny:Ny + Hy, :]
    a[Ny + Hy:, :] = a[Hy:2 * Hy, :]
    return a


def gaussian_case(N, H=3, L=10.0):
    """test_formulations.jl:12-18,156-159: A = exp(-(x^2+y^2)) evaluated from the (linearly extended) coordinate
    vectors, h = 1, on [-L/2, L/2]^2.  Returns A, h, d and the analytic Lorentz force at (fcc), (cfc)."""
    xc, xf, d = coords(N, L, H)
    X, Y = np.meshgrid(xc, xc)
    A = np.exp(-(X ** 2 + Y ** 2))
    h = np.ones_like(A)
    Xf, Yc = np.meshgrid(xf, xc)
    Xc, Yf = np.meshgrid(xc, xf)
    ex = -4 * Xf * np.exp(-2 * (Xf ** 2 + Yc ** 2))   # test_formulations.jl:14
    ey = -4 * Yf * np.exp(-2 * (Xc ** 2 + Yf ** 2))   # test_formulations.jl:15
    return A, h, d, ex, ey


def random_case(Nx, Ny, Hx, Hy, seed, dtype=np.float64, periodic=True):
    """Smooth-ish random A and a positive h, halos periodic-filled (what Oceananigans guarantees before a forcing call)."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((Ny + 2 * Hy, Nx + 2 * Hx))
    h = 1.0 + 0.3 * rng.random((Ny + 2 * Hy, Nx + 2 * Hx))
    if periodic:
        A, h = fill_halo_periodic(A, Nx, Ny, Hx, Hy), fill_halo_periodic(h, Nx, Ny, Hx, Hy)
    return np.ascontiguousarray(A.astype(dtype)), np.ascontiguousarray(h.astype(dtype))


def two_gaussians(X, Y, amp=0.5):
    """divergence_formulation/divergence_sw_mhd.jl:33"""
    return amp * np.exp(-((X - 0.5) ** 2 + Y ** 2)) - amp * np.exp(-((X + 0.5) ** 2 + Y ** 2))


def interior(a, Nx, Ny, Hx, Hy):
    return a[Hy:Hy + Ny, Hx:Hx + Nx]


def poison_halo(a, Nx, Ny, Hx, Hy, x=True, y=True):
    """NaN in the halo cells of the x and / or y direction of a parent, in place (corners belong to both): what a call that reads the
    periodic images instead of the halo cells (SWMHD_WRAP_X / SWMHD_WRAP_Y) must never touch."""
    if x:
        a[:, :Hx] = np.nan
        a[:, Hx + Nx:] = np.nan
    if y:
        a[:Hy, :] = np.nan
        a[Hy + Ny:, :] = np.nan
    return a


def same_bits(got, want, what):
    """The bitwise comparison of the frame tests: `want` rounded to the type of `got`, then NaN in the same places and the same integer
    bits everywhere else, so -0.0 is not 0.0."""
    with np.errstate(all="ignore"):
        want = want.astype(got.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    it = np.int64 if got.dtype == np.float64 else np.int32
    ok = np.array_equal(gn, wn) and np.array_equal(got[~gn].view(it), want[~wn].view(it))
    if not ok:
        bad = np.argwhere((gn != wn) | (~gn & ~wn & (np.ascontiguousarray(got).view(it) != np.ascontiguousarray(want).view(it))))
        print(what, "differs at", bad[:8].tolist(), "of", got.shape, "NaN got/want", int(gn.sum()), int(wn.sum()))
    assert ok, what


G, F = 9.81, 1.0   # gravity and Coriolis parameter of the tendency tests


def term_scales(form, q, dx, dy, force, g=G, f=F):
    """Magnitude of the largest term summed into each of the four tendencies (the S of the tolerances in include/swmhd.h); g, f: the
    gravity and |Coriolis parameter| of the call where they are not the G and F above."""
    q1, q2, h, A = (np.abs(a).max() for a in q)
    hmin = q[2].min()
    rd = 1.0 / dx + 1.0 / dy
    if form == "VectorInvariant":
        zeta = 2 * (q2 / dx + q1 / dy)
        mom = max((q1 + q2) * zeta, 0.5 * (q1 ** 2 + q2 ** 2) * rd, g * h * rd, f * (q1 + q2), force)
        return [mom, mom, (q1 / dx + q2 / dy) * h, (q1 / dx + q2 / dy) * A]
    u, v = q1 / hmin, q2 / hmin
    mom = max((q1 + q2) * (u + v) * rd, 0.5 * g * h * h * rd, f * (q1 + q2), force)
    return [mom, mom, q1 / dx + q2 / dy, (u / dx + v / dy) * A]
