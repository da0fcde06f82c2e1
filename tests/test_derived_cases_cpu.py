"""CPU tests (no GPU) of the numpy restatement of the derived frames (tests/derived_cases.py), the yardstick the device frames are held to
bitwise: exact discrete identities on integer data, second-order convergence to the analytic fields of the reference's initial
conditions, and the two degenerate cases of the potential vorticity and the conservative form."""
import numpy as np
import pytest

import derived_cases as DC


def _pad(a, H):
    return np.pad(a, H, mode="wrap")


def _integers(Nx, Ny, seed):
    return np.random.default_rng(seed).integers(-40, 41, size=(Ny, Nx)).astype(np.float64)


@pytest.mark.parametrize("Nx,Ny,H", [(7, 9, 1), (16, 5, 3), (1, 1, 1), (2, 3, 2)])
def test_discrete_identities_are_exact(Nx, Ny, H):
    """Integer phi at centres and psi at corners, dx = dy = 0.5, periodic images in the halos: every difference and quotient below is
    exactly representable, so curl grad = 0, div of a rotated gradient = 0 and J = div grad hold to the bit."""
    d = 0.5
    phi, psi = _integers(Nx, Ny, 3), _integers(Nx, Ny, 4)
    one = np.ones((Ny + 2 * H, Nx + 2 * H))
    args = (Nx, Ny, H, H, d, d, 0.0, 1)
    # gradient flow: U(i,j) = (phi(i,j) - phi(i-1,j)) / dx, V(i,j) = (phi(i,j) - phi(i,j-1)) / dy
    U, V = (phi - np.roll(phi, 1, axis=1)) / d, (phi - np.roll(phi, 1, axis=0)) / d
    zeta, delta = DC.np_derived_fields(_pad(U, H), _pad(V, H), one, one, *args, names=("vorticity", "divergence"))
    assert np.array_equal(zeta, np.zeros((Ny, Nx)))
    J, = DC.np_derived_fields(one, one, one, _pad(phi, H), *args, names=("current",))
    assert np.array_equal(J, delta) and (Nx * Ny == 1 or np.abs(J).max() > 0)
    lap = (np.roll(phi, -1, 1) - 2 * phi + np.roll(phi, 1, 1)) / d ** 2 + (np.roll(phi, -1, 0) - 2 * phi + np.roll(phi, 1, 0)) / d ** 2
    assert np.array_equal(J, lap)          # (exact in integers: the five-point Laplacian, centred on the cell itself)
    # rotated gradient: U(i,j) = -(psi(i,j+1) - psi(i,j)) / dy, V(i,j) = (psi(i+1,j) - psi(i,j)) / dx
    U, V = -(np.roll(psi, -1, axis=0) - psi) / d, (np.roll(psi, -1, axis=1) - psi) / d
    zeta, delta = DC.np_derived_fields(_pad(U, H), _pad(V, H), one, one, *args, names=("vorticity", "divergence"))
    assert np.array_equal(delta, np.zeros((Ny, Nx)))
    lap = (np.roll(psi, -1, 1) - 2 * psi + np.roll(psi, 1, 1)) / d ** 2 + (np.roll(psi, -1, 0) - 2 * psi + np.roll(psi, 1, 0)) / d ** 2
    assert np.array_equal(zeta, lap)       # the vorticity of a stream function is its Laplacian, at the corner psi sits on


def test_placement_of_single_point_sources():
    """One non-zero value in one parent: which points of which field see it, and with which sign."""
    Nx, Ny, H, d = 6, 5, 2, 0.5
    zero, one = np.zeros((Ny + 2 * H, Nx + 2 * H)), np.ones((Ny + 2 * H, Nx + 2 * H))
    i, j = 2, 1                                            # 0-based interior cell
    spike = zero.copy()
    spike[H + j, H + i] = 1.0
    f = lambda q1, q2, A, n: DC.np_derived_fields(q1, q2, one, A, Nx, Ny, H, H, d, d, 0.0, 1, names=(n,))[0]
    want = np.zeros((Ny, Nx)); want[j, i], want[j, i + 1] = 2.0, -2.0          # zeta = (V(i) - V(i-1)) / dx
    assert np.array_equal(f(zero, spike, zero, "vorticity"), want)
    want = np.zeros((Ny, Nx)); want[j, i], want[j + 1, i] = -2.0, 2.0          #      - (U(j) - U(j-1)) / dy
    assert np.array_equal(f(spike, zero, zero, "vorticity"), want)
    want = np.zeros((Ny, Nx)); want[j, i], want[j, i - 1] = -2.0, 2.0          # delta = (U(i+1) - U(i)) / dx
    assert np.array_equal(f(spike, zero, zero, "divergence"), want)
    want = np.zeros((Ny, Nx)); want[j, i], want[j - 1, i] = -2.0, 2.0          #       + (V(j+1) - V(j)) / dy
    assert np.array_equal(f(zero, spike, zero, "divergence"), want)
    want = np.zeros((Ny, Nx)); want[j, i] = -16.0
    want[j, i - 1] = want[j, i + 1] = want[j - 1, i] = want[j + 1, i] = 4.0
    assert np.array_equal(f(zero, zero, spike, "current"), want)
    # the depth under a corner: the four cells around it, (i-1, j-1) included
    h = one.copy()
    h[H + j, H + i] = 5.0
    q, = DC.np_derived_fields(zero, zero, h, zero, Nx, Ny, H, H, d, d, 4.0, 1, names=("potential_vorticity",))
    want = np.full((Ny, Nx), 4.0); want[j, i] = want[j, i + 1] = want[j + 1, i] = want[j + 1, i + 1] = 2.0
    assert np.array_equal(q, want)
    part, = DC.np_derived_fields(zero, zero, h, zero, Nx, Ny, H, H, d, d, 4.0, 1, names=("potential_vorticity",), rows=(1, 3))
    assert np.array_equal(part, want[1:3])


def _analytic(N, H=1, L=10.0):
    """The reference's vortex u = 5 y e^{-r^2}, v = -5 x e^{-r^2} (SWMHD_example.jl:39-40) plus the gradient of e^{-r^2/2}, and
    A = -e^{-r^2/4} (MHD_visualize.jl:8,19-20), on [-5, 5]^2 with the halos filled analytically."""
    d = L / N
    k = np.arange(-H, N + H)
    xf, xc = -L / 2 + k * d, -L / 2 + (k + 0.5) * d
    Xf, Yc = np.meshgrid(xf, xc)          # (f, c): u
    Xc, Yf = np.meshgrid(xc, xf)          # (c, f): v
    Xcc, Ycc = np.meshgrid(xc, xc)
    Xff, Yff = np.meshgrid(xf, xf)
    e = lambda X, Y, s: np.exp(-(X ** 2 + Y ** 2) / s)
    u = 5 * Yc * e(Xf, Yc, 1) - Xf * e(Xf, Yc, 2)
    v = -5 * Xc * e(Xc, Yf, 1) - Yf * e(Xc, Yf, 2)
    A = -e(Xcc, Ycc, 4)
    I = slice(H, H + N)
    r2f, r2c = (Xff ** 2 + Yff ** 2)[I, I], (Xcc ** 2 + Ycc ** 2)[I, I]
    exact = dict(vorticity=10 * (r2f - 1) * np.exp(-r2f), divergence=(r2c - 2) * np.exp(-r2c / 2),
                 current=-(r2c - 4) / 4 * np.exp(-r2c / 4))
    return u, v, A, d, exact


def test_second_order_convergence():
    """max error over N = 50, 100, 200, 400 fitted as MHD_visualize.jl:101-104 fits it (a line through log10 N, log10 error): the order
    of zeta, delta and J lies in [1.9, 2.1]."""
    Ns, names = (50, 100, 200, 400), ("vorticity", "divergence", "current")
    err = {n: [] for n in names}
    for N in Ns:
        u, v, A, d, exact = _analytic(N)
        got = DC.np_derived_fields(u, v, np.ones_like(A), A, N, N, 1, 1, d, d, 0.0, 1, names=names)
        for n, g in zip(names, got):
            err[n].append(np.abs(g - exact[n]).max())
    for n in names:
        order = -np.polyfit(np.log10(Ns), np.log10(err[n]), 1)[0]
        print(n, "errors", err[n], "order", order)
        assert 1.9 <= order <= 2.1, (n, order)


def test_potential_vorticity_of_uniform_depth_and_the_conservative_form():
    N, H = 24, 2
    u, v, A, d, _ = _analytic(N, H)
    two = np.full_like(A, 2.0)
    for form in (1, 0):
        zeta, q = DC.np_derived_fields(u, v, two, A, N, N, H, H, d, d, 0.75, form, names=("vorticity", "potential_vorticity"))
        assert np.array_equal(q, (zeta + 0.75) / 2) and np.abs(zeta).max() > 1
    one = np.ones_like(A)
    vi = DC.np_derived_fields(u, v, one, A, N, N, H, H, d, d, 0.75, 1)
    assert np.array_equal(DC.np_derived_fields(u, v, one, A, N, N, H, H, d, d, 0.75, 0), vi)
    assert not np.array_equal(DC.np_derived_fields(u, v, two, A, N, N, H, H, d, d, 0.75, 0)[:2], vi[:2])
    assert DC.mask_names(5) == ("vorticity", "current") and DC.mask_names(DC.ALL) == DC.NAMES
