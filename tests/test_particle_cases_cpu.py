"""CPU tests (no GPU) of the numpy restatement of the particle kernels (tests/particle_cases.py), which the GPU tests compare bitwise:
the interpolation is exact for fields that are linear, three stages add up to one time step, the fold lands in the domain, the
reflection is an involution, and the scheme is third order along a path."""
import numpy as np
import pytest

import particle_cases as PC

EPS = np.finfo(np.float64).eps


def linear_parents(Nx, Ny, H, x0, y0, dx, dy, fu, fv):
    """parents of U at (Face, Center) and V at (Center, Face), halos included, from functions of (x, y)"""
    i, j = np.arange(-H, Nx + H), np.arange(-H, Ny + H)
    Xf, Yc = np.meshgrid(x0 + i * dx, y0 + (j + 0.5) * dy)
    Xc, Yf = np.meshgrid(x0 + (i + 0.5) * dx, y0 + j * dy)
    return fu(Xf, Yc), fv(Xc, Yf)


def test_linear_field_is_interpolated_to_rounding():
    Nx, Ny, H, x0, y0, dx, dy = 12, 9, 2, -0.3, 0.7, 0.125, 0.2
    f = lambda X, Y: 0.4 + 1.5 * X - 0.75 * Y
    i, j = np.arange(-H, Nx + H), np.arange(-H, Ny + H)
    rng = np.random.default_rng(3)
    x = x0 + dx * (0.5 + (Nx - 1.5) * rng.random(400))    # interior points: every node around them is a cell of the grid, for a
    y = y0 + dy * (0.5 + (Ny - 1.5) * rng.random(400))    # field at the faces (nodes 0 .. N - 1) and at the centres alike
    fields, locs = [], []
    for loc in range(4):
        X, Y = np.meshgrid(x0 + (i + (0.5 if loc & PC.CENTER_X else 0.0)) * dx, y0 + (j + (0.5 if loc & PC.CENTER_Y else 0.0)) * dy)
        fields.append(f(X, Y))
        locs.append(loc)
    for flags in (0, PC.BOUNDED_X | PC.BOUNDED_Y, PC.WRAP_X, PC.WRAP_Y):      # (interior points: no wrapped node is touched)
        got = PC.sample(fields, locs, x, y, Nx, Ny, H, H, x0, y0, dx, dy, flags)
        want = f(x, y)
        # the node values carry one rounding each of a quantity below 4, the weights a few of sx < 16: a handful of eps of 4
        assert np.abs(got - want).max() <= 32 * EPS * 4.0, flags


def test_uniform_velocity_moves_every_particle_by_dt_U():
    assert sum(PC.RK3_GAMMA) + sum(PC.RK3_ZETA) == pytest.approx(1.0, abs=2 * EPS)
    Nx, Ny, H, x0, y0, dx, dy, dt = 8, 6, 1, 0.0, -1.0, 0.25, 0.5, 0.05
    U0, V0 = 0.75, -0.5
    q1 = np.full((Ny + 2 * H, Nx + 2 * H), U0)
    q2 = np.full_like(q1, V0)
    rng = np.random.default_rng(4)
    x = x0 + Nx * dx * rng.random(50)
    y = y0 + Ny * dy * rng.random(50)
    xs, ys = x.copy(), y.copy()
    gx, gy = np.full(50, np.nan), np.full(50, np.nan)       # stage 1 does not read G-
    for k in range(3):
        xs, ys, gx, gy = PC.stage(q1, q2, None, xs, ys, gx, gy, Nx, Ny, H, H, x0, y0, dx, dy, PC.VECTOR_INVARIANT, dt, PC.RK3_GAMMA[k],
                                  PC.RK3_ZETA[k], PC.WRAP_X | PC.WRAP_Y)
    assert np.all(np.isfinite(xs)) and np.all(np.isfinite(ys))
    want_x = PC.fold(x + dt * U0, x0, Nx * dx, PC.WRAP)
    want_y = PC.fold(y + dt * V0, y0, Ny * dy, PC.WRAP)
    # a few roundings of positions below 4 (a particle that wraps in one form and not in the other differs by a rounding of Lx)
    assert np.abs(xs - want_x).max() <= 16 * EPS * 4.0 and np.abs(ys - want_y).max() <= 16 * EPS * 4.0
    np.testing.assert_array_equal(gx, np.full(50, U0))
    np.testing.assert_array_equal(gy, np.full(50, V0))


@pytest.mark.parametrize("mode", [PC.WRAP, PC.PERIODIC, PC.BOUNDED])
@pytest.mark.parametrize("o, L", [(0.0, 1.0), (-3.7, 2.5), (1e3, 0.3)])
def test_fold_lands_in_the_domain(o, L, mode):
    x = np.concatenate([o + L * np.linspace(-3.0, 3.0, 1201), [1e300, -1e300, o, o + L, np.nextafter(o, -np.inf), np.nextafter(o + L, np.inf)]])
    got = PC.fold(x, o, L, mode)
    assert np.all((got >= o) & (got <= o + L))
    inside = (x >= o) & (x < o + L)
    np.testing.assert_array_equal(got[inside], x[inside])                 # a position inside is not touched
    assert np.isnan(PC.fold(np.array([np.nan]), o, L, mode)[0])           # the clamp leaves a NaN a NaN
    if mode != PC.BOUNDED:      # the periodic image: off by a whole number of periods
        k = (got[:1201] - x[:1201]) / L
        assert np.abs(k - np.round(k)).max() <= 64 * EPS * max(1.0, abs(o) / L)


def test_reflection_is_an_involution():
    o, L = -0.4, 1.6
    d = np.linspace(0.0, L, 400, endpoint=False)[1:]                      # crossings shallower than L
    for wall, x in ((o, o - d), (o + L, o + L + d)):
        once = PC.reflect(x, wall)
        np.testing.assert_array_equal(PC.fold(x, o, L, PC.BOUNDED), np.clip(once, o, o + L))
        assert np.all((once >= o) & (once <= o + L))
        assert np.abs(PC.reflect(once, wall) - x).max() <= 2 * EPS * (abs(o) + 2 * L)
        np.testing.assert_array_equal(PC.fold(once, o, L, PC.BOUNDED), once)      # inside: folding again changes nothing


def rotate(n, dt, Omega):
    """n RK3 steps of particles in the solid-body rotation U = -Omega (y - yc), V = Omega (x - xc), given analytically at the nodes of a
    frozen 32^2 unwrapped grid; returns (start, end) positions"""
    N, H, x0, y0 = 32, 1, 0.0, 0.0
    d = 1.0 / N
    xc = yc = 0.5
    q1, q2 = linear_parents(N, N, H, x0, y0, d, d, lambda X, Y: -Omega * (Y - yc), lambda X, Y: Omega * (X - xc))
    ang = np.linspace(0.0, 2 * np.pi, 7)[:-1]
    x, y = xc + 0.25 * np.cos(ang), yc + 0.25 * np.sin(ang)
    xs, ys, gx, gy = x.copy(), y.copy(), np.full(6, np.nan), np.full(6, np.nan)
    for _ in range(n):
        for k in range(3):
            xs, ys, gx, gy = PC.stage(q1, q2, None, xs, ys, gx, gy, N, N, H, H, x0, y0, d, d, PC.VECTOR_INVARIANT, dt, PC.RK3_GAMMA[k],
                                      PC.RK3_ZETA[k], PC.BOUNDED_X | PC.BOUNDED_Y)
    return (x, y), (xs, ys)


def test_third_order_along_the_path():
    Omega, T, radius = 1.0, 2.0, 0.25
    errs = []
    for n in (10, 20, 40):                     # Omega dt = 0.2, 0.1, 0.05
        (x, y), (xs, ys) = rotate(n, T / n, Omega)
        c, s = np.cos(Omega * T), np.sin(Omega * T)
        ex = 0.5 + c * (x - 0.5) - s * (y - 0.5)
        ey = 0.5 + s * (x - 0.5) + c * (y - 0.5)
        errs.append(np.hypot(xs - ex, ys - ey).max())
    print("errors", errs, "orders", np.log2(errs[0] / errs[1]), np.log2(errs[1] / errs[2]))
    assert errs[2] > 1e-10 * radius            # well above rounding, so the ratios measure the scheme
    assert np.log2(errs[0] / errs[1]) > 2.5 and np.log2(errs[1] / errs[2]) > 2.5
