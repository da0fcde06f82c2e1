"""CPU tests (no GPU) of the reference of the StochasticForcing (tests/stochastic_cases.py): the generator's known answers, the mode
sets, the properties the formulas promise -- a non-divergent pair, the injection rate, the injected band -- and the derived fast bound
against the longdouble value.  The Python side of the package (modes, amplitudes, tables) is compared with the restatement."""
from fractions import Fraction

import numpy as np
import pytest

import stochastic_cases as SC

TWO_PI = 2 * np.pi


def test_philox_known_answers():
    for counter, key, want in SC.KNOWN_ANSWERS:
        assert SC.philox4x32_10(counter, key) == want


def test_uniforms_are_exact():
    """u has 53 bits, and 2 u - 1 is exact in float64."""
    for hi, lo in ((0, 0), (SC.M32, SC.M32), (0x6627e8d5, 0xe169c58d), (1 << 5, 0), (0, 1 << 6), (0x80000000, 0)):
        u = SC.u53(hi, lo)
        exact = Fraction(((hi >> 5) << 26) + (lo >> 6), 1 << 53)
        assert Fraction(float(u)) == exact and 0 <= exact < 1
        assert Fraction(float(np.float64(2.0) * u - np.float64(1.0))) == 2 * exact - 1
    for m in range(50):
        x, y = SC.draw(7, 3, (1 << 32) - 1 + m, 1, m)
        assert -1 <= x < 1 and -1 <= y < 1


def test_mode_sets(swmhd):
    from swmhd_amd.stochastic import amplitudes, forcing_modes, modified_wavenumbers, x_table, y_table
    for (Nx, Ny), k_f, count in SC.MODE_COUNTS:
        modes = SC.forcing_modes(Nx, Ny, TWO_PI, TWO_PI, k_f, 1.0)
        assert len(modes) == count, (Nx, Ny, k_f, len(modes))
        nx, ny = modes[:, 0], modes[:, 1]
        assert np.all((nx >= 0) & (nx < Nx // 2) & (np.abs(ny) < Ny // 2) & ((nx > 0) | (ny > 0)))
        assert [tuple(m) for m in modes] == sorted(tuple(m) for m in modes)      # by nx, then ny
        g = swmhd.RectilinearGrid(size=(Nx, Ny), x=(0, TWO_PI), y=(0, TWO_PI))
        assert np.array_equal(forcing_modes(g, k_f, 1.0), modes)
    # the package's host tables are the restatement's
    g = swmhd.RectilinearGrid(size=(16, 12), x=(0, TWO_PI), y=(0, TWO_PI))
    modes = SC.forcing_modes(16, 12, TWO_PI, TWO_PI, 3.0, 1.0)
    kx, ky = SC.wavenumbers(modes, TWO_PI, TWO_PI)
    for pair in (False, True):
        assert np.array_equal(amplitudes(g, modes, 0.3, pair), SC.amp0(modes, 0.3, pair, TWO_PI, TWO_PI, g.dx, g.dy))
    assert all(np.array_equal(a, b) for a, b in zip(modified_wavenumbers(g, modes), SC.modified(modes, TWO_PI, TWO_PI, g.dx, g.dy)))
    for loc, fx, fy in (((swmhd.Face, swmhd.Center), True, False), ((swmhd.Center, swmhd.Face), False, True)):
        cx, sx = SC.tables(kx, SC.nodes(16, g.dx, fx), np.float64)
        cy, sy = SC.tables(ky, SC.nodes(12, g.dy, fy), np.float64)
        assert np.array_equal(x_table(g, modes, loc)[0::2], cx) and np.array_equal(x_table(g, modes, loc)[1::2], sx)
        assert np.array_equal(y_table(g, modes, loc)[0::2], cy) and np.array_equal(y_table(g, modes, loc)[1::2], sy)


def _pair_fields(Nx, Ny, k_f, rate, dt, n, dtype=np.float64, seed=5, stream=2):
    dx, dy = TWO_PI / Nx, TWO_PI / Ny
    modes = SC.forcing_modes(Nx, Ny, TWO_PI, TWO_PI, k_f, 1.0)
    kx, ky = SC.wavenumbers(modes, TWO_PI, TWO_PI)
    ktx, kty = SC.modified(modes, TWO_PI, TWO_PI, dx, dy)
    amp = SC.amp0(modes, rate, True, TWO_PI, TWO_PI, dx, dy)
    (Pu, Qu), (Pv, Qv) = SC.coefficients(SC.PAIR, amp, ktx, kty, seed, stream, n, 0, 1.0 / np.sqrt(dt), dtype)
    Fu = SC.synth_strict(*SC.tables(kx, SC.nodes(Nx, dx, True), dtype), *SC.tables(ky, SC.nodes(Ny, dy, False), dtype), Pu, Qu)
    Fv = SC.synth_strict(*SC.tables(kx, SC.nodes(Nx, dx, False), dtype), *SC.tables(ky, SC.nodes(Ny, dy, True), dtype), Pv, Qv)
    return Fu, Fv, len(modes)


def test_the_pair_is_non_divergent():
    """max |discrete divergence| <= 64 eps max |F| / min(dx, dy) on 16 x 12 (a probe of the formula gave a value two orders below)."""
    Nx, Ny = 16, 12
    dx, dy = TWO_PI / Nx, TWO_PI / Ny
    for n in range(5):
        Fu, Fv, M = _pair_fields(Nx, Ny, 3.0, 1.0, 1e-2, n)
        assert M == 8
        div = (np.roll(Fu, -1, axis=1) - Fu) / dx + (np.roll(Fv, -1, axis=0) - Fv) / dy
        scale = max(np.abs(Fu).max(), np.abs(Fv).max())
        print(f"max |div| {np.abs(div).max():.3e}, max |F| {scale:.3e}")
        assert np.abs(div).max() <= 64 * np.finfo(np.float64).eps * scale / min(dx, dy)


def test_the_injection_rate():
    """The mean of ½ dt <|F|²> over 400 steps of 8 modes lies within 5 standard errors of rate: the relative standard error of x² for a
    uniform x is 0.894 / sqrt(2 M N)."""
    Nx, Ny, rate, dt, N = 16, 12, 0.7, 1e-2, 400
    vals = []
    for n in range(N):
        Fu, Fv, M = _pair_fields(Nx, Ny, 3.0, rate, dt, n)
        vals.append(0.5 * dt * (np.mean(Fu ** 2) + np.mean(Fv ** 2)))
    se = 0.894 / np.sqrt(2 * M * N)
    dev = (np.mean(vals) / rate - 1) / se
    print(f"mean injection / rate = {np.mean(vals) / rate:.4f}: {dev:+.2f} standard errors")
    assert abs(dev) <= 5


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("M", SC.MODE_COUNT_CASES)
def test_strict_synthesis_is_within_the_fast_bound(dtype, M):
    rng = np.random.default_rng(M)
    Nx, Ny = 9, 7
    cx, sx = (rng.uniform(-1, 1, (M, Nx)).astype(dtype) for _ in range(2))
    cy, sy = (rng.uniform(-1, 1, (M, Ny)).astype(dtype) for _ in range(2))
    P, Q = (rng.uniform(-2, 2, M).astype(dtype) for _ in range(2))
    new0 = rng.uniform(-1, 1, (Ny, Nx)).astype(dtype)
    a = 0.013 * 0.37
    got = SC.correct(new0, SC.synth_strict(cx, sx, cy, sy, P, Q), a)
    F, S = SC.synth_exact(cx, sx, cy, sy, P, Q)
    ref = new0.astype(np.longdouble) + np.longdouble(dtype(a)) * F
    err = np.abs(got.astype(np.longdouble) - ref)
    bound = SC.fast_bound(ref, dtype(a), S, np.finfo(dtype).eps, M)
    print(f"M {M} {np.dtype(dtype).name}: max err / bound = {float((err / bound).max()):.3e}")
    assert np.all(err <= bound)
    assert np.abs(F).max() <= S


def band_reference(oracle, dtype=np.float64):
    """RefModel from rest on the 16 x 16 grid of the band test, BAND_STEPS steps: the reference the GPU spectra test shares."""
    N = SC.BAND_N
    d = SC.BAND_L / N
    shp = (N + 2 * SC.H, N + 2 * SC.H)
    q = [np.zeros(shp, dtype), np.zeros(shp, dtype), np.ones(shp, dtype), np.zeros(shp, dtype)]
    stir = dict(seed=SC.BAND_SEED, stream=0, Lx=SC.BAND_L, Ly=SC.BAND_L, groups=[(SC.PAIR, (0, 1), SC.BAND_KF, SC.BAND_DK, SC.BAND_RATE)])
    r = SC.RefModel(oracle, q, [], [None] * 4, N, N, 1, 1, "classic", dx=d, dy=d, fcor=0.0, stir=stir)
    for _ in range(SC.BAND_STEPS):
        r.step(SC.BAND_DT)
    return r


def test_the_injected_band(oracle):
    """From rest (u = v = 0, h = 1, A = 0, f = 0) on 16 x 16: after BAND_STEPS steps the isotropic power of u, v outside the shells the
    ring covers, +-1 shell, is at most 1e-6 of the whole, for the reference alone; the fraction it gives is recorded in
    stochastic_cases.BAND_REFERENCE_FRACTION."""
    r = band_reference(oracle)
    I = (slice(SC.H, SC.H + SC.BAND_N),) * 2
    power = np.stack([SC.isotropic_power(r.q[k][I]) for k in (0, 1)])
    frac = SC.out_of_band_fraction(power)
    print(f"out-of-band fraction of the reference: {frac:.3e}; total power {power.sum():.3e}")
    assert power.sum() > 0 and r.counter == SC.BAND_STEPS
    assert abs(frac) <= 1e-6
    assert SC.BAND_REFERENCE_FRACTION is not None and abs(frac - SC.BAND_REFERENCE_FRACTION) <= 1e-12
    # h is not stirred: the pair is non-divergent
    assert np.abs(r.q[2][I] - 1).max() <= 1e-9
