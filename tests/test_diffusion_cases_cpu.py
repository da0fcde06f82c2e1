"""CPU tests of the closure's reference (tests/diffusion_cases.py): the correction the engine applies after its stage kernels is the
same RK3 step as Oceananigans' "D is part of the tendency", and a diffusing eigenmode decays by R(z) per step."""
import numpy as np
import pytest

import diffusion_cases as DC
import tracer_cases as T


def _start(oracle, Nx, Ny, form, K):
    q = T.fill_state(oracle, T.state(Nx, Ny, form, 7, rough=False), Nx, Ny, (T.P, T.P))
    tr = [T.fill(oracle, c, Nx, Ny, (T.P, T.P)) for c in T.tracer_fields(Nx, Ny, K, 7, rough=False)]
    return q, tr


@pytest.mark.parametrize("mode", ["classic", "anchor"])
@pytest.mark.parametrize("form,lor", T.FORMS)
def test_correction_is_the_tendency_form(oracle, form, lor, mode):
    """One full RK3 step.  Per stage and cell the two forms round a few different partial results, each bounded by
    M = |U| + dt (|G| + |D|) <= 2 max |U| for these smooth fields and this dt: at most three roundings per stage in the classic form (a D
    apart, the sum in another order, G + D stored), and the anchor form's W = U + (dt/4) G stands for the weighted sum of G and G-
    (gamma1 + zeta2 = 1/4 up to 1 ulp, zeta3 = -gamma2 exactly): 16 eps max |U| covers three stages of either."""
    Nx, Ny, dt = 20, 12, 2e-3
    q, tr = _start(oracle, Nx, Ny, form, 2)
    nu = 3e-3 if form == 1 else 0.0
    coef = [nu, nu, 0.0, 5e-3, 0.0, 2e-3]
    ref = DC.RefModel(oracle, q, tr, coef, Nx, Ny, form, lor, "tendency").step(dt)
    got = DC.RefModel(oracle, q, tr, coef, Nx, Ny, form, lor, mode).step(dt)
    I = ref.I
    eps = np.finfo(np.float64).eps
    for k, (a, b) in enumerate(zip(ref.q + ref.tr, got.q + got.tr)):
        err, mag = np.abs(a[I] - b[I]).max(), np.abs(a[I]).max()
        print(f"form {form} {mode} field {k}: max |difference| = {err:.3e} = {err / (eps * mag):.2f} eps max|U|")
        assert err <= 16 * eps * mag
    # and the closure does something: the undiffused step differs by far more
    plain = DC.RefModel(oracle, q, tr, [0.0] * 6, Nx, Ny, form, lor, "classic").step(dt)
    assert np.abs(plain.q[3][I] - ref.q[3][I]).max() > 1e4 * eps


def test_without_coefficients_it_is_the_tracer_reference(oracle):
    Nx, Ny, dt = 7, 9, 2e-3
    q, tr = _start(oracle, Nx, Ny, 1, 1)
    a = DC.RefModel(oracle, q, tr, [0.0] * 5, Nx, Ny, 1, 1, "classic").step(dt).step(dt)
    b = T.RefModel(oracle, q, tr, Nx, Ny, 1, 1).step(dt).step(dt)
    for x, y in zip(a.q + a.tr, b.q + b.tr):
        assert np.array_equal(x, y)


def test_decay_of_an_eigenmode(oracle):
    q, z, R = DC.decay_case()
    Nx, Ny = DC.DECAY_NX, DC.DECAY_NY
    q = [oracle.fill_halo_periodic(a, Nx, Ny, DC.H, DC.H) for a in q]
    m = DC.RefModel(oracle, q, [], [0.0, 0.0, 0.0, DC.DECAY_C], Nx, Ny, 1, 0, "classic")
    I = m.I
    # the advective tendency of A on a fluid at rest is exactly zero
    G = oracle.tendencies(*q, Nx, Ny, DC.H, DC.H, DC.DX, DC.DY, 1, 0, T.GRAV, T.FCOR)
    assert not np.any(G[3][I]) and not np.any(G[0][I]) and not np.any(G[1][I]) and not np.any(G[2][I])
    # the mode is an eigenvector of the discrete operator: D = -c lambda A to rounding
    D = DC.laplacian_strict(DC.pad1(q[3], Nx, Ny, DC.H, DC.H, False, False), DC.DECAY_C, DC.DX, DC.DY)
    assert np.abs(D - (z / DC.DECAY_DT) * q[3][I]).max() <= 64 * np.finfo(np.float64).eps * np.abs(D).max()
    for _ in range(DC.DECAY_STEPS):
        m.step(DC.DECAY_DT)
    want = R ** DC.DECAY_STEPS * q[3][I]
    dev = np.abs(m.q[3][I] - want).max() / (R ** DC.DECAY_STEPS * np.abs(q[3][I]).max())
    print(f"z = {z:.6f}, R(z)^{DC.DECAY_STEPS} = {R ** DC.DECAY_STEPS:.6f}, relative deviation of the reference = {dev:.3e}")
    assert 0.3 < R ** DC.DECAY_STEPS < 0.7                         # the case decays visibly
    assert 0 < dev <= DC.DECAY_MARGIN
    assert DC.DECAY_MARGIN == 10 * DC.DECAY_REFERENCE_DEVIATION
    assert not np.any(m.q[0][I]) and not np.any(m.q[1][I]) and np.all(m.q[2][I] == 1.0)


def test_operator_restatements_agree():
    """laplacian_strict against laplacian_exact: within the fast bound's own scale, in both precisions (the strict form rounds more
    often than the fast one -- seven divisions and products a side -- so its constant here is larger: 16)."""
    rng = np.random.default_rng(3)
    for dtype in (np.float64, np.float32):
        P = rng.standard_normal((11, 14)).astype(dtype)
        D = DC.laplacian_strict(P, 0.02, DC.DX, DC.DY)
        E, S = DC.laplacian_exact(P, 0.02, DC.DX, DC.DY)
        assert D.dtype == dtype
        assert np.all(np.abs(D - E) <= 16 * np.finfo(dtype).eps * S)
    # pad1: the wrapped images of the interior, or the halo cells
    a = np.arange(7 * 9, dtype=np.float64).reshape(7, 9)       # Ny = 3, Nx = 5, Hy = 2, Hx = 2
    w = DC.pad1(a, 5, 3, 2, 2, True, True)
    assert w[0, 1] == a[4, 2] and w[-1, 1] == a[2, 2] and w[1, 0] == a[2, 6] and w[1, -1] == a[2, 2]
    h = DC.pad1(a, 5, 3, 2, 2, False, False)
    assert np.array_equal(h, a[1:6, 1:8])
