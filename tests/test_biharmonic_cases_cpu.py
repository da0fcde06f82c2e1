"""CPU tests of the biharmonic closure's reference (tests/biharmonic_cases.py) and of the Python class: the restatements agree, an
eigenmode is damped by -c lambda², the correction form is the tendency form, a diffusing eigenmode decays by R(z) per step, and
ScalarBiharmonicDiffusivity and the closure tuple refuse what they must before anything is allocated."""
import ctypes

import numpy as np
import pytest

import biharmonic_cases as BC
import diffusion_cases as DC
import tracer_cases as T


def _start(oracle, Nx, Ny, form, K):
    q = T.fill_state(oracle, T.state(Nx, Ny, form, 7, rough=False), Nx, Ny, (T.P, T.P))
    tr = [T.fill(oracle, c, Nx, Ny, (T.P, T.P)) for c in T.tracer_fields(Nx, Ny, K, 7, rough=False)]
    return q, tr


def test_operator_restatements_agree():
    """biharmonic_strict against biharmonic_exact within a few eps S in both precisions.  The strict form rounds more often than the
    fast one: L has 9 operations on the path to its value and D has 9 more (two differences, two quotients, the product and the sum a
    side, the negation exact), each at most eps/2 of a partial result that S bounds: 9 eps S to first order, 16 eps S asserted."""
    rng = np.random.default_rng(3)
    for dtype in (np.float64, np.float32):
        P = rng.standard_normal((13, 16)).astype(dtype)
        D = BC.biharmonic_strict(P, 0.02, BC.DX, BC.DY)
        E, S = BC.biharmonic_exact(P, 0.02, BC.DX, BC.DY)
        assert D.dtype == dtype and D.shape == E.shape == S.shape == (9, 12)
        worst = float((np.abs(D - E) / (np.finfo(dtype).eps * S)).max())
        print(f"{np.dtype(dtype).name}: max |strict - exact| = {worst:.2f} eps S")
        assert np.all(np.abs(D - E) <= 16 * np.finfo(dtype).eps * S)
    # only the diamond is read: NaN in the cells of the 2 x 2 corner blocks it skips changes nothing
    Q = P.copy()
    for r in (0, 1, -1, -2):
        for c in (0, 1, -1, -2):
            if (r in (0, -1)) or (c in (0, -1)):
                Q[r, c] = np.nan
    assert np.array_equal(BC.biharmonic_strict(Q, 0.02, BC.DX, BC.DY), BC.biharmonic_strict(P, 0.02, BC.DX, BC.DY))


def test_pad2_and_reach_wrap_by_a_true_modulus():
    a = np.arange(9 * 11, dtype=np.float64).reshape(9, 11)       # Ny = 3, Nx = 5, Hy = 3, Hx = 3
    w = BC.pad2(a, 5, 3, 3, 3, True, True)
    assert w.shape == (7, 9)
    assert w[0, 2] == a[4, 3] and w[1, 2] == a[5, 3] and w[-1, 2] == a[4, 3] and w[2, 0] == a[3, 6] and w[2, -1] == a[3, 4]
    assert np.array_equal(BC.pad2(a, 5, 3, 3, 3, False, False), a[1:8, 1:10])
    # widths 1 and 2: every image is the interior itself
    one = np.arange(7 * 7, dtype=np.float64).reshape(7, 7)       # Nx = Ny = 1, H = 3
    assert np.all(BC.pad2(one, 1, 1, 3, 3, True, True) == one[3, 3])
    two = BC.pad2(one, 2, 1, 3, 3, True, False)                  # Nx = 2 wrapped, y halos read
    assert np.array_equal(two[:, 0], two[:, 2]) and np.array_equal(two[:, 1], two[:, 3]) and np.array_equal(two[:, 0], two[:, 4])
    assert np.array_equal(two[:, 2], one[1:6, 3])
    # reach: the union of the diamonds; 13 cells for one cell with read halos, the interior alone for a wrapped 1 x 1
    r = BC.reach(1, 1, 3, 3, (7, 7), False, False, (0, 1))
    assert r.sum() == 13 and r[3, 1] and r[2, 2] and not r[1, 2] and not r[2, 1] and not r[3, 0]
    assert BC.reach(1, 1, 3, 3, (7, 7), True, True, (0, 1)).sum() == 1
    assert BC.reach(5, 3, 3, 3, (9, 11), False, False, (1, 1)).sum() == 0
    r = BC.reach(5, 3, 3, 3, (9, 11), False, False, (0, 3))
    assert r[1, 3:8].all() and not r[0].any() and not r[1, 2] and r[2, 2] and not r[2, 1] and r[3, 1] and not r[3, 0]


def test_an_eigenmode_is_damped_by_lambda_squared():
    """D of sin(kx) sin(ly) is -c lambda² phi to rounding, stated against S, the scale of the operator's rounding: the 16 eps S of the
    strict form (test_operator_restatements_agree) and the rounding of the mode's own samples, eps/2 |phi| each, of which the operator
    makes at most eps/2 S: 32 eps S asserted."""
    q, z, R = BC.decay_case()
    Nx, Ny = BC.DECAY_NX, BC.DECAY_NY
    A = q[3]
    x = (np.arange(-BC.H, Nx + BC.H) + 0.5) * BC.DX
    y = (np.arange(-BC.H, Ny + BC.H) + 0.5) * BC.DY
    assert A.shape == (y.size, x.size)
    P = BC.pad2(A, Nx, Ny, BC.H, BC.H, False, False)             # the analytic mode fills its own halos
    D = BC.biharmonic_strict(P, BC.DECAY_C, BC.DX, BC.DY)
    E, S = BC.biharmonic_exact(P, BC.DECAY_C, BC.DX, BC.DY)
    I = (slice(BC.H, BC.H + Ny), slice(BC.H, BC.H + Nx))
    eps = np.finfo(np.float64).eps
    want = (z / BC.DECAY_DT) * A[I]
    print(f"max |D - (-c lambda² A)| = {float((np.abs(D - want) / (eps * S)).max()):.2f} eps S")
    assert np.all(np.abs(D - want) <= 32 * eps * S)              # 16 eps S of the strict form, as much again for the samples of the mode
    assert np.abs(D).max() > 1e3 * eps * S.max()                 # and D is not lost in that: the check has teeth


@pytest.mark.parametrize("mode", ["classic", "anchor"])
@pytest.mark.parametrize("form,lor", T.FORMS)
def test_correction_is_the_tendency_form(oracle, form, lor, mode):
    """Three RK3 steps on 24 x 20 with both closures.  Per stage and cell the forms round a few different partial results, each
    bounded by M = |U| + dt (|G| + |D|) <= 2 max |U| for these smooth fields and this dt: 16 eps max |U| covers the three stages of one
    step with one closure (tests/test_diffusion_cases_cpu.py); a second correction per stage adds at most two roundings a stage (a D
    apart, one more sum): 22 eps per step, and three steps of a map that does not amplify: 66 eps max |U|."""
    Nx, Ny, dt = 24, 20, 2e-3
    q, tr = _start(oracle, Nx, Ny, form, 1)
    nu4 = 2e-6 if form == 1 else 0.0
    coef = [0.0, 0.0, 0.0, 5e-3, 0.0]
    coef4 = [nu4, nu4, 0.0, 3e-6, 1e-6]
    assert dt * max(coef4) * BC.LAMBDA_MAX ** 2 < 2.51
    ref = BC.RefModel(oracle, q, tr, coef, coef4, Nx, Ny, form, lor, "tendency")
    got = BC.RefModel(oracle, q, tr, coef, coef4, Nx, Ny, form, lor, mode)
    plain = BC.RefModel(oracle, q, tr, coef, [0.0] * 5, Nx, Ny, form, lor, "classic")
    for _ in range(3):
        ref.step(dt); got.step(dt); plain.step(dt)
    I = ref.I
    eps = np.finfo(np.float64).eps
    for k, (a, b) in enumerate(zip(ref.q + ref.tr, got.q + got.tr)):
        err, mag = np.abs(a[I] - b[I]).max(), np.abs(a[I]).max()
        print(f"form {form} {mode} field {k}: max |difference| = {err:.3e} = {err / (eps * mag):.2f} eps max|U|")
        assert err <= 66 * eps * mag
    # and the closure does something: the step without it differs by far more
    assert np.abs(plain.q[3][I] - ref.q[3][I]).max() > 1e4 * eps
    assert np.abs(plain.tr[0][I] - ref.tr[0][I]).max() > 1e4 * eps


def test_without_biharmonic_coefficients_it_is_the_diffusion_reference(oracle):
    Nx, Ny, dt = 7, 9, 2e-3
    q, tr = _start(oracle, Nx, Ny, 1, 1)
    coef = [3e-3, 3e-3, 0.0, 5e-3, 2e-3]
    for mode in ("classic", "anchor", "tendency"):
        a = BC.RefModel(oracle, q, tr, coef, [0.0] * 5, Nx, Ny, 1, 1, mode).step(dt).step(dt)
        b = DC.RefModel(oracle, q, tr, coef, Nx, Ny, 1, 1, mode).step(dt).step(dt)
        for x, y in zip(a.q + a.tr, b.q + b.tr):
            assert np.array_equal(x, y)


def test_decay_of_an_eigenmode(oracle):
    q, z, R = BC.decay_case()
    Nx, Ny = BC.DECAY_NX, BC.DECAY_NY
    q = [oracle.fill_halo_periodic(a, Nx, Ny, BC.H, BC.H) for a in q]
    assert BC.DECAY_DT * BC.DECAY_C * BC.LAMBDA_MAX ** 2 < 2.51        # the grid-scale mode stays inside RK3's interval
    assert 0.02 < -z < 0.032
    m = BC.RefModel(oracle, q, [], [0.0] * 4, [0.0, 0.0, 0.0, BC.DECAY_C], Nx, Ny, 1, 0, "classic")
    I = m.I
    for _ in range(BC.DECAY_STEPS):
        m.step(BC.DECAY_DT)
    Rn = R ** BC.DECAY_STEPS
    dev = np.abs(m.q[3][I] - Rn * q[3][I]).max() / (Rn * np.abs(q[3][I]).max())
    print(f"z = {z:.6f}, R(z)^{BC.DECAY_STEPS} = {Rn:.6f}, relative deviation of the reference = {dev:.3e}")
    assert 0.3 < Rn < 0.7                                              # the case decays visibly
    assert 0 < dev <= BC.DECAY_MARGIN
    assert BC.DECAY_MARGIN == 10 * BC.DECAY_REFERENCE_DEVIATION
    assert not np.any(m.q[0][I]) and not np.any(m.q[1][I]) and np.all(m.q[2][I] == 1.0)


# ---- the class ------------------------------------------------------------------------------------------------------------------------
def test_scalar_biharmonic_diffusivity_values(swmhd):
    S = swmhd
    E = S._lib.SwmhdError
    names = ("u", "v", "h", "A")
    B = S.ScalarBiharmonicDiffusivity
    assert "ScalarBiharmonicDiffusivity" in S.__all__
    c = B(nu=1e-6, kappa=2e-6)
    assert c.coefficients(names, ("c", "d")) == {"u": 1e-6, "v": 1e-6, "h": 0.0, "A": 2e-6, "c": 2e-6, "d": 2e-6}
    c = B(kappa={"A": 3e-6, "d": 1e-6})
    assert c.coefficients(names, ("c", "d")) == {"u": 0.0, "v": 0.0, "h": 0.0, "A": 3e-6, "c": 0.0, "d": 1e-6}
    assert B().coefficients(names) == {"u": 0.0, "v": 0.0, "h": 0.0, "A": 0.0}
    assert repr(B(nu=1e-6)) == "ScalarBiharmonicDiffusivity(nu=1e-06, kappa=0.0)"
    for bad in ({"B": 1e-6}, {"u": 1e-6}, {"h": 1e-6}, {"c": 1e-6}):
        with pytest.raises(E, match="ScalarBiharmonicDiffusivity: kappa names"):
            B(kappa=bad).coefficients(names, ("d",))
    for kw in (dict(nu=-1.0), dict(nu=float("nan")), dict(kappa=float("inf")), dict(kappa={"A": -1e-6}), dict(kappa={3: 1e-6}),
               dict(nu=[[1.0]])):
        with pytest.raises(E, match="ScalarBiharmonicDiffusivity"):
            B(**kw)
    g = S.RectilinearGrid(size=(16, 8), x=(0, 1.6), y=(0, 0.4))
    c = B(nu=1e-6, kappa={"A": 4e-6})
    assert c.max_stable_dt(g) == pytest.approx(2.51 / (4e-6 * (4 / 0.1 ** 2 + 4 / 0.05 ** 2) ** 2), rel=1e-12)
    assert B().max_stable_dt(g) == float("inf")
    m = B(nu=[1e-6, 2e-6], kappa={"A": [0.0, 5e-6], "c": 1e-6}).for_member(1)
    assert isinstance(m, B) and (m.nu, m.kappa) == (2e-6, {"A": 5e-6, "c": 1e-6})
    assert B(nu=[1e-6, 2e-6]).max_stable_dt(g) == B(nu=2e-6).max_stable_dt(g)


def test_closure_tuple_rules(swmhd):
    S = swmhd
    E = S._lib.SwmhdError
    from swmhd_amd.closure import check_closure, closure_for_member, split_closure
    lap, bih = S.ScalarDiffusivity(kappa={"A": 5e-3}), S.ScalarBiharmonicDiffusivity(nu=2e-6)
    names = ("u", "v", "h", "A")
    assert split_closure(None) == (None, None) and split_closure(()) == (None, None)
    assert split_closure(lap) == (lap, None) and split_closure(bih) == (None, bih)
    assert split_closure((bih, lap)) == (lap, bih) and split_closure([lap]) == (lap, None)
    for bad in ((lap, lap), (bih, lap, bih)):
        with pytest.raises(E, match="closure.*at most one"):
            split_closure(bad)
    for bad in (1e-3, (lap, 1e-3), "ScalarDiffusivity", (None,)):
        with pytest.raises(E, match="closure"):
            split_closure(bad)
    assert check_closure(None, names, (), False) == (None, None)
    c2, c4 = check_closure((lap, bih), names, ("c",), False)
    assert c2 == {"u": 0.0, "v": 0.0, "h": 0.0, "A": 5e-3, "c": 0.0} and c4 == {"u": 2e-6, "v": 2e-6, "h": 0.0, "A": 0.0, "c": 0.0}
    assert check_closure(bih, names, (), False) == (None, {"u": 2e-6, "v": 2e-6, "h": 0.0, "A": 0.0})
    # the refusals are those of the Laplacian closure, for either kind and for the tuple
    for c in (bih, (lap, bih)):
        for kw in (dict(bounded=True), dict(slabs=True), dict(ring=True), dict(fused=False)):
            with pytest.raises(E, match="SWMHD_ENOTSUP"):
                check_closure(c, names, (), False, **kw)
        with pytest.raises(E, match="SWMHD_ENOTSUP.*conservative viscous stress"):
            check_closure(c, ("uh", "vh", "h", "A"), (), True)
    assert check_closure(S.ScalarBiharmonicDiffusivity(kappa=1e-6), ("uh", "vh", "h", "A"), (), True)[1]["A"] == 1e-6
    per = (S.ScalarDiffusivity(nu=[1e-3, 2e-3]), S.ScalarBiharmonicDiffusivity(kappa={"A": [0.0, 5e-6]}))
    one = closure_for_member(per, 1)
    assert isinstance(one, tuple) and one[0].nu == 2e-3 and one[1].kappa == {"A": 5e-6}
    assert closure_for_member(None, 0) is None and closure_for_member(per[1], 0).kappa == {"A": 0.0}


def test_constructor_refusals_before_any_device(swmhd, monkeypatch):
    S = swmhd
    E = S._lib.SwmhdError
    import swmhd_amd.ensemble as ens_mod
    import swmhd_amd.model as model_mod

    def no_allocation(*a, **k):
        raise AssertionError("allocated before the refusal")
    monkeypatch.setattr(model_mod, "Field", no_allocation)
    monkeypatch.setattr(ens_mod.torch, "zeros", no_allocation)
    g = S.RectilinearGrid(size=(16, 16), x=(0, 1), y=(0, 1))
    B = S.ScalarBiharmonicDiffusivity
    for c in (B(nu=1e-6, kappa=1e-6), (S.ScalarDiffusivity(kappa=1e-3), B(nu=1e-6))):
        for topo in (("Bounded", "Periodic", "Flat"), ("Periodic", "Bounded", "Flat"), ("Bounded", "Bounded", "Flat")):
            gb = S.RectilinearGrid(size=(16, 16), x=(0, 1), y=(0, 1), topology=topo)
            with pytest.raises(E, match="SWMHD_ENOTSUP"):
                S.ShallowWaterModel(gb, closure=c)
            with pytest.raises(E, match="SWMHD_ENOTSUP"):
                S.BoundedShallowWaterEnsemble(gb, 2, closure=c)
            with pytest.raises(E, match="SWMHD_ENOTSUP"):
                S.ShallowWaterEnsemble(gb, 2, closure=c)
        with pytest.raises(E, match="SWMHD_ENOTSUP"):
            S.ShallowWaterModel(g, closure=c, fused=False)
        with pytest.raises(E, match="SWMHD_ENOTSUP"):
            S.ShallowWaterModel(g, closure=c, ring=ctypes.c_void_p(1))
        with pytest.raises(E, match="SWMHD_ENOTSUP"):
            S.ShallowWaterModel(S.RectilinearGrid(size=(16, 8), x=(0, 1), y=(0, 1), j_offset=0, Ny_global=16), closure=c,
                                decomp=S.SlabDecomposition(16, 2, 0))
        for cls, args in ((S.ShallowWaterModel, (g,)), (S.ShallowWaterEnsemble, (g, 2))):
            with pytest.raises(E, match="SWMHD_ENOTSUP.*conservative viscous stress"):
                cls(*args, formulation=S.ConservativeFormulation, closure=c)
    for cls, args in ((S.ShallowWaterModel, (g,)), (S.ShallowWaterEnsemble, (g, 2))):
        with pytest.raises(E, match="kappa names"):
            cls(*args, closure=B(kappa={"c": 1e-6}))
        with pytest.raises(E, match="kappa names"):
            cls(*args, tracers=("d",), closure=(S.ScalarDiffusivity(kappa={"d": 1e-3}), B(kappa={"A": 1e-6, "c": 1e-6})))
        with pytest.raises(E, match="closure"):
            cls(*args, closure=(B(), 1e-3))
        with pytest.raises(E, match="at most one ScalarBiharmonicDiffusivity"):
            cls(*args, closure=(B(), B()))
    with pytest.raises(E, match="SWMHD_ENOTSUP"):
        S.ShallowWaterEnsemble(g, 2, formulation=S.ConservativeFormulation, closure=B(nu=[0.0, 1e-6]))
    with pytest.raises(E, match="closure coefficient of A"):
        S.ShallowWaterEnsemble(g, 3, closure=B(kappa=[1e-6, 2e-6]))
