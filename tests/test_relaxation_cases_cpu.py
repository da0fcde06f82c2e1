"""CPU tests (no GPU) that pin tests/relaxation_cases.py, the reference of the Relaxation forcing: the strict restatement against the
longdouble value within the stated bound, the reference stepper against tracer_cases.RefModel where there is no forcing and its two
schedules against each other, and the RK3 property -- drag and thermal relaxation of uniform fields decay as the RK3 polynomial."""
import numpy as np
import pytest

import relaxation_cases as RC
import tracer_cases as T

H = RC.H


def _fields(t, seed, shape=(9, 13)):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(shape).astype(t) for _ in range(3)]


@pytest.mark.parametrize("t", [np.float64, np.float32])
def test_strict_is_the_written_order_and_within_the_bound_of_exact(t):
    old, mask, target = _fields(t, 3)
    rate, tval = 0.37, -1.3
    eps = np.finfo(t).eps
    for m, tg in ((None, 0.0), (None, tval), (None, target), (mask, 0.0), (mask, tval), (mask, target)):
        D = RC.relax_strict(old, rate, m, tg)
        assert D.dtype == t
        # the written order, operation by operation
        p = t(rate) * m if m is not None else t(rate)
        d = (tg if isinstance(tg, np.ndarray) else t(tg)) - old
        assert np.array_equal(D, p * d)
        E, S = RC.relax_exact(old, rate, m, tg)
        assert E.dtype == np.longdouble and np.all(S >= 0)
        err = np.abs(D.astype(np.longdouble) - E)
        assert np.all(err <= RC.fast_bound_D(S, eps))
        assert err.max() > 0                                  # (the bound is not met by an exact zero)
        # the update: new + a D in strict order is inside the update bound of the exact value
        new = _fields(t, 4)[0]
        a = 0.013 * 0.37
        got = RC.correct(new, D, a)
        assert got.dtype == t
        ref = new.astype(np.longdouble) + np.longdouble(t(a)) * E
        assert np.all(np.abs(got.astype(np.longdouble) - ref) <= RC.fast_bound(ref, t(a), S, eps))
    # no mask is not a mask of ones times a rounded rate in another order: p = rate exactly
    assert np.array_equal(RC.relax_strict(old, rate, None, 0.0), t(rate) * (t(0.0) - old))
    assert RC.UPDATE_ROUNDINGS == 4 and RC.D_ROUNDINGS == 2


def test_field_kinds_cover_the_six():
    assert len(set(RC.FIELD_KINDS)) == 6
    assert {RC.kind_of(k) for k in range(RC.MAX_FIELDS)} == set(RC.FIELD_KINDS)
    assert len({RC.kind_of(k) for k in range(4)}) == 4
    assert RC.NFIELDS == (1, 4, 12) and RC.MAX_FIELDS == 4 + 8


@pytest.mark.parametrize("form,lor", T.FORMS)
def test_reference_stepper_without_a_forcing_is_the_tracer_reference(oracle, form, lor):
    """No forcing, and one whose rates are 0: bitwise tracer_cases.RefModel, Periodic and a channel."""
    O = oracle
    for Nx, Ny, topo in (T.PERIODIC_GRIDS[0], T.BOUNDED_GRIDS[0]):
        gradA = T.grad_A(topo)
        q = T.fill_state(O, T.state(Nx, Ny, form, 7, rough=False), Nx, Ny, topo, gradA)
        tr = [T.fill(O, c, Nx, Ny, topo) for c in T.tracer_fields(Nx, Ny, 2, 7, rough=False)]
        want = T.RefModel(O, q, tr, Nx, Ny, form, lor, topo, gradA)
        none = RC.RefModel(O, q, tr, [None] * 6, Nx, Ny, form, lor, "classic", topo, gradA)
        zero = RC.RefModel(O, q, tr, [(0.0, None, 1.0)] * 6, Nx, Ny, form, lor, "classic", topo, gradA)
        for _ in range(2):
            want.step(2e-3); none.step(2e-3); zero.step(2e-3)
        for a, b, c in zip(want.q + want.tr, none.q + none.tr, zero.q + zero.tr):
            assert np.array_equal(a, b) and np.array_equal(a, c)


@pytest.mark.parametrize("form,lor", T.FORMS)
def test_classic_and_anchor_schedules_agree(oracle, form, lor):
    """The two schedules of the reference are the same RK3 step up to rounding, and the forcing moves the fields by far more."""
    O = oracle
    Nx, Ny, topo = T.PERIODIC_GRIDS[0]
    q = T.fill_state(O, T.state(Nx, Ny, form, 7, rough=False), Nx, Ny, topo)
    tr = [T.fill(O, c, Nx, Ny, topo) for c in T.tracer_fields(Nx, Ny, 1, 7, rough=False)]
    rng = np.random.default_rng(5)
    mask, target = rng.random((Ny, Nx)), 1.0 + 0.1 * rng.standard_normal((Ny, Nx))
    relax = [(0.8, None, 0.0), (0.8, mask, 0.0), (0.5, None, target), None, (0.3, mask, 0.2)]
    runs = {mode: RC.RefModel(O, q, tr, relax, Nx, Ny, form, lor, mode) for mode in ("classic", "anchor")}
    plain = RC.RefModel(O, q, tr, [None] * 5, Nx, Ny, form, lor, "classic")
    for _ in range(5):
        for r in list(runs.values()) + [plain]:
            r.step(2e-3)
    for a, b, c in zip(runs["classic"].q + runs["classic"].tr, runs["anchor"].q + runs["anchor"].tr, plain.q + plain.tr):
        assert np.abs(a - b).max() <= 1e-13 * np.abs(a).max()
    for k in (0, 1, 2, 4):
        a, c = (runs["classic"].q + runs["classic"].tr)[k], (plain.q + plain.tr)[k]
        assert np.abs(a - c).max() > 1e-6 * np.abs(a).max()


@pytest.mark.parametrize("which", ["drag", "thermal"])
def test_rk3_property_of_the_reference(oracle, which):
    """Uniform fields, f = 0, A = 0: the advective tendencies are exactly zero, so 20 steps multiply u (drag) or h - H_eq (thermal
    relaxation) by P(-r dt)^20.  Prints the reference's deviation, which relaxation_cases records."""
    O = oracle
    Nx, Ny = RC.DECAY_NX, RC.DECAY_NY
    q, relax = RC.decay_case(which)
    G = O.tendencies(*q, Nx, Ny, H, H, RC.DX, RC.DY, 1, 1, T.GRAV, 0.0)
    I = (slice(H, H + Ny), slice(H, H + Nx))
    assert not any(np.any(g[I]) for g in G)
    m = RC.RefModel(O, q, [], relax, Nx, Ny, 1, 1, "classic", fcor=0.0)
    for _ in range(RC.DECAY_STEPS):
        m.step(RC.DECAY_DT)
    Pn = float(RC.decay_polynomial())
    dev = RC.decay_deviation(which, m.q[0] if which == "drag" else m.q[2])
    print(f"{which}: P(z)^{RC.DECAY_STEPS} = {Pn:.6f}, relative deviation of the reference = {dev:.3e}")
    assert 0.5 < Pn < 0.7                                       # the case decays visibly
    assert 0 < dev <= RC.DECAY_MARGIN[which]
    assert RC.DECAY_MARGIN[which] == 10 * RC.DECAY_REFERENCE_DEVIATION[which]
    # nothing else moved
    for k, a in enumerate(m.q):
        if k != (0 if which == "drag" else 2):
            assert np.array_equal(a, q[k])
    # the anchor schedule of the reference holds the property within the same margin
    f = RC.RefModel(O, q, [], relax, Nx, Ny, 1, 1, "anchor", fcor=0.0)
    for _ in range(RC.DECAY_STEPS):
        f.step(RC.DECAY_DT)
    devf = RC.decay_deviation(which, f.q[0] if which == "drag" else f.q[2])
    print(f"{which}: relative deviation of the reference's anchor schedule = {devf:.3e}")
    assert devf <= RC.DECAY_MARGIN[which]
