"""CPU pins of the tracer reference (tests/tracer_cases.py) before a GPU test relies on it: its (q1, q2, h, A) are bitwise
oracle.time_step, a tracer that starts as A with A's boundary conditions stays bitwise A, and a second tracer stays finite."""
import numpy as np
import pytest

import tracer_cases as TC


@pytest.mark.parametrize("form,lor", TC.FORMS)
@pytest.mark.parametrize("Nx,Ny,topo", TC.PERIODIC_GRIDS + TC.BOUNDED_GRIDS)
def test_reference_stepper_is_the_oracles_time_step(oracle, form, lor, Nx, Ny, topo):
    O = oracle
    dt = 2e-3
    gradA = TC.grad_A(topo)
    q = TC.fill_state(O, TC.state(Nx, Ny, form, 5), Nx, Ny, topo, gradA)
    d = TC.fill(O, TC.tracer_fields(Nx, Ny, 2, 5)[1], Nx, Ny, topo)
    ref = TC.RefModel(O, q, [q[3], d], Nx, Ny, form, lor, topo, gradA, tgrads=[gradA, None])
    qo = [a.copy() for a in q]
    for _ in range(5):
        O.time_step(*qo, Nx, Ny, TC.H, TC.H, TC.DX, TC.DY, dt, form, lor, TC.GRAV, TC.FCOR, topo=topo, gradA=gradA)
        ref.step(dt)
    for a, b in zip(ref.q, qo):
        assert np.array_equal(a, b)
    assert np.array_equal(ref.tr[0], ref.q[3])          # c := A stays A, halos included
    assert np.isfinite(ref.tr[1]).all()
    assert not np.array_equal(ref.tr[1], d)             # (and it was advected)
