"""CPU tests of the Coriolis reference (tests/coriolis_cases.py): the correction the engine applies after its stage kernels is the same
RK3 step as Oceananigans' "f x U is part of the tendency"; with beta = 0 it is the oracle's own scalar f; the row tables sit on the
grid's own y; the fast bounds hold for numpy evaluations in both operation orders; and a Rossby wave moves westward at the
quasi-geostrophic speed."""
import numpy as np
import pytest

import coriolis_cases as CC
import tracer_cases as T

GRIDS = [(20, 12, (T.P, T.P)), (13, 10, (T.P, T.B))]
EPS = np.finfo(np.float64).eps


def _start(oracle, Nx, Ny, form, topo):
    return T.fill_state(oracle, T.state(Nx, Ny, form, 7, rough=False), Nx, Ny, topo, T.grad_A(topo))


def _rows(Ny, f0=T.FCOR, beta=0.9, y0=0.35):
    j = np.arange(Ny)
    return f0 + beta * (y0 + (j + 0.5) * T.DY), f0 + beta * (y0 + j * T.DY)


def test_the_three_modes_are_one_step(oracle):
    """One full RK3 step, both formulations, Periodic and (Periodic, Bounded).  Per stage and cell the forms round a few different
    partial results (a D apart, the sum in another order, G + D stored; the anchor's W for the weighted sum of G and G-), each bounded
    by about max |U|.  The largest deviation is measured, printed, recorded in coriolis_cases.MODES_MEASURED_EPS, and the bound is 8
    times the record."""
    worst = 0.0
    for Nx, Ny, topo in GRIDS:
        fc, ff = _rows(Ny)
        for form, lor in T.FORMS:
            q = _start(oracle, Nx, Ny, form, topo)
            kw = dict(topo=topo, gradA=T.grad_A(topo))
            ref = CC.RefModel(oracle, q, fc, ff, Nx, Ny, form, lor, "tendency", **kw).step(2e-3)
            for mode in ("classic", "anchor") if topo == (T.P, T.P) else ("classic",):
                got = CC.RefModel(oracle, q, fc, ff, Nx, Ny, form, lor, mode, **kw).step(2e-3)
                for k, (a, b) in enumerate(zip(ref.q, got.q)):
                    dev = np.abs(a[ref.I] - b[ref.I]).max() / (EPS * np.abs(a[ref.I]).max())
                    print(f"{Nx}x{Ny} {topo} form {form} {mode} field {k}: {dev:.2f} eps max|U|")
                    worst = max(worst, dev)
                    assert dev <= CC.MODES_BOUND_EPS
            # and the term does something: the step without it differs by far more
            plain = CC.RefModel(oracle, q, 0 * fc, 0 * ff, Nx, Ny, form, lor, "classic", **kw).step(2e-3)
            assert np.abs(plain.q[0][ref.I] - ref.q[0][ref.I]).max() > 1e4 * EPS
    print(f"largest deviation between the modes: {worst:.2f} eps max|U| (recorded: {CC.MODES_MEASURED_EPS})")
    assert CC.MODES_BOUND_EPS == 8 * CC.MODES_MEASURED_EPS


def test_beta_zero_is_the_oracles_f_plane(oracle):
    """BetaPlane(f0, 0) in "tendency" mode against the UNCHANGED oracle stepped with fcor = f0: the signs of both terms and the
    interpolation stencils are the reference's.  (The oracle adds f vbar inside its sum of terms, the reference after it: rounding.)"""
    worst = 0.0
    for Nx, Ny, topo in GRIDS:
        fc, ff = np.full(Ny, T.FCOR), np.full(Ny, T.FCOR)
        for form, lor in T.FORMS:
            q = _start(oracle, Nx, Ny, form, topo)
            got = CC.RefModel(oracle, q, fc, ff, Nx, Ny, form, lor, "tendency", topo=topo, gradA=T.grad_A(topo)).step(2e-3)
            want = [a.copy() for a in q]
            oracle.time_step(*want, Nx, Ny, T.H, T.H, T.DX, T.DY, 2e-3, form, lor, T.GRAV, T.FCOR, topo=topo, gradA=T.grad_A(topo))
            off = [a.copy() for a in q]
            oracle.time_step(*off, Nx, Ny, T.H, T.H, T.DX, T.DY, 2e-3, form, lor, T.GRAV, -T.FCOR, topo=topo, gradA=T.grad_A(topo))
            for k, (a, b, c) in enumerate(zip(want, got.q, off)):
                dev = np.abs(a[got.I] - b[got.I]).max() / (EPS * np.abs(a[got.I]).max())
                print(f"{Nx}x{Ny} {topo} form {form} field {k}: {dev:.2f} eps max|U|")
                worst = max(worst, dev)
                assert dev <= CC.FPLANE_BOUND_EPS
            # a wrong sign is far outside: the oracle with -f0 differs from +f0 by orders of magnitude more
            assert np.abs(want[0][got.I] - off[0][got.I]).max() > 1e6 * EPS * np.abs(want[0][got.I]).max()
    print(f"largest deviation from the oracle's f-plane: {worst:.2f} eps max|U| (recorded: {CC.FPLANE_MEASURED_EPS})")
    assert CC.FPLANE_BOUND_EPS == 8 * CC.FPLANE_MEASURED_EPS


def test_rows_sit_on_the_grids_own_y(swmhd):
    """rows(grid) = f0 + beta grid.yc / grid.yf of the interior rows, exactly: on a grid with y[0] != 0 and on a slab grid with
    j_offset != 0 (whose table is then the slab's own part of the whole domain's)."""
    S = swmhd
    f0, beta = 0.8, 1.7
    g = S.RectilinearGrid(size=(8, 6), x=(0, 1), y=(-3.0, -1.5))
    fc, ff = S.BetaPlane(f0, beta).rows(g)
    assert np.array_equal(fc, f0 + beta * g.yc[g.Hy:g.Hy + g.Ny]) and np.array_equal(ff, f0 + beta * g.yf[g.Hy:g.Hy + g.Ny])
    assert fc[0] == f0 + beta * (-3.0 + 0.5 * 0.25) and ff[0] == f0 + beta * -3.0 and fc.shape == ff.shape == (6,)
    whole = S.RectilinearGrid(size=(8, 12), x=(0, 1), y=(2.0, 5.0))
    slab = S.RectilinearGrid(size=(8, 4), x=(0, 1), y=(2.0, 5.0), j_offset=5, Ny_global=12)
    wc, wf = S.BetaPlane(f0, beta).rows(whole)
    sc, sf = S.BetaPlane(f0, beta).rows(slab)
    assert np.array_equal(sc, f0 + beta * slab.yc[3:7]) and np.array_equal(sf, f0 + beta * slab.yf[3:7])
    assert np.array_equal(sc, wc[5:9]) and np.array_equal(sf, wf[5:9])
    # FPlane and a callable
    pc, pf = S.FPlane(0.3).rows(g)
    assert np.array_equal(pc, np.full(6, 0.3)) and np.array_equal(pf, np.full(6, 0.3))
    cc, cf = S.CoriolisProfile(lambda y: np.sin(y)).rows(g)
    assert np.array_equal(cc, np.sin(g.yc[3:9])) and np.array_equal(cf, np.sin(g.yf[3:9]))
    # per member
    b = S.BetaPlane([0.5, 0.8], [1.0, 1.7])
    mc, mf = b.rows(g)
    assert mc.shape == (2, 6) and np.array_equal(mc[1], fc) and np.array_equal(mf[1], ff)
    one = b.for_member(1)
    assert (one.f0, one.beta) == (0.8, 1.7) and np.array_equal(one.rows(g)[0], fc)
    assert b.per_member == 2 and one.per_member is None


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_fast_bounds_hold_for_both_orders(dtype):
    """A numpy evaluation in the strict and in the fast operation order, in float32 and float64, stays inside |D - D_exact| <= 2 eps |f| S
    and |new - ref| <= eps |ref| + 4 eps |a| |f| S -- otherwise the derivation is wrong.  Rough fields, so that sums cancel."""
    rng = np.random.default_rng(4)
    eps = np.finfo(dtype).eps
    Ny, Nx = 23, 37
    P1, P2 = (rng.standard_normal((Ny + 2, Nx + 2)).astype(dtype) for _ in range(2))
    fc, ff = CC.row_values(Ny, dtype)
    exact = CC.coriolis_exact(P1, P2, fc, ff)
    new0 = rng.standard_normal((Ny, Nx)).astype(dtype)
    worst_D = worst_U = 0.0
    for order in (CC.coriolis_strict, CC.coriolis_fast_order):
        for D, (E, fS) in zip(order(P1, P2, fc, ff), exact):
            assert D.dtype == dtype
            err = np.abs(D.astype(np.longdouble) - E)
            assert np.all(err <= CC.fast_bound_D(fS, eps))
            worst_D = max(worst_D, float((err / (eps * fS)).max()))
            for a in (dtype(0.013 * 0.37), dtype(1.0), dtype(-0.25 * 0.013)):
                got = CC.correct(new0, D, a)
                ref = new0.astype(np.longdouble) + np.longdouble(a) * E
                err = np.abs(got.astype(np.longdouble) - ref)
                assert np.all(err <= CC.fast_bound(ref, a, fS, eps))
                worst_U = max(worst_U, float((err / CC.fast_bound(ref, a, fS, eps)).max()))
    print(f"{np.dtype(dtype).name}: largest |D - D_exact| = {worst_D:.2f} eps |f| S (bound 2); largest update error = {worst_U:.2f} of its bound")
    # the two orders give the same D where nothing underflows: the halvings are exact
    for x, y in zip(CC.coriolis_strict(P1, P2, fc, ff), CC.coriolis_fast_order(P1, P2, fc, ff)):
        assert np.array_equal(x, y)


def _rossby_run(swmhd, oracle):
    S, O = swmhd, oracle
    Nx, Ny = CC.ROSSBY_NX, CC.ROSSBY_NY
    topo = (T.P, T.B)
    g = S.RectilinearGrid(size=(Nx, Ny), x=CC.ROSSBY_X, y=CC.ROSSBY_Y, topology=("Periodic", "Bounded", "Flat"))
    fc, ff = S.BetaPlane(CC.ROSSBY_F0, CC.ROSSBY_BETA).rows(g)
    q = T.fill_state(O, CC.rossby_state(g.xc, g.xf, g.yc, g.yf), Nx, Ny, topo, None, g.dx, g.dy)
    m = CC.RefModel(O, q, fc, ff, Nx, Ny, 1, 0, "tendency", topo=topo, dx=g.dx, dy=g.dy)
    times, phases = [0.0], [CC.rossby_phase(m.q[2], g.xc, g.yc)]
    for n in range(1, CC.ROSSBY_STEPS + 1):
        m.step(CC.ROSSBY_DT)
        if n % CC.ROSSBY_EVERY == 0:
            times.append(n * CC.ROSSBY_DT)
            phases.append(CC.rossby_phase(m.q[2], g.xc, g.yc))
    return np.array(times), np.unwrap(np.array(phases)), m


def test_a_rossby_wave_moves_westward_at_the_theoretical_speed(swmhd, oracle):
    """(Periodic, Bounded) 32 x 16, small amplitude, "tendency" mode, f from BetaPlane.rows of a grid whose y starts at 5: the phase of
    the wave decreases (westward), and its speed is -beta / (k^2 + l^2 + f_mid^2 / (g H)) within twice the deviation recorded in
    coriolis_cases.ROSSBY_REFERENCE_DEVIATION.  A sign error sends it east; a y-origin error changes f_mid^2 / (g H), the largest
    term of the denominator, by a factor of (10 / 4)^2."""
    times, phases, m = _rossby_run(swmhd, oracle)
    k, l, f_mid, c_theory = CC.rossby_theory()
    slope = np.polyfit(times, phases, 1)[0]
    c = slope / k
    dev = abs(c / c_theory - 1.0)
    print(f"Rossby wave: c = {c:.5f}, theory {c_theory:.5f}, |c / c_theory - 1| = {dev:.4f} (recorded: {CC.ROSSBY_REFERENCE_DEVIATION}); "
          f"phase moved {phases[-1] - phases[0]:.4f} rad")
    assert c_theory < 0 and c < 0 and phases[-1] - phases[0] < -0.1          # westward, and visibly
    assert CC.ROSSBY_MARGIN == 2 * CC.ROSSBY_REFERENCE_DEVIATION
    assert dev <= CC.ROSSBY_MARGIN
    I = m.I
    assert np.all(np.isfinite(m.q[2])) and np.abs(m.q[2][I] - 1.0).max() < 3 * CC.ROSSBY_ETA0
    # with the origin error (y measured from the south wall) the speed is outside the margin: the test can see it
    f_wrong = CC.ROSSBY_F0 + CC.ROSSBY_BETA * 0.5 * (CC.ROSSBY_Y[1] - CC.ROSSBY_Y[0])
    c_wrong = -CC.ROSSBY_BETA / (k * k + l * l + f_wrong ** 2 / T.GRAV)
    assert abs(c_wrong / c_theory - 1.0) > 2 * CC.ROSSBY_MARGIN
