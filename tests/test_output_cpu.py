"""CPU tests (no GPU) that pin the numpy restatement of the output frames (tests/output_cases.py) and the writer's schedule arithmetic.

(a) B_x, B_y of A = -exp(-r^2/4), h = 1 converge to the analytic field at second order, as MHD_visualize.jl:19-20,55-65,74-75,101-108
    measures.  (b) The frames carry the energies: with plot_cases.np_diagnostics as the yardstick, the magnetic energy summed from the
    B_x, B_y, h frames equals its magnetic energy (both formulations), the kinetic energy summed from the s, h frames its kinetic energy
    (vector-invariant form; the conservative form's KE is the different expression (1/h)(uh^2 + vh^2)), and max|u frame| its max_abs_u
    exactly.  Bar 2e-12: N^2 = 16384 summands x 2^-53 = 1.8e-12 is the most a different summation order could produce, rounded up.
(c) TimeInterval / IterationInterval arithmetic and the up-front capacity check of run()."""
import numpy as np
import pytest

import output_cases as OC
import plot_cases as P

H = 3


def test_magnetic_field_converges_at_second_order():
    Ns, errs = [50, 100, 200, 400], []
    for N in Ns:
        d = 10.0 / N
        k = np.arange(-H, N + H)
        xc, xf = -5 + (k + 0.5) * d, -5 + k * d
        X, Y = np.meshgrid(xc, xc)
        A = -np.exp(-(X ** 2 + Y ** 2) / 4)
        h, z = np.ones_like(A), np.zeros_like(A)
        bx, by = OC.np_output_fields(z, z, h, A, N, N, H, H, d, d, 1, names=("B_x", "B_y"))
        Xc, Yf = np.meshgrid(xc[H:H + N], xf[H:H + N])
        Xf, Yc = np.meshgrid(xf[H:H + N], xc[H:H + N])
        dA = lambda x, y, w: 0.5 * w * np.exp(-(x ** 2 + y ** 2) / 4)     # dA/dw of -exp(-r^2/4)
        errs.append((np.abs(bx + dA(Xc, Yf, Yf)).max(), np.abs(by - dA(Xf, Yc, Xf)).max()))
    e = np.array(errs)
    for c in (0, 1):
        slope = -np.polyfit(np.log10(Ns), np.log10(e[:, c]), 1)[0]
        print("B component", c, "errors", e[:, c], "order", slope)
        assert 1.9 <= slope <= 2.1, (c, slope, e[:, c])


@pytest.mark.parametrize("N", [64, 128])
@pytest.mark.parametrize("form", [1, 0])
def test_frames_carry_the_energies(N, form):
    q, d = P.initial_fields(N, "low_B_low_U", form)
    q[2] = q[2] + 0.1 * np.random.default_rng(1).random(q[2].shape)       # h not constant
    q = OC.wrap_parents(q, N, N, H, H)
    ref = P.np_diagnostics(*q, N, N, d, d, form)
    u, hh, s, bx, by = OC.np_output_fields(*q, N, N, H, H, d, d, form, names=("u", "h", "s", "B_x", "B_y"))
    me = OC.magnetic_density_from_frames(bx, by, hh).sum() * (d * d)
    rel = abs(me - ref["magnetic_energy"]) / ref["magnetic_energy"]
    print(N, form, "ME rel", rel)
    assert rel <= 2e-12
    if form == 1:
        ke = OC.kinetic_energy_from_frames(s, hh, d, d)
        rel = abs(ke - ref["kinetic_energy"]) / ref["kinetic_energy"]
        print(N, form, "KE rel", rel)
        assert rel <= 2e-12
    assert np.abs(u).max() == ref["max_abs_u"]


def test_restatement_rows_and_copies():
    """A row range is the same rows of the whole frame; u v h A of the vector-invariant form are the parents' interior."""
    rng = np.random.default_rng(3)
    Nx, Ny = 20, 12
    q = [rng.standard_normal((Ny + 2 * H, Nx + 2 * H)) for _ in range(4)]
    q[2] = 1.0 + 0.3 * np.abs(q[2])
    for form in (1, 0):
        whole = OC.np_output_fields(*q, Nx, Ny, H, H, 0.1, 0.2, form)
        part = OC.np_output_fields(*q, Nx, Ny, H, H, 0.1, 0.2, form, rows=(3, 9))
        assert whole.shape == (7, Ny, Nx) and np.array_equal(part, whole[:, 3:9])
    I = (slice(H, H + Ny), slice(H, H + Nx))
    vi = OC.np_output_fields(*q, Nx, Ny, H, H, 0.1, 0.2, 1, names=("u", "v", "h", "A"))
    assert all(np.array_equal(vi[k], q[k][I]) for k in range(4))


class _StubModel:
    """What run() and FieldTimeSeries need of a model before the first frame; stepping it is an error."""
    iteration, clock_time = 0, 0.0

    def time_steps(self, n, dt):
        raise AssertionError("run() stepped the model before refusing")


def test_schedule_arithmetic(swmhd):
    S = swmhd
    from swmhd_amd import output as W
    assert S.TimeInterval(0.1).steps(0.01) == 10 and S.IterationInterval(5).steps(0.01) == 5
    its = W.frame_iterations(S.TimeInterval(0.1), 0.01, 3000)              # dt = 0.01 to t = 30
    assert len(its) == 301 and its[1] == 10 and its[-1] == 3000
    assert np.allclose(np.array(its) * 0.01, np.linspace(0.0, 30.0, 301), rtol=0, atol=1e-12)
    with pytest.raises(S._lib.SwmhdError):
        S.TimeInterval(0.1).steps(0.03)                                   # 3.33 steps: Oceananigans would shorten one; we refuse
    with pytest.raises(S._lib.SwmhdError):
        S.IterationInterval(0).steps(0.01)
    with pytest.raises(S._lib.SwmhdError):
        S.FieldTimeSeries(_StubModel(), names=("u", "w"), capacity=4)     # unknown field
    with pytest.raises(S._lib.SwmhdError):
        S.FieldTimeSeries(_StubModel(), capacity=None)
    small = S.FieldTimeSeries(_StubModel(), schedule=S.TimeInterval(0.1), capacity=300)
    with pytest.raises(S._lib.SwmhdError, match="capacity 300 < 301"):
        S.run(_StubModel(), 0.01, stop_time=30.0, writers=[small])         # refused before any step (the stub would assert)
    with pytest.raises(S._lib.SwmhdError):
        S.run(_StubModel(), 0.03, stop_time=30.0, writers=[S.FieldTimeSeries(_StubModel(), capacity=10 ** 6)])
    with pytest.raises(S._lib.SwmhdError):
        S.run(_StubModel(), 0.01, writers=[])                              # neither stop_time nor stop_iteration
