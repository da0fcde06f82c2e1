"""CPU pins of the reference of the zonal spectra (tests/spectra_cases.py): the longdouble FFT against the direct DFT, Parseval, pure
tones through the frame definitions, numpy.fft.rfft in double held to the same bound with the radix-2 constant of exact twiddles, and
what the case list covers.  No GPU, no torch."""
import math

import numpy as np
import pytest

import output_cases as OC
import spectra_cases as SC

LD = SC.LD
ULD = LD(np.finfo(LD).eps) / 2      # unit roundoff of longdouble here


@pytest.mark.parametrize("Nx", [n for n in SC.NXS if n <= SC.DIRECT_MAX])
def test_longdouble_fft_against_the_direct_dft(Nx):
    """Both in longdouble: the direct sum is off by at most (Nx + 2) u sum|x| per mode, the FFT by 10 log2(Nx) u ||x||_2."""
    x = np.random.default_rng(Nx).standard_normal((3, Nx))
    dr, di = SC.dft_direct(x)
    fr, fi = SC.fft_ld(x)
    tol = (Nx + 2) * ULD * np.abs(x).sum(axis=-1, keepdims=True).astype(LD) + 10 * int(math.log2(Nx)) * ULD * np.sqrt((x.astype(LD) ** 2).sum(axis=-1, keepdims=True))
    err = np.maximum(np.abs(dr - fr), np.abs(di - fi))
    print(f"Nx = {Nx}: largest |fft - direct| / tolerance = {float((err / tol).max()):.3f}; of the mean square {float((err / np.sqrt((x ** 2).mean())).max()):.2e}")
    assert (err <= tol).all()
    # and against numpy's double transform, loosely: the indexing and the sign of the exponent
    ref = np.fft.fft(x)
    assert np.abs(fr.astype(np.float64) - ref.real).max() < 1e-12 * Nx and np.abs(fi.astype(np.float64) - ref.imag).max() < 1e-12 * Nx


def test_the_fft_continues_the_direct_dft_above_256():
    x = np.random.default_rng(1).standard_normal((2, 1024))
    a, b = SC.spectrum_of_frames(x)[0], None
    old = SC.DIRECT_MAX
    try:
        SC.DIRECT_MAX = 4096
        b = SC.spectrum_of_frames(x)[0]
    finally:
        SC.DIRECT_MAX = old
    assert float(np.abs(a - b).max()) <= float(1e3 * ULD * (x ** 2).mean())


@pytest.mark.parametrize("Nx", SC.NXS)
def test_parseval(Nx):
    x = np.random.default_rng(100 + Nx).standard_normal((3, Nx)) * 3.0 + 0.5
    want, bound = SC.spectrum_of_frames(x)
    assert want.shape == (Nx // 2 + 1,) and (want >= 0).all() and (bound > 0).all()
    ms = (x.astype(LD) ** 2).sum() / LD(x.size)
    assert abs(want.sum() - ms) <= 8 * Nx * ULD * ms
    assert float(bound.max()) < 1e-12 * float(ms)      # rounding is thirteen orders below an indexing error, which is O(P[k])


def _tone_parents(Nx, Ny, Hx, Hy, k0, a, phases):
    """vector-invariant parents whose u is a cos(2 pi k0 (i-1)/Nx + phi_j), halos periodic; v, h, A plain"""
    i = np.arange(-Hx, Nx + Hx)
    q1 = np.empty((Ny + 2 * Hy, Nx + 2 * Hx))
    for j in range(-Hy, Ny + Hy):
        q1[Hy + j] = a * np.cos(2 * np.pi * ((k0 * i) % Nx) / Nx + phases[j % Ny])
    one = np.ones_like(q1)
    return q1, 0.25 * one, 1.5 * one, 0.0 * one


@pytest.mark.parametrize("Nx", [4, 8, 64, 512, 4096])
def test_pure_tones(Nx):
    Ny, Hx, Hy, a = 3, 2, 2, 1.75
    phases = [0.3, 1.1, 2.9]
    for k0 in sorted({0, 1, Nx // 4, Nx // 2 - 1, Nx // 2}):
        q = _tone_parents(Nx, Ny, Hx, Hy, k0, a, phases)
        want, bound = SC.reference(q, Nx, Ny, Hx, Hy, 0.1, 0.1, 1, (0, Ny), SC.BITS["u"] | SC.BITS["v"] | SC.BITS["h"])
        exact = np.zeros(Nx // 2 + 1, dtype=LD)
        exact[k0] = LD(a) ** 2 / 2 if 0 < k0 < Nx // 2 else np.mean([LD(a) ** 2 * LD(math.cos(p)) ** 2 for p in phases])
        err = np.abs(want[0] - exact)
        assert (err <= bound[0]).all(), (Nx, k0, float(err.max()), np.argmax(err - bound[0]))
        assert float(bound[0].max()) < 1e-12 * a * a
        # v and h are constants: everything at k = 0
        for n, c in ((1, 0.25), (2, 1.5)):
            assert float(want[n][0]) == c * c and float(np.abs(want[n][1:]).max()) <= float(bound[n][1:].max())


@pytest.mark.parametrize("Nx", SC.NXS)
def test_numpy_rfft_in_double_is_within_the_bound_with_the_radix2_constant(Nx):
    """An independent implementation in double: the bound is not wrong in the tight direction."""
    rows = 5
    x = np.random.default_rng(7 * Nx).standard_normal((rows, Nx))
    want, bound = SC.spectrum_of_frames(x, eta=SC.RFFT_ETA)
    f = np.fft.rfft(x, axis=-1) / Nx
    p = f.real ** 2 + f.imag ** 2
    p[:, 1:Nx // 2] *= 2
    fails, ratio = SC.compare(p.mean(axis=0), want, bound)
    print(f"Nx = {Nx}: numpy.fft.rfft largest error / bound = {ratio:.4f} (margin {1 / max(ratio, 1e-300):.0f}x)")
    assert not fails, fails[:5]
    # an indexing error is far outside: the spectrum shifted by one mode
    fails, _ = SC.compare(np.roll(p.mean(axis=0), 1), want, bound)
    assert len(fails) >= Nx // 2


def test_reference_is_the_frame_then_the_dft():
    c = SC.Case(16, 7, 3, 4, False, (2, 5), 0, SC.F32, SC.ALL, SC.WRAP_X | SC.WRAP_Y)
    q = SC.inputs(c)
    dx, dy = SC.spacing(c.dtype)
    fr = SC.frames_of(q, 16, 7, 3, 4, dx, dy, 0, (2, 5), SC.ALL, c.wrap)
    assert fr.shape == (7, 3, 16) and fr.dtype == np.float64 and np.isfinite(fr).all()
    filled = OC.wrap_parents([np.array(a, dtype=np.float64) for a in q], 16, 7, 3, 4)
    assert np.array_equal(fr, OC.np_output_fields(*filled, 16, 7, 3, 4, dx, dy, 0, rows=(2, 5)))
    want, bound = SC.expected(c)
    assert want.shape == (7, 9) and np.isfinite(want.astype(np.float64)).all()
    ms = (fr.astype(LD) ** 2).mean(axis=(1, 2))
    assert (np.abs(want.sum(axis=-1) - ms) <= 1e-17 * ms).all()
    # without the WRAP flags the NaN halo ring of these inputs reaches u (x - 1), v and B_x (y - 1): non-finite spectra there only
    w2, _ = SC.reference(q, 16, 7, 3, 4, dx, dy, 0, (2, 5), SC.ALL, 0)
    assert np.isfinite(w2.astype(np.float64)).all(axis=-1).tolist() == [False, True, True, True, False, True, False]
    assert SC.reference(q, 16, 7, 3, 4, dx, dy, 0, (4, 4), SC.ALL, 0)[0].shape == (7, 0)


def test_case_list_covers_what_the_kernel_can_get_wrong():
    cs = SC.cases()
    assert len({SC.case_id(c) for c in cs}) == len(cs)
    full = lambda c: c.rows is None
    for Nx in SC.NXS:                                   # every log2 Nx from 2 to 12, rows 1, 2, 7, both formulations and precisions
        mine = [c for c in cs if c.Nx == Nx and full(c)]
        assert {1, 2, 7} <= {c.Ny for c in mine}
        assert {c.form for c in mine} == {0, 1} and {np.dtype(c.dtype) for c in mine} == {np.dtype("f8"), np.dtype("f4")}
    assert SC.NXS == tuple(2 ** p for p in range(2, 13))
    for Nx in (8, 64):
        assert set(SC.W_ROWS) <= {c.Ny for c in cs if c.Nx == Nx} and SC.W_ROWS == (255, 256, 257, 513)
        for form in (0, 1):
            assert {c.which for c in cs if c.Nx == Nx and c.form == form} >= {1, 2, 4, 8, 16, 32, 64, 127}
    assert any(c.Nx == 4096 and (SC.rows_of(c)[1] - SC.rows_of(c)[0]) % 2 == 1 and SC.rows_of(c)[1] > 1 for c in cs)
    assert any(c.pitch for c in cs) and any(c.rows not in (None,) and c.rows[0] == c.rows[1] for c in cs)
    assert {c.wrap for c in cs} == {0, SC.WRAP_X, SC.WRAP_Y, SC.WRAP_X | SC.WRAP_Y}
    assert SC.ETA <= 16 and abs(SC.ETA - (4 + 4 * math.sqrt(2))) < 0.01 and SC.ETA >= 4 + 4 * math.sqrt(2)
