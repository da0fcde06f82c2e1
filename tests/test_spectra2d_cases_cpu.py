"""CPU pins of the yardstick of the 2-D / isotropic spectra (tests/spectra2d_cases.py): the longdouble reference against numpy.fft.rfft2
within the bound with exact-twiddle constant RFFT_ETA; a single Fourier mode lands in exactly the predicted entry and shell; Parseval for
P2 and for E; the shell statement against the exact integer rule at wx = wy = 1; NS and the mode counts against the host mirror's
isotropic_shells."""
import numpy as np
import pytest

import spectra2d_cases as S2

LD = S2.LD
PIN_SIZES = [s for s in S2.SIZES if s[0] * s[1] <= 256 * 512]


def _frame(Nx, Ny, seed=0):
    return np.random.default_rng([Nx, Ny, seed]).standard_normal((Ny, Nx))


@pytest.mark.parametrize("Nx,Ny", PIN_SIZES, ids=[f"{a}x{b}" for a, b in PIN_SIZES])
def test_reference_against_rfft2(Nx, Ny):
    F = _frame(Nx, Ny)
    for wx, wy in S2.METRICS[:1] if Nx * Ny > 64 * 64 else S2.METRICS:
        p2, pb, E, Eb = S2.spectra_of_frames(F, wx, wy, eta=S2.RFFT_ETA)
        X = np.fft.rfft2(F).T / (Nx * Ny)                      # (Nx/2 + 1, Ny)
        got = S2.ckx(Nx)[:, None] * (X.real * X.real + X.imag * X.imag)
        fails, ratio = S2.compare(got, p2, pb)
        print(f"{Nx}x{Ny}: rfft2 against the longdouble reference: largest error / bound = {ratio:.4f}")
        assert not fails and 0 < ratio < 1, fails
        sh, NS = S2.shell_index(Nx, Ny, wx, wy), S2.shells(Nx, Ny, wx, wy)
        gotE = np.bincount(sh.ravel(), weights=got.ravel(), minlength=NS)
        fails, ratio = S2.compare(gotE, E, Eb)
        assert not fails and gotE.shape == (NS,), fails


@pytest.mark.parametrize("Nx,Ny,a,b", [(8, 4, 0, 0), (8, 4, 3, 1), (8, 4, 4, 2), (8, 4, 0, 3), (64, 64, 5, 60), (64, 64, 32, 32), (64, 4, 31, 2),
                                       (4, 64, 2, 33), (4, 64, 1, 31)])
def test_single_mode_lands_in_one_entry_and_shell(Nx, Ny, a, b):
    """cos(2 pi (a i/Nx + b j/Ny)), 0 <= a <= Nx/2: all of its mean square stands in entry (a, b) (and, for a = 0 or Nx/2, in its
    conjugate (a, -b) too), and in the shell the statement gives for it."""
    i, j = np.meshgrid(np.arange(Nx), np.arange(Ny))
    F = np.cos(2 * np.pi * (a * i / Nx + b * j / Ny))
    mean2 = float((F * F).mean())
    for wx, wy in S2.METRICS:
        p2, pb, E, Eb = S2.spectra_of_frames(F, wx, wy)
        want = np.zeros((Nx // 2 + 1, Ny))
        where = {(a, b)} | ({(a, (Ny - b) % Ny)} if a in (0, Nx // 2) else set())
        for e in where:
            want[e] = mean2 / len(where)
        assert np.allclose(p2.astype(np.float64), want, rtol=0, atol=1e-14), (Nx, Ny, a, b)
        my = b if b <= Ny // 2 else b - Ny
        s = int(np.floor(np.sqrt(np.float64(wx) * np.float64(a * a) + np.float64(wy) * np.float64(my * my)) + 0.5))
        wantE = np.zeros(S2.shells(Nx, Ny, wx, wy))
        wantE[s] = mean2
        assert np.allclose(E.astype(np.float64), wantE, rtol=0, atol=1e-14), (Nx, Ny, a, b, wx, wy)


@pytest.mark.parametrize("Nx,Ny", [(4, 4), (8, 4), (4, 64), (64, 64), (512, 4)])
def test_parseval(Nx, Ny):
    F = _frame(Nx, Ny, 1)
    mean2 = (F.astype(LD) ** 2).mean()
    for wx, wy in S2.METRICS:
        p2, pb, E, Eb = S2.spectra_of_frames(F, wx, wy)
        assert abs(p2.sum() - mean2) <= 64 * S2.U53 * mean2 * np.log2(Nx * Ny) and abs(E.sum() - mean2) <= 64 * S2.U53 * mean2 * np.log2(Nx * Ny)
        assert (pb > 0).all() and (Eb >= 0).all()


@pytest.mark.parametrize("Nx,Ny", S2.SIZES, ids=[f"{a}x{b}" for a, b in S2.SIZES])
def test_integer_shells_at_unit_metric(Nx, Ny):
    """wx = wy = 1: shell s holds exactly the modes with (2s - 1)^2 <= 4 (mx^2 + my^2) < (2s + 1)^2, in integers."""
    sh = S2.shell_index(Nx, Ny, 1.0, 1.0)
    mx = np.arange(Nx // 2 + 1, dtype=np.int64)[:, None]
    ky = np.arange(Ny, dtype=np.int64)[None, :]
    my = np.where(ky <= Ny // 2, ky, ky - Ny)
    r4 = 4 * (mx * mx + my * my)
    # (s - 1/2 <= r < s + 1/2, squared; at s = 0 the lower side, -1/2 <= r, holds for every mode and is not squared)
    assert ((sh == 0) | ((2 * sh - 1) ** 2 <= r4)).all() and (r4 < (2 * sh + 1) ** 2).all()
    assert sh.max() + 1 == S2.shells(Nx, Ny, 1.0, 1.0) and sh[0, 0] == 0 and sh.max() == sh[Nx // 2, Ny // 2]


def test_shells_are_monotone_in_each_direction():
    """What the column pass relies on: for fixed mx the shell does not decrease with |my| (and likewise in mx)."""
    for Nx, Ny in ((64, 64), (4, 4096), (4096, 4), (256, 512)):
        for wx, wy in S2.METRICS:
            sh = S2.shell_index(Nx, Ny, wx, wy)
            pos = sh[:, :Ny // 2 + 1]
            assert (np.diff(pos, axis=1) >= 0).all() and (np.diff(sh, axis=0) >= 0).all()
            assert (sh[:, Ny // 2 + 1:] == pos[:, 1:Ny // 2][:, ::-1]).all()      # my and -my share a shell


def test_shell_count_and_mode_counts_agree_with_the_host_mirror(swmhd):
    from swmhd_amd import spectra2d as M
    for (Nx, Ny), (Lx, Ly) in zip(S2.SIZES + ((64, 64), (64, 64)), [(10.0, 10.0)] * 10 + [(10.0, 20.0), (10.0 / 0.6, 10.0)]):
        g = swmhd.RectilinearGrid(size=(Nx, Ny), x=(0, Lx), y=(-Ly / 2, Ly / 2))
        dk, wx, wy = M.metric(g)
        assert dk == max(2 * np.pi / Lx, 2 * np.pi / Ly) and max(wx, wy) == 1.0 and 0 < min(wx, wy) <= 1.0
        k, counts = M.isotropic_shells(g)
        NS = S2.shells(Nx, Ny, wx, wy)
        assert NS == M.shells(g) == len(k) == len(counts) == swmhd._lib.lib().swmhd_spectra2d_shells(Nx, Ny, wx, wy)
        assert counts.dtype == np.int64 and counts.sum() == Nx * Ny and np.array_equal(counts, S2.counts(Nx, Ny, wx, wy))
        assert np.array_equal(k, dk * np.arange(NS)) and np.array_equal(M.shell_index(Nx, Ny, wx, wy), S2.shell_index(Nx, Ny, wx, wy))
    g = swmhd.RectilinearGrid(size=(64, 64), x=(0, 10.0), y=(0, 20.0))
    assert M.metric(g)[1:] == (1.0, 0.25)
    assert S2.shells(64, 64, 1.0, 1.0) == 46 and S2.shells(4, 4, 1.0, 1.0) == 4 and S2.shells(4096, 4096, 1.0, 1.0) == 2897
    # 4 x 4 by hand: (0,0) | (+-1,0) (0,+-1) (+-1,+-1) | (2,0) (0,2) (2,+-1) (+-1,2) | (2,2)
    assert S2.counts(4, 4, 1.0, 1.0).tolist() == [1, 8, 6, 1]


def test_case_list_covers_what_it_must():
    cs = S2.cases()
    assert len(cs) == len(set(cs)) and {(c.Nx, c.Ny) for c in cs} >= set(S2.SIZES)
    for size in S2.SIZES:
        mine = [c for c in cs if (c.Nx, c.Ny) == size]
        assert {c.form for c in mine} == {0, 1} and {np.dtype(c.dtype) for c in mine} == {np.dtype("f8"), np.dtype("f4")}
    assert {(c.wx, c.wy) for c in cs} == set(S2.METRICS) and {c.outs for c in cs} == set(S2.OUTS)
    assert {c.which for c in cs} >= {S2.ALL, S2.SPARSE} | {S2.BITS[n] for n in S2.NAMES}
    assert any(c.pitch for c in cs) and {c.wrap for c in cs} == {0, S2.WRAP_X, S2.WRAP_Y, S2.WRAP_X | S2.WRAP_Y}
    assert all(len(e) == 10 for e in S2.ensemble_cases()) and any(e[4] for e in S2.ensemble_cases()) and S2.ENSEMBLE_MEMBERS == 3
