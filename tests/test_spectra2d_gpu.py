"""GPU tests of the 2-D and isotropic spectra (swmhd_spectra2d_*, ShallowWaterModel.isotropic_spectra / power_spectra_2d) and of their
writer (IsotropicSpectrumTimeSeries, run).

The yardstick is tests/spectra2d_cases.py (pinned on the CPU by tests/test_spectra2d_cases_cpu.py): the float64 frame values, a longdouble
DFT along both directions, the shell statement in float64, and the normwise FFT bound per mode with eta = 9.66 over log2 Nx + log2 Ny
stages, summed per shell with gamma_(n-1) E[s].  What does not depend on rounding -- the same call twice, a member against the single
call, a mask against the full mask, WRAP against filled halos, f32 against widened f64, out_shell with and without out_2d, an order of
names -- is compared BITWISE.  Every comparison prints its largest error / bound first."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import plot_cases as P
import spectra2d_cases as S2
import spectra_cases as SC
import zonal_cases as ZC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, SENT = 16, -777.25
SFX = {np.dtype("f8"): "f64", np.dtype("f4"): "f32"}
TORCH = {np.dtype("f8"): torch.float64, np.dtype("f4"): torch.float32}
LD = S2.LD


def _s2(S, dev, dtype, Nx, Ny, Hx, Hy, sy, form, which, flags, wx, wy, outs="both", members=None, stride_m=0, spacing=None):
    """swmhd_[ensemble_]spectra2d_* on the device tensors `dev` (q1, q2, h, A): (E, P2) as numpy, (popcount, NS) and (popcount, Nx/2+1,
    Ny) with a leading members axis for the ensemble call; None for an output not asked for.  Both outputs lie in buffers of sentinels
    -- a guard in front and behind, 3 doubles behind every spectrum and every column, 5 behind every field's plane, 2 behind every
    member -- and the workspace has exactly the stated size with a guard behind it: every sentinel must survive."""
    nf, nkx, NS, M = bin(which).count("1"), Nx // 2 + 1, S2.shells(Nx, Ny, wx, wy), members or 1
    L = S._lib.lib()
    assert L.swmhd_spectra2d_shells(Nx, Ny, wx, wy) == NS
    need = L.swmhd_spectra2d_workspace(Nx, Ny, nf, M, wx, wy)
    assert need == S2.workspace(Nx, Ny, nf, M, wx, wy)
    ws = torch.full((need + 2 * GUARD,), SENT, dtype=torch.float64, device="cuda")
    oss = NS + 3
    osm = nf * oss + 2
    ebuf = torch.full((2 * GUARD + M * osm,), SENT, dtype=torch.float64, device="cuda")
    o2kx = Ny + 3
    o2f = nkx * o2kx + 5
    o2m = nf * o2f + 2
    pbuf = torch.full((2 * GUARD + M * o2m,), SENT, dtype=torch.float64, device="cuda")
    dx, dy = spacing or (S2.DX, S2.DY)
    sfx = SFX[np.dtype(dtype)]
    ptrs = [t.data_ptr() for t in dev]
    eptr = ebuf.data_ptr() + 8 * GUARD if outs in ("both", "shell") else None
    pptr = pbuf.data_ptr() + 8 * GUARD if outs in ("both", "2d") else None
    wsp = ws.data_ptr() + 8 * GUARD
    if members is None:
        rc = getattr(L, f"swmhd_spectra2d_{sfx}")(*ptrs, Nx, Ny, Hx, Hy, sy, dx, dy, form, which, wx, wy, wsp, eptr, oss, pptr, o2kx, o2f, flags,
                                                  S.fields._stream_ptr())
    else:
        rc = getattr(L, f"swmhd_ensemble_spectra2d_{sfx}")(*ptrs, members, stride_m, Nx, Ny, Hx, Hy, sy, dx, dy, form, which, wx, wy, wsp, eptr, oss,
                                                           osm, pptr, o2kx, o2f, o2m, flags, S.fields._stream_ptr())
    S._lib.check(rc, "swmhd_spectra2d")
    w, eb, pb = ws.cpu().numpy(), ebuf.cpu().numpy(), pbuf.cpu().numpy()
    assert (w[:GUARD] == SENT).all() and (w[GUARD + need:] == SENT).all(), "written outside the stated workspace"
    E = P2 = None
    if eptr is None:
        assert (eb == SENT).all(), "out_shell was not asked for"
    else:
        body = eb[GUARD:GUARD + M * osm].reshape(M, osm)
        spec = body[:, :nf * oss].reshape(M, nf, oss)
        assert (eb[:GUARD] == SENT).all() and (eb[GUARD + M * osm:] == SENT).all() and (body[:, nf * oss:] == SENT).all(), "guard of out_shell overwritten"
        assert (spec[:, :, NS:] == SENT).all(), "sentinels behind a shell spectrum overwritten"
        E = spec[:, :, :NS].copy()
        assert not (E == SENT).any(), "a shell was not written"
    if pptr is None:
        assert (pb == SENT).all(), "out_2d was not asked for"
    else:
        body = pb[GUARD:GUARD + M * o2m].reshape(M, o2m)
        fld = body[:, :nf * o2f].reshape(M, nf, o2f)
        cols = fld[:, :, :nkx * o2kx].reshape(M, nf, nkx, o2kx)
        assert (pb[:GUARD] == SENT).all() and (pb[GUARD + M * o2m:] == SENT).all() and (body[:, nf * o2f:] == SENT).all(), "guard of out_2d overwritten"
        assert (fld[:, :, nkx * o2kx:] == SENT).all() and (cols[..., Ny:] == SENT).all(), "sentinels behind a column or a plane overwritten"
        P2 = cols[..., :Ny].copy()
        assert not (P2 == SENT).any(), "an entry of out_2d was not written"
    if members is None:
        E, P2 = (None if E is None else E[0]), (None if P2 is None else P2[0])
    return E, P2


def _upload(parents):
    return [torch.from_numpy(np.array(a)).cuda() for a in parents]


def _case_call(S, c, parents=None, flags=None, dtype=None, spacing=None, outs=None, which=None):
    q = S2.inputs(c) if parents is None else parents
    return _s2(S, _upload(q), c.dtype if dtype is None else dtype, c.Nx, c.Ny, c.Hx, c.Hy, S2.stride_y(c), c.form, c.which if which is None else which,
               c.wrap if flags is None else flags, c.wx, c.wy, outs=c.outs if outs is None else outs, spacing=spacing)


def _check(got, want, label):
    """(E, P2) of a call against expected(): prints the largest error / bound of each, returns the failures"""
    E, P2 = got
    p2, pb, e, ebound = want
    fails = []
    if P2 is not None:
        f, ratio = S2.compare(P2, p2, pb)
        print(f"{label}: P2: largest error / bound = {ratio:.4f}")
        fails += f
    if E is not None:
        f, ratio = S2.compare(E, e, ebound)
        print(f"{label}: E: largest error / bound = {ratio:.4f}")
        fails += f
    return fails


def _same(a, b):
    return all((x is None and y is None) or (x is not None and y is not None and S2.same_bits(x, y)) for x, y in zip(a, b))


CASES = S2.cases()


@pytest.mark.parametrize("c", CASES, ids=[S2.case_id(c) for c in CASES])
def test_every_case_is_within_the_bound_and_repeats_bitwise(swmhd, c):
    got = _case_call(swmhd, c)
    assert not _check(got, S2.expected(c), S2.case_id(c))
    for a in got:
        assert a is None or (np.isfinite(a).all() and (a >= 0).all())
    assert _same(_case_call(swmhd, c), got), "two runs of the same call differ"
    if got[0] is not None:       # a shell that holds no mode gets exactly 0.0
        empty = S2.counts(c.Nx, c.Ny, c.wx, c.wy) == 0
        assert (got[0][:, empty] == 0.0).all() and not np.signbit(got[0][:, empty]).any()


@pytest.mark.parametrize("Nx,Ny,wx,wy", [(8, 4, 4.0, 4.0), (64, 64, 9.0, 2.25), (4, 512, 1.0, 6.25)])
def test_an_empty_shell_is_zero(swmhd, Nx, Ny, wx, wy):
    """A shell width below a spectral spacing (wx or wy > 1: the C call takes any positive metric) leaves shells without a mode: exactly
    +0.0, behind, between and in front of shells that hold modes; the others within the bound."""
    c = S2.Case(Nx, Ny, 3, 4, False, 1, S2.F64, S2.SPARSE, 0, wx, wy, "both")
    got = _case_call(swmhd, c)
    assert not _check(got, S2.expected(c), S2.case_id(c))
    empty = S2.counts(Nx, Ny, wx, wy) == 0
    assert empty.any() and not empty.all() and len(empty) == got[0].shape[-1]
    assert (got[0][:, empty] == 0.0).all() and not np.signbit(got[0][:, empty]).any() and (got[0][:, ~empty] > 0).all()


@pytest.mark.parametrize("Nx,Ny,form,dtype", [(4, 4, 1, S2.F64), (64, 64, 0, S2.F64), (256, 512, 0, S2.F32), (512, 4, 1, S2.F64)])
def test_outputs_and_masks_do_not_change_the_bits(swmhd, Nx, Ny, form, dtype):
    """out_shell alone and out_2d alone have the bits they have together; a mask has the bits of the full mask."""
    c = S2.Case(Nx, Ny, 3, 4, True, form, dtype, S2.ALL, 0, 1.0, 0.25, "both")
    E, P2 = _case_call(swmhd, c)
    assert np.isfinite(E).all() and np.isfinite(P2).all()
    Es, none = _case_call(swmhd, c, outs="shell")
    none2, Pp = _case_call(swmhd, c, outs="2d")
    assert none is None and none2 is None and S2.same_bits(Es, E) and S2.same_bits(Pp, P2)
    for which in (S2.SPARSE, S2.BITS["s"], S2.BITS["u"] | S2.BITS["v"] | S2.BITS["A"]):
        idx = [k for k, n in enumerate(S2.NAMES) if which & S2.BITS[n]]
        e, p = _case_call(swmhd, c, which=which)
        assert S2.same_bits(e, E[idx]) and S2.same_bits(p, P2[idx]), which


ENS = S2.ensemble_cases()


def _ensemble_tensors(members, dtype, per, stride_m):
    dev = []
    for k in range(4):
        t = torch.full((len(members) * stride_m,), float("nan"), dtype=TORCH[np.dtype(dtype)], device="cuda")
        for m, q in enumerate(members):
            t[m * stride_m:m * stride_m + per] = torch.from_numpy(np.array(q[k])).reshape(-1)
        dev.append(t)
    return dev


@pytest.mark.parametrize("e", ENS, ids=[S2.ensemble_case_id(e) for e in ENS])
def test_ensemble_member_has_the_bits_of_the_single_call(swmhd, e):
    """Three members with data of their own, dense or pitched (a gap of NaN between them): every member within the bound of its
    reference and bitwise the single call on that member."""
    S = swmhd
    Nx, Ny, form, dtype, pitched, which, wrap, wx, wy, outs = e
    Hx, Hy, sy, B = S2.ENS_HX, S2.ENS_HY, Nx + 2 * S2.ENS_HX, S2.ENSEMBLE_MEMBERS
    per = (Ny + 2 * Hy) * sy
    stride_m = per + (S2.ENSEMBLE_GAP if pitched else 0)
    members = [S2.ensemble_member_inputs(Nx, Ny, dtype, m, wrap) for m in range(B)]
    got = _s2(S, _ensemble_tensors(members, dtype, per, stride_m), dtype, Nx, Ny, Hx, Hy, sy, form, which, wrap, wx, wy, outs=outs, members=B,
              stride_m=stride_m)
    dx, dy = S2.spacing(dtype)
    for m in range(B):
        want = S2.reference(members[m], Nx, Ny, Hx, Hy, dx, dy, form, which, wx, wy, wrap)
        mine = tuple(None if a is None else a[m] for a in got)
        assert not _check(mine, want, f"{S2.ensemble_case_id(e)} member {m}")
        single = _s2(S, _upload(members[m]), dtype, Nx, Ny, Hx, Hy, sy, form, which, wrap, wx, wy, outs=outs)
        assert _same(mine, single), f"member {m} differs from the single call"
    for a in got:
        assert a is None or (np.isfinite(a).all() and not S2.same_bits(a[0], a[1]))


@pytest.mark.parametrize("Nx,Ny,form,dtype", [(4, 4, 1, S2.F64), (8, 4, 0, S2.F32), (64, 64, 0, S2.F64), (4, 512, 1, S2.F32), (1024, 4, 0, S2.F64)])
def test_wrap_on_nan_halos_has_the_bits_of_the_plain_call_on_filled_halos(swmhd, Nx, Ny, form, dtype):
    for wrap in (S2.WRAP_X | S2.WRAP_Y, S2.WRAP_X, S2.WRAP_Y):
        c = S2.Case(Nx, Ny, 3, 4, False, form, dtype, S2.ALL if Nx * Ny <= 4096 else S2.SPARSE, wrap, 1.0, 1.0, "both")
        filled = [a.astype(dtype) for a in ZC.wrap_ring(S2.inputs(c), Nx, Ny, 3, 4, wrap)]
        plain = _case_call(swmhd, c, parents=filled, flags=0)
        assert np.isfinite(plain[0]).all() and np.isfinite(plain[1]).all()
        assert _same(_case_call(swmhd, c), plain), wrap


def test_wrap_flags_stand_in_for_a_missing_halo(swmhd):
    """Hx = Hy = 0 with both WRAP flags: the reach is served by the periodic images, bitwise as with a halo of one cell."""
    Nx, Ny = 32, 8
    c = S2.Case(Nx, Ny, 1, 1, False, 0, S2.F64, S2.ALL, S2.WRAP_X | S2.WRAP_Y, 0.36, 1.0, "both")
    ref = _case_call(swmhd, c)
    bare = [np.ascontiguousarray(a[1:-1, 1:-1]) for a in S2.inputs(c)]
    got = _s2(swmhd, _upload(bare), S2.F64, Nx, Ny, 0, 0, Nx, 0, S2.ALL, S2.WRAP_X | S2.WRAP_Y, c.wx, c.wy)
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all() and _same(got, ref)


@pytest.mark.parametrize("Nx,Ny,form", [(8, 4, 1), (64, 64, 0), (4, 4096, 1), (4096, 4, 0)])
def test_f32_entry_point_has_the_bits_of_f64_on_the_widened_parents(swmhd, Nx, Ny, form):
    c = S2.Case(Nx, Ny, 3, 4, True, form, S2.F32, S2.ALL if Nx * Ny <= 4096 else S2.SPARSE, 0, 1.0, 1.0, "both")
    narrow = _case_call(swmhd, c)
    wide = _case_call(swmhd, c, parents=[a.astype(np.float64) for a in S2.inputs(c)], dtype=S2.F64, spacing=S2.spacing(S2.F32))
    assert np.isfinite(narrow[0]).all() and np.isfinite(narrow[1]).all() and _same(narrow, wide)


def _poisoned(field, form):
    """The spectra whose stencil holds a NaN placed in `field` (0 q1, 1 q2, 2 h, 3 A) at an interior cell (tests/test_zonal_spectra_gpu.py)"""
    cons = form == 0
    reads = {"u": {0} | ({2} if cons else set()), "v": {1} | ({2} if cons else set()), "h": {2}, "A": {3},
             "s": {0, 1} | ({2} if cons else set()), "B_x": {2, 3}, "B_y": {2, 3}}
    return [field in reads[n] for n in S2.NAMES]


@pytest.mark.parametrize("form", [1, 0])
@pytest.mark.parametrize("field", [0, 1, 2, 3])
def test_one_nan_cell_poisons_exactly_the_fields_whose_stencil_holds_it(swmhd, form, field):
    """A NaN in one cell of member 1 of three: P2 of that member's fields that read the cell is NaN in every entry, and E in every shell
    that holds a mode (an empty shell stays 0.0); every other field, and every other member, has the bits of the clean run."""
    S = swmhd
    Nx, Ny, Hx, Hy, B, bad, y, x = 64, 8, S2.ENS_HX, S2.ENS_HY, 3, 1, 3, 31
    wx, wy = 1.0, 0.25
    sy = Nx + 2 * Hx
    per = (Ny + 2 * Hy) * sy
    members = [S2.ensemble_member_inputs(Nx, Ny, S2.F64, m, 0) for m in range(B)]

    def run(dirty):
        dev = _ensemble_tensors(members, S2.F64, per, per)
        if dirty:
            dev[field][bad * per + (Hy + y) * sy + Hx + x] = float("nan")
        return _s2(S, dev, S2.F64, Nx, Ny, Hx, Hy, sy, form, S2.ALL, 0, wx, wy, members=B, stride_m=per)
    (cE, cP), (dE, dP) = run(False), run(True)
    assert np.isfinite(cE).all() and np.isfinite(cP).all()
    hit = _poisoned(field, form)
    wantP = np.zeros(cP.shape, dtype=bool)
    wantP[bad, hit] = True
    full = S2.counts(Nx, Ny, wx, wy) > 0
    wantE = np.zeros(cE.shape, dtype=bool)
    wantE[bad, hit] = full
    assert wantP.any() and not wantP.all() and np.array_equal(np.isnan(dP), wantP) and np.array_equal(np.isnan(dE), wantE)
    assert S2.same_bits(dP[~wantP], cP[~wantP]) and S2.same_bits(dE[~wantE], cE[~wantE])


# --- the host mirror ---------------------------------------------------------------------------------------------------------------
FORMS = {"VectorInvariant": 1, "Conservative": 0}
N = 32


def _vortex(m):
    u0 = lambda X, Y: Y * np.exp(-(X ** 2 + Y ** 2))
    v0 = lambda X, Y: -X * np.exp(-(X ** 2 + Y ** 2))
    n1, n2 = m.names[:2]
    members = getattr(m, "members", None)
    A0 = P.two_gaussians(0.1) if members is None else [P.two_gaussians(0.1 * (k + 1)) for k in range(members)]
    m.set(**{n1: u0, n2: v0, "h": lambda X, Y: 1.0 + 0.05 * np.exp(-(X ** 2 + Y ** 2)), "A": A0})
    return m


def _make(S, kind, form, Ly=5):
    g = S.RectilinearGrid(size=(N, N), x=(-5, 5), y=(-Ly, Ly))
    return _vortex(S.ShallowWaterEnsemble(g, 3, 9.81, 1.0, formulation=form) if kind == "ensemble" else S.ShallowWaterModel(g, 9.81, 1.0, formulation=form))


def _reference_of_frames(fr, grid):
    from swmhd_amd import spectra2d as M
    _, wx, wy = M.metric(grid)
    return S2.spectra_of_frames(fr, wx, wy)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("kind", ["single", "ensemble"])
def test_writer_beside_the_frames_with_graph_replay(swmhd, kind, form):
    """32 x 32, ten steps through a captured graph with the frame writer and the spectrum writer attached: every stored spectrum is
    bitwise what an eager isotropic_spectra call gives at the same iteration of a twin run, and within the bound of the reference
    applied to the float64 frame stored at that iteration."""
    S = swmhd
    dt, names = 0.002, S2.NAMES
    m = _make(S, kind, form)
    m.capture_graph(dt)
    frames = S.FieldTimeSeries(m, names=names, schedule=S.IterationInterval(2), capacity=8, array_type=torch.float64)
    spectra = S.IsotropicSpectrumTimeSeries(m, names=names, schedule=S.IterationInterval(2), capacity=8)
    S.run(m, dt, stop_iteration=6, writers=[frames, spectra])
    S.run(m, dt, stop_iteration=10, writers=[frames, spectra])
    assert spectra.iterations == [0, 2, 4, 6, 8, 10] == frames.iterations and spectra.times == frames.times and len(spectra) == 6
    lead = () if kind == "single" else (3,)
    NS = S2.shells(N, N, 1.0, 1.0)
    got, fr = spectra.numpy(), frames.numpy()
    assert got.dtype == np.float64 and got.shape == (6,) + lead + (7, NS) and tuple(spectra.spectra.shape) == (8,) + lead + (7, NS)
    _, _, want, bound = _reference_of_frames(fr, m.grid)
    fails, ratio = S2.compare(got, want, bound)
    print(f"{kind} {form}: largest error / bound = {ratio:.4f}")
    assert np.isfinite(got).all() and not fails, fails[:8]
    assert not np.array_equal(got[0], got[-1])
    twin = _make(S, kind, form)
    twin.capture_graph(dt)
    eager = [twin.isotropic_spectra(names).cpu().numpy()]
    for _ in range(5):
        twin.time_steps(2, dt)
        eager.append(twin.isotropic_spectra(names).cpu().numpy())
    assert twin.iteration == m.iteration == 10
    assert S2.same_bits(np.stack(eager), got)
    with pytest.raises(S._lib.SwmhdError):
        for _ in range(3):
            spectra.write()                                              # 8 slots


@pytest.mark.parametrize("form", list(FORMS))
def test_any_order_and_repetition_of_names_and_members(swmhd, form):
    """A permuted and repeated list has the bits of the plain one; `out`; the members of an ensemble have the bits of member(m); a
    rectangular domain (Ly = 2 Lx: wy = 1/4) is what the frame's reference gives."""
    S = swmhd
    m = _make(S, "single", form, Ly=10)
    m.time_steps(3, 0.002)
    NS, nkx = S2.shells(N, N, 1.0, 0.25), N // 2 + 1
    E, P2 = m.isotropic_spectra(S2.NAMES), m.power_spectra_2d(S2.NAMES)
    assert E.dtype == P2.dtype == torch.float64 and tuple(E.shape) == (7, NS) and tuple(P2.shape) == (7, nkx, N) and E.is_cuda and P2.is_cuda
    E, P2 = E.cpu().numpy(), P2.cpu().numpy()
    order = ("B_y", "u", "u", "s", "A", "h", "v", "B_x", "B_y")
    idx = [S2.NAMES.index(n) for n in order]
    assert S2.same_bits(m.isotropic_spectra(order).cpu().numpy(), E[idx]) and S2.same_bits(m.power_spectra_2d(order).cpu().numpy(), P2[idx])
    assert S2.same_bits(m.isotropic_spectra().cpu().numpy(), E[[0, 1, 3]])           # the default: u v A
    out = torch.full((5, 2, NS), SENT, dtype=torch.float64, device="cuda")
    assert m.isotropic_spectra(("s", "A"), out=out[2]) is not None and S2.same_bits(out[2].cpu().numpy(), E[[4, 3]])
    assert (out[[0, 1, 3, 4]] == SENT).all()
    for bad in (torch.empty((2, NS), dtype=torch.float32, device="cuda"), torch.empty((2, NS - 1), dtype=torch.float64, device="cuda"),
                torch.empty((2, NS), dtype=torch.float64)):
        with pytest.raises(S._lib.SwmhdError):
            m.isotropic_spectra(("s", "A"), out=bad)
    fr = m.output_fields(S2.NAMES, array_type=torch.float64).cpu().numpy()
    p2, pb, e, eb = _reference_of_frames(fr, m.grid)
    assert not _check((E, P2), (p2, pb, e, eb), f"{form} against the frame")
    ens = _make(S, "ensemble", form)
    ens.time_steps(3, 0.002)
    all_E, all_P = ens.isotropic_spectra(order).cpu().numpy(), ens.power_spectra_2d(order).cpu().numpy()
    assert all_E.shape == (3, len(order), S2.shells(N, N, 1.0, 1.0)) and all_P.shape == (3, len(order), nkx, N)
    for k in range(3):
        assert S2.same_bits(all_E[k], ens.member(k).isotropic_spectra(order).cpu().numpy()), k
        assert S2.same_bits(all_P[k], ens.member(k).power_spectra_2d(order).cpu().numpy()), k
    assert np.isfinite(all_E).all() and not S2.same_bits(all_E[0], all_E[1])


@pytest.mark.parametrize("form", list(FORMS))
def test_sums_agree_with_the_zonal_spectra(swmhd, form):
    """sum_ky P2[kx, .] is zonal_spectra's P[kx] and sum_s E[s] is sum_k P[k], each within the sum of the two bounds: all are
    statements about the same float64 frame."""
    S = swmhd
    m = _make(S, "single", form)
    m.time_steps(5, 0.002)
    names = ("u", "v", "A", "B_x")
    E, P2 = m.isotropic_spectra(names).cpu().numpy().astype(LD), m.power_spectra_2d(names).cpu().numpy().astype(LD)
    Z = m.zonal_spectra(names).cpu().numpy().astype(LD)
    fr = m.output_fields(names, array_type=torch.float64).cpu().numpy()
    _, zbound = SC.spectrum_of_frames(fr)
    _, pb, _, eb = _reference_of_frames(fr, m.grid)
    # (the test's own sums are in longdouble: no term for them)
    for k, n in enumerate(names):
        tol = pb[k].sum(axis=-1) + zbound[k]
        diff = np.abs(P2[k].sum(axis=-1) - Z[k])
        print(f"{form} {n}: sum_ky P2 against zonal_spectra: largest |difference| / bound = {float((diff / tol).max()):.4f}")
        assert (diff <= tol).all() and (Z[k] > 0).any(), n
        tol = eb[k].sum() + zbound[k].sum()
        print(f"{form} {n}: sum_s E against sum_k P: |difference| / bound = {float(abs(E[k].sum() - Z[k].sum()) / tol):.4f}")
        assert abs(E[k].sum() - Z[k].sum()) <= tol, n


def test_refusals_of_the_host_mirror(swmhd):
    S = swmhd
    Err = S._lib.SwmhdError
    m = S.ShallowWaterModel(S.RectilinearGrid(size=(32, 32), x=(-5, 5), y=(-5, 5)), 9.81, 1.0, tracers=("c",))
    for names in (("u", "c"), ("w",), ("uu",), ()):
        for f in (m.isotropic_spectra, m.power_spectra_2d):
            with pytest.raises(Err):
                f(names)
        with pytest.raises(Err):
            S.IsotropicSpectrumTimeSeries(m, names, capacity=2)
    with pytest.raises(Err, match="capacity"):
        S.IsotropicSpectrumTimeSeries(m, ("u",))                               # no capacity
    for size, topo in (((32, 32), ("Bounded", "Periodic", "Flat")), ((32, 32), ("Periodic", "Bounded", "Flat")), ((48, 32), ("Periodic", "Periodic", "Flat")),
                       ((32, 48), ("Periodic", "Periodic", "Flat"))):
        b = S.ShallowWaterModel(S.RectilinearGrid(size=size, x=(-5, 5), y=(-5, 5), topology=topo), 9.81, 1.0)
        for f in (b.isotropic_spectra, b.power_spectra_2d):
            with pytest.raises(Err):
                f(("u",))
        with pytest.raises(Err):
            S.IsotropicSpectrumTimeSeries(b, ("u",), capacity=2)
        assert getattr(b, "_spectra2d_ws", None) is None                       # refused before anything was allocated
    # the C call answers an unsupported size itself, and writes nothing
    for Nx, Ny in ((48, 32), (32, 48)):
        sy = Nx + 6
        q = _upload(ZC._parents(Nx, Ny, 3, 4, sy, S2.F64, 0, Ny, 0))
        out = torch.full((4096,), SENT, dtype=torch.float64, device="cuda")
        out2 = torch.full((7 * 25 * 48 + 64,), SENT, dtype=torch.float64, device="cuda")
        ws = torch.full((1 << 16,), SENT, dtype=torch.float64, device="cuda")
        rc = S._lib.lib().swmhd_spectra2d_f64(*[t.data_ptr() for t in q], Nx, Ny, 3, 4, sy, S2.DX, S2.DY, 1, S2.ALL, 1.0, 1.0, ws.data_ptr(), out.data_ptr(), 64,
                                              out2.data_ptr(), 48, 25 * 48, 0, S.fields._stream_ptr())
        torch.cuda.synchronize()
        assert rc == 3 and (out == SENT).all() and (out2 == SENT).all() and (ws == SENT).all()


def test_example_writes_isotropic_spectra(tmp_path):
    """examples/run_swmhd.py --isotropic-spectra: the last sample of a 32^2 run of five steps equals a recomputation from the fields the
    run dumped at that iteration (periodic: the ring of halo cells is the periodic image); without the flag no file is written."""
    H = 3
    out = tmp_path / "o"
    exe = [sys.executable, os.path.join(ROOT, "examples", "run_swmhd.py"), "--size", "32", "--stop-time", "0.05", "--every", "5", "--out", str(out)]
    r = subprocess.run(exe + ["--isotropic-spectra", "0.01", "--dump-every", "0.05", "--ic", "gaussians"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out / "isotropic_spectra.npz")
    names = ["u", "v", "A"]
    NS = S2.shells(32, 32, 1.0, 1.0)
    assert list(z["names"]) == names and z["spectra"].shape == (6, 3, NS) and z["spectra"].dtype == np.float64
    assert list(z["iterations"]) == list(range(6)) and np.allclose(z["times"], np.arange(6) * 0.01, rtol=0, atol=1e-12)
    assert np.allclose(z["k"], 2 * np.pi / 10.0 * np.arange(NS), rtol=1e-15, atol=0) and np.array_equal(z["counts"], S2.counts(32, 32, 1.0, 1.0))
    final = np.load(out / "fields_0000005.npz")
    q = [final[n] for n in ("u", "v", "h", "A")]
    which = sum(S2.BITS[n] for n in names)
    _, _, want, bound = S2.reference(q, 32, 32, H, H, 10 / 32, 10 / 32, 1, which, 1.0, 1.0, S2.WRAP_X | S2.WRAP_Y)
    fails, ratio = S2.compare(z["spectra"][-1], want, bound)
    print(f"example: largest error / bound = {ratio:.4f}")
    assert not fails, fails[:8]
    assert z["spectra"][-1, 0, 1:].max() > 0 and not os.path.exists(out / "zonal_spectra.npz")
    os.remove(out / "isotropic_spectra.npz")
    r = subprocess.run(exe, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not os.path.exists(out / "isotropic_spectra.npz")
