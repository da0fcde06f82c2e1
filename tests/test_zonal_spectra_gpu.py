"""GPU tests of the zonal spectra (swmhd_zonal_spectra_*, ShallowWaterModel.zonal_spectra) and of their writer (ZonalSpectrumTimeSeries, run).

The yardstick is tests/spectra_cases.py (pinned on the CPU by tests/test_spectra_cases_cpu.py): the float64 frame values, a longdouble DFT
of every row, and the normwise FFT bound per mode with eta = 9.66 derived from the kernel's butterfly and twiddle source, plus D_rows
roundings of the row summation read off the plan.  What does not depend on rounding -- the same call twice, a member against the single
call, a row range against a grid of just those rows, WRAP against filled halos, an order of names, f32 against widened f64 -- is
compared BITWISE.  Every comparison prints its largest error / bound first."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import diag_cases as DC
import plot_cases as P
import spectra_cases as SC
import zonal_cases as ZC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, SENT = 16, -777.25
SFX = {np.dtype("f8"): "f64", np.dtype("f4"): "f32"}
TORCH = {np.dtype("f8"): torch.float64, np.dtype("f4"): torch.float32}
LD = SC.LD


def _zs(S, dev, dtype, Nx, Ny, Hx, Hy, sy, form, rows, which, flags, members=None, stride_m=0, spacing=None):
    """swmhd_[ensemble_]zonal_spectra_* on the device tensors `dev` (q1, q2, h, A): spectra (popcount, Nx/2 + 1) or (members, popcount,
    Nx/2 + 1) as numpy.  `out` lies in a buffer of sentinels -- a guard in front and behind, 3 doubles after every spectrum, 2 after
    every member -- and the workspace has exactly the stated size with a guard of sentinels behind it: every sentinel must survive."""
    j0, j1 = rows
    n, nf, nk = j1 - j0, bin(which).count("1"), Nx // 2 + 1
    osk, M = nk + 3, members or 1
    osm = nf * osk + 2
    buf = torch.full((2 * GUARD + M * osm,), SENT, dtype=torch.float64, device="cuda")
    L = S._lib.lib()
    need = L.swmhd_zonal_spectra_workspace(Nx, n, nf, M)
    assert need == SC.workspace(Nx, n, nf, M)
    ws = torch.full((need + 2 * GUARD,), SENT, dtype=torch.float64, device="cuda")
    dx, dy = spacing or (SC.DX, SC.DY)
    sfx = SFX[np.dtype(dtype)]
    ptrs = [t.data_ptr() for t in dev]
    out, wsp = buf.data_ptr() + 8 * GUARD, ws.data_ptr() + 8 * GUARD
    if members is None:
        rc = getattr(L, f"swmhd_zonal_spectra_{sfx}")(*ptrs, Nx, Ny, Hx, Hy, sy, dx, dy, form, j0, j1, which, wsp, out, osk, flags, S.fields._stream_ptr())
    else:
        rc = getattr(L, f"swmhd_ensemble_zonal_spectra_{sfx}")(*ptrs, members, stride_m, Nx, Ny, Hx, Hy, sy, dx, dy, form, j0, j1, which, wsp, out, osk,
                                                              osm, flags, S.fields._stream_ptr())
    S._lib.check(rc, "swmhd_zonal_spectra")
    b, w = buf.cpu().numpy(), ws.cpu().numpy()
    assert (w[:GUARD] == SENT).all() and (w[GUARD + need:] == SENT).all(), "written outside the stated workspace"
    body = b[GUARD:GUARD + M * osm].reshape(M, osm)
    spec = body[:, :nf * osk].reshape(M, nf, osk)
    assert (b[:GUARD] == SENT).all() and (b[GUARD + M * osm:] == SENT).all() and (body[:, nf * osk:] == SENT).all(), "guard overwritten"
    assert (spec[:, :, nk:] == SENT).all(), "sentinels behind a spectrum overwritten"
    if n == 0:
        assert (spec == SENT).all(), "an empty row range wrote"
        got = np.zeros((M, nf, 0))
    else:
        got = spec[:, :, :nk].copy()
        assert not (got == SENT).any(), "a spectrum entry was not written"
    return got[0] if members is None else got


def _upload(parents):
    return [torch.from_numpy(np.array(a)).cuda() for a in parents]


def _case_call(S, c, parents=None, flags=None, dtype=None, spacing=None):
    q = SC.inputs(c) if parents is None else parents
    dtype = c.dtype if dtype is None else dtype
    return _zs(S, _upload(q), dtype, c.Nx, c.Ny, c.Hx, c.Hy, SC.stride_y(c), c.form, SC.rows_of(c), c.which, c.wrap if flags is None else flags,
               spacing=spacing)


CASES = SC.cases()


@pytest.mark.parametrize("c", CASES, ids=[SC.case_id(c) for c in CASES])
def test_every_case_is_within_the_bound_and_repeats_bitwise(swmhd, c):
    got = _case_call(swmhd, c)
    want, bound = SC.expected(c)
    fails, ratio = SC.compare(got, want, bound)
    j0, j1 = SC.rows_of(c)
    print(f"{SC.case_id(c)}: eta = {SC.ETA}, D_rows = {SC.depth(j1 - j0)}, largest error / bound = {ratio:.4f}")
    assert not fails, fails[:8]
    if j1 > j0:
        assert np.isfinite(got).all() and (got >= 0).all()
    assert SC.same_bits(_case_call(swmhd, c), got), "two runs of the same call differ"


@pytest.mark.parametrize("Nx,form,dtype", [(4, 1, SC.F64), (64, 0, SC.F64), (256, 0, SC.F32), (1024, 1, SC.F64)])
def test_a_row_range_has_the_bits_of_a_grid_of_just_those_rows(swmhd, Nx, form, dtype):
    """Rows [a, b) of a 7-row grid against the whole of the (b - a)-row grid cut out of it (its halo rows are the neighbours): the order
    of the summation depends on (Nx, rows) alone.  And a mask has the bits of the full mask."""
    Hx, Hy = 3, 4
    c = SC.Case(Nx, 7, Hx, Hy, True, None, form, dtype, SC.ALL, 0)
    q = [np.ascontiguousarray(a.astype(dtype)) for a in DC._random_parents(Nx, 7, Hx, Hy, SC.stride_y(c))]     # (finite all the way: the cut's halo rows)
    dev = _upload(q)
    sy = SC.stride_y(c)
    for (a, b) in ((2, 5), (0, 1), (6, 7), (1, 7)):
        part = _zs(swmhd, dev, dtype, Nx, 7, Hx, Hy, sy, form, (a, b), SC.ALL, 0)
        cut = _upload([p[a:b + 2 * Hy] for p in q])
        whole = _zs(swmhd, cut, dtype, Nx, b - a, Hx, Hy, sy, form, (0, b - a), SC.ALL, 0)
        assert np.isfinite(part).all() and SC.same_bits(part, whole), (a, b)
        for which in (SC.SPARSE, SC.BITS["s"], SC.BITS["u"] | SC.BITS["v"] | SC.BITS["A"]):
            idx = [k for k, n in enumerate(SC.NAMES) if which & SC.BITS[n]]
            assert SC.same_bits(_zs(swmhd, dev, dtype, Nx, 7, Hx, Hy, sy, form, (a, b), which, 0), part[idx]), ((a, b), which)


ENS = SC.ensemble_cases()


@pytest.mark.parametrize("e", ENS, ids=[SC.ensemble_case_id(e) for e in ENS])
def test_ensemble_member_has_the_bits_of_the_single_call(swmhd, e):
    """Three members with data of their own, dense (stride_m = the parent) or pitched (a gap of NaN between them): every member within
    the bound of its reference and bitwise the single call on that member."""
    S = swmhd
    Nx, Ny, form, dtype, pitched, rows, which, wrap = e
    Hx, Hy, sy, B = SC.ENS_HX, SC.ENS_HY, Nx + 2 * SC.ENS_HX, SC.ENSEMBLE_MEMBERS
    r = (0, Ny) if rows is None else rows
    per = (Ny + 2 * Hy) * sy
    stride_m = per + (SC.ENSEMBLE_GAP if pitched else 0)
    members = [SC.ensemble_member_inputs(Nx, Ny, dtype, m, rows, wrap) for m in range(B)]
    dev = []
    for k in range(4):
        t = torch.full((B * stride_m,), float("nan"), dtype=TORCH[np.dtype(dtype)], device="cuda")
        for m in range(B):
            t[m * stride_m:m * stride_m + per] = torch.from_numpy(np.array(members[m][k])).reshape(-1)
        dev.append(t)
    got = _zs(S, dev, dtype, Nx, Ny, Hx, Hy, sy, form, r, which, wrap, members=B, stride_m=stride_m)
    dx, dy = SC.spacing(dtype)
    worst = 0.0
    for m in range(B):
        want, bound = SC.reference(members[m], Nx, Ny, Hx, Hy, dx, dy, form, r, which, wrap)
        fails, ratio = SC.compare(got[m], want, bound)
        worst = max(worst, ratio)
        assert not fails, (m, fails[:8])
        single = _zs(S, _upload(members[m]), dtype, Nx, Ny, Hx, Hy, sy, form, r, which, wrap)
        assert SC.same_bits(got[m], single), f"member {m} differs from the single call"
    print(f"{SC.ensemble_case_id(e)}: largest error / bound = {worst:.4f}")
    assert np.isfinite(got).all() and not SC.same_bits(got[0], got[1])


@pytest.mark.parametrize("Nx,Ny,form,dtype", [(4, 1, 1, SC.F64), (4, 7, 0, SC.F32), (64, 7, 0, SC.F64), (256, 2, 1, SC.F32), (2048, 1, 0, SC.F64)])
def test_wrap_on_nan_halos_has_the_bits_of_the_plain_call_on_filled_halos(swmhd, Nx, Ny, form, dtype):
    for wrap in (SC.WRAP_X | SC.WRAP_Y, SC.WRAP_X, SC.WRAP_Y):
        c = SC.Case(Nx, Ny, 3, 4, False, None, form, dtype, SC.ALL, wrap)
        filled = [a.astype(dtype) for a in ZC.wrap_ring(SC.inputs(c), Nx, Ny, 3, 4, wrap)]
        plain = _case_call(swmhd, c, parents=filled, flags=0)
        assert np.isfinite(plain).all()
        assert SC.same_bits(_case_call(swmhd, c), plain), wrap


def test_wrap_flags_stand_in_for_a_missing_halo(swmhd):
    """Hx = Hy = 0 with both WRAP flags: the reach is served by the periodic images, bitwise as with a filled halo of one cell."""
    Nx, Ny = 32, 5
    c = SC.Case(Nx, Ny, 1, 1, False, None, 0, SC.F64, SC.ALL, SC.WRAP_X | SC.WRAP_Y)
    q = SC.inputs(c)
    ref = _case_call(swmhd, c)
    bare = [np.ascontiguousarray(a[1:-1, 1:-1]) for a in q]
    got = _zs(swmhd, _upload(bare), SC.F64, Nx, Ny, 0, 0, Nx, 0, (0, Ny), SC.ALL, SC.WRAP_X | SC.WRAP_Y)
    assert np.isfinite(got).all() and SC.same_bits(got, ref)


@pytest.mark.parametrize("Nx,Ny,form", [(8, 2, 1), (64, 7, 0), (256, 7, 1), (4096, 2, 0)])
def test_f32_entry_point_has_the_bits_of_f64_on_the_widened_parents(swmhd, Nx, Ny, form):
    c = SC.Case(Nx, Ny, 3, 4, True, None, form, SC.F32, SC.ALL if Nx <= 256 else SC.SPARSE, 0)
    narrow = _case_call(swmhd, c)
    wide = _case_call(swmhd, c, parents=[a.astype(np.float64) for a in SC.inputs(c)], dtype=SC.F64, spacing=SC.spacing(SC.F32))
    assert np.isfinite(narrow).all() and SC.same_bits(narrow, wide)


def _poisoned(field, form):
    """The spectra whose stencil holds a NaN placed in `field` (0 q1, 1 q2, 2 h, 3 A) at an interior cell: spelled out from the frame
    definitions (conservative velocities divide by an interpolated h; s reads u and v; B_x and B_y read A and h)."""
    cons = form == 0
    reads = {"u": {0} | ({2} if cons else set()), "v": {1} | ({2} if cons else set()), "h": {2}, "A": {3},
             "s": {0, 1} | ({2} if cons else set()), "B_x": {2, 3}, "B_y": {2, 3}}
    return [field in reads[n] for n in SC.NAMES]


@pytest.mark.parametrize("form", [1, 0])
@pytest.mark.parametrize("field", [0, 1, 2, 3])
def test_one_nan_cell_poisons_exactly_the_spectra_whose_stencil_holds_it(swmhd, form, field):
    """A NaN in one cell of member 1 of three: the spectra of that member whose field reads the cell are NaN in every entry (a row's
    transform mixes all its cells); every other spectrum, and every other member, has the bits of the clean run."""
    S = swmhd
    Nx, Ny, Hx, Hy, B, bad, y, x = 64, 7, SC.ENS_HX, SC.ENS_HY, 3, 1, 3, 31
    sy = Nx + 2 * Hx
    per = (Ny + 2 * Hy) * sy
    members = [SC.ensemble_member_inputs(Nx, Ny, SC.F64, m, None, 0) for m in range(B)]

    def run(dirty):
        dev = []
        for k in range(4):
            t = torch.cat([torch.from_numpy(np.array(members[m][k])).reshape(-1) for m in range(B)]).cuda()
            if dirty and k == field:
                t[bad * per + (Hy + y) * sy + Hx + x] = float("nan")
            dev.append(t)
        return _zs(S, dev, SC.F64, Nx, Ny, Hx, Hy, sy, form, (0, Ny), SC.ALL, 0, members=B, stride_m=per)
    clean, dirty = run(False), run(True)
    assert np.isfinite(clean).all()
    want_nan = np.zeros(clean.shape, dtype=bool)
    want_nan[bad, _poisoned(field, form), :] = True
    assert want_nan.any() and not want_nan.all() and np.array_equal(np.isnan(dirty), want_nan), np.argwhere(np.isnan(dirty) != want_nan)[:10]
    assert SC.same_bits(dirty[~want_nan], clean[~want_nan])
    # the restatement, run on the same dirty member, puts its NaN in the same places
    q = [np.array(a) for a in members[bad]]
    q[field][Hy + y, Hx + x] = np.nan
    ref = SC.reference(q, Nx, Ny, Hx, Hy, SC.DX, SC.DY, form, (0, Ny), SC.ALL)[0]
    assert np.array_equal(np.isnan(ref.astype(np.float64)), want_nan[bad])


# --- the host mirror ---------------------------------------------------------------------------------------------------------------
FORMS = {"VectorInvariant": 1, "Conservative": 0}
NX, NY = 32, 24


def _vortex(m):
    u0 = lambda X, Y: Y * np.exp(-(X ** 2 + Y ** 2))
    v0 = lambda X, Y: -X * np.exp(-(X ** 2 + Y ** 2))
    n1, n2 = m.names[:2]
    members = getattr(m, "members", None)
    if getattr(m, "_channel", False):
        A0 = [lambda X, Y, gr=gr: gr * Y for gr in m._grads]
    else:
        A0 = P.two_gaussians(0.1) if members is None else [P.two_gaussians(0.1 * (k + 1)) for k in range(members)]
    m.set(**{n1: u0, n2: v0, "h": lambda X, Y: 1.0 + 0.05 * np.exp(-(X ** 2 + Y ** 2)), "A": A0})
    return m


def _make(S, kind, form):
    if kind == "channel":
        g = S.RectilinearGrid(size=(NX, NY), x=(-5, 5), y=(-5, 5), topology=("Periodic", "Bounded", "Flat"))
        grads = [-0.01, -0.05, 0.02]
        bcs = [{"A": S.FieldBoundaryConditions(north=S.GradientBoundaryCondition(gr), south=S.GradientBoundaryCondition(gr))} for gr in grads]
        m = S.BoundedShallowWaterEnsemble(g, 3, 9.81, 1.0, formulation=form, boundary_conditions=bcs)
        m._channel, m._grads = True, grads
        return _vortex(m)
    g = S.RectilinearGrid(size=(NX, NY), x=(-5, 5), y=(-5, 5))
    return _vortex(S.ShallowWaterEnsemble(g, 3, 9.81, 1.0, formulation=form) if kind == "ensemble" else S.ShallowWaterModel(g, 9.81, 1.0, formulation=form))


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("kind", ["single", "ensemble"])
def test_writer_beside_the_frames_with_graph_replay(swmhd, kind, form):
    """32 x 24, ten steps through a captured graph with the frame writer and the spectrum writer attached: every stored spectrum is
    bitwise what an eager zonal_spectra call gives at the same iteration of a twin run, and within the bound of the reference applied
    to the float64 frame stored at that iteration; times and iterations agree; a continued run does not repeat the shared sample."""
    S = swmhd
    dt, names = 0.002, SC.NAMES
    m = _make(S, kind, form)
    m.capture_graph(dt)
    frames = S.FieldTimeSeries(m, names=names, schedule=S.IterationInterval(2), capacity=8, array_type=torch.float64)
    spectra = S.ZonalSpectrumTimeSeries(m, names=names, schedule=S.IterationInterval(2), capacity=8)
    with pytest.raises(S._lib.SwmhdError):
        S.run(m, dt, stop_iteration=10, writers=[frames, S.ZonalSpectrumTimeSeries(m, names=names, schedule=S.IterationInterval(2), capacity=5)])
    assert m.iteration == 0 and len(spectra) == 0
    S.run(m, dt, stop_iteration=6, writers=[frames, spectra])
    S.run(m, dt, stop_iteration=10, writers=[frames, spectra])           # continued: iteration 6 is in both series already
    assert spectra.iterations == [0, 2, 4, 6, 8, 10] == frames.iterations and spectra.times == frames.times and len(spectra) == 6
    lead = () if kind == "single" else (3,)
    got, fr = spectra.numpy(), frames.numpy()
    assert got.dtype == np.float64 and got.shape == (6,) + lead + (7, NX // 2 + 1) and tuple(spectra.spectra.shape) == (8,) + lead + (7, NX // 2 + 1)
    want, bound = SC.spectrum_of_frames(fr)
    fails, ratio = SC.compare(got, want, bound)
    print(f"{kind} {form}: largest error / bound = {ratio:.4f} (D_rows = {SC.depth(NY)})")
    assert np.isfinite(got).all() and not fails, fails[:8]
    assert not np.array_equal(got[0], got[-1])
    # the twin: the same run, eager calls at the same iterations, no writer
    twin = _make(S, kind, form)
    twin.capture_graph(dt)
    eager = [twin.zonal_spectra(names).cpu().numpy()]
    for _ in range(5):
        twin.time_steps(2, dt)
        eager.append(twin.zonal_spectra(names).cpu().numpy())
    assert twin.iteration == m.iteration == 10
    assert SC.same_bits(np.stack(eager), got)
    with pytest.raises(S._lib.SwmhdError):
        for _ in range(3):
            spectra.write()                                              # 8 slots


@pytest.mark.parametrize("form", list(FORMS))
def test_any_order_and_repetition_of_names_and_members(swmhd, form):
    """zonal_spectra of the model: a permuted and repeated list has the bits of the plain one; `out`; the members of an ensemble (periodic
    and channel) have the bits of member(m); the frame is what is transformed."""
    S = swmhd
    m = _make(S, "single", form)
    m.time_steps(3, 0.002)
    plain = m.zonal_spectra(SC.NAMES)
    assert plain.dtype == torch.float64 and tuple(plain.shape) == (7, NX // 2 + 1) and plain.is_cuda
    plain = plain.cpu().numpy()
    order = ("B_y", "u", "u", "s", "A", "h", "v", "B_x", "B_y")
    assert SC.same_bits(m.zonal_spectra(order).cpu().numpy(), plain[[SC.NAMES.index(n) for n in order]])
    assert SC.same_bits(m.zonal_spectra().cpu().numpy(), plain[[0, 1, 3]])           # the default: u v A
    out = torch.full((5, 2, NX // 2 + 1), SENT, dtype=torch.float64, device="cuda")
    assert m.zonal_spectra(("s", "A"), out=out[2]) is not None and SC.same_bits(out[2].cpu().numpy(), plain[[4, 3]])
    assert (out[[0, 1, 3, 4]] == SENT).all()
    for bad in (torch.empty((2, NX // 2 + 1), dtype=torch.float32, device="cuda"), torch.empty((2, NX // 2), dtype=torch.float64, device="cuda"),
                torch.empty((2, NX // 2 + 1), dtype=torch.float64)):
        with pytest.raises(S._lib.SwmhdError):
            m.zonal_spectra(("s", "A"), out=bad)
    fr = m.output_fields(SC.NAMES, array_type=torch.float64).cpu().numpy()
    fails, ratio = SC.compare(plain, *SC.spectrum_of_frames(fr))
    print(f"{form}: largest error / bound against the frame = {ratio:.4f}")
    assert not fails, fails[:8]
    for kind in ("ensemble", "channel"):
        e = _make(S, kind, form)
        e.time_steps(3, 0.002)
        all_m = e.zonal_spectra(order)
        assert tuple(all_m.shape) == (3, len(order), NX // 2 + 1)
        all_m = all_m.cpu().numpy()
        for k in range(3):
            assert SC.same_bits(all_m[k], e.member(k).zonal_spectra(order).cpu().numpy()), (kind, k)
        assert np.isfinite(all_m).all() and not SC.same_bits(all_m[0], all_m[1])
        fr = e.output_fields(order, array_type=torch.float64).cpu().numpy()
        assert not SC.compare(all_m, *SC.spectrum_of_frames(fr))[0], kind


@pytest.mark.parametrize("form", list(FORMS))
def test_parseval_across_features(swmhd, form):
    """sum_k P_u[k] is the row mean of zonal_means("uu"), and v / vv, B_x / B_xB_x, B_y / B_yB_y likewise, within the sum of the two
    bounds: both are statements about the same float64 frame."""
    S = swmhd
    m = _make(S, "single", form)
    m.time_steps(5, 0.002)
    first, second = ("u", "v", "B_x", "B_y"), ("uu", "vv", "B_xB_x", "B_yB_y")
    spec = m.zonal_spectra(first).cpu().numpy()
    prof = m.zonal_means(second).cpu().numpy()
    fr = m.output_fields(first, array_type=torch.float64).cpu().numpy()
    _, sbound = SC.spectrum_of_frames(fr)
    zwant, zsumabs = ZC.means_of_terms(fr * fr)
    zbound = ZC.bound(NX, zsumabs, zwant)
    for k, n in enumerate(first):
        lhs, rhs = spec[k].astype(LD).sum(), prof[k].astype(LD).sum() / LD(NY)
        tol = sbound[k].sum() + LD(zbound[k].astype(LD).sum()) / LD(NY)
        print(f"{form} {n}: sum_k P = {float(lhs):.17g}, mean of {second[k]} = {float(rhs):.17g}, |difference| / bound = {float(abs(lhs - rhs) / tol):.4f}")
        assert lhs > 0 and abs(lhs - rhs) <= tol, n


def test_refusals_of_the_host_mirror(swmhd):
    S = swmhd
    E = S._lib.SwmhdError
    m = S.ShallowWaterModel(S.RectilinearGrid(size=(32, 24), x=(-5, 5), y=(-5, 5)), 9.81, 1.0, tracers=("c",))
    for names in (("u", "c"), ("w",), ("uu",), ()):
        with pytest.raises(E):
            m.zonal_spectra(names)
        with pytest.raises(E):
            S.ZonalSpectrumTimeSeries(m, names, capacity=2)
    with pytest.raises(E):
        S.ZonalSpectrumTimeSeries(m, ("u",))                               # no capacity
    for size, topo in (((32, 24), ("Bounded", "Periodic", "Flat")), ((48, 24), ("Periodic", "Periodic", "Flat"))):
        b = S.ShallowWaterModel(S.RectilinearGrid(size=size, x=(-5, 5), y=(-5, 5), topology=topo), 9.81, 1.0)
        with pytest.raises(E):
            b.zonal_spectra(("u",))
        assert getattr(b, "_spectra_ws", None) is None                     # refused before anything was allocated
    # the C call answers an unsupported size itself, and writes nothing
    c = SC.Case(48, 3, 3, 4, False, None, 1, SC.F64, SC.ALL, 0)
    q = _upload(ZC._parents(48, 3, 3, 4, 54, SC.F64, 0, 3, 0))
    out = torch.full((7 * 25 + 64,), SENT, dtype=torch.float64, device="cuda")
    ws = torch.full((4096,), SENT, dtype=torch.float64, device="cuda")
    rc = S._lib.lib().swmhd_zonal_spectra_f64(*[t.data_ptr() for t in q], 48, 3, 3, 4, 54, SC.DX, SC.DY, 1, 0, 3, SC.ALL, ws.data_ptr(), out.data_ptr(), 25, 0,
                                              S.fields._stream_ptr())
    torch.cuda.synchronize()
    assert rc == 3 and (out == SENT).all() and (ws == SENT).all() and c.Nx == 48


def test_example_writes_zonal_spectra(tmp_path):
    """examples/run_swmhd.py --zonal-spectra: the last sample of a 32^2 run of five steps equals a recomputation from the fields the run
    dumped at that iteration (periodic: the ring of halo cells is the periodic image); the ensemble mode writes (samples, members, ...);
    without the flag no file is written."""
    H = 3
    out = tmp_path / "o"
    exe = [sys.executable, os.path.join(ROOT, "examples", "run_swmhd.py"), "--size", "32", "--stop-time", "0.05", "--every", "5", "--out", str(out)]
    r = subprocess.run(exe + ["--zonal-spectra", "0.01", "--dump-every", "0.05", "--ic", "gaussians"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out / "zonal_spectra.npz")
    names = ["u", "v", "A"]
    assert list(z["names"]) == names and z["spectra"].shape == (6, 3, 17) and z["spectra"].dtype == np.float64
    assert list(z["iterations"]) == list(range(6)) and np.allclose(z["times"], np.arange(6) * 0.01, rtol=0, atol=1e-12)
    assert z["k"].dtype.kind == "i" and list(z["k"]) == list(range(17)) and np.allclose(z["kx"], 2 * np.pi * np.arange(17) / 10.0, rtol=1e-15, atol=0)
    final = np.load(out / "fields_0000005.npz")
    q = [final[n] for n in ("u", "v", "h", "A")]
    which = sum(SC.BITS[n] for n in names)
    want, bound = SC.reference(q, 32, 32, H, H, 10 / 32, 10 / 32, 1, (0, 32), which, SC.WRAP_X | SC.WRAP_Y)
    fails, ratio = SC.compare(z["spectra"][-1], want, bound)
    print(f"example: largest error / bound = {ratio:.4f}")
    assert not fails, fails[:8]
    assert z["spectra"][-1, 0, 1:].max() > 0 and not os.path.exists(out / "frames.npz") and not os.path.exists(out / "zonal_means.npz")
    r = subprocess.run(exe + ["--zonal-spectra", "0.01", "--spectra-names", "A,s,B_x", "--amps", "0.1,0.5", "--formulation", "divergence"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out / "zonal_spectra.npz")
    assert list(z["names"]) == ["A", "s", "B_x"] and z["spectra"].shape == (6, 2, 3, 17) and np.isfinite(z["spectra"]).all()
    os.remove(out / "zonal_spectra.npz")
    r = subprocess.run(exe, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not os.path.exists(out / "zonal_spectra.npz")
