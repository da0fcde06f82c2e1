"""GPU tests of the zonal means (swmhd_zonal_means_*, ShallowWaterModel.zonal_means) and of their writer (ZonalMeanTimeSeries, run).

The yardstick is tests/zonal_cases.py (pinned on the CPU by tests/test_zonal_cases_cpu.py): per-cell terms in IEEE double, rows summed
exactly, divided in longdouble; the bound is D(Nx) 2^-53 sum|term| / Nx plus one rounding of the quotient, D read off the kernel's
summation tree.  What does not depend on the summation's rounding -- the same call twice, a row range, a member, WRAP against filled
halos, an order of names, f32 against widened f64 -- is compared BITWISE.  Every comparison prints its largest error / bound first."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import output_cases as OC
import plot_cases as P
import zonal_cases as ZC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, SENT = 16, -777.25
SFX = {np.dtype("f8"): "f64", np.dtype("f4"): "f32"}
TORCH = {np.dtype("f8"): torch.float64, np.dtype("f4"): torch.float32}


def _zm(S, dev, dtype, Nx, Ny, Hx, Hy, sy, form, rows, which, flags, members=None, stride_m=0, spacing=None):
    """swmhd_[ensemble_]zonal_means_* on the device tensors `dev` (q1, q2, h, A): profiles (popcount, rows) or (members, popcount, rows)
    as numpy.  `out` lies in a buffer of sentinels -- a guard in front and behind, 3 doubles after every profile, 2 after every member
    -- and every sentinel must survive the call."""
    j0, j1 = rows
    n, npf = j1 - j0, bin(which).count("1")
    osk, M = n + 3, members or 1
    osm = npf * osk + 2
    buf = torch.full((2 * GUARD + M * osm,), SENT, dtype=torch.float64, device="cuda")
    dx, dy = spacing or (ZC.DX, ZC.DY)
    sfx = SFX[np.dtype(dtype)]
    ptrs = [t.data_ptr() for t in dev]
    out = buf.data_ptr() + 8 * GUARD
    L = S._lib.lib()
    if members is None:
        rc = getattr(L, f"swmhd_zonal_means_{sfx}")(*ptrs, Nx, Ny, Hx, Hy, sy, dx, dy, form, j0, j1, which, out, osk, flags, S.fields._stream_ptr())
    else:
        rc = getattr(L, f"swmhd_ensemble_zonal_means_{sfx}")(*ptrs, members, stride_m, Nx, Ny, Hx, Hy, sy, dx, dy, form, j0, j1, which, out, osk,
                                                            osm, flags, S.fields._stream_ptr())
    S._lib.check(rc, "swmhd_zonal_means")
    b = buf.cpu().numpy()
    body = b[GUARD:GUARD + M * osm].reshape(M, osm)
    prof = body[:, :npf * osk].reshape(M, npf, osk)
    assert (b[:GUARD] == SENT).all() and (b[GUARD + M * osm:] == SENT).all() and (body[:, npf * osk:] == SENT).all(), "guard overwritten"
    assert (prof[:, :, n:] == SENT).all(), "sentinels behind a profile overwritten"
    got = prof[:, :, :n].copy()
    if n:
        assert not (got == SENT).any(), "a profile entry was not written"
    return got[0] if members is None else got


def _upload(parents):
    return [torch.from_numpy(np.array(a)).cuda() for a in parents]


def _case_call(S, c, parents=None, rows=None, which=None, flags=None, dtype=None, spacing=None):
    q = ZC.inputs(c) if parents is None else parents
    dtype = c.dtype if dtype is None else dtype
    return _zm(S, _upload(q), dtype, c.Nx, c.Ny, c.Hx, c.Hy, ZC.stride_y(c), c.form, ZC.rows_of(c) if rows is None else rows,
               c.which if which is None else which, c.wrap if flags is None else flags, spacing=spacing)


CASES = ZC.cases()


@pytest.mark.parametrize("c", CASES, ids=[ZC.case_id(c) for c in CASES])
def test_every_case_is_within_the_bound_and_repeats_bitwise(swmhd, c):
    got = _case_call(swmhd, c)
    want, sumabs = ZC.expected(c)
    fails, ratio = ZC.compare(got, want, sumabs, c.Nx)
    print(f"{ZC.case_id(c)}: D = {ZC.depth(c.Nx)}, largest error / bound = {ratio:.3f}")
    assert not fails, fails[:8]
    assert ZC.same_bits(_case_call(swmhd, c), got), "two runs of the same call differ"


@pytest.mark.parametrize("Nx,form,dtype", [(5, 1, ZC.F64), (65, 0, ZC.F64), (257, 0, ZC.F32), (513, 1, ZC.F64)])
def test_a_row_range_has_the_bits_of_the_full_call(swmhd, Nx, form, dtype):
    c = ZC.Case(Nx, 7, 3, 4, True, None, form, dtype, ZC.ALL, 0)
    full = _case_call(swmhd, c)
    for rows in ((2, 5), (0, 1), (6, 7), (1, 7)):
        assert ZC.same_bits(_case_call(swmhd, c, rows=rows), full[:, rows[0]:rows[1]]), rows
    for which in (ZC.SPARSE, ZC.BITS["uv"], ZC.BITS["u"] | ZC.BITS["v"] | ZC.BITS["A"]):      # ... and a mask those of the full mask
        idx = [k for k, n in enumerate(ZC.NAMES) if which & ZC.BITS[n]]
        assert ZC.same_bits(_case_call(swmhd, c, which=which, rows=(2, 5)), full[idx, 2:5]), which


ENS = ZC.ensemble_cases()


@pytest.mark.parametrize("e", ENS, ids=[ZC.ensemble_case_id(e) for e in ENS])
def test_ensemble_member_has_the_bits_of_the_single_call(swmhd, e):
    """Three members with data of their own, dense (stride_m = the parent) or pitched (a gap of NaN between them): every member within
    the bound of its reference and bitwise the single call on that member."""
    S = swmhd
    Nx, Ny, form, dtype, pitched, rows, which, wrap = e
    Hx, Hy, sy, B = ZC.ENS_HX, ZC.ENS_HY, Nx + 2 * ZC.ENS_HX, ZC.ENSEMBLE_MEMBERS
    r = (0, Ny) if rows is None else rows
    per = (Ny + 2 * Hy) * sy
    stride_m = per + (ZC.ENSEMBLE_GAP if pitched else 0)
    members = [ZC.ensemble_member_inputs(Nx, Ny, dtype, m, rows, wrap) for m in range(B)]
    dev = []
    for k in range(4):
        t = torch.full((B * stride_m,), float("nan"), dtype=TORCH[np.dtype(dtype)], device="cuda")
        for m in range(B):
            t[m * stride_m:m * stride_m + per] = torch.from_numpy(np.array(members[m][k])).reshape(-1)
        dev.append(t)
    got = _zm(S, dev, dtype, Nx, Ny, Hx, Hy, sy, form, r, which, wrap, members=B, stride_m=stride_m)
    dx, dy = ZC.spacing(dtype)
    worst = 0.0
    for m in range(B):
        want, sumabs = ZC.reference(members[m], Nx, Ny, Hx, Hy, dx, dy, form, r, which, wrap)
        fails, ratio = ZC.compare(got[m], want, sumabs, Nx)
        worst = max(worst, ratio)
        assert not fails, (m, fails[:8])
        single = _zm(S, _upload(members[m]), dtype, Nx, Ny, Hx, Hy, sy, form, r, which, wrap)
        assert ZC.same_bits(got[m], single), f"member {m} differs from the single call"
    print(f"{ZC.ensemble_case_id(e)}: largest error / bound = {worst:.3f}")
    assert not ZC.same_bits(got[0], got[1])


@pytest.mark.parametrize("Nx,Ny,form,dtype", [(3, 1, 1, ZC.F64), (3, 7, 0, ZC.F32), (65, 7, 0, ZC.F64), (257, 2, 1, ZC.F32), (513, 1, 0, ZC.F64)])
def test_wrap_on_nan_halos_has_the_bits_of_the_plain_call_on_filled_halos(swmhd, Nx, Ny, form, dtype):
    for wrap in (ZC.WRAP_X | ZC.WRAP_Y, ZC.WRAP_X, ZC.WRAP_Y):
        c = ZC.Case(Nx, Ny, 3, 4, False, None, form, dtype, ZC.ALL, wrap)
        filled = [a.astype(dtype) for a in ZC.wrap_ring(ZC.inputs(c), Nx, Ny, 3, 4, wrap)]
        plain = _case_call(swmhd, c, parents=filled, flags=0)
        assert np.isfinite(plain).all()
        assert ZC.same_bits(_case_call(swmhd, c), plain), wrap


@pytest.mark.parametrize("Nx,Ny,form", [(5, 2, 1), (65, 7, 0), (257, 7, 1), (513, 2, 0)])
def test_f32_entry_point_has_the_bits_of_f64_on_the_widened_parents(swmhd, Nx, Ny, form):
    c = ZC.Case(Nx, Ny, 3, 4, True, None, form, ZC.F32, ZC.ALL, 0)
    narrow = _case_call(swmhd, c)
    wide = _case_call(swmhd, c, parents=[a.astype(np.float64) for a in ZC.inputs(c)], dtype=ZC.F64, spacing=ZC.spacing(ZC.F32))
    assert np.isfinite(narrow).all() and ZC.same_bits(narrow, wide)


def _nan_rows(field, form, name, y, Ny):
    """Rows of profile `name` whose stencil touches a NaN placed in `field` (0 q1, 1 q2, 2 h, 3 A) at row y, spelled out from the
    definitions of include/swmhd_zonal.h (dy: the offsets of the rows of the parent a term of row j reads)."""
    cons = form == 0
    U = {0: {0}, 2: {0} if cons else set()}                          # U(j): q1(j), cons: h(j)
    V = {1: {0}, 2: {0, -1} if cons else set()}                      # V(j): q2(j), cons: h(j-1), h(j)
    Vxy = {1: {0, 1}, 2: {-1, 0, 1} if cons else set()}              # xy-average of V: V(j), V(j+1)
    BX = {3: {0, -1}, 2: {0, -1}}
    BXxy = {3: {-1, 0, 1}, 2: {-1, 0, 1}}
    BY = {3: {0}, 2: {0}}
    join = lambda *ds: {f: set().union(*[d.get(f, set()) for d in ds]) for f in range(4)}
    reads = {"u": U, "v": V, "h": {2: {0}}, "A": {3: {0}}, "s": join(U, Vxy), "B_x": BX, "B_y": BY, "uu": U, "vv": V, "uv": join(U, Vxy),
             "B_xB_x": BX, "B_yB_y": BY, "B_xB_y": join(BY, BXxy), "vA": join(V, {3: {0, -1}})}[name]
    return {y - d for d in reads.get(field, set()) if 0 <= y - d < Ny}


@pytest.mark.parametrize("form", [1, 0])
@pytest.mark.parametrize("field", [0, 1, 2, 3])
def test_one_nan_cell_poisons_exactly_its_stencil(swmhd, form, field):
    """A NaN in one cell of member 1 of three: NaN exactly in the profile entries whose stencil touches it; every other entry, and
    every other member, has the bits of the clean run."""
    S = swmhd
    Nx, Ny, Hx, Hy, B, bad, y, x = 65, 7, ZC.ENS_HX, ZC.ENS_HY, 3, 1, 3, 31
    sy = Nx + 2 * Hx
    per = (Ny + 2 * Hy) * sy
    members = [ZC.ensemble_member_inputs(Nx, Ny, ZC.F64, m, None, 0) for m in range(B)]

    def run(dirty):
        dev = []
        for k in range(4):
            t = torch.cat([torch.from_numpy(np.array(members[m][k])).reshape(-1) for m in range(B)]).cuda()
            if dirty and k == field:
                t[bad * per + (Hy + y) * sy + Hx + x] = float("nan")
            dev.append(t)
        return _zm(S, dev, ZC.F64, Nx, Ny, Hx, Hy, sy, form, (0, Ny), ZC.ALL, 0, members=B, stride_m=per)
    clean, dirty = run(False), run(True)
    assert np.isfinite(clean).all()
    want_nan = np.zeros(clean.shape, dtype=bool)
    for k, name in enumerate(ZC.NAMES):
        for j in _nan_rows(field, form, name, y, Ny):
            want_nan[bad, k, j] = True
    assert want_nan.any() and np.array_equal(np.isnan(dirty), want_nan), np.argwhere(np.isnan(dirty) != want_nan)[:10]
    assert ZC.same_bits(dirty[~want_nan], clean[~want_nan])
    # the restatement, run on the same dirty member, puts its NaN in the same places
    q = [np.array(a) for a in members[bad]]
    q[field][Hy + y, Hx + x] = np.nan
    ref = ZC.reference(q, Nx, Ny, Hx, Hy, ZC.DX, ZC.DY, form, (0, Ny), ZC.ALL)[0]
    assert np.array_equal(np.isnan(ref.astype(np.float64)), want_nan[bad])


# --- the host mirror ---------------------------------------------------------------------------------------------------------------
H = 3
FORMS = {"VectorInvariant": 1, "Conservative": 0}
FRAME = OC.NAMES
SECOND = ("uu", "vv", "uv", "B_xB_x", "B_yB_y", "B_xB_y", "vA")


def _vortex(m, amp=1.0):
    u0 = lambda X, Y: amp * Y * np.exp(-(X ** 2 + Y ** 2))
    v0 = lambda X, Y: -amp * X * np.exp(-(X ** 2 + Y ** 2))
    n1, n2 = m.names[:2]
    members = getattr(m, "members", None)
    if getattr(m, "_channel", False):
        A0 = [lambda X, Y, gr=gr: gr * Y for gr in m._grads]
    else:
        A0 = P.two_gaussians(0.1) if members is None else [P.two_gaussians(0.1 * (k + 1)) for k in range(members)]
    m.set(**{n1: u0, n2: v0, "h": lambda X, Y: 1.0 + 0.05 * np.exp(-(X ** 2 + Y ** 2)), "A": A0})
    return m


def _make(S, kind, form):
    Nx, Ny = 32, 24
    if kind == "channel":
        g = S.RectilinearGrid(size=(Nx, Ny), x=(-5, 5), y=(-5, 5), topology=("Periodic", "Bounded", "Flat"))
        grads = [-0.01, -0.05, 0.02]
        bcs = [{"A": S.FieldBoundaryConditions(north=S.GradientBoundaryCondition(gr), south=S.GradientBoundaryCondition(gr))} for gr in grads]
        m = S.BoundedShallowWaterEnsemble(g, 3, 9.81, 1.0, formulation=form, boundary_conditions=bcs)
        m._channel, m._grads = True, grads
        return _vortex(m)
    g = S.RectilinearGrid(size=(Nx, Ny), x=(-5, 5), y=(-5, 5))
    return _vortex(S.ShallowWaterEnsemble(g, 3, 9.81, 1.0, formulation=form) if kind == "ensemble" else S.ShallowWaterModel(g, 9.81, 1.0, formulation=form))


def _state(m):
    ts = m._state if getattr(m, "members", None) is not None else [f.data for f in m._raw_fields]
    return [t.cpu().numpy().copy() for t in ts]


def _terms_from_frames(fr, periodic_y):
    """The fourteen per-cell terms from a float64 frame (..., 7, Ny, Nx) of u v h A s B_x B_y, x periodic: the second moments as the
    header writes them, with roll for the neighbours.  Rows whose neighbour row is not in a frame (Bounded y: row -1 for vA, row Ny for
    uv and B_xB_y) are NaN."""
    u, v, h, A, s, bx, by = (fr[..., k, :, :] for k in range(7))
    west = lambda a: np.roll(a, 1, axis=-1)
    north = lambda a: np.roll(a, -1, axis=-2)
    south = lambda a: np.roll(a, 1, axis=-2)
    xy = lambda a: 0.5 * (0.5 * (west(a) + a) + 0.5 * (west(north(a)) + north(a)))
    uv, bb, va = u * xy(v), by * xy(bx), v * (0.5 * (south(A) + A))
    if not periodic_y:
        uv[..., -1, :], bb[..., -1, :], va[..., 0, :] = np.nan, np.nan, np.nan
    return np.stack([u, v, h, A, s, bx, by, u * u, v * v, uv, bx * bx, by * by, bb, va], axis=-3)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("kind", ["single", "ensemble", "channel"])
def test_writer_beside_the_frames_with_graph_replay(swmhd, kind, form):
    """32 x 24, ten steps through a captured graph with both writers attached: every stored profile is within the bound of the row
    means of the float64 frame stored at the same iteration; times and iterations agree; a continued run does not repeat the shared
    sample; the state is bitwise that of the same run without the zonal writer."""
    S = swmhd
    dt, names = 0.002, FRAME + SECOND
    m = _make(S, kind, form)
    m.capture_graph(dt)
    frames = S.FieldTimeSeries(m, names=FRAME, schedule=S.IterationInterval(2), capacity=8, array_type=torch.float64)
    zonal = S.ZonalMeanTimeSeries(m, names=names, schedule=S.IterationInterval(2), capacity=8)
    with pytest.raises(S._lib.SwmhdError):
        S.run(m, dt, stop_iteration=10, writers=[frames, S.ZonalMeanTimeSeries(m, names=names, schedule=S.IterationInterval(2), capacity=5)])
    assert m.iteration == 0 and len(zonal) == 0
    S.run(m, dt, stop_iteration=6, writers=[frames, zonal])
    S.run(m, dt, stop_iteration=10, writers=[frames, zonal])           # continued: iteration 6 is in both series already
    assert zonal.iterations == [0, 2, 4, 6, 8, 10] == frames.iterations and zonal.times == frames.times and len(zonal) == 6
    assert np.allclose(zonal.times, np.arange(6) * 2 * dt, rtol=0, atol=1e-12)
    lead = () if kind == "single" else (3,)
    prof, fr = zonal.numpy(), frames.numpy()
    assert prof.dtype == np.float64 and prof.shape == (6,) + lead + (14, 24) and tuple(zonal.profiles.shape) == (8,) + lead + (14, 24)
    terms = _terms_from_frames(fr, periodic_y=kind != "channel")
    want, sumabs = ZC.means_of_terms(terms)
    known = np.isfinite(want.astype(np.float64))
    assert np.isfinite(prof).all() and known.sum() >= prof.size - 6 * 3 * 3
    fails, ratio = ZC.compare(np.where(known, prof, np.nan), want, sumabs, 32)
    print(f"{kind} {form}: largest error / bound = {ratio:.3f} (D = {ZC.depth(32)})")
    assert not fails, fails[:8]
    assert not np.array_equal(prof[0], prof[-1]) and np.abs(prof[:, ..., 9, :]).max() > 0
    # the same run without the zonal writer: the same state, bit for bit
    twin = _make(S, kind, form)
    twin.capture_graph(dt)
    only = S.FieldTimeSeries(twin, names=FRAME, schedule=S.IterationInterval(2), capacity=8, array_type=torch.float64)
    S.run(twin, dt, stop_iteration=6, writers=[only])
    S.run(twin, dt, stop_iteration=10, writers=[only])
    assert twin.iteration == m.iteration == 10
    for a, b in zip(_state(m), _state(twin)):
        assert np.array_equal(a, b, equal_nan=True)
    assert np.array_equal(only.numpy(), fr)
    with pytest.raises(S._lib.SwmhdError):
        for _ in range(3):
            zonal.write()                                              # 8 slots


@pytest.mark.parametrize("form", list(FORMS))
def test_any_order_and_repetition_of_names(swmhd, form):
    """zonal_means of the model against the C call on its parents; a permuted and repeated list has the bits of the plain one; the
    members of an ensemble those of member(m)."""
    S = swmhd
    m = _make(S, "single", form)
    m.time_steps(3, 0.002)
    plain = m.zonal_means(ZC.NAMES)
    assert plain.dtype == torch.float64 and tuple(plain.shape) == (14, 24) and plain.is_cuda
    plain = plain.cpu().numpy()
    order = ("vA", "u", "B_xB_y", "u", "s", "A", "uv", "h", "vv", "v", "B_x", "uu", "B_y", "B_yB_y", "B_xB_x", "vA")
    got = m.zonal_means(order).cpu().numpy()
    assert ZC.same_bits(got, plain[[ZC.NAMES.index(n) for n in order]])
    assert ZC.same_bits(m.zonal_means().cpu().numpy(), plain[[0, 1, 3]])           # the default: u v A
    out = torch.full((5, 2, 24), SENT, dtype=torch.float64, device="cuda")
    assert m.zonal_means(("uv", "A"), out=out[2]) is not None and ZC.same_bits(out[2].cpu().numpy(), plain[[9, 3]])
    assert (out[[0, 1, 3, 4]] == SENT).all()
    for bad in (torch.empty((2, 24), dtype=torch.float32, device="cuda"), torch.empty((2, 23), dtype=torch.float64, device="cuda"),
                torch.empty((2, 24), dtype=torch.float64)):
        with pytest.raises(S._lib.SwmhdError):
            m.zonal_means(("uv", "A"), out=bad)
    # the frame's row means are what the first moments are
    fr = m.output_fields(FRAME, array_type=torch.float64).cpu().numpy()
    fails, ratio = ZC.compare(plain[:7], *ZC.means_of_terms(fr), 32)
    assert not fails, fails[:8]
    for kind in ("ensemble", "channel"):
        e = _make(S, kind, form)
        e.time_steps(3, 0.002)
        all_m = e.zonal_means(order)
        assert tuple(all_m.shape) == (3, len(order), 24)
        all_m = all_m.cpu().numpy()
        for k in range(3):
            assert ZC.same_bits(all_m[k], e.member(k).zonal_means(order).cpu().numpy()), (kind, k)
        assert not ZC.same_bits(all_m[0], all_m[1])


@pytest.mark.parametrize("topo", [("Periodic", "Bounded"), ("Bounded", "Periodic")])
@pytest.mark.parametrize("form", list(FORMS))
def test_bounded_topologies_with_filled_halos(swmhd, topo, form):
    """After 10 steps of a 40 x 24 grid with one Bounded direction: the reference applied to model.fields, the halos of the Bounded
    direction as the boundary-condition fill left them, the periodic direction wrapped.  The far-wall line is not part of a mean: a
    (f,.) profile on the Bounded x direction averages faces 1..Nx, as the frame holds them."""
    S = swmhd
    from test_model_oracle import Lx, Ly, hf, uf, vf, Af
    Nx, Ny = 40, 24
    g = S.RectilinearGrid(size=(Nx, Ny), x=(0, Lx), y=(0, Ly), topology=(*topo, "Flat"))
    side = ("south", "north") if topo[1] == "Bounded" else ("west", "east")
    bcs = {"A": S.FieldBoundaryConditions(**{s: S.GradientBoundaryCondition(-0.05) for s in side})}
    m = S.ShallowWaterModel(g, 9.81, 1.0, formulation=form, boundary_conditions=bcs)
    A0 = (lambda X, Y: Af(X, Y) - 0.05 * Y) if topo[1] == "Bounded" else (lambda X, Y: Af(X, Y) - 0.05 * X)
    if form == "VectorInvariant":
        m.set(u=uf, v=vf, h=hf, A=A0)
    else:
        m.set(uh=lambda X, Y: hf(X, Y) * uf(X, Y), vh=lambda X, Y: hf(X, Y) * vf(X, Y), h=hf, A=A0)
    m.time_steps(10, 0.002)
    got = m.zonal_means(ZC.NAMES).cpu().numpy()
    q = [f.numpy() for f in m.fields]
    wrap = (ZC.WRAP_Y if topo[1] == "Periodic" else 0) | (ZC.WRAP_X if topo[0] == "Periodic" else 0)
    want, sumabs = ZC.reference(q, Nx, Ny, H, H, g.dx, g.dy, FORMS[form], (0, Ny), ZC.ALL, wrap)
    fails, ratio = ZC.compare(got, want, sumabs, Nx)
    print(f"{topo} {form}: largest error / bound = {ratio:.3f}")
    assert np.isfinite(got).all() and not fails, fails[:8]
    fr = m.output_fields(FRAME, array_type=torch.float64).cpu().numpy()
    assert not ZC.compare(got[:7], *ZC.means_of_terms(fr), Nx)[0]


def test_tracer_and_unknown_names_are_refused(swmhd):
    S = swmhd
    g = S.RectilinearGrid(size=(32, 24), x=(-5, 5), y=(-5, 5))
    m = S.ShallowWaterModel(g, 9.81, 1.0, tracers=("c",))
    for names in (("u", "c"), ("w",), ()):
        with pytest.raises(S._lib.SwmhdError):
            m.zonal_means(names)
        with pytest.raises(S._lib.SwmhdError):
            S.ZonalMeanTimeSeries(m, names, capacity=2)
    with pytest.raises(S._lib.SwmhdError):
        S.ZonalMeanTimeSeries(m, ("u",))                               # no capacity


def test_example_writes_zonal_means(tmp_path):
    """examples/run_swmhd.py --zonal-means: the last sample of a 32^2 run of five steps equals a recomputation from the fields the run
    dumped at that iteration (periodic: the ring of halo cells is the periodic image); the ensemble modes write (samples, members, ...)."""
    out = tmp_path / "o"
    exe = [sys.executable, os.path.join(ROOT, "examples", "run_swmhd.py"), "--size", "32", "--stop-time", "0.05", "--every", "5", "--out", str(out)]
    r = subprocess.run(exe + ["--zonal-means", "0.01", "--dump-every", "0.05", "--ic", "gaussians"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out / "zonal_means.npz")
    names = ["u", "v", "A", "uv", "B_xB_y", "vA"]
    assert list(z["names"]) == names and z["profiles"].shape == (6, 6, 32) and z["profiles"].dtype == np.float64
    assert list(z["iterations"]) == list(range(6)) and np.allclose(z["times"], np.arange(6) * 0.01, rtol=0, atol=1e-12)
    assert z["yc"].shape == (32,) and np.allclose(z["yf"], -5 + np.arange(32) * (10 / 32)) and np.allclose(z["yc"] - z["yf"], 5 / 32) and int(z["j_offset"]) == 0
    final = np.load(out / "fields_0000005.npz")
    q = [final[n] for n in ("u", "v", "h", "A")]
    which = sum(ZC.BITS[n] for n in names)
    assert ZC.names_of(which) == tuple(names)
    want, sumabs = ZC.reference(q, 32, 32, H, H, 10 / 32, 10 / 32, 1, (0, 32), which, ZC.WRAP_X | ZC.WRAP_Y)
    fails, ratio = ZC.compare(z["profiles"][-1], want, sumabs, 32)
    print(f"example: largest error / bound = {ratio:.3f}")
    assert not fails, fails[:8]
    assert np.abs(z["profiles"][-1, 3]).max() > 0
    assert not os.path.exists(out / "frames.npz")
    r = subprocess.run(exe + ["--zonal-means", "0.01", "--zonal-names", "A,vA,s", "--amps", "0.1,0.5", "--formulation", "divergence"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out / "zonal_means.npz")
    assert list(z["names"]) == ["A", "vA", "s"] and z["profiles"].shape == (6, 2, 3, 32) and np.isfinite(z["profiles"]).all()
    r = subprocess.run(exe + ["--zonal-means", "0.05", "--channel", "--gradients=-0.01,-0.05,-0.1"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out / "zonal_means.npz")
    assert z["profiles"].shape == (2, 3, 6, 32) and np.isfinite(z["profiles"]).all() and list(z["iterations"]) == [0, 5]
