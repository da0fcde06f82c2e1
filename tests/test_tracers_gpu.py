"""GPU tests of the passive tracers: the stage kernel through the ABI (swmhd_tracers_rk3_*, k_tracers_tile) and
ShallowWaterModel(tracers=...).

The kernel's tile is TX x TY = 64 x 16 cells (launch_plan.hpp TRACER_TILE_X / _Y, mirrored in tracer_cases.TX / TY); the stage matrix runs
Nx in {3, 7, TX - 1, TX, TX + 1, 2 TX + 1} against Ny in {3, 9, TY - 1, TY, TY + 1} on a diagonal plus corners.

References: tracer_cases (the oracle's tendency of a centre field in the A slot, numpy's update; pinned on the CPU by
test_tracer_cases_cpu.py).  Strict results are compared bitwise.  Fast tendencies are held to the project's tolerance for A
(include/swmhd.h): max|dG| <= tol max(max|G|, S), S = (|u|/dx + |v|/dy) max|c| = helpers.term_scales with c in the A slot,
tol = 1e-13 (fp64, smooth fields), 1e-12 (fp64, rough random fields), 1e-4 (fp32)."""
import ctypes

import numpy as np
import pytest
import torch

import helpers as Hh
import tracer_cases as TC
from host_call_cases import _Recorder

pytestmark = pytest.mark.gpu
H = TC.H
PAD = 5                      # stride_y = Nx + 2 H + PAD
NPDT = {"f64": np.float64, "f32": np.float32}
COEF = dict(dt=0.013, gamma=0.37, zeta=-0.21)      # no RK3 identity that could hide a wrong operand


def dev(a):
    """A pitched device copy of parent a: (tensor of shape (rows, cols + PAD), pad columns = sentinel)."""
    full = np.full((a.shape[0], a.shape[1] + PAD), TC.SENTINEL, dtype=a.dtype)
    full[:, :a.shape[1]] = a
    return torch.from_numpy(full).cuda()


def sentinel_like(a):
    return torch.full((a.shape[0], a.shape[1] + PAD), TC.SENTINEL, dtype=torch.from_numpy(a[:1, :1]).dtype, device="cuda")


def expected(ref, Nx, Ny, rows, dtype):
    """The whole pitched output buffer: the sentinel everywhere but the interior of rows [j0, j1), which holds ref."""
    j0, j1 = rows
    out = np.full((Ny + 2 * H, Nx + 2 * H + PAD), TC.SENTINEL, dtype=dtype)
    if ref is not None:
        out[H + j0:H + j1, H:H + Nx] = Hh.interior(ref, Nx, Ny, H, H)[j0:j1]
    return out


def P(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def launch(L, sfx, q, c, cnew, Gn, Gm, Nx, Ny, dx, dy, form, store, rows, flags, dt, gamma, zeta):
    f = getattr(L.lib(), f"swmhd_tracers_rk3_{sfx}")
    rc = f(q[0].data_ptr(), q[1].data_ptr(), q[2].data_ptr(), P(c), P(cnew) if cnew is not None else None, P(Gn),
           P(Gm) if Gm is not None else None, len(c), Nx, Ny, H, H, Nx + 2 * H + PAD, dx, dy, form, dt, gamma, zeta, store,
           rows[0], rows[1], flags, None)
    L.check(rc, "swmhd_tracers_rk3")


class StageInputs:
    """State, 8 tracers and 8 G- operands of one (shape, formulation, precision), with the oracle's tendencies of the tracers."""

    def __init__(self, O, Nx, Ny, form, sfx, rough=True, K=8):
        dt = NPDT[sfx]
        self.Nx, self.Ny, self.form, self.sfx = Nx, Ny, form, sfx
        seed = 1000 * Nx + Ny
        self.q = [Hh.fill_halo_periodic(a, Nx, Ny, H, H) for a in TC.state(Nx, Ny, form, seed, dt, rough)]
        self.c = [Hh.fill_halo_periodic(a, Nx, Ny, H, H) for a in TC.tracer_fields(Nx, Ny, K, seed, dt, rough)]
        self.Gm = []
        for k in range(K):
            a = np.full(self.q[0].shape, TC.SENTINEL, dtype=dt)
            Hh.interior(a, Nx, Ny, H, H)[...] = np.random.default_rng([seed, 200 + k]).standard_normal((Ny, Nx))
            self.Gm.append(a)
        self.dx, self.dy = float(dt(TC.DX)), float(dt(TC.DY))      # as the call receives them
        self.G = [TC.tracer_tendency(O, self.q, c, Nx, Ny, self.dx, self.dy, form) for c in self.c]


# ----------------------------------------------------------------------------------------------------------------------------------
# stage matrix, strict: bitwise
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("form", [1, 0])
@pytest.mark.parametrize("Nx,Ny", TC.STAGE_SHAPES)
def test_strict_stage_matrix(swmhd, oracle, Nx, Ny, form, sfx):
    """Every stage form (first stage, classic stage with G-, the latter without the G store, tendencies only) for K = 1, 3, 8, once
    with SWMHD_WRAP_X | SWMHD_WRAP_Y and NaN in every halo of q1, q2, h and c, once with filled halos and no wrap, over all rows and
    over rows [2, Ny - 3): cnew and Gn bitwise the reference, and every other element of their pitched parents (halos, the rows
    outside the range, the pad columns) still the sentinel."""
    L = swmhd._lib
    d = StageInputs(oracle, Nx, Ny, form, sfx)
    t = NPDT[sfx]
    first = [TC.substep(c, g, None, Nx, Ny, COEF["dt"], COEF["gamma"], COEF["zeta"], True) for c, g in zip(d.c, d.G)]
    classic = [TC.substep(c, g, m, Nx, Ny, COEF["dt"], COEF["gamma"], COEF["zeta"], False) for c, g, m in zip(d.c, d.G, d.Gm)]
    Gm_d = [dev(a) for a in d.Gm]
    row_ranges = [(0, Ny)] + ([(2, Ny - 3)] if Ny - 3 > 2 else [])
    for wrap in (True, False):
        poison = (lambda a: Hh.poison_halo(a.copy(), Nx, Ny, H, H)) if wrap else (lambda a: a)
        q_d, c_d = [dev(poison(a)) for a in d.q], [dev(poison(a)) for a in d.c]
        flags = L.STRICT | ((L.WRAP_X | L.WRAP_Y) if wrap else 0)
        for K in (1, 3, 8):
            for rows in row_ranges:
                for what, store in (("first", 1), ("classic", 1), ("classic", 0), ("tend", 1)):
                    cnew = [sentinel_like(d.c[0]) for _ in range(K)] if what != "tend" else None
                    Gn = [sentinel_like(d.c[0]) for _ in range(K)]
                    launch(L, sfx, q_d, c_d[:K], cnew, Gn, Gm_d[:K] if what == "classic" else None, Nx, Ny, d.dx, d.dy, form, store, rows,
                           flags, **COEF)
                    torch.cuda.synchronize()
                    tag = (what, store, K, rows, wrap)
                    for k in range(K):
                        assert np.array_equal(Gn[k].cpu().numpy(), expected(d.G[k] if store else None, Nx, Ny, rows, t)), ("Gn", k) + tag
                        if cnew is not None:
                            ref = first[k] if what == "first" else classic[k]
                            assert np.array_equal(cnew[k].cpu().numpy(), expected(ref, Nx, Ny, rows, t)), ("cnew", k) + tag


# ----------------------------------------------------------------------------------------------------------------------------------
# isolation of the tracers of one launch, and the barrier between them
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("form", [1, 0])
def test_tracers_of_one_launch_do_not_mix(swmhd, oracle, form, strict):
    """K = 8 on a grid of 2 x 2 tiles (TX + 1, TY + 1): a NaN in the interior of tracer 3 leaves the other seven bitwise what they are
    without it and reaches tracer 3 only along the stencil (3 cells either way in x and in y, periodic); the same launch run twice
    gives identical bits.  The tracer tile in LDS is reused from one tracer to the next: a missing barrier shows here."""
    L = swmhd._lib
    Nx, Ny = TC.TX + 1, TC.TY + 1
    d = StageInputs(oracle, Nx, Ny, form, "f64")
    i0, j0 = TC.TX - 1, TC.TY            # next to a tile corner
    flags = (L.STRICT if strict else 0) | L.WRAP_X | L.WRAP_Y
    q_d = [dev(a) for a in d.q]
    Gm_d = [dev(a) for a in d.Gm]

    def run(cs):
        c_d = [dev(a) for a in cs]
        cnew, Gn = [sentinel_like(cs[0]) for _ in cs], [sentinel_like(cs[0]) for _ in cs]
        launch(L, "f64", q_d, c_d, cnew, Gn, Gm_d, Nx, Ny, d.dx, d.dy, form, 1, (0, Ny), flags, **COEF)
        torch.cuda.synchronize()
        return [x.cpu().numpy() for x in cnew + Gn]
    clean = run(d.c)
    bad = [a.copy() for a in d.c]
    bad[3][H + j0, H + i0] = np.nan
    out1, out2 = run(bad), run(bad)
    for a, b in zip(out1, out2):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    reach = np.zeros((Ny, Nx), bool)
    for s in range(-3, 4):
        reach[j0, (i0 + s) % Nx] = True
        reach[(j0 + s) % Ny, i0] = True
    for k in range(16):
        a, b = Hh.interior(out1[k][:, :Nx + 2 * H], Nx, Ny, H, H), Hh.interior(clean[k][:, :Nx + 2 * H], Nx, Ny, H, H)
        if k % 8 != 3:
            assert np.array_equal(out1[k], clean[k]), k
        else:
            assert np.isnan(a[j0, i0]) and not np.isnan(a[~reach]).any()
            assert np.array_equal(a[~reach], b[~reach])


# ----------------------------------------------------------------------------------------------------------------------------------
# fast stage against strict
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx,rough", [("f64", False), ("f64", True), ("f32", True), ("f32", False)])
@pytest.mark.parametrize("form", [1, 0])
@pytest.mark.parametrize("Nx,Ny", TC.STAGE_SHAPES + [(96, 96)])
def test_fast_tendencies_within_the_tolerance_of_A(swmhd, Nx, Ny, form, sfx, rough):
    L = swmhd._lib
    t = NPDT[sfx]
    seed = 1000 * Nx + Ny
    q = [Hh.fill_halo_periodic(a, Nx, Ny, H, H) for a in TC.state(Nx, Ny, form, seed, t, rough)]
    c = [Hh.fill_halo_periodic(a, Nx, Ny, H, H) for a in TC.tracer_fields(Nx, Ny, 3, seed, t, rough)]
    dx, dy = float(t(TC.DX)), float(t(TC.DY))
    q_d, c_d = [dev(a) for a in q], [dev(a) for a in c]
    G = {}
    for strict in (True, False):
        Gn = [sentinel_like(c[0]) for _ in c]
        launch(L, sfx, q_d, c_d, None, Gn, None, Nx, Ny, dx, dy, form, 1, (0, Ny), L.STRICT if strict else 0, **COEF)
        torch.cuda.synchronize()
        G[strict] = [Hh.interior(x.cpu().numpy()[:, :Nx + 2 * H], Nx, Ny, H, H).astype(np.float64) for x in Gn]
    tol = 1e-4 if sfx == "f32" else (1e-12 if rough else 1e-13)
    for k in range(3):
        S = Hh.term_scales(TC.FORM_NAME[form], [a.astype(np.float64) for a in q[:3]] + [c[k].astype(np.float64)], dx, dy, 0.0)[3]
        scale = max(np.abs(G[True][k]).max(), S)
        err = np.abs(G[False][k] - G[True][k]).max()
        print(f"tracer fast-vs-strict {sfx} form {form} {Nx}x{Ny} rough={rough} k={k}: {err / scale:.3e} of max(max|G|, S) (tol {tol:g})")
        assert np.isfinite(G[False][k]).all() and err <= tol * scale, (k, err / scale)


# ----------------------------------------------------------------------------------------------------------------------------------
# anchor form
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["VectorInvariant", "Conservative"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_anchor_tracer_stages_equal_classic_stages(swmhd, form, dtype):
    """Fast, periodic, 96^2, dt = 2e-3, the fields of test_rk3_anchor_gpu._model with c := A: anchored tracer stages against classic
    ones through the ABI, with the bounds that test applies to A -- 2 ulp of max|c| after stage 1, 8 ulp after the step, and nothing
    written through Gn by the anchored stages 2 and 3."""
    from test_rk3_anchor_gpu import _model, GAMMA, ZETA
    S, L = swmhd, swmhd._lib
    N, dt = 96, 2e-3
    m = _model(S, N, form, dtype)
    g = m.grid
    ft = getattr(L.lib(), f"swmhd_tendencies_rk3_{m.sfx}")
    tr = getattr(L.lib(), f"swmhd_tracers_rk3_{m.sfx}")
    mk = lambda n=4: [S.Field(g, dtype=dtype) for _ in range(n)]
    PP = lambda fl: L.ptr_array([x.ptr for x in fl])
    U0 = list(m.fields)
    fl = L.WRAP_X | L.WRAP_Y
    args = (g.Nx, g.Ny, g.Hx, g.Hy, U0[0].stride_y, g.dx, g.dy, 9.81, 1.0, m.form_code, m.lorentz_code)
    U1, U2, G0, G1 = mk(), mk(), mk(), mk()       # the states stages 2 and 3 start from
    L.check(ft(PP(U0), PP(U1), PP(G0), None, *args, dt, GAMMA[0], ZETA[0], 1, 0, g.Ny, fl, None), "state 1")
    L.check(ft(PP(U1), PP(U2), PP(G1), PP(G0), *args, dt, GAMMA[1], ZETA[1], 1, 0, g.Ny, fl, None), "state 2")
    targs = (1, g.Nx, g.Ny, g.Hx, g.Hy, U0[0].stride_y, g.dx, g.dy, m.form_code)

    def stage(U, c, cnew, Gn, Gm, gamma, zeta, store, flags):
        L.check(tr(U[0].ptr, U[1].ptr, U[2].ptr, PP(c), PP(cnew), PP(Gn), PP(Gm) if Gm else None, *targs, dt, gamma, zeta, store, 0, g.Ny,
                   flags, None), "tracer stage")
    c0 = [U0[3]]
    c1, c2, c3, g0, g1, gx = mk(1), mk(1), mk(1), mk(1), mk(1), mk(1)
    stage(U0, c0, c1, g0, None, GAMMA[0], ZETA[0], 1, fl)
    stage(U1, c1, c2, g1, g0, GAMMA[1], ZETA[1], 1, fl)
    stage(U2, c2, c3, gx, g1, GAMMA[2], ZETA[2], 0, fl)
    a1, a2, a3, W, junk = mk(1), mk(1), mk(1), mk(1), mk(1)
    fa = fl | L.RK3_ANCHOR
    stage(U0, c0, a1, W, None, GAMMA[0], 0.25, 0, fa)
    stage(U1, a1, a2, junk, W, GAMMA[1], 0.0, 0, fa)
    stage(U2, a2, a3, W, W, GAMMA[2], 0.0, 0, fa)          # Gn may alias Gm
    torch.cuda.synchronize()
    I = g.interior
    eps = float(np.finfo(np.float64 if dtype == torch.float64 else np.float32).eps)
    assert junk[0].data.abs().max().item() == 0
    for what, cs, as_, ulps in (("stage 1", c1, a1, 2), ("step", c3, a3, 8)):
        A_, B_ = cs[0].numpy()[I].astype(np.float64), as_[0].numpy()[I].astype(np.float64)
        scale, err = np.abs(A_).max(), np.abs(A_ - B_).max()
        print(f"anchored tracer {what} {form} {m.sfx}: {err / (eps * scale):.2f} ulp of max|c|")
        assert np.isfinite(B_).all() and err <= ulps * eps * scale, f"anchor {what} off by {err / (eps * scale):.2f} ulp of max|c|"


# ----------------------------------------------------------------------------------------------------------------------------------
# the model
# ----------------------------------------------------------------------------------------------------------------------------------
def _grid(S, Nx, Ny, topo):
    names = {TC.P: "Periodic", TC.B: "Bounded"}
    return S.RectilinearGrid(size=(Nx, Ny), x=(0, TC.DX * Nx), y=(0, TC.DY * Ny), topology=(names[topo[0]], names[topo[1]], "Flat"))


def _bcs(S, topo, names):
    if topo[1] != TC.B:
        return None
    bc = lambda: S.FieldBoundaryConditions(north=S.GradientBoundaryCondition(-0.05), south=S.GradientBoundaryCondition(-0.05))
    return {n: bc() for n in names}


def _setup(S, O, Nx, Ny, topo, form, strict=True, tracers=("c", "d"), dtype=torch.float64):
    """(model, q parents, d parent): rough random state, c := A with A's boundary conditions, d = tanh(y) + noise (no flux)."""
    g = _grid(S, Nx, Ny, topo)
    gradA = TC.grad_A(topo)
    q = TC.fill_state(O, TC.state(Nx, Ny, form, 11), Nx, Ny, topo, gradA, g.dx, g.dy)
    d = TC.fill(O, TC.tracer_fields(Nx, Ny, 2, 11)[1], Nx, Ny, topo, dx=g.dx, dy=g.dy)
    m = S.ShallowWaterModel(g, TC.GRAV, TC.FCOR, formulation=TC.FORM_NAME[form], strict=strict, dtype=dtype, tracers=tracers,
                            boundary_conditions=_bcs(S, topo, ("A", "c") if tracers else ("A",)))
    for f, a in zip(m.fields, q):
        f.data.copy_(torch.from_numpy(a))
    if tracers:
        m.tracers["c"].data.copy_(torch.from_numpy(q[3]))
        m.tracers["d"].data.copy_(torch.from_numpy(d))
    return m, q, d


def _check_model(m, ref, plain):
    m.synchronize()
    A = m.solution["A"].numpy()
    assert np.array_equal(m.tracers["c"].numpy(), A)                         # c := A stays A, halos included
    assert np.array_equal(m.tracers["d"].numpy(), ref.tr[1])
    assert np.array_equal(m.tracers["c"].numpy(), ref.tr[0])
    for f, w, a in zip(m.fields, plain.fields, ref.q):
        assert np.array_equal(f.numpy(), w.numpy()) and np.array_equal(f.numpy(), a)
    assert set(m.solution) == set(m.names) | {"c", "d"}


MODEL_GRIDS = [(20, 12, (TC.P, TC.P)), (13, 10, (TC.P, TC.B))]


@pytest.mark.parametrize("form,lor", TC.FORMS)
@pytest.mark.parametrize("Nx,Ny,topo", MODEL_GRIDS)
@pytest.mark.parametrize("how", ["eager", "graph", "checkpoint"])
def test_strict_model_with_tracers(swmhd, oracle, tmp_path, Nx, Ny, topo, form, lor, how):
    """Strict ShallowWaterModel(tracers=("c", "d")), 10 steps: c := A (with A's gradient condition on the Bounded grid) is bitwise A,
    d bitwise the reference, (q1, q2, h, A) bitwise a model built without tracers and the oracle -- stepped eagerly, through
    capture_graph + time_steps, and across a save_checkpoint / load_checkpoint in mid-run."""
    S, O = swmhd, oracle
    dt = 2e-3
    m, q, d = _setup(S, O, Nx, Ny, topo, form)
    plain, _, _ = _setup(S, O, Nx, Ny, topo, form, tracers=())
    gradA = TC.grad_A(topo)
    ref = TC.RefModel(O, q, [q[3], d], Nx, Ny, form, lor, topo, gradA, [gradA, None], m.grid.dx, m.grid.dy)
    for _ in range(10):
        ref.step(dt)
    plain.time_steps(10, dt)
    if how == "eager":
        for _ in range(10):
            m.time_step(dt)
    elif how == "graph":
        m.capture_graph(dt)
        m.time_steps(10, dt)
    else:
        m.time_steps(5, dt)
        path = str(tmp_path / "ck.npz")
        m.save_checkpoint(path)
        m, _, _ = _setup(S, O, Nx, Ny, topo, form)
        m.tracers["d"].data.zero_()
        m.load_checkpoint(path)
        assert m.iteration == 5
        m.time_steps(5, dt)
    _check_model(m, ref, plain)


@pytest.mark.parametrize("Nx,Ny", [(13, 10), (TC.TX + 1, TC.TY + 1)])
@pytest.mark.parametrize("topo", [(TC.P, TC.B), (TC.B, TC.P), (TC.B, TC.B)])
@pytest.mark.parametrize("form,lor", TC.FORMS)
def test_strict_bounded_tracers(swmhd, oracle, Nx, Ny, topo, form, lor):
    """Bounded topologies at 13 x 10 and at (TX + 1) x (TY + 1), strict, 3 steps of the model: wall orders of the tracer fluxes, the
    default (no-flux) condition on d and, where y is Bounded, the gradient condition on c -- bitwise the reference with `topo`."""
    S, O = swmhd, oracle
    dt = 2e-3
    m, q, d = _setup(S, O, Nx, Ny, topo, form)
    gradA = TC.grad_A(topo)
    ref = TC.RefModel(O, q, [q[3], d], Nx, Ny, form, lor, topo, gradA, [gradA, None], m.grid.dx, m.grid.dy)
    for _ in range(3):
        ref.step(dt)
        m.time_step(dt)
    m.synchronize()
    for f, a in zip(m.fields, ref.q):
        assert np.array_equal(f.numpy(), a)
    assert np.array_equal(m.tracers["c"].numpy(), ref.tr[0]) and np.array_equal(m.tracers["c"].numpy(), m.solution["A"].numpy())
    assert np.array_equal(m.tracers["d"].numpy(), ref.tr[1])


@pytest.mark.parametrize("form", ["VectorInvariant", "Conservative"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_fast_model_tracer_follows_A(swmhd, form, dtype):
    """Fast model, c := A, 10 steps at 96^2: with r = max|A_fast - A_strict| / max|A| measured on models WITHOUT tracers,
    max|c_fast - c_strict| / max|c| <= max(4 r, 8 eps): c and A go through different fast kernels that round the same quantity
    differently, hence the factor 4."""
    from test_rk3_anchor_gpu import _model
    S = swmhd
    N, dt = 96, 2e-3
    eps = float(np.finfo(np.float64 if dtype == torch.float64 else np.float32).eps)
    res = {}
    for strict in (True, False):
        for tr in ((), ("c",)):
            m = _model(S, N, form, dtype, strict=strict, tracers=tr)
            if tr:
                m.set(c=m.solution["A"].numpy())
            m.time_steps(10, dt)
            m.synchronize()
            I = m.grid.interior
            res[strict, bool(tr)] = (m.tracers["c"] if tr else m.solution["A"]).numpy()[I].astype(np.float64)
    A_s, A_f, c_s, c_f = res[True, False], res[False, False], res[True, True], res[False, True]
    assert np.array_equal(c_s, A_s)
    r = np.abs(A_f - A_s).max() / np.abs(A_s).max()
    ratio = np.abs(c_f - c_s).max() / np.abs(c_s).max()
    print(f"fast model tracer {form} {dtype}: r = {r:.3e}, tracer ratio = {ratio:.3e}, bound = {max(4 * r, 8 * eps):.3e}")
    assert np.isfinite(c_f).all() and ratio <= max(4 * r, 8 * eps), (ratio, r)


# ----------------------------------------------------------------------------------------------------------------------------------
# a model without tracers is what it was
# ----------------------------------------------------------------------------------------------------------------------------------
def test_launches_with_and_without_tracers(swmhd):
    S = swmhd
    for topo, fill in (((TC.P, TC.P), []), ((TC.P, TC.B), ["swmhd_fill_halo_f64"])):
        g = _grid(S, 20, 12, topo)
        m = S.ShallowWaterModel(g, tracers=())
        assert m._tr == {} and m._tr_alt == {} and m._tGn == [] and m._tGm == [] and m.tracer_names == ()
        log = []
        m._L = _Recorder(m._L, log)
        m.time_step(1e-3)
        assert log == (["swmhd_tendencies_rk3_f64"] + fill) * 3, log
        del log[:]
        m.time_steps(2, 1e-3)
        assert log == (["swmhd_step_rk3_f64"] if not fill else (["swmhd_tendencies_rk3_f64"] + fill) * 6), log
        m.synchronize()
        # with tracers: one more launch per stage (and one more fill of up to four tracers where halos are filled)
        mt = S.ShallowWaterModel(g, tracers=("c", "d", "e", "f", "g"))
        log = []
        mt._L = _Recorder(mt._L, log)
        mt.time_step(1e-3)
        assert log == (["swmhd_tendencies_rk3_f64", "swmhd_tracers_rk3_f64"] + fill * 3) * 3, log
        mt.synchronize()
        # frames keep their fixed name list: a tracer name points at model.tracers
        with pytest.raises(S._lib.SwmhdError, match=r"model\.tracers\['c'\]"):
            mt.output_fields(("u", "c"))
        with pytest.raises(S._lib.SwmhdError, match=r"model\.tracers\['d'\]"):
            S.FieldTimeSeries(mt, names=("d",), capacity=2)


def test_example_runs_with_a_dye(tmp_path):
    """examples/run_swmhd.py --dye: the tracer's extrema in every progress line (WENO5 keeps tanh(y) within its initial range to a few
    percent), the tracer and its G- in the field dump; without the flag the progress line has no tracer columns."""
    import os, re, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "examples", "run_swmhd.py"), "--size", "64", "--stop-time", "0.4", "--every", "20",
           "--dump-every", "0.4", "--out", str(tmp_path)]
    r = subprocess.run(cmd + ["--dye"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("Time:")]
    assert len(lines) == 3
    for l in lines:
        lo, hi = (float(x) for x in re.search(r"min\(c\): (\S+), max\(c\): (\S+),", l).groups())
        assert -1.05 <= lo <= -0.95 and 0.95 <= hi <= 1.05
    z = np.load(os.path.join(str(tmp_path), "fields_0000040.npz"))
    assert z["tracer_c"].shape == z["A"].shape and "tracer_Gm_c" in z.files and np.isfinite(z["tracer_c"]).all()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "min(c)" not in r.stdout
