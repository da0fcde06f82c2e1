"""GPU tests of the passive tracers of periodic ensembles: the stage kernel's ensemble instantiations through the ABI
(swmhd_ensemble_tracers_rk3_*, swmhd_ensemble_tracers_rk3_params_*) and ShallowWaterEnsemble(tracers=...).

Member shapes (ensemble_tracer_cases.SHAPES): (3, 3), (7, 9), (TX + 1, TY + 1), (2 TX + 1, 9) around the kernel's 64 x 16 tile.  Every
family of parents is one pitched buffer (stride_y = Nx + 2 H + 5, stride_m = (Ny + 2 H) stride_y + 37) that holds the sentinel in the pad
columns, in the gap after every member, in every halo of the inputs (the calls wrap) and everywhere in the outputs.

References: tracer_cases (the oracle's tendency of a centre field in the A slot, numpy's update, RefModel).  Strict results are compared
bitwise.  Fast tendencies are held to the project's tolerance for A (include/swmhd.h) in the norm of
test_tracers_gpu.test_fast_tendencies_within_the_tolerance_of_A: max|dG| <= tol max(max|G|, S), S = helpers.term_scales with c in the
A slot, tol = 1e-13 (fp64, smooth), 1e-12 (fp64, rough), 1e-4 (fp32).  The anchor form stores no G but c + w G with w = dt gamma or
dt (gamma1 + zeta2): there the bound is w times that of G plus the roundings of the update in the element type (the product w and the
final sum), 2 eps max(max|c|, max|c + w G|), against the same expression evaluated in float64 with the strict G."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ensemble_tracer_cases as EC
import helpers as Hh
import tracer_cases as TC
from host_call_cases import _Recorder

pytestmark = pytest.mark.gpu
H = TC.H
NPDT = EC.NPDT
COEF = EC.COEF
TOL = lambda sfx, rough: 1e-4 if sfx == "f32" else (1e-12 if rough else 1e-13)


def dev(flat):
    return torch.from_numpy(flat).cuda()


def sentinel(d, members):
    sy, sm = EC.layout(d.Nx, d.Ny)
    return torch.full((members * sm,), TC.SENTINEL, dtype=torch.float64 if d.sfx == "f64" else torch.float32, device="cuda")


def P(ts, offset=0):
    """Host array of the device pointers of member `offset / stride_m` of each flat tensor."""
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() + offset * t.element_size() for t in ts])


def launch(L, d, q, c, cnew, Gn, Gm, members, store, flags, dt=None, gamma=None, zeta=None, params=None, member0=0):
    """swmhd_ensemble_tracers_rk3 (params None) or _params on `members` members starting at member0 of the flat tensors."""
    sy, sm = EC.layout(d.Nx, d.Ny)
    o = member0 * sm
    f = getattr(L.lib(), f"swmhd_ensemble_tracers_rk3_{'params_' if params is not None else ''}{d.sfx}")
    rc = f(P(q, o)[0], P(q, o)[1], P(q, o)[2], P(c, o), P(cnew, o) if cnew is not None else None, P(Gn, o), P(Gm, o) if Gm is not None else None,
           len(c), members, sm, d.Nx, d.Ny, H, H, sy, d.dx, d.dy, d.form, params.data_ptr() if params is not None else dt, gamma, zeta,
           store, flags, None)
    L.check(rc, "swmhd_ensemble_tracers_rk3")


def inputs_on_device(d, members, K, halos=False, poison=None):
    """(q, c, Gm) flat device tensors of the first `members` members; poison: a member whose every input is NaN."""
    def fam(what, k=None):
        flat = d.family(what, k, members, halos)
        if poison is not None:
            sy, sm = EC.layout(d.Nx, d.Ny)
            flat[poison * sm:(poison + 1) * sm] = np.nan
        return dev(flat)
    return [fam(f) for f in range(3)], [fam("c", k) for k in range(K)], [fam("Gm", k) for k in range(K)]


# ----------------------------------------------------------------------------------------------------------------------------------
# stage matrix, strict: bitwise
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("form", [1, 0])
@pytest.mark.parametrize("Nx,Ny", EC.SHAPES)
def test_strict_stage_matrix(swmhd, oracle, Nx, Ny, form, sfx):
    """members in {1, 3} x K in {1, 3, 8} x {first stage, later stage with G-, tendencies only}, distinct data in every member and
    tracer, SWMHD_WRAP_X | _Y with the sentinel in every input halo: the whole pitched buffer of every cnew[k] and Gn[k] is bitwise the
    sentinel with the oracle's result (tracer in A's place) in every member's interior.  A missing m * stride_m on q1, q2, h, c, cnew,
    Gn or Gm, or a wrong member-to-block mapping, fails here."""
    L = swmhd._lib
    d = EC.stage_inputs(oracle, Nx, Ny, form, sfx)
    t = NPDT[sfx]
    M, K8 = EC.MEMBERS, EC.KMAX
    first = [[TC.substep(d.c[m][k], d.G[m][k], None, Nx, Ny, COEF["dt"], COEF["gamma"], COEF["zeta"], True) for k in range(K8)] for m in range(M)]
    later = [[TC.substep(d.c[m][k], d.G[m][k], d.Gm[m][k], Nx, Ny, COEF["dt"], COEF["gamma"], COEF["zeta"], False) for k in range(K8)] for m in range(M)]
    flags = L.STRICT | L.WRAP_X | L.WRAP_Y
    for members in (1, 3):
        q_d, c_d, Gm_d = inputs_on_device(d, members, K8)
        for K in (1, 3, 8):
            for what in ("first", "later", "tend"):
                cnew = [sentinel(d, members) for _ in range(K)] if what != "tend" else None
                Gn = [sentinel(d, members) for _ in range(K)]
                launch(L, d, q_d, c_d[:K], cnew, Gn, Gm_d[:K] if what == "later" else None, members, 1, flags, **COEF)
                torch.cuda.synchronize()
                for k in range(K):
                    tag = (what, members, K, k)
                    assert np.array_equal(Gn[k].cpu().numpy(), EC.pack([d.G[m][k] for m in range(members)], Nx, Ny, t)), ("Gn",) + tag
                    if cnew is not None:
                        ref = first if what == "first" else later
                        assert np.array_equal(cnew[k].cpu().numpy(), EC.pack([ref[m][k] for m in range(members)], Nx, Ny, t)), ("cnew",) + tag


# ----------------------------------------------------------------------------------------------------------------------------------
# per-member dt
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("form", [1, 0])
@pytest.mark.parametrize("Nx,Ny", [(7, 9), (TC.TX + 1, TC.TY + 1)])
def test_strict_params_equal_scalar_calls(swmhd, oracle, Nx, Ny, form, sfx):
    """Three members with three different dt: the strict _params call is bitwise the scalar call made per member (one member, that
    member's dt), in the first-stage and in the later-stage form; with all rows of the table equal it is bitwise the scalar call on all
    three.  g and f of the table are NaN: a tracer's tendency reads neither."""
    L = swmhd._lib
    d = EC.stage_inputs(oracle, Nx, Ny, form, sfx)
    t = NPDT[sfx]
    M, K = EC.MEMBERS, 3
    flags = L.STRICT | L.WRAP_X | L.WRAP_Y
    q_d, c_d, Gm_d = inputs_on_device(d, M, K)
    table = lambda dts: torch.from_numpy(np.stack([np.full(M, np.nan), np.full(M, np.nan), np.asarray(dts)], axis=1).astype(t)).cuda()
    for gm in (None, Gm_d):
        def run(**kw):
            cnew, Gn = [sentinel(d, M) for _ in range(K)], [sentinel(d, M) for _ in range(K)]
            if kw.get("per_member"):
                for m in range(M):
                    launch(L, d, q_d, c_d, cnew, Gn, gm, 1, 1, flags, dt=float(t(EC.DTS[m])), gamma=COEF["gamma"], zeta=COEF["zeta"], member0=m)
            else:
                launch(L, d, q_d, c_d, cnew, Gn, gm, M, 1, flags, gamma=COEF["gamma"], zeta=COEF["zeta"], **{k: v for k, v in kw.items()})
            torch.cuda.synchronize()
            return [x.cpu().numpy() for x in cnew + Gn]
        for a, b in zip(run(params=table(EC.DTS)), run(per_member=True)):
            assert np.array_equal(a, b)
        # the update did use the member's dt: the oracle's tendency, numpy's update
        out = run(params=table(EC.DTS))
        for k in range(K):
            ref = [TC.substep(d.c[m][k], d.G[m][k], d.Gm[m][k] if gm else None, Nx, Ny, EC.DTS[m], COEF["gamma"], COEF["zeta"], gm is None) for m in range(M)]
            assert np.array_equal(out[k], EC.pack(ref, Nx, Ny, t)), k
        for a, b in zip(run(params=table([COEF["dt"]] * M)), run(dt=float(t(COEF["dt"])))):
            assert np.array_equal(a, b)


def _fast_bounds(d, m, k, sfx, rough):
    """(tol, scale) of tracer k of member m: the tolerance of A and max(max|G|, S) of test_fast_tendencies_within_the_tolerance_of_A."""
    q64 = [a.astype(np.float64) for a in d.q[m][:3]] + [d.c[m][k].astype(np.float64)]
    S = Hh.term_scales(TC.FORM_NAME[d.form], q64, d.dx, d.dy, 0.0)[3]
    return TOL(sfx, rough), S


def _members_interior(flat, d, members):
    sy, sm = EC.layout(d.Nx, d.Ny)
    return [Hh.interior(flat[m * sm:m * sm + (d.Ny + 2 * H) * sy].reshape(d.Ny + 2 * H, sy)[:, :d.Nx + 2 * H], d.Nx, d.Ny, H, H).astype(np.float64)
            for m in range(members)]


def _check_anchor(out, ref_terms, w, tol_scale, eps, tag):
    """out = base + w G (fast, element type) against base + w G_strict in float64: w tol max(max|G|, S) + 2 eps max(|base|, |result|)
    (|w G| <= 2 max(|base|, |result|): half an ulp of the product w is at most eps of that maximum, the final sum's half an ulp less)."""
    base, G = ref_terms
    ref = base + w * G
    err = np.abs(out - ref).max()
    bound = w * tol_scale + 2 * eps * max(np.abs(ref).max(), np.abs(base).max())
    print(f"anchor {tag}: err {err:.3e}, bound {bound:.3e}")
    assert np.isfinite(out).all() and err <= bound, (tag, err, bound)


def _check_update(out, c, G, Gm, dt, t, tol_scale, tag):
    """out = c + dt (gamma G + zeta Gm) (Gm None: c + dt gamma G) of a fast classic stage with COEF's gamma and zeta against the same
    expression in longdouble with the strict G and the coefficients as the kernel receives them.  Bound: that of the single-grid stage
    matrix (stage_cases.stage_bounds): dt weight (tendency bound) + 4 eps max|addends and result|, weight = |gamma| + |zeta| with Gm,
    |gamma| without."""
    LD = np.longdouble
    eps = float(np.finfo(t).eps)
    gam, zet, dtl = LD(t(COEF["gamma"])), LD(t(COEF["zeta"])), LD(t(dt))
    ga, za, dta = abs(float(gam)), abs(float(zet)), float(dtl)
    amax = lambda a: float(np.abs(a).max())
    terms = [dta * ga * amax(G), amax(c)]
    if Gm is None:
        ref, weight = c.astype(LD) + dtl * gam * G.astype(LD), ga
    else:
        ref, weight = c.astype(LD) + dtl * (gam * G.astype(LD) + zet * Gm.astype(LD)), ga + za
        terms.append(dta * za * amax(Gm))
    err = float(np.abs(out.astype(LD) - ref).max())
    bound = dta * weight * tol_scale + 4 * eps * max(terms + [amax(ref)])
    print(f"update {tag}: err {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3g}")
    assert np.isfinite(out).all() and err <= bound, (tag, err, bound)


@pytest.mark.parametrize("sfx,rough", [("f64", False), ("f64", True), ("f32", True), ("f32", False)])
@pytest.mark.parametrize("form", [1, 0])
@pytest.mark.parametrize("Nx,Ny", EC.SHAPES + [(96, 96)])
def test_fast_stages_within_the_tolerance_of_A(swmhd, oracle, Nx, Ny, form, sfx, rough):
    """Fast ensemble stages, 2 members x 3 tracers, with a scalar dt and with the table (two different dt): the classic stage's stored
    Gn against the strict ensemble launch in the norm and with the bound of the single-grid test; the anchored stages' outputs
    (cnew and W of the first, cnew of a later one) with that bound carried through the update (module docstring).  The classic
    stages' new state: cnew of the G- stage, and cnew of the first stage (Gm == NULL; store_G 1 and 0, the latter leaving Gn alone) with
    the scalar dt and with the table, per member and tracer within the G--stage | first-stage bound of the single-grid stage matrix
    (_check_update) with the strict tendency as G and the member's dt."""
    L = swmhd._lib
    M, K = 2, 3
    d = EC.StageInputs(oracle, Nx, Ny, form, sfx, rough, members=M, K=K, reference=False)
    t = NPDT[sfx]
    eps = float(np.finfo(t).eps)
    wrap = L.WRAP_X | L.WRAP_Y
    q_d, c_d, Gm_d = inputs_on_device(d, M, K)
    Gs = [sentinel(d, M) for _ in range(K)]
    launch(L, d, q_d, c_d, None, Gs, None, M, 1, L.STRICT | wrap, **COEF)
    Gf, cf = [sentinel(d, M) for _ in range(K)], [sentinel(d, M) for _ in range(K)]
    launch(L, d, q_d, c_d, cf, Gf, Gm_d, M, 1, wrap, **COEF)                      # classic later stage, G stored
    dts = [float(t(x)) for x in EC.DTS[:M]]
    table = torch.from_numpy(np.stack([np.full(M, np.nan), np.full(M, np.nan), np.asarray(dts)], axis=1).astype(t)).cuda()
    gamma, wz = 8.0 / 15.0, 0.25
    a1, W, a2, junk = ([sentinel(d, M) for _ in range(K)] for _ in range(4))
    p1, pW, p2, pjunk = ([sentinel(d, M) for _ in range(K)] for _ in range(4))
    launch(L, d, q_d, c_d, a1, W, None, M, 0, wrap | L.RK3_ANCHOR, dt=COEF["dt"], gamma=gamma, zeta=wz)        # anchored first stage
    launch(L, d, q_d, c_d, a2, junk, Gm_d, M, 0, wrap | L.RK3_ANCHOR, dt=COEF["dt"], gamma=gamma, zeta=0.0)    # anchored later stage: Gm is W
    launch(L, d, q_d, c_d, p1, pW, None, M, 0, wrap | L.RK3_ANCHOR, gamma=gamma, zeta=wz, params=table)
    launch(L, d, q_d, c_d, p2, pjunk, Gm_d, M, 0, wrap | L.RK3_ANCHOR, gamma=gamma, zeta=0.0, params=table)
    # fast first stage (Gm == NULL), G stored and not, with the scalar dt and with the table; the zeta passed must be ignored
    firsts = {}
    for how in ("scalar", "table"):
        for store in (1, 0):
            cn, gn = [sentinel(d, M) for _ in range(K)], [sentinel(d, M) for _ in range(K)]
            kw = dict(params=table) if how == "table" else dict(dt=COEF["dt"])
            launch(L, d, q_d, c_d, cn, gn, None, M, store, wrap, gamma=COEF["gamma"], zeta=COEF["zeta"], **kw)
            firsts[how, store] = (cn, gn)
    torch.cuda.synchronize()
    host = lambda ts: [_members_interior(x.cpu().numpy(), d, M) for x in ts]
    Gs_h, Gf_h, a1_h, W_h, a2_h, p1_h, pW_h, p2_h = (host(x) for x in (Gs, Gf, a1, W, a2, p1, pW, p2))
    cf_h = host(cf)
    firsts_h = {key: (host(cn), host(gn)) for key, (cn, gn) in firsts.items()}
    for (how, store), (cn, gn) in firsts.items():
        if not store:             # store_G = 0 leaves Gn alone, pad columns, halos and member gaps included
            for x in gn:
                assert np.array_equal(x.cpu().numpy(), np.full(x.numel(), TC.SENTINEL, dtype=t)), (how, store)
    for x in junk + pjunk:        # an anchored later stage writes nothing through Gn
        assert np.array_equal(x.cpu().numpy(), np.full(x.numel(), TC.SENTINEL, dtype=t))
    dt64 = float(t(COEF["dt"]))
    for k in range(K):
        for m in range(M):
            tol, S = _fast_bounds(d, m, k, sfx, rough)
            G = Gs_h[k][m]
            scale = max(np.abs(G).max(), S)
            err = np.abs(Gf_h[k][m] - G).max()
            print(f"ensemble tracer fast-vs-strict {sfx} form {form} {Nx}x{Ny} rough={rough} m={m} k={k}: {err / scale:.3e} of max(max|G|, S) (tol {tol:g})")
            assert np.isfinite(Gf_h[k][m]).all() and err <= tol * scale, (m, k, err / scale)
            c = Hh.interior(d.c[m][k], Nx, Ny, H, H).astype(np.float64)
            Wop = Hh.interior(d.Gm[m][k], Nx, Ny, H, H).astype(np.float64)
            tag = (sfx, form, Nx, Ny, rough, m, k)
            g_t = float(t(gamma))
            _check_anchor(a1_h[k][m], (c, G), dt64 * g_t, tol * scale, eps, ("first cnew",) + tag)
            _check_anchor(W_h[k][m], (c, G), dt64 * wz, tol * scale, eps, ("first W",) + tag)
            _check_anchor(a2_h[k][m], (Wop, G), dt64 * g_t, tol * scale, eps, ("later cnew",) + tag)
            _check_anchor(p1_h[k][m], (c, G), dts[m] * g_t, tol * scale, eps, ("params first cnew",) + tag)
            _check_anchor(pW_h[k][m], (c, G), dts[m] * wz, tol * scale, eps, ("params first W",) + tag)
            _check_anchor(p2_h[k][m], (Wop, G), dts[m] * g_t, tol * scale, eps, ("params later cnew",) + tag)
            # the classic updates: the G- stage (Wop is its Gm) and the first stage, the latter with the member's dt of the table
            _check_update(cf_h[k][m], c, G, Wop, dt64, t, tol * scale, ("later cnew",) + tag)
            for (how, store), (cn_h, gn_h) in firsts_h.items():
                dt_m = dts[m] if how == "table" else dt64
                _check_update(cn_h[k][m], c, G, None, dt_m, t, tol * scale, (f"first cnew {how} store_G={store}",) + tag)
                if store:
                    errG = np.abs(gn_h[k][m] - G).max()
                    assert np.isfinite(gn_h[k][m]).all() and errG <= tol * scale, (how, m, k, errG / scale)


# ----------------------------------------------------------------------------------------------------------------------------------
# isolation of the members
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("form", [1, 0])
def test_a_nan_member_leaves_the_others_alone(swmhd, oracle, form, strict):
    """Three members of 2 x 2 tiles, K = 3: with every input of member 1 NaN (its whole pitch, gap included) the outputs of members 0
    and 2 are bitwise what they are without it, member 1's interiors are NaN, and every sentinel of the outputs is intact."""
    L = swmhd._lib
    Nx, Ny = TC.TX + 1, TC.TY + 1
    d = EC.stage_inputs(oracle, Nx, Ny, form, "f64")
    M, K = EC.MEMBERS, 3
    sy, sm = EC.layout(Nx, Ny)
    flags = (L.STRICT if strict else 0) | L.WRAP_X | L.WRAP_Y

    def run(poison):
        q_d, c_d, Gm_d = inputs_on_device(d, M, K, poison=poison)
        cnew, Gn = [sentinel(d, M) for _ in range(K)], [sentinel(d, M) for _ in range(K)]
        launch(L, d, q_d, c_d, cnew, Gn, Gm_d, M, 1, flags, **COEF)
        torch.cuda.synchronize()
        return [x.cpu().numpy() for x in cnew + Gn]
    clean, bad = run(None), run(1)
    inner = EC.pack([np.ones((Ny + 2 * H, Nx + 2 * H))], Nx, Ny, np.float64) != TC.SENTINEL     # the interior within one member's pitch
    for a, b in zip(clean, bad):
        for m in (0, 2):
            assert np.isfinite(a[m * sm:(m + 1) * sm]).all() and np.array_equal(a[m * sm:(m + 1) * sm], b[m * sm:(m + 1) * sm]), m
        b1 = b[sm:2 * sm]
        assert np.isnan(b1[inner]).all()
        assert (b1[~inner] == TC.SENTINEL).all()                  # its halos, pad columns and gap


# ----------------------------------------------------------------------------------------------------------------------------------
# whole runs of ShallowWaterEnsemble(tracers=...)
# ----------------------------------------------------------------------------------------------------------------------------------
RUN_NX, RUN_NY, RUN_M, RUN_STEPS = 20, 12, 3, 7
RUN_DT = 2e-3
RUN_DTS = [2e-3, 1e-3, 1.5e-3]


def _grid(S):
    return S.RectilinearGrid(size=(RUN_NX, RUN_NY), x=(0, TC.DX * RUN_NX), y=(0, TC.DY * RUN_NY))


def _member_data(O, form):
    """Per member: (q parents, d parent), rough random state and d = tanh(y) + noise, halos filled."""
    out = []
    for m in range(RUN_M):
        q = TC.fill_state(O, TC.state(RUN_NX, RUN_NY, form, 11 + m), RUN_NX, RUN_NY, (TC.P, TC.P))
        dd = TC.fill(O, TC.tracer_fields(RUN_NX, RUN_NY, 2, 11 + m)[1], RUN_NX, RUN_NY, (TC.P, TC.P))
        out.append((q, dd))
    return out


def _ensemble(S, data, form, tracers=("c", "d"), lorentz=True, **kw):
    """Strict pitched ensemble; c := A, d as given, set through set() with parents."""
    g = _grid(S)
    Py, Px = g.parent_shape
    e = S.ShallowWaterEnsemble(g, RUN_M, TC.GRAV, TC.FCOR, formulation=TC.FORM_NAME[form], lorentz_forcing=lorentz, strict=True,
                               member_stride=Py * Px + 13, tracers=tracers, **kw)
    e.set(**{n: np.stack([q[k] for q, _ in data]) for k, n in enumerate(e.names)})
    if tracers:
        e.set(c=np.stack([q[3] for q, _ in data]), d=np.stack([dd for _, dd in data]))
    return e


def _advance(e, how, n=RUN_STEPS):
    """n steps: eagerly; by graph replay with an odd eager step in between; with per-member dt (eager steps, then graph replays)."""
    if how == "eager":
        for _ in range(n):
            e.time_step(RUN_DT)
    elif how == "graph":
        e.capture_graph(RUN_DT)
        e.time_steps(2, RUN_DT)
        e.time_step(RUN_DT)                  # the roles are now the other way round: time_steps must notice
        e.time_steps(n - 3, RUN_DT)
    else:
        e.time_step(RUN_DTS)
        e.time_steps(2, RUN_DTS)
        e.capture_graph(RUN_DTS)
        e.time_steps(n - 3, RUN_DTS)
    assert e.iteration == n
    return RUN_DTS if how == "perdt" else [RUN_DT] * RUN_M


@pytest.mark.parametrize("form,lor", TC.FORMS)
@pytest.mark.parametrize("how", ["eager", "graph", "perdt"])
def test_strict_ensemble_with_tracers(swmhd, oracle, form, lor, how):
    """Strict ShallowWaterEnsemble, 3 pitched members of 20 x 12, tracers (c := A, d), 7 steps: every member's state and tracers bitwise
    RefModel with that member's data and dt; the four state fields bitwise the same ensemble without tracers (per-stage path against
    the native driver); c bitwise A; member(1) stepped on alone bitwise member 1 of the ensemble stepped on."""
    S, O = swmhd, oracle
    data = _member_data(O, form)
    e = _ensemble(S, data, form)
    plain = _ensemble(S, data, form, tracers=())
    dts = _advance(e, how)
    _advance(plain, how)
    e.synchronize(); plain.synchronize()
    sol = e.solution
    assert set(sol) == set(e.names) | {"c", "d"} and set(e.tracers) == {"c", "d"}
    for a, b in zip(e.fields, plain.fields):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    assert np.array_equal(e.tracers["c"].cpu().numpy(), sol["A"].cpu().numpy())          # halos included
    for m, (q, dd) in enumerate(data):
        ref = TC.RefModel(O, q, [q[3], dd], RUN_NX, RUN_NY, form, lor, dx=e.grid.dx, dy=e.grid.dy)
        for _ in range(RUN_STEPS):
            ref.step(dts[m])
        for f, a in zip(e.fields, ref.q):
            assert np.array_equal(f[m].cpu().numpy(), a), m
        assert np.array_equal(e.tracers["c"][m].cpu().numpy(), ref.tr[0]), m
        assert np.array_equal(e.tracers["d"][m].cpu().numpy(), ref.tr[1]), m
    assert np.allclose(e.clock_times, RUN_STEPS * np.asarray(dts), rtol=0, atol=1e-12)
    # hand member 1 over and step both on
    one = e.member(1)
    assert one.tracer_names == ("c", "d") and one.iteration == RUN_STEPS
    for _ in range(2):
        one.time_step(dts[1])
        e.time_step(RUN_DTS if how == "perdt" else RUN_DT)
    one.synchronize(); e.synchronize()
    for f, t in zip(one.fields, e.fields):
        assert np.array_equal(f.numpy(), t[1].cpu().numpy())
    for n in ("c", "d"):
        assert np.array_equal(one.tracers[n].numpy(), e.tracers[n][1].cpu().numpy()), n


@pytest.mark.parametrize("form", [1, 0])
def test_a_tracer_equal_to_A_stays_A_without_forcing(swmhd, oracle, form):
    """lorentz_forcing off, halos filled after every stage (fuse_halo=False): c := A is bitwise A after 4 steps, halos included."""
    S, O = swmhd, oracle
    e = _ensemble(S, _member_data(O, form), form, lorentz=False, fuse_halo=False)
    e.time_steps(4, RUN_DT)
    e.synchronize()
    A, c = e.solution["A"].cpu().numpy(), e.tracers["c"].cpu().numpy()
    assert np.isfinite(A).all() and np.array_equal(c, A)
    assert not np.array_equal(e.tracers["d"].cpu().numpy(), A)


# ----------------------------------------------------------------------------------------------------------------------------------
# the calls an ensemble makes
# ----------------------------------------------------------------------------------------------------------------------------------
def test_calls_with_and_without_tracers(swmhd):
    S = swmhd
    g = _grid(S)
    e = S.ShallowWaterEnsemble(g, 3)
    assert e._tr == {} and e._tr_alt == {} and e._tGn == [] and e._tGm == [] and e.tracer_names == ()
    log = []
    e._L = _Recorder(e._L, log)
    e.time_step(1e-3)
    e.time_steps(2, 1e-3)
    assert log == ["swmhd_ensemble_step_rk3_f64"] * 2, log
    del log[:]
    e.update_state()
    assert log == ["swmhd_ensemble_fill_halo_periodic_f64"], log
    del log[:]
    e.time_steps(3, [1e-3, 2e-3, 1e-3])
    assert log == ["swmhd_ensemble_step_rk3_params_f64"], log
    e.synchronize()
    # with tracers and fused halos: six calls per step, whatever K and the number of members
    names = ("c", "d", "e", "f", "g")
    for members in (1, 3):
        et = S.ShallowWaterEnsemble(g, members, tracers=names)
        log = []
        et._L = _Recorder(et._L, log)
        et.time_step(1e-3)
        assert log == ["swmhd_ensemble_tendencies_rk3_f64", "swmhd_ensemble_tracers_rk3_f64"] * 3, log
        del log[:]
        et.time_steps(2, [1e-3] * members)
        assert log == ["swmhd_ensemble_tendencies_rk3_params_f64", "swmhd_ensemble_tracers_rk3_params_f64"] * 6, log
        del log[:]
        et.synchronize()                   # the lazy fill: the state, then the tracers in groups of four
        assert log == ["swmhd_ensemble_fill_halo_periodic_f64"] * 3, log
    # without fused halos every stage ends with those three fills
    eh = S.ShallowWaterEnsemble(g, 2, tracers=names, fuse_halo=False)
    log = []
    eh._L = _Recorder(eh._L, log)
    eh.time_step(1e-3)
    assert log == (["swmhd_ensemble_tendencies_rk3_f64", "swmhd_ensemble_tracers_rk3_f64"] + ["swmhd_ensemble_fill_halo_periodic_f64"] * 3) * 3, log
    eh.synchronize()
    # frames keep their fixed name list: a tracer name points at the tracers
    with pytest.raises(S._lib.SwmhdError, match=r"tracers\['c'\]"):
        eh.output_fields(("u", "c"))


def test_example_runs_an_amplitude_sweep_with_a_dye(tmp_path):
    """examples/run_swmhd.py --dye --amps 0.1,0.5: the dye's extrema of both members in the progress lines (WENO5 keeps tanh(y) within
    its initial range to a few percent), a finite c of both members in tracers.npz."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "examples", "run_swmhd.py"), "--size", "64", "--stop-time", "0.2", "--every", "10",
           "--amps", "0.1,0.5", "--dye", "--out", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("member ")]
    assert len(lines) == 2 * 3
    for l in lines:
        lo, hi = (float(x) for x in re.search(r"min\(c\): (\S+), max\(c\): (\S+),", l).groups())
        assert -1.05 <= lo <= -0.95 and 0.95 <= hi <= 1.05
    z = np.load(os.path.join(str(tmp_path), "tracers.npz"))
    assert z["c"].shape == (2, 64, 64) and np.isfinite(z["c"]).all() and int(z["iteration"]) == 20
    assert not np.array_equal(z["c"][0], z["c"][1])          # the members' flows differ (amplitude of A), and so does their dye
