"""GPU tests of the StochasticForcing: the two kernels through the ABI (swmhd_[ensemble_]stochastic_coefficients_*,
swmhd_[ensemble_]stochastic_rk3_*) and ShallowWaterModel / ShallowWaterEnsemble(forcing={"u": s, "v": s, "A": s}).

References: tests/stochastic_cases.py (Philox, the coefficients and the synthesis in numpy, pinned on the CPU by
test_stochastic_cases_cpu.py).  The coefficient call and strict results are compared bitwise; fast results are held to the derived bound
|got - ref| <= eps |ref| + (M + 3) eps |a| S against the longdouble value.  The correction kernel's workgroup covers 64 rows (four waves
of 16) of a strip of 64 lanes x 16 bytes where the parents and the x tables share a 16-byte phase and the pitches keep it, and of 64
elements otherwise; it takes the modes in chunks of SWMHD_STOCHASTIC_MODE_CHUNK = 4."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import stochastic_cases as SC
import tracer_cases as TC
from host_call_cases import Transcript

pytestmark = pytest.mark.gpu
NPDT = {"f64": np.float64, "f32": np.float32}
TORCH = {"f64": torch.float64, "f32": torch.float32}
FLOAT = {"f64": ctypes.c_double, "f32": ctypes.c_float}
A_STAGE, W_STAGE = 0.013 * 0.37, 0.013 * 0.25
H = SC.H
V = ctypes.c_void_p
TWO_PI = 2 * np.pi


def _ints(v):
    return (ctypes.c_int * len(v))(*v)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ----------------------------------------------------------------------------------------------------------------------------------
# the coefficient call
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("members", [1, 3])
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_coefficients_are_the_restatement(swmhd, sfx, members):
    """Two draw groups (a pair of 9 modes, a scalar of 256), members with distinct streams, counters and amplitudes, one counter at
    2^32 - 1 (the next step carries into n_hi): three calls, each bitwise the restatement, the counter advanced by exactly one per call,
    the sentinels around the outputs untouched.  members == 1: the single-grid entry point."""
    L = swmhd._lib.lib()
    t = NPDT[sfx]
    rng = np.random.default_rng(members)
    Ms, kinds = [9, 256], [SC.PAIR, SC.SCALAR]
    sizes = [4 * 9, 2 * 256]
    seed, stream0, sdt = 0x123456789abcdef1, 0xfffffffe, 1.0 / np.sqrt(0.013)
    ens = members > 1
    pad, total = 8, sum(sizes)
    stride = total + 2 * pad
    amp = [rng.uniform(0.1, 2.0, (members, max(Ms))) for M in Ms]      # one member pitch for every group: the first M of a row are read
    ktx, kty = rng.uniform(-3, 3, Ms[0]), rng.uniform(-3, 3, Ms[0])
    counters = np.array([(1 << 32) - 1, 5, (1 << 63) + 7][:members], dtype=np.uint64)
    streams = [(stream0 + m) & SC.M32 for m in range(members)]
    coef = torch.full((members, stride), -555.5, dtype=TORCH[sfx], device="cuda")
    d_amp, d_ktx, d_kty = [_dev(a) for a in amp], _dev(ktx), _dev(kty)
    d_counter = _dev(counters.view(np.int64))
    d_streams = _dev(np.array(streams, dtype=np.uint32).view(np.int32))
    es = coef.element_size()
    offs = [pad, pad + sizes[0]]
    args = ((V * 2)(*[coef.data_ptr() + o * es for o in offs]), (V * 2)(*[a.data_ptr() for a in d_amp]), (V * 2)(d_ktx.data_ptr(), None),
            (V * 2)(d_kty.data_ptr(), None), _ints(Ms), _ints(kinds), 2)
    for call in range(3):
        if ens:
            rc = getattr(L, f"swmhd_ensemble_stochastic_coefficients_{sfx}")(d_counter.data_ptr(), *args, members, stride, Ms[1], seed,
                                                                            d_streams.data_ptr(), sdt, None)
        else:
            rc = getattr(L, f"swmhd_stochastic_coefficients_{sfx}")(d_counter.data_ptr(), *args, seed, streams[0], sdt, None)
        assert rc == 0
        torch.cuda.synchronize()
        got = coef.cpu().numpy()
        assert np.array_equal(d_counter.cpu().numpy().view(np.uint64), counters + np.uint64(call + 1))
        for m in range(members):
            n = int(counters[m]) + call
            want = np.full(stride, -555.5, dtype=t)
            pairs = SC.coefficients(SC.PAIR, amp[0][m][:Ms[0]], ktx, kty, seed, streams[m], n, 0, sdt, t)
            want[offs[0]:offs[0] + sizes[0]] = np.concatenate([pairs[0][0], pairs[0][1], pairs[1][0], pairs[1][1]])
            (P, Q), = SC.coefficients(SC.SCALAR, amp[1][m], None, None, seed, streams[m], n, 1, sdt, t)
            want[offs[1]:offs[1] + sizes[1]] = np.concatenate([P, Q])
            u = np.uint64 if t == np.float64 else np.uint32
            assert np.array_equal(got[m].view(u), want.view(u)), (call, m)
            assert np.abs(want[pad:-pad]).max() > 0


# ----------------------------------------------------------------------------------------------------------------------------------
# the correction call through the C ABI: tables and coefficients are random inputs
# ----------------------------------------------------------------------------------------------------------------------------------
NF = SC.MAX_FIELDS
FIELD_MODES = [1, SC.MODE_CHUNK - 1, SC.MODE_CHUNK, SC.MODE_CHUNK + 1, SC.MAX_MODES, 0, 3, 17, 2, 16, 5, 24]      # field 5 has no modes


class Case:
    """NF fields of one (shape, pitch, precision): new, acc and old parents as ONE array (NF, Ny + 2 H, sy) each; x tables with the
    parents' pitch and the interior at column H (the phase of the fields), y tables (2 M, Ny), coefficients (2 M,): random, tables in
    [-1, 1].  new, acc: random interior, NaN in every halo cell and pad column (a stray read poisons the result, a stray write changes
    the bits); old: NaN everywhere (never read)."""

    def __init__(self, Nx, Ny, sy, t, seed):
        self.Nx, self.Ny, self.sy, self.t = Nx, Ny, sy, t
        rng = np.random.default_rng([seed, Nx, Ny])
        shp = (NF, Ny + 2 * H, sy)
        self.I = (slice(None), slice(H, H + Ny), slice(H, H + Nx))
        self.new, self.acc = np.full(shp, np.nan, dtype=t), np.full(shp, np.nan, dtype=t)
        self.new[self.I] = rng.standard_normal((NF, Ny, Nx))
        self.acc[self.I] = rng.standard_normal((NF, Ny, Nx))
        self.old = np.full(shp, np.nan, dtype=t)
        self.cx, self.sx, self.cy, self.sy_, self.P, self.Q = [], [], [], [], [], []
        for M in FIELD_MODES:
            self.cx.append(rng.uniform(-1, 1, (M, Nx)).astype(t)); self.sx.append(rng.uniform(-1, 1, (M, Nx)).astype(t))
            self.cy.append(rng.uniform(-1, 1, (M, Ny)).astype(t)); self.sy_.append(rng.uniform(-1, 1, (M, Ny)).astype(t))
            self.P.append(rng.uniform(-2, 2, M).astype(t)); self.Q.append(rng.uniform(-2, 2, M).astype(t))
        self._strict, self._exact = {}, {}

    def strict(self, k):
        if k not in self._strict:
            self._strict[k] = SC.synth_strict(self.cx[k], self.sx[k], self.cy[k], self.sy_[k], self.P[k], self.Q[k])
        return self._strict[k]

    def exact(self, k):
        if k not in self._exact:
            self._exact[k] = SC.synth_exact(self.cx[k], self.sx[k], self.cy[k], self.sy_[k], self.P[k], self.Q[k])
        return self._exact[k]

    def device_tables(self, x_pitch):
        """(coef, xtab, ytab) lists of device tensors and the pointers the call takes; a field without modes brings null pointers.  x
        tables: rows of x_pitch elements, NaN outside the Nx columns, the interior at column H."""
        es = np.dtype(self.t).itemsize
        keep, coef, xtab, ytab = [], [], [], []
        for k, M in enumerate(FIELD_MODES):
            if M == 0:
                coef.append(None); xtab.append(None); ytab.append(None)
                continue
            xt = np.full((2 * M, x_pitch), np.nan, dtype=self.t)
            xt[0::2, H:H + self.Nx], xt[1::2, H:H + self.Nx] = self.cx[k], self.sx[k]
            yt = np.empty((2 * M, self.Ny), dtype=self.t)
            yt[0::2], yt[1::2] = self.cy[k], self.sy_[k]
            d = [_dev(np.concatenate([self.P[k], self.Q[k]])), _dev(xt), _dev(yt)]
            keep += d
            coef.append(d[0].data_ptr()); xtab.append(d[1].data_ptr() + H * es); ytab.append(d[2].data_ptr())
        return keep, coef, xtab, ytab


def ptrs(tensor, ks, present=None):
    step = tensor.stride(0) * tensor.element_size()
    return (V * len(ks))(*[tensor.data_ptr() + k * step if (present is None or present[i]) else None for i, k in enumerate(ks)])


def check_outputs(c, got, start, ks, scalar, rows, strict, tag):
    t, (j0, j1) = c.t, rows
    eps = np.finfo(t).eps
    want = start.copy()
    R = (slice(H + j0, H + j1), slice(H, H + c.Nx))
    for k in ks:
        M = FIELD_MODES[k]
        if M == 0:
            continue
        if strict:
            want[k][R] = SC.correct(start[k][R], c.strict(k)[j0:j1], scalar)
        else:
            E, S = c.exact(k)
            ref = start[k][R].astype(np.longdouble) + np.longdouble(t(scalar)) * E[j0:j1]
            err = np.abs(got[k][R].astype(np.longdouble) - ref)
            bound = SC.fast_bound(ref, t(scalar), S, eps, M)
            assert np.all(err <= bound), (tag, k, float((err / bound).max()))
            want[k][R] = got[k][R]
    u = np.uint64 if t == np.float64 else np.uint32
    assert np.array_equal(got.view(u), want.view(u)), tag      # (NaN sentinels compare by their bits)


def _pitch(Nx, aligned):
    return (Nx + 2 * H + 1 + 3) // 4 * 4 if aligned else (Nx + 2 * H + 5) | 1


# (fields of the call, with acc for which of them, rows): 12 fields with the mode counts 1, 3, 4, 5, 256 and a field without modes whose
# new is full of NaN; 3 fields, one without modes, no acc, rows [1, Ny - 1); 1 field with acc
def _calls(Ny):
    return [(list(range(NF)), [k % 2 == 0 for k in range(NF)], (0, Ny)),
            ([3, 5, 4], None, (1, Ny - 1)),
            ([2], [True], (0, Ny))]


@pytest.mark.parametrize("pitch", ["aligned", "odd"])
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_stage_matrix(swmhd, sfx, strict, pitch):
    """Shapes one column past a 64-lane strip (66, 130 in fp64 with two elements per lane, 257 in fp32 with four), one row past a
    wave's 16 rows and past the 64-row tile; aligned and odd pitch; row ranges; 1, 3 and 12 fields; mode counts around the chunk and
    256; with and without acc; NaN in every halo cell, in old, and in the new of the field without modes, which must survive."""
    B = swmhd._lib
    L = B.lib()
    t, ft = NPDT[sfx], FLOAT[sfx]
    fn = getattr(L, f"swmhd_stochastic_rk3_{sfx}")
    for Nx, Ny in SC.SHAPES:
        sy = _pitch(Nx, pitch == "aligned")
        c = Case(Nx, Ny, sy, t, 5)
        keep, coef, xtab, ytab = c.device_tables(sy)
        d_old = _dev(c.old)
        for ks, with_acc, rows in _calls(Ny):
            if rows[0] >= rows[1]:
                continue
            new0, acc0 = c.new.copy(), c.acc.copy()
            new0[5] = np.nan                                    # the field without modes
            d_new, d_acc = _dev(new0), _dev(acc0)
            pick = lambda lst: (V * len(ks))(*[lst[k] for k in ks])
            rc = fn(ptrs(d_old, ks), ptrs(d_new, ks), ptrs(d_acc, ks, with_acc) if with_acc else None, pick(coef), pick(xtab), pick(ytab),
                    _ints([FIELD_MODES[k] for k in ks]), len(ks), sy, Ny, Nx, Ny, H, H, sy, ft(A_STAGE), ft(W_STAGE), rows[0], rows[1],
                    B.STRICT if strict else B.FAST, None)
            assert rc == 0
            torch.cuda.synchronize()
            tag = (Nx, Ny, sfx, strict, pitch, tuple(ks))
            check_outputs(c, d_new.cpu().numpy(), new0, ks, ft(A_STAGE).value, rows, strict, tag + ("new",))
            acc_ks = [k for i, k in enumerate(ks) if with_acc and with_acc[i]]
            check_outputs(c, d_acc.cpu().numpy(), acc0, acc_ks, ft(W_STAGE).value, rows, strict, tag + ("acc",))


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_ensemble_members_are_single_grid_calls(swmhd, sfx, strict):
    """Three members with their own coefficients (the tables are the ensemble's), a padded member stride: member m of new and acc is
    bitwise the single-grid call with that member's coefficients.  NaN in every halo cell, in old and between the members."""
    Nx = 66
    _ensemble_abi_case(swmhd, sfx, strict, 3, (Nx, 17), _pitch(Nx, True))


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_ensemble_table_pitch_alone_takes_the_element_path(swmhd, sfx, strict):
    """Two members of 65 x 17 whose parents would take the 16-byte path (stride_y and stride_m multiples of four elements) and whose x
    tables have an odd pitch: the assertions of test_ensemble_members_are_single_grid_calls."""
    Nx = 65
    xp = _pitch(Nx, False)
    assert _pitch(Nx, True) % 4 == 0 and xp % 2 == 1
    _ensemble_abi_case(swmhd, sfx, strict, 2, (Nx, 17), xp)


def _ensemble_abi_case(swmhd, sfx, strict, members, shape, xp):
    B = swmhd._lib
    L = B.lib()
    t, ft = NPDT[sfx], FLOAT[sfx]
    Nx, Ny = shape
    sy = _pitch(Nx, True)
    c = Case(Nx, Ny, sy, t, 9)
    ks = [0, 3, 4]
    Ms = [FIELD_MODES[k] for k in ks]
    rng = np.random.default_rng(4)
    coefs = [rng.uniform(-2, 2, (members, 2 * M)).astype(t) for M in Ms]
    cstride = 2 * max(Ms) + 6
    table = np.full((len(ks), members, cstride), np.nan, dtype=t)
    for i, cf in enumerate(coefs):
        table[i, :, :cf.shape[1]] = cf
    d_table = _dev(table)
    keep, _, xtab, ytab = c.device_tables(xp)
    es = np.dtype(t).itemsize
    stride_m = (Ny + 2 * H) * sy + 4
    assert stride_m % 4 == 0
    flags = B.STRICT if strict else B.FAST

    def parents(src):
        flat = np.full((NF, members * stride_m), np.nan, dtype=t)      # NaN in the halos and between the members
        for m in range(members):
            flat[:, m * stride_m:m * stride_m + (Ny + 2 * H) * sy] = (src + t(0.25 * m)).reshape(NF, -1)
        return flat
    new0, acc0 = parents(c.new), parents(c.acc)
    d_new, d_acc, d_old = _dev(new0), _dev(acc0), _dev(np.full_like(new0, np.nan))
    pick = lambda lst: (V * len(ks))(*[lst[k] for k in ks])
    cptr = (V * len(ks))(*[d_table.data_ptr() + i * members * cstride * es for i in range(len(ks))])
    rc = getattr(L, f"swmhd_ensemble_stochastic_rk3_{sfx}")(ptrs(d_old, ks), ptrs(d_new, ks), ptrs(d_acc, ks), cptr, pick(xtab), pick(ytab),
                                                           _ints(Ms), len(ks), xp, Ny, members, stride_m, cstride, Nx, Ny, H, H, sy, None,
                                                           ft(A_STAGE), ft(W_STAGE), 0, Ny, flags, None)
    assert rc == 0
    torch.cuda.synchronize()
    got_new, got_acc = d_new.cpu().numpy(), d_acc.cpu().numpy()
    for m in range(members):
        sl = slice(m * stride_m, m * stride_m + (Ny + 2 * H) * sy)
        s_new, s_acc = _dev(np.ascontiguousarray(new0[:, sl])), _dev(np.ascontiguousarray(acc0[:, sl]))
        s_old = _dev(np.full((NF, (Ny + 2 * H) * sy), np.nan, dtype=t))
        one = (V * len(ks))(*[d_table.data_ptr() + (i * members + m) * cstride * es for i in range(len(ks))])
        rc = getattr(L, f"swmhd_stochastic_rk3_{sfx}")(ptrs(s_old, ks), ptrs(s_new, ks), ptrs(s_acc, ks), one, pick(xtab), pick(ytab), _ints(Ms),
                                                      len(ks), xp, Ny, Nx, Ny, H, H, sy, ft(A_STAGE), ft(W_STAGE), 0, Ny, flags, None)
        assert rc == 0
        torch.cuda.synchronize()
        u = np.uint64 if t == np.float64 else np.uint32
        assert np.array_equal(got_new[:, sl].view(u), s_new.cpu().numpy().view(u)), m
        assert np.array_equal(got_acc[:, sl].view(u), s_acc.cpu().numpy().view(u)), m
        assert not np.array_equal(got_new[ks[0], sl].view(u), new0[ks[0], sl].view(u))      # (the launch did something)
    for m in range(members):                                    # the padding between the members is untouched
        gap = slice(m * stride_m + (Ny + 2 * H) * sy, (m + 1) * stride_m)
        assert np.all(np.isnan(got_new[:, gap])) and np.all(np.isnan(got_acc[:, gap]))


# ----------------------------------------------------------------------------------------------------------------------------------
# whole runs
# ----------------------------------------------------------------------------------------------------------------------------------
DT, STEPS = 2e-3, 6
RUN_GRIDS = [(16, 12), (66, 17)]
KF, DK, RATE_UV, RATE_A, SEED, STREAM = 3.0, 1.0, 0.05, 0.02, 11, 4
_reference = {}


def _grid(S, Nx, Ny):
    return S.RectilinearGrid(size=(Nx, Ny), x=(0, TWO_PI), y=(0, TWO_PI))


def _start(O, Nx, Ny, g):
    return TC.fill_state(O, TC.state(Nx, Ny, 1, 11, rough=False), Nx, Ny, (TC.P, TC.P), None, g.dx, g.dy)


def _forcing(S, rate_uv=RATE_UV, rate_a=RATE_A, stream=STREAM, drag=None):
    uv, a = S.StochasticForcing(rate_uv, KF, DK, seed=SEED, stream=stream), S.StochasticForcing(rate_a, KF + 1, DK, seed=SEED, stream=stream)
    if drag is None:
        return {"u": uv, "v": uv, "A": a}
    return {"u": (S.Relaxation(drag), uv), "v": (uv, S.Relaxation(drag)), "A": a}


def _stir(rate_uv=RATE_UV, rate_a=RATE_A, stream=STREAM):
    return dict(seed=SEED, stream=stream, Lx=TWO_PI, Ly=TWO_PI,
                groups=[(SC.PAIR, (0, 1), KF, DK, rate_uv), (SC.SCALAR, (3,), KF + 1, DK, rate_a)])


def _model(S, O, Nx, Ny, strict=True, forcing="default", **kw):
    g = _grid(S, Nx, Ny)
    if forcing != "absent":
        kw["forcing"] = _forcing(S) if forcing == "default" else forcing
    m = S.ShallowWaterModel(g, TC.GRAV, TC.FCOR, strict=strict, **kw)
    for f, a in zip(m.fields, _start(O, Nx, Ny, g)):
        f.data.copy_(torch.from_numpy(a))
    return m


def _ref(S, O, Nx, Ny):
    """The reference stepper after STEPS steps, computed once per grid and left unchanged."""
    if (Nx, Ny) not in _reference:
        g = _grid(S, Nx, Ny)
        r = SC.RefModel(O, _start(O, Nx, Ny, g), [], [None] * 4, Nx, Ny, 1, 1, "classic", dx=g.dx, dy=g.dy, stir=_stir())
        for _ in range(STEPS):
            r.step(DT)
        _reference[(Nx, Ny)] = r
    return _reference[(Nx, Ny)]


@pytest.mark.parametrize("how", ["eager", "graph", "checkpoint"])
@pytest.mark.parametrize("Nx,Ny", RUN_GRIDS)
def test_strict_runs_are_the_reference(swmhd, oracle, tmp_path, Nx, Ny, how):
    """Strict model with a vortical pair on u, v and a scalar stirring of A, 6 steps: every field bitwise the reference stepper, halos
    included -- stepped eagerly; through capture_graph with time_steps(3) twice (the second call starts on swapped roles); and across
    a checkpoint saved after 3 steps and loaded into a fresh model, whose counter starts at 0."""
    S, O = swmhd, oracle
    m = _model(S, O, Nx, Ny)
    ref = _ref(S, O, Nx, Ny)
    if how == "eager":
        for _ in range(STEPS):
            m.time_step(DT)
    elif how == "graph":
        m.capture_graph(DT)
        assert int(m._stochastic.counter_values()[0]) == 0          # the warm-up steps' draws are undone
        m.time_steps(3, DT)
        m.time_steps(3, DT)
    else:
        m.time_steps(3, DT)
        path = str(tmp_path / "ck.npz")
        m.save_checkpoint(path)
        assert int(np.load(path)["stochastic_counter"][0]) == 3
        m = _model(S, O, Nx, Ny)
        m.load_checkpoint(path)
        m.time_steps(3, DT)
    m.synchronize()
    assert m.iteration == STEPS and int(m._stochastic.counter_values()[0]) == STEPS
    for f, a in zip(m.fields, ref.q):
        assert np.array_equal(f.numpy(), a)
    plain = _model(S, O, Nx, Ny, forcing=None)
    plain.time_steps(STEPS, DT)
    plain.synchronize()
    for k in (0, 1, 3):
        assert np.abs(plain.fields[k].numpy() - ref.q[k]).max() > 1e-6 * np.abs(ref.q[k]).max()      # the stirring moved the field


def test_old_checkpoints_still_load(swmhd, oracle, tmp_path):
    S, O = swmhd, oracle
    plain = _model(S, O, 16, 12, forcing=None)
    path = str(tmp_path / "old.npz")
    plain.save_checkpoint(path)
    assert "stochastic_counter" not in np.load(path).files
    m = _model(S, O, 16, 12)
    m.time_step(DT)
    m.load_checkpoint(path)
    assert int(m._stochastic.counter_values()[0]) == 1              # no counter in the file: it stays


@pytest.mark.parametrize("Nx,Ny", RUN_GRIDS)
def test_fast_runs_follow_the_strict_run(swmhd, oracle, Nx, Ny):
    """Fast model (anchor form), same run: within the project's fast tolerance of whole runs, 1e-12 max |field|, of the strict result."""
    S, O = swmhd, oracle
    m = _model(S, O, Nx, Ny, strict=False)
    m.time_steps(STEPS, DT)
    m.synchronize()
    ref = _ref(S, O, Nx, Ny)
    for name, f, a in zip(m.names, m.fields, ref.q):
        err = np.abs(f.numpy() - a).max() / np.abs(a).max()
        print(f"fast vs strict {Nx}x{Ny} {name}: {err:.3e}")
        assert err <= 1e-12


def test_the_stochastic_launch_is_last(swmhd, oracle):
    """BetaPlane, both closures, a drag beside the stirring on u and v (a tuple each) and the scalar stirring of A on one strict model:
    bitwise the reference stepper that applies Coriolis, Laplacian, biharmonic, relaxation and the stochastic term in this order --
    and not bitwise one that stirs before it relaxes."""
    import coriolis_cases  # noqa: F401  (RefModel's Coriolis restatement)
    S, O = swmhd, oracle
    Nx, Ny = 66, 17
    g = _grid(S, Nx, Ny)
    beta = S.BetaPlane(1.0, 0.3)
    NU, ETA, NU4, ETA4, DRAG = 3e-3, 5e-3, 2e-5, 3e-5, 0.9
    closure = (S.ScalarDiffusivity(nu=NU, kappa={"A": ETA}), S.ScalarBiharmonicDiffusivity(nu=NU4, kappa={"A": ETA4}))
    m = _model(S, O, Nx, Ny, forcing=_forcing(S, drag=DRAG), coriolis=beta, closure=closure)
    tr = Transcript()
    tr.watch(m)
    tr.do("steps", lambda: [m.time_step(DT) for _ in range(4)])
    m.synchronize()
    names = [c[0] for c in tr.blocks[0][1]]
    stage = ["swmhd_tendencies_rk3_f64", "swmhd_coriolis_rk3_f64", "swmhd_diffusion_rk3_f64", "swmhd_biharmonic_rk3_f64",
             "swmhd_relaxation_rk3_f64"]
    assert names == (stage + ["swmhd_stochastic_coefficients_f64", "swmhd_stochastic_rk3_f64"] + (stage + ["swmhd_stochastic_rk3_f64"]) * 2) * 4, names
    kw = dict(dx=g.dx, dy=g.dy, rows=beta.rows(g), coef=[NU, NU, 0.0, ETA], coef4=[NU4, NU4, 0.0, ETA4], stir=_stir())
    relax = [(DRAG, None, 0.0), (DRAG, None, 0.0), None, None]
    r = SC.RefModel(O, _start(O, Nx, Ny, g), [], relax, Nx, Ny, 1, 1, "classic", **kw)

    class StirFirst(SC.RefModel):
        def _D(self, U):
            return [ds[-1:] + ds[:-1] for ds in super()._D(U)]
    w = StirFirst(O, _start(O, Nx, Ny, g), [], relax, Nx, Ny, 1, 1, "classic", **kw)
    for _ in range(4):
        r.step(DT)
        w.step(DT)
    for f, a in zip(m.fields, r.q):
        assert np.array_equal(f.numpy(), a)
    assert not np.array_equal(w.q[0], r.q[0])      # the order decides the last bits, so the test above pins it


def test_ensemble_members_are_models(swmhd, oracle):
    """Strict ensemble of three members with per-member rates, one of them 0: member m is bitwise the single model with that member's
    rate and stream + m; the ensemble adds one launch per stage and one per step; member(1) carries the counter; a per-member dt raises;
    a replayed ensemble draws what the eager one draws."""
    S, O = swmhd, oracle
    Nx, Ny, Bm = 16, 12, 3
    g = _grid(S, Nx, Ny)
    rates = [0.05, 0.0, 0.2]
    forcing = _forcing(S, rate_uv=rates)
    q = _start(O, Nx, Ny, g)

    def ensemble():
        e = S.ShallowWaterEnsemble(g, Bm, TC.GRAV, TC.FCOR, strict=True, forcing=forcing)
        for t_, a in zip(e._state, q):
            for m in range(Bm):
                t_[m].copy_(torch.from_numpy(a * (1.0 + 0.1 * m)))
        return e
    e = ensemble()
    tr = Transcript()
    tr.watch(e)
    tr.do("steps", e.time_steps, 2, DT)
    step = ["swmhd_ensemble_tendencies_rk3_f64", "swmhd_ensemble_stochastic_coefficients_f64", "swmhd_ensemble_stochastic_rk3_f64"] + \
        ["swmhd_ensemble_tendencies_rk3_f64", "swmhd_ensemble_stochastic_rk3_f64"] * 2
    assert [c[0] for c in tr.blocks[0][1]] == step * 2
    one = e.member(1)
    assert one.forcing["u"].rate == 0.0 and one.forcing["u"] is one.forcing["v"] and one.forcing["A"].stream == STREAM + 1
    assert int(one._stochastic.counter_values()[0]) == 2
    e.time_steps(2, DT)
    one.time_steps(2, DT)
    e.synchronize(); one.synchronize()
    for f, t_ in zip(one.fields, e.fields):
        assert torch.equal(f.data, t_[1])
    for m in range(Bm):
        alone = S.ShallowWaterModel(g, TC.GRAV, TC.FCOR, strict=True, forcing=_forcing(S, rate_uv=rates[m], stream=STREAM + m))
        for f, a in zip(alone._raw_fields, q):
            f.data.copy_(torch.from_numpy(a * (1.0 + 0.1 * m)))
        for _ in range(4):
            alone.time_step(DT)
        alone.synchronize()
        for f, t_ in zip(alone.fields, e.fields):
            assert torch.equal(f.data, t_[m]), m
    for call in (lambda: e.time_step([DT, DT, 2 * DT]), lambda: e.time_steps(2, [DT, DT, 2 * DT]), lambda: e.capture_graph([DT, DT, 2 * DT])):
        with pytest.raises(S._lib.SwmhdError, match="SWMHD_ENOTSUP"):
            call()
    gr = ensemble()
    gr.capture_graph(DT)
    gr.time_steps(4, DT)
    gr.synchronize()
    for a, b in zip(gr.fields, e.fields):
        assert torch.equal(a, b)


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
def test_without_the_class_nothing_changes(swmhd, oracle, strict):
    """Without the class, and with rates that are all 0: the ctypes calls of time_step and time_steps, argument by argument, and the
    state are those of a model built without the argument, and nothing is allocated for the term."""
    S, O = swmhd, oracle
    out = []
    zero = _forcing(S, rate_uv=0.0, rate_a=0.0)
    for forcing in ("absent", None, {}, zero):
        m = _model(S, O, 16, 12, strict=strict, forcing=forcing)
        assert m._stochastic is None and m._corrections == []
        tr = Transcript()
        tr.watch(m)
        tr.do("time_step", m.time_step, DT)
        tr.do("time_steps", m.time_steps, 3, DT)
        m.synchronize()
        out.append((tr.blocks, [f.numpy() for f in m.fields]))
    for o in out[1:]:
        assert o[0] == out[0][0]
        assert all(np.array_equal(x, y) for x, y in zip(o[1], out[0][1]))
    names = [c[0] for _, calls in out[0][0] for c in calls]
    assert not any("stochastic" in n for n in names) and names
    # a drag alone, written as a tuple or not, makes the calls it made
    logs = []
    for drag in ({"u": S.Relaxation(0.5), "v": S.Relaxation(0.5)}, {"u": (S.Relaxation(0.5),), "v": (S.Relaxation(0.5),)},
                 {"u": (S.Relaxation(0.5), zero["u"]), "v": (zero["u"], S.Relaxation(0.5))}):
        m = _model(S, O, 16, 12, strict=strict, forcing=drag)
        tr = Transcript()
        tr.watch(m)
        tr.do("time_steps", m.time_steps, 2, DT)
        m.synchronize()
        logs.append(tr.blocks)
    assert logs[0] == logs[1] == logs[2] and not any("stochastic" in c[0] for c in logs[0][0][1])


def test_the_forcing_adds_one_launch_per_stage_and_one_per_step(swmhd, oracle):
    S, O = swmhd, oracle
    for strict in (True, False):
        m = _model(S, O, 16, 12, strict=strict)
        tr = Transcript()
        tr.watch(m)
        tr.do("step", m.time_steps, 2, DT)
        names = [c[0] for c in tr.blocks[0][1]]
        assert names == (["swmhd_tendencies_rk3_f64", "swmhd_stochastic_coefficients_f64", "swmhd_stochastic_rk3_f64"]
                         + ["swmhd_tendencies_rk3_f64", "swmhd_stochastic_rk3_f64"] * 2) * 2, names
        calls = [c for c in tr.blocks[0][1] if c[0] == "swmhd_stochastic_rk3_f64"]
        assert [c[8] for c in calls] == [3] * 6                   # u, v, A
        # an operand in storing stages only: stages 0, 1 (classic) or stage 0 (anchor)
        assert [c[3] != "null" for c in calls] == ([True, True, False] if strict else [True, False, False]) * 2
        m.synchronize()


def test_the_injected_band_on_the_device(swmhd, oracle):
    """16 x 16 from rest (u = v = 0, h = 1, A = 0, f = 0), the run of the CPU band test on a strict model: isotropic_spectra(("u", "v"))
    has its out-of-band fraction within the spectra tolerance of the reference's recorded value.  Tolerance: the per-mode bound of
    spectra2d_cases summed over all modes, relative to the whole power S, is at most 4 N eps2 + 2 N² eps2² (sum |F^| <= N sqrt(S));
    the fraction is a ratio of two such sums: twice that."""
    import spectra2d_cases as SP
    S = swmhd
    N = SC.BAND_N
    g = S.RectilinearGrid(size=(N, N), x=(0, SC.BAND_L), y=(0, SC.BAND_L))
    s = S.StochasticForcing(SC.BAND_RATE, SC.BAND_KF, SC.BAND_DK, seed=SC.BAND_SEED)
    m = S.ShallowWaterModel(g, TC.GRAV, 0.0, strict=True, forcing={"u": s, "v": s})
    m.set(u=0.0, v=0.0, h=1.0, A=0.0)
    for _ in range(SC.BAND_STEPS):
        m.time_step(SC.BAND_DT)
    spec = m.isotropic_spectra(("u", "v"))
    m.synchronize()
    power = spec.cpu().numpy()
    frac = SC.out_of_band_fraction(power)
    eps2 = SP.ETA * 2 * np.log2(N) * 2.0 ** -53
    tol = 2 * (4 * N * eps2 + 2 * N * N * eps2 * eps2)
    print(f"out-of-band fraction on the device: {frac:.3e} (reference {SC.BAND_REFERENCE_FRACTION:.3e}, tolerance {tol:.3e})")
    assert power.sum() > 0
    assert abs(frac - SC.BAND_REFERENCE_FRACTION) <= tol


# ---- the example ----------------------------------------------------------------------------------------------------------------------
def test_example_runs_with_stirring(tmp_path):
    """examples/run_swmhd.py --stir 0.01,4 --seed 3 --drag 0.05 on 64^2 for a few steps: the progress lines, the dump and its fields
    exist and are finite."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "examples", "run_swmhd.py"), "--size", "64", "--stop-time", "0.1", "--every", "5",
           "--dump-every", "0.1", "--out", str(tmp_path), "--stir", "0.01,4", "--seed", "3", "--drag", "0.05"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "StochasticForcing" in r.stdout and "modes" in r.stdout
    assert len([l for l in r.stdout.splitlines() if l.startswith("Time:")]) >= 2
    z = np.load(os.path.join(str(tmp_path), "fields_0000010.npz"))
    for n in ("u", "v", "h", "A"):
        assert np.isfinite(z[n]).all()
