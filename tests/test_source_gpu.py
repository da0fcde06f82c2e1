"""GPU tests of the static sources -- bathymetry and steady body forces: the kernel through the ABI (swmhd_source_rk3_*,
swmhd_ensemble_source_rk3_*) and ShallowWaterModel / ShallowWaterEnsemble(bathymetry=..., forcing={...: Source(...)}).

References: tests/source_cases.py (the written formula in numpy, pinned on the CPU by test_source_cases_cpu.py).  Strict results are
compared bitwise; fast results are held to the derived bound |got - ref| <= eps |ref| + ((1 + eps/2)^n - 1) |a| M against the longdouble
value, n = 2 for a plain field and 4 for one weighted by the face thickness.  The kernel's workgroup covers SWMHD_SOURCE_TILE_ROWS = 64
rows (four waves of 16) of a strip of 64 lanes x 16 bytes where every parent of the call -- sources and the thickness included -- has
the same 16-byte phase and the pitches keep it, and of 64 elements otherwise: the stage matrix runs both paths.

Lake at rest -- figures of the CPU reference (source_cases.LAKE_REFERENCE_DRIFT), 13 x 11, 20 steps of 2e-3, max(|q1|, |q2|):
fp64 6.9e-16 (vector-invariant) and 8.0e-16 (conservative), fp32 3.6e-7 and 4.1e-7; without the bathymetry 0.27 .. 0.29."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import relaxation_cases as RC
import source_cases as SC
import tracer_cases as TC
from host_call_cases import Transcript

pytestmark = pytest.mark.gpu
NPDT = {"f64": np.float64, "f32": np.float32}
TORCH_DT = {"f64": torch.float64, "f32": torch.float32}
A_STAGE = 0.013 * 0.37              # a = dt gamma of the stage matrix: no RK3 identity that could hide a wrong operand
DT_STAGE = 0.013
NF = SC.MAX_FIELDS
H = SC.H
P, B = TC.P, TC.B


def layout(n):
    """(thickness index, fields without a source) of a call of n fields: one field is its own thickness (kind 1); else the thickness is
    field 2, a plain field WITHOUT a source -- h going along --, and with twelve fields the x-face field 6 has none either."""
    return (0, ()) if n == 1 else (2, (2,) if n == 4 else (2, 6))


class Case:
    """The parents of one (shape, pitch, precision): sources, new and acc each ONE array (NF, Ny + 2 H, sy), so that with sy a multiple
    of four all parents share their 16-byte phase; h one parent (Ny + 2 H, sy) with every cell random, halos too.  new, acc: random
    interior, the sentinel everywhere else.  Field k has the kind source_cases.kind_of(k)."""

    def __init__(self, Nx, Ny, sy, t, seed):
        self.Nx, self.Ny, self.sy, self.t = Nx, Ny, sy, t
        rng = np.random.default_rng([seed, Nx, Ny])
        shp = (NF, Ny + 2 * H, sy)
        self.I = (slice(None), slice(H, H + Ny), slice(H, H + Nx))
        self.src = rng.standard_normal((NF, Ny, Nx)).astype(t)
        self.h = (1.0 + 0.3 * rng.standard_normal((Ny + 2 * H, sy))).astype(t)
        self.new, self.acc = np.full(shp, SC.SENTINEL, dtype=t), np.full(shp, SC.SENTINEL, dtype=t)
        self.new[self.I] = rng.standard_normal((NF, Ny, Nx))
        self.acc[self.I] = rng.standard_normal((NF, Ny, Nx))
        self.kind = [SC.kind_of(k) for k in range(NF)]
        self._strict, self._exact = {}, {}

    def inputs(self, rows, wrap, thick, live):
        """(old, src) parents for a call over `rows`: old is NaN but for the thickness field, and that is NaN in every cell the call may
        not read -- rows outside the range but the one south of it where a live field has kind 2, every halo cell but the column west of
        the rows where a live field has kind 1 and x is not wrapped and the row south of row 0 where one has kind 2 and y is not
        wrapped.  src: NaN in every halo cell, pad column and row outside the range."""
        j0, j1 = rows
        Nx, Ny = self.Nx, self.Ny
        west = any(self.kind[k] == SC.X_FACE for k in live)
        south = any(self.kind[k] == SC.Y_FACE for k in live)
        old = np.full((NF, Ny + 2 * H, self.sy), np.nan, dtype=self.t)
        if j1 > j0 and (west or south):
            ja = j0 - 1 if (south and j0 > 0) else j0
            old[thick, H + ja:H + j1, H:H + Nx] = self.h[H + ja:H + j1, H:H + Nx]
            if west and not wrap[0]:
                old[thick, H + j0:H + j1, H - 1] = self.h[H + j0:H + j1, H - 1]
            if south and j0 == 0:
                if wrap[1]:
                    old[thick, H + Ny - 1, H:H + Nx] = self.h[H + Ny - 1, H:H + Nx]
                else:
                    old[thick, H - 1, H:H + Nx] = self.h[H - 1, H:H + Nx]
        src = np.full((NF, Ny + 2 * H, self.sy), np.nan, dtype=self.t)
        src[:, H + j0:H + j1, H:H + Nx] = self.src[:, j0:j1]
        return old, src

    def _operands(self, k, wrap):
        kind = self.kind[k]
        if kind == SC.PLAIN:
            return self.src[k], kind, None, None
        return self.src[k], kind, self.h[H:H + self.Ny, H:H + self.Nx], SC.neighbour(self.h, self.Nx, self.Ny, kind, *wrap)

    def strict(self, k, wrap):
        if (k, wrap) not in self._strict:
            self._strict[(k, wrap)] = SC.source_strict(*self._operands(k, wrap))
        return self._strict[(k, wrap)]

    def exact(self, k, wrap):
        if (k, wrap) not in self._exact:
            self._exact[(k, wrap)] = SC.source_exact(*self._operands(k, wrap))
        return self._exact[(k, wrap)]


def ptrs(tensor, n, present=None):
    step = tensor.stride(0) * tensor.element_size()
    return (ctypes.c_void_p * n)(*[tensor.data_ptr() + k * step if (present is None or present[k]) else None for k in range(n)])


def check_outputs(c, got, start, ks, dead, scalar, rows, wrap, strict, tag):
    """got, start: (NF, rows, sy) arrays of new or acc after and before the launch; scalar = a or w as the call received it."""
    t, (j0, j1) = c.t, rows
    eps = np.finfo(t).eps
    want = start.copy()
    R = (slice(H + j0, H + j1), slice(H, H + c.Nx))
    for k in ks:
        if k in dead:
            continue
        if strict:
            want[k][R] = SC.correct(start[k][R], c.strict(k, wrap)[j0:j1], scalar)
        else:
            E, M = c.exact(k, wrap)
            ref = start[k][R].astype(np.longdouble) + np.longdouble(t(scalar)) * E[j0:j1]
            err = np.abs(got[k][R].astype(np.longdouble) - ref)
            assert np.all(err <= SC.fast_bound(ref, t(scalar), M[j0:j1], eps, c.kind[k])), (tag, k, float((err / (eps * (np.abs(ref) + M[j0:j1]))).max()))
            want[k][R] = got[k][R]
    # bitwise: the strict values, and everything the launch must not touch (halos, pad columns, rows outside, the fields without a
    # source, the fields without an acc, the fields beyond the list)
    u = np.uint64 if t == np.float64 else np.uint32
    assert np.array_equal(got.view(u), want.view(u)), tag


def _pitch(Nx, aligned):
    return (Nx + 2 * H + 1 + 3) // 4 * 4 if aligned else (Nx + 2 * H + 5) | 1


def _wrap_flags(L, wrap, bounded=False):
    fl = (L.WRAP_X if wrap[0] else 0) | (L.WRAP_Y if wrap[1] else 0)
    if bounded:      # the Bounded flags say only that the direction is not wrapped
        fl |= (0 if wrap[0] else L.BOUNDED_X) | (0 if wrap[1] else L.BOUNDED_Y)
    return fl


@pytest.mark.parametrize("pitch", ["aligned", "odd"])
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_stage_matrix(swmhd, sfx, strict, pitch):
    """Shapes x nfields in {1, 4, 12} (kinds 1, 2, 0 in turn; the thickness a field without a source, and with twelve fields a second
    one without) x {no acc, w = 1 for every field, w = dt / 4 with one acc[k] null} x row ranges {all, [1, Ny - 1), empty}, the four
    wrap modes in turn (coprime to the three acc modes: every pair meets); NaN in every cell of old, of the thickness and of the
    sources that the call may not read; sentinels around every output.  aligned: stride_y a multiple of four elements (the 16-byte
    path); odd: an odd stride_y (one element per lane)."""
    L = swmhd._lib
    t = NPDT[sfx]
    fn = getattr(L.lib(), f"swmhd_source_rk3_{sfx}")
    a = float(t(A_STAGE))
    count = 0
    for Nx, Ny in SC.stage_shapes(np.dtype(t).itemsize, pitch == "aligned"):
        sy = _pitch(Nx, pitch == "aligned")
        c = Case(Nx, Ny, sy, t, 5)
        for n in SC.NFIELDS:
            thick, dead = layout(n)
            live = [k for k in range(n) if k not in dead]
            kinds = (ctypes.c_int * n)(*c.kind[:n])
            has_src = [k not in dead for k in range(n)]
            for rows in SC.row_ranges(Ny):
                for w, null_acc in ((None, None), (1.0, None), (float(t(DT_STAGE / 4)), n - 1)):
                    wrap = SC.WRAPS[count % 4]
                    flags = (L.STRICT if strict else 0) | _wrap_flags(L, wrap, count % 8 >= 4)
                    count += 1
                    old_d, src_d = (torch.from_numpy(x).cuda() for x in c.inputs(rows, wrap, thick, live))
                    new_d, acc_d = torch.from_numpy(c.new).cuda(), torch.from_numpy(c.acc).cuda()
                    has_acc = [k != null_acc for k in range(n)]
                    rc = fn(ptrs(old_d, n), ptrs(new_d, n), ptrs(acc_d, n, has_acc) if w is not None else None, ptrs(src_d, n, has_src),
                            kinds, n, thick, Nx, Ny, H, H, sy, a, w if w is not None else 0.0, rows[0], rows[1], flags, None)
                    L.check(rc, "swmhd_source_rk3")
                    torch.cuda.synchronize()
                    tag = (Nx, Ny, n, w, rows, wrap)
                    check_outputs(c, new_d.cpu().numpy(), c.new, range(n), dead, a, rows, wrap, strict, ("new",) + tag)
                    accs = [k for k in range(n) if has_acc[k]] if w is not None else []
                    check_outputs(c, acc_d.cpu().numpy(), c.acc, accs, dead, w, rows, wrap, strict, ("acc",) + tag)


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_sources_of_another_phase(swmhd, sfx):
    """Sources one element further into their allocation than the fields, which have the pitch of the 16-byte path, take the one-element
    path; the same call with equal phases takes the 16-byte path.  Both are bitwise the restatement in strict, so bitwise equal, and
    the element in front of the shifted array is not touched."""
    L = swmhd._lib
    t = NPDT[sfx]
    Nx, Ny, n = 129, 17, 4
    sy = _pitch(Nx, True)
    c = Case(Nx, Ny, sy, t, 9)
    rows, wrap = (0, Ny), (True, True)
    thick, dead = layout(n)
    old, src = c.inputs(rows, wrap, thick, [k for k in range(n) if k not in dead])
    es = np.dtype(t).itemsize
    kinds = (ctypes.c_int * n)(*c.kind[:n])
    results = []
    for shift in (1, 0):
        old_d, new_d, acc_d = torch.from_numpy(old).cuda(), torch.from_numpy(c.new).cuda(), torch.from_numpy(c.acc).cuda()
        flat = torch.full((src.size + 1,), SC.SENTINEL, dtype=old_d.dtype, device="cuda")
        flat[shift:shift + src.size].copy_(torch.from_numpy(src).reshape(-1))
        at = (ctypes.c_void_p * n)(*[flat.data_ptr() + (shift + k * src[0].size) * es if k not in dead else None for k in range(n)])
        rc = getattr(L.lib(), f"swmhd_source_rk3_{sfx}")(ptrs(old_d, n), ptrs(new_d, n), ptrs(acc_d, n), at, kinds, n, thick, Nx, Ny, H, H, sy,
                                                         float(t(A_STAGE)), 1.0, 0, Ny, L.STRICT | L.WRAP_X | L.WRAP_Y, None)
        L.check(rc, "swmhd_source_rk3")
        torch.cuda.synchronize()
        assert flat[0 if shift else -1].item() == SC.SENTINEL
        got = new_d.cpu().numpy(), acc_d.cpu().numpy()
        check_outputs(c, got[0], c.new, range(n), dead, float(t(A_STAGE)), rows, wrap, True, ("new", shift))
        check_outputs(c, got[1], c.acc, range(n), dead, 1.0, rows, wrap, True, ("acc", shift))
        results.append(got)
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(*results))


# ----------------------------------------------------------------------------------------------------------------------------------
# ensembles through the ABI
# ----------------------------------------------------------------------------------------------------------------------------------
ENS_GEOMETRIES = {
    # the 16-byte path with two strips (128 doubles | 256 floats each) and two row blocks of 64 rows
    "vec-2x2": dict(Nx={"f64": 129, "f32": 257}, Ny=65, sy={"f64": 136, "f32": 264}, gap=8, vec=True),
    # an odd stride_m: one element per lane, two strips of 64 columns, one row block
    "elem-2x1": dict(Nx={"f64": 65, "f32": 65}, Ny=17, sy={"f64": 72, "f32": 72}, gap=9, vec=False),
}


@pytest.mark.parametrize("members", [1, 3])
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_ensemble_members_are_single_grid_calls(swmhd, sfx, members):
    """Four fields in one call (x face, y face, the thickness without a source, plain), stride_m pitched with the sentinel in the gap;
    the sources per member (source_stride_m a whole parent), shared by all members (0), and shared at another 16-byte phase than the
    fields'.  dt: one for all (params NULL; w = 1), and per member from the (g, f, dt) table, each with w = 1 and with SWMHD_RK3_ANCHOR
    (with the table w = 1/4 of each member's dt, without it w as given).  Strict: member m is bitwise the single-grid call with
    a = dt_m gamma formed in the element type as the kernel forms it.  Fast: member m is held to the derived bound."""
    L = swmhd._lib
    t = NPDT[sfx]
    for name, geo in ENS_GEOMETRIES.items():
        for strict in (True, False):
            _ensemble_abi_case(L, sfx, t, members, name, geo, strict)


# the sources' member pitch ALONE breaks the phase: stride_y and stride_m multiples of four elements, an odd source_stride_m -- one element
# per lane, two strips of 64 columns, one row block
SOURCE_PITCH_GEOMETRY = dict(Nx={"f64": 65, "f32": 65}, Ny=17, sy={"f64": 72, "f32": 72}, gap=8, source_gap=9, vec=False)


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_ensemble_source_pitch_alone_takes_the_element_path(swmhd, sfx):
    """Two members of 65 x 17 whose parents would take the 16-byte path and whose per-member sources lie an odd number of elements
    apart: the assertions of test_ensemble_members_are_single_grid_calls -- bitwise the per-member single-grid calls in strict, the
    sentinels in the gaps untouched."""
    geo = SOURCE_PITCH_GEOMETRY
    size = (geo["Ny"] + 2 * H) * geo["sy"][sfx]
    assert geo["sy"][sfx] % 4 == 0 and (size + geo["gap"]) % 4 == 0 and (size + geo["source_gap"]) % 2 == 1
    for strict in (True, False):
        _ensemble_abi_case(swmhd._lib, sfx, NPDT[sfx], 2, "source-elem", geo, strict)


def _ensemble_abi_case(L, sfx, t, members, name, geo, strict):
    Nx, Ny, n = geo["Nx"][sfx], geo["Ny"], 4
    sy = geo["sy"][sfx]
    size = (Ny + 2 * H) * sy
    stride_m = size + geo["gap"]
    source_stride_m = size + geo.get("source_gap", geo["gap"])      # of the sources given per member
    V = 16 // np.dtype(t).itemsize
    assert (sy % V == 0 and stride_m % V == 0 and source_stride_m % V == 0) == geo["vec"]
    es = np.dtype(t).itemsize
    thick, dead = layout(n)
    live = [k for k in range(n) if k not in dead]
    cases = [Case(Nx, Ny, sy, t, 20 + m) for m in range(members)]
    dts = np.array([0.013 * (1 + 0.5 * m) for m in range(members)], dtype=t)
    gamma = t(0.37)
    params = np.stack([np.full(members, 9.81), np.ones(members), dts], axis=1).astype(t)
    single = getattr(L.lib(), f"swmhd_source_rk3_{sfx}")
    ens = getattr(L.lib(), f"swmhd_ensemble_source_rk3_{sfx}")
    wrap = (True, True)
    flags = (L.STRICT if strict else 0) | L.WRAP_X | L.WRAP_Y
    kinds = (ctypes.c_int * n)(*cases[0].kind[:n])
    has_src = [k not in dead for k in range(n)]
    u = np.uint64 if sfx == "f64" else np.uint32

    def pack(arrs, fill, pitch=stride_m):        # (n, members * pitch): field k of member m at [k, m * pitch:]
        out = np.full((n, members * pitch), fill, dtype=t)
        for m, a in enumerate(arrs):
            out[:, m * pitch:m * pitch + size] = a[:n].reshape(n, size)
        return torch.from_numpy(out).cuda()

    def run_ensemble(mode, par, w, anchor, rows):
        """mode: "member" (a source set per member), "shared" (one for all), "shifted" (one for all, one element off the fields' phase)"""
        ins = [c.inputs(rows, wrap, thick, live) for c in cases]
        old_d = pack([i[0] for i in ins], np.nan)
        new_d, acc_d = pack([c.new for c in cases], SC.SENTINEL), pack([c.acc for c in cases], SC.SENTINEL)
        if mode == "member":
            src_d, src_sm = pack([i[1] for i in ins], np.nan, source_stride_m), source_stride_m
            src_p = ptrs(src_d, n, has_src)
        else:
            shift = 1 if mode == "shifted" else 0
            src_d, src_sm = torch.full((n * size + 1,), np.nan, dtype=old_d.dtype, device="cuda"), 0
            src_d[shift:shift + n * size].copy_(torch.from_numpy(ins[0][1][:n]).reshape(-1))
            src_p = (ctypes.c_void_p * n)(*[src_d.data_ptr() + (shift + k * size) * es if has_src[k] else None for k in range(n)])
        par_d = torch.from_numpy(params).cuda()
        rc = ens(ptrs(old_d, n), ptrs(new_d, n), ptrs(acc_d, n), src_p, kinds, n, thick, members, stride_m, src_sm, Nx, Ny, H, H, sy,
                 par_d.data_ptr() if par else None, float(gamma) if par else float(dts[0] * gamma), w, rows[0], rows[1],
                 flags | (L.RK3_ANCHOR if anchor else 0), None)
        L.check(rc, "swmhd_ensemble_source_rk3")
        torch.cuda.synchronize()
        return new_d.cpu().numpy(), acc_d.cpu().numpy()

    def run_single(m, src_case, a, w, rows):
        old, _ = cases[m].inputs(rows, wrap, thick, live)
        _, src = src_case.inputs(rows, wrap, thick, live)
        old_d, src_d = torch.from_numpy(old).cuda(), torch.from_numpy(src).cuda()
        new_d, acc_d = torch.from_numpy(cases[m].new).cuda(), torch.from_numpy(cases[m].acc).cuda()
        rc = single(ptrs(old_d, n), ptrs(new_d, n), ptrs(acc_d, n), ptrs(src_d, n, has_src), kinds, n, thick, Nx, Ny, H, H, sy, a, w, rows[0],
                    rows[1], flags, None)
        L.check(rc, "swmhd_source_rk3")
        torch.cuda.synchronize()
        return new_d.cpu().numpy()[:n].reshape(n, size), acc_d.cpu().numpy()[:n].reshape(n, size)

    quarter = t(0.25)
    for rows in ((0, Ny), (1, Ny - 1)):
        for mode, par, w, anchor in (("member", False, 1.0, False), ("shared", False, float(dts[0] * quarter), True), ("member", True, 1.0, False),
                                     ("shared", True, float(quarter), True), ("shifted", True, float(quarter), True)):
            got_new, got_acc = run_ensemble(mode, par, w, anchor, rows)
            for m in range(members):
                tag = (name, strict, rows, mode, par, anchor, m)
                a_m = float((dts[m] if par else dts[0]) * gamma)
                w_m = float(dts[m] * quarter) if (anchor and par) else w
                lo = m * stride_m
                mine = [g[:, lo:lo + size] for g in (got_new, got_acc)]
                assert np.all(got_new[:, lo + size:lo + stride_m] == SC.SENTINEL) and np.all(got_acc[:, lo + size:lo + stride_m] == SC.SENTINEL), tag
                # the reference of member m: its own fields and thickness, the sources of member m or of member 0 (shared)
                c = cases[m]
                if mode != "member":
                    c = Case(Nx, Ny, sy, t, 20 + m)
                    c.src = cases[0].src
                if strict:
                    one_new, one_acc = run_single(m, c, a_m, w_m, rows)
                    assert np.array_equal(mine[0].view(u), one_new.view(u)), tag
                    assert np.array_equal(mine[1].view(u), one_acc.view(u)), tag
                for got, start, scalar, what in ((mine[0], c.new, a_m, "new"), (mine[1], c.acc, w_m, "acc")):
                    full = start.copy()
                    full[:n] = got.reshape(n, Ny + 2 * H, sy)
                    check_outputs(c, full, start, range(n), dead, scalar, rows, wrap, strict, (what,) + tag)


# ----------------------------------------------------------------------------------------------------------------------------------
# whole runs
# ----------------------------------------------------------------------------------------------------------------------------------
DT, STEPS = 2e-3, 10
RUN_GRIDS = [(13, 11), (48, 40)]
F0, C0 = 0.4, 0.25
_reference = {}


def _grid(S, Nx, Ny, topo=(P, P)):
    names = {P: "Periodic", B: "Bounded"}
    return S.RectilinearGrid(size=(Nx, Ny), x=(0, TC.DX * Nx), y=(0, TC.DY * Ny), topology=(names[topo[0]], names[topo[1]], "Flat"))


def _bottom(x, y, Lx, Ly):
    return 0.2 * np.exp(-((x - 0.4 * Lx) / (0.2 * Lx)) ** 2 - ((y - 0.6 * Ly) / (0.25 * Ly)) ** 2) + 0.05 * np.sin(2 * np.pi * x / Lx + 0 * y)


def _kolmogorov(x, y, Ly):
    return F0 * np.sin(4 * np.pi * y / Ly) + 0 * x


def _tracer_source(x, y, Lx):
    return C0 * np.cos(2 * np.pi * x / Lx) + 0 * y


def _arguments(S, g, names):
    """bathymetry and forcing of the runs: a hill with a sine ridge, a Kolmogorov force on the first momentum-like field, a source of
    tracer c; d is left alone."""
    return dict(bathymetry=lambda x, y: _bottom(x, y, g.Lx, g.Ly),
                forcing={names[0]: S.Source(lambda x, y: _kolmogorov(x, y, g.Ly)), "c": S.Source(lambda x, y: _tracer_source(x, y, g.Lx))})


def _source_list(g, form, topo=(P, P), grav=TC.GRAV, tracers=True, t=np.float64):
    """The same as RefModel takes it: S as source_cases.host_source builds it from the callables evaluated on the grid's nodes."""
    I = (slice(H, H + g.Ny), slice(H, H + g.Nx))
    xc, xf, yc = g.xc[I[1]][None, :], g.xf[I[1]][None, :], g.yc[I[0]][:, None]
    b = _bottom(xc, yc, g.Lx, g.Ly)
    Su = SC.host_source(b, _kolmogorov(xf, yc, g.Ly), grav, g.dx, 1, topo[0] == P, t)
    Sv = SC.host_source(b, 0.0, grav, g.dy, 0, topo[1] == P, t)
    kinds = (SC.PLAIN, SC.PLAIN) if form == 1 else (SC.X_FACE, SC.Y_FACE)
    out = [(kinds[0], Su), (kinds[1], Sv), None, None]
    return out + ([(SC.PLAIN, _tracer_source(xc, yc, g.Lx).astype(t)), None] if tracers else [])


def _start(O, Nx, Ny, form, topo=(P, P)):
    q = TC.fill_state(O, TC.state(Nx, Ny, form, 11, rough=False), Nx, Ny, topo, TC.grad_A(topo))
    d = TC.fill(O, TC.tracer_fields(Nx, Ny, 2, 11, rough=False)[1], Nx, Ny, topo)
    return q, d


def _model(S, O, Nx, Ny, form, strict=True, sources=True, tracers=("c", "d"), **kw):
    g = _grid(S, Nx, Ny)
    q, d = _start(O, Nx, Ny, form)
    names = ("u", "v") if form == 1 else ("uh", "vh")
    if sources:
        args = _arguments(S, g, names)
        if not tracers:
            del args["forcing"]["c"]
        args["forcing"].update(kw.pop("forcing", {}))
        kw.update(args)
    m = S.ShallowWaterModel(g, TC.GRAV, TC.FCOR, formulation=TC.FORM_NAME[form], strict=strict, tracers=tracers, **kw)
    for f, a in zip(m.fields, q):
        f.data.copy_(torch.from_numpy(a))
    if tracers:
        m.tracers["c"].data.copy_(torch.from_numpy(q[3]))
        m.tracers["d"].data.copy_(torch.from_numpy(d))
    return m


def _ref(S, O, Nx, Ny, form, lor):
    """The reference stepper after STEPS steps, computed once per (grid, formulation) and left unchanged."""
    key = (Nx, Ny, form)
    if key not in _reference:
        g = _grid(S, Nx, Ny)
        q, d = _start(O, Nx, Ny, form)
        r = SC.RefModel(O, q, [q[3], d], [None] * 6, Nx, Ny, form, lor, "classic", dx=g.dx, dy=g.dy, source=_source_list(g, form))
        for _ in range(STEPS):
            r.step(DT)
        _reference[key] = r
    return _reference[key]


@pytest.mark.parametrize("how", ["eager", "graph", "checkpoint"])
@pytest.mark.parametrize("form,lor", TC.FORMS)
@pytest.mark.parametrize("Nx,Ny", RUN_GRIDS)
def test_strict_runs_are_the_reference(swmhd, oracle, tmp_path, Nx, Ny, form, lor, how):
    """Strict model over a hill, with a Kolmogorov force and a tracer source, 10 steps: every field bitwise the reference stepper (oracle
    stage + restated correction), halos included -- stepped eagerly; through capture_graph with time_steps(5) twice, so that the second
    call starts on swapped roles; and across a save_checkpoint / load_checkpoint at step 5 (the sources are the constructor's)."""
    S, O = swmhd, oracle
    m = _model(S, O, Nx, Ny, form)
    assert [s[0] for s in m._source] == list(m.names[:2]) + ["c"] and m._source_thickness == (None if form == 1 else "h")
    ref = _ref(S, O, Nx, Ny, form, lor)
    if how == "eager":
        for _ in range(STEPS):
            m.time_step(DT)
    elif how == "graph":
        m.capture_graph(DT)
        m.time_steps(5, DT)
        m.time_steps(5, DT)
    else:
        m.time_steps(5, DT)
        path = str(tmp_path / "ck.npz")
        m.save_checkpoint(path)
        m = _model(S, O, Nx, Ny, form)
        m.tracers["d"].data.zero_()
        m.load_checkpoint(path)
        m.time_steps(5, DT)
    m.synchronize()
    assert m.iteration == STEPS
    for f, a in zip(m.fields, ref.q):
        assert np.array_equal(f.numpy(), a)
    assert np.array_equal(m.tracers["c"].numpy(), ref.tr[0]) and np.array_equal(m.tracers["d"].numpy(), ref.tr[1])


@pytest.mark.parametrize("form,lor", TC.FORMS)
@pytest.mark.parametrize("Nx,Ny", RUN_GRIDS)
def test_fast_runs_follow_the_strict_run(swmhd, oracle, Nx, Ny, form, lor):
    """Fast model (anchor form), same run: within the project's fast tolerance of whole runs, 1e-12 max |field|, of the strict result;
    and the sources have moved every forced field by far more than that."""
    S, O = swmhd, oracle
    m = _model(S, O, Nx, Ny, form, strict=False)
    plain = _model(S, O, Nx, Ny, form, strict=False, sources=False)
    m.time_steps(STEPS, DT)
    plain.time_steps(STEPS, DT)
    m.synchronize(); plain.synchronize()
    ref = _ref(S, O, Nx, Ny, form, lor)
    for name, f, a in zip(list(m.names) + ["c", "d"], m.fields + [m.tracers["c"], m.tracers["d"]], ref.q + ref.tr):
        err = np.abs(f.numpy() - a).max() / np.abs(a).max()
        print(f"fast vs strict {Nx}x{Ny} form {form} {name}: {err:.3e}")
        assert err <= 1e-12
    for k, (f, a) in enumerate(zip(plain.fields + [plain.tracers["c"]], ref.q + ref.tr[:1])):
        if k not in (2, 3):
            assert np.abs(f.numpy() - a).max() > 1e-6 * np.abs(a).max()


@pytest.mark.parametrize("form,lor", TC.FORMS)
def test_bathymetry_in_a_bounded_channel(swmhd, oracle, form, lor):
    """(Periodic, Bounded) strict model with gradient conditions on A over the hill: bitwise the reference stepper built from the
    oracle's Bounded step plus the restated correction, halos included -- the thickness south of row 0 is the filled halo, and the
    wall line of v | vh stays what the fill makes it."""
    S, O = swmhd, oracle
    Nx, Ny, topo = 48, 40, (P, B)
    g = _grid(S, Nx, Ny, topo)
    bcs = {"A": S.FieldBoundaryConditions(north=S.GradientBoundaryCondition(-0.05), south=S.GradientBoundaryCondition(-0.05))}
    m = S.ShallowWaterModel(g, TC.GRAV, TC.FCOR, formulation=TC.FORM_NAME[form], strict=True, boundary_conditions=bcs,
                            bathymetry=lambda x, y: _bottom(x, y, g.Lx, g.Ly))
    q = TC.fill_state(O, TC.state(Nx, Ny, form, 11, rough=False), Nx, Ny, topo, TC.grad_A(topo), g.dx, g.dy)
    for f, a in zip(m.fields, q):
        f.data.copy_(torch.from_numpy(a))
    for _ in range(STEPS):
        m.time_step(DT)
    m.synchronize()
    src = _source_list(g, form, topo, tracers=False)
    src[0] = (src[0][0], SC.host_source(_bottom(g.xc[H:H + Nx][None, :], g.yc[H:H + Ny][:, None], g.Lx, g.Ly), 0.0, TC.GRAV, g.dx, 1, True, np.float64))
    r = SC.RefModel(O, q, [], [None] * 4, Nx, Ny, form, lor, "classic", topo, TC.grad_A(topo), g.dx, g.dy, source=src)
    for _ in range(STEPS):
        r.step(DT)
    for f, a in zip(m.fields, r.q):
        assert np.array_equal(f.numpy(), a)


# ---- the lake at rest -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("form,lor", TC.FORMS)
@pytest.mark.parametrize("name", list(SC.LAKE_TOPOS))
def test_lake_at_rest(swmhd, oracle, name, form, lor, sfx, strict):
    """h = H - b, no flow, A = 0, 20 steps over a 2-D bottom, periodic and in a channel: max(|q1|, |q2|) stays within ten times the drift
    of the CPU reference on the same case (source_cases.LAKE_MARGIN); the same h without the bathymetry reaches at least 1e6 (fp64) /
    1e3 (fp32) times that margin.  Fails where the constructor has no `bathymetry`."""
    S, O = swmhd, oracle
    t, topo = NPDT[sfx], SC.LAKE_TOPOS[name]
    Nx, Ny = SC.LAKE_NX, SC.LAKE_NY
    g = _grid(S, Nx, Ny, topo)
    b = SC.lake_bottom(topo=topo)
    q = SC.lake_state(O, b, topo, t)
    drift = {}
    for key, kw in (("lake", dict(bathymetry=b)), ("flat", {})):
        m = S.ShallowWaterModel(g, SC.LAKE_G, 0.0, formulation=TC.FORM_NAME[form], dtype=TORCH_DT[sfx], strict=strict, **kw)
        for f, a in zip(m.fields, q):
            f.data.copy_(torch.from_numpy(a))
        for _ in range(SC.LAKE_STEPS):
            m.time_step(SC.LAKE_DT)
        m.synchronize()
        drift[key] = SC.lake_drift([f.numpy() for f in m.fields])
        if key == "lake":
            assert np.array_equal(m.bathymetry, b) and m._source is not None
            assert np.abs(m.fields[2].numpy() - q[2]).max() <= 1e3 * SC.LAKE_MARGIN[(name, form, sfx)]
    margin = SC.LAKE_MARGIN[(name, form, sfx)]
    print(f"lake at rest {name} form {form} {sfx} {'strict' if strict else 'fast'}: drift {drift['lake']:.3e}, margin {margin:.3e}, "
          f"without bathymetry {drift['flat']:.3e}")
    assert drift["lake"] <= margin
    assert drift["flat"] >= SC.LAKE_UNBALANCED_FACTOR[sfx] * margin


# ---- the RK3 property --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
def test_rk3_property_on_the_device(swmhd, strict):
    """A uniform tracer under (Relaxation(r), Source(F0)), zero velocity, 8 x 8, 20 steps: c_n = (F0 / r)(1 - R(-r dt)^n) within the
    margin the CPU reference sets (ten times its own deviation); the fast run (anchor form, where a wrong weight of acc shows) like the
    strict one."""
    S = swmhd
    Nx, Ny = SC.RK3_NX, SC.RK3_NY
    g = S.RectilinearGrid(size=(Nx, Ny), x=(0, SC.DX * Nx), y=(0, SC.DY * Ny))
    m = S.ShallowWaterModel(g, TC.GRAV, 0.0, strict=strict, tracers=("c",), forcing={"c": (S.Relaxation(SC.RK3_RATE), S.Source(SC.RK3_F0))})
    m.set(u=0.0, v=0.0, h=1.0, A=0.0, c=0.0)
    tr = Transcript()
    tr.watch(m)
    tr.do("steps", lambda: [m.time_step(SC.RK3_DT) for _ in range(SC.RK3_STEPS)])
    m.synchronize()
    names = [c[0] for c in tr.blocks[0][1]]
    assert names == ["swmhd_tendencies_rk3_f64", "swmhd_tracers_rk3_f64", "swmhd_relaxation_rk3_f64", "swmhd_source_rk3_f64"] * (3 * SC.RK3_STEPS)
    dev = SC.rk3_deviation(m.tracers["c"].numpy())
    print(f"Relaxation + Source on the device ({'strict' if strict else 'fast'}): relative deviation {dev:.3e}, margin {SC.RK3_MARGIN:.3e}")
    assert dev <= SC.RK3_MARGIN
    assert not np.any(m.fields[0].numpy()) and not np.any(m.fields[1].numpy()) and np.all(m.fields[2].numpy() == 1.0)


# ---- unchanged calls ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
def test_without_sources_nothing_changes(swmhd, oracle, strict):
    """bathymetry absent, None and constant, Source(0.0): the ctypes calls of time_step and time_steps, argument by argument, and the
    state are those of a model built without the arguments; so are the recorded host calls of tests/host_call_cases.py."""
    S, O = swmhd, oracle
    out = []
    for kw in ({}, dict(bathymetry=None), dict(bathymetry=np.full((40, 48), 0.3)), dict(bathymetry=lambda x, y: 0.2),
               dict(forcing={"u": S.Source(0.0), "h": S.Source(lambda x, y: 0.0 * x)})):
        for tracers in ((), ("c", "d")):
            m = _model(S, O, 48, 40, 1, strict=strict, sources=False, tracers=tracers, **kw)
            assert m._source is None and m._corrections == []
            tr = Transcript()
            tr.watch(m)
            tr.do("time_step", m.time_step, DT)
            tr.do("time_steps", m.time_steps, 3, DT)
            m.synchronize()
            out.append((bool(tracers), tr.blocks, [f.numpy() for f in m.fields]))
    for with_tracers in (False, True):
        same = [o for o in out if o[0] == with_tracers]
        assert len(same) == 5
        for o in same[1:]:
            assert o[1] == same[0][1]
            assert all(np.array_equal(x, y) for x, y in zip(o[2], same[0][2]))
    names = [c[0] for _, calls in out[0][1] for c in calls]
    assert not any("source" in n for n in names) and names


def test_recorded_host_calls_are_unchanged(swmhd):
    """The two scenarios of tests/host_call_cases.py that hand over arguments which leave no correction against tests/golden/host_calls.json (tests/test_host_calls_gpu.py compares all of them): the new
    arguments at their defaults change no call."""
    import json
    import host_call_cases as HC
    golden = HC.load_golden()
    for name in ("H_absent_given", "H_absent_plain"):
        assert json.loads(json.dumps(HC.run(swmhd, name))) == golden[name], name


def test_a_source_adds_one_launch_per_stage(swmhd, oracle):
    S, O = swmhd, oracle
    for form, thick in ((1, -1), (0, 2)):
        for strict in (True, False):
            m = _model(S, O, 48, 40, form, strict=strict)
            tr = Transcript()
            tr.watch(m)
            tr.do("step", m.time_steps, 2, DT)
            names = [c[0] for c in tr.blocks[0][1]]
            assert names == ["swmhd_tendencies_rk3_f64", "swmhd_tracers_rk3_f64", "swmhd_source_rk3_f64"] * 6, names
            calls = [c for c in tr.blocks[0][1] if c[0] == "swmhd_source_rk3_f64"]
            # q1, q2, c -- and h going along where the conservative fields need the thickness; an operand in storing stages only
            n = 3 if form == 1 else 4
            assert [c[6] for c in calls] == [n] * 6 and [c[7] for c in calls] == [thick] * 6
            assert [c[3] != "null" for c in calls] == ([True, True, False] if strict else [True, False, False]) * 2
            assert [[p != "null" for p in c[4]] for c in calls] == [[True, True, True] if form == 1 else [True, True, False, True]] * 6
            m.synchronize()


# ---- all corrections together ----------------------------------------------------------------------------------------------------------
def test_all_corrections_in_their_order(swmhd, oracle):
    """BetaPlane, both closures, a drag, the sources and the stirring on one strict model: the launches in the order Coriolis, Laplacian,
    biharmonic, relaxation, source, stochastic, and every field bitwise the reference stepper that composes them so -- and not bitwise
    one that puts the source in front of the relaxation."""
    import coriolis_cases  # noqa: F401  (RefModel's Coriolis restatement)
    import stochastic_cases as STC
    S, O = swmhd, oracle
    Nx, Ny = 66, 17
    TWO_PI = 2 * np.pi
    g = S.RectilinearGrid(size=(Nx, Ny), x=(0, TWO_PI), y=(0, TWO_PI))
    beta = S.BetaPlane(1.0, 0.3)
    NU, ETA, NU4, ETA4, DRAG = 3e-3, 5e-3, 2e-5, 3e-5, 0.9
    KF, DK, RATE, SEED, STREAM = 3.0, 1.0, 0.05, 11, 4
    closure = (S.ScalarDiffusivity(nu=NU, kappa={"A": ETA}), S.ScalarBiharmonicDiffusivity(nu=NU4, kappa={"A": ETA4}))
    stir = S.StochasticForcing(RATE, KF, DK, seed=SEED, stream=STREAM)
    forcing = {"u": (S.Relaxation(DRAG), S.Source(lambda x, y: _kolmogorov(x, y, g.Ly)), stir), "v": (stir, S.Relaxation(DRAG)),
               "A": S.Source(0.01)}
    m = S.ShallowWaterModel(g, TC.GRAV, TC.FCOR, strict=True, coriolis=beta, closure=closure, forcing=forcing,
                            bathymetry=lambda x, y: _bottom(x, y, g.Lx, g.Ly))
    start = TC.fill_state(O, TC.state(Nx, Ny, 1, 11, rough=False), Nx, Ny, (P, P), None, g.dx, g.dy)
    for f, a in zip(m.fields, start):
        f.data.copy_(torch.from_numpy(a))
    tr = Transcript()
    tr.watch(m)
    tr.do("steps", lambda: [m.time_step(DT) for _ in range(4)])
    m.synchronize()
    names = [c[0] for c in tr.blocks[0][1]]
    stage = ["swmhd_tendencies_rk3_f64", "swmhd_coriolis_rk3_f64", "swmhd_diffusion_rk3_f64", "swmhd_biharmonic_rk3_f64",
             "swmhd_relaxation_rk3_f64", "swmhd_source_rk3_f64"]
    assert names == (stage + ["swmhd_stochastic_coefficients_f64", "swmhd_stochastic_rk3_f64"] + (stage + ["swmhd_stochastic_rk3_f64"]) * 2) * 4, names
    src = _source_list(g, 1, tracers=False)
    src[3] = (SC.PLAIN, np.full((Ny, Nx), 0.01))
    kw = dict(dx=g.dx, dy=g.dy, rows=beta.rows(g), coef=[NU, NU, 0.0, ETA], coef4=[NU4, NU4, 0.0, ETA4],
              stir=dict(seed=SEED, stream=STREAM, Lx=TWO_PI, Ly=TWO_PI, groups=[(STC.PAIR, (0, 1), KF, DK, RATE)]), source=src)
    relax = [(DRAG, None, 0.0), (DRAG, None, 0.0), None, None]
    r = SC.RefModel(O, start, [], relax, Nx, Ny, 1, 1, "classic", **kw)

    class SourceFirst(SC.RefModel):
        def source_terms(self, U):
            return {}

        def _D(self, U):
            out = super()._D(U)
            for k, d in SC.RefModel.source_terms(self, U).items():
                out[k].insert(max(len(out[k]) - 2, 0), d)      # in front of the relaxation and the stochastic term
            return out
    w = SourceFirst(O, start, [], relax, Nx, Ny, 1, 1, "classic", **kw)
    for _ in range(4):
        r.step(DT)
        w.step(DT)
    for f, a in zip(m.fields, r.q):
        assert np.array_equal(f.numpy(), a)
    assert not np.array_equal(w.q[0], r.q[0])      # the order decides the last bits, so the test above pins it


# ---- ensembles ------------------------------------------------------------------------------------------------------------------------
def _ensemble(S, O, strict, form=0, dts=None, per_member=True):
    Nx, Ny, Bm = 48, 40, 3
    g = _grid(S, Nx, Ny)
    names = ("u", "v") if form == 1 else ("uh", "vh")
    b = _bottom(g.xc[H:H + Nx][None, :], g.yc[H:H + Ny][:, None], g.Lx, g.Ly)
    kw = dict(bathymetry=np.stack([b, 0.0 * b, 1.5 * b]) if per_member else b,
              forcing={names[0]: S.Source(lambda x, y: _kolmogorov(x, y, g.Ly)), "c": S.Source([C0, 0.0, -C0] if per_member else C0)})
    e = S.ShallowWaterEnsemble(g, Bm, [9.81, 5.0, 9.81] if dts is not None else TC.GRAV, TC.FCOR, formulation=TC.FORM_NAME[form], strict=strict,
                               tracers=("c",), member_stride=(Ny + 6) * (Nx + 6) + 10, **kw)
    q, d = _start(O, Nx, Ny, form)
    for t_, a in zip(e._state + [e._tr["c"]], q + [d]):
        for m in range(Bm):
            t_[m].copy_(torch.from_numpy(a * (1.0 + 0.1 * m) if a is not q[2] else a))
    return e


@pytest.mark.parametrize("per_member_dt", [False, True], ids=["dt", "dts"])
@pytest.mark.parametrize("form", [1, 0], ids=["vector-invariant", "conservative"])
def test_ensemble_members_are_models(swmhd, oracle, form, per_member_dt):
    """Strict ensemble of three members with a bottom per member (one of them flat), a scalar tracer source per member and, with
    per-member dt, a g per member, 4 steps: member m is bitwise ShallowWaterModel(bathymetry=that member's, ...) stepped alone.  The
    ensemble adds one launch per stage; shared sources have member stride 0.  The fast ensemble (anchor form; with per-member dt the
    kernel forms dt_m / 4) stays within 1e-12."""
    S, O = swmhd, oracle
    dts = [DT, 1.5 * DT, 0.5 * DT] if per_member_dt else None
    dt = dts if per_member_dt else DT
    e = _ensemble(S, O, True, form, dts)
    assert e._source_stride == 46 * 54 and [s[0] for s in e._source] == list(e.names[:2]) + ["c"]
    shared = _ensemble(S, O, True, form, None, per_member=False)
    assert shared._source_stride == 0 and tuple(shared._source[0][2].shape) == (46, 54)
    start = [[t_[m].clone() for t_ in e._state + [e._tr["c"]]] for m in range(3)]
    tr = Transcript()
    tr.watch(e)
    tr.do("steps", e.time_steps, 2, dt)
    sfx = "params_f64" if per_member_dt else "f64"
    assert [c[0] for c in tr.blocks[0][1]] == [f"swmhd_ensemble_tendencies_rk3_{sfx}", f"swmhd_ensemble_tracers_rk3_{sfx}",
                                               "swmhd_ensemble_source_rk3_f64"] * 6
    e.time_steps(2, dt)
    e.synchronize()
    for m in range(3):
        alone = e._member_model(m)
        assert alone.bathymetry.shape == (40, 48) and np.array_equal(alone.bathymetry, e.bathymetry[m])
        for f, a in zip(alone._raw_fields + [alone._tr["c"]], start[m]):
            f.data.copy_(a)
        for _ in range(4):
            alone.time_step(dts[m] if per_member_dt else DT)
        alone.synchronize()
        for f, t_ in zip(alone.fields + [alone.tracers["c"]], e.fields + [e.tracers["c"]]):
            assert torch.equal(f.data, t_[m]), m
    fast = _ensemble(S, O, False, form, dts)
    fast.time_steps(4, dt)
    fast.synchronize()
    for a, b in zip(fast.fields + [fast.tracers["c"]], e.fields + [e.tracers["c"]]):
        assert ((a - b).abs().amax() <= 1e-12 * b.abs().amax()).item()


def test_ensemble_graph_replay_and_no_source_calls(swmhd, oracle):
    S, O = swmhd, oracle
    e, g = _ensemble(S, O, False), _ensemble(S, O, False)
    e.time_steps(5, DT)
    g.capture_graph(DT)
    g.time_steps(5, DT)
    e.synchronize(); g.synchronize()
    for a, b in zip(e.fields + [e.tracers["c"]], g.fields + [g.tracers["c"]]):
        assert torch.equal(a, b)
    grid = e.grid
    logs = []
    for kw in ({}, {"bathymetry": None}, {"bathymetry": np.full((2, 40, 48), 0.5)}, {"forcing": {"u": S.Source([0.0, 0.0])}}):
        p = S.ShallowWaterEnsemble(grid, 2, **kw)
        assert p._source is None
        tr = Transcript()
        tr.watch(p)
        tr.do("steps", p.time_steps, 2, DT)
        p.synchronize()
        logs.append(tr.blocks)
    assert logs[0] == logs[1] == logs[2] == logs[3] and [c[0] for c in logs[0][0][1]] == ["swmhd_ensemble_step_rk3_f64"]
