"""GPU tests of the Relaxation forcing: the kernel through the ABI (swmhd_relaxation_rk3_*, swmhd_ensemble_relaxation_rk3_*) and
ShallowWaterModel / ShallowWaterEnsemble(forcing=...).

References: tests/relaxation_cases.py (the written formula in numpy, pinned on the CPU by test_relaxation_cases_cpu.py).  Strict results
are compared bitwise; fast results are held to the derived bound |got - ref| <= eps |ref| + 4 eps |a| S against the longdouble value.
The kernel's workgroup covers SWMHD_RELAXATION_TILE_ROWS = 64 rows (four waves of 16) of a strip of 64 lanes x 16 bytes (128 doubles,
256 floats) where every parent of the call -- masks and targets included -- has the same 16-byte phase and the pitches keep it, and of
64 elements otherwise: the stage matrix runs both paths, each one column and one row below, at and above its tile."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import relaxation_cases as RC
import tracer_cases as TC
from host_call_cases import Transcript

pytestmark = pytest.mark.gpu
NPDT = {"f64": np.float64, "f32": np.float32}
A_STAGE = 0.013 * 0.37              # a = dt gamma of the stage matrix: no RK3 identity that could hide a wrong operand
DT_STAGE = 0.013
NF = RC.MAX_FIELDS
H = RC.H
TVAL_UNUSED = 7.75                  # the scalar target handed over beside a target array: never read


class Case:
    """NF parents of old, mask, target, new and acc of one (shape, pitch, precision): each set ONE array (NF, Ny + 2 H, sy), so that with
    sy a multiple of four all parents share their 16-byte phase.  Inputs: random interior, NaN everywhere else.  new, acc: random
    interior, the sentinel everywhere else.  Field k has the kind relaxation_cases.kind_of(k), its own rate and scalar target."""

    def __init__(self, Nx, Ny, sy, t, seed):
        self.Nx, self.Ny, self.sy, self.t = Nx, Ny, sy, t
        rng = np.random.default_rng([seed, Nx, Ny])
        shp = (NF, Ny + 2 * H, sy)
        self.I = (slice(None), slice(H, H + Ny), slice(H, H + Nx))
        self.old, self.mask, self.target = (rng.standard_normal((NF, Ny, Nx)).astype(t) for _ in range(3))
        self.new, self.acc = np.full(shp, RC.SENTINEL, dtype=t), np.full(shp, RC.SENTINEL, dtype=t)
        self.new[self.I] = rng.standard_normal((NF, Ny, Nx))
        self.acc[self.I] = rng.standard_normal((NF, Ny, Nx))
        self.rate = [float(t(0.21 * (k + 1) + 0.01 * k * k)) for k in range(NF)]      # distinct, as the call receives them
        self.tval = [float(t(0.5 - 0.37 * k)) for k in range(NF)]
        self.kind = [RC.kind_of(k) for k in range(NF)]
        self._strict, self._exact = {}, {}

    def inputs(self, rows, dead=()):
        """(old, mask, target) parents for a call over `rows`: NaN in every halo cell, pad column and row outside the range; the fields
        of `dead` (rate 0) have old full of NaN."""
        j0, j1 = rows
        out = []
        for src in (self.old, self.mask, self.target):
            a = np.full((NF, self.Ny + 2 * H, self.sy), np.nan, dtype=self.t)
            a[:, H + j0:H + j1, H:H + self.Nx] = src[:, j0:j1]
            out.append(a)
        for k in dead:
            out[0][k] = np.nan
        return out

    def operands(self, k):
        has_mask, tk = self.kind[k]
        return (self.rate[k], self.mask[k] if has_mask else None, self.target[k] if tk == "array" else (self.tval[k] if tk == "scalar" else 0.0))

    def strict(self, k):
        if k not in self._strict:
            self._strict[k] = RC.relax_strict(self.old[k], *self.operands(k))
        return self._strict[k]

    def exact(self, k):
        if k not in self._exact:
            self._exact[k] = RC.relax_exact(self.old[k], *self.operands(k))
        return self._exact[k]

    def call_tables(self, n, ft, dead=()):
        """(rate, tval) host arrays and the (mask present, target present) lists of the first n fields as a call hands them over."""
        rate = (ft * n)(*[0.0 if k in dead else self.rate[k] for k in range(n)])
        tval = (ft * n)(*[TVAL_UNUSED if self.kind[k][1] == "array" else (self.tval[k] if self.kind[k][1] == "scalar" else 0.0) for k in range(n)])
        return rate, tval, [self.kind[k][0] for k in range(n)], [self.kind[k][1] == "array" for k in range(n)]


def ptrs(tensor, n, present=None):
    step = tensor.stride(0) * tensor.element_size()
    return (ctypes.c_void_p * n)(*[tensor.data_ptr() + k * step if (present is None or present[k]) else None for k in range(n)])


def check_outputs(c, got, start, ks, dead, scalar, rows, strict, tag):
    """got, start: (NF, rows, sy) arrays of new or acc after and before the launch; scalar = a or w as the call received it."""
    t, (j0, j1) = c.t, rows
    eps = np.finfo(t).eps
    want = start.copy()
    R = (slice(H + j0, H + j1), slice(H, H + c.Nx))
    for k in ks:
        if k in dead:
            continue
        if strict:
            want[k][R] = RC.correct(start[k][R], c.strict(k)[j0:j1], scalar)
        else:
            E, S = c.exact(k)
            ref = start[k][R].astype(np.longdouble) + np.longdouble(t(scalar)) * E[j0:j1]
            err = np.abs(got[k][R].astype(np.longdouble) - ref)
            assert np.all(err <= RC.fast_bound(ref, t(scalar), S[j0:j1], eps)), (tag, k, float((err / (eps * (np.abs(ref) + S[j0:j1]))).max()))
            want[k][R] = got[k][R]
    # bitwise: the strict values, and everything the launch must not touch (halos, pad columns, rows outside, the rate == 0 field, the
    # fields without an acc, the fields beyond the list)
    u = np.uint64 if t == np.float64 else np.uint32
    assert np.array_equal(got.view(u), want.view(u)), tag


def _pitch(Nx, aligned):
    return (Nx + 2 * H + 1 + 3) // 4 * 4 if aligned else (Nx + 2 * H + 5) | 1


@pytest.mark.parametrize("pitch", ["aligned", "odd"])
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_stage_matrix(swmhd, sfx, strict, pitch):
    """Shapes x nfields in {1, 4, 12} (the six kinds mixed, distinct rates, the middle one 0 with its old full of NaN) x {no acc, w = 1
    for every field, w = dt / 4 with one acc[k] null} x row ranges {all, [1, Ny - 1), empty}; NaN in every halo cell and in every row
    outside the range of old, mask and target; the flags that mean nothing to the call alternate.  aligned: stride_y a multiple of four
    elements (the 16-byte path); odd: an odd stride_y (one element per lane)."""
    L = swmhd._lib
    t = NPDT[sfx]
    ft = ctypes.c_double if sfx == "f64" else ctypes.c_float
    fn = getattr(L.lib(), f"swmhd_relaxation_rk3_{sfx}")
    a = float(t(A_STAGE))
    extra = [0, L.WRAP_X | L.WRAP_Y, L.BOUNDED_X | L.BOUNDED_Y, L.WRAP_X | L.BOUNDED_Y]
    count = 0
    for Nx, Ny in RC.stage_shapes(np.dtype(t).itemsize, pitch == "aligned"):
        sy = _pitch(Nx, pitch == "aligned")
        c = Case(Nx, Ny, sy, t, 5)
        for n in RC.NFIELDS:
            dead = (n // 2,) if n > 1 else ()
            rate, tval, has_mask, has_target = c.call_tables(n, ft, dead)
            for rows in RC.row_ranges(Ny):
                old_d, mask_d, target_d = (torch.from_numpy(x).cuda() for x in c.inputs(rows, dead))
                for w, null_acc in ((None, None), (1.0, None), (float(t(DT_STAGE / 4)), n - 1)):
                    new_d, acc_d = torch.from_numpy(c.new).cuda(), torch.from_numpy(c.acc).cuda()
                    has_acc = [k != null_acc for k in range(n)]
                    flags = (L.STRICT if strict else 0) | extra[count % 4]
                    count += 1
                    rc = fn(ptrs(old_d, n), ptrs(new_d, n), ptrs(acc_d, n, has_acc) if w is not None else None, ptrs(mask_d, n, has_mask),
                            ptrs(target_d, n, has_target), ctypes.cast(rate, ctypes.c_void_p), ctypes.cast(tval, ctypes.c_void_p), n,
                            Nx, Ny, H, H, sy, a, w if w is not None else 0.0, rows[0], rows[1], flags, None)
                    L.check(rc, "swmhd_relaxation_rk3")
                    torch.cuda.synchronize()
                    tag = (Nx, Ny, n, w, rows)
                    check_outputs(c, new_d.cpu().numpy(), c.new, range(n), dead, a, rows, strict, ("new",) + tag)
                    accs = [k for k in range(n) if has_acc[k]] if w is not None else []
                    check_outputs(c, acc_d.cpu().numpy(), c.acc, accs, dead, w, rows, strict, ("acc",) + tag)


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_masks_and_targets_of_another_phase(swmhd, sfx):
    """Masks and targets one element further into their allocations than the fields, which have the pitch of the 16-byte path, take the
    one-element path; the same call with equal phases takes the 16-byte path.  Both are bitwise the restatement in strict, so bitwise
    equal, and the element in front of the shifted arrays is not touched."""
    L = swmhd._lib
    t = NPDT[sfx]
    ft = ctypes.c_double if sfx == "f64" else ctypes.c_float
    Nx, Ny, n = 129, 17, 6
    sy = _pitch(Nx, True)
    c = Case(Nx, Ny, sy, t, 9)
    rows = (0, Ny)
    rate, tval, has_mask, has_target = c.call_tables(n, ft)
    old, mask, target = c.inputs(rows)
    es = np.dtype(t).itemsize
    results = []
    for shift in (1, 0):
        old_d, new_d, acc_d = torch.from_numpy(old).cuda(), torch.from_numpy(c.new).cuda(), torch.from_numpy(c.acc).cuda()
        flats = []
        for src in (mask, target):
            flat = torch.full((src.size + 1,), RC.SENTINEL, dtype=old_d.dtype, device="cuda")
            flat[shift:shift + src.size].copy_(torch.from_numpy(src).reshape(-1))
            flats.append(flat)
        at = lambda flat, present: (ctypes.c_void_p * n)(*[flat.data_ptr() + (shift + k * mask[0].size) * es if present[k] else None for k in range(n)])
        rc = getattr(L.lib(), f"swmhd_relaxation_rk3_{sfx}")(
            ptrs(old_d, n), ptrs(new_d, n), ptrs(acc_d, n), at(flats[0], has_mask), at(flats[1], has_target), ctypes.cast(rate, ctypes.c_void_p),
            ctypes.cast(tval, ctypes.c_void_p), n, Nx, Ny, H, H, sy, float(t(A_STAGE)), 1.0, 0, Ny, L.STRICT, None)
        L.check(rc, "swmhd_relaxation_rk3")
        torch.cuda.synchronize()
        for flat in flats:
            assert flat[0 if shift else -1].item() == RC.SENTINEL
        got = new_d.cpu().numpy(), acc_d.cpu().numpy()
        check_outputs(c, got[0], c.new, range(n), (), float(t(A_STAGE)), rows, True, ("new", shift))
        check_outputs(c, got[1], c.acc, range(n), (), 1.0, rows, True, ("acc", shift))
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
    """Three fields in one call: field 0 without a mask and with a scalar target per member (the device table), field 1 with the
    SHARED mask (member stride 0) and a target array per member, field 2 with the shared mask and the default target; per-member rates
    (zeros among them) in the device table; stride_m pitched with the sentinel in the gap.  dt: one for all (params NULL; w = 1), and
    per member from the (g, f, dt) table, each with w = 1 and with SWMHD_RK3_ANCHOR (with the table w = 1/4 of each member's dt, without it w
    as given).  Strict: member m is bitwise
    the single-grid call with its own rate, tval and a = dt_m gamma formed in the element type as the kernel forms it.  Fast: member m
    is held to the derived bound of the single-grid stage matrix -- two instantiations need not contract alike."""
    L = swmhd._lib
    t = NPDT[sfx]
    for name, geo in ENS_GEOMETRIES.items():
        for strict in (True, False):
            _ensemble_abi_case(L, sfx, t, members, name, geo, strict)


# the targets' member pitch ALONE breaks the phase: stride_y and stride_m multiples of four elements, an odd target_stride_m -- one element
# per lane, two strips of 64 columns, one row block
TARGET_PITCH_GEOMETRY = dict(Nx={"f64": 65, "f32": 65}, Ny=17, sy={"f64": 72, "f32": 72}, gap=8, target_gap=9, vec=False)


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_ensemble_target_pitch_alone_takes_the_element_path(swmhd, sfx):
    """Two members of 65 x 17 whose parents would take the 16-byte path and whose target arrays lie an odd number of elements apart:
    the assertions of test_ensemble_members_are_single_grid_calls -- bitwise the per-member single-grid calls in strict, the sentinels
    in the gaps untouched."""
    geo = TARGET_PITCH_GEOMETRY
    size = (geo["Ny"] + 2 * H) * geo["sy"][sfx]
    assert geo["sy"][sfx] % 4 == 0 and (size + geo["gap"]) % 4 == 0 and (size + geo["target_gap"]) % 2 == 1
    for strict in (True, False):
        _ensemble_abi_case(swmhd._lib, sfx, NPDT[sfx], 2, "target-elem", geo, strict)


def _ensemble_abi_case(L, sfx, t, members, name, geo, strict):
    Nx, Ny, n = geo["Nx"][sfx], geo["Ny"], 3
    sy = geo["sy"][sfx]
    size = (Ny + 2 * H) * sy
    stride_m = size + geo["gap"]
    target_stride_m = size + geo.get("target_gap", geo["gap"])
    V = 16 // np.dtype(t).itemsize
    assert (sy % V == 0 and stride_m % V == 0 and target_stride_m % V == 0) == geo["vec"]
    ft = ctypes.c_double if sfx == "f64" else ctypes.c_float
    cases = [Case(Nx, Ny, sy, t, 20 + m) for m in range(members)]
    kinds = [(False, "scalar"), (True, "array"), (True, "zero")]
    rates = np.array([[0.31 * (m + 1) + 0.07 * k if (m + k) % 4 != 1 else 0.0 for k in range(n)] for m in range(members)], dtype=t)
    tvals = np.array([[0.9 - 0.4 * m if k == 0 else (TVAL_UNUSED if k == 1 else 0.0) for k in range(n)] for m in range(members)], dtype=t)
    for m, c in enumerate(cases):      # the references of check_outputs take the member's values of the tables and the shared mask
        c.kind[:n] = kinds
        c.rate[:n] = [float(x) for x in rates[m]]
        c.tval[:n] = [float(x) for x in tvals[m]]
        c.mask = cases[0].mask
    dts = np.array([0.013 * (1 + 0.5 * m) for m in range(members)], dtype=t)
    gamma = t(0.37)
    params = np.stack([np.full(members, 9.81), np.ones(members), dts], axis=1).astype(t)
    single = getattr(L.lib(), f"swmhd_relaxation_rk3_{sfx}")
    ens = getattr(L.lib(), f"swmhd_ensemble_relaxation_rk3_{sfx}")
    flags = (L.STRICT if strict else 0) | L.WRAP_X | L.WRAP_Y
    has_mask, has_target = [k[0] for k in kinds], [k[1] == "array" for k in kinds]
    u = np.uint64 if sfx == "f64" else np.uint32
    V_ = ctypes.c_void_p

    def pack(arrs, fill, pitch=stride_m):        # (n, members * pitch): field k of member m at [k, m * pitch:]
        out = np.full((n, members * pitch), fill, dtype=t)
        for m, a in enumerate(arrs):
            out[:, m * pitch:m * pitch + size] = a[:n].reshape(n, size)
        return torch.from_numpy(out).cuda()

    def run_ensemble(par, w, anchor, rows):
        ins = [c.inputs(rows, [k for k in range(n) if rates[m, k] == 0]) for m, c in enumerate(cases)]
        old_d, target_d = pack([i[0] for i in ins], np.nan), pack([i[2] for i in ins], np.nan, target_stride_m)
        mask_d = torch.from_numpy(ins[0][1][:n]).cuda()      # one mask set for all members
        new_d, acc_d = pack([c.new for c in cases], RC.SENTINEL), pack([c.acc for c in cases], RC.SENTINEL)
        rate_d, tval_d, par_d = torch.from_numpy(rates).cuda(), torch.from_numpy(tvals).cuda(), torch.from_numpy(params).cuda()
        rc = ens(ptrs(old_d, n), ptrs(new_d, n), ptrs(acc_d, n), ptrs(mask_d, n, has_mask), ptrs(target_d, n, has_target), rate_d.data_ptr(),
                 tval_d.data_ptr(), n, members, stride_m, 0, target_stride_m, Nx, Ny, H, H, sy, par_d.data_ptr() if par else None,
                 float(gamma) if par else float(dts[0] * gamma), w, rows[0], rows[1], flags | (L.RK3_ANCHOR if anchor else 0), None)
        L.check(rc, "swmhd_ensemble_relaxation_rk3")
        torch.cuda.synchronize()
        return new_d.cpu().numpy(), acc_d.cpu().numpy()

    def run_single(m, a, w, rows):
        c = cases[m]
        dead = [k for k in range(n) if rates[m, k] == 0]
        old_d, mask_d, target_d = (torch.from_numpy(x).cuda() for x in c.inputs(rows, dead))
        new_d, acc_d = torch.from_numpy(c.new).cuda(), torch.from_numpy(c.acc).cuda()
        rc = single(ptrs(old_d, n), ptrs(new_d, n), ptrs(acc_d, n), ptrs(mask_d, n, has_mask), ptrs(target_d, n, has_target),
                    ctypes.cast((ft * n)(*[float(x) for x in rates[m]]), V_), ctypes.cast((ft * n)(*[float(x) for x in tvals[m]]), V_), n,
                    Nx, Ny, H, H, sy, a, w, rows[0], rows[1], flags, None)
        L.check(rc, "swmhd_relaxation_rk3")
        torch.cuda.synchronize()
        return new_d.cpu().numpy()[:n].reshape(n, size), acc_d.cpu().numpy()[:n].reshape(n, size)

    quarter = t(0.25)
    for rows in ((0, Ny), (1, Ny - 1)):
        # params NULL with SWMHD_RK3_ANCHOR: the flag is accepted and w is used as given, there is no dt to scale it with
        for par, w, anchor in ((False, 1.0, False), (False, float(dts[0] * quarter), True), (True, 1.0, False), (True, float(quarter), True)):
            got_new, got_acc = run_ensemble(par, w, anchor, rows)
            for m in range(members):
                tag = (name, strict, rows, par, anchor, m)
                a_m = float((dts[m] if par else dts[0]) * gamma)
                w_m = float(dts[m] * quarter) if (anchor and par) else w
                lo = m * stride_m
                mine = [g[:, lo:lo + size] for g in (got_new, got_acc)]
                assert np.all(got_new[:, lo + size:lo + stride_m] == RC.SENTINEL) and np.all(got_acc[:, lo + size:lo + stride_m] == RC.SENTINEL), tag
                dead = [k for k in range(n) if rates[m, k] == 0]
                if strict:
                    one_new, one_acc = run_single(m, a_m, w_m, rows)
                    assert np.array_equal(mine[0].view(u), one_new.view(u)), tag
                    assert np.array_equal(mine[1].view(u), one_acc.view(u)), tag
                    for k in dead:        # a zero of the device table: that field of that member is untouched
                        assert np.array_equal(one_new[k].view(u), cases[m].new[k].reshape(-1).view(u))
                for got, start, scalar, what in ((mine[0], cases[m].new, a_m, "new"), (mine[1], cases[m].acc, w_m, "acc")):
                    full = start.copy()
                    full[:n] = got.reshape(n, Ny + 2 * H, sy)
                    check_outputs(cases[m], full, start, range(n), dead, scalar, rows, strict, (what,) + tag)


# ----------------------------------------------------------------------------------------------------------------------------------
# whole runs
# ----------------------------------------------------------------------------------------------------------------------------------
DT, STEPS = 2e-3, 10
RUN_GRIDS = [(48, 40), (64, 64)]
P, B = TC.P, TC.B
_reference = {}


def _grid(S, Nx, Ny, topo=(P, P)):
    names = {P: "Periodic", B: "Bounded"}
    return S.RectilinearGrid(size=(Nx, Ny), x=(0, TC.DX * Nx), y=(0, TC.DY * Ny), topology=(names[topo[0]], names[topo[1]], "Flat"))


def _sponge(x, y, Ly):
    return np.exp(-(y / (0.2 * Ly)) ** 2) + np.exp(-((y - Ly) / (0.2 * Ly)) ** 2) + 0 * x


def _h_eq(x, y, Lx, Ly):
    return 1.0 + 0.05 * np.cos(2 * np.pi * x / Lx) * np.sin(2 * np.pi * y / Ly)


def _forcing(S, g, names, tracers=True):
    """Drag on the first momentum-like field, a sponge (mask, target 0) on the second, h towards h_eq(x, y) (a target array), A with a
    mask array and a scalar target, tracer c with a callable mask and a scalar target, d left alone."""
    Lx, Ly = g.Lx, g.Ly
    rng = np.random.default_rng(3)
    f = {names[0]: S.Relaxation(0.9), names[1]: S.Relaxation(2.0, mask=lambda x, y: _sponge(x, y, Ly)),
         "h": S.Relaxation(0.7, target=lambda x, y: _h_eq(x, y, Lx, Ly)),
         "A": S.Relaxation(1.1, mask=rng.random((g.Ny, g.Nx)), target=0.05)}
    if tracers:
        f["c"] = S.Relaxation(0.6, mask=lambda x, y: _sponge(x, y, Ly), target=-0.2)
    return f


def _relax_list(g, tracers=True):
    """The forcing of _forcing as RefModel takes it, the callables evaluated here on the grid's nodes at every field's location."""
    I = (slice(H, H + g.Ny), slice(H, H + g.Nx))
    xc, xf, yc, yf = g.xc[I[1]][None, :], g.xf[I[1]][None, :], g.yc[I[0]][:, None], g.yf[I[0]][:, None]
    rng = np.random.default_rng(3)
    out = [(0.9, None, 0.0), (2.0, _sponge(xc, yf, g.Ly), 0.0), (0.7, None, _h_eq(xc, yc, g.Lx, g.Ly)), (1.1, rng.random((g.Ny, g.Nx)), 0.05)]
    return out + ([(0.6, _sponge(xc, yc, g.Ly), -0.2), None] if tracers else [])


def _start(O, Nx, Ny, form, topo=(P, P)):
    q = TC.fill_state(O, TC.state(Nx, Ny, form, 11, rough=False), Nx, Ny, topo, TC.grad_A(topo))
    d = TC.fill(O, TC.tracer_fields(Nx, Ny, 2, 11, rough=False)[1], Nx, Ny, topo)
    return q, d


def _model(S, O, Nx, Ny, form, strict=True, forcing="default", tracers=("c", "d"), **kw):
    g = _grid(S, Nx, Ny)
    q, d = _start(O, Nx, Ny, form)
    names = ("u", "v") if form == 1 else ("uh", "vh")
    if forcing != "absent":
        kw["forcing"] = _forcing(S, g, names, bool(tracers)) if forcing == "default" else forcing
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
        r = RC.RefModel(O, q, [q[3], d], _relax_list(g), Nx, Ny, form, lor, "classic", dx=g.dx, dy=g.dy)
        for _ in range(STEPS):
            r.step(DT)
        _reference[key] = r
    return _reference[key]


@pytest.mark.parametrize("how", ["eager", "graph", "checkpoint"])
@pytest.mark.parametrize("form,lor", TC.FORMS)
@pytest.mark.parametrize("Nx,Ny", RUN_GRIDS)
def test_strict_runs_are_the_reference(swmhd, oracle, tmp_path, Nx, Ny, form, lor, how):
    """Strict model with five of the six field kinds on u|uh, v|vh, h, A and c, 10 steps: every field bitwise the reference stepper,
    halos included -- stepped eagerly; through capture_graph with time_steps(5) twice, so that the second call starts on swapped roles
    (one eager step, then replays); and across a save_checkpoint / load_checkpoint at step 5 (the forcing is the constructor's)."""
    S, O = swmhd, oracle
    m = _model(S, O, Nx, Ny, form)
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
    and the forcing has moved every forced field by far more than that."""
    S, O = swmhd, oracle
    m = _model(S, O, Nx, Ny, form, strict=False)
    plain = _model(S, O, Nx, Ny, form, strict=False, forcing=None)
    m.time_steps(STEPS, DT)
    plain.time_steps(STEPS, DT)
    m.synchronize(); plain.synchronize()
    ref = _ref(S, O, Nx, Ny, form, lor)
    for name, f, a in zip(list(m.names) + ["c", "d"], m.fields + [m.tracers["c"], m.tracers["d"]], ref.q + ref.tr):
        err = np.abs(f.numpy() - a).max() / np.abs(a).max()
        print(f"fast vs strict {Nx}x{Ny} form {form} {name}: {err:.3e}")
        assert err <= 1e-12
    for f, a in zip(plain.fields + [plain.tracers["c"]], ref.q + ref.tr[:1]):
        assert np.abs(f.numpy() - a).max() > 1e-6 * np.abs(a).max()


def test_all_four_correction_launches_in_their_order(swmhd, oracle):
    """BetaPlane, ScalarDiffusivity, ScalarBiharmonicDiffusivity and the forcing on one strict model: bitwise the reference stepper that
    applies the four corrections in the order Coriolis, Laplacian, biharmonic, relaxation -- and not bitwise one that relaxes first."""
    import coriolis_cases  # noqa: F401  (RefModel's Coriolis restatement)
    S, O = swmhd, oracle
    Nx, Ny, form, lor = 48, 40, 1, 1
    g = _grid(S, Nx, Ny)
    beta = S.BetaPlane(1.0, 0.3)
    NU, ETA, NU4, ETA4 = 3e-3, 5e-3, 2e-5, 3e-5
    closure = (S.ScalarDiffusivity(nu=NU, kappa={"A": ETA, "c": ETA}), S.ScalarBiharmonicDiffusivity(nu=NU4, kappa={"A": ETA4}))
    m = _model(S, O, Nx, Ny, form, coriolis=beta, closure=closure)
    tr = Transcript()
    tr.watch(m)
    tr.do("steps", lambda: [m.time_step(DT) for _ in range(4)])
    m.synchronize()
    names = [c[0] for c in tr.blocks[0][1]]
    assert names == ["swmhd_tendencies_rk3_f64", "swmhd_tracers_rk3_f64", "swmhd_coriolis_rk3_f64", "swmhd_diffusion_rk3_f64",
                     "swmhd_biharmonic_rk3_f64", "swmhd_relaxation_rk3_f64"] * 12, names
    q, d = _start(O, Nx, Ny, form)
    r = RC.RefModel(O, q, [q[3], d], _relax_list(g), Nx, Ny, form, lor, "classic", dx=g.dx, dy=g.dy, rows=beta.rows(g),
                    coef=[NU, NU, 0.0, ETA, ETA, 0.0], coef4=[NU4, NU4, 0.0, ETA4, 0.0, 0.0])
    for _ in range(4):
        r.step(DT)
    for f, a in zip(m.fields + [m.tracers["c"], m.tracers["d"]], r.q + r.tr):
        assert np.array_equal(f.numpy(), a)

    class RelaxFirst(RC.RefModel):
        def _D(self, U):
            return [ds[-1:] + ds[:-1] for ds in super()._D(U)]
    w = RelaxFirst(O, q, [q[3], d], _relax_list(g), Nx, Ny, form, lor, "classic", dx=g.dx, dy=g.dy, rows=beta.rows(g),
                   coef=[NU, NU, 0.0, ETA, ETA, 0.0], coef4=[NU4, NU4, 0.0, ETA4, 0.0, 0.0])
    for _ in range(4):
        w.step(DT)
    assert not np.array_equal(w.q[0], r.q[0])      # the order decides the last bits, so the test above pins it


# ---- the Bounded channel --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,lor", TC.FORMS)
def test_sponge_layers_in_a_bounded_channel(swmhd, oracle, form, lor):
    """(Periodic, Bounded) strict model, gradient conditions on A, a sponge mask on v|vh and on h (towards 1): bitwise the reference
    stepper built from the oracle's Bounded step plus the restated correction, halos included; the wall line of v stays what the fill
    makes it -- that of the same run without forcing."""
    S, O = swmhd, oracle
    Nx, Ny, topo = 48, 40, (P, B)
    g = _grid(S, Nx, Ny, topo)
    bcs = {"A": S.FieldBoundaryConditions(north=S.GradientBoundaryCondition(-0.05), south=S.GradientBoundaryCondition(-0.05))}
    n2 = "v" if form == 1 else "vh"
    sponge = lambda x, y: _sponge(x, y, g.Ly)
    models = {}
    for key, forcing in (("forced", {n2: S.Relaxation(3.0, mask=sponge), "h": S.Relaxation(1.5, mask=sponge, target=1.0)}), ("plain", None)):
        m = S.ShallowWaterModel(g, TC.GRAV, TC.FCOR, formulation=TC.FORM_NAME[form], strict=True, boundary_conditions=bcs, forcing=forcing)
        q = TC.fill_state(O, TC.state(Nx, Ny, form, 11, rough=False), Nx, Ny, topo, TC.grad_A(topo), g.dx, g.dy)
        for f, a in zip(m.fields, q):
            f.data.copy_(torch.from_numpy(a))
        for _ in range(STEPS):
            m.time_step(DT)
        m.synchronize()
        models[key] = m
    I = (slice(H, H + Ny), slice(H, H + Nx))
    xc, yc, yf = g.xc[I[1]][None, :], g.yc[I[0]][:, None], g.yf[I[0]][:, None]
    relax = [None, (3.0, _sponge(xc, yf, g.Ly), 0.0), (1.5, _sponge(xc, yc, g.Ly), 1.0), None]
    r = RC.RefModel(O, q, [], relax, Nx, Ny, form, lor, "classic", topo, TC.grad_A(topo), g.dx, g.dy)
    for _ in range(STEPS):
        r.step(DT)
    for f, a in zip(models["forced"].fields, r.q):
        assert np.array_equal(f.numpy(), a)
    v, v0 = models["forced"].fields[1].numpy(), models["plain"].fields[1].numpy()
    assert np.array_equal(v[H], v0[H]) and np.array_equal(v[H + Ny], v0[H + Ny])      # the south wall line and its northern image
    assert np.abs(v[I] - v0[I]).max() > 1e-6 * np.abs(v0).max()


# ---- unchanged calls ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
def test_without_rates_nothing_changes(swmhd, oracle, strict):
    """forcing absent, None, {} and rates that are all 0: the ctypes calls of time_step and time_steps, argument by argument, and the
    state are those of a model built without the argument."""
    S, O = swmhd, oracle
    out = []
    zero = {"u": S.Relaxation(0.0, mask=np.ones((40, 48)), target=3.0), "h": S.Relaxation(0.0)}
    for forcing in ("absent", None, {}, zero):
        for tracers in ((), ("c", "d")):
            m = _model(S, O, 48, 40, 1, strict=strict, forcing=forcing, tracers=tracers)
            assert m._relaxation is None
            tr = Transcript()
            tr.watch(m)
            tr.do("time_step", m.time_step, DT)
            tr.do("time_steps", m.time_steps, 3, DT)
            m.synchronize()
            out.append((bool(tracers), tr.blocks, [f.numpy() for f in m.fields]))
    for with_tracers in (False, True):
        same = [o for o in out if o[0] == with_tracers]
        assert len(same) == 4
        for o in same[1:]:
            assert o[1] == same[0][1]
            assert all(np.array_equal(x, y) for x, y in zip(o[2], same[0][2]))
    names = [c[0] for _, calls in out[0][1] for c in calls]
    assert not any("relaxation" in n for n in names) and names


def test_the_forcing_adds_one_launch_per_stage(swmhd, oracle):
    S, O = swmhd, oracle
    for strict in (True, False):
        m = _model(S, O, 48, 40, 1, strict=strict, closure=S.ScalarDiffusivity(kappa={"A": 5e-3}))
        tr = Transcript()
        tr.watch(m)
        tr.do("step", m.time_steps, 2, DT)
        names = [c[0] for c in tr.blocks[0][1]]
        assert names == ["swmhd_tendencies_rk3_f64", "swmhd_tracers_rk3_f64", "swmhd_diffusion_rk3_f64", "swmhd_relaxation_rk3_f64"] * 6, names
        calls = [c for c in tr.blocks[0][1] if c[0] == "swmhd_relaxation_rk3_f64"]
        # u, v, h, A, c; an operand in storing stages only: stages 0, 1 (classic) or stage 0 (anchor)
        assert [c[8] for c in calls] == [5] * 6
        assert [c[3] != "null" for c in calls] == ([True, True, False] if strict else [True, False, False]) * 2
        # masks of v, A, c; a target array of h alone
        assert [[p != "null" for p in c[4]] for c in calls] == [[False, True, False, True, True]] * 6
        assert [[p != "null" for p in c[5]] for c in calls] == [[False, False, True, False, False]] * 6
        m.synchronize()


# ---- decay ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
@pytest.mark.parametrize("which", ["drag", "thermal"])
def test_rk3_property_on_the_device(swmhd, oracle, which, strict):
    """Uniform fields, f = 0, A = 0 on 8 x 8, 20 steps: u (drag) or h - H_eq (thermal relaxation) is P(-r dt)^20 of its start within the
    margin the CPU reference sets (ten times its own deviation, relaxation_cases.DECAY_MARGIN), the fast run like the strict one."""
    S = swmhd
    q, relax = RC.decay_case(which)
    Nx, Ny = RC.DECAY_NX, RC.DECAY_NY
    g = S.RectilinearGrid(size=(Nx, Ny), x=(0, RC.DX * Nx), y=(0, RC.DY * Ny))
    forcing = {"u": S.Relaxation(RC.DECAY_RATE)} if which == "drag" else {"h": S.Relaxation(RC.DECAY_RATE, target=RC.DECAY_HEQ)}
    m = S.ShallowWaterModel(g, TC.GRAV, 0.0, strict=strict, forcing=forcing)
    for f, a in zip(m.fields, q):
        f.data.copy_(torch.from_numpy(a))
    for _ in range(RC.DECAY_STEPS):
        m.time_step(RC.DECAY_DT)
    m.synchronize()
    k = 0 if which == "drag" else 2
    dev = RC.decay_deviation(which, m.fields[k].numpy())
    margin = RC.DECAY_MARGIN[which]
    print(f"{which} on the device ({'strict' if strict else 'fast'}): relative deviation {dev:.3e}, margin {margin:.3e}")
    assert dev <= margin
    for j, (f, a) in enumerate(zip(m.fields, q)):
        if j != k:
            assert np.array_equal(f.numpy(), a)


# ---- ensembles ------------------------------------------------------------------------------------------------------------------------
def _ensemble(S, O, strict, dts=None):
    Nx, Ny, Bm = 48, 40, 3
    g = _grid(S, Nx, Ny)
    rng = np.random.default_rng(8)
    forcing = {"u": S.Relaxation([0.9, 0.0, 1.8]), "v": S.Relaxation(2.0, mask=lambda x, y: _sponge(x, y, g.Ly)),
               "h": S.Relaxation([0.7, 0.7, 0.0], target=1.0 + 0.05 * rng.standard_normal((Bm, Ny, Nx))),
               "c": S.Relaxation(0.6, target=[-0.2, 0.0, 0.3])}
    e = S.ShallowWaterEnsemble(g, Bm, TC.GRAV, [1.0, 0.5, 2.0] if dts is not None else TC.FCOR, strict=strict, tracers=("c",), forcing=forcing,
                               member_stride=(Ny + 6) * (Nx + 6) + 10)
    q, d = _start(O, Nx, Ny, 1)
    for t_, a in zip(e._state + [e._tr["c"]], q + [d]):
        for m in range(Bm):
            t_[m].copy_(torch.from_numpy(a * (1.0 + 0.1 * m)))
    return e, forcing


@pytest.mark.parametrize("per_member_dt", [False, True], ids=["dt", "dts"])
def test_ensemble_members_are_models(swmhd, oracle, per_member_dt):
    """Strict ensemble of three members with per-member rates (zeros among them), a shared mask, per-member target arrays and scalar
    targets, and a scalar or per-member dt, 4 steps: member m is bitwise ShallowWaterModel(forcing=that member's) stepped alone, and
    member(1) taken after 2 steps and stepped 2 more alone is bitwise member 1 of the ensemble.  The ensemble adds one launch per stage.
    The fast ensemble (anchor form; with per-member dt the kernel forms dt_m / 4) stays within 1e-12."""
    S, O = swmhd, oracle
    dts = [DT, 1.5 * DT, 0.5 * DT] if per_member_dt else None
    dt = dts if per_member_dt else DT
    e, forcing = _ensemble(S, O, True, dts)
    assert tuple(e.relaxation_rates.shape) == (3, 4) and e._mask_stride == 0 and e._target_stride == 46 * 54
    start = [[t_[m].clone() for t_ in e._state + [e._tr["c"]]] for m in range(3)]
    tr = Transcript()
    tr.watch(e)
    tr.do("steps", e.time_steps, 2, dt)
    sfx = "params_f64" if per_member_dt else "f64"
    assert [c[0] for c in tr.blocks[0][1]] == [f"swmhd_ensemble_tendencies_rk3_{sfx}", f"swmhd_ensemble_tracers_rk3_{sfx}",
                                               "swmhd_ensemble_relaxation_rk3_f64"] * 6
    one = e.member(1)
    assert one.forcing["u"].rate == 0.0 and one.forcing["c"].target == 0.0 and one.forcing["h"].target.shape == (40, 48)
    e.time_steps(2, dt)
    one.time_steps(2, dts[1] if per_member_dt else DT)
    e.synchronize(); one.synchronize()
    for f, t_ in zip(one.fields + [one.tracers["c"]], e.fields + [e.tracers["c"]]):
        assert torch.equal(f.data, t_[1])
    for m in range(3):
        alone = e._member_model(m)
        assert alone.forcing["u"].rate == forcing["u"].rate[m]
        for f, a in zip(alone._raw_fields + [alone._tr["c"]], start[m]):
            f.data.copy_(a)
        for _ in range(4):
            alone.time_step(dts[m] if per_member_dt else DT)
        alone.synchronize()
        for f, t_ in zip(alone.fields + [alone.tracers["c"]], e.fields + [e.tracers["c"]]):
            assert torch.equal(f.data, t_[m]), m
    fast, _ = _ensemble(S, O, False, dts)
    fast.time_steps(4, dt)
    fast.synchronize()
    for a, b in zip(fast.fields + [fast.tracers["c"]], e.fields + [e.tracers["c"]]):
        assert ((a - b).abs().amax() <= 1e-12 * b.abs().amax()).item()


def test_ensemble_graph_replay_and_no_forcing_calls(swmhd, oracle):
    S, O = swmhd, oracle
    e, _ = _ensemble(S, O, False)
    g, _ = _ensemble(S, O, False)
    e.time_steps(5, DT)
    g.capture_graph(DT)
    g.time_steps(5, DT)
    e.synchronize(); g.synchronize()
    for a, b in zip(e.fields + [e.tracers["c"]], g.fields + [g.tracers["c"]]):
        assert torch.equal(a, b)
    grid = e.grid
    logs = []
    for kw in ({}, {"forcing": None}, {"forcing": {}}, {"forcing": {"u": S.Relaxation([0.0, 0.0])}}):
        p = S.ShallowWaterEnsemble(grid, 2, **kw)
        tr = Transcript()
        tr.watch(p)
        tr.do("steps", p.time_steps, 2, DT)
        p.synchronize()
        logs.append(tr.blocks)
    assert logs[0] == logs[1] == logs[2] == logs[3] and [c[0] for c in logs[0][0][1]] == ["swmhd_ensemble_step_rk3_f64"]


# ---- the example ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [["--drag", "0.05"], ["--channel", "--gradients", "-0.01", "--sponge", "0.5,0.3"]], ids=["drag", "sponge"])
def test_example_runs_with_a_forcing(tmp_path, extra):
    """examples/run_swmhd.py --drag 0.05, and --channel --gradients -0.01 --sponge 0.5,0.3, on 64^2 for a few steps: the progress lines,
    the dump and its fields exist and are finite."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "examples", "run_swmhd.py"), "--size", "64", "--stop-time", "0.1", "--every", "5",
           "--dump-every", "0.1", "--out", str(tmp_path)] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Relaxation" in r.stdout
    assert len([l for l in r.stdout.splitlines() if l.startswith("Time:")]) >= 2
    z = np.load(os.path.join(str(tmp_path), "fields_0000010.npz"))
    for n in ("u", "v", "h", "A"):
        assert np.isfinite(z[n]).all()
