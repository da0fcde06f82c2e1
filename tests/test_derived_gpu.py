"""GPU tests of the derived frames (swmhd_derived_fields_*, swmhd_ensemble_derived_fields[_params]_*, derived_fields, and the four names in
FieldTimeSeries).

The yardstick is the numpy restatement in tests/derived_cases.py (pinned on the CPU by tests/test_derived_cases_cpu.py).  The object is
built without FMA contraction and with IEEE divide, so every comparison is BITWISE: float64 frames against the restatement, float32
frames against the restatement rounded to float32, NaN in the same places.  The frames are written into sentinel-filled buffers with
pitched strides, and every element the call does not own must still hold the sentinel afterwards."""
import ctypes
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

import derived_cases as DC
import output_cases as OC
from helpers import same_bits as _same      # bitwise: NaN in the same places, the same bits everywhere else
from output_cases import images as _images  # the periodic images the WRAP flags read, also for Nx < Hx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NP = {"f64": np.float64, "f32": np.float32}
TORCH = {"f64": torch.float64, "f32": torch.float32}
FORMS = {"VectorInvariant": 1, "Conservative": 0}
SENT = -777.25
DX, DY, FCOR = 0.1, 0.12, 0.7
WRAP_X, WRAP_Y = 16, 32


def _real(x, sfx):
    """a spacing or f as the kernel receives it (an f32 call passes floats through the C-ABI)"""
    return x if sfx == "f64" else float(np.float32(x))


def _parents(Nx, Ny, Hx, Hy, sfx, seed, wrap=0):
    """Four random parents in the model type.  Directions without wrap: the first halo ring holds values, every cell beyond it and the
    three corners of the ring that nothing reaches (all but (i-1, j-1)) hold NaN.  Wrapped directions: every halo cell holds NaN."""
    rng = np.random.default_rng(seed)
    shape = (Ny + 2 * Hy, Nx + 2 * Hx)
    q = [rng.standard_normal(shape), rng.standard_normal(shape), 1.0 + 0.3 * rng.random(shape), rng.standard_normal(shape)]
    keep = np.zeros(shape, dtype=bool)
    kx = slice(Hx, Hx + Nx) if wrap & WRAP_X else slice(Hx - 1, Hx + Nx + 1)
    ky = slice(Hy, Hy + Ny) if wrap & WRAP_Y else slice(Hy - 1, Hy + Ny + 1)
    keep[ky, kx] = True
    if not wrap & (WRAP_X | WRAP_Y):
        keep[Hy - 1, Hx + Nx] = keep[Hy + Ny, Hx - 1] = keep[Hy + Ny, Hx + Nx] = False
    return [np.where(keep, a, np.nan).astype(NP[sfx]) for a in q]


class Device:
    """Parents on the device with a pitched row stride (and, for ensembles, a pitched member stride), NaN in every gap"""

    def __init__(self, members_parents, Nx, Ny, Hx, Hy, sfx):
        self.Nx, self.Ny, self.Hx, self.Hy, self.sfx = Nx, Ny, Hx, Hy, sfx
        self.members = len(members_parents)
        Py, Px = Ny + 2 * Hy, Nx + 2 * Hx
        self.sy = Px + 5
        self.stride_m = Py * self.sy + 11
        self.t = []
        for k in range(4):
            host = np.full(self.members * self.stride_m, np.nan, dtype=NP[sfx])
            for m, q in enumerate(members_parents):
                host[m * self.stride_m:m * self.stride_m + Py * self.sy].reshape(Py, self.sy)[:, :Px] = q[k]
            self.t.append(torch.from_numpy(host).cuda())

    def ptrs(self, member=0):
        return [t.data_ptr() + member * self.stride_m * t.element_size() for t in self.t]


def _frame_call(S, dev, form, f, rows, which, out_sfx, flags, mode="single", member=0, params=None):
    """One call of swmhd_[ensemble_]derived_fields[_params]_* into a sentinel-filled buffer with pitched row, field and member strides.
    Returns the fields (members, nf, nrows, Nx) -- (nf, nrows, Nx) for a single grid -- after checking every other element for the sentinel."""
    L = S._lib.lib()
    j0, j1 = rows
    nrows, nf, Nx = j1 - j0, bin(which).count("1"), dev.Nx
    lead, osy = 7, Nx + 3
    osf = nrows * osy + 5
    osm = nf * osf + 9
    members = dev.members if mode != "single" else 1
    buf = torch.full((lead + members * osm + 7,), SENT, dtype=TORCH[out_sfx], device="cuda")
    optr = buf.data_ptr() + lead * buf.element_size()
    grid = (dev.Nx, dev.Ny, dev.Hx, dev.Hy, dev.sy, DX, DY, form)
    frame = (j0, j1, which, optr, buf.element_size(), osy, osf)
    stream = S.fields._stream_ptr()
    if mode == "single":
        rc = getattr(L, f"swmhd_derived_fields_{dev.sfx}")(*dev.ptrs(member), *grid, f, *frame, flags, stream)
    elif mode == "ensemble":
        rc = getattr(L, f"swmhd_ensemble_derived_fields_{dev.sfx}")(*dev.ptrs(), members, dev.stride_m, *grid, f, *frame, osm, flags, stream)
    else:
        rc = getattr(L, f"swmhd_ensemble_derived_fields_params_{dev.sfx}")(*dev.ptrs(), members, dev.stride_m, *grid, params.data_ptr(), *frame, osm,
                                                                          flags, stream)
    S._lib.check(rc, "swmhd_derived_fields")
    flat = buf.cpu().numpy()
    own = np.zeros(flat.shape, dtype=bool)
    idx = (lead + np.arange(members)[:, None, None, None] * osm + np.arange(nf)[None, :, None, None] * osf
           + np.arange(nrows)[None, None, :, None] * osy + np.arange(Nx)[None, None, None, :])
    own[idx.ravel()] = True
    assert (flat[~own] == SENT).all(), f"sentinel overwritten: which={which} rows={rows} {mode}"
    got = flat[idx]
    return got[0] if mode == "single" else got


# --- one grid: every shape, halo, formulation, precision, frame type, mask, row range and wrap -------------------------------------
@pytest.mark.parametrize("Hx,Hy", DC.HALOS, ids=[f"halo{hx}{hy}" for hx, hy in DC.HALOS])
@pytest.mark.parametrize("Nx,Ny", DC.SHAPES, ids=[f"{nx}x{ny}" for nx, ny in DC.SHAPES])
def test_frames_match_the_restatement_bitwise(swmhd, Nx, Ny, Hx, Hy):
    S = swmhd
    ranges = sorted(set(DC.ROW_RANGES(Ny)) | {(min(1, Ny), min(1, Ny))})          # ... and an empty range, which writes nothing
    for sfx in ("f64", "f32"):
        dx, dy, f = _real(DX, sfx), _real(DY, sfx), _real(FCOR, sfx)
        for wrap in (0, WRAP_X, WRAP_Y, WRAP_X | WRAP_Y):
            q = _parents(Nx, Ny, Hx, Hy, sfx, 100 * Nx + Ny + wrap, wrap)
            ref = _images(q, Nx, Ny, Hx, Hy, wrap)
            dev = Device([q], Nx, Ny, Hx, Hy, sfx)
            for form in (1, 0):
                want = DC.np_derived_fields(*ref, Nx, Ny, Hx, Hy, dx, dy, f, form)
                assert np.isfinite(want).all(), "the restatement reached a NaN halo cell"
                for j0, j1 in ranges:
                    part = DC.np_derived_fields(*ref, Nx, Ny, Hx, Hy, dx, dy, f, form, rows=(j0, j1))
                    assert np.array_equal(part, want[:, j0:j1])
                    for which in DC.MASKS:
                        sel = [k for k in range(4) if which >> k & 1]
                        for out_sfx in ("f32", "f64"):
                            got = _frame_call(S, dev, form, FCOR, (j0, j1), which, out_sfx, wrap)
                            _same(got, part[sel], f"{Nx}x{Ny} halo {Hx},{Hy} {sfx} form {form} wrap {wrap} rows {j0}:{j1} mask {which} -> {out_sfx}")


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_a_nan_in_one_cell_of_one_parent(swmhd, sfx):
    """One NaN in an interior cell of each parent in turn: the NaN set of every field is the restatement's (the cells that read it)."""
    S = swmhd
    Nx, Ny, Hx, Hy = 7, 9, 3, 2
    dx, dy, f = _real(DX, sfx), _real(DY, sfx), _real(FCOR, sfx)
    for wrap, cell in ((0, (3, 4)), (WRAP_X | WRAP_Y, (0, 0)), (WRAP_X | WRAP_Y, (Ny - 1, Nx - 1)), (0, (Ny - 1, 0))):
        for k in range(4):
            q = _parents(Nx, Ny, Hx, Hy, sfx, 77, wrap)
            q[k][Hy + cell[0], Hx + cell[1]] = np.nan
            ref = _images(q, Nx, Ny, Hx, Hy, wrap)
            dev = Device([q], Nx, Ny, Hx, Hy, sfx)
            for form in (1, 0):
                want = DC.np_derived_fields(*ref, Nx, Ny, Hx, Hy, dx, dy, f, form)
                counts = np.isnan(want).sum(axis=(1, 2))
                print("parent", k, "cell", cell, "wrap", wrap, "form", form, "NaN per field", counts.tolist())
                assert counts.sum() > 0 and not np.isnan(want).all()
                if form == 1:      # vector-invariant: u, v reach vorticity, divergence and q; A the current alone; h the q alone
                    assert [c > 0 for c in counts] == [[True, True, False, True], [True, True, False, True], [False, False, False, True],
                                                       [False, False, True, False]][k]
                _same(_frame_call(S, dev, form, FCOR, (0, Ny), DC.ALL, "f64", wrap), want, f"NaN in parent {k} at {cell}, wrap {wrap}, form {form}")
                _same(_frame_call(S, dev, form, FCOR, (0, Ny), DC.ALL, "f32", wrap), want, f"NaN in parent {k} at {cell}, wrap {wrap}, form {form}, f32")


def test_a_non_finite_f_reaches_the_potential_vorticity_alone(swmhd):
    S = swmhd
    Nx, Ny, Hx, Hy = 5, 2, 1, 1
    q = _parents(Nx, Ny, Hx, Hy, "f64", 5)
    dev = Device([q], Nx, Ny, Hx, Hy, "f64")
    clean = _frame_call(S, dev, 1, FCOR, (0, Ny), DC.ALL, "f64", 0)
    for bad in (float("nan"), float("inf")):
        got = _frame_call(S, dev, 1, bad, (0, Ny), DC.ALL, "f64", 0)
        _same(got[:3], clean[:3], "the fields without f")
        _same(got, DC.np_derived_fields(*q, Nx, Ny, Hx, Hy, DX, DY, bad, 1), f"f = {bad}")
        assert not np.isfinite(got[3]).any()


# --- ensembles ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("members", [1, 3])
@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("Nx,Ny", [(5, 2), (65, 3)])
def test_ensemble_calls_are_the_single_call_per_member(swmhd, Nx, Ny, sfx, members):
    """Pitched stride_m and out_stride_m, a sentinel in every gap: each member of the scalar form is bitwise the single call; the _params
    form is bitwise the scalar call made per member with that member's f (three distinct values; the g and dt columns hold NaN and
    are not read); a member full of NaN leaves the others alone."""
    S = swmhd
    Hx, Hy = 3, 2
    fs = [0.3, -1.1, 2.5][:members]
    for wrap in (0, WRAP_X | WRAP_Y):
        qs = [_parents(Nx, Ny, Hx, Hy, sfx, 31 + m, wrap) for m in range(members)]
        dev = Device(qs, Nx, Ny, Hx, Hy, sfx)
        table = torch.tensor([[float("nan"), fm, float("nan")] for fm in fs], dtype=TORCH[sfx], device="cuda")
        dirty = [[a.copy() for a in q] for q in qs]
        if members > 1:
            for a in dirty[1]:
                a[:] = np.nan
        dev_dirty = Device(dirty, Nx, Ny, Hx, Hy, sfx)
        for form in (1, 0):
            for which, rows, out_sfx in ((DC.ALL, (0, Ny), "f64"), (DC.ALL, (0, Ny), "f32"), (1 | 4, (1, Ny), "f32"), (8, (0, 1), "f64")):
                tag = f"{Nx}x{Ny} {sfx} members {members} wrap {wrap} form {form} mask {which} rows {rows} -> {out_sfx}"
                sel = [k for k in range(4) if which >> k & 1]
                ens = _frame_call(S, dev, form, FCOR, rows, which, out_sfx, wrap, mode="ensemble")
                par = _frame_call(S, dev, form, None, rows, which, out_sfx, wrap, mode="params", params=table)
                assert ens.shape == par.shape == (members, len(sel), rows[1] - rows[0], Nx)
                for m in range(members):
                    ref = _images(qs[m], Nx, Ny, Hx, Hy, wrap)
                    _same(ens[m], _frame_call(S, dev, form, FCOR, rows, which, out_sfx, wrap, member=m), tag + f" member {m} vs single")
                    _same(ens[m], DC.np_derived_fields(*ref, Nx, Ny, Hx, Hy, _real(DX, sfx), _real(DY, sfx), _real(FCOR, sfx), form, rows=rows)[sel],
                          tag + f" member {m} vs restatement")
                    _same(par[m], _frame_call(S, dev, form, fs[m], rows, which, out_sfx, wrap, member=m), tag + f" member {m} params vs single")
                    _same(par[m], DC.np_derived_fields(*ref, Nx, Ny, Hx, Hy, _real(DX, sfx), _real(DY, sfx), _real(fs[m], sfx), form, rows=rows)[sel],
                          tag + f" member {m} params vs restatement")
                if members > 1 and which & 8:
                    assert not np.array_equal(par[0][-1], ens[0][-1])          # (another f: another q)
                if members > 1:
                    bad = _frame_call(S, dev_dirty, form, FCOR, rows, which, out_sfx, wrap, mode="ensemble")
                    assert np.isnan(bad[1]).all()
                    _same(bad[0], ens[0], tag + " member 0 beside a NaN member")
                    _same(bad[2], ens[2], tag + " member 2 beside a NaN member")


# --- the host mirror -------------------------------------------------------------------------------------------------------------------
H = 3
A_GRAD = -0.05


def _ics(form, chain):
    from test_model_oracle import hf, uf, vf, Af
    A = (lambda X, Y: Af(X, Y) + A_GRAD * Y) if chain else Af
    if form == "VectorInvariant":
        return dict(u=uf, v=vf, h=hf, A=A)
    return dict(uh=lambda X, Y: hf(X, Y) * uf(X, Y), vh=lambda X, Y: hf(X, Y) * vf(X, Y), h=hf, A=A)


def _bcs(S, topo):
    sides = (("west", "east") if topo[0] == "Bounded" else ()) + (("south", "north") if topo[1] == "Bounded" else ())
    return {"A": S.FieldBoundaryConditions(**{s: S.GradientBoundaryCondition(A_GRAD) for s in sides})} if sides else None


def _model(S, Nx, Ny, topo, form, f=0.8, **kw):
    from test_model_oracle import Lx, Ly
    g = S.RectilinearGrid(size=(Nx, Ny), x=(0, Lx), y=(0, Ly), topology=(*topo, "Flat"))
    m = S.ShallowWaterModel(g, 9.81, f, formulation=form, strict=True, boundary_conditions=_bcs(S, topo), **kw)
    return m.set(**_ics(form, topo[1] == "Bounded"))


def _restated(S, m, names, parents=None, f=None):
    """The restatement on the model's parents as they stand: stale halos where the model reads the periodic images itself (_rwrap)"""
    g = m.grid
    raw = parents if parents is not None else [fld.data.cpu().numpy() for fld in m._raw_fields]
    wx, wy = bool(m._rwrap & S._lib.WRAP_X), bool(m._rwrap & S._lib.WRAP_Y)
    q = OC.wrap_parents(raw, g.Nx, g.Ny, g.Hx, g.Hy, wx, wy)
    return DC.np_derived_fields(*q, g.Nx, g.Ny, g.Hx, g.Hy, g.dx, g.dy, m.f if f is None else f, m.form_code, names=names)


@pytest.mark.parametrize("topo", [("Periodic", "Periodic"), ("Periodic", "Bounded"), ("Bounded", "Periodic"), ("Bounded", "Bounded")],
                         ids=["PP", "PB", "BP", "BB"])
@pytest.mark.parametrize("form", list(FORMS))
def test_model_derived_fields(swmhd, topo, form):
    """A strict 48 x 40 model after five steps -- periodic (gather on read: the halos are stale) and the three Bounded topologies with a
    gradient condition on A -- in any order and repetition of names, float64 and float32, and into a caller's tensor."""
    S = swmhd
    m = _model(S, 48, 40, topo, form)
    m.time_steps(5, 0.002)
    got = m.derived_fields(DC.NAMES, array_type=torch.float64)
    assert tuple(got.shape) == (4, 40, 48) and got.dtype == torch.float64
    want = _restated(S, m, DC.NAMES)
    assert np.isfinite(want).all() and all(np.abs(w).max() > 0 for w in want)
    _same(got.cpu().numpy(), want, f"{topo} {form}")
    names = ("potential_vorticity", "current", "current", "vorticity", "divergence")
    got = m.derived_fields(names)
    assert got.dtype == torch.float32 and tuple(got.shape) == (5, 40, 48)
    _same(got.cpu().numpy(), want[[3, 2, 2, 0, 1]], f"{topo} {form} any order, float32")
    out = torch.full((2, 40, 48), SENT, dtype=torch.float64, device="cuda")
    assert m.derived_fields(("divergence", "vorticity"), out=out) is out
    _same(out.cpu().numpy(), want[[1, 0]], f"{topo} {form} out=")
    _same(m.derived_fields().cpu().numpy(), want[[0, 2]], "the default names")
    # among the frame's fields, through output_fields: a launch ends where the kernel changes
    mixed = m.output_fields(("u", "vorticity", "A", "current", "potential_vorticity", "B_x"), array_type=torch.float64).cpu().numpy()
    frame = m.output_fields(("u", "A", "B_x"), array_type=torch.float64).cpu().numpy()
    _same(mixed, np.stack([frame[0], want[0], frame[1], want[2], want[3], frame[2]]), f"{topo} {form} mixed frame")
    with pytest.raises(S._lib.SwmhdError):
        m.derived_fields(("vorticity", "u"))
    with pytest.raises(S._lib.SwmhdError):
        m.derived_fields(("vorticity",), out=torch.empty((1, 40, 47), device="cuda"))


def _writer_case(S, kind):
    from test_model_oracle import Lx, Ly
    names = ("u", "vorticity", "A", "current")
    if kind == "model":
        g = S.RectilinearGrid(size=(32, 24), x=(0, Lx), y=(0, Ly))
        make = lambda: S.ShallowWaterModel(g, 9.81, 0.8).set(**_ics("VectorInvariant", False))
    elif kind == "ensemble":           # periodic, per-member f: the _params entry point
        g = S.RectilinearGrid(size=(32, 24), x=(0, Lx), y=(0, Ly))
        make = lambda: S.ShallowWaterEnsemble(g, 3, 9.81, [0.5, 1.0, 2.0]).set(**_ics("VectorInvariant", False))
        names = ("u", "vorticity", "A", "potential_vorticity")
    else:                              # a channel ensemble, each member its own gradient of A
        g = S.RectilinearGrid(size=(32, 24), x=(0, Lx), y=(0, Ly), topology=("Periodic", "Bounded", "Flat"))
        grads = [-0.01, -0.05, 0.02]
        bcs = [{"A": S.FieldBoundaryConditions(north=S.GradientBoundaryCondition(gr), south=S.GradientBoundaryCondition(gr))} for gr in grads]
        from test_model_oracle import hf, uf, vf, Af
        make = lambda: S.BoundedShallowWaterEnsemble(g, 3, 9.81, 0.8, boundary_conditions=bcs).set(
            u=uf, v=vf, h=hf, A=[lambda X, Y, gr=gr: Af(X, Y) + gr * Y for gr in grads])
    return make, names


@pytest.mark.parametrize("kind", ["model", "ensemble", "channel"])
def test_writer_with_graph_replay(swmhd, kind):
    """FieldTimeSeries of (u, vorticity, A, current | potential_vorticity) through run() with graph replay, a frame every 5 iterations (odd:
    the ping-pong roles flip between frames): frame k is bitwise output_fields / derived_fields of an identical model advanced by the
    same counts and asked directly."""
    S = swmhd
    make, names = _writer_case(S, kind)
    dt, every, nframes = 0.002, 5, 4
    m = make()
    m.capture_graph(dt)
    series = S.FieldTimeSeries(m, names=names, schedule=S.IterationInterval(every), capacity=nframes, array_type=torch.float64)
    S.run(m, dt, stop_iteration=every * (nframes - 1), writers=[series])
    assert len(series) == nframes and series.iterations == list(range(0, every * nframes, every))
    got = series.numpy()
    members = getattr(m, "members", None)
    assert got.shape == (nframes,) + ((members,) if members else ()) + (4, 24, 32)
    twin = make()
    twin.capture_graph(dt)
    for k in range(nframes):
        if k:
            twin.time_steps(every, dt)
        frame = twin.output_fields((names[0], names[2]), array_type=torch.float64).cpu().numpy()
        drv = twin.derived_fields((names[1], names[3]), array_type=torch.float64).cpu().numpy()
        want = np.stack([frame[..., 0, :, :], drv[..., 0, :, :], frame[..., 1, :, :], drv[..., 1, :, :]], axis=-3)
        _same(got[k], want, f"{kind} frame {k}")
    assert not np.array_equal(got[0], got[-1])
    if kind == "ensemble":             # every member's q is the single model's with that member's f
        twin.synchronize()
        for k in range(3):
            mem = twin.member(k)
            assert mem.f == [0.5, 1.0, 2.0][k]
            _same(got[-1][k][3], mem.derived_fields(("potential_vorticity",), array_type=torch.float64).cpu().numpy()[0], f"member {k} q")
        assert not np.array_equal(got[-1][0][3], got[-1][1][3])


def _slab_frames(S, form, topo, Nx, Ny_local, world, plan, dt):
    from test_model_oracle import Lx, Ly
    rings = S.loopback_rings(world, 60.0)
    out, errs = [None] * world, []
    chain = topo[1] == "Bounded"

    def work(r):
        try:
            torch.cuda.set_device(0)
            with torch.cuda.stream(torch.cuda.Stream()):
                dec = S.SlabDecomposition(Ny_local * world, world, r, periodic=not chain)
                g = dec.local_grid(S.RectilinearGrid, Nx, x=(0, Lx), y=(0, Ly), halo=dec.ring_halo(), topology=(*topo, "Flat"))
                m = S.ShallowWaterModel(g, 9.81, 0.8, formulation=form, strict=True, decomp=dec, ring=rings[r], boundary_conditions=_bcs(S, topo))
                m.set(**_ics(form, chain))
                for n in plan:
                    m.time_steps(n, dt)
                frame = m.derived_fields(DC.NAMES, array_type=torch.float64)       # (the exchange of this state is still in flight)
                torch.cuda.current_stream().synchronize()
                out[r] = frame.cpu().numpy()
                m.synchronize()
                m.close()
        except Exception as e:          # noqa: BLE001 -- reported by the main thread
            errs.append((r, repr(e)))
    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errs, errs
    return np.concatenate(out, axis=1)


@pytest.mark.parametrize("topo", [("Periodic", "Periodic"), ("Periodic", "Bounded")], ids=["ring", "chain"])
@pytest.mark.parametrize("form", list(FORMS))
def test_slab_frames_stack_to_the_single_domain_frame(swmhd, topo, form):
    """Two loopback slabs of a 64 x 66 periodic grid (a ring) and of the channel (a chain), strict: each rank's own rows, stacked in y,
    are bitwise the frame of the single domain."""
    S = swmhd
    plan, dt = (1, 2), 0.002
    single = _model(S, 64, 66, topo, form)
    for n in plan:
        single.time_steps(n, dt)
    want = single.derived_fields(DC.NAMES, array_type=torch.float64).cpu().numpy()
    _same(want, _restated(S, single, DC.NAMES), f"single domain {topo} {form}")
    got = _slab_frames(S, form, topo, 64, 33, 2, plan, dt)
    assert np.isfinite(got).all()
    _same(got, want, f"slabs {topo} {form}")


def test_example_writes_derived_frames(tmp_path):
    """examples/run_swmhd.py --frame-fields u,vorticity,current: the last frame of frames.npz is the restatement applied to the fields
    the same run dumped at that iteration."""
    from swmhd_amd import configs
    out = tmp_path / "o"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "run_swmhd.py"), "--size", "64", "--stop-time", "1", "--frames", "0.5",
                        "--frame-fields", "u,vorticity,current", "--dump-every", "1", "--out", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out / "frames.npz")
    assert list(z["names"]) == ["u", "vorticity", "current"] and z["frames"].shape == (3, 3, 64, 64) and z["frames"].dtype == np.float32
    assert list(z["iterations"]) == [0, 50, 100]
    final = np.load(out / "fields_0000100.npz")
    q = [final[n] for n in ("u", "v", "h", "A")]
    want = DC.np_derived_fields(*q, 64, 64, H, H, 10.0 / 64, 10.0 / 64, configs.F, 1, names=("vorticity", "current"))
    _same(z["frames"][-1, 0], q[0][H:H + 64, H:H + 64], "u")
    _same(z["frames"][-1, 1:], want, "vorticity, current")
    assert np.abs(want[0]).max() > 1 and np.abs(want[1]).max() > 0
