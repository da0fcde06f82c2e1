"""GPU tests of the output frames (swmhd_output_fields_*, ShallowWaterModel.output_fields) and of the writer (FieldTimeSeries, run).

The yardstick is the numpy restatement in tests/output_cases.py (pinned on the CPU by tests/test_output_cpu.py).  The object is built
without FMA contraction and with IEEE divide and sqrt, so frames are compared BITWISE: float64 frames against the restatement, float32
frames against the restatement rounded to float32.  Every comparison prints the largest distance in units of the last place first."""
import ctypes
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

import helpers as Hh
import output_cases as OC
import plot_cases as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = OC.NAMES
H = 3
FORMS = {"VectorInvariant": 1, "Conservative": 0}
NP = {torch.float64: np.float64, torch.float32: np.float32}


def _ulps(got, want):
    """largest distance in units of the last place (0 = bitwise equal up to the sign of zero)"""
    it = np.int64 if got.dtype == np.float64 else np.int32
    a, b = got.view(it).astype(np.int64), want.view(it).astype(np.int64)
    return int(np.abs(a - b).max()) if np.isfinite(got).all() else -1


def _same(got, want, what):
    want = want.astype(got.dtype)
    print(what, "max ulp distance", _ulps(got, want))
    assert got.shape == want.shape and np.array_equal(got, want), (what, _ulps(got, want))
    Hh.same_bits(got, want, what)                          # ... and the sign of every zero


def _random_parents(Nx, Ny, dtype, seed):
    rng = np.random.default_rng(seed)
    shape = (Ny + 2 * H, Nx + 2 * H)
    q = [rng.standard_normal(shape), rng.standard_normal(shape), 1.0 + 0.3 * rng.random(shape), rng.standard_normal(shape)]
    return [np.ascontiguousarray(Hh.fill_halo_periodic(a, Nx, Ny, H, H).astype(NP[dtype])) for a in q]


def _model(S, Nx, Ny, form, dtype, parents=None, **kw):
    g = S.RectilinearGrid(size=(Nx, Ny), x=(0, 0.1 * Nx), y=(0, 0.1 * Ny))
    m = S.ShallowWaterModel(g, 9.81, 1.0, formulation=form, dtype=dtype, **kw)
    if parents is not None:
        for f, a in zip(m._raw_fields, parents):
            f.data.copy_(torch.from_numpy(a))
    return m


def _spacing(m):
    """dx, dy as the kernel receives them (an f32 model passes floats through the C-ABI)"""
    g = m.grid
    return (g.dx, g.dy) if m.sfx == "f64" else (float(np.float32(g.dx)), float(np.float32(g.dy)))


def _c_frame(S, m, names, rows=None, out_dtype=torch.float64, flags=0):
    """swmhd_output_fields_* called directly (row range, flags of the caller's choice) on the model's current parents"""
    g = m.grid
    j0, j1 = rows or (0, g.Ny)
    which = sum(S._lib.OUT_BITS[n] for n in names)
    out = torch.full((len(names), j1 - j0, g.Nx), float("nan"), dtype=out_dtype, device="cuda")
    q = m._raw_fields
    rc = getattr(S._lib.lib(), f"swmhd_output_fields_{m.sfx}")(
        q[0].ptr, q[1].ptr, q[2].ptr, q[3].ptr, g.Nx, g.Ny, g.Hx, g.Hy, q[0].stride_y, g.dx, g.dy, m.form_code, j0, j1, which,
        out.data_ptr(), out.element_size(), out.stride(1), out.stride(0), flags, S.fields._stream_ptr())
    S._lib.check(rc, "swmhd_output_fields")
    return out.cpu().numpy()


@pytest.mark.parametrize("Nx,Ny", [(48, 40), (64, 64), (250, 97), (1030, 516)])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("form", list(FORMS))
def test_frames_match_the_restatement_bitwise(swmhd, Nx, Ny, dtype, form):
    S = swmhd
    q = _random_parents(Nx, Ny, dtype, 11 + Nx)
    m = _model(S, Nx, Ny, form, dtype, q)
    dx, dy = _spacing(m)
    want = OC.np_output_fields(*q, Nx, Ny, H, H, dx, dy, FORMS[form])
    tag = f"{Nx}x{Ny} {m.sfx} {form}"
    _same(_c_frame(S, m, ALL), want, tag + " whole f64")
    _same(_c_frame(S, m, ALL, out_dtype=torch.float32), want, tag + " whole f32")
    j0, j1 = 5, Ny - 3
    part = OC.np_output_fields(*q, Nx, Ny, H, H, dx, dy, FORMS[form], rows=(j0, j1))
    assert np.array_equal(part, want[:, j0:j1])
    _same(_c_frame(S, m, ALL, rows=(j0, j1)), part, tag + " rows f64")
    _same(_c_frame(S, m, ("u", "v", "A", "s"), rows=(j0, j1), out_dtype=torch.float32), part[[0, 1, 3, 4]], tag + " rows default frame f32")
    # the public method: default frame in float32, any order of names, float64 on request
    got = m.output_fields()
    assert got.dtype == torch.float32 and tuple(got.shape) == (4, Ny, Nx)
    _same(got.cpu().numpy(), want[[0, 1, 3, 4]], tag + " output_fields()")
    _same(m.output_fields(("B_y", "s", "u", "B_x", "h"), array_type=torch.float64).cpu().numpy(), want[[6, 4, 0, 5, 2]], tag + " any order")
    if form == "VectorInvariant":        # u v h A: the parents' interior, bit for bit
        got = m.output_fields(("u", "v", "h", "A"), array_type=dtype).cpu().numpy()
        assert all(np.array_equal(got[k], q[k][H:H + Ny, H:H + Nx]) for k in range(4))


@pytest.mark.parametrize("Nx,Ny", [(48, 40), (250, 97)])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("form", list(FORMS))
def test_wrap_flags_read_no_halo(swmhd, Nx, Ny, dtype, form):
    S = swmhd
    q = _random_parents(Nx, Ny, dtype, 5)
    filled = _c_frame(S, _model(S, Nx, Ny, form, dtype, q), ALL)
    holed = []
    for a in q:
        b = np.full_like(a, np.nan)
        b[H:H + Ny, H:H + Nx] = a[H:H + Ny, H:H + Nx]
        holed.append(b)
    m = _model(S, Nx, Ny, form, dtype, holed)
    got = _c_frame(S, m, ALL, flags=S._lib.WRAP_X | S._lib.WRAP_Y)
    _same(got, filled, f"wrap {Nx}x{Ny} {m.sfx} {form}")
    j0, j1 = 0, 7
    _same(_c_frame(S, m, ALL, rows=(j0, j1), flags=S._lib.WRAP_X | S._lib.WRAP_Y), filled[:, j0:j1], "wrap, first rows")
    _same(_c_frame(S, m, ALL, rows=(Ny - 4, Ny), flags=S._lib.WRAP_X | S._lib.WRAP_Y), filled[:, Ny - 4:], "wrap, last rows")


@pytest.mark.parametrize("topo", [("Periodic", "Bounded"), ("Bounded", "Bounded")])
@pytest.mark.parametrize("form", list(FORMS))
def test_bounded_topologies(swmhd, topo, form):
    """After 10 steps: the restatement applied to model.fields, halos as the boundary-condition fill left them."""
    S = swmhd
    from test_model_oracle import Lx, Ly, hf, uf, vf, Af
    N = 64
    g = S.RectilinearGrid(size=(N, N), x=(0, Lx), y=(0, Ly), topology=(*topo, "Flat"))
    bcs = {"A": S.FieldBoundaryConditions(north=S.GradientBoundaryCondition(-0.05), south=S.GradientBoundaryCondition(-0.05))}
    m = S.ShallowWaterModel(g, 9.81, 1.0, formulation=form, boundary_conditions=bcs)
    A0 = lambda X, Y: Af(X, Y) - 0.05 * Y
    if form == "VectorInvariant":
        m.set(u=uf, v=vf, h=hf, A=A0)
    else:
        m.set(uh=lambda X, Y: hf(X, Y) * uf(X, Y), vh=lambda X, Y: hf(X, Y) * vf(X, Y), h=hf, A=A0)
    m.time_steps(10, 0.002)
    got = m.output_fields(ALL, array_type=torch.float64).cpu().numpy()
    q = [f.numpy() for f in m.fields]
    assert np.isfinite(got).all()
    _same(got, OC.np_output_fields(*q, N, N, H, H, g.dx, g.dy, FORMS[form]), f"{topo} {form}")


@pytest.mark.parametrize("bounded", [False, True])
@pytest.mark.parametrize("form", list(FORMS))
def test_ensemble_frame_is_every_members_frame(swmhd, bounded, form):
    S = swmhd
    from test_model_oracle import Lx, Ly, hf, uf, vf, Af
    N = 64
    if bounded:
        B = 4
        g = S.RectilinearGrid(size=(N, N), x=(0, Lx), y=(0, Ly), topology=("Periodic", "Bounded", "Flat"))
        grads = [-0.01, -0.05, -0.1, 0.02]
        bcs = [{"A": S.FieldBoundaryConditions(north=S.GradientBoundaryCondition(gr), south=S.GradientBoundaryCondition(gr))} for gr in grads]
        ens = S.BoundedShallowWaterEnsemble(g, B, 9.81, 1.0, formulation=form, boundary_conditions=bcs)
        A0 = [lambda X, Y, gr=gr: Af(X, Y) + gr * Y for gr in grads]
    else:
        B = 8
        g = S.RectilinearGrid(size=(N, N), x=(0, Lx), y=(0, Ly))
        ens = S.ShallowWaterEnsemble(g, B, 9.81, 1.0, formulation=form)
        A0 = [lambda X, Y, a=0.5 + 0.25 * k: a * Af(X, Y) for k in range(B)]
    n1, n2 = ens.names[:2]
    vi = form == "VectorInvariant"
    ens.set(**{n1: uf if vi else (lambda X, Y: hf(X, Y) * uf(X, Y)), n2: vf if vi else (lambda X, Y: hf(X, Y) * vf(X, Y)), "h": hf, "A": A0})
    ens.time_steps(3, 0.002)
    for at in (torch.float64, torch.float32):
        frame = ens.output_fields(ALL, array_type=at)
        assert tuple(frame.shape) == (B, len(ALL), N, N) and frame.dtype == at
        frame = frame.cpu().numpy()
        assert np.isfinite(frame).all()
        for k in range(B):
            _same(frame[k], ens.member(k).output_fields(ALL, array_type=at).cpu().numpy(), f"member {k} bounded={bounded} {form}")
    assert not np.array_equal(frame[0], frame[1])


def _plot_model(S, key, form):
    """The run behind one of the reference's plots (plot_cases.run_model's set-up), returned as a model"""
    N, ic = 64, key
    c = P.ICS[ic]
    topo = tuple("Bounded" if t else "Periodic" for t in c["topo"]) + ("Flat",)
    g = S.RectilinearGrid(size=(N, N), x=(-P.L / 2, P.L / 2), y=(-P.L / 2, P.L / 2), topology=topo)
    bcs = None
    if c["gradA"]:
        side = dict(zip(("west", "east", "south", "north"), c["gradA"]))
        bcs = {"A": S.FieldBoundaryConditions(**{k: S.GradientBoundaryCondition(v) for k, v in side.items() if v is not None})}
    m = S.ShallowWaterModel(g, P.G, P.F, formulation=form, boundary_conditions=bcs)
    zero = lambda X, Y: np.zeros_like(X)
    n1, n2 = m.names[:2]
    m.set(**{n1: c["u"] or zero, n2: c["v"] or zero, "h": lambda X, Y: np.ones_like(X), "A": c["A"]})
    return m


@pytest.mark.parametrize("ic", ["two_Gaussians_low_B", "low_B_low_U"])
@pytest.mark.parametrize("form", list(FORMS))
def test_frames_and_diagnostics_agree_on_the_device(swmhd, ic, form):
    """After 50 steps of a 64^2 plotted run the energies summed from the float64 frames (s, B_x, B_y, h) equal those of
    model.diagnostics() to 2e-12 (N^2 summands x 2^-53, see tests/test_output_cpu.py) and max|u frame| equals max_abs_u exactly.
    The kinetic identity is the vector-invariant form's.  The low_B_low_U run is (Periodic, Bounded): averaging B to the centres of the
    first and the last row needs B_y of the south halo row and the far-wall line of B_x, boundary values that are not part of a frame
    -- there the magnetic energy is compared over rows 2 .. Ny-1 with swmhd_diagnostics on that row range (the C call takes rows;
    model.diagnostics() does not)."""
    S = swmhd
    m = _plot_model(S, ic, form)
    m.time_steps(50, P.DT)
    g = m.grid
    u, hh, s, bx, by = m.output_fields(("u", "h", "s", "B_x", "B_y"), array_type=torch.float64).cpu().numpy()
    d = m.diagnostics()
    assert np.isfinite(s).all() and np.abs(u).max() == d["max_abs_u"]
    j0, rows = (0, g.Ny) if g.topology[1] == "Periodic" else (1, g.Ny - 1)
    me_ref = d["magnetic_energy"]
    if rows != g.Ny:
        ws = torch.empty(S._lib.DIAG_WORKSPACE, dtype=torch.float64, device="cuda")
        o = torch.empty(S._lib.DIAG_NOUT, dtype=torch.float64, device="cuda")
        q = m.fields
        S._lib.check(S._lib.lib().swmhd_diagnostics_f64(q[0].ptr, q[1].ptr, q[2].ptr, q[3].ptr, g.Nx, g.Ny, g.Hx, g.Hy, q[0].stride_y, g.dx,
                                                       g.dy, m.g, 1.0, m.form_code, j0, rows, ws.data_ptr(), o.data_ptr(),
                                                       S.fields._stream_ptr()), "swmhd_diagnostics")
        me_ref = float(o.cpu()[1])
    me = OC.magnetic_density_from_frames(bx, by, hh)[j0:rows].sum() * (g.dx * g.dy)
    print(ic, form, "ME", me, me_ref, "rel", abs(me - me_ref) / me_ref)
    assert me_ref > 0 and abs(me - me_ref) <= 2e-12 * me_ref
    if form == "VectorInvariant":
        ke = OC.kinetic_energy_from_frames(s, hh, g.dx, g.dy)
        print(ic, form, "KE", ke, d["kinetic_energy"], "rel", abs(ke - d["kinetic_energy"]) / d["kinetic_energy"])
        assert d["kinetic_energy"] > 0 and abs(ke - d["kinetic_energy"]) <= 2e-12 * d["kinetic_energy"]


def _vortex(m):
    u0 = lambda X, Y: Y * np.exp(-(X ** 2 + Y ** 2))
    v0 = lambda X, Y: -X * np.exp(-(X ** 2 + Y ** 2))
    n1, n2 = m.names[:2]
    members = getattr(m, "members", None)
    A0 = P.two_gaussians(0.1) if members is None else [P.two_gaussians(0.1 * (k + 1)) for k in range(members)]
    m.set(**{n1: u0, n2: v0, "h": lambda X, Y: np.ones_like(X), "A": A0})
    return m


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("ensemble", [False, True])
@pytest.mark.parametrize("schedule", ["time", "iteration"])
def test_writer_with_graph_replay(swmhd, strict, ensemble, schedule):
    """64^2, dt = 0.01 to t = 1 with a captured graph: TimeInterval(0.1) -> 11 frames, IterationInterval(5) (odd: the ping-pong roles
    flip between frames) -> 21; frame k is bitwise output_fields of an identical model advanced eagerly by the same counts."""
    S = swmhd
    g = S.RectilinearGrid(size=(64, 64), x=(-5, 5), y=(-5, 5))
    make = (lambda: S.ShallowWaterEnsemble(g, 4, 9.81, 1.0, strict=strict)) if ensemble else (lambda: S.ShallowWaterModel(g, 9.81, 1.0, strict=strict))
    sched, every, nframes = (S.TimeInterval(0.1), 10, 11) if schedule == "time" else (S.IterationInterval(5), 5, 21)
    m = _vortex(make())
    m.capture_graph(0.01)
    series = S.FieldTimeSeries(m, schedule=sched, capacity=nframes)
    with pytest.raises(S._lib.SwmhdError):
        S.run(m, 0.01, stop_time=1.0, writers=[S.FieldTimeSeries(m, schedule=sched, capacity=nframes - 1)])
    assert m.iteration == 0
    S.run(m, 0.01, stop_time=1.0, writers=[series])
    assert m.iteration == 100 and len(series) == nframes and series.iterations == list(range(0, 101, every))
    assert np.allclose(series.times, np.arange(nframes) * every * 0.01, rtol=0, atol=1e-12)
    got = series.numpy()
    assert got.dtype == np.float32 and got.shape == (nframes,) + ((4,) if ensemble else ()) + (4, 64, 64)
    twin = _vortex(make())
    for k in range(nframes):
        if k:
            twin.time_steps(every, 0.01)
        _same(got[k], twin.output_fields().cpu().numpy(), f"frame {k}")
    assert not np.array_equal(got[0], got[-1])
    with pytest.raises(S._lib.SwmhdError):
        series.write()                                    # all slots are written


def test_series_save(swmhd, tmp_path):
    S = swmhd
    m = _vortex(S.ShallowWaterModel(S.RectilinearGrid(size=(64, 64), x=(-5, 5), y=(-5, 5)), 9.81, 1.0))
    series = S.FieldTimeSeries(m, names=("A", "B_x", "B_y"), schedule=S.IterationInterval(4), capacity=8, array_type=torch.float64)
    S.run(m, 0.01, stop_iteration=12, writers=[series])
    S.run(m, 0.01, stop_iteration=20, writers=[series])                # a continued run does not repeat the frame it starts from
    series.save(tmp_path / "frames.npz")
    z = np.load(tmp_path / "frames.npz")
    assert list(z["names"]) == ["A", "B_x", "B_y"] and list(z["iterations"]) == [0, 4, 8, 12, 16, 20]
    assert z["frames"].shape == (6, 3, 64, 64) and z["frames"].dtype == np.float64 and list(z["size"]) == [64, 64]
    _same(z["frames"][-1], m.output_fields(("A", "B_x", "B_y"), array_type=torch.float64).cpu().numpy(), "last saved frame")


def _slab_frames(S, form, topo, Nx, Ny_local, world, plan, dt, bcs):
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
                m = S.ShallowWaterModel(g, 9.81, 1.0, formulation=form, strict=True, decomp=dec, ring=rings[r], boundary_conditions=bcs)
                m.set(**_slab_ics(form, chain))
                for n in plan:
                    m.time_steps(n, dt)
                frame = m.output_fields(ALL, array_type=torch.float64)       # (the exchange of this state is still in flight)
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


def _slab_ics(form, chain):
    from test_model_oracle import hf, uf, vf, Af
    A = (lambda X, Y: Af(X, Y) - 0.05 * Y) if chain else Af
    if form == "VectorInvariant":
        return dict(u=uf, v=vf, h=hf, A=A)
    return dict(uh=lambda X, Y: hf(X, Y) * uf(X, Y), vh=lambda X, Y: hf(X, Y) * vf(X, Y), h=hf, A=A)


@pytest.mark.parametrize("topo", [("Periodic", "Periodic"), ("Periodic", "Bounded")])
@pytest.mark.parametrize("form", list(FORMS))
def test_slab_frames_stack_to_the_single_domain_frame(swmhd, topo, form):
    """Two loopback slabs of a 64 x 66 periodic grid (a ring) and of the channel (a chain), strict: the frames stacked in y are bitwise
    the frame of the single domain."""
    S = swmhd
    from test_model_oracle import Lx, Ly
    chain = topo[1] == "Bounded"
    bcs = {"A": S.FieldBoundaryConditions(north=S.GradientBoundaryCondition(-0.05), south=S.GradientBoundaryCondition(-0.05))} if chain else None
    plan, dt = (1, 2), 0.002
    g = S.RectilinearGrid(size=(64, 66), x=(0, Lx), y=(0, Ly), topology=(*topo, "Flat"))
    single = S.ShallowWaterModel(g, 9.81, 1.0, formulation=form, strict=True, boundary_conditions=bcs)
    single.set(**_slab_ics(form, chain))
    for n in plan:
        single.time_steps(n, dt)
    want = single.output_fields(ALL, array_type=torch.float64).cpu().numpy()
    got = _slab_frames(S, form, topo, 64, 33, 2, plan, dt, bcs)
    assert np.isfinite(got).all()
    _same(got, want, f"slabs {topo} {form}")


def test_example_writes_frames(tmp_path):
    out = tmp_path / "o"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "run_swmhd.py"), "--size", "64", "--stop-time", "1", "--frames", "0.1",
                        "--dump-every", "1", "--out", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out / "frames.npz")
    assert list(z["names"]) == ["u", "v", "A", "s"] and z["frames"].shape == (11, 4, 64, 64) and z["frames"].dtype == np.float32
    assert np.allclose(z["times"], np.arange(11) * 0.1, rtol=0, atol=1e-12) and list(z["iterations"]) == list(range(0, 101, 10))
    final = np.load(out / "fields_0000100.npz")
    assert np.array_equal(z["frames"][-1, 2], final["A"][H:H + 64, H:H + 64].astype(np.float32))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "run_swmhd.py"), "--size", "64", "--stop-time", "0.2", "--frames", "0.1",
                        "--frame-fields", "A,B_x,B_y", "--frame-dtype", "f64", "--amps", "0.1,0.5", "--out", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out / "frames.npz")
    assert z["frames"].shape == (3, 2, 3, 64, 64) and z["frames"].dtype == np.float64 and np.isfinite(z["frames"]).all()
