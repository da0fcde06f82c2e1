"""GPU tests of the Lagrangian particles.  The kernel matrix drives the C ABI (include/swmhd_particles.h) and compares bitwise with the
numpy restatement (tests/particle_cases.py): every grid, particle count, element type, formulation, wrap and Bounded flag of the case
list, pitched parents with NaN in every halo cell a wrapped call must not read, sentinels around every particle array, the positions
that must be present (walls, nodes, the half cell below the first centre, +-1e300, +-inf, NaN), stages chained, ensembles against
single calls, the sampler at every location code.  The model-level tests: the state is untouched by the particles, eager steps,
graph replay and an ensemble member agree, checkpoints round-trip, a channel keeps its particles, a uniform flow carries them at its
speed."""
import ctypes

import numpy as np
import pytest
import torch

import particle_cases as PC
from helpers import same_bits

pytestmark = pytest.mark.gpu
SFX = {np.float64: "f64", np.float32: "f32"}
GUARD = 8
SENTINEL = -7.25e77
X0, Y0, DX, DY = -0.75, 2.5, 0.125, 0.2


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class ParticleBuffers:
    """x, y, gx, gy (or any rows) of one call in one device tensor with GUARD sentinels before and after every row"""

    def __init__(self, rows):
        self.n = rows[0].size
        host = np.full((len(rows), self.n + 2 * GUARD), SENTINEL)
        for k, r in enumerate(rows):
            host[k, GUARD:GUARD + self.n] = r.ravel()
        self.t = _dev(host)

    def ptr(self, k):
        return self.t.data_ptr() + 8 * (k * (self.n + 2 * GUARD) + GUARD)

    def read(self, shape=None):
        """the rows back on the host, after the check that no sentinel was touched"""
        host = self.t.cpu().numpy()
        guards = np.concatenate([host[:, :GUARD], host[:, GUARD + self.n:]], axis=1)
        assert np.array_equal(guards.view(np.int64), np.full_like(guards, SENTINEL).view(np.int64)), "a sentinel was overwritten"
        return [r[GUARD:GUARD + self.n].reshape(shape or (self.n,)) for r in host]


def device_stage(S, q, x, y, gx, gy, Nx, Ny, Hx, Hy, form, dt, gamma, zeta, flags):
    """swmhd_particles_rk3_* on pitched parents q = (q1, q2, h) (host arrays whose rows are the pitch): new (x, y, gx, gy)"""
    L = S._lib.lib()
    sfx = SFX[q[0].dtype.type]
    dq = [_dev(a) for a in q]
    buf = ParticleBuffers([x, y, gx, gy])
    rc = getattr(L, f"swmhd_particles_rk3_{sfx}")(dq[0].data_ptr(), dq[1].data_ptr(), dq[2].data_ptr(), buf.ptr(0), buf.ptr(1), buf.ptr(2),
                                                    buf.ptr(3), x.size, Nx, Ny, Hx, Hy, q[0].shape[1], X0, Y0, DX, DY, form, dt, gamma, zeta,
                                                    flags, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return buf.read()


def restated_stage(q, x, y, gx, gy, Nx, Ny, Hx, Hy, form, dt, gamma, zeta, flags):
    W = Nx + 2 * Hx
    return PC.stage(q[0][:, :W], q[1][:, :W], q[2][:, :W], x, y, gx, gy, Nx, Ny, Hx, Hy, X0, Y0, DX, DY, form, dt, gamma, zeta, flags)


def flag_sets():
    """each wrap flag alone, both and neither; the directions that are not wrapped once Periodic and once Bounded"""
    out = []
    for wrap in PC.WRAPS:
        out.append(wrap)
        bounded = (0 if wrap & PC.WRAP_X else PC.BOUNDED_X) | (0 if wrap & PC.WRAP_Y else PC.BOUNDED_Y)
        if bounded:
            out.append(wrap | bounded)
    return out


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("Nx, Ny", PC.GRIDS)
def test_stage_matrix(swmhd, Nx, Ny, dtype):
    rng = np.random.default_rng(Nx * 100 + Ny)
    seed = 0
    for P in PC.COUNTS:
        for form in (PC.VECTOR_INVARIANT, PC.CONSERVATIVE):
            # a direction that is not wrapped reads a filled halo: depths 1 and 3 for every such flag set; the call that wraps both
            # directions reads no halo and takes one depth; pitched rows
            for flags, H in [(fl, H) for fl in flag_sets() for H in (PC.HALOS if fl & (PC.WRAP_X | PC.WRAP_Y) != (PC.WRAP_X | PC.WRAP_Y) else PC.HALOS[1:])]:
                seed += 1
                q = PC.parents(Nx, Ny, H, H, 5, dtype, seed, flags)
                x, y = PC.positions(P, Nx, Ny, X0, Y0, DX, DY, seed)
                zeta = PC.RK3_ZETA[seed % 3]
                gamma = PC.RK3_GAMMA[seed % 3]
                # G- of a stage that does not read it: NaN; else finite values
                gx, gy = (np.full(P, np.nan), np.full(P, np.nan)) if zeta == 0.0 else (rng.standard_normal(P), rng.standard_normal(P))
                args = (Nx, Ny, H, H, form, 0.05, gamma, zeta, flags | (swmhd._lib.STRICT if seed % 4 == 0 else 0))
                got = device_stage(swmhd, q, x, y, gx, gy, *args)
                want = restated_stage(q, x, y, gx, gy, *args)
                what = f"P {P} form {form} flags {flags} H {H}"
                for g_, w_, n in zip(got, want, ("x", "y", "gx", "gy")):
                    same_bits(g_, w_, f"{n}: {what}")
                live = np.isfinite(x) & np.isfinite(y)
                # a particle with a non-finite coordinate is untouched bit for bit, and so is its G- (here: the value it was given)
                for g_, before in zip(got, (x, y, gx, gy)):
                    same_bits(g_[~live], before[~live], f"dead particles: {what}")
                # finite parents and finite positions give finite results, with NaN in G- where zeta == 0 and in every halo a wrapped
                # call must not read -- except where x - x0 overflows (+-1e300 stay finite: the fold clamps them into the domain)
                assert np.all(np.isfinite(got[0][live])) and np.all(np.isfinite(got[1][live])), what
                assert np.all(np.isfinite(got[2][live])) and np.all(np.isfinite(got[3][live])), what
                Lx, Ly = Nx * DX, Ny * DY
                assert np.all((got[0][live] >= X0) & (got[0][live] <= X0 + Lx) & (got[1][live] >= Y0) & (got[1][live] <= Y0 + Ly)), what


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("form", [PC.VECTOR_INVARIANT, PC.CONSERVATIVE], ids=["vi", "cons"])
def test_three_stages_chained(swmhd, form, dtype):
    Nx, Ny, H, P = 67, 33, 3, 257
    for flags in (PC.WRAP_X | PC.WRAP_Y, PC.WRAP_X | PC.BOUNDED_Y, 0):
        q = PC.parents(Nx, Ny, H, H, 3, dtype, 11, flags)
        x, y = PC.positions(P, Nx, Ny, X0, Y0, DX, DY, 12)
        got = want = (x, y, np.full(P, np.nan), np.full(P, np.nan))
        for k in range(3):
            args = (Nx, Ny, H, H, form, 0.3, PC.RK3_GAMMA[k], PC.RK3_ZETA[k], flags)
            got = device_stage(swmhd, q, *got, *args)
            want = restated_stage(q, *want, *args)
        for g_, w_, n in zip(got, want, ("x", "y", "gx", "gy")):
            same_bits(g_, w_, f"{n} after three stages, flags {flags}")
        assert not np.array_equal(got[0][12:], x[12:])


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("table", [False, True], ids=["dt", "params"])
def test_ensemble_members_are_single_calls(swmhd, dtype, table):
    """three members that share no field, position or dt, pitched apart with NaN between them: member m is bitwise the single call"""
    L = swmhd._lib.lib()
    sfx = SFX[dtype]
    Nx, Ny, H, P, M, pitch, gap = 5, 7, 1, 65, 3, 2, 13
    for form, flags in ((PC.VECTOR_INVARIANT, PC.WRAP_X | PC.WRAP_Y), (PC.CONSERVATIVE, PC.WRAP_X | PC.BOUNDED_Y), (PC.CONSERVATIVE, 0)):
        rows, W = Ny + 2 * H, Nx + 2 * H + pitch
        stride_m = rows * W + gap
        members = [PC.parents(Nx, Ny, H, H, pitch, dtype, 40 + m, flags) for m in range(M)]
        flat = [np.full(M * stride_m, np.nan, dtype=dtype) for _ in range(3)]
        for m in range(M):
            for k in range(3):
                flat[k][m * stride_m:m * stride_m + rows * W] = members[m][k].ravel()
        dq = [_dev(a) for a in flat]
        xy = [PC.positions(P, Nx, Ny, X0, Y0, DX, DY, 50 + m) for m in range(M)]
        rng = np.random.default_rng(9)
        g = [(rng.standard_normal(P), rng.standard_normal(P)) for _ in range(M)]
        dts = np.array([0.05, 0.0125, 0.2], dtype=dtype)
        params = _dev(np.stack([np.full(M, 9.81), np.ones(M), dts], axis=1).astype(dtype))
        buf = ParticleBuffers([np.stack([a[0] for a in xy]), np.stack([a[1] for a in xy]), np.stack([a[0] for a in g]), np.stack([a[1] for a in g])])
        gamma, zeta = PC.RK3_GAMMA[1], PC.RK3_ZETA[1]
        rc = getattr(L, f"swmhd_ensemble_particles_rk3_{sfx}")(dq[0].data_ptr(), dq[1].data_ptr(), dq[2].data_ptr(), buf.ptr(0), buf.ptr(1),
                                                                 buf.ptr(2), buf.ptr(3), P, M, stride_m, Nx, Ny, H, H, W, X0, Y0, DX, DY, form,
                                                                 params.data_ptr() if table else None, 0.05, gamma, zeta, flags, None)
        assert rc == 0, rc
        torch.cuda.synchronize()
        got = buf.read((M, P))
        for m in range(M):
            dt = float(dts[m]) if table else 0.05       # (the table's dt in the element type, widened)
            args = (Nx, Ny, H, H, form, dt, gamma, zeta, flags)
            single = device_stage(swmhd, members[m], xy[m][0], xy[m][1], g[m][0], g[m][1], *args)
            want = restated_stage(members[m], xy[m][0], xy[m][1], g[m][0], g[m][1], *args)
            for k, n in enumerate(("x", "y", "gx", "gy")):
                same_bits(got[k][m], single[k], f"member {m} {n} against the single call, flags {flags}")
                same_bits(got[k][m], want[k], f"member {m} {n} against the restatement, flags {flags}")


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("Nx, Ny", [(1, 1), (3, 2), (67, 33)])
def test_sampler(swmhd, Nx, Ny, dtype):
    """every location code, bitwise; NaN for a particle with a non-finite coordinate; a sentinel after the output; ensembles"""
    L = swmhd._lib.lib()
    sfx = SFX[dtype]
    for P in (0, 1, 65, 1000):
        for flags in flag_sets():
            H, pitch = (1, 4) if flags & PC.BOUNDED_Y else (3, 0)
            W = Nx + 2 * H + pitch
            fields = PC.parents(Nx, Ny, H, H, pitch, dtype, 70 + P, flags, n=5)
            locs = [0, 1, 2, 3, 3]
            x, y = PC.positions(P, Nx, Ny, X0, Y0, DX, DY, 71 + P)
            df = [_dev(a) for a in fields]
            pos, out = ParticleBuffers([x, y]), ParticleBuffers([np.zeros(5 * P)])
            rc = getattr(L, f"swmhd_particles_sample_{sfx}")(swmhd._lib.ptr_array([t.data_ptr() for t in df]), (ctypes.c_int * 5)(*locs), 5,
                                                               pos.ptr(0), pos.ptr(1), out.ptr(0), P, Nx, Ny, H, H, W, X0, Y0, DX, DY, flags, None)
            assert rc == 0, rc
            torch.cuda.synchronize()
            got = out.read((5, P))[0]
            want = PC.sample([a[:, :Nx + 2 * H] for a in fields], locs, x, y, Nx, Ny, H, H, X0, Y0, DX, DY, flags)
            same_bits(got, want, f"sample P {P} flags {flags}")
            dead = ~(np.isfinite(x) & np.isfinite(y))
            assert np.all(np.isnan(got[:, dead])) and np.all(np.isfinite(got[:, ~dead]))
            same_bits(pos.read()[0], x, "the sampler leaves the positions alone")
    # an ensemble of two members, a gap between them: (members, nfields, P), member m the single call's
    P, H, flags, M = 63, 2, PC.WRAP_X | PC.WRAP_Y, 2
    W, rows = Nx + 2 * H, Ny + 2 * H
    stride_m = rows * W + 7
    members = [PC.parents(Nx, Ny, H, H, 0, dtype, 90 + m, flags, n=2) for m in range(M)]
    flat = [np.full(M * stride_m, np.nan, dtype=dtype) for _ in range(2)]
    for m in range(M):
        for k in range(2):
            flat[k][m * stride_m:m * stride_m + rows * W] = members[m][k].ravel()
    df = [_dev(a) for a in flat]
    xy = [PC.positions(P, Nx, Ny, X0, Y0, DX, DY, 95 + m) for m in range(M)]
    pos, out = ParticleBuffers([np.stack([a[0] for a in xy]), np.stack([a[1] for a in xy])]), ParticleBuffers([np.zeros(M * 2 * P)])
    rc = getattr(L, f"swmhd_ensemble_particles_sample_{sfx}")(swmhd._lib.ptr_array([t.data_ptr() for t in df]), (ctypes.c_int * 2)(2, 1), 2,
                                                                pos.ptr(0), pos.ptr(1), out.ptr(0), P, M, stride_m, Nx, Ny, H, H, W, X0, Y0, DX, DY,
                                                                flags, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = out.read((M, 2, P))[0]
    for m in range(M):
        same_bits(got[m], PC.sample(members[m], [2, 1], xy[m][0], xy[m][1], Nx, Ny, H, H, X0, Y0, DX, DY, flags), f"ensemble sample, member {m}")


# --- model level ---------------------------------------------------------------------------------------------------------------------
DT = 0.002


def _initial(S, g, model, amp=0.1):
    u = lambda X, Y: amp * np.sin(2 * np.pi * (Y - g.y[0]) / g.Ly) * np.cos(2 * np.pi * (X - g.x[0]) / g.Lx) + 0.3
    v = lambda X, Y: amp * np.cos(2 * np.pi * (Y - g.y[0]) / g.Ly) * np.sin(4 * np.pi * (X - g.x[0]) / g.Lx)
    h = lambda X, Y: 1.0 + 0.05 * np.cos(2 * np.pi * (X - g.x[0]) / g.Lx)
    A = lambda X, Y: 0.2 * np.sin(2 * np.pi * (X - g.x[0]) / g.Lx) * np.sin(2 * np.pi * (Y - g.y[0]) / g.Ly)
    return {model.names[0]: u, model.names[1]: v, "h": h, "A": A}


def _seeds(g, P, seed=5, outside=True):
    rng = np.random.default_rng(seed)
    lo, hi = (-1.0, 2.0) if outside else (0.0, 1.0)
    return g.x[0] + g.Lx * rng.uniform(lo, hi, P), g.y[0] + g.Ly * rng.uniform(lo, hi, P)


def _state(model):
    model.synchronize()
    return [f.numpy().copy() for f in model.fields]


@pytest.mark.parametrize("formulation", ["VectorInvariant", "Conservative"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_state_is_unchanged_by_the_particles(swmhd, dtype, formulation):
    S = swmhd
    g = S.RectilinearGrid(size=(32, 24), x=(-1.0, 1.0), y=(0.0, 1.5))
    x, y = _seeds(g, 100)
    plain = S.ShallowWaterModel(g, formulation=formulation, dtype=dtype)
    model = S.ShallowWaterModel(g, formulation=formulation, dtype=dtype, particles=S.LagrangianParticles(x, y, tracked_fields=("A", "h")))
    for m in (plain, model):
        m.set(**_initial(S, g, m))
    p = model.particles
    assert p.x.dtype == torch.float64 and tuple(p.x.shape) == (100,) and p.x.is_cuda
    xs, ys = p.x.cpu().numpy(), p.y.cpu().numpy()
    assert np.all((xs >= -1.0) & (xs <= 1.0) & (ys >= 0.0) & (ys <= 1.5))        # the seeds were folded into the periodic box
    same_bits(xs, PC.fold(x, -1.0, 32 * g.dx, PC.WRAP), "the folded seeds")
    for _ in range(6):
        model.time_step(DT)
        plain.time_step(DT)
    for a, b in zip(_state(model), _state(plain)):
        same_bits(a, b, "the state of a model with particles")
    assert model.iteration == 6 and np.all(np.isfinite(p.x.cpu().numpy()))
    # tracked fields: the sampler on the model's state, bitwise the restatement
    got = p.sample().cpu().numpy()
    q = dict(zip(model.names, _state(model)))
    want = PC.sample([q["A"], q["h"]], [3, 3], p.x.cpu().numpy(), p.y.cpu().numpy(), 32, 24, 3, 3, -1.0, 0.0, g.dx, g.dy, PC.WRAP_X | PC.WRAP_Y)
    same_bits(got, want, "sample(A, h)")
    same_bits(p.sample((model.names[0],)).cpu().numpy(),
              PC.sample([q[model.names[0]]], [2], p.x.cpu().numpy(), p.y.cpu().numpy(), 32, 24, 3, 3, -1.0, 0.0, g.dx, g.dy, 0), "sample(u)")
    with pytest.raises(S._lib.SwmhdError, match="one of"):
        p.sample(("B_x",))


def test_first_stage_of_a_model_is_the_restatement(swmhd):
    """the model's own launch (its pointers, extents, origin and flags) of stage 1 on the initial state, bitwise the restatement"""
    S = swmhd
    g = S.RectilinearGrid(size=(32, 24), x=(-1.0, 1.0), y=(0.0, 1.5))
    x, y = _seeds(g, 100, outside=False)
    model = S.ShallowWaterModel(g, particles=S.LagrangianParticles(x, y))
    model.set(**_initial(S, g, model))
    q = _state(model)
    p = model.particles
    p.launch(model, DT, 0)
    torch.cuda.synchronize()
    want = PC.stage(q[0], q[1], None, x, y, np.full(100, np.nan), np.full(100, np.nan), 32, 24, 3, 3, -1.0, 0.0, g.dx, g.dy, model.form_code,
                    DT, PC.RK3_GAMMA[0], PC.RK3_ZETA[0], PC.WRAP_X | PC.WRAP_Y)
    for t, w, n in zip(p.state_tensors(), want, ("x", "y", "gx", "gy")):
        same_bits(t.cpu().numpy(), w, n)


def test_eager_graph_and_ensemble_agree(swmhd):
    S = swmhd
    g = S.RectilinearGrid(size=(32, 24), x=(-1.0, 1.0), y=(0.0, 1.5))
    x, y = _seeds(g, 100)
    make = lambda: S.ShallowWaterModel(g, strict=True, particles=S.LagrangianParticles(x, y))
    eager, replay = make(), make()
    for m in (eager, replay):
        m.set(**_initial(S, g, m))
    for _ in range(6):
        eager.time_step(DT)
    replay.capture_graph(DT)
    same_bits(replay.particles.x.cpu().numpy(), PC.fold(x, -1.0, 32 * g.dx, PC.WRAP), "capture_graph restores the positions")
    replay.time_steps(6, DT)
    ens = S.ShallowWaterEnsemble(g, 2, strict=True, particles=S.LagrangianParticles(np.stack([x, x]), np.stack([y, y])))
    ens.set(**_initial(S, g, eager))
    assert tuple(ens.particles.x.shape) == (2, 100)
    ens.time_steps(6, DT)
    torch.cuda.synchronize()
    ex, ey = eager.particles.x.cpu().numpy(), eager.particles.y.cpu().numpy()
    assert not np.array_equal(ex, PC.fold(x, -1.0, 32 * g.dx, PC.WRAP))
    same_bits(replay.particles.x.cpu().numpy(), ex, "graph replay x")
    same_bits(replay.particles.y.cpu().numpy(), ey, "graph replay y")
    for m in range(2):
        same_bits(ens.particles.x[m].cpu().numpy(), ex, f"ensemble member {m} x")
        same_bits(ens.particles.y[m].cpu().numpy(), ey, f"ensemble member {m} y")
    assert tuple(ens.particles.sample(("A",)).shape) == (2, 1, 100)
    # a per-member dt: member 0 steps as the model does
    per = S.ShallowWaterEnsemble(g, 2, strict=True, particles=S.LagrangianParticles(x, y))
    per.set(**_initial(S, g, eager))
    per.time_steps(6, [DT, DT / 2])
    same_bits(per.particles.x[0].cpu().numpy(), ex, "per-member dt, member 0")
    assert not np.array_equal(per.particles.x[1].cpu().numpy(), ex)


def test_checkpoint_round_trip(swmhd, tmp_path):
    S = swmhd
    g = S.RectilinearGrid(size=(32, 24), x=(-1.0, 1.0), y=(0.0, 1.5))
    x, y = _seeds(g, 100)
    a = S.ShallowWaterModel(g, particles=S.LagrangianParticles(x, y))
    a.set(**_initial(S, g, a))
    for _ in range(3):
        a.time_step(DT)
    path = str(tmp_path / "ck.npz")
    a.save_checkpoint(path)
    for _ in range(3):
        a.time_step(DT)
    b = S.ShallowWaterModel(g, particles=S.LagrangianParticles(np.zeros(100), np.zeros(100)))
    b.load_checkpoint(path)
    for _ in range(3):
        b.time_step(DT)
    same_bits(b.particles.x.cpu().numpy(), a.particles.x.cpu().numpy(), "x after a checkpoint")
    same_bits(b.particles.y.cpu().numpy(), a.particles.y.cpu().numpy(), "y after a checkpoint")
    for fa, fb in zip(_state(a), _state(b)):
        same_bits(fb, fa, "state after a checkpoint")


def test_bounded_channel_keeps_its_particles(swmhd):
    S = swmhd
    g = S.RectilinearGrid(size=(16, 12), x=(0.0, 2.0), y=(-0.5, 1.0), topology=("Periodic", "Bounded", "Flat"))
    rng = np.random.default_rng(2)
    x = rng.uniform(-2.0, 4.0, 64)
    y = rng.uniform(-0.5, 1.0, 64)
    y[:4] = [-0.5, 1.0, -0.5 + 1e-9, 1.0 - 1e-9]           # on the walls and next to them
    model = S.ShallowWaterModel(g, particles=S.LagrangianParticles(x, y))
    # a flow into both walls at the particles (v = 0 on the wall faces themselves)
    model.set(u=lambda X, Y: 0.5 + 0 * X, v=lambda X, Y: 2.0 * np.sin(np.pi * (Y + 0.5) / 1.5) * np.cos(np.pi * X), h=lambda X, Y: 1.0 + 0 * X,
              A=lambda X, Y: 0.0 * X)
    for _ in range(10):
        model.time_step(0.01)
    torch.cuda.synchronize()
    xs, ys = model.particles.x.cpu().numpy(), model.particles.y.cpu().numpy()
    assert np.all(np.isfinite(xs)) and np.all(np.isfinite(ys))
    assert np.all((ys >= -0.5) & (ys <= -0.5 + 12 * g.dy)) and np.all((xs >= 0.0) & (xs <= 16 * g.dx))
    assert not np.array_equal(ys[4:], y[4:])
    assert np.all(np.isfinite(model.particles.sample(("v", "A")).cpu().numpy()))


def test_uniform_flow_carries_the_particles(swmhd):
    S = swmhd
    x0, Lx, U0, dt, n = -1.0, 2.0, 0.75, 0.02, 10
    g = S.RectilinearGrid(size=(32, 24), x=(x0, x0 + Lx), y=(0.0, 1.5))
    rng = np.random.default_rng(8)
    x = x0 + Lx * rng.random(100)
    x[:3] = [x0 + Lx - 0.01, x0 + Lx - 0.1, x0 + Lx - 0.149]      # these cross the wrap within t U0 = 0.15
    y = 1.5 * rng.random(100)
    model = S.ShallowWaterModel(g, coriolis_f=0.0, particles=S.LagrangianParticles(x, y))
    model.set(u=lambda X, Y: U0 + 0 * X, v=lambda X, Y: 0.0 * X, h=lambda X, Y: 1.0 + 0 * X, A=lambda X, Y: 0.0 * X)
    for _ in range(n):
        model.time_step(dt)
    t = n * dt
    u_final = model.solution["u"].numpy()[g.interior]
    du = np.abs(u_final - U0).max()
    # the bound: the flow's own departure from U0, read back from the final state, over the time of the run, plus one rounding of a
    # position (at most |x0| + Lx in magnitude) per stage
    eps = np.finfo(np.float64).eps
    bound = t * du + 3 * n * eps * (abs(x0) + Lx)
    got = model.particles.x.cpu().numpy()
    want = PC.fold(x + U0 * t, x0, 32 * g.dx, PC.WRAP)
    d = np.abs(got - want)
    d = np.minimum(d, np.abs(Lx - d))        # (the distance in the periodic box: a particle within the bound of the seam may sit on either side)
    print("uniform flow: max|u - U0|", du, "bound", bound, "max error", d.max())
    assert np.sum(want < x) >= 3             # particles did cross the wrap
    assert d.max() <= bound
    same_bits(model.particles.y.cpu().numpy(), y, "y in a flow with v = 0")


def test_particle_time_series(swmhd, tmp_path):
    S = swmhd
    g = S.RectilinearGrid(size=(32, 24), x=(-1.0, 1.0), y=(0.0, 1.5))
    x, y = _seeds(g, 50)
    model = S.ShallowWaterModel(g, tracers=("c",), particles=S.LagrangianParticles(x, y, tracked_fields=("A",)))
    model.set(**_initial(S, g, model), c=lambda X, Y: X + Y)
    w = S.ParticleTimeSeries(model, names=("x", "A", "y", "c"), schedule=S.IterationInterval(2), capacity=3)
    S.run(model, DT, stop_iteration=4, writers=[w])
    assert len(w) == 3 and w.iterations == [0, 2, 4] and tuple(w.samples.shape) == (3, 4, 50) and w.samples.dtype == torch.float64
    last = w.numpy()[-1]
    same_bits(last[0], model.particles.x.cpu().numpy(), "the series' last x")
    same_bits(last[2], model.particles.y.cpu().numpy(), "the series' last y")
    same_bits(last[[1, 3]], model.particles.sample(("A", "c")).cpu().numpy(), "the series' last A, c")
    path = str(tmp_path / "particles.npz")
    w.save(path)
    z = np.load(path)
    assert z["samples"].shape == (3, 4, 50) and list(z["names"]) == ["x", "A", "y", "c"] and list(z["iterations"]) == [0, 2, 4]
    with pytest.raises(S._lib.SwmhdError, match="x, y or one of"):
        S.ParticleTimeSeries(model, names=("x", "s"), capacity=2)
    with pytest.raises(S._lib.SwmhdError, match="no particles"):
        S.ParticleTimeSeries(S.ShallowWaterModel(g), capacity=2)
    ens = S.ShallowWaterEnsemble(g, 2, particles=S.LagrangianParticles(x, y))
    ens.set(**_initial(S, g, model))
    we = S.ParticleTimeSeries(ens, schedule=S.IterationInterval(1), capacity=2)
    S.run(ens, DT, stop_iteration=1, writers=[we])
    assert tuple(we.samples.shape) == (2, 2, 3, 50)
    same_bits(we.numpy()[1][:, 0], ens.particles.x.cpu().numpy(), "ensemble series x")
