"""GPU tests of the anchor form of the fused RK3 stages (swmhd.h SWMHD_RK3_ANCHOR, common.hpp Rk3Buffers).

With Oceananigans' coefficients gamma1 + zeta2 = 1/4 and zeta3 = -gamma2, so one RK3 step is exactly
    U1 = U0 + dt gamma1 G0,   W = U0 + (dt/4) G0,   U2 = W + dt gamma2 G1,   U3 = W + dt gamma3 G2.
The anchor form must agree with the classic G- form to rounding, stay as conservative over long runs, write W exactly as stated,
and address W through 32-bit byte offsets correctly for parents beyond 2 GiB."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GAMMA = (8.0 / 15.0, 5.0 / 12.0, 3.0 / 4.0)
ZETA = (0.0, -17.0 / 60.0, -5.0 / 12.0)


def _model(S, N, form, dtype, **kw):
    from test_model_oracle import hf, uf, vf, Af, Lx, Ly
    g = S.RectilinearGrid(size=(N, N), x=(0, Lx), y=(0, Ly))
    m = S.ShallowWaterModel(g, 9.81, 1.0, formulation=form, dtype=dtype, **kw)
    if form == "VectorInvariant":
        m.set(u=uf, v=vf, h=hf, A=Af)
    else:
        m.set(uh=lambda X, Y: hf(X, Y) * uf(X, Y), vh=lambda X, Y: hf(X, Y) * vf(X, Y), h=hf, A=Af)
    return m


def _eps(dtype):
    return float(np.finfo(np.float64 if dtype == torch.float64 else np.float32).eps)


@pytest.mark.parametrize("form", ["VectorInvariant", "Conservative"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("N", [96, 1024])
def test_anchor_step_equals_classic_step(swmhd, form, dtype, N):
    """One RK3 step through the ABI, anchor form vs classic G- form, on the LDS-tiled (N = 96) and the row-marching / packed-fp32
    (N = 1024) kernels: the same state within a few ulp of max|U|, after the first stage and after the step."""
    S, L = swmhd, swmhd._lib
    m = _model(S, N, form, dtype)
    g = m.grid
    dt = 2e-4 if N > 512 else 2e-3
    f = getattr(L.lib(), f"swmhd_tendencies_rk3_{m.sfx}")
    mk = lambda: [S.Field(g, dtype=dtype) for _ in range(4)]
    P = lambda fl: L.ptr_array([x.ptr for x in fl])
    U0 = list(m.fields)
    args = (g.Nx, g.Ny, g.Hx, g.Hy, U0[0].stride_y, g.dx, g.dy, 9.81, 1.0, m.form_code, m.lorentz_code)
    fl = L.WRAP_X | L.WRAP_Y
    # classic: U1 (G0), U2 (G1), U3
    c1, c2, c3, G0, G1, Gx = mk(), mk(), mk(), mk(), mk(), mk()
    L.check(f(P(U0), P(c1), P(G0), None, *args, dt, GAMMA[0], ZETA[0], 1, 0, g.Ny, fl, None), "classic 1")
    L.check(f(P(c1), P(c2), P(G1), P(G0), *args, dt, GAMMA[1], ZETA[1], 1, 0, g.Ny, fl, None), "classic 2")
    L.check(f(P(c2), P(c3), P(Gx), P(G1), *args, dt, GAMMA[2], ZETA[2], 0, 0, g.Ny, fl, None), "classic 3")
    # anchor: U1 and W, U2, U3
    a1, a2, a3, W, junk = mk(), mk(), mk(), mk(), mk()
    fa = fl | L.RK3_ANCHOR
    L.check(f(P(U0), P(a1), P(W), None, *args, dt, GAMMA[0], 0.25, 0, 0, g.Ny, fa, None), "anchor 1")
    L.check(f(P(a1), P(a2), P(junk), P(W), *args, dt, GAMMA[1], 0.0, 0, 0, g.Ny, fa, None), "anchor 2")
    L.check(f(P(a2), P(a3), P(W), P(W), *args, dt, GAMMA[2], 0.0, 0, 0, g.Ny, fa, None), "anchor 3")   # Gn may alias Gm
    torch.cuda.synchronize()
    I = g.interior
    eps = _eps(dtype)
    for x in junk:                                   # later anchored stages write no tendencies
        assert x.data.abs().max().item() == 0
    for what, cs, as_, ulps in (("stage 1", c1, a1, 2), ("step", c3, a3, 8)):
        for x, y in zip(cs, as_):
            A_, B_ = x.numpy()[I].astype(np.float64), y.numpy()[I].astype(np.float64)
            scale = np.abs(A_).max()
            err = np.abs(A_ - B_).max()
            assert np.isfinite(B_).all() and err <= ulps * eps * scale, f"anchor {what} off by {err / (eps * scale):.2f} ulp of max|U|"


@pytest.mark.parametrize("form", ["VectorInvariant", "Conservative"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("N", [96, 1024])
def test_anchor_stage_one_writes_W(swmhd, form, dtype, N):
    """The first anchored stage writes W = U0 + (dt/4) G0 into Gn: within 2 ulp of the value formed on the host from G0 of an unfused
    tendency call, plus (dt/4) times the rounding in which G0 itself may differ between two compiled kernel variants (the suite's fast-
    path bar: 1e-12 max|G| in fp64, 1e-4 in fp32).  Nothing outside the interior of W is written."""
    S, L = swmhd, swmhd._lib
    m = _model(S, N, form, dtype)
    g = m.grid
    dt = 2e-4 if N > 512 else 2e-3
    U0 = list(m.fields)
    G0 = [S.Field(g, dtype=dtype) for _ in range(4)]
    U1 = [S.Field(g, dtype=dtype) for _ in range(4)]
    W = [S.Field(g, dtype=dtype) for _ in range(4)]
    for x in W:
        x.data.fill_(-777.25)
    fl = L.WRAP_X | L.WRAP_Y
    L.check(getattr(L.lib(), f"swmhd_tendencies_{m.sfx}")(*[x.ptr for x in U0], *[x.ptr for x in G0], g.Nx, g.Ny, g.Hx, g.Hy,
                                                             U0[0].stride_y, g.dx, g.dy, 9.81, 1.0, m.form_code, m.lorentz_code,
                                                             0, g.Ny, fl, None), "tendencies")
    P = lambda fs: L.ptr_array([x.ptr for x in fs])
    L.check(getattr(L.lib(), f"swmhd_tendencies_rk3_{m.sfx}")(P(U0), P(U1), P(W), None, g.Nx, g.Ny, g.Hx, g.Hy, U0[0].stride_y, g.dx,
                                                                g.dy, 9.81, 1.0, m.form_code, m.lorentz_code, dt, GAMMA[0], 0.25, 0,
                                                                0, g.Ny, fl | L.RK3_ANCHOR, None), "anchor stage 1")
    torch.cuda.synchronize()
    I = g.interior
    eps = _eps(dtype)
    npdt = np.float64 if dtype == torch.float64 else np.float32
    dtw = npdt(npdt(dt) * npdt(0.25))
    for u, gg, w in zip(U0, G0, W):
        u_, g_ = u.numpy()[I].astype(np.float64), gg.numpy()[I].astype(np.float64)
        ref = u_ + float(dtw) * g_
        got = w.numpy()
        gtol = 1e-12 if dtype == torch.float64 else 1e-4
        tol = 2 * np.spacing(np.abs(ref).astype(npdt)).astype(np.float64) + float(dtw) * gtol * np.abs(g_).max()
        err = np.abs(got[I].astype(np.float64) - ref)
        assert np.all(err <= tol), f"W off by up to {(err / tol).max():.2f} x the bound"
        mask = np.ones(got.shape, bool)
        mask[I] = False
        assert np.all(got[mask] == npdt(-777.25))


@pytest.mark.parametrize("form", ["VectorInvariant", "Conservative"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("N", [96, 1024])
def test_anchor_form_over_200_steps(swmhd, form, dtype, N):
    """200 steps of the model: the fused stages run the anchor form, the unfused path (tendencies, then rk3_substep) the classic G-
    form with the same fast kernels.  The states stay close, and the anchor form drifts in total mass and energy no more than the
    classic form does."""
    S = swmhd
    dt = 2e-4 if N > 512 else 2e-3
    eps = _eps(dtype)
    runs = []
    for fused in (True, False):
        m = _model(S, N, form, dtype, fused=fused)
        g = m.grid
        mass = lambda: m.solution["h"].data[g.interior].double().sum().item()
        m0, e0 = mass(), m.diagnostics()["total_energy"]
        m.time_steps(200, dt)
        m.synchronize()
        runs.append(([x.data[g.interior].double().clone() for x in m.fields], abs(mass() - m0) / m0,
                     abs(m.diagnostics()["total_energy"] - e0) / e0))
        del m
    (ua, dma, dea), (uc, dmc, dec) = runs
    state_tol = 1e-10 if dtype == torch.float64 else 2e-3
    for a, c in zip(ua, uc):
        assert torch.isfinite(a).all()
        assert (a - c).abs().max().item() <= state_tol * c.abs().max().item()
    assert dma <= 2 * dmc + 64 * eps, (dma, dmc)
    assert dea <= dec + (1e-10 if dtype == torch.float64 else 1e-4), (dea, dec)


@pytest.mark.parametrize("form", ["VectorInvariant", "Conservative"])
def test_anchor_W_stores_beyond_2GiB(swmhd, form):
    """Parents of 2.16 GiB (16384 x 16400 fp64): the first anchored stage stores W through the G-buffer descriptors at byte offsets
    beyond 2^31 (every top row), and the later stages read it there.  Row-marching kernel vs LDS-tiled kernel (64-bit addressing),
    compared on the GPU for all three stages of a step; nothing outside the interior of W is touched."""
    Nx, Ny, H = 16384, 16400, 3
    S = swmhd
    g = S.RectilinearGrid(size=(Nx, Ny), x=(0, 2 * np.pi), y=(0, 2 * np.pi), halo=(H, H))
    assert (Ny + 2 * H) * (Nx + 2 * H) * 8 > 2 ** 31
    yy = torch.arange(Ny + 2 * H, device="cuda", dtype=torch.float64).reshape(-1, 1) * (2 * np.pi / Ny)
    xx = torch.arange(Nx + 2 * H, device="cuda", dtype=torch.float64).reshape(1, -1) * (2 * np.pi / Nx)
    base = [0.4 * torch.sin(xx) * torch.cos(2 * yy) + 0.2, 0.3 * torch.cos(2 * xx) * torch.sin(yy) - 0.1,
            1.0 + 0.2 * torch.sin(xx + 0.3) * torch.cos(yy), 0.3 * torch.sin(xx) * torch.sin(yy - 0.5)]
    del xx, yy
    res = []
    I = g.interior
    for kern in ("march", "tile"):
        m = S.ShallowWaterModel(g, 9.81, 1.0, formulation=form, kernel=kern, fuse_halo=False)
        for f, b in zip(m.fields, base):
            f.data.copy_(b)
        if form == "Conservative":
            m.fields[0].data.mul_(m.fields[2].data); m.fields[1].data.mul_(m.fields[2].data)
        m.update_state()
        out = []
        for stage in range(3):
            m._stage_fused(1e-5, stage)
            if stage == 0:   # W in Gn, U1 in the alternate buffers
                torch.cuda.synchronize()
                out += [f.data[I][-64:].clone() for f in m.Gn] + [f.data[I][:64].clone() for f in m.Gn]
                for f in m.Gn:
                    assert f.data[:H].abs().max().item() == 0 and f.data[-H:].abs().max().item() == 0
                    assert f.data[:, :H].abs().max().item() == 0 and f.data[:, -H:].abs().max().item() == 0
            m._state, m._alt = m._alt, m._state
            m.Gn, m.Gm = m.Gm, m.Gn
            m.update_state()
        torch.cuda.synchronize()
        out += [f.data[I][-64:].clone() for f in m.fields] + [f.data[I][:64].clone() for f in m.fields]
        res.append(out)
        del m
        torch.cuda.empty_cache()
    for a, b in zip(*res):
        assert torch.isfinite(a).all()
        assert (a - b).abs().max().item() <= 2e-11 * max(b.abs().max().item(), 1.0)
