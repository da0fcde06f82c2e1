"""Full-size oracle parity of the FAST marching kernels on every single-GPU BASELINE workload:
config 2 (1024^2, conservative + divergence forcing), config 3 (4096^2, vector-invariant + Jacobian forcing: the geometry
bench.py times), config 4 slab (8192 x 1024) and config 5 slab (16384 x 2048, fp64 and fp32).

The reference's own full-grid evaluate-and-compare loop is test_formulations.jl:151-189 (every cell of the grid, max-norm);
here the same loop runs at the BASELINE sizes: one Lorentz-operator evaluation and one fused-tendency evaluation, HIP (through the
C-ABI) against the CPU oracle on all host threads -- once on the initial condition and once on the state five RK3 steps later
(configs 2 and 4 start from rest, so only the later state exercises the momentum fluxes).

Tolerance (stated, asserted, and the achieved error is recorded in gpurun_out/fullsize_parity.json):
    max|G_hip - G_oracle| <= TOL * max(max|G|, S),   TOL = 1e-13 (fp64), 2e-5 (fp32 operators), 1e-4 (fp32 tendencies)
(achieved on MI355X, profiles/r03/fullsize_parity.json: <= 5e-15 in fp64, <= 5e-7 in fp32, relative to max(max|G|, S))
S is the magnitude of the largest TERM summed into the tendency (flux / dx, g h / dx, ...): rounding errors scale with the terms,
not with their sum, and at these resolutions the sum is often orders of magnitude smaller than its terms (config 3: the mass
fluxes u h / dx are ~650 while G_h = -div(u h) is ~3e-4, so one ulp of a flux is 2e-10 of max|G_h| in fp64 and 0.15 in fp32 -- the
"0.16 relative error" of the round-1 fp32 sweep was this cancellation, not a kernel defect).  Errors relative to max|G| alone
are recorded as well.
"""
import json
import os

import numpy as np
import pytest
import torch

from helpers import term_scales

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "gpurun_out", "fullsize_parity.json")
NTHREADS = max(1, min(len(os.sched_getaffinity(0)), 32))
G, F = 9.81, 1.0


def record(key, value):
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    d = json.load(open(OUT)) if os.path.exists(OUT) else {}
    d[key] = value
    json.dump(d, open(OUT, "w"), indent=1, sort_keys=True)


def compare(tag, names, got, want, scales, tol, I):
    rec, ok = {}, True
    for n, g_, w, s in zip(names, got, want, scales):
        err = float(np.abs(g_[I].astype(np.float64) - w[I].astype(np.float64)).max())
        gmax = float(np.abs(w[I]).max())
        ref = max(gmax, float(s))
        rec[n] = {"max_abs_err": err, "max_abs_G": gmax, "term_scale": float(s), "err_over_maxG": err / gmax if gmax > 0 else err,
                  "err_over_scale": err / ref if ref > 0 else err, "tol": tol}
        ok = ok and (err <= tol * ref)
    record(tag, rec)
    print(tag, json.dumps(rec))
    assert ok, f"{tag}: out of tolerance: {rec}"


CASES = [("config2", torch.float64), ("config3", torch.float64), ("config4_slab", torch.float64),
         ("config5_slab", torch.float64), ("config5_slab", torch.float32)]


@pytest.mark.parametrize("name,dtype", CASES, ids=[f"{n}-{'f64' if d == torch.float64 else 'f32'}" for n, d in CASES])
def test_fast_kernels_match_oracle_at_baseline_size(swmhd, oracle, name, dtype):
    from swmhd_amd import configs
    S, O = swmhd, oracle
    m, g, cfg = configs.build_model(S, name, dtype=dtype, kernel="march")
    form = m.formulation
    fcode, lcode = (1, 1) if form == "VectorInvariant" else (0, 2)
    f64 = dtype == torch.float64
    sfx = "f64" if f64 else "f32"
    I = g.interior
    op = S.lorentz_force_func if fcode == 1 else S.div_lorentz
    oop = O.lorentz_jacobian if fcode == 1 else O.lorentz_divergence
    dt = 0.2 * min(g.dx, g.dy) / 4.2
    for phase in ("initial", "after_5_steps"):
        if phase == "after_5_steps":
            m.time_steps(5, dt)
        m.synchronize()
        q = [f.numpy() for f in m.fields]
        # --- the reference's own hot path: whole-field Lorentz force ---
        Fx, Fy = op(g, {"A": m.solution["A"], "h": m.solution["h"]}, kernel="march")
        torch.cuda.synchronize()
        want = oop(q[3], q[2], g.Nx, g.Ny, 3, 3, g.dx, g.dy, nthreads=NTHREADS)
        fmax = max(float(np.abs(w[I]).max()) for w in want)
        # terms of the force: (grad A) * (difference of B = grad A / h over one cell) / h
        gA = max(float(np.abs(np.diff(q[3], axis=1)).max()) / g.dx, float(np.abs(np.diff(q[3], axis=0)).max()) / g.dy)
        s_op = gA * (gA / float(q[2].min())) * (1 / g.dx + 1 / g.dy) / float(q[2].min())
        compare(f"{name}/{sfx}/{phase}/lorentz_operator", ["Fx", "Fy"], [Fx.numpy(), Fy.numpy()], want, [s_op, s_op],
                1e-13 if f64 else 2e-5, I)
        # --- fused tendency evaluation (calculate_tendencies!: 4 fields in, 4 tendencies out, forcing fused) ---
        m.calculate_tendencies()
        torch.cuda.synchronize()
        got = [f.numpy() for f in m.Gn]
        wantG = O.tendencies(*q, g.Nx, g.Ny, 3, 3, g.dx, g.dy, fcode, lcode, G, F, nthreads=NTHREADS)
        compare(f"{name}/{sfx}/{phase}/tendencies", list(m.names), got, wantG, term_scales(form, q, g.dx, g.dy, fmax),
                1e-13 if f64 else 1e-4, I)
        del got, wantG, want


def test_config5_precision_sweep_at_slab_size(swmhd):
    """BASELINE config 5: fp32 vs fp64 from identical fp64 initial conditions at the 16384 x 2048 slab -- max|F32 - F64| after one
    RHS evaluation (relative to max(max|G|, term scale): the fp32 run also rounds its INPUTS, so cancelling terms lose
    eps32 * |term|) and of the state after 10 and 100 RK3 steps (relative to max|state|; u and v relative to the common velocity scale max(|u|, |v|))."""
    from swmhd_amd import configs
    S = swmhd
    ms = {}
    for key, dtype in (("f64", torch.float64), ("f32", torch.float32)):
        ms[key], g, cfg = configs.build_model(S, "config5_slab", dtype=dtype)
    I = g.interior
    dt = 0.2 * min(g.dx, g.dy) / 4.2
    rec = {"grid": f"{g.Nx}x{g.Ny}", "dt": dt}
    q = [f.numpy() for f in ms["f64"].fields]
    for m in ms.values():
        m.calculate_tendencies()
    torch.cuda.synchronize()
    scales = term_scales("VectorInvariant", q, g.dx, g.dy, 0.0)
    rec["tendencies_1_eval"] = {}
    for n, a, b, s in zip(ms["f64"].names, ms["f32"].Gn, ms["f64"].Gn, scales):
        d = float((a.data[I].double() - b.data[I]).abs().max()); gm = float(b.data[I].abs().max())
        rec["tendencies_1_eval"][n] = {"err_over_maxG": d / gm, "err_over_scale": d / max(gm, s)}
        assert d <= 4e-6 * max(gm, s), (n, d, gm, s)      # a few eps32 (6e-8) of the largest term
    done = 0
    for nsteps, bar in ((10, 2e-5), (100, 2e-4)):
        for m in ms.values():
            m.time_steps(nsteps - done, dt)
            m.synchronize()
        done = nsteps
        r = {}
        vel = max(float(ms["f64"].solution[n].data[I].abs().max()) for n in ms["f64"].names[:2])
        for n in ms["f64"].names:
            a, b = ms["f32"].solution[n].data[I].double(), ms["f64"].solution[n].data[I]
            # u and v are measured against the common velocity scale: v is a 1e-4 perturbation of a jet with |u| ~ 1
            ref = vel if n in ms["f64"].names[:2] else float(b.abs().max())
            r[n] = float((a - b).abs().max()) / ref
            assert r[n] <= bar, (n, nsteps, r[n])
        rec[f"state_after_{nsteps}_steps"] = r
    e64, e32 = ms["f64"].diagnostics()["total_energy"], ms["f32"].diagnostics()["total_energy"]
    rec["energy_f64"], rec["energy_f32"] = e64, e32
    assert abs(e32 - e64) <= 1e-5 * abs(e64)
    record("config5_slab/precision_sweep", rec)
    print("config5 precision sweep", json.dumps(rec))
