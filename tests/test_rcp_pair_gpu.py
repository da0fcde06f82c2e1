"""The shared reciprocals and the five-instruction velocity indicator of the fp64 vector-invariant row-marching kernel (sw_device.inc
MARCH64: weno_combine_finish_pair for the x-face and the y-face fluxes of h and A, weno_betas4_vel; lorentz_device.inc: the two face
reciprocals of jac_force from one) against the float64 oracle.

As tests/test_weno_arith_gpu.py, whose field sets, shapes, layouts and bounds this file uses: one evaluation per stage variant T (MODE 4),
A1 (MODE 9), A2 (MODE 11) through the C-ABI with SWMHD_MARCH_KERNEL, at 300 x 24 and 506 x 20 (halo lanes, a short last strip, segments
shorter than a window), on 128-lane strips (the default chooser) and, in a child process with SWMHD_T_NT=256, on 256-lane strips with a
folded last strip.  Bound: the project's own (include/swmhd.h),
    max|dG| <= tol * max(max|G|, S),  tol = 1e-13 (1e-12 on the rough random set),
and the substep outputs with test_weno_arith_gpu.bounds at that tol.

Two field sets more, for what a product of two denominators S1 S2 ~ b^12 could get wrong:
    5 scaled     smooth fields of both signs, all four multiplied by 1e8: indicators of h and A b = 3e8 .. 1.6e14, S up to 5e85, S1 S2 up to 6e167
    6 perturbed  a constant state (u, v, h, A) = (0.3, -0.2, 1, 0.5) plus 1e-8 N(0,1) on each: b = 4 eps to eight digits, S1 S2 = 1.9e-64,
                 the low end of the range
(tests/test_rcp_pair_cpu.py: the oracle is finite and well-conditioned on both), and a 20-step anchor-form run that must repeat bitwise."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as Hh
import stage_cases as SC
import test_weno_arith_gpu as WA

pytestmark = pytest.mark.gpu
ROOT = WA.ROOT
SHAPES = WA.SHAPES
SETS = dict(WA.SETS, scaled=1e-13, perturbed=1e-13)      # field set: tol
H = SC.H


def fields(name, Nx, Ny, seed):
    """Parents (u, v, h, A) of a field set, halos periodic-filled: test_weno_arith_gpu's four and the two of this file."""
    if name in WA.SETS:
        return WA.fields(name, Nx, Ny, seed)
    shp = (Ny + 2 * H, Nx + 2 * H)
    j, i = np.meshgrid(np.arange(shp[0]) - H, np.arange(shp[1]) - H, indexing="ij")
    X, Y = 2 * np.pi * i / Nx, 2 * np.pi * j / Ny
    ph = 1e-4 * (seed % 10000)                                # (the operand state of A2 is a second state of the same make)
    if name == "scaled":
        q = [0.3 * np.sin(2 * X + 0.3 + ph) * np.cos(Y), 0.3 * np.cos(3 * X + ph) * np.sin(Y + 0.7),
             1.25 + 0.75 * np.sin(2 * X + 1.0 + ph) * np.cos(Y + 0.2), np.cos(3 * X + 0.5 + ph) * np.sin(Y + 0.1)]
        q = [1e8 * a for a in q]
    elif name == "perturbed":
        r = [np.random.default_rng([seed, k]) for k in range(4)]
        q = [c + 1e-8 * r[k].standard_normal(shp) for k, c in enumerate((0.3, -0.2, 1.0, 0.5))]
    else:
        raise KeyError(name)
    return [np.ascontiguousarray(Hh.fill_halo_periodic(a, Nx, Ny, H, H)) for a in q]


class Data(WA.Data):
    """test_weno_arith_gpu.Data with the field sets of this file."""

    def __init__(self, oracle, name, Nx, Ny, lor):
        self.Nx, self.Ny, self.form, self.lor, self.dtype = Nx, Ny, 1, lor, np.dtype(np.float64)
        self.q = fields(name, Nx, Ny, 7000 + Nx)
        self.aux = fields(name, Nx, Ny, 9000 + Nx)
        for a in self.aux:
            keep = Hh.interior(a, Nx, Ny, H, H).copy()
            a[...] = SC.SENTINEL
            Hh.interior(a, Nx, Ny, H, H)[...] = keep
        self.dx, self.dy, self.grav, self.fcor = SC.DX, SC.DY, float(SC.GRAV), float(SC.FCOR)
        G = oracle.tendencies(*self.q, Nx, Ny, H, H, self.dx, self.dy, 1, lor, self.grav, self.fcor, nthreads=SC.NTHREADS)
        self.G = [Hh.interior(g, Nx, Ny, H, H).copy() for g in G]
        force = 0.0
        if lor:
            F = oracle.lorentz_jacobian(self.q[3], self.q[2], Nx, Ny, H, H, self.dx, self.dy, nthreads=SC.NTHREADS)
            force = max(float(np.abs(Hh.interior(w, Nx, Ny, H, H)).max()) for w in F)
        self.force = force
        self.scales = [float(s) for s in Hh.term_scales("VectorInvariant", self.q, self.dx, self.dy, force)]
        self.Gmax = [float(np.abs(g).max()) for g in self.G]
        self.Umax = [float(np.abs(Hh.interior(a, Nx, Ny, H, H)).max()) for a in self.q]


_DATA = {}


def data_of(oracle, name, Nx, Ny, lor):
    key = (name, Nx, Ny, lor)
    if key not in _DATA:
        _DATA[key] = Data(oracle, name, Nx, Ny, lor)
    return _DATA[key]


def run_set(S, oracle, name, Nx, Ny, lor, lanes):
    """The three variants of one (field set, shape, forcing): (failures, {variant: worst error / bound})."""
    geo = S._lib.tendency_launch_geometry(Nx, Ny, 1, 8, SC.MARCH_KERNEL)
    tail = Nx - (geo["nstrips"] - 1) * SC.TXO[geo["threads"]]
    assert (geo["kind"], geo["threads"], geo["nstrips"], tail) == (2, lanes) + WA.LAYOUT[lanes][Nx], geo
    data = data_of(oracle, name, Nx, Ny, lor)
    tol = SETS[name]
    fails, ratios = [], {}
    for variant in WA.VARIANTS:
        coeffs = SC.COEFFS["rk3"][variant]
        dt = data.dt(coeffs[0])
        operand = data.aux if variant == "A2" else None
        ref = SC.reference_stage(oracle, data.q, operand, variant, coeffs, Nx, Ny, data.dx, data.dy, 1, lor, dt, G=data.G)
        bnd = WA.bounds(data, tol, variant, coeffs, dt, ref)
        out = SC.run_stage(S, data, variant, "rk3")
        for key in bnd:
            for f in range(4):
                got = Hh.interior(out[key][1][f], Nx, Ny, H, H).astype(np.longdouble)
                if not np.isfinite(got).all():
                    fails.append(f"{variant} {key}[{f}]: non-finite")
                    continue
                err = float(np.abs(got - ref[key][f]).max())
                ratios[variant] = max(ratios.get(variant, 0.0), err / bnd[key][f])
                if not err <= bnd[key][f]:
                    fails.append(f"{variant} {key}[{f}]: max error {err:.3e} > bound {bnd[key][f]:.3e}")
    print(f"  {name} {Nx}x{Ny} lor{lor} {lanes} lanes: error / bound " + ", ".join(f"{v} {r:.3g}" for v, r in ratios.items()))
    return fails, ratios


@pytest.mark.parametrize("lor", [1, 0])
@pytest.mark.parametrize("name", list(SETS))
@pytest.mark.parametrize("Nx,Ny", SHAPES)
def test_rcp_pair_default_layout(swmhd, oracle, Nx, Ny, name, lor):
    """128-lane strips (what the chooser gives these widths)."""
    assert not os.environ.get("SWMHD_T_NT") and not os.environ.get("SWMHD_T_LY"), "layout knobs set: the default chooser is not what runs"
    fails, _ = run_set(swmhd, oracle, name, Nx, Ny, lor, 128)
    assert not fails, "\n".join(fails)


def test_rcp_pair_256_lanes(swmhd, tmp_path):
    """The same cases on 256-lane strips with a folded last strip (250 + 50 and 250 + 250 + 6 columns): SWMHD_T_NT=256 in one child
    process, which stops at its first failure."""
    env = {k: v for k, v in os.environ.items() if k not in ("SWMHD_T_NT", "SWMHD_T_LY", "SWMHD_T_FOLD")}
    env["SWMHD_T_NT"] = "256"
    out = tmp_path / "nt256.json"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], env=env, capture_output=True, text=True, timeout=300)
    res = json.load(open(out)) if out.exists() else None
    assert r.returncode == 0 and res and res["ok"], (res and res["failed"], r.stdout[-3000:], r.stderr[-3000:])
    print(r.stdout)
    assert len(res["ratios"]) == len(SHAPES) * len(SETS) * 2


def test_twenty_anchor_steps_repeat_bitwise(swmhd):
    """20 fused RK3 steps (anchor form) of the rough set at 506 x 20 on the marching kernel, twice from the same state: finite and
    bitwise equal.  dt = 1e-5: the tendencies of these fields reach 2.5e3, so a step changes the state by a few per cent."""
    import torch
    S = swmhd
    Nx, Ny = SHAPES[1]
    q = fields("rough", Nx, Ny, 7000 + Nx)
    runs = []
    for _ in range(2):
        g = S.RectilinearGrid(size=(Nx, Ny), x=(0, SC.DX * Nx), y=(0, SC.DY * Ny))
        m = S.ShallowWaterModel(g, float(SC.GRAV), float(SC.FCOR), kernel="march")
        for f_, a in zip(m.fields, q):
            f_.data.copy_(torch.from_numpy(a))
        m.time_steps(20, 1e-5)
        m.synchronize()
        runs.append([f_.numpy()[g.interior].copy() for f_ in m.fields])
    for a, b in zip(*runs):
        assert np.isfinite(a).all()
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert any(not np.array_equal(a, Hh.interior(p, Nx, Ny, H, H)) for a, p in zip(runs[0], q))      # (the steps did run)


def child_main(out_path):
    """Child of test_rcp_pair_256_lanes: every case with SWMHD_T_NT=256 in the environment."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import swmhd_amd as S
    from oracle import oracle as O
    assert os.environ.get("SWMHD_T_NT") == "256"
    failed, ratios = [], {}
    for Nx, Ny in SHAPES:
        for name in SETS:
            for lor in (1, 0):
                if failed:
                    break
                fails, r = run_set(S, O, name, Nx, Ny, lor, 256)
                ratios[f"{name}-{Nx}x{Ny}-lor{lor}"] = r
                failed += [f"{name} {Nx}x{Ny} lor{lor}: {m}" for m in fails]
    with open(out_path, "w") as fh:
        json.dump({"ok": not failed, "failed": failed, "ratios": ratios}, fh, indent=1, sort_keys=True)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(child_main(sys.argv[1]))
