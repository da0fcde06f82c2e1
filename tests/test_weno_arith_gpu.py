"""The arithmetic of the fp64 vector-invariant row-marching kernel (sw_device.inc MARCH64: fused velocity-stencil indicator sums, the
three-fma tail of the WENO combination, one-Newton-step reciprocals in the Lorentz force, the Bernoulli sum Kh + g h formed once per
cell) against the float64 oracle, on field sets chosen for what each reformulation could get wrong.

One evaluation per stage variant the RK3 step and the tendency entry point use -- T (MODE 4), A1 (MODE 9), A2 (MODE 11) of
tests/stage_cases.py -- through the C-ABI with SWMHD_MARCH_KERNEL (kernel_variant 2), compared as tests/test_stage_matrix_gpu.py does:
    max|dG| <= tol * max(max|G|, S),  S = helpers.term_scales            (include/swmhd.h)
    tol = 1e-12 on set 1 (rough random fields of order one), 1e-13 on sets 2-4
and the substep outputs with the bound of stage_cases.stage_bounds at that tol.

Shapes: 300 x 24 and 506 x 20 (4 segments of 6 rows, the last of 6 / 2).  The default chooser gives both 128-lane strips (122 + 122 +
56 and 4 x 122 + 18 columns); with SWMHD_T_NT=256 (a read-once knob, hence a child process) they are 250 + 50 and 250 + 250 + 6
columns, whose last strip runs as a folded half-strip.  Both layouts run: the 128- and the 256-lane variants carry the same arithmetic.

Field sets:
    1 rough     u, v ~ 0.5 N(0,1), h = 1 + 0.3 U(0,1), A ~ N(0,1): both signs of u and of v inside every 64-column wave row, so both
                sides of every reconstruction run in one wave
    2 uniform   h = 1 + 1e-10 noise, u, v = 1e-3 noise, A = 1e-10 noise: every smoothness indicator is of the order of eps, so where
                eps enters the fused indicator sums decides the weights
    3 deep      h = 1e3 (1 + 0.1 smooth relief), u, v of order 1e-3: Kh + g h is g h to 13 digits
    4 magnetic  A of amplitude 1e3 over h in [0.5, 2]: the Lorentz force, through the one-step reciprocals, is the largest term
and a 20-step anchor-form run of set 1 on the marching kernel that must repeat bitwise."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as Hh
import stage_cases as SC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(300, 24), (506, 20)]
SETS = {"rough": 1e-12, "uniform": 1e-13, "deep": 1e-13, "magnetic": 1e-13}      # field set: tol
VARIANTS = ("T", "A1", "A2")                                                    # stage MODE 4, 9, 11
LAYOUT = {128: {300: (3, 56), 506: (5, 18)}, 256: {300: (2, 50), 506: (3, 6)}}  # lanes: Nx: (strips, columns of the last strip)
H = SC.H


def fields(name, Nx, Ny, seed):
    """Parents (u, v, h, A) of a field set, halos periodic-filled."""
    shp = (Ny + 2 * H, Nx + 2 * H)
    r = [np.random.default_rng([seed, k]) for k in range(4)]
    j, i = np.meshgrid(np.arange(shp[0]) - H, np.arange(shp[1]) - H, indexing="ij")
    X, Y = 2 * np.pi * i / Nx, 2 * np.pi * j / Ny          # periodic over the interior
    if name == "rough":
        q = [0.5 * r[0].standard_normal(shp), 0.5 * r[1].standard_normal(shp), 1.0 + 0.3 * r[2].random(shp), r[3].standard_normal(shp)]
    elif name == "uniform":
        q = [1e-3 * r[0].standard_normal(shp), 1e-3 * r[1].standard_normal(shp), 1.0 + 1e-10 * r[2].standard_normal(shp),
             1e-10 * r[3].standard_normal(shp)]
    elif name == "deep":
        q = [1e-3 * np.sin(3 * X + 0.3) * np.cos(Y), 1e-3 * np.cos(2 * X) * np.sin(Y + 0.7),
             1e3 * (1.0 + 0.1 * np.sin(2 * X + 1.0) * np.cos(Y + 0.2)), np.cos(3 * X) * np.sin(Y)]
    elif name == "magnetic":
        q = [0.3 * np.sin(2 * X + 0.3) * np.cos(Y), 0.3 * np.cos(3 * X) * np.sin(Y + 0.7),
             1.25 + 0.75 * np.sin(2 * X + 1.0) * np.cos(Y + 0.2), 1e3 * np.cos(3 * X + 0.5) * np.sin(Y + 0.1)]
    else:
        raise KeyError(name)
    return [np.ascontiguousarray(Hh.fill_halo_periodic(a, Nx, Ny, H, H)) for a in q]


class Data(SC.StageData):
    """stage_cases.StageData of a named field set (vector-invariant, fp64); the operand W of A2 is a second state of the same make."""

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


def bounds(data, tol, variant, coeffs, dt, ref):
    """stage_cases.stage_bounds for T, A1 and A2 with the tolerance of the field set."""
    gam, zet = abs(coeffs[0]), abs(coeffs[1])
    tb = [tol * max(gm, s) for gm, s in zip(data.Gmax, data.scales)]
    if variant == "T":
        return {"Gn": tb}
    eps = float(np.finfo(np.float64).eps)
    amax = lambda a: float(np.abs(np.asarray(a, dtype=np.float64)).max())
    cut = lambda a: Hh.interior(a, data.Nx, data.Ny, H, H)
    base = data.aux if variant == "A2" else data.q
    out = {"qnew": [dt * gam * tb[f] + 4 * eps * max(amax(ref["qnew"][f]), dt * gam * data.Gmax[f], amax(cut(base[f]))) for f in range(4)]}
    if variant == "A1":
        out["Gn"] = [dt * zet * tb[f] + 4 * eps * max(amax(cut(data.q[f])), dt * zet * data.Gmax[f], amax(ref["Gn"][f])) for f in range(4)]
    return out


def run_set(S, oracle, name, Nx, Ny, lor, lanes):
    """The three variants of one (field set, shape, forcing): (failures, {variant: worst error / bound})."""
    geo = S._lib.tendency_launch_geometry(Nx, Ny, 1, 8, SC.MARCH_KERNEL)
    tail = Nx - (geo["nstrips"] - 1) * SC.TXO[geo["threads"]]
    assert (geo["kind"], geo["threads"], geo["nstrips"], tail) == (2, lanes) + LAYOUT[lanes][Nx], geo
    data = data_of(oracle, name, Nx, Ny, lor)
    tol = SETS[name]
    fails, ratios = [], {}
    for variant in VARIANTS:
        coeffs = SC.COEFFS["rk3"][variant]
        dt = data.dt(coeffs[0])
        operand = data.aux if variant == "A2" else None
        ref = SC.reference_stage(oracle, data.q, operand, variant, coeffs, Nx, Ny, data.dx, data.dy, 1, lor, dt, G=data.G)
        bnd = bounds(data, tol, variant, coeffs, dt, ref)
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


def test_rough_set_has_both_signs_in_every_wave():
    """Set 1 as promised: u and v change sign inside every 64-column block of every row (runs without a GPU's help, but belongs here)."""
    for Nx, Ny in SHAPES:
        for a in fields("rough", Nx, Ny, 7000 + Nx)[:2]:
            I = Hh.interior(a, Nx, Ny, H, H)
            for c0 in range(0, Nx, 64):
                blk = I[:, c0:c0 + 64]
                assert ((blk > 0).any(axis=1) & (blk < 0).any(axis=1)).all()


@pytest.mark.parametrize("lor", [1, 0])
@pytest.mark.parametrize("name", list(SETS))
@pytest.mark.parametrize("Nx,Ny", SHAPES)
def test_weno_arith_default_layout(swmhd, oracle, Nx, Ny, name, lor):
    """128-lane strips (what the chooser gives these widths)."""
    assert not os.environ.get("SWMHD_T_NT") and not os.environ.get("SWMHD_T_LY"), "layout knobs set: the default chooser is not what runs"
    fails, _ = run_set(swmhd, oracle, name, Nx, Ny, lor, 128)
    assert not fails, "\n".join(fails)


def test_weno_arith_256_lanes(swmhd, tmp_path):
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
    """20 fused RK3 steps (anchor form) of set 1 on the marching kernel, twice from the same state: finite and bitwise equal.
    dt = 1e-5: the tendencies of these fields reach 2.5e3 (test output above), so a step changes the state by a few per cent."""
    import torch
    S = swmhd
    Nx, Ny = SHAPES[0]
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
    """Child of test_weno_arith_256_lanes: every case with SWMHD_T_NT=256 in the environment."""
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
