"""GPU tests of the folded last strip of the fp64 vector-invariant row-marching kernel (tendency_march_kernels.inc, k_tendency_vi_march;
common.hpp march_geometry).  Where the last 256-lane strip has at most 122 output columns, its workgroups run two 128-lane sub-strips
on two segments.  The folded kernel must agree with the strict kernels at every width that folds (and at one just too wide to fold),
write no row outside the requested range, and give bitwise the results of the unfolded layout (SWMHD_T_FOLD=0) at the same rows per
segment."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TXO = 250   # output columns of a 256-lane strip
# widths whose last 256-lane strip has 1, 6, 96, 122 (folded) and 123 (not folded) output columns, all with 256-lane strips chosen
WIDTHS = {1: 2501, 6: 2506, 96: 1346, 122: 372, 123: 373}


def _rows_for(L, Nx, odd):
    """A row count of at least 330000 / Nx cells (the marching kernel) whose launch has an odd / even number of segments and a short
    last one."""
    r = -(-330000 // Nx)
    for rows in range(r, r + 4000):
        g = L.tendency_launch_geometry(Nx, rows, 1, 8, 0)
        if g["kind"] == 2 and g["nseg"] % 2 == (1 if odd else 0) and rows % g["rows_per_segment"] != 0:
            return rows, g
    raise AssertionError((Nx, odd))


def _state(S, Nx, Ny, seed):
    g = S.RectilinearGrid(size=(Nx, Ny), x=(0, 0.01 * Nx), y=(0, 0.01 * Ny))
    rng = np.random.default_rng(seed)
    P = g.parent_shape
    base = [0.3 * rng.standard_normal(P), 0.3 * rng.standard_normal(P), 1.0 + 0.1 * rng.random(P), 0.2 * rng.standard_normal(P)]
    return g, [S.Field(g, data=torch.from_numpy(b).cuda()) for b in base]


@pytest.mark.parametrize("rem", [1, 6, 96, 122, 123])
@pytest.mark.parametrize("odd", [True, False])
def test_folded_tendencies_match_strict(swmhd, rem, odd):
    """Unfused tendencies (fast, marching kernel) vs the strict kernels on rows [5, 5 + rows) of a grid with 12 more rows, halos read
    as they are: within the fast tolerance (1e-12 of max|G|); rows outside the range and the halos of G keep their sentinel."""
    S, L = swmhd, swmhd._lib
    Nx = WIDTHS[rem]
    rows, geo = _rows_for(L, Nx, odd)
    assert geo["threads"] == 256 and geo["nstrips"] == -(-Nx // TXO)      # 256-lane strips: the layout that folds
    folds = Nx - (geo["nstrips"] - 1) * TXO <= 122
    assert folds == (rem <= 122)
    j0, j1 = 5, 5 + rows
    g, U = _state(S, Nx, rows + 12, 1000 + rem)
    sy = U[0].stride_y
    out = {}
    for name, fl in (("fast", 0), ("strict", L.STRICT)):
        G = [S.Field(g, dtype=torch.float64) for _ in range(4)]
        for x in G:
            x.data.fill_(-555.5)
        L.check(L.lib().swmhd_tendencies_f64(*[x.ptr for x in U], *[x.ptr for x in G], g.Nx, g.Ny, g.Hx, g.Hy, sy, g.dx, g.dy, 9.81,
                                             1.0, 1, 1, j0, j1, fl, None), name)
        torch.cuda.synchronize()
        out[name] = [x.numpy() for x in G]
    I = g.interior
    for f, s in zip(out["fast"], out["strict"]):
        a, b = f[I][j0:j1], s[I][j0:j1]
        assert np.isfinite(a).all()
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()
        mask = np.ones(f.shape, bool)
        mask[g.Hy + j0:g.Hy + j1, g.Hx:g.Hx + Nx] = False
        assert np.all(f[mask] == -555.5)


@pytest.mark.parametrize("rem", [6, 96, 122])
def test_folded_fused_stage_matches_strict(swmhd, rem):
    """One fused RK3 stage of the classic form (the first stage writes U1 and G0) on an odd segment count: U1 and G0 of the
    fast kernel vs the strict one within the fast tolerance, and nothing outside the interior of either written."""
    S, L = swmhd, swmhd._lib
    Nx = WIDTHS[rem]
    rows, geo = _rows_for(L, Nx, True)
    assert geo["threads"] == 256
    g, U = _state(S, Nx, rows, 2000 + rem)
    sy = U[0].stride_y
    P = lambda fs: L.ptr_array([x.ptr for x in fs])
    out = {}
    for name, fl in (("fast", 0), ("strict", L.STRICT)):
        U1 = [S.Field(g, dtype=torch.float64) for _ in range(4)]
        G0 = [S.Field(g, dtype=torch.float64) for _ in range(4)]
        for x in U1 + G0:
            x.data.fill_(-555.5)
        L.check(L.lib().swmhd_tendencies_rk3_f64(P(U), P(U1), P(G0), None, g.Nx, g.Ny, g.Hx, g.Hy, sy, g.dx, g.dy, 9.81, 1.0, 1, 1,
                                                 1e-3, 8.0 / 15.0, 0.0, 1, 0, g.Ny, fl, None), name)
        torch.cuda.synchronize()
        out[name] = [x.numpy() for x in U1]
        out[name + " G0"] = [x.numpy() for x in G0]
    I = g.interior
    for f, s in zip(out["fast"], out["strict"]):
        assert np.abs(f[I] - s[I]).max() <= 1e-12 * np.abs(s[I]).max()
        mask = np.ones(f.shape, bool)
        mask[I] = False
        assert np.all(f[mask] == -555.5)
    # the stored tendencies G0: the bar of test_folded_tendencies_match_strict, and nothing outside the interior written
    for f, s in zip(out["fast G0"], out["strict G0"]):
        assert np.isfinite(f[I]).all()
        assert np.abs(f[I] - s[I]).max() <= 1e-12 * np.abs(s[I]).max()
        mask = np.ones(f.shape, bool)
        mask[I] = False
        assert np.all(f[mask] == -555.5)


_STEPS = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
import swmhd_amd as S
from swmhd_amd import configs
Nx, Ny = int(sys.argv[3]), int(sys.argv[4])
cfg = configs.config3_bickley()
g = S.RectilinearGrid(size=(Nx, Ny), x=cfg["domain"]["x"], y=cfg["domain"]["y"])
m = S.ShallowWaterModel(g)
m.set(u=cfg["u"], v=cfg["v"], h=lambda X, Y: cfg["h"](X, Y) + 0 * X, A=cfg["A"])
m.time_steps(4, 1e-4)
m.synchronize()
np.save(sys.argv[2], np.stack([f.numpy()[g.interior] for f in m.fields]))
"""


@pytest.mark.parametrize("force_ly", ["45", ""])
def test_fold_on_off(swmhd, tmp_path, force_ly):
    """Four fused RK3 steps of the model (anchor form) on a 4096 x 2048 grid (17 strips, the last one folded), in fresh processes with
    and without SWMHD_T_FOLD=0.  At the same rows per segment (SWMHD_T_LY=45): bitwise equal -- a folded lane runs the instructions of
    an unfolded one.  With the default rows per segment the two layouts also cut the rows differently (45 vs 46 rows at 4096 x 2048),
    and a segment's prologue forms the carried fluxes of its first row outside the loop, where the compiler may associate the same
    sums differently: equal within the fast tolerance (1e-12 of max|U|)."""
    script = tmp_path / "steps.py"
    script.write_text(_STEPS)
    res = []
    for fold in ("1", "0"):
        env = dict(os.environ, SWMHD_T_FOLD=fold)
        env.pop("SWMHD_T_LY", None)
        if force_ly:
            env["SWMHD_T_LY"] = force_ly
        out = tmp_path / f"fold{fold}.npy"
        r = subprocess.run([sys.executable, str(script), ROOT, str(out), "4096", "2048"], env=env, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        res.append(np.load(out))
    assert np.isfinite(res[0]).all()
    if force_ly:
        assert np.array_equal(res[0], res[1])
    else:
        for a, b in zip(*res):
            assert np.abs(a - b).max() <= 1e-12 * max(np.abs(b).max(), 1.0)
