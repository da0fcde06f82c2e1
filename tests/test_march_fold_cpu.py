"""CPU tests of the folded last strip of the fp64 vector-invariant row-marching kernel (common.hpp march_geometry,
tendency_march_kernels.inc k_tendency_vi_march): the launch geometry it implies, and the register / LDS budgets of every variant of the
kernel on a gfx950 cross-compile of the fast tendency object."""
import json
import os
import subprocess
import sys

from test_rk3_anchor_cpu import _resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_3WG = 160 * 1024 // 3   # bytes of LDS per workgroup at 3 workgroups per CU (53.3 KB)


def _geometry(fold_env, *shape):
    """swmhd_tendency_launch_geometry in a fresh process (SWMHD_T_* knobs are read once per process)."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("SWMHD_T_")}
    if fold_env is not None:
        env["SWMHD_T_FOLD"] = fold_env
    code = ("import sys, json; sys.path.insert(0, sys.argv[1]); import swmhd_amd as S; "
            "print(json.dumps([S._lib.tendency_launch_geometry(int(a), int(b), 1, 8, 0) for a, b in zip(sys.argv[2::2], sys.argv[3::2])]))")
    r = subprocess.run([sys.executable, "-c", code, ROOT, *map(str, shape)], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout)


def test_fold_geometry(swmhd):
    """4096 columns: 17 strips either way (the query's layout is unchanged); folded, a segment row costs 16.5 workgroups, so 46 segments
    of 90 rows fit the 768 workgroup slots of one round (16 x 46 + 23 = 759) instead of 45 of 92 (765).  SWMHD_T_FOLD=0 restores the
    unfolded layout.  1024 columns keep 128-lane strips (nothing folds there)."""
    on, big, n1024 = _geometry(None, 4096, 4096, 4096, 2048, 1024, 1024)
    off, big_off = _geometry("0", 4096, 4096, 4096, 2048)
    assert on["nstrips"] == off["nstrips"] == 17 and on["threads"] == off["threads"] == 256
    assert (on["nseg"], on["rows_per_segment"]) == (46, 90)
    assert (off["nseg"], off["rows_per_segment"]) == (45, 92)
    assert (big["nseg"], big["rows_per_segment"]) == (46, 45) and (big_off["nseg"], big_off["rows_per_segment"]) == (45, 46)
    assert 16 * on["nseg"] + (on["nseg"] + 1) // 2 <= on["cus"] * on["wg_per_cu"]
    assert n1024["threads"] == 128 and n1024["nstrips"] == 9


def test_vi_march_variants_fit_three_workgroups(tmp_path):
    """Every compiled variant of the vector-invariant marching kernel (fp64 and fp32, both strip widths, every stage MODE the launcher
    instantiates, anchor ones included): no scratch, at most 168 VGPRs and at most 53.3 KB of LDS (3 workgroups of 256 per CU).  The
    fp64 256-lane variants carry the LDS columns of two 128-lane sub-strips: 268 instead of 262."""
    res = _resource_usage(tmp_path)
    vi = {n: u for n, u in res.items() if "k_tendency_vi_marchI" in n and "_pk" not in n}
    modes = {m for n in vi for m in (1, 3, 4, 5, 7, 9, 11) if f"ELi{m}EEEvNS_" in n}
    assert modes == {1, 3, 4, 5, 7, 9, 11}
    assert len(vi) == 2 * 2 * 2 * 7   # fp64 / fp32, Lorentz on / off, 256 / 128 lanes, seven MODEs
    for name, u in vi.items():
        assert u["scratch"] == 0 and u["vgpr"] <= 168 and u["lds"] <= LDS_3WG, (name, u)
    lds = {u["lds"] for n, u in vi.items() if "marchIdLi1ELi256E" in n}
    assert lds == {268 * 24 * 8}, lds   # 24 doubles per LDS column with the Lorentz force
