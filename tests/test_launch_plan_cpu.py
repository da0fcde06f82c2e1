"""CPU tests of the tendency launch plan (swmhd_amd/csrc/launch_plan.hpp): the geometry query reproduces the table recorded from the
library before the launchers were rewritten around a plan (tests/golden/launch_geometry.json), and a host program checks the whole
dispatch sequence of the plans the query cannot show (tests/launch_plan_check.cpp).  Neither launches anything."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
TILE_KERNEL, MARCH_MIN_CELLS = 2, 330000
NX_ALL = [64, 128, 512, 640, 1000, 1024, 1346, 2501, 4096, 8192]
TABLES = {"default": ({}, NX_ALL), "SWMHD_T_FOLD=0": ({"SWMHD_T_FOLD": "0"}, [4096, 1024]), "SWMHD_T_NT=128": ({"SWMHD_T_NT": "128"}, [4096, 1024])}


def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "launch_geometry.json")) as f:
        return json.load(f)


def _clean_env(extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("SWMHD_T_") and k not in ("SWMHD_RING_ROOM", "SWMHD_ENS_RY", "SWMHD_ENS_MAP", "SWMHD_OP_LY")}
    env.update(extra)
    return env


@pytest.mark.parametrize("table", sorted(TABLES))
def test_geometry_query_reproduces_recorded_table(swmhd, table):
    """Every row of the sweep, in a fresh process per knob setting (the knobs are read once).  The ONE exception is named here: a fast
    build with SWMHD_TILE_KERNEL on fewer than 330000 cells.  The launcher has always taken 64 x 4 tiles there and the old query said
    64 x 8; the query now reports the launcher's plan.  Those rows are stored with both values, and no other row may differ."""
    gold = _golden()
    knob, nxs = TABLES[table]
    code = gold["header"]["generated_by"].split('python -c "', 1)[1].rsplit('" ROOT NXS', 1)[0].replace('\\"', '"')
    r = subprocess.run([sys.executable, "-c", code, ROOT, json.dumps(nxs)], env=_clean_env(knob), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout)
    recorded, corrected = gold["tables"][table], {tuple(c[:5]): c for c in gold["corrected"][table]}
    assert len(recorded) == len(nxs) * 7 * 2 * 2 * 6 and [g[:5] for g in got] == [p[:5] for p in recorded]
    excepted = {tuple(p[:5]) for p in recorded if p[4] == TILE_KERNEL and p[0] * p[1] < MARCH_MIN_CELLS}
    assert set(corrected) == excepted and excepted
    for g, p in zip(got, recorded):
        key = tuple(p[:5])
        if key in corrected:
            c = corrected[key]
            assert p[5:] == [1, 256, (p[0] + 63) // 64, (p[1] + 7) // 8, 8, 0, 3, 256]       # what the old query said
            assert c[5:] == [1, 256, (p[0] + 63) // 64, (p[1] + 3) // 4, 4, 0, 3, 256]       # what the launcher does
            assert g == c, (g, c)
        else:
            assert g == p, (g, p)


def test_plan_dispatch_sequences(tmp_path):
    """launch_plan_check.cpp as a host program: the plans of periodic stages in every RK3 stage form, Bounded hybrids with and without
    open sides, two-range and empty-range launches, parents beyond 4 GiB, Bounded grids below the hybrid thresholds, ensembles; the
    plans of the Lorentz operators (cross-overs, the Bounded hybrid and its thresholds, the round cap, and what every shape of the
    operator call matrix of tests/operator_cases.py lands on) and the tiles of a tracer stage.  Then in fresh processes with
    SWMHD_OP_LY=5 and =13 (read once): that many rows per segment, below and above the minimum of 8, also on the matrix's sweep grid."""
    exe = str(tmp_path / "launch_plan_check")
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(HIPCC)))
    cc = subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                         "-I" + os.path.join(ROOT, "swmhd_amd", "csrc"), os.path.join(ROOT, "tests", "launch_plan_check.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    r = subprocess.run([exe], env=_clean_env({}), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "launch plans OK" in r.stdout, r.stdout[-3000:] + r.stderr[-1000:]
    for ly in ("5", "13"):
        r = subprocess.run([exe, "op_ly", ly], env=_clean_env({"SWMHD_OP_LY": ly}), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "launch plans OK" in r.stdout, r.stdout[-3000:] + r.stderr[-1000:]


def test_launchers_do_not_reenter():
    """The tendency and Lorentz launchers enqueue their plans: none calls a launcher of its family, the operators have no geometry
    function of their own, and "Bounded" has one definition."""
    csrc = os.path.join(ROOT, "swmhd_amd", "csrc")
    launch = open(os.path.join(csrc, "tendency_launch.inc")).read()
    uses = [l for l in launch.splitlines() if "LAUNCH_NAME(launch_tendency_" in l]
    # two definitions (single grid, ensemble) and their four explicit instantiations: no call
    assert len(uses) == 6 and all(l.startswith(("hipError_t ", "template hipError_t ")) for l in uses), uses
    lorentz = open(os.path.join(csrc, "lorentz_launch.inc")).read()
    uses = [l for l in lorentz.splitlines() if "launch_lorentz_" in l]
    # two definitions (Jacobian form, divergence form) and their four explicit instantiations: no call
    assert len(uses) == 6 and all(l.startswith(("hipError_t LAUNCH_NAME(", "template hipError_t LAUNCH_NAME(")) for l in uses), uses
    text = "".join(open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".inc", ".hpp")))
    assert "march_rows_per_segment" not in text
    for spelled in ("topo_x == 1 || a.topo_y", "topo_x == 1 || topo_y == 1"):
        assert spelled not in text
    assert text.count("topo_x == 1 || topo_y != 0") == 1
