"""CPU test of the zonal-mean launch plan (zonal_plan and zonal_depth in swmhd_amd/csrc/launch_plan.hpp): a host program prints the plan
(tests/zonal_plan_check.cpp: its own main, launch_plan.hpp only) and the lines are compared with what the kernel's shape implies -- one
wave64 per row, four rows per 256-thread workgroup, the members' workgroups one after the other -- for the shapes of tests/zonal_cases.py,
the two measured shapes, "nothing to do" and the refusal from 2^31 workgroups on.  The depth of the summation tree the plan header states is
the D of the tests' bound."""
import os
import subprocess

import pytest

import zonal_cases as ZC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("zonal_plan") / "zonal_plan_check")
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(HIPCC)))
    cc = subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                         "-I" + os.path.join(ROOT, "swmhd_amd", "csrc"), os.path.join(ROOT, "tests", "zonal_plan_check.cpp"), "-o", path],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    return path


def _run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return [line.split() for line in r.stdout.splitlines()]


def test_shape_is_the_one_the_reference_assumes(exe):
    assert _run(exe, "shape") == [["shape", "256", "64", "4", "4", "256"]]
    assert (ZC.WAVE, ZC.VEC, ZC.TRIP) == (64, 4, 256)


def test_plans(exe):
    pairs = []
    # the row counts of the case list (whole ranges and sub-ranges), single grids and the ensembles' three members
    for rows in sorted({r[1] - r[0] for r in (ZC.rows_of(c) for c in ZC.cases())}):
        pairs += [(rows, 1), (rows, ZC.ENSEMBLE_MEMBERS)]
    # the measured shapes: 4096 rows; 256 members of 64 rows = 16 384 waves
    pairs += [(4096, 1), (64, 256), (5, 65535), (4097, 2)]
    # nothing to do: no rows, no members
    pairs += [(0, 1), (-3, 1), (7, 0), (0, 0)]
    # 2^31 workgroups and more are refused: 2^29 row blocks x 4 members = 2^31; one row block less leaves 2^31 - 4
    pairs += [(2 ** 31 - 1, 1), (2 ** 31 - 1, 4), (2 ** 31 - 3, 4), (2 ** 31 - 4, 4), (2 ** 17, 65535), (2 ** 17 + 1, 65535), (2 ** 17 + 5, 65535)]
    lines = _run(exe, "plan", *[v for p in pairs for v in p])
    assert len(lines) == len(pairs)
    seen = set()
    for (rows, members), line in zip(pairs, lines):
        assert line[0] == "plan" and [int(v) for v in line[1:3]] == [rows, members]
        rpb, row_blocks, blocks, none, too_many = (int(v) for v in line[3:])
        assert rpb == 4
        if rows <= 0 or members <= 0:
            assert none == 1 and too_many == 0 and blocks == 0
            seen.add("none")
            continue
        assert none == 0 and row_blocks == -(-rows // 4) and blocks == row_blocks * members
        assert too_many == (1 if blocks >= 2 ** 31 else 0)
        seen.add("refused" if too_many else "planned")
    assert seen == {"none", "refused", "planned"}
    by = {(int(l[1]), int(l[2])): l for l in lines}
    assert by[(4096, 1)][4:6] == ["1024", "1024"] and by[(64, 256)][4:6] == ["16", "4096"]
    assert by[(2 ** 31 - 1, 4)][7] == "1" and by[(2 ** 31 - 3, 4)][5:] == [str(2 ** 31), "0", "1"]
    assert by[(2 ** 31 - 4, 4)][5:] == [str(2 ** 31 - 4), "0", "0"] and by[(2 ** 31 - 1, 1)][7] == "0"
    assert by[(2 ** 17, 65535)][7] == "0" and by[(2 ** 17 + 1, 65535)][7] == "1"      # 32768 x 65535 < 2^31 <= 32769 x 65535


def test_depth_is_the_bound_of_the_tests(exe):
    nxs = sorted(set(ZC.NXS) | {2, 6, 7, 8, 9, 16, 17, 32, 33, 128, 129, 252, 253, 258, 259, 260, 261, 511, 512, 516, 517, 1030, 4096, 4097})
    lines = _run(exe, "depth", *nxs)
    assert [int(l[1]) for l in lines] == nxs
    for nx, line in zip(nxs, lines):
        assert int(line[2]) == ZC.depth(nx), (nx, line, ZC.depth(nx))
    # spelled out: one cell has no addition; 4 cells one lane; 5 cells two lanes; 256 cells 64 lanes of 4; the 257th cell is lane 0's 5th
    want = {1: 0, 3: 2, 4: 3, 5: 4, 63: 7, 64: 7, 65: 8, 255: 9, 256: 9, 257: 10, 513: 14, 4096: 69}
    for nx, d in want.items():
        assert ZC.depth(nx) == d, (nx, ZC.depth(nx), d)
