"""CPU test of the zonal-spectrum launch plan (spectra_plan and spectra_depth in swmhd_amd/csrc/launch_plan.hpp): a host program prints
the plan (tests/spectra_plan_check.cpp: its own main, launch_plan.hpp only) and the lines are compared with what the shape of the kernels
implies -- W = min(rows, 256) units per (member, field) in pass 1 (a workgroup each from Nx = 512 on, four one-wave units per workgroup
up to Nx = 256), 16 values of k per workgroup in pass 2, 12 Nx bytes of LDS per unit -- for
the (Nx, rows, fields, members) of tests/spectra_cases.py, the measured shapes, "nothing to do", the unsupported sizes and the refusal
from 2^31 workgroups on.  W and the depth D_rows the plan header states are those of the tests' bound, and the workspace is what the C
function answers."""
import os
import subprocess

import pytest

import spectra_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("spectra_plan") / "spectra_plan_check")
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(HIPCC)))
    cc = subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                         "-I" + os.path.join(ROOT, "swmhd_amd", "csrc"), os.path.join(ROOT, "tests", "spectra_plan_check.cpp"), "-o", path],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    return path


def _run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return [line.split() for line in r.stdout.splitlines()]


def test_shape_is_the_one_the_reference_assumes(exe):
    assert _run(exe, "shape") == [["shape", "256", "256", "16", "16", "9", "2", "12", "256", "4"]]
    assert (SC.WMAX, SC.P2_G, SC.MIN_LOG2, SC.MAX_LOG2) == (256, 16, 2, 12)
    assert -(-(2 ** 11 + 1) // 256) == 9      # accumulators of a thread at Nx = 4096: k = tid, tid + 256, ... <= 2048
    assert -(-(2 ** 7 + 1) // 64) == 3        # ... and of a lane of a one-wave unit at Nx = 256: k = lane, lane + 64, lane + 128 <= 128


def _quads():
    quads = set()
    for c in SC.cases():
        j0, j1 = SC.rows_of(c)
        quads.add((c.Nx, j1 - j0, bin(c.which).count("1"), 1))
    for Nx, Ny, _form, _dtype, _pitched, rows, which, _wrap in SC.ensemble_cases():
        n = Ny if rows is None else rows[1] - rows[0]
        quads.add((Nx, n, bin(which).count("1"), SC.ENSEMBLE_MEMBERS))
    return sorted(quads)


def test_plans(exe, swmhd):
    L = swmhd._lib.lib()
    quads = _quads()
    # the measured shapes: 4096^2 with one, three and seven fields; 256 members of 64^2
    quads += [(4096, 4096, 1, 1), (4096, 4096, 3, 1), (4096, 4096, 7, 1), (64, 64, 3, 256), (64, 64, 7, 256), (4, 1, 1, 65535)]
    # nothing to do: no rows, no fields, no members
    quads += [(64, 0, 3, 1), (64, -3, 3, 1), (64, 7, 0, 1), (64, 7, 3, 0), (64, 0, 0, 0)]
    # unsupported sizes: not a power of two, below 4, above 4096 (also with nothing to do)
    quads += [(3, 7, 1, 1), (6, 7, 1, 1), (2, 7, 1, 1), (1, 7, 1, 1), (8192, 7, 1, 1), (192, 7, 2, 3), (0, 7, 1, 1), (-8, 7, 1, 1), (6, 0, 1, 1)]
    # 2^31 workgroups and more are refused (Nx = 512: a workgroup per unit): 256 x 7 x 1198373 >= 2^31 > 256 x 7 x 1198372; 255 rows
    # leave room for more members; at Nx = 8 four units share a workgroup and pass 1 stays below
    quads += [(512, 256, 7, 1198373), (512, 256, 7, 1198372), (512, 300, 7, 1198373), (512, 255, 7, 1198373), (512, 2 ** 31 - 1, 7, 1198372),
              (512, 256, 1, 2 ** 23), (512, 256, 1, 2 ** 23 - 1), (8, 256, 1, 2 ** 23), (8, 256, 1, 2 ** 25), (8, 256, 1, 2 ** 25 - 1)]
    lines = _run(exe, "plan", *[v for q in quads for v in q])
    assert len(lines) == len(quads)
    seen = set()
    for (Nx, rows, nf, members), line in zip(quads, lines):
        assert line[0] == "plan" and [int(v) for v in line[1:5]] == [Nx, rows, nf, members]
        log2n, W, units, nk, blocks1, blocks2, lds, ws, depth, none, unsupported, too_many = (int(v) for v in line[5:])
        supported = Nx in SC.NXS
        assert unsupported == (0 if supported else 1) and log2n == (Nx.bit_length() - 1 if supported else -1)
        assert none == (1 if min(rows, nf, members) <= 0 else 0)
        if unsupported or none:
            assert (W, units, nk, blocks1, blocks2, lds, ws, depth, too_many) == (0,) * 9
            seen.add("unsupported" if unsupported else "none")
            continue
        assert W == min(rows, 256) == SC.plan_W(rows) and nk == Nx // 2 + 1
        assert units == (4 if Nx <= 256 else 1)
        assert blocks1 == -(-W // units) * nf * members and blocks2 == -(-nk // 16) * nf * members
        assert lds == 12 * Nx * units and lds <= 48 * 1024
        assert ws == W * nf * members * nk == SC.workspace(Nx, rows, nf, members)
        assert depth == SC.depth(rows)
        assert too_many == (1 if max(blocks1, blocks2) >= 2 ** 31 else 0)
        if not too_many and members <= 65535:
            assert L.swmhd_zonal_spectra_workspace(Nx, rows, nf, members) == ws
        seen.add("refused" if too_many else "planned")
    assert seen == {"none", "unsupported", "refused", "planned"}
    by = {tuple(int(v) for v in l[1:5]): l for l in lines}
    assert by[(4096, 4096, 7, 1)][5:14] == ["12", "256", "1", "2049", "1792", str(129 * 7), "49152", str(1792 * 2049), "34"]
    assert by[(64, 64, 3, 256)][5:12] == ["6", "64", "4", "33", str(16 * 3 * 256), str(3 * 3 * 256), str(12 * 64 * 4)]
    assert by[(512, 256, 7, 1198373)][-1] == "1" and by[(512, 256, 7, 1198372)][-1] == "0" and by[(512, 300, 7, 1198373)][-1] == "1"
    assert by[(512, 255, 7, 1198373)][-1] == "0" and by[(512, 2 ** 31 - 1, 7, 1198372)][-1] == "0"
    assert by[(512, 256, 1, 2 ** 23)][-1] == "1" and by[(512, 256, 1, 2 ** 23 - 1)][-1] == "0"
    assert by[(8, 256, 1, 2 ** 23)][-1] == "0" and by[(8, 256, 1, 2 ** 25)][-1] == "1" and by[(8, 256, 1, 2 ** 25 - 1)][-1] == "0"


def test_workspace_function_is_a_pure_host_function(swmhd):
    """No device is needed; nothing to do needs no workspace; the size does not depend on whether Nx is a supported size."""
    L = swmhd._lib.lib()
    f = L.swmhd_zonal_spectra_workspace
    assert f(64, 7, 3, 1) == 7 * 3 * 33 and f(64, 300, 7, 2) == 256 * 7 * 2 * 33 and f(4096, 4096, 7, 1) == 256 * 7 * 2049
    assert f(0, 7, 3, 1) == 0 and f(64, 0, 3, 1) == 0 and f(64, 7, 0, 1) == 0 and f(64, 7, 3, 0) == 0 and f(64, -1, 3, 1) == 0
    assert f(4096, 2 ** 31 - 1, 7, 65535) == 256 * 7 * 65535 * 2049      # beyond 2^31 doubles: the answer is 64 bits wide
    for Nx, rows, nf, members in _quads():
        assert f(Nx, rows, nf, members) == SC.workspace(Nx, rows, nf, members)


def test_depth_is_the_bound_of_the_tests(exe):
    rows = sorted(set(range(1, 40)) | {r for q in _quads() for r in q[1:2]} | {63, 64, 65, 240, 241, 255, 256, 257, 511, 512, 513, 768, 769, 4096, 4097, 65536})
    rows = [r for r in rows if r > 0]
    lines = _run(exe, "depth", *rows)
    assert [int(l[1]) for l in lines] == rows
    for r, line in zip(rows, lines):
        assert int(line[2]) == SC.plan_W(r) and int(line[3]) == SC.depth(r), (r, line, SC.depth(r))
    # spelled out: one row has no addition; 2 rows one tree level; 16 rows 4 levels; 17 rows: lane 0 adds two partials, then 4 levels;
    # 256 rows: 16 partials per lane and 4 levels; the 257th row is workgroup 0's second; 4096 rows: 16 per workgroup
    want = {1: 0, 2: 1, 3: 2, 7: 3, 16: 4, 17: 5, 255: 19, 256: 19, 257: 20, 512: 20, 513: 21, 4096: 34}
    for r, d in want.items():
        assert SC.depth(r) == d, (r, SC.depth(r), d)
