"""CPU test of the launch plan of the six strip-march correction launches (strip_plan, common_phase and strip_call_plan in
swmhd_amd/csrc/launch_plan.hpp: Coriolis, diffusion, biharmonic, relaxation, source, stochastic): a host program prints the plan (tests/strip_plan_check.cpp: its own main, launch_plan.hpp only)
and the lines are compared with what the kernels' shape implies -- a wave of 64 lanes x vec columns marching 16 rows, four waves to a
workgroup, the workgroups of launch l (a member, or a member's field) after those of launch l - 1 -- for every shape of the stage
matrices (tests/strip_cases.py) in both precisions at every phase, "nothing to do", and the refusal from 2^31 workgroups on; and the
plan of a whole call, whose phase the further pitches of its kind (a mask's, a target's or a source's member pitch, the pitch of the
stochastic x tables) must keep as well -- 0 standing for "shared or not applicable"."""
import itertools
import os
import subprocess

import pytest

import strip_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LAUNCHES = (1, 3, 3 * 7)      # one grid; three members (Coriolis); three members x seven fields (diffusion)
LIMIT = 2 ** 31


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("strip_plan") / "strip_plan_check")
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(HIPCC)))
    cc = subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                         "-I" + os.path.join(ROOT, "swmhd_amd", "csrc"), os.path.join(ROOT, "tests", "strip_plan_check.cpp"), "-o", path],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    return path


def _run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return [line.split() for line in r.stdout.splitlines()]


def expected(Nx, rows, itemsize, phase, launches):
    """(vec, lead, nstrips, nsb, blocks) as the kernels' shape implies them"""
    vec, lead = (16 // itemsize, phase) if phase >= 0 else (1, 0)
    nstrips, nsb = -(-(Nx + lead) // (64 * vec)), -(-rows // SC.TILE_ROWS)
    return vec, lead, nstrips, nsb, nstrips * nsb * launches


def test_shape_is_the_one_the_cases_assume(exe):
    assert _run(exe, "shape") == [["shape", "64", "4", "16"]]
    assert SC.TILE_ROWS == 4 * 16 and SC.wave_columns(8, True) == 64 * 2 and SC.wave_columns(4, True) == 64 * 4 and SC.wave_columns(4, False) == 64


def test_plans(exe):
    cases = []
    # every shape of the stage matrices, with its whole, inner and empty row range, at every phase, for every count of launches
    for itemsize in (8, 4):
        shapes = sorted(set(SC.stage_shapes(itemsize, True)) | set(SC.stage_shapes(itemsize, False)))
        for Nx, Ny in shapes:
            for rows in sorted({j1 - j0 for j0, j1 in SC.row_ranges(Ny)}):
                cases += [(Nx, rows, itemsize, ph, L) for ph in range(-1, 16 // itemsize) for L in LAUNCHES]
    # the measured shape
    cases += [(4096, 4096, 8, 0, 1), (4096, 4096, 4, 3, 1)]
    # nothing to do: no columns, no rows, no launches
    cases += [(0, 5, 8, 0, 1), (-2, 5, 8, -1, 1), (5, 0, 4, 0, 3), (5, -1, 4, 2, 3), (5, 5, 8, 1, 0), (5, 5, 8, 1, -4), (0, 0, 4, -1, 0)]
    # 2^31 workgroups and more are refused.  1024 strips of single elements (Nx = 65536, phase -1); for each count of launches the
    # fewest row blocks whose product reaches 2^31, and one row block fewer
    refused, accepted = [], []
    for L in LAUNCHES:
        nsb = -(-LIMIT // (1024 * L))
        assert 1024 * nsb * L >= LIMIT > 1024 * (nsb - 1) * L
        refused += [(65536, 64 * nsb, 8, -1, L), (65536, 64 * (nsb - 1) + 1, 4, -1, L)]
        accepted += [(65536, 64 * (nsb - 1), 8, -1, L)]
    # exactly 2^31: 2 x 1 x 2^30, and 2^15 x 2^16 x 1; one block fewer, 2^31 - 1 (a prime): 1 x 1 x (2^31 - 1)
    refused += [(65, 1, 8, -1, 2 ** 30), (2 ** 21, 2 ** 22, 8, -1, 1)]
    accepted += [(1, 1, 8, -1, LIMIT - 1), (2 ** 21, 2 ** 22 - 64, 8, -1, 1)]
    # (strips x row blocks alone beyond 2^31: the product with the launches must not wrap)
    refused += [(2 ** 31 - 1, 2 ** 31 - 1, 8, -1, 65535 * 11), (2 ** 31 - 1, 2 ** 31 - 1, 4, 3, 1)]
    cases += refused + accepted
    lines = _run(exe, "plan", *[v for c in cases for v in c])
    assert len(lines) == len(cases)
    seen = set()
    for c, line in zip(cases, lines):
        assert line[0] == "plan" and tuple(int(v) for v in line[1:6]) == c
        vec, lead, nstrips, nsb, blocks, none, too_many = (int(v) for v in line[6:])
        Nx, rows, itemsize, phase, L = c
        if Nx <= 0 or rows <= 0 or L <= 0:
            assert (none, too_many, blocks) == (1, 0, 0), c
            seen.add("none")
            continue
        want = expected(*c)
        assert none == 0 and (vec, lead, nstrips, nsb) == want[:4], (c, line)
        assert too_many == (1 if want[4] >= LIMIT else 0), (c, line)
        assert blocks == (0 if too_many else want[4]), (c, line)
        seen.add("refused" if too_many else "planned")
    assert seen == {"none", "refused", "planned"}
    by = {tuple(int(v) for v in l[1:6]): [int(v) for v in l[6:]] for l in lines}
    assert by[(4096, 4096, 8, 0, 1)] == [2, 0, 32, 64, 2048, 0, 0] and by[(4096, 4096, 4, 3, 1)] == [4, 3, 17, 64, 1088, 0, 0]
    assert expected(65, 1, 8, -1, 2 ** 30)[4] == LIMIT == expected(2 ** 21, 2 ** 22, 8, -1, 1)[4]
    assert by[(1, 1, 8, -1, LIMIT - 1)][4:] == [LIMIT - 1, 0, 0]
    assert all(by[c][5:] == [0, 1] for c in refused) and all(by[c][5:] == [0, 0] for c in accepted)


def test_common_phase(exe):
    for itemsize in (8, 4):
        V = 16 // itemsize
        for ph in range(V):
            base = 4096 + ph * itemsize
            same = [base, base + 16 * 7, base + 16 * 1000, base + 32]
            assert _run(exe, "phase", itemsize, 2 * V, 0, *same) == [["phase", str(ph)]]
            assert _run(exe, "phase", itemsize, 2 * V, 6 * V, same[0], 0, same[1], 0, 0, same[2]) == [["phase", str(ph)]]      # null entries are skipped
            other = base + itemsize      # the next phase (or, from the last one, phase 0 of the next 16 bytes)
            for k in range(1, 4):
                assert _run(exe, "phase", itemsize, 2 * V, 0, *same[:k], other, *same[k:]) == [["phase", "-1"]]
            assert _run(exe, "phase", itemsize, 2 * V + 1, 0, *same) == [["phase", "-1"]]           # the row pitch does not keep the phase
            assert _run(exe, "phase", itemsize, 2 * V, 5 * V + 1, *same) == [["phase", "-1"]]       # nor does the member pitch


def test_call_plan_further_pitches(exe):
    """strip_call_plan: common_phase's phase, kept or lost by the further pitches, then strip_plan's plan of it."""
    Nx, rows, members, per = 65, 17, 2, 3

    def call(itemsize, sy, members, stride_m, further, addrs):
        out = _run(exe, "call", Nx, rows, itemsize, sy, members, stride_m, per, len(further), *further, *addrs)
        assert len(out) == 1 and out[0][0] == "call"
        return [int(v) for v in out[0][1:]]

    def plan(itemsize, phase, launches):
        return [int(v) for v in _run(exe, "plan", Nx, rows, itemsize, phase, launches)[0][6:]]

    for itemsize in (8, 4):
        V = 16 // itemsize
        for ph in range(V):
            base = 4096 + ph * itemsize
            addrs = [base, base + 16 * 7, 0, base + 16 * 1000]
            sy, stride_m = 20 * V, 600 * V
            kept, lost = plan(itemsize, ph, members * per), plan(itemsize, -1, members * per)
            assert kept[:2] == [V, ph] and lost[:2] == [1, 0]
            # no further pitches: common_phase's answer, on the cases test_common_phase has
            assert _run(exe, "phase", itemsize, sy, stride_m, *addrs) == [["phase", str(ph)]]
            assert call(itemsize, sy, members, stride_m, [], addrs) == kept
            assert call(itemsize, sy + 1, members, stride_m, [], addrs) == lost
            assert call(itemsize, sy, members, stride_m + 1, [], addrs) == lost
            assert call(itemsize, sy, members, stride_m, [], addrs[:1] + [base + itemsize] + addrs[1:]) == lost
            # one grid: stride_m is not looked at, and there is one launch per field
            assert call(itemsize, sy, 0, stride_m + 1, [], addrs) == plan(itemsize, ph, per)
            # 0 and multiples of 16 / itemsize keep the phase, anything else loses it, in any order
            good, bad = [0, V, 7 * V, 1000 * V], [1, V + 1, 1000 * V - 1] + ([2, 3, 5 * V + 2] if V == 4 else [])
            for f in good:
                assert call(itemsize, sy, members, stride_m, [f], addrs) == kept, (itemsize, ph, f)
            for f in bad:
                assert call(itemsize, sy, members, stride_m, [f], addrs) == lost, (itemsize, ph, f)
            for fs in ([0, V], [7 * V, 0, 1000 * V]):
                assert all(call(itemsize, sy, members, stride_m, list(p), addrs) == kept for p in itertools.permutations(fs))
            for fs in ([0, 1], [V, V + 1, 0], [1, 3, 2 * V]):
                assert all(call(itemsize, sy, members, stride_m, list(p), addrs) == lost for p in itertools.permutations(fs))
            # a phase lost already stays lost
            assert call(itemsize, sy + 1, members, stride_m, [0, V], addrs) == lost
