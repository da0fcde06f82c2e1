"""CPU test of the 2-D / isotropic spectrum launch plan (spectra2d_plan, spectra2d_shell(s) in swmhd_amd/csrc/launch_plan.hpp): a host
program prints the plan (tests/spectra2d_plan_check.cpp: its own main, launch_plan.hpp only) and the lines are compared with what the
shape of the kernels implies -- R consecutive rows per workgroup of pass 1 from the LDS budget, one unit per (member, field, kx) in pass 2
(a wave up to Ny = 256, four to a workgroup; a workgroup above), 16 shells per workgroup of pass 3, 20 Ny bytes of LDS per column unit
(80 KiB at Ny = 4096) or the stated fallback without a twiddle table (16 Ny bytes) where the device admits less -- for the shapes of
tests/spectra2d_cases.py, the measured shapes, "nothing to do", the unsupported sizes and the refusal from 2^31 workgroups on.  NS and
the workspace are what the C functions answer, and the shell of a mode is the numpy restatement's."""
import os
import subprocess

import numpy as np
import pytest

import spectra2d_cases as S2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KIB = 1024
FULL = 160 * KIB


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("spectra2d_plan") / "spectra2d_plan_check")
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(HIPCC)))
    cc = subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                         "-I" + os.path.join(ROOT, "swmhd_amd", "csrc"), os.path.join(ROOT, "tests", "spectra2d_plan_check.cpp"), "-o", path],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    return path


def _run(exe, *args):
    r = subprocess.run([exe, *(a if isinstance(a, str) else repr(a) for a in args)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return [line.split() for line in r.stdout.splitlines()]


def test_shape_is_the_one_the_reference_assumes(exe):
    assert _run(exe, "shape") == [["shape", "256", "16", str(80 * KIB), str(FULL), "16", "16", "256", "4"]]
    assert (S2.RMAX, S2.P2_G, S2.P2_K, S2.SMALL, S2.UNITS_SMALL) == (16, 16, 16, 256, 4)


def _inputs():
    """(Nx, Ny, nfields, members, wx, wy, shells, lds_limit)"""
    q = set()
    for c in S2.cases():
        q.add((c.Nx, c.Ny, bin(c.which).count("1"), 1, c.wx, c.wy, int(c.outs != "2d"), FULL))
    for Nx, Ny, _form, _dtype, _pitched, which, _wrap, wx, wy, outs in S2.ensemble_cases():
        q.add((Nx, Ny, bin(which).count("1"), S2.ENSEMBLE_MEMBERS, wx, wy, int(outs != "2d"), FULL))
    return sorted(q)


def test_plans(exe, swmhd):
    L = swmhd._lib.lib()
    quads = _inputs()
    # the measured shapes: 4096^2 with one and three fields, 256 members of 64^2, each with and without shells
    quads += [(4096, 4096, nf, 1, 1.0, 1.0, sh, FULL) for nf in (1, 3) for sh in (1, 0)] + [(64, 64, 3, 256, 1.0, 1.0, sh, FULL) for sh in (1, 0)]
    # a device that admits 64 KiB per workgroup: the column pass at Ny = 4096 without its table, fewer rows per workgroup of pass 1
    quads += [(Nx, Ny, 2, 1, 1.0, 0.25, 1, 64 * KIB) for Nx, Ny in S2.SIZES + ((4096, 4096), (2048, 2048), (1024, 64))]
    quads += [(4096, 4096, 1, 1, 1.0, 1.0, 1, 80 * KIB), (4096, 4096, 1, 1, 1.0, 1.0, 1, 80 * KIB - 1)]
    # nothing to do: no fields, no members
    quads += [(64, 64, 0, 1, 1.0, 1.0, 1, FULL), (64, 64, 3, 0, 1.0, 1.0, 1, FULL), (64, 64, -1, -1, 1.0, 1.0, 0, FULL)]
    # unsupported sizes in either direction: not a power of two, below 4, above 4096 (also with nothing to do)
    quads += [(Nx, Ny, 1, 1, 1.0, 1.0, 1, FULL) for Nx, Ny in ((3, 8), (8, 3), (6, 8), (8, 6), (2, 8), (8, 2), (8192, 8), (8, 8192), (192, 64), (64, 192), (0, 8), (8, -8))]
    quads += [(6, 8, 0, 1, 1.0, 1.0, 1, FULL)]
    # 2^31 workgroups and more are refused.  Pass 2 at Nx = Ny = 512: 257 units per (member, field), a workgroup each:
    # 257 x 7 x 1193710 >= 2^31 > 257 x 7 x 1193709; at Ny = 64 four units share a workgroup
    quads += [(512, 512, 7, 1193710, 1.0, 1.0, 1, FULL), (512, 512, 7, 1193709, 1.0, 1.0, 1, FULL), (512, 64, 7, 1193710, 1.0, 1.0, 1, FULL),
              (4, 4096, 1, 2 ** 23, 1.0, 1.0, 0, FULL), (4, 4096, 1, 2 ** 23 - 1, 1.0, 1.0, 0, FULL)]
    lines = _run(exe, "plan", *[v for q in quads for v in q])
    assert len(lines) == len(quads)
    seen = set()
    by = {}
    for q, line in zip(quads, lines):
        Nx, Ny, nf, members, wx, wy, shells, limit = q
        assert line[0] == "plan" and [int(v) for v in line[1:5]] == [Nx, Ny, nf, members]
        (log2nx, log2ny, nkx, NS, R, pad, units1, units2, table, blocks1, blocks2, blocks3, lds1, lds2, modes, partials, ws, none, unsupported,
         too_many) = (int(v) for v in line[5:])
        by[q] = dict(R=R, lds1=lds1, lds2=lds2, table=table, blocks=(blocks1, blocks2, blocks3), ws=ws, too_many=too_many, NS=NS)
        ok = lambda N: N >= 4 and N <= 4096 and N & (N - 1) == 0
        supported = ok(Nx) and ok(Ny)
        assert unsupported == (0 if supported else 1)
        assert log2nx == (Nx.bit_length() - 1 if ok(Nx) else -1) and log2ny == (Ny.bit_length() - 1 if ok(Ny) else -1)
        assert none == (1 if min(nf, members) <= 0 else 0)
        if unsupported or none:
            assert (nkx, NS, R, pad, units1, units2, table, blocks1, blocks2, blocks3, lds1, lds2, modes, partials, ws, too_many) == (0,) * 16
            seen.add("unsupported" if unsupported else "none")
            continue
        mf = nf * members
        assert nkx == Nx // 2 + 1 and NS == S2.shells(Nx, Ny, wx, wy) == L.swmhd_spectra2d_shells(Nx, Ny, wx, wy)
        assert (R, pad, lds1) == S2.plan_R(Nx, Ny, limit) and R >= 1 and R & (R - 1) == 0 and Ny % R == 0 and R <= 16
        assert lds1 == R * 8 * (Nx + pad) + 4 * Nx and (lds1 <= min(limit, 80 * KIB) or R == 1) and pad == (2 if R > 2 else 0)
        assert units1 == (4 if Nx <= 256 else 1) and R % units1 == 0 and units2 == (4 if Ny <= 256 else 1)
        assert blocks1 == Ny // R * mf and blocks2 == -(-nkx * mf // units2) and blocks3 == (-(-NS // 16) * mf if shells else 0)
        assert table == (1 if 20 * Ny * units2 <= limit else 0) and lds2 == (20 if table else 16) * Ny * units2
        assert max(lds1, lds2) <= min(limit, FULL) or (R == 1 and lds1 == 12 * Nx <= 48 * KIB)
        assert modes == 2 * nkx * Ny * mf and partials == (nkx * NS * mf if shells else 0) and ws == modes + partials
        assert too_many == (1 if max(blocks1, blocks2, blocks3) >= 2 ** 31 else 0)
        if members <= 65535:
            full = L.swmhd_spectra2d_workspace(Nx, Ny, nf, members, wx, wy)
            assert full == S2.workspace(Nx, Ny, nf, members, wx, wy) == modes + nkx * NS * mf
        seen.add("refused" if too_many else "planned")
    assert seen == {"none", "unsupported", "refused", "planned"}
    # spelled out.  4096^2: two rows per workgroup of pass 1 in 80 KiB, a workgroup per column in 80 KiB with its table
    big = by[(4096, 4096, 3, 1, 1.0, 1.0, 1, FULL)]
    assert (big["R"], big["lds1"], big["lds2"], big["table"], big["NS"]) == (2, 80 * KIB, 80 * KIB, 1, 2897)
    assert big["blocks"] == (2048 * 3, 2049 * 3, 182 * 3) and big["ws"] == 3 * (2 * 2049 * 4096 + 2049 * 2897)
    assert by[(4096, 4096, 3, 1, 1.0, 1.0, 0, FULL)]["ws"] == 3 * 2 * 2049 * 4096 and by[(4096, 4096, 3, 1, 1.0, 1.0, 0, FULL)]["blocks"][2] == 0
    # the fallback: a device with 64 KiB per workgroup runs the 4096-column without a table in 64 KiB, and one 48-KiB row at a time
    small = by[(4096, 4096, 2, 1, 1.0, 0.25, 1, 64 * KIB)]
    assert (small["R"], small["lds1"], small["lds2"], small["table"]) == (1, 48 * KIB, 64 * KIB, 0)
    assert by[(4, 4096, 2, 1, 1.0, 0.25, 1, 64 * KIB)]["table"] == 0 and by[(4096, 4, 2, 1, 1.0, 0.25, 1, 64 * KIB)]["table"] == 1
    assert by[(2048, 2048, 2, 1, 1.0, 0.25, 1, 64 * KIB)] ["table"] == 1 and by[(2048, 2048, 2, 1, 1.0, 0.25, 1, 64 * KIB)]["R"] == 2
    assert by[(4096, 4096, 1, 1, 1.0, 1.0, 1, 80 * KIB)]["table"] == 1 and by[(4096, 4096, 1, 1, 1.0, 1.0, 1, 80 * KIB - 1)]["table"] == 0
    assert by[(4096, 4096, 1, 1, 1.0, 1.0, 1, 80 * KIB - 1)]["R"] == 1
    ens = by[(64, 64, 3, 256, 1.0, 1.0, 1, FULL)]
    assert (ens["R"], ens["lds1"], ens["lds2"], ens["NS"]) == (16, 16 * 8 * 66 + 256, 20 * 64 * 4, 46) and ens["blocks"] == (4 * 768, -(-33 * 768 // 4), 3 * 768)
    assert by[(512, 512, 7, 1193710, 1.0, 1.0, 1, FULL)]["too_many"] == 1 and by[(512, 512, 7, 1193709, 1.0, 1.0, 1, FULL)]["too_many"] == 0
    assert by[(512, 64, 7, 1193710, 1.0, 1.0, 1, FULL)]["too_many"] == 0
    assert by[(4, 4096, 1, 2 ** 23, 1.0, 1.0, 0, FULL)]["too_many"] == 1 and by[(4, 4096, 1, 2 ** 23 - 1, 1.0, 1.0, 0, FULL)]["too_many"] == 0


def test_size_functions_are_pure_host_functions(swmhd):
    """No device is needed; arguments that are not positive (and finite) answer 0; the sizes do not depend on whether Nx, Ny are supported."""
    L = swmhd._lib.lib()
    ns, ws = L.swmhd_spectra2d_shells, L.swmhd_spectra2d_workspace
    assert ns(4, 4, 1.0, 1.0) == 4 and ns(64, 64, 1.0, 1.0) == 46 and ns(4096, 4096, 1.0, 1.0) == 2897 and ns(64, 64, 1.0, 0.25) == 37
    assert ns(48, 20, 1.0, 1.0) == 27 and ns(64, 64, 4.0, 4.0) == 92
    for bad in ((0, 64, 1.0, 1.0), (64, -4, 1.0, 1.0), (64, 64, 0.0, 1.0), (64, 64, 1.0, -1.0), (64, 64, float("nan"), 1.0), (64, 64, 1.0, float("inf"))):
        assert ns(*bad) == 0 and ws(bad[0], bad[1], 1, 1, bad[2], bad[3]) == 0
    assert ws(64, 64, 0, 1, 1.0, 1.0) == 0 and ws(64, 64, 1, 0, 1.0, 1.0) == 0
    assert ws(64, 64, 3, 2, 1.0, 1.0) == 6 * (2 * 33 * 64 + 33 * 46)
    assert ws(4096, 4096, 7, 65535, 1.0, 1.0) == 7 * 65535 * (2 * 2049 * 4096 + 2049 * 2897)      # beyond 2^31 doubles: 64 bits wide
    per_field = ws(4096, 4096, 1, 1, 1.0, 1.0) * 8
    assert (2 * 2049 * 4096 * 8, 2049 * 2897 * 8) == (134283264, 47487624) and per_field == 134283264 + 47487624      # the header's 134 MB + 47 MB
    for q in _inputs():
        assert ws(*q[:6]) == S2.workspace(*q[:6])


def test_shell_of_the_plan_is_the_numpy_restatement(exe):
    """Every mode of small planes, and the modes around the corner and along the axes of the largest, under all metrics of the cases and
    two that leave shells empty."""
    for wx, wy in S2.METRICS + ((4.0, 4.0), (9.0, 2.25)):
        for Nx, Ny in ((8, 4), (64, 64), (4096, 4096)):
            sh = S2.shell_index(Nx, Ny, wx, wy)
            if Nx * Ny <= 4096:
                modes = [(mx, ky) for mx in range(Nx // 2 + 1) for ky in range(Ny)]
            else:
                rng = np.random.default_rng([Nx, Ny])
                modes = [(int(a), int(b)) for a, b in zip(rng.integers(0, Nx // 2 + 1, 600), rng.integers(0, Ny, 600))]
                modes += [(Nx // 2, Ny // 2), (Nx // 2, Ny // 2 + 1), (0, Ny - 1), (Nx // 2, 0), (0, Ny // 2)]
            args = [v for mx, ky in modes for v in (mx, ky if ky <= Ny // 2 else ky - Ny)]
            lines = _run(exe, "shell", wx, wy, *args)
            assert [int(l[3]) for l in lines] == [int(sh[mx, ky]) for mx, ky in modes], (wx, wy, Nx, Ny)
