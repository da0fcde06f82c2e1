"""CPU tests (no GPU) of the zonal-spectrum entry points (swmhd_zonal_spectra_*, swmhd_ensemble_zonal_spectra_*,
swmhd_zonal_spectra_workspace): declared, exported and listed; every argument error is returned before any HIP call, with the codes the
zonal means answer to the same defects and then the new refusals in their stated order; a refused call leaves `out` and `workspace`
alone; the host mirror refuses a Bounded x direction, tracers and unsupported sizes before anything is allocated; and no instantiation
of the kernels uses scratch (gfx950 cross-compile)."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import zonal_return_code_cases as ZRC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOAT = {"f64": ctypes.c_double, "f32": ctypes.c_float}
LAUNCHING = [f"swmhd_{e}zonal_spectra_{sfx}" for e in ("", "ensemble_") for sfx in ("f64", "f32")]
SYMBOLS = LAUNCHING + ["swmhd_zonal_spectra_workspace"]
EINVAL, EHALO, ENOTSUP = 1, 2, 3
ZS = (("U", 1), ("V", 2), ("H", 4), ("A", 8), ("SPEED", 16), ("BX", 32), ("BY", 64), ("ALL", 127))
NAMES = ("u", "v", "h", "A", "s", "B_x", "B_y")
SENTINEL = -777.25


def test_spectra_symbols_declared_exported_and_listed(swmhd):
    B = swmhd._lib
    L = B.lib()
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    main, header = strip("swmhd.h"), strip("swmhd_spectra.h")
    assert re.search(r'^#include "swmhd_spectra.h"$', main, flags=re.M)          # swmhd.h brings them along
    declared = sorted(set(re.findall(r"\b(swmhd_[a-z0-9_]+)\s*\(", header)))
    assert declared == sorted(SYMBOLS) == sorted(B.SPECTRA_EXPORTS)
    for name in SYMBOLS:
        assert hasattr(L, name), f"{name} declared in include/swmhd_spectra.h but not exported by libswmhd.so"
        assert getattr(L, name).argtypes is not None
    assert all(getattr(L, n).restype is ctypes.c_int for n in LAUNCHING) and L.swmhd_zonal_spectra_workspace.restype is ctypes.c_int64
    lists = [set(B.EXPORTS), set(B.ZONAL_EXPORTS), set(B.DERIVED_EXPORTS), set(B.SPECTRA_EXPORTS)]      # disjoint
    assert sum(len(s) for s in lists) == len(set().union(*lists))
    assert not re.findall(r"\bswmhd_[a-z0-9_]*spectra[a-z0-9_]*\s*\(", main)          # swmhd.h itself declares none of them
    both = main + header
    for n, bit in ZS:
        assert re.search(rf"#define SWMHD_ZS_{n} {bit}\b", both)
    for n in ("U", "V", "H", "A", "SPEED", "BX", "BY"):      # the seven bits EQUAL the frame's
        out_bit = re.search(rf"#define SWMHD_OUT_{n} (\d+)\b", both).group(1)
        assert re.search(rf"#define SWMHD_ZS_{n} {out_bit}\b", both)
    assert tuple(B.ZS_BITS) == NAMES and B.ZS_BITS == B.OUT_BITS and (B.SPECTRA_MIN_NX, B.SPECTRA_MAX_NX) == (4, 4096)
    assert L.swmhd_version() == 300          # the additions are additive


def _buffers(sfx):
    buf = (FLOAT[sfx] * 64)()                  # (never dereferenced: every call below is refused first)
    obuf = (ctypes.c_double * 256)(*([SENTINEL] * 256))
    wbuf = (ctypes.c_double * 256)(*([SENTINEL] * 256))
    return buf, obuf, wbuf


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_spectra_refusals_without_gpu(swmhd, sfx):
    """Each refusal returns its code on a machine without a GPU (the checks precede every HIP call), in the order SWMHD_EINVAL, SWMHD_EHALO,
    SWMHD_ENOTSUP, "nothing to do", and the sentinels in and around `out` and `workspace` are untouched afterwards."""
    B = swmhd._lib
    L = B.lib()
    buf, obuf, wbuf = _buffers(sfx)
    p = ctypes.cast(buf, ctypes.c_void_p)
    o = ctypes.c_void_p(ctypes.addressof(obuf) + 64 * 8)      # 64 sentinels in front, 192 from `out` on
    w = ctypes.c_void_p(ctypes.addressof(wbuf) + 64 * 8)
    Nx = Ny = 8
    H, sy = 3, 14
    f = getattr(L, f"swmhd_zonal_spectra_{sfx}")

    def one(q1=p, A=p, Nx=Nx, Ny=Ny, Hx=H, Hy=H, sy=None, dx=1.0, dy=1.0, form=1, j0=0, j1=None, which=1 | 2 | 8 | 64, ws=w, out=o, osk=None, flags=0):
        sy = Nx + 2 * Hx if sy is None else sy
        return f(q1, p, p, A, Nx, Ny, Hx, Hy, sy, dx, dy, form, j0, Ny if j1 is None else j1, which, ws, out, Nx // 2 + 1 if osk is None else osk, flags, None)
    assert one(q1=None) == EINVAL and one(A=None) == EINVAL and one(out=None) == EINVAL and one(ws=None) == EINVAL     # null pointers
    assert one(Nx=0) == EINVAL and one(Ny=0) == EINVAL and one(sy=Nx + 2 * H - 1) == EINVAL and one(Hx=-1) == EINVAL   # extents
    assert one(dx=0.0) == EINVAL and one(dy=-1.0) == EINVAL and one(dx=float("nan")) == EINVAL      # spacing
    assert one(form=2) == EINVAL and one(form=-1) == EINVAL                                 # formulation
    assert one(j0=-1) == EINVAL and one(j1=Ny + 1) == EINVAL and one(j0=5, j1=4) == EINVAL  # rows
    assert one(which=0) == EINVAL and one(which=128) == EINVAL and one(which=1 | (1 << 20)) == EINVAL and one(which=-1) == EINVAL
    assert one(which=8192) == EINVAL                                                        # a second moment of the zonal means is no spectrum
    assert one(which=127, j0=4, j1=4) == 0 and one(which=64, j0=4, j1=4) == 0               # (all seven are known)
    assert one(osk=Nx // 2) == EINVAL and one(osk=0) == EINVAL and one(j0=3, j1=6, osk=3) == EINVAL     # Nx/2 + 1 entries, whatever the rows
    for fl in (B.STRICT, B.TILE_KERNEL, B.MARCH_KERNEL, B.BOUNDED_X, B.BOUNDED_Y, B.LEAVE_ROOM, B.RK3_ANCHOR, 8, 1 << 20):
        assert one(flags=fl) == EINVAL, fl                                                  # flags: WRAP_X | WRAP_Y only
        assert one(flags=fl | B.WRAP_X) == EINVAL, fl
    # reach: one cell, or the WRAP flag of THAT direction
    assert one(Hx=0) == EHALO and one(Hy=0) == EHALO and one(Hx=0, flags=B.WRAP_Y) == EHALO and one(Hy=0, flags=B.WRAP_X) == EHALO
    assert one(Hx=0, Hy=0, flags=B.WRAP_X) == EHALO and one(Hx=0, Hy=0, flags=B.WRAP_Y) == EHALO
    assert one(Hx=0, j0=4, j1=4, flags=B.WRAP_X) == 0 and one(Hx=0, Hy=0, j0=4, j1=4, flags=B.WRAP_X | B.WRAP_Y) == 0
    # an argument error outranks the halo
    assert one(Hx=0, q1=None) == EINVAL and one(Hx=0, ws=None) == EINVAL and one(Hx=0, which=0) == EINVAL and one(Hx=0, osk=Nx // 2) == EINVAL
    assert one(Hx=0, sy=Nx - 1) == EINVAL and one(Hy=0, flags=B.STRICT) == EINVAL and one(Hx=0, j0=5, j1=4) == EINVAL and one(Hx=0, dx=0.0) == EINVAL
    # the unsupported sizes: after SWMHD_EINVAL and SWMHD_EHALO, before "nothing to do"
    for bad in (3, 6, 2, 8192):
        assert one(Nx=bad) == ENOTSUP, bad
        assert one(Nx=bad, j0=4, j1=4) == ENOTSUP and one(Nx=bad, flags=B.WRAP_X | B.WRAP_Y) == ENOTSUP
        assert one(Nx=bad, Hx=0) == EHALO and one(Nx=bad, Hy=0, flags=B.WRAP_X) == EHALO                  # the halo outranks it
        assert one(Nx=bad, Hx=0, flags=B.WRAP_X) == ENOTSUP
        assert one(Nx=bad, osk=bad // 2) == EINVAL and one(Nx=bad, ws=None) == EINVAL and one(Nx=bad, which=0) == EINVAL
        assert one(Nx=bad, Hx=0, which=128) == EINVAL and one(Nx=bad, flags=B.STRICT) == EINVAL
    assert one(Nx=1) == ENOTSUP and one(Nx=12) == ENOTSUP and one(Nx=4097) == ENOTSUP and one(Nx=2 ** 20) == ENOTSUP
    for good in (4, 8, 64, 4096):
        assert one(Nx=good, j0=4, j1=4) == 0
    assert one(Hx=0, j0=4, j1=4) == EHALO                                                   # ... and the halo outranks "nothing to do"
    assert one(j0=4, j1=4) == 0 and one(j0=4, j1=4, flags=B.WRAP_X | B.WRAP_Y) == 0 and one(j0=Ny, j1=Ny) == 0   # an empty row range enqueues nothing

    e = getattr(L, f"swmhd_ensemble_zonal_spectra_{sfx}")

    def ens(members=2, stride_m=None, Nx=Nx, which=1 | 2 | 8 | 64, ws=w, out=o, osk=None, osm=None, flags=0, Hx=H, j0=0, j1=Ny, q2=p):
        sy = Nx + 2 * Hx
        osk = Nx // 2 + 1 if osk is None else osk
        return e(p, q2, p, p, members, (Ny + 2 * H) * sy if stride_m is None else stride_m, Nx, Ny, Hx, H, sy, 1.0, 1.0, 1, j0, j1, which, ws, out, osk,
                 bin(which & 127).count("1") * osk if osm is None else osm, flags, None)
    sm = (Ny + 2 * H) * sy
    assert ens(members=0) == EINVAL and ens(members=-2) == EINVAL and ens(members=B.ENSEMBLE_MAX_MEMBERS + 1) == EINVAL
    assert ens(stride_m=sm - 1) == EINVAL                                                   # members would overlap
    assert ens(osm=4 * 5 - 1) == EINVAL and ens(which=127, osm=7 * 5 - 1) == EINVAL         # member spectra would overlap
    assert ens(which=1, osm=4) == EINVAL and ens(which=1, osm=5, Hx=0) == EHALO and ens(which=1, osm=5, Hx=0, flags=B.WRAP_X, j0=2, j1=2) == 0
    assert ens(which=0) == EINVAL and ens(out=None) == EINVAL and ens(ws=None) == EINVAL and ens(q2=None) == EINVAL and ens(flags=B.STRICT) == EINVAL
    assert ens(osk=4) == EINVAL and ens(which=128) == EINVAL
    assert ens(Hx=0) == EHALO and ens(Hx=0, members=0) == EINVAL and ens(Hx=0, osm=0) == EINVAL
    for bad in (3, 6, 2, 8192):
        assert ens(Nx=bad) == ENOTSUP and ens(Nx=bad, j0=2, j1=2) == ENOTSUP and ens(Nx=bad, Hx=0) == EHALO and ens(Nx=bad, members=0) == EINVAL
        assert ens(Nx=bad, osm=0) == EINVAL
    assert ens(members=B.ENSEMBLE_MAX_MEMBERS, j0=2, j1=2) == 0                             # valid and empty: nothing is enqueued
    assert all(v == SENTINEL for v in obuf) and all(v == SENTINEL for v in wbuf)


# --- which code wins: the recorded matrix of the zonal means, answered by the spectra twin ------------------------------------------------
# (as tests/test_zonal_abi.py: with a device a library that wrongly accepted a defect case would launch on host pointers)
no_device = pytest.mark.skipif(torch.cuda.is_available(), reason="the cases pass host pointers: only without a device")
TWINS = [(f"{name}_{sfx}", f"swmhd_{name.replace('zonal_means', 'zonal_spectra')}_{sfx}", name, sfx) for name in ZRC.SIGNATURES for sfx in ("f64", "f32")]


def _twin_call(L, sym, name, sfx, changes):
    """The case of the zonal means on the spectra twin: the same arguments, a workspace in front of `out`."""
    names = ZRC.SIGNATURES[name].split()
    names.insert(names.index("out"), "workspace")
    fn = getattr(L, sym)
    assert len(names) == len(fn.argtypes), (sym, len(names), len(fn.argtypes))
    v = dict(ZRC.BASE, **{a: ZRC._pointer(sfx, a) for a in ZRC.POINTERS}, workspace=ZRC._pointer(sfx, "out"))
    v.update(changes)
    return fn(*[v[a] for a in names])


@no_device
@pytest.mark.parametrize("twin", TWINS, ids=[t[1] for t in TWINS])
def test_every_recorded_zonal_case_gives_the_same_code_from_the_spectra_twin(swmhd, twin):
    """Every label of tests/golden/zonal_return_codes.json that has a counterpart: the defects of the shared arguments (`unknown profile
    bit` 1 << 14 is unknown to the seven-bit mask too; out_stride_m = 15 is one short of two spectra 8 apart as of two profiles).  The
    one without: `out_stride_k one short` is 7 against 8 rows, and a spectrum has Nx/2 + 1 = 5 entries whatever the rows -- that
    defect of the spectra stands in test_spectra_refusals_without_gpu."""
    key, sym, name, sfx = twin
    L = swmhd._lib.lib()
    assert _twin_call(L, sym, name, sfx, {}) == -100          # the baseline gets past every check: it reaches HIP (no device)
    cases, want = ZRC.cases(name), ZRC.load_golden()[key]
    assert len(want) == len(cases) > 100
    wrong, compared = [], 0
    for (kind, label, ch), w in zip(cases, want):
        if "out_stride_k one short" in label:
            continue
        compared += 1
        got = _twin_call(L, sym, name, sfx, ch)
        if str(got) != w:
            wrong.append(f"{label}: {got}, the zonal means recorded {w}")
    assert not wrong, f"{len(wrong)} of {len(cases)} cases:\n" + "\n".join(wrong[:20])
    assert compared > 100 and compared >= len(cases) * 0.85
    # the new defects on top of the recorded ones: a null workspace is an argument error, an unsupported size comes last
    assert _twin_call(L, sym, name, sfx, dict(workspace=None)) == EINVAL and _twin_call(L, sym, name, sfx, dict(workspace=None, Hx=0)) == EINVAL
    for Nx in (3, 6, 2):
        assert _twin_call(L, sym, name, sfx, dict(Nx=Nx)) == ENOTSUP and _twin_call(L, sym, name, sfx, dict(Nx=Nx, Hx=0)) == EHALO
        assert _twin_call(L, sym, name, sfx, dict(Nx=Nx, which=0)) == EINVAL and _twin_call(L, sym, name, sfx, dict(Nx=Nx, j0=4, j1=4)) == ENOTSUP


def test_host_mirror_refuses_before_any_allocation(swmhd):
    """A Bounded x direction, a tracer name, an unknown name and Nx = 192 raise SwmhdError while the names and the grid are being read:
    the stub has no state to launch on and no library handle to size a workspace with."""
    S = swmhd
    E = S._lib.SwmhdError
    from swmhd_amd import spectra as Z
    assert Z._runs(NAMES) == [[1 << k for k in range(7)]]
    assert Z._runs(("u", "v", "A")) == [[1, 2, 8]] and Z._runs(("B_y", "u", "u", "s", "A")) == [[64], [1], [1, 16], [8]]
    for bad in (("u", "w"), ("c",), ("uu",), ("vA",), ("U",)):
        with pytest.raises(E, match="one of u v h A s B_x B_y"):
            Z._runs(bad)
    with pytest.raises(E, match="is a tracer"):
        Z._runs(("u", "c"), tracers=("c",))
    with pytest.raises(E, match="no names"):
        Z._runs(())

    class Stub:      # what zonal_spectra and the writer read of a model before the first allocation
        tracer_names = ("dye",)
        members = None

        def __init__(self, Nx, topology=("Periodic", "Periodic", "Flat")):
            self.grid = S.RectilinearGrid(size=(Nx, 24), x=(0, 1), y=(0, 1), topology=topology)

        def _join(self):
            raise AssertionError("reached the model: the refusals were not checked first")

        @property
        def _L(self):
            raise AssertionError("reached the library: the refusals were not checked first")

    for stub, names, what in ((Stub(64), ("u", "dye"), "is a tracer"), (Stub(64), ("q",), "one of"), (Stub(64), (), "no names"),
                              (Stub(64, ("Bounded", "Periodic", "Flat")), ("u",), "Bounded"), (Stub(64, ("Bounded", "Bounded", "Flat")), ("A",), "Bounded"),
                              (Stub(192), ("u",), "power of two"), (Stub(2), ("u",), "power of two"), (Stub(8192), ("u",), "power of two")):
        with pytest.raises(E, match=what):
            Z.enqueue_zonal_spectra(stub, names)
        with pytest.raises(E, match=what):
            S.ZonalSpectrumTimeSeries(stub, names, capacity=4)
    for cap in (None, 0, -3):
        with pytest.raises(E, match="capacity"):
            S.ZonalSpectrumTimeSeries(Stub(64), ("u", "B_x"), capacity=cap)
    w = S.ZonalSpectrumTimeSeries(Stub(64, ("Periodic", "Bounded", "Flat")), ("u", "B_x"), schedule=S.IterationInterval(3), capacity=2)
    assert len(w) == 0 and w.capacity == 2 and w.times == [] and w.iterations == [] and w.schedule.steps(0.01) == 3 and w.names == ("u", "B_x")
    assert S.ZonalSpectrumTimeSeries(Stub(4), capacity=1).names == ("u", "v", "A") and S.ZonalSpectrumTimeSeries(Stub(4096), capacity=1).schedule == S.TimeInterval(0.1)
    assert "ZonalSpectrumTimeSeries" in S.__all__
    for cls in (S.ShallowWaterModel, S.ShallowWaterEnsemble, S.BoundedShallowWaterEnsemble):
        assert callable(cls.zonal_spectra)
    # the means' names and error texts are what they were
    from swmhd_amd import zonal as ZM
    with pytest.raises(E, match="one of u v h A s B_x B_y uu vv uv"):
        ZM._runs(("w",))


HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# the flags swmhd_amd/csrc/Makefile compiles spectra.o with (STRICT)
STRICT_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"]


def test_spectra_kernels_use_no_scratch(tmp_path):
    """All eight instantiations of pass 1 (model type x ensemble x threads per row) and pass 2 report ScratchSize 0; pass 1 takes its LDS
    at launch (12 Nx bytes per row in flight: launch_plan.hpp), pass 2 a fixed 2 KiB."""
    out = subprocess.run([HIPCC, *STRICT_FLAGS, "--offload-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                          os.path.join(ROOT, "swmhd_amd", "csrc", "spectra.hip"), "-o", str(tmp_path / "s.o")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    res = {}
    for block in re.split(r"remark: [^\n]*Function Name: ", out.stderr)[1:]:
        name = block.split("\n")[0].split(" ")[0]
        num = lambda what: int(re.search(what + r": (\d+)", block).group(1))
        res[name] = (num(r"ScratchSize \[bytes/lane\]"), num(r"LDS Size \[bytes/block\]"), num(r"Occupancy \[waves/SIMD\]"))
    rows = {n: v for n, v in res.items() if "k_spectra_rows" in n}
    sums = {n: v for n, v in res.items() if "k_spectra_sum" in n}
    assert len(rows) == 8 and len(sums) == 1 and len(res) == 9, sorted(res)
    print("waves per SIMD:", {n: v[2] for n, v in res.items()})      # (reported: register allocation is the compiler's)
    assert all(v[0] == 0 for v in res.values()), res
    assert all(v[1] == 0 for v in rows.values()) and all(v[1] == 16 * 16 * 8 for v in sums.values()), res
    assert all(v[2] >= 3 for v in rows.values()), rows      # three 48 KiB workgroups of four waves per CU at Nx = 4096: LDS, not registers, is the limit


def test_makefile_builds_spectra_strict():
    mk = open(os.path.join(ROOT, "swmhd_amd", "csrc", "Makefile")).read()
    assert re.search(r"^spectra\.o: FAST := \$\(STRICT\)$", mk, flags=re.M) and re.search(r"^OBJS \+= spectra\.o$", mk, flags=re.M)
    assert "swmhd_spectra.h" in re.search(r"^HDRS\s*:=(.*)$", mk, flags=re.M).group(1)
