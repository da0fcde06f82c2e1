"""CPU tests (no GPU) of the zonal-mean entry points (swmhd_zonal_means_*, swmhd_ensemble_zonal_means_*): declared and exported, every
argument error is returned before any HIP call and in the order of the output frames' checks, a refused call leaves `out` alone, the
host mirror refuses bad names before any launch, and no instantiation of the kernel uses scratch (gfx950 cross-compile)."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import return_code_cases as RC
import zonal_return_code_cases as ZRC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOAT = {"f64": ctypes.c_double, "f32": ctypes.c_float}
SYMBOLS = [f"swmhd_{e}zonal_means_{sfx}" for e in ("", "ensemble_") for sfx in ("f64", "f32")]
EINVAL, EHALO = 1, 2
ZM = (("U", 1), ("V", 2), ("H", 4), ("A", 8), ("SPEED", 16), ("BX", 32), ("BY", 64), ("UU", 128), ("VV", 256), ("UV", 512), ("BXBX", 1024),
      ("BYBY", 2048), ("BXBY", 4096), ("VA", 8192), ("ALL", 16383))
NAMES = ("u", "v", "h", "A", "s", "B_x", "B_y", "uu", "vv", "uv", "B_xB_x", "B_yB_y", "B_xB_y", "vA")
SENTINEL = -777.25


def test_zonal_symbols_declared_and_exported(swmhd):
    L = swmhd._lib.lib()
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    main, header = strip("swmhd.h"), strip("swmhd_zonal.h")
    assert re.search(r'^#include "swmhd_zonal.h"$', main, flags=re.M)          # swmhd.h brings them along
    declared = sorted(set(re.findall(r"\b(swmhd_[a-z0-9_]+)\s*\(", header)))
    assert declared == sorted(SYMBOLS) == sorted(swmhd._lib.ZONAL_EXPORTS)
    for name in SYMBOLS:
        assert hasattr(L, name), f"{name} declared in include/swmhd_zonal.h but not exported by libswmhd.so"
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is ctypes.c_int
    header = main + header
    for n, bit in ZM:
        assert re.search(rf"#define SWMHD_ZM_{n} {bit}\b", header)
    for n in ("U", "V", "H", "A", "SPEED", "BX", "BY"):      # the low seven bits EQUAL the frame's
        out_bit = re.search(rf"#define SWMHD_OUT_{n} (\d+)\b", header).group(1)
        assert re.search(rf"#define SWMHD_ZM_{n} {out_bit}\b", header)
    B = swmhd._lib
    assert tuple(B.ZM_BITS) == NAMES and [B.ZM_BITS[n] for n in NAMES] == [1 << k for k in range(14)]
    assert all(B.ZM_BITS[n] == b for n, b in B.OUT_BITS.items())
    assert L.swmhd_version() == 300          # the additions are additive


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_zonal_refusals_without_gpu(swmhd, sfx):
    """Each SWMHD_EINVAL / SWMHD_EHALO case returns its code on a machine without a GPU (the checks precede every HIP call), an argument
    error outranks SWMHD_EHALO, and the sentinels in and around `out` are untouched afterwards."""
    B = swmhd._lib
    L = B.lib()
    buf = (FLOAT[sfx] * 64)()                  # (never dereferenced: every call below is refused first)
    p = ctypes.cast(buf, ctypes.c_void_p)
    obuf = (ctypes.c_double * 256)(*([SENTINEL] * 256))
    o = ctypes.c_void_p(ctypes.addressof(obuf) + 64 * 8)      # 64 sentinels in front, 192 from `out` on
    Nx = Ny = 8
    H, sy = 3, 14
    f = getattr(L, f"swmhd_zonal_means_{sfx}")

    def one(q1=p, A=p, Nx=Nx, Ny=Ny, Hx=H, Hy=H, sy=sy, dx=1.0, dy=1.0, form=1, j0=0, j1=Ny, which=1 | 2 | 8 | 512, out=o, osk=Ny, flags=0):
        return f(q1, p, p, A, Nx, Ny, Hx, Hy, sy, dx, dy, form, j0, j1, which, out, osk, flags, None)
    assert one(q1=None) == EINVAL and one(A=None) == EINVAL and one(out=None) == EINVAL      # null pointers
    assert one(Nx=0) == EINVAL and one(Ny=0) == EINVAL and one(sy=Nx + 2 * H - 1) == EINVAL and one(Hx=-1) == EINVAL   # extents
    assert one(dx=0.0) == EINVAL and one(dy=-1.0) == EINVAL and one(dx=float("nan")) == EINVAL      # spacing
    assert one(form=2) == EINVAL and one(form=-1) == EINVAL                                 # formulation
    assert one(j0=-1) == EINVAL and one(j1=Ny + 1) == EINVAL and one(j0=5, j1=4) == EINVAL  # rows
    assert one(which=0) == EINVAL                                                          # empty mask
    assert one(which=1 << 14) == EINVAL and one(which=1 | (1 << 20)) == EINVAL and one(which=-1) == EINVAL   # unknown bits
    assert one(which=16383, j0=4, j1=4) == 0 and one(which=8192, j0=4, j1=4) == 0          # (all fourteen are known)
    assert one(osk=Ny - 1) == EINVAL and one(j0=3, j1=6, osk=2) == EINVAL                   # profiles would overlap
    assert one(j0=3, j1=6, osk=3, Hx=0) == EHALO                                            # ... for a row range: its own extent
    for fl in (B.STRICT, B.TILE_KERNEL, B.MARCH_KERNEL, B.BOUNDED_X, B.BOUNDED_Y, B.LEAVE_ROOM, B.RK3_ANCHOR, 8, 1 << 20):
        assert one(flags=fl) == EINVAL, fl                                                  # flags: WRAP_X | WRAP_Y only
        assert one(flags=fl | B.WRAP_X) == EINVAL, fl
    assert one(Hx=0) == EHALO and one(Hy=0) == EHALO and one(Hy=0, flags=B.WRAP_X | B.WRAP_Y) == EHALO    # reach: one cell
    # an argument error outranks the halo
    assert one(Hx=0, q1=None) == EINVAL and one(Hx=0, which=0) == EINVAL and one(Hx=0, osk=Ny - 1) == EINVAL
    assert one(Hx=0, sy=Nx - 1) == EINVAL and one(Hy=0, flags=B.STRICT) == EINVAL and one(Hx=0, j0=5, j1=4) == EINVAL and one(Hx=0, dx=0.0) == EINVAL
    assert one(Hx=0, j0=4, j1=4) == EHALO                                                   # ... and the halo outranks "nothing to do"
    assert one(j0=4, j1=4) == 0 and one(j0=4, j1=4, osk=0, flags=B.WRAP_X | B.WRAP_Y) == 0 and one(j0=Ny, j1=Ny) == 0   # an empty row range enqueues nothing

    e = getattr(L, f"swmhd_ensemble_zonal_means_{sfx}")
    sm = (Ny + 2 * H) * sy

    def ens(members=2, stride_m=sm, which=1 | 2 | 8 | 512, out=o, osk=Ny, osm=4 * Ny, flags=0, Hx=H, j0=0, j1=Ny, q2=p):
        return e(p, q2, p, p, members, stride_m, Nx, Ny, Hx, H, sy, 1.0, 1.0, 1, j0, j1, which, out, osk, osm, flags, None)
    assert ens(members=0) == EINVAL and ens(members=-2) == EINVAL and ens(members=B.ENSEMBLE_MAX_MEMBERS + 1) == EINVAL
    assert ens(stride_m=sm - 1) == EINVAL                                                   # members would overlap
    assert ens(osm=4 * Ny - 1) == EINVAL and ens(which=16383, osm=14 * Ny - 1) == EINVAL    # member profiles would overlap
    assert ens(which=1, osm=Ny - 1) == EINVAL and ens(which=1, osm=Ny, Hx=0) == EHALO
    assert ens(which=0) == EINVAL and ens(out=None) == EINVAL and ens(q2=None) == EINVAL and ens(flags=B.STRICT) == EINVAL
    assert ens(osk=Ny - 1) == EINVAL and ens(which=1 << 14) == EINVAL
    assert ens(Hx=0) == EHALO and ens(Hx=0, members=0) == EINVAL and ens(Hx=0, osm=0) == EINVAL
    assert ens(members=B.ENSEMBLE_MAX_MEMBERS, j0=2, j1=2, osk=0, osm=0) == 0               # valid and empty: nothing is enqueued
    assert all(v == SENTINEL for v in obuf)


# --- which code wins: the recorded matrix (tests/zonal_return_code_cases.py, tests/golden/zonal_return_codes.json) -------------------
# (as tests/test_return_codes_cpu.py: with a device a library that wrongly accepted a defect case would launch on host pointers)
no_device = pytest.mark.skipif(torch.cuda.is_available(), reason="the cases pass host pointers: only without a device")
ENTRIES = ZRC.entries()


@no_device
def test_every_zonal_entry_point_has_recorded_cases(swmhd):
    """Whoever adds an entry point to include/swmhd_zonal.h (_lib.ZONAL_EXPORTS) records its matrix."""
    assert set(swmhd._lib.ZONAL_EXPORTS) == {sym for _, sym, _, _ in ENTRIES}
    assert set(ZRC.load_golden()) == {key for key, _, _, _ in ENTRIES}
    assert not set(swmhd._lib.ZONAL_EXPORTS) & set(swmhd._lib.EXPORTS)


@no_device
@pytest.mark.parametrize("entry", ENTRIES, ids=[e[0] for e in ENTRIES])
def test_zonal_return_codes_are_the_recorded_ones(swmhd, entry):
    key, _sym, name, _sfx = entry
    cases, want = ZRC.cases(name), ZRC.load_golden()[key]
    assert len(want) == len(cases), "the golden file was recorded for another list of cases"
    got = ZRC.run(swmhd._lib.lib(), entry)
    wrong = [f"{label}: {g}, recorded {w}" for (_, label, _), g, w in zip(cases, got, want) if g != w]
    assert not wrong, f"{len(wrong)} of {len(cases)} cases:\n" + "\n".join(wrong[:20])


@no_device
@pytest.mark.parametrize("entry", ENTRIES, ids=[e[0] for e in ENTRIES])
def test_checks_come_in_the_order_of_the_output_frames(swmhd, entry):
    """Wherever a zonal-mean entry point and its output-frame counterpart have a case of the same label -- every single defect and
    every pair -- the recorded answers are the same code: an argument error outranks SWMHD_EHALO, which outranks an empty row range."""
    key, _sym, name, sfx = entry
    frame = name.replace("zonal_means", "output_fields")
    zc = dict(zip([lab for _, lab, _ in ZRC.cases(name)], ZRC.load_golden()[key]))
    fc = dict(zip([lab for _, lab, _ in RC.cases(frame)], RC.load_golden()[f"{frame}_{sfx}"]))
    common = [lab for lab in zc if lab in fc]
    assert len(common) > 100 and [lab for lab in common if zc[lab] != fc[lab]] == []
    assert zc["Hx = 0"] == "2" and zc["q1 null + Hx = 0"] == "1" and zc["Hx = 0 + out_stride_k one short"] == "1"
    assert zc["Hx = 0 + unknown profile bit"] == "1" and zc["j0 == j1"] == "0" and zc["j0 == j1 + Hx = 0"] == "2"


def test_name_and_constructor_refusals_raise_before_any_launch(swmhd):
    """On a machine without a GPU a launch would fail in its own way; these raise SwmhdError while the names are still being read."""
    S = swmhd
    E = S._lib.SwmhdError
    from swmhd_amd import zonal as Z
    assert Z._runs(NAMES) == [[1 << k for k in range(14)]]
    assert Z._runs(("u", "v", "A")) == [[1, 2, 8]] and Z._runs(("vA", "u", "u", "uv", "s")) == [[8192], [1], [1, 512], [16]]
    for bad in (("u", "w"), ("c",), ("uB",), ("U",), ("B_xB_z",)):
        with pytest.raises(E, match="one of u v h A s B_x B_y uu vv uv B_xB_x B_yB_y B_xB_y vA"):
            Z._runs(bad)
    with pytest.raises(E, match="is a tracer"):
        Z._runs(("u", "c"), tracers=("c",))
    with pytest.raises(E, match="no names"):
        Z._runs(())

    class Stub:      # what zonal_means and the writer read of a model before the first launch
        tracer_names = ("dye",)
        members = None

        def _join(self):
            raise AssertionError("reached the model: the names were not checked first")
    for names in (("u", "dye"), ("q",), ()):
        with pytest.raises(E):
            Z.enqueue_zonal_means(Stub(), names)
        with pytest.raises(E):
            S.ZonalMeanTimeSeries(Stub(), names, capacity=4)
    for cap in (None, 0, -3):
        with pytest.raises(E, match="capacity"):
            S.ZonalMeanTimeSeries(Stub(), ("u", "vA"), capacity=cap)
    w = S.ZonalMeanTimeSeries(Stub(), ("u", "vA"), schedule=S.IterationInterval(3), capacity=2)
    assert len(w) == 0 and w.capacity == 2 and w.times == [] and w.iterations == [] and w.schedule.steps(0.01) == 3 and w.names == ("u", "vA")
    assert S.ZonalMeanTimeSeries(Stub(), capacity=1).names == ("u", "v", "A") and S.ZonalMeanTimeSeries(Stub(), capacity=1).schedule == S.TimeInterval(0.1)
    assert "ZonalMeanTimeSeries" in S.__all__
    for cls in (S.ShallowWaterModel, S.ShallowWaterEnsemble, S.BoundedShallowWaterEnsemble):
        assert callable(cls.zonal_means)
    # the frames' names and error texts are what they were
    from swmhd_amd import output as O
    assert S._lib.OUT_BITS == {"u": 1, "v": 2, "h": 4, "A": 8, "s": 16, "B_x": 32, "B_y": 64}
    with pytest.raises(E, match="one of u v h A s B_x B_y \\(velocities"):
        O._runs(("uu",))


HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# the flags swmhd_amd/csrc/Makefile compiles zonal.o with (STRICT)
STRICT_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"]


def test_zonal_kernels_use_no_scratch_and_no_lds(tmp_path):
    """All eight instantiations (model type x ensemble x mask class) report ScratchSize 0 and no LDS."""
    out = subprocess.run([HIPCC, *STRICT_FLAGS, "--offload-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                          os.path.join(ROOT, "swmhd_amd", "csrc", "zonal.hip"), "-o", str(tmp_path / "z.o")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    res = {}
    for block in re.split(r"remark: [^\n]*Function Name: ", out.stderr)[1:]:
        name = block.split("\n")[0].split(" ")[0]
        num = lambda what: int(re.search(what + r": (\d+)", block).group(1))
        res[name] = (num(r"ScratchSize \[bytes/lane\]"), num(r"LDS Size \[bytes/block\]"), num(r"Occupancy \[waves/SIMD\]"))
    kernels = {n: v for n, v in res.items() if "k_zonal_means" in n}
    assert len(kernels) == 8, sorted(res)
    print("waves per SIMD:", {n: v[2] for n, v in kernels.items()})      # (reported: register allocation is the compiler's)
    assert all(v[0] == 0 and v[1] == 0 for v in kernels.values()), kernels


def test_makefile_builds_zonal_strict():
    mk = open(os.path.join(ROOT, "swmhd_amd", "csrc", "Makefile")).read()
    assert re.search(r"^zonal\.o: FAST := \$\(STRICT\)$", mk, flags=re.M) and re.search(r"^OBJS \+= zonal\.o$", mk, flags=re.M)
