"""CPU tests (no GPU) of the derived-frame entry points (swmhd_derived_fields_*, swmhd_ensemble_derived_fields[_params]_*): declared and
exported, every argument error is returned before any HIP call with the code the output frames' twin answers for the same defect (the
recorded matrix tests/golden/return_codes.json), a refused call leaves `out` alone, the host mirror refuses bad names before any launch,
no instantiation of the kernel uses scratch or LDS (gfx950 cross-compile), and the launch plan holds under the host sanitizers."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import return_code_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOAT = {"f64": ctypes.c_double, "f32": ctypes.c_float}
NAMES = ("derived_fields", "ensemble_derived_fields", "ensemble_derived_fields_params")
SYMBOLS = [f"swmhd_{n}_{sfx}" for n in NAMES for sfx in ("f64", "f32")]
DRV = (("VORTICITY", 1), ("DIVERGENCE", 2), ("CURRENT", 4), ("PV", 8), ("ALL", 15))
FIELDS = ("vorticity", "divergence", "current", "potential_vorticity")
EINVAL, EHALO = 1, 2
SENTINEL = -777.25
# a derived call: its output-frame twin (whose recorded answers it must give) and the argument that follows `formulation`
TWIN = {"derived_fields": ("output_fields", "fcor"), "ensemble_derived_fields": ("ensemble_output_fields", "fcor"),
        "ensemble_derived_fields_params": ("ensemble_output_fields", "params")}


def test_derived_symbols_declared_and_exported(swmhd):
    L, B = swmhd._lib.lib(), swmhd._lib
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    main, header = strip("swmhd.h"), strip("swmhd_derived.h")
    assert re.search(r'^#include "swmhd_derived.h"$', main, flags=re.M)          # swmhd.h brings them along
    declared = sorted(set(re.findall(r"\b(swmhd_[a-z0-9_]+)\s*\(", header)))
    assert declared == sorted(SYMBOLS) == sorted(B.DERIVED_EXPORTS)
    for name in SYMBOLS:
        assert hasattr(L, name), f"{name} declared in include/swmhd_derived.h but not exported by libswmhd.so"
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is ctypes.c_int
    for n, bit in DRV:
        assert re.search(rf"#define SWMHD_DRV_{n} {bit}\b", header)
    assert tuple(B.DRV_BITS) == FIELDS and [B.DRV_BITS[n] for n in FIELDS] == [1, 2, 4, 8]
    assert not set(B.DERIVED_EXPORTS) & (set(B.EXPORTS) | set(B.ZONAL_EXPORTS))
    assert not set(B.DRV_BITS) & set(B.ZM_BITS)
    assert B.OUT_BITS == {"u": 1, "v": 2, "h": 4, "A": 8, "s": 16, "B_x": 32, "B_y": 64}      # the frame's seven are what they were
    assert L.swmhd_version() == 300          # the additions are additive
    # the twins' signatures: coriolis_f (or the table) after the formulation, nothing else
    for sfx in ("f64", "f32"):
        for name, (twin, extra) in TWIN.items():
            want = list(getattr(L, f"swmhd_{twin}_{sfx}").argtypes)
            k = RC.SIGNATURES[twin].split().index("formulation") + 1
            want.insert(k, ctypes.c_void_p if extra == "params" else FLOAT[sfx])
            assert list(getattr(L, f"swmhd_{name}_{sfx}").argtypes) == want, (name, sfx)


def _signature(name):
    twin, extra = TWIN[name]
    args = RC.SIGNATURES[twin].split()
    args.insert(args.index("formulation") + 1, extra)
    return args


def _out_buffer():
    buf = (ctypes.c_double * 256)(*([SENTINEL] * 256))
    return buf, ctypes.c_void_p(ctypes.addressof(buf) + 64 * 8)      # 64 sentinels in front, 192 from `out` on


def _call(L, name, sfx, changes, out):
    """RC.call for a derived entry point: the baseline of the twin's matrix with `changes` on top, `out` a buffer of this test's"""
    fn = getattr(L, f"swmhd_{name}_{sfx}")
    args = _signature(name)
    assert len(args) == len(fn.argtypes)
    v = dict(RC.BASE, flags=0, out=out)
    for k, x in changes.items():
        if k == "flags":
            v["flags"] |= x
        else:
            v[k] = x
    return fn(*[RC._value(v[a], sfx, t) for a, t in zip(args, fn.argtypes)])


# (as tests/test_return_codes_cpu.py: with a device a library that wrongly accepted a defect case would launch on host pointers)
no_device = pytest.mark.skipif(torch.cuda.is_available(), reason="the cases pass host pointers: only without a device")
ENTRIES = [(n, sfx) for n in NAMES for sfx in ("f64", "f32")]


@no_device
@pytest.mark.parametrize("name,sfx", ENTRIES, ids=[f"{n}_{s}" for n, s in ENTRIES])
def test_argument_errors_answer_as_the_output_frames_do(swmhd, name, sfx):
    """Every label recorded for the output-frame twin -- single defects, pairs, the empty row range and each defect on top of it -- gets
    the recorded code from the derived call.  The record is that of the library before this entry point existed."""
    L = swmhd._lib.lib()
    twin = TWIN[name][0]
    cases, want = RC.cases(twin), RC.load_golden()[f"{twin}_{sfx}"]
    assert len(want) == len(cases) > 100, "the golden file was recorded for another list of cases"
    buf, out = _out_buffer()
    assert _call(L, name, sfx, {}, out) == -100          # the baseline gets past every check and reaches HIP (no device)
    wrong = []
    for (kind, label, ch), w in zip(cases, want):
        if "out" in ch:
            ch = dict(ch, out=None)
        got = _call(L, name, sfx, ch, out)
        if str(got) != w:
            wrong.append(f"{label}: {got}, recorded {w}")
    assert not wrong, f"{len(wrong)} of {len(cases)} cases:\n" + "\n".join(wrong[:20])
    by_label = dict(zip([lab for _, lab, _ in cases], want))
    assert by_label["Hx = 0"] == "2" and by_label["q1 null + Hx = 0"] == "1" and by_label["j0 == j1"] == "0" and by_label["j0 == j1 + Hx = 0"] == "2"
    assert all(v == SENTINEL for v in buf)


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_derived_refusals_without_gpu(swmhd, sfx):
    """The two additions to the frame's checks -- a mask outside SWMHD_DRV_ALL, params == NULL -- and their place in the order: an
    argument error outranks SWMHD_EHALO, which outranks an empty row range; coriolis_f is not validated; `out` is left alone.  Every
    call here is refused (or empty) before the first HIP call, so this runs on any machine."""
    B = swmhd._lib
    L = B.lib()
    buf, out = _out_buffer()
    nan = float("nan")
    for name in NAMES:
        one = lambda **ch: _call(L, name, sfx, ch, out)
        assert one(owhich=16) == EINVAL and one(owhich=15 | 16) == EINVAL and one(owhich=127) == EINVAL and one(owhich=-1) == EINVAL
        assert one(owhich=0) == EINVAL and one(owhich=1 << 20) == EINVAL
        for which in (1, 2, 4, 8, 15, 5):                                     # (all four are known)
            assert one(owhich=which, j0=4, j1=4, osm=256) == 0
        assert one(owhich=15, osm=256, j0=4, j1=4, Hx=0) == EHALO and one(owhich=16, Hx=0) == EINVAL
        for fl in (B.STRICT, B.TILE_KERNEL, B.MARCH_KERNEL, B.BOUNDED_X, B.BOUNDED_Y, B.LEAVE_ROOM, B.RK3_ANCHOR, 8, 1 << 20):
            assert one(flags=fl) == EINVAL and one(flags=fl | B.WRAP_X) == EINVAL, fl  # flags: WRAP_X | WRAP_Y only
        assert one(j0=4, j1=4, flags=B.WRAP_X | B.WRAP_Y) == 0 and one(Hy=0, flags=B.WRAP_X | B.WRAP_Y) == EHALO
        assert one(elem=3) == EINVAL and one(osy=7) == EINVAL and one(osf=63) == EINVAL and one(j0=3, j1=6, osf=23) == EINVAL
        assert one(j0=3, j1=6, osf=24, Hx=0) == EHALO
        if name.endswith("params"):
            assert one(params=None) == EINVAL and one(params=None, j0=4, j1=4) == EINVAL and one(params=None, Hx=0) == EINVAL
            assert one(params=None, members=0) == EINVAL and one(params=None, owhich=16) == EINVAL
        else:
            assert one(fcor=nan, j0=4, j1=4) == 0 and one(fcor=nan, Hx=0) == EHALO and one(fcor=float("inf"), owhich=0) == EINVAL
        if name.startswith("ensemble"):
            assert one(members=0) == EINVAL and one(members=B.ENSEMBLE_MAX_MEMBERS + 1) == EINVAL and one(stride_m=14 * 14 - 1) == EINVAL
            assert one(osm=127) == EINVAL and one(owhich=15, osm=255) == EINVAL and one(owhich=15, osm=256, Hx=0) == EHALO
            assert one(members=B.ENSEMBLE_MAX_MEMBERS, j0=2, j1=2, osf=0, osm=0) == 0        # valid and empty: nothing is enqueued
    assert all(v == SENTINEL for v in buf)


def test_name_refusals_raise_before_any_launch(swmhd):
    """On a machine without a GPU a launch would fail in its own way; these raise SwmhdError while the names are still being read."""
    S = swmhd
    E = S._lib.SwmhdError
    from swmhd_amd import derived as D, output as O
    assert D._runs(FIELDS) == [[1, 2, 4, 8]] and D._runs(("current", "vorticity", "vorticity", "potential_vorticity")) == [[4], [1], [1, 8]]
    for bad in (("vorticity", "u"), ("zeta",), ("Vorticity",), ("pv",), ("J",)):
        with pytest.raises(E, match="one of vorticity divergence current potential_vorticity"):
            D._runs(bad)
    with pytest.raises(E, match="'current' is a tracer: frames hold u v h A s B_x B_y only"):       # today's message, before the name is looked up
        D._runs(("current", "zeta"), tracers=("current",))
    with pytest.raises(E, match="no field names"):
        D._runs(())
    # the writer's runs: a run ends where the bits stop ascending and where the kernel changes; the seven alone are what they were
    assert O._frame_runs(("u", "v", "A", "s")) == [(False, [1, 2, 8, 16])] and O._runs(("u", "v", "A", "s")) == [[1, 2, 8, 16]]
    assert O._frame_runs(("u", "vorticity", "A", "current")) == [(False, [1]), (True, [1]), (False, [8]), (True, [4])]
    assert O._frame_runs(("vorticity", "divergence", "u", "v", "potential_vorticity", "current")) == [(True, [1, 2]), (False, [1, 2]), (True, [8]), (True, [4])]
    with pytest.raises(E, match="one of u v h A s B_x B_y \\(velocities"):
        O._frame_runs(("vorticity", "uu"))
    with pytest.raises(E, match="'dye' is a tracer"):
        O._frame_runs(("vorticity", "dye"), tracers=("dye",))
    with pytest.raises(E, match="'vorticity' is a tracer"):                    # RESERVED_NAMES is unchanged: a tracer may bear the name
        O._frame_runs(("u", "vorticity"), tracers=("vorticity",))
    assert S.model.RESERVED_NAMES == ("u", "v", "uh", "vh", "h", "A", "s", "B_x", "B_y")

    class Stub:      # what derived_fields and the writer read of a model before the first launch
        tracer_names = ("dye",)
        members = None

        def _join(self):
            raise AssertionError("reached the model: the names were not checked first")
    for names in (("vorticity", "dye"), ("q",), ("u",), ()):
        with pytest.raises(E):
            D.enqueue_derived(Stub(), names)
    for names in (("u", "vorticity", "dye"), ("vorticity", "zeta")):
        with pytest.raises(E):
            O.enqueue_frame(Stub(), names)
        with pytest.raises(E):
            S.FieldTimeSeries(Stub(), names, capacity=4)
    w = S.FieldTimeSeries(Stub(), ("u", "vorticity", "A", "current"), schedule=S.IterationInterval(3), capacity=2)
    assert len(w) == 0 and w.names == ("u", "vorticity", "A", "current")
    g = S.RectilinearGrid(size=(8, 6), x=(0, 1), y=(0, 1))

    class Shaped:
        grid, members = g, 3
    assert O.frame_shape(Shaped, ("u", "vorticity", "current")) == (3, 3, 6, 8)
    for cls in (S.ShallowWaterModel, S.ShallowWaterEnsemble, S.BoundedShallowWaterEnsemble):
        assert callable(cls.derived_fields)


HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# the flags swmhd_amd/csrc/Makefile compiles derived.o with (STRICT)
STRICT_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"]


def test_derived_kernels_use_no_scratch_and_no_lds(tmp_path):
    """All twelve instantiations (model type x frame type x {one grid, ensemble, ensemble with the table}) report ScratchSize 0 and no LDS."""
    out = subprocess.run([HIPCC, *STRICT_FLAGS, "--offload-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                          os.path.join(ROOT, "swmhd_amd", "csrc", "derived.hip"), "-o", str(tmp_path / "d.o")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    res = {}
    for block in re.split(r"remark: [^\n]*Function Name: ", out.stderr)[1:]:
        name = block.split("\n")[0].split(" ")[0]
        num = lambda what: int(re.search(what + r": (\d+)", block).group(1))
        res[name] = (num(r"ScratchSize \[bytes/lane\]"), num(r"LDS Size \[bytes/block\]"), num(r"Occupancy \[waves/SIMD\]"), num(r" VGPRs"))
    kernels = {n: v for n, v in res.items() if "k_derived_fields" in n}
    assert len(kernels) == 12, sorted(res)
    print("waves per SIMD, VGPRs:", {n: v[2:] for n, v in kernels.items()})      # (reported: register allocation is the compiler's)
    assert all(v[0] == 0 and v[1] == 0 for v in kernels.values()), kernels


def test_makefile_builds_derived_strict():
    mk = open(os.path.join(ROOT, "swmhd_amd", "csrc", "Makefile")).read()
    assert re.search(r"^derived\.o: FAST := \$\(STRICT\)$", mk, flags=re.M) and re.search(r"^OBJS \+= derived\.o$", mk, flags=re.M)
    assert re.search(r"^HDRS\s*:=.*include/swmhd_derived\.h", mk, flags=re.M)


def test_launch_plan_under_the_host_sanitizers(tmp_path):
    """tests/derived_plan_check.cpp as a stand-alone host program built with the address and undefined-behaviour sanitizers, host code
    only (nothing here is compiled for or run on a device): every chunk of every row has one thread, nothing is planned without rows
    or members, 2^31 workgroups and more are refused, no arithmetic on the way overflows."""
    exe = str(tmp_path / "derived_plan_check")
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(HIPCC)))
    cc = subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined", "-static-libsan", "-fno-sanitize-recover=all",
                         "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + os.path.join(ROOT, "swmhd_amd", "csrc"),
                         os.path.join(ROOT, "tests", "derived_plan_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "derived plans OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    r = subprocess.run([exe, "plan", "64", "64", "256", "4096", "4096", "1", "5", "0", "1"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    assert [l.split() for l in r.stdout.splitlines()] == [
        "plan 64 64 256 16 1024 4 256 0 0".split(), "plan 4096 4096 1 1024 4194304 16384 1 0 0".split(), "plan 5 0 1 0 0 0 0 1 0".split()]
