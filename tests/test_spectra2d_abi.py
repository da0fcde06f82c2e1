"""CPU tests (no GPU) of the 2-D / isotropic spectrum entry points (swmhd_spectra2d_*, swmhd_ensemble_spectra2d_*, swmhd_spectra2d_shells,
swmhd_spectra2d_workspace): declared, exported and listed; every argument error is returned before any HIP call, in the stated order
SWMHD_EINVAL, SWMHD_EHALO, SWMHD_ENOTSUP; a refused call leaves the outputs and the workspace alone; the host mirror refuses Bounded
directions, tracers, unsupported sizes and y-slabs before anything is allocated; no instantiation of the kernels uses scratch (gfx950
cross-compile); and the code shared with the zonal spectra stands once, in spectra_device.inc."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOAT = {"f64": ctypes.c_double, "f32": ctypes.c_float}
LAUNCHING = [f"swmhd_{e}spectra2d_{sfx}" for e in ("", "ensemble_") for sfx in ("f64", "f32")]
SYMBOLS = LAUNCHING + ["swmhd_spectra2d_shells", "swmhd_spectra2d_workspace"]
EINVAL, EHALO, ENOTSUP = 1, 2, 3
NAMES = ("u", "v", "h", "A", "s", "B_x", "B_y")
SENTINEL = -777.25
NAN, INF = float("nan"), float("inf")


def test_spectra2d_symbols_declared_exported_and_listed(swmhd):
    B = swmhd._lib
    L = B.lib()
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    main, header = strip("swmhd.h"), strip("swmhd_spectra2d.h")
    assert re.search(r'^#include "swmhd_spectra2d.h"$', main, flags=re.M)          # swmhd.h brings them along
    declared = sorted(set(re.findall(r"\b(swmhd_[a-z0-9_]+)\s*\(", header)))
    assert declared == sorted(SYMBOLS) == sorted(B.SPECTRA2D_EXPORTS)
    for name in SYMBOLS:
        assert hasattr(L, name), f"{name} declared in include/swmhd_spectra2d.h but not exported by libswmhd.so"
        assert getattr(L, name).argtypes is not None
    assert all(getattr(L, n).restype is ctypes.c_int for n in LAUNCHING)
    assert L.swmhd_spectra2d_workspace.restype is ctypes.c_int64 and L.swmhd_spectra2d_shells.restype is ctypes.c_int
    lists = [set(B.EXPORTS), set(B.ZONAL_EXPORTS), set(B.DERIVED_EXPORTS), set(B.SPECTRA_EXPORTS), set(B.DIFFUSION_EXPORTS), set(B.CORIOLIS_EXPORTS),
             set(B.SPECTRA2D_EXPORTS)]      # disjoint
    assert sum(len(s) for s in lists) == len(set().union(*lists))
    assert not re.findall(r"\bswmhd_[a-z0-9_]*spectra2d[a-z0-9_]*\s*\(", main + strip("swmhd_spectra.h"))      # no other header declares them
    assert "#define" not in header.replace("#define SWMHD_SPECTRA2D_H", "")          # the mask bits are SWMHD_ZS_*: no new ones
    assert L.swmhd_version() == 300          # the additions are additive
    assert "IsotropicSpectrumTimeSeries" in swmhd.__all__
    for cls in (swmhd.ShallowWaterModel, swmhd.ShallowWaterEnsemble, swmhd.BoundedShallowWaterEnsemble):
        assert callable(cls.isotropic_spectra) and callable(cls.power_spectra_2d)


def _callers(swmhd, sfx):
    """(one, ens, bufs, consts): the single and the ensemble call on host buffers of sentinels, every argument a keyword with a valid
    default.  (The buffers are never dereferenced: without a device no call gets as far, and with one only refused calls are made.)"""
    B = swmhd._lib
    L = B.lib()
    buf = (FLOAT[sfx] * 64)()                  # (never dereferenced: every call below is refused first)
    bufs = [(ctypes.c_double * 256)(*([SENTINEL] * 256)) for _ in range(3)]
    p = ctypes.cast(buf, ctypes.c_void_p)
    o, o2, w = (ctypes.c_void_p(ctypes.addressof(b) + 64 * 8) for b in bufs)      # 64 sentinels in front
    Nx = Ny = 8
    H = 3
    NS = L.swmhd_spectra2d_shells(Nx, Ny, 1.0, 1.0)
    assert NS == 7
    f = getattr(L, f"swmhd_spectra2d_{sfx}")

    def one(q1=p, A=p, Nx=Nx, Ny=Ny, Hx=H, Hy=H, sy=None, dx=1.0, dy=1.0, form=1, which=1 | 2 | 8 | 64, wx=1.0, wy=1.0, ws=w, out=o, oss=None,
            out2=o2, o2kx=None, o2f=None, flags=0):
        sy = Nx + 2 * Hx if sy is None else sy
        ns = max(L.swmhd_spectra2d_shells(Nx, Ny, wx, wy), 1)
        o2kx = Ny if o2kx is None else o2kx
        return f(q1, p, p, A, Nx, Ny, Hx, Hy, sy, dx, dy, form, which, wx, wy, ws, out, ns if oss is None else oss, out2, o2kx,
                 (Nx // 2 + 1) * o2kx if o2f is None else o2f, flags, None)

    e = getattr(L, f"swmhd_ensemble_spectra2d_{sfx}")

    def ens(members=2, stride_m=None, Nx=Nx, Ny=Ny, which=1 | 2 | 8 | 64, wx=1.0, ws=w, out=o, oss=None, osm=None, out2=o2, o2m=None, flags=0, Hx=H, q2=p):
        sy = Nx + 2 * Hx
        ns = max(L.swmhd_spectra2d_shells(Nx, Ny, wx, 1.0), 1)
        oss = ns if oss is None else oss
        nf, o2f = bin(which & 127).count("1"), (Nx // 2 + 1) * Ny
        return e(p, q2, p, p, members, (Ny + 2 * H) * sy if stride_m is None else stride_m, Nx, Ny, Hx, H, sy, 1.0, 1.0, 1, which, wx, 1.0, ws, out, oss,
                 nf * oss if osm is None else osm, out2, Ny, o2f, nf * o2f if o2m is None else o2m, flags, None)
    return one, ens, bufs, (B, L, Nx, Ny, H, NS)


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_spectra2d_refusals_without_gpu(swmhd, sfx):
    """Each refusal returns its code on a machine without a GPU (the checks precede every HIP call), in the order SWMHD_EINVAL, SWMHD_EHALO,
    SWMHD_ENOTSUP, and the sentinels in and around the outputs and the workspace are untouched afterwards."""
    one, ens, bufs, (B, L, Nx, Ny, H, NS) = _callers(swmhd, sfx)
    assert one(q1=None) == EINVAL and one(A=None) == EINVAL and one(ws=None) == EINVAL                  # null pointers
    assert one(out=None, out2=None) == EINVAL                                                           # both outputs null
    assert one(Nx=0) == EINVAL and one(Ny=0) == EINVAL and one(sy=Nx + 2 * H - 1) == EINVAL and one(Hx=-1) == EINVAL   # extents
    assert one(dx=0.0) == EINVAL and one(dy=-1.0) == EINVAL and one(dx=NAN) == EINVAL                   # spacing
    assert one(form=2) == EINVAL and one(form=-1) == EINVAL                                             # formulation
    assert one(which=0) == EINVAL and one(which=128) == EINVAL and one(which=1 | (1 << 20)) == EINVAL and one(which=-1) == EINVAL and one(which=8192) == EINVAL
    for fl in (B.STRICT, B.TILE_KERNEL, B.MARCH_KERNEL, B.BOUNDED_X, B.BOUNDED_Y, B.LEAVE_ROOM, B.RK3_ANCHOR, 8, 1 << 20):
        assert one(flags=fl) == EINVAL and one(flags=fl | B.WRAP_X) == EINVAL, fl                       # flags: WRAP_X | WRAP_Y only
    for bad in (0.0, -1.0, NAN, INF, -INF):                                                             # the metric: finite and positive
        assert one(wx=bad) == EINVAL and one(wy=bad) == EINVAL, bad
    # a stride too small for its extent -- of an output that is asked for
    assert one(oss=NS - 1) == EINVAL and one(oss=0) == EINVAL and one(wx=4.0, wy=4.0, oss=11) == EINVAL      # NS follows the metric: 12
    assert one(o2kx=Ny - 1) == EINVAL and one(o2f=5 * Ny - 1) == EINVAL and one(o2kx=Ny + 1, o2f=5 * Ny + 4) == EINVAL
    # reach: one cell, or the WRAP flag of THAT direction
    assert one(Hx=0) == EHALO and one(Hy=0) == EHALO and one(Hx=0, flags=B.WRAP_Y) == EHALO and one(Hy=0, flags=B.WRAP_X) == EHALO
    assert one(Hx=0, Hy=0, flags=B.WRAP_X) == EHALO and one(Hx=0, Hy=0, flags=B.WRAP_Y) == EHALO
    # an argument error outranks the halo
    assert one(Hx=0, q1=None) == EINVAL and one(Hx=0, ws=None) == EINVAL and one(Hx=0, which=0) == EINVAL and one(Hx=0, oss=NS - 1) == EINVAL
    assert one(Hx=0, wx=0.0) == EINVAL and one(Hy=0, flags=B.STRICT) == EINVAL and one(Hx=0, out=None, out2=None) == EINVAL
    # the unsupported sizes, in either direction: after SWMHD_EINVAL and SWMHD_EHALO
    for bad in (3, 6, 2, 8192, 12, 1):
        for kw in (dict(Nx=bad), dict(Ny=bad)):
            assert one(**kw) == ENOTSUP and one(**kw, flags=B.WRAP_X | B.WRAP_Y) == ENOTSUP and one(**kw, out2=None) == ENOTSUP, kw
            assert one(**kw, Hx=0) == EHALO and one(**kw, Hy=0, flags=B.WRAP_X) == EHALO                      # the halo outranks it
            assert one(**kw, Hx=0, Hy=0, flags=B.WRAP_X | B.WRAP_Y) == ENOTSUP
            assert one(**kw, ws=None) == EINVAL and one(**kw, which=0) == EINVAL and one(**kw, wy=NAN) == EINVAL and one(**kw, oss=0) == EINVAL
            assert one(**kw, Hx=0, which=128) == EINVAL and one(**kw, flags=B.STRICT) == EINVAL
    sm = (Ny + 2 * H) * (Nx + 2 * H)
    assert ens(members=0) == EINVAL and ens(members=-2) == EINVAL and ens(members=B.ENSEMBLE_MAX_MEMBERS + 1) == EINVAL
    assert ens(stride_m=sm - 1) == EINVAL                                                   # members would overlap
    assert ens(osm=4 * NS - 1) == EINVAL and ens(which=127, osm=7 * NS - 1) == EINVAL and ens(o2m=4 * 5 * Ny - 1) == EINVAL and ens(o2m=0) == EINVAL
    assert ens(which=0) == EINVAL and ens(out=None, out2=None) == EINVAL and ens(ws=None) == EINVAL and ens(q2=None) == EINVAL
    assert ens(flags=B.STRICT) == EINVAL and ens(oss=NS - 1) == EINVAL and ens(which=128) == EINVAL and ens(wx=-1.0) == EINVAL
    assert ens(Hx=0) == EHALO and ens(Hx=0, members=0) == EINVAL and ens(Hx=0, osm=0) == EINVAL
    for bad in (3, 6, 2, 8192):
        for kw in (dict(Nx=bad), dict(Ny=bad)):
            assert ens(**kw) == ENOTSUP and ens(**kw, Hx=0) == EHALO and ens(**kw, members=0) == EINVAL and ens(**kw, osm=0) == EINVAL
    assert all(v == SENTINEL for b in bufs for v in b)


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_valid_calls_get_past_every_check(swmhd, sfx):
    """Without a device a call that passes every check reaches HIP and fails there (-100, hipErrorNoDevice): the boundary of each
    refusal from its valid side.  Only without a device: with one these calls would launch on host pointers."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("the calls pass host pointers: only without a device")
    one, ens, bufs, (B, L, Nx, Ny, H, NS) = _callers(swmhd, sfx)
    assert one() == -100 and one(out=None) == -100 and one(out2=None) == -100
    assert one(oss=NS - 1, out=None) == -100 and one(oss=NS) == -100                # the stride of an output that is not asked for is not read
    assert one(o2kx=Ny - 1, out2=None) == -100 and one(o2kx=Ny + 1, o2f=5 * Ny + 5) == -100
    assert L.swmhd_spectra2d_shells(Nx, Ny, 4.0, 4.0) == 12 and one(wx=4.0, wy=4.0, oss=12) == -100
    assert one(Hx=0, Hy=0, flags=B.WRAP_X | B.WRAP_Y) == -100 and one(Hx=0, flags=B.WRAP_X) == -100
    for Nx_, Ny_ in ((4, 4), (4, 4096), (4096, 4), (64, 512)):
        assert one(Nx=Nx_, Ny=Ny_) == -100
    assert ens() == -100 and ens(members=B.ENSEMBLE_MAX_MEMBERS) == -100
    assert ens(osm=4 * NS - 1, out=None) == -100 and ens(o2m=4 * 5 * Ny - 1, out2=None) == -100
    assert all(v == SENTINEL for b in bufs for v in b)


def test_host_mirror_refuses_before_any_allocation(swmhd):
    """A Bounded direction (either one), a tracer name, an unknown name, a size that is no power of two (either one) and a y-slab
    decomposition raise SwmhdError while the names and the grid are being read: the stub has no state and no library handle."""
    S = swmhd
    E = S._lib.SwmhdError
    from swmhd_amd import spectra2d as Z

    class Decomp:
        def __init__(self, n):
            self.world_size = n

    class Stub:
        tracer_names = ("dye",)
        members = None

        def __init__(self, Nx, Ny=32, topology=("Periodic", "Periodic", "Flat"), ranks=1, ring=None):
            self.grid = S.RectilinearGrid(size=(Nx, Ny), x=(0, 1), y=(0, 1), topology=topology)
            self.decomp, self._ring = Decomp(ranks), ring

        def _join(self):
            raise AssertionError("reached the model: the refusals were not checked first")

        @property
        def _L(self):
            raise AssertionError("reached the library: the refusals were not checked first")

    PB, BP = ("Periodic", "Bounded", "Flat"), ("Bounded", "Periodic", "Flat")
    for stub, names, what in ((Stub(64), ("u", "dye"), "is a tracer"), (Stub(64), ("q",), "one of"), (Stub(64), (), "no names"),
                              (Stub(64, topology=BP), ("u",), "Bounded"), (Stub(64, topology=PB), ("A",), "Bounded"),
                              (Stub(64, topology=("Bounded", "Bounded", "Flat")), ("A",), "Bounded"),
                              (Stub(48), ("u",), "Nx = 48: a power of two"), (Stub(64, 48), ("u",), "Ny = 48: a power of two"), (Stub(2), ("u",), "power of two"),
                              (Stub(64, 8192), ("u",), "power of two"), (Stub(64, ranks=2), ("u",), "SWMHD_ENOTSUP.*every row"),
                              (Stub(64, ring=object()), ("u",), "SWMHD_ENOTSUP.*every row")):
        for call in (Z.enqueue_isotropic_spectra, Z.enqueue_power_spectra_2d):
            with pytest.raises(E, match=what):
                call(stub, names)
        with pytest.raises(E, match=what):
            S.IsotropicSpectrumTimeSeries(stub, names, capacity=4)
    for cap in (None, 0, -3):
        with pytest.raises(E, match="capacity"):
            S.IsotropicSpectrumTimeSeries(Stub(64), ("u", "B_x"), capacity=cap)
    w = S.IsotropicSpectrumTimeSeries(Stub(64, 4), ("u", "B_x"), schedule=S.IterationInterval(3), capacity=2)
    assert len(w) == 0 and w.capacity == 2 and w.times == [] and w.iterations == [] and w.schedule.steps(0.01) == 3 and w.names == ("u", "B_x")
    assert S.IsotropicSpectrumTimeSeries(Stub(4, 4), capacity=1).names == ("u", "v", "A") and S.IsotropicSpectrumTimeSeries(Stub(4096, 4096), capacity=1).schedule == S.TimeInterval(0.1)
    assert Z.isotropic_shape(Stub(64, 64), ("u", "v")) == (2, 46)


HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# the flags swmhd_amd/csrc/Makefile compiles spectra2d.o with (STRICT)
STRICT_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"]


def test_spectra2d_kernels_use_no_scratch(tmp_path):
    """All eight instantiations of pass 1 (model type x ensemble x threads per row), the three of pass 2 (a wave or a workgroup per column;
    with and without the twiddle table) and pass 3 report ScratchSize 0; passes 1 and 2 take their LDS at launch, pass 3 a fixed 2 KiB;
    two workgroups of passes 1 and 2 fit the registers of a CU (what 80 KiB of LDS each admit)."""
    out = subprocess.run([HIPCC, *STRICT_FLAGS, "--offload-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                          os.path.join(ROOT, "swmhd_amd", "csrc", "spectra2d.hip"), "-o", str(tmp_path / "s.o")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    res = {}
    for block in re.split(r"remark: [^\n]*Function Name: ", out.stderr)[1:]:
        name = block.split("\n")[0].split(" ")[0]
        num = lambda what: int(re.search(what + r": (\d+)", block).group(1))
        res[name] = (num(r"ScratchSize \[bytes/lane\]"), num(r"LDS Size \[bytes/block\]"), num(r"Occupancy \[waves/SIMD\]"))
    rows = {n: v for n, v in res.items() if "k_s2d_rows" in n}
    cols = {n: v for n, v in res.items() if "k_s2d_cols" in n}
    sums = {n: v for n, v in res.items() if "k_s2d_shells" in n}
    assert len(rows) == 8 and len(cols) == 3 and len(sums) == 1 and len(res) == 12, sorted(res)
    print("waves per SIMD:", {n: v[2] for n, v in res.items()})      # (reported: register allocation is the compiler's)
    assert all(v[0] == 0 for v in res.values()), res
    assert all(v[1] == 0 for v in rows.values()) and all(v[1] == 0 for v in cols.values()) and all(v[1] == 16 * 16 * 8 for v in sums.values()), res
    assert all(v[2] >= 2 for v in res.values()), res


def test_makefile_builds_spectra2d_strict_and_the_shared_code_stands_once():
    csrc = os.path.join(ROOT, "swmhd_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^spectra2d\.o: FAST := \$\(STRICT\)$", mk, flags=re.M) and re.search(r"^OBJS \+= spectra2d\.o$", mk, flags=re.M)
    assert "swmhd_spectra2d.h" in re.search(r"^HDRS\s*:=(.*)$", mk, flags=re.M).group(1)
    inc = open(os.path.join(csrc, "spectra_device.inc")).read()
    for src in ("spectra.hip", "spectra2d.hip"):
        text = open(os.path.join(csrc, src)).read()
        assert '#include "spectra_device.inc"' in text
        for stated_once in ("struct alignas(16) cplx", "cplx cmul(", "cplx twiddle(", "double frame_value(", "void dif_stage(", "sincospi("):
            assert stated_once not in text and inc.count(stated_once) == 1, (src, stated_once)
