"""CPU tests (no GPU) of the output-frame entry points (swmhd_output_fields_*, swmhd_ensemble_output_fields_*): declared and exported,
every argument error is returned before any HIP call, and no instantiation of the kernel uses scratch (gfx950 cross-compile)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOAT = {"f64": ctypes.c_double, "f32": ctypes.c_float}
SYMBOLS = [f"swmhd_{e}output_fields_{sfx}" for e in ("", "ensemble_") for sfx in ("f64", "f32")]
EINVAL, EHALO = 1, 2


def test_output_symbols_declared_and_exported(swmhd):
    L = swmhd._lib.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "swmhd.h")).read(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} not declared in include/swmhd.h"
        assert hasattr(L, name), f"{name} not exported by libswmhd.so"
        assert name in swmhd._lib.EXPORTS
    for n, bit in (("U", 1), ("V", 2), ("H", 4), ("A", 8), ("SPEED", 16), ("BX", 32), ("BY", 64)):
        assert re.search(rf"#define SWMHD_OUT_{n} {bit}\b", header)
    assert swmhd._lib.OUT_BITS == {"u": 1, "v": 2, "h": 4, "A": 8, "s": 16, "B_x": 32, "B_y": 64}
    assert L.swmhd_version() == 300          # the additions are additive


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_output_refusals_without_gpu(swmhd, sfx):
    """Each SWMHD_EINVAL / SWMHD_EHALO case returns its code on a machine without a GPU: the checks precede every HIP call."""
    B = swmhd._lib
    L = B.lib()
    buf = (FLOAT[sfx] * 64)()                  # (never dereferenced: every call below is refused first)
    p = ctypes.cast(buf, ctypes.c_void_p)
    Nx = Ny = 8
    H, sy = 3, 14
    f = getattr(L, f"swmhd_output_fields_{sfx}")

    def one(q1=p, A=p, Nx=Nx, Ny=Ny, Hx=H, Hy=H, sy=sy, dx=1.0, form=1, j0=0, j1=Ny, which=1 | 2 | 8 | 16, out=p, elem=4, osy=Nx,
            osf=Nx * Ny, flags=0):
        return f(q1, p, p, A, Nx, Ny, Hx, Hy, sy, dx, 1.0, form, j0, j1, which, out, elem, osy, osf, flags, None)
    assert one(q1=None) == EINVAL and one(A=None) == EINVAL and one(out=None) == EINVAL      # null pointers
    assert one(which=0) == EINVAL                                                          # empty mask
    assert one(which=128) == EINVAL and one(which=1 | 256) == EINVAL and one(which=-1) == EINVAL   # unknown bits
    assert one(elem=2) == EINVAL and one(elem=16) == EINVAL and one(elem=0) == EINVAL      # element size: 4 or 8
    assert one(osy=Nx - 1) == EINVAL                                                        # frame row shorter than Nx
    assert one(osf=Nx * Ny - 1) == EINVAL                                                   # fields would overlap
    assert one(j0=3, j1=6, osf=3 * Nx - 1) == EINVAL                                        # ... for a row range: its own extent
    assert one(j0=-1) == EINVAL and one(j1=Ny + 1) == EINVAL and one(j0=5, j1=4) == EINVAL  # bad rows
    for fl in (B.STRICT, B.TILE_KERNEL, B.BOUNDED_X, B.BOUNDED_Y, B.LEAVE_ROOM, 8, 1 << 20):
        assert one(flags=fl) == EINVAL, fl                                                  # flags: WRAP_X | WRAP_Y only
    assert one(Nx=0) == EINVAL and one(sy=Nx + 2 * H - 1) == EINVAL and one(dx=0.0) == EINVAL and one(form=2) == EINVAL
    assert one(Hx=0) == EHALO and one(Hy=0, flags=B.WRAP_X | B.WRAP_Y) == EHALO             # reach: one cell
    assert one(j0=4, j1=4) == 0 and one(j0=4, j1=4, osf=0, flags=B.WRAP_X | B.WRAP_Y, elem=8) == 0   # an empty row range enqueues nothing

    e = getattr(L, f"swmhd_ensemble_output_fields_{sfx}")
    sm = (Ny + 2 * H) * sy

    def ens(members=2, stride_m=sm, which=1 | 2 | 8 | 16, out=p, elem=4, osy=Nx, osf=Nx * Ny, osm=4 * Nx * Ny, flags=0, Hx=H, j0=0, j1=Ny):
        return e(p, p, p, p, members, stride_m, Nx, Ny, Hx, H, sy, 1.0, 1.0, 1, j0, j1, which, out, elem, osy, osf, osm, flags, None)
    assert ens(members=0) == EINVAL and ens(members=-2) == EINVAL and ens(members=B.ENSEMBLE_MAX_MEMBERS + 1) == EINVAL
    assert ens(stride_m=sm - 1) == EINVAL                                                   # members would overlap
    assert ens(osm=4 * Nx * Ny - 1) == EINVAL                                               # member frames would overlap
    assert ens(which=0) == EINVAL and ens(out=None) == EINVAL and ens(elem=3) == EINVAL and ens(flags=B.STRICT) == EINVAL
    assert ens(osy=Nx - 1) == EINVAL and ens(osf=Nx * Ny - 1) == EINVAL
    assert ens(Hx=0) == EHALO
    assert ens(members=B.ENSEMBLE_MAX_MEMBERS, j0=2, j1=2) == 0                             # valid and empty: nothing is enqueued


HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# the flags swmhd_amd/csrc/Makefile compiles output.o with (STRICT)
STRICT_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"]


def test_output_kernels_use_no_scratch(tmp_path):
    """All eight instantiations (model type x frame type x ensemble) report ScratchSize 0."""
    out = subprocess.run([HIPCC, *STRICT_FLAGS, "--offload-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                          os.path.join(ROOT, "swmhd_amd", "csrc", "output.hip"), "-o", str(tmp_path / "o.o")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    res = {}
    for block in re.split(r"remark: [^\n]*Function Name: ", out.stderr)[1:]:
        name = block.split("\n")[0].split(" ")[0]
        res[name] = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", block).group(1))
    kernels = {n: s for n, s in res.items() if "k_output_fields" in n}
    assert len(kernels) == 8, sorted(res)
    assert all(s == 0 for s in kernels.values()), kernels


def test_makefile_builds_output_strict():
    mk = open(os.path.join(ROOT, "swmhd_amd", "csrc", "Makefile")).read()
    assert re.search(r"^output\.o: FAST := \$\(STRICT\)$", mk, flags=re.M) and re.search(r"^OBJS \+= output\.o$", mk, flags=re.M)
