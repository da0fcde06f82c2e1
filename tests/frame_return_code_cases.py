"""Cases of the return-code test in tests/test_frame_return_codes_cpu.py: which code wins when a call of swmhd_[ensemble_]derived_fields
[_params]_*, swmhd_[ensemble_]zonal_spectra_* or swmhd_[ensemble_]spectra2d_* carries one argument defect, or two.

The matrix is built as tests/zonal_return_code_cases.py builds that of the zonal means, and with its labels where the argument is the
same: a valid baseline call on an 8 x 8 grid with halo 3 and a row stride of 14 (pointers: small host buffers), then, in this order,
    every single defect;  every pair of defects that do not set the same argument (flag defects are OR-ed);
    the empty valid call (j0 == j1), which returns before any launch, and that call with every single defect on top.
swmhd_spectra2d_* takes no row range and has no empty valid call (a call without fields or members is an argument error), so its
matrix ends with the pairs.  The defects hold all three answers: SWMHD_EINVAL, SWMHD_EHALO (with the wrap flag of the OTHER direction
for every family, and of the SAME direction for the derived frames, whose reach does not depend on the flags) and, for the spectra,
SWMHD_ENOTSUP (a size that is no power of two).  A pair may cancel one of its defects (Nx = 6 makes a stride of 13 long enough): the
other one still answers, and the recording says with what.
This module stands alone.  The entry points are those of _lib.DERIVED_EXPORTS, _lib.SPECTRA_EXPORTS and _lib.SPECTRA2D_EXPORTS that
launch (the names that end in _f64 / _f32); the test holds that every one of them has cases here and recorded answers.

Without a device a call that reaches HIP answers -100, so every case here returns before the first HIP call.
tests/golden/frame_return_codes.json holds the answers of the library before the checks of these calls were gathered in
csrc/api_args.hpp, one string of digits per entry point.  To record it again, on a machine WITHOUT a GPU run
    SWMHD_LIBRARY=/path/to/libswmhd.so python tests/frame_return_code_cases.py [path of the .json]
The recorder fails, rather than drop the case, when a defect case answers 0 or a negative code, when an empty case answers anything
but 0, or when the baseline does not get past its checks.  Re-record only together with a deliberate change of a return code."""
import ctypes as C
import itertools
import json
import math
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frame_return_codes.json")
FLOAT = {"f64": C.c_double, "f32": C.c_float}
STRICT, WRAP_X, WRAP_Y, BOUNDED_X, BOUNDED_Y, UNKNOWN = 1, 16, 32, 256, 512, 1 << 20
MAX_MEMBERS = 65535

GRID = "Nx Ny Hx Hy sy"
ENS = "members stride_m"
DRV_OUT = "j0 j1 which out elem osy osf"
SIGNATURES = {
    "derived_fields": f"q1 q2 h A {GRID} dx dy formulation fcor {DRV_OUT} flags stream",
    "ensemble_derived_fields": f"q1 q2 h A {ENS} {GRID} dx dy formulation fcor {DRV_OUT} osm flags stream",
    "ensemble_derived_fields_params": f"q1 q2 h A {ENS} {GRID} dx dy formulation params {DRV_OUT} osm flags stream",
    "zonal_spectra": f"q1 q2 h A {GRID} dx dy formulation j0 j1 which workspace out osk flags stream",
    "ensemble_zonal_spectra": f"q1 q2 h A {ENS} {GRID} dx dy formulation j0 j1 which workspace out osk osm flags stream",
    "spectra2d": f"q1 q2 h A {GRID} dx dy formulation which wx wy workspace out_shell oss out_2d o2kx o2f flags stream",
    "ensemble_spectra2d": f"q1 q2 h A {ENS} {GRID} dx dy formulation which wx wy workspace out_shell oss osm out_2d o2kx o2f o2m flags stream",
}
POINTERS = ("q1", "q2", "h", "A", "params", "workspace", "out", "out_shell", "out_2d")
COMMON = dict(Nx=8, Ny=8, Hx=3, Hy=3, sy=14, dx=1.0, dy=1.0, formulation=1, fcor=0.5, j0=0, j1=8, which=3, flags=0, stream=None, members=2,
              stride_m=14 * 14)
# two fields of 8 rows of 8 elements; two spectra of Nx/2 + 1 = 5 entries; two of NS = 7 shells and two half-planes of 5 x 8 modes
BASE = {"derived": dict(COMMON, elem=8, osy=8, osf=64, osm=128), "spectra": dict(COMMON, osk=5, osm=10),
        "spectra2d": dict(COMMON, wx=1.0, wy=1.0, oss=7, osm=14, o2kx=8, o2f=40, o2m=80)}


def family(name):
    return "derived" if "derived" in name else ("spectra2d" if "spectra2d" in name else "spectra")


def defects(name):
    """[(label, {argument: value})] of entry point `name`, in a fixed order (labels: those of zonal_return_code_cases.defects)."""
    args, fam = SIGNATURES[name].split(), family(name)
    ens = "members" in args
    d = [(f"{a} null", {a: None}) for a in args if a in POINTERS and a not in ("out_shell", "out_2d")]
    if fam == "spectra2d":
        d.append(("out_shell and out_2d null", dict(out_shell=None, out_2d=None)))
    d += [("Nx = 0", dict(Nx=0)), ("sy one short", dict(sy=13)), ("dx = 0", dict(dx=0.0)), ("dx = NaN", dict(dx=math.nan))]
    if "j1" in args:
        d.append(("rows beyond Ny", dict(j1=9)))
    d += [("unknown flag", dict(flags=UNKNOWN)), ("BOUNDED_X | WRAP_X", dict(flags=BOUNDED_X | WRAP_X)),
          (f"flags {STRICT}", dict(flags=STRICT)), (f"flags {BOUNDED_Y}", dict(flags=BOUNDED_Y)),
          ("Hx = 0", dict(Hx=0)), ("Hx = 0 under WRAP_Y", dict(Hx=0, flags=WRAP_Y)), ("formulation 5", dict(formulation=5))]
    if fam == "derived":
        d.append(("Hx = 0 under WRAP_X", dict(Hx=0, flags=WRAP_X)))
    if ens:
        d += [("members = 0", dict(members=0)), ("members above the maximum", dict(members=MAX_MEMBERS + 1)),
              ("stride_m one short", dict(stride_m=14 * 14 - 1))]
    d += [("which = 0", dict(which=0)), ("unknown field bit", dict(which=16 if fam == "derived" else 128))]
    if fam == "derived":
        d += [("out_elem_size 3", dict(elem=3)), ("out_stride_y one short", dict(osy=7)), ("out_stride_f one short", dict(osf=63))]
        if ens:
            d.append(("out_stride_m one short", dict(osm=127)))
    elif fam == "spectra":
        d += [("out_stride_k one short", dict(osk=4)), ("Nx = 6", dict(Nx=6))]
        if ens:
            d.append(("out_stride_m one short", dict(osm=9)))
    else:
        d += [("wx = 0", dict(wx=0.0)), ("wx = NaN", dict(wx=math.nan)), ("wy = inf", dict(wy=math.inf)),
              ("out_stride_s one short", dict(oss=6)), ("out2_stride_kx one short", dict(o2kx=7)), ("out2_stride_f one short", dict(o2f=39)),
              ("Nx = 6", dict(Nx=6)), ("Ny = 6", dict(Ny=6))]
        if ens:
            d += [("out_stride_m one short", dict(osm=13)), ("out2_stride_m one short", dict(o2m=79))]
    return d


EMPTY = ("j0 == j1", dict(j0=4, j1=4))


def _merge(*changes):
    """One dict of argument changes, or None where two of them set the same argument (flags apart: they are OR-ed)."""
    out = {}
    for ch in changes:
        for k, v in ch.items():
            if k == "flags":
                out[k] = out.get(k, 0) | v
            elif k in out:
                return None
            else:
                out[k] = v
    return out


def cases(name):
    """[(kind, label, changes)] of entry point `name`: kind 'defect' (answer > 0), 'empty' (answer 0) or 'empty+defect' (answer >= 0)."""
    d, out = defects(name), []
    out += [("defect", lab, ch) for lab, ch in d]
    for (la, a), (lb, b) in itertools.combinations(d, 2):
        m = _merge(a, b)
        if m is not None:
            out.append(("defect", f"{la} + {lb}", m))
    if "j0" not in SIGNATURES[name].split():
        return out
    le, e = EMPTY
    out.append(("empty", le, e))
    for la, a in d:
        m = _merge(e, a)
        if m is not None:
            out.append(("empty+defect", f"{le} + {la}", m))
    return out


_BUFFERS = {}


def _pointer(sfx, label):
    if (sfx, label) not in _BUFFERS:
        _BUFFERS[(sfx, label)] = (FLOAT[sfx] * 64)() if label in ("q1", "q2", "h", "A", "params") else (C.c_double * 64)()
    return C.cast(_BUFFERS[(sfx, label)], C.c_void_p)


def entries():
    """[(key, symbol, name, sfx)] of every entry point of the matrix; key = the symbol's name without 'swmhd_'."""
    return [(f"{name}_{sfx}", f"swmhd_{name}_{sfx}", name, sfx) for name in SIGNATURES for sfx in ("f64", "f32")]


def call(L, sym, name, sfx, changes):
    fn = getattr(L, sym)
    names = SIGNATURES[name].split()
    assert len(names) == len(fn.argtypes), (sym, len(names), len(fn.argtypes))
    v = dict(BASE[family(name)], **{a: _pointer(sfx, a) for a in POINTERS})
    v.update(changes)
    return fn(*[v[a] for a in names])


def run(L, key_sym_name_sfx):
    """The answers of one entry point's matrix, as a string of digits; anything outside 0..9 is an error of the case, not a code."""
    _, sym, name, sfx = key_sym_name_sfx
    digits = []
    for kind, label, ch in cases(name):
        rc = call(L, sym, name, sfx, ch)
        ok = rc > 0 if kind == "defect" else (rc == 0 if kind == "empty" else rc >= 0)
        if not ok or rc > 9:
            raise AssertionError(f"{sym}: {kind} case '{label}' answered {rc}")
        digits.append(str(rc))
    return "".join(digits)


def launching(_lib):
    """The entry points of the three export lists that launch"""
    return {s for s in _lib.DERIVED_EXPORTS + _lib.SPECTRA_EXPORTS + _lib.SPECTRA2D_EXPORTS if s.endswith(("_f64", "_f32"))}


def load_golden(path=GOLDEN):
    with open(path) as fh:
        return json.load(fh)


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from swmhd_amd import _lib
    L = _lib.lib()
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    missing = sorted(launching(_lib) - {sym for _, sym, _, _ in entries()})
    assert not missing, f"entry points without cases: {missing}"
    recorded = {}
    for e in entries():
        _, sym, name, sfx = e
        rc = call(L, sym, name, sfx, {})      # the baseline gets past every check: it reaches HIP (no device: -100)
        assert rc == -100, f"{sym}: the baseline call answered {rc}"
        recorded[e[0]] = run(L, e)
    with open(out, "w") as fh:
        json.dump(recorded, fh, separators=(",", ":"), sort_keys=True)
        fh.write("\n")
    print(f"{out}: {len(recorded)} entry points, {sum(len(v) for v in recorded.values())} cases, {os.path.getsize(out)} bytes")
