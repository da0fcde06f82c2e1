"""Cases of the return-code tests in tests/test_zonal_abi.py: which code wins when a call of swmhd_zonal_means_* or
swmhd_ensemble_zonal_means_* carries one argument defect, or two.

The matrix is built as tests/return_code_cases.py builds those of the entry points of include/swmhd.h, and with its labels, so that a
case here and the case of the same label of swmhd_[ensemble_]output_fields_* can be compared: a valid baseline call on an 8 x 8 grid
with halo 3 and a row stride of 14 (pointers: small host buffers), then, in this order,
    every single defect;  every pair of defects that do not set the same argument (flag defects are OR-ed);
    the empty valid call (j0 == j1), which returns before any launch, and that call with every single defect on top.
This module stands alone (it reads nothing of return_code_cases but is laid out like it): the entry points of include/swmhd_zonal.h
are listed in _lib.ZONAL_EXPORTS, and tests/test_zonal_abi.py holds that every name there has cases here and recorded answers.

Without a device a call that reaches HIP answers -100, so every case here returns before the first HIP call.
tests/golden/zonal_return_codes.json holds the answers of the commit that added the entry points, one string of digits per entry
point.  To record it again, on a machine WITHOUT a GPU run
    SWMHD_LIBRARY=/path/to/libswmhd.so python tests/zonal_return_code_cases.py [path of the .json]
The recorder fails, rather than drop the case, when a defect case answers 0 or a negative code, when an empty case answers anything
but 0, or when the baseline does not get past its checks.  Re-record only together with a deliberate change of a return code."""
import ctypes as C
import itertools
import json
import math
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zonal_return_codes.json")
FLOAT = {"f64": C.c_double, "f32": C.c_float}
STRICT, WRAP_X, BOUNDED_X, BOUNDED_Y, UNKNOWN = 1, 16, 256, 512, 1 << 20
MAX_MEMBERS = 65535

GRID = "Nx Ny Hx Hy sy"
SIGNATURES = {
    "zonal_means": f"q1 q2 h A {GRID} dx dy formulation j0 j1 which out osk flags stream",
    "ensemble_zonal_means": f"q1 q2 h A members stride_m {GRID} dx dy formulation j0 j1 which out osk osm flags stream",
}
POINTERS = ("q1", "q2", "h", "A", "out")
BASE = dict(Nx=8, Ny=8, Hx=3, Hy=3, sy=14, dx=1.0, dy=1.0, formulation=1, j0=0, j1=8, which=3, osk=8, osm=16, flags=0, stream=None,
            members=2, stride_m=14 * 14)


def defects(name):
    """[(label, {argument: value})] of entry point `name`, in a fixed order (labels: those of return_code_cases.defects)."""
    ens = "members" in SIGNATURES[name].split()
    d = [(f"{a} null", {a: None}) for a in POINTERS]
    d += [("Nx = 0", dict(Nx=0)), ("sy one short", dict(sy=13)), ("dx = 0", dict(dx=0.0)), ("dx = NaN", dict(dx=math.nan)),
          ("rows beyond Ny", dict(j1=9)),
          ("unknown flag", dict(flags=UNKNOWN)), ("BOUNDED_X | WRAP_X", dict(flags=BOUNDED_X | WRAP_X)),
          (f"flags {STRICT}", dict(flags=STRICT)), (f"flags {BOUNDED_Y}", dict(flags=BOUNDED_Y)),
          ("Hx = 0", dict(Hx=0)), ("formulation 5", dict(formulation=5))]
    if ens:
        d += [("members = 0", dict(members=0)), ("members above the maximum", dict(members=MAX_MEMBERS + 1)),
              ("stride_m one short", dict(stride_m=14 * 14 - 1))]
    d += [("which = 0", dict(which=0)), ("unknown profile bit", dict(which=1 << 14)), ("out_stride_k one short", dict(osk=7))]
    if ens:
        d.append(("out_stride_m one short", dict(osm=15)))
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
        _BUFFERS[(sfx, label)] = (C.c_double * 64)() if label == "out" else (FLOAT[sfx] * 64)()
    return C.cast(_BUFFERS[(sfx, label)], C.c_void_p)


def entries():
    """[(key, symbol, name, sfx)] of every entry point of the matrix; key = the symbol's name without 'swmhd_'."""
    return [(f"{name}_{sfx}", f"swmhd_{name}_{sfx}", name, sfx) for name in SIGNATURES for sfx in ("f64", "f32")]


def call(L, sym, name, sfx, changes):
    fn = getattr(L, sym)
    names = SIGNATURES[name].split()
    assert len(names) == len(fn.argtypes), (sym, len(names), len(fn.argtypes))
    v = dict(BASE, **{a: _pointer(sfx, a) for a in POINTERS})
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


def load_golden(path=GOLDEN):
    with open(path) as fh:
        return json.load(fh)


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from swmhd_amd import _lib
    L = _lib.lib()
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    missing = sorted(set(_lib.ZONAL_EXPORTS) - {sym for _, sym, _, _ in entries()})
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
