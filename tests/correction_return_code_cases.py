"""Cases of the return-code test in tests/test_correction_return_codes_cpu.py: which code wins when a call of one of the four per-stage
correction launches -- swmhd_[ensemble_]coriolis_rk3_*, swmhd_[ensemble_]diffusion_rk3_*, swmhd_[ensemble_]biharmonic_rk3_*,
swmhd_[ensemble_]relaxation_rk3_* -- carries one argument defect, or two.

The matrix is built as tests/frame_return_code_cases.py builds its own: a valid baseline call on an 8 x 8 grid with halo 3 and a row
stride of 14 (pointers: small host buffers; two fields for the calls that take a list of them), then, in this order,
    every single defect;  every pair of defects that do not set the same argument (flag defects are OR-ed);
    the empty valid call (j0 == j1), which returns before any launch, and that call with every single defect on top.
A defect that sets an entry of a pointer array or of a host table sets that whole argument.  The defects hold all three answers:
SWMHD_EINVAL, SWMHD_ENOTSUP and SWMHD_EHALO.

Not every change in the list is an error to every entry point: the relaxation calls read no halo and take Hx = 0, a wrapped direction
needs no halo in any of them, a negative scalar target is a target like another, and the ensemble calls do not look at their device
tables of coefficients, rates and targets.  Such a change is marked `sure = False` for that entry point; it is in the matrix because
its place in a pair says where the checks it passes stand among the others.  Alone, or paired with another of its kind, it must get
past every check ("L": the call reached HIP, which answers -100 without a device).  A pair with one of them in it may answer either
way -- Hx = 0 also makes a stride of 13 long enough -- and the recording says which.
This module stands alone.  The entry points are those of _lib.CORIOLIS_EXPORTS, DIFFUSION_EXPORTS, BIHARMONIC_EXPORTS and
RELAXATION_EXPORTS (all sixteen launch); the test holds that every one of them has cases here and recorded answers.

Without a device a call that reaches HIP answers -100, so every case here returns before the first HIP call or fails in it at once.
tests/golden/correction_return_codes.json holds the answers of the library before the checks of these calls were gathered in shared
helpers, one string per entry point, one character per case.  To record it again, on a machine WITHOUT a GPU run
    SWMHD_LIBRARY=/path/to/libswmhd.so python tests/correction_return_code_cases.py [path of the .json]
The recorder fails, rather than drop the case, when a sure defect (or a pair of them) answers 0 or a negative code, when an empty case
answers anything but 0, when another case answers 0 or a negative code other than -100, or when the baseline does not get past its
checks.  Re-record only together with a deliberate change of a return code."""
import ctypes as C
import itertools
import json
import math
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "correction_return_codes.json")
FLOAT = {"f64": C.c_double, "f32": C.c_float}
STRICT, TILE, MARCH, WRAP_X, WRAP_Y, LEAVE_ROOM, BOUNDED_X, BOUNDED_Y = 1, 2, 4, 16, 32, 64, 256, 512
GM_IS_PREV_STATE, OPEN_SOUTH, OPEN_NORTH, UNKNOWN = 1024, 4096, 8192, 1 << 20
MAX_MEMBERS = 65535
MAX_FIELDS = {"diffusion": 11, "biharmonic": 11, "relaxation": 12}      # SWMHD_DIFFUSION_MAX_FIELDS, SWMHD_RELAXATION_MAX_FIELDS
NO_DEVICE = -100

GRID = "Nx Ny Hx Hy sy"
ENS = "members stride_m"
TAIL = "a w j0 j1 flags stream"
SIGNATURES = {
    "coriolis_rk3": f"q1 q2 n1 n2 a1 a2 frow {GRID} {TAIL}",
    "ensemble_coriolis_rk3": f"q1 q2 n1 n2 a1 a2 frow {ENS} {GRID} params {TAIL}",
    "diffusion_rk3": f"old nw acc coef nfields {GRID} dx dy {TAIL}",
    "ensemble_diffusion_rk3": f"old nw acc coef nfields {ENS} {GRID} dx dy params {TAIL}",
    "biharmonic_rk3": f"old nw acc coef nfields {GRID} dx dy {TAIL}",
    "ensemble_biharmonic_rk3": f"old nw acc coef nfields {ENS} {GRID} dx dy params {TAIL}",
    "relaxation_rk3": f"old nw acc mask target rate tval nfields {GRID} {TAIL}",
    "ensemble_relaxation_rk3": f"old nw acc mask target rate tval nfields {ENS} mask_sm target_sm {GRID} params {TAIL}",
}
ARRAYS = ("old", "nw", "acc", "mask", "target")       # host arrays of pointers: a tuple of buffer labels (None: a null entry)
TABLES = ("coef", "rate", "tval")                     # host arrays of values (the ensemble calls: device tables, never read)
POINTERS = ("q1", "q2", "n1", "n2", "a1", "a2", "frow", "params")
SM = 14 * 14
COMMON = dict(Nx=8, Ny=8, Hx=3, Hy=3, sy=14, dx=1.0, dy=1.0, a=0.01, w=1.0, j0=0, j1=8, flags=0, stream=None, members=2, stride_m=SM,
              mask_sm=SM, target_sm=SM, nfields=2, coef=(1e-3, 2e-3), rate=(0.5, 0.2), tval=(0.0, 1.0),
              **{a: a for a in POINTERS}, **{a: (a + "0", a + "1") for a in ARRAYS})


def family(name):
    return name.replace("ensemble_", "").replace("_rk3", "")


def _set(seq, k, value):
    return seq[:k] + (value,) + seq[k + 1:]


def defects(name):
    """[(label, {argument: value}, sure)] of entry point `name`, in a fixed order; sure: an error to this entry point whatever else
    the call holds that is no error (see the module's docstring)."""
    args, fam = SIGNATURES[name].split(), family(name)
    ens, B = "members" in args, COMMON
    d = []
    add = lambda label, sure=True, **ch: d.append((label, ch, sure))
    notsup = [TILE, MARCH, GM_IS_PREV_STATE, OPEN_SOUTH, OPEN_NORTH, LEAVE_ROOM]
    if fam == "coriolis":
        for a in ("q1", "q2", "n1", "n2", "frow"):
            add(f"{a} null", **{a: None})
        add("a1 without a2", a2=None, acc_pair=1)      # (acc_pair: no argument; it keeps the two, which together are a valid call,
        add("a2 without a1", a1=None, acc_pair=1)      # from being paired)
        for out, src in (("n1", "q1"), ("n2", "q1"), ("n1", "q2"), ("a1", "q1"), ("a2", "q2"), ("n2", "n1"), ("a1", "n1"), ("a2", "n2"), ("a2", "a1")):
            add(f"{out} = {src}", **{out: src})
    else:
        tables = ("coef",) if fam != "relaxation" else ("rate", "tval")
        for a in ("old", "nw") + tables:
            add(f"{a} null", **{a: None})
        for a in ("old", "nw"):
            for k in (0, 1):
                add(f"{a}[{k}] null", **{a: _set(B[a], k, None)})
        add("nfields = 0", nfields=0)
        add("nfields above the maximum", nfields=MAX_FIELDS[fam] + 1)
        inputs = ("old",) if fam != "relaxation" else ("old", "mask", "target")
        for k, src in ((0, "old0"), (0, "old1"), (1, "nw0")):
            add(f"nw[{k}] = {src}", nw=_set(B["nw"], k, src))
        for k, src in ((0, "nw0"), (0, "nw1"), (0, "old0"), (1, "old0"), (1, "acc0")):
            add(f"acc[{k}] = {src}", acc=_set(B["acc"], k, src))
        for a in inputs[1:]:
            add(f"nw[0] = {a}[1]", nw=_set(B["nw"], 0, a + "1"))
            add(f"nw[1] = {a}[1]", nw=_set(B["nw"], 1, a + "1"))
            add(f"acc[0] = {a}[0]", acc=_set(B["acc"], 0, a + "0"))
            add(f"acc[1] = {a}[0]", acc=_set(B["acc"], 1, a + "0"))
        for a in tables:      # (the ensemble calls take device tables and do not look at them)
            add(f"{a}[1] negative", sure=not ens and a != "tval", **{a: _set(B[a], 1, -1.0)})
            add(f"{a}[0] NaN", sure=not ens, **{a: _set(B[a], 0, math.nan)})
    add("a NaN", a=math.nan)
    add("w NaN", w=math.nan)
    add("Nx = 0", Nx=0)
    add("sy one short", sy=13)
    add("rows beyond Ny", j1=9)
    if "dx" in args:
        add("dx = 0", dx=0.0)
    add("unknown flag", flags=UNKNOWN)
    for fl in notsup + ([BOUNDED_X, BOUNDED_Y] if fam in ("diffusion", "biharmonic") else []):
        add(f"flags {fl}", flags=fl)
    add("BOUNDED_X | WRAP_X", flags=BOUNDED_X | WRAP_X)
    add("Hx = 0", sure=fam != "relaxation", Hx=0)
    add("Hx = 0 under WRAP_X", sure=False, Hx=0, flags=WRAP_X)
    add("Hy = 0 under WRAP_X", sure=fam != "relaxation", Hy=0, flags=WRAP_X)
    if fam == "biharmonic":
        add("Hx = 1", Hx=1)
    if ens:
        add("members = 0", members=0)
        add("members above the maximum", members=MAX_MEMBERS + 1)
        add("stride_m one short", stride_m=SM - 1)
        if fam == "relaxation":
            add("mask stride_m one short", mask_sm=SM - 1)
            add("target stride_m one short", target_sm=SM - 1)
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
    """[(kind, label, changes)] of entry point `name`.  kind: 'defect' (answer > 0), 'accepted' (the call reaches HIP), 'open' (either
    of the two), 'empty' (answer 0) or 'empty+defect' (answer >= 0)."""
    d, out = defects(name), []
    out += [("defect" if sure else "accepted", lab, ch) for lab, ch, sure in d]
    for (la, a, sa), (lb, b, sb) in itertools.combinations(d, 2):
        m = _merge(a, b)
        if m is not None:
            out.append(("defect" if sa and sb else ("open" if sa or sb else "accepted"), f"{la} + {lb}", m))
    le, e = EMPTY
    out.append(("empty", le, e))
    for la, a, _ in d:
        m = _merge(e, a)
        if m is not None:
            out.append(("empty+defect", f"{le} + {la}", m))
    return out


_BUFFERS = {}


def _pointer(sfx, label):
    if label is None:
        return None
    if (sfx, label) not in _BUFFERS:
        _BUFFERS[(sfx, label)] = (FLOAT[sfx] * 64)()
    return C.cast(_BUFFERS[(sfx, label)], C.c_void_p)


def _argument(sfx, name, value, width):
    """`value` as the entry point takes it.  The arrays are `width` long (the largest nfields of the matrix), filled up with buffers of
    their own and with 0: no check reads past nfields entries, and none would leave the array if it did."""
    if value is None:
        return None
    if name in ARRAYS:
        labels = value + tuple(f"{name}{k}" for k in range(len(value), width))
        return (C.c_void_p * width)(*[getattr(_pointer(sfx, lab), "value", None) for lab in labels])
    if name in TABLES:
        return (FLOAT[sfx] * width)(*value)
    return _pointer(sfx, value) if name in POINTERS else value


def entries():
    """[(key, symbol, name, sfx)] of every entry point of the matrix; key = the symbol's name without 'swmhd_'."""
    return [(f"{name}_{sfx}", f"swmhd_{name}_{sfx}", name, sfx) for name in SIGNATURES for sfx in ("f64", "f32")]


def call(L, sym, name, sfx, changes):
    fn = getattr(L, sym)
    names = SIGNATURES[name].split()
    assert len(names) == len(fn.argtypes), (sym, len(names), len(fn.argtypes))
    v = dict(COMMON, **changes)
    width = MAX_FIELDS.get(family(name), 0) + 1
    return fn(*[_argument(sfx, a, v[a], width) for a in names])


def run(L, key_sym_name_sfx):
    """The answers of one entry point's matrix, one character per case: the code, or 'L' for a call that reached HIP; anything else is
    an error of the case, not a code."""
    _, sym, name, sfx = key_sym_name_sfx
    chars = []
    for kind, label, ch in cases(name):
        rc = call(L, sym, name, sfx, ch)
        ok = {"defect": rc > 0, "accepted": rc == NO_DEVICE, "open": rc > 0 or rc == NO_DEVICE, "empty": rc == 0, "empty+defect": rc >= 0}[kind]
        if not ok or rc > 9:
            raise AssertionError(f"{sym}: {kind} case '{label}' answered {rc}")
        chars.append("L" if rc == NO_DEVICE else str(rc))
    return "".join(chars)


def launching(_lib):
    """The entry points of the four export lists (every one of them launches)"""
    return set(_lib.CORIOLIS_EXPORTS + _lib.DIFFUSION_EXPORTS + _lib.BIHARMONIC_EXPORTS + _lib.RELAXATION_EXPORTS)


def load_golden(path=GOLDEN):
    with open(path) as fh:
        return json.load(fh)


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from swmhd_amd import _lib
    L = _lib.lib()
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    missing = sorted(launching(_lib) ^ {sym for _, sym, _, _ in entries()})
    assert not missing, f"entry points without cases, or cases without entry points: {missing}"
    recorded = {}
    for e in entries():
        _, sym, name, sfx = e
        rc = call(L, sym, name, sfx, {})      # the baseline gets past every check: it reaches HIP (no device: -100)
        assert rc == NO_DEVICE, f"{sym}: the baseline call answered {rc}"
        recorded[e[0]] = run(L, e)
    with open(out, "w") as fh:
        json.dump(recorded, fh, separators=(",", ":"), sort_keys=True)
        fh.write("\n")
    print(f"{out}: {len(recorded)} entry points, {sum(len(v) for v in recorded.values())} cases, {os.path.getsize(out)} bytes")
