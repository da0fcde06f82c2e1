"""Cases of test_return_codes_cpu.py: which return code wins when a call into libswmhd.so carries one argument defect, or two.

For every launching entry point of `_lib.EXPORTS`, in f64 and f32, a valid baseline call on an 8 x 8 grid with halo 3 and a row stride
of 14 (pointers: small host buffers, every role its own), and a list of defects, each a change of one or a few arguments that makes
the call invalid whatever the other arguments are.  The matrix of an entry point, in this order:
    every single defect;  every pair of defects that do not set the same argument;
    the "empty" valid calls that return before any launch (nsteps = 0; j0 == j1 where the entry returns before its launcher), and
    each of them with every single defect on top (a driver that runs no stage checks little: those answers may be 0).
Flag defects are OR-ed into the call's flags, so a pair of them is both bits at once; "flags!" replaces the flags.
The ring calls always get a null ring: it is refused, but only after the flag checks of swmhd_ring_step_rk3_bc.
swmhd_rk3_substep and the diagnostics have a row range but hand an empty one to their launcher, so they have no empty case here.

Without a device a call that reaches HIP answers -100, so every case here returns before the first HIP call, and the matrix runs in
well under a second.  tests/golden/return_codes.json holds the answers of the commit BEFORE the argument checks and the flag decoding
of the C host layer were gathered in csrc/api_args.hpp, one string of digits per entry point.  To record it again, build the library
of the commit whose answers are wanted, and on a machine WITHOUT a GPU run
    SWMHD_LIBRARY=/path/to/that/libswmhd.so python tests/return_code_cases.py [path of the .json]
The recorder fails, rather than drop the case, when a defect case answers 0 or a negative code, when an empty case answers anything
but 0, or when a baseline (ring calls apart) does not get past its checks.  Re-record only together with a deliberate change of a
return code."""
import ctypes as C
import itertools
import json
import math
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "return_codes.json")
FLOAT = {"f64": C.c_double, "f32": C.c_float}

STRICT, TILE, MARCH, WRAP_X, WRAP_Y, LEAVE_ROOM = 1, 2, 4, 16, 32, 64
BOUNDED_X, BOUNDED_Y, GM_PREV, ANCHOR, OPEN_SOUTH, OPEN_NORTH = 256, 512, 1024, 2048, 4096, 8192
UNKNOWN = 1 << 20
MAX_MEMBERS = 65535


def P(label):
    return ("P", label)


def Arr(label, n=4, null=None):
    """An array of n pointers to the buffers (label, 0 .. n-1); entry `null` is a null pointer."""
    return ("A", label, n, null)


GRID = "Nx Ny Hx Hy sy"
STEP = f"q q_alt Ga Gb {GRID} dx dy g fcor formulation lorentz dt nsteps flags state_in_alt stream"
ENS = "members stride_m " + GRID
SIGNATURES = {
    "lorentz_jacobian": f"A h Fx Fy {GRID} dx dy flags stream",
    "lorentz_jacobian_rows": f"A h Fx Fy {GRID} dx dy j0 j1 flags stream",
    "lorentz_divergence": f"A h Fx Fy {GRID} dx dy flags stream",
    "lorentz_divergence_rows": f"A h Fx Fy {GRID} dx dy topo_x topo_y j0 j1 flags stream",
    "fill_halo_periodic": f"f1 {GRID} which stream",
    "fill_halo": f"f nf {GRID} topo_x topo_y face_x face_y gradient dx dy stream",
    "fill_halo_walls": f"f nf {GRID} topo_x walls_y face_x face_y gradient dx dy stream",
    "fill_halo_periodic_multi": f"f nf {GRID} which stream",
    "tendencies": f"q1 q2 h A G1 G2 Gh GA {GRID} dx dy g fcor formulation lorentz j0 j1 flags stream",
    "tendencies_rk3": f"q qnew Gn Gm {GRID} dx dy g fcor formulation lorentz dt gamma zeta store_G j0 j1 flags stream",
    "rk3_substep": f"U Gn Gm {GRID} dt gamma zeta j0 j1 flags stream",
    "tracers_rk3": f"q1 q2 h c cnew tGn tGm K {GRID} dx dy formulation dt gamma zeta store_G j0 j1 flags stream",
    "step_rk3": STEP,
    "diagnostics": f"q1 q2 h A {GRID} dx dy g href formulation j0 j1 ws out stream",
    "output_fields": f"q1 q2 h A {GRID} dx dy formulation j0 j1 owhich out elem osy osf flags stream",
    "ensemble_tendencies_rk3": f"q qnew Gn Gm {ENS} dx dy g fcor formulation lorentz dt gamma zeta store_G flags stream",
    "ensemble_tendencies_rk3_params": f"q qnew Gn Gm {ENS} dx dy params formulation lorentz gamma zeta store_G flags stream",
    "ensemble_step_rk3": f"q q_alt Ga Gb {ENS} dx dy g fcor formulation lorentz dt nsteps flags state_in_alt stream",
    "ensemble_step_rk3_params": f"q q_alt Ga Gb {ENS} dx dy params formulation lorentz nsteps flags state_in_alt stream",
    "ensemble_step_rk3_bc": f"q q_alt Ga Gb {ENS} dx dy g fcor formulation lorentz dt nsteps gradient flags state_in_alt stream",
    "ensemble_step_rk3_bc_params": f"q q_alt Ga Gb {ENS} dx dy params formulation lorentz nsteps gradient flags state_in_alt stream",
    "ensemble_fill_halo_periodic": f"f nf {ENS} which stream",
    "ensemble_fill_halo": f"f nf {ENS} topo_x topo_y face_x face_y gradient dx dy stream",
    "ensemble_diagnostics": f"q1 q2 h A {ENS} dx dy g href formulation ws out stream",
    "ensemble_diagnostics_params": f"q1 q2 h A {ENS} dx dy params href formulation ws out stream",
    "ensemble_tracers_rk3": f"q1 q2 h c cnew tGn tGm K {ENS} dx dy formulation dt gamma zeta store_G flags stream",
    "ensemble_tracers_rk3_params": f"q1 q2 h c cnew tGn tGm K {ENS} dx dy formulation params gamma zeta store_G flags stream",
    "ensemble_output_fields": f"q1 q2 h A {ENS} dx dy formulation j0 j1 owhich out elem osy osf osm flags stream",
    "ring_exchange_y": f"ring f nf {GRID} stream",
    "ring_exchange_y_sides": f"ring f nf {GRID} sides stream",
    "ring_step_rk3": "ring " + STEP,
    "ring_step_rk3_bc": f"ring q q_alt Ga Gb {GRID} dx dy g fcor formulation lorentz dt nsteps gradient flags state_in_alt stream",
    "tendency_launch_geometry": "Nx rows formulation elem flags geo_out",
}
UNTYPED = ("tendency_launch_geometry",)     # one symbol, no _f64 / _f32

BASE = dict(
    Nx=8, Ny=8, Hx=3, Hy=3, sy=14, dx=1.0, dy=1.0, g=9.81, fcor=1.0, href=1.0, formulation=1, lorentz=1, dt=0.01, gamma=8.0 / 15.0, zeta=0.0,
    store_G=1, j0=0, j1=8, flags=0, stream=None, state_in_alt=None, ring=None, gradient=None, members=2, stride_m=14 * 14, nsteps=1, nf=4,
    which=3, topo_x=0, topo_y=0, face_x=1, face_y=2, walls_y=3, sides=3, K=2, owhich=3, elem=8, osy=8, osf=64, osm=128, rows=8,
    A=P("A"), h=P("h"), Fx=P("Fx"), Fy=P("Fy"), f1=P("f1"), q1=P("q1"), q2=P("q2"), G1=P("G1"), G2=P("G2"), Gh=P("Gh"), GA=P("GA"),
    ws=P("ws"), out=P("out"), params=P("params"), geo_out=P("geo_out"),
    q=Arr("q"), qnew=Arr("qnew"), q_alt=Arr("qnew"), Gn=Arr("Gn"), Ga=Arr("Gn"), Gb=Arr("Gb"), Gm=None, f=Arr("f"), U=Arr("U"),
    c=Arr("c", 9, 8), cnew=Arr("cnew", 9, 8), tGn=Arr("tGn", 9, 8), tGm=None,      # nine entries, the ninth null: K = 9 must be refused unread
)
BASE_FLAGS = {"ensemble_step_rk3_bc": BOUNDED_Y, "ensemble_step_rk3_bc_params": BOUNDED_Y, "ring_step_rk3_bc": BOUNDED_Y}

# pointers whose null is a defect on its own, pointer arrays (null entry: index 1, inside nf = 4 and K = 2), and the read state a new state may not alias
NEEDED = "A h Fx Fy f1 q1 q2 G1 G2 Gh GA ws out q qnew q_alt Gn Ga Gb f U c tGn geo_out".split()
ARRAYS = dict(q=4, qnew=4, q_alt=4, Gn=4, Ga=4, Gb=4, Gm=4, f=4, U=4, c=9, cnew=9, tGn=9, tGm=9)
ALIAS = dict(qnew=Arr("q"), q_alt=Arr("q"), cnew=Arr("c", 9, 8))

PERIODIC_ENS = ("ensemble_tendencies_rk3", "ensemble_tendencies_rk3_params", "ensemble_step_rk3", "ensemble_step_rk3_params")
BC_ENS = ("ensemble_step_rk3_bc", "ensemble_step_rk3_bc_params")
TRACERS = ("tracers_rk3", "ensemble_tracers_rk3", "ensemble_tracers_rk3_params")
# flag sets an entry knows and refuses (SWMHD_ENOTSUP, or SWMHD_EINVAL where the operand the flag speaks of is missing)
UNSUPPORTED = {
    "tendencies": (BOUNDED_X | MARCH, BOUNDED_Y | MARCH, GM_PREV, ANCHOR, OPEN_SOUTH),
    "tendencies_rk3": (BOUNDED_X | MARCH, BOUNDED_Y | MARCH, GM_PREV | STRICT, ANCHOR | BOUNDED_Y, ANCHOR | GM_PREV, OPEN_SOUTH),
    "step_rk3": (BOUNDED_X, BOUNDED_Y, GM_PREV, OPEN_NORTH),
    "ring_step_rk3": (BOUNDED_X, BOUNDED_Y, WRAP_Y),
    "ring_step_rk3_bc": (MARCH, GM_PREV, ANCHOR, WRAP_Y, OPEN_SOUTH, LEAVE_ROOM),
    "tracers_rk3": (MARCH, GM_PREV, OPEN_SOUTH, OPEN_NORTH, LEAVE_ROOM, ANCHOR | BOUNDED_X),
    "ensemble_tracers_rk3": (MARCH, GM_PREV, OPEN_SOUTH, OPEN_NORTH, LEAVE_ROOM, BOUNDED_X, BOUNDED_Y),
    "ensemble_tracers_rk3_params": (MARCH, GM_PREV, OPEN_SOUTH, OPEN_NORTH, LEAVE_ROOM, BOUNDED_X, BOUNDED_Y),
    "rk3_substep": (TILE, WRAP_X),
    "output_fields": (STRICT, BOUNDED_Y),
    "ensemble_output_fields": (STRICT, BOUNDED_Y),
}
for _n in ("lorentz_jacobian", "lorentz_jacobian_rows", "lorentz_divergence", "lorentz_divergence_rows"):
    UNSUPPORTED[_n] = (WRAP_X, BOUNDED_X, LEAVE_ROOM)
for _n in PERIODIC_ENS:
    UNSUPPORTED[_n] = (BOUNDED_X, BOUNDED_Y, MARCH, GM_PREV, LEAVE_ROOM, OPEN_SOUTH)
for _n in BC_ENS:
    UNSUPPORTED[_n] = (MARCH, GM_PREV, LEAVE_ROOM, ANCHOR, OPEN_NORTH)
# entries with the WENO stencil (halo 3), with the one-cell stencils (halo 1), and those that wrap a period on read
HALO3 = ("lorentz_divergence", "lorentz_divergence_rows", "tendencies", "tendencies_rk3", "step_rk3") + PERIODIC_ENS + BC_ENS + TRACERS
HALO1 = ("diagnostics", "ensemble_diagnostics", "ensemble_diagnostics_params", "output_fields", "ensemble_output_fields")
WRAPS = ("tendencies", "tendencies_rk3", "step_rk3") + PERIODIC_ENS + BC_ENS + TRACERS
FILLS = ("fill_halo_periodic", "fill_halo_periodic_multi", "ensemble_fill_halo_periodic", "fill_halo", "fill_halo_walls", "ensemble_fill_halo")
ANCHOR_STRICT = ("tendencies", "tendencies_rk3", "step_rk3") + PERIODIC_ENS + TRACERS


def defects(name):
    """[(label, {argument: value})] of entry point `name`, in a fixed order."""
    args = SIGNATURES[name].split()
    d = []
    if name.startswith("ring_"):
        d.append(("null ring", {}))
    for a in args:
        if a in NEEDED:
            d.append((f"{a} null", {a: None}))
        if a in ARRAYS:
            d.append((f"{a}[1] null", {a: Arr(BASE[a][1] if BASE[a] else a, ARRAYS[a], 1)}))
        if a in ALIAS:
            d.append((f"{a} aliases the state read", {a: ALIAS[a]}))
    if "Nx" in args:
        d.append(("Nx = 0", dict(Nx=0)))
    if "sy" in args:
        d.append(("sy one short", dict(sy=13)))
    if "dx" in args:
        d += [("dx = 0", dict(dx=0.0)), ("dx = NaN", dict(dx=math.nan))]
    if "j1" in args:
        d.append(("rows beyond Ny", dict(j1=9)))
    if "flags" in args and name not in UNTYPED:
        d += [("unknown flag", dict(flags=UNKNOWN)), ("BOUNDED_X | WRAP_X", dict(flags=BOUNDED_X | WRAP_X))]
        d += [(f"flags {fl}", dict(flags=fl)) for fl in UNSUPPORTED.get(name, ())]
        if name in ANCHOR_STRICT:
            d.append(("ANCHOR | STRICT", dict(flags=ANCHOR | STRICT)))
        if name in BASE_FLAGS:
            d.append(("no Bounded direction", {"flags!": 0}))
    if name in HALO3:
        d.append(("Hx = 2", dict(Hx=2)))
    if name.startswith("lorentz_jacobian"):
        d.append(("Hx = 1", dict(Hx=1)))
    if name in HALO1:
        d.append(("Hx = 0", dict(Hx=0)))
    if name in ("fill_halo", "ensemble_fill_halo"):
        d.append(("wall without a halo line", dict(topo_x=1, Hx=0)))
    if name == "fill_halo_walls":
        d.append(("wall without a halo line", dict(Hy=0)))
    if name in WRAPS:
        d.append(("period shorter than the halo", dict(Nx=2, flags=WRAP_X)))
    if name in FILLS:
        d.append(("period shorter than the halo", dict(Nx=2)))
    if "formulation" in args:
        d.append(("formulation 5", dict(formulation=5)))
    if "lorentz" in args:
        d.append(("forcing of the other formulation", dict(lorentz=2)))
    if "members" in args:
        d += [("members = 0", dict(members=0)), ("members above the maximum", dict(members=MAX_MEMBERS + 1)),
              ("stride_m one short", dict(stride_m=14 * 14 - 1))]
    if "params" in args:
        d.append(("params null", dict(params=None)))
    if "nf" in args and not name.startswith("ring_"):
        d.append(("nf = 5", dict(nf=5)))
    if "which" in args:
        d.append(("which = 4", dict(which=4)))
    if "topo_x" in args:
        d.append(("topology code 5", dict(topo_x=5)))
    if "walls_y" in args:
        d.append(("walls_y = 4", dict(walls_y=4)))
    if "K" in args:
        d += [("K = 0", dict(K=0)), ("K = 9", dict(K=9)), ("no cnew, store_G = 0", dict(cnew=None, store_G=0)),
              ("no cnew, anchor form", dict(cnew=None, flags=ANCHOR))]
    if "nsteps" in args:
        d.append(("nsteps = -1", dict(nsteps=-1)))
    if "owhich" in args:
        d += [("which = 0", dict(owhich=0)), ("element size 3", dict(elem=3)), ("out_stride_y < Nx", dict(osy=7))]
    if "osm" in args:
        d.append(("out_stride_m one short", dict(osm=127)))
    if name == "tendency_launch_geometry":
        d += [("rows = 0", dict(rows=0)), ("element size 3", dict(elem=3))]
    return d


# entries that return 0 for an empty row range before their launcher is called
EMPTY_ROWS = ("lorentz_jacobian_rows", "lorentz_divergence_rows", "tendencies", "tendencies_rk3", "tracers_rk3", "output_fields",
              "ensemble_output_fields")


def empties(name):
    e = []
    if "nsteps" in SIGNATURES[name].split() and not name.startswith("ring_"):
        e.append(("nsteps = 0", dict(nsteps=0)))
    if name in EMPTY_ROWS:
        e.append(("j0 == j1", dict(j0=4, j1=4)))
    return e


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
    for le, e in empties(name):
        out.append(("empty", le, e))
        for la, a in d:
            m = _merge(e, a)
            if m is not None:
                out.append(("empty+defect", f"{le} + {la}", m))
    return out


_BUFFERS = {}


def _pointer(sfx, label, k=0):
    key = (sfx, label, k)
    if key not in _BUFFERS:
        _BUFFERS[key] = (C.c_int * 8)() if label == "geo_out" else (FLOAT[sfx] * 64)()
    return C.cast(_BUFFERS[key], C.c_void_p)


def _value(v, sfx, argtype):
    if isinstance(v, tuple) and v[0] == "P":
        p = _pointer(sfx, v[1])
        return C.cast(p, argtype) if argtype is not C.c_void_p else p
    if isinstance(v, tuple) and v[0] == "A":
        _, label, n, null = v
        return (C.c_void_p * n)(*[None if k == null else _pointer(sfx, label, k) for k in range(n)])
    return v


def entries():
    """[(key, symbol, name, sfx)] of every entry point of the matrix; key = the symbol's name without 'swmhd_'."""
    out = []
    for name in SIGNATURES:
        for sfx in (("f64",) if name in UNTYPED else ("f64", "f32")):
            sym = f"swmhd_{name}" + ("" if name in UNTYPED else f"_{sfx}")
            out.append((sym[len("swmhd_"):], sym, name, sfx))
    return out


def call(L, sym, name, sfx, changes):
    fn = getattr(L, sym)
    names = SIGNATURES[name].split()
    assert len(names) == len(fn.argtypes), (sym, len(names), len(fn.argtypes))
    v = dict(BASE, flags=BASE_FLAGS.get(name, 0))
    if "flags!" in changes:
        v["flags"] = changes["flags!"]
    for k, x in changes.items():
        if k == "flags":
            v["flags"] |= x
        elif k != "flags!":
            v[k] = x
    return fn(*[_value(v[a], sfx, t) for a, t in zip(names, fn.argtypes)])


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
    launching = [s for s in _lib.EXPORTS if s.endswith(("_f64", "_f32"))] + ["swmhd_tendency_launch_geometry"]
    missing = sorted(set(launching) - {sym for _, sym, _, _ in entries()})
    assert not missing, f"launching entry points without cases: {missing}"
    recorded = {}
    for e in entries():
        _, sym, name, sfx = e
        if not name.startswith("ring_"):      # the baseline gets past every check: it reaches HIP (no device: -100) or, with nothing to launch, answers 0
            rc = call(L, sym, name, sfx, {})
            assert rc in (0, -100), f"{sym}: the baseline call answered {rc}"
        recorded[e[0]] = run(L, e)
    with open(out, "w") as fh:
        json.dump(recorded, fh, separators=(",", ":"), sort_keys=True)
        fh.write("\n")
    print(f"{out}: {len(recorded)} entry points, {sum(len(v) for v in recorded.values())} cases, {os.path.getsize(out)} bytes")
