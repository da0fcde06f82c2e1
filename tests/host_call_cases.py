"""Scenarios of test_host_calls_gpu.py: what the Python host layer asks of libswmhd.so, call by call.

A `_Recorder` in the place of `model._L` logs every entry point of the library that a model or an ensemble calls, with its arguments:
ints as they are, floats as float.hex(), None as "null", the stream (the last argument of every launching entry point) and the byref
out-argument as the words "stream" and "out", a host array of floats (the gradient values of a halo fill) as its values, and every device
pointer -- a raw address, an entry of a pointer array, a device table -- as "p<k>", k the order in which that address first appears in the
scenario.  The transcript names no attribute of the Python classes: it pins which buffer plays which role in every call, how many calls
a step makes and in which order, whatever the host code that makes them looks like.

tests/golden/host_calls.json holds the transcripts of the commit BEFORE the host layer was folded into shared helpers (one RK3 operand
schedule, one halo fill, shared set-up helpers).  To record it again, check that commit out, copy this file next to its tests and
run, on a machine with the GPU and the built library,
    python tests/host_call_cases.py [path of the .json, default tests/golden/host_calls.json]
Re-record it only together with a deliberate change of the C calls; a refactor of the host layer must reproduce it unchanged.
The H_ scenarios -- the four per-stage correction launches (Coriolis, the two closures, the forcing), alone, together, on a channel, in
ensembles, and given arguments that leave none -- were recorded the same way from the commit before those launches were folded into
one ordered list (swmhd_amd/corrections.py); the sixteen older scenarios decoded to the same transcripts before and after.

Shapes: 20 x 12 is narrower than one 64-column tile and no multiple of the 16-row tile, and at Ny = 12 >= Hy every wrap and fill branch
is live; 16 x 12 with three members gives the ensemble's fold mapping more than one tile per member in y only.  Larger shapes add no
host path.  Slab models (ring, chain, loopback, p2p) need several threads or ranks and are compared bitwise with the single model by
their own tests.

Temporaries: a scenario keeps every object it gets back alive and hands the ensemble's frame a tensor allocated up front, so that no
address passed to the library is freed and handed out again under another label within a scenario."""
import ctypes as C
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "host_calls.json")
DT = 1e-3
P, B = "Periodic", "Bounded"


class _Recorder:
    """The library handle with every entry point it hands out wrapped to record its name when called -- or, given `describe`,
    [name, argument, ...] with the arguments as describe(function, args) words them."""

    def __init__(self, lib, log, describe=None):
        self._lib, self._log, self._describe = lib, log, describe

    def __getattr__(self, name):
        f = getattr(self._lib, name)

        def call(*a):
            self._log.append(name if self._describe is None else [name] + self._describe(f, a))
            return f(*a)
        return call


class Transcript:
    """The blocks [label, calls] of one scenario; one pointer numbering for all of them."""

    def __init__(self):
        self.blocks, self._calls, self._labels, self.held = [], [], {}, []

    def watch(self, model):
        model._L = _Recorder(model._L, self._calls, self._describe)
        return model

    def do(self, label, fn, *args):
        del self._calls[:]
        self.held.append(fn(*args))
        self.blocks.append([label, list(self._calls)])
        return self.held[-1]

    def _pointer(self, address):
        address = getattr(address, "value", address)
        if not address:
            return "null"
        return self._labels.setdefault(address, f"p{len(self._labels)}")

    def _describe(self, f, args):
        words = []
        for k, (a, t) in enumerate(zip(args, f.argtypes)):
            if t is C.c_void_p and k == len(args) - 1:
                words.append("stream")
            elif a is None:
                words.append("null")
            elif isinstance(a, C.Array) and a._type_ in (C.c_double, C.c_float):
                words.append([float(x).hex() for x in a])
            elif isinstance(a, C.Array):
                words.append([self._pointer(x) for x in a])
            elif t is C.c_void_p:
                words.append(self._pointer(a))
            elif t in (C.c_double, C.c_float):
                words.append(float(a).hex())
            elif type(a).__name__ == "CArgObject":      # ctypes.byref(...)
                words.append("out")
            else:
                words.append(int(a))
        assert len(words) == len(args) == len(f.argtypes)
        return words


# --- initial conditions: smooth, positive h; what they are does not change a call -------------------------------------------------
def _h(X, Y):
    return 1.0 + 0.1 * np.sin(np.pi * X) * np.cos(np.pi * Y / 1.2)


def _u(X, Y):
    return 0.1 * np.sin(np.pi * X)


def _v(X, Y):
    return 0.05 * np.sin(np.pi * Y / 1.2)


def _A(X, Y):
    return 0.02 * np.cos(np.pi * X) * np.sin(np.pi * Y / 1.2)


def _tracer(k):
    return lambda X, Y: np.tanh(Y - 0.6) + 0.1 * k


def _grid(S, Nx, Ny, topo):
    return S.RectilinearGrid(size=(Nx, Ny), x=(0, 0.1 * Nx), y=(0, 0.1 * Ny), topology=(topo[0], topo[1], "Flat"))


def _initial(names, tracers=()):
    ic = dict(zip(names, (_u, _v, _h, _A)))
    if names[0] == "uh":
        ic["uh"], ic["vh"] = (lambda X, Y: _h(X, Y) * _u(X, Y)), (lambda X, Y: _h(X, Y) * _v(X, Y))
    ic.update({n: _tracer(k) for k, n in enumerate(tracers)})
    return ic


def _a_gradient(S, value=-0.05):
    g = S.GradientBoundaryCondition
    return S.FieldBoundaryConditions(north=g(value), south=g(value))


def _model(S, t, topo=(P, P), **kw):
    m = t.watch(S.ShallowWaterModel(_grid(S, 20, 12, topo), **kw))
    t.do("set", lambda: m.set(**_initial(m.names, m.tracer_names)))
    return m


# --- the scenarios ----------------------------------------------------------------------------------------------------------------
def periodic_fast(S, t):
    m = _model(S, t)
    t.do("time_step", m.time_step, DT)
    t.do("time_steps(3)", m.time_steps, 3, DT)
    t.do("diagnostics", m.diagnostics)
    t.do("output_fields", m.output_fields)
    t.do("solution", lambda: m.solution)


def strict_eager_halos(S, t, **kw):
    m = _model(S, t, dtype=torch.float32, strict=True, fuse_halo=False, **kw)
    t.do("time_step", m.time_step, DT)


def unfused(S, t):
    m = _model(S, t, fused=False)
    t.do("time_step", m.time_step, DT)


def bounded(S, t, strict, formulation):
    m = _model(S, t, (P, B), strict=strict, formulation=formulation, boundary_conditions={"A": _a_gradient(S)})
    t.do("time_step", m.time_step, DT)
    t.do("time_steps(2)", m.time_steps, 2, DT)


def tracers(S, t, topo, strict, bcs):
    m = _model(S, t, topo, strict=strict, tracers=("c", "d", "e", "f", "g"), boundary_conditions=bcs)
    t.do("time_step", m.time_step, DT)
    t.do("time_step", m.time_step, DT)
    t.do("solution", lambda: m.solution)


def model_graph(S, t, names):
    m = _model(S, t, tracers=names)
    t.do("capture_graph", m.capture_graph, DT)
    t.do("time_steps(5)", m.time_steps, 5, DT)
    t.do("time_steps(4), roles swapped", m.time_steps, 4, DT)      # one eager step restores the captured roles first
    t.do("time_step", m.time_step, DT)
    t.do("time_steps(4)", m.time_steps, 4, DT)
    t.do("time_steps(2, 2 dt)", m.time_steps, 2, 2 * DT)
    m.synchronize()


def ensemble(S, t, per_member, bounded_y):
    members = 3
    g, dt = ([9.81, 9.0, 10.5], [DT, 0.5 * DT, 0.75 * DT]) if per_member else (9.81, DT)
    grid = _grid(S, 16, 12, (P, B if bounded_y else P))
    if bounded_y:
        bcs = [{"A": _a_gradient(S, v)} for v in (-0.05, 0.0, 0.03)]
        e = S.BoundedShallowWaterEnsemble(grid, members, gravitational_acceleration=g, boundary_conditions=bcs)
    else:
        e = S.ShallowWaterEnsemble(grid, members, gravitational_acceleration=g)
    t.watch(e)
    frame = torch.empty((members, 4, grid.Ny, grid.Nx), dtype=torch.float32, device="cuda")
    t.do("set", lambda: e.set(**_initial(e.names)))
    t.do("time_step", e.time_step, dt)
    t.do("time_steps(3)", e.time_steps, 3, dt)
    if not bounded_y:
        t.do("capture_graph", e.capture_graph, dt)
        t.do("time_steps(5)", e.time_steps, 5, dt)
        t.do("time_steps(4), roles swapped", e.time_steps, 4, dt)
    t.do("diagnostics", e.diagnostics)
    t.do("output_fields", lambda: e.output_fields(out=frame))
    t.do("member(1)", e.member, 1)
    e.synchronize()


# --- the per-stage correction launches: BetaPlane Coriolis, the two closures, the Relaxation forcing ------------------------------
def _mask(X, Y):
    return 0.5 + 0.5 * np.cos(np.pi * X) + 0.0 * Y


def _target(X, Y):
    return 0.1 * np.sin(np.pi * Y / 1.2) + 0.0 * X


def _correction(S, kind):
    """The keyword arguments of a model with the one correction `kind`."""
    if kind == "coriolis":
        return dict(coriolis=S.BetaPlane(f0=1.0, beta=0.5))
    if kind == "diffusion":         # h has no coefficient and A's is 0: the field filter drops two of the four
        return dict(closure=S.ScalarDiffusivity(nu=1e-3, kappa={"A": 0.0, "c": 2e-3}), tracers=("c",))
    if kind == "biharmonic":
        return dict(closure=S.ScalarBiharmonicDiffusivity(nu=1e-6, kappa={"A": 2e-6}))
    # a mask and a target array, a scalar target, and a rate of 0 (that field has no part in the launch)
    return dict(forcing={"u": S.Relaxation(0.5, mask=_mask, target=_target), "h": S.Relaxation(0.2, target=1.0), "A": S.Relaxation(0.0)})


def _all_corrections(S):
    return dict(coriolis=S.BetaPlane(f0=1.0, beta=0.5),
                closure=(S.ScalarDiffusivity(nu=1e-3, kappa={"A": 2e-3, "d": 1e-3}), S.ScalarBiharmonicDiffusivity(nu=1e-6, kappa={"c": 3e-6})),
                forcing={"v": S.Relaxation(0.5, mask=_mask), "h": S.Relaxation(0.2, target=_target), "c": S.Relaxation(0.1, target=0.3)})


def one_correction(S, t, kind, strict):
    m = _model(S, t, strict=strict, **_correction(S, kind))
    t.do("time_step", m.time_step, DT)
    t.do("time_steps(3)", m.time_steps, 3, DT)
    m.synchronize()


def all_corrections(S, t, strict):
    m = _model(S, t, strict=strict, tracers=("c", "d"), **_all_corrections(S))
    t.do("time_step", m.time_step, DT)
    t.do("time_steps(3)", m.time_steps, 3, DT)
    t.do("capture_graph", m.capture_graph, DT)
    t.do("time_steps(5)", m.time_steps, 5, DT)
    m.synchronize()


def channel_corrections(S, t, strict):
    """(Periodic, Bounded): the two corrections a Bounded grid takes."""
    kw = dict(_correction(S, "coriolis"), **_correction(S, "relaxation"))
    m = _model(S, t, (P, B), strict=strict, boundary_conditions={"A": _a_gradient(S)}, **kw)
    t.do("time_step", m.time_step, DT)
    t.do("time_steps(3)", m.time_steps, 3, DT)
    m.synchronize()


def absent_corrections(S, t, given):
    """Arguments that leave no correction: the transcript with them is the transcript without them (test_host_calls_gpu asserts it)."""
    kw = dict(coriolis_f=0.7)
    if given:
        kw = dict(coriolis=S.FPlane(0.7), forcing={},
                  closure=(S.ScalarDiffusivity(nu=0.0, kappa={"A": 0.0}), S.ScalarBiharmonicDiffusivity(nu=0.0, kappa=0.0)))
    m = _model(S, t, **kw)
    t.do("time_step", m.time_step, DT)
    t.do("time_steps(3)", m.time_steps, 3, DT)
    m.synchronize()


def ensemble_corrections(S, t, table, per_member_dt, member_targets, tracers=()):
    """A periodic ensemble with all four corrections.  table: per-member g, so that the ensemble has its parameter table and every
    correction call takes dt from it; without it (scalar g, scalar dt) the calls take a = dt gamma and no table."""
    members = 3
    grid = _grid(S, 16, 12, (P, P))
    dt = [DT, 0.5 * DT, 0.75 * DT] if per_member_dt else DT
    X = np.linspace(0.0, 1.0, grid.Nx)[None, :] + np.zeros((grid.Ny, 1))
    target = np.stack([0.1 * (k + 1) * np.sin(np.pi * X) for k in range(members)]) if member_targets else 0.05
    e = S.ShallowWaterEnsemble(
        grid, members, gravitational_acceleration=[9.81, 9.0, 10.5] if table else 9.81, tracers=tracers,
        coriolis=S.BetaPlane(f0=1.0, beta=[0.5, 0.0, -0.3]),
        closure=(S.ScalarDiffusivity(nu=[1e-3, 2e-3, 0.0], kappa={"A": 1e-3}), S.ScalarBiharmonicDiffusivity(nu=1e-6)),
        forcing={"u": S.Relaxation([0.5, 0.2, 0.1], mask=np.cos(np.pi * X) ** 2, target=target),
                 "h": S.Relaxation([0.2, 0.0, 0.3], target=[1.0, 1.1, 0.9]), "A": S.Relaxation(0.0)})
    t.watch(e)
    t.do("set", lambda: e.set(**_initial(e.names, e.tracer_names)))
    t.do("time_step", e.time_step, dt)
    t.do("time_steps(3)", e.time_steps, 3, dt)
    if not per_member_dt:
        t.do("capture_graph", e.capture_graph, dt)
        t.do("time_steps(4)", e.time_steps, 4, dt)
    e.synchronize()


VI, CONS = "VectorInvariant", "Conservative"
SCENARIOS = {
    "A_periodic_fast": (periodic_fast, {}),
    "B_f32_strict_eager_halos": (strict_eager_halos, {}),
    "B_f32_strict_eager_halos_tile": (strict_eager_halos, dict(kernel="tile")),
    "C_unfused": (unfused, {}),
    "D_bounded_fast_vi": (bounded, dict(strict=False, formulation=VI)),
    "D_bounded_fast_cons": (bounded, dict(strict=False, formulation=CONS)),
    "D_bounded_strict_vi": (bounded, dict(strict=True, formulation=VI)),
    "D_bounded_strict_cons": (bounded, dict(strict=True, formulation=CONS)),
    "E_tracers_periodic_fast": (tracers, dict(topo=(P, P), strict=False, bcs=None)),
    "E_tracers_bounded_strict": (tracers, dict(topo=(P, B), strict=True, bcs="d")),
    "F_graph": (model_graph, dict(names=())),
    "F_graph_two_tracers": (model_graph, dict(names=("c", "d"))),
    "G_ensemble_scalar": (ensemble, dict(per_member=False, bounded_y=False)),
    "G_ensemble_per_member": (ensemble, dict(per_member=True, bounded_y=False)),
    "G_bounded_ensemble_scalar": (ensemble, dict(per_member=False, bounded_y=True)),
    "G_bounded_ensemble_per_member": (ensemble, dict(per_member=True, bounded_y=True)),
    **{f"H_{kind}_{'strict' if strict else 'fast'}": (one_correction, dict(kind=kind, strict=strict))
       for kind in ("coriolis", "diffusion", "biharmonic", "relaxation") for strict in (False, True)},
    "H_all_fast": (all_corrections, dict(strict=False)),
    "H_all_strict": (all_corrections, dict(strict=True)),
    "H_channel_fast": (channel_corrections, dict(strict=False)),
    "H_channel_strict": (channel_corrections, dict(strict=True)),
    "H_absent_given": (absent_corrections, dict(given=True)),
    "H_absent_plain": (absent_corrections, dict(given=False)),
    "H_ensemble_scalar_dt": (ensemble_corrections, dict(table=True, per_member_dt=False, member_targets=False)),
    "H_ensemble_per_member_dt": (ensemble_corrections, dict(table=True, per_member_dt=True, member_targets=True)),
    "H_ensemble_no_table_tracers": (ensemble_corrections, dict(table=False, per_member_dt=False, member_targets=True, tracers=("c",))),
}


def run(S, name):
    """The transcript of scenario `name`: a list of [label, [[entry point, argument, ...], ...]]."""
    fn, kw = SCENARIOS[name]
    kw = dict(kw)
    if kw.get("bcs") == "d":
        kw["bcs"] = {"d": _a_gradient(S)}
    t = Transcript()
    fn(S, t, **kw)
    torch.cuda.synchronize()
    del t.held[:]       # (the recorder of a model refers back to the transcript: without this the models would wait for the cycle collector)
    return t.blocks


# --- the golden file: every distinct call once, the scenarios as indices into that table ------------------------------------------
def encode(transcripts):
    table, index = [], {}
    scenarios = {}
    for name, blocks in transcripts.items():
        scenarios[name] = []
        for label, calls in blocks:
            ids = []
            for c in calls:
                key = json.dumps(c)
                if key not in index:
                    index[key] = len(table)
                    table.append(c)
                ids.append(index[key])
            scenarios[name].append([label, ids])
    return {"calls": table, "scenarios": scenarios}


def load_golden(path=GOLDEN):
    with open(path) as fh:
        z = json.load(fh)
    return {name: [[label, [z["calls"][k] for k in ids]] for label, ids in blocks] for name, blocks in z["scenarios"].items()}


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import swmhd_amd
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    # through JSON once, so that what is written is what a test will read back (lists, not tuples)
    recorded = {name: json.loads(json.dumps(run(swmhd_amd, name))) for name in sorted(SCENARIOS)}
    with open(out, "w") as fh:
        json.dump(encode(recorded), fh, separators=(",", ":"))
        fh.write("\n")
    print(f"{out}: {len(recorded)} scenarios, {sum(len(c) for b in recorded.values() for _, c in b)} calls, {os.path.getsize(out)} bytes")
