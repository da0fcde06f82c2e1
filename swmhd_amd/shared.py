"""Helpers ShallowWaterModel and the ensembles share on the host: formulation codes, boundary-condition checks, gradient rows, the
diagnostics dict, the RK3 schedule, and the tail of a fused RK3 stage (tracers, corrections and buffer swaps).  Nothing here touches a
device itself."""
from . import _lib
from .grid import FieldBoundaryConditions

VectorInvariantFormulation, ConservativeFormulation = "VectorInvariant", "Conservative"
RK3_GAMMA = (8.0 / 15.0, 5.0 / 12.0, 3.0 / 4.0)
RK3_ZETA = (0.0, -17.0 / 60.0, -5.0 / 12.0)
RK3_ANCHOR_WEIGHT = 0.25    # gamma1 + zeta2 = 8/15 - 17/60


def rk3_stage(stage, anchor):
    """(gamma, zeta, store_G, anchor) of RK3 stage 0, 1 or 2 -- the schedule of the C step drivers (common.hpp Rk3Buffers).
    anchor (fast builds, periodic grids): gamma1 + zeta2 = 1/4 and zeta3 = -gamma2 make the step exactly U1 = U0 + dt gamma1 G0,
    W = U0 + (dt/4) G0, U2 = W + dt gamma2 G1, U3 = W + dt gamma3 G2 -- one stored operand W, 96 B/cell in every stage
    (swmhd.h SWMHD_RK3_ANCHOR; zeta is the weight of W in the first stage).  Otherwise the classic G- form."""
    if anchor:
        return RK3_GAMMA[stage], RK3_ANCHOR_WEIGHT if stage == 0 else 0.0, 0, True
    return RK3_GAMMA[stage], RK3_ZETA[stage], 1 if stage < 2 else 0, False


def formulation_codes(formulation, lorentz_forcing):
    """(form_code, lorentz_code, names of the four prognostic fields); the forcing is the one that goes with the formulation in the
    reference (SWMHD_example.jl:30-31, divergence_sw_mhd.jl:28-29)."""
    vi = formulation == VectorInvariantFormulation
    lorentz = _lib.LORENTZ_NONE if not lorentz_forcing else (_lib.LORENTZ_JACOBIAN if vi else _lib.LORENTZ_DIVERGENCE)
    return (_lib.VECTOR_INVARIANT if vi else _lib.CONSERVATIVE), lorentz, (("u", "v") if vi else ("uh", "vh")) + ("h", "A")


def check_boundary_conditions(boundary_conditions, bounded, names=None):
    """SwmhdError for a boundary condition on a Periodic side (bounded = (x is Bounded, y is Bounded)); with `names`, also for an
    entry that is not a FieldBoundaryConditions of one of them.  Touches no device."""
    for name, bc in boundary_conditions.items():
        if names is not None and name not in names:
            raise _lib.SwmhdError(f"boundary condition for {name!r}: the fields are {names}")
        if names is not None and not isinstance(bc, FieldBoundaryConditions):
            raise _lib.SwmhdError(f"boundary condition for {name!r}: a FieldBoundaryConditions, not {type(bc).__name__}")
        sides = [(bc.west, 0), (bc.east, 0), (bc.south, 1), (bc.north, 1)]
        if any(b is not None and not bounded[d] for b, d in sides):
            raise _lib.SwmhdError(f"boundary condition on a Periodic side of {name} (Oceananigans rejects it as well)")


def gradient_values(boundary_conditions, names):
    """One row (west, east, south, north) of GradientBoundaryCondition values for each name, NaN = the default boundary condition."""
    bcs = [boundary_conditions.get(n) for n in names]
    return [bc.gradients() if bc is not None else [float("nan")] * 4 for bc in bcs]


def diagnostics_dict(v):
    """The 7 values of swmhd_diagnostics_* (KE, ME, PE, max|u|, max|v|, max|A|, min h) by name, with their total energy."""
    return dict(kinetic_energy=v[0], magnetic_energy=v[1], potential_energy=v[2], total_energy=v[0] + v[1] + v[2],
                max_abs_u=v[3], max_abs_v=v[4], max_abs_A=v[5], min_h=v[6])


def correction_operand(stage, anchor, dt):
    """(has_operand, w, flag) of a per-stage correction launch (corrections.Correction.launch) of RK3 stage `stage`: whether the
    stage stores an operand for later stages that the correction must reach too, with which weight, and the flag that says what the
    weight means.  Classic form: the tendency Gn, weight 1, where the stage stores it.  Anchor form: the anchor W in Gn at stage 0,
    weight dt / 4 -- with dt None (an ensemble's table) the weight 1/4 of dt, and the kernel forms dt_m / 4 (SWMHD_RK3_ANCHOR, which
    only the ensemble calls take)."""
    store = rk3_stage(stage, anchor)[2]
    if anchor and stage == 0:
        return True, RK3_ANCHOR_WEIGHT if dt is None else dt * RK3_ANCHOR_WEIGHT, _lib.RK3_ANCHOR
    if not anchor and store:
        return True, 1.0, 0
    return False, 0.0, 0


def finish_stage(o, dt, stage, fused=True, step_dt=None):
    """What follows the state's launch of RK3 stage `stage` of `o` (a ShallowWaterModel or a ShallowWaterEnsemble), before its halo
    fill: the tracers through the same stage in one launch (o._tracer_stage), advected by the state the stage STARTED from -- still
    o._state here -- then the correction launches of o._corrections on that same state, each correcting what the launches before it
    have written, in the order of the list (corrections.correction_list states it: it decides the last bits) -- then the particles'
    launch on that state (o.particles, where the object has them) -- then the pointer swaps: the new tracers and the new state become current, and G- <- Gn for both (store_tendencies!, 0 bytes).  fused=False: the
    state was advanced in place by a substep, only its G sets swap.  step_dt: with dt None (an ensemble's table), the one dt all members
    share, or None where they differ; handed to the corrections that ask for it (needs_step_dt), every other entry is called as launch(o, dt, stage)."""
    if o._tr:
        o._tracer_stage(dt, stage)
    for c in o._corrections:
        if getattr(c, "needs_step_dt", False):
            c.launch(o, dt, stage, step_dt)
        else:
            c.launch(o, dt, stage)
    # Lagrangian particles (swmhd_amd.particles): one launch, advected by the state the stage STARTED from -- still o._state here
    if getattr(o, "particles", None) is not None:
        o.particles.launch(o, dt, stage)
    if o._tr:
        o._tr, o._tr_alt = o._tr_alt, o._tr
        o._tGn, o._tGm = o._tGm, o._tGn
    if fused:
        o._state, o._alt = o._alt, o._state
    o.Gn, o.Gm = o.Gm, o.Gn


def fill_groups(names):
    """The tracer names in groups of at most four: the limit of one halo-fill call."""
    return [names[k:k + 4] for k in range(0, len(names), 4)]
