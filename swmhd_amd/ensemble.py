"""Ensembles: B independent runs of one periodic grid stepped together on one GPU (swmhd_ensemble_* in include/swmhd.h).

The reference's runs are sweeps of small grids -- 64^2 and 128^2, two formulations, initial conditions that differ in the amplitude of A
(SWMHD_example.jl:11,35-37; divergence_sw_mhd.jl:11,32-34; its twelve energy_plots/*).  A 64^2 grid gives the chip 16 workgroups per
stage; an ensemble of B members gives it 16 B, in the same three launches per RK3 step.  Every member has the grid, formulation, forcing
and precision of the ensemble; members differ in their state and, where sequences are given, in g, f and dt.  Member m of field f is row m of a (members, Ny+2Hy, Nx+2Hx) tensor: the
halo-padded parent a ShallowWaterModel would hold.  `member(m)` hands one member to the single-grid tools (checkpoints, inspection).

BoundedShallowWaterEnsemble does the same for a grid with Bounded directions, each member with its own boundary conditions: the
reference's commented channel experiment (A_bcs = GradientBoundaryCondition(-0.05) north and south, SWMHD_example.jl:18-22,
divergence_sw_mhd.jl:17-21,34) as a sweep over the gradient.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .closure import check_closure, closure_for_member
from .coriolis import check_coriolis, row_table
from .corrections import correction_list, live_fields, member_table, needs_stages
from .fields import _SFX, _stream_ptr
from .forcing import check_bathymetry, check_forcing, check_source, check_stochastic, device_parents, forcing_for_member
from .grid import Center, Face
from .model import ShallowWaterModel, rk3_operands, tracer_names
from .particles import check_particles
from .stochastic import StochasticState
from .shared import (VectorInvariantFormulation, check_boundary_conditions, diagnostics_dict, fill_groups, finish_stage,
                     formulation_codes, gradient_values)

LOCS = ((Face, Center), (Center, Face), (Center, Center), (Center, Center))


def is_per_member(v):
    """True for a sequence (one value per member), False for a scalar."""
    return isinstance(v, (list, tuple)) or np.ndim(v) > 0


def per_member_values(v, members, name):
    """(values, per_member): float64 array of `members` values from a scalar or a sequence of exactly `members` numbers."""
    if not is_per_member(v):
        return np.full(members, float(v)), False
    arr = np.asarray(v, dtype=np.float64)
    if arr.ndim != 1 or arr.shape[0] != members:
        raise _lib.SwmhdError(f"{name}: {arr.size if arr.ndim == 1 else arr.shape} values for {members} members (a scalar or one per member)")
    return arr.copy(), True


class ShallowWaterEnsemble:
    """`members` ShallowWaterModels of one periodic grid in one set of tensors.  Arguments as ShallowWaterModel's; `member_stride`
    (elements, >= (Ny+2Hy)(Nx+2Hx)) pitches the members apart inside one allocation (the gaps are never read or written).
    fuse_halo=False fills every member's halos after each stage instead of reading the periodic images (ShallowWaterModel's option).

    Parameter sweeps: gravitational_acceleration and coriolis_f take a scalar or a sequence of `members` values, and so does the dt of
    time_step, time_steps and capture_graph.  As soon as anything is per member the ensemble holds `parameters`, the (members, 3)
    device table of (g, f, dt) in its dtype, and steps through the swmhd_ensemble_*_params entry points; with scalars everywhere it
    calls exactly what it always called.  `clock_times` has every member's model time; `clock_time` is their common value and raises
    once per-member time steps have made them differ.

    Passive tracers: `tracers=("c", "d")` gives every member those centre fields (ShallowWaterModel's argument, same names and limit),
    laid out like the state.  Such an ensemble steps stage by stage: swmhd_ensemble_tendencies_rk3[_params], then
    swmhd_ensemble_tracers_rk3[_params] on the state the stage started from -- six launches per step for all tracers of all members
    with fused halos -- and its four state fields come out bitwise what the native driver gives the ensemble without tracers.

    Coriolis: `coriolis=BetaPlane(f0=..., beta=...)` (ShallowWaterModel's argument; swmhd_amd.coriolis) with a scalar or one value per
    member for f0 and for beta -- a sweep of beta.  `coriolis_rows` is the (members, 2, Ny) device table of f at the centres and the
    faces of every member's rows; such an ensemble steps stage by stage with one more launch per stage for all members
    (swmhd_ensemble_coriolis_rk3_*), under a scalar or a per-member dt.  FPlane(f) is coriolis_f=f and changes no call.

    Closure: `closure=ScalarDiffusivity(nu=..., kappa=...)` (ShallowWaterModel's argument) with a scalar or one value per member for
    every coefficient -- a sweep of the Reynolds or the magnetic Prandtl number.  `diffusion_coefficients` is the (members, fields
    with a coefficient) device table; such an ensemble steps stage by stage as one with tracers does, with one more launch per stage
    for all members (swmhd_ensemble_diffusion_rk3_*), under a scalar or a per-member dt.  Without a closure, or with coefficients
    that are all 0, the ensemble calls exactly what it calls without the argument.  `closure=ScalarBiharmonicDiffusivity(...)`, or a
    tuple with one of each kind, likewise: `biharmonic_coefficients` is its device table, its launch (swmhd_ensemble_biharmonic_rk3_*)
    follows the Laplacian's.

    Forcing: `forcing={"u": Relaxation(rate, mask, target), ...}` (ShallowWaterModel's argument; swmhd_amd.forcing) with a scalar or one
    value per member for every rate and scalar target, and masks and target arrays of shape (Ny, Nx) for all members or (members, Ny,
    Nx) -- a sweep of the drag; a `Source(value)` takes a scalar per member or an array (members, Ny, Nx), and `bathymetry=` an array
    (Ny, Nx) for all members or (members, Ny, Nx) (one more launch per stage, swmhd_ensemble_source_rk3_*, after the relaxation's).  `relaxation_rates` and `relaxation_targets` are the (members, forced fields) device tables; such an
    ensemble steps stage by stage with one more launch per stage for all members (swmhd_ensemble_relaxation_rk3_*), after the
    closures' launches, under a scalar or a per-member dt.  Without a forcing, or with rates that are all 0, the ensemble calls exactly
    what it calls without the argument."""

    def __init__(self, grid, members, gravitational_acceleration=9.81, coriolis_f=1.0, formulation=VectorInvariantFormulation,
                 lorentz_forcing=True, dtype=torch.float64, strict=False, device="cuda", member_stride=None, decomp=None,
                 fuse_halo=True, tracers=(), closure=None, coriolis=None, forcing=None, bathymetry=None, particles=None):
        self.tracer_names = tracer_names(tracers)      # checked before anything touches a device
        # coriolis = FPlane | BetaPlane | CoriolisProfile (ShallowWaterModel's argument; values may be per member).  None and FPlane: the
        # f of the stage kernels.  Otherwise they get f = 0 and _coriolis holds the parameter whose rows a correction launch adds
        self.coriolis = coriolis
        coriolis_f, self._coriolis = check_coriolis(coriolis, coriolis_f, 1.0)
        self.closure = closure
        coefs, coefs4 = check_closure(closure, formulation_codes(formulation, lorentz_forcing)[2], self.tracer_names,
                                      formulation != VectorInvariantFormulation)      # (a Bounded grid: _check_topology, below)
        if decomp is not None or grid.Ny_global != grid.Ny or grid.j_offset != 0:
            raise _lib.SwmhdError("ShallowWaterEnsemble runs on one GPU: no slab decomposition")
        self._check_topology(grid)
        if torch.device(device).type != "cuda":
            raise _lib.SwmhdError("ShallowWaterEnsemble runs on the GPU only (no CPU fallback)")
        if dtype not in _SFX:
            raise _lib.SwmhdError(f"dtype {dtype}: float64 or float32")
        self.members = int(members)
        if not 1 <= self.members <= _lib.ENSEMBLE_MAX_MEMBERS:
            raise _lib.SwmhdError(f"members = {members}: 1 .. {_lib.ENSEMBLE_MAX_MEMBERS}")
        # checked before anything touches a device
        # the closure's coefficients: a scalar or one value per member each; the fields all of whose values are 0 have no launch
        columns = lambda cs: live_fields({n: per_member_values(c, self.members, f"closure coefficient of {n}")[0] for n, c in (cs or {}).items()})
        self._diffusion, self._biharmonic = columns(coefs), columns(coefs4)
        rows = row_table(self._coriolis, grid, self.members) if self._coriolis is not None else None
        # the forcing: names, shapes, values and refusals, the callables evaluated; the fields all of whose rates are 0 have no launch
        self.forcing = forcing
        relax = check_forcing(forcing, grid, formulation_codes(formulation, lorentz_forcing)[2], self.tracer_names, self.members)
        # its StochasticForcing entries (swmhd_amd.stochastic): a scalar or per-member rate, member m draws with stream + m
        stir = check_stochastic(forcing, grid, formulation_codes(formulation, lorentz_forcing)[2], self.tracer_names, self.members,
                                formulation != VectorInvariantFormulation)
        self.g_values, g_seq = per_member_values(gravitational_acceleration, self.members, "gravitational_acceleration")
        self.f_values, f_seq = per_member_values(coriolis_f, self.members, "coriolis_f")
        # bathymetry (ShallowWaterModel's argument; also (members, Ny, Nx)) and the Source entries of `forcing`: one static field per
        # forced field, per member where b, g or a Source is, else one array for all members
        self.bathymetry = check_bathymetry(bathymetry, grid, self.members)
        sources, self._source_thickness = check_source(forcing, self.bathymetry, grid, formulation_codes(formulation, lorentz_forcing)[2],
                                                       self.tracer_names, self.g_values if g_seq else float(gravitational_acceleration),
                                                       self.members, formulation != VectorInvariantFormulation)
        # particles = LagrangianParticles(x, y, tracked_fields), x and y of shape (P,) or (members, P): refusals and the positions brought
        # into the domain, before anything is allocated
        seeds = check_particles(particles, grid, formulation_codes(formulation, lorentz_forcing)[2], self.tracer_names, self.members)
        self.grid = grid
        self.g = self.g_values if g_seq else float(gravitational_acceleration)
        self.f = self.f_values if f_seq else float(coriolis_f)
        self.formulation, self.strict, self.dtype = formulation, strict, dtype
        self.lorentz_forcing = lorentz_forcing
        self.form_code, self.lorentz_code, self.names = formulation_codes(formulation, lorentz_forcing)
        self.sfx = _SFX[dtype]
        self._flags = _lib.STRICT if strict else _lib.FAST
        # periodic "gather on read", as in ShallowWaterModel: no halo fill between stages, halos filled lazily (_ensure_halos)
        self._rwrap = (_lib.WRAP_X | _lib.WRAP_Y) if (fuse_halo and grid.Nx >= grid.Hx and grid.Ny >= grid.Hy) else 0
        self._halo_stale = False
        Py, Px = grid.parent_shape
        self.stride_m = int(member_stride) if member_stride is not None else Py * Px
        if self.stride_m < Py * Px:
            raise _lib.SwmhdError(f"member_stride {member_stride} < (Ny+2Hy)(Nx+2Hx) = {Py * Px}")

        def mk():
            if self.stride_m == Py * Px:
                return torch.zeros((self.members, Py, Px), dtype=dtype, device=device)
            flat = torch.zeros(self.members * self.stride_m, dtype=dtype, device=device)
            return flat.as_strided((self.members, Py, Px), (self.stride_m, Px, 1))
        self._state, self._alt = [mk() for _ in LOCS], [mk() for _ in LOCS]
        self.Gn, self.Gm = [mk() for _ in LOCS], [mk() for _ in LOCS]
        # tracers: a current and an alternate set and two G sets like the state's, swapped with them stage by stage (finish_stage)
        self._tr, self._tr_alt = {n: mk() for n in self.tracer_names}, {n: mk() for n in self.tracer_names}
        self._tGn, self._tGm = [mk() for _ in self.tracer_names], [mk() for _ in self.tracer_names]
        self._anchor = not strict                      # the stage form of the native driver (common.hpp: Rk3Buffers)
        self.clock_times = np.zeros(self.members)
        self.clock_time, self.iteration = 0.0, 0
        self._L = _lib.lib()
        self.parameters, self._table_dt = None, None
        # (members, fields with a coefficient) on the device, in the ensemble's dtype, fields in the order of the launch: the tables of
        # swmhd_ensemble_diffusion_rk3_* and of swmhd_ensemble_biharmonic_rk3_*
        dev = self._state[0].device
        table = lambda cs: member_table([cs[n] for n in self.names + self.tracer_names if n in cs], dtype, dev) if cs is not None else None
        self.diffusion_coefficients, self.biharmonic_coefficients = table(self._diffusion), table(self._biharmonic)
        # (members, 2, Ny) on the device, in the ensemble's dtype and rounded to it: fc then ff of every member, the table of
        # swmhd_ensemble_coriolis_rk3_*; built once
        self.coriolis_rows = None
        if rows is not None:
            self.coriolis_rows = torch.from_numpy(rows).to(device=dev, dtype=dtype)
        # the forcing on the device: (members, forced fields) tables of rates and scalar targets, and every mask and target array as
        # parents of the fields' shape and pitch -- (Py, Px) shared by all members where none of that kind is per member (member stride
        # 0), else (members, Py, Px) each: the call has one member stride for the masks and one for the targets
        self._relaxation, self.relaxation_rates, self.relaxation_targets = None, None, None
        if relax is not None:
            def parents(arrs):
                per = any(a is not None and a.ndim == 3 for a in arrs)
                arrs = [np.broadcast_to(a, (self.members,) + a.shape[-2:]) if (per and a is not None) else a for a in arrs]
                return [device_parents(grid, a, dtype, dev) for a in arrs], (Py * Px if per else 0)
            masks, self._mask_stride = parents([m for _, _, m, _ in relax])
            targets, self._target_stride = parents([t if np.ndim(t) >= 2 else None for _, _, _, t in relax])
            tvals = [np.zeros(self.members) if np.ndim(t) >= 2 else np.broadcast_to(np.asarray(t, dtype=np.float64), (self.members,))
                     for _, _, _, t in relax]
            self.relaxation_rates = member_table([r for _, r, _, _ in relax], dtype, dev)
            self.relaxation_targets = member_table(tvals, dtype, dev)
            self._relaxation = [(n, m, t) for (n, _, _, _), m, t in zip(relax, masks, targets)]
        # the static sources on the device: parents of the fields' shape and pitch -- (Py, Px) shared by all members where no field is per
        # member (member stride 0), else (members, Py, Px) each: the call has one member stride for the sources
        self._source, self._source_stride = None, 0
        if sources is not None:
            per = any(S.ndim == 3 for _, _, S in sources)
            self._source_stride = Py * Px if per else 0
            self._source = [(n, k, device_parents(grid, np.broadcast_to(S, (self.members,) + S.shape[-2:]) if per else S, dtype, dev))
                            for n, k, S in sources]
        # the stochastic forcing on the device: one step counter and one set of coefficient pairs per member; None where inactive
        self._stochastic = StochasticState(stir, grid, dtype, dev, self.members) if stir is not None else None
        # the correction launches that follow every stage, in their order (finish_stage runs them); empty without any
        self._corrections = correction_list(self, self._state[0].stride(1))
        # the particles of every member on the device: x, y and the stored velocity G-, (members, P) float64 (finish_stage runs their launch)
        self.particles = particles
        if particles is not None:
            particles.bind(self, seeds, dev)
        if g_seq or f_seq:
            self._make_parameters()

    # --- per-member parameters and clocks ------------------------------------------------------------------------
    def _make_parameters(self):
        """The device table (members, 3) of (g, f, dt); the dt column is written by _set_table_dt before the first step."""
        host = np.stack([self.g_values, self.f_values, np.zeros(self.members)], axis=1)
        self.parameters = torch.from_numpy(host).to(device=self._state[0].device, dtype=self.dtype)
        self._table_dt = None
        self._graph = None      # (a graph captured with scalar arguments does not read the table)

    def _dt_values(self, dt):
        """None for a scalar dt on an ensemble without per-member parameters (the scalar entry points), else the dt of every member."""
        if not is_per_member(dt) and self.parameters is None:
            return None
        return per_member_values(dt, self.members, "dt")[0]

    def _set_table_dt(self, dts):
        """Write the dt column of the table (stream-ordered) unless it holds these values already."""
        if self.parameters is None:
            self._make_parameters()
        if self._table_dt is None or not np.array_equal(self._table_dt, dts):
            self.parameters[:, 2].copy_(torch.from_numpy(dts).to(self.dtype))
            self._table_dt = dts.copy()

    @staticmethod
    def _dt_key(dt):
        return tuple(float(x) for x in dt) if is_per_member(dt) else dt

    @property
    def clock_time(self):
        """The model time all members share; SwmhdError once per-member time steps have made their times differ (see clock_times)."""
        if self._clocks_differ:
            raise _lib.SwmhdError("clock_time: the members' times differ after per-member time steps; read clock_times")
        return self._clock_time

    @clock_time.setter
    def clock_time(self, t):
        self._clock_time, self._clocks_differ = t, False
        self.clock_times[:] = t

    def _advance_clock(self, n, dt, dts):
        if dts is None or np.all(dts == dts[0]):
            step = dt if dts is None else (dt if not is_per_member(dt) else float(dts[0]))
            if not self._clocks_differ:
                self._clock_time += n * step
                self.clock_times[:] = self._clock_time
                return
            dts = np.full(self.members, float(step))
        self.clock_times += n * dts
        self._clocks_differ = True

    def _clock_state(self):
        return self._clock_time, self._clocks_differ, self.clock_times.copy()

    def _restore_clock(self, state):
        self._clock_time, self._clocks_differ = state[0], state[1]
        self.clock_times[:] = state[2]

    def _check_topology(self, grid):
        if grid.topo_codes() != (_lib.PERIODIC, _lib.PERIODIC):
            raise _lib.SwmhdError("ShallowWaterEnsemble supports (Periodic, Periodic) grids only (SWMHD_ENOTSUP): use "
                                  "BoundedShallowWaterEnsemble for Bounded grids")

    # --- state ---------------------------------------------------------------------------------------------------
    def set(self, **kw):
        """set!(model, ...) for every member.  Each value: a callable (X, Y) used for every member, a list of `members` callables,
        or an array of shape (members, Ny, Nx) (interiors) or (members, Ny+2Hy, Nx+2Hx) (parents).  Tracers by their names, as A."""
        g = self.grid
        B = self.members
        for k, v in kw.items():
            target, loc = (self._tr[k], (Center, Center)) if k in self._tr else (self._state[self.names.index(k)], LOCS[self.names.index(k)])
            X, Y = g.nodes(loc)
            evaluate = lambda fn: np.asarray(fn(X, Y), dtype=np.float64) + np.zeros(g.parent_shape)
            if callable(v):
                full = np.repeat(evaluate(v)[None], B, axis=0)
            elif isinstance(v, (list, tuple)) and all(callable(fn) for fn in v):
                if len(v) != B:
                    raise ValueError(f"{k}: {len(v)} callables for {B} members")
                full = np.stack([evaluate(fn) for fn in v])
            else:
                arr = np.asarray(v, dtype=np.float64)
                if arr.shape == (B, g.Ny, g.Nx):
                    full = np.zeros((B,) + g.parent_shape)
                    full[(slice(None),) + g.interior] = arr
                elif arr.shape == (B,) + g.parent_shape:
                    full = arr
                else:
                    raise ValueError(f"{k}: shape {arr.shape}, expected ({B}, {g.Ny}, {g.Nx}) or ({B}, {g.parent_shape[0]}, {g.parent_shape[1]})")
            target.copy_(torch.from_numpy(np.ascontiguousarray(full)).to(self.dtype))
        self.update_state()
        return self

    @property
    def fields(self):
        """The four prognostic tensors (members, Ny+2Hy, Nx+2Hx) in the order of `names`, halos current."""
        self._ensure_halos()
        return list(self._state)

    @property
    def solution(self):
        """The prognostic tensors by name (u|uh, v|vh, h, A, then the tracers), halos current."""
        self._ensure_halos()
        return {**dict(zip(self.names, self._state)), **self._tr}

    @property
    def tracers(self):
        """The passive tracers by name, (members, Ny+2Hy, Nx+2Hx) each, halos current."""
        self._ensure_halos()
        return dict(self._tr)

    def _ptrs(self, ts):
        return _lib.ptr_array([t.data_ptr() for t in ts])

    def _ensure_halos(self):
        if self._halo_stale:
            self.update_state()

    def update_state(self):
        """fill_halo_regions! of every member: one launch for all four fields of all members, and one for every four tracers."""
        g = self.grid
        self._halo_stale = False
        f = getattr(self._L, f"swmhd_ensemble_fill_halo_periodic_{self.sfx}")
        for ts in [self._state] + [[self._tr[n] for n in grp] for grp in fill_groups(self.tracer_names)]:
            _lib.check(f(self._ptrs(ts), len(ts), self.members, self.stride_m, g.Nx, g.Ny, g.Hx, g.Hy, self._state[0].stride(1),
                         _lib.HALO_X | _lib.HALO_Y, _stream_ptr()), "swmhd_ensemble_fill_halo_periodic")

    # --- time stepping with tracers: stage by stage, as ShallowWaterModel.time_step (two launches per stage for all members) ----
    def _stage_fused(self, dt, stage):
        """RK3 stage `stage` of the state of every member in one launch (swmhd_ensemble_tendencies_rk3, or _params with dt None): reads
        the current state, writes the alternate set, with the operands the native driver picks (rk3_operands)."""
        g = self.grid
        gamma, zeta, store, anchor_flag, third = rk3_operands(stage, self._anchor, self.Gn, self.Gm)
        head = (self._ptrs(self._state), self._ptrs(self._alt), self._ptrs(self.Gn), self._ptrs(third) if third is not None else None,
                self.members, self.stride_m, g.Nx, g.Ny, g.Hx, g.Hy, self._state[0].stride(1), g.dx, g.dy)
        tail = (gamma, zeta, store, self._flags | self._rwrap | anchor_flag, _stream_ptr())
        if dt is not None:
            f = getattr(self._L, f"swmhd_ensemble_tendencies_rk3_{self.sfx}")
            _lib.check(f(*head, self.g, self.f, self.form_code, self.lorentz_code, dt, *tail), "swmhd_ensemble_tendencies_rk3")
        else:
            f = getattr(self._L, f"swmhd_ensemble_tendencies_rk3_params_{self.sfx}")
            _lib.check(f(*head, self.parameters.data_ptr(), self.form_code, self.lorentz_code, *tail), "swmhd_ensemble_tendencies_rk3_params")

    def _tracer_stage(self, dt, stage):
        """All tracers of all members through RK3 stage `stage` in one launch (swmhd_ensemble_tracers_rk3, or _params with dt None),
        advected by the state the stage started from: after _stage_fused and BEFORE the state sets are swapped (finish_stage)."""
        g = self.grid
        q, names = self._state, self.tracer_names
        gamma, zeta, store, anchor_flag, third = rk3_operands(stage, self._anchor, self._tGn, self._tGm)
        head = (q[0].data_ptr(), q[1].data_ptr(), q[2].data_ptr(), self._ptrs([self._tr[n] for n in names]),
                self._ptrs([self._tr_alt[n] for n in names]), self._ptrs(self._tGn), self._ptrs(third) if third is not None else None,
                len(names), self.members, self.stride_m, g.Nx, g.Ny, g.Hx, g.Hy, q[0].stride(1), g.dx, g.dy, self.form_code)
        tail = (gamma, zeta, store, self._flags | self._rwrap | anchor_flag, _stream_ptr())
        par = dt is None
        f = getattr(self._L, f"swmhd_ensemble_tracers_rk3_{'params_' if par else ''}{self.sfx}")
        _lib.check(f(*head, self.parameters.data_ptr() if par else dt, *tail), "swmhd_ensemble_tracers_rk3" + ("_params" if par else ""))

    def _stage_steps(self, dt, n, step_dt=None):
        """n steps stage by stage (dt: the scalar, or None for the table; step_dt: the one dt all members share, or None where they
        differ -- what a correction whose call takes no table is given).  Without fused halos every stage ends with the periodic fill
        of the state and of the tracers, as the native driver fills the state."""
        for _ in range(n):
            for stage in range(3):
                self._stage_fused(dt, stage)
                finish_stage(self, dt, stage, step_dt=step_dt)
                if not self._rwrap:
                    self.update_state()

    # --- time stepping (the native ensemble step driver: 3 launches per RK3 step for all members) ---------------------
    def _enqueue_steps(self, dt, n, swapped):
        """n steps through swmhd_ensemble_step_rk3 (dt: the scalar) or, with dt None, swmhd_ensemble_step_rk3_params (the table)."""
        g = self.grid
        head = (self._ptrs(self._state), self._ptrs(self._alt), self._ptrs(self.Gn), self._ptrs(self.Gm), self.members, self.stride_m,
                g.Nx, g.Ny, g.Hx, g.Hy, self._state[0].stride(1), g.dx, g.dy)
        tail = (n, self._flags | self._rwrap, ctypes.byref(swapped), _stream_ptr())
        if dt is not None:
            f = getattr(self._L, f"swmhd_ensemble_step_rk3_{self.sfx}")
            _lib.check(f(*head, self.g, self.f, self.form_code, self.lorentz_code, dt, *tail), "swmhd_ensemble_step_rk3")
        else:
            f = getattr(self._L, f"swmhd_ensemble_step_rk3_params_{self.sfx}")
            _lib.check(f(*head, self.parameters.data_ptr(), self.form_code, self.lorentz_code, *tail), "swmhd_ensemble_step_rk3_params")

    def _native_steps(self, dt, n):
        if self._stochastic is not None and is_per_member(dt):
            raise _lib.SwmhdError("StochasticForcing with a per-member dt is not supported (SWMHD_ENOTSUP): its amplitude carries "
                                  "1/sqrt(dt), which the coefficient draw takes as one number")
        dts = self._dt_values(dt)
        if dts is not None:
            self._set_table_dt(dts)
        swapped = ctypes.c_int(0)
        if needs_stages(self):
            self._stage_steps(dt if dts is None else None, n, None if is_per_member(dt) else float(dt))
        else:
            self._enqueue_steps(dt if dts is None else None, n, swapped)
        if swapped.value:
            self._state, self._alt = self._alt, self._state
            self.Gn, self.Gm = self.Gm, self.Gn
        if n > 0 and self._rwrap:
            self._halo_stale = True
        self._advance_clock(n, dt, dts)
        self.iteration += n

    def time_step(self, dt):
        self._native_steps(dt, 1)

    def capture_graph(self, dt):
        """Capture TWO RK3 steps of every member into one HIP graph (ShallowWaterModel.capture_graph: same role tracking).  dt: a scalar
        or one value per member; with per-member parameters the graph reads the table at replay, and time_steps keeps its dt column
        at the captured values."""
        self._ensure_halos()
        saved = self._state + self.Gm + [self._tr[n] for n in self.tracer_names] + self._tGm
        if self._stochastic is not None:      # the warm-up steps advance the step counters: a replayed run draws what an eager run draws
            saved = saved + [self._stochastic.counter]
        if self.particles is not None:        # the warm-up steps move the particles
            saved = saved + self.particles.state_tensors()
        keep = [t.clone() for t in saved]
        t0, i0 = self._clock_state(), self.iteration
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self.time_step(dt); self.time_step(dt)
        torch.cuda.current_stream().wait_stream(side)
        self._graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self._graph):
            self.time_step(dt); self.time_step(dt)
        self._graph_dt = self._dt_key(dt)
        self._graph_roles = self._roles()
        for t, k in zip(saved, keep):   # (the two warm-up steps left every role where it was)
            t.copy_(k)
        self._halo_stale = False
        self._restore_clock(t0)
        self.iteration = i0
        return self

    def _roles(self):
        return tuple(t.data_ptr() for t in self._state) + tuple(t.data_ptr() for t in self.Gn)

    def time_steps(self, n, dt):
        """n RK3 steps of every member: graph replays (2 steps each) when a graph was captured for this dt, else the step driver."""
        gr = getattr(self, "_graph", None)
        same_dt = gr is not None and self._graph_dt == self._dt_key(dt)     # the captured dt VALUES, scalar or per member
        if same_dt and n >= 2 and self._roles() != self._graph_roles:
            self._native_steps(dt, 1)           # an odd number of steps since capture: one eager step restores the captured roles
            n -= 1
        if same_dt and n >= 2 and self._roles() == self._graph_roles:
            dts = self._dt_values(dt)
            if dts is not None:
                self._set_table_dt(dts)         # the graph reads the table when it runs
            for _ in range(n // 2):
                gr.replay()
                self._halo_stale = self._halo_stale or bool(self._rwrap)
                self._advance_clock(2, dt, dts)
                self.iteration += 2
            n = n % 2
        if n > 0:
            self._native_steps(dt, n)

    # --- diagnostics (SWMHD_example.jl:47-77) ------------------------------------------------------------------------
    def diagnostics_into(self, out, h_ref=1.0):
        """Enqueue every member's 7 diagnostics (KE, ME, PE, max|u|, max|v|, max|A|, min h; ShallowWaterModel.diagnostics order)
        into `out`, a contiguous float64 device tensor of shape (members, 7).  No host synchronisation."""
        g = self.grid
        if not (out.is_cuda and out.dtype == torch.float64 and tuple(out.shape) == (self.members, _lib.DIAG_NOUT) and out.is_contiguous()):
            raise _lib.SwmhdError(f"diagnostics_into: need a contiguous float64 CUDA tensor of shape ({self.members}, {_lib.DIAG_NOUT})")
        self._ensure_halos()
        if not hasattr(self, "_diag_ws"):
            self._diag_ws = torch.empty(_lib.ensemble_diag_workspace(self.members, g.Nx, g.Ny), dtype=torch.float64, device=out.device)
        q = self._state
        par = self.parameters is not None       # potential energy with each member's g, from the table
        f = getattr(self._L, f"swmhd_ensemble_diagnostics_{'params_' if par else ''}{self.sfx}")
        rc = f(q[0].data_ptr(), q[1].data_ptr(), q[2].data_ptr(), q[3].data_ptr(), self.members, self.stride_m, g.Nx, g.Ny, g.Hx, g.Hy,
               q[0].stride(1), g.dx, g.dy, self.parameters.data_ptr() if par else self.g, h_ref, self.form_code,
               self._diag_ws.data_ptr(), out.data_ptr(), _stream_ptr())
        _lib.check(rc, "swmhd_ensemble_diagnostics_params" if par else "swmhd_ensemble_diagnostics")
        return out

    def diagnostics(self, h_ref=1.0):
        """One dict per member with the keys of ShallowWaterModel.diagnostics."""
        out = self.diagnostics_into(torch.empty((self.members, _lib.DIAG_NOUT), dtype=torch.float64, device=self._state[0].device), h_ref)
        return [diagnostics_dict(v) for v in out.cpu().tolist()]

    # --- output frames of all members in one launch (swmhd_ensemble_output_fields_*) ---------------------------------
    def output_fields(self, names=("u", "v", "A", "s"), out=None, array_type=torch.float32):
        """ShallowWaterModel.output_fields for every member: the device tensor (members, len(names), Ny, Nx); member m of it is
        bitwise member(m).output_fields(...).  One launch, no host synchronisation."""
        from .output import enqueue_frame
        return enqueue_frame(self, names, out, array_type)

    # --- derived frames of all members in one launch (swmhd_ensemble_derived_fields[_params]_*) ----------------------
    def derived_fields(self, names=("vorticity", "current"), out=None, array_type=torch.float32):
        """ShallowWaterModel.derived_fields for every member: the device tensor (members, len(names), Ny, Nx); member m of it is
        bitwise member(m).derived_fields(...), the potential vorticity with member m's coriolis_f (from the parameter table where the
        ensemble has one).  One launch, no host synchronisation."""
        from .derived import enqueue_derived
        return enqueue_derived(self, names, out, array_type)

    # --- zonal means of all members in one launch (swmhd_ensemble_zonal_means_*) -------------------------------------
    def zonal_means(self, names=("u", "v", "A"), out=None):
        """ShallowWaterModel.zonal_means for every member: the float64 device tensor (members, len(names), Ny); member m of it is
        bitwise member(m).zonal_means(...).  One launch, no host synchronisation."""
        from .zonal import enqueue_zonal_means
        return enqueue_zonal_means(self, names, out)

    # --- zonal spectra of all members in two launches (swmhd_ensemble_zonal_spectra_*) --------------------------------
    def zonal_spectra(self, names=("u", "v", "A"), out=None):
        """ShallowWaterModel.zonal_spectra for every member: the float64 device tensor (members, len(names), Nx/2 + 1); member m of it
        is bitwise member(m).zonal_spectra(...).  No host synchronisation."""
        from .spectra import enqueue_zonal_spectra
        return enqueue_zonal_spectra(self, names, out)

    # --- 2-D and isotropic spectra of all members in three launches (swmhd_ensemble_spectra2d_*) --------------------
    def isotropic_spectra(self, names=("u", "v", "A"), out=None):
        """ShallowWaterModel.isotropic_spectra for every member: the float64 device tensor (members, len(names), NS); member m of it is
        bitwise member(m).isotropic_spectra(...).  No host synchronisation."""
        from .spectra2d import enqueue_isotropic_spectra
        return enqueue_isotropic_spectra(self, names, out)

    def power_spectra_2d(self, names=("u", "v", "A"), out=None):
        """ShallowWaterModel.power_spectra_2d for every member: (members, len(names), Nx/2 + 1, Ny)."""
        from .spectra2d import enqueue_power_spectra_2d
        return enqueue_power_spectra_2d(self, names, out)

    # --- one member as a ShallowWaterModel (checkpoints, inspection) ------------------------------------------------
    def member(self, m):
        """A ShallowWaterModel holding a copy of member m (state and tracers with halos, their G-, the member's g, f, clock and
        iteration)."""
        if not 0 <= m < self.members:
            raise IndexError(f"member {m} of {self.members}")
        self._ensure_halos()
        model = self._member_model(m)
        for fld, t in zip(model._raw_fields, self._state):
            fld.data.copy_(t[m])
        for fld, t in zip(model.Gm, self.Gm):
            fld.data.copy_(t[m])
        for k, n in enumerate(self.tracer_names):
            model._tr[n].data.copy_(self._tr[n][m])
            model._tGm[k].data.copy_(self._tGm[k][m])
        if self._stochastic is not None and model._stochastic is not None:
            model._stochastic.counter.copy_(self._stochastic.counter[m:m + 1])
        model.clock_time, model.iteration = float(self.clock_times[m]), self.iteration
        return model

    def _member_model(self, m):
        f = {"coriolis_f": float(self.f_values[m])} if self._coriolis is None else {"coriolis": self._coriolis.for_member(m)}
        return ShallowWaterModel(self.grid, float(self.g_values[m]), formulation=self.formulation,
                                 lorentz_forcing=self.lorentz_forcing, dtype=self.dtype, device=self._state[0].device, strict=self.strict,
                                 tracers=self.tracer_names, closure=closure_for_member(self.closure, m),
                                 forcing=forcing_for_member(self.forcing, m),
                                 bathymetry=self.bathymetry[m] if np.ndim(self.bathymetry) == 3 else self.bathymetry, **f)

    def synchronize(self):
        """Wait for everything enqueued; afterwards the halos of every member are current."""
        self._ensure_halos()
        torch.cuda.synchronize()


class BoundedShallowWaterEnsemble(ShallowWaterEnsemble):
    """`members` ShallowWaterModels of one grid with at least one Bounded direction, each with its own boundary conditions.
    `boundary_conditions`: one dict {name: FieldBoundaryConditions} for every member (ShallowWaterModel's argument), or a list of
    `members` such dicts (None entries: defaults).  Other arguments as ShallowWaterEnsemble's; fuse_halo=True lets the stage read the
    periodic images of a Periodic direction (the boundary-condition fill after every stage writes all halos either way).

    Every RK3 stage is one launch of the wall kernel for all members (G- form, as ShallowWaterModel.time_step runs a Bounded grid),
    followed by one boundary-condition fill of all members (swmhd_ensemble_step_rk3_bc).  Halos are always current."""

    def __init__(self, grid, members, gravitational_acceleration=9.81, coriolis_f=1.0, formulation=VectorInvariantFormulation,
                 lorentz_forcing=True, dtype=torch.float64, strict=False, device="cuda", member_stride=None, decomp=None,
                 fuse_halo=True, boundary_conditions=None, tracers=(), closure=None, coriolis=None, forcing=None, bathymetry=None,
                 particles=None):
        coriolis_f, varying = check_coriolis(coriolis, coriolis_f, 1.0)       # before anything is allocated
        check_bathymetry(bathymetry, grid, int(members), bounded_ensemble=True)      # (None passes; anything else is refused)
        check_forcing(forcing, grid, formulation_codes(formulation, lorentz_forcing)[2], tracer_names(tracers), int(members),
                      bounded_ensemble=True)       # (None and {} pass; anything else is refused before anything is allocated)
        if particles is not None:     # before anything is allocated
            raise _lib.SwmhdError("particles on a Bounded ensemble are not supported (SWMHD_ENOTSUP): swmhd_ensemble_step_rk3_bc is one "
                                  "native call and has no per-stage entry point for the particles' launch")
        if varying is not None:
            raise _lib.SwmhdError("coriolis = f(y) on a Bounded ensemble is not supported (SWMHD_ENOTSUP): swmhd_ensemble_step_rk3_bc is "
                                  "one native call and has no per-stage entry point for the correction launch")
        if closure is not None:       # before anything is allocated
            raise _lib.SwmhdError("closure on a Bounded ensemble is not supported (SWMHD_ENOTSUP): the wall faces of u and v and the "
                                  "gradient conditions need a kernel body of their own")
        if tracer_names(tracers):     # before anything is allocated
            raise _lib.SwmhdError("tracers on a Bounded ensemble are not supported (SWMHD_ENOTSUP): swmhd_ensemble_step_rk3_bc steps the "
                                  "four fields only and that schedule has no per-stage entry point")
        tx, ty = grid.topo_codes()
        self._bounded = (tx == _lib.BOUNDED, ty == _lib.BOUNDED)
        if not any(self._bounded):
            raise _lib.SwmhdError("BoundedShallowWaterEnsemble needs a Bounded direction: use ShallowWaterEnsemble for (Periodic, Periodic)")
        names = formulation_codes(formulation, lorentz_forcing)[2]
        B = int(members)
        if isinstance(boundary_conditions, (list, tuple)):
            if len(boundary_conditions) != B:
                raise _lib.SwmhdError(f"boundary_conditions: {len(boundary_conditions)} entries for {members} members")
            per_member = [dict(bc or {}) for bc in boundary_conditions]
        else:
            per_member = [dict(boundary_conditions or {})] * max(B, 0)
        for bcs in per_member:
            check_boundary_conditions(bcs, self._bounded, names)
        super().__init__(grid, members, gravitational_acceleration, coriolis_f, formulation, lorentz_forcing, dtype, strict, device,
                         member_stride, decomp, fuse_halo)
        self.coriolis = coriolis      # (None or an FPlane: its f went to the base class as coriolis_f)
        self._member_bcs = per_member
        # (members, 4 fields, 4 sides: west, east, south, north), NaN = default; in the ensemble's dtype (f32: rounded to nearest as the
        # single model's ctypes.c_float values are)
        table = [gradient_values(bcs, self.names) for bcs in per_member]
        self.gradients = torch.tensor(table, dtype=torch.float64).to(device=self._state[0].device, dtype=dtype)
        # the kernel reads the periodic images of a Periodic direction, as ShallowWaterModel sets _rwrap; halos never go stale
        self._kwrap = 0
        if fuse_halo and grid.Nx >= grid.Hx and grid.Ny >= grid.Hy:
            self._kwrap = (0 if self._bounded[0] else _lib.WRAP_X) | (0 if self._bounded[1] else _lib.WRAP_Y)
        self._rwrap = 0
        self._flags |= (_lib.BOUNDED_X if self._bounded[0] else 0) | (_lib.BOUNDED_Y if self._bounded[1] else 0)

    def _check_topology(self, grid):
        pass   # (checked in __init__)

    def update_state(self):
        """fill_halo_regions! of every member with its boundary conditions (swmhd_ensemble_fill_halo: two launches for all)."""
        g = self.grid
        self._halo_stale = False
        tx, ty = g.topo_codes()
        f = getattr(self._L, f"swmhd_ensemble_fill_halo_{self.sfx}")
        _lib.check(f(self._ptrs(self._state), 4, self.members, self.stride_m, g.Nx, g.Ny, g.Hx, g.Hy, self._state[0].stride(1), tx, ty,
                     0b0001, 0b0010, self.gradients.data_ptr(), g.dx, g.dy, _stream_ptr()), "swmhd_ensemble_fill_halo")

    def _enqueue_steps(self, dt, n, swapped):
        g = self.grid
        head = (self._ptrs(self._state), self._ptrs(self._alt), self._ptrs(self.Gn), self._ptrs(self.Gm), self.members, self.stride_m,
                g.Nx, g.Ny, g.Hx, g.Hy, self._state[0].stride(1), g.dx, g.dy)
        tail = (n, self.gradients.data_ptr(), self._flags | self._kwrap, ctypes.byref(swapped), _stream_ptr())
        if dt is not None:
            f = getattr(self._L, f"swmhd_ensemble_step_rk3_bc_{self.sfx}")
            _lib.check(f(*head, self.g, self.f, self.form_code, self.lorentz_code, dt, *tail), "swmhd_ensemble_step_rk3_bc")
        else:
            f = getattr(self._L, f"swmhd_ensemble_step_rk3_bc_params_{self.sfx}")
            _lib.check(f(*head, self.parameters.data_ptr(), self.form_code, self.lorentz_code, *tail), "swmhd_ensemble_step_rk3_bc_params")

    def _member_model(self, m):
        return ShallowWaterModel(self.grid, float(self.g_values[m]), float(self.f_values[m]), formulation=self.formulation,
                                 lorentz_forcing=self.lorentz_forcing, dtype=self.dtype, device=self._state[0].device, strict=self.strict,
                                 boundary_conditions=self._member_bcs[m])
