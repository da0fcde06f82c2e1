"""Host-side mirror of the ShallowWaterModel configuration the reference builds, driving the HIP engine.

Reference call sites being mirrored:
    jacobian_formulation/SWMHD_example.jl:21-42     ShallowWaterModel(grid, timestepper=:RungeKutta3, WENO5 ..., g=9.81,
        coriolis=FPlane(f=1), tracers=(:A), forcing=(u=Forcing(lorentz_force_func_x,...), v=...),
        formulation=VectorInvariantFormulation()); set!(model, u=, v=, h=, A=); Simulation(model, dt=0.01)
    divergence_formulation/divergence_sw_mhd.jl:19-39  same with ConservativeFormulation, forcing on uh, vh
One `time_step(dt)` == Oceananigans' RK3 `time_step!`: 3 x {calculate_tendencies!, rk3_substep!, store_tendencies!
(pointer swap), update_state! (halo fill)}.  All arithmetic happens in libswmhd.so; there is no CPU path.
"""
import numpy as np
import torch

from . import _lib
from .closure import check_closure
from .coriolis import check_coriolis, row_table
from .corrections import correction_list, live_fields, needs_stages
from .distributed import SlabDecomposition, agree_rc, exchange_y_halos
from .fields import Field, _SFX, _stream_ptr
from .forcing import check_bathymetry, check_forcing, check_source, check_stochastic, device_parents
from .particles import check_particles
from .stochastic import StochasticState
from .grid import Center, Face
from .shared import (RK3_GAMMA, RK3_ZETA, ConservativeFormulation, VectorInvariantFormulation, check_boundary_conditions,
                     diagnostics_dict, fill_groups, finish_stage, formulation_codes, gradient_values, rk3_stage)

# names a passive tracer may not take: the prognostic fields of either formulation and the derived output fields
RESERVED_NAMES = ("u", "v", "uh", "vh", "h", "A", "s", "B_x", "B_y")


def tracer_names(tracers):
    """`tracers=` of ShallowWaterModel as a tuple of checked names (the reference's `tracers = (:A)` is a tuple of names: every
    further one is a centre field advected like A).  Raises SwmhdError; touches no device."""
    if tracers is None:
        return ()
    names = (tracers,) if isinstance(tracers, str) else tuple(tracers)
    for n in names:
        if not isinstance(n, str) or not n:
            raise _lib.SwmhdError(f"tracers: {n!r} is not a name (a non-empty string)")
        if n in RESERVED_NAMES:
            raise _lib.SwmhdError(f"tracers: {n!r} names a field of the model or of its output frames ({' '.join(RESERVED_NAMES)})")
    if len(set(names)) != len(names):
        raise _lib.SwmhdError(f"tracers: duplicate names in {names!r}")
    if len(names) > _lib.MAX_TRACERS:
        raise _lib.SwmhdError(f"tracers: {len(names)} names, at most {_lib.MAX_TRACERS} (SWMHD_MAX_TRACERS)")
    return names


def rk3_operands(stage, anchor, Gn, Gm):
    """(gamma, zeta, store_G, extra flag, third operand) of a fused stage on the G sets Gn, Gm as they are when the stage is enqueued:
    rk3_stage plus SWMHD_RK3_ANCHOR or 0 and the fields to pass as G- (None: no third operand).  The state and the tracers both take
    theirs from here (the schedule of Rk3Buffers::stage in common.hpp): the tracers are only right with the operand the state picks."""
    gamma, zeta, store, anchor = rk3_stage(stage, anchor)
    if anchor:
        # stage 0 writes W into Gn; the per-stage swap of Gn and G- (time_step) hands it to stage 1 as G- and to stage 2 as Gn
        return gamma, zeta, store, _lib.RK3_ANCHOR, None if stage == 0 else (Gm if stage == 1 else Gn)
    return gamma, zeta, store, 0, Gm if stage > 0 else None


def loopback_rings(nranks, timeout_s=60.0):
    """`nranks` swmhd_ring handles of the in-process loopback transport (swmhd_ring_create_loopback): rank k's exchange copies the
    edge rows of ranks k-1 and k+1 (mod nranks) on the same GPU with RCCL's rendezvous semantics.  Pass handle k as
    `ShallowWaterModel(..., decomp=SlabDecomposition(Ny, nranks, k), ring=handle)` and drive each model from its own thread."""
    import ctypes
    arr = (ctypes.c_void_p * nranks)()
    _lib.check(_lib.lib().swmhd_ring_create_loopback(arr, nranks, float(timeout_s)), "swmhd_ring_create_loopback")
    return [ctypes.c_void_p(arr[k]) for k in range(nranks)]


class ShallowWaterModel:
    def __init__(self, grid, gravitational_acceleration=9.81, coriolis_f=1.0, formulation=VectorInvariantFormulation,
                 lorentz_forcing=True, dtype=torch.float64, device="cuda", strict=False, decomp=None, group=None,
                 overlap=True, fused=True, kernel="auto", fuse_halo=True, native_ring=True, boundary_conditions=None, ring=None,
                 tracers=(), closure=None, coriolis=None, forcing=None, bathymetry=None, particles=None):
        # coriolis = FPlane | BetaPlane | CoriolisProfile (swmhd_amd.coriolis), checked before anything is allocated.  None and FPlane:
        # the scalar f of the stage kernels, exactly the calls made without the argument.  Otherwise the stage kernels get f = 0 and
        # _coriolis holds the parameter whose rows a correction launch adds after every stage (corrections.correction_list)
        self.coriolis = coriolis
        coriolis_f, self._coriolis = check_coriolis(coriolis, coriolis_f, 1.0, decomp is not None and decomp.world_size > 1,
                                                    ring is not None, fused)
        if np.ndim(coriolis_f) or (self._coriolis is not None and self._coriolis.per_member is not None):
            raise _lib.SwmhdError(f"coriolis = {coriolis!r}: per-member values belong to an ensemble")
        rows = row_table(self._coriolis, grid) if self._coriolis is not None else None
        # passive tracers (swmhd_tracers_rk3_*): names and what they cannot be combined with are checked before anything is allocated
        self.tracer_names = tracer_names(tracers)
        if self.tracer_names:
            if decomp is not None and decomp.world_size > 1:
                raise _lib.SwmhdError("tracers on a y-slab decomposition are not supported (SWMHD_ENOTSUP): one rank only")
            if ring is not None:
                raise _lib.SwmhdError("tracers with ring= are not supported (SWMHD_ENOTSUP): the slab driver steps the four fields only")
            if not fused:
                raise _lib.SwmhdError("tracers need the fused stage kernel (SWMHD_ENOTSUP): fused=False has no tracer substep")
        # closure = ScalarDiffusivity(...) | ScalarBiharmonicDiffusivity(...) | a tuple with at most one of each: names and refusals are
        # checked before anything is allocated too.  _diffusion, _biharmonic: the coefficient of every field that has one of that kind;
        # None without such a closure and with one whose coefficients are all 0, and then the model makes exactly the calls it makes
        # without it
        self.closure = closure
        coefs, coefs4 = check_closure(closure, formulation_codes(formulation, lorentz_forcing)[2], self.tracer_names,
                                      formulation != VectorInvariantFormulation, any(c == _lib.BOUNDED for c in grid.topo_codes()),
                                      decomp is not None and decomp.world_size > 1, ring is not None, fused)
        self._diffusion = live_fields({n: float(c) for n, c in (coefs or {}).items()})
        self._biharmonic = live_fields({n: float(c) for n, c in (coefs4 or {}).items()})
        # forcing = {"u": Relaxation(...), "h": ..., "c": ...}: names, shapes, values and refusals are checked, and the callables
        # evaluated, before anything is allocated too.  _relaxation: the forced fields with a rate, in the order of the launch; None
        # without a forcing and with one whose rates are all 0, and then the model makes exactly the calls it makes without it
        self.forcing = forcing
        relax = check_forcing(forcing, grid, formulation_codes(formulation, lorentz_forcing)[2], self.tracer_names, None,
                              decomp is not None and decomp.world_size > 1, ring is not None, fused)
        # the StochasticForcing entries of `forcing` (swmhd_amd.stochastic): their draw groups; None without the class and with rates
        # that are all 0, and then nothing is allocated or enqueued for it
        stir = check_stochastic(forcing, grid, formulation_codes(formulation, lorentz_forcing)[2], self.tracer_names, None,
                                formulation != VectorInvariantFormulation)
        # bathymetry = b(x, y) at the cell centres (a callable, an array (Ny, Nx) or None): h stays the fluid thickness, the surface is
        # h + b.  Its slope and the Source entries of `forcing` are one static field per forced field, built here in float64, before
        # anything is allocated: _source is the list of (name, kind, S) of a correction launch (corrections.correction_list); None
        # without either and with fields that are all 0 (a constant b), and then the model makes exactly the calls it makes without them
        self.bathymetry = check_bathymetry(bathymetry, grid, None, decomp is not None and decomp.world_size > 1, ring is not None, fused)
        sources, self._source_thickness = check_source(forcing, self.bathymetry, grid, formulation_codes(formulation, lorentz_forcing)[2],
                                                       self.tracer_names, float(gravitational_acceleration), None,
                                                       formulation != VectorInvariantFormulation)
        # particles = LagrangianParticles(x, y, tracked_fields) (swmhd_amd.particles): refusals and the positions brought into the domain,
        # before anything is allocated.  None: the model makes exactly the calls it makes without the argument
        seeds = check_particles(particles, grid, formulation_codes(formulation, lorentz_forcing)[2], self.tracer_names, None,
                                decomp is not None and decomp.world_size > 1, ring is not None, fused)
        self.grid, self.g, self.f = grid, float(gravitational_acceleration), float(coriolis_f)
        self.formulation = formulation
        self.form_code, self.lorentz_code, self.names = formulation_codes(formulation, lorentz_forcing)
        self.strict = strict
        self._flags = (_lib.STRICT if strict else _lib.FAST) | _lib.KERNEL_FLAGS[kernel]
        # topology = (Periodic | Bounded, Periodic | Bounded, Flat): Bounded directions get wall reconstructions in the kernels
        # (SWMHD_BOUNDED_X / _Y) and the boundary-condition halo fill (swmhd_fill_halo) instead of the periodic copy
        tx, ty = grid.topo_codes()
        self._bounded = (tx == _lib.BOUNDED, ty == _lib.BOUNDED)
        self._flags |= (_lib.BOUNDED_X if self._bounded[0] else 0) | (_lib.BOUNDED_Y if self._bounded[1] else 0)
        # the anchor form of the fused stages (rk3_stage): fast builds on periodic grids; the state and the tracers both go by this
        self._anchor = not strict and not any(self._bounded)
        self.decomp = decomp or SlabDecomposition(grid.Ny_global, 1, 0)
        # y-slabs: a Periodic y direction is a ring (periodic decomposition; x may be Bounded, its walls are local to every slab), a
        # Bounded one a chain (SlabDecomposition(..., periodic=False)) with the south wall on rank 0 and the north wall on rank P-1
        self._chain = not self.decomp.periodic
        if self._bounded[1] and self.decomp.ring and not self._chain:
            raise _lib.SwmhdError("y-slab decomposition (ring halo exchange) of a Bounded-y grid needs a chain: "
                                  "SlabDecomposition(..., periodic=False) (SWMHD_ENOTSUP)")
        if self._chain and not self._bounded[1]:
            raise _lib.SwmhdError("a chain decomposition (SlabDecomposition(..., periodic=False)) needs a Bounded y direction")
        if self._chain:   # the cut sides of this slab: reconstructions next to them are those of the whole domain's interior rows
            self._flags |= (_lib.OPEN_SOUTH if self.decomp.south is not None else 0) | (_lib.OPEN_NORTH if self.decomp.north is not None else 0)
        # boundary_conditions = {"A": FieldBoundaryConditions(north = GradientBoundaryCondition(-0.05), ...)}  (SWMHD_example.jl:18-22)
        self.boundary_conditions = dict(boundary_conditions or {})
        check_boundary_conditions(self.boundary_conditions, self._bounded)
        self.group, self.overlap = group, overlap
        locs = ((Face, Center), (Center, Face), (Center, Center), (Center, Center))
        mk = lambda loc: Field(grid, loc, dtype, device)
        self._state = {n: mk(l) for n, l in zip(self.names, locs)}
        self.fused = fused                    # one kernel per RK3 stage (tendencies + substep), state ping-ponged
        # Periodic "gather on read" (SWMHD_WRAP_X / _Y): the tendency kernels take the periodic image instead of the halo cell, so
        # no halo-fill launch runs between RK3 stages -- x and y on one GPU, x on a slab (its y halos come from the ring).  The halos
        # of the state are then filled lazily, when something other than a tendency kernel is about to read them (_ensure_halos).
        self._rwrap = 0
        if fuse_halo and grid.Nx >= grid.Hx and grid.Ny >= grid.Hy:
            self._rwrap = (0 if self._bounded[0] else _lib.WRAP_X) | (0 if (self.decomp.ring or self._bounded[1]) else _lib.WRAP_Y)
        self._halo_stale = False
        self._exchange_in_flight = False      # torch p2p overlap path: a y exchange is queued on the comm stream
        self._alt = {n: mk(l) for n, l in zip(self.names, locs)} if fused else None
        self.Gn = [mk(l) for l in locs]     # Gⁿ
        self.Gm = [mk(l) for l in locs]     # G⁻
        # tracers: centre fields with an alternate set and two G sets like the state, swapped together with the state's (time_step)
        cc = (Center, Center)
        self._tr = {n: mk(cc) for n in self.tracer_names}
        self._tr_alt = {n: mk(cc) for n in self.tracer_names}
        self._tGn = [mk(cc) for _ in self.tracer_names]
        self._tGm = [mk(cc) for _ in self.tracer_names]
        self.sfx = _SFX[dtype]
        self.clock_time, self.iteration = 0.0, 0
        self._comm_stream = torch.cuda.Stream() if (self.decomp.ring and torch.cuda.is_available()) else None
        self._L = _lib.lib()
        self.tendency_events = None   # bench.py: list collecting (start, end) HIP events around every tendency launch
        if any(not f.data.is_cuda for f in self._state.values()):
            raise _lib.SwmhdError("ShallowWaterModel runs on the GPU only (no CPU fallback)")
        # (2, Ny) on the device, in the model's dtype and rounded to it: fc then ff, the table of swmhd_coriolis_rk3_*; built once
        self.coriolis_rows = None
        if rows is not None:
            self.coriolis_rows = torch.from_numpy(rows).to(device=self._raw_fields[0].data.device, dtype=dtype)
        # (name, rate, mask, target) of every forced field: mask and target arrays on the device as parents of the fields' shape and
        # pitch, in the model's dtype and rounded to it (None: no mask; a float: a scalar target); built once
        self._relaxation = None
        if relax is not None:
            dev = self._raw_fields[0].data.device
            up = lambda a: device_parents(grid, a, dtype, dev)
            self._relaxation = [(n, float(r), up(m), up(t) if np.ndim(t) else float(t)) for n, r, m, t in relax]
        # (name, kind, S) of every field with a static source: S on the device as a parent of the fields' shape and pitch, rounded once to
        # the model's dtype; built once
        self._source = None
        if sources is not None:
            self._source = [(n, k, device_parents(grid, S, dtype, self._raw_fields[0].data.device)) for n, k, S in sources]
        # the stochastic forcing on the device: step counter, coefficient pairs, tables (StochasticState); None where inactive
        self._stochastic = StochasticState(stir, grid, dtype, self._raw_fields[0].data.device) if stir is not None else None
        # the correction launches that follow every stage, in their order (finish_stage runs them); empty without any
        self._corrections = correction_list(self, self._raw_fields[0].stride_y)
        # the particles on the device: x, y and the stored velocity G-, float64 whatever the dtype; finish_stage runs their launch
        self.particles = particles
        if particles is not None:
            particles.bind(self, seeds, self._raw_fields[0].data.device)
        # y-slab ring: the native RCCL ring (swmhd_ring_*) when the process group is RCCL; torch.distributed p2p otherwise
        # (gloo rehearsals).  The ring's step driver needs the fused stage kernel and a slab taller than its two strips.
        # `ring`: a swmhd_ring handle created by the caller -- one of swmhd_ring_create_loopback's (loopback_rings below): several
        # slabs of one domain in ONE process on one GPU, each driven from its own host thread and stream.  The model owns it.
        self._ring = None
        if ring is not None:
            if not (self.decomp.ring and fused and grid.Ny > 2 * grid.Hy):
                raise _lib.SwmhdError("ring= needs a ring decomposition, the fused stage kernel and a slab taller than its two strips")
            self._ring, self._comm_stream = ring, None
        elif self.decomp.ring and native_ring and fused and grid.Ny > 2 * grid.Hy:
            self._ring = self._create_ring()

    def _create_ring(self):
        import ctypes, os
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized() and dist.get_backend(self.group) == "nccl"):
            return None
        dev = self._raw_fields[0].data.device
        rccl = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")     # the copy torch has loaded
        rccl = rccl.encode() if os.path.exists(rccl) else None
        # The ranks AGREE that every one of them can load RCCL (swmhd_ring_available: dlopen + symbol lookup, creates nothing) before any
        # of them enters the collective ncclCommInitRank: a rank that cannot must not leave its peers blocked inside communicator creation
        # -- then all of them take the torch.distributed p2p path instead.
        rc = self._L.swmhd_ring_available(rccl)
        ok = torch.tensor([1 if rc == 0 else 0], dtype=torch.int32, device=dev)
        dist.all_reduce(ok, op=dist.ReduceOp.MIN, group=self.group)
        if int(ok.item()) == 0:
            if rc != 0:
                import sys
                print(f"swmhd_amd: native ring unavailable ({self._L.swmhd_strerror(rc).decode()}); using torch.distributed p2p",
                      file=sys.stderr)
            return None
        ident = torch.zeros(_lib.RING_ID_BYTES, dtype=torch.uint8)
        if self.decomp.rank == 0:
            buf = (ctypes.c_ubyte * _lib.RING_ID_BYTES)()
            _lib.check(self._L.swmhd_ring_unique_id(rccl, buf), "swmhd_ring_unique_id")
            ident = torch.tensor(list(buf), dtype=torch.uint8)
        ident = ident.to(dev)
        src = dist.get_global_rank(self.group, 0) if self.group is not None else 0
        dist.broadcast(ident, src=src, group=self.group)
        raw = bytes(ident.cpu().tolist())
        ring = ctypes.c_void_p()
        with torch.cuda.device(dev):
            rc = self._L.swmhd_ring_create(ctypes.byref(ring), rccl, self.decomp.world_size, self.decomp.rank,
                                           (ctypes.c_ubyte * _lib.RING_ID_BYTES).from_buffer_copy(raw))
        # every rank learns whether ALL communicators exist: a rank that failed raises, and so do its peers (they destroy theirs
        # first) -- otherwise they would block in the first exchange until the launcher's deadline
        worst = agree_rc(rc, self.group, dev)
        if worst != 0:
            if rc == 0:
                self._L.swmhd_ring_destroy(ring)
                raise _lib.SwmhdError(f"swmhd_ring_create failed on another rank (rc {worst}); this rank destroyed its communicator")
            _lib.check(rc, "swmhd_ring_create")
        self._comm_stream = None      # the ring owns the comm stream of the native path
        return ring

    def _ring_check(self, rc, what):
        if rc == 4:   # SWMHD_ECOMM
            raise _lib.SwmhdError(f"{what}: {self._L.swmhd_ring_last_error(self._ring).decode()}")
        _lib.check(rc, what)

    def ring_time_launches(self, n):
        """bench.py: have the native ring driver record HIP events around its next n interior launches."""
        self._ring_check(self._L.swmhd_ring_time_launches(self._ring, n), "swmhd_ring_time_launches")

    def ring_launch_times(self, capacity=4096):
        import ctypes
        ms, rows = (ctypes.c_float * capacity)(), (ctypes.c_int * capacity)()
        n = self._L.swmhd_ring_launch_times(self._ring, ms, rows, capacity)
        return [(ms[k], rows[k]) for k in range(max(n, 0))]

    def _join(self):
        """Order the current stream behind whatever halo exchange is still in flight."""
        if self._ring is not None:
            self._ring_check(self._L.swmhd_ring_join(self._ring, _stream_ptr()), "swmhd_ring_join")
        if self._comm_stream is not None:
            torch.cuda.current_stream().wait_stream(self._comm_stream)
        self._exchange_in_flight = False

    def close(self):
        """Release the ring (RCCL communicator, comm stream).  Collective over the ranks like its creation; call it before
        torch.distributed.destroy_process_group()."""
        ring, self._ring = getattr(self, "_ring", None), None
        if ring is not None:
            self._L.swmhd_ring_destroy(ring)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- set!(model, u=..., v=..., h=..., A=...) ---------------------------------------------------------------
    def set(self, **kw):
        self._join()
        for k, v in kw.items():
            (self._tr[k] if k in self._tr else self._state[k]).set(v)
        self.update_state()
        return self

    @property
    def solution(self):
        """The prognostic fields by name (u|uh, v|vh, h, A, then the tracers), halos current."""
        self._ensure_halos()
        return {**self._state, **self._tr} if self._tr else self._state

    @property
    def tracers(self):
        """The passive tracers by name, halos current."""
        self._ensure_halos()
        return dict(self._tr)

    @property
    def fields(self):
        self._ensure_halos()
        return [self._state[n] for n in self.names]

    @property
    def _raw_fields(self):
        """The prognostic fields without touching their halos (which may be stale between stages)."""
        return [self._state[n] for n in self.names]

    def _ensure_halos(self):
        if self._halo_stale:
            self.update_state()

    # --- update_state!: fill halos (periodic x locally; y locally or by ring exchange) --------------------------
    def _fill(self, fields, names, face_x, face_y, which, stream=None, tag=""):
        """fill_halo_regions! of at most four fields (the limit of the fills) in one call: the periodic copy of the directions in
        `which`, or with a Bounded direction the boundary-condition fill with the fields' own gradient values (default: NaN) and face
        bits (bit k set: field k is a face field in that direction).  `which` without HALO_Y is a slab, whose y halos come from its
        neighbours: there the fill takes y walls only where this slab has them (none on a ring).  `tag` marks the call in an error."""
        import ctypes
        g = self.grid
        head = (_lib.ptr_array([f.ptr for f in fields]), len(fields), g.Nx, g.Ny, g.Hx, g.Hy, fields[0].stride_y)
        if not any(self._bounded):
            f = getattr(self._L, f"swmhd_fill_halo_periodic_multi_{self.sfx}")
            return _lib.check(f(*head, which, _stream_ptr(stream)), "fill_halo_multi" + tag)
        grads = sum(gradient_values(self.boundary_conditions, names), [])
        grads = ((ctypes.c_double if self.sfx == "f64" else ctypes.c_float) * len(grads))(*grads)
        tx, ty = g.topo_codes()
        what, ty = ("swmhd_fill_halo", ty) if which & _lib.HALO_Y else ("swmhd_fill_halo_walls", self.decomp.walls_y())
        f = getattr(self._L, f"{what}_{self.sfx}")
        _lib.check(f(*head, tx, ty, face_x, face_y, grads, g.dx, g.dy, _stream_ptr(stream)), what + tag)

    def _fill_x(self, stream=None):
        """The halo fill after a stage: the tracers first, in groups of four centre fields, then the state."""
        for grp in fill_groups(self.tracer_names):
            self._fill([self._tr[n] for n in grp], grp, 0, 0, _lib.HALO_X | _lib.HALO_Y, stream, " (tracers)")
        self._fill(self._raw_fields, self.names, 0b0001, 0b0010, _lib.HALO_X | (0 if self.decomp.ring else _lib.HALO_Y), stream)

    def update_state(self):
        self._join()
        self._halo_stale = False
        self._fill_x()
        q = self._raw_fields
        if self._ring is not None:
            g = self.grid
            if self._chain:      # nothing travels across the chain's walls
                f = getattr(self._L, f"swmhd_ring_exchange_y_sides_{self.sfx}")
                rc = f(self._ring, _lib.ptr_array([x.ptr for x in q]), 4, g.Nx, g.Ny, g.Hx, g.Hy, q[0].stride_y, self.decomp.cuts(),
                       _stream_ptr())
            else:
                f = getattr(self._L, f"swmhd_ring_exchange_y_{self.sfx}")
                rc = f(self._ring, _lib.ptr_array([x.ptr for x in q]), 4, g.Nx, g.Ny, g.Hx, g.Hy, q[0].stride_y, _stream_ptr())
            self._ring_check(rc, "swmhd_ring_exchange_y")
        elif self.decomp.ring:
            exchange_y_halos([f.data for f in q], self.grid.Ny, self.grid.Hy, self.decomp, self.group)

    # --- calculate_tendencies! ------------------------------------------------------------------------------
    def calculate_tendencies(self, rows=None, stream=None):
        if self.tendency_events is not None and rows is None:
            e0, e1 = _lib.TimingEvent(), _lib.TimingEvent()
            e0.record()
            self._calculate_tendencies(rows, stream)
            e1.record()
            self.tendency_events.append((e0, e1, self.grid.Ny))
        else:
            self._calculate_tendencies(rows, stream)

    def _calculate_tendencies(self, rows=None, stream=None):
        g = self.grid
        q = self._raw_fields
        j0, j1 = (0, g.Ny) if rows is None else rows
        f = getattr(self._L, f"swmhd_tendencies_{self.sfx}")
        rc = f(q[0].ptr, q[1].ptr, q[2].ptr, q[3].ptr, self.Gn[0].ptr, self.Gn[1].ptr, self.Gn[2].ptr, self.Gn[3].ptr,
               g.Nx, g.Ny, g.Hx, g.Hy, q[0].stride_y, g.dx, g.dy, self.g, self.f, self.form_code, self.lorentz_code,
               j0, j1, self._flags | self._rwrap, _stream_ptr(stream))
        _lib.check(rc, "swmhd_tendencies")

    def _substep(self, dt, stage):
        g = self.grid
        U = _lib.ptr_array([f.ptr for f in self._raw_fields])
        Gn = _lib.ptr_array([f.ptr for f in self.Gn])
        Gm = _lib.ptr_array([f.ptr for f in self.Gm]) if stage > 0 else None
        f = getattr(self._L, f"swmhd_rk3_substep_{self.sfx}")
        rc = f(U, Gn, Gm, g.Nx, g.Ny, g.Hx, g.Hy, self._raw_fields[0].stride_y, dt, RK3_GAMMA[stage], RK3_ZETA[stage], 0, g.Ny,
               _lib.STRICT if self.strict else _lib.FAST, _stream_ptr())
        _lib.check(rc, "swmhd_rk3_substep")

    def _stage_fused(self, dt, stage, rows=None, extra_flags=0):
        """calculate_tendencies! + rk3_substep! in one launch: reads the current state, writes the new state into the
        alternate buffers (swmhd_tendencies_rk3_*)."""
        g = self.grid
        j0, j1 = (0, g.Ny) if rows is None else rows
        q = _lib.ptr_array([f.ptr for f in self._raw_fields])
        qn = _lib.ptr_array([self._alt[n].ptr for n in self.names])
        Gn = _lib.ptr_array([f.ptr for f in self.Gn])
        gamma, zeta, store, anchor_flag, third = rk3_operands(stage, self._anchor, self.Gn, self.Gm)
        Gm = _lib.ptr_array([f.ptr for f in third]) if third is not None else None
        f = getattr(self._L, f"swmhd_tendencies_rk3_{self.sfx}")
        timed = self.tendency_events is not None and 2 * (j1 - j0) > g.Ny    # whole grid, or the interior launch of a slab
        if timed:
            e0, e1 = _lib.TimingEvent(), _lib.TimingEvent()
            e0.record()
        rc = f(q, qn, Gn, Gm, g.Nx, g.Ny, g.Hx, g.Hy, self._raw_fields[0].stride_y, g.dx, g.dy, self.g, self.f, self.form_code,
               self.lorentz_code, dt, gamma, zeta, store, j0, j1,
               self._flags | self._rwrap | extra_flags | anchor_flag, _stream_ptr())
        if timed:
            e1.record()
            self.tendency_events.append((e0, e1, j1 - j0))
        _lib.check(rc, "swmhd_tendencies_rk3")

    def _tracer_stage(self, dt, stage):
        """All tracers through RK3 stage `stage` in one launch (swmhd_tracers_rk3_*), advected by the state the stage started from: call
        it after _stage_fused and BEFORE the state sets are swapped.  Same (gamma, zeta, store_G, anchor) as the state's stage."""
        g = self.grid
        q = self._raw_fields
        names = self.tracer_names
        P = _lib.ptr_array
        gamma, zeta, store, anchor_flag, third = rk3_operands(stage, self._anchor, self._tGn, self._tGm)
        flags = (self._flags & ~(_lib.TILE_KERNEL | _lib.MARCH_KERNEL)) | self._rwrap | anchor_flag
        Gm = P([f.ptr for f in third]) if third is not None else None
        f = getattr(self._L, f"swmhd_tracers_rk3_{self.sfx}")
        rc = f(q[0].ptr, q[1].ptr, q[2].ptr, P([self._tr[n].ptr for n in names]), P([self._tr_alt[n].ptr for n in names]),
               P([x.ptr for x in self._tGn]), Gm, len(names), g.Nx, g.Ny, g.Hx, g.Hy, q[0].stride_y, g.dx, g.dy, self.form_code,
               dt, gamma, zeta, store, 0, g.Ny, flags, _stream_ptr())
        _lib.check(rc, "swmhd_tracers_rk3")

    # --- time_step!(model, dt): RungeKutta3 ------------------------------------------------------------------
    def _native_steps(self, dt, n):
        """n RK3 steps in ONE C call that enqueues every launch: the native ring driver (swmhd_ring_step_rk3_*) on a slab, the step
        driver (swmhd_step_rk3_*) on one GPU."""
        import ctypes
        gr, ring, bounded = self.grid, self._ring is not None, any(self._bounded)
        wrap = self._rwrap & _lib.WRAP_X if ring else self._rwrap     # (a slab's y halos come from the ring)
        if ring and bounded:
            wrap = 0                  # (the Bounded slab driver fills every halo between the stages: its state's halos stay current)
        if ring and self._halo_stale and not wrap:
            self.update_state()
        swapped = ctypes.c_int(0)
        # the arguments the three drivers share: up to nsteps, and state_in_alt, stream after the flags
        head = (_lib.ptr_array([f.ptr for f in self._raw_fields]), _lib.ptr_array([self._alt[nm].ptr for nm in self.names]),
                _lib.ptr_array([f.ptr for f in self.Gn]), _lib.ptr_array([f.ptr for f in self.Gm]), gr.Nx, gr.Ny, gr.Hx, gr.Hy,
                self._raw_fields[0].stride_y, gr.dx, gr.dy, self.g, self.f, self.form_code, self.lorentz_code, dt, n)
        tail = (ctypes.byref(swapped), _stream_ptr())
        if ring and bounded:
            # Bounded slabs (a chain, or Bounded x on a ring): the driver decides the cut sides itself and fills the boundary conditions
            # from a device table of the 16 gradient values
            if getattr(self, "_grad_dev", None) is None:
                q0 = self._raw_fields[0].data
                grads = sum(gradient_values(self.boundary_conditions, self.names), [])
                self._grad_dev = torch.tensor(grads, dtype=q0.dtype, device=q0.device)
            fl = self._flags & ~(_lib.OPEN_SOUTH | _lib.OPEN_NORTH)
            step = getattr(self._L, f"swmhd_ring_step_rk3_bc_{self.sfx}")
            self._ring_check(step(self._ring, *head, self._grad_dev.data_ptr(), fl, *tail), "swmhd_ring_step_rk3_bc")
        elif ring:
            step = getattr(self._L, f"swmhd_ring_step_rk3_{self.sfx}")
            self._ring_check(step(self._ring, *head, self._flags | wrap, *tail), "swmhd_ring_step_rk3")
        else:
            _lib.check(getattr(self._L, f"swmhd_step_rk3_{self.sfx}")(*head, self._flags | wrap, *tail), "swmhd_step_rk3")
        if swapped.value:
            self._state, self._alt = self._alt, self._state
            self.Gn, self.Gm = self.Gm, self.Gn
        if n > 0 and wrap:
            self._halo_stale = True       # the wrapped halos were not filled (a slab: the y exchange of the final state is in flight, see _join)
        self.clock_time += n * dt
        self.iteration += n

    def time_step(self, dt):
        if self._ring is not None:
            return self._native_steps(dt, 1)
        g, H = self.grid, 3          # strips and per-stage exchange: the stencil's reach, whatever the grid's halo depth
        multi = self.decomp.ring
        overlap = multi and self.overlap and self._comm_stream is not None and g.Ny > 2 * H
        for stage in range(3):
            # one RK3 stage over a row range: either the fused kernel or tendencies followed (later) by the substep
            run = (lambda rows=None, fl=0: self._stage_fused(dt, stage, rows, fl)) if self.fused else (lambda rows=None, fl=0: self.calculate_tendencies(rows=rows))
            if overlap and self._exchange_in_flight:
                # x halos are current; the y exchange of the previous stage is in flight on the comm stream.  Interior rows run
                # on the main stream; the two H-row boundary strips are queued on the COMM stream behind the exchange, so they
                # start the moment the halo rows land and overlap the tail of the interior kernel.
                run((H, g.Ny - H), _lib.LEAVE_ROOM)    # leave workgroup slots for the comm stream's kernels
                with torch.cuda.stream(self._comm_stream):
                    run((0, H))
                    run((g.Ny - H, g.Ny))
                torch.cuda.current_stream().wait_stream(self._comm_stream)
            else:
                run()
            if not self.fused:
                self._substep(dt, stage)
            finish_stage(self, dt, stage, self.fused)    # the tracers' launch, then the swaps of state, tracers and G sets
            if any(self._bounded) or not (self._rwrap & _lib.WRAP_X):
                self._fill_x()                           # (otherwise the next stage reads the periodic images itself)
            else:
                self._halo_stale = True
            if multi:
                if overlap:
                    self._comm_stream.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(self._comm_stream):
                        exchange_y_halos([f.data for f in self._raw_fields], g.Ny, g.Hy, self.decomp, self.group, depth=H)
                    self._exchange_in_flight = True
                else:
                    exchange_y_halos([f.data for f in self._raw_fields], g.Ny, g.Hy, self.decomp, self.group, depth=H)
        self.clock_time += dt
        self.iteration += 1

    # --- HIP-graph replay of the step (single GPU): the reference's own grids are 64^2 .. 128^2 (SWMHD_example.jl:11), where a
    #     step is 6 launches of ~10 us kernels and the host would otherwise set the pace --------------------------------
    def capture_graph(self, dt):
        """Capture TWO RK3 steps (6 fused stages + 6 halo fills) into one HIP graph; two, because the ping-ponged state and the
        G-/Gn pointers return to their original roles after an even number of stages.  `time_steps` then replays it."""
        if self.decomp.ring or not self.fused:
            raise _lib.SwmhdError("capture_graph: single-GPU fused path only (halo exchange is not capturable)")
        self._ensure_halos()
        saved = self._raw_fields + self.Gm + [self._tr[n] for n in self.tracer_names] + self._tGm
        keep = [f.data.clone() for f in saved]
        # the step counter of a stochastic forcing: the warm-up steps draw and advance it, a replayed run must draw what an eager run draws
        counter = self._stochastic.counter.clone() if self._stochastic is not None else None
        # the particles' positions and stored velocity: the warm-up steps move them
        parts = self.particles.state_tensors() if self.particles is not None else []
        keep_parts = [t.clone() for t in parts]
        t0, i0 = self.clock_time, self.iteration
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):          # warm-up outside capture (lazy module loads etc.)
            self.time_step(dt); self.time_step(dt)
        torch.cuda.current_stream().wait_stream(side)
        self._graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self._graph):
            self.time_step(dt); self.time_step(dt)
        self._graph_dt = dt
        # the graph has the device pointers of THIS role assignment baked in (state in `solution`, scratch in `_alt`, Gn/Gm as
        # they are now): it may only be replayed while the roles are the same, i.e. after an even number of eager steps
        self._graph_roles = self._roles()
        for f, k in zip(saved, keep):   # capture does not execute; undo the two warm-up steps (which left every role where it was)
            f.data.copy_(k)
        if counter is not None:
            self._stochastic.counter.copy_(counter)
        for t, k in zip(parts, keep_parts):
            t.copy_(k)
        self._halo_stale = False
        self.clock_time, self.iteration = t0, i0
        return self

    def _roles(self):
        """Which buffer plays which role right now (every RK3 step swaps state<->scratch and Gn<->G- an odd number of times)."""
        return tuple(f.ptr for f in self._raw_fields) + tuple(f.ptr for f in self.Gn)

    def time_steps(self, n, dt):
        """n RK3 steps: graph replays (2 steps each) when a graph was captured for this dt; otherwise the native step driver
        (swmhd_step_rk3_*: one C call enqueues all 6n launches) on a single GPU, or Python-driven stages on several."""
        g = getattr(self, "_graph", None)
        if g is not None and self._graph_dt == dt and n >= 2 and self._roles() != self._graph_roles:
            # an odd number of steps has run since capture (a leftover step of an earlier call, or a plain time_step): the
            # graph would read the scratch buffers as the state.  One eager step restores the captured roles.
            self._driver_steps(dt, 1)
            n -= 1
        if g is not None and self._graph_dt == dt and self._roles() == self._graph_roles:
            for _ in range(n // 2):
                g.replay()
                self._halo_stale = self._halo_stale or bool(self._rwrap)
                self.clock_time += 2 * dt
                self.iteration += 2
            n = n % 2
        if n > 0:
            self._driver_steps(dt, n)

    def _driver_steps(self, dt, n):
        if self._ring is not None or (not self.decomp.ring and self.fused and self.tendency_events is None and not any(self._bounded)
                                      and not needs_stages(self)):
            return self._native_steps(dt, n)
        for _ in range(n):
            self.time_step(dt)

    # --- diagnostics (SWMHD_example.jl:47-77): energies and extrema in one device pass ------------------------
    def diagnostics(self, h_ref=1.0):
        """dict(kinetic_energy, magnetic_energy, potential_energy, total_energy, max_abs_u, max_abs_v, max_abs_A, min_h)
        over the whole (possibly decomposed) domain; energies as the reference's mean(...)*Lx*Ly."""
        g = self.grid
        self._join()
        if not hasattr(self, "_diag_ws"):
            self._diag_ws = torch.empty(_lib.DIAG_WORKSPACE, dtype=torch.float64, device=self.fields[0].data.device)
            self._diag_out = torch.empty(_lib.DIAG_NOUT, dtype=torch.float64, device=self.fields[0].data.device)
        q = self.fields
        f = getattr(self._L, f"swmhd_diagnostics_{self.sfx}")
        rc = f(q[0].ptr, q[1].ptr, q[2].ptr, q[3].ptr, g.Nx, g.Ny, g.Hx, g.Hy, q[0].stride_y, g.dx, g.dy, self.g, h_ref,
               self.form_code, 0, g.Ny, self._diag_ws.data_ptr(), self._diag_out.data_ptr(), _stream_ptr())
        _lib.check(rc, "swmhd_diagnostics")
        out = self._diag_out.clone()
        if self.decomp.world_size > 1:   # the only collective in the package, 7 scalars, off the data path
            import torch.distributed as dist
            sums, maxs, mins = out[:3].clone(), out[3:6].clone(), out[6:].clone()
            if sums.is_cuda and dist.get_backend(self.group) == "gloo":
                sums, maxs, mins = sums.cpu(), maxs.cpu(), mins.cpu()
            dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=self.group)
            dist.all_reduce(maxs, op=dist.ReduceOp.MAX, group=self.group)
            dist.all_reduce(mins, op=dist.ReduceOp.MIN, group=self.group)
            out = torch.cat([sums.cpu(), maxs.cpu(), mins.cpu()])
        return diagnostics_dict(out.cpu().tolist())

    # --- output frames (the reference's field writer, SWMHD_example.jl:80-84): one launch, no host synchronisation -------
    def output_fields(self, names=("u", "v", "A", "s"), out=None, array_type=torch.float32):
        """Enqueue one frame of the current state: the device tensor (len(names), Ny, Nx) of the named fields -- u v h A s B_x B_y,
        s = sqrt(u^2 + v^2), B = (-dA/dy, dA/dx) / h (swmhd_output_fields_* in include/swmhd.h) -- halo-stripped, in `array_type` (or
        into `out`, float32 or float64 of that shape).  On a y-slab: this rank's rows.  Reads the periodic images where the step leaves
        the halos stale, so no halo fill runs in front of it.  See swmhd_amd.output for the writer (FieldTimeSeries, run)."""
        from .output import enqueue_frame
        return enqueue_frame(self, names, out, array_type)

    # --- derived frames (Oceananigans: ∂x(v) - ∂y(u) handed to the writer): one launch, no halo fill, no host synchronisation ----
    def derived_fields(self, names=("vorticity", "current"), out=None, array_type=torch.float32):
        """Enqueue the differenced fields of the current state: the device tensor (len(names), Ny, Nx) of vorticity (dv/dx - du/dy at
        the corners), divergence (du/dx + dv/dy at the centres), current (J = laplace(A) at the centres) and potential_vorticity
        ((vorticity + coriolis_f) / h at the corners) -- swmhd_derived_fields_* in include/swmhd_derived.h; u, v are the frame's
        velocities for the conservative model too -- halo-stripped, in `array_type` (or into `out`, float32 or float64 of that shape),
        any order and repetition of names.  Points: i = 1..Nx, j = 1..Ny, on Bounded directions too.  On a y-slab: this rank's rows.
        Reads the periodic images where the step leaves the halos stale.  FieldTimeSeries takes these names among the frame's."""
        from .derived import enqueue_derived
        return enqueue_derived(self, names, out, array_type)

    # --- zonal means (Oceananigans: Average(u, dims = 1)): one launch, no frame-sized buffer, no host synchronisation ----
    def zonal_means(self, names=("u", "v", "A"), out=None):
        """Enqueue the x-averaged profiles of the current state: the float64 device tensor (len(names), Ny), row j of profile k =
        (sum over i = 1..Nx of term_k(i, j)) / Nx -- the frame fields u v h A s B_x B_y and the second moments uu vv uv B_xB_x B_yB_y
        B_xB_y vA (swmhd_zonal_means_* in include/swmhd_zonal.h; uv is the Reynolds stress, B_xB_y the Maxwell stress, -d(vA)/dy the whole
        right-hand side of the mean potential).  The points averaged are the frame's, on Bounded directions too.  On a y-slab: this
        rank's rows.  The summation order depends on Nx alone, so a profile is reproducible bit for bit.  Eddy quantities are the
        caller's subtraction: <u'v'> = <uv> - <u><v> cancels where the eddies are weak, and loses that many digits.  See
        swmhd_amd.zonal for the writer (ZonalMeanTimeSeries)."""
        from .zonal import enqueue_zonal_means
        return enqueue_zonal_means(self, names, out)

    # --- zonal spectra: a row FFT in LDS and a row average, two launches, no frame-sized buffer, no host synchronisation ----
    def zonal_spectra(self, names=("u", "v", "A"), out=None):
        """Enqueue the zonal power spectra of the current state: the float64 device tensor (len(names), Nx/2 + 1), entry k of spectrum
        F = the mean over the rows of c_k |F^_j[k]|^2, F^_j the DFT along x of row j of the float64 frame field F (u v h A s B_x B_y)
        divided by Nx, c_k = 1 at k = 0 and k = Nx/2 and 2 between, so that the entries sum to the mean of F^2
        (swmhd_zonal_spectra_* in include/swmhd_spectra.h).  Nx must be a power of two from 4 to 4096 and the x direction Periodic.  On a
        y-slab: the spectrum of this rank's rows.  The summation order depends on (Nx, Ny) alone, so a spectrum is reproducible bit for
        bit.  See swmhd_amd.spectra for the writer (ZonalSpectrumTimeSeries)."""
        from .spectra import enqueue_zonal_spectra
        return enqueue_zonal_spectra(self, names, out)

    # --- 2-D and isotropic spectra: the row FFT keeping its modes, a column FFT in LDS and the shell sum, three launches ----
    def isotropic_spectra(self, names=("u", "v", "A"), out=None):
        """Enqueue the isotropic power spectra of the current state: the float64 device tensor (len(names), NS), entry s of spectrum F =
        the sum of P2[kx, ky] over the modes whose shell floor(sqrt(wx kx^2 + wy my^2) + 1/2) is s, P2 = c_kx |F^[kx, ky]|^2 of the 2-D
        DFT of the float64 frame field F divided by Nx Ny, so that the entries sum to the mean of F^2 (swmhd_spectra2d_* in
        include/swmhd_spectra2d.h).  The shell width is max(2 pi/Lx, 2 pi/Ly); swmhd_amd.spectra2d.isotropic_shells(grid) gives the
        wavenumbers and the mode counts.  Both sizes must be powers of two from 4 to 4096 and both directions Periodic; a model on a
        y-slab of several ranks is refused (a 2-D transform needs every row).  Bit-reproducible.  See swmhd_amd.spectra2d for the
        writer (IsotropicSpectrumTimeSeries)."""
        from .spectra2d import enqueue_isotropic_spectra
        return enqueue_isotropic_spectra(self, names, out)

    def power_spectra_2d(self, names=("u", "v", "A"), out=None):
        """Enqueue the 2-D power spectra P2[kx, ky] of the current state: the float64 device tensor (len(names), Nx/2 + 1, Ny), ky in
        FFT order (0 .. Ny/2, then -Ny/2 + 1 .. -1); its entries sum to the mean of F^2.  What isotropic_spectra sums over shells."""
        from .spectra2d import enqueue_power_spectra_2d
        return enqueue_power_spectra_2d(self, names, out)

    # --- checkpoint: prognostic fields with halos + G⁻ + clock, one .npz per rank ---------------------------------
    def save_checkpoint(self, path):
        import numpy as np
        self.synchronize()
        np.savez(path, time=self.clock_time, iteration=self.iteration,
                 **{n: f.numpy() for n, f in zip(self.names, self.fields)},
                 **{"Gm_" + n: f.numpy() for n, f in zip(self.names, self.Gm)},
                 **{"tracer_" + n: self._tr[n].numpy() for n in self.tracer_names},
                 **{"tracer_Gm_" + n: f.numpy() for n, f in zip(self.tracer_names, self._tGm)},
                 **({"stochastic_counter": self._stochastic.counter_values()} if self._stochastic is not None else {}),
                 **({"particles_x": self.particles.x.cpu().numpy(), "particles_y": self.particles.y.cpu().numpy()}
                    if self.particles is not None else {}))      # (G- is dead at step boundaries: zeta_1 = 0)

    def load_checkpoint(self, path):
        import numpy as np
        self._join()
        z = np.load(path, allow_pickle=False)
        self._halo_stale = False              # the checkpoint holds the parents, halos included
        for n, f in zip(self.names, self._raw_fields):
            f.data.copy_(torch.from_numpy(z[n]).to(f.data.dtype))
        for n, f in zip(self.names, self.Gm):
            f.data.copy_(torch.from_numpy(z["Gm_" + n]).to(f.data.dtype))
        for n, f in zip(self.tracer_names, self._tGm):
            self._tr[n].data.copy_(torch.from_numpy(z["tracer_" + n]).to(f.data.dtype))
            f.data.copy_(torch.from_numpy(z["tracer_Gm_" + n]).to(f.data.dtype))
        if self._stochastic is not None and "stochastic_counter" in z.files:      # (older checkpoints have none: the counter stays)
            self._stochastic.set_counter(z["stochastic_counter"])
        if self.particles is not None and "particles_x" in z.files:      # (a checkpoint without particles: the positions stay)
            self.particles.x.copy_(torch.from_numpy(z["particles_x"]))
            self.particles.y.copy_(torch.from_numpy(z["particles_y"]))
        self.clock_time, self.iteration = float(z["time"]), int(z["iteration"])
        return self

    def synchronize(self):
        """Wait for everything enqueued; afterwards the halos of the state are current (they are filled lazily, see __init__)."""
        self._ensure_halos()
        self._join()
        torch.cuda.synchronize()
