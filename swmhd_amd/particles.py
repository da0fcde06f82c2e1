"""Lagrangian particles carried by a ShallowWaterModel or a ShallowWaterEnsemble, and the writer that collects them on the device.

Oceananigans' `LagrangianParticles(x=..., y=..., tracked_fields=...)`.  Shallow-water MHD has a particular use for it: in the ideal model
the potential obeys dA/dt + u.grad A = 0, so A read along a trajectory is constant, the trajectories are the frozen-in field lines and
the drift of `sample("A")` along them measures the numerical resistivity of the scheme directly.  Particle dispersion is the Lagrangian
statistic of the stirred runs StochasticForcing serves.

Positions are one more prognostic of the model's RK3 (include/swmhd_particles.h states the scheme, the index rules and the fold): every
stage is ONE gather-bound launch (swmhd_[ensemble_]particles_rk3_*) behind the stage's corrections, on the state the stage started
from, with no host synchronisation; it captures into the graph of capture_graph.  Positions and the stored velocity G- are float64
whatever the model's dtype.  `sample(names)` interpolates prognostic fields and tracers to the positions (`tracked_fields`), and
ParticleTimeSeries speaks the writer protocol of swmhd_amd.output.run().

Not built: particles on y-slabs and on Bounded ensembles (refused), unwrapped positions across a periodic box (keep the sampled
velocities), a sort of the particles by cell, inertial or charged particles, particles that feed back on the flow.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._series import DeviceTimeSeries, lead_shape
from .fields import _stream_ptr
from .output import TimeInterval
from .shared import RK3_GAMMA, RK3_ZETA

POSITION_NAMES = ("x", "y")


def fold_periodic(x, x0, L):
    """The kernel's periodic fold on the host (numpy, float64, the same operations): x - L floor((x - x0) / L), clamped into
    [x0, x0 + L]; non-finite values stay as they are."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        folded = x - L * np.floor((x - x0) / L)
        folded = np.where(folded < x0, x0, np.where(folded > x0 + L, x0 + L, folded))
    return np.where(np.isfinite(x), folded, x)


def _positions(v, what, members):
    """`v` as a float64 host array (P,), or (members, P) for an ensemble (a (P,) array is every member's)."""
    a = np.array(v, dtype=np.float64)
    if members is None:
        if a.ndim != 1:
            raise _lib.SwmhdError(f"LagrangianParticles: {what} has shape {a.shape}: one array of P positions")
        return a
    if a.ndim == 1:
        return np.repeat(a[None], members, axis=0)
    if a.ndim != 2 or a.shape[0] != members:
        raise _lib.SwmhdError(f"LagrangianParticles: {what} has shape {a.shape}: (P,) or ({members}, P)")
    return a


def seeded(a, axis, grid, bounded, what):
    """Initial positions of one direction brought into the domain: folded where the direction is Periodic, refused (SwmhdError) where
    it is Bounded and a position lies outside [x0, x0 + N d] -- the extent as the kernel forms it."""
    lo, N, d = (grid.x[0], grid.Nx, grid.dx) if axis == 0 else (grid.y[0], grid.Ny_global, grid.dy)
    lo, L = float(lo), float(N) * float(d)
    if not bounded:
        return fold_periodic(a, lo, L)
    if not np.all((a >= lo) & (a <= lo + L)):
        raise _lib.SwmhdError(f"LagrangianParticles: {what} positions outside the Bounded domain [{lo}, {lo + L}]")
    return a


class LagrangianParticles:
    """`LagrangianParticles(x, y, tracked_fields=())`: P particles at (x[p], y[p]), handed to ONE model as
    `ShallowWaterModel(grid, ..., particles=...)` or `ShallowWaterEnsemble(grid, members, ..., particles=...)`.  x, y: arrays of one
    length P; for an ensemble (P,) (every member's) or (members, P).  Positions outside a Periodic direction are folded into it,
    positions outside a Bounded one refused.  tracked_fields: names among the model's four prognostic fields and its tracers, what
    `sample()` returns by default.

    On the model: `x`, `y` are float64 device tensors (P,) -- (members, P) on an ensemble --, current after every step; `set(x=, y=)`
    replaces them; `sample(names)` is the float64 device tensor (len(names), P) -- (members, len(names), P) -- of the fields
    interpolated to the positions, one launch, no synchronisation."""

    def __init__(self, x, y, tracked_fields=()):
        self._x0, self._y0 = np.array(x, dtype=np.float64), np.array(y, dtype=np.float64)
        if self._x0.shape != self._y0.shape or self._x0.ndim not in (1, 2):
            raise _lib.SwmhdError(f"LagrangianParticles: x {self._x0.shape} and y {self._y0.shape}: two arrays of one length P")
        self.tracked_fields = (tracked_fields,) if isinstance(tracked_fields, str) else tuple(tracked_fields)
        self._o = None
        self.x = self.y = self._gx = self._gy = None

    @property
    def P(self):
        return self._x0.shape[-1]

    # --- the constructors' side: checks before anything is allocated, then the device tensors -------------------------------------
    def check(self, grid, names, tracers, members=None, slab=False, ring=False, fused=True):
        """Everything a model refuses about its particles, before it allocates: returns the host positions (x, y) brought into the
        domain."""
        if self._o is not None:
            raise _lib.SwmhdError("LagrangianParticles: these particles belong to another model already")
        if slab:
            raise _lib.SwmhdError("particles on a y-slab decomposition are not supported (SWMHD_ENOTSUP): one rank only")
        if ring:
            raise _lib.SwmhdError("particles with ring= are not supported (SWMHD_ENOTSUP): the slab driver steps the four fields only")
        if not fused:
            raise _lib.SwmhdError("particles need the fused stage kernel (SWMHD_ENOTSUP): fused=False keeps no state for the stage to read")
        for n in self.tracked_fields:
            if n not in tuple(names) + tuple(tracers):
                raise _lib.SwmhdError(f"LagrangianParticles: tracked field {n!r}: one of {' '.join(tuple(names) + tuple(tracers))}")
        tx, ty = grid.topo_codes()
        x = seeded(_positions(self._x0, "x", members), 0, grid, tx == _lib.BOUNDED, "x")
        y = seeded(_positions(self._y0, "y", members), 1, grid, ty == _lib.BOUNDED, "y")
        return x, y

    def bind(self, o, xy, device):
        """Allocate x, y and G- on `device` for the model or ensemble `o`.  G- starts as NaN: it is dead at step boundaries (zeta_1 = 0)."""
        self._o = o
        self.x, self.y = (torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in xy)
        self._gx, self._gy = torch.full_like(self.x, float("nan")), torch.full_like(self.y, float("nan"))

    def state_tensors(self):
        """x, y and G-: what a graph capture saves around its warm-up steps."""
        return [self.x, self.y, self._gx, self._gy]

    # --- the user's side -----------------------------------------------------------------------------------------------------------
    def set(self, x=None, y=None):
        """Replace positions (shapes as the constructor's, folded or refused as there).  The values are folded on the host and copied
        from pageable memory: the call blocks the host until the copy is done; it is ordered with the current stream on the device."""
        o = self._o
        tx, ty = o.grid.topo_codes()
        members = getattr(o, "members", None)
        for v, axis, t, bounded in ((x, 0, self.x, tx == _lib.BOUNDED), (y, 1, self.y, ty == _lib.BOUNDED)):
            if v is None:
                continue
            a = seeded(_positions(v, "xy"[axis], members), axis, o.grid, bounded, "xy"[axis])
            if a.shape != tuple(t.shape):
                raise _lib.SwmhdError(f"LagrangianParticles.set: {'xy'[axis]} has shape {a.shape}, the particles {tuple(t.shape)}")
            t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        return self

    def _call_head(self, o):
        """(is an ensemble, flags, (Nx, Ny, Hx, Hy, stride_y, x0, y0, dx, dy)) of a particle call on `o` as it stands now: the periodic
        images where the step leaves the halos stale, the parent's filled halo elsewhere; a Bounded direction reflects."""
        g = o.grid
        ens = getattr(o, "members", None) is not None
        bounded = getattr(o, "_bounded", (False, False))
        flags = (_lib.STRICT if o.strict else _lib.FAST) | o._rwrap
        flags |= (_lib.BOUNDED_X if bounded[0] else 0) | (_lib.BOUNDED_Y if bounded[1] else 0)
        sy = o._state[0].stride(1) if ens else o._raw_fields[0].stride_y
        return ens, flags, (g.Nx, g.Ny, g.Hx, g.Hy, sy, float(g.x[0]), float(g.y[0]), g.dx, g.dy)

    def launch(self, o, dt, stage):
        """Enqueue the particles' launch of RK3 stage `stage` (shared.finish_stage: after the corrections, BEFORE the sets are swapped,
        so o._state is the state the stage started from), with the stage's own (gamma, zeta) -- never the anchor operands.  dt None: an
        ensemble's parameter table."""
        ens, flags, grid = self._call_head(o)
        q = [t.data_ptr() for t in o._state[:3]] if ens else [f.ptr for f in o._raw_fields[:3]]
        head = (*q, self.x.data_ptr(), self.y.data_ptr(), self._gx.data_ptr(), self._gy.data_ptr(), self.P)
        tail = (RK3_GAMMA[stage], RK3_ZETA[stage], flags, _stream_ptr())
        if ens:
            f = getattr(o._L, f"swmhd_ensemble_particles_rk3_{o.sfx}")
            params = o.parameters.data_ptr() if dt is None else None
            rc = f(*head, o.members, o.stride_m, *grid, o.form_code, params, 1.0 if dt is None else dt, *tail)
        else:
            f = getattr(o._L, f"swmhd_particles_rk3_{o.sfx}")
            rc = f(*head, *grid, o.form_code, dt, *tail)
        _lib.check(rc, "swmhd_particles_rk3")

    def sample(self, names=None, out=None):
        """The fields `names` (default: tracked_fields) of the model's current state interpolated to the positions: the float64 device
        tensor (len(names), P), with a leading `members` axis on an ensemble.  Names: the model's four prognostic names and its
        tracers, as they are stored (uh is uh).  Enqueues only."""
        o = self._o
        names = self.tracked_fields if names is None else ((names,) if isinstance(names, str) else tuple(names))
        if not names:
            raise _lib.SwmhdError("LagrangianParticles.sample: no names")
        ens, flags, grid = self._call_head(o)
        known = tuple(o.names) + tuple(o.tracer_names)
        ptrs, locs = [], []
        for n in names:
            if n not in known:
                raise _lib.SwmhdError(f"LagrangianParticles.sample: {n!r}: one of {' '.join(known)}")
            k = known.index(n)
            if ens:
                t = o._state[k] if k < 4 else o._tr[n]
                ptrs.append(t.data_ptr())
            else:
                ptrs.append((o._state[n] if k < 4 else o._tr[n]).ptr)
            # u | uh: (Face, Center); v | vh: (Center, Face); everything else at the centres
            locs.append(_lib.PARTICLES_CENTER_Y if k == 0 else (_lib.PARTICLES_CENTER_X if k == 1 else _lib.PARTICLES_CENTER_X | _lib.PARTICLES_CENTER_Y))
        shape = lead_shape(o) + (len(names), self.P)
        if out is None:
            out = torch.empty(shape, dtype=torch.float64, device=self.x.device)
        elif not (out.is_cuda and out.dtype == torch.float64 and tuple(out.shape) == shape and out.is_contiguous()):
            raise _lib.SwmhdError(f"LagrangianParticles.sample: out must be a contiguous float64 CUDA tensor of shape {shape}")
        cap = _lib.PARTICLES_MAX_FIELDS
        if len(names) > cap and ens:
            raise _lib.SwmhdError(f"LagrangianParticles.sample: at most {cap} names per call on an ensemble")
        for k0 in range(0, len(names), cap):
            n = min(cap, len(names) - k0)
            args = (_lib.ptr_array(ptrs[k0:k0 + n]), (ctypes.c_int * n)(*locs[k0:k0 + n]), n, self.x.data_ptr(), self.y.data_ptr(),
                    out.data_ptr() + 8 * k0 * self.P, self.P)
            if ens:
                rc = getattr(o._L, f"swmhd_ensemble_particles_sample_{o.sfx}")(*args, o.members, o.stride_m, *grid, flags, _stream_ptr())
            else:
                rc = getattr(o._L, f"swmhd_particles_sample_{o.sfx}")(*args, *grid, flags, _stream_ptr())
            _lib.check(rc, "swmhd_particles_sample")
        return out


def check_particles(particles, grid, names, tracers, members=None, slab=False, ring=False, fused=True):
    """`particles=` of a constructor, before anything is allocated: None, or the host positions of a LagrangianParticles."""
    if particles is None:
        return None
    if not isinstance(particles, LagrangianParticles):
        raise _lib.SwmhdError(f"particles: a LagrangianParticles, not {type(particles).__name__}")
    return particles.check(grid, names, tracers, members, slab, ring, fused)


class ParticleTimeSeries(DeviceTimeSeries):
    """A writer of particle samples for run(): `capacity` samples of `names` in one float64 device tensor, plus the host lists `times`
    and `iterations`.  samples: (capacity, len(names), P); for an ensemble (capacity, members, len(names), P).  Names: "x" and "y" are
    the positions, every other name a field sampled at them (LagrangianParticles.sample).  The tensor is allocated when the first
    sample is written.  `write` only enqueues; `numpy` and `save` are the calls that synchronise."""

    _data, _unit = "samples", "samples"
    samples = DeviceTimeSeries.tensor

    def __init__(self, model, names=("x", "y", "A"), schedule=TimeInterval(0.1), capacity=None):
        super().__init__(model, names, schedule, capacity)

    def _check_names(self):
        p = getattr(self.model, "particles", None)
        if p is None:
            raise _lib.SwmhdError("ParticleTimeSeries: the model has no particles")
        if not self.names:
            raise _lib.SwmhdError("ParticleTimeSeries: no names")
        known = tuple(self.model.names) + tuple(self.model.tracer_names)
        for n in self.names:
            if n not in POSITION_NAMES and n not in known:
                raise _lib.SwmhdError(f"ParticleTimeSeries: {n!r}: x, y or one of {' '.join(known)}")

    def _sample_shape(self):
        return lead_shape(self.model) + (len(self.names), self.model.particles.P)

    def _enqueue(self, out):
        p = self.model.particles
        tracked = [n for n in self.names if n not in POSITION_NAMES]
        values = p.sample(tracked) if tracked else None
        for k, n in enumerate(self.names):
            row = out.select(-2, k)
            row.copy_(p.x if n == "x" else (p.y if n == "y" else values.select(-2, tracked.index(n))))

    def save(self, path):
        """One .npz: samples, names, times, iterations and the grid extents (synchronises)."""
        g = self.model.grid
        self._savez(path, size=np.array([g.Nx, g.Ny]), x_extent=np.array(g.x, dtype=np.float64), y_extent=np.array(g.y, dtype=np.float64))
