"""Output frames and the writer that collects them on the device.

The reference's run loop does three things per iteration: it steps the model, writes the energies, and every 0.1 time units writes
the FIELDS (u, v, A, s), s = sqrt(u^2 + v^2):
    JLD2OutputWriter(model, (; u, v, A = model.tracers.A, s), schedule = TimeInterval(0.1))   jacobian_formulation/SWMHD_example.jl:67-68,80-84
    the same with u = uh / h, v = vh / h                                                      divergence_formulation/divergence_sw_mhd.jl:64-66,75-82
Its movies are made of those frames, and MHD_visualize.jl:55-65 looks at B_x = -dA/dy / h, B_y = dA/dx / h.

`output_fields` (a method of ShallowWaterModel and of the ensembles) enqueues ONE kernel (swmhd_output_fields_*, include/swmhd.h) that
writes the selected fields -- derived ones included, halo-stripped, in the writer's element type, for all members of an ensemble --
into a device tensor, without a host synchronisation.  FieldTimeSeries + run() are the writer and the run loop around it.  File
formats and plotting stay out of scope: `FieldTimeSeries.save` writes one .npz.
"""
from dataclasses import dataclass

import torch

from . import _lib
from ._series import DeviceTimeSeries, cut_runs, lead_shape, out_tensor, state_pointers
from .derived import ELEM_TYPES, TRACER_MESSAGE, check_coriolis_names, launch as launch_derived
from .fields import _stream_ptr

DEFAULT_NAMES = ("u", "v", "A", "s")    # the reference's writer
_MESSAGES = (TRACER_MESSAGE, f"output field {{n!r}}: one of {' '.join(_lib.OUT_BITS)} (velocities u, v also for the conservative model); "
             f"frames also take the derived fields {' '.join(_lib.DRV_BITS)}", "output_fields: no field names")


def _runs(names, tracers=()):
    """The frame's fields as launches (cut_runs): bit order u v h A s B_x B_y -- one launch for the default frame."""
    return cut_runs(names, _lib.OUT_BITS, tracers, _MESSAGES)


def _frame_runs(names, tracers=()):
    """[(derived, bits)]: `names` as launches where the derived fields of swmhd_amd.derived (vorticity divergence current
    potential_vorticity) stand among the seven of the frame: a run also ends where the kernel changes.  Without a derived name these
    are the runs of _runs, refusals included."""
    if not any(n in _lib.DRV_BITS and n not in tracers for n in names):
        return [(False, bits) for bits in _runs(names, tracers)]
    runs = []
    for n in names:
        drv = n in _lib.DRV_BITS and n not in tracers
        if not drv:
            _runs((n,), tracers)          # (refuses a tracer or an unknown name, with the frame's message)
        bit = (_lib.DRV_BITS if drv else _lib.OUT_BITS)[n]
        if runs and runs[-1][0] == drv and bit > runs[-1][1][-1]:
            runs[-1][1].append(bit)
        else:
            runs.append((drv, [bit]))
    return runs


def frame_shape(model, names):
    return lead_shape(model) + (len(names), model.grid.Ny, model.grid.Nx)


def enqueue_frame(model, names=DEFAULT_NAMES, out=None, array_type=torch.float32):
    """ShallowWaterModel.output_fields / ShallowWaterEnsemble.output_fields: see there."""
    names = tuple(names)
    runs = _frame_runs(names, getattr(model, "tracer_names", ()))
    check_coriolis_names(model, names)
    g = model.grid
    ptrs, sy, dev, ens = state_pointers(model)
    out = out_tensor(out, frame_shape(model, names), ELEM_TYPES, dev, "output_fields", "x", array_type)
    # The model steps with SWMHD_WRAP_* exactly where its halos may be stale (_rwrap): the kernel then reads the periodic image
    # itself, so a frame needs no halo fill in front of it.  Everywhere else the halos are kept current by the step.
    flags = model._rwrap
    sfx = model.sfx
    k = 0
    for derived, bits in runs:
        which = sum(bits)
        first = out.select(-3, k)
        if derived:                       # (the kernel of swmhd_amd.derived: same frame layout, same flags)
            launch_derived(model, ptrs, sy, ens, which, first, out)
            k += len(bits)
            continue
        if ens:
            f = getattr(model._L, f"swmhd_ensemble_output_fields_{sfx}")
            rc = f(*ptrs, model.members, model.stride_m, g.Nx, g.Ny, g.Hx, g.Hy, sy, g.dx, g.dy, model.form_code, 0, g.Ny, which,
                   first.data_ptr(), out.element_size(), out.stride(-2), out.stride(-3), out.stride(0), flags, _stream_ptr())
        else:
            f = getattr(model._L, f"swmhd_output_fields_{sfx}")
            rc = f(*ptrs, g.Nx, g.Ny, g.Hx, g.Hy, sy, g.dx, g.dy, model.form_code, 0, g.Ny, which,
                   first.data_ptr(), out.element_size(), out.stride(-2), out.stride(-3), flags, _stream_ptr())
        _lib.check(rc, "swmhd_output_fields")
        k += len(bits)
    return out


# --- schedules (Oceananigans.Utils: TimeInterval, IterationInterval) ----------------------------------------------------------
def _whole(ratio, what):
    n = round(ratio)
    if n < 1 or abs(ratio - n) > 1e-9 * max(1.0, abs(ratio)):
        raise _lib.SwmhdError(f"{what} = {ratio!r} is not a whole number of time steps: this engine runs a fixed dt "
                              "(Oceananigans would shorten a step to land on the time; choose an interval that dt divides)")
    return int(n)


@dataclass(frozen=True)
class IterationInterval:
    interval: int

    def steps(self, dt):
        if int(self.interval) != self.interval or self.interval < 1:
            raise _lib.SwmhdError(f"IterationInterval({self.interval!r}): a positive whole number of iterations")
        return int(self.interval)


@dataclass(frozen=True)
class TimeInterval:
    """TimeInterval(T) with the fixed dt of this engine is IterationInterval(round(T / dt)); T / dt must be whole to 1e-9."""
    interval: float

    def steps(self, dt):
        return _whole(self.interval / dt, f"TimeInterval({self.interval!r}) / dt")


def frame_iterations(schedule, dt, nsteps):
    """Iterations (counted from the start of a run of `nsteps` steps) at which `schedule` writes: 0, n, 2n, ... <= nsteps."""
    n = schedule.steps(dt)
    return list(range(0, nsteps + 1, n))


class FieldTimeSeries(DeviceTimeSeries):
    """The reference's field writer on the device: `capacity` frames of `names` in one tensor, plus the host lists `times` and
    `iterations`.  frames: (capacity, len(names), Ny, Nx); for an ensemble (capacity, members, len(names), Ny, Nx); on a y-slab the
    rank's own rows.  Names: u v h A s B_x B_y (velocities also for the conservative model, which stores uh, vh) and, in any mixture
    with them, the derived fields vorticity divergence current potential_vorticity (swmhd_amd.derived: a kernel of their own, so a
    launch ends where the kernel changes).

    array_type defaults to float32.  That default is this library's: the reference's field writer was given no array type and its
    NetCDF writer (the energies) is the one that asks for Array{Float64}; what Oceananigans' JLD2 writer stores unasked is
    library-internal and unpinned here, like the rest of assumption A9.  Pass torch.float64 for exact frames.

    The tensor (capacity x frame bytes: 268 MB per 4096^2 float32 frame of four fields) is allocated when the first frame is written.
    `write` only enqueues; `numpy` and `save` are the calls that synchronise."""

    _data, _unit = "frames", "frames"
    frames = DeviceTimeSeries.tensor

    def __init__(self, model, names=DEFAULT_NAMES, schedule=TimeInterval(0.1), capacity=None, array_type=torch.float32):
        self.array_type = self.dtype = array_type
        super().__init__(model, names, schedule, capacity)

    def _check_names(self):
        _frame_runs(self.names, getattr(self.model, "tracer_names", ()))
        check_coriolis_names(self.model, self.names)
        if self.array_type not in ELEM_TYPES:
            raise _lib.SwmhdError(f"array_type {self.array_type}: torch.float32 or torch.float64")

    def _sample_shape(self):
        return frame_shape(self.model, self.names)

    def _enqueue(self, out):
        enqueue_frame(self.model, self.names, out=out)

    def save(self, path):
        """One .npz: frames, names, times, iterations and the grid extents (synchronises)."""
        import numpy as np
        g = self.model.grid
        self._savez(path, size=np.array([g.Nx, g.Ny]), x=np.array(g.x, dtype=np.float64), y=np.array(g.y, dtype=np.float64),
                    j_offset=g.j_offset, Ny_global=g.Ny_global)


def run(model, dt, stop_time=None, stop_iteration=None, writers=()):
    """run!(simulation): step `model` (a ShallowWaterModel or an ensemble) to stop_time or stop_iteration with the writers attached.
    Every writer gets a frame of the state the run starts from (as Oceananigans' writers do at iteration 0) and then one whenever its
    schedule is due: model.time_steps(n, dt) -- graph replays when a graph was captured for dt -- followed by one output_fields launch.
    Nothing here synchronises with the device.  Refuses up front (SwmhdError, before any step) when a writer's capacity is too small.
    An ensemble with per-member g and f runs here under a scalar dt; a per-member dt is refused."""
    if isinstance(dt, (list, tuple)) or getattr(dt, "ndim", 0) > 0:
        raise _lib.SwmhdError("run: a per-member dt is not supported (schedules in time units across members whose clocks diverge); "
                              "step the ensemble with time_steps(n, dts) and write frames by iteration")
    if (stop_time is None) == (stop_iteration is None):
        raise _lib.SwmhdError("run: give stop_time or stop_iteration")
    it0, t0 = model.iteration, model.clock_time
    if stop_iteration is not None:
        nsteps = int(stop_iteration) - it0
    else:
        ratio = (stop_time - t0) / dt
        nsteps = 0 if abs(ratio) <= 1e-9 else _whole(ratio, "(stop_time - time) / dt")
    if nsteps < 0:
        raise _lib.SwmhdError("run: the model is already past the stop")
    plans = []
    for w in writers:
        due = frame_iterations(w.schedule, dt, nsteps)
        if w.iterations and w.iterations[-1] == it0:
            due = due[1:]                               # a continued run: this state is in the series already
        if len(w) + len(due) > w.capacity:
            raise _lib.SwmhdError(f"FieldTimeSeries capacity {w.capacity} < {len(w) + len(due)} frames: this run writes {len(due)} "
                                  f"({nsteps} steps, one frame every {w.schedule.steps(dt)}) on top of {len(w)}")
        plans.append((w, set(due)))
    done = 0
    while True:
        for w, due in plans:
            if done in due:
                w.write(time=t0 + done * dt)
        if done == nsteps:
            break
        nxt = min([min((k for k in due if k > done), default=nsteps) for _, due in plans] + [nsteps])
        model.time_steps(nxt - done, dt)
        done = nxt
    return model
