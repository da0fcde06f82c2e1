"""Zonal means and the writer that collects them on the device.

What a channel run is read for are its x-averaged profiles (Oceananigans: Average(u, dims = 1) handed to an output writer): the mean
flow and the mean potential, and the stresses and fluxes that drive them -- <uv> (Reynolds), <B_x B_y> (Maxwell), <vA>, whose
y-derivative is the whole right-hand side of dĀ/dt.  `zonal_means` (a method of ShallowWaterModel and of the ensembles) enqueues ONE
kernel (swmhd_zonal_means_*, include/swmhd_zonal.h) that reduces the named quantities of every row along x, for all members of an ensemble,
into a float64 device tensor, without a frame-sized buffer and without a host synchronisation.  ZonalMeanTimeSeries speaks the writer
protocol of swmhd_amd.output.run().  Averages along y or over time, zonal means of tracers and eddy quantities are out of scope: the
eddy stress <u'v'> = <uv> - <u><v> is the user's subtraction (it cancels where the eddies are weak: |<u'v'>| << |<u><v>| loses that
many digits of the two float64 profiles).
"""
import torch

from . import _lib
from .fields import _stream_ptr
from .output import TimeInterval

DEFAULT_NAMES = ("u", "v", "A")


def _runs(names, tracers=()):
    """The profiles as launches: the kernel writes the profiles of a mask in bit order (u v h A s B_x B_y uu vv uv B_xB_x B_yB_y B_xB_y
    vA), so `names` is cut into runs that ascend in that order, as output._runs cuts a frame -- one launch for any ascending list, and
    any order or repetition of names is honoured."""
    runs = []
    for n in names:
        if n in tracers:
            raise _lib.SwmhdError(f"zonal mean {n!r} is a tracer: profiles are {' '.join(_lib.ZM_BITS)} only")
        if n not in _lib.ZM_BITS:
            raise _lib.SwmhdError(f"zonal mean {n!r}: one of {' '.join(_lib.ZM_BITS)} (velocities u, v also for the conservative model)")
        bit = _lib.ZM_BITS[n]
        if runs and bit > runs[-1][-1]:
            runs[-1].append(bit)
        else:
            runs.append([bit])
    if not runs:
        raise _lib.SwmhdError("zonal_means: no names")
    return runs


def profile_shape(model, names):
    members = getattr(model, "members", None)
    return ((members,) if members is not None else ()) + (len(names), model.grid.Ny)


def enqueue_zonal_means(model, names=DEFAULT_NAMES, out=None):
    """ShallowWaterModel.zonal_means / ShallowWaterEnsemble.zonal_means: see there."""
    names = tuple(names)
    runs = _runs(names, getattr(model, "tracer_names", ()))
    ens = getattr(model, "members", None) is not None
    g = model.grid
    if ens:
        q = model._state                  # (whichever set of tensors is the state NOW: the ping-pong roles flip every stage)
        ptrs, sy, dev = [t.data_ptr() for t in q], q[0].stride(1), q[0].device
    else:
        model._join()                     # a ring exchange of this state may still be in flight
        q = model._raw_fields
        ptrs, sy, dev = [f.ptr for f in q], q[0].stride_y, q[0].data.device
    shape = profile_shape(model, names)
    if out is None:
        out = torch.empty(shape, dtype=torch.float64, device=dev)
    elif not (out.is_cuda and out.dtype == torch.float64 and tuple(out.shape) == shape and out.stride(-1) == 1):
        raise _lib.SwmhdError(f"zonal_means: out must be a float64 CUDA tensor of shape {shape} with unit stride in y")
    flags = model._rwrap                  # as enqueue_frame: the periodic images where the step leaves the halos stale
    sfx = model.sfx
    k = 0
    for bits in runs:
        which = sum(bits)
        first = out.select(-2, k)
        if ens:
            f = getattr(model._L, f"swmhd_ensemble_zonal_means_{sfx}")
            rc = f(*ptrs, model.members, model.stride_m, g.Nx, g.Ny, g.Hx, g.Hy, sy, g.dx, g.dy, model.form_code, 0, g.Ny, which,
                   first.data_ptr(), out.stride(-2), out.stride(0), flags, _stream_ptr())
        else:
            f = getattr(model._L, f"swmhd_zonal_means_{sfx}")
            rc = f(*ptrs, g.Nx, g.Ny, g.Hx, g.Hy, sy, g.dx, g.dy, model.form_code, 0, g.Ny, which,
                   first.data_ptr(), out.stride(-2), flags, _stream_ptr())
        _lib.check(rc, "swmhd_zonal_means")
        k += len(bits)
    return out


class ZonalMeanTimeSeries:
    """A writer of x-averaged profiles for run(): `capacity` samples of `names` in one float64 device tensor, plus the host lists
    `times` and `iterations`.  profiles: (capacity, len(names), Ny); for an ensemble (capacity, members, len(names), Ny); on a y-slab
    the rank's own rows.  Names: u v h A s B_x B_y uu vv uv B_xB_x B_yB_y B_xB_y vA (include/swmhd_zonal.h).

    A sample is members x len(names) x Ny doubles, where a frame is that times Nx.  The tensor is allocated when the first sample is
    written.  `write` only enqueues; `numpy` and `save` are the calls that synchronise."""

    def __init__(self, model, names=DEFAULT_NAMES, schedule=TimeInterval(0.1), capacity=None):
        self.model, self.names, self.schedule = model, tuple(names), schedule
        _runs(self.names, getattr(model, "tracer_names", ()))
        if capacity is None or int(capacity) < 1:
            raise _lib.SwmhdError("ZonalMeanTimeSeries: capacity (samples) must be given: the profiles stay on the device")
        self.capacity = int(capacity)
        self.times, self.iterations = [], []
        self._profiles = None

    def __len__(self):
        return len(self.times)

    @property
    def profiles(self):
        """The device tensor of all `capacity` slots; the first len(self) hold samples."""
        if self._profiles is None:
            m = self.model
            dev = m._state[0].device if getattr(m, "members", None) is not None else m._raw_fields[0].data.device
            self._profiles = torch.empty((self.capacity,) + profile_shape(m, self.names), dtype=torch.float64, device=dev)
        return self._profiles

    def write(self, time=None):
        """Enqueue the profiles of the model's current state into the next slot."""
        k = len(self.times)
        if k >= self.capacity:
            raise _lib.SwmhdError(f"ZonalMeanTimeSeries: all {self.capacity} slots are written")
        enqueue_zonal_means(self.model, self.names, out=self.profiles[k])
        self.times.append(self.model.clock_time if time is None else time)
        self.iterations.append(self.model.iteration)

    def numpy(self):
        """The samples written so far as a host array (synchronises)."""
        return self.profiles[:len(self.times)].cpu().numpy()

    def save(self, path):
        """One .npz: profiles, names, times, iterations, the y coordinates of the rows at cell centres (u h A s B_y ...) and at faces
        (v B_x vA ...), and the slab's row offset (synchronises)."""
        import numpy as np
        g = self.model.grid
        rows = slice(g.Hy, g.Hy + g.Ny)
        np.savez(path, profiles=self.numpy(), names=np.array(self.names), times=np.array(self.times, dtype=np.float64),
                 iterations=np.array(self.iterations, dtype=np.int64), yc=np.array(g.yc[rows], dtype=np.float64),
                 yf=np.array(g.yf[rows], dtype=np.float64), j_offset=g.j_offset, Ny_global=g.Ny_global)
