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
from ._series import DeviceTimeSeries, cut_runs, lead_shape, out_tensor, state_pointers
from .fields import _stream_ptr
from .output import TimeInterval

DEFAULT_NAMES = ("u", "v", "A")
_MESSAGES = (f"zonal mean {{n!r}} is a tracer: profiles are {' '.join(_lib.ZM_BITS)} only",
             f"zonal mean {{n!r}}: one of {' '.join(_lib.ZM_BITS)} (velocities u, v also for the conservative model)", "zonal_means: no names")


def _runs(names, tracers=()):
    """The profiles as launches (cut_runs): bit order u v h A s B_x B_y uu vv uv B_xB_x B_yB_y B_xB_y vA."""
    return cut_runs(names, _lib.ZM_BITS, tracers, _MESSAGES)


def profile_shape(model, names):
    return lead_shape(model) + (len(names), model.grid.Ny)


def enqueue_zonal_means(model, names=DEFAULT_NAMES, out=None):
    """ShallowWaterModel.zonal_means / ShallowWaterEnsemble.zonal_means: see there."""
    names = tuple(names)
    runs = _runs(names, getattr(model, "tracer_names", ()))
    g = model.grid
    ptrs, sy, dev, ens = state_pointers(model)
    out = out_tensor(out, profile_shape(model, names), (torch.float64,), dev, "zonal_means", "y")
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


class ZonalMeanTimeSeries(DeviceTimeSeries):
    """A writer of x-averaged profiles for run(): `capacity` samples of `names` in one float64 device tensor, plus the host lists
    `times` and `iterations`.  profiles: (capacity, len(names), Ny); for an ensemble (capacity, members, len(names), Ny); on a y-slab
    the rank's own rows.  Names: u v h A s B_x B_y uu vv uv B_xB_x B_yB_y B_xB_y vA (include/swmhd_zonal.h).

    A sample is members x len(names) x Ny doubles, where a frame is that times Nx.  The tensor is allocated when the first sample is
    written.  `write` only enqueues; `numpy` and `save` are the calls that synchronise."""

    _data, _unit = "profiles", "samples"
    profiles = DeviceTimeSeries.tensor

    def __init__(self, model, names=DEFAULT_NAMES, schedule=TimeInterval(0.1), capacity=None):
        super().__init__(model, names, schedule, capacity)

    def _check_names(self):
        _runs(self.names, getattr(self.model, "tracer_names", ()))

    def _sample_shape(self):
        return profile_shape(self.model, self.names)

    def _enqueue(self, out):
        enqueue_zonal_means(self.model, self.names, out=out)

    def save(self, path):
        """One .npz: profiles, names, times, iterations, the y coordinates of the rows at cell centres (u h A s B_y ...) and at faces
        (v B_x vA ...), and the slab's row offset (synchronises)."""
        import numpy as np
        g = self.model.grid
        rows = slice(g.Hy, g.Hy + g.Ny)
        self._savez(path, yc=np.array(g.yc[rows], dtype=np.float64), yf=np.array(g.yf[rows], dtype=np.float64), j_offset=g.j_offset,
                    Ny_global=g.Ny_global)
