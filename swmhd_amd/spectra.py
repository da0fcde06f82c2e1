"""Zonal wavenumber spectra and the writer that collects them on the device.

An instability run is read by the growth of single zonal wavenumbers of v and A, a turbulent run by how kinetic and magnetic energy
spread over wavenumber.  `zonal_spectra` (a method of ShallowWaterModel and of the ensembles) enqueues two kernels
(swmhd_zonal_spectra_*, include/swmhd_spectra.h) that transform every row of the named frame fields along x by a double-precision FFT
held in LDS and average |F^[k]|^2 over the rows into a float64 device tensor of Nx/2 + 1 entries per field:
    P_F[k] = mean over rows of c_k |(1/Nx) sum_i F(i,j) exp(-2 pi i k (i-1)/Nx)|^2,   c_k = 1 at k = 0 and k = Nx/2, else 2,
so that sum_k P_F[k] is the mean of F^2 (Parseval).  No frame-sized buffer, no FFT library, no host synchronisation.
ZonalSpectrumTimeSeries speaks the writer protocol of swmhd_amd.output.run().

Error: per row |got - p[k]| <= c_k (2 |F^[k]| eps sqrt(S) + eps^2 S), S the row's mean square, eps = eta log2(Nx) 2^-53 with eta = 9.66:
Higham's radix-2 constant mu + gamma_4 (sqrt(2) + mu) (Accuracy and Stability of Numerical Algorithms, Thm 24.2) for the kernel's
butterfly y1 = (a - b) w -- one rounding of the difference, sqrt(2) gamma_2 of the unfused complex product -- with twiddles taken from
sincospi of the exact fraction 2k/Nx (2 ulp per component: mu = 4 * 2^-53), never from a recurrence; the half-length transform's two
trivial stages, the untangling pass and re^2 + im^2 fit into the log2(Nx) stages counted (include/swmhd_spectra.h has the account).

2-D and isotropic spectra: swmhd_amd.spectra2d.  Not built: spectra along y alone, cross- and co-spectra, per-row spectra, sizes other than 2^p (4 .. 4096),
tracers, and the slab-global average -- on y-slabs each rank gets the spectrum of its own rows, and the global one is the row-weighted
mean of the ranks', the caller's to form.  The kinetic-energy spectrum (P_u + P_v)/2 and the magnetic one are the user's sums.
"""
import math

import torch

from . import _lib
from ._series import DeviceTimeSeries, cached_workspace, cut_runs, lead_shape, out_tensor, state_pointers
from .fields import _stream_ptr
from .output import TimeInterval

DEFAULT_NAMES = ("u", "v", "A")
_MESSAGES = (f"zonal spectrum {{n!r}} is a tracer: spectra are {' '.join(_lib.ZS_BITS)} only",
             f"zonal spectrum {{n!r}}: one of {' '.join(_lib.ZS_BITS)} (velocities u, v also for the conservative model)", "zonal_spectra: no names")


def _runs(names, tracers=()):
    """The spectra as launches (cut_runs): bit order u v h A s B_x B_y."""
    return cut_runs(names, _lib.ZS_BITS, tracers, _MESSAGES)


def _check(model, names):
    """What is refused before anything is allocated: names, a Bounded x direction, an unsupported Nx.  Returns the runs."""
    runs = _runs(names, getattr(model, "tracer_names", ()))
    g = model.grid
    if g.topology[0] != "Periodic":
        raise _lib.SwmhdError("zonal_spectra: the x direction is Bounded: a DFT of a non-periodic row is not a spectrum")
    Nx = g.Nx
    if Nx < _lib.SPECTRA_MIN_NX or Nx > _lib.SPECTRA_MAX_NX or Nx & (Nx - 1):
        raise _lib.SwmhdError(f"zonal_spectra: Nx = {Nx}: a power of two from {_lib.SPECTRA_MIN_NX} to {_lib.SPECTRA_MAX_NX} is supported")
    return runs


def spectrum_shape(model, names):
    return lead_shape(model) + (len(names), model.grid.Nx // 2 + 1)


def enqueue_zonal_spectra(model, names=DEFAULT_NAMES, out=None):
    """ShallowWaterModel.zonal_spectra / ShallowWaterEnsemble.zonal_spectra: see there."""
    names = tuple(names)
    runs = _check(model, names)
    g = model.grid
    ptrs, sy, dev, ens = state_pointers(model)
    out = out_tensor(out, spectrum_shape(model, names), (torch.float64,), dev, "zonal_spectra", "k")
    # (the workspace: what the C function states for the largest run asked for so far)
    need = model._L.swmhd_zonal_spectra_workspace(g.Nx, g.Ny, max(len(bits) for bits in runs), getattr(model, "members", None) or 1)
    ws = cached_workspace(model, "_spectra_ws", need, dev)
    flags = model._rwrap                  # as enqueue_frame: the periodic images where the step leaves the halos stale
    sfx = model.sfx
    k = 0
    for bits in runs:                     # (the runs share the workspace: launches on one stream run one after the other)
        which = sum(bits)
        first = out.select(-2, k)
        if ens:
            f = getattr(model._L, f"swmhd_ensemble_zonal_spectra_{sfx}")
            rc = f(*ptrs, model.members, model.stride_m, g.Nx, g.Ny, g.Hx, g.Hy, sy, g.dx, g.dy, model.form_code, 0, g.Ny, which,
                   ws.data_ptr(), first.data_ptr(), out.stride(-2), out.stride(0), flags, _stream_ptr())
        else:
            f = getattr(model._L, f"swmhd_zonal_spectra_{sfx}")
            rc = f(*ptrs, g.Nx, g.Ny, g.Hx, g.Hy, sy, g.dx, g.dy, model.form_code, 0, g.Ny, which,
                   ws.data_ptr(), first.data_ptr(), out.stride(-2), flags, _stream_ptr())
        _lib.check(rc, "swmhd_zonal_spectra")
        k += len(bits)
    return out


class ZonalSpectrumTimeSeries(DeviceTimeSeries):
    """A writer of zonal spectra for run(): `capacity` samples of `names` in one float64 device tensor, plus the host lists `times` and
    `iterations`.  spectra: (capacity, len(names), Nx/2 + 1); for an ensemble (capacity, members, len(names), Nx/2 + 1); on a y-slab the
    spectrum of the rank's own rows.  Names: u v h A s B_x B_y (include/swmhd_spectra.h).

    The tensor is allocated when the first sample is written.  `write` only enqueues; `numpy` and `save` are the calls that
    synchronise."""

    _data, _unit = "spectra", "samples"
    spectra = DeviceTimeSeries.tensor

    def __init__(self, model, names=DEFAULT_NAMES, schedule=TimeInterval(0.1), capacity=None):
        super().__init__(model, names, schedule, capacity)

    def _check_names(self):
        _check(self.model, self.names)

    def _sample_shape(self):
        return spectrum_shape(self.model, self.names)

    def _enqueue(self, out):
        enqueue_zonal_spectra(self.model, self.names, out=out)

    def save(self, path):
        """One .npz: spectra, names, times, iterations, the integer wavenumbers k = 0 .. Nx/2 and kx = 2 pi k / Lx (synchronises)."""
        import numpy as np
        g = self.model.grid
        k = np.arange(g.Nx // 2 + 1, dtype=np.int64)
        self._savez(path, k=k, kx=2.0 * math.pi * k / g.Lx)
