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
from .fields import _stream_ptr
from .output import TimeInterval

DEFAULT_NAMES = ("u", "v", "A")


def _runs(names, tracers=()):
    """The spectra as launches: the kernels write the spectra of a mask in bit order (u v h A s B_x B_y), so `names` is cut into runs
    that ascend in that order, as zonal._runs cuts the profiles: any order or repetition of names is honoured."""
    runs = []
    for n in names:
        if n in tracers:
            raise _lib.SwmhdError(f"zonal spectrum {n!r} is a tracer: spectra are {' '.join(_lib.ZS_BITS)} only")
        if n not in _lib.ZS_BITS:
            raise _lib.SwmhdError(f"zonal spectrum {n!r}: one of {' '.join(_lib.ZS_BITS)} (velocities u, v also for the conservative model)")
        bit = _lib.ZS_BITS[n]
        if runs and bit > runs[-1][-1]:
            runs[-1].append(bit)
        else:
            runs.append([bit])
    if not runs:
        raise _lib.SwmhdError("zonal_spectra: no names")
    return runs


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
    members = getattr(model, "members", None)
    return ((members,) if members is not None else ()) + (len(names), model.grid.Nx // 2 + 1)


def _workspace(model, nfields, dev):
    """The cached device workspace of a model: grown to what the C function states for the largest run asked for so far."""
    g = model.grid
    need = model._L.swmhd_zonal_spectra_workspace(g.Nx, g.Ny, nfields, getattr(model, "members", None) or 1)
    ws = getattr(model, "_spectra_ws", None)
    if ws is None or ws.numel() < need or ws.device != dev:
        ws = torch.empty((need,), dtype=torch.float64, device=dev)
        model._spectra_ws = ws
    return ws


def enqueue_zonal_spectra(model, names=DEFAULT_NAMES, out=None):
    """ShallowWaterModel.zonal_spectra / ShallowWaterEnsemble.zonal_spectra: see there."""
    names = tuple(names)
    runs = _check(model, names)
    ens = getattr(model, "members", None) is not None
    g = model.grid
    if ens:
        q = model._state                  # (whichever set of tensors is the state NOW: the ping-pong roles flip every stage)
        ptrs, sy, dev = [t.data_ptr() for t in q], q[0].stride(1), q[0].device
    else:
        model._join()                     # a ring exchange of this state may still be in flight
        q = model._raw_fields
        ptrs, sy, dev = [f.ptr for f in q], q[0].stride_y, q[0].data.device
    shape = spectrum_shape(model, names)
    if out is None:
        out = torch.empty(shape, dtype=torch.float64, device=dev)
    elif not (out.is_cuda and out.dtype == torch.float64 and tuple(out.shape) == shape and out.stride(-1) == 1):
        raise _lib.SwmhdError(f"zonal_spectra: out must be a float64 CUDA tensor of shape {shape} with unit stride in k")
    ws = _workspace(model, max(len(bits) for bits in runs), dev)
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


class ZonalSpectrumTimeSeries:
    """A writer of zonal spectra for run(): `capacity` samples of `names` in one float64 device tensor, plus the host lists `times` and
    `iterations`.  spectra: (capacity, len(names), Nx/2 + 1); for an ensemble (capacity, members, len(names), Nx/2 + 1); on a y-slab the
    spectrum of the rank's own rows.  Names: u v h A s B_x B_y (include/swmhd_spectra.h).

    The tensor is allocated when the first sample is written.  `write` only enqueues; `numpy` and `save` are the calls that
    synchronise."""

    def __init__(self, model, names=DEFAULT_NAMES, schedule=TimeInterval(0.1), capacity=None):
        self.model, self.names, self.schedule = model, tuple(names), schedule
        _check(model, self.names)
        if capacity is None or int(capacity) < 1:
            raise _lib.SwmhdError("ZonalSpectrumTimeSeries: capacity (samples) must be given: the spectra stay on the device")
        self.capacity = int(capacity)
        self.times, self.iterations = [], []
        self._spectra = None

    def __len__(self):
        return len(self.times)

    @property
    def spectra(self):
        """The device tensor of all `capacity` slots; the first len(self) hold samples."""
        if self._spectra is None:
            m = self.model
            dev = m._state[0].device if getattr(m, "members", None) is not None else m._raw_fields[0].data.device
            self._spectra = torch.empty((self.capacity,) + spectrum_shape(m, self.names), dtype=torch.float64, device=dev)
        return self._spectra

    def write(self, time=None):
        """Enqueue the spectra of the model's current state into the next slot."""
        k = len(self.times)
        if k >= self.capacity:
            raise _lib.SwmhdError(f"ZonalSpectrumTimeSeries: all {self.capacity} slots are written")
        enqueue_zonal_spectra(self.model, self.names, out=self.spectra[k])
        self.times.append(self.model.clock_time if time is None else time)
        self.iterations.append(self.model.iteration)

    def numpy(self):
        """The samples written so far as a host array (synchronises)."""
        return self.spectra[:len(self.times)].cpu().numpy()

    def save(self, path):
        """One .npz: spectra, names, times, iterations, the integer wavenumbers k = 0 .. Nx/2 and kx = 2 pi k / Lx (synchronises)."""
        import numpy as np
        g = self.model.grid
        k = np.arange(g.Nx // 2 + 1, dtype=np.int64)
        np.savez(path, spectra=self.numpy(), names=np.array(self.names), times=np.array(self.times, dtype=np.float64),
                 iterations=np.array(self.iterations, dtype=np.int64), k=k, kx=2.0 * math.pi * k / g.Lx)
