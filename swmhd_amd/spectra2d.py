"""2-D and isotropic power spectra and the writer that collects the isotropic ones on the device.

A turbulence run is published by its spectrum over the modulus of the wavenumber, E(|k|): the kinetic and the magnetic cascade, the
inverse cascade of <A^2>; on a beta-plane the full (kx, ky) plane is wanted as well, for the anisotropy of the jets.
`isotropic_spectra` and `power_spectra_2d` (methods of ShallowWaterModel and of the ensembles) enqueue three kernels
(swmhd_spectra2d_*, include/swmhd_spectra2d.h): the row FFT of the zonal spectra keeping its complex modes, a column FFT in LDS, and
the shell sum, all in double:
    P2[kx, ky] = c_kx |1/(Nx Ny) sum_ij F(i,j) exp(-2 pi i (kx (i-1)/Nx + ky (j-1)/Ny))|^2,  kx = 0 .. Nx/2, ky = 0 .. Ny-1 (FFT order),
    E[s]       = sum of P2 over the modes whose shell is s,   shell = floor(sqrt(wx mx^2 + wy my^2) + 1/2),   s = 0 .. NS-1,
with c_kx = 1 at kx = 0 and Nx/2, else 2, so that sum P2 = sum_s E[s] = the mean of F^2.  The shell width is dk = max(2 pi/Lx, 2 pi/Ly)
and wx = (2 pi/Lx / dk)^2, wy = (2 pi/Ly / dk)^2: a square domain has wx = wy = 1 and integer shells.  `isotropic_shells(grid)` gives
k = s dk and the number of modes of every shell -- divide by it for a spectral density.  No frame-sized float64 copy to the host, no
FFT library, no host synchronisation.  IsotropicSpectrumTimeSeries speaks the writer protocol of swmhd_amd.output.run().

Error: |got - P2| <= c_kx (2 |F^| eps sqrt(S) + eps^2 S), S the mean of F^2, eps = 9.66 (log2 Nx + log2 Ny) 2^-53; a shell: the sum of
its modes' bounds plus gamma_(n-1) E[s] (include/swmhd_spectra2d.h has the derivation).

Both directions must be Periodic and both sizes a power of two from 4 to 4096.  The transform needs every row, so a model on a y-slab
decomposition of more than one rank (ring=) is refused.  The device workspace (the complex half-plane, 2 (Nx/2+1) Ny doubles per
field, and the column partials, (Nx/2+1) NS doubles per field: 134 MB + 47 MB per field at 4096^2) is cached on the model.
"""
import math

import torch

from . import _lib
from ._series import DeviceTimeSeries, cached_workspace, lead_shape, out_tensor, state_pointers
from .fields import _stream_ptr
from .output import TimeInterval
from .spectra import DEFAULT_NAMES, _runs


def metric(grid):
    """(dk, wx, wy): the shell width max(2 pi/Lx, 2 pi/Ly) and the squared ratios of the two spectral spacings to it."""
    dkx, dky = 2.0 * math.pi / grid.Lx, 2.0 * math.pi / grid.Ly
    dk = max(dkx, dky)
    return dk, (dkx / dk) ** 2, (dky / dk) ** 2


def shell_index(Nx, Ny, wx, wy):
    """The shell of every mode (kx = 0 .. Nx/2, ky = 0 .. Ny-1 in FFT order) as an int64 array (Nx/2 + 1, Ny): the statement of
    include/swmhd_spectra2d.h in IEEE double -- two products, one sum, sqrt, + 0.5, floor -- so bit for bit the kernel's."""
    import numpy as np
    mx = np.arange(Nx // 2 + 1, dtype=np.int64)[:, None]
    ky = np.arange(Ny, dtype=np.int64)[None, :]
    my = np.where(ky <= Ny // 2, ky, ky - Ny)
    a = np.float64(wx) * (mx * mx).astype(np.float64)
    b = np.float64(wy) * (my * my).astype(np.float64)
    r2 = a + b
    return np.floor(np.sqrt(r2) + 0.5).astype(np.int64)


def isotropic_shells(grid):
    """(k, counts): k = s dk of the NS shells and the number of modes of the full (Nx x Ny) plane in each (they sum to Nx Ny; a mode
    with 0 < kx < Nx/2 stands for itself and its conjugate)."""
    import numpy as np
    dk, wx, wy = metric(grid)
    Nx, Ny = grid.Nx, grid.Ny
    sh = shell_index(Nx, Ny, wx, wy)
    NS = int(sh[Nx // 2, Ny // 2]) + 1
    c = np.full((Nx // 2 + 1, 1), 2, dtype=np.int64)
    c[0] = c[Nx // 2] = 1
    counts = np.bincount(sh.ravel(), weights=np.broadcast_to(c, sh.shape).ravel(), minlength=NS).astype(np.int64)
    return dk * np.arange(NS, dtype=np.float64), counts


def _check(model, names, what):
    """What is refused before anything is allocated: names, a Bounded direction, an unsupported size, a y-slab decomposition."""
    runs = _runs(names, getattr(model, "tracer_names", ()))
    g = model.grid
    if g.topology[0] != "Periodic" or g.topology[1] != "Periodic":
        raise _lib.SwmhdError(f"{what}: a direction is Bounded: a DFT of a non-periodic field is not a spectrum")
    for n, N in (("Nx", g.Nx), ("Ny", g.Ny)):
        if N < _lib.SPECTRA_MIN_NX or N > _lib.SPECTRA_MAX_NX or N & (N - 1):
            raise _lib.SwmhdError(f"{what}: {n} = {N}: a power of two from {_lib.SPECTRA_MIN_NX} to {_lib.SPECTRA_MAX_NX} is supported")
    ranks = getattr(getattr(model, "decomp", None), "world_size", 1)
    if ranks > 1 or getattr(model, "_ring", None) is not None:
        raise _lib.SwmhdError(f"{what}: not supported (SWMHD_ENOTSUP) on a y-slab decomposition ({ranks} ranks, or ring=): a 2-D "
                              "transform needs every row, and the slab-global transform is not built")
    return runs


def shells(grid):
    """NS of the grid, from the statement of the header (no library call)."""
    _, wx, wy = metric(grid)
    a = wx * float((grid.Nx // 2) ** 2)
    b = wy * float((grid.Ny // 2) ** 2)
    return int(math.floor(math.sqrt(a + b) + 0.5)) + 1


def _enqueue(model, names, shell_out, plane_out, what):
    names = tuple(names)
    runs = _check(model, names, what)
    g = model.grid
    _, wx, wy = metric(g)
    NS, nkx = shells(g), g.Nx // 2 + 1
    ptrs, sy, dev, ens = state_pointers(model)
    outs = []
    for out, tail, row_stride in ((shell_out, (len(names), NS), 0), (plane_out, (len(names), nkx, g.Ny), g.Ny)):
        if out is not None:      # (True: allocate)
            out = out_tensor(None if out is True else out, lead_shape(model) + tail, (torch.float64,), dev, what, "its last axis",
                             row_stride=row_stride)
        outs.append(out)
    eo, po = outs
    # (the workspace: what the C function states for the largest run asked for so far)
    need = model._L.swmhd_spectra2d_workspace(g.Nx, g.Ny, max(len(bits) for bits in runs), getattr(model, "members", None) or 1, wx, wy)
    ws = cached_workspace(model, "_spectra2d_ws", need, dev)
    flags = model._rwrap                  # as enqueue_frame: the periodic images where the step leaves the halos stale
    sfx = model.sfx
    k = 0
    for bits in runs:                     # (the runs share the workspace: launches on one stream run one after the other)
        which = sum(bits)
        e1 = eo.select(-2, k) if eo is not None else None
        p1 = po.select(-3, k) if po is not None else None
        eargs = (e1.data_ptr(), eo.stride(-2)) if eo is not None else (None, 0)
        pargs = (p1.data_ptr(), po.stride(-2), po.stride(-3)) if po is not None else (None, 0, 0)
        if ens:
            f = getattr(model._L, f"swmhd_ensemble_spectra2d_{sfx}")
            rc = f(*ptrs, model.members, model.stride_m, g.Nx, g.Ny, g.Hx, g.Hy, sy, g.dx, g.dy, model.form_code, which, wx, wy,
                   ws.data_ptr(), *eargs, eo.stride(0) if eo is not None else 0, *pargs, po.stride(0) if po is not None else 0,
                   flags, _stream_ptr())
        else:
            f = getattr(model._L, f"swmhd_spectra2d_{sfx}")
            rc = f(*ptrs, g.Nx, g.Ny, g.Hx, g.Hy, sy, g.dx, g.dy, model.form_code, which, wx, wy, ws.data_ptr(), *eargs, *pargs,
                   flags, _stream_ptr())
        _lib.check(rc, "swmhd_spectra2d")
        k += len(bits)
    return eo, po


def enqueue_isotropic_spectra(model, names=DEFAULT_NAMES, out=None):
    """ShallowWaterModel.isotropic_spectra / the ensembles': see there."""
    return _enqueue(model, names, True if out is None else out, None, "isotropic_spectra")[0]


def enqueue_power_spectra_2d(model, names=DEFAULT_NAMES, out=None):
    """ShallowWaterModel.power_spectra_2d / the ensembles': see there."""
    return _enqueue(model, names, None, True if out is None else out, "power_spectra_2d")[1]


def isotropic_shape(model, names):
    return lead_shape(model) + (len(names), shells(model.grid))


class IsotropicSpectrumTimeSeries(DeviceTimeSeries):
    """A writer of isotropic spectra for run(): `capacity` samples of `names` in one float64 device tensor, plus the host lists `times`
    and `iterations`.  spectra: (capacity, len(names), NS); for an ensemble (capacity, members, len(names), NS).  Names: u v h A s B_x
    B_y (include/swmhd_spectra2d.h).

    The tensor is allocated when the first sample is written.  `write` only enqueues; `numpy` and `save` are the calls that
    synchronise."""

    _data, _unit = "spectra", "samples"
    spectra = DeviceTimeSeries.tensor

    def __init__(self, model, names=DEFAULT_NAMES, schedule=TimeInterval(0.1), capacity=None):
        super().__init__(model, names, schedule, capacity)

    def _check_names(self):
        _check(self.model, self.names, "IsotropicSpectrumTimeSeries")

    def _sample_shape(self):
        return isotropic_shape(self.model, self.names)

    def _enqueue(self, out):
        enqueue_isotropic_spectra(self.model, self.names, out=out)

    def save(self, path):
        """One .npz: spectra, names, times, iterations, k = s dk of the shells and counts, their mode counts (synchronises)."""
        import numpy as np
        k, counts = isotropic_shells(self.model.grid)
        self._savez(path, k=k, counts=counts)
