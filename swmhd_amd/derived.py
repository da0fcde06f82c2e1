"""Derived frames: relative vorticity, velocity divergence, vertical current and potential vorticity, made on the device.

A 2-D MHD turbulence run is read by zeta = dv/dx - du/dy, J = laplace(A), the divergence (the gravity-wave part, and the first thing to
look at when a run goes unstable) and the shallow-water potential vorticity q = (zeta + f) / h.  In Oceananigans each is one line handed
to the writer; here `derived_fields` (a method of ShallowWaterModel and of the ensembles) enqueues ONE kernel (swmhd_derived_fields_*,
include/swmhd_derived.h) that differences the four parents into a halo-stripped device tensor in the writer's element type, for all
members of an ensemble, without a halo fill in front and without a host synchronisation.  The writer is swmhd_amd.output's
FieldTimeSeries, which takes these names mixed with the seven of the frame.  Zonal means and integrals of these fields are out of scope
(DESIGN.md section 7).
"""
import torch

from . import _lib
from ._series import cut_runs, lead_shape, out_tensor, state_pointers    # (state_pointers: also for those who import it from here)
from .fields import _stream_ptr

DEFAULT_NAMES = ("vorticity", "current")
ELEM_TYPES = (torch.float32, torch.float64)      # the element types of a frame
# a tracer among the names of a frame, derived or not: the frame's answer
TRACER_MESSAGE = f"output field {{n!r}} is a tracer: frames hold {' '.join(_lib.OUT_BITS)} only; read model.tracers[{{n!r}}]"
_MESSAGES = (TRACER_MESSAGE, f"derived field {{n!r}}: one of {' '.join(_lib.DRV_BITS)}", "derived_fields: no field names")


def _runs(names, tracers=()):
    """The fields as launches (cut_runs): bit order vorticity divergence current potential_vorticity."""
    return cut_runs(names, _lib.DRV_BITS, tracers, _MESSAGES)


def check_coriolis_names(model, names):
    """SwmhdError for potential_vorticity of a model whose Coriolis parameter varies with y: the kernel takes one scalar f."""
    if getattr(model, "_coriolis", None) is not None and "potential_vorticity" in names:
        raise _lib.SwmhdError(f"potential_vorticity under coriolis = {model.coriolis!r} is not supported (SWMHD_ENOTSUP): "
                              "swmhd_derived_fields_* takes a scalar f; vorticity is available")


def launch(model, ptrs, sy, ens, which, first, out):
    """One swmhd_[ensemble_]derived_fields[_params]_* launch: the fields of mask `which` into `out` from its field `first` on."""
    g, sfx = model.grid, model.sfx
    frame = (0, g.Ny, which, first.data_ptr(), out.element_size(), out.stride(-2), out.stride(-3))
    if not ens:
        f = getattr(model._L, f"swmhd_derived_fields_{sfx}")
        rc = f(*ptrs, g.Nx, g.Ny, g.Hx, g.Hy, sy, g.dx, g.dy, model.form_code, model.f, *frame, model._rwrap, _stream_ptr())
    else:
        par = model.parameters is not None      # each member's f, from the table
        f = getattr(model._L, f"swmhd_ensemble_derived_fields_{'params_' if par else ''}{sfx}")
        rc = f(*ptrs, model.members, model.stride_m, g.Nx, g.Ny, g.Hx, g.Hy, sy, g.dx, g.dy, model.form_code,
               model.parameters.data_ptr() if par else model.f, *frame, out.stride(0), model._rwrap, _stream_ptr())
    _lib.check(rc, "swmhd_derived_fields")


def enqueue_derived(model, names=DEFAULT_NAMES, out=None, array_type=torch.float32):
    """ShallowWaterModel.derived_fields / ShallowWaterEnsemble.derived_fields: see there."""
    names = tuple(names)
    runs = _runs(names, getattr(model, "tracer_names", ()))
    check_coriolis_names(model, names)
    ptrs, sy, dev, ens = state_pointers(model)
    out = out_tensor(out, lead_shape(model) + (len(names), model.grid.Ny, model.grid.Nx), ELEM_TYPES, dev, "derived_fields", "x", array_type)
    k = 0
    for bits in runs:
        launch(model, ptrs, sy, ens, sum(bits), out.select(-3, k), out)
        k += len(bits)
    return out
