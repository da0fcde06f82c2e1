"""The per-stage correction launches of a ShallowWaterModel or a ShallowWaterEnsemble: the terms that are not in the stage kernel and are
added, one launch each, to what it wrote -- a Coriolis parameter that varies with y, the two closures, the forcing.  `correction_list`
builds the ordered list an object holds as `_corrections`, `Correction.launch` makes the call of every kind for both classes
(shared.finish_stage runs the list), and the set-up the constructors share is here too.  Only `member_table` touches a device."""
import ctypes

import numpy as np
import torch

from . import _lib
from .fields import _stream_ptr
from .shared import correction_operand, rk3_stage


def live_fields(coefs):
    """`coefs` ({field: a value, or one per member}, or None) without the fields whose values are all 0, which take no part in the
    launch; None where nothing is left, and then the object makes exactly the calls it makes without the argument."""
    return {n: c for n, c in (coefs or {}).items() if np.any(np.asarray(c) != 0.0)} or None


def member_table(columns, dtype, device):
    """The (members, fields) device table of an ensemble call, in `dtype` and rounded to it, from one (members,) column per field."""
    return torch.from_numpy(np.ascontiguousarray(np.stack(columns, axis=1))).to(device=device, dtype=dtype)


def _host_table(sfx, values):
    """The host table of a single-grid call: one value per field in the call's element type."""
    return ((ctypes.c_double if sfx == "f64" else ctypes.c_float) * len(values))(*values)


class Correction:
    """One correction launch of `o`: swmhd_[ensemble_]<stem>_rk3_*, D evaluated on the state the stage started from and added with
    a = dt gamma to the `names` fields (state or tracers) the stage wrote and, where the stage stores an operand for later stages, to
    it with the weight w (shared.correction_operand).  Every such entry point takes
        the three field sets (old, new, acc), `middle`, [members, stride_m, member_strides,] Nx, Ny, Hx, Hy, sy, [dx, dy,] [params,]
        a, w, j0, j1, flags, stream
    with the bracketed ensemble arguments for an ensemble, which passes a = gamma and the parameter table where every member has its
    own dt (dt None), and SWMHD_RK3_ANCHOR where w is a weight of that dt.  `middle`: what is the kind's own -- the row table; the
    coefficients and the number of fields; masks, targets, rates, scalar targets and the number of fields -- built once.  unpacked:
    the field sets go as single pointers, not as arrays (the Coriolis call names its two fields).  spacings: the call takes dx, dy."""

    def __init__(self, o, stride_y, stem, names, middle, spacings=False, unpacked=False, member_strides=()):
        g, order = o.grid, o.names + o.tracer_names
        ens = hasattr(o, "members")
        self.stem, self.names, self.middle, self.unpacked = stem, tuple(names), tuple(middle), unpacked
        self.symbol = f"swmhd_{'ensemble_' if ens else ''}{stem}_rk3"
        self._index = [order.index(n) for n in names]
        self._members = (o.members, o.stride_m, *member_strides) if ens else None
        self._grid = (g.Nx, g.Ny, g.Hx, g.Hy, stride_y) + ((g.dx, g.dy) if spacings else ())
        self._rows = (0, g.Ny)

    def launch(self, o, dt, stage):
        """Enqueue the launch of RK3 stage `stage`: after the stage's own launch and the tracers', BEFORE the sets are swapped."""
        listed = lambda s: list(s.values()) if isinstance(s, dict) else list(s)
        pick = lambda state, tracers: [(listed(state) + listed(tracers))[k].data.data_ptr() for k in self._index]
        has, w, flag = correction_operand(stage, o._anchor, dt)
        sets = [pick(o._state, o._tr), pick(o._alt, o._tr_alt), pick(o.Gn, o._tGn) if has else None]
        if self.unpacked:
            head = [p for s in sets for p in (s or [None] * len(self._index))]
        else:
            head = [_lib.ptr_array(s) if s is not None else None for s in sets]
        gamma = rk3_stage(stage, o._anchor)[0]
        a = gamma if dt is None else dt * gamma
        flags = (_lib.STRICT if o.strict else _lib.FAST) | o._rwrap
        f = getattr(o._L, f"{self.symbol}_{o.sfx}")
        if self._members is None:
            rc = f(*head, *self.middle, *self._grid, a, w, *self._rows, flags, _stream_ptr())
        else:
            params = o.parameters.data_ptr() if dt is None else None
            rc = f(*head, *self.middle, *self._members, *self._grid, params, a, w, *self._rows, flags | flag, _stream_ptr())
        _lib.check(rc, self.symbol)


class StochasticCorrection(Correction):
    """The stochastic forcing's launch (swmhd_[ensemble_]stochastic_rk3_*): Correction's call with the coefficient draw of the step
    (swmhd_[ensemble_]stochastic_coefficients_*, which advances the device counter) enqueued in front of the stage-0 launch, so that
    the coefficients are renewed once per step and held over its three stages.  The amplitude carries 1/sqrt(dt), which the draw is
    given as one number: an ensemble whose corrections are handed dt None (a parameter table) hands over step_dt, the one dt its
    members share, and the call goes without the table."""

    needs_step_dt = True      # (shared.finish_stage hands over the one dt the members share beside dt)

    def launch(self, o, dt, stage, step_dt=None):
        st = o._stochastic
        if dt is None:
            dt = step_dt
        if dt is None:
            raise _lib.SwmhdError("StochasticForcing with a per-member dt is not supported (SWMHD_ENOTSUP): its amplitude carries 1/sqrt(dt)")
        if stage == 0:
            st.draw(o, dt)
        super().launch(o, dt, stage)


def correction_list(o, stride_y):
    """The active corrections of `o` (its data attributes _coriolis, _diffusion, _biharmonic, _relaxation, _source and _stochastic: None
    where inactive) in the order of their launches: Coriolis, Laplacian, biharmonic, relaxation, source, stochastic.  Each corrects what
    the launches before it have written, so the new field is ((((((stage + a D_cor) + a D_lap) + a D_bih) + a D_relax) + a D_src) +
    a F_stoch), and this order
    decides the last bits where several are present.  Empty without any: then the object may step through its native driver (needs_stages).  stride_y: the
    pitch of the object's fields.  A further term is one more entry here, after the ones whose result it is to correct: its stem,
    its fields and its `middle`; the C entry points take the argument layout Correction states."""
    ens = hasattr(o, "members")
    order = o.names + o.tracer_names
    out = []
    if o._coriolis is not None:
        # D = f(y_j) (vbar, -ubar) on the two momentum-like fields; the rows of member m in block m of the table
        out.append(Correction(o, stride_y, "coriolis", order[:2], (o.coriolis_rows.data_ptr(),), unpacked=True))
    for stem, coefs in (("diffusion", o._diffusion), ("biharmonic", o._biharmonic)):
        if coefs is not None:
            # D = coef laplace(field), D = -coef laplace(laplace(field)); the coefficients of member m in row m of the device table
            names = [n for n in order if n in coefs]
            coef = getattr(o, f"{stem}_coefficients").data_ptr() if ens else _host_table(o.sfx, [coefs[n] for n in names])
            out.append(Correction(o, stride_y, stem, names, (coef, len(names)), spacings=True))
    if o._relaxation is not None:
        # D = rate mask (target - field); _relaxation: (name, ..., mask, target) of every forced field, mask and target device
        # parents where they are arrays.  It reads no halo, so a Bounded grid takes it as a periodic one does
        rel = o._relaxation
        parents = lambda k: _lib.ptr_array([r[k].data_ptr() if torch.is_tensor(r[k]) else None for r in rel])
        if ens:
            tables, strides = (o.relaxation_rates.data_ptr(), o.relaxation_targets.data_ptr()), (o._mask_stride, o._target_stride)
        else:
            tables = (_host_table(o.sfx, [r[1] for r in rel]), _host_table(o.sfx, [0.0 if torch.is_tensor(r[-1]) else r[-1] for r in rel]))
            strides = ()
        out.append(Correction(o, stride_y, "relaxation", [r[0] for r in rel], (parents(-2), parents(-1), *tables, len(rel)),
                              member_strides=strides))
    if getattr(o, "_source", None) is not None:
        # D = S, or S times the thickness of the state the stage started from at the field's face (the conservative uh, vh); _source:
        # (name, kind, S) of every field with a static source -- bathymetry and Source entries --, S a device parent.  Where a kind needs
        # the thickness, h goes along in the call's field list without a source of its own
        src = o._source
        names = [n for n in order if n in [s[0] for s in src] or n == o._source_thickness]
        by = {s[0]: s for s in src}
        middle = (_lib.ptr_array([by[n][2].data_ptr() if n in by else None for n in names]),
                  (ctypes.c_int * len(names))(*[by[n][1] if n in by else _lib.SOURCE_PLAIN for n in names]), len(names),
                  names.index(o._source_thickness) if o._source_thickness is not None else -1)
        out.append(Correction(o, stride_y, "source", names, middle, member_strides=(o._source_stride,) if ens else ()))
    if getattr(o, "_stochastic", None) is not None:
        # F = the sum of the step's random Fourier modes; _stochastic.fields: (name, mode count, coefficients, x table, y table) of
        # every stirred field.  It reads no state: `old` goes along for the common layout only
        st = o._stochastic
        col = lambda k: [f[k] for f in st.fields]
        middle = (_lib.ptr_array(col(2)), _lib.ptr_array(col(3)), _lib.ptr_array(col(4)), (ctypes.c_int * len(st.fields))(*col(1)),
                  len(st.fields), st.x_pitch, st.y_pitch)
        out.append(StochasticCorrection(o, stride_y, "stochastic", col(0), middle, member_strides=(st.coef_stride,) if ens else ()))
    return out


def needs_stages(o):
    """Whether `o` must step stage by stage: its native step driver steps the four fields only, with a scalar f, and no particles."""
    return bool(o._tr or o._corrections or getattr(o, "particles", None) is not None)
