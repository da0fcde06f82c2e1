"""Relaxation: Oceananigans' `forcing = (u = Relaxation(rate, mask, target), h = ...)` for the shallow-water MHD engine -- the term
rate * mask(x, y) * (target(x, y) - φ) added to the tendency of the prognostic field φ of that name, one extra launch per RK3 stage for
all forced fields (swmhd_relaxation_rk3_* in include/swmhd_relaxation.h).  Large-scale drag is Relaxation(rate) on the two momentum-like
fields, a sponge layer a Relaxation with a mask, Newtonian relaxation of h one with a target array.

Source and `bathymetry=`: a field that does not change in time added to the tendency, under "uh" / "vh" times the thickness at the
face -- a steady body force and the slope of the bottom, which the host folds into one static field per forced field (check_source),
one extra launch per RK3 stage (swmhd_source_rk3_* in include/swmhd_source.h).

Only device_parents touches a device, and only when a model that has passed its checks asks for it."""
import math

import numpy as np

from . import _lib
from .closure import RK3_REAL_AXIS_BOUND
from .fields import LOCS
from .grid import Center
from .stochastic import MAX_MODES, PAIR, SCALAR, StochasticForcing, forcing_modes


def _nodes(grid, loc):
    """(x, y) of the grid's own interior nodes at `loc`, x as (1, Nx) and y as (Ny, 1)."""
    x = (grid.xc if loc[0] == Center else grid.xf)[grid.Hx:grid.Hx + grid.Nx]
    y = (grid.yc if loc[1] == Center else grid.yf)[grid.Hy:grid.Hy + grid.Ny]
    return x[None, :], y[:, None]


def _finite(arr, what):
    if not np.all(np.isfinite(arr)):
        raise _lib.SwmhdError(f"Relaxation: {what} has values that are not finite")
    return arr


class Relaxation:
    """rate: a finite scalar >= 0 (1 / time), for a ShallowWaterEnsemble also a sequence with one value per member.  mask: None (1
    everywhere), a callable (x, y) or an array (Ny, Nx).  target: a scalar (for an ensemble also one per member), a callable (x, y) or an
    array (Ny, Nx).  For an ensemble the arrays may also be (members, Ny, Nx).  Callables are evaluated once, when the model is built,
    on the grid's own nodes at the location of the field (x of shape (1, Nx), y of shape (Ny, 1)); the arrays are rounded to the
    model's dtype.  The time step is not limited by the forcing: see max_stable_dt."""

    def __init__(self, rate, mask=None, target=0.0):
        r = np.asarray(rate, dtype=np.float64) if not callable(rate) else None
        if r is None or r.ndim > 1 or not np.all(np.isfinite(r)) or np.any(r < 0):
            raise _lib.SwmhdError(f"Relaxation: rate = {rate!r}: finite values >= 0 (a scalar, or one per member of an ensemble)")
        self.rate = float(r) if r.ndim == 0 else r.copy()
        self.mask = mask if mask is None or callable(mask) else self._array(mask, "mask", (2, 3))
        if callable(target):
            self.target = target
        else:
            t = self._array(target, "target", (0, 1, 2, 3))
            self.target = float(t) if t.ndim == 0 else t

    @staticmethod
    def _array(value, what, ndims):
        try:
            arr = np.array(value, dtype=np.float64)
        except (TypeError, ValueError):
            arr = None
        if arr is None or arr.ndim not in ndims:
            raise _lib.SwmhdError(f"Relaxation: {what} = {type(value).__name__}: a callable (x, y), an array (Ny, Nx)"
                                  + (" or a scalar" if what == "target" else " or None"))
        return _finite(arr, what)

    def __repr__(self):
        show = lambda v: v.__name__ if callable(v) else (f"array{v.shape}" if np.ndim(v) > 1 else repr(v))
        return f"Relaxation(rate={self.rate!r}, mask={show(self.mask) if self.mask is not None else None}, target={show(self.target)})"

    @property
    def per_member(self):
        """True where anything holds one value or one array per member of an ensemble."""
        return np.ndim(self.rate) == 1 or (not callable(self.target) and np.ndim(self.target) in (1, 3)) or \
            (self.mask is not None and not callable(self.mask) and self.mask.ndim == 3)

    def for_member(self, m):
        """The Relaxation of member m of an ensemble: every per-member sequence or array replaced by its entry m."""
        rate = float(self.rate[m]) if np.ndim(self.rate) else self.rate
        target = self.target if callable(self.target) or np.ndim(self.target) in (0, 2) else \
            (float(self.target[m]) if np.ndim(self.target) == 1 else self.target[m])
        mask = self.mask[m] if (self.mask is not None and not callable(self.mask) and self.mask.ndim == 3) else self.mask
        return Relaxation(rate, mask, target)

    def evaluate(self, grid, loc, name="", members=None):
        """(mask, target) on `grid` at `loc` as float64 host values: mask None or an array (Ny, Nx) / (members, Ny, Nx); target a float,
        an array (members,) of scalars, or an array (Ny, Nx) / (members, Ny, Nx).  members None: a single model, which takes nothing
        per member.  SwmhdError for a wrong shape or a value that is not finite."""
        shape = (grid.Ny, grid.Nx)
        x, y = _nodes(grid, loc)

        def field(v, what):
            if callable(v):
                arr = np.asarray(v(x, y), dtype=np.float64)
                try:
                    arr = np.broadcast_to(arr, shape).copy()
                except ValueError:
                    raise _lib.SwmhdError(f"forcing of {name}: {what}(x, y) has shape {arr.shape}, not {shape}") from None
                return _finite(arr, f"{what} of {name}")
            ok = (shape,) if members is None else (shape, (members,) + shape)
            if v.shape not in ok:
                raise _lib.SwmhdError(f"forcing of {name}: {what} of shape {v.shape}, expected {' or '.join(map(str, ok))}")
            return v
        if members is None and self.per_member:
            raise _lib.SwmhdError(f"forcing of {name}: per-member values belong to an ensemble")
        mask = None if self.mask is None else field(self.mask, "mask")
        t = self.target
        if callable(t) or np.ndim(t) >= 2:
            target = field(t, "target")
        elif np.ndim(t) == 1:
            if t.shape[0] != members:
                raise _lib.SwmhdError(f"forcing of {name}: {t.shape[0]} targets for {members} members (a scalar or one per member)")
            target = t.copy()
        else:
            target = float(t)
        if np.ndim(self.rate) == 1 and self.rate.shape[0] != members:
            raise _lib.SwmhdError(f"forcing of {name}: {self.rate.shape[0]} rates for {members} members (a scalar or one per member)")
        return mask, target

    def max_stable_dt(self, grid=None, location=(Center, Center)):
        """2.51 / (rate max|mask|): the largest dt at which RK3 damps the relaxation where it is fastest (the term's eigenvalue there
        is -rate mask; RK3 is stable on the negative real axis down to -2.51).  inf with rate 0.  A callable mask needs the grid and
        the location of the field to be evaluated.  Documented, not enforced: advection and waves limit dt as well."""
        if self.mask is None:
            mmax = 1.0
        elif callable(self.mask):
            if grid is None:
                raise _lib.SwmhdError("Relaxation.max_stable_dt: a callable mask needs the grid (and the location of the field)")
            mmax = float(np.max(np.abs(np.asarray(self.mask(*_nodes(grid, location)), dtype=np.float64))))
        else:
            mmax = float(np.max(np.abs(self.mask)))
        rmax = float(np.max(self.rate)) * mmax
        return math.inf if rmax == 0.0 else RK3_REAL_AXIS_BOUND / rmax


class Source:
    """A steady source: `value` added to the tendency of the prognostic field it is given for, every RK3 stage (swmhd_source_rk3_* in
    include/swmhd_source.h) -- a Kolmogorov body force, a tracer source.  value: a callable (x, y) evaluated once, when the model is
    built, on the grid's own nodes at the location of the field (x of shape (1, Nx), y of shape (Ny, 1)); an array (Ny, Nx); or a
    scalar.  For a ShallowWaterEnsemble also an array (members, Ny, Nx) or one scalar per member.  Under "uh" / "vh" it is an
    acceleration as under "u" / "v": the device multiplies it by the thickness at the face.  It does not depend on time or on the
    state, and it does not limit the time step."""

    def __init__(self, value):
        if callable(value):
            self.value = value
            return
        try:
            arr = np.array(value, dtype=np.float64)
        except (TypeError, ValueError):
            arr = None
        if arr is None or arr.ndim > 3:
            raise _lib.SwmhdError(f"Source: value = {type(value).__name__}: a callable (x, y), an array (Ny, Nx) or a scalar")
        if not np.all(np.isfinite(arr)):
            raise _lib.SwmhdError("Source: value has values that are not finite")
        self.value = float(arr) if arr.ndim == 0 else arr

    def __repr__(self):
        v = self.value
        return f"Source({v.__name__ if callable(v) else (f'array{v.shape}' if np.ndim(v) else repr(v))})"

    @property
    def per_member(self):
        """True where the value holds one scalar or one array per member of an ensemble."""
        return not callable(self.value) and np.ndim(self.value) in (1, 3)

    def for_member(self, m):
        """The Source of member m of an ensemble."""
        return Source(self.value[m]) if self.per_member else self

    def evaluate(self, grid, loc, name="", members=None):
        """The value on `grid` at `loc` as float64 host values: an array (Ny, Nx), or (members, Ny, Nx) where it is per member.
        members None: a single model, which takes nothing per member.  SwmhdError for a wrong shape or a value that is not finite."""
        shape = (grid.Ny, grid.Nx)
        v = self.value
        if callable(v):
            arr = np.asarray(v(*_nodes(grid, loc)), dtype=np.float64)
            try:
                arr = np.broadcast_to(arr, shape).copy()
            except ValueError:
                raise _lib.SwmhdError(f"forcing of {name}: Source(x, y) has shape {arr.shape}, not {shape}") from None
            if not np.all(np.isfinite(arr)):
                raise _lib.SwmhdError(f"forcing of {name}: Source(x, y) has values that are not finite")
            return arr
        if members is None and self.per_member:
            raise _lib.SwmhdError(f"forcing of {name}: per-member values belong to an ensemble")
        if np.ndim(v) == 0:
            return np.full(shape, float(v))
        if np.ndim(v) == 1:
            if v.shape[0] != members:
                raise _lib.SwmhdError(f"forcing of {name}: {v.shape[0]} sources for {members} members (a scalar or one per member)")
            return np.broadcast_to(v[:, None, None], (members,) + shape).copy()
        ok = (shape,) if members is None else (shape, (members,) + shape)
        if v.shape not in ok:
            raise _lib.SwmhdError(f"forcing of {name}: Source of shape {v.shape}, expected {' or '.join(map(str, ok))}")
        return v.copy()


def check_bathymetry(bathymetry, grid, members=None, slabs=False, ring=False, fused=True, bounded_ensemble=False):
    """`bathymetry=` of a model or an ensemble as float64 host values at the cell centres: None, an array (Ny, Nx) or, for an ensemble,
    (members, Ny, Nx); a callable (x, y) is evaluated once on the centres.  The refusals are made here, before anything is allocated."""
    if bathymetry is None:
        return None
    if bounded_ensemble:
        raise _lib.SwmhdError("bathymetry on a Bounded ensemble is not supported (SWMHD_ENOTSUP): swmhd_ensemble_step_rk3_bc is one native "
                              "call and has no per-stage entry point for the correction launch")
    if slabs:
        raise _lib.SwmhdError("bathymetry on a y-slab decomposition is not supported (SWMHD_ENOTSUP): one rank only")
    if ring:
        raise _lib.SwmhdError("bathymetry with ring= is not supported (SWMHD_ENOTSUP): the slab driver steps the four fields only")
    if not fused:
        raise _lib.SwmhdError("bathymetry needs the fused stage kernel (SWMHD_ENOTSUP): fused=False leaves no copy of the state a stage "
                              "started from")
    shape = (grid.Ny, grid.Nx)
    if callable(bathymetry):
        b = np.asarray(bathymetry(*_nodes(grid, (Center, Center))), dtype=np.float64)
        try:
            b = np.broadcast_to(b, shape).copy()
        except ValueError:
            raise _lib.SwmhdError(f"bathymetry(x, y) has shape {b.shape}, not {shape}") from None
    else:
        try:
            b = np.array(bathymetry, dtype=np.float64)
        except (TypeError, ValueError):
            b = None
        ok = (shape,) if members is None else (shape, (members,) + shape)
        if b is None or b.shape not in ok:
            raise _lib.SwmhdError(f"bathymetry = {type(bathymetry).__name__}" + (f" of shape {b.shape}" if b is not None else "") +
                                  f": a callable (x, y), an array {' or '.join(map(str, ok))}, or None")
    if not np.all(np.isfinite(b)):
        raise _lib.SwmhdError("bathymetry has values that are not finite")
    return b


def bathymetry_slope(b, g, spacing, axis, periodic):
    """-g ((b[i] - b[i-1]) / spacing) along `axis` (-1: x, -2: y) in float64, the operations in this order: the acceleration of the
    bottom's slope at the faces of that direction.  b is wrapped in a Periodic direction; on the wall line of a Bounded one (face 0) the
    value is 0 -- the boundary fill resets that line anyway.  g: a float, or an array (members, 1, 1)."""
    d = (b - np.roll(b, 1, axis=axis)) / spacing
    if not periodic:
        d[(Ellipsis, 0) if axis == -1 else (Ellipsis, 0, slice(None))] = 0.0
    return -(g * d)


def check_source(forcing, bathymetry, grid, names, tracer_names, g, members=None, conservative=False):
    """The static sources of a model or an ensemble whose `forcing` has passed check_forcing and whose `bathymetry` check_bathymetry:
    per field the final S in float64, built once --
        S_u = F_u - g ((b[i,j] - b[i-1,j]) / dx),  S_v = F_v - g ((b[i,j] - b[i,j-1]) / dy),  S = F for h, A and the tracers,
    F the field's Source or 0 (bathymetry_slope has the wrap and the walls).  Returns (sources, thickness): sources a list of (name,
    kind, S) in the order of `names` then `tracer_names`, S of shape (Ny, Nx) or, where anything is per member, (members, Ny, Nx), kind
    SWMHD_SOURCE_PLAIN or, for uh / vh of the conservative formulation, _X_FACE / _Y_FACE (the expression is the same: the device
    multiplies by the thickness at the face); the fields whose S is identically 0 left out.  thickness: "h" where a kind needs it, else
    None.  (None, None) where nothing is left, and then the model makes exactly the calls it makes without the arguments.
    g: a float, or an array (members,)."""
    fields = tuple(names) + tuple(tracer_names)
    F = {}
    for n in fields:
        s = split_entry(n, forcing[n])[2] if (forcing and n in forcing) else None
        if s is not None:
            F[n] = s.evaluate(grid, LOCS.get(n, (Center, Center)), n, members)
    if bathymetry is not None:
        tx, ty = grid.topo_codes()
        gv = np.asarray(g, dtype=np.float64)
        gv = float(gv) if gv.ndim == 0 else gv[:, None, None]
        for n, spacing, axis, topo in ((names[0], grid.dx, -1, tx), (names[1], grid.dy, -2, ty)):
            slope = bathymetry_slope(bathymetry, gv, spacing, axis, topo == _lib.PERIODIC)
            F[n] = F[n] + slope if n in F else slope
    out = []
    for n in fields:
        if n in F and np.any(F[n] != 0.0):
            kind = _lib.SOURCE_PLAIN
            if conservative and n in names[:2]:
                kind = _lib.SOURCE_X_FACE if n == names[0] else _lib.SOURCE_Y_FACE
            out.append((n, kind, F[n]))
    if not out:
        return None, None
    return out, ("h" if any(k != _lib.SOURCE_PLAIN for _, k, _ in out) else None)


def split_entry(name, value):
    """(Relaxation or None, StochasticForcing or None, Source or None) of one value of the `forcing=` dict: one of the classes, or a
    tuple with at most one of each."""
    items = value if isinstance(value, tuple) else (value,)
    relax = [v for v in items if isinstance(v, Relaxation)]
    stir = [v for v in items if isinstance(v, StochasticForcing)]
    source = [v for v in items if isinstance(v, Source)]
    if not items or len(relax) + len(stir) + len(source) != len(items) or len(relax) > 1 or len(stir) > 1 or len(source) > 1:
        bad = next((v for v in items if not isinstance(v, (Relaxation, StochasticForcing, Source))), value)
        raise _lib.SwmhdError(f"forcing of {name!r}: a Relaxation, a StochasticForcing, a Source or a tuple with at most one of each, not "
                              f"{type(bad).__name__}")
    return (relax[0] if relax else None), (stir[0] if stir else None), (source[0] if source else None)


def check_stochastic(forcing, grid, names, tracer_names, members=None, conservative=False):
    """The refusals of the StochasticForcing entries of `forcing` (which has passed check_forcing), before anything is
    allocated, and the draw groups of the model: a list of dicts (kind, names, forcing, modes, rate) in the order of the fields, rate a
    float or an array (members,) -- or None without the class or with rates that are all 0, and then the model makes exactly the calls
    it makes without it."""
    if not forcing:
        return None
    fields = tuple(names) + tuple(tracer_names)
    stir = {n: s for n, s in ((n, split_entry(n, v)[1]) for n, v in forcing.items()) if s is not None}
    if not stir:
        return None
    if grid.topo_codes() != (_lib.PERIODIC, _lib.PERIODIC):
        raise _lib.SwmhdError("StochasticForcing needs a (Periodic, Periodic) grid (SWMHD_ENOTSUP): its modes are periodic")
    mom = fields[:2]
    if any(n in stir for n in mom):
        if conservative:
            raise _lib.SwmhdError(f"StochasticForcing on {mom[0]!r}, {mom[1]!r} is not supported (SWMHD_ENOTSUP): the conservative "
                                  "formulation would need h F; stir the vector-invariant model")
        if not all(n in stir for n in mom) or stir[mom[0]] is not stir[mom[1]]:
            raise _lib.SwmhdError(f"StochasticForcing on the momentum: the SAME object under {mom[0]!r} and {mom[1]!r} (one stream "
                                  "function stirs both); one name without the other is refused")
    first = next(iter(stir.values()))
    if any((s.seed, s.stream) != (first.seed, first.stream) for s in stir.values()):
        raise _lib.SwmhdError("StochasticForcing: the entries of one model share one seed and one stream (their draws differ by group)")
    groups = []
    for n in fields:
        s = stir.get(n)
        if s is None or n == mom[1]:
            continue
        pair = n == mom[0]
        if np.ndim(s.rate) == 1 and (members is None or s.rate.shape[0] != members):
            raise _lib.SwmhdError(f"forcing of {n}: {s.rate.shape[0]} rates" + (" belong to an ensemble" if members is None else
                                                                                   f" for {members} members (a scalar or one per member)"))
        modes = forcing_modes(grid, s.k_f, s.dk)
        if len(modes) == 0 or len(modes) > MAX_MODES:
            raise _lib.SwmhdError(f"forcing of {n}: {len(modes)} modes in the ring k_f = {s.k_f}, dk = {s.dk} (1 .. {MAX_MODES}: "
                                  "SWMHD_STOCHASTIC_MAX_MODES)")
        groups.append(dict(kind=PAIR if pair else SCALAR, names=mom if pair else (n,), forcing=s, modes=modes, rate=s.rate))
    if not any(np.any(np.asarray(g["rate"]) != 0.0) for g in groups):
        return None
    return groups


def forcing_for_member(forcing, m):
    """The `forcing=` argument of member m of an ensemble: every Relaxation, Source and StochasticForcing in it by its for_member; one
    StochasticForcing under two names stays one object."""
    if forcing is None:
        return None
    made = {}
    one = lambda v: made.setdefault(id(v), v.for_member(m))
    return {n: tuple(one(v) for v in r) if isinstance(r, tuple) else one(r) for n, r in forcing.items()}


def check_forcing(forcing, grid, names, tracer_names, members=None, slabs=False, ring=False, fused=True, bounded_ensemble=False):
    """The refusals of a model or ensemble with `forcing`, before anything is allocated; a value is a Relaxation, a StochasticForcing
    (swmhd_amd.stochastic, whose own refusals check_stochastic makes), a Source (check_source builds its field) or a tuple with at most
    one of each.  Returns the forced fields in the order of
    `names` then `tracer_names`, as a list of (name, rate, mask, target) of host values (Relaxation.evaluate; rate a float or an array
    (members,)), the fields whose rates are all 0 left out -- or None where nothing is left, and then the model makes exactly the calls
    it makes without the argument."""
    if forcing is None:
        return None
    if not isinstance(forcing, dict):
        raise _lib.SwmhdError(f"forcing: a dict {{field name: Relaxation | StochasticForcing | Source}} or None, not {type(forcing).__name__}")
    if not forcing:
        return None
    fields = tuple(names) + tuple(tracer_names)
    other = {"u": "uh", "v": "vh", "uh": "u", "vh": "v"}
    for n, r in forcing.items():
        if n not in fields:
            if n in other and other[n] in fields:
                raise _lib.SwmhdError(f"forcing of {n!r}: this formulation's prognostic field is {other[n]!r}, and the term acts on the "
                                      "prognostic field of its name")
            raise _lib.SwmhdError(f"forcing of {n!r}: the prognostic fields are {fields!r}")
        split_entry(n, r)      # a Relaxation, a StochasticForcing, a Source or a tuple with at most one of each
    if bounded_ensemble:
        raise _lib.SwmhdError("forcing on a Bounded ensemble is not supported (SWMHD_ENOTSUP): swmhd_ensemble_step_rk3_bc is one native "
                              "call and has no per-stage entry point for the correction launch")
    if slabs:
        raise _lib.SwmhdError("forcing on a y-slab decomposition is not supported (SWMHD_ENOTSUP): one rank only")
    if ring:
        raise _lib.SwmhdError("forcing with ring= is not supported (SWMHD_ENOTSUP): the slab driver steps the four fields only")
    if not fused:
        raise _lib.SwmhdError("forcing needs the fused stage kernel (SWMHD_ENOTSUP): fused=False leaves no copy of the state a stage "
                              "started from")
    out = []
    for n in fields:
        r = split_entry(n, forcing[n])[0] if n in forcing else None
        if r is None:
            continue
        mask, target = r.evaluate(grid, LOCS.get(n, (Center, Center)), n, members)
        if np.any(np.asarray(r.rate) != 0.0):
            out.append((n, r.rate if members is None else (np.full(members, r.rate) if np.ndim(r.rate) == 0 else r.rate), mask, target))
    return out or None


def padded(grid, arr):
    """`arr` (..., Ny, Nx) as float64 halo-padded parents (..., Ny + 2 Hy, Nx + 2 Hx), halos 0 (they are never read)."""
    full = np.zeros(arr.shape[:-2] + grid.parent_shape)
    full[(Ellipsis,) + grid.interior] = arr
    return full


def device_parents(grid, arr, dtype, device):
    """`arr` (None, or (Ny, Nx) / (members, Ny, Nx) host values) on the device as halo-padded parents of the model's parent shape and
    pitch, rounded to `dtype`; None stays None."""
    import torch
    if arr is None:
        return None
    return torch.from_numpy(np.ascontiguousarray(padded(grid, arr))).to(device=device, dtype=dtype)
