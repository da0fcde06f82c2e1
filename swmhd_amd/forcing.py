"""Relaxation: Oceananigans' `forcing = (u = Relaxation(rate, mask, target), h = ...)` for the shallow-water MHD engine -- the term
rate * mask(x, y) * (target(x, y) - φ) added to the tendency of the prognostic field φ of that name, one extra launch per RK3 stage for
all forced fields (swmhd_relaxation_rk3_* in include/swmhd_relaxation.h).  Large-scale drag is Relaxation(rate) on the two momentum-like
fields, a sponge layer a Relaxation with a mask, Newtonian relaxation of h one with a target array.  Only device_parents touches a
device, and only when a model that has passed its checks asks for it."""
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


def split_entry(name, value):
    """(Relaxation or None, StochasticForcing or None) of one value of the `forcing=` dict: either class, or a tuple with at most one
    of each."""
    items = value if isinstance(value, tuple) else (value,)
    relax = [v for v in items if isinstance(v, Relaxation)]
    stir = [v for v in items if isinstance(v, StochasticForcing)]
    if not items or len(relax) + len(stir) != len(items) or len(relax) > 1 or len(stir) > 1:
        bad = next((v for v in items if not isinstance(v, (Relaxation, StochasticForcing))), value)
        raise _lib.SwmhdError(f"forcing of {name!r}: a Relaxation, a StochasticForcing or a tuple with at most one of each, not "
                              f"{type(bad).__name__}")
    return (relax[0] if relax else None), (stir[0] if stir else None)


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
    """The `forcing=` argument of member m of an ensemble: every Relaxation and StochasticForcing in it by its for_member; one
    StochasticForcing under two names stays one object."""
    if forcing is None:
        return None
    made = {}
    one = lambda v: made.setdefault(id(v), v.for_member(m))
    return {n: tuple(one(v) for v in r) if isinstance(r, tuple) else one(r) for n, r in forcing.items()}


def check_forcing(forcing, grid, names, tracer_names, members=None, slabs=False, ring=False, fused=True, bounded_ensemble=False):
    """The refusals of a model or ensemble with `forcing`, before anything is allocated; a value is a Relaxation, a StochasticForcing
    (swmhd_amd.stochastic, whose own refusals check_stochastic makes) or a tuple with at most one of each.  Returns the forced fields in the order of
    `names` then `tracer_names`, as a list of (name, rate, mask, target) of host values (Relaxation.evaluate; rate a float or an array
    (members,)), the fields whose rates are all 0 left out -- or None where nothing is left, and then the model makes exactly the calls
    it makes without the argument."""
    if forcing is None:
        return None
    if not isinstance(forcing, dict):
        raise _lib.SwmhdError(f"forcing: a dict {{field name: Relaxation}} or None, not {type(forcing).__name__}")
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
        split_entry(n, r)      # a Relaxation, a StochasticForcing or a tuple with at most one of each
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
