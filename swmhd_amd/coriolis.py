"""Coriolis parameters: Oceananigans' `coriolis = FPlane(f = ...)` and `coriolis = BetaPlane(f₀ = ..., β = ...)` for the shallow-water MHD
engine, and any f(y) as a callable.  FPlane(f) is the model's scalar `coriolis_f`.  A parameter that varies with y runs the stage kernels
with f = 0 and adds f(y_j) (v̄, -ū) by one extra launch per RK3 stage (swmhd_coriolis_rk3_* in include/swmhd_coriolis.h).  Nothing here
touches a device."""
import numpy as np

from . import _lib


def _checked(value, what):
    """`value` as a float, or as a float64 array for a sequence (one value per member of an ensemble); finite."""
    arr = np.asarray(value, dtype=np.float64)
    if arr.ndim > 1 or not np.all(np.isfinite(arr)):
        raise _lib.SwmhdError(f"{what} = {value!r}: finite values (a scalar, or one per member of an ensemble)")
    return float(arr) if arr.ndim == 0 else arr.copy()


def _pick(v, m):
    return float(v[m]) if np.ndim(v) else v


class CoriolisProfile:
    """f(y) given as a callable on numpy arrays of y.  rows(grid) evaluates it at the centres and at the south faces of the grid's
    rows -- where u and v live -- from the grid's own coordinates, which include a slab's j_offset."""

    def __init__(self, func):
        if not callable(func):
            raise _lib.SwmhdError(f"CoriolisProfile: a callable f(y), not {type(func).__name__}")
        self.func = func

    def __repr__(self):
        return f"CoriolisProfile({self.func!r})"

    def f(self, y):
        return self.func(y)

    def rows(self, grid):
        """(fc, ff): f at grid.yc and at grid.yf of the Ny interior rows, float64 arrays of shape (Ny,) -- or (members, Ny) where a
        parameter has one value per member."""
        sl = slice(grid.Hy, grid.Hy + grid.Ny)
        out = []
        for y in (grid.yc[sl], grid.yf[sl]):
            v = np.asarray(self.f(y), dtype=np.float64)
            if v.shape[-1:] != y.shape or v.ndim > 2:
                v = v + np.zeros_like(y)      # (a callable that returns a constant)
            if not np.all(np.isfinite(v)):
                raise _lib.SwmhdError(f"{self!r}: f(y) is not finite on the rows of the grid")
            out.append(v)
        return tuple(out)

    def for_member(self, m):
        """The parameter of member m of an ensemble: every per-member sequence replaced by its entry m."""
        return self

    @property
    def per_member(self):
        """The number of members the parameter has values for, or None where every value is a scalar."""
        return None


class FPlane(CoriolisProfile):
    """A constant f: the model's `coriolis_f` (a scalar, or for an ensemble one value per member), inside the stage kernels."""

    def __init__(self, f=1.0):
        self.f0 = _checked(f, "FPlane: f")

    def __repr__(self):
        return f"FPlane(f={self.f0!r})"

    def f(self, y):
        return np.multiply.outer(np.asarray(self.f0), np.ones_like(y))

    def for_member(self, m):
        return FPlane(_pick(self.f0, m))

    @property
    def per_member(self):
        return len(self.f0) if np.ndim(self.f0) else None


class BetaPlane(CoriolisProfile):
    """f = f0 + beta y, y the grid's own coordinate.  For a ShallowWaterEnsemble f0 and beta may each be a sequence with one entry per
    member."""

    def __init__(self, f0=1.0, beta=0.0):
        self.f0, self.beta = _checked(f0, "BetaPlane: f0"), _checked(beta, "BetaPlane: beta")
        n = {len(v) for v in (self.f0, self.beta) if np.ndim(v)}
        if len(n) > 1:
            raise _lib.SwmhdError(f"BetaPlane: f0 and beta have {sorted(n)} values: one per member each, or scalars")

    def __repr__(self):
        return f"BetaPlane(f0={self.f0!r}, beta={self.beta!r})"

    def f(self, y):
        if np.ndim(self.f0) or np.ndim(self.beta):
            return np.asarray(self.f0).reshape(-1, 1) + np.asarray(self.beta).reshape(-1, 1) * y
        return self.f0 + self.beta * y

    def for_member(self, m):
        return BetaPlane(_pick(self.f0, m), _pick(self.beta, m))

    @property
    def per_member(self):
        n = [len(v) for v in (self.f0, self.beta) if np.ndim(v)]
        return n[0] if n else None


def check_coriolis(coriolis, coriolis_f, default_f, slabs=False, ring=False, fused=True):
    """`coriolis=` of a model or an ensemble, before anything is allocated.  Returns (f for the stage kernels, the parameter whose rows
    go into the table or None): None and FPlane give (coriolis_f or the FPlane's f, None) -- exactly the calls made without the
    argument -- anything else (0.0, coriolis).  SwmhdError for what is not supported."""
    if coriolis is None:
        return coriolis_f, None
    if not isinstance(coriolis, CoriolisProfile):
        raise _lib.SwmhdError(f"coriolis: an FPlane, a BetaPlane, a CoriolisProfile or None, not {type(coriolis).__name__}")
    if not (np.ndim(coriolis_f) == 0 and float(coriolis_f) == default_f):
        raise _lib.SwmhdError("coriolis= and coriolis_f= are two names of one parameter: give one of them")
    if isinstance(coriolis, FPlane):
        return coriolis.f0, None
    if slabs:
        raise _lib.SwmhdError("coriolis = f(y) on a y-slab decomposition is not supported (SWMHD_ENOTSUP): one rank only")
    if ring:
        raise _lib.SwmhdError("coriolis = f(y) with ring= is not supported (SWMHD_ENOTSUP): the slab driver has no per-stage entry for the "
                              "correction launch")
    if not fused:
        raise _lib.SwmhdError("coriolis = f(y) needs the fused stage kernel (SWMHD_ENOTSUP): fused=False leaves no copy of the state a "
                              "stage started from")
    return 0.0, coriolis


def row_table(coriolis, grid, members=None):
    """The host table of swmhd_[ensemble_]coriolis_rk3_*: float64 (2, Ny) -- fc then ff -- or (members, 2, Ny)."""
    fc, ff = coriolis.rows(grid)
    tab = np.stack([fc, ff], axis=-2)
    if members is None:
        if tab.ndim != 2:
            raise _lib.SwmhdError(f"{coriolis!r}: per-member values belong to an ensemble")
        return np.ascontiguousarray(tab)
    if tab.ndim == 2:
        tab = np.repeat(tab[None], members, axis=0)
    if tab.shape[0] != members:
        raise _lib.SwmhdError(f"{coriolis!r}: {tab.shape[0]} values for {members} members (a scalar or one per member)")
    return np.ascontiguousarray(tab)
