"""ScalarDiffusivity: Oceananigans' `closure = ScalarDiffusivity(ν = ..., κ = (A = η, c = ...))` for the shallow-water MHD engine --
ν ∇²(u, v) and κ ∇²(A, tracers), one extra launch per RK3 stage (swmhd_diffusion_rk3_* in include/swmhd_diffusion.h).  h is never
diffused.  ScalarBiharmonicDiffusivity: Oceananigans' hyperviscosity closure of the same name, -ν ∇⁴(u, v) and -κ ∇⁴(A, tracers), one
more launch per RK3 stage (swmhd_biharmonic_rk3_* in include/swmhd_biharmonic.h).  `closure=` takes either, or a tuple with at most one
of each.  Nothing here touches a device."""
import math

import numpy as np

from . import _lib

# the RK3 stability bound on the negative real axis: |R(z)| <= 1 for z in [-2.51, 0], R(z) = 1 + z + z^2/2 + z^3/6
RK3_REAL_AXIS_BOUND = 2.51


def _checked(value, what, cls="ScalarDiffusivity"):
    """`value` as a float, or as a float64 array for a sequence (one value per member of an ensemble); finite and >= 0."""
    arr = np.asarray(value, dtype=np.float64)
    if arr.ndim > 1 or not np.all(np.isfinite(arr)) or np.any(arr < 0):
        raise _lib.SwmhdError(f"{cls}: {what} = {value!r}: finite values >= 0 (a scalar, or one per member of an ensemble)")
    return float(arr) if arr.ndim == 0 else arr.copy()


class ScalarDiffusivity:
    """nu: the viscosity of u and v.  kappa: the diffusivity of A and of every tracer -- a scalar for all of them, or a dict by name
    ({"A": eta, "c": ...}; names left out get 0).  For a ShallowWaterEnsemble every value may be a sequence with one entry per member.
    The time step is not limited by the closure: see max_stable_dt."""

    def __init__(self, nu=0.0, kappa=0.0):
        self.nu = _checked(nu, "nu")
        if isinstance(kappa, dict):
            for n in kappa:
                if not isinstance(n, str):
                    raise _lib.SwmhdError(f"ScalarDiffusivity: kappa key {n!r} is not a field name")
            self.kappa = {n: _checked(v, f"kappa[{n!r}]") for n, v in kappa.items()}
        else:
            self.kappa = _checked(kappa, "kappa")

    def __repr__(self):
        return f"ScalarDiffusivity(nu={self.nu!r}, kappa={self.kappa!r})"

    def coefficients(self, names, tracer_names=()):
        """The coefficient of every field of `names` (the four prognostic names of the model) followed by the tracers, in that order:
        nu for the first two, 0 for h, kappa for A and the tracers.  SwmhdError for a kappa name that is neither A nor a tracer."""
        diffused = ("A",) + tuple(tracer_names)
        if isinstance(self.kappa, dict):
            unknown = [n for n in self.kappa if n not in diffused]
            if unknown:
                raise _lib.SwmhdError(f"ScalarDiffusivity: kappa names {unknown!r}: the fields kappa applies to are {diffused!r}")
        kap = (lambda n: self.kappa.get(n, 0.0)) if isinstance(self.kappa, dict) else (lambda n: self.kappa)
        out = {names[0]: self.nu, names[1]: self.nu, names[2]: 0.0, names[3]: kap("A")}
        out.update({n: kap(n) for n in tracer_names})
        return out

    def for_member(self, m):
        """The closure of member m of an ensemble: every per-member sequence replaced by its entry m."""
        pick = lambda v: float(v[m]) if np.ndim(v) else v
        kappa = {n: pick(v) for n, v in self.kappa.items()} if isinstance(self.kappa, dict) else pick(self.kappa)
        return ScalarDiffusivity(pick(self.nu), kappa)

    def max_stable_dt(self, grid):
        """2.51 / (4 max(c) (1/dx² + 1/dy²)): the largest dt at which RK3 damps the grid-scale mode of the 5-point Laplacian with the
        largest coefficient (its eigenvalue is -4 c (1/dx² + 1/dy²); RK3 is stable on the negative real axis down to -2.51).  inf
        without diffusion.  Documented, not enforced: advection and waves limit dt as well."""
        values = [self.nu] + (list(self.kappa.values()) if isinstance(self.kappa, dict) else [self.kappa])
        cmax = max(float(np.max(v)) for v in values)
        if cmax == 0.0:
            return math.inf
        return RK3_REAL_AXIS_BOUND / (4.0 * cmax * (1.0 / grid.dx ** 2 + 1.0 / grid.dy ** 2))


def _checked4(value, what):
    return _checked(value, what, "ScalarBiharmonicDiffusivity")


class ScalarBiharmonicDiffusivity:
    """Hyperviscosity: -nu ∇²∇²(u, v) and -kappa ∇²∇²(A, tracers).  nu and kappa as ScalarDiffusivity's -- a scalar, kappa also a dict
    by name ({"A": eta4, "c": ...}; names left out get 0), every value a sequence with one entry per member for a ShallowWaterEnsemble --
    in units of length⁴ / time.  The time step is not limited by the closure: see max_stable_dt."""

    def __init__(self, nu=0.0, kappa=0.0):
        self.nu = _checked4(nu, "nu")
        if isinstance(kappa, dict):
            for n in kappa:
                if not isinstance(n, str):
                    raise _lib.SwmhdError(f"ScalarBiharmonicDiffusivity: kappa key {n!r} is not a field name")
            self.kappa = {n: _checked4(v, f"kappa[{n!r}]") for n, v in kappa.items()}
        else:
            self.kappa = _checked4(kappa, "kappa")

    def __repr__(self):
        return f"ScalarBiharmonicDiffusivity(nu={self.nu!r}, kappa={self.kappa!r})"

    def coefficients(self, names, tracer_names=()):
        """The coefficient of every field of `names` (the four prognostic names of the model) followed by the tracers, in that order:
        nu for the first two, 0 for h, kappa for A and the tracers.  SwmhdError for a kappa name that is neither A nor a tracer."""
        diffused = ("A",) + tuple(tracer_names)
        if isinstance(self.kappa, dict):
            unknown = [n for n in self.kappa if n not in diffused]
            if unknown:
                raise _lib.SwmhdError(f"ScalarBiharmonicDiffusivity: kappa names {unknown!r}: the fields kappa applies to are {diffused!r}")
        kap = (lambda n: self.kappa.get(n, 0.0)) if isinstance(self.kappa, dict) else (lambda n: self.kappa)
        out = {names[0]: self.nu, names[1]: self.nu, names[2]: 0.0, names[3]: kap("A")}
        out.update({n: kap(n) for n in tracer_names})
        return out

    def for_member(self, m):
        """The closure of member m of an ensemble: every per-member sequence replaced by its entry m."""
        pick = lambda v: float(v[m]) if np.ndim(v) else v
        kappa = {n: pick(v) for n, v in self.kappa.items()} if isinstance(self.kappa, dict) else pick(self.kappa)
        return ScalarBiharmonicDiffusivity(pick(self.nu), kappa)

    def max_stable_dt(self, grid):
        """2.51 / (max(c) (4/dx² + 4/dy²)²): the largest dt at which RK3 damps the grid-scale mode of the 13-point operator with the
        largest coefficient (its eigenvalue is -c (4/dx² + 4/dy²)², the square of the 5-point Laplacian's; RK3 is stable on the negative
        real axis down to -2.51).  inf without diffusion.  Documented, not enforced: advection and waves limit dt as well."""
        values = [self.nu] + (list(self.kappa.values()) if isinstance(self.kappa, dict) else [self.kappa])
        cmax = max(float(np.max(v)) for v in values)
        if cmax == 0.0:
            return math.inf
        return RK3_REAL_AXIS_BOUND / (cmax * (4.0 / grid.dx ** 2 + 4.0 / grid.dy ** 2) ** 2)


def split_closure(closure):
    """(ScalarDiffusivity or None, ScalarBiharmonicDiffusivity or None) of a `closure=` argument: None, one closure, or a tuple or list
    with at most one of each kind (Oceananigans' closure tuple).  SwmhdError for anything else."""
    if closure is None:
        return None, None
    items = tuple(closure) if isinstance(closure, (tuple, list)) else (closure,)
    lap = bih = None
    for c in items:
        if isinstance(c, ScalarDiffusivity):
            if lap is not None:
                raise _lib.SwmhdError("closure: a tuple holds at most one ScalarDiffusivity")
            lap = c
        elif isinstance(c, ScalarBiharmonicDiffusivity):
            if bih is not None:
                raise _lib.SwmhdError("closure: a tuple holds at most one ScalarBiharmonicDiffusivity")
            bih = c
        else:
            raise _lib.SwmhdError("closure: a ScalarDiffusivity, a ScalarBiharmonicDiffusivity, a tuple with at most one of each, or None, "
                                  f"not {type(c).__name__}")
    return lap, bih


def closure_for_member(closure, m):
    """The `closure=` argument of member m of an ensemble: every closure in it by its for_member."""
    if closure is None:
        return None
    if isinstance(closure, (tuple, list)):
        return tuple(c.for_member(m) for c in closure)
    return closure.for_member(m)


def check_closure(closure, names, tracer_names, formulation_is_conservative, bounded=False, slabs=False, ring=False, fused=True):
    """The refusals of a model or ensemble with `closure`, before anything is allocated; returns (the Laplacian coefficients by field
    name, the biharmonic coefficients by field name), each None where `closure` has no closure of that kind."""
    lap, bih = split_closure(closure)
    if lap is None and bih is None:
        return None, None
    coefs = tuple(c.coefficients(names, tracer_names) if c is not None else None for c in (lap, bih))
    if bounded:
        raise _lib.SwmhdError("closure on a grid with a Bounded direction is not supported (SWMHD_ENOTSUP): the wall faces of u and v "
                              "and the gradient conditions need a kernel body of their own")
    if slabs:
        raise _lib.SwmhdError("closure on a y-slab decomposition is not supported (SWMHD_ENOTSUP): one rank only")
    if ring:
        raise _lib.SwmhdError("closure with ring= is not supported (SWMHD_ENOTSUP): the slab driver steps the four fields only")
    if not fused:
        raise _lib.SwmhdError("closure needs the fused stage kernel (SWMHD_ENOTSUP): fused=False leaves no copy of the state a stage "
                              "started from")
    if formulation_is_conservative and any(c is not None and np.any(np.asarray(c.nu) != 0) for c in (lap, bih)):
        raise _lib.SwmhdError("closure: nu != 0 with ConservativeFormulation is not supported (SWMHD_ENOTSUP): Oceananigans' conservative "
                              "viscous stress nu h grad(uh / h) is a different operator; kappa works in both formulations")
    return coefs
