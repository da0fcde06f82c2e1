"""StochasticForcing: band-limited stirring that is white in time, for forced-dissipative turbulence runs -- the term Oceananigans users
write as a per-iteration callback that refills a forcing array.  `forcing={"u": s, "v": s}` with ONE StochasticForcing under both
momentum names stirs the flow with F = (-δy ψ, δx ψ) of a random corner stream function ψ, exactly non-divergent on the C-grid;
`forcing={"A": s}` adds a random source to any centre field.  The coefficients are drawn on the device once per time step from a
counter-based generator (Philox4x32-10: reproducible bit for bit from `seed`, `stream` and the step counter) and held over the three
RK3 stages; every stage adds the synthesised field in one launch, after the other corrections (include/swmhd_stochastic.h states the
formulas).  The checks of a `forcing=` argument stand in swmhd_amd.forcing (check_stochastic), which imports this module; this one
imports nothing from it.  Only StochasticState touches a device, and only when a model that has passed its checks asks for it."""
import ctypes
import math

import numpy as np

from . import _lib
from .fields import LOCS
from .grid import Center

MAX_MODES = _lib.STOCHASTIC_MAX_MODES
SCALAR, PAIR = 0, 1


class StochasticForcing:
    """rate: the mean injection rate, a finite scalar >= 0, for a ShallowWaterEnsemble also one value per member -- of kinetic energy
    per unit mass for the vortical pair (½ dt <|F|²> = rate), of ½φ² for a scalar field.  k_f, dk: the ring of forced wavenumbers,
    k_f - dk/2 <= |k| < k_f + dk/2 (forcing_modes).  seed: 0 .. 2^64 - 1, the generator's key.  stream: 0 .. 2^32 - 1; member m of an
    ensemble draws with stream + m.  A model's entries share one seed and one stream: their draws differ by their group index."""

    def __init__(self, rate, k_f, dk, seed=0, stream=0):
        r = np.asarray(rate, dtype=np.float64) if not callable(rate) else None
        if r is None or r.ndim > 1 or not np.all(np.isfinite(r)) or np.any(r < 0):
            raise _lib.SwmhdError(f"StochasticForcing: rate = {rate!r}: finite values >= 0 (a scalar, or one per member of an ensemble)")
        self.rate = float(r) if r.ndim == 0 else r.copy()
        for what, v in (("k_f", k_f), ("dk", dk)):
            if not (isinstance(v, (int, float, np.integer, np.floating)) and math.isfinite(v) and v > 0):
                raise _lib.SwmhdError(f"StochasticForcing: {what} = {v!r}: a finite wavenumber > 0")
        self.k_f, self.dk = float(k_f), float(dk)
        for what, v, bits in (("seed", seed, 64), ("stream", stream, 32)):
            if not (isinstance(v, (int, np.integer)) and 0 <= int(v) < (1 << bits)):
                raise _lib.SwmhdError(f"StochasticForcing: {what} = {v!r}: an integer 0 .. 2^{bits} - 1")
        self.seed, self.stream = int(seed), int(stream)

    def __repr__(self):
        return f"StochasticForcing(rate={self.rate!r}, k_f={self.k_f!r}, dk={self.dk!r}, seed={self.seed}, stream={self.stream})"

    def for_member(self, m):
        """The StochasticForcing of member m of an ensemble: its rate, and the stream stream + m (mod 2^32)."""
        rate = float(self.rate[m]) if np.ndim(self.rate) else self.rate
        return StochasticForcing(rate, self.k_f, self.dk, self.seed, (self.stream + m) & 0xffffffff)


def forcing_modes(grid, k_f, dk):
    """The integer pairs (nx, ny), an int array (M, 2) ordered by nx then ny, with 0 <= nx < Nx/2, |ny| < Ny/2 (the integer
    quotients, as in C: an odd size leaves its highest wavenumber out, as an even one leaves its Nyquist wavenumber out), in the
    half-plane nx > 0 or (nx == 0 and ny > 0), and k_f - dk/2 <= hypot(2π nx/Lx, 2π ny/Ly) < k_f + dk/2."""
    nx, ny = np.meshgrid(np.arange(0, grid.Nx // 2), np.arange(-(grid.Ny // 2) + 1, grid.Ny // 2), indexing="ij")
    k = np.hypot(2.0 * np.pi * nx / grid.Lx, 2.0 * np.pi * ny / grid.Ly)
    keep = (k >= k_f - dk / 2) & (k < k_f + dk / 2) & ((nx > 0) | (ny > 0))
    return np.stack([nx[keep], ny[keep]], axis=1).astype(np.int64).reshape(-1, 2)      # (row-major: by nx, then ny)


def wavenumbers(grid, modes):
    """(kx, ky) of `modes` as float64 arrays (M,)."""
    return 2.0 * np.pi * modes[:, 0] / grid.Lx, 2.0 * np.pi * modes[:, 1] / grid.Ly


def modified_wavenumbers(grid, modes):
    """(k̃x, k̃y) = (sin(kx dx/2)/(dx/2), sin(ky dy/2)/(dy/2)): what the C-grid's two-point difference makes of a mode."""
    kx, ky = wavenumbers(grid, modes)
    return np.sin(kx * grid.dx / 2) / (grid.dx / 2), np.sin(ky * grid.dy / 2) / (grid.dy / 2)


def amplitudes(grid, modes, rate, pair):
    """amp0 (M,) in float64: sqrt(6 rate / M), for the vortical pair divided by hypot(k̃x, k̃y)."""
    amp = np.full(len(modes), np.sqrt(6.0 * rate / len(modes)))
    return amp / np.hypot(*modified_wavenumbers(grid, modes)) if pair else amp


def _nodes(grid, loc):
    x = (grid.xc if loc[0] == Center else grid.xf)[grid.Hx:grid.Hx + grid.Nx]
    y = (grid.yc if loc[1] == Center else grid.yf)[grid.Hy:grid.Hy + grid.Ny]
    return x, y


def x_table(grid, modes, loc):
    """(2 M, Nx) float64: row 2 m = cos(kx_m x_i), row 2 m + 1 = sin(kx_m x_i) at the interior nodes of a field at `loc`."""
    kx, _ = wavenumbers(grid, modes)
    arg = kx[:, None] * _nodes(grid, loc)[0][None, :]
    return np.stack([np.cos(arg), np.sin(arg)], axis=1).reshape(2 * len(modes), grid.Nx)


def y_table(grid, modes, loc):
    """(2 M, Ny) float64: row 2 m = cos(ky_m y_j), row 2 m + 1 = sin(ky_m y_j)."""
    _, ky = wavenumbers(grid, modes)
    arg = ky[:, None] * _nodes(grid, loc)[1][None, :]
    return np.stack([np.cos(arg), np.sin(arg)], axis=1).reshape(2 * len(modes), grid.Ny)


class StochasticState:
    """What a model or an ensemble with a stochastic forcing holds on the device: the step counter (one uint64 per member, kept in an
    int64 tensor), the coefficient pairs of the current step, the amplitude and wavenumber tables of the draw, and the x and y tables
    of every stirred field.  `fields`: (name, mode count, coefficient pointer, x table pointer, y table pointer) in launch order."""

    def __init__(self, groups, grid, dtype, device, members=None):
        import torch
        self.members, self.ensemble = (members or 1), members is not None
        self.seed, self.stream = groups[0]["forcing"].seed, groups[0]["forcing"].stream
        self.counter = torch.zeros(self.members, dtype=torch.int64, device=device)
        self.substreams = torch.tensor([((self.stream + m) & 0xffffffff) - (1 << 32 if (self.stream + m) & 0x80000000 else 0)
                                        for m in range(self.members)], dtype=torch.int32, device=device)
        sizes = [(4 if g["kind"] == PAIR else 2) * len(g["modes"]) for g in groups]
        self.coef_stride = sum(sizes)
        self.coefficients = torch.zeros((self.members, self.coef_stride), dtype=dtype, device=device)
        elem = self.coefficients.element_size()
        up64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device)
        self.kinds = [g["kind"] for g in groups]
        self.nmodes = [len(g["modes"]) for g in groups]
        self.max_modes = max(self.nmodes)
        self._amp, self._ktx, self._kty, self._tables = [], [], [], []
        self.fields, offset = [], 0
        Px = grid.parent_shape[1]
        self.x_pitch, self.y_pitch = Px, grid.Ny
        for g, size in zip(groups, sizes):
            M, pair = len(g["modes"]), g["kind"] == PAIR
            rates = np.broadcast_to(np.asarray(g["rate"], dtype=np.float64), (self.members,))
            # (members, max_modes): one pitch for every group of the call
            amp = np.zeros((self.members, self.max_modes))
            for m in range(self.members):
                amp[m, :M] = amplitudes(grid, g["modes"], rates[m], pair)
            self._amp.append(up64(amp))
            ktx, kty = modified_wavenumbers(grid, g["modes"])
            self._ktx.append(up64(ktx))
            self._kty.append(up64(kty))
            for k, n in enumerate(g["names"]):
                loc = LOCS.get(n, (Center, Center))
                # x table: rows of the parents' pitch with the interior at column Hx, so that it shares the fields' 16-byte phase
                xt = np.zeros((2 * M, Px))
                xt[:, grid.Hx:grid.Hx + grid.Nx] = x_table(grid, g["modes"], loc)
                xt = torch.from_numpy(xt).to(device=device, dtype=dtype)
                yt = torch.from_numpy(y_table(grid, g["modes"], loc)).to(device=device, dtype=dtype)
                self._tables += [xt, yt]
                self.fields.append((n, M, self.coefficients.data_ptr() + (offset + 2 * M * k) * elem, xt.data_ptr() + grid.Hx * elem,
                                    yt.data_ptr()))
            offset += size
        P, I = _lib.ptr_array, lambda v: (ctypes.c_int * len(v))(*v)
        offs = np.cumsum([0] + sizes[:-1])
        self._draw_args = (P([self.coefficients.data_ptr() + int(o) * elem for o in offs]), P([a.data_ptr() for a in self._amp]),
                           P([a.data_ptr() for a in self._ktx]), P([a.data_ptr() for a in self._kty]), I(self.nmodes), I(self.kinds),
                           len(groups))

    def draw(self, o, dt):
        """Enqueue the coefficient draw of one time step of `o`: it reads and advances the device counter."""
        from .fields import _stream_ptr
        sdt = 1.0 / math.sqrt(dt)
        if self.ensemble:
            f = getattr(o._L, f"swmhd_ensemble_stochastic_coefficients_{o.sfx}")
            rc = f(self.counter.data_ptr(), *self._draw_args, self.members, self.coef_stride, self.max_modes, self.seed,
                   self.substreams.data_ptr(), sdt, _stream_ptr())
        else:
            f = getattr(o._L, f"swmhd_stochastic_coefficients_{o.sfx}")
            rc = f(self.counter.data_ptr(), *self._draw_args, self.seed, self.stream, sdt, _stream_ptr())
        _lib.check(rc, "swmhd_stochastic_coefficients")

    def counter_values(self):
        """The step counters as a uint64 host array (members,)."""
        return self.counter.cpu().numpy().view(np.uint64).copy()

    def set_counter(self, values):
        import torch
        v = np.broadcast_to(np.asarray(values, dtype=np.uint64), (self.members,)).copy()
        self.counter.copy_(torch.from_numpy(v.view(np.int64)))
