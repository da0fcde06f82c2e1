"""numpy restatement of the output frames (swmhd_output_fields_* in include/swmhd.h), the yardstick of tests/test_output_*.py.

The reference's writer stores (u, v, A, s), s = sqrt(u^2 + v^2) (SWMHD_example.jl:67-68,80-84; divergence_sw_mhd.jl:64-66,75-82 with
u = uh / h, v = vh / h), and MHD_visualize.jl:55-65 looks at B_x = -dA/dy / h, B_y = dA/dx / h.  Placement as in
plot_cases.np_diagnostics: a binary operation sits where its first operand is, the second is interpolated there, a divisor field is
interpolated.  Everything in IEEE double, in the operation order the kernel documents, so the device frames can be compared bitwise.

Also here: the call matrix of tests/test_output_matrix_gpu.py (SHAPES .. ROW_RANGES), which cells of which parent a frame cell reads
(FIELD_REACH, REACH, keep_mask, reached_cells) and the periodic images the WRAP flags read (wrap_parents, images); all of it pinned on
the CPU by tests/test_output_cases_cpu.py."""
import numpy as np

NAMES = ("u", "v", "h", "A", "s", "B_x", "B_y")
BITS = {n: 1 << k for k, n in enumerate(NAMES)}            # SWMHD_OUT_*: bit k of `which` is field k, and the frame's slots are in bit order
ALL = 127
PARENTS = ("q1", "q2", "h", "A")
WRAP_X, WRAP_Y = 16, 32                                    # SWMHD_WRAP_X, SWMHD_WRAP_Y

# ---- the call matrix of tests/test_output_matrix_gpu.py -----------------------------------------------------------------------------
# (Nx, Ny), the edge shapes of derived_cases.SHAPES: one cell (under wrap the west neighbour is the cell itself, ym = yp = 0); less than
# a chunk of 4 cells; one chunk exactly; 1, 3, 0 and 1 cells in the last chunk; a row of exactly 16 chunks; 257 chunks x 2 rows = 514
# threads, so the (row, chunk) decode crosses a 256-thread workgroup
SHAPES = ((1, 1), (2, 3), (4, 1), (5, 2), (7, 9), (64, 2), (65, 3), (1025, 2))
HALOS = ((1, 1), (3, 2))
ALL_MASKS = range(1, 128)


def mask_of(*names):
    return sum(BITS[n] for n in set(names))


# each single name, all seven, the writer's default frame, (s,), (B_x, B_y), (v, B_x)
MASKS = tuple(dict.fromkeys([BITS[n] for n in NAMES] + [ALL, mask_of("u", "v", "A", "s"), mask_of("s"), mask_of("B_x", "B_y"),
                                                        mask_of("v", "B_x")]))


def ROW_RANGES(Ny):
    """all rows, [1, Ny), [0, 1) and an empty range (which writes nothing); each once"""
    return tuple(dict.fromkeys([(0, Ny), (1, Ny), (0, 1), (min(1, Ny), min(1, Ny))]))


def mask_names(which):
    return tuple(n for n in NAMES if which & BITS[n])


# ---- reach: which cells of which parent a frame cell (i, j) reads, as offsets (di, dj), read off the definitions above ---------------
# FIELD_REACH[form][field][parent]; a parent that is absent is not read by that field.  form 1 = vector-invariant, 0 = conservative.
_C, _W, _S = (0, 0), (-1, 0), (0, -1)
_V4 = {_W, _C, (-1, 1), (0, 1)}                            # V at (i-1, j), (i, j), (i-1, j+1), (i, j+1): what the speed averages
FIELD_REACH = {
    1: {"u": {"q1": {_C}}, "v": {"q2": {_C}}, "h": {"h": {_C}}, "A": {"A": {_C}},
        "s": {"q1": {_C}, "q2": _V4},
        "B_x": {"A": {_C, _S}, "h": {_S, _C}},
        "B_y": {"A": {_C, _W}, "h": {_W, _C}}},
    0: {"u": {"q1": {_C}, "h": {_W, _C}}, "v": {"q2": {_C}, "h": {_S, _C}}, "h": {"h": {_C}}, "A": {"A": {_C}},
        # U(i, j): h west and here; V(i', j'): h south of it and at it, for the four V of _V4
        "s": {"q1": {_C}, "q2": _V4, "h": {(-1, -1), _W, (-1, 1), _S, _C, (0, 1)}},
        "B_x": {"A": {_C, _S}, "h": {_S, _C}},
        "B_y": {"A": {_C, _W}, "h": {_W, _C}}},
}
# REACH[form][parent]: the offsets at which ANY field reads that parent
REACH = {form: {p: frozenset().union(*(r.get(p, ()) for r in fr.values())) for p in PARENTS} for form, fr in FIELD_REACH.items()}


def _wrapped(idx, N, on):
    return idx % N if on else idx


def keep_mask(Nx, Ny, Hx, Hy, form, parent, wrap=0):
    """(Ny + 2 Hy, Nx + 2 Hx) bool: the HALO cells of `parent` that some interior frame cell reads (REACH), neighbours of a wrapped
    direction taken at (x mod Nx, y mod Ny) as the kernel takes them -- so a wrapped direction keeps none of its halo."""
    read = np.zeros((Ny + 2 * Hy, Nx + 2 * Hx), dtype=bool)
    for di, dj in REACH[form][parent]:
        jj = _wrapped(np.arange(Ny) + dj, Ny, wrap & WRAP_Y)
        ii = _wrapped(np.arange(Nx) + di, Nx, wrap & WRAP_X)
        read[np.ix_(Hy + jj, Hx + ii)] = True
    read[Hy:Hy + Ny, Hx:Hx + Nx] = False
    return read


def reached_cells(Nx, Ny, form, name, parent, cell, wrap=0):
    """(Ny, Nx) bool: the cells of field `name` that read cell (J, I) of `parent` (FIELD_REACH); J, I count from the first interior
    cell, so a halo cell has a negative index or one from Ny / Nx on."""
    J, I = cell
    out = np.zeros((Ny, Nx), dtype=bool)
    for di, dj in FIELD_REACH[form][name].get(parent, ()):
        jj = _wrapped(np.arange(Ny) + dj, Ny, wrap & WRAP_Y)
        ii = _wrapped(np.arange(Nx) + di, Nx, wrap & WRAP_X)
        out |= (jj == J)[:, None] & (ii == I)[None, :]
    return out


def images(parents, Nx, Ny, Hx, Hy, wrap):
    """What the WRAP flags make of the parents: the halos of the wrapped directions replaced by the periodic images of the interior
    (wrap_parents, which this equals wherever a period covers the halo; here also for Nx < Hx or Ny < Hy), as float64."""
    ix = (np.arange(-Hx, Nx + Hx) % Nx) + Hx if wrap & WRAP_X else np.arange(Nx + 2 * Hx)
    iy = (np.arange(-Hy, Ny + Hy) % Ny) + Hy if wrap & WRAP_Y else np.arange(Ny + 2 * Hy)
    out = [np.asarray(a, dtype=np.float64)[np.ix_(iy, ix)] for a in parents]
    if Nx >= Hx and Ny >= Hy:
        ref = wrap_parents(parents, Nx, Ny, Hx, Hy, bool(wrap & WRAP_X), bool(wrap & WRAP_Y))
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(out, ref))
    return out


def wrap_parents(parents, Nx, Ny, Hx, Hy, wrap_x=True, wrap_y=True):
    """The parents with the halos of the wrapped directions replaced by the periodic images of the interior."""
    out = []
    for a in parents:
        a = np.array(a, dtype=np.float64)
        if wrap_x:
            a[:, :Hx], a[:, Hx + Nx:] = a[:, Nx:Nx + Hx].copy(), a[:, Hx:2 * Hx].copy()
        if wrap_y:
            a[:Hy, :], a[Hy + Ny:, :] = a[Ny:Ny + Hy, :].copy(), a[Hy:2 * Hy, :].copy()
        out.append(a)
    return out


def np_output_fields(q1, q2, h, A, Nx, Ny, Hx, Hy, dx, dy, form, names=NAMES, rows=None):
    """(len(names), rows, Nx) float64: the named fields at indices 1..Nx x rows [j0, j1) from halo-padded parents (halos as given).
    form 1 = vector-invariant (q = u, v), 0 = conservative (q = uh, vh)."""
    j0, j1 = (0, Ny) if rows is None else rows
    q1, q2, h, A = (np.asarray(a, dtype=np.float64) for a in (q1, q2, h, A))
    dx, dy = np.float64(dx), np.float64(dy)
    S = lambda a, di, dj: a[Hy + j0 + dj:Hy + j1 + dj, Hx + di:Hx + di + Nx]
    U = lambda di, dj: S(q1, di, dj) if form == 1 else S(q1, di, dj) / (0.5 * (S(h, di - 1, dj) + S(h, di, dj)))
    V = lambda di, dj: S(q2, di, dj) if form == 1 else S(q2, di, dj) / (0.5 * (S(h, di, dj - 1) + S(h, di, dj)))

    def field(n):
        if n == "u":
            return U(0, 0)
        if n == "v":
            return V(0, 0)
        if n == "h":
            return S(h, 0, 0)
        if n == "A":
            return S(A, 0, 0)
        if n == "s":
            g00, g10, g01, g11 = V(-1, 0), V(0, 0), V(-1, 1), V(0, 1)
            u = U(0, 0)
            return np.sqrt(u * u + 0.5 * (0.5 * (g00 * g00 + g10 * g10) + 0.5 * (g01 * g01 + g11 * g11)))
        if n == "B_x":
            return -((S(A, 0, 0) - S(A, 0, -1)) / dy) / (0.5 * (S(h, 0, -1) + S(h, 0, 0)))
        if n == "B_y":
            return ((S(A, 0, 0) - S(A, -1, 0)) / dx) / (0.5 * (S(h, -1, 0) + S(h, 0, 0)))
        raise KeyError(n)
    with np.errstate(all="ignore"):                        # NaN and Inf parents: the same results, no warnings
        return np.stack([np.array(field(n), dtype=np.float64) for n in names])


def kinetic_energy_from_frames(s, h, dx, dy):
    """Σ ½ h ℑxᶜ(s²) Δx Δy with x periodic (face Nx+1 is face 1): the kinetic energy of the Jacobian driver (SWMHD_example.jl:74)."""
    s2 = s * s
    return (0.5 * h * (0.5 * (s2 + np.roll(s2, -1, axis=1)))).sum() * (dx * dy)


def magnetic_density_from_frames(bx, by, h):
    """½ h ℑyᶜ[B_x² + ℑxyᶜᶠ(B_y²)] per cell, x and y periodic (SWMHD_example.jl:75 / divergence_sw_mhd.jl:72).  On a Bounded-y grid the
    first and the last row are wrong (they need B_y of the south halo row and the far-wall line of B_x, which are not part of a frame):
    sum rows [1:-1] there."""
    c = by * by
    east = np.roll(c, -1, axis=1)
    z = bx * bx + 0.5 * (0.5 * (np.roll(c, 1, axis=0) + np.roll(east, 1, axis=0)) + 0.5 * (c + east))
    return 0.5 * h * (0.5 * (z + np.roll(z, -1, axis=0)))
