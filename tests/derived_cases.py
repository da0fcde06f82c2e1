"""numpy restatement of the derived frames (swmhd_derived_fields_* in include/swmhd_derived.h), the yardstick of tests/test_derived_*.py,
and the shapes the GPU tests run.

C-grid, indices as in output_cases: U, V are the frame velocities (q1, q2 vector-invariant; q1 / ℑxᶠh, q2 / ℑyᶠh conservative), and
    vorticity            @(f,f)  (V(i,j) − V(i−1,j)) / Δx − (U(i,j) − U(i,j−1)) / Δy
    divergence           @(c,c)  (U(i+1,j) − U(i,j)) / Δx + (V(i,j+1) − V(i,j)) / Δy
    current              @(c,c)  ((A(i+1,j) − A(i,j))/Δx − (A(i,j) − A(i−1,j))/Δx) / Δx + ((A(i,j+1) − A(i,j))/Δy − (A(i,j) − A(i,j−1))/Δy) / Δy
    potential_vorticity  @(f,f)  (ζ(i,j) + f) / (0.5*(0.5*(h(i−1,j−1) + h(i,j−1)) + 0.5*(h(i−1,j) + h(i,j))))
Everything in IEEE double, in the operation order written, so the device frames can be compared bitwise.  Neighbours are read from the
halos as given; for the kernel's SWMHD_WRAP_* flags hand in output_cases.wrap_parents(...)."""
import numpy as np

from output_cases import wrap_parents  # noqa: F401  (re-exported: the periodic images the WRAP flags read)

NAMES = ("vorticity", "divergence", "current", "potential_vorticity")
BITS = {n: 1 << k for k, n in enumerate(NAMES)}
ALL = 15

# (Nx, Ny) of the GPU tests: one cell (both x-neighbours are the same cell under wrap); less than a chunk; one chunk exactly; a chunk
# across the row end; odd sizes; a row of exactly 16 chunks; one cell past it; a row that crosses a 256-thread workgroup
SHAPES = ((1, 1), (2, 3), (4, 1), (5, 2), (7, 9), (64, 2), (65, 3), (1025, 2))
HALOS = ((1, 1), (3, 2))
MASKS = (1, 2, 4, 8, ALL, 1 | 4)
ROW_RANGES = lambda Ny: ((0, Ny), (1, Ny), (0, 1))


def mask_names(which):
    return tuple(n for n in NAMES if which & BITS[n])


def np_derived_fields(q1, q2, h, A, Nx, Ny, Hx, Hy, dx, dy, f, form, names=NAMES, rows=None):
    """(len(names), rows, Nx) float64: the named fields at indices 1..Nx x rows [j0, j1) from halo-padded parents (halos as given).
    form 1 = vector-invariant (q = u, v), 0 = conservative (q = uh, vh)."""
    j0, j1 = (0, Ny) if rows is None else rows
    q1, q2, h, A = (np.asarray(a, dtype=np.float64) for a in (q1, q2, h, A))
    dx, dy, f = np.float64(dx), np.float64(dy), np.float64(f)
    S = lambda a, di, dj: a[Hy + j0 + dj:Hy + j1 + dj, Hx + di:Hx + di + Nx]
    U = lambda di, dj: S(q1, di, dj) if form == 1 else S(q1, di, dj) / (0.5 * (S(h, di - 1, dj) + S(h, di, dj)))
    V = lambda di, dj: S(q2, di, dj) if form == 1 else S(q2, di, dj) / (0.5 * (S(h, di, dj - 1) + S(h, di, dj)))
    zeta = lambda: (V(0, 0) - V(-1, 0)) / dx - (U(0, 0) - U(0, -1)) / dy

    def field(n):
        if n == "vorticity":
            return zeta()
        if n == "divergence":
            return (U(1, 0) - U(0, 0)) / dx + (V(0, 1) - V(0, 0)) / dy
        if n == "current":
            a = S(A, 0, 0)
            return ((S(A, 1, 0) - a) / dx - (a - S(A, -1, 0)) / dx) / dx + ((S(A, 0, 1) - a) / dy - (a - S(A, 0, -1)) / dy) / dy
        if n == "potential_vorticity":
            return (zeta() + f) / (0.5 * (0.5 * (S(h, -1, -1) + S(h, 0, -1)) + 0.5 * (S(h, -1, 0) + S(h, 0, 0))))
        raise KeyError(n)
    with np.errstate(all="ignore"):
        return np.stack([np.array(field(n), dtype=np.float64) for n in names])
