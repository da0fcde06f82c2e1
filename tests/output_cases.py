"""numpy restatement of the output frames (swmhd_output_fields_* in include/swmhd.h), the yardstick of tests/test_output_*.py.

The reference's writer stores (u, v, A, s), s = sqrt(u^2 + v^2) (SWMHD_example.jl:67-68,80-84; divergence_sw_mhd.jl:64-66,75-82 with
u = uh / h, v = vh / h), and MHD_visualize.jl:55-65 looks at B_x = -dA/dy / h, B_y = dA/dx / h.  Placement as in
plot_cases.np_diagnostics: a binary operation sits where its first operand is, the second is interpolated there, a divisor field is
interpolated.  Everything in IEEE double, in the operation order the kernel documents, so the device frames can be compared bitwise."""
import numpy as np

NAMES = ("u", "v", "h", "A", "s", "B_x", "B_y")


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
