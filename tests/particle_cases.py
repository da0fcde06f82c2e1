"""The numpy restatement of the particle kernels (swmhd_amd/csrc/particles.hip, include/swmhd_particles.h) and the case list of their
tests: one RK3 stage of the positions, the fold, and the sampler.  float64 throughout, one operation per line in the kernel's order,
the field values cast as the kernel casts them (read in the element type, widened to double).  Vectorised over the particles; a
particle with a non-finite coordinate is left exactly as it is."""
import numpy as np

WRAP, PERIODIC, BOUNDED = 0, 1, 2          # how a direction is indexed and folded (common.hpp PARTICLE_*)
WRAP_X, WRAP_Y, BOUNDED_X, BOUNDED_Y = 16, 32, 256, 512
CONSERVATIVE, VECTOR_INVARIANT = 0, 1
CENTER_X, CENTER_Y = 1, 2
RK3_GAMMA = (8.0 / 15.0, 5.0 / 12.0, 3.0 / 4.0)
RK3_ZETA = (0.0, -17.0 / 60.0, -5.0 / 12.0)
BLOCK = 256

# --- the case list of the GPU matrix ---------------------------------------------------------------------------------------------
GRIDS = ((1, 1), (3, 2), (5, 7), (64, 4), (67, 33))
COUNTS = (0, 1, 63, 64, 65, 257, 1000)
WRAPS = (WRAP_X | WRAP_Y, WRAP_X, WRAP_Y, 0)
HALOS = (1, 3)


def modes(flags):
    """(mode_x, mode_y) of a call's flags"""
    mx = WRAP if flags & WRAP_X else (BOUNDED if flags & BOUNDED_X else PERIODIC)
    my = WRAP if flags & WRAP_Y else (BOUNDED if flags & BOUNDED_Y else PERIODIC)
    return mx, my


def axis(p, o, d, center, N, H, mode):
    """(i0, i1, iw, t) of particle_axis: the two nodes around the coordinates p, the index before i0, the weight of i1.  Indices are
    brought into range in floating point, before the conversion."""
    with np.errstate(all="ignore"):
        s = p - o
        s = s / d
        if center:
            s = s - 0.5
        fl = np.floor(s)
        t = s - fl
        if mode == WRAP:
            m = np.fmod(fl, float(N))
            m = np.where(m < 0.0, m + float(N), m)
            m = np.where(m >= 0.0, m, 0.0)
            i0 = m.astype(np.int64)
            i1 = np.where(i0 + 1 == N, 0, i0 + 1)
            iw = np.where(i0 == 0, N - 1, i0 - 1)
        else:
            c = np.minimum(np.maximum(fl, float(-H)), float(N + H - 2))
            i0 = c.astype(np.int64)
            i1 = i0 + 1
            iw = np.maximum(i0 - 1, -H)
    return i0, i1, iw, t


def bilinear(tx, ty, f00, f10, f01, f11):
    ox = 1.0 - tx
    oy = 1.0 - ty
    a = ox * f00
    b = tx * f10
    lo = a + b
    a = ox * f01
    b = tx * f11
    hi = a + b
    a = oy * lo
    b = ty * hi
    return a + b


def fold(x, o, L, mode):
    """particle_fold: into [o, o + L] -- the periodic image, or one reflection at the wall crossed; then the clamp (NaN stays NaN)"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        hi = o + L
        if mode == BOUNDED:
            lo_side = 2.0 * o
            lo_side = lo_side - x
            hi_side = 2.0 * hi
            hi_side = hi_side - x
            x = np.where(x < o, lo_side, np.where(x > hi, hi_side, x))
        else:
            r = x - o
            r = r / L
            r = np.floor(r)
            r = L * r
            x = x - r
        return np.where(x < o, o, np.where(x > hi, hi, x))


def reflect(x, wall):
    """the mirror image of x at `wall` (the operation of the Bounded fold)"""
    t = 2.0 * wall
    return t - x


def _at(f, H, j, i):
    """parent f (float64 copy of the element type) at interior indices (j, i)"""
    return f[j + H[1], i + H[0]]


def node_velocities(q1, q2, h, cons, ux, uy, vx, vy, H):
    """The four node values of U (at ux, uy) and of V (at vx, vy), widened; conservative: q / (0.5 (h before the face + h at it))"""
    U = [_at(q1, H, uy[a], ux[b]) for a, b in ((0, 0), (0, 1), (1, 0), (1, 1))]      # 00, 10, 01, 11: (row, column) = (y, x)
    V = [_at(q2, H, vy[a], vx[b]) for a, b in ((0, 0), (0, 1), (1, 0), (1, 1))]
    if cons:
        with np.errstate(all="ignore"):
            # U node (column c, row r): h at the column before it and at it, same row; i1's column before is i0
            cols = {0: (ux[2], ux[0]), 1: (ux[0], ux[1])}
            for n, (a, b) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
                hw = _at(h, H, uy[a], cols[b][0])
                hc = _at(h, H, uy[a], cols[b][1])
                den = hw + hc
                den = 0.5 * den
                U[n] = U[n] / den
            rows = {0: (vy[2], vy[0]), 1: (vy[0], vy[1])}
            for n, (a, b) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
                hs = _at(h, H, rows[a][0], vx[b])
                hc = _at(h, H, rows[a][1], vx[b])
                den = hs + hc
                den = 0.5 * den
                V[n] = V[n] / den
    return U, V


def stage(q1, q2, h, x, y, gx, gy, Nx, Ny, Hx, Hy, x0, y0, dx, dy, form, dt, gamma, zeta, flags):
    """One RK3 stage of the positions: returns new (x, y, gx, gy).  q1, q2, h: parents in their element type (h may be None for the
    vector-invariant form).  Non-finite particles keep x, y, gx, gy bit for bit."""
    x, y, gx, gy = (np.array(a, dtype=np.float64) for a in (x, y, gx, gy))
    live = np.isfinite(x) & np.isfinite(y)
    xs, ys = np.where(live, x, x0), np.where(live, y, y0)          # (no address is formed from a dead particle: any value serves)
    mx, my = modes(flags)
    cons = form == CONSERVATIVE
    q1, q2 = q1.astype(np.float64), q2.astype(np.float64)
    h = h.astype(np.float64) if h is not None else None
    ux = axis(xs, x0, dx, False, Nx, Hx, mx)
    uy = axis(ys, y0, dy, True, Ny, Hy, my)
    vx = axis(xs, x0, dx, True, Nx, Hx, mx)
    vy = axis(ys, y0, dy, False, Ny, Hy, my)
    U, V = node_velocities(q1, q2, h, cons, ux, uy, vx, vy, (Hx, Hy))
    with np.errstate(all="ignore"):
        Gx = bilinear(ux[3], uy[3], *U)
        Gy = bilinear(vx[3], vy[3], *V)
        rx = gamma * Gx
        ry = gamma * Gy
        if zeta != 0.0:
            t = zeta * gx
            rx = rx + t
            t = zeta * gy
            ry = ry + t
        t = dt * rx
        xn = xs + t
        t = dt * ry
        yn = ys + t
        Lx = float(Nx) * dx
        Ly = float(Ny) * dy
        xn = fold(xn, x0, Lx, mx)
        yn = fold(yn, y0, Ly, my)
    return np.where(live, xn, x), np.where(live, yn, y), np.where(live, Gx, gx), np.where(live, Gy, gy)


def sample(fields, locs, x, y, Nx, Ny, Hx, Hy, x0, y0, dx, dy, flags):
    """The sampler: (nfields, P) float64, NaN for a particle with a non-finite coordinate"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    live = np.isfinite(x) & np.isfinite(y)
    xs, ys = np.where(live, x, x0), np.where(live, y, y0)
    mx, my = modes(flags)
    out = np.empty((len(fields), x.shape[0]))
    for k, (f, loc) in enumerate(zip(fields, locs)):
        f = f.astype(np.float64)
        fx = axis(xs, x0, dx, bool(loc & CENTER_X), Nx, Hx, mx)
        fy = axis(ys, y0, dy, bool(loc & CENTER_Y), Ny, Hy, my)
        v = [_at(f, (Hx, Hy), fy[a], fx[b]) for a, b in ((0, 0), (0, 1), (1, 0), (1, 1))]
        with np.errstate(all="ignore"):
            out[k] = np.where(live, bilinear(fx[3], fy[3], *v), np.nan)
    return out


# --- inputs ------------------------------------------------------------------------------------------------------------------------
def fill_halo(a, Nx, Ny, Hx, Hy):
    """periodic halo fill of a parent (x first, then y over the padded width), in place"""
    for k in range(Hx):
        a[:, Hx - 1 - k] = a[:, Hx + (Nx - 1 - k) % Nx]
        a[:, Hx + Nx + k] = a[:, Hx + k % Nx]
    for k in range(Hy):
        a[Hy - 1 - k, :] = a[Hy + (Ny - 1 - k) % Ny, :]
        a[Hy + Ny + k, :] = a[Hy + k % Ny, :]
    return a


def parents(Nx, Ny, Hx, Hy, pitch, dtype, seed, flags, n=3):
    """n random pitched parents (rows of Nx + 2 Hx + pitch elements; the returned arrays are views of width Nx + 2 Hx; the third is a
    positive thickness) with filled halos, and NaN in every halo cell of a wrapped direction -- which the call must not read -- and in
    the pitch gap."""
    rng = np.random.default_rng(seed)
    W = Nx + 2 * Hx
    out = []
    for k in range(n):
        full = np.full((Ny + 2 * Hy, W + pitch), np.nan)
        a = full[:, :W]
        a[Hy:Hy + Ny, Hx:Hx + Nx] = (1.0 + 0.3 * rng.random((Ny, Nx))) if k == 2 else rng.standard_normal((Ny, Nx))
        fill_halo(a, Nx, Ny, Hx, Hy)
        if flags & WRAP_X:
            a[:, :Hx] = np.nan
            a[:, Hx + Nx:] = np.nan
        if flags & WRAP_Y:
            a[:Hy, :] = np.nan
            a[Hy + Ny:, :] = np.nan
        out.append(full.astype(dtype))
    return out


def positions(P, Nx, Ny, x0, y0, dx, dy, seed, bounded=(False, False)):
    """P positions: the ones that must be present first (as many as fit P, in this order) -- non-finite ones, on x0, on x0 + Lx, on a
    node, in the half cell below the first centre, +-1e300 -- then random ones inside the domain and, in a direction that is not
    Bounded, up to two periods outside it."""
    rng = np.random.default_rng(seed)
    Lx, Ly = Nx * dx, Ny * dy
    nan, inf = float("nan"), float("inf")
    xs = [nan, x0, x0 + Lx, x0 + dx * min(1, Nx - 1), x0 + 0.25 * dx, 1e300, -1e300, inf, x0 + 0.3 * Lx, -inf, x0 + 0.5 * dx, x0 + Lx - 0.25 * dx]
    ys = [y0 + 0.5 * Ly, y0 + Ly, y0, y0 + 0.5 * dy, y0 + 0.25 * dy, y0 + 0.1 * Ly, -1e300, y0, nan, y0 + 0.2 * Ly, y0 + dy * min(1, Ny - 1), 1e300]
    if bounded[0]:      # (a Bounded direction: far-away values are legal for the call but of no interest; keep the special ones inside)
        xs = [v if not np.isfinite(v) or x0 <= v <= x0 + Lx else x0 + 0.7 * Lx for v in xs]
    if bounded[1]:
        ys = [v if not np.isfinite(v) or y0 <= v <= y0 + Ly else y0 + 0.7 * Ly for v in ys]
    x = x0 + Lx * (rng.random(P) if bounded[0] else rng.uniform(-2.0, 3.0, P))
    y = y0 + Ly * (rng.random(P) if bounded[1] else rng.uniform(-2.0, 3.0, P))
    inside = rng.random(P) < 0.6
    x = np.where(inside, x0 + Lx * rng.random(P), x)
    y = np.where(inside, y0 + Ly * rng.random(P), y)
    n = min(P, len(xs))
    x[:n], y[:n] = xs[:n], ys[:n]
    return x, y
