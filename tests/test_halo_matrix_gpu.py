"""The halo-fill entry points through the C-ABI at edge shapes and arguments, bit for bit against numpy and the CPU oracle:
swmhd_fill_halo_periodic_* (k_halo_x, k_halo_y), swmhd_fill_halo_periodic_multi_* and swmhd_ensemble_fill_halo_periodic_*
(k_halo_multi), swmhd_fill_halo_* and swmhd_fill_halo_walls_* (k_halo_bc) of swmhd_amd/csrc/halo.hip.

Periodic fills: reference helpers.fill_halo_periodic, restated per `which` bit (reference_periodic; for X | Y it is asserted to BE
helpers.fill_halo_periodic).  Shapes (1, 1) with H = 1, (3, 3) with H = 3 (N == H), (3, 40), (40, 3), (37, 21), (300, 5) (more than
one block); halos (3, 3), (2, 5), (5, 2), (3, 9) wherever H <= N (a deeper halo is refused: SWMHD_EHALO); a pitched stride_y; which =
X, Y, X | Y; 1, 3 and 4 fields; both precisions.  Every parent cell starts as a value of its own and the pitch padding as a sentinel;
the whole parent, padding included, must equal the reference; the interior is unchanged; which = X leaves every y-halo row and
which = Y (multi) every x-halo column and corner untouched.
    The single-field and the multi-field call agree bit for bit for which = X and X | Y.  For which = Y alone they are DIFFERENT by
    their own documents and compared outside the corners only: swmhd_fill_halo_periodic copies the y halos "over the full padded
    width" (include/swmhd.h: the corners take what the x-halo columns of the interior rows hold at that time), k_halo_multi leaves the
    corners "to the caller's x fill".  Each is held to its own reference there.
Boundary-condition fills: reference oracle.fill_halo per field (equality is bitwise: halo.hip is built without contraction), all four
topologies, centre and face fields, gradients on some sides and NaN (the default condition) on others, Hx != Hy, shapes (7, 8),
(3, 3), (70, 9), both precisions; swmhd_fill_halo_walls with walls_y = 0 .. 3: a cut side's halo rows and first interior line are
what the x pass left; walls_y = 3 is swmhd_fill_halo with a Bounded y."""
import ctypes

import numpy as np
import pytest

import helpers as Hh

pytestmark = pytest.mark.gpu
SENTINEL = -555.5
PAD = 5
X, Y = 1, 2
DTYPES = [np.float64, np.float32]
P, B = 0, 1


def _sfx(dtype):
    return "f64" if np.dtype(dtype) == np.float64 else "f32"


def distinct_parents(n, Nx, Ny, Hx, Hy, pad, dtype, seed):
    """n parents of shape (Ny + 2 Hy, Nx + 2 Hx + pad): a different value in every cell of every parent (integers + 0.25, exact in
    fp32), the sentinel in the pitch padding."""
    rows, W = Ny + 2 * Hy, Nx + 2 * Hx
    vals = np.random.default_rng(seed).permutation(n * rows * W).reshape(n, rows, W) + 0.25
    assert vals.max() < 2 ** 22
    out = np.full((n, rows, W + pad), SENTINEL, dtype=dtype)
    out[:, :, :W] = vals
    return [np.ascontiguousarray(a) for a in out]


def reference_periodic(a, Nx, Ny, Hx, Hy, which, multi):
    """The periodic fill of one parent for the bits of `which`.  X: the x halos of the interior rows.  Y: the y halos from the
    interior rows -- over the full padded width for the single-field call (after X, if set), over the interior columns for the
    multi-field call, which with X | Y fills the corners from the interior cell (x mod Nx, y mod Ny): the same values."""
    a = a.copy()
    W = Nx + 2 * Hx
    I = slice(Hy, Hy + Ny)
    if which & X:
        a[I, :Hx] = a[I, Nx:Nx + Hx]
        a[I, Nx + Hx:W] = a[I, Hx:2 * Hx]
    if which & Y:
        cols = slice(0, W) if (not multi or which & X) else slice(Hx, Hx + Nx)
        a[:Hy, cols] = a[Ny:Ny + Hy, cols]
        a[Ny + Hy:, cols] = a[Hy:2 * Hy, cols]
    return a


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


PERIODIC_CASES = [
    # Nx, Ny, Hx, Hy, pitched
    (1, 1, 1, 1, False), (1, 1, 1, 1, True),
    (3, 3, 3, 3, False), (3, 3, 3, 3, True), (3, 3, 2, 3, False),
    (3, 40, 3, 3, False), (3, 40, 2, 5, True), (3, 40, 3, 9, False),
    (40, 3, 3, 3, True), (40, 3, 5, 2, False),
    (37, 21, 3, 3, False), (37, 21, 2, 5, True), (37, 21, 5, 2, False), (37, 21, 3, 9, True),
    (300, 5, 3, 3, True), (300, 5, 2, 5, False), (300, 5, 5, 2, True),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=_sfx)
@pytest.mark.parametrize("Nx,Ny,Hx,Hy,pitch", PERIODIC_CASES, ids=[f"{c[0]}x{c[1]}-H{c[2]}_{c[3]}{'-pitch' if c[4] else ''}" for c in PERIODIC_CASES])
def test_periodic_fills_match_numpy(swmhd, Nx, Ny, Hx, Hy, pitch, dtype):
    import torch
    L = swmhd._lib
    sfx = _sfx(dtype)
    pad = PAD if pitch else 0
    sy = Nx + 2 * Hx + pad
    W = Nx + 2 * Hx
    base = distinct_parents(4, Nx, Ny, Hx, Hy, pad, dtype, [Nx, Ny, Hx, Hy])
    assert same(reference_periodic(base[0][:, :W], Nx, Ny, Hx, Hy, X | Y, False), Hh.fill_halo_periodic(base[0][:, :W], Nx, Ny, Hx, Hy))
    assert same(reference_periodic(base[0][:, :W], Nx, Ny, Hx, Hy, X | Y, True), Hh.fill_halo_periodic(base[0][:, :W], Nx, Ny, Hx, Hy))
    corners = np.zeros(base[0].shape, dtype=bool)
    for r in (slice(0, Hy), slice(Hy + Ny, None)):
        corners[r, :Hx] = True
        corners[r, Nx + Hx:W] = True
    for which in (X, Y, X | Y):
        for nf in (1, 3, 4):
            dev = [torch.from_numpy(a.copy()).cuda() for a in base[:nf]]
            L.check(getattr(L.lib(), f"swmhd_fill_halo_periodic_multi_{sfx}")(L.ptr_array([t.data_ptr() for t in dev]), nf, Nx, Ny, Hx, Hy, sy,
                                                                               which, None), "multi")
            one = torch.from_numpy(base[0].copy()).cuda()
            L.check(getattr(L.lib(), f"swmhd_fill_halo_periodic_{sfx}")(one.data_ptr(), Nx, Ny, Hx, Hy, sy, which, None), "single")
            torch.cuda.synchronize()
            multi = [t.cpu().numpy() for t in dev]
            single = one.cpu().numpy()
            tag = (which, nf)
            for f in range(nf):
                assert same(multi[f], reference_periodic(base[f], Nx, Ny, Hx, Hy, which, True)), ("multi", tag, f)
                assert same(multi[f][Hy:Hy + Ny, Hx:Hx + Nx], base[f][Hy:Hy + Ny, Hx:Hx + Nx]), ("interior", tag, f)
                assert (multi[f][:, W:] == SENTINEL).all(), ("padding", tag, f)
                if which == Y:      # corners and x halos untouched
                    assert same(multi[f][:, :Hx], base[f][:, :Hx]) and same(multi[f][:, Nx + Hx:], base[f][:, Nx + Hx:]), ("x halos", tag, f)
                if which == X:      # y-halo rows untouched
                    assert same(multi[f][:Hy], base[f][:Hy]) and same(multi[f][Hy + Ny:], base[f][Hy + Ny:]), ("y halos", tag, f)
            assert same(single, reference_periodic(base[0], Nx, Ny, Hx, Hy, which, False)), ("single", tag)
            if which == X:
                assert same(single[:Hy], base[0][:Hy]) and same(single[Hy + Ny:], base[0][Hy + Ny:]), ("y halos, single", tag)
            if which == Y:          # (module docstring) the two calls differ in the corners by their documents
                assert same(np.where(corners, 0, single).astype(dtype), np.where(corners, 0, multi[0]).astype(dtype)), ("single vs multi", tag)
            else:
                assert same(single, multi[0]), ("single vs multi", tag)


def test_periodic_fills_refuse_a_halo_deeper_than_the_grid(swmhd):
    import torch
    L = swmhd._lib
    t = torch.zeros((40 + 18) * (3 + 10), dtype=torch.float64, device="cuda")
    assert L.lib().swmhd_fill_halo_periodic_f64(t.data_ptr(), 3, 40, 5, 9, 13, 3, None) == 2          # SWMHD_EHALO: Hx > Nx
    assert L.lib().swmhd_fill_halo_periodic_multi_f64(L.ptr_array([t.data_ptr()]), 1, 3, 40, 5, 9, 13, 3, None) == 2
    assert L.lib().swmhd_fill_halo_periodic_f64(t.data_ptr(), 3, 40, 3, 9, 8, 3, None) == 1           # stride_y < Nx + 2 Hx
    torch.cuda.synchronize()
    assert (t == 0).all()


ENSEMBLE_CASES = [(3, 3, 3, 3, False), (40, 3, 5, 2, True), (37, 21, 3, 3, False), (37, 21, 3, 9, True), (300, 5, 2, 5, False), (1, 1, 1, 1, True)]


@pytest.mark.parametrize("dtype", DTYPES, ids=_sfx)
@pytest.mark.parametrize("Nx,Ny,Hx,Hy,pitch", ENSEMBLE_CASES, ids=[f"{c[0]}x{c[1]}-H{c[2]}_{c[3]}{'-pitch' if c[4] else ''}" for c in ENSEMBLE_CASES])
def test_ensemble_periodic_fill(swmhd, Nx, Ny, Hx, Hy, pitch, dtype):
    """3 members at a pitched stride_m: the gaps between members keep their sentinel, every member equals the reference and the
    single-grid multi-field call on it."""
    import torch
    L = swmhd._lib
    sfx = _sfx(dtype)
    M, gap = 3, 13
    pad = PAD if pitch else 0
    sy = Nx + 2 * Hx + pad
    n = (Ny + 2 * Hy) * sy
    stride_m = n + gap
    for which in (X, Y, X | Y):
        for nf in (1, 4):
            base = distinct_parents(M * nf, Nx, Ny, Hx, Hy, pad, dtype, [Nx, Ny, Hx, Hy, which, nf])
            host = [np.full(M * stride_m, SENTINEL, dtype=dtype) for _ in range(nf)]
            for m in range(M):
                for f in range(nf):
                    host[f][m * stride_m:m * stride_m + n] = base[m * nf + f].ravel()
            dev = [torch.from_numpy(a.copy()).cuda() for a in host]
            L.check(getattr(L.lib(), f"swmhd_ensemble_fill_halo_periodic_{sfx}")(L.ptr_array([t.data_ptr() for t in dev]), nf, M, stride_m, Nx, Ny,
                                                                                  Hx, Hy, sy, which, None), "ensemble")
            torch.cuda.synchronize()
            got = [t.cpu().numpy() for t in dev]
            for m in range(M):
                alone = [torch.from_numpy(base[m * nf + f].copy()).cuda() for f in range(nf)]
                L.check(getattr(L.lib(), f"swmhd_fill_halo_periodic_multi_{sfx}")(L.ptr_array([t.data_ptr() for t in alone]), nf, Nx, Ny, Hx, Hy,
                                                                                   sy, which, None), "multi")
                torch.cuda.synchronize()
                for f in range(nf):
                    member = got[f][m * stride_m:m * stride_m + n].reshape(Ny + 2 * Hy, sy)
                    assert same(member, reference_periodic(base[m * nf + f], Nx, Ny, Hx, Hy, which, True)), (which, nf, m, f)
                    assert same(member, alone[f].cpu().numpy()), (which, nf, m, f)
                    assert (got[f][m * stride_m + n:(m + 1) * stride_m] == SENTINEL).all(), ("gap", which, nf, m, f)


# ---- boundary conditions -------------------------------------------------------------------------------------------------------
FACE_X, FACE_Y = 1, 2                  # bit f: field f is at Face in x / y -- (u, v, h, A): u is bit 0 of face_x, v bit 1 of face_y
LOC = [(True, False), (False, True), (False, False), (False, False)]
NAN = float("nan")
# (west, east, south, north) per field: gradients on some sides, the default condition on the others; sides a face field has its
# wall on ignore the value
GRADS = [(NAN, NAN, 0.3, NAN), (NAN, -0.7, NAN, NAN), (0.25, NAN, NAN, -0.2), (NAN, 0.07, 0.125, -0.05)]
DXY = (0.1, 0.12)
BC_SHAPES = [(7, 8, 3, 3), (7, 8, 2, 3), (3, 3, 3, 3), (3, 3, 1, 2), (70, 9, 3, 3), (70, 9, 3, 2)]
TOPOS = [(P, P), (P, B), (B, P), (B, B)]


def bc_reference(oracle, base, Nx, Ny, Hx, Hy, topo, dtype):
    """oracle.fill_halo of each of the four fields (u, v, h, A) with GRADS."""
    dx, dy = DXY
    return [oracle.fill_halo(base[f].copy(), Nx, Ny, Hx, Hy, topo=topo, face=LOC[f], grad=[None if g != g else g for g in GRADS[f]],
                             dx=dx, dy=dy) for f in range(4)]


def grad_table(dtype):
    ct = ctypes.c_double if np.dtype(dtype) == np.float64 else ctypes.c_float
    return (ct * 16)(*[g for f in GRADS for g in f])


@pytest.mark.parametrize("dtype", DTYPES, ids=_sfx)
@pytest.mark.parametrize("topo", TOPOS, ids=["PP", "PB", "BP", "BB"])
@pytest.mark.parametrize("Nx,Ny,Hx,Hy", BC_SHAPES, ids=[f"{c[0]}x{c[1]}-H{c[2]}_{c[3]}" for c in BC_SHAPES])
def test_fill_halo_matches_the_oracle_at_edge_shapes(swmhd, oracle, Nx, Ny, Hx, Hy, topo, dtype):
    import torch
    L = swmhd._lib
    sfx = _sfx(dtype)
    sy = Nx + 2 * Hx
    base = distinct_parents(4, Nx, Ny, Hx, Hy, 0, dtype, [Nx, Ny, Hx, Hy, 7])
    want = bc_reference(oracle, base, Nx, Ny, Hx, Hy, topo, dtype)
    for nf in (4, 1, 3):
        dev = [torch.from_numpy(a.copy()).cuda() for a in base[:nf]]
        L.check(getattr(L.lib(), f"swmhd_fill_halo_{sfx}")(L.ptr_array([t.data_ptr() for t in dev]), nf, Nx, Ny, Hx, Hy, sy, topo[0], topo[1],
                                                            FACE_X, FACE_Y, grad_table(dtype), DXY[0], DXY[1], None), "fill_halo")
        torch.cuda.synchronize()
        for f in range(nf):
            got = dev[f].cpu().numpy()
            assert same(got, want[f]), (nf, f, np.argwhere(got != want[f])[:5])
    # no gradient table: the default condition everywhere
    dev = [torch.from_numpy(a.copy()).cuda() for a in base]
    L.check(getattr(L.lib(), f"swmhd_fill_halo_{sfx}")(L.ptr_array([t.data_ptr() for t in dev]), 4, Nx, Ny, Hx, Hy, sy, topo[0], topo[1],
                                                        FACE_X, FACE_Y, None, DXY[0], DXY[1], None), "fill_halo")
    torch.cuda.synchronize()
    for f in range(4):
        w = oracle.fill_halo(base[f].copy(), Nx, Ny, Hx, Hy, topo=topo, face=LOC[f], dx=DXY[0], dy=DXY[1])
        assert same(dev[f].cpu().numpy(), w), ("defaults", f)


@pytest.mark.parametrize("dtype", DTYPES, ids=_sfx)
@pytest.mark.parametrize("tx", [P, B], ids=["Px", "Bx"])
@pytest.mark.parametrize("Nx,Ny,Hx,Hy", BC_SHAPES, ids=[f"{c[0]}x{c[1]}-H{c[2]}_{c[3]}" for c in BC_SHAPES])
def test_fill_halo_walls_matches_the_oracle(swmhd, oracle, Nx, Ny, Hx, Hy, tx, dtype):
    """walls_y = 3 is swmhd_fill_halo with a Bounded y (= the oracle's).  A cut side is left to the neighbour: its halo rows, and the
    first interior line where a wall of a face field would sit, hold what the x pass left -- the parent's halo rows as they were, the
    interior rows with their x halos filled (= the interior rows of the oracle's fill with a Periodic y, whose y pass writes halo rows
    only)."""
    import torch
    L = swmhd._lib
    sfx = _sfx(dtype)
    sy = Nx + 2 * Hx
    base = distinct_parents(4, Nx, Ny, Hx, Hy, 0, dtype, [Nx, Ny, Hx, Hy, 9])
    full = bc_reference(oracle, base, Nx, Ny, Hx, Hy, (tx, B), dtype)
    xonly = [b.copy() for b in base]
    for f, w in enumerate(bc_reference(oracle, base, Nx, Ny, Hx, Hy, (tx, P), dtype)):
        xonly[f][Hy:Hy + Ny] = w[Hy:Hy + Ny]
    for walls in (0, 1, 2, 3):
        dev = [torch.from_numpy(a.copy()).cuda() for a in base]
        L.check(getattr(L.lib(), f"swmhd_fill_halo_walls_{sfx}")(L.ptr_array([t.data_ptr() for t in dev]), 4, Nx, Ny, Hx, Hy, sy, tx, walls,
                                                                  FACE_X, FACE_Y, grad_table(dtype), DXY[0], DXY[1], None), "walls")
        torch.cuda.synchronize()
        for f in range(4):
            want = xonly[f].copy()
            if walls & 1:
                want[:Hy + 1] = full[f][:Hy + 1]        # the south halo and the wall line (a face field's; a centre field's is the x pass's)
            if walls & 2:
                want[Hy + Ny:] = full[f][Hy + Ny:]      # the north wall sits on the first halo line
            got = dev[f].cpu().numpy()
            assert same(got, want), (walls, f, np.argwhere(got != want)[:5])
            if walls == 3:
                assert same(got, full[f])
            if not walls & 1:
                # (the x pass owns the first interior line's x halos and, with a Bounded x, the west wall of u on it)
                assert same(got[:Hy], base[f][:Hy]) and same(got[Hy], xonly[f][Hy]), ("south cut", walls, f)
                assert same(got[Hy, Hx + 1:Hx + Nx], base[f][Hy, Hx + 1:Hx + Nx]), ("south cut, first interior line", walls, f)
            if not walls & 2:
                assert same(got[Hy + Ny:], base[f][Hy + Ny:]), ("north cut", walls, f)
