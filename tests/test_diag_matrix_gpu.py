"""swmhd_diagnostics_f64 / _f32 and swmhd_ensemble_diagnostics_* (k_diag_partial, k_diag_final of swmhd_amd/csrc/diagnostics.hip)
against the longdouble reference of tests/diag_cases.py (pinned on the CPU by tests/test_diag_cases_cpu.py), through the C-ABI: shapes
below, at and above one block, one trip and two trips of the grid-stride loop (256 threads x 1024 blocks = 262 144 cells per trip),
both formulations and precisions, halos (1, 1), (3, 3) and (2, 5), a pitched stride_y, row ranges (sub-range, single rows at both ends,
empty), and one non-finite cell in u, A or h.

Tolerances, derived from the kernel and not from what it achieves:
    energies   |got - want| <= (R + D) 2^-53 sum|term|.  R = 2 x 16: the magnetic energy is the longest per-cell expression with 16
               roundings (counted in diag_cases.R_CELL: 5 per face value B, squared: 11, five more up to 0.5 h (...)), doubled for
               FMA contraction (the file is built -ffp-contract=fast); every addend is a square times a positive h, so relative
               errors of the parts bound that of the term.  D = serial trips of a thread (ceil(cells / 262 144)) + 8 tree levels of
               the 256-thread block + 4 serial partials per thread in the final fold + 8 tree levels + 1 for the scale dx dy:
               22 to 24 here.  The reference is exact to 2^-63 per term and sums exactly, so it has no share.
    extrema    equal bit for bit, clean or not.  |u|, |A| and h are exact; the conservative form's uh / (0.5 (h- + h)) is one
               correctly rounded division of an exactly halved sum, which the reference forms in double.  A NaN cell gives NaN (the
               maximum / minimum of the reference's progress callback propagate it, SWMHD_example.jl:47-65); the payload is not pinned.
    non-finite energies: NaN where the reference has NaN, +Inf where it has +Inf.

Side effects, per case: the inputs are bitwise unchanged; workspace[7 * 1024:] and out[7:] keep their sentinel; the workspace starts
as NaN, so a partial the kernel leaves unwritten makes the (finite) results NaN; a second call gives the same bits.

Achieved error / bound ratios and times: profiles/diag_matrix/README.md."""
import numpy as np
import pytest

import diag_cases as DC

pytestmark = pytest.mark.gpu
CASES = DC.cases()
ENSEMBLE_CASES = DC.ensemble_cases()
SENTINEL = -555.5
TAIL = 64                   # sentinel elements behind the workspace and behind out


def _sfx(dtype):
    return "f64" if np.dtype(dtype) == np.float64 else "f32"


def run_case(S, c, q=None):
    """One call of swmhd_diagnostics for case c on the parents q (default: the case's inputs), twice.  Returns the 7 outputs and a
    list of violated side-effect assertions."""
    import torch
    L = S._lib
    q = DC.inputs(c) if q is None else q
    j0, j1 = DC.rows_of(c)
    tq = [torch.from_numpy(np.array(a)).cuda() for a in q]
    nws = L.DIAG_WORKSPACE
    runs = []
    for _ in range(2):
        ws = torch.full((nws + TAIL,), float("nan"), dtype=torch.float64, device="cuda")
        ws[nws:] = SENTINEL
        out = torch.full((DC.NQ + TAIL,), SENTINEL, dtype=torch.float64, device="cuda")
        rc = getattr(L.lib(), f"swmhd_diagnostics_{_sfx(c.dtype)}")(*[t.data_ptr() for t in tq], c.Nx, c.Ny, c.Hx, c.Hy, DC.stride_y(c),
                                                                      DC.DX, DC.DY, DC.GRAV, DC.HREF, c.form, j0, j1, ws.data_ptr(),
                                                                      out.data_ptr(), None)
        L.check(rc, DC.case_id(c))
        torch.cuda.synchronize()
        runs.append((ws.cpu().numpy(), out.cpu().numpy()))
    fails = []
    for a, t in zip(q, tq):
        if a.tobytes() != t.cpu().numpy().tobytes():
            fails.append("an input was changed")
    (ws, out), (ws2, out2) = runs
    if not (ws[nws:] == SENTINEL).all():
        fails.append("the kernel wrote behind workspace[7 * 1024]")
    if not (out[DC.NQ:] == SENTINEL).all():
        fails.append("the kernel wrote behind out[7]")
    if c.nonfinite is None and np.isnan(ws[:nws]).any():
        fails.append(f"{int(np.isnan(ws[:nws]).sum())} elements of workspace[:7 * 1024] were not written")
    if out[:DC.NQ].tobytes() != out2[:DC.NQ].tobytes() or ws.tobytes() != ws2.tobytes():
        fails.append("two calls differ")
    return out[:DC.NQ].copy(), fails


WORST = {}


@pytest.mark.parametrize("c", CASES, ids=DC.case_id)
def test_diag_matrix(swmhd, c):
    want, sumabs = DC.expected(c)
    got, fails = run_case(swmhd, c)
    cmp_fails, ratio = DC.compare(got, want, sumabs, DC.ncell_of(c))
    WORST[_sfx(c.dtype)] = max(WORST.get(_sfx(c.dtype), 0.0), ratio)
    print(f"{DC.case_id(c)}: energy error / bound {ratio:.3g} (worst so far {WORST}); got {got.tolist()}")
    fails += cmp_fails
    if c.rows is not None and c.rows[0] == c.rows[1]:
        if got.tolist() != list(DC.EMPTY):
            fails.append(f"empty range: got {got.tolist()}")
    elif c.nonfinite is None and not np.isfinite(got).all():
        fails.append(f"non-finite results from finite inputs: {got.tolist()}")
    if c.nonfinite is not None:
        # the outputs the non-finite cell does not reach are bitwise the clean run's
        clean_got, clean_fails = run_case(swmhd, DC.clean(c))
        fails += [f"clean twin: {m}" for m in clean_fails]
        clean_want, _ = DC.expected(DC.clean(c))
        for k in range(DC.NQ):
            if DC.same_bits(want[k], clean_want[k]) and not DC.same_bits(got[k], clean_got[k]):
                fails.append(f"{DC.NAMES[k]} differs from the clean run's, which the reference's does not")
    assert not fails, "\n".join(fails)


def test_row_ranges_add_up(swmhd):
    """Beside the comparison of every range with the reference: on one un-poisoned input the sub-ranges [0, 5), [5, 17), [17, 21)
    give energies that add up to the whole range's within the bound (the three bounds add up to the whole range's: same R and D, and
    the sums of |term| add), and extrema that combine exactly."""
    c = DC.Case(37, 21, 3, 3, False, None, 0, np.float64, None)
    q = [np.ascontiguousarray(a) for a in DC._random_parents(37, 21, 3, 3, 43)]
    whole, fails = run_case(swmhd, c, q)
    parts = []
    for rows in ((0, 5), (5, 17), (17, 21)):
        got, f = run_case(swmhd, c._replace(rows=rows), q)
        parts.append(got)
        fails += f
    assert not fails, fails
    want, sumabs = DC.reference(*q, 37, 21, 3, 3, DC.DX, DC.DY, DC.GRAV, DC.HREF, 0, 0, 21, np.float64)
    for k in range(3):
        assert abs(sum(np.longdouble(p[k]) for p in parts) - want[k]) <= DC.energy_bound(37 * 21, sumabs[k])
    for k in (3, 4, 5):
        assert whole[k] == max(p[k] for p in parts)
    assert whole[6] == min(p[6] for p in parts)


@pytest.mark.parametrize("e", ENSEMBLE_CASES, ids=DC.ensemble_case_id)
def test_ensemble_members_match_the_reference(swmhd, e):
    """swmhd_ensemble_diagnostics_* (and _params with three different g) on 3 members at a pitched stride_m with NaN between the
    members: each member against the reference -- below 262 144 cells this is the launch of nb < 1024 partial blocks whose final fold
    takes the identity element for the missing ones -- and bitwise against swmhd_diagnostics on the member alone.  A non-finite member
    leaves the others bitwise at their clean values."""
    import torch
    Nx, Ny, form, dtype, params, bad = e
    L = swmhd._lib
    M, H, sy = DC.ENSEMBLE_MEMBERS, 3, Nx + 6
    sfx = _sfx(dtype)
    stride_m = (Ny + 2 * H) * sy + DC.ENSEMBLE_GAP
    members = [DC.ensemble_member_inputs(Nx, Ny, dtype, m, bad == m) for m in range(M)]
    g = DC.ENSEMBLE_G if params else (DC.GRAV,) * M

    def call(member_inputs):
        host = [np.full(M * stride_m, np.nan, dtype=dtype) for _ in range(4)]
        for m, q in enumerate(member_inputs):
            for f in range(4):
                host[f][m * stride_m:m * stride_m + (Ny + 2 * H) * sy] = q[f].ravel()
        dev = [torch.from_numpy(a).cuda() for a in host]
        nws = L.ensemble_diag_workspace(M, Nx, Ny)
        ws = torch.full((nws + TAIL,), float("nan"), dtype=torch.float64, device="cuda")
        ws[nws:] = SENTINEL
        out = torch.full((M * DC.NQ + TAIL,), SENTINEL, dtype=torch.float64, device="cuda")
        ptrs = [t.data_ptr() for t in dev]
        if params:
            tab = torch.from_numpy(np.array([[g[m], 1.0, 0.01] for m in range(M)], dtype=dtype)).cuda()
            rc = getattr(L.lib(), f"swmhd_ensemble_diagnostics_params_{sfx}")(*ptrs, M, stride_m, Nx, Ny, H, H, sy, DC.DX, DC.DY, tab.data_ptr(),
                                                                               DC.HREF, form, ws.data_ptr(), out.data_ptr(), None)
        else:
            rc = getattr(L.lib(), f"swmhd_ensemble_diagnostics_{sfx}")(*ptrs, M, stride_m, Nx, Ny, H, H, sy, DC.DX, DC.DY, DC.GRAV, DC.HREF, form,
                                                                        ws.data_ptr(), out.data_ptr(), None)
        L.check(rc, DC.ensemble_case_id(e))
        torch.cuda.synchronize()
        ws, out = ws.cpu().numpy(), out.cpu().numpy()
        assert (ws[nws:] == SENTINEL).all() and (out[M * DC.NQ:] == SENTINEL).all(), "wrote behind the workspace or behind out"
        assert all(a.tobytes() == t.cpu().numpy().tobytes() for a, t in zip(host, dev)), "an input was changed"
        return out[:M * DC.NQ].reshape(M, DC.NQ).copy()

    got = call(members)
    fails = []
    for m in range(M):
        want, sumabs = DC.reference(*members[m], Nx, Ny, H, H, DC.DX, DC.DY, g[m], DC.HREF, form, 0, Ny, dtype)
        f, ratio = DC.compare(got[m], want, sumabs, Nx * Ny)
        print(f"{DC.ensemble_case_id(e)} member {m}: energy error / bound {ratio:.3g}; got {got[m].tolist()}")
        fails += [f"member {m}: {x}" for x in f]
        if bad != m and not np.isfinite(got[m]).all():
            fails.append(f"member {m} is finite but its results are not: {got[m].tolist()}")
        # bitwise the single-grid call on the member alone (include/swmhd.h)
        if not params:
            alone, sf = run_case(swmhd, DC.Case(Nx, Ny, H, H, False, None, form, dtype, None), members[m])
            fails += [f"member {m} alone: {x}" for x in sf if not (bad == m and "not written" in x)]
            if not all(DC.same_bits(a, b) for a, b in zip(alone, got[m])):
                fails.append(f"member {m}: ensemble {got[m].tolist()} != single grid {alone.tolist()}")
    if bad is not None:
        clean = call([DC.ensemble_member_inputs(Nx, Ny, dtype, m, False) for m in range(M)])
        for m in range(M):
            if m != bad and clean[m].tobytes() != got[m].tobytes():
                fails.append(f"member {m} changed with the non-finite member {bad}")
        assert np.isnan(got[bad][[0, 1, 2, 6]]).all(), got[bad]
    assert not fails, "\n".join(fails)
