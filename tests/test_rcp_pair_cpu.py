"""The arithmetic of the fp64 marching kernel's shared reciprocals and five-instruction velocity indicator (sw_device.inc MARCH64:
weno_combine_parts / weno_combine_finish / weno_combine_finish_pair, weno_betas4_vel), restated in numpy and checked without a GPU:

  * the pair finish (r12 = 1/(S1 S2), 1/S1 = S2 r12, 1/S2 = S1 r12) equals the two single finishes to rounding;
  * the five-instruction indicator 13/3 (e_u^2 + e_v^2) + (g_u^2 + g_v^2 + eps) equals the six-instruction one;
  * over indicators b from 4 eps up to the documented upper bound of the pair form, b <= 1e25 (sw_device.inc, include/swmhd.h), the
    product S1 S2 is finite and its reciprocal a normal number -- it stays finite up to b = 3.5e25 and overflows just beyond b = 4.0e25, so the bound is a real one;
  * the two extra field sets of tests/test_rcp_pair_gpu.py (all fields scaled by 1e8; perturbations of 1e-8 on a constant state) give
    the oracle a finite, well-conditioned problem: inputs perturbed by one part in 1e16 move its tendencies by a small fraction of
    the bound the GPU test allows.

float64 arithmetic here has no fma, so "to rounding" means a few eps of the quantity's own scale, stated at each check; the reference is
the same expression in longdouble."""
import numpy as np
import pytest

import helpers as Hh
import stage_cases as SC
import test_rcp_pair_gpu as RP

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
SW_EPS = 1e-6
B_MIN, B_MAX, B_SAFE, B_OVERFLOW = 4 * SW_EPS, 1e25, 3.5e25, 4.0e25      # the domain of the pair form as documented


def diffs(q):
    """WenoDiffs of five upwind-ordered values (last axis)."""
    d = [q[..., k + 1] - q[..., k] for k in range(4)]
    e = [d[k + 1] - d[k] for k in range(3)]
    return d, e


def g_terms(d, pos):
    kA, kB = (3.0, 1.0) if pos else (1.0, 3.0)
    return kB * d[3] - kA * d[2], d[1] + d[2], kA * d[1] - kB * d[0]


def betas4(q, eps4, pos, start=None):
    """weno_betas4 (start None) / the accumulating form the parent used for the second stencil (start = the first one's b_k)."""
    d, e = diffs(q)
    g = g_terms(d, pos)
    k = q.dtype.type(13.0) / q.dtype.type(3.0)
    base = [eps4] * 3 if start is None else start
    return [(k * e[2 - i]) * e[2 - i] + (g[i] * g[i] + base[i]) for i in range(3)]


def betas4_vel(qu, qv, eps4, pos):
    """weno_betas4_vel: the 13/3 factor once."""
    du, eu = diffs(qu)
    dv, ev = diffs(qv)
    gu, gv = g_terms(du, pos), g_terms(dv, pos)
    k = qu.dtype.type(13.0) / qu.dtype.type(3.0)
    return [k * (eu[2 - i] * eu[2 - i] + ev[2 - i] * ev[2 - i]) + (gu[i] * gu[i] + (gv[i] * gv[i] + eps4)) for i in range(3)]


def parts(q, b):
    """weno_combine_parts: (S, num, dd, c)."""
    T = q.dtype.type
    d, e = diffs(q)
    f1, f2 = e[1] - e[0], e[2] - e[1]
    tau = b[2] - b[0]
    t2 = tau * tau
    s = [x * x for x in b]
    q0, q1, q2 = s[1] * s[2], s[0] * s[2], s[0] * s[1]
    P = s[0] * q0
    m0, m1, m2 = t2 * q0 + P, t2 * q1 + P, t2 * q2 + P
    S = m2 / T(3) + (T(2) * m1 + m0)
    num = m0 * f2 + (T(2) / T(3)) * (m2 * f1)
    return S, num, T(2) * d[2] + d[1], q[..., 2]


def finish(p, r):
    S, num, dd, c = p
    return c + (dd - num * r) / c.dtype.type(6)


def stencils(rng, n, scale):
    """n upwind-ordered five-value stencils: a smooth part and a rough part of the given scale, a jump in some of them."""
    x = np.arange(5.0)
    q = scale * (rng.standard_normal((n, 1)) + 0.3 * rng.standard_normal((n, 1)) * x + 0.2 * rng.standard_normal((n, 5)))
    q[::3, 3:] += scale * 2.0
    return q


# neighbouring values of h, A may differ by up to 5.4e11 and the indicator stay inside b <= 1e25: the largest scale below keeps the
# differences of `stencils` (|d| up to ~4 scale) inside that
SCALES = [0.0, 1e-12, 1e-8, 1e-3, 1.0, 1e4, 1e8, 1e11]


@pytest.mark.parametrize("pos", [True, False])
def test_five_instruction_indicator_equals_the_six_instruction_one(pos):
    rng = np.random.default_rng(11)
    for scale in SCALES:
        for eps4 in (8 * SW_EPS, 32 * SW_EPS):
            qu, qv = stencils(rng, 400, scale), stencils(rng, 400, scale)
            six = betas4(qv, None, pos, start=betas4(qu, eps4, pos))
            five = betas4_vel(qu, qv, eps4, pos)
            ref = betas4_vel(qu.astype(LD), qv.astype(LD), LD(eps4), pos)
            for a, b, r in zip(six, five, ref):
                assert (b >= eps4).all() and np.isfinite(b).all()
                # a sum of non-negative terms, each formed with at most four roundings (g: two, its square, the 13/3 factor) and added
                # with at most four more: 8 eps of the sum covers either form; the forms then agree to 16
                assert (np.abs(b - r) <= 8 * EPS * r).all(), scale
                assert (np.abs(a - r) <= 8 * EPS * r).all(), scale
                assert (np.abs(a - b) <= 16 * EPS * r).all(), scale


@pytest.mark.parametrize("pos", [True, False])
def test_pair_finish_equals_the_two_single_finishes(pos):
    rng = np.random.default_rng(12)
    worst = 0.0
    for sa in SCALES:
        for sb in SCALES:                                  # every pairing of scales: S1 and S2 up to 140 decades apart
            qa, qb = stencils(rng, 200, sa), stencils(rng, 200, sb)
            pa = parts(qa, betas4(qa, 4 * SW_EPS, pos))
            pb = parts(qb, betas4_vel(qb, stencils(rng, 200, sb), 8 * SW_EPS, pos))
            Sa, Sb = pa[0], pb[0]
            prod = Sa * Sb
            assert np.isfinite(prod).all() and (prod > 0).all()
            r12 = 1.0 / prod
            assert (r12 >= np.finfo(np.float64).tiny).all()                 # a normal number: v_rcp_f64 need not handle denormals
            for p, S, other in ((pa, Sa, Sb), (pb, Sb, Sa)):
                single, pair = finish(p, 1.0 / S), finish(p, other * r12)
                # 1/S by the pair: the product, its reciprocal and the last multiply round once each -> within 2 eps of 1/S (and the
                # correctly rounded 1/S within eps/2); the kernel's one-Newton-step reciprocal adds its 2.2e-15 to either form alike
                assert (np.abs(other * r12 * S - 1.0) <= 2.5 * EPS).all()
                # the reciprocal multiplies only num/6; the rest of the finish rounds at the scale of the values it adds
                S_, num, dd, c = p
                corr = np.abs(num) / S / 6.0
                bound = 2.5 * EPS * corr + 2 * EPS * (np.abs(c) + np.abs(dd) / 6.0 + corr)
                assert (np.abs(pair - single) <= bound).all(), (sa, sb)
                pl = [x.astype(LD) for x in p]
                exact = finish(pl, 1 / pl[0])
                assert (np.abs(pair - exact) <= 2 * bound).all(), (sa, sb)
                worst = max(worst, float((np.abs(pair - single) / np.maximum(bound, 1e-300)).max()))
    print(f"pair against single finish: worst difference / bound {worst:.3g}")


def test_product_is_finite_inside_the_documented_bound_and_not_beyond():
    T = np.float64
    rng = np.random.default_rng(13)
    # indicator triples over the whole domain, corners included
    lo, hi = np.log10(B_MIN), np.log10(B_MAX)
    b = 10.0 ** rng.uniform(lo, hi, size=(20000, 3))
    corners = np.array([[x, y, z] for x in (B_MIN, B_MAX) for y in (B_MIN, B_MAX) for z in (B_MIN, B_MAX)])
    b = np.concatenate([b, corners, np.full((1, 3), B_MAX)])
    q = np.zeros((b.shape[0], 5))
    S = parts(q, [b[:, 0], b[:, 1], b[:, 2]])[0]
    bmax, bmin = b.max(axis=1), b.min(axis=1)
    assert (S <= (20.0 / 3.0) * bmax ** 6 * (1 + 8 * EPS)).all()              # the bounds the domain is derived from
    assert (S >= (10.0 / 3.0) * bmin ** 6 * (1 - 8 * EPS)).all()
    # every pairing of the extremes
    Smax, Smin = S.max(), S.min()
    assert Smin >= 1.3e-32 and Smin * Smin >= 1.8e-64
    with np.errstate(over="raise"):
        prod = T(Smax) * T(Smax)
        assert np.isfinite(prod) and prod <= 44.5 * B_MAX ** 12
        assert 1.0 / prod >= np.finfo(T).tiny
        assert np.isfinite(T(Smax) * S).all() and (T(Smin) * S > 0).all()
    # just inside: every triple with b <= 3.5e25 is covered by S <= 20/3 b^6; equal indicators (tau = 0, S = 10/3 b^6) are the largest S
    # there is, and with them the product overflows just beyond b = 4.0e25
    for triple in ([B_MIN, B_SAFE, B_SAFE], [B_SAFE, B_SAFE, B_MIN], [B_SAFE] * 3):
        S_in = T(parts(np.zeros((1, 5)), [T(x) for x in triple])[0])
        assert np.isfinite(S_in * S_in) and S_in <= (10.0 / 3.0) * B_SAFE ** 6 * (1 + 8 * EPS)
    S_out = T(parts(np.zeros((1, 5)), [T(1.01 * B_OVERFLOW)] * 3)[0])
    with np.errstate(over="ignore"):
        assert np.isfinite(S_out) and np.isinf(S_out * S_out)                # (the single form is still fine there: it overflows from 1.9e51 on)
    # the field scale behind the bound (the kernel pairs the h and A reconstructions): neighbouring values differing by at most D give
    # b <= 33.4 D^2, so D <= 5.4e11 keeps b <= 1e25
    assert 33.4 * 5.4e11 ** 2 <= B_MAX
    worst = np.array([[0.0, 1.0, 0.0, 1.0, 0.0], [1.0, 0.0, 1.0, 0.0, 1.0]])   # |d| = 1 with alternating sign: the largest e and g
    for pos in (True, False):
        assert max(float(x.max()) for x in betas4(worst, 0.0, pos)) <= 33.4


@pytest.mark.parametrize("name", ["scaled", "perturbed"])
@pytest.mark.parametrize("Nx,Ny", RP.SHAPES)
def test_oracle_is_finite_and_well_conditioned_on_the_extra_sets(oracle, name, Nx, Ny):
    """What the GPU test compares against must itself be trustworthy there: finite, and stable under input perturbations of one part
    in 1e16 to within a tenth of the bound the GPU test allows (tol x max(max|G|, S))."""
    H = SC.H
    q = RP.fields(name, Nx, Ny, 7000 + Nx)
    tend = lambda f: [Hh.interior(g, Nx, Ny, H, H).copy() for g in
                      oracle.tendencies(*f, Nx, Ny, H, H, SC.DX, SC.DY, 1, 1, float(SC.GRAV), float(SC.FCOR), nthreads=SC.NTHREADS)]
    G = tend(q)
    F = oracle.lorentz_jacobian(q[3], q[2], Nx, Ny, H, H, SC.DX, SC.DY, nthreads=SC.NTHREADS)
    force = max(float(np.abs(Hh.interior(w, Nx, Ny, H, H)).max()) for w in F)
    scales = [float(s) for s in Hh.term_scales("VectorInvariant", q, SC.DX, SC.DY, force)]
    assert all(np.isfinite(g).all() for g in G) and np.isfinite(force) and all(np.isfinite(s) and s > 0 for s in scales)
    rng = np.random.default_rng(5)
    qp = []
    for a in q:
        I = Hh.interior(a, Nx, Ny, H, H) * (1.0 + 1e-16 * rng.choice([-1.0, 1.0], size=(Ny, Nx)))     # (rounds to +-1 ulp or to nothing)
        b = np.zeros_like(a)
        Hh.interior(b, Nx, Ny, H, H)[...] = I
        qp.append(np.ascontiguousarray(Hh.fill_halo_periodic(b, Nx, Ny, H, H)))
    Gp = tend(qp)
    tol = RP.SETS[name]
    for f in range(4):
        bound = tol * max(float(np.abs(G[f]).max()), scales[f])
        moved = float(np.abs(Gp[f] - G[f]).max())
        print(f"  {name} {Nx}x{Ny} field {f}: max|G| {np.abs(G[f]).max():.3e}, S {scales[f]:.3e}, moved {moved:.3e} = {moved / bound:.3g} of the bound")
        assert moved <= 0.1 * bound
