// Device math shared by the tendency kernels: WENO5 (Z weights), upwinding, centred 4th-order interpolation.
// Included inside namespace swmhd { namespace { ... } } of a translation unit that has defined STRICT.
//
// STRICT: expression trees identical to oracle/sw_rhs.inc (which restates Oceananigans' published scheme; PARITY
//         UNPINNED against the library itself) -- bit-identical results when compiled -ffp-contract=off.
// FAST:   one Newton-refined reciprocal per reconstruction instead of four IEEE divides, upwind side selected
//         before reconstructing (the other side is multiplied by zero in upwind_biased_product), FMA contraction.

// Packed fp32: `sw_f2` = two adjacent columns per lane in one 64-bit register pair; every helper below is generic over it (clang
// turns its arithmetic into v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32: one issue slot for two columns).  Comparisons give
// per-element masks and `m ? a : b` selects per element.
// (the typedef lives in common.hpp: the Lorentz operator kernels use it too)
template <typename T> struct is_f64 { static constexpr bool value = false; };
template <> struct is_f64<double> { static constexpr bool value = true; };
template <typename T> struct is_pk { static constexpr bool value = false; };
template <> struct is_pk<sw_f2> { static constexpr bool value = true; };

template <typename T> __device__ __forceinline__ T sq(T x) { return x * x; }

// 1/x: IEEE divide in strict builds; v_rcp + Newton steps in fast builds (fp64: 2 steps ~ 0.5 ulp-ish, fp32: hw rcp).
template <typename T> __device__ __forceinline__ T recip(T x) {
    if constexpr (STRICT) {
        return T(1) / x;
    } else if constexpr (is_pk<T>::value) {
        T r; r.x = __builtin_amdgcn_rcpf(x.x); r.y = __builtin_amdgcn_rcpf(x.y);   // (no packed reciprocal: one v_rcp_f32 per column)
        return r;
    } else if constexpr (is_f64<T>::value) {
        double r = __builtin_amdgcn_rcp(x);
        double e = __builtin_fma(-x, r, 1.0);
        r = __builtin_fma(r, e, r);
        e = __builtin_fma(-x, r, 1.0);
        return __builtin_fma(r, e, r);
    } else {
        return __builtin_amdgcn_rcpf(x);
    }
}

template <typename T> __device__ __forceinline__ T beta_a(T p1, T p2, T p3) { return T(13.0 / 12.0) * sq(p1 - T(2) * p2 + p3) + T(0.25) * sq(T(3) * p1 - T(4) * p2 + p3); }
template <typename T> __device__ __forceinline__ T beta_b(T p1, T p2, T p3) { return T(13.0 / 12.0) * sq(p1 - T(2) * p2 + p3) + T(0.25) * sq(p1 - p3); }
template <typename T> __device__ __forceinline__ T beta_c(T p1, T p2, T p3) { return T(13.0 / 12.0) * sq(p1 - T(2) * p2 + p3) + T(0.25) * sq(p1 - T(4) * p2 + T(3) * p3); }
template <typename T> __device__ __forceinline__ T pL0(T p1, T p2, T p3) { return T(1.0 / 3.0) * p1 + T(5.0 / 6.0) * p2 - T(1.0 / 6.0) * p3; }
template <typename T> __device__ __forceinline__ T pL1(T p1, T p2, T p3) { return -T(1.0 / 6.0) * p1 + T(5.0 / 6.0) * p2 + T(1.0 / 3.0) * p3; }
template <typename T> __device__ __forceinline__ T pL2(T p1, T p2, T p3) { return T(1.0 / 3.0) * p1 - T(7.0 / 6.0) * p2 + T(11.0 / 6.0) * p3; }
template <typename T> __device__ __forceinline__ T pR0(T p1, T p2, T p3) { return T(11.0 / 6.0) * p1 - T(7.0 / 6.0) * p2 + T(1.0 / 3.0) * p3; }
template <typename T> __device__ __forceinline__ T pR1(T p1, T p2, T p3) { return T(1.0 / 3.0) * p1 + T(5.0 / 6.0) * p2 - T(1.0 / 6.0) * p3; }
template <typename T> __device__ __forceinline__ T pR2(T p1, T p2, T p3) { return -T(1.0 / 6.0) * p1 + T(5.0 / 6.0) * p2 + T(1.0 / 3.0) * p3; }

#define SW_C3_0 T(3.0 / 10.0)
#define SW_C3_1 T(3.0 / 5.0)
#define SW_C3_2 T(1.0 / 10.0)
#define SW_EPS T(1e-6)

// strict: Z-WENO weights exactly as the oracle's zweno_w
template <typename T>
__device__ __forceinline__ void zweno_w(T b0, T b1, T b2, T d0, T d1, T d2, T &w0, T &w1, T &w2) {
    T tau = b2 - b0;
    if (tau < T(0)) tau = -tau;
    T a0 = d0 * (T(1) + sq(tau / (b0 + SW_EPS)));
    T a1 = d1 * (T(1) + sq(tau / (b1 + SW_EPS)));
    T a2 = d2 * (T(1) + sq(tau / (b2 + SW_EPS)));
    T s = a0 + a1 + a2;
    w0 = a0 / s; w1 = a1 / s; w2 = a2 / s;
}

// fast: sum_k w_k p_k with w_k = a_k / sum a, a_k = d_k (1 + tau^2/b_k^2), evaluated with ONE reciprocal:
// multiply numerator and denominator by b0^2 b1^2 b2^2 (fp64 range is ample: b >= 1e-6).  fp32 keeps per-term rcp.
template <typename T>
__device__ __forceinline__ T zweno_combine_fast(T b0, T b1, T b2, T d0, T d1, T d2, T p0, T p1, T p2) {
    T tau = b2 - b0;
    T t2 = tau * tau;
    b0 += SW_EPS; b1 += SW_EPS; b2 += SW_EPS;
    if constexpr (is_f64<T>::value) {
        T s0 = b0 * b0, s1 = b1 * b1, s2 = b2 * b2;
        T n0 = d0 * (s0 + t2) * (s1 * s2);
        T n1 = d1 * (s1 + t2) * (s0 * s2);
        T n2 = d2 * (s2 + t2) * (s0 * s1);
        return (n0 * p0 + n1 * p1 + n2 * p2) * recip<T>(n0 + n1 + n2);
    } else {
        T r0 = recip<T>(b0), r1 = recip<T>(b1), r2 = recip<T>(b2);
        T a0 = d0 * (T(1) + t2 * r0 * r0), a1 = d1 * (T(1) + t2 * r1 * r1), a2 = d2 * (T(1) + t2 * r2 * r2);
        return (a0 * p0 + a1 * p1 + a2 * p2) * recip<T>(a0 + a1 + a2);
    }
}

// q[0..5] = ψ(f-3 .. f+2) around face f.  Strict forms, as the oracle's weno_left / weno_right.
// The right-biased smoothness indicators are NOT the mirror images of the left-biased ones: the library version the reference ran
// (Oceananigans v0.7x, `right_biased_β₀/β₂`) applies the end-point forms (ψ₁-4ψ₂+3ψ₃)² to its ψ₀ = (f, f+1, f+2) and (3ψ₁-4ψ₂+ψ₃)² to
// its ψ₂ = (f-2, f-1, f) -- the left-biased forms swapped, not reflected.  Pinned by the reference's energy plots (DESIGN.md
// section 3: the reflected form misses the late-time energy drift of every vector-invariant run, this form reproduces it).
template <typename T> __device__ __forceinline__ T weno_left(const T *q) {
    T b0 = beta_a(q[2], q[3], q[4]), b1 = beta_b(q[1], q[2], q[3]), b2 = beta_c(q[0], q[1], q[2]);
    T w0, w1, w2; zweno_w<T>(b0, b1, b2, SW_C3_0, SW_C3_1, SW_C3_2, w0, w1, w2);
    return w0 * pL0(q[2], q[3], q[4]) + w1 * pL1(q[1], q[2], q[3]) + w2 * pL2(q[0], q[1], q[2]);
}
template <typename T> __device__ __forceinline__ T weno_right(const T *q) {
    T b0 = beta_c(q[3], q[4], q[5]), b1 = beta_b(q[2], q[3], q[4]), b2 = beta_a(q[1], q[2], q[3]);
    T w0, w1, w2; zweno_w<T>(b0, b1, b2, SW_C3_2, SW_C3_1, SW_C3_0, w0, w1, w2);
    return w0 * pR0(q[3], q[4], q[5]) + w1 * pR1(q[2], q[3], q[4]) + w2 * pR2(q[1], q[2], q[3]);
}
template <typename T> __device__ __forceinline__ T weno_left_vel(const T *z, const T *u, const T *v) {
    T b0 = T(0.5) * (beta_a(u[2], u[3], u[4]) + beta_a(v[2], v[3], v[4]));
    T b1 = T(0.5) * (beta_b(u[1], u[2], u[3]) + beta_b(v[1], v[2], v[3]));
    T b2 = T(0.5) * (beta_c(u[0], u[1], u[2]) + beta_c(v[0], v[1], v[2]));
    T w0, w1, w2; zweno_w<T>(b0, b1, b2, SW_C3_0, SW_C3_1, SW_C3_2, w0, w1, w2);
    return w0 * pL0(z[2], z[3], z[4]) + w1 * pL1(z[1], z[2], z[3]) + w2 * pL2(z[0], z[1], z[2]);
}
template <typename T> __device__ __forceinline__ T weno_right_vel(const T *z, const T *u, const T *v) {
    T b0 = T(0.5) * (beta_c(u[3], u[4], u[5]) + beta_c(v[3], v[4], v[5]));
    T b1 = T(0.5) * (beta_b(u[2], u[3], u[4]) + beta_b(v[2], v[3], v[4]));
    T b2 = T(0.5) * (beta_a(u[1], u[2], u[3]) + beta_a(v[1], v[2], v[3]));
    T w0, w1, w2; zweno_w<T>(b0, b1, b2, SW_C3_2, SW_C3_1, SW_C3_0, w0, w1, w2);
    return w0 * pR0(z[3], z[4], z[5]) + w1 * pR1(z[2], z[3], z[4]) + w2 * pR2(z[1], z[2], z[3]);
}

// upwind_biased_product (Oceananigans.Advection; same expression as sw_mhd_divergence_functions.jl:3)
template <typename T> __device__ __forceinline__ T upw(T u, T pL, T pR) {
    T au = (u < T(0)) ? -u : u;
    if constexpr (STRICT) return ((u + au) * pL + (u - au) * pR) / T(2);
    else return T(0.5) * ((u + au) * pL + (u - au) * pR);
}

// ---- fast WENO5-Z in difference form -------------------------------------------------------------------------------
// Five values ordered from the upwind-most cell, (a,b,c,d,e) = psi(f-3..f+1) for flow in +x / psi(f+2..f-2) for flow in -x;
// the face lies between c and d.  The candidate values and optimal weights are mirror images of each other; the smoothness
// indicators are NOT (see weno_right above): in this ordering the left-biased side has g0 = d4 - 3 d3, g2 = 3 d2 - d1 and the
// right-biased side g0 = 3 d4 - d3, g2 = d2 - 3 d1, i.e. g0 = kB d4 - kA d3, g2 = kA d2 - kB d1 with (kA, kB) = (3, 1) | (1, 3).  With first differences d1..d4, second differences
// e1..e3 and third differences f1, f2 the three candidate values are  p1 = c + (d2 + 2 d3)/6,  p0 = p1 - f2/6,  p2 = p1 - f1/3
// and the smoothness indicators are  b0 = 13/12 e3^2 + 1/4 (d4 - 3 d3)^2,  b1 = 13/12 e2^2 + 1/4 (d2 + d3)^2,
// b2 = 13/12 e1^2 + 1/4 (3 d2 - d1)^2.   With Z weights  w_k ~ c_k (1 + tau^2 / b_k^2)  (c = 3/10, 6/10, 1/10) multiplied
// through by b0^2 b1^2 b2^2,   value = p1 - (n0 f2 + 2 n2 f1) / (6 (n0 + n1 + n2)).
// The single reciprocal multiplies only the nonlinear correction (third differences), so v_rcp_f64 + ONE Newton step
// (2.2e-15 relative, tools/rcp_probe.hip) is ample.  ~55 fp64 instructions instead of ~65 for the textbook form.
template <typename T> struct WenoDiffs { T d1, d2, d3, d4, e1, e2, e3; };
template <typename T> __device__ __forceinline__ WenoDiffs<T> weno_diffs(const T *q) {
    WenoDiffs<T> w;
    w.d1 = q[1] - q[0]; w.d2 = q[2] - q[1]; w.d3 = q[3] - q[2]; w.d4 = q[4] - q[3];
    w.e1 = w.d2 - w.d1; w.e2 = w.d3 - w.d2; w.e3 = w.d4 - w.d3;
    return w;
}
// FOUR TIMES the smoothness indicators of the three sub-stencils, plus `eps4`: the Z weights depend only on ratios of the
// b_k = beta_k + eps (tau = |b2 - b0| scales with them), so any common factor is free -- and 4 beta = 13/3 e^2 + g^2 costs one
// multiply less per indicator than 13/12 e^2 + 1/4 g^2; eps rides in on the first fma.
template <typename T> __device__ __forceinline__ T fma_(T a, T b, T c) {
    if constexpr (is_f64<T>::value) return __builtin_fma(a, b, c);
    else if constexpr (is_pk<T>::value) return __builtin_elementwise_fma(a, b, c);
    else return __builtin_fmaf(a, b, c);
}
// `pos`: the left-biased side (flow towards +); a per-element mask for the packed type.
template <typename T, typename M> __device__ __forceinline__ void weno_betas4(const WenoDiffs<T> &w, T eps4, M pos, T &b0, T &b1, T &b2) {
    const T kA = pos ? T(3) : T(1), kB = pos ? T(1) : T(3);
    const T g0 = fma_<T>(kB, w.d4, -(kA * w.d3)), g1 = w.d2 + w.d3, g2 = fma_<T>(kA, w.d2, -(kB * w.d1));
    b0 = fma_<T>(T(13.0 / 3.0) * w.e3, w.e3, fma_<T>(g0, g0, eps4));
    b1 = fma_<T>(T(13.0 / 3.0) * w.e2, w.e2, fma_<T>(g1, g1, eps4));
    b2 = fma_<T>(T(13.0 / 3.0) * w.e1, w.e1, fma_<T>(g2, g2, eps4));
}
// ---- MARCH64: the arithmetic of the fp64 vector-invariant marching kernel ----------------------------------------------
// The helpers below take a compile-time switch `MARCH64` (default off).  Only k_tendency_vi_march<double, ...> turns it on; every
// other kernel instantiates the forms above and below exactly as before (their register budgets are pinned by tests, and editing a
// shared helper in place re-rolls the allocation of all of them).  The MARCH64 forms are algebraically the same expressions with
// fewer instructions; results differ by rounding only.
//
// The velocity-stencil indicator is the sum of the u- and the v-stencil's.  Formed in one chain per b_k, eps riding in on the innermost
// fma (no separate bu_k + bv_k adds), and with the 13/3 factor paid once: five instructions
//     b_k = 13/3 (e_u^2 + e_v^2) + (g_u^2 + g_v^2 + eps)
// where accumulating weno_betas4 over the two stencils took six (a 13/3 e multiply and two fmas, twice).
template <typename T, typename M> __device__ __forceinline__ void weno_betas4_vel(const WenoDiffs<T> &wu, const WenoDiffs<T> &wv, T eps4, M pos, T &b0, T &b1, T &b2) {
    const T kA = pos ? T(3) : T(1), kB = pos ? T(1) : T(3);
    const T gu0 = fma_<T>(kB, wu.d4, -(kA * wu.d3)), gu1 = wu.d2 + wu.d3, gu2 = fma_<T>(kA, wu.d2, -(kB * wu.d1));
    const T gv0 = fma_<T>(kB, wv.d4, -(kA * wv.d3)), gv1 = wv.d2 + wv.d3, gv2 = fma_<T>(kA, wv.d2, -(kB * wv.d1));
    b0 = fma_<T>(T(13.0 / 3.0), fma_<T>(wu.e3, wu.e3, wv.e3 * wv.e3), fma_<T>(gu0, gu0, fma_<T>(gv0, gv0, eps4)));
    b1 = fma_<T>(T(13.0 / 3.0), fma_<T>(wu.e2, wu.e2, wv.e2 * wv.e2), fma_<T>(gu1, gu1, fma_<T>(gv1, gv1, eps4)));
    b2 = fma_<T>(T(13.0 / 3.0), fma_<T>(wu.e1, wu.e1, wv.e1 * wv.e1), fma_<T>(gu2, gu2, fma_<T>(gv2, gv2, eps4)));
}
// 1/h for the centre B of the Lorentz force: one Newton step under MARCH64 (lorentz_device.inc: recip_newton1), else recip
template <typename T, bool MARCH64> __device__ __forceinline__ T recip_lorentz(T x) {
    if constexpr (MARCH64) return recip_newton1(x);
    else return recip<T>(x);
}
// MARCH64: weno_combine_diff (below) in two parts, so that two reconstructions can share ONE v_rcp_f64.  The first part is everything
// up to the reciprocal: S, num (as below), dd = d2 + 2 d3 and the centre value c; the finish takes r ~ 1/S:
//     value = c + (1/6) [dd - num r].
template <typename T> struct WenoParts { T S, num, dd, c; };
template <typename T> __device__ __forceinline__ WenoParts<T> weno_combine_parts(const WenoDiffs<T> &wz, T c, T b0, T b1, T b2) {
    const T f1 = wz.e2 - wz.e1, f2 = wz.e3 - wz.e2;
    const T tau = b2 - b0, t2 = tau * tau;
    const T s0 = b0 * b0, s1 = b1 * b1, s2 = b2 * b2;
    const T q0 = s1 * s2, q1 = s0 * s2, q2 = s0 * s1, P = s0 * q0;
    const T m0 = fma_<T>(t2, q0, P), m1 = fma_<T>(t2, q1, P), m2 = fma_<T>(t2, q2, P);
    WenoParts<T> p;
    p.S = fma_<T>(T(1.0 / 3.0), m2, fma_<T>(T(2), m1, m0));
    p.num = fma_<T>(m0, f2, T(2.0 / 3.0) * (m2 * f1));
    p.dd = fma_<T>(T(2), wz.d3, wz.d2);
    p.c = c;
    return p;
}
template <typename T> __device__ __forceinline__ T weno_combine_finish(const WenoParts<T> &p, T r) {
    return fma_<T>(T(1.0 / 6.0), fma_<T>(-p.num, r, p.dd), p.c);
}
// Two reconstructions, one reciprocal: r12 = 1/(S1 S2) by v_rcp_f64 + one Newton step, then 1/S1 = S2 r12 and 1/S2 = S1 r12 -- one
// multiply, one v_rcp_f64, two fmas and two multiplies (~8 issue slots at the ~3 slots of a v_rcp_f64, tools/valu_probe.hip) where two
// separate reciprocals with their Newton steps take ~10.  Each 1/S carries two roundings more than the single form (the product's and the last
// multiply's: 2.4e-15 instead of 2.2e-15 relative) and multiplies only the nonlinear correction.
// DOMAIN (no run-time guard: a select per reconstruction would cost what the pairing saves).  S = m0 + 2 m1 + m2/3 with
// m_k = P + tau^2 q_k <= 2 b^6 for indicators b_k <= b, so 10/3 b_min^6 <= S <= 20/3 b^6; equal indicators give S = 10/3 b^6.
//   lower end: b_k >= 4 eps = 4e-6 gives S >= 1.3e-32 and S1 S2 >= 1.8e-64: no underflow;
//   upper end: S1 S2 <= 44.5 b^12 is finite for every b <= 3.5e25 and, at 11.1 b^12 for equal indicators, overflows (1.8e308) from
//   b = 4.0e25 on.  The documented domain is b <= 1e25: there S1 S2 <= 4.5e301 and r12 is a normal number.  (The
//   single form, S alone, overflows from b = 1.9e51 on.)  The kernel pairs the reconstructions of h and A only (x-face fluxes, y-face fluxes):
//   with neighbouring values differing by at most D their b <= 33.4 D^2, so b <= 1e25 holds while neighbouring h and neighbouring A
//   differ by no more than 5.4e11.  The velocity-stencil reconstructions keep the single form and its range.
template <typename T> __device__ __forceinline__ void weno_combine_finish_pair(const WenoParts<T> &pa, const WenoParts<T> &pb, T &va, T &vb) {
    const T r = recip_newton1(pa.S * pb.S);
    va = weno_combine_finish<T>(pa, pb.S * r);
    vb = weno_combine_finish<T>(pb, pa.S * r);
}
// value at the face given the differences of the reconstructed quantity (wz, centre value c) and b_k ~ beta_k + eps (any
// common factor).  With s_k = b_k^2, q_k = prod_{j != k} s_j, P = s0 s1 s2 the multiplied-through weights are
// m_k = P + tau^2 q_k (times c_k = 3/10, 6/10, 1/10); everything is divided by c_0.
// MARCH64: value = c + (1/6) [(d2 + 2 d3) - num r] in three fmas (p1 and the last fma above take five).
template <typename T, bool MARCH64 = false> __device__ __forceinline__ T weno_combine_diff(const WenoDiffs<T> &wz, T c, T b0, T b1, T b2) {
    const T p1 = c + fma_<T>(T(1.0 / 3.0), wz.d3, T(1.0 / 6.0) * wz.d2);
    const T f1 = wz.e2 - wz.e1, f2 = wz.e3 - wz.e2;
    const T tau = b2 - b0, t2 = tau * tau;
    if constexpr (is_f64<T>::value) {
        const T s0 = b0 * b0, s1 = b1 * b1, s2 = b2 * b2;
        const T q0 = s1 * s2, q1 = s0 * s2, q2 = s0 * s1, P = s0 * q0;
        const T m0 = fma_<T>(t2, q0, P), m1 = fma_<T>(t2, q1, P), m2 = fma_<T>(t2, q2, P);
        const T S = fma_<T>(T(1.0 / 3.0), m2, fma_<T>(T(2), m1, m0));            // (0.3 m0 + 0.6 m1 + 0.1 m2) / 0.3
        const T num = fma_<T>(m0, f2, T(2.0 / 3.0) * (m2 * f1));               // (0.3 m0 f2 + 0.2 m2 f1) / 0.3
        double r = __builtin_amdgcn_rcp(S);
        r = __builtin_fma(r, __builtin_fma(-S, r, 1.0), r);
        if constexpr (MARCH64) return weno_combine_finish<T>(WenoParts<T>{S, num, fma_<T>(T(2), wz.d3, wz.d2), c}, r);   // (the single form: velocity stencils, segment prologues)
        else return fma_<T>(T(-1.0 / 6.0) * num, r, p1);
    } else {   // fp32: the multiplied-through weights would leave the exponent range; per-term reciprocals instead
        const T r0 = recip<T>(b0), r1 = recip<T>(b1), r2 = recip<T>(b2);
        const T a0 = T(0.3) * (T(1) + t2 * r0 * r0), a1 = T(0.6) * (T(1) + t2 * r1 * r1), a2 = T(0.1) * (T(1) + t2 * r2 * r2);
        return p1 - (T(1.0 / 6.0) * (a0 * f2 + T(2) * a2 * f1)) * recip<T>(a0 + a1 + a2);
    }
}
// MARCH64: weno5_upwind_ordered / upwind_weno (below) up to the reciprocal: the marching kernel pairs two of them in
// weno_combine_finish_pair and multiplies by the advecting velocity itself.
template <typename T, typename M> __device__ __forceinline__ WenoParts<T> weno5_upwind_ordered_parts(const T *q, M pos) {
    const WenoDiffs<T> w = weno_diffs<T>(q);
    T b0, b1, b2;
    weno_betas4<T>(w, T(4) * SW_EPS, pos, b0, b1, b2);
    return weno_combine_parts<T>(w, q[2], b0, b1, b2);
}
template <typename T> __device__ __forceinline__ WenoParts<T> upwind_weno_parts(T u, const T *q) {
    const auto pos = u >= T(0);
    T w[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) w[k] = pos ? q[k] : q[5 - k];
    return weno5_upwind_ordered_parts<T>(w, pos);
}
template <typename T, bool MARCH64 = false, typename M> __device__ __forceinline__ T weno5_upwind_ordered(const T *q, M pos) {
    const WenoDiffs<T> w = weno_diffs<T>(q);
    T b0, b1, b2;
    weno_betas4<T>(w, T(4) * SW_EPS, pos, b0, b1, b2);
    return weno_combine_diff<T, MARCH64>(w, q[2], b0, b1, b2);
}
// Same with VelocityStencil smoothness: reconstructs z using the mean of the u- and v-stencil indicators (here: 8x the mean).
template <typename T, bool MARCH64 = false, typename M> __device__ __forceinline__ T weno5_vel_upwind_ordered(const T *z, const T *u, const T *v, M pos) {
    if constexpr (MARCH64) {
        T b0, b1, b2;
        weno_betas4_vel<T>(weno_diffs<T>(u), weno_diffs<T>(v), T(8) * SW_EPS, pos, b0, b1, b2);
        return weno_combine_diff<T, true>(weno_diffs<T>(z), z[2], b0, b1, b2);
    }
    T bu0, bu1, bu2, bv0, bv1, bv2;
    weno_betas4<T>(weno_diffs<T>(u), T(0), pos, bu0, bu1, bu2);
    weno_betas4<T>(weno_diffs<T>(v), T(8) * SW_EPS, pos, bv0, bv1, bv2);
    return weno_combine_diff<T>(weno_diffs<T>(z), z[2], bu0 + bv0, bu1 + bv1, bu2 + bv2);
}

// upwind_biased_product(u, weno_left(q), weno_right(q)).
// fast: reconstruct only the upwind side, from the values in upwind order.
template <typename T, bool MARCH64 = false> __device__ __forceinline__ T upwind_weno(T u, const T *q) {
    if constexpr (STRICT) {
        return upw<T>(u, weno_left<T>(q), weno_right<T>(q));
    } else {
        const auto pos = u >= T(0);
        T w[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) w[k] = pos ? q[k] : q[5 - k];
        return u * weno5_upwind_ordered<T, MARCH64>(w, pos);
    }
}
template <typename T> __device__ __forceinline__ T upwind_weno_vel(T u, const T *z, const T *us, const T *vs) {
    if constexpr (STRICT) {
        return upw<T>(u, weno_left_vel<T>(z, us, vs), weno_right_vel<T>(z, us, vs));
    } else {
        const auto pos = u >= T(0);
        T wz[5], wu[5], wv[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) { wz[k] = pos ? z[k] : z[5 - k]; wu[k] = pos ? us[k] : us[5 - k]; wv[k] = pos ? vs[k] : vs[5 - k]; }
        return u * weno5_vel_upwind_ordered<T>(wz, wu, wv, pos);
    }
}

// upwind_weno_vel for the y direction of the marching kernel, from RAW columns: z[6] = zeta(c, jo-2 .. jo+3) at the vorticity
// points, uw[7] = u(c, jo-3 .. jo+3) and sv[6] = v(c-1, j) + v(c, j) for j = jo-2 .. jo+3.  The velocity-stencil indicators
// need only DIFFERENCES of uf = (u(j-1) + u(j))/2 and vf = sv/2, and they are quadratic in them: with D = 2 d they come out
// 4x larger, the sign of the (mirrored) stencil drops out, and -- all b_k carrying the same factor -- the weights are unchanged.
// Saves forming uf, vf (24 ops) and one select per field.
template <typename T, bool MARCH64 = false> __device__ __forceinline__ T upwind_weno_vel_raw(T u, const T *z, const T *uw, const T *sv) {
    const auto pos = u >= T(0);
    T Du[5], Dv[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) { Du[k] = uw[k + 2] - uw[k]; Dv[k] = sv[k + 1] - sv[k]; }   // 2 (uf[k+1] - uf[k]), 2 (vf[k+1] - vf[k])
    WenoDiffs<T> wu, wv;
    wu.d1 = pos ? Du[0] : Du[4]; wu.d2 = pos ? Du[1] : Du[3]; wu.d3 = Du[2]; wu.d4 = pos ? Du[3] : Du[1];
    wv.d1 = pos ? Dv[0] : Dv[4]; wv.d2 = pos ? Dv[1] : Dv[3]; wv.d3 = Dv[2]; wv.d4 = pos ? Dv[3] : Dv[1];
    wu.e1 = wu.d2 - wu.d1; wu.e2 = wu.d3 - wu.d2; wu.e3 = wu.d4 - wu.d3;
    wv.e1 = wv.d2 - wv.d1; wv.e2 = wv.d3 - wv.d2; wv.e3 = wv.d4 - wv.d3;
    T wz[5];
    if constexpr (MARCH64) {
        T b0, b1, b2;
        weno_betas4_vel<T>(wu, wv, T(32) * SW_EPS, pos, b0, b1, b2);
#pragma unroll
        for (int k = 0; k < 5; ++k) wz[k] = pos ? z[k] : z[5 - k];
        return u * weno_combine_diff<T, true>(weno_diffs<T>(wz), wz[2], b0, b1, b2);
    }
    T bu0, bu1, bu2, bv0, bv1, bv2;
    weno_betas4<T>(wu, T(0), pos, bu0, bu1, bu2);
    weno_betas4<T>(wv, T(32) * SW_EPS, pos, bv0, bv1, bv2);            // 16 beta_u + 16 beta_v + 32 eps = 32 (mean + eps)
#pragma unroll
    for (int k = 0; k < 5; ++k) wz[k] = pos ? z[k] : z[5 - k];
    return u * weno_combine_diff<T>(weno_diffs<T>(wz), wz[2], bu0 + bv0, bu1 + bv1, bu2 + bv2);
}

// ---- topologically conditional reconstruction (Bounded directions): oracle/sw_rhs.inc left_order / right_order / sym_fourth ----
// WENO5 (boundary buffer 2) -> UpwindBiasedThirdOrder (buffer 1) -> first order; CenteredFourthOrder (buffer 1) -> second order.
// idx = the interpolant's own 1-based index (face index for face interpolants, centre index for centre interpolants), N = cells.
__device__ __forceinline__ int left_order(bool bounded, int idx, int N) {
    if (!bounded || (idx > 2 && idx < N)) return 5;
    return (idx > 1 && idx < N + 1) ? 3 : 1;
}
__device__ __forceinline__ int right_order(bool bounded, int idx, int N) {
    if (!bounded || (idx > 1 && idx < N - 1)) return 5;
    return (idx > 0 && idx < N) ? 3 : 1;
}
__device__ __forceinline__ bool sym_fourth(bool bounded, int idx, int N) { return !bounded || (idx > 1 && idx < N); }
template <typename T> __device__ __forceinline__ T left_value(int order, const T *q) {
    if (order == 5) return weno_left<T>(q);
    if (order == 3) { if constexpr (STRICT) return (T(2) * q[3] + T(5) * q[2] - q[1]) / T(6); else return (T(2) * q[3] + T(5) * q[2] - q[1]) * T(1.0 / 6.0); }
    return q[2];
}
template <typename T> __device__ __forceinline__ T right_value(int order, const T *q) {
    if (order == 5) return weno_right<T>(q);
    if (order == 3) { if constexpr (STRICT) return (-q[4] + T(5) * q[3] + T(2) * q[2]) / T(6); else return (-q[4] + T(5) * q[3] + T(2) * q[2]) * T(1.0 / 6.0); }
    return q[3];
}
// upwind_biased_product(u, left(q), right(q)) with the orders of a Bounded direction (oL = oR = 5: the periodic forms above)
template <typename T> __device__ __forceinline__ T upwind_recon(T u, const T *q, int oL, int oR) {
    if (oL == 5 && oR == 5) return upwind_weno<T>(u, q);
    if constexpr (STRICT) {
        return upw<T>(u, left_value<T>(oL, q), right_value<T>(oR, q));
    } else {   // only the upwind side contributes
        const auto pos = u >= T(0);
        const int o = pos ? oL : oR;
        if (o == 5) { T w[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) w[k] = pos ? q[k] : q[5 - k];
            return u * weno5_upwind_ordered<T>(w, pos); }
        return u * (pos ? left_value<T>(o, q) : right_value<T>(o, q));
    }
}
template <typename T> __device__ __forceinline__ T upwind_recon_vel(T u, const T *z, const T *us, const T *vs, int oL, int oR) {
    if (oL == 5 && oR == 5) return upwind_weno_vel<T>(u, z, us, vs);
    if constexpr (STRICT) {
        const T L = oL == 5 ? weno_left_vel<T>(z, us, vs) : left_value<T>(oL, z);
        const T R = oR == 5 ? weno_right_vel<T>(z, us, vs) : right_value<T>(oR, z);
        return upw<T>(u, L, R);
    } else {
        const auto pos = u >= T(0);
        const int o = pos ? oL : oR;
        if (o == 5) { T wz[5], wu[5], wv[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) { wz[k] = pos ? z[k] : z[5 - k]; wu[k] = pos ? us[k] : us[5 - k]; wv[k] = pos ? vs[k] : vs[5 - k]; }
            return u * weno5_vel_upwind_ordered<T>(wz, wu, wv, pos); }
        return u * (pos ? left_value<T>(o, z) : right_value<T>(o, z));
    }
}

// symmetric_interpolate for WENO5 = CenteredFourthOrder: ℑ³ = ℑ − ℑ(δ²)/6, midway between b and c
template <typename T> __device__ __forceinline__ T sym4(T a, T b, T c, T d) {
    if constexpr (STRICT) {
        T d2b = (c - b) - (b - a), d2c = (d - c) - (c - b);
        return (b + c) / T(2) - ((d2b + d2c) / T(2)) / T(6);
    } else {
        return T(7.0 / 12.0) * (b + c) - T(1.0 / 12.0) * (a + d);
    }
}
// ... CenteredSecondOrder inside the boundary buffer of a Bounded direction
template <typename T> __device__ __forceinline__ T symc(bool fourth, T a, T b, T c, T d) {
    if (fourth) return sym4<T>(a, b, c, d);
    if constexpr (STRICT) return (b + c) / T(2); else return T(0.5) * (b + c);
}
