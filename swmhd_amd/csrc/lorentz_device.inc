// Device functions of the two Lorentz-force formulations, written against accessor functors so that the stand-alone
// operator kernels and the fused tendency kernels share one implementation.  Included inside
// namespace swmhd { namespace { ... } } after STRICT is defined.
//
//   Jacobian form    jacobian_formulation/sw_mhd_jacobian_functions.jl:1-26
//   divergence form  divergence_formulation/sw_mhd_divergence_functions.jl:1-170   (periodic interior branches)
//
// An accessor F(ii, jj) returns the value at tile-local cell (ii, jj); Julia's (i, j) <-> (ii, jj) by a constant shift.

template <typename T>
struct Geo {
    T dx, dy, rdx, rdy;
};

// 1/x for fast builds: fp64 v_rcp + two Newton steps (full accuracy to rounding), fp32 the hardware reciprocal -- instead of the
// ~12-instruction IEEE divides
template <typename T> __device__ __forceinline__ T fast_recip(T x) {
    if constexpr (sizeof(T) == 8 && !__is_same(T, double)) {          // packed fp32 pair (sw_device.inc's sw_f2): one v_rcp_f32 per column
        T r; r.x = __builtin_amdgcn_rcpf(x.x); r.y = __builtin_amdgcn_rcpf(x.y);
        return r;
    } else if constexpr (sizeof(T) == 8) {
        double r = __builtin_amdgcn_rcp(x);
        double e = __builtin_fma(-x, r, 1.0);
        r = __builtin_fma(r, e, r);
        e = __builtin_fma(-x, r, 1.0);
        return __builtin_fma(r, e, r);
    } else {
        return __builtin_amdgcn_rcpf(x);   // v_rcp_f32 (1 ulp) instead of the ~12-instruction correctly rounded fp32 divide
    }
}

// 1/x from v_rcp_f64 and ONE Newton step (2.2e-15 relative, tools/rcp_probe.hip): two FMAs less than fast_recip.  Used only by the fp64
// vector-invariant marching kernel, whose Lorentz term is held to 1e-13 of its scale; the stand-alone operator kernels keep fast_recip.
__device__ __forceinline__ double recip_newton1(double x) {
    const double r = __builtin_amdgcn_rcp(x);
    return __builtin_fma(r, __builtin_fma(-x, r, 1.0), r);
}

// reference :3   upwind_biased_product(ũ, ψᴸ, ψᴿ) = ((ũ + |ũ|) ψᴸ + (ũ − |ũ|) ψᴿ) / 2
template <typename T>
__device__ __forceinline__ T upwind_biased_product(T u, T pL, T pR) {
    T au = (u < T(0)) ? -u : u;
    if constexpr (STRICT) return ((u + au) * pL + (u - au) * pR) / T(2);
    else return T(0.5) * ((u + au) * pL + (u - au) * pR);
}
// reference :25-32  third-order biased interpolants:  left = (2c0 + 5cm1 − cm2)/6, right = (−cp1 + 5c0 + 2cm1)/6
template <typename T>
__device__ __forceinline__ T left3(T cm2, T cm1, T c0) {
    if constexpr (STRICT) return (T(2) * c0 + T(5) * cm1 - cm2) / T(6);
    else return (T(2) * c0 + T(5) * cm1 - cm2) * T(1.0 / 6.0);
}
template <typename T>
__device__ __forceinline__ T right3(T cm1, T c0, T cp1) {
    if constexpr (STRICT) return (-cp1 + T(5) * c0 + T(2) * cm1) / T(6);
    else return (-cp1 + T(5) * c0 + T(2) * cm1) * T(1.0 / 6.0);
}

// ---- Jacobian form ---------------------------------------------------------------------------------
// cell-centre Bx, By (:1-7):  By = ℑxᶜᵃᵃ(∂xᶠᶜᶜ A)/h ;  Bx = −ℑyᵃᶜᵃ(∂yᶜᶠᶜ A)/h
template <typename T, typename AF, typename HF>
__device__ __forceinline__ void jac_centre_B(const AF &A_, const HF &H_, int ii, int jj, const Geo<T> &g, T &bx, T &by) {
    T hc = H_(ii, jj);
    if constexpr (STRICT) {
        by = (((A_(ii, jj) - A_(ii - 1, jj)) / g.dx + (A_(ii + 1, jj) - A_(ii, jj)) / g.dx) / T(2)) / hc;
        bx = -(((A_(ii, jj) - A_(ii, jj - 1)) / g.dy + (A_(ii, jj + 1) - A_(ii, jj)) / g.dy) / T(2)) / hc;
    } else {
        T rh = fast_recip<T>(hc);
        by = (T(0.5) * g.rdx) * (A_(ii + 1, jj) - A_(ii - 1, jj)) * rh;
        bx = -(T(0.5) * g.rdy) * (A_(ii, jj + 1) - A_(ii, jj - 1)) * rh;
    }
}
// lorentz_force_func_x/y (:20-26) = jacobian_x/y (:10-18) / face-averaged h, given centre B accessors
// RCP1 (fast builds, T = double): the two face reciprocals from one recip_newton1 of the product of the two h sums
template <typename T, bool RCP1 = false, typename AF, typename HF, typename BXF, typename BYF>
__device__ __forceinline__ void jac_force(const AF &A_, const HF &H_, const BXF &BX_, const BYF &BY_, int i, int j,
                                          const Geo<T> &g, T &fx, T &fy) {
    if constexpr (STRICT) {
        T dxA = (A_(i, j) - A_(i - 1, j)) / g.dx;
        T g00 = (BX_(i - 1, j) - BX_(i - 1, j - 1)) / g.dy, g10 = (BX_(i, j) - BX_(i, j - 1)) / g.dy;
        T g01 = (BX_(i - 1, j + 1) - BX_(i - 1, j)) / g.dy, g11 = (BX_(i, j + 1) - BX_(i, j)) / g.dy;
        T T1 = ((g00 + g10) / T(2) + (g01 + g11) / T(2)) / T(2);
        T d00 = (A_(i - 1, j) - A_(i - 1, j - 1)) / g.dy, d10 = (A_(i, j) - A_(i, j - 1)) / g.dy;
        T d01 = (A_(i - 1, j + 1) - A_(i - 1, j)) / g.dy, d11 = (A_(i, j + 1) - A_(i, j)) / g.dy;
        T T2 = ((d00 + d10) / T(2) + (d01 + d11) / T(2)) / T(2);
        T dxBx = (BX_(i, j) - BX_(i - 1, j)) / g.dx;
        T p1 = dxA * T1, p2 = T2 * dxBx;
        T jx = p1 - p2;
        fx = (T(1) / ((H_(i - 1, j) + H_(i, j)) / T(2))) * jx;
        T e00 = (A_(i, j - 1) - A_(i - 1, j - 1)) / g.dx, e10 = (A_(i + 1, j - 1) - A_(i, j - 1)) / g.dx;
        T e01 = dxA, e11 = (A_(i + 1, j) - A_(i, j)) / g.dx;
        T T3 = ((e00 + e10) / T(2) + (e01 + e11) / T(2)) / T(2);
        T dyBy = (BY_(i, j) - BY_(i, j - 1)) / g.dy;
        T q00 = (BY_(i, j - 1) - BY_(i - 1, j - 1)) / g.dx, q10 = (BY_(i + 1, j - 1) - BY_(i, j - 1)) / g.dx;
        T q01 = (BY_(i, j) - BY_(i - 1, j)) / g.dx, q11 = (BY_(i + 1, j) - BY_(i, j)) / g.dx;
        T T4 = ((q00 + q10) / T(2) + (q01 + q11) / T(2)) / T(2);
        T p3 = T3 * dyBy, p4 = d10 * T4;
        T jy = p3 - p4;
        fy = (T(1) / ((H_(i, j - 1) + H_(i, j)) / T(2))) * jy;
    } else {
        const T qy = T(0.25) * g.rdy, qx = T(0.25) * g.rdx;
        T dxA = (A_(i, j) - A_(i - 1, j)) * g.rdx;
        T dyA = (A_(i, j) - A_(i, j - 1)) * g.rdy;
        T T1 = qy * ((BX_(i - 1, j + 1) - BX_(i - 1, j - 1)) + (BX_(i, j + 1) - BX_(i, j - 1)));
        T T2 = qy * ((A_(i - 1, j + 1) - A_(i - 1, j - 1)) + (A_(i, j + 1) - A_(i, j - 1)));
        T dxBx = (BX_(i, j) - BX_(i - 1, j)) * g.rdx;
        T T3 = qx * ((A_(i + 1, j - 1) - A_(i - 1, j - 1)) + (A_(i + 1, j) - A_(i - 1, j)));
        T dyBy = (BY_(i, j) - BY_(i, j - 1)) * g.rdy;
        T T4 = qx * ((BY_(i + 1, j - 1) - BY_(i - 1, j - 1)) + (BY_(i + 1, j) - BY_(i - 1, j)));
        if constexpr (RCP1) {   // both from ONE reciprocal, of the product of the two h sums: 1/hx = hy r, 1/hy = hx r (h^2 is far inside the range)
            const T hx = H_(i - 1, j) + H_(i, j), hy = H_(i, j - 1) + H_(i, j);
            const T r2 = T(2) * recip_newton1(hx * hy);
            fx = (dxA * T1 - T2 * dxBx) * (hy * r2);
            fy = (T3 * dyBy - dyA * T4) * (hx * r2);
        } else {
            fx = (dxA * T1 - T2 * dxBx) * (T(2) * fast_recip<T>(H_(i - 1, j) + H_(i, j)));
            fy = (T3 * dyBy - dyA * T4) * (T(2) * fast_recip<T>(H_(i, j - 1) + H_(i, j)));
        }
    }
}

// ---- divergence form -------------------------------------------------------------------------------
// face-located hBx, Bx (fcc) and hBy, By (cfc)  (:134-148)
template <typename T, typename AF, typename HF>
__device__ __forceinline__ void div_faces(const AF &A_, const HF &H_, int ii, int jj, const Geo<T> &g, T &hbx, T &bx, T &hby,
                                          T &by) {
    if constexpr (STRICT) {
        T d00 = (A_(ii - 1, jj) - A_(ii - 1, jj - 1)) / g.dy, d10 = (A_(ii, jj) - A_(ii, jj - 1)) / g.dy;
        T d01 = (A_(ii - 1, jj + 1) - A_(ii - 1, jj)) / g.dy, d11 = (A_(ii, jj + 1) - A_(ii, jj)) / g.dy;
        T m = ((d00 + d10) / T(2) + (d01 + d11) / T(2)) / T(2);   // ℑxyᶠᶜᵃ(∂yᶜᶠᶜ A)
        hbx = -m;
        bx = -m / ((H_(ii - 1, jj) + H_(ii, jj)) / T(2));
        T e00 = (A_(ii, jj - 1) - A_(ii - 1, jj - 1)) / g.dx, e10 = (A_(ii + 1, jj - 1) - A_(ii, jj - 1)) / g.dx;
        T e01 = (A_(ii, jj) - A_(ii - 1, jj)) / g.dx, e11 = (A_(ii + 1, jj) - A_(ii, jj)) / g.dx;
        T n = ((e00 + e10) / T(2) + (e01 + e11) / T(2)) / T(2);   // ℑxyᶜᶠᵃ(∂xᶠᶜᶜ A)
        hby = n;
        by = n / ((H_(ii, jj - 1) + H_(ii, jj)) / T(2));
    } else {
        T m = -(T(0.25) * g.rdy) * ((A_(ii - 1, jj + 1) - A_(ii - 1, jj - 1)) + (A_(ii, jj + 1) - A_(ii, jj - 1)));
        T n = (T(0.25) * g.rdx) * ((A_(ii + 1, jj - 1) - A_(ii - 1, jj - 1)) + (A_(ii + 1, jj) - A_(ii - 1, jj)));
        hbx = m;
        bx = m * (T(2) * fast_recip<T>(H_(ii - 1, jj) + H_(ii, jj)));
        hby = n;
        by = n * (T(2) * fast_recip<T>(H_(ii, jj - 1) + H_(ii, jj)));
    }
}
// the four Maxwell-stress fluxes (:38-132, :150-160), periodic branch (:54-56, :78-80, :102-104, :126-128);
// Ax = dy, Ay = dx (dz = 1)
template <typename T> __device__ __forceinline__ T half_sum(T a, T b) { return STRICT ? (a + b) / T(2) : T(0.5) * (a + b); }

// `Bounded` wall branches of the four fluxes (reference :42-53, :66-77, :90-101, :114-125).  n is the flux's 1-based index along
// the bounded direction; the reference tests n == a, a+1, b-1, b in that order:
//   code 1: both sides = 1st-order right-biased value     code 2: left = 1st-order left,  right = 3rd-order right
//   code 3: left = 3rd-order left, right = 1st-order right code 4: both sides = 1st-order left-biased value    0: interior
__device__ __forceinline__ int wall_code(int bounded, int n, int a, int b) {
    if (!bounded) return 0;
    return n == a ? 1 : (n == a + 1 ? 2 : (n == b - 1 ? 3 : (n == b ? 4 : 0)));
}
template <typename T>
__device__ __forceinline__ void biased_pair(int code, T l3, T r3, T l1, T r1, T &L, T &R) {
    switch (code) {
        case 1: L = r1; R = r1; break;
        case 2: L = l1; R = r3; break;
        case 3: L = l3; R = r1; break;
        case 4: L = l1; R = l1; break;
        default: L = l3; R = r3;
    }
}

template <typename T, typename HBXF, typename BXF>   // lorentz_flux_hBx_bx @ccc ; wall indices i = 0, 1, Nx-1, Nx
__device__ __forceinline__ T div_F1(const HBXF &HBX_, const BXF &BX_, int ii, int jj, const Geo<T> &g, int code = 0) {
    T ut = half_sum<T>(HBX_(ii, jj), HBX_(ii + 1, jj));
    T uL, uR;
    biased_pair<T>(code, left3<T>(BX_(ii - 1, jj), BX_(ii, jj), BX_(ii + 1, jj)), right3<T>(BX_(ii, jj), BX_(ii + 1, jj), BX_(ii + 2, jj)),
                   BX_(ii, jj), BX_(ii + 1, jj), uL, uR);
    return (g.dy * T(1)) * upwind_biased_product<T>(ut, uL, uR);
}
template <typename T, typename HBYF, typename BXF>   // lorentz_flux_hBy_bx @ffc ; wall indices j = 1, 2, Ny, Ny+1
__device__ __forceinline__ T div_F2(const HBYF &HBY_, const BXF &BX_, int ii, int jj, const Geo<T> &g, int code = 0) {
    T vt = half_sum<T>(HBY_(ii - 1, jj), HBY_(ii, jj));
    T uL, uR;
    biased_pair<T>(code, left3<T>(BX_(ii, jj - 2), BX_(ii, jj - 1), BX_(ii, jj)), right3<T>(BX_(ii, jj - 1), BX_(ii, jj), BX_(ii, jj + 1)),
                   BX_(ii, jj - 1), BX_(ii, jj), uL, uR);
    return (g.dx * T(1)) * upwind_biased_product<T>(vt, uL, uR);
}
template <typename T, typename HBXF, typename BYF>   // lorentz_flux_hBx_by @ffc ; wall indices i = 1, 2, Nx, Nx+1
__device__ __forceinline__ T div_G1(const HBXF &HBX_, const BYF &BY_, int ii, int jj, const Geo<T> &g, int code = 0) {
    T ut = half_sum<T>(HBX_(ii, jj - 1), HBX_(ii, jj));
    T vL, vR;
    biased_pair<T>(code, left3<T>(BY_(ii - 2, jj), BY_(ii - 1, jj), BY_(ii, jj)), right3<T>(BY_(ii - 1, jj), BY_(ii, jj), BY_(ii + 1, jj)),
                   BY_(ii - 1, jj), BY_(ii, jj), vL, vR);
    return (g.dy * T(1)) * upwind_biased_product<T>(ut, vL, vR);
}
template <typename T, typename HBYF, typename BYF>   // lorentz_flux_hBy_by @ccc ; wall indices j = 0, 1, Ny-1, Ny
__device__ __forceinline__ T div_G2(const HBYF &HBY_, const BYF &BY_, int ii, int jj, const Geo<T> &g, int code = 0) {
    T vt = half_sum<T>(HBY_(ii, jj), HBY_(ii, jj + 1));
    T vL, vR;
    biased_pair<T>(code, left3<T>(BY_(ii, jj - 1), BY_(ii, jj), BY_(ii, jj + 1)), right3<T>(BY_(ii, jj), BY_(ii, jj + 1), BY_(ii, jj + 2)),
                   BY_(ii, jj), BY_(ii, jj + 1), vL, vR);
    return (g.dx * T(1)) * upwind_biased_product<T>(vt, vL, vR);
}
