// Fused tendency kernel, LDS-tiled form (v1): all four tendencies (G_q1, G_q2, G_h, G_A) of the shallow-water MHD
// model in one pass over the prognostic fields, the Lorentz force fused in (no Fx/Fy round trip through HBM).
//
// This is the whole-field form of Oceananigans' ShallowWaterModel tendency kernels *including* the reference's forcing
// callback (SURVEY.md 8(a) row A9 + A1-A8):
//   FORM 1  VectorInvariantFormulation (u, v, h) + tracer A, forcing = lorentz_force_func_x/y   SWMHD_example.jl:21-33
//   FORM 0  ConservativeFormulation   (uh, vh, h) + tracer A, forcing = div_lorentz_x/y         divergence_sw_mhd.jl:19-31
// The base RHS restates the library's published scheme (oracle/sw_rhs.inc, PARITY UNPINNED); the forcing is the
// reference's own code (lorentz_device.inc).  STRICT builds are bit-identical to the oracle.
//
// Kernels only: included by tendency_fast.hip / tendency_strict.hip with SWMHD_STRICT defined, after launch_plan.hpp (cons_minwaves)
// and before tendency_launch.inc, which launches them.

#ifndef SWMHD_STRICT
#error "include with SWMHD_STRICT defined"
#endif

namespace swmhd {
namespace {

constexpr bool STRICT = (SWMHD_STRICT != 0);

#include <type_traits>
#include "tile_common.inc"
#include "lorentz_device.inc"
#include "sw_device.inc"

// Ensemble workgroup (ENS variant): pick the member, point every field of `a` at it, return the tile index within the member.
template <typename T>
__device__ __forceinline__ unsigned ens_member(EnsTendArgs<T> &a, unsigned ntiles, unsigned &m) {
    unsigned t;
    if (a.fold) {
        const unsigned L = xcd_remap(blockIdx.x, ntiles * (unsigned)a.members);
        m = L / ntiles; t = L - m * ntiles;
    } else {
        m = blockIdx.y; t = xcd_remap(blockIdx.x, ntiles);
    }
    const long o = (long)m * a.stride_m;
    a.q1 += o; a.q2 += o; a.h += o; a.A += o;
    a.G1 += o; a.G2 += o; a.Gh += o; a.GA += o;
#pragma unroll
    for (int f = 0; f < 4; ++f) {
        if (a.Unew[f]) a.Unew[f] += o;
        if (a.Gm[f]) a.Gm[f] += o;
    }
    return t;
}

// Per-member parameters (PAR variant): (g, f, dt) of member m from the device table, and the products of dt the host forms for one
// grid (tend_common: dtg = dt * gamma, dtw = dt * zeta in the first anchored stage), each one multiply in T of the same operands.  m
// comes from blockIdx alone, so the address is workgroup-uniform and the three values arrive by scalar loads: no VGPR holds them.
// (cu and cg, the coefficient form of the marching kernels, are not read by this kernel.)
template <typename T>
__device__ __forceinline__ void ens_member_params(EnsParTendArgs<T> &a, unsigned m) {
    const T *p = a.params + (long)ENS_NPARAMS * m;
    a.grav = p[0]; a.fcor = p[1]; a.dt = p[2];
    a.dtg = a.dt * a.gamma;
    a.dtw = a.dt * a.zeta;
}

// The G- forms of the fused substep in fast builds, U + dt (gamma G [+ zeta Gm]), with their rounding written down as explicit fused
// multiply-adds in T: c1 = dt gamma and c2 = dt zeta (one multiply each, of uniform operands), then fma(c1, G, U) for a first stage and
// fma(c2, Gm, fma(c1, G, U)) with a G- operand -- one v_fma per addend, no separate add.  Written as U + (dt gamma) G the expression
// was regrouped under -fassociative-math and contracted under -ffp-contract=fast as the compiler liked, and differently in the
// single-grid and the ensemble instantiation of the kernel below (last bits of the new state: tests/test_ensemble_stage_matrix_gpu.py).
// An fma intrinsic is neither split nor regrouped, and reassociate(off) keeps the two multiplies that feed it as written, so every
// instantiation rounds alike and an ensemble member is bitwise the single grid in these forms, as it is in the anchor form, whose
// products come from the host.  (#pragma clang fp contract(off) would NOT do: with -ffp-contract=fast the backend still fuses.)
__device__ __forceinline__ float fma_t(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_t(double a, double b, double c) { return __builtin_fma(a, b, c); }
template <typename T>
__device__ __forceinline__ T substep_pinned(T U, T dt, T gamma, T G) {   // first stage
#pragma clang fp reassociate(off)
    const T c1 = dt * gamma;
    return fma_t(c1, G, U);
}
template <typename T>
__device__ __forceinline__ T substep_pinned(T U, T dt, T gamma, T G, T zeta, T Gm) {
#pragma clang fp reassociate(off)
    const T c1 = dt * gamma, c2 = dt * zeta;
    return fma_t(c2, Gm, fma_t(c1, G, U));
}

// FORM: 0 conservative, 1 vector invariant.  LOR: 0 none, 1 Jacobian (FORM 1 only), 2 divergence (FORM 0 only).
// BND: at least one direction is Bounded -- reconstructions near walls drop to the boundary schemes (sw_device.inc) and the divergence-
// form Lorentz fluxes take the reference's wall branches (sw_mhd_divergence_functions.jl:42-53,66-77,90-101,114-125).  With
// BND = false every order is the compile-time constant 5 and the code is the periodic kernel.
// ENS: ensemble launch (EnsTendArgs) -- the workgroup's member offsets every field pointer; otherwise the body is the same.
// PAR (with ENS): the member also brings its own g, f and dt (EnsParTendArgs, ens_member_params); the body is the same again.
template <typename T, int FORM, int LOR, int TX, int TYB, int RY, bool BND = false, bool ENS = false, bool PAR = false>
__global__ __launch_bounds__(TX *TYB) void k_tendency_tile(TileArgs<T, ENS, PAR> a, int ntx, int nty) {
    static_assert(ENS || !PAR, "per-member parameters need an ensemble launch");
    constexpr int TY = TYB * RY, NT = TX * TYB;
    constexpr int W = TX + 6, HH = TY + 6;
    __shared__ T s1[HH][W];   // u | uh   (Face, Center)
    __shared__ T s2[HH][W];   // v | vh   (Center, Face)
    __shared__ T sh[HH][W];   // h
    __shared__ T sA[HH][W];   // A
    // Lorentz intermediates: LOR 1 -> centre Bx, By on tile+1 ; LOR 2 -> face hBx, Bx, hBy, By on tile+2
    constexpr int LW = LOR == 1 ? TX + 2 : (LOR == 2 ? TX + 4 : 1), LH = LOR == 1 ? TY + 2 : (LOR == 2 ? TY + 4 : 1);
    constexpr int LO = LOR == 1 ? 1 : 2;
    __shared__ T sL0[LH][LW];
    __shared__ T sL1[LH][LW];
    __shared__ T sL2[LOR == 2 ? LH : 1][LOR == 2 ? LW : 1];
    __shared__ T sL3[LOR == 2 ? LH : 1][LOR == 2 ? LW : 1];

    unsigned bid;
    if constexpr (ENS) {
        unsigned m;
        bid = ens_member<T>(a, (unsigned)(ntx * nty), m);
        if constexpr (PAR) ens_member_params<T>(a, m);
    } else bid = xcd_remap(blockIdx.x, (unsigned)(ntx * nty));
    // tile rows of the optional second row range follow those of the first
    const int tyi = (int)(bid / ntx), ntya = (a.j1 - a.j0 + TY - 1) / TY;
    const bool second = tyi >= ntya;
    int txi = (int)(bid % ntx);
    if (a.edge_cols && txi > 0) txi = (a.Nx + TX - 1) / TX - (ntx - txi);   // x-wall frame: tile column 0 and the last one (or two)
    const int x0 = txi * TX, y0 = second ? a.j0b + (tyi - ntya) * TY : a.j0 + tyi * TY, jend = second ? a.j1b : a.j1;
    const int tid = threadIdx.y * TX + threadIdx.x;
    const int xlo = -a.Hx, xhi = a.Nx + a.Hx - 1, ylo = -a.Hy, yhi = a.Ny + a.Hy - 1;
    const Geo<T> g{a.dx, a.dy, a.rdx, a.rdy};

    load_tile<T, W, HH, NT>(s1, a.q1, a.sy, x0 - 3, y0 - 3, xlo, xhi, ylo, yhi, tid, a.Nx, a.Ny, a.wrap);
    load_tile<T, W, HH, NT>(s2, a.q2, a.sy, x0 - 3, y0 - 3, xlo, xhi, ylo, yhi, tid, a.Nx, a.Ny, a.wrap);
    load_tile<T, W, HH, NT>(sh, a.h, a.sy, x0 - 3, y0 - 3, xlo, xhi, ylo, yhi, tid, a.Nx, a.Ny, a.wrap);
    load_tile<T, W, HH, NT>(sA, a.A, a.sy, x0 - 3, y0 - 3, xlo, xhi, ylo, yhi, tid, a.Nx, a.Ny, a.wrap);
    __syncthreads();

    auto U_ = [&](int ii, int jj) -> T { return s1[jj + 3][ii + 3]; };
    auto V_ = [&](int ii, int jj) -> T { return s2[jj + 3][ii + 3]; };
    auto H_ = [&](int ii, int jj) -> T { return sh[jj + 3][ii + 3]; };
    auto A_ = [&](int ii, int jj) -> T { return sA[jj + 3][ii + 3]; };
    auto L0_ = [&](int ii, int jj) -> T { return sL0[jj + LO][ii + LO]; };
    auto L1_ = [&](int ii, int jj) -> T { return sL1[jj + LO][ii + LO]; };
    auto L2_ = [&](int ii, int jj) -> T { return sL2[jj + LO][ii + LO]; };
    auto L3_ = [&](int ii, int jj) -> T { return sL3[jj + LO][ii + LO]; };

    if constexpr (LOR == 1) {
        for (int e = tid; e < LW * LH; e += NT) {
            int r = e / LW, c = e - r * LW;
            T bx, by;
            jac_centre_B<T>(A_, H_, c - 1, r - 1, g, bx, by);
            sL0[r][c] = bx; sL1[r][c] = by;
        }
        __syncthreads();
    } else if constexpr (LOR == 2) {
        for (int e = tid; e < LW * LH; e += NT) {
            int r = e / LW, c = e - r * LW;
            T hbx, bx, hby, by;
            div_faces<T>(A_, H_, c - 2, r - 2, g, hbx, bx, hby, by);
            sL0[r][c] = hbx; sL1[r][c] = bx; sL2[r][c] = hby; sL3[r][c] = by;
        }
        __syncthreads();
    }

    // gather ψ(f-3 .. f+2) along x / y
    auto gx6 = [&](auto &F, int f, int jj, T *q) {
#pragma unroll
        for (int m = 0; m < 6; ++m) q[m] = F(f - 3 + m, jj);
    };
    auto gy6 = [&](auto &F, int ii, int f, T *q) {
#pragma unroll
        for (int m = 0; m < 6; ++m) q[m] = F(ii, f - 3 + m);
    };
    // orders of the interpolant of tile-local index (ii | jj) in x | y: its 1-based index is x0 + ii + 1 | y0 + jj + 1
    const bool bx = BND && a.topo_x == 1, by = BND && (a.topo_y & 1);
    // y-slab of a Bounded-y chain (TOPO_OPEN_*): an open side moves the slab's row indices TOPO_FAR away from that wall position, so
    // the wall tests below see the rows next to a cut as interior rows; (0, Ny) for a whole Bounded direction
    const int yb = BND && (a.topo_y & TOPO_OPEN_SOUTH) ? TOPO_FAR : 0;
    const int yN = BND ? a.Ny + yb + ((a.topo_y & TOPO_OPEN_NORTH) ? TOPO_FAR : 0) : a.Ny;
    auto oLx = [&](int ii) -> int { return BND ? left_order(bx, x0 + ii + 1, a.Nx) : 5; };
    auto oRx = [&](int ii) -> int { return BND ? right_order(bx, x0 + ii + 1, a.Nx) : 5; };
    auto oLy = [&](int jj) -> int { return BND ? left_order(by, yb + y0 + jj + 1, yN) : 5; };
    auto oRy = [&](int jj) -> int { return BND ? right_order(by, yb + y0 + jj + 1, yN) : 5; };
    auto s4x = [&](int ii) -> bool { return BND ? sym_fourth(bx, x0 + ii + 1, a.Nx) : true; };
    auto s4y = [&](int jj) -> bool { return BND ? sym_fourth(by, yb + y0 + jj + 1, yN) : true; };
    // advective_tracer_flux_x/y(U, c) = A_face * upwind(U[i,j], cL, cR)   (face interpolants: index = the face's)
    auto tflux_x = [&](auto &Uf, auto &C, int ii, int jj) -> T { T q[6]; gx6(C, ii, jj, q); return g.dy * upwind_recon<T>(Uf(ii, jj), q, oLx(ii), oRx(ii)); };
    auto tflux_y = [&](auto &Vf, auto &C, int ii, int jj) -> T { T q[6]; gy6(C, ii, jj, q); return g.dx * upwind_recon<T>(Vf(ii, jj), q, oLy(jj), oRy(jj)); };
    auto div_centered = [&](auto &Q1, auto &Q2, int ii, int jj) -> T {   // (1/Az)(δx(Δy q1) + δy(Δx q2))
        if constexpr (STRICT) return T(1) / (g.dx * g.dy) * ((g.dy * Q1(ii + 1, jj) - g.dy * Q1(ii, jj)) + (g.dx * Q2(ii, jj + 1) - g.dx * Q2(ii, jj)));
        else return (Q1(ii + 1, jj) - Q1(ii, jj)) * g.rdx + (Q2(ii, jj + 1) - Q2(ii, jj)) * g.rdy;
    };
    auto avg4 = [&](T p, T q, T r, T s) -> T {   // ((p+q)/2 + (r+s)/2)/2
        if constexpr (STRICT) return ((p + q) / T(2) + (r + s) / T(2)) / T(2);
        else return T(0.25) * ((p + q) + (r + s));
    };
    const T rAz = STRICT ? T(0) : g.rdx * g.rdy;

    const int i = threadIdx.x, gxi = x0 + i;
#pragma unroll 1
    for (int r = 0; r < RY; ++r) {
        const int j = threadIdx.y * RY + r, gyj = y0 + j;
        T G1, G2, Gh, GA;
        if constexpr (FORM == 1) {
            // ---------------- VectorInvariantFormulation ----------------
            auto zeta = [&](int ii, int jj) -> T {   // ζ₃ᶠᶠᶜ = (δxᶠ(Δy v) − δyᶠ(Δx u))/Az
                if constexpr (STRICT) return ((g.dy * V_(ii, jj) - g.dy * V_(ii - 1, jj)) - (g.dx * U_(ii, jj) - g.dx * U_(ii, jj - 1))) / (g.dx * g.dy);
                else return (V_(ii, jj) - V_(ii - 1, jj)) * g.rdx - (U_(ii, jj) - U_(ii, jj - 1)) * g.rdy;
            };
            auto u_ff = [&](int ii, int jj) -> T { return half_sum<T>(U_(ii, jj - 1), U_(ii, jj)); };
            auto v_ff = [&](int ii, int jj) -> T { return half_sum<T>(V_(ii - 1, jj), V_(ii, jj)); };
            auto Kh = [&](int ii, int jj) -> T {     // (ℑxᶜ(u²) + ℑyᶜ(v²))/2
                if constexpr (STRICT) return ((sq(U_(ii, jj)) + sq(U_(ii + 1, jj))) / T(2) + (sq(V_(ii, jj)) + sq(V_(ii, jj + 1))) / T(2)) / T(2);
                else return T(0.25) * ((sq(U_(ii, jj)) + sq(U_(ii + 1, jj))) + (sq(V_(ii, jj)) + sq(V_(ii, jj + 1))));
            };
            T z[6], us[6], vs[6];
            // vertical_vorticity_U = −upwind(v̂, ζL, ζR) along y
            T vhat;
            if constexpr (STRICT) vhat = (((g.dx * V_(i - 1, j) + g.dx * V_(i - 1, j + 1)) / T(2) + (g.dx * V_(i, j) + g.dx * V_(i, j + 1)) / T(2)) / T(2)) / g.dx;
            else vhat = T(0.25) * ((V_(i - 1, j) + V_(i - 1, j + 1)) + (V_(i, j) + V_(i, j + 1)));
#pragma unroll
            for (int m = 0; m < 6; ++m) { int jj = j - 2 + m; z[m] = zeta(i, jj); us[m] = u_ff(i, jj); vs[m] = v_ff(i, jj); }
            T vortU = -upwind_recon_vel<T>(vhat, z, us, vs, oLy(j), oRy(j));   // centre interpolant in y, index j
            T uhat;
            if constexpr (STRICT) uhat = (((g.dy * U_(i, j - 1) + g.dy * U_(i + 1, j - 1)) / T(2) + (g.dy * U_(i, j) + g.dy * U_(i + 1, j)) / T(2)) / T(2)) / g.dy;
            else uhat = T(0.25) * ((U_(i, j - 1) + U_(i + 1, j - 1)) + (U_(i, j) + U_(i + 1, j)));
#pragma unroll
            for (int m = 0; m < 6; ++m) { int ii = i - 2 + m; z[m] = zeta(ii, j); us[m] = u_ff(ii, j); vs[m] = v_ff(ii, j); }
            T vortV = upwind_recon_vel<T>(uhat, z, us, vs, oLx(i), oRx(i));    // centre interpolant in x, index i
            T k00 = Kh(i, j);
            T Fx = T(0), Fy = T(0);
            if constexpr (LOR == 1) jac_force<T>(A_, H_, L0_, L1_, i, j, g, Fx, Fy);
            if constexpr (STRICT) {
                T bern_u = (k00 - Kh(i - 1, j)) / g.dx;
                T div_u = vortU + bern_u;
                T pgx = a.grav * ((H_(i, j) - H_(i - 1, j)) / g.dx);
                T xfU = -a.fcor * avg4(V_(i - 1, j), V_(i, j), V_(i - 1, j + 1), V_(i, j + 1));
                G1 = -div_u - pgx - xfU + Fx;
                T bern_v = (k00 - Kh(i, j - 1)) / g.dy;
                T div_v = vortV + bern_v;
                T pgy = a.grav * ((H_(i, j) - H_(i, j - 1)) / g.dy);
                T yfU = a.fcor * avg4(U_(i, j - 1), U_(i + 1, j - 1), U_(i, j), U_(i + 1, j));
                G2 = -div_v - pgy - yfU + Fy;
                T Az = g.dx * g.dy;
                Gh = -(T(1) / Az * ((tflux_x(U_, H_, i + 1, j) - tflux_x(U_, H_, i, j)) + (tflux_y(V_, H_, i, j + 1) - tflux_y(V_, H_, i, j))));
                T div_Uc = T(1) / Az * ((tflux_x(U_, A_, i + 1, j) - tflux_x(U_, A_, i, j)) + (tflux_y(V_, A_, i, j + 1) - tflux_y(V_, A_, i, j)));
                GA = -div_Uc + A_(i, j) * div_centered(U_, V_, i, j);
            } else {
                G1 = -vortU - (k00 - Kh(i - 1, j)) * g.rdx - a.grav * (H_(i, j) - H_(i - 1, j)) * g.rdx
                     + a.fcor * avg4(V_(i - 1, j), V_(i, j), V_(i - 1, j + 1), V_(i, j + 1)) + Fx;
                G2 = -vortV - (k00 - Kh(i, j - 1)) * g.rdy - a.grav * (H_(i, j) - H_(i, j - 1)) * g.rdy
                     - a.fcor * avg4(U_(i, j - 1), U_(i + 1, j - 1), U_(i, j), U_(i + 1, j)) + Fy;
                Gh = -rAz * ((tflux_x(U_, H_, i + 1, j) - tflux_x(U_, H_, i, j)) + (tflux_y(V_, H_, i, j + 1) - tflux_y(V_, H_, i, j)));
                GA = -rAz * ((tflux_x(U_, A_, i + 1, j) - tflux_x(U_, A_, i, j)) + (tflux_y(V_, A_, i, j + 1) - tflux_y(V_, A_, i, j)))
                     + A_(i, j) * div_centered(U_, V_, i, j);
            }
        } else {
            // ---------------- ConservativeFormulation ----------------
            // x / y as the reference writes it (strict) | x * (Newton reciprocal of y) (fast: ~5 instructions instead of the ~15 of an
            // IEEE fp64 divide, 16 of them per cell here; the marching kernels do the same)
            auto dv = [&](T x, T y) -> T { if constexpr (STRICT) return x / y; else return x * recip<T>(y); };
            auto h_ff = [&](int ii, int jj) -> T { return avg4(H_(ii - 1, jj - 1), H_(ii, jj - 1), H_(ii - 1, jj), H_(ii, jj)); };
            auto flux_huu = [&](int ii, int jj) -> T {   // @ccc
                T q[6]; gx6(U_, ii + 1, jj, q);
                T ut = symc<T>(s4x(ii), g.dy * U_(ii - 1, jj), g.dy * U_(ii, jj), g.dy * U_(ii + 1, jj), g.dy * U_(ii + 2, jj));
                return dv(upwind_recon<T>(ut, q, oLx(ii), oRx(ii)), H_(ii, jj));
            };
            auto flux_hvu = [&](int ii, int jj) -> T {   // @ffc
                T q[6]; gy6(U_, ii, jj, q);
                T vt = symc<T>(s4x(ii), g.dx * V_(ii - 2, jj), g.dx * V_(ii - 1, jj), g.dx * V_(ii, jj), g.dx * V_(ii + 1, jj));
                return dv(upwind_recon<T>(vt, q, oLy(jj), oRy(jj)), h_ff(ii, jj));
            };
            auto flux_huv = [&](int ii, int jj) -> T {   // @ffc
                T q[6]; gx6(V_, ii, jj, q);
                T ut = symc<T>(s4y(jj), g.dy * U_(ii, jj - 2), g.dy * U_(ii, jj - 1), g.dy * U_(ii, jj), g.dy * U_(ii, jj + 1));
                return dv(upwind_recon<T>(ut, q, oLx(ii), oRx(ii)), h_ff(ii, jj));
            };
            auto flux_hvv = [&](int ii, int jj) -> T {   // @ccc
                T q[6]; gy6(V_, ii, jj + 1, q);
                T vt = symc<T>(s4y(jj), g.dx * V_(ii, jj - 1), g.dx * V_(ii, jj), g.dx * V_(ii, jj + 1), g.dx * V_(ii, jj + 2));
                return dv(upwind_recon<T>(vt, q, oLy(jj), oRy(jj)), H_(ii, jj));
            };
            T Fx = T(0), Fy = T(0);
            if constexpr (LOR == 2) {
                const T rAzs = T(1) / (g.dx * g.dy);
                // wall codes of the reference's Bounded branches (0 on periodic grids); Julia indices of this cell: (gxi+1, gyj+1)
                const int iJ = gxi + 1, jJ = yb + gyj + 1;
                const int cF1 = BND ? wall_code(bx, iJ, 0, a.Nx) : 0, cF1m = BND ? wall_code(bx, iJ - 1, 0, a.Nx) : 0;
                const int cG1 = BND ? wall_code(bx, iJ, 1, a.Nx + 1) : 0, cG1p = BND ? wall_code(bx, iJ + 1, 1, a.Nx + 1) : 0;
                const int cF2 = BND ? wall_code(by, jJ, 1, yN + 1) : 0, cF2p = BND ? wall_code(by, jJ + 1, 1, yN + 1) : 0;
                const int cG2 = BND ? wall_code(by, jJ, 0, yN) : 0, cG2m = BND ? wall_code(by, jJ - 1, 0, yN) : 0;
                Fx = rAzs * ((div_F1<T>(L0_, L1_, i, j, g, cF1) - div_F1<T>(L0_, L1_, i - 1, j, g, cF1m)) + (div_F2<T>(L2_, L1_, i, j + 1, g, cF2p) - div_F2<T>(L2_, L1_, i, j, g, cF2)));
                Fy = rAzs * ((div_G1<T>(L0_, L3_, i + 1, j, g, cG1p) - div_G1<T>(L0_, L3_, i, j, g, cG1)) + (div_G2<T>(L2_, L3_, i, j, g, cG2) - div_G2<T>(L2_, L3_, i, j - 1, g, cG2m)));
            }
            const T Vol = g.dx * g.dy;
            const T hg = T(0.5) * a.grav;
            T div_u = T(1) / Vol * ((flux_huu(i, j) - flux_huu(i - 1, j)) + (flux_hvu(i, j + 1) - flux_hvu(i, j)));
            T pgx = STRICT ? (hg * sq(H_(i, j)) - hg * sq(H_(i - 1, j))) / g.dx : (hg * sq(H_(i, j)) - hg * sq(H_(i - 1, j))) * g.rdx;
            T xfU = -a.fcor * avg4(V_(i - 1, j), V_(i, j), V_(i - 1, j + 1), V_(i, j + 1));
            G1 = -div_u - pgx - xfU + Fx;
            T div_v = T(1) / Vol * ((flux_huv(i + 1, j) - flux_huv(i, j)) + (flux_hvv(i, j) - flux_hvv(i, j - 1)));
            T pgy = STRICT ? (hg * sq(H_(i, j)) - hg * sq(H_(i, j - 1))) / g.dy : (hg * sq(H_(i, j)) - hg * sq(H_(i, j - 1))) * g.rdy;
            T yfU = a.fcor * avg4(U_(i, j - 1), U_(i + 1, j - 1), U_(i, j), U_(i + 1, j));
            G2 = -div_v - pgy - yfU + Fy;
            T dUh;
            if constexpr (STRICT) dUh = T(1) / Vol * ((g.dy * U_(i + 1, j) - g.dy * U_(i, j)) + (g.dx * V_(i, j + 1) - g.dx * V_(i, j)));
            else dUh = (U_(i + 1, j) - U_(i, j)) * g.rdx + (V_(i, j + 1) - V_(i, j)) * g.rdy;
            Gh = -dUh;
            T he = half_sum<T>(H_(i, j), H_(i + 1, j)), hw = half_sum<T>(H_(i - 1, j), H_(i, j));
            T hn = half_sum<T>(H_(i, j), H_(i, j + 1)), hs = half_sum<T>(H_(i, j - 1), H_(i, j));
            T fxe = dv(tflux_x(U_, A_, i + 1, j), he), fxw = dv(tflux_x(U_, A_, i, j), hw);
            T fyn = dv(tflux_y(V_, A_, i, j + 1), hn), fys = dv(tflux_y(V_, A_, i, j), hs);
            T div_Uc = T(1) / Vol * ((fxe - fxw) + (fyn - fys));
            T ue = dv(U_(i + 1, j), he), uw = dv(U_(i, j), hw), vn = dv(V_(i, j + 1), hn), vs_ = dv(V_(i, j), hs);
            T c_div_U = A_(i, j) * (T(1) / Vol * ((g.dy * ue - g.dy * uw) + (g.dx * vn - g.dx * vs_)));
            GA = -div_Uc + c_div_U;
        }
        if (gxi < a.Nx && gyj < jend) {
            const long o = (long)gyj * a.sy + gxi;
            if (a.store_G) { a.G1[o] = G1; a.G2[o] = G2; a.Gh[o] = Gh; a.GA[o] = GA; }
            if (a.fuse) {   // rk3_substep! fused in: the old state of this cell is already in LDS
                const T Gs[4] = {G1, G2, Gh, GA};
                const T Us[4] = {U_(i, j), V_(i, j), H_(i, j), A_(i, j)};
                T *const Gp[4] = {a.G1, a.G2, a.Gh, a.GA};
#pragma unroll
                for (int f = 0; f < 4; ++f) {
                    T un;
                    if (!STRICT && !BND && a.anchor) {   // anchor form (common.hpp: Rk3Buffers): W out through the G pointers, or W in through Gm
                        if (a.first) {
                            un = Us[f] + a.dtg * Gs[f];
                            Gp[f][o] = Us[f] + a.dtw * Gs[f];
                        } else {
                            un = a.Gm[f][o] + a.dtg * Gs[f];
                        }
                    } else if (a.first) {
                        if constexpr (STRICT) un = Us[f] + a.dt * a.gamma * Gs[f];
                        else un = substep_pinned<T>(Us[f], a.dt, a.gamma, Gs[f]);
                    } else if (!STRICT && a.gm_prev) {
                        un = Us[f] + (a.dt * a.gamma) * Gs[f] + a.zeta * (Us[f] - a.Gm[f][o]);
                    } else {
                        if constexpr (STRICT) un = Us[f] + a.dt * (a.gamma * Gs[f] + a.zeta * a.Gm[f][o]);
                        else un = substep_pinned<T>(Us[f], a.dt, a.gamma, Gs[f], a.zeta, a.Gm[f][o]);
                    }
                    a.Unew[f][o] = un;
                }
            }
        }
    }
}

// rk3_substep!:  U += Δt (γⁿ Gⁿ + ζⁿ G⁻)  for the four prognostic fields in one launch (interior only)
template <typename T>
__global__ void k_rk3_substep(Rk3Args<T> a) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = a.j0 + blockIdx.y;
    if (x >= a.Nx || y >= a.j1) return;
    const long o = (long)y * a.sy + x;
#pragma unroll
    for (int f = 0; f < 4; ++f) {
        T u = a.U[f][o];
        if (a.first) {
            if constexpr (STRICT) u += a.dt * a.gamma * a.Gn[f][o];
            else u += (a.dt * a.gamma) * a.Gn[f][o];
        } else {
            u += a.dt * (a.gamma * a.Gn[f][o] + a.zeta * a.Gm[f][o]);
        }
        a.U[f][o] = u;
    }
}

#if !SWMHD_STRICT
#include "tendency_march_kernels.inc"
#include "tendency_pk_kernels.inc"
#endif

}  // namespace
}  // namespace swmhd
