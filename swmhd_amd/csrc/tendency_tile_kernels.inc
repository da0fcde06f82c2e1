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
// Included by tendency_fast.hip / tendency_strict.hip with SWMHD_STRICT and LAUNCH_SFX defined.

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
__device__ __forceinline__ unsigned ens_member(EnsTendArgs<T> &a, unsigned ntiles) {
    unsigned m, t;
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

// FORM: 0 conservative, 1 vector invariant.  LOR: 0 none, 1 Jacobian (FORM 1 only), 2 divergence (FORM 0 only).
// BND: at least one direction is Bounded -- reconstructions near walls drop to the boundary schemes (sw_device.inc) and the divergence-
// form Lorentz fluxes take the reference's wall branches (sw_mhd_divergence_functions.jl:42-53,66-77,90-101,114-125).  With
// BND = false every order is the compile-time constant 5 and the code is the periodic kernel.
// ENS: ensemble launch (EnsTendArgs) -- the workgroup's member offsets every field pointer; otherwise the body is the same.
template <typename T, int FORM, int LOR, int TX, int TYB, int RY, bool BND = false, bool ENS = false>
__global__ __launch_bounds__(TX *TYB) void k_tendency_tile(TileArgs<T, ENS> a, int ntx, int nty) {
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
    if constexpr (ENS) bid = ens_member<T>(a, (unsigned)(ntx * nty));
    else bid = xcd_remap(blockIdx.x, (unsigned)(ntx * nty));
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
                        else un = Us[f] + (a.dt * a.gamma) * Gs[f];
                    } else if (!STRICT && a.gm_prev) {
                        un = Us[f] + (a.dt * a.gamma) * Gs[f] + a.zeta * (Us[f] - a.Gm[f][o]);
                    } else {
                        un = Us[f] + a.dt * (a.gamma * Gs[f] + a.zeta * a.Gm[f][o]);
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

#define LAUNCH_NAME_(base, sfx) base##sfx
#define LAUNCH_NAME(base, sfx) LAUNCH_NAME_(base, sfx)

constexpr long SW_MARCH_MIN_CELLS = 330000L;

#if !SWMHD_STRICT
// Geometry of the marching tendency kernels.  Vector-invariant kernel: <= 168 VGPRs and 0.19 KB of LDS per lane -> 12 waves per
// CU, i.e. 3 / 6 workgroups of 256 / 128 threads.  Conservative kernel: 2 workgroups of 256 per CU (69 KB LDS).
// Knobs (read once): SWMHD_T_LY rows per segment, SWMHD_T_NT workgroup size (128 or 256), SWMHD_T_FOLD=0 no folded last strip (A/B).
// Folded last strip (fp64 vector-invariant kernel, 256 lanes, last strip <= 122 output columns; tendency_march_kernels.inc): 4096
// columns run 16 full workgroups and half a folded one per segment row instead of 17 -- LY 90 instead of 92 in one round.
// Packed-fp32 kernel (tendency_pk_kernels.inc): vector-invariant model, x read with periodic wrapping, even Nx.  256 lanes = 512
// columns per strip, 504 of them output; 3 workgroups per CU (<= 168 VGPRs, 46 KB LDS).
static bool tendency_uses_packed_fp32(int Nx, int formulation, int wrap) {
    return formulation == 1 && (wrap & 1) && (Nx % 2 == 0) && Nx >= 8;
}
static MarchGeometry packed_fp32_geometry(int Nx, int rows, int leave_room) {
    static int ly_cache = 0;
    static const int cols[1] = {512}, wgs[1] = {3};   // in columns: 2 per lane, 4 halo columns a side -> 504 output columns per strip
    MarchGeometry g = march_geometry(Nx, rows, 4, cols, wgs, 1, 6, leave_room != 0, 0, env_knob("SWMHD_T_LY", ly_cache));
    g.nt = 256;
    return g;
}
static bool tendency_fold_enabled() {
    static const bool on = [] { const char *e = getenv("SWMHD_T_FOLD"); return !e || atoi(e) != 0; }();
    return on;
}
// fold_ok: the launch may fold its last strip (one row range: the slab driver's two-range launches keep full strips)
static MarchGeometry tendency_march_geometry(int Nx, int rows, int formulation, int leave_room, int elem_size, int mode = 7,
                                             bool fold_ok = true) {
    static int ly_cache = 0, nt_cache = 0;
    const int force_ly = env_knob("SWMHD_T_LY", ly_cache), force_nt = env_knob("SWMHD_T_NT", nt_cache);
    if (formulation == 1) {
        // (384-thread workgroups cover 4096 columns with 3 % fewer lanes -- 11 strips instead of 17 -- but measured 37 % SLOWER on
        //  MI355X, 1.75 vs 1.275 ms per step: six waves per barrier leave each SIMD too little to overlap; removed after that measurement)
        static const int nts[2] = {256, 128}, wgs64[2] = {3, 6}, wgs32[2] = {4, 8};   // fp32: <= 128 VGPRs, 4 waves per SIMD
        const int fold_nt = elem_size == 8 && fold_ok && tendency_fold_enabled() ? 256 : 0;
        return march_geometry(Nx, rows, 3, nts, elem_size == 8 ? wgs64 : wgs32, 2, 6, leave_room != 0, force_nt, force_ly, fold_nt);
    }
    // (128-thread workgroups where they waste >= 5 % fewer lanes in the last strip: 1024 columns = 5 strips of 250 or 9 of 122)
    const int w = cons_minwaves(mode, elem_size);                          // per stage variant (tendency_march_kernels.inc)
    const int nts[2] = {256, 128}, wgs[2] = {w, 2 * w};
    return march_geometry(Nx, rows, 3, nts, wgs, 2, 6, leave_room != 0, force_nt, force_ly);
}
// Compiled stage variant (MODE: bits at k_tendency_vi_march) of the marching kernels for a call; sets a.drop_G where a variant that
// stores G serves a stage that must not.
template <typename T> static int march_stage_mode(TendArgs<T> &a, int formulation) {
    int mode = (a.fuse ? 1 : 0) | ((a.fuse && !a.first) ? 2 : 0) | ((a.store_G || !a.fuse) ? 4 : 0) | (a.anchor ? 8 : 0);
    const bool cons64 = formulation == 0 && sizeof(T) == 8;
    // The previous-state operand (gm_prev) lives in the stage-2 variant (coefficient form).  Conservative model: the last RK3 stage
    // (MODE 3) runs on the stage-2 variant (3 workgroups per CU, no scratch) with its G stores dropped by the hardware: 4096^2 step
    // 1.39-1.40 -> 1.36 ms.  (The same substitution bought nothing for the vector-invariant kernel, whose MODE 3 already has its third
    // workgroup: 398-403 vs 403-408 us.)
    if (mode == 3 && (a.gm_prev || (cons64 && cons_minwaves(7, 8) > cons_minwaves(3, 8)))) { mode = 7; a.drop_G = 1; }
    // ... and the first stage without a G store (MODE 1, two workgroups per CU) on the MODE-5 variant, likewise
    if (mode == 1 && cons64 && cons_minwaves(5, 8) > cons_minwaves(1, 8)) { mode = 5; a.drop_G = 1; }
    return mode;
}
template <typename T> using MarchKernel = void (*)(TendArgs<T>, int, int, int);
template <typename T, int MODE> static MarchKernel<T> march_kernel(int formulation, int lorentz, int nt, bool packed) {
    if constexpr (std::is_same<T, float>::value) {
        if (packed) return lorentz == 1 ? k_tendency_vi_march_pk<1, 256, MODE> : k_tendency_vi_march_pk<0, 256, MODE>;
    }
    if (formulation == 1) {
        if (nt == 128) return lorentz == 1 ? k_tendency_vi_march<T, 1, 128, MODE> : k_tendency_vi_march<T, 0, 128, MODE>;
        return lorentz == 1 ? k_tendency_vi_march<T, 1, 256, MODE> : k_tendency_vi_march<T, 0, 256, MODE>;
    }
    if (nt == 128) return lorentz == 2 ? k_tendency_cons_march<T, 2, 128, MODE> : k_tendency_cons_march<T, 0, 128, MODE>;
    return lorentz == 2 ? k_tendency_cons_march<T, 2, 256, MODE> : k_tendency_cons_march<T, 0, 256, MODE>;
}
template <typename T> static MarchKernel<T> march_kernel(int mode, int formulation, int lorentz, int nt, bool packed) {
    switch (mode) {
    case 1: return march_kernel<T, 1>(formulation, lorentz, nt, packed);
    case 3: return march_kernel<T, 3>(formulation, lorentz, nt, packed);
    case 4: return march_kernel<T, 4>(formulation, lorentz, nt, packed);
    case 5: return march_kernel<T, 5>(formulation, lorentz, nt, packed);
    case 7: return march_kernel<T, 7>(formulation, lorentz, nt, packed);
    case 9: return march_kernel<T, 9>(formulation, lorentz, nt, packed);
    case 11: return march_kernel<T, 11>(formulation, lorentz, nt, packed);
    default: return nullptr;
    }
}
#endif

// LDS-tiled kernel, 64 x 4 threads, RY output rows per thread; ENS: every tile of a.members members (grid folded or 2-D, see EnsTendArgs)
template <typename T, int RY, bool BND = false, bool ENS = false>
static hipError_t launch_tile(const TileArgs<T, ENS> &a, int formulation, int lorentz, int ntx, int nty, hipStream_t s) {
    constexpr int TX = 64, TYB = 4;
    dim3 grid(ntx * nty);
    const dim3 block(TX, TYB);
    if constexpr (ENS) grid = a.fold ? dim3(ntx * nty * a.members) : dim3(ntx * nty, a.members);
    if (formulation == 1 && lorentz == 1) hipLaunchKernelGGL((k_tendency_tile<T, 1, 1, TX, TYB, RY, BND, ENS>), grid, block, 0, s, a, ntx, nty);
    else if (formulation == 1 && lorentz == 0) hipLaunchKernelGGL((k_tendency_tile<T, 1, 0, TX, TYB, RY, BND, ENS>), grid, block, 0, s, a, ntx, nty);
    else if (formulation == 0 && lorentz == 2) hipLaunchKernelGGL((k_tendency_tile<T, 0, 2, TX, TYB, RY, BND, ENS>), grid, block, 0, s, a, ntx, nty);
    else if (formulation == 0 && lorentz == 0) hipLaunchKernelGGL((k_tendency_tile<T, 0, 0, TX, TYB, RY, BND, ENS>), grid, block, 0, s, a, ntx, nty);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

template <typename T>
hipError_t LAUNCH_NAME(launch_tendency_, LAUNCH_SFX)(const TendArgs<T> &a, int formulation, int lorentz, hipStream_t s) {
    constexpr int TX = 64, TYB = 4, RY = 2;
    const bool two = a.j1b > a.j0b;   // a second row range: one launch of the LDS-tiled kernel serves both; other kernels take two launches
    const int rows_b = two ? a.j1b - a.j0b : 0;
    [[maybe_unused]] const int rows = a.j1 - a.j0 + rows_b;
    auto one_by_one = [&]() {
        TendArgs<T> b = a;
        b.j0b = b.j1b = 0;
        hipError_t e = LAUNCH_NAME(launch_tendency_, LAUNCH_SFX)<T>(b, formulation, lorentz, s);
        if (e != hipSuccess) return e;
        b.j0 = a.j0b; b.j1 = a.j1b;
        return LAUNCH_NAME(launch_tendency_, LAUNCH_SFX)<T>(b, formulation, lorentz, s);
    };
    if (two && a.j1 <= a.j0) return one_by_one();
    int ntx = (a.Nx + TX - 1) / TX, nty = (a.j1 - a.j0 + TYB * RY - 1) / (TYB * RY) + (rows_b + TYB * RY - 1) / (TYB * RY);
    if (ntx <= 0 || nty <= 0) return hipSuccess;
    if (a.edge_cols) {   // first and last tile column; the last two where the last one is narrower than 8 columns
        const int ne = (a.Nx % TX == 0 || a.Nx % TX >= 8) ? 2 : 3;
        ntx = ntx < ne ? ntx : ne;
    }
#if !SWMHD_STRICT
    // Kernel choice: the row-marching kernels overtake the tile kernel between 512^2 and 640^2 cells for both formulations (tools/crossover.py:
    // 640^2 82 vs 111 us/step, 1024^2 119 vs 184, 1280^2 161 vs 276; at 512^2 the tile kernel with its fused halo fill wins 60 : 80); small
    // grids and the 3-row boundary strips of the overlapped multi-GPU step take the tile kernel.  kernel_variant 1 / 2 force
    // tile / marching.  Segments may be as short as 6 rows (as many warm-up rows as output rows): on mid-size grids filling the
    // chip matters more than the warm-up overhead (1024^2: 42 us/stage at LY = 7, 54 at 16).
    // (the marching kernels address memory with 32-bit byte offsets: fields of 4 GiB or more stay on the tile kernel)
    const bool fits32 = (long)(a.Ny + 2 * a.Hy) * a.sy * (long)sizeof(T) < (1L << 32) - 64;
    const bool bnd = a.topo_x == 1 || a.topo_y != 0;   // Bounded: LDS-tiled kernel only
    const bool march = !bnd && fits32 && (a.kernel_variant == 2 || (a.kernel_variant == 0 && (long)a.Nx * rows >= SW_MARCH_MIN_CELLS));
    // Large Bounded grids: a cell further than a few cells from a wall has exactly the periodic formulas (every reconstruction at full
    // order, no wall branch of the Lorentz fluxes).  So the row-marching kernel computes ALL rows as if the grid were periodic, reading
    // the boundary-condition halos from memory, and the LDS-tiled Bounded kernel then overwrites a frame: 8 rows along each y wall and
    // the outermost 64-column tile column along each x wall (fused substep included: both launches compute from the same old state).
    // 4096^2 (Bounded, Bounded), RK3 step incl. the boundary-condition fills: 3.12 -> 1.49 ms (vector-invariant), 4.34 -> 1.67
    // (conservative); periodic 1.31 / 1.36 in the same call (tools/time_bounded.py).
    if (bnd && !two && !a.edge_cols && fits32 && a.kernel_variant == 0 && (long)a.Nx * rows >= SW_MARCH_MIN_CELLS && a.Nx >= 4 * TX &&
        a.Ny >= 48) {
        constexpr int FW = 8;
        TendArgs<T> p = a;
        p.topo_x = p.topo_y = 0;
        hipError_t e = LAUNCH_NAME(launch_tendency_, LAUNCH_SFX)<T>(p, formulation, lorentz, s);
        if (e != hipSuccess) return e;
        TendArgs<T> f = a;
        f.kernel_variant = 1;
        if (a.topo_y != 0) {   // a frame along each actual y wall (a y-slab's cut side has none: TOPO_OPEN_*)
            const int a0 = a.j0, a1 = a.j1 < FW ? a.j1 : FW, b0 = a.j0 > a.Ny - FW ? a.j0 : a.Ny - FW, b1 = a.j1;
            f.j0 = a0; f.j1 = a1 > a0 ? a1 : a0; f.j0b = b0; f.j1b = b1 > b0 ? b1 : b0;
            if (a.topo_y & TOPO_OPEN_SOUTH) f.j1 = f.j0;
            if (a.topo_y & TOPO_OPEN_NORTH) f.j1b = f.j0b;
            if (f.j1 <= f.j0 && f.j1b > f.j0b) { f.j0 = f.j0b; f.j1 = f.j1b; f.j0b = f.j1b = 0; }
            if (f.j1 > f.j0 || f.j1b > f.j0b) {
                e = LAUNCH_NAME(launch_tendency_, LAUNCH_SFX)<T>(f, formulation, lorentz, s);
                if (e != hipSuccess) return e;
            }
        }
        if (a.topo_x == 1) {
            f.j0 = a.j0; f.j1 = a.j1; f.j0b = f.j1b = 0; f.edge_cols = 1;
            e = LAUNCH_NAME(launch_tendency_, LAUNCH_SFX)<T>(f, formulation, lorentz, s);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
    // (two ranges on a marching kernel: the segments of the second range follow those of the first, same LY)
    auto two_range_segments = [&](int LY) { return (a.j1 - a.j0 + LY - 1) / LY + (rows_b + LY - 1) / LY; };
    // (one 9-12-row segment per zone instead of two 6-row ones -- a single round of workgroups in the slots the interior launch leaves
    //  free -- measured slower: 4096 x 512 ring-of-one step +22 % over plain instead of +11 %)
    if (march) {
        TendArgs<T> ax = a;
        const int mode = march_stage_mode(ax, formulation);
        const bool packed = sizeof(T) == 4 && tendency_uses_packed_fp32(a.Nx, formulation, a.wrap);   // two columns per lane, packed arithmetic
        // (a folded workgroup's rows without an output store one row beyond the parent: that offset must fit 32 bits too)
        const bool fold_ok = !two && (long)(a.Ny + 2 * a.Hy + 1) * a.sy * (long)sizeof(T) < (1L << 32) - 64;
        MarchGeometry mg = packed ? packed_fp32_geometry(a.Nx, rows, a.leave_room)
                                  : tendency_march_geometry(a.Nx, rows, formulation, a.leave_room, (int)sizeof(T), mode, fold_ok);
        if (two) mg.nseg = two_range_segments(mg.LY);
        ax.fold_last = mg.fold;
        const MarchKernel<T> k = march_kernel<T>(mode, formulation, lorentz, mg.nt, packed);
        if (!k) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k, dim3(mg.blocks()), dim3(mg.nt), 0, s, ax, mg.nstrips, mg.nseg, mg.LY);
        return hipGetLastError();
    }
#endif
#if !SWMHD_STRICT
    // Small grids (the reference's own 64^2 .. 128^2, SWMHD_example.jl:11, up to where the marching kernels take over) and thin
    // strips: there are at most a few tiles per CU, so the launch lasts about as long as ONE tile takes; one output row per lane
    // (64 x 4 tiles) instead of two halves the dependent arithmetic of that tile (64^2 .. 256^2: 41 -> 27 us per RK3 step,
    // 512^2: 60 -> 52).  Larger grids forced onto the tile kernel keep 64 x 8 tiles (less halo per cell).
    if (!(a.topo_x == 1 || a.topo_y != 0) && (long)a.Nx * rows < SW_MARCH_MIN_CELLS) {
        constexpr int RY1 = 1;
        const int nty1 = (a.j1 - a.j0 + TYB * RY1 - 1) / (TYB * RY1) + (rows_b + TYB * RY1 - 1) / (TYB * RY1);
        return launch_tile<T, RY1>(a, formulation, lorentz, ntx, nty1, s);
    }
#endif
    if (a.topo_x == 1 || a.topo_y != 0) return launch_tile<T, RY, true>(a, formulation, lorentz, ntx, nty, s);
    return launch_tile<T, RY>(a, formulation, lorentz, ntx, nty, s);
}

// Ensemble stage: the LDS-tiled kernel over every tile of every member (periodic members, one row range).  Tile height as a single
// model of the member's size would take it: 64 x 4 tiles (RY = 1) below SW_MARCH_MIN_CELLS cells per member in fast builds -- the
// same compiled body as that model's launch, so a member's results are bitwise those of the single model -- and 64 x 8 otherwise
// (strict builds, and members the single model would march over).  Members are folded into blockIdx.x by default.  Both choices were
// measured (tools/time_ensemble.py, profiles/ensemble/).  Knobs (read once; measurement only): SWMHD_ENS_RY = 1 | 2 forces the tile
// height, SWMHD_ENS_MAP = 1 folds the member into blockIdx.x, 2 makes it blockIdx.y.
// Bounded members (a.topo_x or a.topo_y = 1) always take the wall kernel with 64 x 8 tiles, the tile a single Bounded model takes
// below SW_MARCH_MIN_CELLS; larger members run it where a single model takes the marching kernel plus the wall frame.  SWMHD_ENS_RY does
// not apply to them.  Strict members are bitwise single models.  Fast members are not: with reassociation the compiler groups the
// uniform factors of the fused substep differently in this instantiation (an ulp in a few cells per stage), within the fast tolerances.
template <typename T>
hipError_t LAUNCH_NAME(launch_tendency_ensemble_, LAUNCH_SFX)(const EnsTendArgs<T> &a, int formulation, int lorentz, hipStream_t s) {
    constexpr int TX = 64, TYB = 4;
    static int ry_cache = 0, map_cache = 0;
    const int rows = a.j1 - a.j0;
    if (rows <= 0 || a.members <= 0) return hipSuccess;
    const bool bnd = a.topo_x == 1 || a.topo_y == 1;
    const int force_ry = bnd ? 0 : env_knob("SWMHD_ENS_RY", ry_cache), map = env_knob("SWMHD_ENS_MAP", map_cache);
    const int ry = bnd ? 2 : (force_ry == 1 || force_ry == 2 ? force_ry : ((!STRICT && (long)a.Nx * rows < SW_MARCH_MIN_CELLS) ? 1 : 2));
    const int ntx = (a.Nx + TX - 1) / TX, nty = (rows + TYB * ry - 1) / (TYB * ry);
    const long blocks = (long)ntx * nty * a.members;
    if (blocks >= (1L << 31) || (map == 2 && a.members > 65535)) return hipErrorInvalidConfiguration;
    EnsTendArgs<T> e = a;
    e.fold = map == 2 ? 0 : 1;
    if (bnd) return launch_tile<T, 2, true, true>(e, formulation, lorentz, ntx, nty, s);
    return ry == 1 ? launch_tile<T, 1, false, true>(e, formulation, lorentz, ntx, nty, s)
                   : launch_tile<T, 2, false, true>(e, formulation, lorentz, ntx, nty, s);
}

template <typename T>
hipError_t LAUNCH_NAME(launch_rk3_substep_, LAUNCH_SFX)(const Rk3Args<T> &a, hipStream_t s) {
    if (a.j1 <= a.j0) return hipSuccess;
    hipLaunchKernelGGL((k_rk3_substep<T>), dim3((a.Nx + 255) / 256, a.j1 - a.j0), dim3(256), 0, s, a);
    return hipGetLastError();
}

#if !SWMHD_STRICT
int tendency_launch_geometry(int Nx, int rows, int formulation, int elem_size, int kernel_variant, int leave_room, int wrap, int out[8]) {
    const bool march = (kernel_variant == 2 || (kernel_variant == 0 && (long)Nx * rows >= SW_MARCH_MIN_CELLS));
    if (march && elem_size == 4 && tendency_uses_packed_fp32(Nx, formulation, wrap)) {   // kind 3: packed fp32, two columns per lane
        const MarchGeometry mg = packed_fp32_geometry(Nx, rows, leave_room);
        out[0] = 3; out[1] = mg.nt; out[2] = mg.nstrips; out[3] = mg.nseg; out[4] = mg.LY; out[5] = mg.wg_per_cu; out[6] = 2;
    } else if (march) {
        const MarchGeometry mg = tendency_march_geometry(Nx, rows, formulation, leave_room, elem_size);
        out[0] = 2; out[1] = mg.nt; out[2] = mg.nstrips; out[3] = mg.nseg; out[4] = mg.LY; out[5] = mg.wg_per_cu; out[6] = 3;
    } else {
        const int ry = (kernel_variant == 1 || (long)Nx * rows >= SW_MARCH_MIN_CELLS) ? 2 : 1;
        out[0] = 1; out[1] = 256; out[2] = (Nx + 63) / 64; out[3] = (rows + 4 * ry - 1) / (4 * ry); out[4] = 4 * ry; out[5] = 0; out[6] = 3;
    }
    out[7] = device_cu_count();
    return 0;
}
#endif

template hipError_t LAUNCH_NAME(launch_tendency_, LAUNCH_SFX)<double>(const TendArgs<double> &, int, int, hipStream_t);
template hipError_t LAUNCH_NAME(launch_tendency_, LAUNCH_SFX)<float>(const TendArgs<float> &, int, int, hipStream_t);
template hipError_t LAUNCH_NAME(launch_tendency_ensemble_, LAUNCH_SFX)<double>(const EnsTendArgs<double> &, int, int, hipStream_t);
template hipError_t LAUNCH_NAME(launch_tendency_ensemble_, LAUNCH_SFX)<float>(const EnsTendArgs<float> &, int, int, hipStream_t);
template hipError_t LAUNCH_NAME(launch_rk3_substep_, LAUNCH_SFX)<double>(const Rk3Args<double> &, hipStream_t);
template hipError_t LAUNCH_NAME(launch_rk3_substep_, LAUNCH_SFX)<float>(const Rk3Args<float> &, hipStream_t);

}  // namespace swmhd
