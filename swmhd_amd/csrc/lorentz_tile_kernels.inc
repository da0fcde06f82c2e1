// Lorentz-force operator kernels, LDS-tiled form.  Included by lorentz_fast.hip and lorentz_strict.hip with
// SWMHD_STRICT = 0 / 1; kernels only (what is launched: plan_lorentz, launch_plan.hpp; the launchers: lorentz_launch.inc).
//
//   k_lorentz_jacobian    lorentz_force_func_x/y   jacobian_formulation/sw_mhd_jacobian_functions.jl:1-26
//   k_lorentz_divergence  div_lorentz_x/y          divergence_formulation/sw_mhd_divergence_functions.jl:1-170
//
// The reference evaluates these by deep function composition with no sharing (~300 array loads per output).  Here a
// workgroup stages one 2-D tile of A and h (with the stencil's halo) into LDS with x-coalesced loads, computes every
// shared intermediate exactly once per tile (centre B for the Jacobian form; face hBx,Bx,hBy,By for the divergence
// form) into LDS, then each lane walks RY consecutive rows of one column so column-direction values stay in registers.
//
// STRICT build: reference evaluation order, IEEE divides, TU compiled -ffp-contract=off => bit-identical to the oracle.
// FAST build: reciprocal multiplies, merged centred differences, FMA contraction.

#ifndef SWMHD_STRICT
#error "include with SWMHD_STRICT defined"
#endif

namespace swmhd {
namespace {

constexpr bool STRICT = (SWMHD_STRICT != 0);

#include "tile_common.inc"
#include "lorentz_device.inc"

// Jacobian form.  Tile TX x (TYB*RY); A halo 2, h halo 1.
template <typename T, int TX, int TYB, int RY>
__global__ __launch_bounds__(TX *TYB) void k_lorentz_jacobian(OpArgs<T> a, int ntx, int nty) {
    constexpr int TY = TYB * RY, NT = TX * TYB;
    constexpr int AW = TX + 4, AH = TY + 4, BW = TX + 2, BH = TY + 2;
    __shared__ T sA[AH][AW];
    __shared__ T sh[BH][BW];
    __shared__ T sBx[BH][BW];
    __shared__ T sBy[BH][BW];

    const unsigned bid = xcd_remap(blockIdx.x, (unsigned)(ntx * nty));
    const int x0 = (int)(bid % ntx) * TX, y0 = a.j0 + (int)(bid / ntx) * TY;
    const int tid = threadIdx.y * TX + threadIdx.x;
    const int xlo = -a.Hx, xhi = a.Nx + a.Hx - 1, ylo = -a.Hy, yhi = a.Ny + a.Hy - 1;
    const Geo<T> g{a.dx, a.dy, a.rdx, a.rdy};

    load_tile<T, AW, AH, NT>(sA, a.A, a.sy, x0 - 2, y0 - 2, xlo, xhi, ylo, yhi, tid);
    load_tile<T, BW, BH, NT>(sh, a.h, a.sy, x0 - 1, y0 - 1, xlo, xhi, ylo, yhi, tid);
    __syncthreads();

    auto A_ = [&](int ii, int jj) -> T { return sA[jj + 2][ii + 2]; };
    auto H_ = [&](int ii, int jj) -> T { return sh[jj + 1][ii + 1]; };
    auto BX_ = [&](int ii, int jj) -> T { return sBx[jj + 1][ii + 1]; };
    auto BY_ = [&](int ii, int jj) -> T { return sBy[jj + 1][ii + 1]; };

    for (int e = tid; e < BW * BH; e += NT) {   // phase 1: centre B on tile + 1
        int r = e / BW, c = e - r * BW;
        T bx, by;
        jac_centre_B<T>(A_, H_, c - 1, r - 1, g, bx, by);
        sBx[r][c] = bx;
        sBy[r][c] = by;
    }
    __syncthreads();

    const int i = threadIdx.x, gx = x0 + i;
#pragma unroll
    for (int r = 0; r < RY; ++r) {              // phase 2
        const int j = threadIdx.y * RY + r, gy = y0 + j;
        T fx, fy;
        jac_force<T>(A_, H_, BX_, BY_, i, j, g, fx, fy);
        if (gx < a.Nx && gy < a.j1) {
            a.Fx[(long)gy * a.sy + gx] = fx;
            a.Fy[(long)gy * a.sy + gx] = fy;
        }
    }
}

// Divergence form.  Tile TX x (TYB*RY); A and h halo 3; face quantities on the tile + 2.
template <typename T, int TX, int TYB, int RY>
__global__ __launch_bounds__(TX *TYB) void k_lorentz_divergence(OpArgs<T> a, int ntx, int nty) {
    constexpr int TY = TYB * RY, NT = TX * TYB;
    constexpr int AW = TX + 6, AH = TY + 6, FW = TX + 4, FH = TY + 4;
    __shared__ T sA[AH][AW];
    __shared__ T sh[AH][AW];
    __shared__ T sHBx[FH][FW];
    __shared__ T sBx[FH][FW];
    __shared__ T sHBy[FH][FW];
    __shared__ T sBy[FH][FW];

    const unsigned bid = xcd_remap(blockIdx.x, (unsigned)(ntx * nty));
    int txi = (int)(bid % ntx);
    if (a.edge_cols && txi > 0) txi = (a.Nx + TX - 1) / TX - (ntx - txi);   // x-wall frame: tile column 0 and the last one (or two)
    const int x0 = txi * TX, y0 = a.j0 + (int)(bid / ntx) * TY;
    const int tid = threadIdx.y * TX + threadIdx.x;
    const int xlo = -a.Hx, xhi = a.Nx + a.Hx - 1, ylo = -a.Hy, yhi = a.Ny + a.Hy - 1;
    const Geo<T> g{a.dx, a.dy, a.rdx, a.rdy};

    load_tile<T, AW, AH, NT>(sA, a.A, a.sy, x0 - 3, y0 - 3, xlo, xhi, ylo, yhi, tid);
    load_tile<T, AW, AH, NT>(sh, a.h, a.sy, x0 - 3, y0 - 3, xlo, xhi, ylo, yhi, tid);
    __syncthreads();

    auto A_ = [&](int ii, int jj) -> T { return sA[jj + 3][ii + 3]; };
    auto H_ = [&](int ii, int jj) -> T { return sh[jj + 3][ii + 3]; };
    auto HBX_ = [&](int ii, int jj) -> T { return sHBx[jj + 2][ii + 2]; };
    auto BX_ = [&](int ii, int jj) -> T { return sBx[jj + 2][ii + 2]; };
    auto HBY_ = [&](int ii, int jj) -> T { return sHBy[jj + 2][ii + 2]; };
    auto BY_ = [&](int ii, int jj) -> T { return sBy[jj + 2][ii + 2]; };

    for (int e = tid; e < FW * FH; e += NT) {   // phase 1: face quantities on tile + 2
        int r = e / FW, c = e - r * FW;
        T hbx, bx, hby, by;
        div_faces<T>(A_, H_, c - 2, r - 2, g, hbx, bx, hby, by);
        sHBx[r][c] = hbx; sBx[r][c] = bx; sHBy[r][c] = hby; sBy[r][c] = by;
    }
    __syncthreads();

    // phase 2: fluxes + divergence (:162-170); y-direction fluxes are carried up the column.  Julia indices of this lane's
    // cell are (x0+i+1, y0+j+1); the wall codes select the reference's Bounded branches (all 0 on periodic grids).
    const int i = threadIdx.x, gx = x0 + i, jb = threadIdx.y * RY;
    const int bx = a.topo_x == 1, by = a.topo_y == 1;
    const int iJ = gx + 1;
    const int cF1 = wall_code(bx, iJ, 0, a.Nx), cF1m = wall_code(bx, iJ - 1, 0, a.Nx);
    const int cG1 = wall_code(bx, iJ, 1, a.Nx + 1), cG1p = wall_code(bx, iJ + 1, 1, a.Nx + 1);
    const T rAz = T(1) / (a.dx * a.dy);
    T f2 = div_F2<T>(HBY_, BX_, i, jb, g, wall_code(by, y0 + jb + 1, 1, a.Ny + 1));
    T g2 = div_G2<T>(HBY_, BY_, i, jb - 1, g, wall_code(by, y0 + jb, 0, a.Ny));
#pragma unroll
    for (int r = 0; r < RY; ++r) {
        const int j = jb + r, gy = y0 + j, jJ = gy + 1;
        T f2n = div_F2<T>(HBY_, BX_, i, j + 1, g, wall_code(by, jJ + 1, 1, a.Ny + 1));
        T g2n = div_G2<T>(HBY_, BY_, i, j, g, wall_code(by, jJ, 0, a.Ny));
        T fx = rAz * ((div_F1<T>(HBX_, BX_, i, j, g, cF1) - div_F1<T>(HBX_, BX_, i - 1, j, g, cF1m)) + (f2n - f2));
        T fy = rAz * ((div_G1<T>(HBX_, BY_, i + 1, j, g, cG1p) - div_G1<T>(HBX_, BY_, i, j, g, cG1)) + (g2n - g2));
        f2 = f2n; g2 = g2n;
        if (gx < a.Nx && gy < a.j1) {
            a.Fx[(long)gy * a.sy + gx] = fx;
            a.Fy[(long)gy * a.sy + gx] = fy;
        }
    }
}

#if !SWMHD_STRICT
#include "lorentz_march_kernels.inc"
#endif

}  // namespace
}  // namespace swmhd
