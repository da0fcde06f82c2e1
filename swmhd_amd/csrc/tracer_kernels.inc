// Passive tracers: ONE launch advances all K extra centre fields c_k through one RK3 stage,
//     G_k = -(1/Az)(dx(flux_x(U, c_k)) + dy(flux_y(V, c_k))) + c_k div(U),     cnew_k = c_k + dt (gamma G_k + zeta Gm_k),
// the equation of A without its coupling back into the flow (k_tendency_tile's GA, both formulations, Bounded orders included).
// The advecting state (q1, q2, h) is the one the stage STARTS from; it is loaded once per tile and what every tracer shares is
// formed once: the face velocities, the conservative form's face depths (fast builds: their reciprocals) and, per thread, the
// divergence of its cells.  Then, for each tracer: tile + 3-cell halo into LDS, every face flux of the tile ONCE into LDS (the tile
// kernel evaluates a face at i and again at i + 1: the same expression of the same inputs, so strict results are its bits), then the
// flux difference, c div U and the RK3 update per cell.  Three barriers per tracer: after the tile is loaded, after the fluxes are
// written, and after the last read of the tile (the cell's own c in the update) before the next tracer's tile overwrites it.
//
// The same body serves periodic ensembles (swmhd_ensemble_tracers_rk3[_params]): the ENS / PAR instantiations walk the members.
//
// Kernels and launchers; included by tracer_fast.hip / tracer_strict.hip with SWMHD_STRICT and LAUNCH_SFX defined.

#ifndef SWMHD_STRICT
#error "include with SWMHD_STRICT defined"
#endif

namespace swmhd {
namespace {

constexpr bool STRICT = (SWMHD_STRICT != 0);

#include "tile_common.inc"
#include "lorentz_device.inc"
#include "sw_device.inc"

// FORM: 0 conservative, 1 vector invariant.  BND: at least one direction is Bounded (wall orders of the reconstructions).
// 64 x TYB threads; a thread owns column threadIdx.x of rows threadIdx.y * RY .. + RY - 1 of a TX x (TYB RY) tile.
// ENS: ensemble launch (EnsTracerArgs) -- blockIdx.x runs over the tiles of all members (XCD-remapped over all of them, so a member's
// tiles share an XCD, as in k_tendency_tile's folded mapping) and the workgroup's member offset `mo` enters every address; otherwise
// the body is the same.  PAR (with ENS): the member also brings its own dt (EnsParTracerArgs); the body is the same again.
template <typename T, int FORM, bool BND, int TX, int TYB, int RY, bool ENS = false, bool PAR = false>
__global__ __launch_bounds__(TX *TYB) void k_tracers_tile(TracerTileArgs<T, ENS, PAR> a, int ntx, int nty) {
    static_assert(ENS || !PAR, "per-member parameters need an ensemble launch");
    static_assert(!ENS || !BND, "ensemble members are periodic");
    constexpr int TY = TYB * RY, NT = TX * TYB;
    constexpr int W = TX + 6, HH = TY + 6;
    constexpr bool CONS = FORM == 0;
    __shared__ T sC[HH][W];             // tracer k with its 3-cell halo; before the tracer loop: h on tile + 1 (conservative)
    __shared__ T sU[TY][TX + 1];        // u | uh at the x-faces 0 .. TX of the tile's rows
    __shared__ T sV[TY + 1][TX];        // v | vh at the y-faces 0 .. TY of the tile's columns
    __shared__ T sHx[CONS ? TY : 1][CONS ? TX + 1 : 1];       // conservative: h at the x-faces (fast: its reciprocal)
    __shared__ T sHy[CONS ? TY + 1 : 1][CONS ? TX : 1];       //               h at the y-faces (fast: its reciprocal)
    __shared__ T sFx[TY][TX + 1];       // flux of tracer k through the x-faces
    __shared__ T sFy[TY + 1][TX];       //                  through the y-faces
    static_assert(!CONS || (TY + 2) * (TX + 2) <= HH * W, "h on tile + 1 is staged in the tracer tile");

    unsigned bid;
    long mo = 0;                        // element offset of this workgroup's member in every parent
    T dt = a.dt, dtg = a.dtg, dtw = a.dtw;
    if constexpr (ENS) {
        const unsigned ntiles = (unsigned)(ntx * nty);
        const unsigned L = xcd_remap(blockIdx.x, ntiles * (unsigned)a.members), m = L / ntiles;
        bid = L - m * ntiles;
        mo = (long)m * a.stride_m;
        if constexpr (PAR) {            // m comes from blockIdx alone: a scalar load; the products as the host forms them for one grid
            dt = a.params[(long)ENS_NPARAMS * m + 2];
            dtg = dt * a.gamma;
            dtw = dt * a.zeta;
        }
    } else bid = xcd_remap(blockIdx.x, (unsigned)(ntx * nty));
    const int tyi = (int)(bid / ntx), txi = (int)(bid % ntx);
    const int x0 = txi * TX, y0 = a.j0 + tyi * TY;
    const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * TX + tx;
    const int xlo = -a.Hx, xhi = a.Nx + a.Hx - 1, ylo = -a.Hy, yhi = a.Ny + a.Hy - 1;
    const Geo<T> g{a.dx, a.dy, a.rdx, a.rdy};

    load_tile<T, TX + 1, TY, NT>(sU, a.q1 + mo, a.sy, x0, y0, xlo, xhi, ylo, yhi, tid, a.Nx, a.Ny, a.wrap);
    load_tile<T, TX, TY + 1, NT>(sV, a.q2 + mo, a.sy, x0, y0, xlo, xhi, ylo, yhi, tid, a.Nx, a.Ny, a.wrap);
    if constexpr (CONS) {
        auto &sH = *reinterpret_cast<T(*)[TY + 2][TX + 2]>(&sC[0][0]);
        load_tile<T, TX + 2, TY + 2, NT>(sH, a.h + mo, a.sy, x0 - 1, y0 - 1, xlo, xhi, ylo, yhi, tid, a.Nx, a.Ny, a.wrap);
        __syncthreads();
        auto H_ = [&](int ii, int jj) -> T { return sH[jj + 1][ii + 1]; };
        // he = hw of the next cell, hn = hs of the next row: one value per face
        for (int e = tid; e < TY * (TX + 1); e += NT) {
            const int r = e / (TX + 1), c = e - r * (TX + 1);
            const T hf = half_sum<T>(H_(c - 1, r), H_(c, r));
            sHx[r][c] = STRICT ? hf : recip<T>(hf);
        }
        for (int e = tid; e < (TY + 1) * TX; e += NT) {
            const int r = e / TX, c = e - r * TX;
            const T hf = half_sum<T>(H_(c, r - 1), H_(c, r));
            sHy[r][c] = STRICT ? hf : recip<T>(hf);
        }
    }
    __syncthreads();   // (conservative: also the last read of h before tracer 0 takes its place)

    // x / h_face as the tile kernel forms it: x / y (strict), x * recip(y) (fast; the reciprocal is the stored one)
    auto over_hx = [&](T x, int ii, int jj) -> T { if constexpr (STRICT) return x / sHx[jj][ii]; else return x * sHx[jj][ii]; };
    auto over_hy = [&](T x, int ii, int jj) -> T { if constexpr (STRICT) return x / sHy[jj][ii]; else return x * sHy[jj][ii]; };
    // div U of this thread's cells (the factor of c in the tendency)
    T divU[RY];
#pragma unroll
    for (int r = 0; r < RY; ++r) {
        const int j = ty * RY + r;
        if constexpr (CONS) {
            const T ue = over_hx(sU[j][tx + 1], tx + 1, j), uw = over_hx(sU[j][tx], tx, j);
            const T vn = over_hy(sV[j + 1][tx], tx, j + 1), vs_ = over_hy(sV[j][tx], tx, j);
            divU[r] = T(1) / (g.dx * g.dy) * ((g.dy * ue - g.dy * uw) + (g.dx * vn - g.dx * vs_));
        } else if constexpr (STRICT) {
            divU[r] = T(1) / (g.dx * g.dy) * ((g.dy * sU[j][tx + 1] - g.dy * sU[j][tx]) + (g.dx * sV[j + 1][tx] - g.dx * sV[j][tx]));
        } else {
            divU[r] = (sU[j][tx + 1] - sU[j][tx]) * g.rdx + (sV[j + 1][tx] - sV[j][tx]) * g.rdy;
        }
    }

    // orders of the interpolant of tile-local index (ii | jj): its 1-based index is x0 + ii + 1 | y0 + jj + 1
    const bool bx = BND && a.topo_x == 1, by = BND && a.topo_y == 1;
    auto oLx = [&](int ii) -> int { return BND ? left_order(bx, x0 + ii + 1, a.Nx) : 5; };
    auto oRx = [&](int ii) -> int { return BND ? right_order(bx, x0 + ii + 1, a.Nx) : 5; };
    auto oLy = [&](int jj) -> int { return BND ? left_order(by, y0 + jj + 1, a.Ny) : 5; };
    auto oRy = [&](int jj) -> int { return BND ? right_order(by, y0 + jj + 1, a.Ny) : 5; };
    // advective_tracer_flux_x/y(U, c) = A_face * upwind(U[i,j], cL, cR), over the face depth in the conservative form
    auto flux_x = [&](int ii, int jj) -> T {
        T q[6];
#pragma unroll
        for (int m = 0; m < 6; ++m) q[m] = sC[jj + 3][ii + m];          // c(ii - 3 .. ii + 2, jj)
        const T f = g.dy * upwind_recon<T>(sU[jj][ii], q, oLx(ii), oRx(ii));
        if constexpr (CONS) return over_hx(f, ii, jj); else return f;
    };
    auto flux_y = [&](int ii, int jj) -> T {
        T q[6];
#pragma unroll
        for (int m = 0; m < 6; ++m) q[m] = sC[jj + m][ii + 3];          // c(ii, jj - 3 .. jj + 2)
        const T f = g.dx * upwind_recon<T>(sV[jj][ii], q, oLy(jj), oRy(jj));
        if constexpr (CONS) return over_hy(f, ii, jj); else return f;
    };
    const T rAz = STRICT ? T(0) : g.rdx * g.rdy;
    const int gxi = x0 + tx;

#pragma unroll 1
    for (int k = 0; k < a.K; ++k) {
        load_tile<T, W, HH, NT>(sC, a.c[k] + mo, a.sy, x0 - 3, y0 - 3, xlo, xhi, ylo, yhi, tid, a.Nx, a.Ny, a.wrap);
        __syncthreads();
        // every face of the tile once: the thread's own west and south faces, then column TX (wave 0) and row TY (the last wave)
#pragma unroll 1
        for (int r = 0; r < RY; ++r) {
            const int j = ty * RY + r;
            sFx[j][tx] = flux_x(tx, j);
            sFy[j][tx] = flux_y(tx, j);
        }
        if (ty == 0 && tx < TY) sFx[tx][TX] = flux_x(TX, tx);
        if (ty == TYB - 1) sFy[TY][tx] = flux_y(tx, TY);
        __syncthreads();
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            const int j = ty * RY + r, gyj = y0 + j;
            const T c = sC[j + 3][tx + 3];
            const T fxe = sFx[j][tx + 1], fxw = sFx[j][tx], fyn = sFy[j + 1][tx], fys = sFy[j][tx];
            T G;
            if constexpr (STRICT || CONS) {
                const T div_Uc = T(1) / (g.dx * g.dy) * ((fxe - fxw) + (fyn - fys));
                G = -div_Uc + c * divU[r];
            } else {
                G = -rAz * ((fxe - fxw) + (fyn - fys)) + c * divU[r];
            }
            if (gxi < a.Nx && gyj < a.j1) {
                const long o = mo + (long)gyj * a.sy + gxi;
                if (a.store_G) a.Gn[k][o] = G;
                if (a.fuse) {
                    T un;
                    if (!STRICT && !BND && a.anchor) {   // anchor form (common.hpp: Rk3Buffers): W out through Gn, or W in through Gm
                        if (a.first) {
                            un = c + dtg * G;
                            a.Gn[k][o] = c + dtw * G;
                        } else {
                            un = a.Gm[k][o] + dtg * G;
                        }
                    } else if (a.first) {
                        if constexpr (STRICT) un = c + dt * a.gamma * G;
                        else un = c + (dt * a.gamma) * G;
                    } else {
                        un = c + dt * (a.gamma * G + a.zeta * a.Gm[k][o]);
                    }
                    a.cnew[k][o] = un;
                }
            }
        }
        __syncthreads();   // the last read of tracer k's tile is behind every thread before tracer k + 1 is loaded over it
    }
}

}  // namespace

#define LAUNCH_NAME_(base, sfx) base##sfx
#define LAUNCH_NAME(base, sfx) LAUNCH_NAME_(base, sfx)


// The stage kernel over the tiles of tracer_tiles (launch_plan.hpp): one grid, or (ENS) every tile of every member in one launch, the
// member folded into blockIdx.x.  Ensemble members are periodic.
template <typename T, bool ENS = false, bool PAR = false>
static hipError_t launch_tracer_tiles(const TracerTileArgs<T, ENS, PAR> &a, int formulation, hipStream_t s) {
    constexpr int TX = TRACER_TILE_X, TYB = 4, RY = TRACER_TILE_Y / TYB;
    int members = 1;
    if constexpr (ENS) members = a.members;
    const TracerTiles t = tracer_tiles(a.Nx, a.j1 - a.j0, a.K, members);
    if (t.none) return hipSuccess;
    const bool bnd = is_bounded(a.topo_x, a.topo_y);
    if (ENS && bnd) return hipErrorInvalidValue;
    if (t.too_many) return hipErrorInvalidConfiguration;
    void (*k)(TracerTileArgs<T, ENS, PAR>, int, int) = nullptr;
    if (formulation == 1) {
        if constexpr (!ENS) { if (bnd) k = k_tracers_tile<T, 1, true, TX, TYB, RY>; }
        if (!k) k = k_tracers_tile<T, 1, false, TX, TYB, RY, ENS, PAR>;
    } else if (formulation == 0) {
        if constexpr (!ENS) { if (bnd) k = k_tracers_tile<T, 0, true, TX, TYB, RY>; }
        if (!k) k = k_tracers_tile<T, 0, false, TX, TYB, RY, ENS, PAR>;
    } else return hipErrorInvalidValue;
    hipLaunchKernelGGL(k, dim3((unsigned)t.blocks), dim3(TX, TYB), 0, s, a, t.ntx, t.nty);
    return hipGetLastError();
}

template <typename T>
hipError_t LAUNCH_NAME(launch_tracers_, LAUNCH_SFX)(const TracerArgs<T> &a, int formulation, hipStream_t s) {
    return launch_tracer_tiles<T>(a, formulation, s);
}
template hipError_t LAUNCH_NAME(launch_tracers_, LAUNCH_SFX)<double>(const TracerArgs<double> &, int, hipStream_t);
template hipError_t LAUNCH_NAME(launch_tracers_, LAUNCH_SFX)<float>(const TracerArgs<float> &, int, hipStream_t);

template <typename T>
hipError_t LAUNCH_NAME(launch_tracers_ensemble_, LAUNCH_SFX)(const EnsTracerArgs<T> &a, int formulation, hipStream_t s) {
    return launch_tracer_tiles<T, true>(a, formulation, s);
}
template <typename T>
hipError_t LAUNCH_NAME(launch_tracers_ensemble_params_, LAUNCH_SFX)(const EnsParTracerArgs<T> &a, int formulation, hipStream_t s) {
    if (!a.params) return hipErrorInvalidValue;
    return launch_tracer_tiles<T, true, true>(a, formulation, s);
}
template hipError_t LAUNCH_NAME(launch_tracers_ensemble_, LAUNCH_SFX)<double>(const EnsTracerArgs<double> &, int, hipStream_t);
template hipError_t LAUNCH_NAME(launch_tracers_ensemble_, LAUNCH_SFX)<float>(const EnsTracerArgs<float> &, int, hipStream_t);
template hipError_t LAUNCH_NAME(launch_tracers_ensemble_params_, LAUNCH_SFX)<double>(const EnsParTracerArgs<double> &, int, hipStream_t);
template hipError_t LAUNCH_NAME(launch_tracers_ensemble_params_, LAUNCH_SFX)<float>(const EnsParTracerArgs<float> &, int, hipStream_t);

}  // namespace swmhd
