// Zonal means: x-averaged profiles of the output fields and of the second moments that drive the mean flow, reduced on the device in
// one launch over the four prognostic parents (swmhd_zonal_means_*, include/swmhd_zonal.h).
//
//   profile[k][j] = (Σ_{i=1..Nx} term_k(i, j)) / Nx
// Per-cell terms: the frame definitions and their placement rule (frame_device.inc), with U V BX BY the frame values:
//   u v h A s B_x B_y   the frame fields themselves (mask bits = SWMHD_OUT_*)
//   uu    @fc  U·U             vv    @cf  V·V             uv    @fc  U · ℑxyᶠᶜ(V)     0.5*(0.5*(V(i−1,j)+V(i,j)) + 0.5*(V(i−1,j+1)+V(i,j+1)))
//   B_xB_x @cf BX·BX           B_yB_y @fc BY·BY           B_xB_y @fc BY · ℑxyᶠᶜ(BX)   same grouping
//   vA    @cf  V · (0.5*(A(i,j−1)+A(i,j)))
// The points averaged are the frame's, i = 1..Nx, on Bounded directions too: the far-wall line of a face field is not part of the mean.
// This object is built without FMA contraction and with IEEE divide / sqrt (Makefile: STRICT), so every term is bitwise a plain numpy
// restatement (tests/zonal_cases.py) and only the summation has a tolerance.
//
// Shape: one wave64 per row, four rows per 256-thread workgroup (launch_plan.hpp: zonal_plan) -- no LDS, no barrier, no atomics.  Lane l
// takes the 4-cell chunks l, l + 64, ... of its row (32 B of an fp64 parent per load where the chunk lies inside the row, single elements
// where it crosses the end: load_row of frame_device.inc, shared with output.hip), adds their terms serially in x order, and a butterfly
// (__shfl_xor, 32 .. 1) adds the 64 lane sums; both operands of a butterfly level are the same pair in both lanes and addition commutes,
// so every lane ends with the same bits and lane 0 stores.  The order is a function of Nx alone (zonal_depth): not of the row range, the
// member count, the strides or the grid.  64-wide members: 256 x 64 rows = 16 384 waves; a 4096-wide row: 16 trips per lane.
// `which` is wave-uniform: what a mask does not ask for is neither loaded nor computed, and rows y ± 1 are read only for s, uv, B_xB_y
// (y + 1) and v (conservative), B_x, vA and their products (y − 1).
// Reach: one cell (x−1, y−1, y+1); with SWMHD_WRAP_X / _Y those neighbours are taken at (x mod Nx, y mod Ny) instead of the halo.
#include "api_args.hpp"
#include "common.hpp"

namespace swmhd {
namespace {

#include "frame_device.inc"   // frame_vel .. frame_xy_mean, frame_west, load_row: shared with output.hip and derived.hip

constexpr int NPROF = 14;
static_assert(ZONAL_VEC == FRAME_VEC, "a trip of a lane is one chunk of the frame");

template <typename T>
struct ZonalArgs {
    const T *q1, *q2, *h, *A;   // interior cell (1,1) of the parents, as OpArgs
    double *out;
    int Nx, Ny, j0, j1;
    long sy, osk;
    double dx, dy;
    int form, which, wrap;      // wrap: bit 0 = x, bit 1 = y
    long row_blocks, stride_m, osm;   // ensembles: member blockIdx.x / row_blocks
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int d = ZONAL_WAVE / 2; d >= 1; d >>= 1) v += __shfl_xor(v, d, ZONAL_WAVE);
    return v;
}

// M: the profiles this instantiation can produce (a.which lies within it); what M excludes is compiled out.  Two are built: every
// profile (all nine row loads and fourteen sums live: 2 waves per SIMD), and ZM_ROW -- u v h A uu vv vA, the mean flow, the mean
// potential and its flux, which never read row y + 1 -- in half the registers (4 waves per SIMD).  Same statements, no contraction:
// a profile has the same bits from either.
constexpr int ZM_ROW = SWMHD_ZM_U | SWMHD_ZM_V | SWMHD_ZM_H | SWMHD_ZM_A | SWMHD_ZM_UU | SWMHD_ZM_VV | SWMHD_ZM_VA;

template <typename T, bool ENS, int M>
__global__ __launch_bounds__(ZONAL_NT, M == ZM_ROW ? 4 : 2) void k_zonal_means(ZonalArgs<T> a) {
    // (the wave index through readfirstlane: the row, its pointers and every branch on the mask are then scalar to the compiler too)
    const int lane = threadIdx.x & (ZONAL_WAVE - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x / ZONAL_WAVE);
    long rb = blockIdx.x;
    double *out = a.out;
    if constexpr (ENS) {
        const long m = rb / a.row_blocks, o = m * a.stride_m;
        rb -= m * a.row_blocks;
        a.q1 += o; a.q2 += o; a.h += o; a.A += o;
        out += m * a.osm;
    }
    const long row = rb * ZONAL_ROWS + wave;
    if (row >= (long)(a.j1 - a.j0)) return;   // (the whole wave)
    const int y = a.j0 + (int)row;
    // (frame_device.inc: frame_rows, written out: through the function this kernel's scalar code is scheduled differently)
    const int ym = (y == 0 && (a.wrap & 2)) ? a.Ny - 1 : y - 1;
    const int yp = (y == a.Ny - 1 && (a.wrap & 2)) ? 0 : y + 1;
    const long r0 = (long)y * a.sy, rm = (long)ym * a.sy, rp = (long)yp * a.sy;

    // which values, and which rows of which parent, this mask needs (wave-uniform)
    const int w = a.which & M;
    const bool cons = a.form == SWMHD_CONSERVATIVE;
    const bool wantS = w & SWMHD_ZM_SPEED, wantUV = w & SWMHD_ZM_UV, wantBB = w & SWMHD_ZM_BXBY, wantVA = w & SWMHD_ZM_VA;
    const bool needU = w & (SWMHD_ZM_U | SWMHD_ZM_SPEED | SWMHD_ZM_UU | SWMHD_ZM_UV);
    const bool needV0 = w & (SWMHD_ZM_V | SWMHD_ZM_SPEED | SWMHD_ZM_VV | SWMHD_ZM_UV | SWMHD_ZM_VA);
    const bool needVp = wantS || wantUV;
    const bool needBX0 = w & (SWMHD_ZM_BX | SWMHD_ZM_BXBX | SWMHD_ZM_BXBY), needBXp = wantBB;
    const bool needBY = w & (SWMHD_ZM_BY | SWMHD_ZM_BYBY | SWMHD_ZM_BXBY);
    const bool ld_h0 = (w & SWMHD_ZM_H) || needBX0 || needBXp || needBY || (cons && (needU || needV0 || needVp));
    const bool ld_hm = needBX0 || (cons && needV0), ld_hp = needBXp || (cons && needVp);
    const bool ld_A0 = (w & SWMHD_ZM_A) || needBX0 || needBXp || needBY || wantVA;
    const bool ld_Am = needBX0 || wantVA, ld_Ap = needBXp;

    constexpr int R = ZONAL_VEC + 1;
    double acc[NPROF];
#pragma unroll
    for (int p = 0; p < NPROF; ++p) acc[p] = 0.0;

    // (the cells left, Nx - x0, decide everything: x0 + 4 or x0 + 256 may pass 2^31 where Nx is near it)
    for (int x0 = lane * ZONAL_VEC; x0 < a.Nx;) {
        const int nvalid = a.Nx - x0;
        const bool full = nvalid >= ZONAL_VEC;
        const int xl = frame_west(x0, a.Nx, a.wrap);
        double q1_0[R], q2_0[R], q2_p[R], h_m[R], h_0[R], h_p[R], A_m[R], A_0[R], A_p[R];
        if (needU) load_row<true>(a.q1 + r0, x0, xl, full, a.Nx, q1_0);
        if (needV0) load_row<true>(a.q2 + r0, x0, xl, full, a.Nx, q2_0);
        if (needVp) load_row<true>(a.q2 + rp, x0, xl, full, a.Nx, q2_p);
        if (ld_h0) load_row<true>(a.h + r0, x0, xl, full, a.Nx, h_0);
        if (ld_hm) load_row<true>(a.h + rm, x0, xl, full, a.Nx, h_m);
        if (ld_hp) load_row<true>(a.h + rp, x0, xl, full, a.Nx, h_p);
        if (ld_A0) load_row<true>(a.A + r0, x0, xl, full, a.Nx, A_0);
        if (ld_Am) load_row<true>(a.A + rm, x0, xl, full, a.Nx, A_m);
        if (ld_Ap) load_row<true>(a.A + rp, x0, xl, full, a.Nx, A_p);

        // frame values: U and BY at the chunk's faces; V and BX on rows y and y + 1 from the west neighbour on (ℑxyᶠᶜ reads it)
        double U[ZONAL_VEC], BY[ZONAL_VEC], V0[R], Vp[R], BX0[R], BXp[R];
        if (needU) {
#pragma unroll
            for (int k = 0; k < ZONAL_VEC; ++k) U[k] = frame_vel(cons, q1_0[k + 1], h_0[k], h_0[k + 1]);
        }
        if (needV0) {
#pragma unroll
            for (int i = 0; i < R; ++i) V0[i] = frame_vel(cons, q2_0[i], h_m[i], h_0[i]);
        }
        if (needVp) {
#pragma unroll
            for (int i = 0; i < R; ++i) Vp[i] = frame_vel(cons, q2_p[i], h_0[i], h_p[i]);
        }
        if (needBX0) {
#pragma unroll
            for (int i = 0; i < R; ++i) BX0[i] = frame_bx(A_0[i], A_m[i], a.dy, h_m[i], h_0[i]);
        }
        if (needBXp) {
#pragma unroll
            for (int i = 0; i < R; ++i) BXp[i] = frame_bx(A_p[i], A_0[i], a.dy, h_0[i], h_p[i]);
        }
        if (needBY) {
#pragma unroll
            for (int k = 0; k < ZONAL_VEC; ++k) BY[k] = frame_by(A_0[k + 1], A_0[k], a.dx, h_0[k], h_0[k + 1]);
        }

        // the terms of cell x0 + k, added in x order (acc[p]: bit p of the mask)
#pragma unroll
        for (int k = 0; k < ZONAL_VEC; ++k) {
            if (k < nvalid) {
                if (w & SWMHD_ZM_U) acc[0] += U[k];
                if (w & SWMHD_ZM_V) acc[1] += V0[k + 1];
                if (w & SWMHD_ZM_H) acc[2] += h_0[k + 1];
                if (w & SWMHD_ZM_A) acc[3] += A_0[k + 1];
                if (wantS) acc[4] += frame_speed(U[k], V0[k], V0[k + 1], Vp[k], Vp[k + 1]);
                if (w & SWMHD_ZM_BX) acc[5] += BX0[k + 1];
                if (w & SWMHD_ZM_BY) acc[6] += BY[k];
                if (w & SWMHD_ZM_UU) acc[7] += U[k] * U[k];
                if (w & SWMHD_ZM_VV) acc[8] += V0[k + 1] * V0[k + 1];
                if (wantUV) acc[9] += U[k] * frame_xy_mean(V0[k], V0[k + 1], Vp[k], Vp[k + 1]);
                if (w & SWMHD_ZM_BXBX) acc[10] += BX0[k + 1] * BX0[k + 1];
                if (w & SWMHD_ZM_BYBY) acc[11] += BY[k] * BY[k];
                if (wantBB) acc[12] += BY[k] * frame_xy_mean(BX0[k], BX0[k + 1], BXp[k], BXp[k + 1]);
                if (wantVA) acc[13] += V0[k + 1] * (0.5 * (A_m[k + 1] + A_0[k + 1]));
            }
        }
        if (nvalid <= ZONAL_TRIP) break;
        x0 += ZONAL_TRIP;
    }

    // the 64 lane sums of every requested profile, then the mean: profile number = set bits below bit p
    out += row;
    const double n = (double)a.Nx;
#pragma unroll
    for (int p = 0; p < NPROF; ++p) {
        if (w & (1 << p)) {
            const double s = wave_sum(acc[p]);
            if (lane == 0) *out = s / n;
            out += a.osk;
        }
    }
}

// the profiles: `which` of them at out; profile and (ensembles) member stride in doubles
struct ZonalOut {
    int which;
    double *out;
    int64_t osk, osm = 0;
};

template <typename T>
int zonal_common(const T *q1, const T *q2, const T *h, const T *A, const Grid &g, int form, const Rows &r, const ZonalOut &o, int flags,
                 void *stream, const Ens *ens = nullptr) {
    if (!frame_source_ok(q1, q2, h, A, g, form) || !o.out || !g.rows_ok(r.j0, r.j1)) return SWMHD_EINVAL;
    if (o.which <= 0 || (o.which & ~SWMHD_ZM_ALL) || (flags & ~FRAME_FLAGS)) return SWMHD_EINVAL;
    if (o.osk < (int64_t)(r.j1 - r.j0) || !frame_members_ok(ens, g)) return SWMHD_EINVAL;
    if (ens && o.osm < (int64_t)__builtin_popcount((unsigned)o.which) * o.osk) return SWMHD_EINVAL;
    if (!frame_halo_ok(g)) return SWMHD_EHALO;
    const ZonalPlan p = zonal_plan(r.j1 - r.j0, ens ? ens->members : 1);
    if (p.none) return SWMHD_OK;
    if (p.too_many) return hiprc(hipErrorInvalidConfiguration);
    ZonalArgs<T> a;
    set_frame_source(a, q1, q2, h, A, g, form, o.which, flags, ens);
    a.out = o.out;
    a.j0 = r.j0; a.j1 = r.j1;
    a.osk = (long)o.osk; a.row_blocks = p.row_blocks; a.osm = ens ? (long)o.osm : 0;
    const dim3 grid((unsigned)p.blocks);
    hipStream_t s = (hipStream_t)stream;
    const bool lean = !(o.which & ~ZM_ROW);
    if (ens) {
        if (lean) hipLaunchKernelGGL((k_zonal_means<T, true, ZM_ROW>), grid, dim3(ZONAL_NT), 0, s, a);
        else hipLaunchKernelGGL((k_zonal_means<T, true, SWMHD_ZM_ALL>), grid, dim3(ZONAL_NT), 0, s, a);
    } else {
        if (lean) hipLaunchKernelGGL((k_zonal_means<T, false, ZM_ROW>), grid, dim3(ZONAL_NT), 0, s, a);
        else hipLaunchKernelGGL((k_zonal_means<T, false, SWMHD_ZM_ALL>), grid, dim3(ZONAL_NT), 0, s, a);
    }
    return hiprc(hipGetLastError());
}

}  // namespace
}  // namespace swmhd

extern "C" {

#define SWMHD_DEF_ZONAL(sfx, T)                                                                                                      \
    int swmhd_zonal_means_##sfx(const T *q1, const T *q2, const T *h, const T *A, int Nx, int Ny, int Hx, int Hy, int64_t sy, T dx,  \
                                T dy, int formulation, int j0, int j1, int which, double *out, int64_t out_stride_k, int flags,     \
                                void *stream) {                                                                                      \
        return swmhd::zonal_common<T>(q1, q2, h, A, swmhd::Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, formulation, swmhd::Rows{j0, j1},      \
                                      swmhd::ZonalOut{which, out, out_stride_k}, flags, stream);                                    \
    }                                                                                                                                \
    int swmhd_ensemble_zonal_means_##sfx(const T *q1, const T *q2, const T *h, const T *A, int members, int64_t stride_m, int Nx,   \
                                         int Ny, int Hx, int Hy, int64_t sy, T dx, T dy, int formulation, int j0, int j1, int which, \
                                         double *out, int64_t out_stride_k, int64_t out_stride_m, int flags, void *stream) {        \
        const swmhd::Ens e{members, stride_m};                                                                                       \
        return swmhd::zonal_common<T>(q1, q2, h, A, swmhd::Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, formulation, swmhd::Rows{j0, j1},      \
                                      swmhd::ZonalOut{which, out, out_stride_k, out_stride_m}, flags, stream, &e);                  \
    }

SWMHD_DEF_ZONAL(f64, double)
SWMHD_DEF_ZONAL(f32, float)

}  // extern "C"
