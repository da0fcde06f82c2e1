// Shared host/device declarations for libswmhd (gfx950).  Internal: the public surface is include/swmhd.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <type_traits>

namespace swmhd {

// Arguments of the Lorentz operator kernels.  Pointers address interior cell (i,j) = (1,1) of the
// halo-padded parent (Julia indexing), so 0-based cell (x,y) is ptr[y*sy + x] and halo cells have
// negative x / y.
template <typename T>
struct OpArgs {
    const T *A;
    const T *h;
    T *Fx;
    T *Fy;
    int Nx, Ny, Hx, Hy;
    long sy;
    T dx, dy, rdx, rdy;
    int j0, j1;  // rows [j0, j1) are computed (0-based)
    int topo_x, topo_y;
    int kernel_variant;  // 0 = by size, 1 = LDS-tiled kernel, 2 = row-marching kernel
    int edge_cols;       // LDS-tiled divergence kernel: only tile column 0 and the last one (or two): the x-wall frame of a Bounded grid
};

// launchers, one pair per translation unit (fast: reciprocal multiplies + FMA; strict: reference op order,
// compiled with -ffp-contract=off)
template <typename T> hipError_t launch_lorentz_jacobian_fast(const OpArgs<T> &a, hipStream_t s);
template <typename T> hipError_t launch_lorentz_jacobian_strict(const OpArgs<T> &a, hipStream_t s);
template <typename T> hipError_t launch_lorentz_divergence_fast(const OpArgs<T> &a, hipStream_t s);
template <typename T> hipError_t launch_lorentz_divergence_strict(const OpArgs<T> &a, hipStream_t s);

template <typename T>
hipError_t launch_fill_halo_periodic(T *interior, int Nx, int Ny, int Hx, int Hy, long sy, int which, hipStream_t s);
// up to 4 fields in one launch; corners resolved by wrapping both coordinates, so x and y halos need no ordering
// members > 0: an ensemble -- the same fill for each of `members` copies at interiors[k] + m * stride_m, in one launch
template <typename T>
hipError_t launch_fill_halo_periodic_multi(T *const *interiors, int nfields, int Nx, int Ny, int Hx, int Hy, long sy,
                                           int which, hipStream_t s, int members = 0, long stride_m = 0);
// fill_halo_regions! for any (Periodic | Bounded) topology pair with Oceananigans' default boundary conditions or gradient BCs
// (oracle_fill_halo): west/east pass, then south/north pass over the padded width.  face_x/face_y: bit f set = field f is
// located at Face in that direction; grad[f][4] = west, east, south, north GradientBoundaryCondition values (NaN = default).
// topo_y may carry TOPO_OPEN_SOUTH / TOPO_OPEN_NORTH (launch_plan.hpp): that side of a y-slab is a cut to its neighbour, not a wall.
// index offset that puts an open side's rows out of reach of every wall test (left_order / right_order / sym_fourth / wall_code)
constexpr int TOPO_FAR = 1 << 20;
template <typename T>
struct HaloBc {
    T *f[4];
    T grad[4][4];
    int nf, Nx, Ny, Hx, Hy, topo_x, topo_y, face_x, face_y;
    long sy;
    T dx, dy;
};
template <typename T> hipError_t launch_fill_halo_bc(const HaloBc<T> &a, hipStream_t s);
// The same fill for an ensemble (swmhd_ensemble_fill_halo_*): member blockIdx.y at f[k] + m * stride_m, its gradient values in a
// DEVICE table gtab[m * 4 * nf + 4 * f + side] (NaN = default; gtab == nullptr: defaults everywhere).  HaloBc::grad is not read.
template <typename T>
struct HaloBcEns : HaloBc<T> {
    long stride_m;
    int members;
    const T *gtab;
};
template <typename T> hipError_t launch_fill_halo_bc_ensemble(const HaloBcEns<T> &a, hipStream_t s);

// Arguments of the fused tendency kernels; pointers address interior cell (1,1) like OpArgs.
template <typename T>
struct TendArgs {
    const T *q1, *q2, *h, *A;   // (u|uh, v|vh, h, A)
    T *G1, *G2, *Gh, *GA;
    int Nx, Ny, Hx, Hy;
    long sy;
    T dx, dy, rdx, rdy, grav, fcor;
    int j0, j1;
    int j0b, j1b;         // optional SECOND row range served by the same launch (LDS-tiled kernel; empty when j1b <= j0b): the two
                          // boundary strips of a y-slab are one launch on the exchange's critical path instead of two
    // optional fused RK3 substep (fuse != 0):  Unew[f] = U[f] + dt (gamma G[f] + zeta Gm[f])  written to a SECOND set of
    // fields (neighbouring workgroups still read the old U through their halos); store_G = 0 skips writing G (last stage)
    int fuse, first, store_G;
    int gm_prev;          // Gm[] holds the previous STATE U- (U = U- + dt gamma- G-), zeta holds zeta/gamma-: Unew = U + dt gamma G + zeta (U - U-)
    int drop_G;           // marching kernels: issue the G stores with an out-of-range offset (the hardware drops them): lets the last RK3
                          // stage run the stage-2 kernel variant where that one has the better register allocation
    int wrap;             // periodic index wrapping of the READS: bit0 = x, bit1 = y -- the kernel takes (x mod Nx, y mod Ny) instead of the
                          // halo cells, so the caller need not have filled those halos (no halo-fill launch between RK3 stages)
    int kernel_variant;   // 0 = by size, 1 = LDS-tiled kernel, 2 = row-marching kernel
    int topo_x, topo_y;   // 0 Periodic, 1 Bounded (wall orders of the reconstructions; the LDS-tiled kernel implements them); topo_y of a
                          // y-slab of a Bounded-y chain also carries TOPO_OPEN_SOUTH / TOPO_OPEN_NORTH: that side is a cut, not a wall
    int leave_room;       // marching kernels: leave ~5 % of the workgroup slots free for another stream's kernels
    int edge_cols;        // LDS-tiled kernel: only the first and the last (narrow last: last two) 64-column tile columns -- the x-wall frame of a Bounded grid
    int fold_last;        // vector-invariant marching kernel: the last column strip is folded (MarchGeometry::fold; set by the launcher)
    T *Unew[4];
    const T *Gm[4];
    T dt, gamma, zeta;
    T dtg;                // dt * gamma, formed on the host (a uniform fp64 product would sit in a VGPR pair for the whole kernel)
    T cu, cg;             // the substep in coefficient form, Unew = (U + cu U) + dt gamma G + cg Gm: (0, dt zeta) for Gm = G-, (zeta', -zeta') for
                          // Gm = previous state (gm_prev).  The stage variant that reads Gm AND stores G (the second RK3 stage) uses this form,
                          // so that one compiled kernel serves both operands without a branch (a branch there cost the other variants their
                          // register allocation: 80 B of scratch).
    int anchor;           // RK3 in anchor form (RK3_ANCHOR below): first stage (first != 0) stores Unew = U + dtg G and W = U + dtw G, the latter
                          // through G1..GA; later stages read W from Gm and store Unew = W + dtg G.  No G store in either.
    T dtw;                // dt * (gamma1 + zeta2), formed on the host like dtg (first anchored stage only)
};
// Ensemble launches (swmhd_ensemble_*): `members` copies of one periodic grid stepped together, member m of every parent at
// ptr + m * stride_m (elements).  The tile kernel's ENS variant adds that offset to all of its field pointers.
template <typename T>
struct EnsTendArgs : TendArgs<T> {
    long stride_m;
    int members;
    int fold;             // 1: the member is folded into blockIdx.x (XCD-remapped over all tiles of all members, so a member's tiles
                          // share an XCD); 0: the member is blockIdx.y and the remap runs over the tiles of one member
};
// Per-member parameters (swmhd_ensemble_*_params): member m takes (g, f, dt) from the DEVICE table params[3 m .. 3 m + 2] when the
// kernel runs.  The tile kernel's PAR variant loads them after it has found its member and forms dtg and dtw from the member's dt as the
// host does for one grid (one multiply in T each); grav, fcor, dt, dtg and dtw of the base struct are not read.
template <typename T>
struct EnsParTendArgs : EnsTendArgs<T> {
    const T *params;
};
constexpr int ENS_NPARAMS = 3;   // = SWMHD_ENSEMBLE_NPARAMS
template <typename T, bool ENS, bool PAR = false>
using TileArgs = std::conditional_t<PAR, EnsParTendArgs<T>, std::conditional_t<ENS, EnsTendArgs<T>, TendArgs<T>>>;
// ---- RK3 stage schedule of the step drivers (step_common in swmhd_api.hip, both schedules of ring_step in ring.hip) --------------
// Oceananigans' RungeKutta3 (TimeSteppers): gamma = 8/15, 5/12, 3/4; zeta = -, -17/60, -5/12.  Since gamma1 + zeta2 = 1/4 and
// zeta3 = -gamma2, the step is exactly
//     U1 = U0 + dt gamma1 G0,   W = U0 + (dt/4) G0,   U2 = W + dt gamma2 G1,   U3 = W + dt gamma3 G2
// with ONE stored operand, the anchor W.  Fast periodic builds run it in that form (RK3_ANCHOR): stage 1 reads U0 and writes U1 and
// W, stages 2 and 3 read their state and W and write the new state -- 96 B/cell in every stage (288 B/cell-step, as the from-state
// G- form had, but split 64 / 128 / 96 there).  Strict builds and Bounded grids keep the classic G- form (store_tendencies!).
constexpr int GM_IS_PREV_STATE = 1024;   // = SWMHD_GM_IS_PREV_STATE (swmhd.h, which the kernel sources do not include)
constexpr int RK3_ANCHOR = 2048;         // = SWMHD_RK3_ANCHOR
constexpr double RK3_ANCHOR_WEIGHT = 0.25;   // gamma1 + zeta2 = 8/15 - 17/60
template <typename T>
struct Rk3Stage {
    T gamma, zeta;        // anchor form: zeta = gamma1 + zeta2 in the first stage (the weight of W), unused later
    int store_G;
    const T *const *Gm;   // G- operand: none (first stage), the G- buffers, or (anchor form) the buffers that hold W
    int flags;            // RK3_ANCHOR for the anchor form, else 0
};
template <typename T>
struct Rk3Buffers {
    T *cur[4], *alt[4], *gn[4], *gm[4];   // state read, state written, G written, G- read
    int swaps = 0;                        // stages run so far: odd = the newest state is in the caller's alternate buffers
    bool set(T *const *q, T *const *q_alt, T *const *Ga, T *const *Gb) {
        for (int f = 0; f < 4; ++f) {
            if (!q[f] || !q_alt[f] || !Ga[f] || !Gb[f]) return false;
            cur[f] = q[f]; alt[f] = q_alt[f]; gn[f] = Ga[f]; gm[f] = Gb[f];
        }
        return true;
    }
    // Stage st of a step.  Anchor form: the first stage writes W into gn; rotate() then moves that buffer to gm (read by the second
    // stage) and back to gn (read by the third) -- the G roles still swap once per stage, so two steps restore them.
    Rk3Stage<T> stage(int st, bool anchor) const {
        const T gam[3] = {T(8.0 / 15.0), T(5.0 / 12.0), T(3.0 / 4.0)};
        const T zet[3] = {T(0), T(-17.0 / 60.0), T(-5.0 / 12.0)};
        if (anchor) return {gam[st], st == 0 ? T(RK3_ANCHOR_WEIGHT) : T(0), 0, st == 0 ? nullptr : (st == 1 ? gm : gn), RK3_ANCHOR};
        return {gam[st], zet[st], st < 2 ? 1 : 0, st == 0 ? nullptr : gm, 0};   // (the last stage's G is never read)
    }
    // after a stage: the new state becomes current, and G- <- G (store_tendencies!: pointer swaps)
    void rotate() {
        for (int f = 0; f < 4; ++f) { T *t = cur[f]; cur[f] = alt[f]; alt[f] = t; t = gn[f]; gn[f] = gm[f]; gm[f] = t; }
        ++swaps;
    }
};

template <typename T>
struct Rk3Args {
    T *U[4];
    const T *Gn[4];
    const T *Gm[4];
    int Nx;
    long sy;
    int j0, j1;
    T dt, gamma, zeta;
    int first;
};
// Memory operations of the marching kernels are STRAIGHT-LINE code: every iteration issues the same loads and the same stores.
// Lanes / iterations that own no output (strip-halo lanes, columns beyond Nx, warm-up rows) still issue their stores, with an
// out-of-range buffer offset that the hardware drops, and loads are made unconditional by clamping.  Reason: the compiler's
// s_waitcnt insertion assumes, at every control-flow join, the incoming path with the FEWEST operations in flight; with an
// `if (col_ok)` around the stores (an execz branch) or a `continue` in the warm-up rows the wait for a prefetched row
// degenerated to vmcnt(0) at the top of every iteration -- each wave also waited for the stores it had just issued and for
// the row it had prefetched one iteration ago (PF rows of prefetch were in effect none).  With a fixed pattern the exact wait
// is stated once, at the end of the iteration: only operations OLDER than the row about to enter the windows must be back.
typedef int sw_v2i __attribute__((ext_vector_type(2)));
// packed fp32: two adjacent columns of a row in one 64-bit register pair (v_pk_* arithmetic); _u = as it lies in global memory,
// where a pair is only dword-aligned (the interior starts Hx = 3 floats into a row)
typedef float sw_f2 __attribute__((ext_vector_type(2)));
typedef sw_f2 sw_f2_u __attribute__((aligned(4)));
constexpr unsigned SW_OOB = 0xFFFFFFC0u;   // >= any parent's size in bytes (the launcher keeps parents below 4 GiB - 64 B)
template <typename T> __device__ __forceinline__ __amdgpu_buffer_rsrc_t out_rsrc(T *parent, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(parent, 0, (int)bytes, 0x00020000);
}
template <typename T> __device__ __forceinline__ void buffer_store(T v, __amdgpu_buffer_rsrc_t r, unsigned off) {
    if constexpr (sizeof(T) == 8) __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(sw_v2i, v), r, off, 0, 0);
    else __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v), r, off, 0, 0);
}
// s_waitcnt vmcnt(N) alone (gfx9 encoding: vmcnt[3:0] | expcnt[6:4] | lgkmcnt[11:8] | vmcnt[5:4] at [15:14])
template <int N> __device__ __forceinline__ void wait_vmem_all_but() {
    static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit counter");
    __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | (7 << 4) | (15 << 8));
}

// Wave priority that falls with progress ("laggards first") for the row-marching kernels.  Their grid is ONE round of resident
// workgroups, so the workgroups sharing a CU start together -- but the SIMD arbiter issues oldest-wave-first, and with equal
// priorities they finish one after the other: measured for the vector-invariant tendency kernel at 55 %, 75 % and 100 % of the
// launch (profiles/r01/workgroup_timeline.json), i.e. the last quarter of the launch ran one wave per SIMD, which cannot hide
// the ~8-cycle dependent-issue latency of fp64 (tools/valu_probe.hip).  Dropping a wave's priority at 60 / 85 / 95 % of its rows
// lets the others catch up: all workgroups finish within 10 % of each other, launch -6 %.
struct ProgressPriority {
    int t1, t2, t3;
    __device__ __forceinline__ explicit ProgressPriority(int niter)
        : t1((niter * 3) / 5), t2((niter * 17) / 20), t3((niter * 19) / 20) {
        __builtin_amdgcn_s_setprio(3);
    }
    __device__ __forceinline__ void at(int it) const {
        if (it == t1) __builtin_amdgcn_s_setprio(2);
        if (it == t2) __builtin_amdgcn_s_setprio(1);
        if (it == t3) __builtin_amdgcn_s_setprio(0);
    }
};
// (Slab driver, two streams on one chip: starting the interior launch one priority level lower and holding the boundary-zone launch
//  beside it at the top level was measured and dropped -- the ring-of-one step got 2-8 % SLOWER at every slab height: the falling
//  priorities are what keeps the interior's own workgroups in step.)

// (launch geometry and kernel choice of the tendency kernels: launch_plan.hpp, host only)
template <typename T> hipError_t launch_tendency_fast(const TendArgs<T> &a, int formulation, int lorentz, hipStream_t s);
template <typename T> hipError_t launch_tendency_strict(const TendArgs<T> &a, int formulation, int lorentz, hipStream_t s);
template <typename T> hipError_t launch_rk3_substep_fast(const Rk3Args<T> &a, hipStream_t s);
// ensemble stage: every tile of every member in one launch of the LDS-tiled kernel (rows [a.j0, a.j1) of each member; no second range,
// no Bounded frame: Bounded members run the wall kernel on every tile).  The launcher sets a.fold.
template <typename T> hipError_t launch_tendency_ensemble_fast(const EnsTendArgs<T> &a, int formulation, int lorentz, hipStream_t s);
template <typename T> hipError_t launch_tendency_ensemble_strict(const EnsTendArgs<T> &a, int formulation, int lorentz, hipStream_t s);
// the same stage with per-member (g, f, dt): the PAR instantiations of the same kernels, same plan, same member mapping
template <typename T> hipError_t launch_ensemble_params_stage_fast(const EnsParTendArgs<T> &a, int formulation, int lorentz, hipStream_t s);
template <typename T> hipError_t launch_ensemble_params_stage_strict(const EnsParTendArgs<T> &a, int formulation, int lorentz, hipStream_t s);
// (internal twins of exported calls for the slab driver: api_args.hpp, host only)
template <typename T> hipError_t launch_rk3_substep_strict(const Rk3Args<T> &a, hipStream_t s);

// Passive tracers (swmhd_tracers_rk3_*, tracer_kernels.inc): K extra centre fields advected by the state (q1, q2, h) a stage starts
// from, all of them through that RK3 stage in ONE launch of an LDS-tiled kernel.  Pointers address interior cell (1,1) like TendArgs;
// fuse / first / store_G / anchor / wrap / topo / dtg / dtw mean what they mean there.
constexpr int MAX_TRACERS = 8;            // = SWMHD_MAX_TRACERS (the workgroup's tile: TRACER_TILE_X / _Y, launch_plan.hpp)
template <typename T>
struct TracerArgs {
    const T *q1, *q2, *h;
    const T *c[MAX_TRACERS];
    T *cnew[MAX_TRACERS], *Gn[MAX_TRACERS];
    const T *Gm[MAX_TRACERS];
    int K, Nx, Ny, Hx, Hy;
    long sy;
    T dx, dy, rdx, rdy;
    int j0, j1;
    int fuse, first, store_G, anchor, wrap, topo_x, topo_y;
    T dt, gamma, zeta, dtg, dtw;
};
template <typename T> hipError_t launch_tracers_fast(const TracerArgs<T> &a, int formulation, hipStream_t s);
template <typename T> hipError_t launch_tracers_strict(const TracerArgs<T> &a, int formulation, hipStream_t s);
// Tracers of an ensemble (swmhd_ensemble_tracers_rk3_*): all K tracers of all `members` periodic members through one stage in ONE
// launch, member m of every parent (q1, q2, h, c[k], cnew[k], Gn[k], Gm[k]) at ptr + m * stride_m.  The kernel's ENS variant folds the
// member into blockIdx.x (EnsTendArgs::fold = 1) and adds the offset where it forms an address; the pointer arrays are not rewritten
// (they are indexed by the tracer loop: a modified copy would live in scratch).  All rows of every member; j0 / j1 = 0 / Ny.
template <typename T>
struct EnsTracerArgs : TracerArgs<T> {
    long stride_m;
    int members;
};
// Per-member dt from the DEVICE table params[3 m + 2] (EnsParTendArgs; g and f do not enter a tracer's tendency): the PAR variant forms
// dtg and dtw from it as the host does for one grid; dt, dtg and dtw of the base struct are not read.
template <typename T>
struct EnsParTracerArgs : EnsTracerArgs<T> {
    const T *params;
};
template <typename T, bool ENS, bool PAR = false>
using TracerTileArgs = std::conditional_t<PAR, EnsParTracerArgs<T>, std::conditional_t<ENS, EnsTracerArgs<T>, TracerArgs<T>>>;
template <typename T> hipError_t launch_tracers_ensemble_fast(const EnsTracerArgs<T> &a, int formulation, hipStream_t s);
template <typename T> hipError_t launch_tracers_ensemble_strict(const EnsTracerArgs<T> &a, int formulation, hipStream_t s);
template <typename T> hipError_t launch_tracers_ensemble_params_fast(const EnsParTracerArgs<T> &a, int formulation, hipStream_t s);
template <typename T> hipError_t launch_tracers_ensemble_params_strict(const EnsParTracerArgs<T> &a, int formulation, hipStream_t s);

// What the per-stage correction launches (strip_device.inc) share: a term D of the state the stage started from, added to what the stage
// kernels have written with the weights a (new state) and w (stored tendency or anchor).  Pointers address interior cell (1,1) like
// TendArgs; wrap as there.  members > 0: an ensemble -- member m of every parent at ptr + m * stride_m; with params != nullptr its dt is
// params[3 m + 2] and the kernel forms a_m = dt a (a: gamma) and, with `anchor`, w_m = dt w (w: the anchor's weight), else w_m = w.
template <typename T>
struct StripArgs {
    int Nx, Ny, j0, j1, wrap;
    long sy;
    T a, w;
    int members, anchor;
    long stride_m;
    const T *params;
};

// ScalarDiffusivity closure (swmhd_diffusion_rk3_*, diffusion.hip): D_k = coef_k laplace(old_k) of up to 3 + MAX_TRACERS fields in ONE
// launch: nw[k] += a D_k and, where acc[k] != nullptr, acc[k] += w D_k.  An ensemble member's coefficients stand in the DEVICE table
// coef_tab[m * nfields + k] (coef is not read).
constexpr int DIFFUSION_MAX_FIELDS = 3 + MAX_TRACERS;   // = SWMHD_DIFFUSION_MAX_FIELDS
template <typename T>
struct DiffusionArgs : StripArgs<T> {
    const T *old[DIFFUSION_MAX_FIELDS];
    T *nw[DIFFUSION_MAX_FIELDS], *acc[DIFFUSION_MAX_FIELDS];
    T coef[DIFFUSION_MAX_FIELDS];
    int nfields;
    T dx, dy;
    const T *coef_tab;
};
template <typename T> hipError_t launch_diffusion_fast(const DiffusionArgs<T> &a, hipStream_t s);
template <typename T> hipError_t launch_diffusion_strict(const DiffusionArgs<T> &a, hipStream_t s);
// ScalarBiharmonicDiffusivity closure (swmhd_biharmonic_rk3_*, biharmonic.hip): the same arguments, D_k = -coef_k laplace(laplace(old_k)),
// which reads two cells around
template <typename T> hipError_t launch_biharmonic_fast(const DiffusionArgs<T> &a, hipStream_t s);
template <typename T> hipError_t launch_biharmonic_strict(const DiffusionArgs<T> &a, hipStream_t s);

// BetaPlane Coriolis (swmhd_coriolis_rk3_*, coriolis.hip): D1 = fc[j] vbar, D2 = -(ff[j] ubar) of the two momentum-like fields q1, q2 in
// ONE launch, added to what the stage kernels (run with f = 0) have written: n1 += a D1, n2 += a D2 and, where a1 != nullptr (then a2
// too), a1 += w D1, a2 += w D2.  frow: the DEVICE table fc[0..Ny) then ff[0..Ny); an ensemble member's table at frow + m * 2 Ny.
template <typename T>
struct CoriolisArgs : StripArgs<T> {
    const T *q1, *q2;
    T *n1, *n2, *a1, *a2;
    const T *frow;
};
template <typename T> hipError_t launch_coriolis_fast(const CoriolisArgs<T> &a, hipStream_t s);
template <typename T> hipError_t launch_coriolis_strict(const CoriolisArgs<T> &a, hipStream_t s);

// Relaxation forcing (swmhd_relaxation_rk3_*, relaxation.hip): D_k = (rate_k mask_k) (target_k - old_k) of up to 4 + MAX_TRACERS fields in
// ONE launch: nw[k] += a D_k and, where acc[k] != nullptr, acc[k] += w D_k.  mask[k] == nullptr: no mask; target[k] == nullptr: the scalar
// tval[k].  An ensemble member's masks and targets stand at ptr + m * mask_stride_m / target_stride_m (0: shared), its rates and scalar
// targets in the DEVICE tables rate_tab / tval_tab [m * nfields + k] (rate and tval are not read).
constexpr int RELAXATION_MAX_FIELDS = 4 + MAX_TRACERS;   // = SWMHD_RELAXATION_MAX_FIELDS
template <typename T>
struct RelaxationArgs : StripArgs<T> {
    const T *old[RELAXATION_MAX_FIELDS], *mask[RELAXATION_MAX_FIELDS], *target[RELAXATION_MAX_FIELDS];
    T *nw[RELAXATION_MAX_FIELDS], *acc[RELAXATION_MAX_FIELDS];
    T rate[RELAXATION_MAX_FIELDS], tval[RELAXATION_MAX_FIELDS];
    int nfields;
    long mask_stride_m, target_stride_m;
    const T *rate_tab, *tval_tab;
};
template <typename T> hipError_t launch_relaxation_fast(const RelaxationArgs<T> &a, hipStream_t s);
template <typename T> hipError_t launch_relaxation_strict(const RelaxationArgs<T> &a, hipStream_t s);

// Static sources (swmhd_source_rk3_*, source.hip): D_k = src_k (kind 0) or the thickness `hold` of the state the stage started from,
// interpolated to the x face (kind 1) or the y face (kind 2), times src_k, of up to 4 + MAX_TRACERS fields in ONE launch: nw[k] += a D_k
// and, where acc[k] != nullptr, acc[k] += w D_k.  An ensemble member's sources stand at ptr + m * source_stride_m (0: shared), its
// thickness at hold + m * stride_m.  old is carried for pack_fields and never read.
constexpr int SOURCE_MAX_FIELDS = 4 + MAX_TRACERS;   // = SWMHD_SOURCE_MAX_FIELDS
template <typename T>
struct SourceArgs : StripArgs<T> {
    const T *old[SOURCE_MAX_FIELDS], *src[SOURCE_MAX_FIELDS];
    T *nw[SOURCE_MAX_FIELDS], *acc[SOURCE_MAX_FIELDS];
    int kind[SOURCE_MAX_FIELDS];
    const T *hold;
    int nfields;
    long source_stride_m;
};
template <typename T> hipError_t launch_source_fast(const SourceArgs<T> &a, hipStream_t s);
template <typename T> hipError_t launch_source_strict(const SourceArgs<T> &a, hipStream_t s);

// Stochastic forcing (swmhd_stochastic_rk3_*, stochastic.hip): F_k = sum over M[k] modes of cx (P cy + Q sy) + sx (Q cy - P sy) of up to
// 4 + MAX_TRACERS fields in ONE launch: nw[k] += a F_k and, where acc[k] != nullptr, acc[k] += w F_k.  coef[k]: P[0 .. M) then Q[0 .. M);
// xtab[k] / ytab[k]: rows 2 m (cos) and 2 m + 1 (sin) of xp / yp elements, at column / row 0 of the interior.  An ensemble member's
// coefficients stand at coef[k] + m * coef_stride_m; the tables are shared.  old is carried for pack_fields and never read.
constexpr int STOCHASTIC_MAX_FIELDS = 4 + MAX_TRACERS;   // = SWMHD_STOCHASTIC_MAX_FIELDS
constexpr int STOCHASTIC_MAX_MODES = 256;                // = SWMHD_STOCHASTIC_MAX_MODES
constexpr int STOCHASTIC_MODE_CHUNK = 4;                 // = SWMHD_STOCHASTIC_MODE_CHUNK
template <typename T>
struct StochasticArgs : StripArgs<T> {
    const T *old[STOCHASTIC_MAX_FIELDS], *coef[STOCHASTIC_MAX_FIELDS], *xtab[STOCHASTIC_MAX_FIELDS], *ytab[STOCHASTIC_MAX_FIELDS];
    T *nw[STOCHASTIC_MAX_FIELDS], *acc[STOCHASTIC_MAX_FIELDS];
    int M[STOCHASTIC_MAX_FIELDS];
    int nfields;
    long xp, yp, coef_stride_m;
};
template <typename T> hipError_t launch_stochastic_fast(const StochasticArgs<T> &a, hipStream_t s);
template <typename T> hipError_t launch_stochastic_strict(const StochasticArgs<T> &a, hipStream_t s);
// The coefficient draw of one time step (swmhd_stochastic_coefficients_*, stochastic_coefficients.hip): one workgroup per member.
// kind 0: coef = P, Q of M each; kind 1: Pu, Qu, Pv, Qv of M each.  amp0, ktx, kty: DEVICE doubles; member m reads amp0 + m * amp_stride_m
// and writes coef + m * coef_stride_m, with substreams[m] (nullptr: `substream` for the one member).
template <typename T>
struct StochasticCoefArgs {
    unsigned long long *counter;
    T *coef[STOCHASTIC_MAX_FIELDS];
    const double *amp0[STOCHASTIC_MAX_FIELDS], *ktx[STOCHASTIC_MAX_FIELDS], *kty[STOCHASTIC_MAX_FIELDS];
    int M[STOCHASTIC_MAX_FIELDS], kind[STOCHASTIC_MAX_FIELDS];
    int ngroups, members;
    long coef_stride_m, amp_stride_m;
    unsigned seed_lo, seed_hi, substream;
    const unsigned *substreams;
    double sdt;
};
template <typename T> hipError_t launch_stochastic_coefficients(const StochasticCoefArgs<T> &a, hipStream_t s);

// Lagrangian particles (swmhd_particles_rk3_*, swmhd_particles_sample_*, particles.hip; include/swmhd_particles.h states the scheme).
// Field pointers address interior cell (1,1) like TendArgs; x, y, gx, gy (and out) are dense per member.  mode_x, mode_y: how a
// direction is indexed and folded -- PARTICLE_WRAP: the true modulus, interior cells only; PARTICLE_PERIODIC: the parent as it is
// (clamped), folded periodically; PARTICLE_BOUNDED: the parent as it is, reflected.  members > 0: an ensemble, member = blockIdx.x / nblk;
// with params != nullptr its dt is params[3 m + 2], widened.
constexpr int PARTICLES_BLOCK = 256;        // = SWMHD_PARTICLES_BLOCK
constexpr int PARTICLES_MAX_FIELDS = 12;    // = SWMHD_PARTICLES_MAX_FIELDS
constexpr int PARTICLE_WRAP = 0, PARTICLE_PERIODIC = 1, PARTICLE_BOUNDED = 2;
struct ParticleGrid {
    long P;
    int Nx, Ny, Hx, Hy;
    long sy;
    double x0, y0, dx, dy;
    int mode_x, mode_y;
    int members;
    long stride_m;
    unsigned nblk;      // workgroups of one member: ceil(P / PARTICLES_BLOCK)
};
template <typename T>
struct ParticleArgs : ParticleGrid {
    const T *q1, *q2, *h;
    double *x, *y, *gx, *gy;
    int cons;
    double dt, gamma, zeta;
    const T *params;
};
template <typename T>
struct ParticleSampleArgs : ParticleGrid {
    const T *f[PARTICLES_MAX_FIELDS];
    int loc[PARTICLES_MAX_FIELDS];
    int nfields;
    const double *x, *y;
    double *out;
};
template <typename T> hipError_t launch_particles(const ParticleArgs<T> &a, hipStream_t s);
template <typename T> hipError_t launch_particles_sample(const ParticleSampleArgs<T> &a, hipStream_t s);

// energies + extrema; workspace >= SWMHD_DIAG_WORKSPACE doubles, out = 7 doubles (both device memory).  members > 0: an ensemble,
// rows [j0, j1) of each member at ptr + m * stride_m, out = members x 7, workspace >= SWMHD_ENSEMBLE_DIAG_WORKSPACE.  params != nullptr
// (ensembles only): member m's g is params[3 m] (DEVICE table), grav is not read
template <typename T>
hipError_t launch_diagnostics(const T *q1, const T *q2, const T *h, const T *A, int Nx, int Ny, int j0, int j1, long sy, T dx, T dy,
                              T grav, T href, int form, double *workspace, double *out, hipStream_t s, int members = 0, long stride_m = 0,
                              const T *params = nullptr);

// Periodic "gather on read": with TendArgs::wrap the tendency kernels map a halo index to its periodic image in the interior when
// they LOAD (one integer select per row / per lane, outside the arithmetic), so the state needs no halo-fill launch between RK3
// stages: 3 launches per step instead of 6 on one GPU, and no x-halo kernel in front of the ring exchange on a slab.  (Round 1 had
// the tile kernel scatter the images on write instead; that could not serve the marching kernels without costing them registers.)
__device__ __forceinline__ int wrap_index(int v, int n, int lo, int hi, bool wrap) {
    if (wrap) v = v < 0 ? v + n : (v >= n ? v - n : v);
    return v < lo ? lo : (v > hi ? hi : v);   // (lanes / rows beyond one period only feed outputs that are never stored)
}

// XCD-aware block remap (cdna_hip_programming.md T1): hardware deals consecutive block ids round-robin
// over the 8 XCDs; remapping gives each XCD (and its private 4 MiB L2) a contiguous run of tiles, so the
// halo rows/columns that y-/x-adjacent tiles share are L2 hits instead of second HBM/MALL fetches.
// Bijective for any grid size.
__device__ __forceinline__ unsigned xcd_remap(unsigned bid, unsigned nblk) {
    constexpr unsigned NXCD = 8;
    unsigned q = nblk / NXCD, r = nblk % NXCD;  // XCDs [0,r) own q+1 blocks, the rest q
    unsigned x = bid % NXCD, k = bid / NXCD;
    unsigned base = x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q;
    return base + k;
}

}  // namespace swmhd
