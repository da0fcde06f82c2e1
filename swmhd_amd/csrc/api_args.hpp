// Host-only argument layer of the C ABI (swmhd_api.hip, ring.hip, the host tails of output.hip, zonal.hip, spectra.hip and spectra2d.hip): what a valid halo-padded grid is,
// what the physics arguments may be, what the SWMHD_* flag bits mean and which of them each family of entry points takes -- each said
// once.  No kernel, no launch.  Internal, like common.hpp.
#pragma once
#include "../../include/swmhd.h"
#include "launch_plan.hpp"
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace swmhd {

inline int hiprc(hipError_t e) { return e == hipSuccess ? SWMHD_OK : -(int)e; }

// face_x / face_y of the boundary-condition fill of the four prognostic fields: u|uh at Face in x, v|vh at Face in y
constexpr int FACE_X = 0b0001, FACE_Y = 0b0010;

// ---- the grid: a halo-padded parent, x fastest ----------------------------------------------------------------------------------
// dx, dy are held as double: an fp32 caller's values convert exactly, both ways.  Calls without spacings leave them at 1.
struct Grid {
    int Nx, Ny, Hx, Hy;
    int64_t sy;
    double dx = 1.0, dy = 1.0;
    bool stride_ok() const { return sy >= (int64_t)Nx + 2 * Hx; }
    bool extents_ok() const { return Nx > 0 && Ny > 0 && Hx >= 0 && Hy >= 0 && stride_ok(); }
    bool spacing_ok() const { return dx > 0.0 && dy > 0.0; }   // (NaN fails)
    bool halo_at_least(int n) const { return Hx >= n && Hy >= n; }
    // one period covers the halo in the directions of `wrap` (bit 0 x, bit 1 y)
    bool period_covers_halo(int wrap) const { return !((wrap & 1) && Hx > Nx) && !((wrap & 2) && Hy > Ny); }
    bool rows_ok(int j0, int j1, int ext = 0) const { return j0 >= -ext && j1 <= Ny + ext && j0 <= j1; }
    long offset() const { return (long)Hy * sy + Hx; }   // parent -> interior cell (1,1), where every kernel argument points
    template <typename P> P *interior(P *p) const { return p + offset(); }
    int64_t min_member_stride() const { return ((int64_t)Ny + 2 * Hy) * sy; }
};

// ---- the physics of a call (the first four fields, in the order every exported call has them) and the scalars of one RK3 stage ------
// The *_params calls leave grav, fcor and dt at 0: the kernels take them from the device table (Ens::params).
template <typename T>
struct Physics {
    T grav = T(0), fcor = T(0);
    int formulation = SWMHD_VECTOR_INVARIANT, lorentz = SWMHD_LORENTZ_NONE;
    T dt = T(0), gamma = T(0), zeta = T(0);
    int store_G = 1;
};
inline bool formulation_ok(int f) { return f == SWMHD_CONSERVATIVE || f == SWMHD_VECTOR_INVARIANT; }
// the Jacobian forcing acts on (u, v), the divergence forcing on (uh, vh)  (SWMHD_example.jl:30-31, divergence_sw_mhd.jl:28-29)
inline bool forcing_ok(int formulation, int lorentz) {
    return lorentz == SWMHD_LORENTZ_NONE || (formulation == SWMHD_VECTOR_INVARIANT && lorentz == SWMHD_LORENTZ_JACOBIAN) ||
           (formulation == SWMHD_CONSERVATIVE && lorentz == SWMHD_LORENTZ_DIVERGENCE);
}
inline bool topology_ok(int topo_x, int topo_y) {
    return (topo_x == SWMHD_BOUNDED || topo_x == SWMHD_PERIODIC) && (topo_y == SWMHD_BOUNDED || topo_y == SWMHD_PERIODIC);
}

// rows [j0, j1) and, for the slab driver's twin, a second range [j0b, j1b) above the first (empty when j1b <= j0b)
struct Rows {
    int j0, j1, j0b = 0, j1b = 0;
    bool second() const { return j1b > j0b; }
};

// ---- the flag bits, decoded -------------------------------------------------------------------------------------------------------
struct Flags {
    int bits;
    bool strict;
    int kernel_variant;   // 0 = by size, 1 = LDS-tiled kernel, 2 = row-marching kernel
    int wrap;             // bit 0 = x, bit 1 = y
    int topo_x, topo_y;   // topology codes; topo_y with the TOPO_OPEN_* bits of a chain slab's cut sides
    int leave_room, anchor, gm_prev;
    int bounded() const { return bits & (SWMHD_BOUNDED_X | SWMHD_BOUNDED_Y); }
};
inline Flags decode_flags(int f) {
    Flags d;
    d.bits = f;
    d.strict = (f & SWMHD_STRICT) != 0;
    d.kernel_variant = (f & SWMHD_TILE_KERNEL) ? 1 : ((f & SWMHD_MARCH_KERNEL) ? 2 : 0);
    d.wrap = ((f & SWMHD_WRAP_X) ? 1 : 0) | ((f & SWMHD_WRAP_Y) ? 2 : 0);
    d.topo_x = (f & SWMHD_BOUNDED_X) ? SWMHD_BOUNDED : SWMHD_PERIODIC;
    d.topo_y = ((f & SWMHD_BOUNDED_Y) ? SWMHD_BOUNDED : SWMHD_PERIODIC) | ((f & SWMHD_OPEN_SOUTH) ? TOPO_OPEN_SOUTH : 0) |
               ((f & SWMHD_OPEN_NORTH) ? TOPO_OPEN_NORTH : 0);
    d.leave_room = (f & SWMHD_LEAVE_ROOM) ? 1 : 0;
    d.anchor = (f & SWMHD_RK3_ANCHOR) ? 1 : 0;
    d.gm_prev = (f & SWMHD_GM_IS_PREV_STATE) ? 1 : 0;
    return d;
}
// a direction is Bounded or wrapped on read, never both
inline bool bounded_wrap_conflict(int f) {
    return ((f & SWMHD_BOUNDED_X) && (f & SWMHD_WRAP_X)) || ((f & SWMHD_BOUNDED_Y) && (f & SWMHD_WRAP_Y));
}

// ---- which flags each family of entry points takes --------------------------------------------------------------------------------
// *_FLAGS: accepted.  *_NOTSUP: known and refused with SWMHD_ENOTSUP.  Any other bit: SWMHD_EINVAL.  (Combinations a family refuses
// beyond that -- the anchor form of a strict build, walls on the marching kernel -- are refused where the family checks its call.)
constexpr int KERNEL_FLAGS = SWMHD_TILE_KERNEL | SWMHD_MARCH_KERNEL, WRAP_FLAGS = SWMHD_WRAP_X | SWMHD_WRAP_Y;
constexpr int BOUNDED_FLAGS = SWMHD_BOUNDED_X | SWMHD_BOUNDED_Y, OPEN_FLAGS = SWMHD_OPEN_SOUTH | SWMHD_OPEN_NORTH;
constexpr int LORENTZ_FLAGS = SWMHD_STRICT | KERNEL_FLAGS;
constexpr int SUBSTEP_FLAGS = SWMHD_STRICT;
constexpr int OUTPUT_FLAGS = WRAP_FLAGS;
constexpr int ZONAL_FLAGS = WRAP_FLAGS;   // swmhd_zonal_means: the frame's
constexpr int DERIVED_FLAGS = WRAP_FLAGS; // swmhd_derived_fields: the frame's
constexpr int SPECTRA_FLAGS = WRAP_FLAGS; // swmhd_zonal_spectra: the frame's
constexpr int SPECTRA2D_FLAGS = WRAP_FLAGS; // swmhd_spectra2d: the frame's
// swmhd_tendencies[_rk3], swmhd_step_rk3 and the slab drivers' stages
constexpr int TEND_FLAGS = SWMHD_STRICT | KERNEL_FLAGS | WRAP_FLAGS | SWMHD_LEAVE_ROOM | BOUNDED_FLAGS | SWMHD_GM_IS_PREV_STATE |
                           SWMHD_RK3_ANCHOR | OPEN_FLAGS;
// swmhd_tracers_rk3; the tracers of an ensemble (periodic members only) refuse the Bounded flags as well
constexpr int TRACER_FLAGS = SWMHD_STRICT | SWMHD_TILE_KERNEL | WRAP_FLAGS | BOUNDED_FLAGS | SWMHD_RK3_ANCHOR;
constexpr int TRACER_NOTSUP = SWMHD_MARCH_KERNEL | SWMHD_GM_IS_PREV_STATE | OPEN_FLAGS | SWMHD_LEAVE_ROOM;
// swmhd_diffusion_rk3 and its ensemble form (periodic grids only; SWMHD_RK3_ANCHOR: what `w` means to the ensemble call with a table)
constexpr int DIFFUSION_FLAGS = SWMHD_STRICT | WRAP_FLAGS | SWMHD_RK3_ANCHOR;
constexpr int DIFFUSION_NOTSUP = BOUNDED_FLAGS | KERNEL_FLAGS | SWMHD_GM_IS_PREV_STATE | OPEN_FLAGS | SWMHD_LEAVE_ROOM;
// swmhd_coriolis_rk3 and its ensemble form: the Bounded flags say only that the direction is not wrapped (the filled halo carries the
// wall), so a direction with both its flags is an argument error; SWMHD_RK3_ANCHOR as for the diffusion calls
constexpr int CORIOLIS_FLAGS = SWMHD_STRICT | WRAP_FLAGS | BOUNDED_FLAGS | SWMHD_RK3_ANCHOR;
constexpr int CORIOLIS_NOTSUP = KERNEL_FLAGS | SWMHD_GM_IS_PREV_STATE | OPEN_FLAGS | SWMHD_LEAVE_ROOM;
// swmhd_ensemble_*: the periodic family, and the boundary-condition family (swmhd_ensemble_fill_halo, swmhd_ensemble_step_rk3_bc),
// which accepts Bounded directions and runs the stage in G- form
constexpr int ENS_FLAGS = SWMHD_STRICT | SWMHD_TILE_KERNEL | WRAP_FLAGS | SWMHD_RK3_ANCHOR;
constexpr int ENS_NOTSUP = BOUNDED_FLAGS | SWMHD_MARCH_KERNEL | SWMHD_GM_IS_PREV_STATE | SWMHD_LEAVE_ROOM;
constexpr int ENS_BC_FLAGS = SWMHD_STRICT | SWMHD_TILE_KERNEL | WRAP_FLAGS | BOUNDED_FLAGS;
constexpr int ENS_BC_NOTSUP = SWMHD_MARCH_KERNEL | SWMHD_GM_IS_PREV_STATE | SWMHD_LEAVE_ROOM | SWMHD_RK3_ANCHOR;
// swmhd_ring_step_rk3_bc (SWMHD_OPEN_* unknown: the chain decides its walls)
constexpr int RING_BC_FLAGS = SWMHD_STRICT | SWMHD_TILE_KERNEL | WRAP_FLAGS | BOUNDED_FLAGS | SWMHD_LEAVE_ROOM;
constexpr int RING_BC_NOTSUP = SWMHD_MARCH_KERNEL | SWMHD_GM_IS_PREV_STATE | SWMHD_RK3_ANCHOR;
// Two answers to one defect, each kept as it was: a wrapped period shorter than the halo (Grid::period_covers_halo) is SWMHD_EHALO to
// the tendency calls (tend_common) and SWMHD_EINVAL to the tracer calls (tracers_common).

// ---- ensembles --------------------------------------------------------------------------------------------------------------------
// `members` copies of one grid, member m of every parent at ptr + m * stride_m.  The single-grid helpers take it as an optional last
// argument and check everything else exactly as for one grid.
struct Ens {
    int members;
    int64_t stride_m;
    bool bc = false;    // the boundary-condition family
    bool par = false;   // the *_params calls: `params` is the DEVICE table of members x (g, f, dt) in the call's element type
    const void *params = nullptr;
};
// the checks of the ensemble itself (the caller's single-grid checks follow): table, member count, member stride, flags; none: a single grid
inline int ens_check(const Ens *ens, const Grid &g, int flags) {
    if (!ens) return SWMHD_OK;
    const Ens &e = *ens;
    const int ok = e.bc ? ENS_BC_FLAGS : ENS_FLAGS, notsup = e.bc ? ENS_BC_NOTSUP : ENS_NOTSUP;
    if (e.par && !e.params) return SWMHD_EINVAL;
    if (e.members < 1 || e.members > SWMHD_ENSEMBLE_MAX_MEMBERS) return SWMHD_EINVAL;
    if (g.Ny <= 0 || g.Hy < 0 || g.sy <= 0 || e.stride_m < g.min_member_stride()) return SWMHD_EINVAL;
    if (flags & ~(ok | notsup)) return SWMHD_EINVAL;
    if (flags & notsup) return SWMHD_ENOTSUP;
    return SWMHD_OK;
}

// ---- what OpArgs, TendArgs and TracerArgs share -----------------------------------------------------------------------------------
// extents, stride, spacings and their reciprocals (formed in the kernel's element type), topology codes; pointers: Grid::interior
template <typename Args>
void set_grid(Args &a, const Grid &g, int topo_x, int topo_y) {
    using T = decltype(a.dx);
    a.Nx = g.Nx; a.Ny = g.Ny; a.Hx = g.Hx; a.Hy = g.Hy; a.sy = (long)g.sy;
    a.dx = T(g.dx); a.dy = T(g.dy); a.rdx = T(1) / a.dx; a.rdy = T(1) / a.dy;
    a.topo_x = topo_x; a.topo_y = topo_y;
}

// ---- what the slab driver (ring.hip) shares with the exported calls of the same names: same checks, same return codes --------------
// sides of a boundary-condition fill: topology codes and the Face bits of the fields (common.hpp: HaloBc)
struct BcSides { int topo_x, topo_y, face_x, face_y; };
// rows r of one RK3 stage; both ranges of r in ONE launch where the kernel chosen supports it
template <typename T>
int tendencies_rk3(const T *const *q, T *const *qnew, T *const *Gn, const T *const *Gm, const Grid &g, const Physics<T> &ph, const Rows &r,
                   int flags, void *stream, const Ens *ens = nullptr);
template <typename T> int fill_halo_periodic_multi(T *const *f, int nf, const Grid &g, int which, void *stream, const Ens *ens = nullptr);
// swmhd_fill_halo of one y-slab: x as s.topo_x says (s.topo_y is not read), y walls only on the sides of walls_y (bit 0 south, bit 1
// north), the other y sides untouched.  gradient: HOST array of 4 nf values (gtab == nullptr), or gtab: a DEVICE table of 4 nf values.
template <typename T>
int fill_halo_walls(T *const *f, int nf, const Grid &g, BcSides s, int walls_y, const T *gradient, const T *gtab, void *stream);

}  // namespace swmhd
