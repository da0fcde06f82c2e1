// Host-only argument layer of the C ABI (swmhd_api.hip, ring.hip, the host tails of output.hip, derived.hip, zonal.hip, spectra.hip and spectra2d.hip): what a valid halo-padded grid is,
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
    // a stencil of this radius finds its cells in every direction: in the halo, or, in the directions of `wrap`, in the periodic image
    bool halo_or_wrap(int radius, int wrap) const { return (Hx >= radius || (wrap & 1)) && (Hy >= radius || (wrap & 2)); }
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
// swmhd_output_fields, swmhd_derived_fields, swmhd_zonal_means, swmhd_zonal_spectra, swmhd_spectra2d: the diagnostics that read a frame
constexpr int FRAME_FLAGS = WRAP_FLAGS;
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
// swmhd_relaxation_rk3 and its ensemble form: radius 0, so neither the WRAP nor the Bounded flags mean anything to it; both are accepted,
// a direction with both its flags is an argument error as everywhere; SWMHD_RK3_ANCHOR as for the diffusion calls
constexpr int RELAXATION_FLAGS = SWMHD_STRICT | WRAP_FLAGS | BOUNDED_FLAGS | SWMHD_RK3_ANCHOR;
constexpr int RELAXATION_NOTSUP = KERNEL_FLAGS | SWMHD_GM_IS_PREV_STATE | OPEN_FLAGS | SWMHD_LEAVE_ROOM;
// swmhd_source_rk3 and its ensemble form take relaxation's flags: the WRAP flags say where the thickness one cell west or south of a
// row's cells is read (the periodic image, else the filled halo), the Bounded flags only that the direction is not wrapped
constexpr int SOURCE_FLAGS = RELAXATION_FLAGS;
constexpr int SOURCE_NOTSUP = RELAXATION_NOTSUP;
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

// ---- what the diagnostics that read a frame share (output.hip, derived.hip, zonal.hip, spectra.hip, spectra2d.hip) -----------------
// Every check here answers SWMHD_EINVAL, and every SWMHD_EINVAL check of those calls precedes their other answers (SWMHD_EHALO, then
// SWMHD_ENOTSUP, then "nothing to do"), so the order among these is not observable (tests/golden/*return_codes.json hold the rest).
// the four parents, the grid and the formulation
inline bool frame_source_ok(const void *q1, const void *q2, const void *h, const void *A, const Grid &g, int form) {
    return q1 && q2 && h && A && g.extents_ok() && g.spacing_ok() && formulation_ok(form);
}
// member count and member stride of the parents; none: a single grid
inline bool frame_members_ok(const Ens *ens, const Grid &g) {
    return !ens || (ens->members >= 1 && ens->members <= SWMHD_ENSEMBLE_MAX_MEMBERS && ens->stride_m >= g.min_member_stride());
}
// Two halo rules, each kept as it was: the frames, the derived frames and the zonal means ask for one halo cell whatever the wrap
// flags; the two spectra ask for it only in a direction that is not wrapped.  Both answer SWMHD_EHALO.
inline bool frame_halo_ok(const Grid &g) { return g.halo_at_least(1); }
inline bool spectra_halo_ok(const Grid &g, int flags) { return (g.Hx >= 1 || (flags & SWMHD_WRAP_X)) && (g.Hy >= 1 || (flags & SWMHD_WRAP_Y)); }
// a frame (swmhd_output_fields, swmhd_derived_fields): `which` fields of `elem`-byte elements at out; row, field and (ensembles) member
// stride in elements.  frame_ok: rows r of the fields of mask `all` fit it
struct Frame {
    int which;
    void *out;
    int elem;
    int64_t osy, osf, osm = 0;
};
inline bool frame_ok(const Frame &o, int all, const Grid &g, const Rows &r, const Ens *ens) {
    if (!o.out || !g.rows_ok(r.j0, r.j1) || o.which <= 0 || (o.which & ~all) || (o.elem != 4 && o.elem != 8)) return false;
    if (o.osy < g.Nx || o.osf < (int64_t)(r.j1 - r.j0) * o.osy) return false;
    return !ens || o.osm >= (int64_t)__builtin_popcount((unsigned)o.which) * o.osf;
}
// what OutArgs, DrvArgs, ZonalArgs, SpectraArgs and S2dArgs share: the parents at interior cell (1,1), extents, stride, spacings,
// formulation, mask, wrap bits and member stride
template <typename Args, typename T>
void set_frame_source(Args &a, const T *q1, const T *q2, const T *h, const T *A, const Grid &g, int form, int which, int flags, const Ens *ens) {
    a.q1 = g.interior(q1); a.q2 = g.interior(q2); a.h = g.interior(h); a.A = g.interior(A);
    a.Nx = g.Nx; a.Ny = g.Ny; a.sy = (long)g.sy;
    a.dx = g.dx; a.dy = g.dy;
    a.form = form; a.which = which;
    a.wrap = decode_flags(flags).wrap;
    a.stride_m = ens ? (long)ens->stride_m : 0;
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
