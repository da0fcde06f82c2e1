/* Lagrangian particles of the shallow-water MHD engine: part of the C ABI of include/swmhd.h, which includes this file (include that
 * one).  The entry points stand in a header of their own for the reason swmhd_zonal.h gives.  Symbols are added and none changed:
 * SWMHD_VERSION is unchanged. */
#ifndef SWMHD_PARTICLES_H
#define SWMHD_PARTICLES_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * P particles advected by the flow through one RK3 stage: their positions are one more prognostic of the same RK3.  The tendency of a
 * position is the velocity there, evaluated from the state the stage STARTED from at the position the stage started from (as the
 * tracers' is).  Per particle, with the stage's (gamma, zeta):
 *   G   = (U(x, y), V(x, y))                 bilinear, below
 *   x  += dt (gamma Gx + zeta Gx-)           y likewise; then the fold, below
 *   G- <- G                                  gx, gy: two doubles per particle
 * With zeta == 0 (stage 1) G- is not read: it may hold anything, NaN included.  Third order along the path.  Oceananigans steps its
 * LagrangianParticles forward-Euler per substep with (gamma + zeta) dt, which is not third order along the path; the scheme here
 * differs so that the drift of A read along a trajectory measures the resistivity of the field scheme and not the particles' own error.
 * Positions and G- are float64 whatever the element type of the fields; field values are read in the element type and widened; all
 * arithmetic is in double, every operation rounded once in the order written, no contraction, IEEE divide.  There is ONE body: the
 * kernel is bound by the latency of its gathers, so it has no fast variant; SWMHD_STRICT is accepted and changes nothing, and the
 * results are bitwise a numpy restatement (tests/particle_cases.py) in strict and fast models alike.
 *
 * Node velocities (the grid's own xf / yc and xc / yf): U[i,j] at (x0 + i dx, y0 + (j + 1/2) dy), V[i,j] at (x0 + (i + 1/2) dx,
 * y0 + j dy).  formulation SWMHD_VECTOR_INVARIANT: q1, q2 themselves (h is not read and may be NULL).  SWMHD_CONSERVATIVE: U[i,j] =
 * q1[i,j] / (0.5 (h[i-1,j] + h[i,j])), V[i,j] = q2[i,j] / (0.5 (h[i,j-1] + h[i,j])): the frames' velocities, operand for operand.
 *
 * Interpolation, written for a field at (Face, Center) as U is; Center in x subtracts 0.5 from sx as well, Face in y does not from sy:
 *   sx = (x - x0) / dx,        i = floor(sx), tx = sx - i
 *   sy = (y - y0) / dy - 0.5,  j = floor(sy), ty = sy - j
 *   U  = (1 - ty) ((1 - tx) U[i,j] + tx U[i+1,j]) + ty ((1 - tx) U[i,j+1] + tx U[i+1,j+1])
 * Indices.  A direction with SWMHD_WRAP_X / _Y: the index is the true modulus i mod Nx, formed in floating point (fmod of floor(sx),
 * made non-negative) BEFORE any conversion to an integer, and i + 1 wraps to 0; only interior cells are read (the fused stages leave
 * the halos stale); grids 1 to 3 cells wide are right.  A direction without the flag: the parent is read as it is and needs a filled
 * halo of depth >= 1; floor(sx) is clamped, in floating point, to [-Hx, Nx + Hx - 2], so i and i + 1 stay inside the parent (tx is
 * that of the unclamped sx); the h west (south) of a node is read at max(i - 1, -Hx).  So every finite position, 1e300 included, gives
 * in-range addresses.  A particle with a non-finite coordinate is not read, not advanced and not written, nor is its G-; no address is
 * formed from it.
 * The fold after the update, with Lx = Nx dx (one rounding) and hi = x0 + Lx:
 *   a direction without SWMHD_BOUNDED_X / _Y (Periodic):  x -= Lx floor((x - x0) / Lx)
 *   a direction with it:  one reflection at the wall crossed, x < x0: x = 2 x0 - x;  x > hi: x = 2 hi - x
 *   then, in both, a clamp into [x0, hi] (x < x0 ? x0 : x > hi ? hi : x, which leaves a NaN a NaN).
 * SWMHD_BOUNDED_X / _Y mean only this: "not wrapped, reflect" (the filled halo carries the wall, as for swmhd_coriolis_rk3_*).
 * Bytes per particle and stage (fp64 fields, vector-invariant): 8 gathers of 8 B = 64 B, and 64 B of x, y, G- traffic (16 read and 16
 * written of x, y; 16 read and 16 written of G-), 48 B where zeta == 0.  Conservative: 20 gathers (8 of q, 12 of h: neighbouring
 * nodes share theirs).  A gather is element-granular and uncoalesced; it rests on L2 and the Infinity Cache.
 *
 * x, y, gx, gy: DEVICE arrays of P doubles, updated in place.  q1, q2, h: halo-padded parents (stride_y >= Nx + 2 Hx, as everywhere in
 * swmhd.h).  Flags: SWMHD_STRICT, SWMHD_WRAP_X / _Y, SWMHD_BOUNDED_X / _Y.
 * Checks, in this order, every one before the first HIP call:
 *   SWMHD_EINVAL   null q1, q2, x, y, gx or gy, or two of x, y, gx, gy the same; bad extents or pitch; dx, dy not > 0 or x0, y0 not
 *                  finite; unknown flag bits, or SWMHD_BOUNDED and SWMHD_WRAP of one direction together; P < 0; dt, gamma or zeta
 *                  not finite; an unknown formulation; h NULL for SWMHD_CONSERVATIVE; (ensembles) members outside
 *                  1 .. SWMHD_ENSEMBLE_MAX_MEMBERS, stride_m < (Ny + 2 Hy) stride_y.
 *   SWMHD_ENOTSUP  SWMHD_TILE_KERNEL, SWMHD_MARCH_KERNEL, SWMHD_GM_IS_PREV_STATE, SWMHD_OPEN_SOUTH / _NORTH, SWMHD_LEAVE_ROOM,
 *                  SWMHD_RK3_ANCHOR (positions have no anchor form: they always take the stage's own gamma and zeta).
 *   SWMHD_EHALO    Hx < 1 without SWMHD_WRAP_X, or Hy < 1 without SWMHD_WRAP_Y.
 * P == 0 enqueues nothing.  2^31 workgroups (of SWMHD_PARTICLES_BLOCK particles each, times members) or more are refused with the
 * negated HIP error of an invalid configuration.
 * Launch: one plain launch, one lane per particle, no atomics, no LDS, no hand-off between workgroups; it captures into a graph.  All
 * gathers of a particle are issued before anything waits on them.
 *
 * Ensembles: swmhd_ensemble_particles_rk3_* does the same for `members` copies: member m of the fields at ptr + m * stride_m
 * (elements), member m of x, y, gx, gy is row m of dense (members, P) arrays.  params == NULL: dt as above for every member.  params !=
 * NULL: the DEVICE table of members x (g, f, dt) of the swmhd_ensemble_*_params calls, in the fields' element type; then dt is taken as
 * 1 and member m steps with dt_m from the table (widened to double), as the sibling corrections do.
 * ---------------------------------------------------------------------------------------------- */
#define SWMHD_PARTICLES_BLOCK 256
int swmhd_particles_rk3_f64(const double *q1, const double *q2, const double *h, double *x, double *y, double *gx, double *gy, int64_t P,
                            int Nx, int Ny, int Hx, int Hy, int64_t stride_y, double x0, double y0, double dx, double dy, int formulation,
                            double dt, double gamma, double zeta, int flags, void *stream);
int swmhd_particles_rk3_f32(const float *q1, const float *q2, const float *h, double *x, double *y, double *gx, double *gy, int64_t P,
                            int Nx, int Ny, int Hx, int Hy, int64_t stride_y, double x0, double y0, double dx, double dy, int formulation,
                            double dt, double gamma, double zeta, int flags, void *stream);
int swmhd_ensemble_particles_rk3_f64(const double *q1, const double *q2, const double *h, double *x, double *y, double *gx, double *gy,
                                     int64_t P, int members, int64_t stride_m, int Nx, int Ny, int Hx, int Hy, int64_t stride_y, double x0,
                                     double y0, double dx, double dy, int formulation, const double *params, double dt, double gamma,
                                     double zeta, int flags, void *stream);
int swmhd_ensemble_particles_rk3_f32(const float *q1, const float *q2, const float *h, double *x, double *y, double *gx, double *gy,
                                     int64_t P, int members, int64_t stride_m, int Nx, int Ny, int Hx, int Hy, int64_t stride_y, double x0,
                                     double y0, double dx, double dy, int formulation, const float *params, double dt, double gamma,
                                     double zeta, int flags, void *stream);

/* ------------------------------------------------------------------------------------------------
 * tracked_fields: nfields parents interpolated to the particle positions, out[k, p] = field k at (x[p], y[p]), float64, dense
 * (nfields, P); for an ensemble (members, nfields, P).  fields: a HOST array of nfields DEVICE pointers to parents; loc: a HOST array
 * of nfields location codes, SWMHD_PARTICLES_CENTER_X (1) | SWMHD_PARTICLES_CENTER_Y (2), a bit clear meaning Face in that direction
 * (u: 2, v: 1, h, A and tracers: 3).  The fields are interpolated as they are stored (uh is uh).  Interpolation and index rules are
 * those of the stage; nothing is folded; a particle with a non-finite coordinate samples as NaN.  Flags: SWMHD_STRICT, SWMHD_WRAP_X /
 * _Y, SWMHD_BOUNDED_X / _Y (not wrapped; nothing else to the sampler).
 * Checks, in this order, every one before the first HIP call:
 *   SWMHD_EINVAL   null fields, loc, x, y or out, nfields outside 1 .. SWMHD_PARTICLES_MAX_FIELDS, a null fields[k], a loc[k]
 *                  outside 0 .. 3; bad extents or pitch; dx, dy not > 0 or x0, y0 not finite; unknown flag bits, or SWMHD_BOUNDED and
 *                  SWMHD_WRAP of one direction together; P < 0; (ensembles) members and stride_m as above.
 *   SWMHD_ENOTSUP, SWMHD_EHALO   as above.
 * P == 0 enqueues nothing; the launch is the stage's: one lane per particle, the four gathers of a field issued together.
 * ---------------------------------------------------------------------------------------------- */
#define SWMHD_PARTICLES_MAX_FIELDS 12
#define SWMHD_PARTICLES_CENTER_X 1
#define SWMHD_PARTICLES_CENTER_Y 2
int swmhd_particles_sample_f64(const double *const *fields, const int *loc, int nfields, const double *x, const double *y, double *out,
                               int64_t P, int Nx, int Ny, int Hx, int Hy, int64_t stride_y, double x0, double y0, double dx, double dy,
                               int flags, void *stream);
int swmhd_particles_sample_f32(const float *const *fields, const int *loc, int nfields, const double *x, const double *y, double *out,
                               int64_t P, int Nx, int Ny, int Hx, int Hy, int64_t stride_y, double x0, double y0, double dx, double dy,
                               int flags, void *stream);
int swmhd_ensemble_particles_sample_f64(const double *const *fields, const int *loc, int nfields, const double *x, const double *y,
                                        double *out, int64_t P, int members, int64_t stride_m, int Nx, int Ny, int Hx, int Hy,
                                        int64_t stride_y, double x0, double y0, double dx, double dy, int flags, void *stream);
int swmhd_ensemble_particles_sample_f32(const float *const *fields, const int *loc, int nfields, const double *x, const double *y,
                                        double *out, int64_t P, int members, int64_t stride_m, int Nx, int Ny, int Hx, int Hy,
                                        int64_t stride_y, double x0, double y0, double dx, double dy, int flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SWMHD_PARTICLES_H */
