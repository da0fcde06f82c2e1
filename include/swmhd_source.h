/* Static sources of the shallow-water MHD engine -- bathymetry and steady body forces: part of the C ABI of include/swmhd.h, which
 * includes this file (include that one).  The entry points stand in a header of their own for the reason swmhd_zonal.h gives.  Symbols
 * are added and none changed: SWMHD_VERSION is unchanged. */
#ifndef SWMHD_SOURCE_H
#define SWMHD_SOURCE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * A field that does not change in time, added to the tendency of a list of fields through one RK3 stage, as a correction of what the
 * stage kernels have written.  Per field k that has a source and interior cell, on the state the stage STARTED from:
 *   kind_k = SWMHD_SOURCE_PLAIN (0):   D = S_k[i,j]
 *   kind_k = SWMHD_SOURCE_X_FACE (1):  D = ((h_old[i-1,j] + h_old[i,j]) / 2) S_k[i,j]
 *   kind_k = SWMHD_SOURCE_Y_FACE (2):  D = ((h_old[i,j-1] + h_old[i,j]) / 2) S_k[i,j]
 *   new_k   += a D                                   a = dt gamma of the stage
 *   acc_k   += w D        where acc_k is given       w as in swmhd_relaxation.h (1: the stored tendency; dt/4: the anchor W)
 * h_old = old[thickness], `thickness` an index into the call's field list, or -1 where no field has kind 1 or 2.  (x + y) / 2 is the
 * interpolation of the stage kernels to a face.  The vector-invariant model forces u, v, h, A and tracers with kind 0; the conservative
 * model forces uh with kind 1 and vh with kind 2, so that S is an acceleration there too, and h goes along as the thickness.
 * nfields = 1 .. SWMHD_SOURCE_MAX_FIELDS (= 4 + SWMHD_MAX_TRACERS).
 *
 * Bathymetry is this term: with the bottom b at the cell centres the host hands over S_u = F_u - g (b[i,j] - b[i-1,j]) / dx (S_v
 * likewise with dy; F a body force or 0).  Under kind 1 / 2 the force on uh is g (h[i-1] + h[i]) / 2 (b[i] - b[i-1]) / dx.  This
 * INTERPOLATED form is a decision: the conservative stage kernel forms the pressure force as the difference of g h^2 / 2, which is
 * exactly g (h[i-1] + h[i]) / 2 (h[i] - h[i-1]) / dx, so only the interpolated thickness keeps a lake at rest (h + b constant, no
 * flow) at rest to rounding.  g h[i,j] (b[i] - b[i-1]) / dx, which some Oceananigans releases are believed to use, leaves a tenth of
 * the unbalanced force (tests/test_source_cases_cpu.py measures both).
 *
 *   strict (SWMHD_STRICT): every operation above rounded once, in the order written, no contraction: bitwise a numpy restatement.
 *   fast:   the same expression; the compiler may fuse a D + new (and w D + acc) into one FMA.  With eps the spacing of the element
 *           type at 1 and ref = new_0 + a D_exact:
 *             kind 0: D is a load and has no rounding; the update rounds a D (where not fused) and the sum: 2 roundings,
 *                     |new - ref| <= (eps/2) |ref| + ((1 + eps/2)^1 - 1) (1 + eps/2) |a| |S|;
 *             kind 1, 2: the sum of the two h (the halving is exact), the product with S, then the update: 4 roundings, 3 where fused,
 *                     |new - ref| <= (eps/2) |ref| + ((1 + eps/2)^3 - 1) (1 + eps/2) |a| M,  M = ((|h_w| + |h|) / 2) |S|.
 *           Both are inside the bound the tests hold the fast result to, with n = 2 (kind 0) and n = 4 (kind 1, 2):
 *             |new - ref| <= eps |ref| + ((1 + eps/2)^n - 1) |a| M      (M = |S| for kind 0); the same for acc with w.
 *           The strict order has the same count.
 * Pointers: old, new, acc, source are HOST arrays of nfields DEVICE pointers to halo-padded parents (stride_y >= Nx + 2 Hx, as
 * everywhere in swmhd.h); a source has the Hx, Hy and stride_y of the fields, and its halo cells are never read.  kind: a HOST array of
 * nfields values.  acc may be NULL (no field has one), and so may any acc[k] and any source[k].
 * A field with source[k] == NULL is neither read nor written -- except old[thickness], which is read as h_old whether or not that
 * field has a source of its own.
 * What is read: source, new and acc at the interior cells of rows [j_begin, j_end), nothing of old but h_old; h_old at those cells and,
 * where a field of kind 1 is live, one cell west of them, where a field of kind 2 is live, one cell south.  With SWMHD_WRAP_X / _Y that
 * cell is the periodic image (the fused stages leave the halos stale); without the flag it is the halo cell, which must be filled.
 * Bounded directions need no body of their own: their filled halo is read like any other, and S is 0 on a wall line.
 * Bytes per cell, field and stage (fp64): 8 read of S, 8 + 8 of new: 24; + 8 of h_old for kind 1 or 2 (the west cell comes from the
 * neighbouring lane, the row to the south is carried down the march); + 16 with acc.
 * Flags: SWMHD_STRICT, SWMHD_WRAP_X / _Y, SWMHD_RK3_ANCHOR (read by the ensemble call with `params` only, see there); SWMHD_BOUNDED_X /
 * _Y are accepted and say only that the direction is not wrapped.
 * Checks, in this order, every one before the first HIP call:
 *   SWMHD_EINVAL   null old / new / source / kind, nfields outside 1 .. SWMHD_SOURCE_MAX_FIELDS; bad extents, pitch or rows
 *                  (0 <= j_begin <= j_end <= Ny); unknown flag bits, or SWMHD_BOUNDED and SWMHD_WRAP of one direction together; a null
 *                  old[k] or new[k]; new[k] or acc[k] equal to any old[m] or source[m], or to another output; a or w not finite;
 *                  then a kind[k] outside 0 .. 2; thickness outside -1 .. nfields - 1; thickness == -1 while a field with a source has
 *                  kind 1 or 2.
 *   SWMHD_ENOTSUP  SWMHD_TILE_KERNEL, SWMHD_MARCH_KERNEL, SWMHD_GM_IS_PREV_STATE, SWMHD_OPEN_SOUTH / _NORTH, SWMHD_LEAVE_ROOM (the flags
 *                  swmhd_relaxation_rk3_* refuses).
 *   SWMHD_EHALO    a field with a source has kind 1 or 2, and Hx < 1 without SWMHD_WRAP_X or Hy < 1 without SWMHD_WRAP_Y (as
 *                  swmhd_coriolis_rk3_*).  A call of plain fields accepts a halo of depth 0.
 * An empty row range, or sources that are all NULL, enqueue nothing.
 * Launch: one plain launch for all fields, no atomics, no LDS, no hand-off between workgroups; it captures into a graph.  A wave
 * marches down SWMHD_SOURCE_TILE_ROWS / 4 rows of a strip of 64 lanes, the loads of a row's streams issued one row ahead of its
 * arithmetic; a lane holds 16 bytes of a row (2 doubles, 4 floats) where all parents of the call, sources included, have the same
 * 16-byte phase and stride_y (and the member strides) keep it, else one element.
 *
 * Ensembles: swmhd_ensemble_source_rk3_* does the same for `members` copies, member m of every field parent at ptr + m * stride_m
 * (elements) and of every source at ptr + m * source_stride_m; source_stride_m == 0 is one array shared by all members.  params, a, w
 * and SWMHD_RK3_ANCHOR exactly as in swmhd_ensemble_relaxation_rk3_*: params == NULL: a and w as above for every member; params !=
 * NULL: the DEVICE table of members x (g, f, dt); then `a` is taken as gamma and the kernel forms a_m = dt_m gamma, and with
 * SWMHD_RK3_ANCHOR w_m = dt_m w (without the flag w_m = w).  Further SWMHD_EINVAL: members outside 1 .. SWMHD_ENSEMBLE_MAX_MEMBERS,
 * stride_m < (Ny + 2 Hy) stride_y, source_stride_m neither 0 nor >= (Ny + 2 Hy) stride_y -- checked with the first group.
 * ---------------------------------------------------------------------------------------------- */
#define SWMHD_SOURCE_MAX_FIELDS 12
#define SWMHD_SOURCE_TILE_ROWS 64
#define SWMHD_SOURCE_PLAIN 0
#define SWMHD_SOURCE_X_FACE 1
#define SWMHD_SOURCE_Y_FACE 2
int swmhd_source_rk3_f64(const double *const *old, double *const *new_, double *const *acc, const double *const *source, const int *kind,
                         int nfields, int thickness, int Nx, int Ny, int Hx, int Hy, int64_t stride_y, double a, double w, int j_begin,
                         int j_end, int flags, void *stream);
int swmhd_source_rk3_f32(const float *const *old, float *const *new_, float *const *acc, const float *const *source, const int *kind,
                         int nfields, int thickness, int Nx, int Ny, int Hx, int Hy, int64_t stride_y, float a, float w, int j_begin,
                         int j_end, int flags, void *stream);
int swmhd_ensemble_source_rk3_f64(const double *const *old, double *const *new_, double *const *acc, const double *const *source,
                                  const int *kind, int nfields, int thickness, int members, int64_t stride_m, int64_t source_stride_m,
                                  int Nx, int Ny, int Hx, int Hy, int64_t stride_y, const double *params, double a, double w, int j_begin,
                                  int j_end, int flags, void *stream);
int swmhd_ensemble_source_rk3_f32(const float *const *old, float *const *new_, float *const *acc, const float *const *source,
                                  const int *kind, int nfields, int thickness, int members, int64_t stride_m, int64_t source_stride_m,
                                  int Nx, int Ny, int Hx, int Hy, int64_t stride_y, const float *params, float a, float w, int j_begin,
                                  int j_end, int flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SWMHD_SOURCE_H */
