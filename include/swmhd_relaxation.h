/* Relaxation forcing of the shallow-water MHD engine: part of the C ABI of include/swmhd.h, which includes this file (include that
 * one).  The entry points stand in a header of their own for the reason swmhd_zonal.h gives.  Symbols are added and none changed:
 * SWMHD_VERSION is unchanged. */
#ifndef SWMHD_RELAXATION_H
#define SWMHD_RELAXATION_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * Linear relaxation of a list of fields through one RK3 stage, as a correction of what the stage kernels have written.  Per field k
 * and interior cell, on the state the stage STARTED from:
 *   p        = rate_k mask_k[i,j]                    mask_k NULL: p = rate_k
 *   d        = t - old_k[i,j]                        t = target_k[i,j]; target_k NULL: t = tval_k
 *   D        = p d
 *   new_k   += a D                                   a = dt gamma of the stage
 *   acc_k   += w D        where acc_k is given       w = 1: acc is the stored tendency G^n (classic G- form)
 *                                                    w = dt/4: acc is the anchor W of SWMHD_RK3_ANCHOR's first stage
 * Oceananigans' `forcing = (u = Relaxation(rate, mask, target), ...)` adds rate * mask(x, y) * (target(x, y) - phi) to the tendency G
 * of the field; correcting new and the stored operand of the later stages reaches the same RK3 step up to rounding.  Drag (no mask,
 * target 0), sponge layers (a mask) and Newtonian relaxation of h (a target array) are this one term.  The term has radius 0, so u, v,
 * h, A and the tracers go through one launch: nfields = 1 .. SWMHD_RELAXATION_MAX_FIELDS (= 4 + SWMHD_MAX_TRACERS).
 *   strict (SWMHD_STRICT): every operation above rounded once, in the order written, no contraction: Oceananigans' rate * mask *
 *           (target - phi) evaluated left to right, bitwise a numpy restatement.
 *   fast:   the same expression; the compiler may fuse a D + new (and w D + acc) into one FMA.  With S = |rate| |mask| (|t| + |old|) and
 *           eps the spacing of the element type at 1: D takes three roundings of at most eps/2 each (p, d, their product), so
 *           |D - D_exact| <= ((1 + eps/2)^3 - 1) S <= 2 eps S.  The update adds the rounding of a D where it is not fused and the
 *           rounding of the result -- five roundings in all, four where fused, the chain swmhd_coriolis.h counts:
 *           |new - ref| <= (eps/2) |ref| + ((1 + eps/2)^5 - 1) |a| S for ref = new_0 + a D_exact, which is inside the bound the tests
 *           hold it to, |new - ref| <= eps |ref| + 4 eps |a| S; the same for acc with w.  The strict order has the same count.
 * Pointers: old, new, acc, mask, target are HOST arrays of nfields DEVICE pointers to halo-padded parents (stride_y >= Nx + 2 Hx, as
 * everywhere in swmhd.h); masks and targets have the Hx, Hy and stride_y of the fields.  acc, mask and target may be NULL (no field has
 * one), and so may any acc[k], mask[k], target[k].  rate, tval: HOST arrays of nfields values; tval[k] is read where target[k] is NULL.
 * Only the interior cells of rows [j_begin, j_end) are read (old, mask, target) and written (new, acc): no halo cell of any parent is
 * read, so Bounded grids need no body of their own -- the wall line of the wall-normal velocity, which this call writes like any
 * other, is reset by the boundary-condition fill that follows every Bounded stage (swmhd_fill_halo).
 * A field with rate == 0 is neither read nor written.
 * Bytes per cell, field and stage (fp64): 8 read of old, 8 + 8 of new: 24; +8 with a mask, +8 with a target array, +16 with acc: <= 56.
 * Flags: SWMHD_STRICT, SWMHD_RK3_ANCHOR (read by the ensemble call with `params` only, see there); SWMHD_WRAP_X / _Y and
 * SWMHD_BOUNDED_X / _Y are accepted and mean nothing here.
 * Checks, in this order, every one before the first HIP call:
 *   SWMHD_EINVAL   null old / new / rate / tval, nfields outside 1 .. SWMHD_RELAXATION_MAX_FIELDS; bad extents, pitch or rows
 *                  (0 <= j_begin <= j_end <= Ny); unknown flag bits, or SWMHD_BOUNDED and SWMHD_WRAP of one direction together; a null
 *                  old[k] or new[k]; new[k] or acc[k] equal to any old[m], mask[m] or target[m], or to another output; a rate that is
 *                  negative or not finite, a tval that is not finite; a or w not finite.
 *   SWMHD_ENOTSUP  SWMHD_TILE_KERNEL, SWMHD_MARCH_KERNEL, SWMHD_GM_IS_PREV_STATE, SWMHD_OPEN_SOUTH / _NORTH, SWMHD_LEAVE_ROOM.
 * There is no SWMHD_EHALO: a halo of depth 0 is accepted.
 * An empty row range, or rates that are all 0, enqueue nothing.
 * Launch: one plain launch, no atomics, no LDS, no hand-off between workgroups; it captures into a graph.  A wave marches down
 * SWMHD_RELAXATION_TILE_ROWS / 4 rows of a strip of 64 lanes, the loads of a row's streams issued one row ahead of its arithmetic; a
 * lane holds 16 bytes of a row (2 doubles, 4 floats) where all parents of the call, masks and targets included, have the same 16-byte
 * phase and stride_y (and the member strides) keep it, else one element.
 *
 * Ensembles: swmhd_ensemble_relaxation_rk3_* does the same for `members` copies, member m of every field parent at ptr + m * stride_m
 * (elements), of every mask at ptr + m * mask_stride_m and of every target at ptr + m * target_stride_m; a stride of 0 is one array
 * shared by all members.  rate and tval are DEVICE tables, [m * nfields + k]; they are not checked, and a zero rate skips that field of
 * that member.  params == NULL: a and w as above for every member.  params != NULL: the DEVICE table of members x (g, f, dt) of the
 * swmhd_ensemble_*_params calls; then `a` is taken as gamma and the kernel forms a_m = dt_m gamma, and with SWMHD_RK3_ANCHOR `w` is
 * taken as the anchor's weight and w_m = dt_m w (without the flag w_m = w).  Further SWMHD_EINVAL: members outside 1 ..
 * SWMHD_ENSEMBLE_MAX_MEMBERS, stride_m < (Ny + 2 Hy) stride_y, mask_stride_m or target_stride_m neither 0 nor >= (Ny + 2 Hy) stride_y
 * -- all checked first.
 * ---------------------------------------------------------------------------------------------- */
#define SWMHD_RELAXATION_MAX_FIELDS 12
#define SWMHD_RELAXATION_TILE_ROWS 64
int swmhd_relaxation_rk3_f64(const double *const *old, double *const *new_, double *const *acc, const double *const *mask,
                             const double *const *target, const double *rate, const double *tval, int nfields, int Nx, int Ny, int Hx,
                             int Hy, int64_t stride_y, double a, double w, int j_begin, int j_end, int flags, void *stream);
int swmhd_relaxation_rk3_f32(const float *const *old, float *const *new_, float *const *acc, const float *const *mask,
                             const float *const *target, const float *rate, const float *tval, int nfields, int Nx, int Ny, int Hx,
                             int Hy, int64_t stride_y, float a, float w, int j_begin, int j_end, int flags, void *stream);
int swmhd_ensemble_relaxation_rk3_f64(const double *const *old, double *const *new_, double *const *acc, const double *const *mask,
                                      const double *const *target, const double *rate, const double *tval, int nfields, int members,
                                      int64_t stride_m, int64_t mask_stride_m, int64_t target_stride_m, int Nx, int Ny, int Hx, int Hy,
                                      int64_t stride_y, const double *params, double a, double w, int j_begin, int j_end, int flags,
                                      void *stream);
int swmhd_ensemble_relaxation_rk3_f32(const float *const *old, float *const *new_, float *const *acc, const float *const *mask,
                                      const float *const *target, const float *rate, const float *tval, int nfields, int members,
                                      int64_t stride_m, int64_t mask_stride_m, int64_t target_stride_m, int Nx, int Ny, int Hx, int Hy,
                                      int64_t stride_y, const float *params, float a, float w, int j_begin, int j_end, int flags,
                                      void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SWMHD_RELAXATION_H */
