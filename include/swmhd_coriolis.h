/* BetaPlane Coriolis of the shallow-water MHD engine: part of the C ABI of include/swmhd.h, which includes this file (include that
 * one).  The entry points stand in a header of their own for the reason swmhd_zonal.h gives.  Symbols are added and none changed:
 * SWMHD_VERSION is unchanged. */
#ifndef SWMHD_CORIOLIS_H
#define SWMHD_CORIOLIS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * A Coriolis parameter that varies with y, f(y_j), through one RK3 stage, as a correction of what the stage kernel has written.  The
 * Coriolis term of the tendencies is additive and linear in f (G_u += f vbar, G_v -= f ubar; the same with uh, vh in the conservative
 * model), so the stage kernel is run with f = 0, where its own term is an exact no-op, and this call adds the term in full:
 *   vbar  = ((q2[i-1,j] + q2[i,j]) / 2 + (q2[i-1,j+1] + q2[i,j+1]) / 2) / 2       at (Face, Center), where q1 lives
 *   ubar  = ((q1[i,j-1] + q1[i+1,j-1]) / 2 + (q1[i,j] + q1[i+1,j]) / 2) / 2       at (Center, Face), where q2 lives
 *   D1    =   fc[j] vbar         fc[j] = f at the centre of row j
 *   D2    = -(ff[j] ubar)        ff[j] = f at the south face of row j
 *   q1_new += a D1,  q2_new += a D2                     a = dt gamma of the stage
 *   q1_acc += w D1,  q2_acc += w D2    where given      w = 1: acc is the stored tendency G^n (classic G- form)
 *                                                       w = dt/4: acc is the anchor W of SWMHD_RK3_ANCHOR's first stage
 * on the state the stage STARTED from (q1_old, q2_old).  Oceananigans' `coriolis = BetaPlane(f0, beta)` adds D to the tendency;
 * correcting new and the stored operand of the later stages reaches the same RK3 step up to rounding.
 *   strict (SWMHD_STRICT): every operation above rounded once, in the order written, no contraction: bitwise a numpy restatement.
 *   fast:   vbar = 0.25 ((. + .) + (. + .)) (the halvings are exact, so the same value), FMA allowed in the updates.  With
 *           S = (|.| + |.| + |.| + |.|) / 4 of the four values and eps the spacing of the element type at 1: every value goes through
 *           three roundings of at most eps/2 each before D stands (the sum of its pair, the sum of the pairs, the product with f):
 *           |D - D_exact| <= ((1 + eps/2)^3 - 1) |f| S <= 2 eps |f| S.  The update adds the rounding of a D where it is not fused and
 *           the rounding of the result: |new - ref| <= (eps/2) |ref| + ((1 + eps/2)^5 - 1) |a| |f| S for ref = new_0 + a D_exact, which
 *           is inside the bound the tests hold it to, |new - ref| <= eps |ref| + 4 eps |a| |f| S; the same for acc with w.  The strict
 *           order has the same count.
 * Pointers: DEVICE pointers to halo-padded parents (stride_y >= Nx + 2 Hx, as everywhere in swmhd.h).  q1_acc and q2_acc are both NULL
 * or both given.  frow: a DEVICE table of 2 Ny values in the element type, fc[0 .. Ny) then ff[0 .. Ny); it is not checked.  Only the
 * interior cells of rows [j_begin, j_end) of new and acc are written; old is read there and one cell around: with SWMHD_WRAP_X /
 * SWMHD_WRAP_Y the periodic image (x mod Nx, y mod Ny) of the interior -- the fused stages leave the halos stale -- and without the
 * flag a filled halo of depth >= 1.  Bounded directions need no body of their own: the filled halo carries the wall, and the wall
 * line of the wall-normal velocity, which this call writes like any other, is reset by the boundary-condition fill that follows
 * every Bounded stage (swmhd_fill_halo).
 * Bytes per cell and stage (fp64): 8 + 8 read of old, (8 + 8) x 2 of new: 48; with acc 80.
 * Flags: SWMHD_STRICT, SWMHD_WRAP_X, SWMHD_WRAP_Y, SWMHD_RK3_ANCHOR (read by the ensemble call with `params` only, see there);
 * SWMHD_BOUNDED_X / _Y are accepted and mean only that the direction is not wrapped.
 * Checks, in this order, every one before the first HIP call:
 *   SWMHD_EINVAL   a null old, new or frow; one acc without the other; bad extents, pitch or rows (0 <= j_begin <= j_end <= Ny);
 *                  unknown flag bits, or SWMHD_BOUNDED and SWMHD_WRAP of one direction together; an output equal to an input or to
 *                  another output; a or w not finite; (ensembles) members outside 1 .. SWMHD_ENSEMBLE_MAX_MEMBERS, stride_m <
 *                  (Ny + 2 Hy) stride_y.
 *   SWMHD_ENOTSUP  SWMHD_TILE_KERNEL, SWMHD_MARCH_KERNEL, SWMHD_GM_IS_PREV_STATE, SWMHD_OPEN_SOUTH / _NORTH, SWMHD_LEAVE_ROOM.
 *   SWMHD_EHALO    halo < 1 in a direction without the WRAP flag of that direction.
 * An empty row range enqueues nothing.
 * Launch: one plain launch, no atomics, no LDS, no hand-off between workgroups; it captures into a graph.  A wave marches down
 * SWMHD_CORIOLIS_TILE_ROWS / 4 rows of a strip of 64 lanes; a lane holds 16 bytes of a row (2 doubles, 4 floats) where all six parents
 * have the same 16-byte phase and stride_y (and stride_m) keep it, else one element.
 *
 * Ensembles: swmhd_ensemble_coriolis_rk3_* does the same for `members` copies, member m of every parent at ptr + m * stride_m
 * (elements) and its table at frow + m * 2 Ny.  params == NULL: a and w as above for every member.  params != NULL: the DEVICE table of
 * members x (g, f, dt) of the swmhd_ensemble_*_params calls (f is not read); then `a` is taken as gamma and the kernel forms
 * a_m = dt_m gamma, and with SWMHD_RK3_ANCHOR `w` is taken as the anchor's weight and w_m = dt_m w (without the flag w_m = w).
 * ---------------------------------------------------------------------------------------------- */
#define SWMHD_CORIOLIS_TILE_ROWS 64
int swmhd_coriolis_rk3_f64(const double *q1_old, const double *q2_old, double *q1_new, double *q2_new, double *q1_acc, double *q2_acc,
                           const double *frow, int Nx, int Ny, int Hx, int Hy, int64_t stride_y, double a, double w,
                           int j_begin, int j_end, int flags, void *stream);
int swmhd_coriolis_rk3_f32(const float *q1_old, const float *q2_old, float *q1_new, float *q2_new, float *q1_acc, float *q2_acc,
                           const float *frow, int Nx, int Ny, int Hx, int Hy, int64_t stride_y, float a, float w,
                           int j_begin, int j_end, int flags, void *stream);
int swmhd_ensemble_coriolis_rk3_f64(const double *q1_old, const double *q2_old, double *q1_new, double *q2_new, double *q1_acc,
                                    double *q2_acc, const double *frow, int members, int64_t stride_m, int Nx, int Ny, int Hx, int Hy,
                                    int64_t stride_y, const double *params, double a, double w, int j_begin, int j_end, int flags,
                                    void *stream);
int swmhd_ensemble_coriolis_rk3_f32(const float *q1_old, const float *q2_old, float *q1_new, float *q2_new, float *q1_acc,
                                    float *q2_acc, const float *frow, int members, int64_t stride_m, int Nx, int Ny, int Hx, int Hy,
                                    int64_t stride_y, const float *params, float a, float w, int j_begin, int j_end, int flags,
                                    void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SWMHD_CORIOLIS_H */
