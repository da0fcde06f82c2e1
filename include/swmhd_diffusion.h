/* ScalarDiffusivity closure of the shallow-water MHD engine: part of the C ABI of include/swmhd.h, which includes this file (include
 * that one).  The entry points stand in a header of their own for the reason swmhd_zonal.h gives.  Symbols are added and none changed:
 * SWMHD_VERSION is unchanged. */
#ifndef SWMHD_DIFFUSION_H
#define SWMHD_DIFFUSION_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * Laplacian diffusion of a list of fields through one RK3 stage, as a correction of what the stage kernels have written:
 *   D_k      = coef_k laplace(old_k)                 on the state the stage STARTED from
 *   new_k   += a D_k                                 a = dt gamma of the stage
 *   acc_k   += w D_k      where acc_k is given       w = 1: acc is the stored tendency G^n (classic G- form)
 *                                                    w = dt/4: acc is the anchor W of SWMHD_RK3_ANCHOR's first stage
 * Oceananigans' `closure = ScalarDiffusivity(nu = ..., kappa = ...)` adds D to the tendency G of the field; correcting new and the stored
 * operand of the later stages reaches the same RK3 step up to rounding.  On the uniform periodic grid the operator is the same at faces
 * and centres, so u, v, A and the tracers go through one launch: nfields = 1 .. SWMHD_DIFFUSION_MAX_FIELDS (= 3 + SWMHD_MAX_TRACERS).
 *   strict (SWMHD_STRICT): Fx_i = c ((phi_i - phi_{i-1}) / dx), Fy_j likewise, D = (Fx_{i+1} - Fx_i) / dx + (Fy_{j+1} - Fy_j) / dy; then
 *           new + a D and acc + w D, every operation rounded once, IEEE divides.
 *   fast:   D = (c rdx2) ((phi_e + phi_w) - 2 phi) + (c rdy2) ((phi_n + phi_s) - 2 phi), rdx2 = 1 / (dx dx); FMA allowed.  With
 *           S = |c|/dx^2 (|phi_e| + 2 |phi| + |phi_w|) + |c|/dy^2 (|phi_n| + 2 |phi| + |phi_s|) and eps the spacing of the element type
 *           at 1:  |D - D_exact| <= 8 eps S  (seven roundings: three in c rdx2, the neighbours' sum, the difference, the product, the last
 *           sum), |new - (new_0 + a D_exact)| <= eps |.| + 10 eps |a| S, and the same for acc with w.
 * Pointers: old, new, acc are HOST arrays of nfields DEVICE pointers to halo-padded parents (stride_y >= Nx + 2 Hx, as everywhere in
 * swmhd.h).  acc may be NULL (no field has one), and so may any acc[k].  Only the interior cells of rows [j_begin, j_end) of new and acc
 * are written; `old` is read there and one cell around: with SWMHD_WRAP_X / SWMHD_WRAP_Y the periodic image (x mod Nx, y mod Ny) instead
 * of the halo cell -- the fused stages leave the halos stale -- and without the flag a filled halo of depth >= 1.
 * coef: a HOST array of nfields values.  A field with coef == 0 is neither read nor written.
 * Bytes per cell, field and stage (fp64): 8 read of old, 8 + 8 of new: 24; with acc 40.
 * Flags: SWMHD_STRICT, SWMHD_WRAP_X, SWMHD_WRAP_Y, SWMHD_RK3_ANCHOR (read by the ensemble call with `params` only, see there).
 * Checks, in this order, every one before the first HIP call:
 *   SWMHD_EINVAL   null old / new / coef, nfields outside 1 .. SWMHD_DIFFUSION_MAX_FIELDS; bad extents, pitch, spacing or rows
 *                  (0 <= j_begin <= j_end <= Ny); unknown flag bits; a null old[k] or new[k]; new[k] or acc[k] equal to any old[m], or
 *                  to another output; a coefficient that is negative or not finite; a or w not finite.
 *   SWMHD_ENOTSUP  SWMHD_BOUNDED_X / _Y (the wall faces of u and v and the gradient conditions need a body of their own),
 *                  SWMHD_TILE_KERNEL, SWMHD_MARCH_KERNEL, SWMHD_GM_IS_PREV_STATE, SWMHD_OPEN_SOUTH / _NORTH, SWMHD_LEAVE_ROOM.
 *   SWMHD_EHALO    halo < 1 in a direction without the WRAP flag of that direction.
 * An empty row range, or coefficients that are all 0, enqueue nothing.
 * Launch: one plain launch, no atomics, no LDS, no hand-off between workgroups; it captures into a graph.  A wave marches down
 * SWMHD_DIFFUSION_TILE_ROWS / 4 rows of a strip of 64 lanes; a lane holds 16 bytes of a row (2 doubles, 4 floats) where all parents
 * of the call have the same 16-byte phase and stride_y (and stride_m) keep it, else one element.
 *
 * Ensembles: swmhd_ensemble_diffusion_rk3_* does the same for `members` copies, member m of every parent at ptr + m * stride_m
 * (elements).  coef is a DEVICE table, coef[m * nfields + k]; it is not checked, and a zero entry skips that field of that member.
 * params == NULL: a and w as above for every member.  params != NULL: the DEVICE table of members x (g, f, dt) of the
 * swmhd_ensemble_*_params calls; then `a` is taken as gamma and the kernel forms a_m = dt_m gamma, and with SWMHD_RK3_ANCHOR `w` is
 * taken as the anchor's weight and w_m = dt_m w (without the flag w_m = w).  Further SWMHD_EINVAL: members outside 1 ..
 * SWMHD_ENSEMBLE_MAX_MEMBERS, stride_m < (Ny + 2 Hy) stride_y -- both checked first.
 * ---------------------------------------------------------------------------------------------- */
#define SWMHD_DIFFUSION_MAX_FIELDS 11
#define SWMHD_DIFFUSION_TILE_ROWS 64
int swmhd_diffusion_rk3_f64(const double *const *old, double *const *new_, double *const *acc, const double *coef, int nfields,
                            int Nx, int Ny, int Hx, int Hy, int64_t stride_y, double dx, double dy, double a, double w,
                            int j_begin, int j_end, int flags, void *stream);
int swmhd_diffusion_rk3_f32(const float *const *old, float *const *new_, float *const *acc, const float *coef, int nfields,
                            int Nx, int Ny, int Hx, int Hy, int64_t stride_y, float dx, float dy, float a, float w,
                            int j_begin, int j_end, int flags, void *stream);
int swmhd_ensemble_diffusion_rk3_f64(const double *const *old, double *const *new_, double *const *acc, const double *coef, int nfields,
                                     int members, int64_t stride_m, int Nx, int Ny, int Hx, int Hy, int64_t stride_y,
                                     double dx, double dy, const double *params, double a, double w, int j_begin, int j_end,
                                     int flags, void *stream);
int swmhd_ensemble_diffusion_rk3_f32(const float *const *old, float *const *new_, float *const *acc, const float *coef, int nfields,
                                     int members, int64_t stride_m, int Nx, int Ny, int Hx, int Hy, int64_t stride_y,
                                     float dx, float dy, const float *params, float a, float w, int j_begin, int j_end,
                                     int flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SWMHD_DIFFUSION_H */
