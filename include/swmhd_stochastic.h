/* Stochastic forcing of the shallow-water MHD engine: part of the C ABI of include/swmhd.h, which includes this file (include that
 * one).  The entry points stand in a header of their own for the reason swmhd_zonal.h gives.  Symbols are added and none changed:
 * SWMHD_VERSION is unchanged. */
#ifndef SWMHD_STOCHASTIC_H
#define SWMHD_STOCHASTIC_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * Band-limited stirring that is white in time: a sum of M Fourier modes with random coefficients, drawn once per time step on the
 * device and held over the three RK3 stages of the step.  Two calls: swmhd_stochastic_coefficients_* draws the coefficient pairs of a
 * step, swmhd_stochastic_rk3_* adds the synthesised field to what the stage kernels have written.
 *
 * ---- the field (swmhd_stochastic_rk3_*) ----
 * Per field k with M_k = nmodes[k] modes and interior cell (i, j), with the tables of the field's own nodes
 *   cx[m][i] = cos(kx_m x_i), sx[m][i] = sin(kx_m x_i), cy[m][j] = cos(ky_m y_j), sy[m][j] = sin(ky_m y_j)
 * and the coefficient pairs (P_m, Q_m) of the step:
 *   F = 0
 *   for m ascending:
 *       R = P*cy[m][j] + Q*sy[m][j]
 *       T = Q*cy[m][j] - P*sy[m][j]
 *       F = F + cx[m][i]*R
 *       F = F + sx[m][i]*T
 *   new_k += a F                                     a = dt gamma of the stage
 *   acc_k += w F        where acc_k is given         w = 1: acc is the stored tendency G^n (classic G- form)
 *                                                    w = dt/4: acc is the anchor W of SWMHD_RK3_ANCHOR's first stage
 * which is F = sum_m P_m cos(theta_m) + Q_m sin(theta_m), theta_m = kx_m x_i + ky_m y_j.  R and T depend on the row only.  The a, w,
 * SWMHD_RK3_ANCHOR and acc semantics are those of swmhd_relaxation.h.  `old` is accepted for the layout the correction calls share and
 * is never read.  F is never stored: every stage recomputes it from the tables and the coefficients.
 *   strict (SWMHD_STRICT): every operation above rounded once, in the order written, no contraction: bitwise a numpy restatement.
 *   fast:   the same expression and the same order of the modes; the compiler may contract a product and a sum into one FMA (2 FMA
 *           per mode and cell).  With tables of magnitude at most 1, S = 2 sum_m (|P_m| + |Q_m|) bounds the sum of the magnitudes of
 *           the 2 M terms cx R, sx T, and u = eps/2 (eps: the spacing of the element type at 1).  A term carries at most three
 *           roundings of its own (the two products and the sum inside R or T count two for each addend, the product with cx or sx
 *           one) and at most 2 M roundings of the running sum; a F and the final sum add two more:
 *           |new - ref| <= u |ref| + ((1 + u)^(2 M + 5) - 1) |a| S for ref = new_0 + a F_exact, which for M <= 256 is inside the bound
 *           the tests hold it to,
 *               |new - ref| <= eps |ref| + (M + 3) eps |a| S;
 *           the same for acc with w.  The strict order has the same count; an FMA only removes roundings.
 * Tables (DEVICE memory, in the element type, built once by the caller in float64 and rounded):
 *   xtab[k]: row 2 m holds cx[m][0 .. Nx), row 2 m + 1 holds sx[m][0 .. Nx), rows x_pitch elements apart (x_pitch >= Nx);
 *   ytab[k]: row 2 m holds cy[m][0 .. Ny), row 2 m + 1 holds sy[m][0 .. Ny), rows y_pitch elements apart (y_pitch >= Ny);
 *   coef[k]: P[0 .. M_k) then Q[0 .. M_k).
 * old, new, acc, coef, xtab, ytab are HOST arrays of nfields DEVICE pointers; nmodes is a HOST array of nfields counts.  A field whose
 * mode count is 0 is neither read nor written, and its table pointers may be NULL.  acc may be NULL, and so may any acc[k].
 * nfields = 1 .. SWMHD_STOCHASTIC_MAX_FIELDS, nmodes[k] = 0 .. SWMHD_STOCHASTIC_MAX_MODES.
 * Bytes per cell, field and stage (fp64): 8 + 8 of new: 16; + 16 with acc.  The x tables are read once per tile of
 * SWMHD_STOCHASTIC_TILE_ROWS rows (2 M 8 / 64 bytes per cell) and stay in cache, like the y tables and the coefficients.
 * Flops per cell and field: 2 FMA per mode in fast builds (2 multiplications and 2 additions in strict ones), plus 4 per mode and
 * row for R and T, which a workgroup forms once for its rows and not once per lane.
 * Flags: SWMHD_STRICT, SWMHD_RK3_ANCHOR; SWMHD_WRAP_X / _Y and SWMHD_BOUNDED_X / _Y are accepted and mean nothing here (radius 0).
 * Checks, in this order, every one before the first HIP call:
 *   SWMHD_EINVAL   those of swmhd_relaxation_rk3_* (null old / new, nfields, extents, pitch, rows, unknown flag bits, Bounded and
 *                  wrapped at once, null old[k] / new[k], an output equal to an old or to another output, a or w not finite; for
 *                  ensembles members and stride_m), then: null coef / xtab / ytab / nmodes; a mode count outside 0 ..
 *                  SWMHD_STOCHASTIC_MAX_MODES; for a field with modes a null or misaligned (not a multiple of the element size)
 *                  coef[k], xtab[k] or ytab[k]; x_pitch < Nx, y_pitch < Ny; for ensembles coef_stride_m < 2 nmodes[k].
 *   SWMHD_ENOTSUP  params != NULL (a per-member dt: the amplitude carries 1/sqrt(dt), which the coefficient call is given as one
 *                  number); SWMHD_TILE_KERNEL, SWMHD_MARCH_KERNEL, SWMHD_GM_IS_PREV_STATE, SWMHD_OPEN_SOUTH / _NORTH, SWMHD_LEAVE_ROOM.
 * There is no SWMHD_EHALO.  An empty row range, or mode counts that are all 0, enqueue nothing.
 * Launch: one plain launch, plain vector loads and stores, no atomics, no hand-off between workgroups; it captures into a graph.  A
 * workgroup of four waves owns SWMHD_STOCHASTIC_TILE_ROWS rows of a strip of 64 lanes; a lane keeps its columns (16 bytes of a row
 * where the parents and the x tables share a 16-byte phase, else one element) and one accumulator per row of its wave.  The modes go
 * by in chunks of SWMHD_STOCHASTIC_MODE_CHUNK: the workgroup forms R, T of the chunk's modes and its rows once, in LDS; a lane loads the
 * chunk's cx, sx of its columns once and keeps them in registers over its rows, reading R, T at one LDS address for the whole wave.
 * The registers do not grow with M.
 *
 * Ensembles: swmhd_ensemble_stochastic_rk3_* does the same for `members` copies, member m of every field parent at ptr + m * stride_m
 * and of every coef[k] at coef[k] + m * coef_stride_m (elements); the tables and the mode counts are shared by all members.
 *
 * ---- the coefficients (swmhd_stochastic_coefficients_*) ----
 * One small launch per time step: one workgroup per member.  It reads the member's 64-bit step counter n from DEVICE memory, writes
 * the coefficient pairs of every draw group and mode, and then advances the counter by one; a workgroup barrier separates every read
 * of the counter from its update.  Plain vector stores; it captures into a graph.  Always built strict.
 * Random numbers: Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57, Weyl constants 0x9E3779B9, 0xBB67AE85, ten rounds),
 *   key = (seed_lo, seed_hi), counter = (n_lo, n_hi, m + 65536 * group, substream),
 * m the mode index, group the index of the draw group within the call.  Known answers (counter / key / output):
 *   00000000 00000000 00000000 00000000 / 00000000 00000000 / 6627e8d5 e169c58d bc57ac4c 9b00dbd8
 *   ffffffff ffffffff ffffffff ffffffff / ffffffff ffffffff / 408f276d 41c83b0e a20bc7c6 6d5451fd
 *   243f6a88 85a308d3 13198a2e 03707344 / a4093822 299f31d0 / d16cfe09 94fdcceb 5001e420 24126ea1
 * From the four output words w0 .. w3: u1 = ((w0 >> 5) 2^26 + (w1 >> 6)) 2^-53, u2 likewise from w2, w3.  The coefficients are uniform,
 * not Gaussian, so that no transcendental function runs on the device.  All arithmetic in double, one rounding per operation, in
 * this order, and cast to the element type at the end:
 *   c = amp0[m] * sdt,  P = c * (2 u1 - 1),  Q = c * (2 u2 - 1)                   (2 u - 1 is exact)
 *   kind SWMHD_STOCHASTIC_SCALAR:  coef = P[0 .. M), Q[0 .. M)                       F = sum P cos + Q sin at the field's nodes
 *   kind SWMHD_STOCHASTIC_PAIR:    coef = Pu, Qu, Pv, Qv of M each,
 *       Pu = -(kty[m] * Q), Qu = kty[m] * P, Pv = ktx[m] * Q, Qv = -(ktx[m] * P)
 * The pair is F = (-delta_y psi, delta_x psi) of the corner stream function psi = sum P cos + Q sin with the C-grid's own differences,
 * ktx = sin(kx dx/2)/(dx/2), kty = sin(ky dy/2)/(dy/2) the modified wavenumbers: F_u = sum Pu cos + Qu sin at (xf, yc), F_v = sum Pv cos
 * + Qv sin at (xc, yf), whose discrete divergence is zero to rounding.  The first 2 M values are the coef[k] of the u field of
 * swmhd_stochastic_rk3_*, the last 2 M that of v.
 * counter: DEVICE, one uint64 per member.  coef, amp0, ktx, kty: HOST arrays of ngroups DEVICE pointers; amp0, ktx, kty point to M
 * doubles (for f32 too), ktx and kty are read for pairs only.  nmodes, kind: HOST arrays of ngroups values.  sdt = 1 / sqrt(dt), formed
 * by the caller.  Ensembles: member m writes coef[g] + m * coef_stride_m and reads amp0[g] + m * amp_stride_m (0: one table for all
 * members) and draws with substream[m] (a DEVICE table of members uint32).
 * Checks, every one before the first HIP call, SWMHD_EINVAL: null counter (or not 8-byte aligned), coef, amp0, nmodes, kind; ngroups
 * outside 1 .. SWMHD_STOCHASTIC_MAX_FIELDS; a mode count outside 1 .. SWMHD_STOCHASTIC_MAX_MODES; an unknown kind; a null or misaligned
 * coef[g] or amp0[g]; for a pair null ktx / kty or a null or misaligned ktx[g] / kty[g]; sdt not finite or not positive; for ensembles
 * members outside 1 .. SWMHD_ENSEMBLE_MAX_MEMBERS, a null substream table, coef_stride_m < the values a group writes, amp_stride_m
 * neither 0 nor >= nmodes[g].
 * ---------------------------------------------------------------------------------------------- */
#define SWMHD_STOCHASTIC_MAX_FIELDS 12
#define SWMHD_STOCHASTIC_MAX_MODES 256
#define SWMHD_STOCHASTIC_TILE_ROWS 64
#define SWMHD_STOCHASTIC_MODE_CHUNK 4
#define SWMHD_STOCHASTIC_SCALAR 0
#define SWMHD_STOCHASTIC_PAIR 1
int swmhd_stochastic_coefficients_f64(uint64_t *counter, double *const *coef, const double *const *amp0, const double *const *ktx,
                                      const double *const *kty, const int *nmodes, const int *kind, int ngroups, uint64_t seed,
                                      uint32_t substream, double sdt, void *stream);
int swmhd_stochastic_coefficients_f32(uint64_t *counter, float *const *coef, const double *const *amp0, const double *const *ktx,
                                      const double *const *kty, const int *nmodes, const int *kind, int ngroups, uint64_t seed,
                                      uint32_t substream, double sdt, void *stream);
int swmhd_ensemble_stochastic_coefficients_f64(uint64_t *counter, double *const *coef, const double *const *amp0, const double *const *ktx,
                                               const double *const *kty, const int *nmodes, const int *kind, int ngroups, int members,
                                               int64_t coef_stride_m, int64_t amp_stride_m, uint64_t seed, const uint32_t *substream,
                                               double sdt, void *stream);
int swmhd_ensemble_stochastic_coefficients_f32(uint64_t *counter, float *const *coef, const double *const *amp0, const double *const *ktx,
                                               const double *const *kty, const int *nmodes, const int *kind, int ngroups, int members,
                                               int64_t coef_stride_m, int64_t amp_stride_m, uint64_t seed, const uint32_t *substream,
                                               double sdt, void *stream);
int swmhd_stochastic_rk3_f64(const double *const *old, double *const *new_, double *const *acc, const double *const *coef,
                             const double *const *xtab, const double *const *ytab, const int *nmodes, int nfields, int64_t x_pitch,
                             int64_t y_pitch, int Nx, int Ny, int Hx, int Hy, int64_t stride_y, double a, double w, int j_begin, int j_end,
                             int flags, void *stream);
int swmhd_stochastic_rk3_f32(const float *const *old, float *const *new_, float *const *acc, const float *const *coef,
                             const float *const *xtab, const float *const *ytab, const int *nmodes, int nfields, int64_t x_pitch,
                             int64_t y_pitch, int Nx, int Ny, int Hx, int Hy, int64_t stride_y, float a, float w, int j_begin, int j_end,
                             int flags, void *stream);
int swmhd_ensemble_stochastic_rk3_f64(const double *const *old, double *const *new_, double *const *acc, const double *const *coef,
                                      const double *const *xtab, const double *const *ytab, const int *nmodes, int nfields,
                                      int64_t x_pitch, int64_t y_pitch, int members, int64_t stride_m, int64_t coef_stride_m, int Nx, int Ny,
                                      int Hx, int Hy, int64_t stride_y, const double *params, double a, double w, int j_begin, int j_end,
                                      int flags, void *stream);
int swmhd_ensemble_stochastic_rk3_f32(const float *const *old, float *const *new_, float *const *acc, const float *const *coef,
                                      const float *const *xtab, const float *const *ytab, const int *nmodes, int nfields, int64_t x_pitch,
                                      int64_t y_pitch, int members, int64_t stride_m, int64_t coef_stride_m, int Nx, int Ny, int Hx, int Hy,
                                      int64_t stride_y, const float *params, float a, float w, int j_begin, int j_end, int flags,
                                      void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SWMHD_STOCHASTIC_H */
