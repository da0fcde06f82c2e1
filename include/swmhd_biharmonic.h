/* ScalarBiharmonicDiffusivity closure of the shallow-water MHD engine (hyperviscosity): part of the C ABI of include/swmhd.h, which
 * includes this file (include that one).  The entry points stand in a header of their own for the reason swmhd_zonal.h gives.  Symbols
 * are added and none changed: SWMHD_VERSION is unchanged. */
#ifndef SWMHD_BIHARMONIC_H
#define SWMHD_BIHARMONIC_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * Biharmonic diffusion of a list of fields through one RK3 stage, as a correction of what the stage kernels (and the launches before
 * this one: finish_stage runs the Laplacian closure first) have written:
 *   D_k      = -coef_k laplace(laplace(old_k))       on the state the stage STARTED from
 *   new_k   += a D_k                                 a = dt gamma of the stage
 *   acc_k   += w D_k      where acc_k is given       w = 1: acc is the stored tendency G^n (classic G- form)
 *                                                    w = dt/4: acc is the anchor W of SWMHD_RK3_ANCHOR's first stage
 * Oceananigans' `closure = ScalarBiharmonicDiffusivity(nu = ..., kappa = ...)`.  a, w, SWMHD_RK3_ANCHOR and the per-member dt of
 * `params` mean what they mean in swmhd_diffusion.h, and the argument lists are those of the four calls there.  One launch for all
 * fields: nfields = 1 .. SWMHD_DIFFUSION_MAX_FIELDS.
 *   strict (SWMHD_STRICT): L = ((phi_e - phi) / dx - (phi - phi_w) / dx) / dx + ((phi_n - phi) / dy - (phi - phi_s) / dy) / dy at the cell
 *           and its four neighbours; Fx_i = c ((L_i - L_{i-1}) / dx), Fy_j likewise; D = -((Fx_{i+1} - Fx_i) / dx + (Fy_{j+1} - Fy_j) / dy);
 *           then new + a D and acc + w D, every operation rounded once, IEEE divides, no contraction.
 *   fast:   the composed form with reciprocals from the host, rdx2 = 1 / (dx dx), rdy2 likewise; FMA allowed:
 *             L = rdx2 ((phi_e + phi_w) - 2 phi) + rdy2 ((phi_n + phi_s) - 2 phi)                      at the cell and its four neighbours
 *             D = (-(c rdx2)) ((L_e + L_w) - 2 L) + (-(c rdy2)) ((L_n + L_s) - 2 L)
 *           With Labs(psi) = (psi_e + 2 psi + psi_w) / dx^2 + (psi_n + 2 psi + psi_s) / dy^2, S = c Labs(Labs(|phi|)) and eps the spacing
 *           of the element type at 1 (a rounding is at most eps/2 of its result):
 *             L: six roundings (two in rdx2, the neighbours' sum, the difference -- 2 phi is exact --, the product, the last sum), each
 *                relative to a partial result that Labs(|phi|) bounds: |L - L_exact| <= 3 eps Labs(|phi|) to first order.  The outer
 *                operator multiplies that by at most c Labs(.): 3 eps S.
 *             D: seven roundings of its own (three in c rdx2 -- the negation is exact --, the neighbours' sum, the difference, the
 *                product, the last sum), each relative to a partial result that c Labs(|L|) <= S (1 + 3 eps) bounds: 3.5 eps S.
 *           13 roundings, 6.5 eps S to first order:  |D - D_exact| <= 8 eps S  (K = 8; the rest covers the second-order terms), and
 *           |new - (new_0 + a D_exact)| <= eps |.| + 10 eps |a| S (the rounding of the result, a times the error of D, the rounding of
 *           a D where it is not fused), and the same for acc with w: the constants of swmhd_diffusion.h, whose count of seven roundings
 *           it bounds by 8 eps as well.
 * Pointers: as in swmhd_diffusion.h.  Only the interior cells of rows [j_begin, j_end) of new and acc are written; `old` is read there
 * and in the 13-cell diamond of radius 2 around every such cell, and nowhere else: with SWMHD_WRAP_X / SWMHD_WRAP_Y the periodic image
 * (x mod Nx, y mod Ny: a true modulus, right for Nx, Ny = 1, 2, 3) instead of the halo cell, and without the flag a filled halo of depth
 * >= 2, its four diagonal cells (-1,-1) .. (Nx,Ny) included.
 * coef: a HOST array of nfields values >= 0.  A field with coef == 0 is neither read nor written.
 * Bytes per cell, field and stage (fp64): 8 x 20/16 read of old (a wave segment of 16 rows reads two rows below and two above it),
 * 8 + 8 of new: 26; with acc 42 (the Laplacian: 25 / 41 with its one row each side).
 * Flags: SWMHD_STRICT, SWMHD_WRAP_X, SWMHD_WRAP_Y, SWMHD_RK3_ANCHOR (read by the ensemble call with `params` only).
 * Checks, in this order, every one before the first HIP call: those of swmhd_diffusion.h, with
 *   SWMHD_EHALO    halo < 2 in a direction without the WRAP flag of that direction.
 * (The overlap checks are the same: other workgroups still read old two rows around theirs.)
 * An empty row range, or coefficients that are all 0, enqueue nothing.
 * Launch: one plain launch, no atomics, no LDS, no barrier; it captures into a graph.  The strips, rows per wave and the 16-byte
 * vector rule are those of the Laplacian launch (SWMHD_DIFFUSION_TILE_ROWS).
 *
 * Ensembles: swmhd_ensemble_biharmonic_rk3_* as swmhd_ensemble_diffusion_rk3_*: coef is a DEVICE table coef[m * nfields + k], not
 * checked, a zero entry skips that field of that member; params as there.
 * ---------------------------------------------------------------------------------------------- */
int swmhd_biharmonic_rk3_f64(const double *const *old, double *const *new_, double *const *acc, const double *coef, int nfields,
                             int Nx, int Ny, int Hx, int Hy, int64_t stride_y, double dx, double dy, double a, double w,
                             int j_begin, int j_end, int flags, void *stream);
int swmhd_biharmonic_rk3_f32(const float *const *old, float *const *new_, float *const *acc, const float *coef, int nfields,
                             int Nx, int Ny, int Hx, int Hy, int64_t stride_y, float dx, float dy, float a, float w,
                             int j_begin, int j_end, int flags, void *stream);
int swmhd_ensemble_biharmonic_rk3_f64(const double *const *old, double *const *new_, double *const *acc, const double *coef, int nfields,
                                      int members, int64_t stride_m, int Nx, int Ny, int Hx, int Hy, int64_t stride_y,
                                      double dx, double dy, const double *params, double a, double w, int j_begin, int j_end,
                                      int flags, void *stream);
int swmhd_ensemble_biharmonic_rk3_f32(const float *const *old, float *const *new_, float *const *acc, const float *coef, int nfields,
                                      int members, int64_t stride_m, int Nx, int Ny, int Hx, int Hy, int64_t stride_y,
                                      float dx, float dy, const float *params, float a, float w, int j_begin, int j_end,
                                      int flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SWMHD_BIHARMONIC_H */
