/* 2-D and isotropic power spectra of the shallow-water MHD engine: part of the C ABI of include/swmhd.h, which includes this file
 * (include that one).  A header of its own for the reason swmhd_zonal.h gives: the symbol lists of the other headers are pinned.
 * SWMHD_VERSION is unchanged. */
#ifndef SWMHD_SPECTRA2D_H
#define SWMHD_SPECTRA2D_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * For a frame field F -- one of SWMHD_ZS_U .. SWMHD_ZS_BY of swmhd_spectra.h, with the values, operand locations, conservative
 * velocities and halo rule of swmhd_zonal_spectra_*; the input of the transform is bitwise the float64 frame -- of the WHOLE grid:
 *   F^[kx,ky] = 1/(Nx Ny) Σ_i Σ_j F(i,j) exp(−2πi (kx (i−1)/Nx + ky (j−1)/Ny)),   kx = 0..Nx/2,  ky = 0..Ny−1
 *   P2[kx,ky] = c_kx |F^[kx,ky]|²,      c_kx = 1 at kx = 0 and kx = Nx/2, else 2        (Σ over all entries = mean of F²)
 *   my        = ky for ky <= Ny/2, else ky − Ny;     mx = kx
 *   r2        = wx * (double)(mx*mx) + wy * (double)(my*my)          (two products, one sum, in this order, no contraction)
 *   shell     = (int)floor(sqrt(r2) + 0.5)
 *   E[s]      = Σ over the (kx,ky) of shell s of P2[kx,ky],           s = 0 .. NS−1
 * wx, wy > 0 are the squared ratios of the two spectral spacings to the shell width Δk: wx = (2π/Lx / Δk)², wy = (2π/Ly / Δk)².
 * NS = floor(sqrt(wx (Nx/2)² + wy (Ny/2)²) + 0.5) + 1 = swmhd_spectra2d_shells(Nx, Ny, wx, wy): the shell of the corner mode, plus one.
 * A shell that holds no mode gets exactly 0.0.  Σ_s E[s] is the mean of F².  The shell of a mode is a statement in IEEE double (the
 * object is built without contraction, with IEEE sqrt), so a restatement in numpy gives the same shell for every mode, bit for bit.
 * The kinetic and magnetic spectra, and a spectral density (E[s] over the mode count of the shell), are the caller's.
 *
 * Outputs, both DEVICE memory, always double; at least one must be non-null:
 *   out_shell  spectrum number n of `which` (counting set bits from bit 0) at out_shell + n * out_stride_s, NS entries; member m at
 *              + m * out_stride_m.
 *   out_2d     P2 of spectrum n at out_2d + n * out2_stride_f, entry (kx, ky) at + kx * out2_stride_kx + ky: kx-major, ky contiguous
 *              in natural FFT order (0 .. Ny/2, then −Ny/2+1 .. −1); member m at + m * out2_stride_m.
 * `workspace` is DEVICE memory of at least swmhd_spectra2d_workspace(Nx, Ny, popcount(which), members, wx, wy) doubles (members = 1 for
 * the single call): the complex half-plane, 2 (Nx/2+1) Ny doubles per member and field, and the column partials, (Nx/2+1) NS doubles
 * per member and field.  At 4096² that is about 134 MB + 47 MB per field.  With out_shell null the partials are not touched and the
 * first part alone suffices.  Both functions of sizes are pure host functions and launch nothing; they answer 0 for arguments that are
 * not positive (and finite).
 * Flags: only SWMHD_WRAP_X | SWMHD_WRAP_Y, with the meaning they have for the frames.
 * Checks, in this order, every one before the first HIP call; nothing is written on any error:
 *   SWMHD_EINVAL   as swmhd_zonal_spectra_* without the rows (null parent or workspace, bad extents / spacing / formulation, `which`
 *                  empty or with unknown bits, unknown flags, members out of range, stride_m < (Ny+2Hy) stride_y), and: both outputs
 *                  null; wx or wy not finite and positive; for a non-null output a stride too small for its extent: out_stride_s < NS,
 *                  out_stride_m < (number of spectra) * out_stride_s, out2_stride_kx < Ny, out2_stride_f < (Nx/2+1) * out2_stride_kx,
 *                  out2_stride_m < (number of spectra) * out2_stride_f.
 *   SWMHD_EHALO    halo < 1 in a direction without the WRAP flag of that direction.
 *   SWMHD_ENOTSUP  Nx or Ny is not a power of two, or lies outside 4 .. 4096.
 * Launches: three plain launches on the caller's stream (two when out_shell is null), no atomics, no hand-off between workgroups, no
 * device-wide synchronisation; all capture into a graph.
 *   Pass 1, rows: the load, butterfly and untangling statements of the zonal spectra; the modes X[kx]/Nx go to the workspace transposed,
 *     (member, field, kx, j) with j contiguous; a workgroup finishes R consecutive rows before it stores (R from the LDS budget: 16 rows
 *     up to Nx = 512, 2 at Nx = 4096).
 *   Pass 2, columns: one unit per (member, field, kx) -- a wave up to Ny = 256, a workgroup above -- loads its Ny complex values into
 *     LDS, runs a complex radix-2 decimation-in-frequency FFT of length Ny (the butterfly of pass 1; twiddles from a sincospi quarter
 *     table, no recurrence; the last two stages have the twiddles 1 and −i), scales by 1/Ny (exact), forms c_kx (re² + im²) for every
 *     natural ky, stores the column of out_2d and adds the column's modes shell by shell: for fixed mx the shell does not decrease with
 *     |my|, so a shell is a run of |my|; its modes are added one after the other, my = a for ascending a, then my = −a for ascending a.
 *     Zeros stand where a shell has no mode of the column.
 *   Pass 3, shells: the Nx/2 + 1 column partials of every s, lane g of 16 the partials of kx = g, g + 16, ... one after the other, then a
 *     4-level tree.
 * The order of every sum is a function of (Nx, Ny, wx, wy) alone: a result has the same bits whatever the member count, the mask, the
 * strides or the device.
 * LDS: the column unit takes 20 Ny bytes, 80 KiB at Ny = 4096.  Where a device admits less per workgroup, the column pass runs without
 * its twiddle table (sincospi per butterfly: the same values) in 16 Ny bytes.
 *
 * Tolerance.  With S = Σ |F^|² over all Nx·Ny modes (the mean of F²) and ε₂ = η (log2 Nx + log2 Ny) 2^-53, η = 9.66:
 *   |got − P2[kx,ky]| <= c_kx (2 |F^[kx,ky]| ε₂ sqrt(S) + ε₂² S)
 * and for a shell the sum of its modes' bounds plus γ_{n_s − 1} E[s], n_s the mode count of the shell (all terms are >= 0, so this holds
 * for any order of summation).  Derivation: swmhd_spectra.h shows that pass 1 delivers every row j with a normwise error of at most
 * ε_x sqrt(S_j), ε_x = η log2(Nx) u, u = 2^-53, S_j the row's mean square.  Let G[kx,j] be the exact row modes (all Nx of them; the
 * stored half carries the other by conjugation) and G~ the computed ones: ||G~ − G||_F² = Σ_j ||row error||² <= ε_x² Σ_j S_j, and
 * (1/Ny) Σ_j S_j = S.  The exact column transform C (the DFT along j with its factor 1/Ny) maps a column c to modes of norm
 * ||c||_2 / sqrt(Ny): it is unitary up to that exact scale, so the row error arrives in the 2-D modes with Frobenius norm at most
 * ε_x sqrt(S).  The computed column transform is the same radix-2 decimation-in-frequency algorithm with the same butterfly statement
 * (y0 = a + b, y1 = (a − b) w; unfused product; twiddles from sincospi of the exact fraction: η_b = 4 + 4 sqrt(2) = 9.657) on complex
 * data: log2 Ny stages of which the last two have exact twiddles, so by Thm 24.2 of Higham (Accuracy and Stability of Numerical
 * Algorithms, 2nd ed.) its own normwise error is at most ((log2 Ny − 2) η_b + 2) u times the norm of its input, and the input's
 * Frobenius norm over the plane is at most (1 + ε_x) sqrt(S) in the units of the output.  The scaling is exact; re² + im² rounds three
 * times and the product with c_kx is exact: 1u in ε as for the rows.  In all ε₂ / u <= η_b (log2 Nx + log2 Ny) − (2 η_b − 3), and the
 * 16 u left over exceed the second-order terms (ε_x times the column constant: of order (24 · 9.66 u)²) by thirteen orders.  The error
 * of one mode is at most the Frobenius norm of the error of the plane; |got − P2| = c | |F~|² − |F^|² | <= c (2 |F^| δ + δ²) with
 * δ <= ε₂ sqrt(S).  No slack factor, and no constant other than the row transform's.
 * ---------------------------------------------------------------------------------------------- */
int swmhd_spectra2d_shells(int Nx, int Ny, double wx, double wy);
int64_t swmhd_spectra2d_workspace(int Nx, int Ny, int nfields, int members, double wx, double wy);
int swmhd_spectra2d_f64(const double *q1, const double *q2, const double *h, const double *A,
                        int Nx, int Ny, int Hx, int Hy, int64_t stride_y, double dx, double dy, int formulation, int which,
                        double wx, double wy, double *workspace, double *out_shell, int64_t out_stride_s,
                        double *out_2d, int64_t out2_stride_kx, int64_t out2_stride_f, int flags, void *stream);
int swmhd_spectra2d_f32(const float *q1, const float *q2, const float *h, const float *A,
                        int Nx, int Ny, int Hx, int Hy, int64_t stride_y, float dx, float dy, int formulation, int which,
                        double wx, double wy, double *workspace, double *out_shell, int64_t out_stride_s,
                        double *out_2d, int64_t out2_stride_kx, int64_t out2_stride_f, int flags, void *stream);
int swmhd_ensemble_spectra2d_f64(const double *q1, const double *q2, const double *h, const double *A,
                                 int members, int64_t stride_m, int Nx, int Ny, int Hx, int Hy, int64_t stride_y,
                                 double dx, double dy, int formulation, int which, double wx, double wy, double *workspace,
                                 double *out_shell, int64_t out_stride_s, int64_t out_stride_m,
                                 double *out_2d, int64_t out2_stride_kx, int64_t out2_stride_f, int64_t out2_stride_m,
                                 int flags, void *stream);
int swmhd_ensemble_spectra2d_f32(const float *q1, const float *q2, const float *h, const float *A,
                                 int members, int64_t stride_m, int Nx, int Ny, int Hx, int Hy, int64_t stride_y,
                                 float dx, float dy, int formulation, int which, double wx, double wy, double *workspace,
                                 double *out_shell, int64_t out_stride_s, int64_t out_stride_m,
                                 double *out_2d, int64_t out2_stride_kx, int64_t out2_stride_f, int64_t out2_stride_m,
                                 int flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SWMHD_SPECTRA2D_H */
