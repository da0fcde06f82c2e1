/* Zonal wavenumber spectra of the shallow-water MHD engine: part of the C ABI of include/swmhd.h, which includes this file (include that
 * one).  The entry points stand in a header of their own for the reason swmhd_zonal.h gives: the launching symbols that swmhd.h itself
 * declares are pinned, symbol by symbol, by a recorded matrix of return codes.  The checks of these calls are held against the recorded
 * matrix of the zonal means label by label (tests/test_spectra_abi.py).  SWMHD_VERSION is unchanged. */
#ifndef SWMHD_SPECTRA_H
#define SWMHD_SPECTRA_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * Zonal spectra: the one-sided power spectrum along x of a frame field F, averaged over the requested rows, made on the device by a
 * double-precision FFT of each row held in LDS:
 *   F^_j[k]   = (1/Nx) Σ_{i=1..Nx} F(i,j) exp(−2πi k (i−1)/Nx)
 *   p_j[k]    = |F^_j[k]|² at k = 0 and k = Nx/2,   2 |F^_j[k]|² for 0 < k < Nx/2
 *   P_F[k]    = (1/rows) Σ_{j=j_begin+1..j_end} p_j[k]              k = 0 .. Nx/2
 * so that Σ_k P_F[k] is the mean of F² over the same points (Parseval).  The kinetic-energy spectrum (P_u + P_v)/2 and the magnetic one
 * are the caller's sums.
 * F(i,j): the float64 frame values of "Output frames" in swmhd.h -- SWMHD_ZS_U .. SWMHD_ZS_BY, the low seven bits, EQUAL SWMHD_OUT_U ..
 * SWMHD_OUT_BY -- with the frame's definitions, operand locations, conservative velocities q / ℑh, reach (x−1, y−1, y+1) and halo rule.
 * The input of the transform is bitwise the float64 frame; an fp32 model is widened per cell.  There is one FFT precision: double.
 * Layout: `out` is DEVICE memory, always double.  Spectrum number n of `which` (counting set bits from bit 0) starts at out + n *
 * out_stride_k and has Nx/2 + 1 entries; member m at + m * out_stride_m.  `workspace` is DEVICE memory of at least
 * swmhd_zonal_spectra_workspace(Nx, j_end − j_begin, popcount(which), members) doubles (members = 1 for the single call); that function
 * is a pure host function and launches nothing.
 * Flags: only SWMHD_WRAP_X | SWMHD_WRAP_Y, with the meaning they have for the frames.
 * Checks, in this order, every one before the first HIP call:
 *   SWMHD_EINVAL   as swmhd_zonal_means_* (null pointer, bad extents / spacing / formulation / rows, `which` empty or with unknown bits,
 *                  unknown flags, members out of range, stride_m < (Ny+2Hy) stride_y), and: null workspace, out_stride_k < Nx/2 + 1,
 *                  out_stride_m < (number of spectra) * out_stride_k.
 *   SWMHD_EHALO    halo < 1 in a direction without the WRAP flag of that direction.
 *   SWMHD_ENOTSUP  Nx is not a power of two, or lies outside 4 .. 4096.  Nothing is written.
 * An empty row range enqueues nothing.
 * Launches: two plain launches on the caller's stream, no atomics, no hand-off between workgroups, no device-wide synchronisation; both
 * capture into a graph.  Pass 1: W = min(rows, 256) units per (member, field) -- a 256-thread workgroup each from Nx = 512 on, one wave
 * each (four to a workgroup) up to Nx = 256; unit w transforms the rows j_begin + w, j_begin + w + W, ... one after the other and adds
 * their p_j[k] in that order, then stores its partial spectrum to the workspace.
 * Pass 2 adds the W partials of every k -- lane g of 16 the partials g, g + 16, ... serially, then a 4-level tree -- and divides by
 * rows.  The order is a function of (Nx, rows) alone: a spectrum has the same bits whatever the member count, the mask, the strides or
 * the device.
 * Transform: the row's Nx reals are taken as Nx/2 complex z[n] = F(2n+1) + i F(2n+2); an in-place radix-2 decimation-in-frequency FFT of
 * length Nx/2 (log2 Nx − 1 stages; y0 = a + b, y1 = (a − b) w) leaves Z in bit-reversed order, and the untangling pass
 *   E = (Z[k] + conj Z[Nx/2 − k]) / 2,  O = −i (Z[k] − conj Z[Nx/2 − k]) / 2,  X[k] = E + w_Nx^k O
 * gives the Nx/2 + 1 modes.  Twiddles: w_Nx^k = cospi(2k/Nx) − i sinpi(2k/Nx) for 0 <= k < Nx/4 from sincospi of the exact fraction, once
 * per unit into LDS; w^(k + Nx/4) = −i w^k is a swap and a sign, exact.  No recurrence.
 * Tolerance.  Per row, with S_j = Σ_k |F^_j[k]|² over all Nx modes and ε = η log2(Nx) 2^-53:
 *   |got_j[k] − p_j[k]| <= c_k (2 |F^_j[k]| ε sqrt(S_j) + ε² S_j),   c_k = 1 at k = 0 and k = Nx/2, else 2,
 * the spectrum's bound is the mean of the row bounds plus D_rows 2^-53 P[k] plus one rounding of the quotient, D_rows = ceil(rows/W) − 1
 * + ceil(W/16) − 1 + ceil(log2(min(16, W)))  (launch_plan.hpp: spectra_depth).
 * η = 9.66.  Derivation (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Thm 24.2 and its proof; u = 2^-53): a stage
 * whose computed factor differs from the exact one by at most η_b u in every 2x2 block perturbs the result normwise by η_b u, and L such
 * stages by L η_b u to first order.  A butterfly with a nontrivial twiddle: the subtraction rounds once per component (u), the complex
 * product in four multiplications and two additions without contraction by sqrt(2) γ_2, the stored twiddle is off by μ:
 * η_b u = μ + γ_4 (sqrt(2) + μ), Higham's radix-2 value.  sincospi is accurate to 2 ulp per component = 4u relative, so μ = 4u and
 * η_b = 4 + 4 sqrt(2) = 9.657.  The last two stages of the decimation-in-frequency transform have the twiddles 1 and −i only (exact
 * products): u each.  The untangling pass is two stages: the sums and differences (u; the halving is exact) and E + w O (a product, then
 * a sum: η_b u).  The scaling by 1/Nx is exact (a power of two); re² + im² rounds three times on positive terms, 2u of p, which is 1u in ε
 * because |F^[k]| <= sqrt(S).  In all ε / u <= (log2 Nx − 2) η_b + 4 for Nx >= 8 and η_b + 3 for Nx = 4: at most log2(Nx) η_b, and the
 * 2 η_b − 4 left over (15 u) exceeds the second-order terms (of order (12 · 9.66 u)²) by thirteen orders.  No slack factor.
 * ---------------------------------------------------------------------------------------------- */
#define SWMHD_ZS_U 1
#define SWMHD_ZS_V 2
#define SWMHD_ZS_H 4
#define SWMHD_ZS_A 8
#define SWMHD_ZS_SPEED 16
#define SWMHD_ZS_BX 32
#define SWMHD_ZS_BY 64
#define SWMHD_ZS_ALL 127
int64_t swmhd_zonal_spectra_workspace(int Nx, int rows, int nfields, int members);
int swmhd_zonal_spectra_f64(const double *q1, const double *q2, const double *h, const double *A,
                            int Nx, int Ny, int Hx, int Hy, int64_t stride_y, double dx, double dy, int formulation,
                            int j_begin, int j_end, int which, double *workspace, double *out, int64_t out_stride_k, int flags,
                            void *stream);
int swmhd_zonal_spectra_f32(const float *q1, const float *q2, const float *h, const float *A,
                            int Nx, int Ny, int Hx, int Hy, int64_t stride_y, float dx, float dy, int formulation,
                            int j_begin, int j_end, int which, double *workspace, double *out, int64_t out_stride_k, int flags,
                            void *stream);
int swmhd_ensemble_zonal_spectra_f64(const double *q1, const double *q2, const double *h, const double *A,
                                     int members, int64_t stride_m, int Nx, int Ny, int Hx, int Hy, int64_t stride_y,
                                     double dx, double dy, int formulation, int j_begin, int j_end, int which,
                                     double *workspace, double *out, int64_t out_stride_k, int64_t out_stride_m, int flags,
                                     void *stream);
int swmhd_ensemble_zonal_spectra_f32(const float *q1, const float *q2, const float *h, const float *A,
                                     int members, int64_t stride_m, int Nx, int Ny, int Hx, int Hy, int64_t stride_y,
                                     float dx, float dy, int formulation, int j_begin, int j_end, int which,
                                     double *workspace, double *out, int64_t out_stride_k, int64_t out_stride_m, int flags,
                                     void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SWMHD_SPECTRA_H */
