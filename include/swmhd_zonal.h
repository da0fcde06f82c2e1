/* Zonal means of the shallow-water MHD engine: part of the C ABI of include/swmhd.h, which includes this file (include that one).
 * The entry points stand in a header of their own because the set of launching symbols that swmhd.h itself declares is pinned,
 * symbol by symbol, by a recorded matrix of return codes (tests/return_code_cases.py, tests/golden/return_codes.json); the checks of
 * these calls have a recorded matrix of their own (tests/zonal_return_code_cases.py, tests/golden/zonal_return_codes.json), held
 * against that of the output frames label by label (tests/test_zonal_abi.py).  SWMHD_VERSION is unchanged. */
#ifndef SWMHD_ZONAL_H
#define SWMHD_ZONAL_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * Zonal means: x-averaged profiles of the output fields and of the products whose y-derivatives drive the mean flow and the mean
 * potential of a channel (Oceananigans: Average(u, dims = 1) handed to an output writer), reduced on the device in ONE launch:
 *   profile[k][j] = (Σ_{i=1..Nx} term_k(i, j)) / Nx        in double, for every row j_begin+1..j_end and every member.
 * Terms: the per-cell definitions of "Output frames" in swmhd.h -- same operand-location rule, all arithmetic in double, conservative
 * velocities q / ℑh -- with U, V, BX, BY the frame values of SWMHD_OUT_U, _V, _BX, _BY:
 *   SWMHD_ZM_U .. SWMHD_ZM_BY   the low seven bits EQUAL SWMHD_OUT_U .. SWMHD_OUT_BY: first moments of u v h A s B_x B_y, each the row
 *                               mean of the float64 frame
 *   SWMHD_ZM_UU    @(f,c)  U·U                       SWMHD_ZM_VV    @(c,f)  V·V
 *   SWMHD_ZM_UV    @(f,c)  U · ℑxyᶠᶜ(V), grouped as in the speed: 0.5*(0.5*(V(i−1,j)+V(i,j)) + 0.5*(V(i−1,j+1)+V(i,j+1)))   (Reynolds stress)
 *   SWMHD_ZM_BXBX  @(c,f)  BX·BX                     SWMHD_ZM_BYBY  @(f,c)  BY·BY
 *   SWMHD_ZM_BXBY  @(f,c)  BY · ℑxyᶠᶜ(BX), same grouping                                                                      (Maxwell stress)
 *   SWMHD_ZM_VA    @(c,f)  V · (0.5*(A(i,j−1)+A(i,j)))   -- −∂y of it is the whole right-hand side of ∂t Ā
 * Points averaged: the frame's points, i = 1..Nx, on Bounded directions too -- the far-wall line (i = Nx+1) of a face field is a boundary
 * value and not part of the mean, so on a Bounded x direction a (f,·) profile averages the faces 1..Nx.  Eddy quantities are the caller's
 * subtraction (⟨u'v'⟩ = ⟨uv⟩ − ⟨u⟩⟨v⟩, with its cancellation where the eddies are weak).
 * Layout: `out` is DEVICE memory, always double.  Profile number k of `which` (counting set bits from bit 0) starts at out + k *
 * out_stride_k, its entry for row j (0-based) is at + (j − j_begin), member m at + m * out_stride_m.  out_stride_k >= j_end − j_begin.
 * Reach: that of the frame (x−1, y−1, y+1): halo >= 1, filled (SWMHD_EHALO), or SWMHD_WRAP_X / SWMHD_WRAP_Y as for the frames; flags: only
 * those two.  Rows j ± 1 are read only where a requested profile needs them.  One launch, enqueue-only, no workspace, no atomics; an empty
 * row range enqueues nothing.
 *   SWMHD_EINVAL  null pointer, bad extents / spacing / formulation / rows, `which` empty or with unknown bits, out_stride_k < j_end −
 *                 j_begin, unknown flags; ensemble: members out of range, stride_m < (Ny+2Hy) stride_y, out_stride_m < (number of
 *                 profiles) * out_stride_k.   Then SWMHD_EHALO: halo < 1.   Every check precedes the first HIP call.
 * Ensemble form: all members in one launch, member m's parents at ptr + m * stride_m.
 * Summation: one wavefront per row; lane l adds the terms of the 4-cell chunks l, l+64, l+128, ... of the row serially in x order, then
 *   a 6-level butterfly adds the 64 lane sums.  The order is a function of Nx alone: a profile entry has the same bits whatever the row
 *   range, the member count, the strides or the launch.
 * Tolerances: every per-cell term is bitwise that of the expression above evaluated in IEEE double (the object is compiled without FMA
 *   contraction and with IEEE divide and sqrt); |profile − exact mean| <= D(Nx) 2^-53 Σ_i |term| / Nx plus one rounding of the quotient,
 *   D(Nx) = 4 floor(Nx/256) + min(4, Nx mod 256) − 1 + ceil(log2(min(64, ceil(Nx/4))))  (tests/zonal_cases.py).
 * ---------------------------------------------------------------------------------------------- */
#define SWMHD_ZM_U 1
#define SWMHD_ZM_V 2
#define SWMHD_ZM_H 4
#define SWMHD_ZM_A 8
#define SWMHD_ZM_SPEED 16
#define SWMHD_ZM_BX 32
#define SWMHD_ZM_BY 64
#define SWMHD_ZM_UU 128
#define SWMHD_ZM_VV 256
#define SWMHD_ZM_UV 512
#define SWMHD_ZM_BXBX 1024
#define SWMHD_ZM_BYBY 2048
#define SWMHD_ZM_BXBY 4096
#define SWMHD_ZM_VA 8192
#define SWMHD_ZM_ALL 16383
int swmhd_zonal_means_f64(const double *q1, const double *q2, const double *h, const double *A,
                          int Nx, int Ny, int Hx, int Hy, int64_t stride_y, double dx, double dy, int formulation,
                          int j_begin, int j_end, int which, double *out, int64_t out_stride_k, int flags, void *stream);
int swmhd_zonal_means_f32(const float *q1, const float *q2, const float *h, const float *A,
                          int Nx, int Ny, int Hx, int Hy, int64_t stride_y, float dx, float dy, int formulation,
                          int j_begin, int j_end, int which, double *out, int64_t out_stride_k, int flags, void *stream);
int swmhd_ensemble_zonal_means_f64(const double *q1, const double *q2, const double *h, const double *A,
                                   int members, int64_t stride_m, int Nx, int Ny, int Hx, int Hy, int64_t stride_y,
                                   double dx, double dy, int formulation, int j_begin, int j_end, int which,
                                   double *out, int64_t out_stride_k, int64_t out_stride_m, int flags, void *stream);
int swmhd_ensemble_zonal_means_f32(const float *q1, const float *q2, const float *h, const float *A,
                                   int members, int64_t stride_m, int Nx, int Ny, int Hx, int Hy, int64_t stride_y,
                                   float dx, float dy, int formulation, int j_begin, int j_end, int which,
                                   double *out, int64_t out_stride_k, int64_t out_stride_m, int flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SWMHD_ZONAL_H */
