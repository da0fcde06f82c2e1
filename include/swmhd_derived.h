/* Derived frames of the shallow-water MHD engine: part of the C ABI of include/swmhd.h, which includes this file (include that one).
 * The entry points stand in a header of their own for the reason swmhd_zonal.h gives: the launching symbols that swmhd.h itself
 * declares, and the seven fields of SWMHD_OUT_ALL, are pinned by recorded matrices and existing tests.  The argument checks of these
 * calls are held against the recorded answers of the output frames label by label (tests/test_derived_abi.py).  SWMHD_VERSION is
 * unchanged. */
#ifndef SWMHD_DERIVED_H
#define SWMHD_DERIVED_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * Derived frames: the fields a 2-D MHD turbulence run is read by, differenced on the device in ONE pass over the four prognostic
 * parents (Oceananigans: ∂x(v) − ∂y(u) handed to an output writer).  C-grid, indices as in "Output frames" of swmhd.h; U, V are the
 * frame velocities (q1, q2 vector-invariant; q1 / ℑxᶠh, q2 / ℑyᶠh conservative).  All arithmetic in IEEE double, in exactly the order
 * written; Δx, Δy and f arrive in the model type and are widened; there is no Δx²: divide twice.
 *   SWMHD_DRV_VORTICITY  @(f,f)  ζ(i,j) = (V(i,j) − V(i−1,j)) / Δx − (U(i,j) − U(i,j−1)) / Δy
 *   SWMHD_DRV_DIVERGENCE @(c,c)  δ(i,j) = (U(i+1,j) − U(i,j)) / Δx + (V(i,j+1) − V(i,j)) / Δy
 *   SWMHD_DRV_CURRENT    @(c,c)  J(i,j) = ((A(i+1,j) − A(i,j))/Δx − (A(i,j) − A(i−1,j))/Δx) / Δx
 *                                       + ((A(i,j+1) − A(i,j))/Δy − (A(i,j) − A(i,j−1))/Δy) / Δy
 *   SWMHD_DRV_PV         @(f,f)  q(i,j) = (ζ(i,j) + f) / (0.5*(0.5*(h(i−1,j−1) + h(i,j−1)) + 0.5*(h(i−1,j) + h(i,j))))
 * J = ∇²A is the divergence of the face gradients that the frame's B_y, B_x are made of (before their division by h); the ℑxy of q is
 * grouped as in the speed of the frame.
 * Points written: i = 1..Nx, rows j_begin+1..j_end, for every field, on Bounded directions too.  Layout: that of the output frames --
 * field number k of `which` (counting set bits from bit 0) at out + k * out_stride_f, row j (0-based) at + (j − j_begin) * out_stride_y,
 * x contiguous, member m at + m * out_stride_m; strides in ELEMENTS of out_elem_size bytes (4: float, 8: double; computed in double and
 * rounded once).
 * Reach: one cell in all four directions plus the (i−1, j−1) corner: halo >= 1, filled (SWMHD_EHALO).  Neighbours come from the halos
 * as they stand: on Bounded grids that includes the far-wall line of U, V and the gradient-condition halos of A.  With SWMHD_WRAP_X /
 * SWMHD_WRAP_Y the neighbours are taken at (x mod Nx, y mod Ny) instead, and no halo cell of that direction is read at all.  flags:
 * only those two.  Rows j ± 1 of a parent are read only where a requested field needs them.  One launch, enqueue-only; an empty row
 * range enqueues nothing.
 *   SWMHD_EINVAL  the cases of swmhd_output_fields_*, in its order, with SWMHD_DRV_ALL in place of SWMHD_OUT_ALL; _params: params null
 *                 (among the ensemble checks).   Then SWMHD_EHALO: halo < 1.   Every check precedes the first HIP call, and a refused
 *                 call writes nothing.  coriolis_f is not validated: a non-finite f gives a non-finite q and nothing else.
 * Ensemble forms: all members in one launch, member m's parents at ptr + m * stride_m.  swmhd_ensemble_derived_fields_* takes one f
 * for all members; swmhd_ensemble_derived_fields_params_* takes the DEVICE table of (g, f, dt) per member of the other *_params calls
 * in place of it: member m uses params[3m + 1]; g and dt are not read.
 * Tolerances: none -- the object is compiled without FMA contraction and with IEEE divide, so every value is bitwise that of the
 *   expression above (tests/derived_cases.py is that restatement in numpy; tests/test_derived_gpu.py compares bitwise, float frames
 *   against the restatement rounded to float).
 * ---------------------------------------------------------------------------------------------- */
#define SWMHD_DRV_VORTICITY 1
#define SWMHD_DRV_DIVERGENCE 2
#define SWMHD_DRV_CURRENT 4
#define SWMHD_DRV_PV 8
#define SWMHD_DRV_ALL 15
int swmhd_derived_fields_f64(const double *q1, const double *q2, const double *h, const double *A,
                             int Nx, int Ny, int Hx, int Hy, int64_t stride_y, double dx, double dy, int formulation,
                             double coriolis_f, int j_begin, int j_end, int which, void *out, int out_elem_size,
                             int64_t out_stride_y, int64_t out_stride_f, int flags, void *stream);
int swmhd_derived_fields_f32(const float *q1, const float *q2, const float *h, const float *A,
                             int Nx, int Ny, int Hx, int Hy, int64_t stride_y, float dx, float dy, int formulation,
                             float coriolis_f, int j_begin, int j_end, int which, void *out, int out_elem_size,
                             int64_t out_stride_y, int64_t out_stride_f, int flags, void *stream);
int swmhd_ensemble_derived_fields_f64(const double *q1, const double *q2, const double *h, const double *A,
                                      int members, int64_t stride_m, int Nx, int Ny, int Hx, int Hy, int64_t stride_y,
                                      double dx, double dy, int formulation, double coriolis_f, int j_begin, int j_end, int which,
                                      void *out, int out_elem_size, int64_t out_stride_y, int64_t out_stride_f,
                                      int64_t out_stride_m, int flags, void *stream);
int swmhd_ensemble_derived_fields_f32(const float *q1, const float *q2, const float *h, const float *A,
                                      int members, int64_t stride_m, int Nx, int Ny, int Hx, int Hy, int64_t stride_y,
                                      float dx, float dy, int formulation, float coriolis_f, int j_begin, int j_end, int which,
                                      void *out, int out_elem_size, int64_t out_stride_y, int64_t out_stride_f,
                                      int64_t out_stride_m, int flags, void *stream);
int swmhd_ensemble_derived_fields_params_f64(const double *q1, const double *q2, const double *h, const double *A,
                                             int members, int64_t stride_m, int Nx, int Ny, int Hx, int Hy, int64_t stride_y,
                                             double dx, double dy, int formulation, const double *params, int j_begin, int j_end,
                                             int which, void *out, int out_elem_size, int64_t out_stride_y, int64_t out_stride_f,
                                             int64_t out_stride_m, int flags, void *stream);
int swmhd_ensemble_derived_fields_params_f32(const float *q1, const float *q2, const float *h, const float *A,
                                             int members, int64_t stride_m, int Nx, int Ny, int Hx, int Hy, int64_t stride_y,
                                             float dx, float dy, int formulation, const float *params, int j_begin, int j_end,
                                             int which, void *out, int out_elem_size, int64_t out_stride_y, int64_t out_stride_f,
                                             int64_t out_stride_m, int flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SWMHD_DERIVED_H */
