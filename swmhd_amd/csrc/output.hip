// Output frames: the fields an output writer stores, produced on the device in one pass over the four prognostic parents.
//
// The reference writes (u, v, A, s) every 0.1 time units, s = sqrt(u^2 + v^2), and looks at B_x = -dA/dy / h, B_y = dA/dx / h:
//   JLD2OutputWriter(model, (; u, v, A, s), schedule = TimeInterval(0.1))     jacobian_formulation/SWMHD_example.jl:67-68,80-84
//   the same with u = uh / h, v = vh / h                                       divergence_formulation/divergence_sw_mhd.jl:64-66,75-82
//   B_x, B_y                                                                   MHD_visualize.jl:55-65
// Definitions: the reference's expressions placed the way diagnostics.hip places them (a binary operation sits at its FIRST operand's
// location, the second operand is interpolated there, a divisor field is interpolated), all arithmetic in double:
//   U     @fc  q1                      (vector-invariant)    q1 / ℑxᶠh    (conservative)
//   V     @cf  q2                                            q2 / ℑyᶠh
//   H, A  @cc  copies
//   SPEED @fc  sqrt(U² + ℑxyᶠᶜ(V²))
//   BX    @cf  −((A(j) − A(j−1)) / Δy) / ℑyᶠh
//   BY    @fc   ((A(i) − A(i−1)) / Δx) / ℑxᶠh
// This object is built without FMA contraction and with IEEE divide / sqrt (Makefile: STRICT), so a frame is reproducible against a
// plain numpy restatement (tests/output_cases.py).
//
// The kernel carries no state: one-shot workgroups in address order, four cells of a row per thread (32 B of an fp64 parent, one
// 16-byte store of a float32 frame), a chunk that crosses the end of a row falls back to single elements.  Parents and frames are
// only element-aligned (the interior starts Hx elements into a row; a frame row is Nx elements), hence the under-aligned vector types.
// Reach: one cell (x−1, y−1, y+1).  With SWMHD_WRAP_X / _Y those neighbours are taken at (x mod Nx, y mod Ny) instead of the halo.
#include "api_args.hpp"
#include "common.hpp"

namespace swmhd {
namespace {

constexpr int OUT_NT = 256, OUT_VEC = 4;

typedef double out_d4 __attribute__((ext_vector_type(4), aligned(8)));
typedef float out_f4 __attribute__((ext_vector_type(4), aligned(4)));
template <typename T> struct OutVec;
template <> struct OutVec<double> { typedef out_d4 type; };
template <> struct OutVec<float> { typedef out_f4 type; };

template <typename T>
struct OutArgs {
    const T *q1, *q2, *h, *A;   // interior cell (1,1) of the parents, as OpArgs
    void *out;
    int Nx, Ny, j0, j1, nchunk;
    long sy, osy, osf;
    double dx, dy;
    int form, which, wrap;      // wrap: bit 0 = x, bit 1 = y
    long stride_m, ostride_m;   // ensembles: member blockIdx.y
};

// values x0-1, x0 .. x0+3 of one row: r[0] is the west neighbour of the chunk, r[1 + k] cell x0 + k
template <typename T>
__device__ __forceinline__ void load_row(const T *__restrict__ row, int x0, int xl, bool full, int Nx, double (&r)[OUT_VEC + 1]) {
    r[0] = (double)row[xl];
    if (full) {
        const typename OutVec<T>::type v = *reinterpret_cast<const typename OutVec<T>::type *>(row + x0);
#pragma unroll
        for (int k = 0; k < OUT_VEC; ++k) r[1 + k] = (double)v[k];
    } else {
#pragma unroll
        for (int k = 0; k < OUT_VEC; ++k) r[1 + k] = (double)row[x0 + k < Nx ? x0 + k : Nx - 1];   // (beyond the row: never stored)
    }
}

template <typename O>
__device__ __forceinline__ void store_chunk(O *__restrict__ p, const double (&v)[OUT_VEC], bool full, int nvalid) {
    if (full) {
        typename OutVec<O>::type w;
#pragma unroll
        for (int k = 0; k < OUT_VEC; ++k) w[k] = (O)v[k];
        *reinterpret_cast<typename OutVec<O>::type *>(p) = w;
    } else {
#pragma unroll
        for (int k = 0; k < OUT_VEC; ++k)
            if (k < nvalid) p[k] = (O)v[k];
    }
}

template <typename T, typename O, bool ENS>
__global__ __launch_bounds__(OUT_NT) void k_output_fields(OutArgs<T> a) {
    const long t = (long)blockIdx.x * OUT_NT + threadIdx.x;
    const int row = (int)(t / a.nchunk);
    const int y = a.j0 + row;
    if (y >= a.j1) return;
    const int x0 = (int)(t - (long)row * a.nchunk) * OUT_VEC;
    O *out = static_cast<O *>(a.out);
    if constexpr (ENS) {
        const long o = (long)blockIdx.y * a.stride_m;
        a.q1 += o; a.q2 += o; a.h += o; a.A += o;
        out += (long)blockIdx.y * a.ostride_m;
    }
    out += (long)row * a.osy + x0;
    const bool full = x0 + OUT_VEC <= a.Nx;
    const int nvalid = a.Nx - x0;
    const int xl = (x0 == 0 && (a.wrap & 1)) ? a.Nx - 1 : x0 - 1;
    const int ym = (y == 0 && (a.wrap & 2)) ? a.Ny - 1 : y - 1;
    const int yp = (y == a.Ny - 1 && (a.wrap & 2)) ? 0 : y + 1;
    const long r0 = (long)y * a.sy, rm = (long)ym * a.sy, rp = (long)yp * a.sy;

    // which rows of which parent this mask reads (wave-uniform)
    const int w = a.which;
    const bool cons = a.form == SWMHD_CONSERVATIVE;
    const bool wantU = w & (SWMHD_OUT_U | SWMHD_OUT_SPEED), wantV = w & (SWMHD_OUT_V | SWMHD_OUT_SPEED), wantS = w & SWMHD_OUT_SPEED;
    const bool wantBx = w & SWMHD_OUT_BX, wantBy = w & SWMHD_OUT_BY;
    constexpr int R = OUT_VEC + 1;
    double q1_0[R], q2_0[R], q2_p[R], h_m[R], h_0[R], h_p[R], A_m[R], A_0[R];
    if (wantU) load_row(a.q1 + r0, x0, xl, full, a.Nx, q1_0);
    if (wantV) load_row(a.q2 + r0, x0, xl, full, a.Nx, q2_0);
    if (wantS) load_row(a.q2 + rp, x0, xl, full, a.Nx, q2_p);
    if ((w & SWMHD_OUT_H) || wantBx || wantBy || (cons && (wantU || wantV))) load_row(a.h + r0, x0, xl, full, a.Nx, h_0);
    if (wantBx || (cons && wantV)) load_row(a.h + rm, x0, xl, full, a.Nx, h_m);
    if (cons && wantS) load_row(a.h + rp, x0, xl, full, a.Nx, h_p);
    if ((w & SWMHD_OUT_A) || wantBx || wantBy) load_row(a.A + r0, x0, xl, full, a.Nx, A_0);
    if (wantBx) load_row(a.A + rm, x0, xl, full, a.Nx, A_m);

    // velocities: U at the chunk's faces, V on rows y and y + 1 from the west neighbour on (the speed interpolates V² to the u faces)
    double U[OUT_VEC], V0[R], Vp[R], res[OUT_VEC];
    if (wantU) {
#pragma unroll
        for (int k = 0; k < OUT_VEC; ++k) U[k] = cons ? q1_0[k + 1] / (0.5 * (h_0[k] + h_0[k + 1])) : q1_0[k + 1];
    }
    if (wantV) {
#pragma unroll
        for (int i = 0; i < R; ++i) V0[i] = cons ? q2_0[i] / (0.5 * (h_m[i] + h_0[i])) : q2_0[i];
    }
    if (wantS) {
#pragma unroll
        for (int i = 0; i < R; ++i) Vp[i] = cons ? q2_p[i] / (0.5 * (h_0[i] + h_p[i])) : q2_p[i];
    }

    if (w & SWMHD_OUT_U) {
        store_chunk(out, U, full, nvalid);
        out += a.osf;
    }
    if (w & SWMHD_OUT_V) {
#pragma unroll
        for (int k = 0; k < OUT_VEC; ++k) res[k] = V0[k + 1];
        store_chunk(out, res, full, nvalid);
        out += a.osf;
    }
    if (w & SWMHD_OUT_H) {
#pragma unroll
        for (int k = 0; k < OUT_VEC; ++k) res[k] = h_0[k + 1];
        store_chunk(out, res, full, nvalid);
        out += a.osf;
    }
    if (w & SWMHD_OUT_A) {
#pragma unroll
        for (int k = 0; k < OUT_VEC; ++k) res[k] = A_0[k + 1];
        store_chunk(out, res, full, nvalid);
        out += a.osf;
    }
    if (wantS) {
#pragma unroll
        for (int k = 0; k < OUT_VEC; ++k) {
            const double g00 = V0[k], g10 = V0[k + 1], g01 = Vp[k], g11 = Vp[k + 1];
            res[k] = sqrt(U[k] * U[k] + 0.5 * (0.5 * (g00 * g00 + g10 * g10) + 0.5 * (g01 * g01 + g11 * g11)));
        }
        store_chunk(out, res, full, nvalid);
        out += a.osf;
    }
    if (wantBx) {
#pragma unroll
        for (int k = 0; k < OUT_VEC; ++k) res[k] = -((A_0[k + 1] - A_m[k + 1]) / a.dy) / (0.5 * (h_m[k + 1] + h_0[k + 1]));
        store_chunk(out, res, full, nvalid);
        out += a.osf;
    }
    if (wantBy) {
#pragma unroll
        for (int k = 0; k < OUT_VEC; ++k) res[k] = ((A_0[k + 1] - A_0[k]) / a.dx) / (0.5 * (h_0[k] + h_0[k + 1]));
        store_chunk(out, res, full, nvalid);
    }
}

// the frame: `which` fields of `elem`-byte elements at out; row, field and (ensembles) member stride in elements
struct OutFrame {
    int which;
    void *out;
    int elem;
    int64_t osy, osf, osm = 0;
};

template <typename T>
int output_common(const T *q1, const T *q2, const T *h, const T *A, const Grid &g, int form, const Rows &r, const OutFrame &o, int flags,
                  void *stream, const Ens *ens = nullptr) {
    if (!q1 || !q2 || !h || !A || !o.out) return SWMHD_EINVAL;
    if (!g.extents_ok() || !g.spacing_ok() || !formulation_ok(form) || !g.rows_ok(r.j0, r.j1)) return SWMHD_EINVAL;
    if (o.which <= 0 || (o.which & ~SWMHD_OUT_ALL)) return SWMHD_EINVAL;
    if (o.elem != 4 && o.elem != 8) return SWMHD_EINVAL;
    if (flags & ~OUTPUT_FLAGS) return SWMHD_EINVAL;
    const int nf = __builtin_popcount((unsigned)o.which);
    if (o.osy < g.Nx || o.osf < (int64_t)(r.j1 - r.j0) * o.osy) return SWMHD_EINVAL;
    if (ens) {
        if (ens->members < 1 || ens->members > SWMHD_ENSEMBLE_MAX_MEMBERS) return SWMHD_EINVAL;
        if (ens->stride_m < g.min_member_stride() || o.osm < (int64_t)nf * o.osf) return SWMHD_EINVAL;
    }
    if (!g.halo_at_least(1)) return SWMHD_EHALO;
    if (r.j0 == r.j1) return SWMHD_OK;
    OutArgs<T> a;
    a.q1 = g.interior(q1); a.q2 = g.interior(q2); a.h = g.interior(h); a.A = g.interior(A);
    a.out = o.out;
    a.Nx = g.Nx; a.Ny = g.Ny; a.j0 = r.j0; a.j1 = r.j1; a.nchunk = (g.Nx + OUT_VEC - 1) / OUT_VEC;
    a.sy = (long)g.sy; a.osy = (long)o.osy; a.osf = (long)o.osf;
    a.dx = g.dx; a.dy = g.dy;
    a.form = form; a.which = o.which;
    a.wrap = decode_flags(flags).wrap;
    a.stride_m = ens ? (long)ens->stride_m : 0; a.ostride_m = ens ? (long)o.osm : 0;
    const long threads = (long)(r.j1 - r.j0) * a.nchunk;
    const dim3 grid((unsigned)((threads + OUT_NT - 1) / OUT_NT), ens ? ens->members : 1);
    hipStream_t s = (hipStream_t)stream;
    if (ens) {
        if (o.elem == 4) hipLaunchKernelGGL((k_output_fields<T, float, true>), grid, dim3(OUT_NT), 0, s, a);
        else hipLaunchKernelGGL((k_output_fields<T, double, true>), grid, dim3(OUT_NT), 0, s, a);
    } else {
        if (o.elem == 4) hipLaunchKernelGGL((k_output_fields<T, float, false>), grid, dim3(OUT_NT), 0, s, a);
        else hipLaunchKernelGGL((k_output_fields<T, double, false>), grid, dim3(OUT_NT), 0, s, a);
    }
    return hiprc(hipGetLastError());
}

}  // namespace
}  // namespace swmhd

extern "C" {

#define SWMHD_DEF_OUTPUT(sfx, T)                                                                                                     \
    int swmhd_output_fields_##sfx(const T *q1, const T *q2, const T *h, const T *A, int Nx, int Ny, int Hx, int Hy, int64_t sy,     \
                                  T dx, T dy, int formulation, int j0, int j1, int which, void *out, int out_elem_size,             \
                                  int64_t out_stride_y, int64_t out_stride_f, int flags, void *stream) {                           \
        return swmhd::output_common<T>(q1, q2, h, A, swmhd::Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, formulation, swmhd::Rows{j0, j1},     \
                                       swmhd::OutFrame{which, out, out_elem_size, out_stride_y, out_stride_f}, flags, stream);      \
    }                                                                                                                                \
    int swmhd_ensemble_output_fields_##sfx(const T *q1, const T *q2, const T *h, const T *A, int members, int64_t stride_m, int Nx, \
                                           int Ny, int Hx, int Hy, int64_t sy, T dx, T dy, int formulation, int j0, int j1,         \
                                           int which, void *out, int out_elem_size, int64_t out_stride_y, int64_t out_stride_f,     \
                                           int64_t out_stride_m, int flags, void *stream) {                                         \
        const swmhd::Ens e{members, stride_m};                                                                                       \
        return swmhd::output_common<T>(q1, q2, h, A, swmhd::Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, formulation, swmhd::Rows{j0, j1},     \
                                       swmhd::OutFrame{which, out, out_elem_size, out_stride_y, out_stride_f, out_stride_m}, flags, stream, &e);  \
    }

SWMHD_DEF_OUTPUT(f64, double)
SWMHD_DEF_OUTPUT(f32, float)

}  // extern "C"
