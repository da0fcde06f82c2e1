// Output frames: the fields an output writer stores, produced on the device in one pass over the four prognostic parents.
//
// The reference writes (u, v, A, s) every 0.1 time units, s = sqrt(u^2 + v^2), and looks at B_x = -dA/dy / h, B_y = dA/dx / h:
//   JLD2OutputWriter(model, (; u, v, A, s), schedule = TimeInterval(0.1))     jacobian_formulation/SWMHD_example.jl:67-68,80-84
//   the same with u = uh / h, v = vh / h                                       divergence_formulation/divergence_sw_mhd.jl:64-66,75-82
//   B_x, B_y                                                                   MHD_visualize.jl:55-65
// Definitions: the reference's expressions placed the way diagnostics.hip places them -- the placement rule and the statements of U, V,
// SPEED, BX, BY stand in frame_device.inc; H and A @cc are copies.
// This object is built without FMA contraction and with IEEE divide / sqrt (Makefile: STRICT), so a frame is reproducible against a
// plain numpy restatement (tests/output_cases.py).
//
// The kernel carries no state: one-shot workgroups in address order, four cells of a row per thread (32 B of an fp64 parent, one
// 16-byte store of a float32 frame), a chunk that crosses the end of a row falls back to single elements (frame_device.inc: load_row,
// store_chunk).
// Reach: one cell (x−1, y−1, y+1).  With SWMHD_WRAP_X / _Y those neighbours are taken at (x mod Nx, y mod Ny) instead of the halo.
#include "api_args.hpp"
#include "common.hpp"

namespace swmhd {
namespace {

#include "frame_device.inc"   // frame_vel .. frame_by, frame_rows, frame_west, FrameVec, load_row, store_chunk: shared with zonal.hip and derived.hip

constexpr int OUT_NT = 256, OUT_VEC = FRAME_VEC;

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
    const int xl = frame_west(x0, a.Nx, a.wrap);
    const auto [r0, rm, rp] = frame_rows(y, a.Ny, a.sy, a.wrap);

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
        for (int k = 0; k < OUT_VEC; ++k) U[k] = frame_vel(cons, q1_0[k + 1], h_0[k], h_0[k + 1]);
    }
    if (wantV) {
#pragma unroll
        for (int i = 0; i < R; ++i) V0[i] = frame_vel(cons, q2_0[i], h_m[i], h_0[i]);
    }
    if (wantS) {
#pragma unroll
        for (int i = 0; i < R; ++i) Vp[i] = frame_vel(cons, q2_p[i], h_0[i], h_p[i]);
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
        for (int k = 0; k < OUT_VEC; ++k) res[k] = frame_speed(U[k], V0[k], V0[k + 1], Vp[k], Vp[k + 1]);
        store_chunk(out, res, full, nvalid);
        out += a.osf;
    }
    if (wantBx) {
#pragma unroll
        for (int k = 0; k < OUT_VEC; ++k) res[k] = frame_bx(A_0[k + 1], A_m[k + 1], a.dy, h_m[k + 1], h_0[k + 1]);
        store_chunk(out, res, full, nvalid);
        out += a.osf;
    }
    if (wantBy) {
#pragma unroll
        for (int k = 0; k < OUT_VEC; ++k) res[k] = frame_by(A_0[k + 1], A_0[k], a.dx, h_0[k], h_0[k + 1]);
        store_chunk(out, res, full, nvalid);
    }
}

template <typename T>
int output_common(const T *q1, const T *q2, const T *h, const T *A, const Grid &g, int form, const Rows &r, const Frame &o, int flags,
                  void *stream, const Ens *ens = nullptr) {
    if (!frame_source_ok(q1, q2, h, A, g, form) || !frame_ok(o, SWMHD_OUT_ALL, g, r, ens)) return SWMHD_EINVAL;
    if ((flags & ~FRAME_FLAGS) || !frame_members_ok(ens, g)) return SWMHD_EINVAL;
    if (!frame_halo_ok(g)) return SWMHD_EHALO;
    if (r.j0 == r.j1) return SWMHD_OK;
    OutArgs<T> a;
    set_frame_source(a, q1, q2, h, A, g, form, o.which, flags, ens);
    a.out = o.out;
    a.j0 = r.j0; a.j1 = r.j1; a.nchunk = (g.Nx + OUT_VEC - 1) / OUT_VEC;
    a.osy = (long)o.osy; a.osf = (long)o.osf; a.ostride_m = ens ? (long)o.osm : 0;
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
                                       swmhd::Frame{which, out, out_elem_size, out_stride_y, out_stride_f}, flags, stream);         \
    }                                                                                                                                \
    int swmhd_ensemble_output_fields_##sfx(const T *q1, const T *q2, const T *h, const T *A, int members, int64_t stride_m, int Nx, \
                                           int Ny, int Hx, int Hy, int64_t sy, T dx, T dy, int formulation, int j0, int j1,         \
                                           int which, void *out, int out_elem_size, int64_t out_stride_y, int64_t out_stride_f,     \
                                           int64_t out_stride_m, int flags, void *stream) {                                         \
        const swmhd::Ens e{members, stride_m};                                                                                       \
        return swmhd::output_common<T>(q1, q2, h, A, swmhd::Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, formulation, swmhd::Rows{j0, j1},     \
                                       swmhd::Frame{which, out, out_elem_size, out_stride_y, out_stride_f, out_stride_m}, flags, stream, &e);  \
    }

SWMHD_DEF_OUTPUT(f64, double)
SWMHD_DEF_OUTPUT(f32, float)

}  // extern "C"
