// Derived frames: relative vorticity, velocity divergence, vertical current and shallow-water potential vorticity, differenced on the
// device in one pass over the four prognostic parents (swmhd_derived_fields_*, include/swmhd_derived.h).
//
// In Oceananigans these are one line each (∂x(v) − ∂y(u) handed to the writer); the reference itself looks at B = (−∂yA, ∂xA) / h
// (MHD_visualize.jl:55-65), whose curl without the division is J.  C-grid, indices as in output.hip; U, V the frame velocities
// (q1, q2 vector-invariant; q1 / ℑxᶠh, q2 / ℑyᶠh conservative); all arithmetic in double, in the order written:
//   ζ  @ff  (V(i,j) − V(i−1,j)) / Δx − (U(i,j) − U(i,j−1)) / Δy
//   δ  @cc  (U(i+1,j) − U(i,j)) / Δx + (V(i,j+1) − V(i,j)) / Δy
//   J  @cc  ((A(i+1,j) − A(i,j))/Δx − (A(i,j) − A(i−1,j))/Δx) / Δx + ((A(i,j+1) − A(i,j))/Δy − (A(i,j) − A(i,j−1))/Δy) / Δy
//   q  @ff  (ζ + f) / (0.5*(0.5*(h(i−1,j−1) + h(i,j−1)) + 0.5*(h(i−1,j) + h(i,j))))
// This object is built without FMA contraction and with IEEE divide (Makefile: STRICT), so a frame is reproducible against a plain
// numpy restatement (tests/derived_cases.py).
//
// The shape is k_output_fields' (output.hip): one-shot workgroups in address order (launch_plan.hpp: derived_plan), four cells of a
// row per thread (32 B of an fp64 parent, one 16-byte store of a float32 frame), the member in blockIdx.y, a chunk that crosses the
// end of a row falls back to single elements; the velocities, the vector types and the chunk store are those of frame_device.inc.  A
// row window here has the east neighbour x0+4 as well as the west neighbour x0−1, each a single element, loaded only where the mask
// needs it, so this file keeps a load_row of its own.
// Reach: one cell (x±1, y±1) and the (x−1, y−1) corner.  With SWMHD_WRAP_X / _Y those neighbours are taken at (x mod Nx, y mod Ny):
// no halo cell of that direction is read.
#include "api_args.hpp"
#include "common.hpp"

namespace swmhd {
namespace {

#include "frame_device.inc"   // frame_vel, frame_xy_mean, frame_rows, frame_west, FrameVec, store_chunk: shared with output.hip and zonal.hip

constexpr int DRV_W = DERIVED_VEC + 2;   // a row window: values x0-1, x0 .. x0+3, x0+4
static_assert(DERIVED_VEC == FRAME_VEC, "a thread's cells are one chunk of the frame");

template <typename T>
struct DrvArgs {
    const T *q1, *q2, *h, *A;   // interior cell (1,1) of the parents, as OpArgs
    void *out;
    int Nx, Ny, j0, j1, nchunk;
    long sy, osy, osf;
    double dx, dy, f;
    int form, which, wrap;      // wrap: bit 0 = x, bit 1 = y
    long stride_m, ostride_m;   // ensembles: member blockIdx.y
    const T *params;            // *_params: the device table of (g, f, dt) per member
};

// where the chunk's neighbours are: xl west of x0, xe east of the row's last cell (only read where the chunk ends the row)
struct DrvCols {
    int x0, xl, xe, nvalid;
    bool full;
};

// one row: r[0] the west neighbour (where `west`), r[1 + k] cell x0 + k, r[5] the east neighbour of the chunk (where `east`).  A ragged
// chunk takes the row's east neighbour into the slot behind its last cell; slots beyond that are never used.
template <typename T>
__device__ __forceinline__ void load_row(const T *__restrict__ row, const DrvCols &c, bool west, bool east, double (&r)[DRV_W]) {
    if (west) r[0] = (double)row[c.xl];
    if (c.full) {
        const typename FrameVec<T>::type v = *reinterpret_cast<const typename FrameVec<T>::type *>(row + c.x0);
#pragma unroll
        for (int k = 0; k < DERIVED_VEC; ++k) r[1 + k] = (double)v[k];
        if (east) r[1 + DERIVED_VEC] = (double)row[c.nvalid == DERIVED_VEC ? c.xe : c.x0 + DERIVED_VEC];
    } else {
#pragma unroll
        for (int k = 0; k < DERIVED_VEC; ++k) {
            const bool inside = k < c.nvalid, behind = east && k == c.nvalid;
            r[1 + k] = (inside || behind) ? (double)row[inside ? c.x0 + k : c.xe] : 0.0;   // (0: never stored)
        }
        r[1 + DERIVED_VEC] = 0.0;
    }
}

// MODE: 0 one grid, 1 ensemble with one f, 2 ensemble with the parameter table
template <typename T, typename O, int MODE>
__global__ __launch_bounds__(DERIVED_NT) void k_derived_fields(DrvArgs<T> a) {
    const long t = (long)blockIdx.x * DERIVED_NT + threadIdx.x;
    const int row = (int)(t / a.nchunk);
    const int y = a.j0 + row;
    if (y >= a.j1) return;
    DrvCols c;
    c.x0 = (int)(t - (long)row * a.nchunk) * DERIVED_VEC;
    O *out = static_cast<O *>(a.out);
    double f = a.f;
    if constexpr (MODE != 0) {
        const long o = (long)blockIdx.y * a.stride_m;
        a.q1 += o; a.q2 += o; a.h += o; a.A += o;
        out += (long)blockIdx.y * a.ostride_m;
        if constexpr (MODE == 2) f = (double)a.params[3 * (long)blockIdx.y + 1];   // (wave-uniform address: one scalar load)
    }
    out += (long)row * a.osy + c.x0;
    c.nvalid = a.Nx - c.x0;
    c.full = c.nvalid >= DERIVED_VEC;
    c.xl = frame_west(c.x0, a.Nx, a.wrap);
    c.xe = (a.wrap & 1) ? 0 : a.Nx;
    const auto [r0, rm, rp] = frame_rows(y, a.Ny, a.sy, a.wrap);
    const bool full = c.full;
    const int nvalid = c.nvalid;

    // which rows of which parent this mask reads, and which of their two single neighbours (wave-uniform)
    const int w = a.which;
    const bool cons = a.form == SWMHD_CONSERVATIVE;
    const bool wantZ = w & (SWMHD_DRV_VORTICITY | SWMHD_DRV_PV), wantD = w & SWMHD_DRV_DIVERGENCE, wantJ = w & SWMHD_DRV_CURRENT;
    const bool wantQ = w & SWMHD_DRV_PV;
    double q1_m[DRV_W], q1_0[DRV_W], q2_0[DRV_W], q2_p[DRV_W], h_m[DRV_W], h_0[DRV_W], h_p[DRV_W], A_m[DRV_W], A_0[DRV_W], A_p[DRV_W];
    if (wantZ) load_row(a.q1 + rm, c, false, false, q1_m);
    if (wantZ || wantD) load_row(a.q1 + r0, c, false, wantD, q1_0);
    if (wantZ || wantD) load_row(a.q2 + r0, c, wantZ, false, q2_0);
    if (wantD) load_row(a.q2 + rp, c, false, false, q2_p);
    if (wantQ || (cons && (wantZ || wantD))) load_row(a.h + rm, c, true, false, h_m);
    if (wantQ || (cons && (wantZ || wantD))) load_row(a.h + r0, c, true, cons && wantD, h_0);
    if (cons && wantD) load_row(a.h + rp, c, false, false, h_p);
    if (wantJ) {
        load_row(a.A + rm, c, false, false, A_m);
        load_row(a.A + r0, c, true, true, A_0);
        load_row(a.A + rp, c, false, false, A_p);
    }

    // velocities by window slot p (cell x0 − 1 + p): U on rows y − 1 and y at the chunk's faces (row y: the east neighbour's face too),
    // V on row y from the west neighbour on and on row y + 1
    double Um[DRV_W], U0[DRV_W], V0[DRV_W], Vp[DRV_W], res[DERIVED_VEC], zeta[DERIVED_VEC];
    if (wantZ) {
#pragma unroll
        for (int p = 1; p <= DERIVED_VEC; ++p) Um[p] = frame_vel(cons, q1_m[p], h_m[p - 1], h_m[p]);
    }
    if (wantZ || wantD) {
#pragma unroll
        for (int p = 1; p <= DERIVED_VEC; ++p) {
            U0[p] = frame_vel(cons, q1_0[p], h_0[p - 1], h_0[p]);
            V0[p] = frame_vel(cons, q2_0[p], h_m[p], h_0[p]);
        }
    }
    if (wantZ) V0[0] = frame_vel(cons, q2_0[0], h_m[0], h_0[0]);
    if (wantD) {
        U0[DERIVED_VEC + 1] = frame_vel(cons, q1_0[DERIVED_VEC + 1], h_0[DERIVED_VEC], h_0[DERIVED_VEC + 1]);
#pragma unroll
        for (int p = 1; p <= DERIVED_VEC; ++p) Vp[p] = frame_vel(cons, q2_p[p], h_0[p], h_p[p]);
    }

    if (wantZ) {
#pragma unroll
        for (int k = 0; k < DERIVED_VEC; ++k) zeta[k] = (V0[k + 1] - V0[k]) / a.dx - (U0[k + 1] - Um[k + 1]) / a.dy;
    }
    if (w & SWMHD_DRV_VORTICITY) {
        store_chunk(out, zeta, full, nvalid);
        out += a.osf;
    }
    if (wantD) {
#pragma unroll
        for (int k = 0; k < DERIVED_VEC; ++k) res[k] = (U0[k + 2] - U0[k + 1]) / a.dx + (Vp[k + 1] - V0[k + 1]) / a.dy;
        store_chunk(out, res, full, nvalid);
        out += a.osf;
    }
    if (wantJ) {
#pragma unroll
        for (int k = 0; k < DERIVED_VEC; ++k)
            res[k] = ((A_0[k + 2] - A_0[k + 1]) / a.dx - (A_0[k + 1] - A_0[k]) / a.dx) / a.dx +
                     ((A_p[k + 1] - A_0[k + 1]) / a.dy - (A_0[k + 1] - A_m[k + 1]) / a.dy) / a.dy;
        store_chunk(out, res, full, nvalid);
        out += a.osf;
    }
    if (wantQ) {
#pragma unroll
        for (int k = 0; k < DERIVED_VEC; ++k) res[k] = (zeta[k] + f) / frame_xy_mean(h_m[k], h_m[k + 1], h_0[k], h_0[k + 1]);
        store_chunk(out, res, full, nvalid);
    }
}

template <typename T, int MODE>
void launch(const DrvArgs<T> &a, int elem, dim3 grid, hipStream_t s) {
    if (elem == 4) hipLaunchKernelGGL((k_derived_fields<T, float, MODE>), grid, dim3(DERIVED_NT), 0, s, a);
    else hipLaunchKernelGGL((k_derived_fields<T, double, MODE>), grid, dim3(DERIVED_NT), 0, s, a);
}

// the checks of output_common (output.hip) with SWMHD_DRV_ALL for the mask; f: the scalar (ens->par: the table instead)
template <typename T>
int derived_common(const T *q1, const T *q2, const T *h, const T *A, const Grid &g, int form, T f, const Rows &r, const Frame &o,
                   int flags, void *stream, const Ens *ens = nullptr) {
    if (!frame_source_ok(q1, q2, h, A, g, form) || !frame_ok(o, SWMHD_DRV_ALL, g, r, ens)) return SWMHD_EINVAL;
    if ((flags & ~FRAME_FLAGS) || !frame_members_ok(ens, g) || (ens && ens->par && !ens->params)) return SWMHD_EINVAL;
    if (!frame_halo_ok(g)) return SWMHD_EHALO;
    const DerivedPlan p = derived_plan(g.Nx, r.j1 - r.j0, ens ? ens->members : 1);
    if (p.none) return SWMHD_OK;
    if (p.too_many) return hiprc(hipErrorInvalidConfiguration);
    DrvArgs<T> a;
    set_frame_source(a, q1, q2, h, A, g, form, o.which, flags, ens);
    a.out = o.out;
    a.j0 = r.j0; a.j1 = r.j1; a.nchunk = p.nchunk; a.f = (double)f;
    a.osy = (long)o.osy; a.osf = (long)o.osf; a.ostride_m = ens ? (long)o.osm : 0;
    a.params = ens && ens->par ? static_cast<const T *>(ens->params) : nullptr;
    const dim3 grid((unsigned)p.blocks, (unsigned)p.members);
    hipStream_t s = (hipStream_t)stream;
    if (!ens) launch<T, 0>(a, o.elem, grid, s);
    else if (!ens->par) launch<T, 1>(a, o.elem, grid, s);
    else launch<T, 2>(a, o.elem, grid, s);
    return hiprc(hipGetLastError());
}

}  // namespace
}  // namespace swmhd

extern "C" {

#define SWMHD_DEF_DERIVED(sfx, T)                                                                                                    \
    int swmhd_derived_fields_##sfx(const T *q1, const T *q2, const T *h, const T *A, int Nx, int Ny, int Hx, int Hy, int64_t sy,    \
                                   T dx, T dy, int formulation, T coriolis_f, int j0, int j1, int which, void *out,                 \
                                   int out_elem_size, int64_t out_stride_y, int64_t out_stride_f, int flags, void *stream) {        \
        return swmhd::derived_common<T>(q1, q2, h, A, swmhd::Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, formulation, coriolis_f,             \
                                        swmhd::Rows{j0, j1}, swmhd::Frame{which, out, out_elem_size, out_stride_y, out_stride_f}, \
                                        flags, stream);                                                                              \
    }                                                                                                                                \
    int swmhd_ensemble_derived_fields_##sfx(const T *q1, const T *q2, const T *h, const T *A, int members, int64_t stride_m,        \
                                            int Nx, int Ny, int Hx, int Hy, int64_t sy, T dx, T dy, int formulation, T coriolis_f,  \
                                            int j0, int j1, int which, void *out, int out_elem_size, int64_t out_stride_y,          \
                                            int64_t out_stride_f, int64_t out_stride_m, int flags, void *stream) {                  \
        const swmhd::Ens e{members, stride_m};                                                                                       \
        return swmhd::derived_common<T>(q1, q2, h, A, swmhd::Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, formulation, coriolis_f,             \
                                        swmhd::Rows{j0, j1},                                                                         \
                                        swmhd::Frame{which, out, out_elem_size, out_stride_y, out_stride_f, out_stride_m}, flags, \
                                        stream, &e);                                                                                 \
    }                                                                                                                                \
    int swmhd_ensemble_derived_fields_params_##sfx(const T *q1, const T *q2, const T *h, const T *A, int members, int64_t stride_m, \
                                                   int Nx, int Ny, int Hx, int Hy, int64_t sy, T dx, T dy, int formulation,         \
                                                   const T *params, int j0, int j1, int which, void *out, int out_elem_size,        \
                                                   int64_t out_stride_y, int64_t out_stride_f, int64_t out_stride_m, int flags,     \
                                                   void *stream) {                                                                   \
        const swmhd::Ens e{members, stride_m, false, true, params};                                                                  \
        return swmhd::derived_common<T>(q1, q2, h, A, swmhd::Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, formulation, T(0),                   \
                                        swmhd::Rows{j0, j1},                                                                         \
                                        swmhd::Frame{which, out, out_elem_size, out_stride_y, out_stride_f, out_stride_m}, flags, \
                                        stream, &e);                                                                                 \
    }

SWMHD_DEF_DERIVED(f64, double)
SWMHD_DEF_DERIVED(f32, float)

}  // extern "C"
