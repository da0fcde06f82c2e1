// ScalarBiharmonicDiffusivity closure: D_k = -c_k laplace(laplace(phi_k)) of a list of fields, evaluated on the state an RK3 stage STARTED
// from (`old`) and added to what the stage kernels and the launches before this one have already written:
//     nw[k] += a D_k          (a = dt gamma)
//     acc[k] += w D_k         (where acc[k] != nullptr: w = 1 for the stored tendency Gn, dt/4 for the anchor W)
// One launch for all fields (swmhd_biharmonic_rk3_*), or for all fields of all members of an ensemble (swmhd_ensemble_biharmonic_rk3_*).
// The footprint is the 13-cell diamond of radius 2; on the uniform periodic grid it is the same at faces and centres.
//
// Both forms are the composed one, L = laplace(phi) at the cell and its four neighbours, then the 5-point operator on L:
// Strict (IEEE divides, no contraction: Makefile STRICT):
//     L = ((e - p) / dx - (p - w) / dx) / dx + ((n - p) / dy - (p - s) / dy) / dy
//     Fx_i = c ((L_i - L_{i-1}) / dx),  Fy_j likewise,  D = -((Fx_{i+1} - Fx_i) / dx + (Fy_{j+1} - Fy_j) / dy)
// Fast:   L = rdx2 ((e + w) - 2 p) + rdy2 ((n + s) - 2 p),  D = (-(c rdx2)) ((L_e + L_w) - 2 L) + (-(c rdy2)) ((L_n + L_s) - 2 L),
//         rdx2 = 1 / (dx dx) formed on the host.  Roundings: include/swmhd_biharmonic.h.
//
// Work: the strip march of strip_device.inc (Strip2; launch_plan.hpp strip_plan, unchanged; one launch per member and field).  A wave
// carries three rows of L (j - 1, j, j + 1) and the rows j, j + 1 of `old` that, with the row j + 2 it loads, give the next row of L:
// every row of `old` is loaded once per wave and L is formed once per cell and wave row (two extra rows of L and four of `old` per
// segment of 16).  The x-neighbours of a lane's first and last element, of `old` and of L, come from the neighbouring lanes (wave
// shuffles); lanes 0 and 63 read theirs of `old` from memory and form L of the column next to them themselves, from the cell two
// columns out (west2_of / east2_of) and the diagonal cells, which are the west / east neighbours of the rows j - 1 and j + 1 and are
// carried.  Fast fp64: 14 VALU operations per cell (6 for L, 6 for D, 2 updates) against 26 .. 42 bytes: memory-bound.
// The field and the member come from blockIdx alone: the pointer tables are read from the kernel argument with a scalar index.
#include "common.hpp"
#include "launch_plan.hpp"

namespace swmhd {
namespace {

#include "strip_device.inc"   // STRICT, Strip2, strip_block, strip_scalars, strip_plan_of, STRIP_KERNEL, strip_launch

template <typename T, int VEC, bool ENS>
__global__ __launch_bounds__(STRIP_WAVE *STRIP_WAVES) void k_biharmonic(DiffusionArgs<T> a, T rdx2, T rdy2, int lead, int nstrips, int nsb) {
    const StripBlock b = strip_block(nstrips, nsb, a.j0, a.j1);   // outer: m nfields + k
    const int k = ENS ? (int)(b.outer % (unsigned)a.nfields) : (int)b.outer;
    T c, av = a.a, wv = a.w;
    long mo = 0;
    if constexpr (ENS) {
        const unsigned m = b.outer / (unsigned)a.nfields;
        mo = (long)m * a.stride_m;
        c = a.coef_tab[b.outer];
        strip_scalars<T>(a, m, av, wv);
    } else {
        c = a.coef[k];
    }
    if (c == T(0)) return;   // (uniform over the workgroup) neither read nor written
    const T *__restrict__ old = a.old[k] + mo;
    T *__restrict__ nw = a.nw[k] + mo;
    T *__restrict__ acc = a.acc[k] ? a.acc[k] + mo : nullptr;
    const int r0 = b.r0, r1 = b.r1;
    if (r0 >= r1) return;   // (uniform over the wave)
    const long sy = a.sy;
    const Strip2<T, VEC> st(a.Nx, a.Ny, sy, a.wrap, b.strip, threadIdx.x, lead);
    const T dx = a.dx, dy = a.dy;
    const T ncx = -(c * rdx2), ncy = -(c * rdy2);   // (fast form only)

    // columns beyond [0, Nx) that the call reads of row y: 2 in the rows it computes, 1 and 0 in the two rows around them
    auto reach_of = [&](int y) -> int { return 2 - max(max(a.j0 - y, y - (a.j1 - 1)), 0); };
    auto lap = [&](T p, T pw, T pe, T ps, T pn) -> T {
        if constexpr (STRICT) return ((pe - p) / dx - (p - pw) / dx) / dx + ((pn - p) / dy - (p - ps) / dy) / dy;
        else return rdx2 * ((pe + pw) - T(2) * p) + rdy2 * ((pn + ps) - T(2) * p);
    };
    // L of a lane's columns of one row: its rows below and above, its neighbours beyond the group
    auto lap_row = [&](const T (&vs)[VEC], const T (&vc)[VEC], const T (&vn)[VEC], T west, T east, T (&L)[VEC]) {
#pragma unroll
        for (int e = 0; e < VEC; ++e)
            L[e] = lap(vc[e], e == 0 ? west : vc[e > 0 ? e - 1 : 0], e == VEC - 1 ? east : vc[e < VEC - 1 ? e + 1 : e], vs[e], vn[e]);
    };

    T v0[VEC], vp[VEC], Lm[VEC], L0[VEC], Lp[VEC];
    T wm, w0, em, e0;   // old west and east of the group in rows j - 1 and j
    {
        T va[VEC], vb[VEC];
        st.load_in(old + st.row_of(r0 - 2), reach_of(r0 - 2), va);
        st.load_in(old + st.row_of(r0 - 1), reach_of(r0 - 1), vb);
        st.load_in(old + st.row_of(r0), 2, v0);
        st.load_in(old + st.row_of(r0 + 1), reach_of(r0 + 1), vp);
        wm = st.west_of(old + st.row_of(r0 - 1), reach_of(r0 - 1), vb);
        em = st.east_of(old + st.row_of(r0 - 1), reach_of(r0 - 1), vb);
        w0 = st.west_of(old + st.row_of(r0), 2, v0);
        e0 = st.east_of(old + st.row_of(r0), 2, v0);
        lap_row(va, vb, v0, wm, em, Lm);
        lap_row(vb, v0, vp, w0, e0, L0);
    }
    for (int j = r0; j < r1; ++j) {
        T vq[VEC];
        st.load_in(old + st.row_of(j + 2), reach_of(j + 2), vq);
        const T *rowp = old + st.row_of(j + 1);
        const T wp = st.west_of(rowp, reach_of(j + 1), vp), ep = st.east_of(rowp, reach_of(j + 1), vp);
        lap_row(v0, vp, vq, wp, ep, Lp);
        const long ro = (long)j * sy;
        // L west and east of the group in row j: the neighbouring lane's, and at the ends of the wave from the cells around that column
        T Lw = __shfl_up(L0[VEC - 1], 1), Le = __shfl_down(L0[0], 1);
        const T w2 = st.west2_of(old + ro, 2), e2 = st.east2_of(old + ro, 2);
        if (st.lane == 0) Lw = lap(w0, w2, v0[0], wm, wp);
        if (st.lane == STRIP_WAVE - 1) Le = lap(e0, v0[VEC - 1], e2, em, ep);
        T un[VEC], ua[VEC];
        st.cols.load(nw + ro, un);
        if (acc) st.cols.load(acc + ro, ua);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const T l = L0[e], lw = e == 0 ? Lw : L0[e > 0 ? e - 1 : 0], le = e == VEC - 1 ? Le : L0[e < VEC - 1 ? e + 1 : e];
            const T ls = Lm[e], ln = Lp[e];
            T D;
            if constexpr (STRICT) {
                const T Fxw = c * ((l - lw) / dx), Fxe = c * ((le - l) / dx);
                const T Fys = c * ((l - ls) / dy), Fyn = c * ((ln - l) / dy);
                D = -((Fxe - Fxw) / dx + (Fyn - Fys) / dy);
            } else {
                D = ncx * ((le + lw) - T(2) * l) + ncy * ((ln + ls) - T(2) * l);
            }
            un[e] = un[e] + av * D;
            ua[e] = acc ? ua[e] + wv * D : T(0);
        }
        st.cols.store(nw + ro, un);
        if (acc) st.cols.store(acc + ro, ua);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            Lm[e] = L0[e];
            L0[e] = Lp[e];
            v0[e] = vp[e];
            vp[e] = vq[e];
        }
        wm = w0; w0 = wp;
        em = e0; e0 = ep;
    }
}

}  // namespace

template <typename T>
hipError_t LAUNCH_NAME(launch_biharmonic_, LAUNCH_SFX)(const DiffusionArgs<T> &a, hipStream_t s) {
    const void *ptrs[3 * DIFFUSION_MAX_FIELDS];
    for (int k = 0; k < a.nfields; ++k) { ptrs[3 * k] = a.old[k]; ptrs[3 * k + 1] = a.nw[k]; ptrs[3 * k + 2] = a.acc[k]; }
    const StripPlan p = strip_plan_of<T>(a, ptrs, 3 * a.nfields, a.nfields);
    const T rdx2 = T(1) / (a.dx * a.dx), rdy2 = T(1) / (a.dy * a.dy);
    return strip_launch(STRIP_KERNEL(k_biharmonic, T, p, a), p, s, a, rdx2, rdy2);
}
template hipError_t LAUNCH_NAME(launch_biharmonic_, LAUNCH_SFX)<double>(const DiffusionArgs<double> &, hipStream_t);
template hipError_t LAUNCH_NAME(launch_biharmonic_, LAUNCH_SFX)<float>(const DiffusionArgs<float> &, hipStream_t);

}  // namespace swmhd
