// ScalarDiffusivity closure: D_k = c_k laplace(phi_k) of a list of fields, evaluated on the state an RK3 stage STARTED from (`old`,
// which the ping-pong of the fused stages leaves in memory) and added to what the stage kernels have already written:
//     nw[k] += a D_k          (a = dt gamma)
//     acc[k] += w D_k         (where acc[k] != nullptr: w = 1 for the stored tendency Gn, dt/4 for the anchor W)
// One launch for all fields (swmhd_diffusion_rk3_*), or for all fields of all members of an ensemble (swmhd_ensemble_diffusion_rk3_*).
// On the uniform periodic grid the 5-point operator is the same at faces and centres, so u, v, A and the tracers share this body.
//
// Strict (the order of Oceananigans' flux divergence, IEEE divides, no contraction: Makefile STRICT):
//     Fx_i = c ((phi_i - phi_{i-1}) / dx),  Fy_j likewise,  D = (Fx_{i+1} - Fx_i) / dx + (Fy_{j+1} - Fy_j) / dy
// Fast:   D = (c rdx2) ((phi_e + phi_w) - 2 phi) + (c rdy2) ((phi_n + phi_s) - 2 phi),  rdx2 = 1 / (dx dx) formed on the host.
//         Roundings against the exact value, in units of S = |c|/dx^2 (|e| + 2|phi| + |w|) + |c|/dy^2 (|n| + 2|phi| + |s|): three in
//         c rdx2, one in the sum of the neighbours, one in the difference (2 phi is exact), one in the product, one in the last sum.
//
// Work: the strip march of strip_device.inc (launch_plan.hpp strip_plan; one launch per member and field).  The rows j - 1, j, j + 1 of
// `old` are carried in registers, so a row is loaded once per wave; the x-neighbours of a lane's first and last element come from the
// neighbouring lanes (wave shuffles) and, for lanes 0 and 63, from memory.  Per cell and field: 8 B read of old, 8 + 8 of nw, 8 + 8 of
// acc (fp64).  The field and the member come from blockIdx alone: the pointer tables are read from the kernel argument with a scalar
// index.
#include "common.hpp"
#include "launch_plan.hpp"

namespace swmhd {
namespace {

#include "strip_device.inc"   // STRICT, Strip, strip_block, strip_scalars, strip_plan_of, STRIP_KERNEL, strip_launch

template <typename T, int VEC, bool ENS>
__global__ __launch_bounds__(STRIP_WAVE *STRIP_WAVES) void k_diffusion(DiffusionArgs<T> a, T rdx2, T rdy2, int lead, int nstrips, int nsb) {
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
    const Strip<T, VEC> st(a.Nx, a.Ny, sy, a.wrap, b.strip, threadIdx.x, lead);

    const T cx = c * rdx2, cy = c * rdy2;   // (fast form only)
    T vm[VEC], v0[VEC], vp[VEC];
    st.load_in(old + st.row_of(r0 - 1), vm);
    st.load_in(old + st.row_of(r0), v0);
    for (int j = r0; j < r1; ++j) {
        st.load_in(old + st.row_of(j + 1), vp);
        const long ro = (long)j * sy;
        const T west = st.west_of(old + ro, v0), east = st.east_of(old + ro, v0);
        T un[VEC], ua[VEC];
        st.cols.load(nw + ro, un);
        if (acc) st.cols.load(acc + ro, ua);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const T p = v0[e], pw = e == 0 ? west : v0[e > 0 ? e - 1 : 0], pe = e == VEC - 1 ? east : v0[e < VEC - 1 ? e + 1 : e];
            const T ps = vm[e], pn = vp[e];
            T D;
            if constexpr (STRICT) {
                const T Fxw = c * ((p - pw) / a.dx), Fxe = c * ((pe - p) / a.dx);
                const T Fys = c * ((p - ps) / a.dy), Fyn = c * ((pn - p) / a.dy);
                D = (Fxe - Fxw) / a.dx + (Fyn - Fys) / a.dy;
            } else {
                D = cx * ((pe + pw) - T(2) * p) + cy * ((pn + ps) - T(2) * p);
            }
            un[e] = un[e] + av * D;
            ua[e] = acc ? ua[e] + wv * D : T(0);
        }
        st.cols.store(nw + ro, un);
        if (acc) st.cols.store(acc + ro, ua);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            vm[e] = v0[e];
            v0[e] = vp[e];
        }
    }
}

}  // namespace

template <typename T>
hipError_t LAUNCH_NAME(launch_diffusion_, LAUNCH_SFX)(const DiffusionArgs<T> &a, hipStream_t s) {
    const void *ptrs[3 * DIFFUSION_MAX_FIELDS];
    for (int k = 0; k < a.nfields; ++k) { ptrs[3 * k] = a.old[k]; ptrs[3 * k + 1] = a.nw[k]; ptrs[3 * k + 2] = a.acc[k]; }
    const StripPlan p = strip_plan_of<T>(a, ptrs, 3 * a.nfields, a.nfields);
    const T rdx2 = T(1) / (a.dx * a.dx), rdy2 = T(1) / (a.dy * a.dy);
    return strip_launch(STRIP_KERNEL(k_diffusion, T, p, a), p, s, a, rdx2, rdy2);
}
template hipError_t LAUNCH_NAME(launch_diffusion_, LAUNCH_SFX)<double>(const DiffusionArgs<double> &, hipStream_t);
template hipError_t LAUNCH_NAME(launch_diffusion_, LAUNCH_SFX)<float>(const DiffusionArgs<float> &, hipStream_t);

}  // namespace swmhd
