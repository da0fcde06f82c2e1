// BetaPlane Coriolis: f(y) (v̄, -ū) of the two momentum-like fields, evaluated on the state an RK3 stage STARTED from (`q1`, `q2`, which
// the ping-pong of the fused stages leaves in memory) and added to what the stage kernel -- run with f = 0, where its own Coriolis
// term is an exact no-op -- has already written:
//     vbar = ((q2[i-1,j] + q2[i,j]) / 2 + (q2[i-1,j+1] + q2[i,j+1]) / 2) / 2         D1 =   fc[j] vbar          (u at (Face, Center))
//     ubar = ((q1[i,j-1] + q1[i+1,j-1]) / 2 + (q1[i,j] + q1[i+1,j]) / 2) / 2         D2 = -(ff[j] ubar)         (v at (Center, Face))
//     n1 += a D1, n2 += a D2          (a = dt gamma)
//     a1 += w D1, a2 += w D2          (where given: w = 1 for the stored tendency Gn, dt/4 for the anchor W)
// the interpolations in the order of the oracle (oracle/sw_rhs.inc: G_u += f vbar, G_v -= f ubar; the same with uh, vh).  One launch
// (swmhd_coriolis_rk3_*), or one for all members of an ensemble (swmhd_ensemble_coriolis_rk3_*).  The same body serves Periodic and
// Bounded directions: a direction that is not wrapped reads its filled halo, which carries the wall.
//
// Strict (no contraction: Makefile STRICT): every operation above rounded once, in that order.
// Fast:   vbar = 0.25 ((. + .) + (. + .)) -- the halvings are exact, so this is the strict value -- and the updates may fuse.
//
// Work: the strip march of strip_device.inc (launch_plan.hpp strip_plan; one launch per member).  The rows j - 1, j of q1 and j, j + 1
// of q2 are carried in registers, so a row is loaded once per wave; the i - 1 neighbour of a lane's first element and the i + 1
// neighbour of its last come from the neighbouring lanes (wave shuffles) and, for lanes 0 and 63, from memory.  fc[j], ff[j] are
// uniform over the wave.
// Per cell (fp64): 8 + 8 B read of q1, q2, (8 + 8) x 2 of n1, n2: 48 B; with a1, a2 80 B.
#include "common.hpp"
#include "launch_plan.hpp"

namespace swmhd {
namespace {

#include "strip_device.inc"   // STRICT, Strip, strip_block, strip_scalars, strip_plan_of, STRIP_KERNEL, strip_launch

// the mean of four values at a cell corner: s = the pair of row j' (west + east of it), n = the pair of the row above
template <typename T>
__device__ __forceinline__ T mean4(T s0, T s1, T n0, T n1) {
    if constexpr (STRICT) return ((s0 + s1) / T(2) + (n0 + n1) / T(2)) / T(2);
    else return T(0.25) * ((s0 + s1) + (n0 + n1));
}

template <typename T, int VEC, bool ENS>
__global__ __launch_bounds__(STRIP_WAVE *STRIP_WAVES) void k_coriolis(CoriolisArgs<T> a, int lead, int nstrips, int nsb) {
    const StripBlock b = strip_block(nstrips, nsb, a.j0, a.j1);   // outer: the member
    T av = a.a, wv = a.w;
    long mo = 0;
    const T *__restrict__ frow = a.frow;
    if constexpr (ENS) {
        mo = (long)b.outer * a.stride_m;
        frow += (long)b.outer * 2 * a.Ny;
        strip_scalars<T>(a, b.outer, av, wv);
    }
    const T *__restrict__ q1 = a.q1 + mo, *__restrict__ q2 = a.q2 + mo;
    T *__restrict__ n1 = a.n1 + mo, *__restrict__ n2 = a.n2 + mo;
    T *__restrict__ a1 = a.a1 ? a.a1 + mo : nullptr, *__restrict__ a2 = a.a1 ? a.a2 + mo : nullptr;
    const int r0 = b.r0, r1 = b.r1, Ny = a.Ny;
    if (r0 >= r1) return;   // (uniform over the wave)
    const long sy = a.sy;
    const Strip<T, VEC> st(a.Nx, Ny, sy, a.wrap, b.strip, threadIdx.x, lead);

    // q1: rows j - 1 (um) and j (u0) with their east neighbours; q2: rows j (v0) and j + 1 (vp) with their west neighbours
    T um[VEC], u0[VEC], v0[VEC], vp[VEC];
    const T *p = q1 + st.row_of(r0 - 1);
    st.load_in(p, um);
    T um_e = st.east_of(p, um);
    p = q2 + st.row_of(r0);
    st.load_in(p, v0);
    T v0_w = st.west_of(p, v0);
    for (int j = r0; j < r1; ++j) {
        const long ro = (long)j * sy;
        p = q1 + ro;
        st.load_in(p, u0);
        const T u0_e = st.east_of(p, u0);
        p = q2 + st.row_of(j + 1);
        st.load_in(p, vp);
        const T vp_w = st.west_of(p, vp);
        const T fc = frow[j], ff = frow[Ny + j];
        T w1[VEC], w2[VEC], c1[VEC], c2[VEC];
        st.cols.load(n1 + ro, w1);
        st.cols.load(n2 + ro, w2);
        if (a1) {
            st.cols.load(a1 + ro, c1);
            st.cols.load(a2 + ro, c2);
        }
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const T vbar = mean4<T>(e == 0 ? v0_w : v0[e > 0 ? e - 1 : 0], v0[e], e == 0 ? vp_w : vp[e > 0 ? e - 1 : 0], vp[e]);
            const T ubar = mean4<T>(um[e], e == VEC - 1 ? um_e : um[e < VEC - 1 ? e + 1 : e], u0[e], e == VEC - 1 ? u0_e : u0[e < VEC - 1 ? e + 1 : e]);
            const T D1 = fc * vbar, D2 = -(ff * ubar);
            w1[e] = w1[e] + av * D1;
            w2[e] = w2[e] + av * D2;
            c1[e] = a1 ? c1[e] + wv * D1 : T(0);
            c2[e] = a1 ? c2[e] + wv * D2 : T(0);
        }
        st.cols.store(n1 + ro, w1);
        st.cols.store(n2 + ro, w2);
        if (a1) {
            st.cols.store(a1 + ro, c1);
            st.cols.store(a2 + ro, c2);
        }
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            um[e] = u0[e];
            v0[e] = vp[e];
        }
        um_e = u0_e;
        v0_w = vp_w;
    }
}

}  // namespace

template <typename T>
hipError_t LAUNCH_NAME(launch_coriolis_, LAUNCH_SFX)(const CoriolisArgs<T> &a, hipStream_t s) {
    const void *const ptrs[6] = {a.q1, a.q2, a.n1, a.n2, a.a1, a.a2};
    const StripPlan p = strip_plan_of<T>(a, ptrs, 6, 1);
    return strip_launch(STRIP_KERNEL(k_coriolis, T, p, a), p, s, a);
}
template hipError_t LAUNCH_NAME(launch_coriolis_, LAUNCH_SFX)<double>(const CoriolisArgs<double> &, hipStream_t);
template hipError_t LAUNCH_NAME(launch_coriolis_, LAUNCH_SFX)<float>(const CoriolisArgs<float> &, hipStream_t);

}  // namespace swmhd
