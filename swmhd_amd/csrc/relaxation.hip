// Relaxation forcing: D_k = (rate_k mask_k) (target_k - phi_k) of a list of fields, evaluated on the state an RK3 stage STARTED from
// (`old`, which the ping-pong of the fused stages leaves in memory) and added to what the stage kernels have already written:
//     nw[k] += a D_k          (a = dt gamma)
//     acc[k] += w D_k         (where acc[k] != nullptr: w = 1 for the stored tendency Gn, dt/4 for the anchor W)
// One launch for all fields (swmhd_relaxation_rk3_*), or for all fields of all members of an ensemble
// (swmhd_ensemble_relaxation_rk3_*).  The term has radius 0: u, v, h, A and the tracers share this body, no halo cell is read, and a
// Bounded grid needs no body of its own.
//
// Strict and fast are one expression, in Oceananigans' order rate * mask * (target - phi):
//     p = rate mask (mask == nullptr: p = rate),  d = t - phi (t = target, or the scalar tval),  D = p d
// Strict objects round every operation once (no contraction: Makefile STRICT); in fast objects a D + nw and w D + acc may fuse.
// Roundings: include/swmhd_relaxation.h.
//
// Work: the strip march of strip_device.inc (Strip0; launch_plan.hpp strip_plan, unchanged; one launch per member and field).  Nothing
// is carried from row to row, so the march is a software pipeline instead: two row buffers A and B in turn, the loads of every stream
// of a row (old, mask, target, nw, acc) issued together and one row ahead -- B's before the arithmetic and the stores of A, A's next
// before those of B -- so that a wave waits for one row while the loads of the other are in flight, with no copy between the buffers.
// Whether a field has a mask, a target array or an acc is decided ONCE per workgroup (uniform), and whether a lane's group lies wholly
// inside the row once per lane: the loop under them (relax_march) is straight-line code, so no load waits for another to keep a
// register apart.  Per cell and field (fp64): 8 B read of old, 8 + 8 of nw: 24; + 8 mask, + 8 target, + 8 + 8 acc.  The field and the
// member come from blockIdx alone: the pointer tables are read from the kernel argument with a scalar index.
#include "common.hpp"
#include "launch_plan.hpp"

namespace swmhd {
namespace {

#include "strip_device.inc"   // STRICT, Strip0, strip_block, strip_scalars, strip_pipeline, strip_plan_of, STRIP_KERNEL, strip_launch

template <typename T>
struct RelaxPtrs {
    const T *__restrict__ old, *__restrict__ mask, *__restrict__ target;
    T *__restrict__ nw, *__restrict__ acc;
    T r, tv, av, wv;
    long sy;
};

// rows [r0, r1) of one lane.  FULL: the lane's group lies inside the row (16-byte accesses), else only its columns inside are touched
template <typename T, int VEC, bool FULL, bool MASK, bool TARGET, bool ACC>
__device__ __forceinline__ void relax_march(const Strip0<T, VEC> &st, const RelaxPtrs<T> &q, int r0, int r1) {
    struct Row {
        T o[VEC], mk[VEC], tg[VEC], un[VEC], ua[VEC];
    };
    auto load_row = [&](int j, Row &w) {
        const long ro = (long)j * q.sy;
        st.template load<FULL>(q.old + ro, w.o);
        if constexpr (MASK) st.template load<FULL>(q.mask + ro, w.mk);
        if constexpr (TARGET) st.template load<FULL>(q.target + ro, w.tg);
        st.template load<FULL>(q.nw + ro, w.un);
        if constexpr (ACC) st.template load<FULL>(q.acc + ro, w.ua);
    };
    auto finish_row = [&](int j, const Row &w) {
        const long ro = (long)j * q.sy;
        T un[VEC], ua[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            T p = q.r, t = q.tv;
            if constexpr (MASK) p = q.r * w.mk[e];
            if constexpr (TARGET) t = w.tg[e];
            const T d = t - w.o[e];
            const T D = p * d;
            un[e] = w.un[e] + q.av * D;
            if constexpr (ACC) ua[e] = w.ua[e] + q.wv * D;
        }
        st.template store<FULL>(q.nw + ro, un);
        if constexpr (ACC) st.template store<FULL>(q.acc + ro, ua);
    };
    strip_pipeline<Row>(r0, r1, load_row, finish_row);
}

template <typename T, int VEC, bool MASK, bool TARGET, bool ACC>
__device__ __forceinline__ void relax_lane(const Strip0<T, VEC> &st, const RelaxPtrs<T> &q, int r0, int r1) {
    if (st.full) relax_march<T, VEC, true, MASK, TARGET, ACC>(st, q, r0, r1);
    else if (st.any) relax_march<T, VEC, false, MASK, TARGET, ACC>(st, q, r0, r1);   // (the ragged groups at the two ends of a row)
}

template <typename T, int VEC, bool ENS>
__global__ __launch_bounds__(STRIP_WAVE *STRIP_WAVES) void k_relaxation(RelaxationArgs<T> a, int lead, int nstrips, int nsb) {
    const StripBlock b = strip_block(nstrips, nsb, a.j0, a.j1);   // outer: m nfields + k
    const int k = ENS ? (int)(b.outer % (unsigned)a.nfields) : (int)b.outer;
    RelaxPtrs<T> q;
    q.av = a.a; q.wv = a.w; q.sy = a.sy;
    long mo = 0, mmo = 0, tmo = 0;
    if constexpr (ENS) {
        const unsigned m = b.outer / (unsigned)a.nfields;
        mo = (long)m * a.stride_m;
        mmo = (long)m * a.mask_stride_m;
        tmo = (long)m * a.target_stride_m;
        q.r = a.rate_tab[b.outer];
        q.tv = a.tval_tab[b.outer];
        strip_scalars<T>(a, m, q.av, q.wv);
    } else {
        q.r = a.rate[k];
        q.tv = a.tval[k];
    }
    if (q.r == T(0)) return;   // (uniform over the workgroup) neither read nor written
    q.old = a.old[k] + mo;
    q.mask = a.mask[k] ? a.mask[k] + mmo : nullptr;
    q.target = a.target[k] ? a.target[k] + tmo : nullptr;
    q.nw = a.nw[k] + mo;
    q.acc = a.acc[k] ? a.acc[k] + mo : nullptr;
    const int r0 = __builtin_amdgcn_readfirstlane(b.r0), r1 = __builtin_amdgcn_readfirstlane(b.r1);   // (uniform over the wave: scalar loop bounds)
    if (r0 >= r1) return;
    const Strip0<T, VEC> st(a.Nx, b.strip, threadIdx.x, lead);
    // the kind of the field, uniform over the workgroup: bit 0 a mask, bit 1 a target array, bit 2 an acc
    switch ((q.mask ? 1 : 0) | (q.target ? 2 : 0) | (q.acc ? 4 : 0)) {
    case 0: relax_lane<T, VEC, false, false, false>(st, q, r0, r1); break;
    case 1: relax_lane<T, VEC, true, false, false>(st, q, r0, r1); break;
    case 2: relax_lane<T, VEC, false, true, false>(st, q, r0, r1); break;
    case 3: relax_lane<T, VEC, true, true, false>(st, q, r0, r1); break;
    case 4: relax_lane<T, VEC, false, false, true>(st, q, r0, r1); break;
    case 5: relax_lane<T, VEC, true, false, true>(st, q, r0, r1); break;
    case 6: relax_lane<T, VEC, false, true, true>(st, q, r0, r1); break;
    default: relax_lane<T, VEC, true, true, true>(st, q, r0, r1); break;
    }
}

}  // namespace

template <typename T>
hipError_t LAUNCH_NAME(launch_relaxation_, LAUNCH_SFX)(const RelaxationArgs<T> &a, hipStream_t s) {
    const void *ptrs[5 * RELAXATION_MAX_FIELDS];
    for (int k = 0; k < a.nfields; ++k) {
        ptrs[5 * k] = a.old[k]; ptrs[5 * k + 1] = a.nw[k]; ptrs[5 * k + 2] = a.acc[k]; ptrs[5 * k + 3] = a.mask[k]; ptrs[5 * k + 4] = a.target[k];
    }
    // (the masks' and the targets' member pitches are read for an ensemble only)
    const bool ens = a.members > 0;
    const StripPlan p = strip_plan_of<T>(a, ptrs, 5 * a.nfields, a.nfields, {ens ? a.mask_stride_m : 0, ens ? a.target_stride_m : 0});
    return strip_launch(STRIP_KERNEL(k_relaxation, T, p, a), p, s, a);
}
template hipError_t LAUNCH_NAME(launch_relaxation_, LAUNCH_SFX)<double>(const RelaxationArgs<double> &, hipStream_t);
template hipError_t LAUNCH_NAME(launch_relaxation_, LAUNCH_SFX)<float>(const RelaxationArgs<float> &, hipStream_t);

}  // namespace swmhd
