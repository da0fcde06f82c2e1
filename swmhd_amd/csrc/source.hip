// Static sources -- bathymetry and steady body forces: a field S_k that does not change in time, added to the tendency of a list of fields,
// in the conservative formulation first multiplied by the thickness at the field's face.  Evaluated on the state an RK3 stage STARTED
// from (`hold` = old[thickness], which the ping-pong of the fused stages leaves in memory) and added to what the launches before have
// written:
//     kind 0: D = S_k[i,j]        kind 1: D = ((h[i-1,j] + h[i,j]) / 2) S_k[i,j]        kind 2: D = ((h[i,j-1] + h[i,j]) / 2) S_k[i,j]
//     nw[k] += a D                (a = dt gamma)
//     acc[k] += w D               (where acc[k] != nullptr: w = 1 for the stored tendency Gn, dt/4 for the anchor W)
// One launch for all fields (swmhd_source_rk3_*), or for all fields of all members of an ensemble (swmhd_ensemble_source_rk3_*).
//
// Strict and fast are one expression, (x + y) / 2 the interpolation of the oracle (the halving is exact).  Strict objects round every
// operation once (no contraction: Makefile STRICT); in fast objects a D + nw and w D + acc may fuse.  Roundings: include/swmhd_source.h.
//
// Work: the strip march of strip_device.inc (launch_plan.hpp strip_plan, unchanged; one launch per member and field).  The kind of a
// field and whether it has an acc are decided ONCE per workgroup (uniform).
//   kind 0 (source_plain): Strip0 and the software pipeline of strip_pipeline -- two row buffers A and B in turn, the loads of every stream of
//     a row (S, nw, acc) issued together and one row ahead, whether a lane's group lies wholly inside the row decided once per lane.
//     Nothing of `old` is read.
//   kind 1, 2 (source_weighted): Strip (radius 1: the wrap of row_of and of the columns), the same two buffers.  The west h of a lane's
//     first column comes from the neighbouring lane by a wave shuffle at the time of the arithmetic -- so the loads stay one row ahead --
//     and from memory only in lane 0 of a wave; that load is issued with the row's.  For kind 2 the h row j - 1 is CARRIED from the
//     previous row of the march and loaded once, at the first row of a lane's segment.  So h costs 8 B per cell (fp64), not 16.
// Per cell and field (fp64): 8 B read of S, 8 + 8 of nw: 24; + 8 of h for kind 1, 2; + 8 + 8 with acc.  The field and the member come
// from blockIdx alone: the pointer tables are read from the kernel argument with a scalar index.
#include "common.hpp"
#include "launch_plan.hpp"

namespace swmhd {
namespace {

#include "strip_device.inc"   // STRICT, vec_load, Strip, Strip0, strip_block, strip_scalars, strip_pipeline, strip_plan_of, STRIP_KERNEL, strip_launch

template <typename T>
struct SourcePtrs {
    const T *__restrict__ h, *__restrict__ src;
    T *__restrict__ nw, *__restrict__ acc;
    T av, wv;
    long sy;
};

template <typename T, int VEC, bool ACC>
__device__ __forceinline__ void source_update(const T (&D)[VEC], const T (&un0)[VEC], const T (&ua0)[VEC], T av, T wv, T (&un)[VEC], T (&ua)[VEC]) {
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        un[e] = un0[e] + av * D[e];
        if constexpr (ACC) ua[e] = ua0[e] + wv * D[e];
    }
}

// kind 0, rows [r0, r1) of one lane.  FULL: the lane's group lies inside the row (16-byte accesses), else only its columns inside are touched
template <typename T, int VEC, bool FULL, bool ACC>
__device__ __forceinline__ void source_plain_march(const Strip0<T, VEC> &st, const SourcePtrs<T> &q, int r0, int r1) {
    struct Row {
        T s[VEC], un[VEC], ua[VEC];
    };
    auto load_row = [&](int j, Row &w) {
        const long ro = (long)j * q.sy;
        st.template load<FULL>(q.src + ro, w.s);
        st.template load<FULL>(q.nw + ro, w.un);
        if constexpr (ACC) st.template load<FULL>(q.acc + ro, w.ua);
    };
    auto finish_row = [&](int j, const Row &w) {
        const long ro = (long)j * q.sy;
        T un[VEC], ua[VEC];
        source_update<T, VEC, ACC>(w.s, w.un, w.ua, q.av, q.wv, un, ua);
        st.template store<FULL>(q.nw + ro, un);
        if constexpr (ACC) st.template store<FULL>(q.acc + ro, ua);
    };
    strip_pipeline<Row>(r0, r1, load_row, finish_row);
}

template <typename T, int VEC, bool ACC>
__device__ __forceinline__ void source_plain(const SourceArgs<T> &a, const StripBlock &b, const SourcePtrs<T> &q, int lead, int r0, int r1) {
    const Strip0<T, VEC> st(a.Nx, b.strip, threadIdx.x, lead);
    if (st.full) source_plain_march<T, VEC, true, ACC>(st, q, r0, r1);
    else if (st.any) source_plain_march<T, VEC, false, ACC>(st, q, r0, r1);   // (the ragged groups at the two ends of a row)
}

// kind 1 (x face) and 2 (y face), rows [r0, r1) of a wave: every lane takes part in the shuffles, so the lanes are not split by `full`
template <typename T, int VEC, int KIND, bool ACC>
__device__ __forceinline__ void source_weighted(const SourceArgs<T> &a, const StripBlock &b, const SourcePtrs<T> &q, int lead, int r0, int r1) {
    const Strip<T, VEC> st(a.Nx, a.Ny, q.sy, a.wrap, b.strip, threadIdx.x, lead);
    // the columns of h a lane reads: its own inside [0, Nx) and, for the x face, column -1 (the halo cell or its periodic image)
    bool okh[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) okh[e] = KIND == 1 ? (st.ok[e] && st.cols.xv + e < st.Nx) : st.cols.inside[e];
    // lane 0 of a wave has no lane to its west: where its first column is a cell, it reads the column before from memory
    const bool west_mem = KIND == 1 && st.lane == 0 && st.cols.xv >= 0 && st.cols.xv < st.Nx;
    struct Row {
        T h[VEC], s[VEC], un[VEC], ua[VEC], hw;
    };
    auto load_h = [&](const T *p, T (&v)[VEC]) {
        if (st.cols.full) {
            vec_load<T, VEC>(p + st.cols.xv, v);
        } else {
#pragma unroll
            for (int e = 0; e < VEC; ++e) v[e] = okh[e] ? p[st.col[e]] : T(0);
        }
    };
    auto load_row = [&](int j, Row &w) {
        const long ro = (long)j * q.sy;
        load_h(q.h + ro, w.h);
        if constexpr (KIND == 1) w.hw = west_mem ? q.h[ro + st.colw] : T(0);
        st.cols.load(q.src + ro, w.s);
        st.cols.load(q.nw + ro, w.un);
        if constexpr (ACC) st.cols.load(q.acc + ro, w.ua);
    };
    auto finish_row = [&](int j, const Row &w, const T (&south)[VEC]) {
        const long ro = (long)j * q.sy;
        T west = T(0);
        if constexpr (KIND == 1) {
            west = __shfl_up(w.h[VEC - 1], 1);
            if (st.lane == 0) west = w.hw;
        }
        T D[VEC], un[VEC], ua[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const T other = KIND == 1 ? (e == 0 ? west : w.h[e > 0 ? e - 1 : 0]) : south[e];
            D[e] = ((other + w.h[e]) / T(2)) * w.s[e];
        }
        source_update<T, VEC, ACC>(D, w.un, w.ua, q.av, q.wv, un, ua);
        st.cols.store(q.nw + ro, un);
        if constexpr (ACC) st.cols.store(q.acc + ro, ua);
    };
    auto carry = [&](T (&c)[VEC], const Row &w) {
        if constexpr (KIND == 2) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) c[e] = w.h[e];
        }
    };
    // the h row south of the segment's first: loaded once (row -1: the halo row or, wrapped, row Ny - 1), then carried
    T c[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) c[e] = T(0);
    if constexpr (KIND == 2) load_h(q.h + st.row_of(r0 - 1), c);
    // strip_pipeline's march with the carry behind each finished row, written out: handed to strip_pipeline (a carry hook and closures
    // that hold c) the one-element kernels come out with other instructions (profiles/strip_scaffold/README.md)
    Row A, B;
    int j = r0;
    load_row(j, A);
    while (j + 2 < r1) {
        load_row(j + 1, B);
        finish_row(j, A, c);
        carry(c, A);
        load_row(j + 2, A);
        finish_row(j + 1, B, c);
        carry(c, B);
        j += 2;
    }
    if (j + 1 < r1) {
        load_row(j + 1, B);
        finish_row(j, A, c);
        carry(c, A);
        finish_row(j + 1, B, c);
    } else {
        finish_row(j, A, c);
    }
}

template <typename T, int VEC, bool ENS>
__global__ __launch_bounds__(STRIP_WAVE *STRIP_WAVES) void k_source(SourceArgs<T> a, int lead, int nstrips, int nsb) {
    const StripBlock b = strip_block(nstrips, nsb, a.j0, a.j1);   // outer: m nfields + k
    const int k = ENS ? (int)(b.outer % (unsigned)a.nfields) : (int)b.outer;
    SourcePtrs<T> q;
    q.av = a.a; q.wv = a.w; q.sy = a.sy;
    long mo = 0, so = 0;
    if constexpr (ENS) {
        const unsigned m = b.outer / (unsigned)a.nfields;
        mo = (long)m * a.stride_m;
        so = (long)m * a.source_stride_m;
        strip_scalars<T>(a, m, q.av, q.wv);
    }
    const int kind = a.kind[k];
    q.h = kind != 0 ? a.hold + mo : nullptr;
    q.src = a.src[k] + so;
    q.nw = a.nw[k] + mo;
    q.acc = a.acc[k] ? a.acc[k] + mo : nullptr;
    const int r0 = __builtin_amdgcn_readfirstlane(b.r0), r1 = __builtin_amdgcn_readfirstlane(b.r1);   // (uniform over the wave: scalar loop bounds)
    if (r0 >= r1) return;
    // the kind of the field and whether it has an acc, uniform over the workgroup
    switch (2 * kind + (q.acc ? 1 : 0)) {
    case 0: source_plain<T, VEC, false>(a, b, q, lead, r0, r1); break;
    case 1: source_plain<T, VEC, true>(a, b, q, lead, r0, r1); break;
    case 2: source_weighted<T, VEC, 1, false>(a, b, q, lead, r0, r1); break;
    case 3: source_weighted<T, VEC, 1, true>(a, b, q, lead, r0, r1); break;
    case 4: source_weighted<T, VEC, 2, false>(a, b, q, lead, r0, r1); break;
    default: source_weighted<T, VEC, 2, true>(a, b, q, lead, r0, r1); break;
    }
}

}  // namespace

template <typename T>
hipError_t LAUNCH_NAME(launch_source_, LAUNCH_SFX)(const SourceArgs<T> &a, hipStream_t s) {
    const void *ptrs[3 * SOURCE_MAX_FIELDS + 1];
    for (int k = 0; k < a.nfields; ++k) {
        ptrs[3 * k] = a.nw[k]; ptrs[3 * k + 1] = a.acc[k]; ptrs[3 * k + 2] = a.src[k];
    }
    ptrs[3 * a.nfields] = a.hold;
    // (the sources' member pitch is read for an ensemble only)
    const StripPlan p = strip_plan_of<T>(a, ptrs, 3 * a.nfields + 1, a.nfields, {a.members > 0 ? a.source_stride_m : 0});
    return strip_launch(STRIP_KERNEL(k_source, T, p, a), p, s, a);
}
template hipError_t LAUNCH_NAME(launch_source_, LAUNCH_SFX)<double>(const SourceArgs<double> &, hipStream_t);
template hipError_t LAUNCH_NAME(launch_source_, LAUNCH_SFX)<float>(const SourceArgs<float> &, hipStream_t);

}  // namespace swmhd
