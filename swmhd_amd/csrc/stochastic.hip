// Stochastic forcing: F_k = sum_m cx[m][i] R_m[j] + sx[m][i] T_m[j] of a list of fields, R = P cy + Q sy, T = Q cy - P sy the row factors of
// the step's coefficient pairs (P, Q) (stochastic_coefficients.hip draws them), added to what the stage kernels have already written:
//     nw[k] += a F_k          (a = dt gamma)
//     acc[k] += w F_k         (where acc[k] != nullptr: w = 1 for the stored tendency Gn, dt/4 for the anchor W)
// One launch for all fields (swmhd_stochastic_rk3_*), or for all fields of all members of an ensemble
// (swmhd_ensemble_stochastic_rk3_*).  The term reads no state at all: F is recomputed in every stage and never stored.
//
// Strict and fast are one expression and one order of the modes (ascending, per cell):
//     R = P*cy + Q*sy,  T = Q*cy - P*sy,  F = F + cx*R,  F = F + sx*T
// Strict objects round every operation once (no contraction: Makefile STRICT); in fast objects every line is one FMA behind a product,
// two FMA per mode and cell.  Roundings and the fast bound: include/swmhd_stochastic.h.
//
// Work: the strip geometry of strip_device.inc (Strip0; launch_plan.hpp strip_plan, unchanged; one launch per member and field), but
// unlike the five memory-bound terms this one is compute-bound (2 M FMA per cell against 16 or 32 bytes), so the march is turned inside
// out: a lane keeps its columns AND one accumulator for each of its wave's STRIP_WAVE_ROWS rows, and the modes go by in chunks of
// STOCHASTIC_MODE_CHUNK.  Per chunk the workgroup (four waves, 64 rows of one strip) forms R, T of the chunk's modes and its rows once,
// into LDS (2 x 4 x 64 values: 4 KiB in fp64) -- 4 flops per mode and ROW instead of per mode and cell -- and a lane loads the chunk's cx,
// sx of its columns once and keeps them in registers over its 16 rows: the x tables are read once per tile, not once per row.  In the row
// loop every lane of a wave reads R, T of (mode, row) at ONE LDS address (a broadcast, no bank conflict; R and T side by side, one
// 16-byte read in fp64) and issues 2 VEC FMA behind it.  Registers: 16 VEC accumulators + 2 x 4 VEC table values, whatever M is, held under a bound of two waves per SIMD
// (a chunk of 8 takes every VGPR and some AGPRs, runs one wave per SIMD and measured a third slower).  Two
// workgroup barriers per chunk; no wave leaves before the last one (a wave without rows, and a lane without columns, only skips its
// own loads and stores).  The field and the member come from blockIdx alone.
#include "common.hpp"
#include "launch_plan.hpp"

namespace swmhd {
namespace {

#include "strip_device.inc"   // STRICT, Strip0, strip_block, strip_plan_of, STRIP_KERNEL, strip_launch

constexpr int MC = STOCHASTIC_MODE_CHUNK;
constexpr int TILE_ROWS = STRIP_WAVES * STRIP_WAVE_ROWS;
constexpr int NT = STRIP_WAVE * STRIP_WAVES;
static_assert((MC * TILE_ROWS) % NT == 0, "every thread forms the same number of row factors of a chunk");

template <typename T>
struct alignas(2 * sizeof(T)) RowFactor {
    T R, Tm;
};

// F[rr][e] of the rows [0, nrows) of this wave gains the modes [0, mc) of the chunk in LDS.  WHOLE: mc == MC and nrows == STRIP_WAVE_ROWS
template <typename T, int VEC, bool WHOLE>
__device__ __forceinline__ void add_chunk(T (&F)[STRIP_WAVE_ROWS][VEC], const T (&cx)[MC][VEC], const T (&sx)[MC][VEC],
                                          const RowFactor<T> (*rt)[TILE_ROWS], int wrow, int mc, int nrows) {
#pragma unroll
    for (int rr = 0; rr < STRIP_WAVE_ROWS; ++rr) {
        if (WHOLE || rr < nrows) {
#pragma unroll
            for (int c = 0; c < MC; ++c) {
                if (WHOLE || c < mc) {
                    const RowFactor<T> f = rt[c][wrow + rr];   // one address for the whole wave
#pragma unroll
                    for (int e = 0; e < VEC; ++e) {
                        F[rr][e] = F[rr][e] + cx[c][e] * f.R;
                        F[rr][e] = F[rr][e] + sx[c][e] * f.Tm;
                    }
                }
            }
        }
    }
}

template <typename T, int VEC, bool ENS>
__global__ __launch_bounds__(STRIP_WAVE *STRIP_WAVES, 2) void k_stochastic(StochasticArgs<T> a, int lead, int nstrips, int nsb) {
    __shared__ RowFactor<T> rt[MC][TILE_ROWS];
    const StripBlock b = strip_block(nstrips, nsb, a.j0, a.j1);   // outer: m nfields + k
    const int k = ENS ? (int)(b.outer % (unsigned)a.nfields) : (int)b.outer;
    long mo = 0, co = 0;
    if constexpr (ENS) {
        const unsigned m = b.outer / (unsigned)a.nfields;
        mo = (long)m * a.stride_m;
        co = (long)m * a.coef_stride_m;
    }
    const int M = a.M[k];   // >= 1: the host leaves the fields without modes out
    const T *__restrict__ coef = a.coef[k] + co;
    const T *__restrict__ xt = a.xtab[k];
    const T *__restrict__ yt = a.ytab[k];
    T *__restrict__ nw = a.nw[k] + mo;
    T *__restrict__ acc = a.acc[k] ? a.acc[k] + mo : nullptr;
    const long xp = a.xp, yp = a.yp;
    const int wave = (int)threadIdx.y, tid = wave * STRIP_WAVE + (int)threadIdx.x;
    const int wrow = wave * STRIP_WAVE_ROWS;
    const int row0 = __builtin_amdgcn_readfirstlane(b.r0) - wrow;   // the first row of the workgroup's tile
    const int r0 = __builtin_amdgcn_readfirstlane(b.r0), r1 = __builtin_amdgcn_readfirstlane(b.r1);   // (uniform over the wave)
    const int nrows = r1 - r0;   // <= 0: a wave past j1
    const Strip0<T, VEC> st(a.Nx, b.strip, threadIdx.x, lead);
    const bool work = st.any && nrows > 0;

    T F[STRIP_WAVE_ROWS][VEC];
#pragma unroll
    for (int rr = 0; rr < STRIP_WAVE_ROWS; ++rr)
#pragma unroll
        for (int e = 0; e < VEC; ++e) F[rr][e] = T(0);

    for (int m0 = 0; m0 < M; m0 += MC) {
        const int mc = min(MC, M - m0);
        __syncthreads();   // the chunk before this one has been consumed
#pragma unroll
        for (int i = 0; i < MC * TILE_ROWS / NT; ++i) {
            const int en = tid + i * NT, c = en / TILE_ROWS, r = en % TILE_ROWS, j = row0 + r;
            if (c < mc && j < a.j1) {
                const int m = m0 + c;
                const T P = coef[m], Q = coef[M + m];
                const T cyv = yt[(long)(2 * m) * yp + j], syv = yt[(long)(2 * m + 1) * yp + j];
                RowFactor<T> f;
                f.R = P * cyv + Q * syv;
                f.Tm = Q * cyv - P * syv;
                rt[c][r] = f;
            }
        }
        __syncthreads();
        if (work) {
            T cx[MC][VEC], sx[MC][VEC];
#pragma unroll
            for (int c = 0; c < MC; ++c) {
                if (c < mc) {
                    st.load(xt + (long)(2 * (m0 + c)) * xp, cx[c]);
                    st.load(xt + (long)(2 * (m0 + c) + 1) * xp, sx[c]);
                } else {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) cx[c][e] = sx[c][e] = T(0);   // (never used)
                }
            }
            if (mc == MC && nrows == STRIP_WAVE_ROWS) add_chunk<T, VEC, true>(F, cx, sx, rt, wrow, mc, nrows);
            else add_chunk<T, VEC, false>(F, cx, sx, rt, wrow, mc, nrows);
        }
    }
    if (!work) return;   // (after the last barrier)

    const T av = a.a, wv = a.w;
#pragma unroll
    for (int rr = 0; rr < STRIP_WAVE_ROWS; ++rr) {
        if (rr < nrows) {
            const long ro = (long)(r0 + rr) * a.sy;
            T un[VEC], ua[VEC];
            // (st.load / st.store would form nw + ro and acc + ro once, ahead of the branch on st.full, not once in each of its arms:
            //  another instruction mix in all eight kernels, so the four dispatches of the updated rows stay written out)
            if (st.full) st.template load<true>(nw + ro, un);
            else st.template load<false>(nw + ro, un);
            if (acc) {
                if (st.full) st.template load<true>(acc + ro, ua);
                else st.template load<false>(acc + ro, ua);
            }
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                un[e] = un[e] + av * F[rr][e];
                if (acc) ua[e] = ua[e] + wv * F[rr][e];
            }
            if (st.full) st.template store<true>(nw + ro, un);
            else st.template store<false>(nw + ro, un);
            if (acc) {
                if (st.full) st.template store<true>(acc + ro, ua);
                else st.template store<false>(acc + ro, ua);
            }
        }
    }
}

}  // namespace

template <typename T>
hipError_t LAUNCH_NAME(launch_stochastic_, LAUNCH_SFX)(const StochasticArgs<T> &a, hipStream_t s) {
    const void *ptrs[3 * STOCHASTIC_MAX_FIELDS];
    for (int k = 0; k < a.nfields; ++k) {
        ptrs[3 * k] = a.nw[k]; ptrs[3 * k + 1] = a.acc[k]; ptrs[3 * k + 2] = a.xtab[k];
    }
    // (the x tables are shared by the members: their pitch counts for one grid too)
    const StripPlan p = strip_plan_of<T>(a, ptrs, 3 * a.nfields, a.nfields, {a.xp});
    return strip_launch(STRIP_KERNEL(k_stochastic, T, p, a), p, s, a);
}
template hipError_t LAUNCH_NAME(launch_stochastic_, LAUNCH_SFX)<double>(const StochasticArgs<double> &, hipStream_t);
template hipError_t LAUNCH_NAME(launch_stochastic_, LAUNCH_SFX)<float>(const StochasticArgs<float> &, hipStream_t);

}  // namespace swmhd
