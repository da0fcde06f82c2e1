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
// Work: a wave owns a strip of 64 VEC columns and marches down CORIOLIS_WAVE_ROWS rows of it, VEC = 16 bytes of elements per lane where
// all six parents have the same 16-byte phase and the pitches keep it (else VEC = 1): launch_plan.hpp coriolis_plan.  The rows j - 1, j
// of q1 and j, j + 1 of q2 are carried in registers, so a row is loaded once per wave; the i - 1 neighbour of a lane's first element
// and the i + 1 neighbour of its last come from the neighbouring lanes (wave shuffles) and, for lanes 0 and 63, from memory.  No LDS, no
// barrier: the four waves of a workgroup are four consecutive row segments of one strip.  fc[j], ff[j] are uniform over the wave.
// Per cell (fp64): 8 + 8 B read of q1, q2, (8 + 8) x 2 of n1, n2: 48 B; with a1, a2 80 B.
#include "common.hpp"
#include "launch_plan.hpp"

#ifndef SWMHD_CORIOLIS_STRICT
#error "compile with -DSWMHD_CORIOLIS_STRICT=0 or 1 (Makefile)"
#endif

namespace swmhd {
namespace {

constexpr bool STRICT = (SWMHD_CORIOLIS_STRICT != 0);
constexpr int WAVE = CORIOLIS_WAVE, WAVES = CORIOLIS_WAVES, WAVE_ROWS = CORIOLIS_WAVE_ROWS;

template <typename T, int VEC>
__device__ __forceinline__ void vec_load(const T *p, T (&v)[VEC]) {
    if constexpr (VEC == 1) {
        v[0] = p[0];
    } else {
        using V = T __attribute__((ext_vector_type(VEC)));
        const V t = *reinterpret_cast<const V *>(p);
#pragma unroll
        for (int e = 0; e < VEC; ++e) v[e] = t[e];
    }
}
template <typename T, int VEC>
__device__ __forceinline__ void vec_store(T *p, const T (&v)[VEC]) {
    if constexpr (VEC == 1) {
        p[0] = v[0];
    } else {
        using V = T __attribute__((ext_vector_type(VEC)));
        V t;
#pragma unroll
        for (int e = 0; e < VEC; ++e) t[e] = v[e];
        *reinterpret_cast<V *>(p) = t;
    }
}

// the mean of four values at a cell corner: s = the pair of row j' (west + east of it), n = the pair of the row above
template <typename T>
__device__ __forceinline__ T mean4(T s0, T s1, T n0, T n1) {
    if constexpr (STRICT) return ((s0 + s1) / T(2) + (n0 + n1) / T(2)) / T(2);
    else return T(0.25) * ((s0 + s1) + (n0 + n1));
}

// blockIdx.x = (m nsb + sb) nstrips + strip (CoriolisPlan)
template <typename T, int VEC, bool ENS>
__global__ __launch_bounds__(WAVE *WAVES) void k_coriolis(CoriolisArgs<T> a, int lead, int nstrips, int nsb) {
    const unsigned ntiles = (unsigned)(nstrips * nsb);
    const unsigned L = xcd_remap(blockIdx.x, gridDim.x), m = L / ntiles, tile = L - m * ntiles;
    T av = a.a, wv = a.w;
    long mo = 0;
    const T *__restrict__ frow = a.frow;
    if constexpr (ENS) {
        mo = (long)m * a.stride_m;
        frow += (long)m * 2 * a.Ny;
        if (a.params) {   // the products as the host forms them for one grid
            const T dt = a.params[3 * (long)m + 2];
            av = dt * a.a;
            if (a.anchor) wv = dt * a.w;
        }
    }
    const T *__restrict__ q1 = a.q1 + mo, *__restrict__ q2 = a.q2 + mo;
    T *__restrict__ n1 = a.n1 + mo, *__restrict__ n2 = a.n2 + mo;
    T *__restrict__ a1 = a.a1 ? a.a1 + mo : nullptr, *__restrict__ a2 = a.a1 ? a.a2 + mo : nullptr;

    const int strip = (int)(tile % (unsigned)nstrips), sb = (int)(tile / (unsigned)nstrips);
    const int lane = threadIdx.x;
    const int r0 = a.j0 + (sb * WAVES + (int)threadIdx.y) * WAVE_ROWS, r1 = min(r0 + WAVE_ROWS, a.j1);
    if (r0 >= r1) return;   // (uniform over the wave)
    const int Nx = a.Nx, Ny = a.Ny;
    const long sy = a.sy;
    const bool wrapx = a.wrap & 1, wrapy = a.wrap & 2;
    const int xv = (strip * WAVE + lane) * VEC - lead;
    const bool full = xv >= 0 && xv + VEC <= Nx;
    // column x of a row as it is read: -1 and Nx are the halo cells or, wrapped, their periodic images; anything further is not read
    auto column = [&](int x, bool &ok) -> int {
        ok = x >= -1 && x <= Nx;
        if (wrapx) x = x < 0 ? Nx - 1 : (x >= Nx ? 0 : x);
        return ok ? x : 0;
    };
    int col[VEC];
    bool ok[VEC], inside[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        col[e] = column(xv + e, ok[e]);
        inside[e] = xv + e >= 0 && xv + e < Nx;
    }
    bool okw, oke;
    const int colw = column(xv - 1, okw), cole = column(xv + VEC, oke);

    auto row_of = [&](int y) -> long {   // y in [-1, Ny]
        if (wrapy) y = y < 0 ? Ny - 1 : (y >= Ny ? 0 : y);
        return (long)y * sy;
    };
    auto load_in = [&](const T *p, T(&v)[VEC]) {   // p: the row of q1 or q2
        if (full) {
            vec_load<T, VEC>(p + xv, v);
        } else {
#pragma unroll
            for (int e = 0; e < VEC; ++e) v[e] = ok[e] ? p[col[e]] : T(0);
        }
    };
    // the neighbour beyond a lane's group: from the next lane, at the ends of the wave from memory
    auto east_of = [&](const T *p, const T(&v)[VEC]) -> T {
        T x = __shfl_down(v[0], 1);
        if (lane == WAVE - 1) x = oke ? p[cole] : T(0);
        return x;
    };
    auto west_of = [&](const T *p, const T(&v)[VEC]) -> T {
        T x = __shfl_up(v[VEC - 1], 1);
        if (lane == 0) x = okw ? p[colw] : T(0);
        return x;
    };
    auto load_out = [&](const T *p, T(&v)[VEC]) {   // p: the row of n1, n2, a1 or a2
        if (full) {
            vec_load<T, VEC>(p + xv, v);
        } else {
#pragma unroll
            for (int e = 0; e < VEC; ++e) v[e] = inside[e] ? p[xv + e] : T(0);
        }
    };
    auto store_out = [&](T *p, const T(&v)[VEC]) {
        if (full) {
            vec_store<T, VEC>(p + xv, v);
        } else {
#pragma unroll
            for (int e = 0; e < VEC; ++e)
                if (inside[e]) p[xv + e] = v[e];
        }
    };

    // q1: rows j - 1 (um) and j (u0) with their east neighbours; q2: rows j (v0) and j + 1 (vp) with their west neighbours
    T um[VEC], u0[VEC], v0[VEC], vp[VEC];
    const T *p = q1 + row_of(r0 - 1);
    load_in(p, um);
    T um_e = east_of(p, um);
    p = q2 + row_of(r0);
    load_in(p, v0);
    T v0_w = west_of(p, v0);
    for (int j = r0; j < r1; ++j) {
        const long ro = (long)j * sy;
        p = q1 + ro;
        load_in(p, u0);
        const T u0_e = east_of(p, u0);
        p = q2 + row_of(j + 1);
        load_in(p, vp);
        const T vp_w = west_of(p, vp);
        const T fc = frow[j], ff = frow[Ny + j];
        T w1[VEC], w2[VEC], c1[VEC], c2[VEC];
        load_out(n1 + ro, w1);
        load_out(n2 + ro, w2);
        if (a1) {
            load_out(a1 + ro, c1);
            load_out(a2 + ro, c2);
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
        store_out(n1 + ro, w1);
        store_out(n2 + ro, w2);
        if (a1) {
            store_out(a1 + ro, c1);
            store_out(a2 + ro, c2);
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

// the 16-byte phase (in elements) all parents of the call share, or -1: then the kernel takes one element per lane
template <typename T>
int common_phase(const CoriolisArgs<T> &a) {
    constexpr int V = 16 / (int)sizeof(T);
    if (a.sy % V != 0 || (a.members > 0 && a.stride_m % V != 0)) return -1;
    auto phase = [](const void *p) { return (int)(((uintptr_t)p / sizeof(T)) % V); };
    const int ph = phase(a.q1);
    if (phase(a.q2) != ph || phase(a.n1) != ph || phase(a.n2) != ph) return -1;
    if (a.a1 && (phase(a.a1) != ph || phase(a.a2) != ph)) return -1;
    return ph;
}

}  // namespace

#define LAUNCH_NAME_(base, sfx) base##sfx
#define LAUNCH_NAME(base, sfx) LAUNCH_NAME_(base, sfx)
#if SWMHD_CORIOLIS_STRICT
#define LAUNCH_SFX strict
#else
#define LAUNCH_SFX fast
#endif

template <typename T>
hipError_t LAUNCH_NAME(launch_coriolis_, LAUNCH_SFX)(const CoriolisArgs<T> &a, hipStream_t s) {
    constexpr int V = 16 / (int)sizeof(T);
    const CoriolisPlan p = coriolis_plan(a.Nx, a.j1 - a.j0, (int)sizeof(T), common_phase(a), a.members > 0 ? a.members : 1);
    if (p.none) return hipSuccess;
    if (p.too_many) return hipErrorInvalidConfiguration;
    void (*k)(CoriolisArgs<T>, int, int, int);
    if (a.members > 0) k = p.vec == V ? k_coriolis<T, V, true> : k_coriolis<T, 1, true>;
    else k = p.vec == V ? k_coriolis<T, V, false> : k_coriolis<T, 1, false>;
    hipLaunchKernelGGL(k, dim3((unsigned)p.blocks), dim3(WAVE, WAVES), 0, s, a, p.lead, p.nstrips, p.nsb);
    return hipGetLastError();
}
template hipError_t LAUNCH_NAME(launch_coriolis_, LAUNCH_SFX)<double>(const CoriolisArgs<double> &, hipStream_t);
template hipError_t LAUNCH_NAME(launch_coriolis_, LAUNCH_SFX)<float>(const CoriolisArgs<float> &, hipStream_t);

}  // namespace swmhd
