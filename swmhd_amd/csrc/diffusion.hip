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
// Work: a wave owns a strip of 64 VEC columns and marches down DIFFUSION_WAVE_ROWS rows of it, VEC = 16 bytes of elements per lane
// where every pointer of the call has the same 16-byte phase and the pitches keep it (else VEC = 1).  The rows j - 1, j, j + 1 of `old`
// are carried in registers, so a row is loaded once per wave; the x-neighbours of a lane's first and last element come from the
// neighbouring lanes (wave shuffles) and, for lanes 0 and 63, from memory.  No LDS, no barrier: the four waves of a workgroup are four
// consecutive row segments of one strip.  Per cell and field: 8 B read of old, 8 + 8 of nw, 8 + 8 of acc (fp64).
// The field and the member come from blockIdx alone: the pointer tables are read from the kernel argument with a scalar index.
#include "common.hpp"

#ifndef SWMHD_DIFFUSION_STRICT
#error "compile with -DSWMHD_DIFFUSION_STRICT=0 or 1 (Makefile)"
#endif

namespace swmhd {
namespace {

constexpr bool STRICT = (SWMHD_DIFFUSION_STRICT != 0);
constexpr int WAVE = 64, WAVES = 4, WAVE_ROWS = 16;   // workgroup tile: (64 VEC) x (WAVES WAVE_ROWS) = SWMHD_DIFFUSION_TILE_ROWS rows

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

// lead: columns by which the vector groups start left of x = 0, so that a group inside [0, Nx) is 16-byte aligned in every parent.
// nstrips x nsb: strips of 64 VEC columns x blocks of WAVES row segments; blockIdx.x = ((m nfields + k) nsb + sb) nstrips + strip.
template <typename T, int VEC, bool ENS>
__global__ __launch_bounds__(WAVE *WAVES) void k_diffusion(DiffusionArgs<T> a, T rdx2, T rdy2, int lead, int nstrips, int nsb) {
    const unsigned ntiles = (unsigned)(nstrips * nsb);
    const unsigned L = xcd_remap(blockIdx.x, gridDim.x), mk = L / ntiles, tile = L - mk * ntiles;
    const int k = ENS ? (int)(mk % (unsigned)a.nfields) : (int)mk;
    T c, av = a.a, wv = a.w;
    long mo = 0;
    if constexpr (ENS) {
        const unsigned m = mk / (unsigned)a.nfields;
        mo = (long)m * a.stride_m;
        c = a.coef_tab[mk];
        if (a.params) {   // the products as the host forms them for one grid
            const T dt = a.params[3 * (long)m + 2];
            av = dt * a.a;
            if (a.anchor) wv = dt * a.w;
        }
    } else {
        c = a.coef[k];
    }
    if (c == T(0)) return;   // (uniform over the workgroup) neither read nor written
    const T *__restrict__ old = a.old[k] + mo;
    T *__restrict__ nw = a.nw[k] + mo;
    T *__restrict__ acc = a.acc[k] ? a.acc[k] + mo : nullptr;

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

    auto load_old = [&](int y, T(&v)[VEC]) {   // y in [-1, Ny]
        if (wrapy) y = y < 0 ? Ny - 1 : (y >= Ny ? 0 : y);
        const T *p = old + (long)y * sy;
        if (full) {
            vec_load<T, VEC>(p + xv, v);
        } else {
#pragma unroll
            for (int e = 0; e < VEC; ++e) v[e] = ok[e] ? p[col[e]] : T(0);
        }
    };
    auto load_out = [&](const T *p, T(&v)[VEC]) {   // p: the row of nw or acc
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

    const T cx = c * rdx2, cy = c * rdy2;   // (fast form only)
    T vm[VEC], v0[VEC], vp[VEC];
    load_old(r0 - 1, vm);
    load_old(r0, v0);
    for (int j = r0; j < r1; ++j) {
        load_old(j + 1, vp);
        const long ro = (long)j * sy;
        T west = __shfl_up(v0[VEC - 1], 1), east = __shfl_down(v0[0], 1);
        if (lane == 0) west = okw ? old[ro + colw] : T(0);
        if (lane == WAVE - 1) east = oke ? old[ro + cole] : T(0);
        T un[VEC], ua[VEC];
        load_out(nw + ro, un);
        if (acc) load_out(acc + ro, ua);
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
        store_out(nw + ro, un);
        if (acc) store_out(acc + ro, ua);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            vm[e] = v0[e];
            v0[e] = vp[e];
        }
    }
}

// the 16-byte phase (in elements) all parents of the call share, or -1: then the kernel takes one element per lane
template <typename T>
int common_phase(const DiffusionArgs<T> &a) {
    constexpr int V = 16 / (int)sizeof(T);
    if (a.sy % V != 0 || (a.members > 0 && a.stride_m % V != 0)) return -1;
    auto phase = [](const void *p) { return (int)(((uintptr_t)p / sizeof(T)) % V); };
    const int ph = phase(a.old[0]);
    for (int k = 0; k < a.nfields; ++k) {
        if (phase(a.old[k]) != ph || phase(a.nw[k]) != ph) return -1;
        if (a.acc[k] && phase(a.acc[k]) != ph) return -1;
    }
    return ph;
}

}  // namespace

#define LAUNCH_NAME_(base, sfx) base##sfx
#define LAUNCH_NAME(base, sfx) LAUNCH_NAME_(base, sfx)
#if SWMHD_DIFFUSION_STRICT
#define LAUNCH_SFX strict
#else
#define LAUNCH_SFX fast
#endif

template <typename T>
hipError_t LAUNCH_NAME(launch_diffusion_, LAUNCH_SFX)(const DiffusionArgs<T> &a, hipStream_t s) {
    constexpr int V = 16 / (int)sizeof(T);
    const int rows = a.j1 - a.j0;
    if (rows <= 0 || a.nfields <= 0) return hipSuccess;
    const int ph = common_phase(a), vec = ph >= 0 ? V : 1, lead = ph >= 0 ? ph : 0;
    const long nstrips = ((long)a.Nx + lead + (long)WAVE * vec - 1) / ((long)WAVE * vec);
    const long nsb = ((long)rows + WAVES * WAVE_ROWS - 1) / (WAVES * WAVE_ROWS);
    const long blocks = (long)(a.members > 0 ? a.members : 1) * a.nfields * nstrips * nsb;
    if (blocks > 0x7fffffffL) return hipErrorInvalidConfiguration;
    const T rdx2 = T(1) / (a.dx * a.dx), rdy2 = T(1) / (a.dy * a.dy);
    void (*k)(DiffusionArgs<T>, T, T, int, int, int);
    if (a.members > 0) k = vec == V ? k_diffusion<T, V, true> : k_diffusion<T, 1, true>;
    else k = vec == V ? k_diffusion<T, V, false> : k_diffusion<T, 1, false>;
    hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(WAVE, WAVES), 0, s, a, rdx2, rdy2, lead, (int)nstrips, (int)nsb);
    return hipGetLastError();
}
template hipError_t LAUNCH_NAME(launch_diffusion_, LAUNCH_SFX)<double>(const DiffusionArgs<double> &, hipStream_t);
template hipError_t LAUNCH_NAME(launch_diffusion_, LAUNCH_SFX)<float>(const DiffusionArgs<float> &, hipStream_t);

}  // namespace swmhd
