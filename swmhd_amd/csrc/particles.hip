// Lagrangian particles: positions advected by the flow as one more prognostic of the RK3, and fields sampled at them
// (swmhd_particles_rk3_*, swmhd_particles_sample_* and their ensemble forms; include/swmhd_particles.h states the scheme, the index
// rules and the fold).  Per particle and stage, on the state the stage STARTED from:
//     G = (U(x, y), V(x, y))      bilinear between the four nodes around the particle
//     x += dt (gamma Gx + zeta Gx-), y likewise, folded into the domain;  G- <- G
// One lane per particle, one plain launch, no atomics, no LDS.  Built with the STRICT flags (Makefile): no contraction, IEEE divide;
// every operation below is rounded once in the order written, so the result is bitwise the numpy restatement of the tests.  There is
// no fast variant: a lane's time is the latency of its gathers -- eight element-granular loads (twenty in the conservative form) that
// do not coalesce and rest on L2 and the Infinity Cache -- not its ~60 flops.  So all indices are formed first and all gathers issued
// before the first use of any of them.
// Safety: an address is formed only from a finite position, and every index is brought into range IN FLOATING POINT (fmod for a wrapped
// direction, a clamp for the others) before it is converted to an integer; see particle_axis.
#include "common.hpp"

namespace swmhd {
namespace {

// the two nodes around a coordinate in one direction: indices i0, i1 (= i0 + 1, wrapped), the index west / south of i0 for the
// thickness of the conservative form, and the weight t of i1
struct ParticleAxis {
    int i0, i1, iw;
    double t;
};

// p: the coordinate; o, d: origin and spacing; center: the field's nodes stand at cell centres in this direction; N, H: cells and halo
__device__ __forceinline__ ParticleAxis particle_axis(double p, double o, double d, bool center, int N, int H, int mode) {
    double s = (p - o) / d;
    if (center) s = s - 0.5;
    const double fl = floor(s);      // (finite or +-inf for a finite p; never NaN)
    ParticleAxis a;
    a.t = s - fl;
    if (mode == PARTICLE_WRAP) {
        double m = fmod(fl, (double)N);      // exact; |m| < N, the sign of fl
        if (m < 0.0) m = m + (double)N;      // exact: integers below 2^31
        m = m >= 0.0 ? m : 0.0;              // (fl = +-inf: fmod is NaN)
        a.i0 = (int)m;                       // 0 .. N - 1
        a.i1 = a.i0 + 1 == N ? 0 : a.i0 + 1;
        a.iw = a.i0 == 0 ? N - 1 : a.i0 - 1;
    } else {
        const double c = fmin(fmax(fl, (double)-H), (double)(N + H - 2));      // H >= 1: the range is not empty
        a.i0 = (int)c;                       // -H .. N + H - 2
        a.i1 = a.i0 + 1;                     // .. N + H - 1: the last cell of the parent
        a.iw = a.i0 - 1 < -H ? -H : a.i0 - 1;
    }
    return a;
}

__device__ __forceinline__ double particle_bilinear(double tx, double ty, double f00, double f10, double f01, double f11) {
    const double ox = 1.0 - tx, oy = 1.0 - ty;
    const double lo = ox * f00 + tx * f10;
    const double hi = ox * f01 + tx * f11;
    return oy * lo + ty * hi;
}

// into [o, o + L]: periodic image or one reflection at the wall crossed, then the clamp (which leaves a NaN a NaN)
__device__ __forceinline__ double particle_fold(double x, double o, double L, int mode) {
    const double hi = o + L;
    if (mode == PARTICLE_BOUNDED) {
        if (x < o) x = 2.0 * o - x;
        else if (x > hi) x = 2.0 * hi - x;
    } else {
        x = x - L * floor((x - o) / L);
    }
    return x < o ? o : (x > hi ? hi : x);
}

// member and particle of a lane: false beyond the last particle
__device__ __forceinline__ bool particle_of_lane(const ParticleGrid &a, unsigned &m, long &p) {
    m = a.members > 0 ? blockIdx.x / a.nblk : 0u;
    const unsigned b = blockIdx.x - m * a.nblk;
    p = (long)b * PARTICLES_BLOCK + threadIdx.x;
    return p < a.P;
}

template <typename T>
__global__ __launch_bounds__(PARTICLES_BLOCK) void k_particles(ParticleArgs<T> a) {
    unsigned m;
    long p;
    if (!particle_of_lane(a, m, p)) return;
    const long po = (long)m * a.P + p;
    const double x = a.x[po], y = a.y[po];
    if (!(__builtin_isfinite(x) && __builtin_isfinite(y))) return;      // not read, not advanced, not written
    const long mo = (long)m * a.stride_m, sy = a.sy;
    const T *__restrict__ q1 = a.q1 + mo, *__restrict__ q2 = a.q2 + mo;
    // U at (Face, Center), V at (Center, Face)
    const ParticleAxis ux = particle_axis(x, a.x0, a.dx, false, a.Nx, a.Hx, a.mode_x), uy = particle_axis(y, a.y0, a.dy, true, a.Ny, a.Hy, a.mode_y);
    const ParticleAxis vx = particle_axis(x, a.x0, a.dx, true, a.Nx, a.Hx, a.mode_x), vy = particle_axis(y, a.y0, a.dy, false, a.Ny, a.Hy, a.mode_y);
    const long ur0 = (long)uy.i0 * sy, ur1 = (long)uy.i1 * sy, vr0 = (long)vy.i0 * sy, vr1 = (long)vy.i1 * sy;
    // every gather, before anything waits on one
    const T u00 = q1[ur0 + ux.i0], u10 = q1[ur0 + ux.i1], u01 = q1[ur1 + ux.i0], u11 = q1[ur1 + ux.i1];
    const T v00 = q2[vr0 + vx.i0], v10 = q2[vr0 + vx.i1], v01 = q2[vr1 + vx.i0], v11 = q2[vr1 + vx.i1];
    const bool prev = a.zeta != 0.0;      // (uniform)
    double gxm = 0.0, gym = 0.0;
    if (prev) {
        gxm = a.gx[po];
        gym = a.gy[po];
    }
    double U00 = (double)u00, U10 = (double)u10, U01 = (double)u01, U11 = (double)u11;
    double V00 = (double)v00, V10 = (double)v10, V01 = (double)v01, V11 = (double)v11;
    if (a.cons) {      // (uniform) the frames' velocities: q / (0.5 (h west | south of the face + h at it))
        const T *__restrict__ h = a.h + mo;
        const long vrw = (long)vy.iw * sy;
        const T hw0 = h[ur0 + ux.iw], hc0 = h[ur0 + ux.i0], he0 = h[ur0 + ux.i1];
        const T hw1 = h[ur1 + ux.iw], hc1 = h[ur1 + ux.i0], he1 = h[ur1 + ux.i1];
        const T hs0 = h[vrw + vx.i0], hm0 = h[vr0 + vx.i0], hn0 = h[vr1 + vx.i0];
        const T hs1 = h[vrw + vx.i1], hm1 = h[vr0 + vx.i1], hn1 = h[vr1 + vx.i1];
        U00 = U00 / (0.5 * ((double)hw0 + (double)hc0));
        U10 = U10 / (0.5 * ((double)hc0 + (double)he0));
        U01 = U01 / (0.5 * ((double)hw1 + (double)hc1));
        U11 = U11 / (0.5 * ((double)hc1 + (double)he1));
        V00 = V00 / (0.5 * ((double)hs0 + (double)hm0));
        V10 = V10 / (0.5 * ((double)hs1 + (double)hm1));
        V01 = V01 / (0.5 * ((double)hm0 + (double)hn0));
        V11 = V11 / (0.5 * ((double)hm1 + (double)hn1));
    }
    const double Gx = particle_bilinear(ux.t, uy.t, U00, U10, U01, U11);
    const double Gy = particle_bilinear(vx.t, vy.t, V00, V10, V01, V11);
    const double dt = a.params ? (double)a.params[3 * (long)m + 2] : a.dt;
    double rx = a.gamma * Gx, ry = a.gamma * Gy;
    if (prev) {
        rx = rx + a.zeta * gxm;
        ry = ry + a.zeta * gym;
    }
    const double xn = x + dt * rx, yn = y + dt * ry;
    a.x[po] = particle_fold(xn, a.x0, (double)a.Nx * a.dx, a.mode_x);
    a.y[po] = particle_fold(yn, a.y0, (double)a.Ny * a.dy, a.mode_y);
    a.gx[po] = Gx;
    a.gy[po] = Gy;
}

template <typename T>
__global__ __launch_bounds__(PARTICLES_BLOCK) void k_particles_sample(ParticleSampleArgs<T> a) {
    unsigned m;
    long p;
    if (!particle_of_lane(a, m, p)) return;
    const long po = (long)m * a.P + p;
    const double x = a.x[po], y = a.y[po];
    double *__restrict__ out = a.out + (long)m * a.nfields * a.P + p;
    if (!(__builtin_isfinite(x) && __builtin_isfinite(y))) {
        for (int k = 0; k < a.nfields; ++k) out[(long)k * a.P] = __builtin_nan("");
        return;
    }
    const long mo = (long)m * a.stride_m, sy = a.sy;
    // the axes of the two locations in each direction: Face, Center
    const ParticleAxis xf = particle_axis(x, a.x0, a.dx, false, a.Nx, a.Hx, a.mode_x), xc = particle_axis(x, a.x0, a.dx, true, a.Nx, a.Hx, a.mode_x);
    const ParticleAxis yf = particle_axis(y, a.y0, a.dy, false, a.Ny, a.Hy, a.mode_y), yc = particle_axis(y, a.y0, a.dy, true, a.Ny, a.Hy, a.mode_y);
    for (int k = 0; k < a.nfields; ++k) {      // (uniform: the tables are read from the kernel argument with a scalar index)
        const int loc = a.loc[k];
        const ParticleAxis fx = (loc & 1) ? xc : xf, fy = (loc & 2) ? yc : yf;
        const T *__restrict__ f = a.f[k] + mo;
        const long r0 = (long)fy.i0 * sy, r1 = (long)fy.i1 * sy;
        const T f00 = f[r0 + fx.i0], f10 = f[r0 + fx.i1], f01 = f[r1 + fx.i0], f11 = f[r1 + fx.i1];
        out[(long)k * a.P] = particle_bilinear(fx.t, fy.t, (double)f00, (double)f10, (double)f01, (double)f11);
    }
}

// workgroups of one member and of the launch; false from 2^31 on
inline bool particle_blocks(ParticleGrid &g, long &blocks) {
    const long nblk = (g.P + PARTICLES_BLOCK - 1) / PARTICLES_BLOCK, members = g.members > 0 ? g.members : 1;
    if (nblk >= (1L << 31) || nblk * members >= (1L << 31)) return false;      // (in this order: the product cannot overflow)
    g.nblk = (unsigned)nblk;
    blocks = nblk * members;
    return true;
}

}  // namespace

template <typename T>
hipError_t launch_particles(const ParticleArgs<T> &args, hipStream_t s) {
    ParticleArgs<T> a = args;
    long blocks;
    if (a.P <= 0) return hipSuccess;
    if (!particle_blocks(a, blocks)) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_particles<T>, dim3((unsigned)blocks), dim3(PARTICLES_BLOCK), 0, s, a);
    return hipGetLastError();
}
template hipError_t launch_particles<double>(const ParticleArgs<double> &, hipStream_t);
template hipError_t launch_particles<float>(const ParticleArgs<float> &, hipStream_t);

template <typename T>
hipError_t launch_particles_sample(const ParticleSampleArgs<T> &args, hipStream_t s) {
    ParticleSampleArgs<T> a = args;
    long blocks;
    if (a.P <= 0) return hipSuccess;
    if (!particle_blocks(a, blocks)) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_particles_sample<T>, dim3((unsigned)blocks), dim3(PARTICLES_BLOCK), 0, s, a);
    return hipGetLastError();
}
template hipError_t launch_particles_sample<double>(const ParticleSampleArgs<double> &, hipStream_t);
template hipError_t launch_particles_sample<float>(const ParticleSampleArgs<float> &, hipStream_t);

}  // namespace swmhd
