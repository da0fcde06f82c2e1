// The coefficient draw of the stochastic forcing (swmhd_stochastic_coefficients_*, include/swmhd_stochastic.h): once per time step, one
// workgroup per member.  Every thread reads the member's step counter n, a workgroup barrier follows, and only then thread 0 stores
// n + 1: no read of the counter can see its update.  Thread t draws the modes t, t + 256, ... of every group: Philox4x32-10 with
// key = seed and counter = (n_lo, n_hi, mode + 65536 group, substream), two uniforms of 53 bits from the four words, and the
// coefficients in double, one rounding per operation (this object is built with the STRICT flags: Makefile), cast to the element
// type at the end.  Integer arithmetic and a handful of double multiplications: nothing here is hot.
#include "common.hpp"

namespace swmhd {
namespace {

constexpr int COEF_NT = 256;

__device__ __forceinline__ void philox4x32_10(unsigned (&c)[4], unsigned k0, unsigned k1) {
    constexpr unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const unsigned hi0 = __umulhi(M0, c[0]), lo0 = M0 * c[0], hi1 = __umulhi(M1, c[2]), lo1 = M1 * c[2];
        const unsigned n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
        k0 += W0; k1 += W1;
    }
}

// ((hi >> 5) 2^26 + (lo >> 6)) 2^-53: 53 bits, exact in double
__device__ __forceinline__ double u53(unsigned hi, unsigned lo) {
    return ((double)(hi >> 5) * 67108864.0 + (double)(lo >> 6)) * (1.0 / 9007199254740992.0);
}

template <typename T>
__global__ __launch_bounds__(COEF_NT) void k_stochastic_coefficients(StochasticCoefArgs<T> a) {
    const unsigned mem = blockIdx.x;
    const unsigned long long n = a.counter[mem];
    __syncthreads();   // every read of the counter is behind us
    if (threadIdx.x == 0) a.counter[mem] = n + 1ull;
    const unsigned sub = a.substreams ? a.substreams[mem] : a.substream;
    for (int g = 0; g < a.ngroups; ++g) {
        const int M = a.M[g];
        const double *amp0 = a.amp0[g] + (long)mem * a.amp_stride_m;
        T *out = a.coef[g] + (long)mem * a.coef_stride_m;
        for (int m = (int)threadIdx.x; m < M; m += COEF_NT) {
            unsigned c[4] = {(unsigned)n, (unsigned)(n >> 32), (unsigned)m + 65536u * (unsigned)g, sub};
            philox4x32_10(c, a.seed_lo, a.seed_hi);
            const double x = 2.0 * u53(c[0], c[1]) - 1.0, y = 2.0 * u53(c[2], c[3]) - 1.0;   // exact
            const double cm = amp0[m] * a.sdt;
            const double P = cm * x, Q = cm * y;
            if (a.kind[g] == 0) {
                out[m] = (T)P; out[M + m] = (T)Q;
            } else {
                const double kx = a.ktx[g][m], ky = a.kty[g][m];
                out[m] = (T)(-(ky * Q)); out[M + m] = (T)(ky * P);
                out[2 * M + m] = (T)(kx * Q); out[3 * M + m] = (T)(-(kx * P));
            }
        }
    }
}

}  // namespace

template <typename T>
hipError_t launch_stochastic_coefficients(const StochasticCoefArgs<T> &a, hipStream_t s) {
    hipLaunchKernelGGL(k_stochastic_coefficients<T>, dim3((unsigned)a.members), dim3(COEF_NT), 0, s, a);
    return hipGetLastError();
}
template hipError_t launch_stochastic_coefficients<double>(const StochasticCoefArgs<double> &, hipStream_t);
template hipError_t launch_stochastic_coefficients<float>(const StochasticCoefArgs<float> &, hipStream_t);

}  // namespace swmhd
