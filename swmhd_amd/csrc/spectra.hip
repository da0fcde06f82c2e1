// Zonal spectra: the one-sided power spectrum along x of the output fields, averaged over rows, made on the device in two launches over
// the four prognostic parents (swmhd_zonal_spectra_*, include/swmhd_spectra.h).
//
//   P_F[k] = (1/rows) Σ_j c_k |(1/Nx) Σ_i F(i,j) exp(−2πi k (i−1)/Nx)|²,  k = 0 .. Nx/2,  c_k = 1 at the two ends, else 2
// F(i,j): the float64 frame values u v h A s B_x B_y (mask bits = SWMHD_OUT_*), per cell the frame definitions of frame_device.inc as
// spectra_device.inc::frame_value states them for one cell of one field; the object is built without FMA contraction and with IEEE
// divide / sqrt (Makefile: STRICT), so the input of the transform is bitwise the float64 frame (tests/output_cases.np_output_fields).
//
// Pass 1 (k_spectra_rows): unit (member, field, w) takes the rows j0 + w, j0 + w + W, ... (launch_plan.hpp: spectra_plan) one after the
// other.  A unit is a workgroup of SPECTRA_NT threads from Nx = 512 on and one wave up to Nx = 256 (four units of consecutive w per
// workgroup, each with its own LDS).  Per row: the frame values go to LDS as Nx doubles = M = Nx/2 complex z[n] = (F(2n+1), F(2n+2)); an
// in-place radix-2 decimation-in-frequency FFT of length M (log2 M stages, a barrier after each) leaves Z[k] at position bitreverse(k);
// the untangling pass forms X[k] = E + w_Nx^k O from Z[k] and Z[M − k] for the k of the thread (k = lane, lane + threads of the unit, ...: at most
// SPECTRA_ACC of them) and adds c_k |X[k]/Nx|² to the thread's accumulator of that k.  After the last row the accumulators go to the
// workspace.  Pass 2 (k_spectra_sum): the W partials of every k in the fixed tree of spectra_depth, divided by rows.
// LDS per unit: 8 Nx bytes of row + 4 Nx bytes of twiddles (w_Nx^k, 0 <= k < Nx/4; the other quarter is −i times these: a swap and a sign).
// Banks: in every stage lane t takes butterfly t (and t + 256, ...: four in flight, read before the first is written), so the lanes of a wave read consecutive 16-byte elements wherever the half-span is 16
// elements or more (a 256-byte bank row per 16 lanes: conflict-free); the power-of-two stride lies between the two operands of ONE
// thread, which are two instructions.  In the last four stages (half-span 8 .. 1) 16 lanes cover two bank rows: two-way.
// The member, the field and the row are taken from blockIdx: scalar values, so every branch on them is a scalar branch.
#include "api_args.hpp"
#include "common.hpp"

namespace swmhd {
namespace {

template <typename T>
struct SpectraArgs {
    const T *q1, *q2, *h, *A;   // interior cell (1,1) of the parents, as OpArgs
    double *ws, *out;
    int Nx, Ny, j0, j1;
    long sy, osk;
    double dx, dy;
    int form, which, wrap;      // wrap: bit 0 = x, bit 1 = y
    int W, nf, log2n;
    long stride_m, osm;
};

#include "spectra_device.inc"   // cplx, twiddle, frame_value, load_row, dif_stage, untangle: shared with spectra2d.hip

// TPR: threads of one row.  SPECTRA_NT (one row per workgroup) from Nx = 512 on; 64 (one wave per row, SPECTRA_NT / 64 rows of
// consecutive w side by side in one workgroup) up to Nx = 256, where a row has at most 64 butterflies per stage (spectra_plan: units).
// (three workgroups per CU: what the 48 KiB of LDS at Nx = 4096 admit; the registers are held to that)
template <typename T, bool ENS, int TPR>
__global__ __launch_bounds__(SPECTRA_NT, 3) void k_spectra_rows(SpectraArgs<T> a) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int UPB = SPECTRA_NT / TPR;                        // rows side by side
    constexpr int ACC = TPR == SPECTRA_NT ? SPECTRA_ACC : 3;     // modes of a thread: ceil((Nx/2 + 1) / TPR)
    constexpr int NB = TPR == SPECTRA_NT ? 4 : 1;                // butterflies of a thread in flight
    // (the unit through readfirstlane where it is a wave: its row, pointers and branches are then scalar to the compiler too)
    const int unit = UPB == 1 ? 0 : __builtin_amdgcn_readfirstlane(threadIdx.x / TPR), lane = threadIdx.x % TPR;
    const int N = a.Nx, M = N >> 1, Q = N >> 2, LM = a.log2n - 1;   // M = 2^LM
    double *x_row = lds + (long)unit * (N + 2 * Q);
    cplx *z = reinterpret_cast<cplx *>(x_row);
    cplx *tw = z + M;
    // (member, field, w) of this unit: blockIdx.x = (m * nf + f) * wblocks + wb, w = wb * UPB + unit
    const int wblocks = (a.W + UPB - 1) / UPB;
    long b = blockIdx.x;
    const int w = (int)(b % wblocks) * UPB + unit;
    b /= wblocks;
    const int f = (int)(b % a.nf), m = (int)(b / a.nf);
    if constexpr (ENS) {
        const long o = (long)m * a.stride_m;
        a.q1 += o; a.q2 += o; a.h += o; a.A += o;
    }
    const int bit = field_bit(a.which, f);
    const bool cons = a.form == SWMHD_CONSERVATIVE;

    for (int k = lane; k < Q; k += TPR) tw[k] = twiddle_entry(k, N);

    double acc[ACC];
#pragma unroll
    for (int r = 0; r < ACC; ++r) acc[r] = 0.0;
    const double inv = 1.0 / (double)N;   // exact

    // every unit of a workgroup makes the trips of unit 0 (the barriers are the workgroup's); a unit beyond W, or past its last row, idles
    const int rows = a.j1 - a.j0, trips = (rows + a.W - 1) / a.W;
    for (int trip = 0; trip < trips; ++trip) {
        const int row = w + trip * a.W;
        const bool active = w < a.W && row < rows;
        if (active) load_row<TPR>(a, x_row, bit, cons, a.j0 + row, lane);
        __syncthreads();   // (also: the twiddles of the first row)

        // decimation in frequency: half-span hs = M/2 .. 1; butterfly t: block t / hs, offset j = t mod hs; twiddle w_M^(j M/(2 hs)) = w_Nx^(j M/hs)
        for (int lh = LM - 1; lh >= 0; --lh) {
            if (active) dif_stage<TPR, NB>(z, tw, lane, M >> 1, lh, LM - lh, Q);
            __syncthreads();
        }

        // untangle: Z[k] is at bitreverse_LM(k).  k = 0: X[0] = Re Z[0] + Im Z[0]; k = M: Re Z[0] − Im Z[0]
        if (active) {
#pragma unroll
            for (int r = 0; r < ACC; ++r) {
                const int k = lane + r * TPR;
                if (k <= M) {
                    const cplx X = untangle(z, tw, k, M, LM, Q, inv);
                    acc[r] += ((k == 0 || k == M) ? 1.0 : 2.0) * (X.re * X.re + X.im * X.im);
                }
            }
        }
        __syncthreads();   // the next row overwrites z
    }

    if (w < a.W) {
        double *ws = a.ws + ((b * a.W) + w) * (long)(M + 1);   // b: member * nf + field
#pragma unroll
        for (int r = 0; r < ACC; ++r) {
            const int k = lane + r * TPR;
            if (k <= M) ws[k] = acc[r];
        }
    }
}

// one (member, field) per blockIdx.y-free list: blockIdx.x = mf * kblocks + kb; thread = kk + SPECTRA_P2_K * g
__global__ __launch_bounds__(SPECTRA_P2_K * SPECTRA_P2_G) void k_spectra_sum(const double *__restrict__ ws, double *__restrict__ out, int nk,
                                                                              int W, int nf, int kblocks, int rows, long osk, long osm) {
    __shared__ double part[SPECTRA_P2_G][SPECTRA_P2_K];
    const int kk = threadIdx.x % SPECTRA_P2_K, g = threadIdx.x / SPECTRA_P2_K;
    const long mf = blockIdx.x / kblocks;
    const int kb = (int)(blockIdx.x - mf * kblocks);
    const int k = kb * SPECTRA_P2_K + kk;
    double s = 0.0;
    if (k < nk) {
        const double *p = ws + mf * W * (long)nk + k;
        for (int w = g; w < W; w += SPECTRA_P2_G) s += p[(long)w * nk];
    }
    part[g][kk] = s;
    __syncthreads();
#pragma unroll
    for (int d = SPECTRA_P2_G / 2; d >= 1; d >>= 1) {
        if (g < d) part[g][kk] += part[g + d][kk];
        __syncthreads();
    }
    if (g == 0 && k < nk) {
        const long m = mf / nf, f = mf - m * nf;
        out[m * osm + f * osk + k] = part[0][kk] / (double)rows;
    }
}

struct SpectraOut {
    int which;
    double *ws, *out;
    int64_t osk, osm = 0;
};

template <typename T>
int spectra_common(const T *q1, const T *q2, const T *h, const T *A, const Grid &g, int form, const Rows &r, const SpectraOut &o, int flags,
                   void *stream, const Ens *ens = nullptr) {
    if (!frame_source_ok(q1, q2, h, A, g, form) || !o.out || !o.ws || !g.rows_ok(r.j0, r.j1)) return SWMHD_EINVAL;
    if (o.which <= 0 || (o.which & ~SWMHD_ZS_ALL) || (flags & ~FRAME_FLAGS)) return SWMHD_EINVAL;
    const int nf = __builtin_popcount((unsigned)o.which);
    if (o.osk < (int64_t)g.Nx / 2 + 1 || !frame_members_ok(ens, g) || (ens && o.osm < (int64_t)nf * o.osk)) return SWMHD_EINVAL;
    if (!spectra_halo_ok(g, flags)) return SWMHD_EHALO;
    const int members = ens ? ens->members : 1;
    const SpectraPlan p = spectra_plan(g.Nx, r.j1 - r.j0, nf, members);
    if (p.unsupported) return SWMHD_ENOTSUP;
    if (p.none) return SWMHD_OK;
    if (p.too_many) return hiprc(hipErrorInvalidConfiguration);
    SpectraArgs<T> a;
    set_frame_source(a, q1, q2, h, A, g, form, o.which, flags, ens);
    a.ws = o.ws; a.out = o.out;
    a.j0 = r.j0; a.j1 = r.j1;
    a.osk = (long)o.osk; a.osm = ens ? (long)o.osm : 0;
    a.W = p.W; a.nf = nf; a.log2n = p.log2n;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid1((unsigned)p.blocks1), grid2((unsigned)p.blocks2);
    constexpr int WAVE = 64;
    if (p.units == 1) {
        if (ens) hipLaunchKernelGGL((k_spectra_rows<T, true, SPECTRA_NT>), grid1, dim3(SPECTRA_NT), (size_t)p.lds_bytes, s, a);
        else hipLaunchKernelGGL((k_spectra_rows<T, false, SPECTRA_NT>), grid1, dim3(SPECTRA_NT), (size_t)p.lds_bytes, s, a);
    } else {
        static_assert(SPECTRA_UNITS_SMALL == SPECTRA_NT / WAVE, "a small row is one wave's");
        if (ens) hipLaunchKernelGGL((k_spectra_rows<T, true, WAVE>), grid1, dim3(SPECTRA_NT), (size_t)p.lds_bytes, s, a);
        else hipLaunchKernelGGL((k_spectra_rows<T, false, WAVE>), grid1, dim3(SPECTRA_NT), (size_t)p.lds_bytes, s, a);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hiprc(e);
    hipLaunchKernelGGL(k_spectra_sum, grid2, dim3(SPECTRA_P2_K * SPECTRA_P2_G), 0, s, o.ws, o.out, p.nk, p.W, nf,
                       (p.nk + SPECTRA_P2_K - 1) / SPECTRA_P2_K, r.j1 - r.j0, (long)o.osk, a.osm);
    return hiprc(hipGetLastError());
}

}  // namespace
}  // namespace swmhd

extern "C" {

int64_t swmhd_zonal_spectra_workspace(int Nx, int rows, int nfields, int members) {
    if (Nx <= 0 || rows <= 0 || nfields <= 0 || members <= 0) return 0;
    return (int64_t)swmhd::spectra_W(rows) * nfields * members * ((int64_t)Nx / 2 + 1);
}

#define SWMHD_DEF_SPECTRA(sfx, T)                                                                                                    \
    int swmhd_zonal_spectra_##sfx(const T *q1, const T *q2, const T *h, const T *A, int Nx, int Ny, int Hx, int Hy, int64_t sy,     \
                                  T dx, T dy, int formulation, int j0, int j1, int which, double *workspace, double *out,           \
                                  int64_t out_stride_k, int flags, void *stream) {                                                  \
        return swmhd::spectra_common<T>(q1, q2, h, A, swmhd::Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, formulation, swmhd::Rows{j0, j1},    \
                                        swmhd::SpectraOut{which, workspace, out, out_stride_k}, flags, stream);                     \
    }                                                                                                                                \
    int swmhd_ensemble_zonal_spectra_##sfx(const T *q1, const T *q2, const T *h, const T *A, int members, int64_t stride_m, int Nx, \
                                           int Ny, int Hx, int Hy, int64_t sy, T dx, T dy, int formulation, int j0, int j1,         \
                                           int which, double *workspace, double *out, int64_t out_stride_k, int64_t out_stride_m,   \
                                           int flags, void *stream) {                                                               \
        const swmhd::Ens e{members, stride_m};                                                                                       \
        return swmhd::spectra_common<T>(q1, q2, h, A, swmhd::Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, formulation, swmhd::Rows{j0, j1},    \
                                        swmhd::SpectraOut{which, workspace, out, out_stride_k, out_stride_m}, flags, stream, &e);   \
    }

SWMHD_DEF_SPECTRA(f64, double)
SWMHD_DEF_SPECTRA(f32, float)

}  // extern "C"
