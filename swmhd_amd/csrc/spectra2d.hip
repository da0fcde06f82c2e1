// 2-D and isotropic power spectra of the output fields, made on the device in three launches over the four prognostic parents
// (swmhd_spectra2d_*, include/swmhd_spectra2d.h: the definitions, the shell statement and the bound).
//
//   F^[kx,ky] = 1/(Nx Ny) Σ_i Σ_j F(i,j) exp(−2πi (kx (i−1)/Nx + ky (j−1)/Ny)),  P2 = c_kx |F^|²,  E[s] = Σ over the modes of shell s of P2
// The object is built STRICT like spectra.o: the input of the transform is bitwise the float64 frame, the shell of a mode is bitwise a
// numpy restatement, and the butterfly is the statement the error constant is derived for (spectra_device.inc, shared with spectra.hip).
//
// Pass 1 (k_s2d_rows): a workgroup takes R consecutive rows of one (member, field) (launch_plan.hpp: spectra2d_plan), each into an LDS
// buffer of its own; the rows are transformed as k_spectra_rows does it -- a wave per row, SPECTRA_UNITS_SMALL rows side by side, up to
// Nx = 256; the whole workgroup on one row after the other above.  Then item (k, r), r fastest, untangles mode k of row r and stores
// X[k]/Nx to the workspace at ((member * nf + field) * nkx + k) * Ny + row: R consecutive 16-byte elements of one line per k.  The R row
// buffers are N + pad doubles apart, so the R lanes that read the same element of R rows fall on different banks.
// Pass 2 (k_s2d_cols): unit (member, field, kx) -- a wave, SPECTRA_UNITS_SMALL to a workgroup, up to Ny = 256; a workgroup above --
// loads its column (Ny contiguous complex values) into LDS, transforms it in place (dif_stage; log2 Ny stages, a barrier after each),
// takes Z[ky] from position bitreverse(ky), scales by 1/Ny and holds p[ky] = c_kx (re² + im²) in registers (ky = lane, lane + TPR, ...).
// It stores the column of out_2d from there.  For the shells it writes p in natural order over the column in LDS and the shell of every
// |my| = 0 .. Ny/2 beside it (a non-decreasing sequence); the lane of shell s finds the run [lo, hi) of |my| of that shell by bisection
// and adds p[my = a], a = lo .. hi − 1, then p[my = −a] for the a of the run in 1 .. Ny/2 − 1, one after the other from 0.0, and stores
// the sum -- 0.0 where the run is empty -- to partial[((member * nf + field) * nkx + kx) * NS + s].
// Pass 3 (k_s2d_shells): k_spectra_sum's order over the nkx partials of every s, without the division.
// The member, the field and kx are taken from blockIdx (through readfirstlane where a unit is a wave): scalar values and scalar branches.
#include "api_args.hpp"
#include "common.hpp"

#include <atomic>
#include <cmath>

namespace swmhd {
namespace {

template <typename T>
struct S2dArgs {
    const T *q1, *q2, *h, *A;   // interior cell (1,1) of the parents, as OpArgs
    double *ws;                 // the complex half-plane
    int Nx, Ny;
    long sy;
    double dx, dy;
    int form, which, wrap;      // wrap: bit 0 = x, bit 1 = y
    int nf, log2n, R, log2r, pad;
    long stride_m;
};

struct S2dColArgs {
    const double *modes;        // (member, field, kx, j) complex
    double *partial;            // (member, field, kx, s), or null
    double *out2;               // or null
    int Ny, log2ny, nkx, NS, nf;
    long units;                 // members * nf * nkx
    long o2kx, o2f, o2m;
    double wx, wy;
};

#include "spectra_device.inc"

template <typename T, bool ENS, int TPR>
__global__ __launch_bounds__(SPECTRA_NT, 2) void k_s2d_rows(S2dArgs<T> a) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int UPB = SPECTRA_NT / TPR;                        // rows side by side
    constexpr int NB = TPR == SPECTRA_NT ? 4 : 1;                // butterflies of a thread in flight
    const int unit = UPB == 1 ? 0 : __builtin_amdgcn_readfirstlane(threadIdx.x / TPR), lane = threadIdx.x % TPR;
    const int N = a.Nx, M = N >> 1, Q = N >> 2, LM = a.log2n - 1, R = a.R;
    const int rs = N + a.pad;                                    // doubles from one row buffer to the next
    cplx *tw = reinterpret_cast<cplx *>(lds + (long)R * rs);
    // (member, field, row block): blockIdx.x = (m * nf + f) * (Ny / R) + rb
    const int rblocks = a.Ny / R;
    long b = blockIdx.x;
    const int y0 = (int)(b % rblocks) * R;
    b /= rblocks;
    const int f = (int)(b % a.nf), m = (int)(b / a.nf);
    if constexpr (ENS) {
        const long o = (long)m * a.stride_m;
        a.q1 += o; a.q2 += o; a.h += o; a.A += o;
    }
    const int bit = field_bit(a.which, f);
    const bool cons = a.form == SWMHD_CONSERVATIVE;

    for (int k = threadIdx.x; k < Q; k += SPECTRA_NT) tw[k] = twiddle_entry(k, N);

    // every unit makes the trips of unit 0 (the barriers are the workgroup's); R is a multiple of UPB (launch_plan.hpp), so none idles
    for (int r0 = 0; r0 < R; r0 += UPB) {
        const int r = r0 + unit;
        const bool active = r < R;
        double *x_row = lds + (long)r * rs;
        cplx *z = reinterpret_cast<cplx *>(x_row);
        if (active) load_row<TPR>(a, x_row, bit, cons, y0 + r, lane);
        __syncthreads();   // (also: the twiddles)
        for (int lh = LM - 1; lh >= 0; --lh) {
            if (active) dif_stage<TPR, NB>(z, tw, lane, M >> 1, lh, LM - lh, Q);
            __syncthreads();
        }
    }

    // transposed store: item = k * R + r; (b: member * nf + field)
    const double inv = 1.0 / (double)N;   // exact
    cplx *out = reinterpret_cast<cplx *>(a.ws) + (b * (M + 1)) * (long)a.Ny + y0;
    const int items = (M + 1) << a.log2r;
    for (int it = threadIdx.x; it < items; it += SPECTRA_NT) {
        const int r = it & (R - 1), k = it >> a.log2r;
        const cplx *z = reinterpret_cast<const cplx *>(lds + (long)r * rs);
        out[(long)k * a.Ny + r] = untangle(z, tw, k, M, LM, Q, inv);
    }
}

// the shell of mode (mx, my): the statement of the header, in IEEE double without contraction (launch_plan.hpp: spectra2d_shell)
__device__ __forceinline__ int shell_of(int mx, int my, double wx, double wy) {
    const double a = wx * (double)(mx * mx);
    const double b = wy * (double)(my * my);
    const double r2 = a + b;
    return (int)floor(sqrt(r2) + 0.5);
}

// TPR: threads of one column.  PER: values of a thread, Ny / TPR at most.
template <int TPR, bool TABLE>
__global__ __launch_bounds__(SPECTRA_NT, 2) void k_s2d_cols(S2dColArgs a) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int UPB = SPECTRA_NT / TPR;
    constexpr int NB = TPR == SPECTRA_NT ? 4 : 1;
    constexpr int PER = (TPR == SPECTRA_NT ? (1 << SPECTRA_MAX_LOG2) : SPECTRA_SMALL_NX) / TPR;
    const int unit = UPB == 1 ? 0 : __builtin_amdgcn_readfirstlane(threadIdx.x / TPR), lane = threadIdx.x % TPR;
    const int L = a.Ny, Q = L >> 2, LY = a.log2ny, half = L >> 1;
    cplx *z = reinterpret_cast<cplx *>(lds + (long)unit * (TABLE ? 2 * L + 2 * Q : 2 * L));
    cplx *tw = z + L;                                            // (not read without a table)
    const long u = (long)blockIdx.x * UPB + unit;                // (member * nf + field) * nkx + kx
    const bool active = u < a.units;
    const long mf = u / a.nkx;
    const int kx = (int)(u - mf * a.nkx);

    if (TABLE && active)
        for (int k = lane; k < Q; k += TPR) tw[k] = twiddle_entry(k, L);
    if (active) {
        const cplx *col = reinterpret_cast<const cplx *>(a.modes) + u * L;
        for (int j = lane; j < L; j += TPR) z[j] = col[j];
    }
    __syncthreads();
    // decimation in frequency of length L: half-span hs = L/2 .. 1; twiddle w_L^(j L/(2 hs))
    for (int lh = LY - 1; lh >= 0; --lh) {
        if (active) dif_stage<TPR, NB, TABLE>(z, tw, lane, half, lh, LY - 1 - lh, Q);
        __syncthreads();
    }

    const double inv = 1.0 / (double)L, ck = (kx == 0 || kx == a.nkx - 1) ? 1.0 : 2.0;   // inv: exact
    double p[PER];
#pragma unroll
    for (int r = 0; r < PER; ++r) {
        const int ky = lane + r * TPR;
        p[r] = 0.0;
        if (active && ky < L) {
            const cplx Z = z[__brev((unsigned)ky) >> (32 - LY)];
            const double re = Z.re * inv, im = Z.im * inv;
            p[r] = ck * (re * re + im * im);
        }
    }
    if (a.out2 && active) {
        const long m = mf / a.nf, f = mf - m * a.nf;
        double *o = a.out2 + m * a.o2m + f * a.o2f + kx * a.o2kx;
#pragma unroll
        for (int r = 0; r < PER; ++r) {
            const int ky = lane + r * TPR;
            if (ky < L) o[ky] = p[r];
        }
    }
    if (!a.partial) return;   // (uniform: no barrier is left behind by a part of the workgroup)
    __syncthreads();          // every Z is read
    double *pw = reinterpret_cast<double *>(z);      // L doubles: p in natural order
    int *sa = reinterpret_cast<int *>(pw + L);       // half + 1 ints: the shell of |my| = 0 .. L/2 (behind p, within the column's 2 L doubles)
    if (active) {
#pragma unroll
        for (int r = 0; r < PER; ++r) {
            const int ky = lane + r * TPR;
            if (ky < L) pw[ky] = p[r];
        }
        for (int t = lane; t <= half; t += TPR) sa[t] = shell_of(kx, t, a.wx, a.wy);
    }
    __syncthreads();
    if (!active) return;
    const int smin = sa[0], smax = sa[half];
    double *part = a.partial + u * (long)a.NS;
    // first index in [0, half + 1) whose shell is >= s
    auto lower = [&](int s) {
        int lo = 0, hi = half + 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (sa[mid] < s) lo = mid + 1;
            else hi = mid;
        }
        return lo;
    };
    for (int s = lane; s < a.NS; s += TPR) {
        double sum = 0.0;
        if (s >= smin && s <= smax) {
            const int lo = lower(s), hi = lower(s + 1);
            for (int t = lo; t < hi; ++t) sum += pw[t];                                        // my = t: ky = t
            for (int t = lo < 1 ? 1 : lo; t < (hi < half ? hi : half); ++t) sum += pw[L - t];  // my = −t: ky = L − t
        }
        part[s] = sum;
    }
}

// blockIdx.x = mf * sblocks + sb; thread = ss + SPECTRA_P2_K * g: lane g adds the partials of kx = g, g + G, ..., then the tree
__global__ __launch_bounds__(SPECTRA_P2_K * SPECTRA_P2_G) void k_s2d_shells(const double *__restrict__ partial, double *__restrict__ out, int NS,
                                                                             int nkx, int nf, int sblocks, long oss, long osm) {
    __shared__ double part[SPECTRA_P2_G][SPECTRA_P2_K];
    const int ss = threadIdx.x % SPECTRA_P2_K, g = threadIdx.x / SPECTRA_P2_K;
    const long mf = blockIdx.x / sblocks;
    const int sb = (int)(blockIdx.x - mf * sblocks);
    const int s = sb * SPECTRA_P2_K + ss;
    double sum = 0.0;
    if (s < NS) {
        const double *p = partial + mf * nkx * (long)NS + s;
        for (int k = g; k < nkx; k += SPECTRA_P2_G) sum += p[(long)k * NS];
    }
    part[g][ss] = sum;
    __syncthreads();
#pragma unroll
    for (int d = SPECTRA_P2_G / 2; d >= 1; d >>= 1) {
        if (g < d) part[g][ss] += part[g + d][ss];
        __syncthreads();
    }
    if (g == 0 && s < NS) {
        const long m = mf / nf, f = mf - m * nf;
        out[m * osm + f * oss + s] = part[0][ss];
    }
}

// bytes of LDS a workgroup may take on the current device: asked once per process (a query, not a stream operation: legal in a capture)
long device_lds_limit() {
    static std::atomic<long> cached{0};
    long v = cached.load(std::memory_order_relaxed);
    if (v > 0) return v;
    int dev = 0, bytes = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&bytes, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess || bytes <= 0)
        return 64L * 1024;   // (not cached: the next call asks again)
    cached.store(bytes, std::memory_order_relaxed);
    return bytes;
}

struct S2dOut {
    int which;
    double wx, wy;
    double *ws, *shell;
    int64_t oss;
    double *out2;
    int64_t o2kx, o2f;
    int64_t osm = 0, o2m = 0;
};

template <typename T>
int spectra2d_common(const T *q1, const T *q2, const T *h, const T *A, const Grid &g, int form, const S2dOut &o, int flags, void *stream,
                     const Ens *ens = nullptr) {
    if (!frame_source_ok(q1, q2, h, A, g, form) || !o.ws || (!o.shell && !o.out2)) return SWMHD_EINVAL;
    if (o.which <= 0 || (o.which & ~SWMHD_ZS_ALL) || (flags & ~FRAME_FLAGS) || !frame_members_ok(ens, g)) return SWMHD_EINVAL;
    if (!(o.wx > 0.0) || !(o.wy > 0.0) || !std::isfinite(o.wx) || !std::isfinite(o.wy)) return SWMHD_EINVAL;
    const int nf = __builtin_popcount((unsigned)o.which);
    const int NS = spectra2d_shells(g.Nx, g.Ny, o.wx, o.wy);
    if (NS <= 0) return SWMHD_EINVAL;
    const int64_t nkx = (int64_t)g.Nx / 2 + 1;
    if (o.shell && o.oss < NS) return SWMHD_EINVAL;
    if (o.out2 && (o.o2kx < g.Ny || o.o2f / nkx < o.o2kx)) return SWMHD_EINVAL;   // (a >= n b  <=>  a / n >= b: no overflow)
    if (ens && ((o.shell && o.osm / nf < o.oss) || (o.out2 && o.o2m / nf < o.o2f))) return SWMHD_EINVAL;
    if (!spectra_halo_ok(g, flags)) return SWMHD_EHALO;
    const int members = ens ? ens->members : 1;
    if (spectra_log2(g.Nx) < 0 || spectra_log2(g.Ny) < 0) return SWMHD_ENOTSUP;
    const Spectra2dPlan p = spectra2d_plan(g.Nx, g.Ny, nf, members, o.wx, o.wy, o.shell != nullptr, device_lds_limit());
    if (p.unsupported) return SWMHD_ENOTSUP;
    if (p.none) return SWMHD_OK;
    if (p.too_many) return hiprc(hipErrorInvalidConfiguration);
    S2dArgs<T> a;
    set_frame_source(a, q1, q2, h, A, g, form, o.which, flags, ens);
    a.ws = o.ws;
    a.nf = nf; a.log2n = p.log2nx; a.R = p.R; a.pad = p.pad;
    a.log2r = 0;
    while ((1 << a.log2r) < p.R) ++a.log2r;
    hipStream_t s = (hipStream_t)stream;
    constexpr int WAVE = 64;
    static_assert(SPECTRA_UNITS_SMALL == SPECTRA_NT / WAVE, "a small row or column is one wave's");
    const dim3 grid1((unsigned)p.blocks1), grid2((unsigned)p.blocks2), grid3((unsigned)p.blocks3), nt(SPECTRA_NT);
    if (p.units1 == 1) {
        if (ens) hipLaunchKernelGGL((k_s2d_rows<T, true, SPECTRA_NT>), grid1, nt, (size_t)p.lds1, s, a);
        else hipLaunchKernelGGL((k_s2d_rows<T, false, SPECTRA_NT>), grid1, nt, (size_t)p.lds1, s, a);
    } else {
        if (ens) hipLaunchKernelGGL((k_s2d_rows<T, true, WAVE>), grid1, nt, (size_t)p.lds1, s, a);
        else hipLaunchKernelGGL((k_s2d_rows<T, false, WAVE>), grid1, nt, (size_t)p.lds1, s, a);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hiprc(e);
    S2dColArgs c;
    c.modes = o.ws;
    c.partial = o.shell ? o.ws + p.modes : nullptr;
    c.out2 = o.out2;
    c.Ny = g.Ny; c.log2ny = p.log2ny; c.nkx = p.nkx; c.NS = p.NS; c.nf = nf;
    c.units = (long)p.nkx * nf * members;
    c.o2kx = (long)o.o2kx; c.o2f = (long)o.o2f; c.o2m = ens ? (long)o.o2m : 0;
    c.wx = o.wx; c.wy = o.wy;
    if (p.units2 == 1) {
        if (p.table) hipLaunchKernelGGL((k_s2d_cols<SPECTRA_NT, true>), grid2, nt, (size_t)p.lds2, s, c);
        else hipLaunchKernelGGL((k_s2d_cols<SPECTRA_NT, false>), grid2, nt, (size_t)p.lds2, s, c);
    } else {
        hipLaunchKernelGGL((k_s2d_cols<WAVE, true>), grid2, nt, (size_t)p.lds2, s, c);
    }
    e = hipGetLastError();
    if (e != hipSuccess || !o.shell) return hiprc(e);
    hipLaunchKernelGGL(k_s2d_shells, grid3, dim3(SPECTRA_P2_K * SPECTRA_P2_G), 0, s, c.partial, o.shell, p.NS, p.nkx, nf,
                       (p.NS + SPECTRA_P2_K - 1) / SPECTRA_P2_K, (long)o.oss, ens ? (long)o.osm : 0);
    return hiprc(hipGetLastError());
}

}  // namespace
}  // namespace swmhd

extern "C" {

int swmhd_spectra2d_shells(int Nx, int Ny, double wx, double wy) { return swmhd::spectra2d_shells(Nx, Ny, wx, wy); }

int64_t swmhd_spectra2d_workspace(int Nx, int Ny, int nfields, int members, double wx, double wy) {
    if (Nx <= 0 || Ny <= 0 || nfields <= 0 || members <= 0) return 0;
    const int64_t NS = swmhd::spectra2d_shells(Nx, Ny, wx, wy), nkx = (int64_t)Nx / 2 + 1;
    if (NS <= 0) return 0;
    return (2 * nkx * Ny + nkx * NS) * nfields * members;
}

#define SWMHD_DEF_SPECTRA2D(sfx, T)                                                                                                    \
    int swmhd_spectra2d_##sfx(const T *q1, const T *q2, const T *h, const T *A, int Nx, int Ny, int Hx, int Hy, int64_t sy, T dx,     \
                              T dy, int formulation, int which, double wx, double wy, double *workspace, double *out_shell,           \
                              int64_t out_stride_s, double *out_2d, int64_t out2_stride_kx, int64_t out2_stride_f, int flags,         \
                              void *stream) {                                                                                          \
        return swmhd::spectra2d_common<T>(q1, q2, h, A, swmhd::Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, formulation,                          \
                                          swmhd::S2dOut{which, wx, wy, workspace, out_shell, out_stride_s, out_2d, out2_stride_kx,    \
                                                        out2_stride_f},                                                                \
                                          flags, stream);                                                                              \
    }                                                                                                                                  \
    int swmhd_ensemble_spectra2d_##sfx(const T *q1, const T *q2, const T *h, const T *A, int members, int64_t stride_m, int Nx,       \
                                       int Ny, int Hx, int Hy, int64_t sy, T dx, T dy, int formulation, int which, double wx,         \
                                       double wy, double *workspace, double *out_shell, int64_t out_stride_s, int64_t out_stride_m,   \
                                       double *out_2d, int64_t out2_stride_kx, int64_t out2_stride_f, int64_t out2_stride_m,          \
                                       int flags, void *stream) {                                                                      \
        const swmhd::Ens e{members, stride_m};                                                                                         \
        return swmhd::spectra2d_common<T>(q1, q2, h, A, swmhd::Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, formulation,                          \
                                          swmhd::S2dOut{which, wx, wy, workspace, out_shell, out_stride_s, out_2d, out2_stride_kx,    \
                                                        out2_stride_f, out_stride_m, out2_stride_m},                                  \
                                          flags, stream, &e);                                                                          \
    }

SWMHD_DEF_SPECTRA2D(f64, double)
SWMHD_DEF_SPECTRA2D(f32, float)

}  // extern "C"
