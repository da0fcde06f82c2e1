// What the zonal spectra (spectra.hip) and the 2-D / isotropic spectra (spectra2d.hip) share, stated once: the frame value of one cell,
// the complex type, the twiddle quarter table, one stage of the in-place radix-2 decimation-in-frequency FFT in LDS and the untangling
// of a real row's half-length transform.  Device code only; both objects are built STRICT (no contraction, IEEE divide / sqrt), and the
// error constant η = 9.66 of include/swmhd_spectra.h is derived for exactly these statements.

struct alignas(16) cplx { double re, im; };
__device__ __forceinline__ cplx cmul(cplx a, cplx w) { return cplx{a.re * w.re - a.im * w.im, a.re * w.im + a.im * w.re}; }
// w_N^idx, 0 <= idx < N/2, from the quarter table of Q = N/4 entries: w^(idx) = −i w^(idx − N/4) beyond it
__device__ __forceinline__ cplx twiddle(const cplx *tw, int idx, int Q) {
    if (idx < Q) return tw[idx];
    const cplx t = tw[idx - Q];
    return cplx{t.im, -t.re};
}
// entry k of the quarter table of w_N: cospi(2k/N) − i sinpi(2k/N)  (2k/N: exact, N is a power of two)
__device__ __forceinline__ cplx twiddle_entry(int k, int N) {
    double s, c;
    sincospi((double)(2 * k) / (double)N, &s, &c);
    return cplx{c, -s};
}
// the same value without a table (TABLE = false: sincospi per butterfly), bit for bit
template <bool TABLE>
__device__ __forceinline__ cplx twiddle_at(const cplx *tw, int idx, int Q) {
    if constexpr (TABLE) {
        return twiddle(tw, idx, Q);
    } else {
        if (idx < Q) return twiddle_entry(idx, 4 * Q);
        const cplx t = twiddle_entry(idx - Q, 4 * Q);
        return cplx{t.im, -t.re};
    }
}

// the frame value of field `bit` at cell x of row y (0-based interior indices): the definitions of frame_device.inc, with which these
// statements must agree bit for bit (the spectra tests hold them to the frame), written out for one cell of one field: routed through
// frame_device.inc's helpers the two row kernels compile to other code objects, and a listing that changes is a change to measure.
// (Args: q1 q2 h A at interior cell (1,1), dx, dy)
template <typename Args>
__device__ __forceinline__ double frame_value(const Args &a, int bit, bool cons, long r0, long rm, long rp, int x, int xl) {
    auto ld = [](auto *p, long o) { return (double)p[o]; };
    auto U = [&](int i, int il) { return cons ? ld(a.q1, r0 + i) / (0.5 * (ld(a.h, r0 + il) + ld(a.h, r0 + i))) : ld(a.q1, r0 + i); };
    auto V0 = [&](int i) { return cons ? ld(a.q2, r0 + i) / (0.5 * (ld(a.h, rm + i) + ld(a.h, r0 + i))) : ld(a.q2, r0 + i); };
    auto Vp = [&](int i) { return cons ? ld(a.q2, rp + i) / (0.5 * (ld(a.h, r0 + i) + ld(a.h, rp + i))) : ld(a.q2, rp + i); };
    switch (bit) {
    case SWMHD_ZS_U: return U(x, xl);
    case SWMHD_ZS_V: return V0(x);
    case SWMHD_ZS_H: return ld(a.h, r0 + x);
    case SWMHD_ZS_A: return ld(a.A, r0 + x);
    case SWMHD_ZS_SPEED: {
        const double u = U(x, xl), g00 = V0(xl), g10 = V0(x), g01 = Vp(xl), g11 = Vp(x);
        return sqrt(u * u + 0.5 * (0.5 * (g00 * g00 + g10 * g10) + 0.5 * (g01 * g01 + g11 * g11)));
    }
    case SWMHD_ZS_BX: return -((ld(a.A, r0 + x) - ld(a.A, rm + x)) / a.dy) / (0.5 * (ld(a.h, rm + x) + ld(a.h, r0 + x)));
    default: return ((ld(a.A, r0 + x) - ld(a.A, r0 + xl)) / a.dx) / (0.5 * (ld(a.h, r0 + xl) + ld(a.h, r0 + x)));   // SWMHD_ZS_BY
    }
}

// field number f of the mask `which` (counting set bits from bit 0): its bit
__device__ __forceinline__ int field_bit(int which, int f) {
    int bit = 0;
    for (int p = 0, n = 0; p < 7; ++p) {
        if (which & (1 << p)) {
            if (n == f) bit = 1 << p;
            ++n;
        }
    }
    return bit;
}

// the row y of field `bit` as N doubles in LDS, by the TPR lanes of a unit
template <int TPR, typename Args>
__device__ __forceinline__ void load_row(const Args &a, double *x_row, int bit, bool cons, int y, int lane) {
    const int N = a.Nx;
    const int ym = (y == 0 && (a.wrap & 2)) ? a.Ny - 1 : y - 1;
    const int yp = (y == a.Ny - 1 && (a.wrap & 2)) ? 0 : y + 1;
    const long r0 = (long)y * a.sy, rm = (long)ym * a.sy, rp = (long)yp * a.sy;
#pragma unroll 4
    for (int x = lane; x < N; x += TPR) {
        const int xl = (x == 0 && (a.wrap & 1)) ? N - 1 : x - 1;
        x_row[x] = frame_value(a, bit, cons, r0, rm, rp, x, xl);
    }
}

// One stage of the decimation in frequency, by the TPR lanes of a unit: half-span hs = 2^lh; butterfly t of `nbut`: block t / hs, offset
// j = t mod hs, operands z[i0], z[i0 + hs], twiddle w^(j << sh) of the table's root; y0 = a + b, y1 = (a − b) w.  NB butterflies of the
// thread at a time: all their operands are read before the first is written.  The caller's barrier follows.
template <int TPR, int NB, bool TABLE = true>
__device__ __forceinline__ void dif_stage(cplx *z, const cplx *tw, int lane, int nbut, int lh, int sh, int Q) {
    const int hs = 1 << lh;
    for (int base = lane; base < nbut; base += TPR * NB) {
        cplx p[NB], q[NB], wv[NB];
        int i0[NB];
#pragma unroll
        for (int n = 0; n < NB; ++n) {
            const int t = base + n * TPR;
            if (t < nbut) {
                const int j = t & (hs - 1);
                i0[n] = ((t >> lh) << (lh + 1)) + j;
                p[n] = z[i0[n]];
                q[n] = z[i0[n] + hs];
                wv[n] = twiddle_at<TABLE>(tw, j << sh, Q);
            }
        }
#pragma unroll
        for (int n = 0; n < NB; ++n) {
            if (base + n * TPR < nbut) {
                const cplx d{p[n].re - q[n].re, p[n].im - q[n].im};
                z[i0[n]] = cplx{p[n].re + q[n].re, p[n].im + q[n].im};
                z[i0[n] + hs] = cmul(d, wv[n]);
            }
        }
    }
}

// untangle: mode k (0 <= k <= M) of the real row of 2M values whose half-length transform Z stands in z with Z[k] at bitreverse_LM(k),
// scaled by inv = 1/(2M) (exact).  k = 0: X[0] = Re Z[0] + Im Z[0]; k = M: Re Z[0] − Im Z[0]; tw: the quarter table of w_2M, Q = M/2
__device__ __forceinline__ cplx untangle(const cplx *z, const cplx *tw, int k, int M, int LM, int Q, double inv) {
    double xr, xi;
    if (k == 0 || k == M) {
        const cplx z0 = z[0];
        xr = k == 0 ? z0.re + z0.im : z0.re - z0.im;
        xi = 0.0;
    } else {
        const cplx p = z[__brev((unsigned)k) >> (32 - LM)], q = z[__brev((unsigned)(M - k)) >> (32 - LM)];
        const cplx E{0.5 * (p.re + q.re), 0.5 * (p.im - q.im)};
        const cplx O{0.5 * (p.im + q.im), -(0.5 * (p.re - q.re))};
        const cplx wo = cmul(O, twiddle(tw, k, Q));
        xr = E.re + wo.re;
        xi = E.im + wo.im;
    }
    xr *= inv;
    xi *= inv;
    return cplx{xr, xi};
}
