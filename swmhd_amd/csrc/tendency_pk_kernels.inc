// Packed-fp32 instantiation of the row-marching vector-invariant tendency kernel (BASELINE config 5's fp32 leg).
//
// CDNA4 issues an UNPACKED fp32 VALU instruction at the same cost as an fp64 one (4 cycles per wave), which is why the plain
// float instantiation of k_tendency_vi_march is only ~1.4x faster than fp64.  Here every lane owns TWO adjacent columns held as
// one 64-bit register pair (sw_f2, sw_device.inc) and all arithmetic is packed (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32): the
// same ~580 issue slots per row now advance two columns.  Same organisation as the fp64 kernel (register windows along y, LDS row
// rings along x, two barriers per row, prologue, fused Lorentz force and RK3 substep, straight-line memory operations); differences:
//   * a strip is NT lanes = 2 NT columns with 2 halo LANES per side (4 columns; the stencils need 3): 504 output columns per
//     256-lane workgroup; global accesses are 8-byte pairs (512-B wave rows, as in fp64);
//   * LDS rows hold plain floats; the pair at column offset k is one ds_read_b64 (k even) or ds_read2_b32 (k odd);
//   * the upwind side of an x-direction stencil differs between the two columns of a lane, so it is chosen by per-element selects
//     (the fp64 kernel picks it by lane-local LDS addressing);
//   * reciprocals are v_rcp_f32 per column (there is no packed reciprocal).
// Requires SWMHD_WRAP_X (periodic images taken on read: a lane's pair never straddles a halo boundary) and an even Nx; the
// launcher falls back to the unpacked kernel otherwise.  Results differ from the unpacked fp32 kernel only by rounding.
//
// Included from tendency_tile_kernels.inc (fast build) inside namespace swmhd { namespace { ... } }.

// (sw_f2_u, common.hpp: a pair in global memory is only dword-aligned -- Hx = 3 is odd)

template <int LOR, int NT, int MODE>
__global__ __launch_bounds__(NT, 3) void k_tendency_vi_march_pk(TendArgs<float> a, int nstrips, int nseg, int LY) {
    using T = sw_f2;
    using S = float;
    constexpr bool FUSE = (MODE & 1) != 0, HAS_GM = (MODE & 2) != 0, STORE_G = (MODE & 4) != 0, ANCHOR = (MODE & 8) != 0;
    constexpr bool STORE_W = ANCHOR && FUSE && !HAS_GM;   // MODE as in k_tendency_vi_march
    constexpr int XL = 2, PAD = 4, RW = 2 * NT + 2 * PAD, TXO = 2 * (NT - 2 * XL);
    __shared__ __attribute__((aligned(8))) S Ru[3][RW];    // u rows jo-1, jo (+1)
    __shared__ __attribute__((aligned(8))) S Rvn[1][RW];   // v newest row
    __shared__ __attribute__((aligned(8))) S RA[4][RW];    // A rows jo-1 .. jo+1 (+1 being written)
    __shared__ __attribute__((aligned(8))) S RH[2][RW];    // h row jo (+1)
    __shared__ __attribute__((aligned(8))) S RBx[3][RW];   // centre Bx rows jo-1 .. jo+1
    __shared__ __attribute__((aligned(8))) S RBy[3][RW];
    __shared__ __attribute__((aligned(8))) S RFh[1][RW];   // x-face flux of h, row jo
    __shared__ __attribute__((aligned(8))) S RFA[1][RW];
    __shared__ __attribute__((aligned(8))) S RK[1][RW];    // Kh(c, jo)
    __shared__ __attribute__((aligned(8))) S RZ[1][RW];    // zeta(c, jo) and the velocities at the vorticity point
    __shared__ __attribute__((aligned(8))) S RUf[1][RW];
    __shared__ __attribute__((aligned(8))) S RVf[1][RW];

    const unsigned bid = xcd_remap(blockIdx.x, (unsigned)(nstrips * nseg));
    const int strip = (int)(bid % nstrips), seg = (int)(bid / nstrips);
    const int x0 = strip * TXO;
    int J0, J1;
    segment_rows(a, seg, LY, J0, J1);
    const int lane = threadIdx.x, lc = 2 * lane + PAD;   // local column of this lane's first element
    const int gx0 = x0 - 2 * XL + 2 * lane;              // its global column
    const bool wy = (a.wrap & 2) != 0;
    const int xlo = -a.Hx, xhi = a.Nx + a.Hx - 1, ylo = -a.Hy, yhi = a.Ny + a.Hy - 1;
    auto wrapx = [&](int x) -> int { return wrap_index(x, a.Nx, xlo, xhi, true); };
    const T rdx = T(a.rdx), rdy = T(a.rdy);
    const Geo<T> g{T(a.dx), T(a.dy), T(a.rdx), T(a.rdy)};
    const bool col_ok = (lane >= XL) && (lane < NT - XL) && (gx0 < a.Nx);

    // the pair of this lane's two columns at column offset k of an LDS row / its own pair stored
    auto P = [&](const S *row, int k) -> T { T v; v.x = row[lc + k]; v.y = row[lc + k + 1]; return v; };
    auto W = [&](S *row, T v) { *reinterpret_cast<T *>(row + lc) = v; };

    T uw[8], vw[7], vlw[7], hw[7], aw[7];   // windows, one element longer than the stencils: the prefetched row lands in the last
    T fhy = T(0), fay = T(0), km = T(0);

    const long off0 = (long)a.Hy * a.sy + a.Hx;
    const int isy = (int)a.sy;
    auto LD = [&](const S *interior, unsigned ob) -> T { return *reinterpret_cast<const sw_f2_u *>(reinterpret_cast<const char *>(interior - off0) + ob); };
    auto LD1 = [&](const S *interior, unsigned ob) -> S { return *reinterpret_cast<const S *>(reinterpret_cast<const char *>(interior - off0) + ob); };
    // one period holds the whole strip's pairs contiguously: column gx0 wraps as a pair (Nx and gx0 are even); lanes beyond one
    // period are clamped (they feed nothing that is stored)
    const int gxw = wrap_index(gx0, a.Nx, xlo, xhi - 1, true);
    const unsigned colb = (unsigned)(gxw + a.Hx) * (unsigned)sizeof(S);
    auto rowoff = [&](int row) -> unsigned { return (unsigned)((row + a.Hy) * isy) * (unsigned)sizeof(S); };
    const unsigned pbytes = (unsigned)((a.Ny + 2 * a.Hy) * isy) * (unsigned)sizeof(S);
    __amdgpu_buffer_rsrc_t rG[4], rU[4];
    if constexpr (STORE_G || STORE_W) {
        rG[0] = out_rsrc(a.G1 - off0, pbytes); rG[1] = out_rsrc(a.G2 - off0, pbytes);
        rG[2] = out_rsrc(a.Gh - off0, pbytes); rG[3] = out_rsrc(a.GA - off0, pbytes);
    }
    if constexpr (FUSE) {
#pragma unroll
        for (int f = 0; f < 4; ++f) rU[f] = out_rsrc(a.Unew[f] - off0, pbytes);
    }

    {   // ---- prologue (see k_tendency_vi_march): seven rows in one burst, carried quantities computed directly ----
        const unsigned colm = (unsigned)(wrapx(gx0 - 1) + a.Hx) * (unsigned)sizeof(S);   // column left of the pair
        const unsigned colp = (unsigned)(wrapx(gx0 + 2) + a.Hx) * (unsigned)sizeof(S);   // column right of the pair
        unsigned ro[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) ro[k] = rowoff(wrap_index(J0 - 3 + k, a.Ny, ylo, yhi, wy));
        T pu[7], pv[7], ph[7], pa[7];
        S pvl[6];
#pragma unroll
        for (int k = 0; k < 7; ++k) { pu[k] = LD(a.q1, ro[k] + colb); pv[k] = LD(a.q2, ro[k] + colb); ph[k] = LD(a.h, ro[k] + colb); pa[k] = LD(a.A, ro[k] + colb); }
#pragma unroll
        for (int k = 0; k < 6; ++k) pvl[k] = LD1(a.q2, ro[k + 1] + colm);
        const S ue_r = LD1(a.q1, ro[2] + colp);                                 // u right of the pair, row J0-1
        S a_wm = 0, a_em = 0, a_wo = 0, a_eo = 0;
        if constexpr (LOR == 1) {
            a_wm = LD1(a.A, ro[2] + colm); a_em = LD1(a.A, ro[2] + colp);
            a_wo = LD1(a.A, ro[3] + colm); a_eo = LD1(a.A, ro[3] + colp);
        }
#pragma unroll
        for (int k = 0; k < 7; ++k) uw[k] = pu[k];
#pragma unroll
        for (int k = 0; k < 6; ++k) { vw[k] = pv[k + 1]; vlw[k] = T{pvl[k], pv[k + 1].x}; hw[k] = ph[k + 1]; aw[k] = pa[k + 1]; }
        uw[7] = T(0); vw[6] = T(0); vlw[6] = T(0); hw[6] = T(1); aw[6] = T(0);
        fhy = upwind_weno<T>(vw[2], ph);
        fay = upwind_weno<T>(vw[2], pa);
        const T ue_m = T{uw[2].y, ue_r};                                        // u(c+1, J0-1) for both columns
        km = T(0.25) * ((sq(uw[2]) + sq(ue_m)) + (sq(vw[1]) + sq(vw[2])));
        const int q3o = ((J0 % 3) + 3) % 3, q3m = (q3o + 2) % 3;
        W(Ru[q3m], uw[2]);
        W(RA[(J0 - 1) & 3], aw[1]);
        W(RA[J0 & 3], aw[2]);
        if constexpr (LOR == 1) {
            const T rhm = recip<T>(hw[1]), rho = recip<T>(hw[2]);
            const T cxm = T{aw[1].y - a_wm, a_em - aw[1].x}, cxo = T{aw[2].y - a_wo, a_eo - aw[2].x};   // A(c+1) - A(c-1), rows J0-1, J0
            W(RBy[q3m], (T(0.5) * rdx) * cxm * rhm);
            W(RBx[q3m], -(T(0.5) * rdy) * (aw[2] - aw[0]) * rhm);
            W(RBy[q3o], (T(0.5) * rdx) * cxo * rho);
            W(RBx[q3o], -(T(0.5) * rdy) * (aw[3] - aw[1]) * rho);
        }
    }

    const int niter = (J1 - J0) + 6;
    const ProgressPriority prio(niter);
    for (int it = 6; it < niter; ++it) {
        prio.at(it);
        T *const U = uw, *const V = vw, *const VL = vlw, *const Hh = hw, *const Aa = aw;
        const int jr = J0 - 3 + it, jo = jr - 3;
        {
            const unsigned ob = rowoff(wrap_index(jr + 1, a.Ny, ylo, yhi, wy)) + colb;
            uw[7] = LD(a.q1, ob); vw[6] = LD(a.q2, ob); hw[6] = LD(a.h, ob); aw[6] = LD(a.A, ob);
        }
        T gm0 = T(0), gm1 = T(0), gm2 = T(0), gm3 = T(0);
        const unsigned rowb = rowoff(jo);
        const int s3o = ((jo % 3) + 3) % 3, s3m = (s3o + 2) % 3, s3p = (s3o + 1) % 3;
        const int s4o = jo & 3, s4p = (jo + 1) & 3;

        // ---- P1 ----
        W(Ru[s3o], U[3]);
        W(RH[jo & 1], Hh[2]);
        W(RA[s4p], Aa[3]);
        W(Rvn[0], V[5]);
        __syncthreads();

        // ---- P2 ----
        VL[5] = P(Rvn[0], -1);
        if constexpr (LOR == 1) {
            const T cxA = P(RA[s4p], 1) - P(RA[s4p], -1);
            const T cyA = Aa[4] - Aa[2];
            const T rh = recip<T>(Hh[3]);
            W(RBy[s3p], (T(0.5) * rdx) * cxA * rh);
            W(RBx[s3p], -(T(0.5) * rdy) * cyA * rh);
        }
        {
            const T ue2 = P(Ru[s3o], 1);
            W(RK[0], T(0.25) * ((sq(U[3]) + sq(ue2)) + (sq(V[2]) + sq(V[3]))));
        }
        W(RZ[0], (V[2] - VL[2]) * rdx - (U[3] - U[2]) * rdy);
        W(RUf[0], T(0.5) * (U[2] + U[3]));
        W(RVf[0], T(0.5) * (VL[2] + V[2]));
        {
            const T uadv = U[3];
            T qh[6], qa[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) { qh[k] = P(RH[jo & 1], k - 3); qa[k] = P(RA[s4o], k - 3); }
            W(RFh[0], upwind_weno<T>(uadv, qh));
            W(RFA[0], upwind_weno<T>(uadv, qa));
        }
        __syncthreads();
        if constexpr (FUSE && HAS_GM) {
            const unsigned og = rowb + colb;
            gm0 = LD(a.Gm[0], og); gm1 = LD(a.Gm[1], og); gm2 = LD(a.Gm[2], og); gm3 = LD(a.Gm[3], og);
        }

        // ---- P3 ----
        const T fhy_n = upwind_weno<T>(V[3], Hh);
        const T fay_n = upwind_weno<T>(V[3], Aa);
        T zy[6], svy[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            zy[k] = (V[k] - VL[k]) * rdx - (U[k + 1] - U[k]) * rdy;
            svy[k] = VL[k] + V[k];
        }
        const T vhat = T(0.25) * (svy[2] + svy[3]);
        const T vortU = -upwind_weno_vel_raw<T>(vhat, zy, U, svy);
        const T ue = P(Ru[s3o], 1);
        const T uhat = T(0.25) * ((U[2] + P(Ru[s3m], 1)) + (U[3] + ue));
        T vortV;
        {   // zeta reconstructed along x to (c,f): stencil points f-3 .. f+2 of the face sequence = columns c-2 .. c+3
            T zx[6], ufx[6], vfx[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) { zx[k] = P(RZ[0], k - 2); ufx[k] = P(RUf[0], k - 2); vfx[k] = P(RVf[0], k - 2); }
            vortV = upwind_weno_vel<T>(uhat, zx, ufx, vfx);
        }
        const T kc = P(RK[0], 0), kl = P(RK[0], -1);
        const T hl = P(RH[jo & 1], -1);
        T Fx = T(0), Fy = T(0);
        if constexpr (LOR == 1) {
            auto A_ = [&](int di, int dj) -> T { return di == 0 ? Aa[2 + dj] : P(RA[(jo + dj) & 3], di); };
            auto H_ = [&](int di, int dj) -> T { return di == 0 ? Hh[2 + dj] : hl; };
            auto BX_ = [&](int di, int dj) -> T { return P(RBx[dj < 0 ? s3m : (dj > 0 ? s3p : s3o)], di); };
            auto BY_ = [&](int di, int dj) -> T { return P(RBy[dj < 0 ? s3m : (dj > 0 ? s3p : s3o)], di); };
            jac_force<T>(A_, H_, BX_, BY_, 0, 0, g, Fx, Fy);
        }
        const T G1 = -vortU - (kc - kl) * rdx - T(a.grav) * (Hh[2] - hl) * rdx + T(a.fcor) * vhat + Fx;
        const T G2 = -vortV - (kc - km) * rdy - T(a.grav) * (Hh[2] - Hh[1]) * rdy - T(a.fcor) * uhat + Fy;
        const T Gh = -((P(RFh[0], 1) - P(RFh[0], 0)) * rdx + (fhy_n - fhy) * rdy);
        const T GA = -((P(RFA[0], 1) - P(RFA[0], 0)) * rdx + (fay_n - fay) * rdy)
                     + Aa[2] * ((ue - U[3]) * rdx + (V[3] - V[2]) * rdy);
        const unsigned o = col_ok ? rowb + colb : SW_OOB;
        const T Gs[4] = {G1, G2, Gh, GA};
        if constexpr (STORE_G) {
            const unsigned oG = a.drop_G ? SW_OOB : o;      // (last RK3 stage running this variant: nothing reads its G)
#pragma unroll
            for (int f = 0; f < 4; ++f) buffer_store<T>(Gs[f], rG[f], oG);
        }
        if constexpr (FUSE) {
            const T Us[4] = {U[3], V[2], Hh[2], Aa[2]};
            const T Gms[4] = {gm0, gm1, gm2, gm3};
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                T un;
                if constexpr (!HAS_GM) un = Us[f] + T(a.dtg) * Gs[f];
                else if constexpr (ANCHOR) un = fma_<T>(T(a.dtg), Gs[f], Gms[f]);
                else if constexpr (STORE_G) un = fma_<T>(T(a.cg), Gms[f], fma_<T>(T(a.dtg), Gs[f], fma_<T>(T(a.cu), Us[f], Us[f])));
                else un = Us[f] + T(a.dt) * (T(a.gamma) * Gs[f] + T(a.zeta) * Gms[f]);
                buffer_store<T>(un, rU[f], o);
            }
        }
        if constexpr (STORE_W) {
            const T Us[4] = {U[3], V[2], Hh[2], Aa[2]};
#pragma unroll
            for (int f = 0; f < 4; ++f) buffer_store<T>(Us[f] + T(a.dtw) * Gs[f], rG[f], o);
        }
        fhy = fhy_n; fay = fay_n; km = kc;
        constexpr int YOUNGER = ((FUSE && HAS_GM) ? 4 : 0) + (STORE_G ? 4 : 0) + (FUSE ? 4 : 0) + (STORE_W ? 4 : 0);
        wait_vmem_all_but<YOUNGER>();
        // shift the windows by one row
#pragma unroll
        for (int k = 0; k < 7; ++k) uw[k] = uw[k + 1];
#pragma unroll
        for (int k = 0; k < 6; ++k) { vw[k] = vw[k + 1]; vlw[k] = vlw[k + 1]; hw[k] = hw[k + 1]; aw[k] = aw[k + 1]; }
    }
}
