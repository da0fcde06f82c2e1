// Lorentz-force operator kernels, row-marching form (fast builds only).  Same arithmetic as the fast tile kernels
// (lorentz_device.inc) but organised for HBM streaming:
//   * a workgroup owns a strip of NT-2*XH columns and marches up LY rows; one lane = one column;
//   * y-direction stencil values live in register windows (each A/h row is loaded from HBM exactly once per strip,
//     x-coalesced 512-B wave rows, PF rows ahead of use so >= 2 rows of loads are always in flight per wave);
//   * x-neighbours come from short LDS row rings; every shared intermediate (centre Bx,By / face hBx,Bx,hBy,By) is
//     computed once per cell with one Newton reciprocal and published for the neighbours;
//   * no y-halo re-reads except the 4 (Jacobian) / 6 (divergence) warm-up rows per LY-row segment.
//
//   k_lorentz_jacobian_march    lorentz_force_func_x/y   jacobian_formulation/sw_mhd_jacobian_functions.jl:1-26
//   k_lorentz_divergence_march  div_lorentz_x/y          divergence_formulation/sw_mhd_divergence_functions.jl:1-170
//
// Included from lorentz_fast.hip inside namespace swmhd { namespace { ... } }.

// Workgroup-wide rendezvous between the publish and consume phases.  With one wave per workgroup (NT == 64) LDS operations
// of that wave already execute in program order, so only the compiler has to be fenced: no s_barrier at all.
template <int NT> __device__ __forceinline__ void phase_sync() {
    if constexpr (NT == 64) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    } else {
        __syncthreads();
    }
}

template <typename T, int NT, int PF>
__global__ __launch_bounds__(NT) void k_lorentz_jacobian_march(OpArgs<T> a, int nstrips, int nseg, int LY) {
    constexpr int XH = 2, RW = NT + 2 * XH, TXO = NT - 2 * XH;
    __shared__ T RA[4][RW];    // A rows jo-1 .. jo+1 (+1 being written)
    __shared__ T Rh[2][RW];    // h row jo
    __shared__ T RBx[3][RW];   // centre Bx rows jo-1 .. jo+1
    __shared__ T RBy[3][RW];

    const unsigned bid = xcd_remap(blockIdx.x, (unsigned)(nstrips * nseg));
    const int strip = (int)(bid % nstrips), seg = (int)(bid / nstrips);
    const int x0 = strip * TXO;
    const int J0 = a.j0 + seg * LY;
    const int J1 = (J0 + LY < a.j1) ? J0 + LY : a.j1;
    const int c = threadIdx.x, lc = c + XH;
    const int gx = x0 - XH + c;
    const int gxc = clampi(gx, -a.Hx, a.Nx + a.Hx - 1);
    const int ylo = -a.Hy, yhi = a.Ny + a.Hy - 1;
    const Geo<T> g{a.dx, a.dy, a.rdx, a.rdy};
    const bool col_ok = (c >= XH) && (c < NT - XH) && (gx < a.Nx);

    T aw[5], hw[4];   // A(c, jo-2 .. jo+2), h(c, jo-1 .. jo+2)
#pragma unroll
    for (int k = 0; k < 5; ++k) aw[k] = T(0);
#pragma unroll
    for (int k = 0; k < 4; ++k) hw[k] = T(1);
    T pa[PF], ph[PF];   // rows in flight
    auto ldrow = [&](int row, T &na, T &nh) {
        const long o = (long)clampi(row, ylo, yhi) * a.sy + gxc;
        na = a.A[o]; nh = a.h[o];
    };
    // Prologue: the four rows the windows need (J0-2 .. J0+1), the PF rows in flight and the x-neighbour values of the two centre-B
    // rows the first output row reads (J0-1, J0) are loaded in one burst; those B rows and the two A rows are published without a
    // barrier (the first iteration's barrier orders them).  Replaces four warm-up iterations per segment (eight barriers, four
    // dependent HBM round trips).
    {
        const int gxm = clampi(gx - 1, -a.Hx, a.Nx + a.Hx - 1), gxp = clampi(gx + 1, -a.Hx, a.Nx + a.Hx - 1);
        long ro[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) ro[k] = (long)clampi(J0 - 2 + k, ylo, yhi) * a.sy;
#pragma unroll
        for (int k = 0; k < 4; ++k) aw[k + 1] = a.A[ro[k] + gxc];      // shifted down by the first iteration
#pragma unroll
        for (int k = 0; k < 3; ++k) hw[k + 1] = a.h[ro[k + 1] + gxc];
        const T awm = a.A[ro[1] + gxm], aem = a.A[ro[1] + gxp], awo = a.A[ro[2] + gxm], aeo = a.A[ro[2] + gxp];
#pragma unroll
        for (int k = 0; k < PF; ++k) ldrow(J0 + 2 + k, pa[k], ph[k]);
        const int q3o = ((J0 % 3) + 3) % 3, q3m = (q3o + 2) % 3;
        RA[(J0 - 1) & 3][lc] = aw[2];
        RA[J0 & 3][lc] = aw[3];
        const T rhm = fast_recip<T>(hw[1]), rho = fast_recip<T>(hw[2]);
        RBy[q3m][lc] = (T(0.5) * g.rdx) * (aem - awm) * rhm;
        RBx[q3m][lc] = -(T(0.5) * g.rdy) * (aw[3] - aw[1]) * rhm;
        RBy[q3o][lc] = (T(0.5) * g.rdx) * (aeo - awo) * rho;
        RBx[q3o][lc] = -(T(0.5) * g.rdy) * (aw[4] - aw[2]) * rho;
    }

    const int niter = (J1 - J0) + 4;
    const ProgressPriority prio(niter);
    for (int it = 4; it < niter; ++it) {
        prio.at(it);
        const int jr = J0 - 2 + it, jo = jr - 2;
#pragma unroll
        for (int k = 0; k < 4; ++k) aw[k] = aw[k + 1];
#pragma unroll
        for (int k = 0; k < 3; ++k) hw[k] = hw[k + 1];
        aw[4] = pa[0]; hw[3] = ph[0];
#pragma unroll
        for (int k = 0; k + 1 < PF; ++k) { pa[k] = pa[k + 1]; ph[k] = ph[k + 1]; }
        if (it + PF < niter) ldrow(jr + PF, pa[PF - 1], ph[PF - 1]);

        const int s3o = ((jo % 3) + 3) % 3, s3m = (s3o + 2) % 3, s3p = (s3o + 1) % 3;
        const int s4p = (jo + 1) & 3;
        RA[s4p][lc] = aw[3];          // A(c, jo+1)
        Rh[jo & 1][lc] = hw[1];       // h(c, jo)
        phase_sync<NT>();
        {   // centre B at row jo+1 (reference :1-7), once per cell
            const T cxA = RA[s4p][lc + 1] - RA[s4p][lc - 1];
            const T cyA = aw[4] - aw[2];
            const T rh = fast_recip<T>(hw[2]);
            RBy[s3p][lc] = (T(0.5) * g.rdx) * cxA * rh;
            RBx[s3p][lc] = -(T(0.5) * g.rdy) * cyA * rh;
        }
        phase_sync<NT>();
        const T hl = Rh[jo & 1][lc - 1];
        auto A_ = [&](int di, int dj) -> T { return di == 0 ? aw[2 + dj] : RA[(jo + dj) & 3][lc + di]; };
        auto H_ = [&](int di, int dj) -> T { return di == 0 ? hw[1 + dj] : hl; };
        auto BX_ = [&](int di, int dj) -> T { return RBx[dj < 0 ? s3m : (dj > 0 ? s3p : s3o)][lc + di]; };
        auto BY_ = [&](int di, int dj) -> T { return RBy[dj < 0 ? s3m : (dj > 0 ? s3p : s3o)][lc + di]; };
        T fx, fy;
        jac_force<T>(A_, H_, BX_, BY_, 0, 0, g, fx, fy);
        if (col_ok) {
            const long o = (long)jo * a.sy + gx;
            a.Fx[o] = fx;
            a.Fy[o] = fy;
        }
    }
}

template <typename T, int NT, int PF>
__global__ __launch_bounds__(NT) void k_lorentz_divergence_march(OpArgs<T> a, int nstrips, int nseg, int LY) {
    constexpr int XH = 3, RW = NT + 2 * XH, TXO = NT - 2 * XH;
    __shared__ T RA[4][RW];     // A rows jf-1 .. jf+1 (jf = jo+2 is the row whose face quantities are being formed)
    __shared__ T Rh[2][RW];     // h row jf
    // face quantities are formed two rows ahead of their x-stencil use; each lane keeps them in registers and publishes
    // only the row the neighbours need now (keeps LDS at 31 KB -> 5 workgroups per CU)
    __shared__ T RBx[2][RW];    // face Bx  (fcc) row jo
    __shared__ T RHBx[3][RW];   // face hBx (fcc) rows jo-1, jo
    __shared__ T RBy[2][RW];    // face By  (cfc) row jo
    __shared__ T RHBy[2][RW];   // face hBy (cfc) row jo+1

    const unsigned bid = xcd_remap(blockIdx.x, (unsigned)(nstrips * nseg));
    const int strip = (int)(bid % nstrips), seg = (int)(bid / nstrips);
    const int x0 = strip * TXO;
    const int J0 = a.j0 + seg * LY;
    const int J1 = (J0 + LY < a.j1) ? J0 + LY : a.j1;
    const int c = threadIdx.x, lc = c + XH;
    const int gx = x0 - XH + c;
    const int gxc = clampi(gx, -a.Hx, a.Nx + a.Hx - 1);
    const int ylo = -a.Hy, yhi = a.Ny + a.Hy - 1;
    const Geo<T> g{a.dx, a.dy, a.rdx, a.rdy};
    const bool col_ok = (c >= XH) && (c < NT - XH) && (gx < a.Nx);
    const T rAz = a.rdx * a.rdy;

    // windows of this lane's column: A(c, jf-1 .. jf+1), h(c, jf-1 .. jf), and the face quantities it formed earlier
    T aw[3], hw[2];
    T bxw[5], byw[5], hbxw[4], hbyw[4];   // Bx/By (c, jo-2 .. jo+2), hBx/hBy (c, jo-1 .. jo+2)
#pragma unroll
    for (int k = 0; k < 3; ++k) aw[k] = T(0);
    hw[0] = hw[1] = T(1);
#pragma unroll
    for (int k = 0; k < 5; ++k) { bxw[k] = T(0); byw[k] = T(0); }
#pragma unroll
    for (int k = 0; k < 4; ++k) { hbxw[k] = T(0); hbyw[k] = T(0); }
    T f2 = T(0), g2 = T(0);   // carried: F2(c, jo), G2(c, jo-1)
    T pa[PF], ph[PF];
    auto ldrow = [&](int row, T &na, T &nh) {
        const long o = (long)clampi(row, ylo, yhi) * a.sy + gxc;
        na = a.A[o]; nh = a.h[o];
    };
    {   // ---- prologue: rows J0-3 .. J0+2 of A and h, the PF rows in flight and the x-neighbour values in ONE burst; the face quantities
        //      of rows J0-2 .. J0+1, the carried y-fluxes F2(c, J0), G2(c, J0-1) and the LDS rows the first output row reads but does not
        //      write are formed directly.  Replaces six warm-up iterations per segment (13 % of a 46-row segment).
        const int jo = J0;
        auto colx = [&](int dxi) -> int { return clampi(gx + dxi, -a.Hx, a.Nx + a.Hx - 1); };
        const int cm1 = colx(-1), cm2 = colx(-2), cp1 = colx(1);
        long ro[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) ro[k] = (long)clampi(J0 - 3 + k, ylo, yhi) * a.sy;
        T qa[6], qh[6], Am1[6], Ap1[5], Am2[2], Hm1[4];
#pragma unroll
        for (int k = 0; k < 6; ++k) { qa[k] = a.A[ro[k] + gxc]; qh[k] = a.h[ro[k] + gxc]; Am1[k] = a.A[ro[k] + cm1]; }
#pragma unroll
        for (int k = 0; k < 5; ++k) Ap1[k] = a.A[ro[k] + cp1];
        Am2[0] = a.A[ro[2] + cm2]; Am2[1] = a.A[ro[3] + cm2];
#pragma unroll
        for (int k = 0; k < 4; ++k) Hm1[k] = a.h[ro[k + 1] + cm1];
#pragma unroll
        for (int k = 0; k < PF; ++k) ldrow(J0 + 3 + k, pa[k], ph[k]);
        // face quantities of rows r = jo-2+t, t = 0 .. 3 (reference :134-148); q-index of row r is t+1
        T m_[4], n_[4], bx_[4], by_[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            m_[t] = -(T(0.25) * g.rdy) * ((Am1[t + 2] - Am1[t]) + (qa[t + 2] - qa[t]));
            n_[t] = (T(0.25) * g.rdx) * ((Ap1[t] - Am1[t]) + (Ap1[t + 1] - Am1[t + 1]));
            bx_[t] = m_[t] * (T(2) * fast_recip<T>(Hm1[t] + qh[t + 1]));
            by_[t] = n_[t] * (T(2) * fast_recip<T>(qh[t] + qh[t + 1]));
        }
        // windows as the first output iteration (it = 6, jo = J0) finds them BEFORE its shifts
        aw[1] = qa[4]; aw[2] = qa[5];                 // A(c, jo+1), A(c, jo+2)
        hw[0] = qh[4]; hw[1] = qh[5];                 // h(c, jo+1), h(c, jo+2)
        bxw[1] = bx_[0]; bxw[2] = bx_[1]; bxw[3] = bx_[2]; bxw[4] = bx_[3];   // bxw[k] = Bx(c, jo-3+k)
        byw[1] = by_[0]; byw[2] = by_[1]; byw[3] = by_[2]; byw[4] = by_[3];
        hbxw[2] = m_[2]; hbxw[3] = m_[3];             // hbxw[k] = hBx(c, jo-2+k)
        hbyw[2] = n_[2]; hbyw[3] = n_[3];
        const int r3o = ((jo % 3) + 3) % 3, r3m = (r3o + 2) % 3;
        RHBx[r3m][lc] = m_[1];                        // hBx(c, jo-1)
        RA[(jo + 1) & 3][lc] = qa[4];
        RA[(jo + 2) & 3][lc] = qa[5];
        const T hby_w = (T(0.25) * g.rdx) * ((qa[2] - Am2[0]) + (qa[3] - Am2[1]));   // hBy(c-1, jo)
        f2 = g.dx * upwind_biased_product<T>(T(0.5) * (hby_w + n_[2]), left3<T>(bx_[0], bx_[1], bx_[2]), right3<T>(bx_[1], bx_[2], bx_[3]));
        g2 = g.dx * upwind_biased_product<T>(T(0.5) * (n_[1] + n_[2]), left3<T>(by_[0], by_[1], by_[2]), right3<T>(by_[1], by_[2], by_[3]));
    }

    const int niter = (J1 - J0) + 6;
    const ProgressPriority prio(niter);
    for (int it = 6; it < niter; ++it) {
        prio.at(it);
        const int jr = J0 - 3 + it, jf = jr - 1, jo = jr - 3;
        aw[0] = aw[1]; aw[1] = aw[2]; aw[2] = pa[0];   // A(c, jf-1 .. jf+1)
        const T hnew = ph[0];                          // h(c, jr); the window lags one row: h(c, jf-1 .. jf)
#pragma unroll
        for (int k = 0; k + 1 < PF; ++k) { pa[k] = pa[k + 1]; ph[k] = ph[k + 1]; }
        if (it + PF < niter) ldrow(jr + PF, pa[PF - 1], ph[PF - 1]);

        const int r3o = ((jo % 3) + 3) % 3, r3m = (r3o + 2) % 3;
        RA[jr & 3][lc] = aw[2];       // A(c, jr)
        Rh[jf & 1][lc] = hw[1];       // h(c, jf)   (hw still holds rows jf-1, jf here: shifted at the end of the iteration)
        // the windows still hold last iteration's rows here: bxw[k] = Bx(c, jo-3+k), hbxw[k] = hBx(c, jo-2+k), same for By
        RBx[jo & 1][lc] = bxw[3];     // Bx(c, jo)
        RHBx[r3o][lc] = hbxw[2];      // hBx(c, jo)      (row jo-1 was published by the previous iteration)
        RBy[jo & 1][lc] = byw[3];     // By(c, jo)
        RHBy[(jo + 1) & 1][lc] = hbyw[3];   // hBy(c, jo+1)
        phase_sync<NT>();
        {   // face quantities of row jf (reference :134-148), once per face
            const T *am = RA[(jf - 1) & 3], *a0 = RA[jf & 3], *ap = RA[(jf + 1) & 3];
            const T m = -(T(0.25) * g.rdy) * ((ap[lc - 1] - am[lc - 1]) + (aw[2] - aw[0]));
            const T n = (T(0.25) * g.rdx) * ((am[lc + 1] - am[lc - 1]) + (a0[lc + 1] - a0[lc - 1]));
            const T bx = m * (T(2) * fast_recip<T>(Rh[jf & 1][lc - 1] + hw[1]));
            const T by = n * (T(2) * fast_recip<T>(hw[0] + hw[1]));
#pragma unroll
            for (int k = 0; k < 4; ++k) { bxw[k] = bxw[k + 1]; byw[k] = byw[k + 1]; }
#pragma unroll
            for (int k = 0; k < 3; ++k) { hbxw[k] = hbxw[k + 1]; hbyw[k] = hbyw[k + 1]; }
            bxw[4] = bx; byw[4] = by; hbxw[3] = m; hbyw[3] = n;
        }
        hw[0] = hw[1]; hw[1] = hnew;
        // y-direction fluxes (own column): F2(c, jo+1) and G2(c, jo); carried values give F2(c, jo), G2(c, jo-1)
        //   bxw[k] = Bx(c, jo-2+k), byw likewise; hbxw[k] = hBx(c, jo-1+k), hbyw likewise
        const T *hby1 = RHBy[(jo + 1) & 1];
        const T f2n = g.dx * upwind_biased_product<T>(T(0.5) * (hby1[lc - 1] + hbyw[2]),
                                                       left3<T>(bxw[1], bxw[2], bxw[3]), right3<T>(bxw[2], bxw[3], bxw[4]));
        const T g2n = g.dx * upwind_biased_product<T>(T(0.5) * (hbyw[1] + hbyw[2]),
                                                       left3<T>(byw[1], byw[2], byw[3]), right3<T>(byw[2], byw[3], byw[4]));
        {
            const T *bx0 = RBx[jo & 1], *hbx0 = RHBx[r3o], *hbxm = RHBx[r3m], *by0 = RBy[jo & 1];
            auto F1 = [&](int cc) -> T {   // lorentz_flux_hBx_bx @ccc (cc, jo)
                return g.dy * upwind_biased_product<T>(T(0.5) * (hbx0[cc] + hbx0[cc + 1]), left3<T>(bx0[cc - 1], bx0[cc], bx0[cc + 1]),
                                                       right3<T>(bx0[cc], bx0[cc + 1], bx0[cc + 2]));
            };
            auto G1 = [&](int cc) -> T {   // lorentz_flux_hBx_by @ffc (cc, jo)
                return g.dy * upwind_biased_product<T>(T(0.5) * (hbxm[cc] + hbx0[cc]), left3<T>(by0[cc - 2], by0[cc - 1], by0[cc]),
                                                       right3<T>(by0[cc - 1], by0[cc], by0[cc + 1]));
            };
            const T fx = rAz * ((F1(lc) - F1(lc - 1)) + (f2n - f2));
            const T fy = rAz * ((G1(lc + 1) - G1(lc)) + (g2n - g2));
            if (col_ok) {
                const long o = (long)jo * a.sy + gx;
                a.Fx[o] = fx;
                a.Fy[o] = fy;
            }
        }
        f2 = f2n; g2 = g2n;
    }
}
