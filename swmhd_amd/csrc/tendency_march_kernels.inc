// Fused tendency kernel, row-marching form (fast build only) for the VectorInvariantFormulation + Jacobian-form Lorentz
// forcing (the model of jacobian_formulation/SWMHD_example.jl:21-33; BASELINE config 3, the headline).
//
// The tile kernel recomputes every face flux twice and every vorticity value ~12x and re-reads a 3-cell halo per 64x8 tile.
// Here a workgroup owns a strip of NT-6 columns and marches up LY rows:
//   * one lane = one column; the y-direction stencils (h, A, u, v and the left neighbour's v: 6-7 rows each) live in
//     REGISTER windows that shift by one row per iteration -> every y-face flux is computed once and carried;
//   * x-direction stencils read short LDS row rings (23 rows in all: only the rows being differenced now), with the upwind
//     side chosen by lane-local LDS addressing; every x-face flux and the vorticity row are computed once and shared;
//   * centre Bx, By for the Lorentz force are computed once per cell (one reciprocal of h) into 3-row LDS rings;
//   * the next row's loads (and the G- values of the output row) are issued a full iteration ahead of use; all global
//     traffic is x-coalesced 512-B wave rows addressed as SGPR base + one shared 32-bit VGPR offset; the RK3 substep is
//     fused (the old state is in the register windows).
// Two workgroup barriers per row.  152-168 VGPRs / 48 KB LDS -> 3 workgroups per CU.  What bounds it: DESIGN.md section 4.1.
// Results differ from the strict/oracle order only by rounding (tests: <= 1e-12 max-norm).
//
// (needs <type_traits>)
// Included from tendency_fast.hip inside namespace swmhd { namespace { ... } } after sw_device.inc / lorentz_device.inc.

// Memory operations are straight-line code (buffer stores with out-of-range offsets for lanes that own no output column,
// compile-time stage MODE, explicit exact wait): see common.hpp.  Before: 25 % of wave time in s_waitcnt
// (profiles/r01/tendency_pmc_sq.json), every wave waiting for the stores it had just issued.
// MODE: bit 0 = fused RK3 substep (writes Unew), bit 1 = the substep reads G- (not the first stage), bit 2 = store G, bit 3 = RK3 in
// anchor form (common.hpp: Rk3Buffers) -- with bits 0 (9): store Unew = U + dtg G and W = U + dtw G (W through the G descriptors); with
// bits 0, 1 (11): read W where G- is read otherwise, store Unew = W + dtg G.  Both move 96 B/cell in fp64.
// A segment starts with a PROLOGUE: the seven rows its windows need are loaded in ONE burst (plus eleven x-neighbour values) and what
// the steady loop carries in is computed directly -- the two y-face fluxes at the segment's first face, Kh of the row below, two rows
// of centre B and the LDS rows the first iteration reads but does not write: about half a row's worth of arithmetic, no barrier.
// (Round 1 filled the windows with six full warm-up iterations per segment: twelve barriers, twelve x-flux reconstructions, six
// dependent HBM round trips -- 4-8 % of the launch on 1024^2 grids and 4096 x 512 slabs.)
//
// The windows are one element longer than a stencil: each row works on elements [0, n) and has its prefetched row land in element n;
// one shift by one per row follows.
// Rows [J0, J1) of segment `seg`: LY-row segments of the launch's row range, then those of its optional second range (the two
// boundary zones of a slab in one launch, TendArgs::j0b/j1b).
template <typename TA> __device__ __forceinline__ void segment_rows(const TA &a, int seg, int LY, int &J0, int &J1) {
    const int nsa = (a.j1 - a.j0 + LY - 1) / LY;
    const bool second = seg >= nsa;
    const int base = second ? a.j0b + (seg - nsa) * LY : a.j0 + seg * LY, end = second ? a.j1b : a.j1;
    J0 = base;
    J1 = base + LY < end ? base + LY : end;
}

// Folded last strip (TendArgs::fold_last, fp64 with 256 lanes): where the last strip has at most NT/2 - 2 XH output columns (4096 columns:
// 16 strips of 250 and one of 96), its workgroups run waves 0-1 and waves 2-3 as two independent 128-lane sub-strips of that strip, each
// with its own halo lanes and its own LDS columns, on two segments.  A segment row then costs 16.5 workgroups instead of 17.  Block ids:
// per pair of segments, the full strips of the first, then those of the second, then one folded workgroup for both.  The halves share the
// barriers, so both run as many iterations as the longer segment; the shorter half (last segment, or none at an odd segment count) runs
// its extra iterations with every store dropped and its G- loads on its own last row.
template <typename T, int LOR, int NT, int MODE>
__global__ __launch_bounds__(NT, 3) void k_tendency_vi_march(TendArgs<T> a, int nstrips, int nseg, int LY) {
    constexpr bool FUSE = (MODE & 1) != 0, HAS_GM = (MODE & 2) != 0, STORE_G = (MODE & 4) != 0, ANCHOR = (MODE & 8) != 0;
    constexpr bool STORE_W = ANCHOR && FUSE && !HAS_GM;   // first anchored stage: W goes out through the G descriptors
    constexpr bool FOLDS = NT == 256 && sizeof(T) == 8;  // built with the folded layout (the launcher folds nothing else)
    constexpr bool M64 = is_f64<T>::value;               // the MARCH64 arithmetic of sw_device.inc: every fp64 variant of this kernel, nothing else
    constexpr int XH = 3, NH = NT / 2, TXO = NT - 2 * XH;
    constexpr int RW = FOLDS ? 2 * (NH + 2 * XH) : NT + 2 * XH;   // LDS columns: a full strip, or two sub-strips side by side
    __shared__ T Ru[3][RW];    // u rows jo-1, jo (+1: written while the previous row's readers may still run)
    __shared__ T Rvn[1][RW];   // v newest row (to fetch the left neighbour's value for the vl window)
    __shared__ __attribute__((aligned(16))) T RHA[4][RW][2];   // per column (A, h): A rows jo-1 .. jo+1 (+1 being written), h row jo --
                                                              // interleaved so that the x-flux stencils fetch both with one address
    __shared__ T RBx[3][RW];   // centre Bx rows jo-1 .. jo+1
    __shared__ T RBy[3][RW];   // centre By rows jo-1 .. jo+1
    __shared__ T RFh[1][RW];   // x-face flux of h at face c, row jo
    __shared__ T RFA[1][RW];   // x-face flux of A
    __shared__ T RK[1][RW];    // Kh(c, jo) (fp64: Kh + g h): computed once per cell in P2, read by the right neighbour in P3
    __shared__ T RZUV[RW][3];  // per column: zeta(c, jo) and the velocities uf, vf at the vorticity point, for the x-direction stencil
                               // (interleaved: one LDS address per stencil point serves all three; 24-B stride is conflict-free)

    const bool fold = FOLDS && a.fold_last;
    const int nfull = fold ? nstrips - 1 : nstrips;   // full strips
    const unsigned bid = xcd_remap(blockIdx.x, (unsigned)(fold ? nfull * nseg + (nseg + 1) / 2 : nstrips * nseg));
    int strip = (int)(bid % nstrips), seg = (int)(bid / nstrips);
    bool half_wg = false;   // a folded workgroup
    int hf = 0;             // this wave's sub-strip in it
    if (fold) {
        const int pr = (int)bid / (2 * nfull + 1), r = (int)bid - pr * (2 * nfull + 1);   // segments 2 pr, 2 pr + 1
        half_wg = r >= (2 * pr + 1 < nseg ? 2 : 1) * nfull;                              // (after the pair's full-strip workgroups)
        if (half_wg) hf = __builtin_amdgcn_readfirstlane((int)threadIdx.x / NH);         // (wave-uniform: the row arithmetic stays scalar)
        strip = half_wg ? nfull : r % nfull;
        seg = 2 * pr + (half_wg ? hf : r / nfull);
    }
    int J0, J1, niter;
    segment_rows(a, seg - hf, LY, J0, J1);   // a folded workgroup iterates over its first segment, the longer one
    niter = (J1 - J0) + 6;
    if (hf) {
        if (seg < nseg) segment_rows(a, seg, LY, J0, J1);
        else J0 = J1 = a.j1;                 // (odd segment count: the last folded workgroup's second half has no rows)
    }
    const int x0 = strip * TXO;
    const int c = threadIdx.x - hf * NH, lc = c + XH + hf * (NH + 2 * XH);   // lane and LDS column within the (sub-)strip
    const int gx = x0 - XH + c;
    const bool wx = (a.wrap & 1) != 0, wy = (a.wrap & 2) != 0;   // periodic images instead of halo cells (common.hpp)
    const int gxc = wrap_index(gx, a.Nx, -a.Hx, a.Nx + a.Hx - 1, wx);
    const int ylo = -a.Hy, yhi = a.Ny + a.Hy - 1;
    const T rdx = a.rdx, rdy = a.rdy;
    const Geo<T> g{a.dx, a.dy, a.rdx, a.rdy};
    const bool col_ok = (c >= XH) && (c < (half_wg ? NH : NT) - XH) && (gx < a.Nx);

    // register windows of this lane's column, one element longer than the stencils (see above): element k holds row jo-3+k (uw) /
    // jo-2+k (the others).
    // zw / svw: vorticity zeta(c, j) and v(c-1, j) + v(c, j) at the vorticity points of rows jo-2 .. jo+3 -- computed ONCE per incoming row
    // (round 2 kept the left neighbour's v instead and rebuilt all six of each every iteration: ~25 instructions per row)
    T uw[8], vw[7], zw[7], svw[7], hw[7], aw[7];
    T fhy = T(0), fay = T(0), km = T(0);   // carried: y-face fluxes at face jo, Kh(c, jo-1)

    // All global accesses use (uniform parent pointer in SGPRs) + (one 32-bit byte offset in a VGPR): the offset is shared by
    // the four fields of a row, so a row costs one integer multiply-add instead of four 64-bit address computations.  The host
    // only selects this kernel for fields smaller than 4 GiB.
    const long off0 = (long)a.Hy * a.sy + a.Hx;
    const int isy = (int)a.sy;
    auto LD = [&](const T *interior, unsigned ob) -> T { return *reinterpret_cast<const T *>(reinterpret_cast<const char *>(interior - off0) + ob); };
    // one lane-invariant column offset serves every access: the row loads, the G- loads (lanes that own no output column
    // read some in-bounds cell and ignore it) and the stores (those lanes pass SW_OOB instead)
    const unsigned colb = (unsigned)(gxc + a.Hx) * (unsigned)sizeof(T);
    auto rowoff = [&](int row) -> unsigned { return (unsigned)((row + a.Hy) * isy) * (unsigned)sizeof(T); };
    const unsigned pbytes = (unsigned)((a.Ny + 2 * a.Hy) * isy) * (unsigned)sizeof(T);
    const unsigned rowlast = rowoff(J1 - 1);
    __amdgpu_buffer_rsrc_t rG[4], rU[4];
    if constexpr (STORE_G || STORE_W) {
        rG[0] = out_rsrc(a.G1 - off0, pbytes); rG[1] = out_rsrc(a.G2 - off0, pbytes);
        rG[2] = out_rsrc(a.Gh - off0, pbytes); rG[3] = out_rsrc(a.GA - off0, pbytes);
    }
    if constexpr (FUSE) {
#pragma unroll
        for (int f = 0; f < 4; ++f) rU[f] = out_rsrc(a.Unew[f] - off0, pbytes);
    }

    {   // ---- prologue ----
        // rows J0-3 .. J0+3 of the four fields, the left neighbour's v for rows J0-2 .. J0+3, and the x-neighbour values of the
        // carried quantities (neighbouring lanes load the same lines: L1/L2 hits), all in flight together
        const unsigned colm = (unsigned)(wrap_index(gx - 1, a.Nx, -a.Hx, a.Nx + a.Hx - 1, wx) + a.Hx) * (unsigned)sizeof(T);
        const unsigned colp = (unsigned)(wrap_index(gx + 1, a.Nx, -a.Hx, a.Nx + a.Hx - 1, wx) + a.Hx) * (unsigned)sizeof(T);
        unsigned ro[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) ro[k] = rowoff(wrap_index(J0 - 3 + k, a.Ny, ylo, yhi, wy));
        T pu[7], pv[7], ph[7], pa[7], pvl[5];
#pragma unroll
        for (int k = 0; k < 7; ++k) { pu[k] = LD(a.q1, ro[k] + colb); pv[k] = LD(a.q2, ro[k] + colb); ph[k] = LD(a.h, ro[k] + colb); pa[k] = LD(a.A, ro[k] + colb); }
#pragma unroll
        for (int k = 0; k < 5; ++k) pvl[k] = LD(a.q2, ro[k + 1] + colm);
        const T ue_m = LD(a.q1, ro[2] + colp);                                   // u(c+1, J0-1)
        T a_wm = T(0), a_em = T(0), a_wo = T(0), a_eo = T(0);
        if constexpr (LOR == 1) {
            a_wm = LD(a.A, ro[2] + colm); a_em = LD(a.A, ro[2] + colp);           // A(c-1, J0-1), A(c+1, J0-1)
            a_wo = LD(a.A, ro[3] + colm); a_eo = LD(a.A, ro[3] + colp);           // A(c-1, J0),   A(c+1, J0)
        }
        // the windows as the first iteration (output row jo = J0) expects them
#pragma unroll
        for (int k = 0; k < 7; ++k) uw[k] = pu[k];
#pragma unroll
        for (int k = 0; k < 6; ++k) { vw[k] = pv[k + 1]; hw[k] = ph[k + 1]; aw[k] = pa[k + 1]; }
#pragma unroll
        for (int k = 0; k < 5; ++k) {     // rows J0-2 .. J0+2; row J0+3 (element 5) is computed by the first iteration
            zw[k] = (pv[k + 1] - pvl[k]) * rdx - (pu[k + 1] - pu[k]) * rdy;
            svw[k] = pvl[k] + pv[k + 1];
        }
        uw[7] = T(0); vw[6] = T(0); zw[5] = T(0); zw[6] = T(0); svw[5] = T(0); svw[6] = T(0); hw[6] = T(1); aw[6] = T(0);
        // carried in: y-face fluxes at face J0 (advecting velocity v(c, J0), stencil rows J0-3 .. J0+2) and Kh(c, J0-1)
        fhy = upwind_weno<T, M64>(vw[2], ph);
        fay = upwind_weno<T, M64>(vw[2], pa);
        km = T(0.25) * ((sq(uw[2]) + sq(ue_m)) + (sq(vw[1]) + sq(vw[2])));
        if constexpr (M64) km = fma_<T>(a.grav, hw[1], km);   // (M64 carries the Bernoulli sum Kh + g h: see RK below)
        // LDS rows the first iteration reads but does not write: u(J0-1); A(J0-1), A(J0); centre B of rows J0-1, J0
        const int q3o = ((J0 % 3) + 3) % 3, q3m = (q3o + 2) % 3;
        Ru[q3m][lc] = uw[2];
        RHA[(J0 - 1) & 3][lc][0] = aw[1];
        RHA[J0 & 3][lc][0] = aw[2];
        if constexpr (LOR == 1) {
            const T rhm = recip_lorentz<T, M64>(hw[1]), rho = recip_lorentz<T, M64>(hw[2]);
            RBy[q3m][lc] = (T(0.5) * rdx) * (a_em - a_wm) * rhm;
            RBx[q3m][lc] = -(T(0.5) * rdy) * (aw[2] - aw[0]) * rhm;
            RBy[q3o][lc] = (T(0.5) * rdx) * (a_eo - a_wo) * rho;
            RBx[q3o][lc] = -(T(0.5) * rdy) * (aw[3] - aw[1]) * rho;
        }
    }

    // One output row.
    auto body = [&](const int it) {
        constexpr int LU = 7, LW = 6;   // landing elements of the prefetched row
        T *const U = uw, *const V = vw, *const Z = zw, *const SV = svw, *const Hh = hw, *const Aa = aw;
        const int jr = J0 - 3 + it;   // newest row in the windows
        const int jo = jr - 3;        // output row of this iteration
        {   // prefetch row jr+1 straight into the free window elements
            const unsigned ob = rowoff(wrap_index(jr + 1, a.Ny, ylo, yhi, wy)) + colb;
            uw[LU] = LD(a.q1, ob); vw[LW] = LD(a.q2, ob); hw[LW] = LD(a.h, ob); aw[LW] = LD(a.A, ob);
        }
        // G⁻ (W) of the output row is needed only at the very end of the iteration: issue its loads after the second barrier so their
        // HBM latency hides under the arithmetic in between
        T gm0 = T(0), gm1 = T(0), gm2 = T(0), gm3 = T(0);
        // Rows without an output (the extra iterations of a folded workgroup's shorter half): stores at pbytes + colb, beyond the
        // parent (dropped by the hardware); G- loads on the half's last row.  (Clamping the row itself instead cost 16-164 B of scratch.)
        const bool live = jo < J1;
        const unsigned rowb = live ? rowoff(jo) : pbytes;
        const unsigned og = (live ? rowb : rowlast) + colb;

        const int s3o = ((jo % 3) + 3) % 3, s3m = (s3o + 2) % 3, s3p = (s3o + 1) % 3;   // ring slots of rows jo, jo-1, jo+1
        const int s4o = jo & 3, s4p = (jo + 1) & 3;

        // ---- P1: publish the rows x-stencils will need ----
        Ru[s3o][lc] = U[3];       // u(c, jo)
        RHA[s4o][lc][1] = Hh[2];  // h(c, jo)
        RHA[s4p][lc][0] = Aa[3];  // A(c, jo+1)
        Rvn[0][lc] = V[5];        // v(c, jr)
        __syncthreads();

        // ---- P2: left neighbour's newest v; centre B at row jo+1; Kh and x-face fluxes at row jo ----
        {   // the newest row of the vorticity windows
            const T vl = Rvn[0][lc - 1];
            Z[5] = (V[5] - vl) * rdx - (U[6] - U[5]) * rdy;
            SV[5] = vl + V[5];
        }
        if constexpr (LOR == 1) {
            const T cxA = RHA[s4p][lc + 1][0] - RHA[s4p][lc - 1][0];
            const T cyA = Aa[4] - Aa[2];
            const T rh = recip_lorentz<T, M64>(Hh[3]);
            RBy[s3p][lc] = (T(0.5) * rdx) * cxA * rh;
            RBx[s3p][lc] = -(T(0.5) * rdy) * cyA * rh;
        }
        {   // Kh(c, jo): once per cell (read back below, together with the left neighbour's: nothing is held across the barrier)
            const T ue2 = Ru[s3o][lc + 1];
            const T kh = T(0.25) * ((sq(U[3]) + sq(ue2)) + (sq(V[2]) + sq(V[3])));
            if constexpr (M64) RK[0][lc] = fma_<T>(a.grav, Hh[2], kh);   // Kh + g h: G1 and G2 then need one difference each
            else RK[0][lc] = kh;
        }
        // vorticity and the velocities at the vorticity point (f,f) for row jo: consumed by the x-direction stencil
        RZUV[lc][0] = Z[2];
        RZUV[lc][1] = T(0.5) * (U[2] + U[3]);
        RZUV[lc][2] = T(0.5) * SV[2];
        {
            const T uadv = U[3];
            const bool pos = uadv >= T(0);
            const int base = pos ? lc - 3 : lc + 2, st = pos ? 1 : -1;
            T qh[5], qa[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) { const T *r = RHA[s4o][base + st * k]; qa[k] = r[0]; qh[k] = r[1]; }
            if constexpr (M64) {   // the two reconstructions share one reciprocal (sw_device.inc: weno_combine_finish_pair)
                T rh_, ra_;
                weno_combine_finish_pair<T>(weno5_upwind_ordered_parts<T>(qh, pos), weno5_upwind_ordered_parts<T>(qa, pos), rh_, ra_);
                RFh[0][lc] = uadv * rh_;
                RFA[0][lc] = uadv * ra_;
            } else {
                RFh[0][lc] = uadv * weno5_upwind_ordered<T, M64>(qh, pos);
                RFA[0][lc] = uadv * weno5_upwind_ordered<T, M64>(qa, pos);
            }
        }
        __syncthreads();
        if constexpr (FUSE && HAS_GM) {   // G- of the output row: needed at the very end, ~2/3 of an iteration away
            gm0 = LD(a.Gm[0], og); gm1 = LD(a.Gm[1], og); gm2 = LD(a.Gm[2], og); gm3 = LD(a.Gm[3], og);
        }

        // ---- P3: everything else for row jo ----
        // y-face fluxes at face jo+1 (advecting velocity v(c, jo+1)); the face-jo values are carried
        // (M64: the two reconstructions share one reciprocal, as RFh / RFA above)
        T fhy_n, fay_n;
        if constexpr (M64) {
            weno_combine_finish_pair<T>(upwind_weno_parts<T>(V[3], Hh), upwind_weno_parts<T>(V[3], Aa), fhy_n, fay_n);
            fhy_n *= V[3]; fay_n *= V[3];
        } else {
            fhy_n = upwind_weno<T, M64>(V[3], Hh);
            fay_n = upwind_weno<T, M64>(V[3], Aa);
        }
        // vertical_vorticity_U: zeta reconstructed along y to (f,c), VelocityStencil smoothness
        const T vhat = T(0.25) * (SV[2] + SV[3]);
        const T vortU = -upwind_weno_vel_raw<T, M64>(vhat, Z, U, SV);
        // vertical_vorticity_V: zeta reconstructed along x to (c,f); upwind-ordered reads (lane-local LDS addressing)
        const T *su0 = Ru[s3m], *su1 = Ru[s3o];
        const T ue = su1[lc + 1];
        const T uhat = T(0.25) * ((su0[lc] + su0[lc + 1]) + (U[3] + ue));
        T vortV;
        {
            const bool pos = uhat >= T(0);
            const int base = pos ? lc - 2 : lc + 3, st = pos ? 1 : -1;
            T zx[5], ufx[5], vfx[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) { const T *r = RZUV[base + st * k]; zx[k] = r[0]; ufx[k] = r[1]; vfx[k] = r[2]; }
            vortV = uhat * weno5_vel_upwind_ordered<T, M64>(zx, ufx, vfx, pos);
        }
        const T kc = RK[0][lc], kl = RK[0][lc - 1];   // Kh(c, jo) and the left neighbour's
        const T hl = RHA[s4o][lc - 1][1];
        T Fx = T(0), Fy = T(0);
        if constexpr (LOR == 1) {
            auto A_ = [&](int di, int dj) -> T { return di == 0 ? Aa[2 + dj] : RHA[(jo + dj) & 3][lc + di][0]; };
            auto H_ = [&](int di, int dj) -> T { return di == 0 ? Hh[2 + dj] : hl; };   // only (-1,0) is off-column
            auto BX_ = [&](int di, int dj) -> T { return RBx[dj < 0 ? s3m : (dj > 0 ? s3p : s3o)][lc + di]; };
            auto BY_ = [&](int di, int dj) -> T { return RBy[dj < 0 ? s3m : (dj > 0 ? s3p : s3o)][lc + di]; };
            jac_force<T, M64>(A_, H_, BX_, BY_, 0, 0, g, Fx, Fy);
        }
        T G1, G2;
        if constexpr (M64) {   // kc, kl, km are Bernoulli sums
            G1 = -vortU - (kc - kl) * rdx + a.fcor * vhat + Fx;
            G2 = -vortV - (kc - km) * rdy - a.fcor * uhat + Fy;
        } else {
            G1 = -vortU - (kc - kl) * rdx - a.grav * (Hh[2] - hl) * rdx + a.fcor * vhat + Fx;
            G2 = -vortV - (kc - km) * rdy - a.grav * (Hh[2] - Hh[1]) * rdy - a.fcor * uhat + Fy;
        }
        const T Gh = -((RFh[0][lc + 1] - RFh[0][lc]) * rdx + (fhy_n - fhy) * rdy);
        const T GA = -((RFA[0][lc + 1] - RFA[0][lc]) * rdx + (fay_n - fay) * rdy)
                     + Aa[2] * ((ue - U[3]) * rdx + (V[3] - V[2]) * rdy);
        // lanes / rows without an output: dropped by the hardware (the G- offset serves where there is one: one VALU add less)
        const unsigned o = FUSE && HAS_GM ? (col_ok && live ? og : SW_OOB) : (col_ok ? rowb + colb : SW_OOB);
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
                if constexpr (!HAS_GM) un = Us[f] + a.dtg * Gs[f];
                else if constexpr (ANCHOR) un = fma_<T>(a.dtg, Gs[f], Gms[f]);                                                  // W + dt gamma G
                else if constexpr (STORE_G) un = fma_<T>(a.cg, Gms[f], fma_<T>(a.dtg, Gs[f], fma_<T>(a.cu, Us[f], Us[f])));   // (common.hpp: cu, cg)
                else un = Us[f] + a.dt * (a.gamma * Gs[f] + a.zeta * Gms[f]);
                buffer_store<T>(un, rU[f], o);
            }
        }
        if constexpr (STORE_W) {
            const T Us[4] = {U[3], V[2], Hh[2], Aa[2]};
#pragma unroll
            for (int f = 0; f < 4; ++f) buffer_store<T>(Us[f] + a.dtw * Gs[f], rG[f], o);
        }
        fhy = fhy_n; fay = fay_n; km = kc;
        // The prefetched row must have landed; the memory operations issued after it (G- loads, stores) need not.  Stated
        // explicitly because the compiler would place its own wait behind the loop's back edge, where it has to assume the
        // worst over all incoming paths (vmcnt(0)).
        constexpr int YOUNGER = ((FUSE && HAS_GM) ? 4 : 0) + (STORE_G ? 4 : 0) + (FUSE ? 4 : 0) + (STORE_W ? 4 : 0);
        wait_vmem_all_but<YOUNGER>();
    };
    // after each row: shift the windows by one
    auto shift1 = [&]() {
#pragma unroll
        for (int k = 0; k < 7; ++k) uw[k] = uw[k + 1];
#pragma unroll
        for (int k = 0; k < 6; ++k) { vw[k] = vw[k + 1]; hw[k] = hw[k + 1]; aw[k] = aw[k + 1]; }
#pragma unroll
        for (int k = 0; k < 5; ++k) { zw[k] = zw[k + 1]; svw[k] = svw[k + 1]; }
    };

    const ProgressPriority prio(niter);
    int it = 6;
    // (A pair-unrolled loop -- one window rotation per TWO rows, 569 instead of 580 VALU instructions per row -- needs a few registers
    // more than the 168 a third wave per SIMD leaves: 8-52 bytes of scratch per lane depending on the stage variant.  Round 3, same call,
    // 4096^2 (profiles/r03/ab_rotation.txt): on the variants that read G- (MODE 3, 7: 8 / 12 B scratch) it equalled the plain loop within
    // the noise -- 388.7 / 495.8 / 406.5 vs 392.8 / 494.5 / 407.4 us per stage -- while 28 B of scratch cost the last stage 20 % (493 vs
    // 408 us).  It was removed after that measurement.)
    for (; it < niter; ++it) {
        prio.at(it);
        body(it);
        shift1();
    }
}

// ====================================================================================================================
// ConservativeFormulation (uh, vh, h) + tracer A with the divergence-form Lorentz forcing: the model of
// divergence_formulation/divergence_sw_mhd.jl:19-31 (BASELINE configs 2 and 4).  Same organisation as above:
//   own-column windows: uh, vh, A (rows jo-2 .. jo+3), h (rows jo-1 .. jo+3) and the face quantities of the Lorentz force;
//   LDS rings for x-access: uh row jo; vh rows jo, jo+1; h rows jo .. jo+2; A rows jo .. jo+3; Bx, hBx, By, hBy;
//   x-face fluxes (huu @ccc, huv @ffc, tracer flux, Lorentz F1/G1) are computed once in P2 and shared through LDS;
//   y-face fluxes (hvu, hvv, tracer flux, Lorentz F2/G2) are computed once and carried in registers.
// ====================================================================================================================
// Workgroups of 256 per CU (= waves per SIMD) the conservative kernel is compiled for, per stage variant: bit MODE of the mask set =
// 3, else 2.  At 168 VGPRs the variants need 0 (MODE 7), 12 (MODE 5), 20-60 (others) bytes of scratch per lane.  Measured on MI355X
// in one call (4096^2 step / 8192x1024 slab step): no variant at 3: 1.514 / 0.758 ms; MODE 7: 1.474 / 0.728; MODE 7+5: 1.452 / 0.721;
// all fused stages: 1.504 / 0.747 -- a third workgroup pays only where (almost) nothing spills.  The anchor variants (MODE 9, 11) need 0
// bytes of scratch at two workgroups and 12 at three; 4096^2 step, same call, alternating processes (profiles/rk3_anchor/README.md): two
// workgroups 1.435 ms (stages 454 / 485 / 480 us), three 1.365 ms (445 / 455 / 451 us) -- three it is.
// (CONS_W3_MODES and cons_minwaves are defined in launch_plan.hpp: the launch geometry reads the same table)
template <typename T, int LOR, int NT, int MODE>   // MODE as in k_tendency_vi_march
__global__ __launch_bounds__(NT, cons_minwaves(MODE, (int)sizeof(T))) void k_tendency_cons_march(TendArgs<T> a, int nstrips, int nseg, int LY) {
    constexpr bool FUSE = (MODE & 1) != 0, HAS_GM = (MODE & 2) != 0, STORE_G = (MODE & 4) != 0, ANCHOR = (MODE & 8) != 0;
    constexpr bool STORE_W = ANCHOR && FUSE && !HAS_GM;
    constexpr int XH = 3, RW = NT + 2 * XH, TXO = NT - 2 * XH;
    __shared__ T Ruh[3][RW];    // uh rows jo-1, jo (+1: the next row is published while this row's readers may still run)
    __shared__ T Rvh[3][RW];    // vh rows jo, jo+1
    // Ring depths are the minimum the two barriers allow (3 workgroups per CU need <= 52 KB each): a row that is read only in P2 may
    // be overwritten by the NEXT iteration's P1, because every wave passes the second barrier after its P2 reads.
    __shared__ T Rh[3][RW];     // h rows jo .. jo+2 (row jo is read in P2 only: its slot takes row jo+3 next iteration)
    __shared__ T RA[4][RW];     // A rows jo .. jo+3, all read in P2 only (the Lorentz faces of row jo+2 need rows jo+1 .. jo+3)
    __shared__ T RXu[1][RW];    // huu(c, jo)   momentum_flux_huu @ccc
    __shared__ T RXv[1][RW];    // huv(c, jo)   momentum_flux_huv @ffc
    __shared__ T RXa[1][RW];    // tracer x-flux at face c (already divided by ℑxᶠ h)
    __shared__ T RUe[1][RW];    // u = uh/ℑxᶠh at face c (for c div U)
    __shared__ T RBx[1][RW];    // face Bx row jo   (P2 only)
    __shared__ T RHBx[2][RW];   // face hBx rows jo-1, jo (P2 only)
    __shared__ T RBy[1][RW];    // face By row jo   (P2 only)
    __shared__ T RHBy[2][RW];
    __shared__ T RF1[1][RW];    // Lorentz F1(c, jo) @ccc
    __shared__ T RG1[1][RW];    // Lorentz G1(c, jo) @ffc

    const unsigned bid = xcd_remap(blockIdx.x, (unsigned)(nstrips * nseg));
    const int strip = (int)(bid % nstrips), seg = (int)(bid / nstrips);
    const int x0 = strip * TXO;
    int J0, J1;
    segment_rows(a, seg, LY, J0, J1);
    const int c = threadIdx.x, lc = c + XH;
    const int gx = x0 - XH + c;
    const bool wx = (a.wrap & 1) != 0, wy = (a.wrap & 2) != 0;   // periodic images instead of halo cells (common.hpp)
    const int gxc = wrap_index(gx, a.Nx, -a.Hx, a.Nx + a.Hx - 1, wx);
    const int ylo = -a.Hy, yhi = a.Ny + a.Hy - 1;
    const T rdx = a.rdx, rdy = a.rdy;
    const Geo<T> g{a.dx, a.dy, a.rdx, a.rdy};
    const bool col_ok = (c >= XH) && (c < NT - XH) && (gx < a.Nx);
    const T hg = T(0.5) * a.grav;

    T uw[6], vw[6], aw[6], hw[5];   // uh, vh, A (c, jo-2 .. jo+3);  h (c, jo-1 .. jo+3)
#pragma unroll
    for (int k = 0; k < 6; ++k) { uw[k] = T(0); vw[k] = T(0); aw[k] = T(0); }
#pragma unroll
    for (int k = 0; k < 5; ++k) hw[k] = T(1);
    // Lorentz faces: Bx/By (c, jo-2 .. jo+2) in windows.  hBx / hBy are NOT kept as windows (12 VGPRs, the difference between two
    // and three workgroups per CU): hBy(c, jo+2) waits one iteration in `hby_pub` and is read back from its LDS ring afterwards;
    // hBx(c, jo+1) is re-formed from Bx and the face-averaged h one iteration before it is published (`hbx_pub`).
    T bxw[5], byw[5], hbx_pub = T(0), hby_pub = T(0);
#pragma unroll
    for (int k = 0; k < 5; ++k) { bxw[k] = T(0); byw[k] = T(0); }
    // carried south-face values; the momentum and Lorentz y-fluxes enter uh / vh only through their difference: d1 = F2 - hvu, d2 = G2 - hvv
    T d1 = T(0), d2 = T(0), fya_s = T(0), hff_s = T(1), vs_ = T(0);

    // 32-bit byte offsets from the uniform parent pointers, straight-line memory operations (see k_tendency_vi_march)
    const long off0 = (long)a.Hy * a.sy + a.Hx;
    const int isy = (int)a.sy;
    auto LD = [&](const T *interior, unsigned ob) -> T { return *reinterpret_cast<const T *>(reinterpret_cast<const char *>(interior - off0) + ob); };
    const unsigned colb = (unsigned)(gxc + a.Hx) * (unsigned)sizeof(T);
    auto rowoff = [&](int row) -> unsigned { return (unsigned)((row + a.Hy) * isy) * (unsigned)sizeof(T); };
    auto ldrow = [&](int row, T &nu, T &nv, T &nh, T &na) {
        const unsigned ob = rowoff(wrap_index(row, a.Ny, ylo, yhi, wy)) + colb;
        nu = LD(a.q1, ob); nv = LD(a.q2, ob); nh = LD(a.h, ob); na = LD(a.A, ob);
    };
    const unsigned pbytes = (unsigned)((a.Ny + 2 * a.Hy) * isy) * (unsigned)sizeof(T);
    __amdgpu_buffer_rsrc_t rG[4], rU[4];
    if constexpr (STORE_G || STORE_W) {
        rG[0] = out_rsrc(a.G1 - off0, pbytes); rG[1] = out_rsrc(a.G2 - off0, pbytes);
        rG[2] = out_rsrc(a.Gh - off0, pbytes); rG[3] = out_rsrc(a.GA - off0, pbytes);
    }
    if constexpr (FUSE) {
#pragma unroll
        for (int f = 0; f < 4; ++f) rU[f] = out_rsrc(a.Unew[f] - off0, pbytes);
    }
    auto insert_row = [&](T nu, T nv, T nh, T na) {
#pragma unroll
        for (int k = 0; k < 5; ++k) { uw[k] = uw[k + 1]; vw[k] = vw[k + 1]; aw[k] = aw[k + 1]; }
#pragma unroll
        for (int k = 0; k < 4; ++k) hw[k] = hw[k + 1];
        uw[5] = nu; vw[5] = nv; aw[5] = na; hw[4] = nh;
    };
    {   // ---- prologue (as in k_tendency_vi_march): rows J0-3 .. J0+3 of the four fields and the x-neighbour values of everything the first
        //      row inherits, in one burst; then the Lorentz faces of rows J0-2 .. J0+1, the south-face fluxes of row J0 and the LDS rows
        //      the first iteration reads but does not write.  Replaces six warm-up iterations per segment.
        const int jo = J0;
        auto colo = [&](int dxi) -> unsigned { return (unsigned)(wrap_index(gx + dxi, a.Nx, -a.Hx, a.Nx + a.Hx - 1, wx) + a.Hx) * (unsigned)sizeof(T); };
        const unsigned cm1 = colo(-1), cm2 = colo(-2), cp1 = colo(1);
        unsigned ro[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) ro[k] = rowoff(wrap_index(J0 - 3 + k, a.Ny, ylo, yhi, wy));
        T pu[7], pv[7], ph[7], pa[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) { pu[k] = LD(a.q1, ro[k] + colb); pv[k] = LD(a.q2, ro[k] + colb); ph[k] = LD(a.h, ro[k] + colb); pa[k] = LD(a.A, ro[k] + colb); }
        T Hm1[4], Am1[6], Ap1[5], Am2[2];
#pragma unroll
        for (int k = 0; k < 4; ++k) Hm1[k] = LD(a.h, ro[k + 1] + cm1);          // h(c-1, jo-2 .. jo+1)
        const T Vm2 = LD(a.q2, ro[3] + cm2), Vm1 = LD(a.q2, ro[3] + cm1), Vp1 = LD(a.q2, ro[3] + cp1);   // vh(c-2, c-1, c+1; jo)
        if constexpr (LOR == 2) {
#pragma unroll
            for (int k = 0; k < 6; ++k) Am1[k] = LD(a.A, ro[k] + cm1);            // A(c-1, jo-3 .. jo+2)
#pragma unroll
            for (int k = 0; k < 5; ++k) Ap1[k] = LD(a.A, ro[k] + cp1);            // A(c+1, jo-3 .. jo+1)
            Am2[0] = LD(a.A, ro[2] + cm2); Am2[1] = LD(a.A, ro[3] + cm2);         // A(c-2, jo-1), A(c-2, jo)
        }
        // windows as the first steady iteration (output row jo = J0) expects them
#pragma unroll
        for (int k = 0; k < 6; ++k) { uw[k] = pu[k + 1]; vw[k] = pv[k + 1]; aw[k] = pa[k + 1]; }
#pragma unroll
        for (int k = 0; k < 5; ++k) hw[k] = ph[k + 2];
        T F2 = T(0), G2 = T(0);
        if constexpr (LOR == 2) {
            // face quantities of rows r = jo-2+t, t = 0 .. 3 (reference :134-148); p-index of row r is t+1
            T m_[4], n_[4], bx_[4], by_[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                m_[t] = -(T(0.25) * rdy) * ((Am1[t + 2] - Am1[t]) + (pa[t + 2] - pa[t]));
                n_[t] = (T(0.25) * rdx) * ((Ap1[t] - Am1[t]) + (Ap1[t + 1] - Am1[t + 1]));
                bx_[t] = m_[t] * (T(2) * recip<T>(Hm1[t] + ph[t + 1]));
                by_[t] = n_[t] * (T(2) * recip<T>(ph[t] + ph[t + 1]));
            }
            bxw[1] = bx_[0]; bxw[2] = bx_[1]; bxw[3] = bx_[2]; bxw[4] = bx_[3];   // pre-shift naming: bxw[k] = Bx(c, jo-3+k)
            byw[1] = by_[0]; byw[2] = by_[1]; byw[3] = by_[2]; byw[4] = by_[3];
            hbx_pub = m_[2];                       // hBx(c, jo): published by the first iteration
            hby_pub = n_[3];                       // hBy(c, jo+1)
            RHBx[(jo + 1) & 1][lc] = m_[1];        // hBx(c, jo-1)
            RHBy[jo & 1][lc] = n_[2];              // hBy(c, jo)
            const T hby_w = (T(0.25) * rdx) * ((pa[2] - Am2[0]) + (pa[3] - Am2[1]));   // hBy(c-1, jo)
            F2 = g.dx * upwind_biased_product<T>(T(0.5) * (hby_w + n_[2]), left3<T>(bx_[0], bx_[1], bx_[2]), right3<T>(bx_[1], bx_[2], bx_[3]));
            G2 = g.dx * upwind_biased_product<T>(T(0.5) * (n_[1] + n_[2]), left3<T>(by_[0], by_[1], by_[2]), right3<T>(by_[1], by_[2], by_[3]));
        }
        // south-face values of row jo: hvu and the tracer flux at face jo, hvv at centre jo-1, h_ff and v at face jo
        const T hff0 = T(0.25) * ((Hm1[1] + ph[2]) + (Hm1[2] + ph[3]));
        const T vtf = g.dx * sym4<T>(Vm2, Vm1, pv[3], Vp1);
        const T hvu0 = upwind_weno<T>(vtf, pu) * recip<T>(hff0);
        const T rhyf = T(2) * recip<T>(ph[2] + ph[3]);
        fya_s = g.dx * upwind_weno<T>(pv[3], pa) * rhyf;
        vs_ = pv[3] * rhyf;
        const T vtc = g.dx * sym4<T>(pv[1], pv[2], pv[3], pv[4]);
        T hvv0;
        {
            const auto pos = vtc >= T(0);
            T q[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) q[k] = pos ? pv[k] : pv[5 - k];
            hvv0 = vtc * weno5_upwind_ordered<T>(q, pos) * recip<T>(ph[2]);
        }
        d1 = F2 - hvu0; d2 = G2 - hvv0; hff_s = hff0;
        // LDS rows the first iteration reads but does not write
        const int r3o = ((jo % 3) + 3) % 3, r3m = (r3o + 2) % 3, r3p = (r3o + 1) % 3;
        Ruh[r3m][lc] = uw[1];               // uh(c, jo-1)
        Rvh[r3o][lc] = vw[2];               // vh(c, jo)
        Rh[r3o][lc] = hw[1];                // h(c, jo)
        Rh[r3p][lc] = hw[2];                // h(c, jo+1)
        RA[jo & 3][lc] = aw[2]; RA[(jo + 1) & 3][lc] = aw[3]; RA[(jo + 2) & 3][lc] = aw[4];   // A(c, jo .. jo+2)
    }

    auto body = [&](const int it) {
        const int jr = J0 - 3 + it, jo = jr - 3, jf = jr - 1;   // newest row, output row, Lorentz face row (= jo+2)
        T nu, nv, nh, na;
        ldrow(jr + 1, nu, nv, nh, na);
        T gm0 = T(0), gm1 = T(0), gm2 = T(0), gm3 = T(0);
        const unsigned rowb = rowoff(jo);
        const int r3o = ((jo % 3) + 3) % 3, r3m = (r3o + 2) % 3, r3p = (r3o + 1) % 3;

        // ---- P1: publish raw rows (and the Lorentz face rows the neighbours need now, from last iteration's windows) ----
        Ruh[r3o][lc] = uw[2];               // uh(c, jo)
        Rvh[r3p][lc] = vw[3];               // vh(c, jo+1)
        Rh[r3m][lc] = hw[3];                // h(c, jo+2)   (jo+2 = jo-1 mod 3)
        RA[jr & 3][lc] = aw[5];             // A(c, jo+3)
        if constexpr (LOR == 2) {           // windows still hold last iteration's rows: bxw[k] = Bx(c, jo-3+k)
            RBx[0][lc] = bxw[3];
            RHBx[jo & 1][lc] = hbx_pub;        // hBx(c, jo)
            RBy[0][lc] = byw[3];
            RHBy[(jo + 1) & 1][lc] = hby_pub;  // hBy(c, jo+1)
        }
        __syncthreads();

        // ---- P2: x-direction fluxes of row jo (once per face) + Lorentz faces of row jo+2 ----
        const T *su = Ruh[r3o], *sv0 = Rvh[r3o], *sv1 = Rvh[r3p], *sh0 = Rh[r3o], *sh1 = Rh[r3p], *sa0 = RA[jo & 3];
        const T hc = hw[1], hl = sh0[lc - 1];            // h(c, jo), h(c-1, jo)
        const T rhc = recip<T>(hc);
        const T rhxf = T(2) * recip<T>(hl + hc);         // 1/ℑxᶠh (c, jo)
        {
            // momentum_flux_huu @ccc: upwind(ℑ³xᶜ(Ax uh), WENOx(uh) at centre c) / h
            const T ut = g.dy * sym4<T>(su[lc - 1], su[lc], su[lc + 1], su[lc + 2]);
            {
                const bool pos = ut >= T(0);
                const int base = pos ? lc - 2 : lc + 3, st = pos ? 1 : -1;
                T q[5];
#pragma unroll
                for (int k = 0; k < 5; ++k) q[k] = su[base + st * k];
                RXu[0][lc] = ut * weno5_upwind_ordered<T>(q, pos) * rhc;
            }
            // momentum_flux_huv @ffc: upwind(ℑ³yᶠ(Ax uh), WENOx(vh) at face c) / ℑxyᶠᶠh   (h_ff(c, jo) carried from last iteration)
            const T utf = g.dy * sym4<T>(uw[0], uw[1], uw[2], uw[3]);
            {
                const bool pos = utf >= T(0);
                const int base = pos ? lc - 3 : lc + 2, st = pos ? 1 : -1;
                T q[5];
#pragma unroll
                for (int k = 0; k < 5; ++k) q[k] = sv0[base + st * k];
                RXv[0][lc] = utf * weno5_upwind_ordered<T>(q, pos) * recip<T>(hff_s);
            }
            // tracer x-flux at face c: Ax upwind(uh(c,jo), WENOx(A)) / ℑxᶠh ; and the face velocity for c div U
            {
                const T uadv = uw[2];
                const bool pos = uadv >= T(0);
                const int base = pos ? lc - 3 : lc + 2, st = pos ? 1 : -1;
                T q[5];
#pragma unroll
                for (int k = 0; k < 5; ++k) q[k] = sa0[base + st * k];
                RXa[0][lc] = g.dy * uadv * weno5_upwind_ordered<T>(q, pos) * rhxf;
                RUe[0][lc] = uadv * rhxf;
            }
        }
        __builtin_amdgcn_sched_barrier(0);   // (scheduling fence: P2's phases are scheduled one after the other)
        if constexpr (LOR == 2) {
            // Lorentz x-direction fluxes of row jo from the face rows published in P1 (reference :38-60, :86-108)
            const T *bx0 = RBx[0], *hbx0 = RHBx[jo & 1], *hbxm = RHBx[(jo + 1) & 1], *by0 = RBy[0];
            RF1[0][lc] = g.dy * upwind_biased_product<T>(T(0.5) * (hbx0[lc] + hbx0[lc + 1]), left3<T>(bx0[lc - 1], bx0[lc], bx0[lc + 1]),
                                                         right3<T>(bx0[lc], bx0[lc + 1], bx0[lc + 2]));
            RG1[0][lc] = g.dy * upwind_biased_product<T>(T(0.5) * (hbxm[lc] + hbx0[lc]), left3<T>(by0[lc - 2], by0[lc - 1], by0[lc]),
                                                         right3<T>(by0[lc - 1], by0[lc], by0[lc + 1]));
            __builtin_amdgcn_sched_barrier(0);
            // face quantities of row jf = jo+2 (reference :134-148), once per face
            const T *am = RA[(jf - 1) & 3], *a0 = RA[jf & 3], *ap = RA[(jf + 1) & 3], *shf = Rh[r3m];
            const T m = -(T(0.25) * rdy) * ((ap[lc - 1] - am[lc - 1]) + (aw[5] - aw[3]));
            const T n = (T(0.25) * rdx) * ((am[lc + 1] - am[lc - 1]) + (a0[lc + 1] - a0[lc - 1]));
            const T bx = m * (T(2) * recip<T>(shf[lc - 1] + hw[3]));
            const T by = n * (T(2) * recip<T>(hw[2] + hw[3]));
#pragma unroll
            for (int k = 0; k < 4; ++k) { bxw[k] = bxw[k + 1]; byw[k] = byw[k + 1]; }
            bxw[4] = bx; byw[4] = by;
            hby_pub = n;                                               // hBy(c, jo+2): published by the next iteration
            hbx_pub = bxw[3] * (T(0.5) * (sh1[lc - 1] + hw[2]));         // hBx(c, jo+1) = Bx * face-averaged h
        }
        __syncthreads();
        if constexpr (FUSE && HAS_GM) {   // G- of the output row: needed at the very end of the iteration
            const unsigned og = rowb + colb;
            gm0 = LD(a.Gm[0], og); gm1 = LD(a.Gm[1], og); gm2 = LD(a.Gm[2], og); gm3 = LD(a.Gm[3], og);
        }

        // ---- P3: y-direction fluxes at the north face (jo+1), carried south-face values, assemble ----
        const T hn1 = hw[2];                                   // h(c, jo+1)
        const T hff_n = T(0.25) * ((hl + hc) + (sh1[lc - 1] + hn1));   // ℑxyᶠᶠh (c, jo+1)
        const T rhyf_n = T(2) * recip<T>(hc + hn1);            // 1/ℑyᶠh (c, jo+1)
        // momentum_flux_hvu @ffc (c, jo+1): upwind(ℑ³xᶠ(Ay vh)(c, jo+1), WENOy(uh) at face jo+1) / h_ff
        const T vtf = g.dx * sym4<T>(sv1[lc - 2], sv1[lc - 1], vw[3], sv1[lc + 1]);
        const T hvu_n = upwind_weno<T>(vtf, uw) * recip<T>(hff_n);
        // tracer y-flux at face jo+1: Ay upwind(vh(c, jo+1), WENOy(A)) / ℑyᶠh
        const T fya_n = g.dx * upwind_weno<T>(vw[3], aw) * rhyf_n;
        const T vn = vw[3] * rhyf_n;                           // v at face jo+1
        // momentum_flux_hvv @ccc (c, jo): upwind(ℑ³yᶜ(Ay vh)(c, jo) [rows jo-1 .. jo+2], WENOy(vh) at centre jo [rows jo-2 .. jo+3]) / h
        const T vtc = g.dx * sym4<T>(vw[1], vw[2], vw[3], vw[4]);
        T hvv_c;
        {
            const bool pos = vtc >= T(0);
            // centre jo lies between faces jo and jo+1: upwind-ordered stencil vh(jo-2 .. jo+2) or vh(jo+3 .. jo-1)
            T q[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) q[k] = pos ? vw[k] : vw[5 - k];
            hvv_c = vtc * weno5_upwind_ordered<T>(q, pos) * rhc;
        }
        T f2n = T(0), g2n = T(0);
        if constexpr (LOR == 2) {   // Lorentz y-direction fluxes: F2(c, jo+1) @ffc, G2(c, jo) @ccc (reference :62-84, :110-132)
            const T *hby1 = RHBy[(jo + 1) & 1];
            // after the P2 shift: bxw[k] = Bx(c, jo-2+k); hBy(c, jo) and hBy(c, jo+1) come back from the ring they were published to
            const T hby_o = RHBy[jo & 1][lc], hby_n = hby1[lc];
            f2n = g.dx * upwind_biased_product<T>(T(0.5) * (hby1[lc - 1] + hby_n), left3<T>(bxw[1], bxw[2], bxw[3]), right3<T>(bxw[2], bxw[3], bxw[4]));
            g2n = g.dx * upwind_biased_product<T>(T(0.5) * (hby_o + hby_n), left3<T>(byw[1], byw[2], byw[3]), right3<T>(byw[2], byw[3], byw[4]));
        }
        const T d1n = f2n - hvu_n, d2n = g2n - hvv_c;
        const T rAz = rdx * rdy;
        // x-differences of (Lorentz - momentum) fluxes; the y-differences come from the carried d1, d2
        T xu = -(RXu[0][lc] - RXu[0][lc - 1]), xv = -(RXv[0][lc + 1] - RXv[0][lc]);
        if constexpr (LOR == 2) {
            xu += RF1[0][lc] - RF1[0][lc - 1];
            xv += RG1[0][lc + 1] - RG1[0][lc];
        }
        // uh: −(1/V)(δx huu + δy hvu) − ∂x(½ g h²) + f ℑxyᶠᶜ(vh) + Fx,   Fx = (1/Az)(δx F1 + δy F2)   (reference :162-165)
        const T vbar = T(0.25) * ((sv0[lc - 1] + vw[2]) + (sv1[lc - 1] + vw[3]));
        const T G1 = rAz * (xu + (d1n - d1)) - (hg * sq(hc) - hg * sq(hl)) * rdx + a.fcor * vbar;
        // vh: −(1/V)(δx huv + δy hvv) − ∂y(½ g h²) − f ℑxyᶜᶠ(uh) + Fy,   Fy = (1/Az)(δx G1 + δy G2)   (reference :167-170)
        const T ubar = T(0.25) * ((uw[1] + Ruh[r3m][lc + 1]) + (uw[2] + su[lc + 1]));
        const T G2 = rAz * (xv + (d2n - d2)) - (hg * sq(hc) - hg * sq(hw[0])) * rdy - a.fcor * ubar;
        // h: −(1/Az)(δx(Δy uh) + δy(Δx vh))
        const T ue_t = su[lc + 1];
        const T Gh = -((ue_t - uw[2]) * rdx + (vw[3] - vw[2]) * rdy);
        // A: −(1/Az)(δx fx + δy fy) + A (δx(Δy u) + δy(Δx v))/Az with u = uh/ℑxᶠh, v = vh/ℑyᶠh
        const T GA = -rAz * ((RXa[0][lc + 1] - RXa[0][lc]) + (fya_n - fya_s))
                     + aw[2] * ((RUe[0][lc + 1] - RUe[0][lc]) * rdx + (vn - vs_) * rdy);
        const unsigned o = col_ok ? rowb + colb : SW_OOB;   // lanes without an output column: dropped by the hardware
        const T Gs[4] = {G1, G2, Gh, GA};
        if constexpr (STORE_G) {
            const unsigned oG = a.drop_G ? SW_OOB : o;      // (last RK3 stage running this variant: nothing reads its G)
#pragma unroll
            for (int f = 0; f < 4; ++f) buffer_store<T>(Gs[f], rG[f], oG);
        }
        if constexpr (FUSE) {
            const T Us[4] = {uw[2], vw[2], hc, aw[2]};
            const T Gms[4] = {gm0, gm1, gm2, gm3};
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                T un;
                if constexpr (!HAS_GM) un = Us[f] + a.dtg * Gs[f];
                else if constexpr (ANCHOR) un = fma_<T>(a.dtg, Gs[f], Gms[f]);
                else if constexpr (STORE_G) un = fma_<T>(a.cg, Gms[f], fma_<T>(a.dtg, Gs[f], fma_<T>(a.cu, Us[f], Us[f])));   // (common.hpp: cu, cg)
                else un = Us[f] + a.dt * (a.gamma * Gs[f] + a.zeta * Gms[f]);
                buffer_store<T>(un, rU[f], o);
            }
        }
        if constexpr (STORE_W) {
            const T Us[4] = {uw[2], vw[2], hc, aw[2]};
#pragma unroll
            for (int f = 0; f < 4; ++f) buffer_store<T>(Us[f] + a.dtw * Gs[f], rG[f], o);
        }
        d1 = d1n; d2 = d2n; fya_s = fya_n; hff_s = hff_n; vs_ = vn;
        constexpr int YOUNGER = ((FUSE && HAS_GM) ? 4 : 0) + (STORE_G ? 4 : 0) + (FUSE ? 4 : 0) + (STORE_W ? 4 : 0);
        wait_vmem_all_but<YOUNGER>();   // the prefetched row is back; younger G- loads and stores need not be
        insert_row(nu, nv, nh, na);
    };

    const int niter = (J1 - J0) + 6;
    const ProgressPriority prio(niter);
    for (int it = 6; it < niter; ++it) {
        prio.at(it);
        body(it);
    }
}
