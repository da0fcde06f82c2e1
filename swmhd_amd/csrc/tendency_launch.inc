// Launchers of the fused tendency kernels: each asks launch_plan.hpp what to enqueue (plan_tendency: data, decided once per call) and
// enqueues it.  Included by tendency_fast.hip / tendency_strict.hip after the kernels (tendency_tile_kernels.inc, same translation
// unit: the kernels stay in its anonymous namespace), with SWMHD_STRICT and LAUNCH_SFX defined.

namespace swmhd {

#define LAUNCH_NAME_(base, sfx) base##sfx
#define LAUNCH_NAME(base, sfx) LAUNCH_NAME_(base, sfx)

template <typename T> static TendPlanIn plan_input(const TendArgs<T> &a, int formulation, int members) {
    TendPlanIn in{};
    in.Nx = a.Nx; in.Ny = a.Ny; in.Hy = a.Hy; in.sy = a.sy; in.elem_size = (int)sizeof(T);
    in.j0 = a.j0; in.j1 = a.j1; in.j0b = a.j0b; in.j1b = a.j1b;
    in.formulation = formulation; in.strict = STRICT;
    in.kernel_variant = a.kernel_variant; in.wrap = a.wrap; in.leave_room = a.leave_room;
    in.topo_x = a.topo_x; in.topo_y = a.topo_y; in.edge_cols = a.edge_cols;
    in.fuse = a.fuse; in.first = a.first; in.store_G = a.store_G; in.gm_prev = a.gm_prev; in.anchor = a.anchor;
    in.members = members;
    return in;
}

#if !SWMHD_STRICT
template <typename T> using MarchKernel = void (*)(TendArgs<T>, int, int, int);
template <typename T, int MODE> static MarchKernel<T> march_kernel(int formulation, int lorentz, int nt, bool packed) {
    if constexpr (std::is_same<T, float>::value) {
        if (packed) return lorentz == 1 ? k_tendency_vi_march_pk<1, 256, MODE> : k_tendency_vi_march_pk<0, 256, MODE>;
    }
    if (formulation == 1) {
        if (nt == 128) return lorentz == 1 ? k_tendency_vi_march<T, 1, 128, MODE> : k_tendency_vi_march<T, 0, 128, MODE>;
        return lorentz == 1 ? k_tendency_vi_march<T, 1, 256, MODE> : k_tendency_vi_march<T, 0, 256, MODE>;
    }
    if (nt == 128) return lorentz == 2 ? k_tendency_cons_march<T, 2, 128, MODE> : k_tendency_cons_march<T, 0, 128, MODE>;
    return lorentz == 2 ? k_tendency_cons_march<T, 2, 256, MODE> : k_tendency_cons_march<T, 0, 256, MODE>;
}
template <typename T> static MarchKernel<T> march_kernel(int mode, int formulation, int lorentz, int nt, bool packed) {
    switch (mode) {
    case 1: return march_kernel<T, 1>(formulation, lorentz, nt, packed);
    case 3: return march_kernel<T, 3>(formulation, lorentz, nt, packed);
    case 4: return march_kernel<T, 4>(formulation, lorentz, nt, packed);
    case 5: return march_kernel<T, 5>(formulation, lorentz, nt, packed);
    case 7: return march_kernel<T, 7>(formulation, lorentz, nt, packed);
    case 9: return march_kernel<T, 9>(formulation, lorentz, nt, packed);
    case 11: return march_kernel<T, 11>(formulation, lorentz, nt, packed);
    default: return nullptr;
    }
}
#endif
// a marching entry of a plan (fast builds only: a strict plan has none)
template <typename T>
static hipError_t launch_march(const TendLaunch &l, TendArgs<T> &a, int formulation, int lorentz, hipStream_t s) {
#if !SWMHD_STRICT
    if (l.drop_G) a.drop_G = 1;
    a.fold_last = l.mg.fold;
    const MarchKernel<T> k = march_kernel<T>(l.mode, formulation, lorentz, l.mg.nt, l.kernel == TendKernel::MARCH_PACKED);
    if (!k) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k, dim3(l.mg.blocks()), dim3(l.mg.nt), 0, s, a, l.mg.nstrips, l.mg.nseg, l.mg.LY);
    return hipGetLastError();
#else
    return hipErrorInvalidValue;
#endif
}

// LDS-tiled kernel, 64 x 4 threads, RY output rows per thread; ENS: every tile of a.members members (grid folded or 2-D, see EnsTendArgs)
template <typename T, int RY, bool BND = false, bool ENS = false, bool PAR = false>
static hipError_t launch_tile(const TileArgs<T, ENS, PAR> &a, int formulation, int lorentz, int ntx, int nty, hipStream_t s) {
    constexpr int TX = TILE_X, TYB = 4;
    dim3 grid(ntx * nty);
    const dim3 block(TX, TYB);
    if constexpr (ENS) grid = a.fold ? dim3(ntx * nty * a.members) : dim3(ntx * nty, a.members);
    if (formulation == 1 && lorentz == 1) hipLaunchKernelGGL((k_tendency_tile<T, 1, 1, TX, TYB, RY, BND, ENS, PAR>), grid, block, 0, s, a, ntx, nty);
    else if (formulation == 1 && lorentz == 0) hipLaunchKernelGGL((k_tendency_tile<T, 1, 0, TX, TYB, RY, BND, ENS, PAR>), grid, block, 0, s, a, ntx, nty);
    else if (formulation == 0 && lorentz == 2) hipLaunchKernelGGL((k_tendency_tile<T, 0, 2, TX, TYB, RY, BND, ENS, PAR>), grid, block, 0, s, a, ntx, nty);
    else if (formulation == 0 && lorentz == 0) hipLaunchKernelGGL((k_tendency_tile<T, 0, 0, TX, TYB, RY, BND, ENS, PAR>), grid, block, 0, s, a, ntx, nty);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}
// One tendency call: the launches of its plan in order, each with the caller's arguments and that entry's row ranges, topology and
// edge_cols.
template <typename T>
hipError_t LAUNCH_NAME(launch_tendency_, LAUNCH_SFX)(const TendArgs<T> &a, int formulation, int lorentz, hipStream_t s) {
    const TendPlan plan = plan_tendency(plan_input(a, formulation, 0));
    for (int i = 0; i < plan.n; ++i) {
        const TendLaunch &l = plan.e[i];
        TendArgs<T> b = a;
        b.j0 = l.j0; b.j1 = l.j1; b.j0b = l.j0b; b.j1b = l.j1b;
        b.topo_x = l.topo_x; b.topo_y = l.topo_y; b.edge_cols = l.edge_cols;
        hipError_t e = hipErrorInvalidValue;
        // (the kernels lie in the code object in the order in which they are first named here; a strict plan has TILE_RY2 and TILE_BOUNDED only)
        if (!l.tile()) e = launch_march<T>(l, b, formulation, lorentz, s);
#if !SWMHD_STRICT
        else if (l.kernel == TendKernel::TILE_RY1) e = launch_tile<T, 1>(b, formulation, lorentz, l.ntx, l.nty, s);
#endif
        else if (l.kernel == TendKernel::TILE_BOUNDED) e = launch_tile<T, 2, true>(b, formulation, lorentz, l.ntx, l.nty, s);
        else if (l.kernel == TendKernel::TILE_RY2) e = launch_tile<T, 2>(b, formulation, lorentz, l.ntx, l.nty, s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// Ensemble stage: the LDS-tiled kernel over every tile of every member (one row range), at the tile height of the plan -- that of a
// single model of the member's size, so the compiled body is that model's and a periodic member's results are bitwise the single
// model's.  Bounded members always take the wall kernel, where a large single model takes the marching kernel plus the wall frame.
// Strict members are bitwise single models.  Fast Bounded members and members with their own parameters are promised the fast tolerances
// only: the fused substep rounds alike in every instantiation (substep_pinned), the tendencies are reassociated per instantiation.
// Members are folded into blockIdx.x by default.  Tile height and mapping were measured (tools/time_ensemble.py, profiles/ensemble/).
// Knob (read once; measurement only): SWMHD_ENS_MAP = 1 folds the member into blockIdx.x, 2 makes it blockIdx.y (launch_plan.hpp
// ensemble_member_map, which swmhd_ensemble_launch_geometry reports).
template <typename T, bool PAR>
static hipError_t launch_ensemble_stage(const TileArgs<T, true, PAR> &a, int formulation, int lorentz, hipStream_t s) {
    if (a.j1 <= a.j0 || a.members <= 0) return hipSuccess;
    TendPlanIn in = plan_input<T>(a, formulation, a.members);
    in.j0b = in.j1b = in.edge_cols = 0;
    const TendPlan plan = plan_tendency(in);
    if (plan.n != 1 || !plan.e[0].tile()) return plan.n ? hipErrorInvalidValue : hipSuccess;
    const TendLaunch &l = plan.e[0];
    const int map = ensemble_member_map();
    const long blocks = (long)l.ntx * l.nty * a.members;
    if (blocks >= (1L << 31) || (map == 2 && a.members > 65535)) return hipErrorInvalidConfiguration;
    TileArgs<T, true, PAR> e = a;
    e.fold = map == 2 ? 0 : 1;
    if (l.kernel == TendKernel::TILE_BOUNDED) return launch_tile<T, 2, true, true, PAR>(e, formulation, lorentz, l.ntx, l.nty, s);
    return l.kernel == TendKernel::TILE_RY1 ? launch_tile<T, 1, false, true, PAR>(e, formulation, lorentz, l.ntx, l.nty, s)
                                            : launch_tile<T, 2, false, true, PAR>(e, formulation, lorentz, l.ntx, l.nty, s);
}
template <typename T>
hipError_t LAUNCH_NAME(launch_tendency_ensemble_, LAUNCH_SFX)(const EnsTendArgs<T> &a, int formulation, int lorentz, hipStream_t s) {
    return launch_ensemble_stage<T, false>(a, formulation, lorentz, s);
}
// The same stage with per-member (g, f, dt) from a device table: the PAR instantiation of whichever kernel the plan names (the plan
// does not depend on the parameters), same member mapping.
template <typename T>
hipError_t LAUNCH_NAME(launch_ensemble_params_stage_, LAUNCH_SFX)(const EnsParTendArgs<T> &a, int formulation, int lorentz, hipStream_t s) {
    if (!a.params) return hipErrorInvalidValue;
    return launch_ensemble_stage<T, true>(a, formulation, lorentz, s);
}

template <typename T>
hipError_t LAUNCH_NAME(launch_rk3_substep_, LAUNCH_SFX)(const Rk3Args<T> &a, hipStream_t s) {
    if (a.j1 <= a.j0) return hipSuccess;
    hipLaunchKernelGGL((k_rk3_substep<T>), dim3((a.Nx + 255) / 256, a.j1 - a.j0), dim3(256), 0, s, a);
    return hipGetLastError();
}

template hipError_t LAUNCH_NAME(launch_tendency_, LAUNCH_SFX)<double>(const TendArgs<double> &, int, int, hipStream_t);
template hipError_t LAUNCH_NAME(launch_tendency_, LAUNCH_SFX)<float>(const TendArgs<float> &, int, int, hipStream_t);
template hipError_t LAUNCH_NAME(launch_tendency_ensemble_, LAUNCH_SFX)<double>(const EnsTendArgs<double> &, int, int, hipStream_t);
template hipError_t LAUNCH_NAME(launch_tendency_ensemble_, LAUNCH_SFX)<float>(const EnsTendArgs<float> &, int, int, hipStream_t);
template hipError_t LAUNCH_NAME(launch_ensemble_params_stage_, LAUNCH_SFX)<double>(const EnsParTendArgs<double> &, int, int, hipStream_t);
template hipError_t LAUNCH_NAME(launch_ensemble_params_stage_, LAUNCH_SFX)<float>(const EnsParTendArgs<float> &, int, int, hipStream_t);
template hipError_t LAUNCH_NAME(launch_rk3_substep_, LAUNCH_SFX)<double>(const Rk3Args<double> &, hipStream_t);
template hipError_t LAUNCH_NAME(launch_rk3_substep_, LAUNCH_SFX)<float>(const Rk3Args<float> &, hipStream_t);

}  // namespace swmhd
