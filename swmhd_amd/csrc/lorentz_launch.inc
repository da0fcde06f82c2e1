// Launchers of the Lorentz operator kernels: each asks launch_plan.hpp what to enqueue (plan_lorentz: data, decided once per call) and
// enqueues it.  Included by lorentz_fast.hip / lorentz_strict.hip after the kernels (lorentz_tile_kernels.inc, same translation unit:
// the kernels stay in its anonymous namespace), with SWMHD_STRICT and LAUNCH_SFX defined.

namespace swmhd {

#define LAUNCH_NAME_(base, sfx) base##sfx
#define LAUNCH_NAME(base, sfx) LAUNCH_NAME_(base, sfx)

// One operator call: the launches of its plan in order, each with the caller's arguments and that entry's rows, topology and edge_cols.
// (the kernels lie in the code object in the order in which they are first named: marching before tile, Jacobian form before divergence)
template <typename T, bool DIV>
static hipError_t enqueue_lorentz(const OpArgs<T> &a, hipStream_t s) {
    constexpr int TYB = 4;
    const OpPlan plan = plan_lorentz({a.Nx, a.Ny, a.j0, a.j1, DIV, STRICT, a.kernel_variant, a.topo_x, a.topo_y, a.edge_cols});
    for (int i = 0; i < plan.n; ++i) {
        const OpLaunch &l = plan.e[i];
        OpArgs<T> b = a;
        b.j0 = l.j0; b.j1 = l.j1; b.topo_x = l.topo_x; b.topo_y = l.topo_y; b.edge_cols = l.edge_cols;
        if (l.kernel == OpKernel::MARCH) {   // (fast builds only: a strict plan has none)
#if !SWMHD_STRICT
            // (swept NT in {64,128,256,512} x PF in {1..4} on MI355X: all within 8 %.  A wavefront-shuffle variant -- one wave per
            // workgroup, x neighbours by DPP lane shifts, no LDS -- measured 10-24 % slower; a packed two-columns-per-lane fp32 variant
            // 117.7 vs 116.0 us at 16384 x 2048: with the hardware reciprocal the unpacked kernel is HBM-bound at the fp64 kernel's
            // rate, 4.6 TB/s.  Both were removed, DESIGN.md 4.1)
            constexpr int NT = OP_MARCH_NT, PF = 2;
            void (*k)(OpArgs<T>, int, int, int);
            if constexpr (DIV) k = k_lorentz_divergence_march<T, NT, PF>;
            else k = k_lorentz_jacobian_march<T, NT, PF>;
            hipLaunchKernelGGL(k, dim3(l.mg.blocks()), dim3(l.mg.nt), 0, s, b, l.mg.nstrips, l.mg.nseg, l.mg.LY);
#else
            return hipErrorInvalidValue;
#endif
        } else {
            void (*k)(OpArgs<T>, int, int);
            if constexpr (DIV) k = k_lorentz_divergence<T, TILE_X, TYB, OP_DIV_TILE_Y / TYB>;
            else k = k_lorentz_jacobian<T, TILE_X, TYB, OP_JAC_TILE_Y / TYB>;
            hipLaunchKernelGGL(k, dim3(l.ntx * l.nty), dim3(TILE_X, TYB), 0, s, b, l.ntx, l.nty);
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

template <typename T>
hipError_t LAUNCH_NAME(launch_lorentz_jacobian_, LAUNCH_SFX)(const OpArgs<T> &a, hipStream_t s) {
    return enqueue_lorentz<T, false>(a, s);
}
template <typename T>
hipError_t LAUNCH_NAME(launch_lorentz_divergence_, LAUNCH_SFX)(const OpArgs<T> &a, hipStream_t s) {
    return enqueue_lorentz<T, true>(a, s);
}

template hipError_t LAUNCH_NAME(launch_lorentz_jacobian_, LAUNCH_SFX)<double>(const OpArgs<double> &, hipStream_t);
template hipError_t LAUNCH_NAME(launch_lorentz_jacobian_, LAUNCH_SFX)<float>(const OpArgs<float> &, hipStream_t);
template hipError_t LAUNCH_NAME(launch_lorentz_divergence_, LAUNCH_SFX)<double>(const OpArgs<double> &, hipStream_t);
template hipError_t LAUNCH_NAME(launch_lorentz_divergence_, LAUNCH_SFX)<float>(const OpArgs<float> &, hipStream_t);

}  // namespace swmhd
