// C-ABI of libswmhd.so (include/swmhd.h): argument validation + kernel launches.  No torch types, no
// global state; every call only enqueues work on the caller's stream.
#include "../../include/swmhd.h"
#include "api_args.hpp"
#include "common.hpp"
#include <initializer_list>
#include <math.h>

using namespace swmhd;

namespace {

template <typename T>
int lorentz_common(bool divergence, const T *A, const T *h, T *Fx, T *Fy, const Grid &g, const Rows &r, int flags, void *stream,
                   int topo_x = SWMHD_PERIODIC, int topo_y = SWMHD_PERIODIC) {
    if (!A || !h || !Fx || !Fy) return SWMHD_EINVAL;
    if (!g.extents_ok() || !g.spacing_ok() || !g.rows_ok(r.j0, r.j1)) return SWMHD_EINVAL;
    if (!g.halo_at_least(divergence ? 3 : 2)) return SWMHD_EHALO;
    if (!topology_ok(topo_x, topo_y)) return SWMHD_EINVAL;
    if (!divergence && (topo_x != SWMHD_PERIODIC || topo_y != SWMHD_PERIODIC)) return SWMHD_EINVAL;
    if (flags & ~LORENTZ_FLAGS) return SWMHD_EINVAL;
    if (r.j0 == r.j1) return SWMHD_OK;
    const Flags fl = decode_flags(flags);
    OpArgs<T> a;
    set_grid(a, g, topo_x, topo_y);
    a.A = g.interior(A); a.h = g.interior(h); a.Fx = g.interior(Fx); a.Fy = g.interior(Fy);
    a.j0 = r.j0; a.j1 = r.j1;
    a.kernel_variant = fl.kernel_variant;
    a.edge_cols = 0;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e;
    if (divergence) e = fl.strict ? launch_lorentz_divergence_strict<T>(a, s) : launch_lorentz_divergence_fast<T>(a, s);
    else e = fl.strict ? launch_lorentz_jacobian_strict<T>(a, s) : launch_lorentz_jacobian_fast<T>(a, s);
    return hiprc(e);
}

template <typename T>
int halo_common(T *f, const Grid &g, int which, void *stream) {
    if (!f || !g.extents_ok()) return SWMHD_EINVAL;
    if (!g.period_covers_halo(3)) return SWMHD_EHALO;
    if (which & ~(SWMHD_HALO_X | SWMHD_HALO_Y)) return SWMHD_EINVAL;
    return hiprc(launch_fill_halo_periodic<T>(g.interior(f), g.Nx, g.Ny, g.Hx, g.Hy, (long)g.sy, which, (hipStream_t)stream));
}

// the checks of swmhd_fill_halo (and of the ensemble); sets every field of `a` but the gradient values
template <typename T>
int halo_bc_args(HaloBc<T> &a, T *const *f, int nf, const Grid &g, const BcSides &s, const Ens *ens = nullptr) {
    if (const int rc = ens_check(ens, g, 0)) return rc;
    if (!f || nf < 1 || nf > 4 || !g.extents_ok()) return SWMHD_EINVAL;
    if (!topology_ok(s.topo_x, s.topo_y)) return SWMHD_EINVAL;
    if (!g.period_covers_halo(3)) return SWMHD_EHALO;
    if ((s.topo_x == SWMHD_BOUNDED && g.Hx < 1) || (s.topo_y == SWMHD_BOUNDED && g.Hy < 1)) return SWMHD_EHALO;   // the far wall lives in the first halo line
    if (!g.spacing_ok()) return SWMHD_EINVAL;
    for (int k = 0; k < 4; ++k) a.f[k] = nullptr;
    for (int k = 0; k < nf; ++k) {
        if (!f[k]) return SWMHD_EINVAL;
        a.f[k] = g.interior(f[k]);
    }
    a.nf = nf; a.Nx = g.Nx; a.Ny = g.Ny; a.Hx = g.Hx; a.Hy = g.Hy; a.sy = (long)g.sy; a.dx = T(g.dx); a.dy = T(g.dy);
    a.topo_x = s.topo_x; a.topo_y = s.topo_y; a.face_x = s.face_x; a.face_y = s.face_y;
    return SWMHD_OK;
}

// HaloBc::grad from a HOST array of 4 nf values (NULL: defaults everywhere)
template <typename T>
void host_gradient(HaloBc<T> &a, const T *gradient) {
    for (int k = 0; k < 4; ++k)
        for (int e = 0; e < 4; ++e) a.grad[k][e] = (gradient && k < a.nf) ? gradient[4 * k + e] : T(NAN);
}

// gradient: HOST array of 4 nf values (one grid), or with `ens` a DEVICE table of members x 4 nf values; NULL = defaults everywhere
template <typename T>
int halo_bc_common(T *const *f, int nf, const Grid &g, const BcSides &s, const T *gradient, void *stream, const Ens *ens = nullptr) {
    HaloBcEns<T> a;
    if (const int rc = halo_bc_args<T>(a, f, nf, g, s, ens)) return rc;
    host_gradient<T>(a, ens ? nullptr : gradient);
    if (!ens) return hiprc(launch_fill_halo_bc<T>(a, (hipStream_t)stream));
    a.stride_m = (long)ens->stride_m; a.members = ens->members; a.gtab = gradient;
    return hiprc(launch_fill_halo_bc_ensemble<T>(a, (hipStream_t)stream));
}

// q = (u|uh, v|vh, h, A), G = their tendencies.  Unew (optional): the second state a fused RK3 stage writes, Gm its G- operand (none: the
// first stage), the stage scalars in ph.
template <typename T>
int tend_common(const T *const *q, T *const *G, const Grid &g, const Physics<T> &ph, const Rows &r, int flags, void *stream,
                T *const *Unew = nullptr, const T *const *Gm = nullptr, const Ens *ens = nullptr) {
    if (const int rc = ens_check(ens, g, flags)) return rc;
    for (int f = 0; f < 4; ++f)
        if (!q[f] || !G[f]) return SWMHD_EINVAL;
    if (!g.extents_ok() || !g.spacing_ok()) return SWMHD_EINVAL;
    // Rows may reach up to Hy - 3 rows into the y halo (the stencil stays inside the padded array) unless y is wrapped or Bounded:
    // a slab with a deep halo evaluates its neighbours' edge rows itself instead of exchanging them every stage (ring.hip).
    const int ext = ((flags & (SWMHD_WRAP_Y | SWMHD_BOUNDED_Y)) || g.Hy < 3) ? 0 : g.Hy - 3;
    if (!g.rows_ok(r.j0, r.j1, ext)) return SWMHD_EINVAL;
    if (r.second() && (r.j0b < r.j1 || r.j1b > g.Ny + ext)) return SWMHD_EINVAL;
    if (flags & ~TEND_FLAGS) return SWMHD_EINVAL;
    if ((flags & OPEN_FLAGS) && (!(flags & SWMHD_BOUNDED_Y) || ens)) return SWMHD_EINVAL;   // a cut of a Bounded y direction
    const Flags fl = decode_flags(flags);
    if (fl.gm_prev) {   // fast, periodic, fused stage with a G- operand only (a Bounded grid's frame launch would read cells the first launch has overwritten)
        if (!Unew || !Gm) return SWMHD_EINVAL;
        if (fl.strict || fl.bounded()) return SWMHD_ENOTSUP;
    }
    if (fl.anchor) {    // fast, periodic, fused stage only; one operand form at a time
        if (!Unew || fl.gm_prev) return SWMHD_EINVAL;
        if (fl.strict || fl.bounded()) return SWMHD_ENOTSUP;
    }
    if (bounded_wrap_conflict(flags)) return SWMHD_EINVAL;
    if (fl.bounded() && (flags & SWMHD_MARCH_KERNEL)) return SWMHD_ENOTSUP;   // walls: LDS-tiled kernel only
    if (!g.period_covers_halo(fl.wrap)) return SWMHD_EHALO;
    if (!formulation_ok(ph.formulation) || !forcing_ok(ph.formulation, ph.lorentz)) return SWMHD_EINVAL;
    if (!g.halo_at_least(3)) return SWMHD_EHALO;
    if (r.j0 == r.j1 && !r.second()) return SWMHD_OK;
    TendArgs<T> a;
    set_grid(a, g, fl.topo_x, fl.topo_y);
    a.q1 = g.interior(q[0]); a.q2 = g.interior(q[1]); a.h = g.interior(q[2]); a.A = g.interior(q[3]);
    a.G1 = g.interior(G[0]); a.G2 = g.interior(G[1]); a.Gh = g.interior(G[2]); a.GA = g.interior(G[3]);
    a.grav = ph.grav; a.fcor = ph.fcor; a.j0 = r.j0; a.j1 = r.j1;
    a.j0b = r.second() ? r.j0b : 0; a.j1b = r.second() ? r.j1b : 0;
    a.fuse = 0; a.first = 0; a.store_G = 1; a.drop_G = 0; a.dt = a.gamma = a.zeta = T(0);
    a.gm_prev = fl.gm_prev; a.cu = a.cg = a.dtg = a.dtw = T(0);
    a.anchor = fl.anchor; a.wrap = fl.wrap; a.leave_room = fl.leave_room; a.kernel_variant = fl.kernel_variant;
    a.edge_cols = 0; a.fold_last = 0;
    for (int f = 0; f < 4; ++f) { a.Unew[f] = nullptr; a.Gm[f] = nullptr; }
    if (Unew) {
        a.fuse = 1; a.first = Gm ? 0 : 1; a.store_G = ph.store_G ? 1 : 0; a.dt = ph.dt; a.gamma = ph.gamma; a.zeta = ph.zeta;
        a.cu = a.gm_prev ? ph.zeta : T(0); a.cg = a.gm_prev ? -ph.zeta : ph.dt * ph.zeta; a.dtg = ph.dt * ph.gamma;
        if (a.anchor) {   // no G store: the first stage writes W through the G pointers, later stages only read W
            a.store_G = 0; a.cu = a.cg = T(0);
            a.dtw = Gm ? T(0) : ph.dt * ph.zeta;
        }
        for (int f = 0; f < 4; ++f) { a.Unew[f] = g.interior(Unew[f]); a.Gm[f] = Gm ? g.interior(Gm[f]) : nullptr; }
    }
    hipStream_t s = (hipStream_t)stream;
    const int form = ph.formulation, lor = ph.lorentz;
    if (ens) {
        EnsTendArgs<T> e;
        static_cast<TendArgs<T> &>(e) = a;
        e.stride_m = (long)ens->stride_m; e.members = ens->members; e.fold = 1;
        if (ens->par) {   // (g, f, dt and the products of dt come from the table, in the kernel)
            EnsParTendArgs<T> ep;
            static_cast<EnsTendArgs<T> &>(ep) = e;
            ep.params = static_cast<const T *>(ens->params);
            return hiprc(fl.strict ? launch_ensemble_params_stage_strict<T>(ep, form, lor, s) : launch_ensemble_params_stage_fast<T>(ep, form, lor, s));
        }
        return hiprc(fl.strict ? launch_tendency_ensemble_strict<T>(e, form, lor, s) : launch_tendency_ensemble_fast<T>(e, form, lor, s));
    }
    return hiprc(fl.strict ? launch_tendency_strict<T>(a, form, lor, s) : launch_tendency_fast<T>(a, form, lor, s));
}

template <typename T>
int rk3_common(T *const *U, const T *const *Gn, const T *const *Gm, const Grid &g, const Physics<T> &ph, const Rows &r, int flags,
               void *stream) {
    if (!U || !Gn || !g.extents_ok()) return SWMHD_EINVAL;
    if (!g.rows_ok(r.j0, r.j1) || (flags & ~SUBSTEP_FLAGS)) return SWMHD_EINVAL;
    Rk3Args<T> a;
    for (int f = 0; f < 4; ++f) {
        if (!U[f] || !Gn[f] || (Gm && !Gm[f])) return SWMHD_EINVAL;
        a.U[f] = g.interior(U[f]); a.Gn[f] = g.interior(Gn[f]); a.Gm[f] = g.interior(Gm ? Gm[f] : Gn[f]);
    }
    a.Nx = g.Nx; a.sy = (long)g.sy; a.j0 = r.j0; a.j1 = r.j1; a.dt = ph.dt; a.gamma = ph.gamma; a.zeta = ph.zeta; a.first = Gm ? 0 : 1;
    hipStream_t s = (hipStream_t)stream;
    return hiprc((flags & SWMHD_STRICT) ? launch_rk3_substep_strict<T>(a, s) : launch_rk3_substep_fast<T>(a, s));
}

// swmhd_tracers_rk3: K passive tracers through one RK3 stage in one launch (tracer_kernels.inc); q = (u|uh, v|vh, h), the state that
// advects them.  Every check precedes the first HIP call.  With `ens` (swmhd_ensemble_tracers_rk3[_params]): the tracers of every
// member of a periodic ensemble; the ensemble's own argument errors come first, then the single-grid checks in their order, with the
// Bounded flags among the unsupported ones.
template <typename T>
int tracers_common(const T *const *q, const T *const *c, T *const *cnew, T *const *Gn, const T *const *Gm, int K, const Grid &g,
                   const Physics<T> &ph, const Rows &r, int flags, void *stream, const Ens *ens = nullptr) {
    const int notsup = TRACER_NOTSUP | (ens ? BOUNDED_FLAGS : 0);
    if (const int rc = ens_check(ens, g, 0)) return rc;
    if (!q[0] || !q[1] || !q[2] || !c || !Gn) return SWMHD_EINVAL;
    if (K < 1 || K > SWMHD_MAX_TRACERS) return SWMHD_EINVAL;
    if (!g.extents_ok() || !g.spacing_ok() || !g.rows_ok(r.j0, r.j1)) return SWMHD_EINVAL;
    if (!formulation_ok(ph.formulation)) return SWMHD_EINVAL;
    if (flags & ~(TRACER_FLAGS | notsup)) return SWMHD_EINVAL;
    const Flags fl = decode_flags(flags);
    if (!cnew && !ph.store_G) return SWMHD_EINVAL;   // tendencies only: they must be stored
    if (!cnew && fl.anchor) return SWMHD_EINVAL;     // the anchor form is a form of the update
    for (int k = 0; k < K; ++k) {
        if (!c[k] || !Gn[k] || (cnew && !cnew[k]) || (Gm && !Gm[k])) return SWMHD_EINVAL;
        if (!cnew) continue;
        if (cnew[k] == q[0] || cnew[k] == q[1] || cnew[k] == q[2]) return SWMHD_EINVAL;
        for (int m = 0; m < K; ++m)
            if (cnew[k] == c[m] || (m != k && cnew[k] == cnew[m])) return SWMHD_EINVAL;   // neighbouring workgroups still read c through their halos
    }
    if (bounded_wrap_conflict(flags)) return SWMHD_EINVAL;
    if (!g.period_covers_halo(fl.wrap)) return SWMHD_EINVAL;   // (SWMHD_EHALO from tend_common: api_args.hpp)
    if (flags & notsup) return SWMHD_ENOTSUP;
    if (fl.anchor && (fl.strict || fl.bounded())) return SWMHD_ENOTSUP;
    if (!g.halo_at_least(3)) return SWMHD_EHALO;
    if (r.j0 == r.j1) return SWMHD_OK;
    TracerArgs<T> a;
    set_grid(a, g, fl.topo_x, fl.topo_y);
    a.q1 = g.interior(q[0]); a.q2 = g.interior(q[1]); a.h = g.interior(q[2]);
    for (int k = 0; k < MAX_TRACERS; ++k) {
        const bool on = k < K;
        a.c[k] = on ? g.interior(c[k]) : nullptr; a.Gn[k] = on ? g.interior(Gn[k]) : nullptr;
        a.cnew[k] = on && cnew ? g.interior(cnew[k]) : nullptr; a.Gm[k] = on && Gm ? g.interior(Gm[k]) : nullptr;
    }
    a.K = K; a.j0 = r.j0; a.j1 = r.j1;
    a.fuse = cnew ? 1 : 0; a.first = Gm ? 0 : 1; a.store_G = ph.store_G ? 1 : 0;
    a.anchor = fl.anchor; a.wrap = fl.wrap;
    a.dt = ph.dt; a.gamma = ph.gamma; a.zeta = ph.zeta; a.dtg = ph.dt * ph.gamma; a.dtw = T(0);
    if (a.anchor) {   // no G store: the first stage writes W through Gn, later stages only read W (tend_common)
        a.store_G = 0;
        a.dtw = Gm ? T(0) : ph.dt * ph.zeta;
    }
    hipStream_t s = (hipStream_t)stream;
    const int form = ph.formulation;
    if (ens) {
        EnsTracerArgs<T> e;
        static_cast<TracerArgs<T> &>(e) = a;
        e.stride_m = (long)ens->stride_m; e.members = ens->members;
        if (ens->par) {   // (dt and its products come from the table, in the kernel)
            EnsParTracerArgs<T> ep;
            static_cast<EnsTracerArgs<T> &>(ep) = e;
            ep.params = static_cast<const T *>(ens->params);
            return hiprc(fl.strict ? launch_tracers_ensemble_params_strict<T>(ep, form, s) : launch_tracers_ensemble_params_fast<T>(ep, form, s));
        }
        return hiprc(fl.strict ? launch_tracers_ensemble_strict<T>(e, form, s) : launch_tracers_ensemble_fast<T>(e, form, s));
    }
    return hiprc(fl.strict ? launch_tracers_strict<T>(a, form, s) : launch_tracers_fast<T>(a, form, s));
}

// ---- what the per-stage correction calls share (swmhd_coriolis_rk3, swmhd_diffusion_rk3, swmhd_biharmonic_rk3, swmhd_relaxation_rk3) ----
// Every check here answers SWMHD_EINVAL, and every SWMHD_EINVAL check of those calls precedes their other answers (SWMHD_ENOTSUP, then
// SWMHD_EHALO, then "nothing to do"), so the order among these is not observable (tests/golden/correction_return_codes.json holds the rest).
// member count and member strides: of the parents, then of a call's per-member masks and targets (0: one for all members); none: a single grid
bool correction_members_ok(const Ens *ens, const Grid &g, int64_t mask_sm = 0, int64_t target_sm = 0) {
    if (!ens) return true;
    const int64_t need = g.min_member_stride();
    return ens->members >= 1 && ens->members <= SWMHD_ENSEMBLE_MAX_MEMBERS && ens->stride_m >= need && (mask_sm == 0 || mask_sm >= need) &&
           (target_sm == 0 || target_sm >= need);
}
// no output is an input -- other workgroups still read old around their rows, and a mask or target may be shared by several fields -- or
// another output; a null entry is an absent one
template <typename T>
bool outputs_apart(const T *const *out, int nout, const T *const *in, int nin) {
    for (int k = 0; k < nout; ++k) {
        if (!out[k]) continue;
        for (int m = 0; m < nin; ++m)
            if (out[k] == in[m]) return false;
        for (int m = 0; m < k; ++m)
            if (out[k] == out[m]) return false;
    }
    return true;
}
// a correction over a list of fields: what it reads, what the stage wrote and (optional, as is each of its entries) the stored operand
template <typename T>
struct FieldSets {
    const T *const *old;
    T *const *nw, *const *acc;
    int nfields;
};
// the checks of such a call, the values of its host tables apart: sets and entries present, 1 .. max_fields fields, members, grid, rows,
// flags among `known`, a and w finite, outputs apart from old and from the `read_only` lists (at most two; a null list is absent)
template <typename T>
bool field_correction_ok(const FieldSets<T> &f, int max_fields, std::initializer_list<const T *const *> read_only, const Grid &g, T a, T w,
                         const Rows &r, int flags, int known, const Ens *ens, int64_t mask_sm = 0, int64_t target_sm = 0) {
    constexpr int CAP = SWMHD_RELAXATION_MAX_FIELDS;
    static_assert(CAP >= SWMHD_DIFFUSION_MAX_FIELDS, "the call with the longest list sizes the arrays below");
    if (!f.old || !f.nw || f.nfields < 1 || f.nfields > max_fields || max_fields > CAP || read_only.size() > 2) return false;
    if (!correction_members_ok(ens, g, mask_sm, target_sm)) return false;
    if (!g.extents_ok() || !g.spacing_ok() || !g.rows_ok(r.j0, r.j1) || (flags & ~known)) return false;
    if (!isfinite((double)a) || !isfinite((double)w)) return false;
    const T *out[2 * CAP], *in[3 * CAP];
    int nin = 0;
    for (int k = 0; k < f.nfields; ++k) {
        if (!f.old[k] || !f.nw[k]) return false;
        out[2 * k] = f.nw[k]; out[2 * k + 1] = f.acc ? f.acc[k] : nullptr;
        in[nin++] = f.old[k];
        for (const T *const *list : read_only)
            if (list) in[nin++] = list[k];
    }
    return outputs_apart<T>(out, 2 * f.nfields, in, nin);
}

// what the per-stage correction calls pass on alike (StripArgs, common.hpp)
template <typename T>
void set_strip(StripArgs<T> &s, const Grid &g, const Rows &r, const Flags &fl, T a, T w, const Ens *ens) {
    s.Nx = g.Nx; s.Ny = g.Ny; s.j0 = r.j0; s.j1 = r.j1; s.wrap = fl.wrap; s.sy = (long)g.sy; s.a = a; s.w = w;
    s.members = ens ? ens->members : 0; s.anchor = fl.anchor; s.stride_m = ens ? (long)ens->stride_m : 0;
    s.params = ens ? static_cast<const T *>(ens->params) : nullptr;
}

// The fields of `f` that live(k) keeps, packed to the front of d.old, d.nw and d.acc (DiffusionArgs, RelaxationArgs) at interior cell
// (1,1), the slots behind them nulled.  more(slot, k): what else field k brings into its slot; k < 0: the slot is unused.  Returns the
// number of fields kept.
template <typename Args, typename T, typename Live, typename More>
int pack_fields(Args &d, int slots, const FieldSets<T> &f, const Grid &g, Live live, More more) {
    int n = 0;
    for (int k = 0; k < f.nfields; ++k) {
        if (!live(k)) continue;
        d.old[n] = g.interior(f.old[k]); d.nw[n] = g.interior(f.nw[k]);
        d.acc[n] = (f.acc && f.acc[k]) ? g.interior(f.acc[k]) : nullptr;
        more(n++, k);
    }
    for (int k = n; k < slots; ++k) {
        d.old[k] = nullptr; d.nw[k] = nullptr; d.acc[k] = nullptr;
        more(k, -1);
    }
    return n;
}

// swmhd_diffusion_rk3: nw[k] += a coef[k] laplace(old[k]), acc[k] += w coef[k] laplace(old[k]) of up to SWMHD_DIFFUSION_MAX_FIELDS fields in
// one launch (diffusion.hip).  Every check precedes the first HIP call.  With `ens` (swmhd_ensemble_diffusion_rk3): `coef` is the DEVICE
// table of members x nfields values and is not looked at; ens->params (optional) brings every member's dt.  One grid: the fields with
// coef == 0 are left out of the launch here.
// radius: 1 the Laplacian (diffusion_common), 2 the biharmonic operator (biharmonic_common, below): the halo a direction without its
// WRAP flag needs, and the launcher.  The checks and their order are the same for both.
template <typename T>
int stencil_closure_common(int radius, const T *const *old, T *const *nw, T *const *acc, const T *coef, int nfields, const Grid &g, T a, T w,
                           const Rows &r, int flags, void *stream, const Ens *ens) {
    const FieldSets<T> f{old, nw, acc, nfields};
    if (!coef || !field_correction_ok<T>(f, SWMHD_DIFFUSION_MAX_FIELDS, {}, g, a, w, r, flags, DIFFUSION_FLAGS | DIFFUSION_NOTSUP, ens)) return SWMHD_EINVAL;
    if (!ens)
        for (int k = 0; k < nfields; ++k)
            if (!isfinite((double)coef[k]) || coef[k] < T(0)) return SWMHD_EINVAL;
    if (flags & DIFFUSION_NOTSUP) return SWMHD_ENOTSUP;
    const Flags fl = decode_flags(flags);
    if (!g.halo_or_wrap(radius, fl.wrap)) return SWMHD_EHALO;
    if (r.j0 == r.j1) return SWMHD_OK;
    DiffusionArgs<T> d;
    const int n = pack_fields(d, DIFFUSION_MAX_FIELDS, f, g, [&](int k) { return ens || coef[k] != T(0); },
                              [&](int slot, int k) { d.coef[slot] = (ens || k < 0) ? T(0) : coef[k]; });
    if (n == 0) return SWMHD_OK;
    set_strip(d, g, r, fl, a, w, ens);
    d.nfields = n; d.dx = T(g.dx); d.dy = T(g.dy); d.coef_tab = ens ? coef : nullptr;
    hipStream_t s = (hipStream_t)stream;
    if (radius == 2) return hiprc(fl.strict ? launch_biharmonic_strict<T>(d, s) : launch_biharmonic_fast<T>(d, s));
    return hiprc(fl.strict ? launch_diffusion_strict<T>(d, s) : launch_diffusion_fast<T>(d, s));
}
template <typename T>
int diffusion_common(const T *const *old, T *const *nw, T *const *acc, const T *coef, int nfields, const Grid &g, T a, T w, const Rows &r,
                     int flags, void *stream, const Ens *ens = nullptr) {
    return stencil_closure_common<T>(1, old, nw, acc, coef, nfields, g, a, w, r, flags, stream, ens);
}
// swmhd_biharmonic_rk3: nw[k] -= a coef[k] laplace(laplace(old[k])), acc[k] likewise with w (biharmonic.hip): diffusion_common's arguments,
// checks and order (include/swmhd_biharmonic.h); SWMHD_EHALO below a halo of 2, and other workgroups read old two rows around theirs.
template <typename T>
int biharmonic_common(const T *const *old, T *const *nw, T *const *acc, const T *coef, int nfields, const Grid &g, T a, T w, const Rows &r,
                      int flags, void *stream, const Ens *ens = nullptr) {
    return stencil_closure_common<T>(2, old, nw, acc, coef, nfields, g, a, w, r, flags, stream, ens);
}

// swmhd_coriolis_rk3: n1 += a fc vbar, n2 -= a ff ubar (and a1, a2 with w) in one launch (coriolis.hip).  Every check precedes the first
// HIP call, in the order include/swmhd_coriolis.h states.  With `ens` (swmhd_ensemble_coriolis_rk3): frow holds one table per member;
// ens->params (optional) brings every member's dt.
template <typename T>
int coriolis_common(const T *q1, const T *q2, T *n1, T *n2, T *a1, T *a2, const T *frow, const Grid &g, T a, T w, const Rows &r, int flags,
                    void *stream, const Ens *ens = nullptr) {
    if (!q1 || !q2 || !n1 || !n2 || !frow) return SWMHD_EINVAL;
    if ((a1 == nullptr) != (a2 == nullptr)) return SWMHD_EINVAL;
    if (!g.extents_ok() || !g.rows_ok(r.j0, r.j1)) return SWMHD_EINVAL;
    if ((flags & ~(CORIOLIS_FLAGS | CORIOLIS_NOTSUP)) || bounded_wrap_conflict(flags)) return SWMHD_EINVAL;
    const T *const in[2] = {q1, q2};
    const T *const out[4] = {n1, n2, a1, a2};
    if (!outputs_apart<T>(out, 4, in, 2)) return SWMHD_EINVAL;
    if (!isfinite((double)a) || !isfinite((double)w)) return SWMHD_EINVAL;
    if (!correction_members_ok(ens, g)) return SWMHD_EINVAL;
    if (flags & CORIOLIS_NOTSUP) return SWMHD_ENOTSUP;
    const Flags fl = decode_flags(flags);
    if (!g.halo_or_wrap(1, fl.wrap)) return SWMHD_EHALO;
    if (r.j0 == r.j1) return SWMHD_OK;
    CoriolisArgs<T> c;
    c.q1 = g.interior(q1); c.q2 = g.interior(q2); c.n1 = g.interior(n1); c.n2 = g.interior(n2);
    c.a1 = a1 ? g.interior(a1) : nullptr; c.a2 = a2 ? g.interior(a2) : nullptr;
    c.frow = frow;
    set_strip(c, g, r, fl, a, w, ens);
    hipStream_t s = (hipStream_t)stream;
    return hiprc(fl.strict ? launch_coriolis_strict<T>(c, s) : launch_coriolis_fast<T>(c, s));
}

// swmhd_relaxation_rk3: nw[k] += a D_k, acc[k] += w D_k with D_k = (rate[k] mask[k]) (target[k] - old[k]) of up to
// SWMHD_RELAXATION_MAX_FIELDS fields in one launch (relaxation.hip).  Every check precedes the first HIP call, in the order
// include/swmhd_relaxation.h states.  With `ens` (swmhd_ensemble_relaxation_rk3): `rate` and `tval` are the DEVICE tables of members x
// nfields values and are not looked at; mask_sm / target_sm pitch the members' masks and targets (0: shared); ens->params (optional)
// brings every member's dt.  One grid: the fields with rate == 0 are left out of the launch here.  (Radius 0, but a shared mask or
// target is read by other fields' workgroups: no output may be one.)
template <typename T>
int relaxation_common(const T *const *old, T *const *nw, T *const *acc, const T *const *mask, const T *const *target, const T *rate,
                      const T *tval, int nfields, const Grid &g, T a, T w, const Rows &r, int flags, void *stream, const Ens *ens = nullptr,
                      int64_t mask_sm = 0, int64_t target_sm = 0) {
    const FieldSets<T> f{old, nw, acc, nfields};
    if (!rate || !tval || bounded_wrap_conflict(flags)) return SWMHD_EINVAL;
    if (!field_correction_ok<T>(f, SWMHD_RELAXATION_MAX_FIELDS, {mask, target}, g, a, w, r, flags, RELAXATION_FLAGS | RELAXATION_NOTSUP, ens,
                                mask_sm, target_sm)) return SWMHD_EINVAL;
    if (!ens)
        for (int k = 0; k < nfields; ++k)
            if (!isfinite((double)rate[k]) || rate[k] < T(0) || !isfinite((double)tval[k])) return SWMHD_EINVAL;
    if (flags & RELAXATION_NOTSUP) return SWMHD_ENOTSUP;
    const Flags fl = decode_flags(flags);
    if (r.j0 == r.j1) return SWMHD_OK;
    RelaxationArgs<T> d;
    const int n = pack_fields(d, RELAXATION_MAX_FIELDS, f, g, [&](int k) { return ens || rate[k] != T(0); }, [&](int slot, int k) {
        d.mask[slot] = (k >= 0 && mask && mask[k]) ? g.interior(mask[k]) : nullptr;
        d.target[slot] = (k >= 0 && target && target[k]) ? g.interior(target[k]) : nullptr;
        d.rate[slot] = (ens || k < 0) ? T(0) : rate[k]; d.tval[slot] = (ens || k < 0) ? T(0) : tval[k];
    });
    if (n == 0) return SWMHD_OK;
    set_strip(d, g, r, fl, a, w, ens);
    d.wrap = 0;   // (nothing around a cell is read)
    d.nfields = n; d.mask_stride_m = ens ? (long)mask_sm : 0; d.target_stride_m = ens ? (long)target_sm : 0;
    d.rate_tab = ens ? rate : nullptr; d.tval_tab = ens ? tval : nullptr;
    hipStream_t s = (hipStream_t)stream;
    return hiprc(fl.strict ? launch_relaxation_strict<T>(d, s) : launch_relaxation_fast<T>(d, s));
}

// swmhd_particles_rk3, swmhd_particles_sample (particles.hip): the flags both take, what the grid of a call must be, and how a
// direction is indexed and folded.  Every check precedes the first HIP call, in the order include/swmhd_particles.h states.
constexpr int PARTICLES_FLAGS = SWMHD_STRICT | WRAP_FLAGS | BOUNDED_FLAGS;
constexpr int PARTICLES_NOTSUP = KERNEL_FLAGS | SWMHD_GM_IS_PREV_STATE | OPEN_FLAGS | SWMHD_LEAVE_ROOM | SWMHD_RK3_ANCHOR;
static_assert(PARTICLES_BLOCK == SWMHD_PARTICLES_BLOCK && PARTICLES_MAX_FIELDS == SWMHD_PARTICLES_MAX_FIELDS, "common.hpp mirrors swmhd_particles.h");
inline bool particles_grid_ok(const Grid &g, double x0, double y0, int64_t P, int flags) {
    if (!g.extents_ok() || !g.spacing_ok() || !isfinite(g.dx) || !isfinite(g.dy) || !isfinite(x0) || !isfinite(y0)) return false;
    if ((flags & ~(PARTICLES_FLAGS | PARTICLES_NOTSUP)) || bounded_wrap_conflict(flags) || P < 0) return false;
    return true;
}
inline int particles_after_einval(const Grid &g, int flags) {
    if (flags & PARTICLES_NOTSUP) return SWMHD_ENOTSUP;
    const Flags fl = decode_flags(flags);
    if (!g.halo_or_wrap(1, fl.wrap)) return SWMHD_EHALO;
    return SWMHD_OK;
}
inline void set_particle_grid(ParticleGrid &a, const Grid &g, double x0, double y0, int64_t P, int flags, const Ens *ens) {
    a.P = (long)P; a.Nx = g.Nx; a.Ny = g.Ny; a.Hx = g.Hx; a.Hy = g.Hy; a.sy = (long)g.sy;
    a.x0 = x0; a.y0 = y0; a.dx = g.dx; a.dy = g.dy;
    a.mode_x = (flags & SWMHD_WRAP_X) ? PARTICLE_WRAP : ((flags & SWMHD_BOUNDED_X) ? PARTICLE_BOUNDED : PARTICLE_PERIODIC);
    a.mode_y = (flags & SWMHD_WRAP_Y) ? PARTICLE_WRAP : ((flags & SWMHD_BOUNDED_Y) ? PARTICLE_BOUNDED : PARTICLE_PERIODIC);
    a.members = ens ? ens->members : 0; a.stride_m = ens ? (long)ens->stride_m : 0; a.nblk = 0;
}
template <typename T>
int particles_common(const T *q1, const T *q2, const T *h, double *x, double *y, double *gx, double *gy, int64_t P, const Grid &g, double x0,
                     double y0, int form, double dt, double gamma, double zeta, int flags, void *stream, const Ens *ens = nullptr) {
    if (!q1 || !q2 || !x || !y || !gx || !gy) return SWMHD_EINVAL;
    if (x == y || x == gx || x == gy || y == gx || y == gy || gx == gy) return SWMHD_EINVAL;
    if (!particles_grid_ok(g, x0, y0, P, flags)) return SWMHD_EINVAL;
    if (!isfinite(dt) || !isfinite(gamma) || !isfinite(zeta)) return SWMHD_EINVAL;
    if (!formulation_ok(form) || (form == SWMHD_CONSERVATIVE && !h)) return SWMHD_EINVAL;
    if (!correction_members_ok(ens, g)) return SWMHD_EINVAL;
    if (const int rc = particles_after_einval(g, flags)) return rc;
    if (P == 0) return SWMHD_OK;
    ParticleArgs<T> a;
    set_particle_grid(a, g, x0, y0, P, flags, ens);
    a.q1 = g.interior(q1); a.q2 = g.interior(q2); a.h = h ? g.interior(h) : nullptr;
    a.x = x; a.y = y; a.gx = gx; a.gy = gy;
    a.cons = form == SWMHD_CONSERVATIVE;
    a.params = ens ? (const T *)ens->params : nullptr;
    a.dt = a.params ? 1.0 : dt; a.gamma = gamma; a.zeta = zeta;
    return hiprc(launch_particles<T>(a, (hipStream_t)stream));
}
template <typename T>
int particles_sample_common(const T *const *fields, const int *loc, int nfields, const double *x, const double *y, double *out, int64_t P,
                            const Grid &g, double x0, double y0, int flags, void *stream, const Ens *ens = nullptr) {
    if (!fields || !loc || !x || !y || !out || nfields < 1 || nfields > SWMHD_PARTICLES_MAX_FIELDS) return SWMHD_EINVAL;
    for (int k = 0; k < nfields; ++k)
        if (!fields[k] || loc[k] < 0 || loc[k] > (SWMHD_PARTICLES_CENTER_X | SWMHD_PARTICLES_CENTER_Y)) return SWMHD_EINVAL;
    if (out == x || out == y) return SWMHD_EINVAL;
    if (!particles_grid_ok(g, x0, y0, P, flags)) return SWMHD_EINVAL;
    if (!correction_members_ok(ens, g)) return SWMHD_EINVAL;
    if (const int rc = particles_after_einval(g, flags)) return rc;
    if (P == 0) return SWMHD_OK;
    ParticleSampleArgs<T> a;
    set_particle_grid(a, g, x0, y0, P, flags, ens);
    for (int k = 0; k < PARTICLES_MAX_FIELDS; ++k) {
        a.f[k] = k < nfields ? g.interior(fields[k]) : nullptr;
        a.loc[k] = k < nfields ? loc[k] : 0;
    }
    a.nfields = nfields; a.x = x; a.y = y; a.out = out;
    return hiprc(launch_particles_sample<T>(a, (hipStream_t)stream));
}

// swmhd_stochastic_rk3: nw[k] += a F_k, acc[k] += w F_k with F_k the sum of nmodes[k] Fourier modes from the tables and the step's
// coefficient pairs, of up to SWMHD_STOCHASTIC_MAX_FIELDS fields in one launch (stochastic.hip).  Every check precedes the first HIP
// call, in the order include/swmhd_stochastic.h states: relaxation_common's, then the tables.  With `ens`
// (swmhd_ensemble_stochastic_rk3): coef_sm pitches the members' coefficients; a parameter table (a per-member dt) is refused.  The
// fields without modes are left out of the launch here.
template <typename T>
bool table_ok(const T *p) { return p && (uintptr_t)p % sizeof(T) == 0; }
template <typename T>
int stochastic_common(const T *const *old, T *const *nw, T *const *acc, const T *const *coef, const T *const *xtab, const T *const *ytab,
                      const int *nmodes, int nfields, int64_t xp, int64_t yp, const Grid &g, T a, T w, const Rows &r, int flags, void *stream,
                      const Ens *ens = nullptr, int64_t coef_sm = 0) {
    const FieldSets<T> f{old, nw, acc, nfields};
    if (bounded_wrap_conflict(flags)) return SWMHD_EINVAL;
    if (!field_correction_ok<T>(f, SWMHD_STOCHASTIC_MAX_FIELDS, {}, g, a, w, r, flags, RELAXATION_FLAGS | RELAXATION_NOTSUP, ens)) return SWMHD_EINVAL;
    if (!coef || !xtab || !ytab || !nmodes || xp < g.Nx || yp < g.Ny) return SWMHD_EINVAL;
    for (int k = 0; k < nfields; ++k) {
        if (nmodes[k] < 0 || nmodes[k] > SWMHD_STOCHASTIC_MAX_MODES) return SWMHD_EINVAL;
        if (nmodes[k] == 0) continue;
        if (!table_ok(coef[k]) || !table_ok(xtab[k]) || !table_ok(ytab[k])) return SWMHD_EINVAL;
        if (ens && coef_sm < 2 * (int64_t)nmodes[k]) return SWMHD_EINVAL;
    }
    if (ens && ens->params) return SWMHD_ENOTSUP;
    if (flags & RELAXATION_NOTSUP) return SWMHD_ENOTSUP;
    const Flags fl = decode_flags(flags);
    if (r.j0 == r.j1) return SWMHD_OK;
    StochasticArgs<T> d;
    const int n = pack_fields(d, STOCHASTIC_MAX_FIELDS, f, g, [&](int k) { return nmodes[k] != 0; }, [&](int slot, int k) {
        d.coef[slot] = k >= 0 ? coef[k] : nullptr; d.xtab[slot] = k >= 0 ? xtab[k] : nullptr; d.ytab[slot] = k >= 0 ? ytab[k] : nullptr;
        d.M[slot] = k >= 0 ? nmodes[k] : 0;
    });
    if (n == 0) return SWMHD_OK;
    set_strip(d, g, r, fl, a, w, ens);
    d.wrap = 0;   // (nothing around a cell is read)
    d.params = nullptr;
    d.nfields = n; d.xp = (long)xp; d.yp = (long)yp; d.coef_stride_m = ens ? (long)coef_sm : 0;
    hipStream_t s = (hipStream_t)stream;
    return hiprc(fl.strict ? launch_stochastic_strict<T>(d, s) : launch_stochastic_fast<T>(d, s));
}

// swmhd_source_rk3: nw[k] += a D_k, acc[k] += w D_k with D_k = source[k], or source[k] times old[thickness] interpolated to the x face
// (kind 1) or the y face (kind 2), of up to SWMHD_SOURCE_MAX_FIELDS fields in one launch (source.hip).  Every check precedes the first
// HIP call, in the order include/swmhd_source.h states.  With `ens` (swmhd_ensemble_source_rk3): source_sm pitches the members' sources
// (0: shared); ens->params (optional) brings every member's dt.  The fields without a source are left out of the launch here.
template <typename T>
int source_common(const T *const *old, T *const *nw, T *const *acc, const T *const *source, const int *kind, int nfields, int thickness,
                  const Grid &g, T a, T w, const Rows &r, int flags, void *stream, const Ens *ens = nullptr, int64_t source_sm = 0) {
    const FieldSets<T> f{old, nw, acc, nfields};
    if (!source || !kind || bounded_wrap_conflict(flags)) return SWMHD_EINVAL;
    if (!field_correction_ok<T>(f, SWMHD_SOURCE_MAX_FIELDS, {source}, g, a, w, r, flags, SOURCE_FLAGS | SOURCE_NOTSUP, ens, source_sm)) return SWMHD_EINVAL;
    if (thickness < -1 || thickness >= nfields) return SWMHD_EINVAL;
    bool weighted = false;
    for (int k = 0; k < nfields; ++k) {
        if (kind[k] < SWMHD_SOURCE_PLAIN || kind[k] > SWMHD_SOURCE_Y_FACE) return SWMHD_EINVAL;
        weighted = weighted || (source[k] && kind[k] != SWMHD_SOURCE_PLAIN);
    }
    if (weighted && thickness < 0) return SWMHD_EINVAL;
    if (flags & SOURCE_NOTSUP) return SWMHD_ENOTSUP;
    const Flags fl = decode_flags(flags);
    if (weighted && !g.halo_or_wrap(1, fl.wrap)) return SWMHD_EHALO;
    if (r.j0 == r.j1) return SWMHD_OK;
    SourceArgs<T> d;
    const int n = pack_fields(d, SOURCE_MAX_FIELDS, f, g, [&](int k) { return source[k] != nullptr; }, [&](int slot, int k) {
        d.src[slot] = k >= 0 ? g.interior(source[k]) : nullptr;
        d.kind[slot] = k >= 0 ? kind[k] : 0;
    });
    if (n == 0) return SWMHD_OK;
    set_strip(d, g, r, fl, a, w, ens);
    d.hold = weighted ? g.interior(old[thickness]) : nullptr;
    d.nfields = n; d.source_stride_m = ens ? (long)source_sm : 0;
    hipStream_t s = (hipStream_t)stream;
    return hiprc(fl.strict ? launch_source_strict<T>(d, s) : launch_source_fast<T>(d, s));
}
static_assert(SOURCE_MAX_FIELDS == SWMHD_SOURCE_MAX_FIELDS && SWMHD_SOURCE_MAX_FIELDS <= SWMHD_RELAXATION_MAX_FIELDS, "common.hpp mirrors swmhd_source.h; field_correction_ok sizes its arrays by the relaxation call");

// swmhd_stochastic_coefficients: the draw of one time step (stochastic_coefficients.hip).  Without `ens`: one grid, with `substream`.
template <typename T>
int stochastic_coefficients_common(uint64_t *counter, T *const *coef, const double *const *amp0, const double *const *ktx,
                                   const double *const *kty, const int *nmodes, const int *kind, int ngroups, bool ens, int members,
                                   int64_t coef_sm, int64_t amp_sm, uint64_t seed, uint32_t substream, const uint32_t *substreams, double sdt,
                                   void *stream) {
    if (!counter || (uintptr_t)counter % 8 != 0 || !coef || !amp0 || !nmodes || !kind) return SWMHD_EINVAL;
    if (ngroups < 1 || ngroups > SWMHD_STOCHASTIC_MAX_FIELDS) return SWMHD_EINVAL;
    if (!isfinite(sdt) || !(sdt > 0.0)) return SWMHD_EINVAL;
    if (ens && (members < 1 || members > SWMHD_ENSEMBLE_MAX_MEMBERS || !substreams)) return SWMHD_EINVAL;
    StochasticCoefArgs<T> d;
    for (int g = 0; g < STOCHASTIC_MAX_FIELDS; ++g) {
        d.coef[g] = nullptr; d.amp0[g] = d.ktx[g] = d.kty[g] = nullptr; d.M[g] = 0; d.kind[g] = 0;
    }
    for (int g = 0; g < ngroups; ++g) {
        const int M = nmodes[g];
        if (M < 1 || M > SWMHD_STOCHASTIC_MAX_MODES) return SWMHD_EINVAL;
        if (kind[g] != SWMHD_STOCHASTIC_SCALAR && kind[g] != SWMHD_STOCHASTIC_PAIR) return SWMHD_EINVAL;
        const bool pair = kind[g] == SWMHD_STOCHASTIC_PAIR;
        if (!table_ok(coef[g]) || !table_ok(amp0[g])) return SWMHD_EINVAL;
        if (pair && (!ktx || !kty || !table_ok(ktx[g]) || !table_ok(kty[g]))) return SWMHD_EINVAL;
        if (ens && (coef_sm < (pair ? 4 : 2) * (int64_t)M || (amp_sm != 0 && amp_sm < M))) return SWMHD_EINVAL;
        d.coef[g] = coef[g]; d.amp0[g] = amp0[g]; d.ktx[g] = pair ? ktx[g] : nullptr; d.kty[g] = pair ? kty[g] : nullptr;
        d.M[g] = M; d.kind[g] = kind[g];
    }
    d.counter = reinterpret_cast<unsigned long long *>(counter);
    d.ngroups = ngroups; d.members = ens ? members : 1;
    d.coef_stride_m = ens ? (long)coef_sm : 0; d.amp_stride_m = ens ? (long)amp_sm : 0;
    d.seed_lo = (unsigned)(seed & 0xffffffffull); d.seed_hi = (unsigned)(seed >> 32);
    d.substream = substream; d.substreams = ens ? substreams : nullptr; d.sdt = sdt;
    return hiprc(launch_stochastic_coefficients<T>(d, (hipStream_t)stream));
}

// The RK3 step driver.  Periodic: stages in anchor form (fast) and a periodic fill of whatever the kernel does not wrap.  Bounded
// ensembles (ens->bc, swmhd_ensemble_step_rk3_bc): ShallowWaterModel.time_step's Bounded schedule -- every stage in G- form, then the
// boundary-condition fill of the four fields, gradient values from the DEVICE table bc_gradient.  ph: the model and dt.
template <typename T>
int step_common(T *const *q, T *const *q_alt, T *const *Ga, T *const *Gb, const Grid &g, const Physics<T> &ph, int nsteps, int flags,
                int *state_in_alt, void *stream, const Ens *ens = nullptr, const T *bc_gradient = nullptr) {
    const bool bc = ens && ens->bc;
    if (const int rc = ens_check(ens, g, flags)) return rc;
    if (!q || !q_alt || !Ga || !Gb || nsteps < 0) return SWMHD_EINVAL;
    const Flags fl = decode_flags(flags);
    if (!bc && fl.bounded()) return SWMHD_ENOTSUP;   // the periodic driver's halo fill is the periodic one
    if (bc && !fl.bounded()) return SWMHD_EINVAL;    // periodic grids have the periodic driver
    if (bounded_wrap_conflict(flags)) return SWMHD_EINVAL;
    Rk3Buffers<T> b;
    if (!b.set(q, q_alt, Ga, Gb)) return SWMHD_EINVAL;
    const BcSides sides{fl.topo_x, fl.topo_y, FACE_X, FACE_Y};
    if (bc) {   // the fill's own checks, before the first launch
        HaloBc<T> a;
        if (const int rc = halo_bc_args<T>(a, b.cur, 4, g, sides, ens)) return rc;
    }
    const bool anchor = !fl.strict && !bc;   // (common.hpp: Rk3Buffers)
    const int need = (SWMHD_HALO_X | SWMHD_HALO_Y) & ~fl.wrap;   // whatever the kernel does not wrap itself (SWMHD_HALO_* = the wrap bits)
    Physics<T> st = ph;
    for (int n = 0; n < nsteps; ++n)
        for (int k = 0; k < 3; ++k) {
            const Rk3Stage<T> sg = b.stage(k, anchor);
            st.gamma = sg.gamma; st.zeta = sg.zeta; st.store_G = sg.store_G;
            int rc = tendencies_rk3<T>(b.cur, b.alt, b.gn, sg.Gm, g, st, Rows{0, g.Ny}, flags | sg.flags, stream, ens);
            if (rc) return rc;
            b.rotate();
            if (bc) rc = halo_bc_common<T>(b.cur, 4, g, sides, bc_gradient, stream, ens);
            else if (need) rc = fill_halo_periodic_multi<T>(b.cur, 4, g, need, stream, ens);
            if (rc) return rc;
        }
    if (state_in_alt) *state_in_alt = b.swaps & 1;
    return SWMHD_OK;
}
static_assert(SWMHD_HALO_X == 1 && SWMHD_HALO_Y == 2, "step_common takes Flags::wrap for the directions a fill may skip");

// q = (u|uh, v|vh, h, A); of ph: grav (not read where the ensemble's table holds it) and the formulation
template <typename T>
int diag_common(const T *const *q, const Grid &g, const Physics<T> &ph, T href, const Rows &r, double *ws, double *out, void *stream,
                const Ens *ens = nullptr) {
    if (const int rc = ens_check(ens, g, 0)) return rc;
    if (!q[0] || !q[1] || !q[2] || !q[3] || !ws || !out) return SWMHD_EINVAL;
    if (!g.extents_ok() || !g.spacing_ok() || !g.rows_ok(r.j0, r.j1) || !formulation_ok(ph.formulation)) return SWMHD_EINVAL;
    if (!g.halo_at_least(1)) return SWMHD_EHALO;
    return hiprc(launch_diagnostics<T>(g.interior(q[0]), g.interior(q[1]), g.interior(q[2]), g.interior(q[3]), g.Nx, g.Ny, r.j0, r.j1,
                                       (long)g.sy, T(g.dx), T(g.dy), ph.grav, href, ph.formulation, ws, out, (hipStream_t)stream, ens ? ens->members : 0,
                                       ens ? (long)ens->stride_m : 0, ens && ens->par ? static_cast<const T *>(ens->params) : nullptr));
}

}  // namespace

// the three that the slab driver shares (api_args.hpp)
template <typename T>
int swmhd::fill_halo_periodic_multi(T *const *f, int nf, const Grid &g, int which, void *stream, const Ens *ens) {
    if (const int rc = ens_check(ens, g, 0)) return rc;
    if (!f || nf < 1 || nf > 4 || !g.extents_ok()) return SWMHD_EINVAL;
    if (!g.period_covers_halo(3)) return SWMHD_EHALO;
    if (which & ~(SWMHD_HALO_X | SWMHD_HALO_Y)) return SWMHD_EINVAL;
    T *p[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int k = 0; k < nf; ++k) {
        if (!f[k]) return SWMHD_EINVAL;
        p[k] = g.interior(f[k]);
    }
    return hiprc(launch_fill_halo_periodic_multi<T>(p, nf, g.Nx, g.Ny, g.Hx, g.Hy, (long)g.sy, which, (hipStream_t)stream,
                                                    ens ? ens->members : 0, ens ? (long)ens->stride_m : 0));
}

template <typename T>
int swmhd::fill_halo_walls(T *const *f, int nf, const Grid &g, BcSides s, int walls_y, const T *gradient, const T *gtab, void *stream) {
    if (walls_y & ~3) return SWMHD_EINVAL;
    HaloBcEns<T> a;
    s.topo_y = SWMHD_BOUNDED;
    if (const int rc = halo_bc_args<T>(a, f, nf, g, s)) return rc;
    a.topo_y = SWMHD_BOUNDED | ((walls_y & 1) ? 0 : TOPO_OPEN_SOUTH) | ((walls_y & 2) ? 0 : TOPO_OPEN_NORTH);
    host_gradient<T>(a, gradient);
    if (!gtab) return hiprc(launch_fill_halo_bc<T>(a, (hipStream_t)stream));
    a.stride_m = 0; a.members = 1; a.gtab = gtab;   // (the ensemble fill of one member reads its values from the device table)
    return hiprc(launch_fill_halo_bc_ensemble<T>(a, (hipStream_t)stream));
}

template <typename T>
int swmhd::tendencies_rk3(const T *const *q, T *const *qnew, T *const *Gn, const T *const *Gm, const Grid &g, const Physics<T> &ph,
                          const Rows &r, int flags, void *stream, const Ens *ens) {
    if (const int rc = ens_check(ens, g, flags)) return rc;
    if (!q || !qnew || !Gn) return SWMHD_EINVAL;
    for (int f = 0; f < 4; ++f) {
        if (!q[f] || !qnew[f] || !Gn[f] || (Gm && !Gm[f])) return SWMHD_EINVAL;
        for (int k = 0; k < 4; ++k)
            if (qnew[f] == q[k]) return SWMHD_EINVAL;   // the new state must not alias the state being read through halos
    }
    return tend_common<T>(q, Gn, g, ph, r, flags, stream, qnew, Gm, ens);
}

namespace swmhd {
static_assert(GM_IS_PREV_STATE == SWMHD_GM_IS_PREV_STATE, "common.hpp mirrors swmhd.h");
static_assert(RK3_ANCHOR == SWMHD_RK3_ANCHOR, "common.hpp mirrors swmhd.h");
static_assert(ENS_NPARAMS == SWMHD_ENSEMBLE_NPARAMS, "common.hpp mirrors swmhd.h");
static_assert(MAX_TRACERS == SWMHD_MAX_TRACERS, "common.hpp mirrors swmhd.h");
#define SW_INST(T)                                                                                                                  \
    template int tendencies_rk3<T>(const T *const *, T *const *, T *const *, const T *const *, const Grid &, const Physics<T> &,      \
                                   const Rows &, int, void *, const Ens *);                                                         \
    template int fill_halo_periodic_multi<T>(T *const *, int, const Grid &, int, void *, const Ens *);                              \
    template int fill_halo_walls<T>(T *const *, int, const Grid &, BcSides, int, const T *, const T *, void *);
SW_INST(double)
SW_INST(float)
#undef SW_INST
}  // namespace swmhd

extern "C" {

int swmhd_version(void) { return SWMHD_VERSION; }

const char *swmhd_strerror(int rc) {
    switch (rc) {
        case SWMHD_OK: return "success";
        case SWMHD_EINVAL: return "invalid argument (null pointer, bad extents, stride, spacing, row range or flags)";
        case SWMHD_EHALO: return "halo too small for the operator's stencil (Jacobian form needs 2, divergence form 3)";
        case SWMHD_ENOTSUP: return "not supported by this build (or: the RCCL library could not be loaded)";
        case SWMHD_ECOMM: return "RCCL reported an error (swmhd_ring_last_error has its text)";
        default: return rc < 0 ? hipGetErrorString((hipError_t)(-rc)) : "unknown swmhd error";
    }
}

int swmhd_event_create(void **event) {
    if (!event) return SWMHD_EINVAL;
    hipEvent_t e;
    const hipError_t rc = hipEventCreateWithFlags(&e, hipEventDisableSystemFence);
    if (rc != hipSuccess) return hiprc(rc);
    *event = (void *)e;
    return SWMHD_OK;
}
int swmhd_event_record(void *event, void *stream) {
    return event ? hiprc(hipEventRecord((hipEvent_t)event, (hipStream_t)stream)) : SWMHD_EINVAL;
}
int swmhd_event_elapsed_ms(void *start, void *stop, float *ms) {
    if (!start || !stop || !ms) return SWMHD_EINVAL;
    const hipError_t rc = hipEventSynchronize((hipEvent_t)stop);
    if (rc != hipSuccess) return hiprc(rc);
    return hiprc(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
}
int swmhd_event_destroy(void *event) { return event ? hiprc(hipEventDestroy((hipEvent_t)event)) : SWMHD_OK; }

int swmhd_tendency_launch_geometry(int Nx, int rows, int formulation, int elem_size, int flags, int out[8]) {
    if (!out || Nx <= 0 || rows <= 0 || (elem_size != 4 && elem_size != 8)) return SWMHD_EINVAL;
    if (!formulation_ok(formulation)) return SWMHD_EINVAL;
    const Flags fl = decode_flags(flags);
    return tendency_launch_geometry(Nx, rows, formulation, elem_size, fl.strict, fl.kernel_variant, fl.leave_room, fl.wrap, out);
}

int swmhd_ensemble_launch_geometry(int Nx, int Ny, int formulation, int elem_size, int flags, int members, int out[8]) {
    if (!out || Nx <= 0 || Ny <= 0 || (elem_size != 4 && elem_size != 8)) return SWMHD_EINVAL;
    if (!formulation_ok(formulation) || members < 1 || members > SWMHD_ENSEMBLE_MAX_MEMBERS) return SWMHD_EINVAL;
    if ((flags & ~(ENS_FLAGS | BOUNDED_FLAGS)) || bounded_wrap_conflict(flags)) return SWMHD_EINVAL;
    const Flags fl = decode_flags(flags);
    return ensemble_launch_geometry(Nx, Ny, formulation, elem_size, fl.strict, fl.wrap, fl.topo_x, fl.topo_y, members, out) ? SWMHD_EINVAL : SWMHD_OK;
}

// The exported wrappers: each packs its C scalars into a Grid, a Physics (stage scalars by name; the *_params calls leave out what
// their table holds) and, for ensembles, an Ens, and makes one call.
#define SWMHD_DEF_API(sfx, T)                                                                                                                         \
    int swmhd_lorentz_jacobian_##sfx(const T *A, const T *h, T *Fx, T *Fy, int Nx, int Ny, int Hx, int Hy, int64_t sy, T dx, T dy, int flags,         \
                                     void *stream) {                                                                                                  \
        return lorentz_common<T>(false, A, h, Fx, Fy, Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, Rows{0, Ny}, flags, stream);                                  \
    }                                                                                                                                                 \
    int swmhd_lorentz_jacobian_rows_##sfx(const T *A, const T *h, T *Fx, T *Fy, int Nx, int Ny, int Hx, int Hy, int64_t sy, T dx, T dy, int j0,       \
                                          int j1, int flags, void *stream) {                                                                          \
        return lorentz_common<T>(false, A, h, Fx, Fy, Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, Rows{j0, j1}, flags, stream);                                 \
    }                                                                                                                                                 \
    int swmhd_lorentz_divergence_##sfx(const T *A, const T *h, T *Fx, T *Fy, int Nx, int Ny, int Hx, int Hy, int64_t sy, T dx, T dy, int flags,       \
                                       void *stream) {                                                                                                \
        return lorentz_common<T>(true, A, h, Fx, Fy, Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, Rows{0, Ny}, flags, stream);                                   \
    }                                                                                                                                                 \
    int swmhd_lorentz_divergence_rows_##sfx(const T *A, const T *h, T *Fx, T *Fy, int Nx, int Ny, int Hx, int Hy, int64_t sy, T dx, T dy, int tx,     \
                                            int ty, int j0, int j1, int flags, void *stream) {                                                        \
        return lorentz_common<T>(true, A, h, Fx, Fy, Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, Rows{j0, j1}, flags, stream, tx, ty);                          \
    }                                                                                                                                                 \
    int swmhd_fill_halo_periodic_##sfx(T *f, int Nx, int Ny, int Hx, int Hy, int64_t sy, int which, void *stream) {                                   \
        return halo_common<T>(f, Grid{Nx, Ny, Hx, Hy, sy}, which, stream);                                                                            \
    }                                                                                                                                                 \
    int swmhd_fill_halo_##sfx(T *const *f, int nf, int Nx, int Ny, int Hx, int Hy, int64_t sy, int topo_x, int topo_y, int face_x, int face_y,        \
                              const T *gradient, T dx, T dy, void *stream) {                                                                          \
        return halo_bc_common<T>(f, nf, Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, BcSides{topo_x, topo_y, face_x, face_y}, gradient, stream);                 \
    }                                                                                                                                                 \
    int swmhd_fill_halo_walls_##sfx(T *const *f, int nf, int Nx, int Ny, int Hx, int Hy, int64_t sy, int topo_x, int walls_y, int face_x, int face_y, \
                                    const T *gradient, T dx, T dy, void *stream) {                                                                    \
        return fill_halo_walls<T>(f, nf, Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, BcSides{topo_x, SWMHD_BOUNDED, face_x, face_y}, walls_y,                   \
                                    gradient, nullptr, stream);                                                                                       \
    }                                                                                                                                                 \
    int swmhd_fill_halo_periodic_multi_##sfx(T *const *f, int nf, int Nx, int Ny, int Hx, int Hy, int64_t sy, int which, void *stream) {              \
        return fill_halo_periodic_multi<T>(f, nf, Grid{Nx, Ny, Hx, Hy, sy}, which, stream);                                                           \
    }                                                                                                                                                 \
    int swmhd_tendencies_##sfx(const T *q1, const T *q2, const T *h, const T *A, T *G1, T *G2, T *Gh, T *GA, int Nx, int Ny, int Hx, int Hy,          \
                               int64_t sy, T dx, T dy, T g, T f, int formulation, int lorentz, int j0, int j1, int flags, void *stream) {             \
        const T *const q[4] = {q1, q2, h, A};                                                                                                         \
        T *const G[4] = {G1, G2, Gh, GA};                                                                                                             \
        return tend_common<T>(q, G, Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, Physics<T>{g, f, formulation, lorentz}, Rows{j0, j1}, flags, stream);           \
    }                                                                                                                                                 \
    int swmhd_tendencies_rk3_##sfx(const T *const *q, T *const *qnew, T *const *Gn, const T *const *Gm, int Nx, int Ny, int Hx, int Hy, int64_t sy,   \
                                   T dx, T dy, T g, T f, int formulation, int lorentz, T dt, T gamma, T zeta, int store_G, int j0, int j1, int flags, \
                                   void *stream) {                                                                                                    \
        Physics<T> ph{g, f, formulation, lorentz}; ph.dt = dt; ph.gamma = gamma; ph.zeta = zeta; ph.store_G = store_G;                                \
        return tendencies_rk3<T>(q, qnew, Gn, Gm, Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, ph, Rows{j0, j1}, flags, stream);                                 \
    }                                                                                                                                                 \
    int swmhd_tracers_rk3_##sfx(const T *q1, const T *q2, const T *h, const T *const *c, T *const *cnew, T *const *Gn, const T *const *Gm,            \
                                int ntracers, int Nx, int Ny, int Hx, int Hy, int64_t sy, T dx, T dy, int formulation, T dt, T gamma, T zeta,         \
                                int store_G, int j0, int j1, int flags, void *stream) {                                                               \
        const T *const q[3] = {q1, q2, h};                                                                                                            \
        Physics<T> ph; ph.formulation = formulation; ph.dt = dt; ph.gamma = gamma; ph.zeta = zeta; ph.store_G = store_G;                              \
        return tracers_common<T>(q, c, cnew, Gn, Gm, ntracers, Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, ph, Rows{j0, j1}, flags, stream);                    \
    }                                                                                                                                                 \
    int swmhd_ensemble_tracers_rk3_##sfx(const T *q1, const T *q2, const T *h, const T *const *c, T *const *cnew, T *const *Gn, const T *const *Gm,   \
                                         int ntracers, int members, int64_t stride_m, int Nx, int Ny, int Hx, int Hy, int64_t sy, T dx, T dy,         \
                                         int formulation, T dt, T gamma, T zeta, int store_G, int flags, void *stream) {                              \
        const T *const q[3] = {q1, q2, h};                                                                                                            \
        const Ens e{members, stride_m};                                                                                                               \
        Physics<T> ph; ph.formulation = formulation; ph.dt = dt; ph.gamma = gamma; ph.zeta = zeta; ph.store_G = store_G;                              \
        return tracers_common<T>(q, c, cnew, Gn, Gm, ntracers, Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, ph, Rows{0, Ny}, flags, stream, &e);                 \
    }                                                                                                                                                 \
    int swmhd_ensemble_tracers_rk3_params_##sfx(const T *q1, const T *q2, const T *h, const T *const *c, T *const *cnew, T *const *Gn,                \
                                                const T *const *Gm, int ntracers, int members, int64_t stride_m, int Nx, int Ny, int Hx, int Hy,      \
                                                int64_t sy, T dx, T dy, int formulation, const T *params, T gamma, T zeta, int store_G, int flags,    \
                                                void *stream) {                                                                                       \
        const T *const q[3] = {q1, q2, h};                                                                                                            \
        const Ens e{members, stride_m, false, true, params};                                                                                          \
        Physics<T> ph; ph.formulation = formulation; ph.gamma = gamma; ph.zeta = zeta; ph.store_G = store_G;                                          \
        return tracers_common<T>(q, c, cnew, Gn, Gm, ntracers, Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, ph, Rows{0, Ny}, flags, stream, &e);                 \
    }                                                                                                                                                 \
    int swmhd_diagnostics_##sfx(const T *q1, const T *q2, const T *h, const T *A, int Nx, int Ny, int Hx, int Hy, int64_t sy, T dx, T dy, T g,        \
                                T href, int form, int j0, int j1, double *ws, double *out, void *stream) {                                            \
        const T *const q[4] = {q1, q2, h, A};                                                                                                         \
        Physics<T> ph; ph.grav = g; ph.formulation = form;                                                                                            \
        return diag_common<T>(q, Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, ph, href, Rows{j0, j1}, ws, out, stream);                                          \
    }                                                                                                                                                 \
    int swmhd_step_rk3_##sfx(T *const *q, T *const *q_alt, T *const *Ga, T *const *Gb, int Nx, int Ny, int Hx, int Hy, int64_t sy, T dx, T dy, T g,   \
                             T f, int formulation, int lorentz, T dt, int nsteps, int flags, int *state_in_alt, void *stream) {                       \
        Physics<T> ph{g, f, formulation, lorentz}; ph.dt = dt;                                                                                        \
        return step_common<T>(q, q_alt, Ga, Gb, Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, ph, nsteps, flags, state_in_alt, stream);                           \
    }                                                                                                                                                 \
    int swmhd_rk3_substep_##sfx(T *const *U, const T *const *Gn, const T *const *Gm, int Nx, int Ny, int Hx, int Hy, int64_t sy, T dt, T gamma,       \
                                T zeta, int j0, int j1, int flags, void *stream) {                                                                    \
        Physics<T> ph; ph.dt = dt; ph.gamma = gamma; ph.zeta = zeta;                                                                                  \
        return rk3_common<T>(U, Gn, Gm, Grid{Nx, Ny, Hx, Hy, sy}, ph, Rows{j0, j1}, flags, stream);                                                   \
    }                                                                                                                                                 \
    int swmhd_ensemble_tendencies_rk3_##sfx(const T *const *q, T *const *qnew, T *const *Gn, const T *const *Gm, int members, int64_t stride_m,       \
                                            int Nx, int Ny, int Hx, int Hy, int64_t sy, T dx, T dy, T g, T f, int formulation, int lorentz, T dt,     \
                                            T gamma, T zeta, int store_G, int flags, void *stream) {                                                  \
        const Ens e{members, stride_m};                                                                                                               \
        Physics<T> ph{g, f, formulation, lorentz}; ph.dt = dt; ph.gamma = gamma; ph.zeta = zeta; ph.store_G = store_G;                                \
        return tendencies_rk3<T>(q, qnew, Gn, Gm, Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, ph, Rows{0, Ny}, flags, stream, &e);                              \
    }                                                                                                                                                 \
    int swmhd_ensemble_step_rk3_##sfx(T *const *q, T *const *q_alt, T *const *Ga, T *const *Gb, int members, int64_t stride_m, int Nx, int Ny,        \
                                      int Hx, int Hy, int64_t sy, T dx, T dy, T g, T f, int formulation, int lorentz, T dt, int nsteps, int flags,    \
                                      int *state_in_alt, void *stream) {                                                                              \
        const Ens e{members, stride_m};                                                                                                               \
        Physics<T> ph{g, f, formulation, lorentz}; ph.dt = dt;                                                                                        \
        return step_common<T>(q, q_alt, Ga, Gb, Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, ph, nsteps, flags, state_in_alt, stream, &e);                       \
    }                                                                                                                                                 \
    int swmhd_ensemble_fill_halo_periodic_##sfx(T *const *f, int nf, int members, int64_t stride_m, int Nx, int Ny, int Hx, int Hy, int64_t sy,       \
                                                int which, void *stream) {                                                                            \
        const Ens e{members, stride_m};                                                                                                               \
        return fill_halo_periodic_multi<T>(f, nf, Grid{Nx, Ny, Hx, Hy, sy}, which, stream, &e);                                                       \
    }                                                                                                                                                 \
    int swmhd_ensemble_diagnostics_##sfx(const T *q1, const T *q2, const T *h, const T *A, int members, int64_t stride_m, int Nx, int Ny, int Hx,     \
                                         int Hy, int64_t sy, T dx, T dy, T g, T href, int form, double *ws, double *out, void *stream) {              \
        const T *const q[4] = {q1, q2, h, A};                                                                                                         \
        const Ens e{members, stride_m};                                                                                                               \
        Physics<T> ph; ph.grav = g; ph.formulation = form;                                                                                            \
        return diag_common<T>(q, Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, ph, href, Rows{0, Ny}, ws, out, stream, &e);                                       \
    }                                                                                                                                                 \
    int swmhd_ensemble_fill_halo_##sfx(T *const *f, int nf, int members, int64_t stride_m, int Nx, int Ny, int Hx, int Hy, int64_t sy, int topo_x,    \
                                       int topo_y, int face_x, int face_y, const T *gradient, T dx, T dy, void *stream) {                             \
        const Ens e{members, stride_m, true};                                                                                                         \
        return halo_bc_common<T>(f, nf, Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, BcSides{topo_x, topo_y, face_x, face_y}, gradient, stream, &e);             \
    }                                                                                                                                                 \
    int swmhd_ensemble_step_rk3_bc_##sfx(T *const *q, T *const *q_alt, T *const *Ga, T *const *Gb, int members, int64_t stride_m, int Nx, int Ny,     \
                                         int Hx, int Hy, int64_t sy, T dx, T dy, T g, T f, int formulation, int lorentz, T dt, int nsteps,            \
                                         const T *gradient, int flags, int *state_in_alt, void *stream) {                                             \
        const Ens e{members, stride_m, true};                                                                                                         \
        Physics<T> ph{g, f, formulation, lorentz}; ph.dt = dt;                                                                                        \
        return step_common<T>(q, q_alt, Ga, Gb, Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, ph, nsteps, flags, state_in_alt, stream, &e, gradient);             \
    }                                                                                                                                                 \
    int swmhd_ensemble_tendencies_rk3_params_##sfx(const T *const *q, T *const *qnew, T *const *Gn, const T *const *Gm, int members,                  \
                                                   int64_t stride_m, int Nx, int Ny, int Hx, int Hy, int64_t sy, T dx, T dy, const T *params,         \
                                                   int formulation, int lorentz, T gamma, T zeta, int store_G, int flags, void *stream) {             \
        const Ens e{members, stride_m, false, true, params};                                                                                          \
        Physics<T> ph; ph.formulation = formulation; ph.lorentz = lorentz; ph.gamma = gamma; ph.zeta = zeta; ph.store_G = store_G;                    \
        return tendencies_rk3<T>(q, qnew, Gn, Gm, Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, ph, Rows{0, Ny}, flags, stream, &e);                              \
    }                                                                                                                                                 \
    int swmhd_ensemble_step_rk3_params_##sfx(T *const *q, T *const *q_alt, T *const *Ga, T *const *Gb, int members, int64_t stride_m, int Nx, int Ny, \
                                             int Hx, int Hy, int64_t sy, T dx, T dy, const T *params, int formulation, int lorentz, int nsteps,       \
                                             int flags, int *state_in_alt, void *stream) {                                                            \
        const Ens e{members, stride_m, false, true, params};                                                                                          \
        Physics<T> ph; ph.formulation = formulation; ph.lorentz = lorentz;                                                                            \
        return step_common<T>(q, q_alt, Ga, Gb, Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, ph, nsteps, flags, state_in_alt, stream, &e);                       \
    }                                                                                                                                                 \
    int swmhd_ensemble_step_rk3_bc_params_##sfx(T *const *q, T *const *q_alt, T *const *Ga, T *const *Gb, int members, int64_t stride_m, int Nx,      \
                                                int Ny, int Hx, int Hy, int64_t sy, T dx, T dy, const T *params, int formulation, int lorentz,        \
                                                int nsteps, const T *gradient, int flags, int *state_in_alt, void *stream) {                          \
        const Ens e{members, stride_m, true, true, params};                                                                                           \
        Physics<T> ph; ph.formulation = formulation; ph.lorentz = lorentz;                                                                            \
        return step_common<T>(q, q_alt, Ga, Gb, Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, ph, nsteps, flags, state_in_alt, stream, &e, gradient);             \
    }                                                                                                                                                 \
    int swmhd_ensemble_diagnostics_params_##sfx(const T *q1, const T *q2, const T *h, const T *A, int members, int64_t stride_m, int Nx, int Ny,      \
                                                int Hx, int Hy, int64_t sy, T dx, T dy, const T *params, T href, int form, double *ws, double *out,   \
                                                void *stream) {                                                                                       \
        const T *const q[4] = {q1, q2, h, A};                                                                                                         \
        const Ens e{members, stride_m, false, true, params};                                                                                          \
        Physics<T> ph; ph.formulation = form;                                                                                                         \
        return diag_common<T>(q, Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, ph, href, Rows{0, Ny}, ws, out, stream, &e);                                       \
    }

SWMHD_DEF_API(f64, double)
SWMHD_DEF_API(f32, float)

// include/swmhd_diffusion.h
#define SWMHD_DEF_DIFFUSION(sfx, T)                                                                                                                    \
    int swmhd_diffusion_rk3_##sfx(const T *const *old, T *const *nw, T *const *acc, const T *coef, int nfields, int Nx, int Ny, int Hx, int Hy,       \
                                  int64_t sy, T dx, T dy, T a, T w, int j0, int j1, int flags, void *stream) {                                        \
        return diffusion_common<T>(old, nw, acc, coef, nfields, Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, a, w, Rows{j0, j1}, flags, stream);                 \
    }                                                                                                                                                 \
    int swmhd_ensemble_diffusion_rk3_##sfx(const T *const *old, T *const *nw, T *const *acc, const T *coef, int nfields, int members,                 \
                                           int64_t stride_m, int Nx, int Ny, int Hx, int Hy, int64_t sy, T dx, T dy, const T *params, T a, T w,       \
                                           int j0, int j1, int flags, void *stream) {                                                                 \
        const Ens e{members, stride_m, false, params != nullptr, params};                                                                             \
        return diffusion_common<T>(old, nw, acc, coef, nfields, Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, a, w, Rows{j0, j1}, flags, stream, &e);             \
    }

SWMHD_DEF_DIFFUSION(f64, double)
SWMHD_DEF_DIFFUSION(f32, float)

// include/swmhd_biharmonic.h
#define SWMHD_DEF_BIHARMONIC(sfx, T)                                                                                                                   \
    int swmhd_biharmonic_rk3_##sfx(const T *const *old, T *const *nw, T *const *acc, const T *coef, int nfields, int Nx, int Ny, int Hx, int Hy,      \
                                   int64_t sy, T dx, T dy, T a, T w, int j0, int j1, int flags, void *stream) {                                       \
        return biharmonic_common<T>(old, nw, acc, coef, nfields, Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, a, w, Rows{j0, j1}, flags, stream);                \
    }                                                                                                                                                 \
    int swmhd_ensemble_biharmonic_rk3_##sfx(const T *const *old, T *const *nw, T *const *acc, const T *coef, int nfields, int members,                \
                                            int64_t stride_m, int Nx, int Ny, int Hx, int Hy, int64_t sy, T dx, T dy, const T *params, T a, T w,      \
                                            int j0, int j1, int flags, void *stream) {                                                                \
        const Ens e{members, stride_m, false, params != nullptr, params};                                                                             \
        return biharmonic_common<T>(old, nw, acc, coef, nfields, Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, a, w, Rows{j0, j1}, flags, stream, &e);            \
    }

SWMHD_DEF_BIHARMONIC(f64, double)
SWMHD_DEF_BIHARMONIC(f32, float)

// include/swmhd_coriolis.h
#define SWMHD_DEF_CORIOLIS(sfx, T)                                                                                                                     \
    int swmhd_coriolis_rk3_##sfx(const T *q1, const T *q2, T *n1, T *n2, T *a1, T *a2, const T *frow, int Nx, int Ny, int Hx, int Hy, int64_t sy,     \
                                 T a, T w, int j0, int j1, int flags, void *stream) {                                                                 \
        return coriolis_common<T>(q1, q2, n1, n2, a1, a2, frow, Grid{Nx, Ny, Hx, Hy, sy}, a, w, Rows{j0, j1}, flags, stream);                         \
    }                                                                                                                                                 \
    int swmhd_ensemble_coriolis_rk3_##sfx(const T *q1, const T *q2, T *n1, T *n2, T *a1, T *a2, const T *frow, int members, int64_t stride_m,         \
                                          int Nx, int Ny, int Hx, int Hy, int64_t sy, const T *params, T a, T w, int j0, int j1, int flags,           \
                                          void *stream) {                                                                                             \
        const Ens e{members, stride_m, false, params != nullptr, params};                                                                             \
        return coriolis_common<T>(q1, q2, n1, n2, a1, a2, frow, Grid{Nx, Ny, Hx, Hy, sy}, a, w, Rows{j0, j1}, flags, stream, &e);                     \
    }

SWMHD_DEF_CORIOLIS(f64, double)
SWMHD_DEF_CORIOLIS(f32, float)

// include/swmhd_relaxation.h
#define SWMHD_DEF_RELAXATION(sfx, T)                                                                                                                   \
    int swmhd_relaxation_rk3_##sfx(const T *const *old, T *const *nw, T *const *acc, const T *const *mask, const T *const *target, const T *rate,     \
                                   const T *tval, int nfields, int Nx, int Ny, int Hx, int Hy, int64_t sy, T a, T w, int j0, int j1, int flags,       \
                                   void *stream) {                                                                                                    \
        return relaxation_common<T>(old, nw, acc, mask, target, rate, tval, nfields, Grid{Nx, Ny, Hx, Hy, sy}, a, w, Rows{j0, j1}, flags, stream);    \
    }                                                                                                                                                 \
    int swmhd_ensemble_relaxation_rk3_##sfx(const T *const *old, T *const *nw, T *const *acc, const T *const *mask, const T *const *target,           \
                                            const T *rate, const T *tval, int nfields, int members, int64_t stride_m, int64_t mask_stride_m,          \
                                            int64_t target_stride_m, int Nx, int Ny, int Hx, int Hy, int64_t sy, const T *params, T a, T w, int j0,   \
                                            int j1, int flags, void *stream) {                                                                        \
        const Ens e{members, stride_m, false, params != nullptr, params};                                                                             \
        return relaxation_common<T>(old, nw, acc, mask, target, rate, tval, nfields, Grid{Nx, Ny, Hx, Hy, sy}, a, w, Rows{j0, j1}, flags, stream,     \
                                    &e, mask_stride_m, target_stride_m);                                                                              \
    }

SWMHD_DEF_RELAXATION(f64, double)
SWMHD_DEF_RELAXATION(f32, float)

// include/swmhd_stochastic.h
#define SWMHD_DEF_STOCHASTIC(sfx, T)                                                                                                                   \
    int swmhd_stochastic_coefficients_##sfx(uint64_t *counter, T *const *coef, const double *const *amp0, const double *const *ktx,                   \
                                            const double *const *kty, const int *nmodes, const int *kind, int ngroups, uint64_t seed,                 \
                                            uint32_t substream, double sdt, void *stream) {                                                           \
        return stochastic_coefficients_common<T>(counter, coef, amp0, ktx, kty, nmodes, kind, ngroups, false, 0, 0, 0, seed, substream, nullptr,      \
                                                 sdt, stream);                                                                                        \
    }                                                                                                                                                 \
    int swmhd_ensemble_stochastic_coefficients_##sfx(uint64_t *counter, T *const *coef, const double *const *amp0, const double *const *ktx,          \
                                                     const double *const *kty, const int *nmodes, const int *kind, int ngroups, int members,          \
                                                     int64_t coef_stride_m, int64_t amp_stride_m, uint64_t seed, const uint32_t *substream,           \
                                                     double sdt, void *stream) {                                                                      \
        return stochastic_coefficients_common<T>(counter, coef, amp0, ktx, kty, nmodes, kind, ngroups, true, members, coef_stride_m, amp_stride_m,    \
                                                 seed, 0, substream, sdt, stream);                                                                    \
    }                                                                                                                                                 \
    int swmhd_stochastic_rk3_##sfx(const T *const *old, T *const *nw, T *const *acc, const T *const *coef, const T *const *xtab,                      \
                                   const T *const *ytab, const int *nmodes, int nfields, int64_t xp, int64_t yp, int Nx, int Ny, int Hx, int Hy,      \
                                   int64_t sy, T a, T w, int j0, int j1, int flags, void *stream) {                                                   \
        return stochastic_common<T>(old, nw, acc, coef, xtab, ytab, nmodes, nfields, xp, yp, Grid{Nx, Ny, Hx, Hy, sy}, a, w, Rows{j0, j1}, flags,     \
                                    stream);                                                                                                          \
    }                                                                                                                                                 \
    int swmhd_ensemble_stochastic_rk3_##sfx(const T *const *old, T *const *nw, T *const *acc, const T *const *coef, const T *const *xtab,             \
                                            const T *const *ytab, const int *nmodes, int nfields, int64_t xp, int64_t yp, int members,                \
                                            int64_t stride_m, int64_t coef_stride_m, int Nx, int Ny, int Hx, int Hy, int64_t sy, const T *params,     \
                                            T a, T w, int j0, int j1, int flags, void *stream) {                                                      \
        const Ens e{members, stride_m, false, params != nullptr, params};                                                                             \
        return stochastic_common<T>(old, nw, acc, coef, xtab, ytab, nmodes, nfields, xp, yp, Grid{Nx, Ny, Hx, Hy, sy}, a, w, Rows{j0, j1}, flags,     \
                                    stream, &e, coef_stride_m);                                                                                       \
    }

SWMHD_DEF_STOCHASTIC(f64, double)
SWMHD_DEF_STOCHASTIC(f32, float)

// include/swmhd_source.h
#define SWMHD_DEF_SOURCE(sfx, T)                                                                                                                       \
    int swmhd_source_rk3_##sfx(const T *const *old, T *const *nw, T *const *acc, const T *const *source, const int *kind, int nfields,                \
                               int thickness, int Nx, int Ny, int Hx, int Hy, int64_t sy, T a, T w, int j0, int j1, int flags, void *stream) {        \
        return source_common<T>(old, nw, acc, source, kind, nfields, thickness, Grid{Nx, Ny, Hx, Hy, sy}, a, w, Rows{j0, j1}, flags, stream);         \
    }                                                                                                                                                 \
    int swmhd_ensemble_source_rk3_##sfx(const T *const *old, T *const *nw, T *const *acc, const T *const *source, const int *kind, int nfields,       \
                                        int thickness, int members, int64_t stride_m, int64_t source_stride_m, int Nx, int Ny, int Hx, int Hy,        \
                                        int64_t sy, const T *params, T a, T w, int j0, int j1, int flags, void *stream) {                             \
        const Ens e{members, stride_m, false, params != nullptr, params};                                                                             \
        return source_common<T>(old, nw, acc, source, kind, nfields, thickness, Grid{Nx, Ny, Hx, Hy, sy}, a, w, Rows{j0, j1}, flags, stream, &e,      \
                                source_stride_m);                                                                                                     \
    }

SWMHD_DEF_SOURCE(f64, double)
SWMHD_DEF_SOURCE(f32, float)

// include/swmhd_particles.h
#define SWMHD_DEF_PARTICLES(sfx, T)                                                                                                                    \
    int swmhd_particles_rk3_##sfx(const T *q1, const T *q2, const T *h, double *x, double *y, double *gx, double *gy, int64_t P, int Nx, int Ny,      \
                                  int Hx, int Hy, int64_t sy, double x0, double y0, double dx, double dy, int form, double dt, double gamma,          \
                                  double zeta, int flags, void *stream) {                                                                             \
        return particles_common<T>(q1, q2, h, x, y, gx, gy, P, Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, x0, y0, form, dt, gamma, zeta, flags, stream);       \
    }                                                                                                                                                 \
    int swmhd_ensemble_particles_rk3_##sfx(const T *q1, const T *q2, const T *h, double *x, double *y, double *gx, double *gy, int64_t P,             \
                                           int members, int64_t stride_m, int Nx, int Ny, int Hx, int Hy, int64_t sy, double x0, double y0,           \
                                           double dx, double dy, int form, const T *params, double dt, double gamma, double zeta, int flags,          \
                                           void *stream) {                                                                                            \
        const Ens e{members, stride_m, false, params != nullptr, params};                                                                             \
        return particles_common<T>(q1, q2, h, x, y, gx, gy, P, Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, x0, y0, form, dt, gamma, zeta, flags, stream, &e);   \
    }                                                                                                                                                 \
    int swmhd_particles_sample_##sfx(const T *const *fields, const int *loc, int nfields, const double *x, const double *y, double *out, int64_t P,   \
                                     int Nx, int Ny, int Hx, int Hy, int64_t sy, double x0, double y0, double dx, double dy, int flags,               \
                                     void *stream) {                                                                                                  \
        return particles_sample_common<T>(fields, loc, nfields, x, y, out, P, Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, x0, y0, flags, stream);               \
    }                                                                                                                                                 \
    int swmhd_ensemble_particles_sample_##sfx(const T *const *fields, const int *loc, int nfields, const double *x, const double *y, double *out,     \
                                              int64_t P, int members, int64_t stride_m, int Nx, int Ny, int Hx, int Hy, int64_t sy, double x0,        \
                                              double y0, double dx, double dy, int flags, void *stream) {                                             \
        const Ens e{members, stride_m, false, false, nullptr};                                                                                        \
        return particles_sample_common<T>(fields, loc, nfields, x, y, out, P, Grid{Nx, Ny, Hx, Hy, sy, dx, dy}, x0, y0, flags, stream, &e);           \
    }

SWMHD_DEF_PARTICLES(f64, double)
SWMHD_DEF_PARTICLES(f32, float)

}  // extern "C"
