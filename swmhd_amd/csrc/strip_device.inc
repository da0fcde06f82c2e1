// What the six per-stage correction launches (coriolis.hip, diffusion.hip, biharmonic.hip, relaxation.hip, source.hip, stochastic.hip)
// share, stated once; included inside their anonymous namespace, after common.hpp and launch_plan.hpp.  A wave owns a strip of STRIP_WAVE
// lanes x VEC columns and marches down STRIP_WAVE_ROWS rows of it, VEC = 16 bytes of elements per lane where every pointer of the call has
// the same 16-byte phase and the pitches keep it (else VEC = 1): launch_plan.hpp strip_call_plan.  The STRIP_WAVES waves of a workgroup
// are consecutive row segments of one strip.  Here: the strict / fast switch and the launcher's name, the vector access, the columns of
// one lane (StripCols) and the strips built on them (Strip0 for a term of radius 0, Strip for a stencil of radius 1, Strip2 for radius 2),
// the decoding of blockIdx.x (strip_block), the per-member scalars (strip_scalars), the two-buffer
// row pipeline of the terms that carry nothing from row to row (strip_pipeline), and the host's plan, pick of an instantiation and
// launch (strip_plan_of, STRIP_KERNEL, strip_launch).  The carried rows and the arithmetic are each kernel's own.
#ifndef SWMHD_STRIP_STRICT
#error "compile with -DSWMHD_STRIP_STRICT=0 or 1 (Makefile)"
#endif
constexpr bool STRICT = (SWMHD_STRIP_STRICT != 0);
#define LAUNCH_NAME_(base, sfx) base##sfx
#define LAUNCH_NAME(base, sfx) LAUNCH_NAME_(base, sfx)
#if SWMHD_STRIP_STRICT
#define LAUNCH_SFX strict
#else
#define LAUNCH_SFX fast
#endif

template <typename T, int VEC>
__device__ __forceinline__ void vec_load(const T *p, T (&v)[VEC]) {
    if constexpr (VEC == 1) {
        v[0] = p[0];
    } else {
        using V = T __attribute__((ext_vector_type(VEC)));
        const V t = *reinterpret_cast<const V *>(p);
#pragma unroll
        for (int e = 0; e < VEC; ++e) v[e] = t[e];
    }
}
template <typename T, int VEC>
__device__ __forceinline__ void vec_store(T *p, const T (&v)[VEC]) {
    if constexpr (VEC == 1) {
        p[0] = v[0];
    } else {
        using V = T __attribute__((ext_vector_type(VEC)));
        V t;
#pragma unroll
        for (int e = 0; e < VEC; ++e) t[e] = v[e];
        *reinterpret_cast<V *>(p) = t;
    }
}

// The VEC columns xv .. xv + VEC - 1 of one lane, and the access to a row that is updated: read and written at the lane's own columns
// inside [0, Nx) and nowhere else.  lead: columns by which the vector groups start left of x = 0, so that a group inside [0, Nx) is
// 16-byte aligned in every parent.  full: the whole group lies inside (one 16-byte access).  Columns outside [0, Nx) load T(0) and store
// nothing.  load / store<FULL>: for a caller that decides FULL once per lane, outside its row loop; load / store: decided at the access.
// inside[] is filled by the strip built on this, in the one loop over the columns in which it fills what else it keeps per column (two
// loops give the same values and another instruction order in half of the kernels: profiles/strip_scaffold/README.md).
template <typename T, int VEC>
struct StripCols {
    int xv;
    bool full;
    bool inside[VEC];

    __device__ __forceinline__ StripCols(int Nx, int strip, int lane, int lead) : xv((strip * STRIP_WAVE + lane) * VEC - lead) {
        full = xv >= 0 && xv + VEC <= Nx;
    }
    __device__ __forceinline__ bool is_inside(int e, int Nx) const { return xv + e >= 0 && xv + e < Nx; }
    template <bool FULL>
    __device__ __forceinline__ void load(const T *p, T (&v)[VEC]) const {   // p: a row
        if constexpr (FULL) {
            vec_load<T, VEC>(p + xv, v);
        } else {
#pragma unroll
            for (int e = 0; e < VEC; ++e) v[e] = inside[e] ? p[xv + e] : T(0);
        }
    }
    template <bool FULL>
    __device__ __forceinline__ void store(T *p, const T (&v)[VEC]) const {
        if constexpr (FULL) {
            vec_store<T, VEC>(p + xv, v);
        } else {
#pragma unroll
            for (int e = 0; e < VEC; ++e)
                if (inside[e]) p[xv + e] = v[e];
        }
    }
    __device__ __forceinline__ void load(const T *p, T (&v)[VEC]) const {
        if (full) load<true>(p, v);
        else load<false>(p, v);
    }
    __device__ __forceinline__ void store(T *p, const T (&v)[VEC]) const {
        if (full) store<true>(p, v);
        else store<false>(p, v);
    }
};

// Strip for a term of radius 0 (relaxation.hip, stochastic.hip, the plain fields of source.hip): no neighbour column and no halo.
// any: at least one of the lane's columns lies inside [0, Nx).
template <typename T, int VEC>
struct Strip0 : StripCols<T, VEC> {
    bool any;

    __device__ __forceinline__ Strip0(int Nx, int strip, int lane, int lead) : StripCols<T, VEC>(Nx, strip, lane, lead) {
        any = false;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            this->inside[e] = this->is_inside(e, Nx);
            any = any || this->inside[e];
        }
    }
};

// Strip for a stencil of radius 1 (coriolis.hip, diffusion.hip, the weighted fields of source.hip): the lane's columns and their two
// neighbours.  A column as it is read: -1 and Nx are the halo cells or, wrapped, their periodic images; nothing further out is read.
// Lanes outside [0, Nx) load T(0).
template <typename T, int VEC>
struct Strip {
    int Nx, Ny, lane, colw, cole;
    long sy;
    bool wrapy, okw, oke;
    int col[VEC];
    bool ok[VEC];
    StripCols<T, VEC> cols;   // (a member, and the last: as a base class, laid out first, it gives source.hip's one-element kernels other instructions)

    __device__ __forceinline__ Strip(int Nx_, int Ny_, long sy_, int wrap, int strip, int lane_, int lead)
        : Nx(Nx_), Ny(Ny_), lane(lane_), sy(sy_), wrapy(wrap & 2), cols(Nx_, strip, lane_, lead) {
        const bool wrapx = wrap & 1;
        const int xv = cols.xv;
        auto column = [&](int x, bool &valid) -> int {
            valid = x >= -1 && x <= Nx;
            if (wrapx) x = x < 0 ? Nx - 1 : (x >= Nx ? 0 : x);
            return valid ? x : 0;
        };
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            col[e] = column(xv + e, ok[e]);
            cols.inside[e] = cols.is_inside(e, Nx);
        }
        colw = column(xv - 1, okw);
        cole = column(xv + VEC, oke);
    }
    __device__ __forceinline__ long row_of(int y) const {   // y in [-1, Ny]
        if (wrapy) y = y < 0 ? Ny - 1 : (y >= Ny ? 0 : y);
        return (long)y * sy;
    }
    __device__ __forceinline__ void load_in(const T *p, T (&v)[VEC]) const {   // p: a row that is read with its halo
        if (cols.full) {
            vec_load<T, VEC>(p + cols.xv, v);
        } else {
#pragma unroll
            for (int e = 0; e < VEC; ++e) v[e] = ok[e] ? p[col[e]] : T(0);
        }
    }
    // the neighbour beyond a lane's group: from the next lane, at the ends of the wave from memory
    __device__ __forceinline__ T east_of(const T *p, const T (&v)[VEC]) const {
        T x = __shfl_down(v[0], 1);
        if (lane == STRIP_WAVE - 1) x = oke ? p[cole] : T(0);
        return x;
    }
    __device__ __forceinline__ T west_of(const T *p, const T (&v)[VEC]) const {
        T x = __shfl_up(v[VEC - 1], 1);
        if (lane == 0) x = okw ? p[colw] : T(0);
        return x;
    }
};

// Strip for a stencil of radius 2 (biharmonic.hip): the same lanes, groups and lead, with two columns and two rows around.  A column as
// it is read: -2 .. Nx + 1 are the halo cells or, wrapped, their periodic images by a TRUE modulus (x mod Nx: a width of 1 or 2 folds
// more than once); nothing further out is read.  `reach` (0, 1 or 2) of a row: how many columns beyond [0, Nx) the call may read of it --
// 2 for a row that is computed, 1 and 0 for the first and the second row beyond the computed ones -- so that the reads of a call are the
// 13-cell diamonds of its cells and no more.  dist: how far a column lies outside [0, Nx) (0: inside).
template <typename T, int VEC>
struct Strip2 {
    int Nx, Ny, lane, colw, cole, colw2, cole2, distw, diste, distw2, diste2;
    long sy;
    bool wrapy;
    int col[VEC], dist[VEC];
    StripCols<T, VEC> cols;

    __device__ __forceinline__ static int fold(int v, int n) {   // v mod n for v in [-2, n + 1], n >= 1
        if (v < 0) v += n;
        if (v < 0) v += n;
        if (v >= n) v -= n;
        if (v >= n) v -= n;
        return v;
    }
    __device__ __forceinline__ Strip2(int Nx_, int Ny_, long sy_, int wrap, int strip, int lane_, int lead)
        : Nx(Nx_), Ny(Ny_), lane(lane_), sy(sy_), wrapy(wrap & 2), cols(Nx_, strip, lane_, lead) {
        const bool wrapx = wrap & 1;
        const int xv = cols.xv;
        auto column = [&](int x, int &d) -> int {
            d = x < 0 ? -x : (x >= Nx ? x - Nx + 1 : 0);
            if (d > 2) return 0;   // (never read: reach <= 2)
            return wrapx ? fold(x, Nx) : x;
        };
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            col[e] = column(xv + e, dist[e]);
            cols.inside[e] = dist[e] == 0;
        }
        colw = column(xv - 1, distw);
        cole = column(xv + VEC, diste);
        colw2 = column(xv - 2, distw2);
        cole2 = column(xv + VEC + 1, diste2);
    }
    __device__ __forceinline__ long row_of(int y) const {   // y in [-2, Ny + 1]
        if (wrapy) y = fold(y, Ny);
        return (long)y * sy;
    }
    __device__ __forceinline__ void load_in(const T *p, int reach, T (&v)[VEC]) const {   // p: a row that is read with its halo
        if (cols.full) {
            vec_load<T, VEC>(p + cols.xv, v);
        } else {
#pragma unroll
            for (int e = 0; e < VEC; ++e) v[e] = dist[e] <= reach ? p[col[e]] : T(0);
        }
    }
    // the neighbour beyond a lane's group: from the next lane, at the ends of the wave from memory
    __device__ __forceinline__ T east_of(const T *p, int reach, const T (&v)[VEC]) const {
        T x = __shfl_down(v[0], 1);
        if (lane == STRIP_WAVE - 1) x = diste <= reach ? p[cole] : T(0);
        return x;
    }
    __device__ __forceinline__ T west_of(const T *p, int reach, const T (&v)[VEC]) const {
        T x = __shfl_up(v[VEC - 1], 1);
        if (lane == 0) x = distw <= reach ? p[colw] : T(0);
        return x;
    }
    // two columns beyond the group, for the two lanes at the ends of the wave, which have no lane to take a derived row value of their
    // neighbouring column from and form it themselves: from memory; T(0) in every other lane
    __device__ __forceinline__ T east2_of(const T *p, int reach) const {
        return (lane == STRIP_WAVE - 1 && diste2 <= reach) ? p[cole2] : T(0);
    }
    __device__ __forceinline__ T west2_of(const T *p, int reach) const {
        return (lane == 0 && distw2 <= reach) ? p[colw2] : T(0);
    }
};

// blockIdx.x = (outer nsb + sb) nstrips + strip (StripPlan); the wave's rows are [r0, r1), empty (uniformly) past j1
struct StripBlock {
    unsigned outer;
    int strip, r0, r1;
};
__device__ __forceinline__ StripBlock strip_block(int nstrips, int nsb, int j0, int j1) {
    const unsigned ntiles = (unsigned)(nstrips * nsb);
    const unsigned L = xcd_remap(blockIdx.x, gridDim.x), outer = L / ntiles, tile = L - outer * ntiles;
    const int strip = (int)(tile % (unsigned)nstrips), sb = (int)(tile / (unsigned)nstrips);
    const int r0 = j0 + (sb * STRIP_WAVES + (int)threadIdx.y) * STRIP_WAVE_ROWS;
    return StripBlock{outer, strip, r0, min(r0 + STRIP_WAVE_ROWS, j1)};
}

// member m of an ensemble with a (g, f, dt) table: the products as the host forms them for one grid
template <typename T>
__device__ __forceinline__ void strip_scalars(const StripArgs<T> &a, unsigned m, T &av, T &wv) {
    if (a.params) {
        const T dt = a.params[3 * (long)m + 2];
        av = dt * a.a;
        if (a.anchor) wv = dt * a.w;
    }
}

// The march of a term that carries nothing from row to row, as a software pipeline: two row buffers A and B in turn, the loads of every
// stream of a row issued together (load_row) and one row ahead of its arithmetic and stores (finish_row), with no copy between the
// buffers.  The steady loop has no branch inside: B's loads are issued before A's row is finished and A's next loads before B's row is,
// so every wait is for one row's loads while the other row's are in flight.  The last one or two rows follow it.  carry(row): what a
// finished row leaves for the next one's finish_row; the default leaves nothing.  (The weighted fields of source.hip, which carry one
// row of h, keep this march written out -- and the default goes through the hook, not around it: either change gives the kernels
// other instructions, profiles/strip_scaffold/README.md.)
template <typename Row, typename Load, typename Finish, typename Carry>
__device__ __forceinline__ void strip_pipeline(int r0, int r1, Load load_row, Finish finish_row, Carry carry) {
    Row A, B;
    int j = r0;
    load_row(j, A);
    while (j + 2 < r1) {
        load_row(j + 1, B);
        finish_row(j, A);
        carry(A);
        load_row(j + 2, A);
        finish_row(j + 1, B);
        carry(B);
        j += 2;
    }
    if (j + 1 < r1) {
        load_row(j + 1, B);
        finish_row(j, A);
        carry(A);
        finish_row(j + 1, B);
    } else {
        finish_row(j, A);
    }
}
template <typename Row, typename Load, typename Finish>
__device__ __forceinline__ void strip_pipeline(int r0, int r1, Load load_row, Finish finish_row) {
    strip_pipeline<Row>(r0, r1, load_row, finish_row, [](const Row &) {});
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
// the plan of a call (launch_plan.hpp strip_call_plan) over the n pointers of ptrs, per_member launches for each member; further: the
// pitches of the kind that must keep the phase besides sy and stride_m
template <typename T>
StripPlan strip_plan_of(const StripArgs<T> &a, const void *const *ptrs, int n, int per_member, std::initializer_list<long> further = {}) {
    return strip_call_plan(a.Nx, a.j1 - a.j0, (int)sizeof(T), ptrs, n, a.sy, a.members, a.stride_m, per_member, further);
}
// the instantiation of kernel template k<T, VEC, ENS> that a plan and a call ask for
#define STRIP_KERNEL(k, T, plan, args)                                                                               \
    ((args).members > 0 ? ((plan).vec > 1 ? k<T, 16 / (int)sizeof(T), true> : k<T, 1, true>)                         \
                        : ((plan).vec > 1 ? k<T, 16 / (int)sizeof(T), false> : k<T, 1, false>))
// the launch of a picked kernel(args..., lead, nstrips, nsb) over the plan's workgroups; nothing to compute is no error
template <typename K, typename... Args>
hipError_t strip_launch(K kernel, const StripPlan &p, hipStream_t s, const Args &...args) {
    if (p.none) return hipSuccess;
    if (p.too_many) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(kernel, dim3((unsigned)p.blocks), dim3(STRIP_WAVE, STRIP_WAVES), 0, s, args..., p.lead, p.nstrips, p.nsb);
    return hipGetLastError();
}
