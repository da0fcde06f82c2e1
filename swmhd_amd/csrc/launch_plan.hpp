// Host-only launch planning of the fused tendency kernels, the Lorentz operator kernels, the tracer stage kernel, the six strip-march
// corrections (Coriolis, diffusion, biharmonic, relaxation, source, stochastic), the zonal-mean kernel, the derived-frame kernel and the zonal-spectrum kernels: what a call will enqueue, decided as data before anything is launched.
// No kernel, no launch call, no device memory: the only HIP call is the compute-unit query of device_cu_count(), so this header also
// compiles into a plain host program (tests/launch_plan_check.cpp).  Internal, like common.hpp.
#pragma once
#include <hip/hip_runtime_api.h>
#include <initializer_list>
#include <stdlib.h>

namespace swmhd {

// ---- topology codes of TendArgs / OpArgs / HaloBc -------------------------------------------------------------------------------
// 0 Periodic, 1 Bounded.  A Bounded y direction cut into y-slabs (swmhd_ring_step_rk3_bc, SWMHD_OPEN_SOUTH / _NORTH): bits above the
// topology code 1 in TendArgs::topo_y and HaloBc::topo_y mark a side that is a cut to a neighbouring slab, not a wall.  Reconstructions
// see the rows next to it as far from any wall (order 5 / centred 4th, no wall branch of the divergence forcing); the boundary-condition
// fill leaves its halo rows alone (they come from the neighbour).  topo_y == 1 is the whole Bounded direction, both sides walls.
constexpr int TOPO_OPEN_SOUTH = 2, TOPO_OPEN_NORTH = 4;
// THE test for "this grid has a wall kernel to run" (topo_y != 0, not == 1: a slab's topo_y carries the open-side bits)
constexpr bool is_bounded(int topo_x, int topo_y) { return topo_x == 1 || topo_y != 0; }

// Frame of a Bounded grid that the wall kernels recompute after a periodic-formula kernel has run over rows [j0, j1): FRAME_ROWS rows
// along each y wall that is a real wall (empty ranges along open sides and on a Periodic y direction), and the outermost tile columns
// along the x walls.  A cell further from a wall has exactly the periodic formulas.
constexpr int TILE_X = 64, FRAME_ROWS = 8;
// tile columns of the x-wall frame (TendArgs / OpArgs::edge_cols): the first and the last; the last two where the last one is narrower
// than 8 columns
inline int frame_tile_columns(int Nx) {
    const int ntx = (Nx + TILE_X - 1) / TILE_X, ne = (Nx % TILE_X == 0 || Nx % TILE_X >= 8) ? 2 : 3;
    return ntx < ne ? ntx : ne;
}
struct BoundedFrame {
    int s0, s1, n0, n1;   // south rows [s0, s1), north rows [n0, n1); s1 <= s0 / n1 <= n0: none
    bool x_walls;         // the x direction is Bounded: frame_tile_columns() tile columns over rows [j0, j1)
};
inline BoundedFrame bounded_frame(int Ny, int j0, int j1, int topo_x, int topo_y) {
    BoundedFrame f{j0, j0, j1, j1, topo_x == 1};
    if (topo_y != 0 && !(topo_y & TOPO_OPEN_SOUTH)) f.s1 = j1 < FRAME_ROWS ? j1 : FRAME_ROWS;
    if (topo_y != 0 && !(topo_y & TOPO_OPEN_NORTH)) f.n0 = j0 > Ny - FRAME_ROWS ? j0 : Ny - FRAME_ROWS;
    return f;
}

// ---- launch geometry of the row-marching kernels --------------------------------------------------------------------------
// One workgroup = a strip of nt - 2*xh output columns x LY rows; the grid is a whole number of rounds of resident workgroups.
// Folded last strip (fold = 1): where the last strip has at most nt/2 - 2*xh output columns, each of its workgroups runs two
// half-width sub-strips of nt/2 lanes on two segments, so a segment row costs nstrips - 1/2 workgroups instead of nstrips.
struct MarchGeometry {
    int nt;        // threads per workgroup (strip width incl. 2*xh halo lanes)
    int nstrips, nseg, LY;
    int wg_per_cu; // resident workgroups per CU the kernel is built for
    int fold;      // 1: the last strip is folded (nstrips still counts it as one strip)
    int blocks() const { return fold ? (nstrips - 1) * nseg + (nseg + 1) / 2 : nstrips * nseg; }
};
// Compute units of the current device (hipDeviceAttributeMultiprocessorCount; 256 on MI355X), cached per process.
inline int device_cu_count() {
    static int cus = 0;
    if (cus <= 0) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
            n = 256;
        cus = n;
    }
    return cus;
}
// Tuning knobs are read from the environment ONCE per process (not on every launch).
inline int env_knob(const char *name, int &cache) {   // cache: 0 = not read yet, -1 = unset, > 0 = value
    if (cache == 0) {
        const char *e = getenv(name);
        const int v = e ? atoi(e) : 0;
        cache = v > 0 ? v : -1;
    }
    return cache > 0 ? cache : 0;
}
// Share of the workgroup slots an interior launch of the slab driver leaves free for the comm stream's kernels, in 64ths: 3 (4.7 %),
// and 1 (1.6 %) for slabs of 3072 rows and more -- the boundary work per step is fixed, a long interior launch gives it time enough in
// few slots, and every slot costs the interior launch its share of the chip (4096 x 4096 ring-of-one step: +1.4-1.9 % over the plain
// step with 1, +3.7-4.0 % with 3; 4096 x 2048: +4.8-5.2 % vs +4.6-4.7 %; three alternating runs each).  SWMHD_RING_ROOM overrides (tuning).
inline int leave_room_64ths(int rows) {
    static int cache = 0;
    const int v = env_knob("SWMHD_RING_ROOM", cache);
    return v > 0 ? (v < 32 ? v : 32) : (rows >= 3072 ? 1 : 3);
}
// Strip width: the FIRST candidate workgroup size unless a later one covers Nx with at least 5 % fewer lanes (1024 columns: 5 strips x
// 256 lanes = 1280, but 9 x 128 = 1152).  Rows per segment: the smallest whole number of rounds of resident workgroups
// (wg_per_cu x CUs slots; ~5 % fewer with leave_room, so that another stream's kernels find room) whose segments are at most
// 128 rows, but never shorter than ly_min rows.  fold_nt: the workgroup size whose kernel can fold its last strip (0: none); the strip
// width is chosen first, and folding then only changes how many workgroups a segment row costs.  max_rounds: how many rounds are tried
// before the segments fall back to 32 rows.
inline MarchGeometry march_geometry(int Nx, int rows, int xh, const int *nts, const int *wgs, int ncand, int ly_min, bool leave_room,
                                    int force_nt, int force_ly, int fold_nt = 0, int max_rounds = 64) {
    MarchGeometry g{};
    long best = -1;
    for (int k = 0; k < ncand; ++k) {
        const int txo = nts[k] - 2 * xh, ns = (Nx + txo - 1) / txo;
        const long lanes = (long)ns * nts[k];
        const bool take = force_nt ? nts[k] == force_nt : (best < 0 || lanes * 20 <= best * 19);
        if (take) { best = lanes; g.nt = nts[k]; g.nstrips = ns; g.wg_per_cu = wgs[k]; }
    }
    if (best < 0) { g.nt = nts[0]; g.nstrips = (Nx + nts[0] - 2 * xh - 1) / (nts[0] - 2 * xh); g.wg_per_cu = wgs[0]; }
    g.fold = fold_nt && g.nt == fold_nt && g.nstrips > 1 && Nx - (g.nstrips - 1) * (g.nt - 2 * xh) <= g.nt / 2 - 2 * xh ? 1 : 0;
    const int halves = 2 * g.nstrips - g.fold;   // half-workgroups per segment row
    int slots = device_cu_count() * g.wg_per_cu;
    if (leave_room) slots -= (slots * leave_room_64ths(rows)) / 64;
    int LY = 32;
    for (int k = 1; k <= max_rounds; ++k) {
        const int ns = (2 * slots * k) / halves;
        if (ns < 1) continue;
        const int ly = (rows + ns - 1) / ns;
        if (ly <= 128) { LY = ly < ly_min ? ly_min : ly; break; }
    }
    if (force_ly > 0) LY = force_ly;
    g.LY = LY;
    g.nseg = (rows + LY - 1) / LY;
    return g;
}

// Workgroups per CU of the conservative marching kernel, per stage variant (MODE: bits at k_tendency_vi_march).  ONE definition for the
// kernel's __launch_bounds__ and for the geometry that fills the slots it implies.  fp64: the variants of CONS_W3_MODES fit three
// workgroups of 256 (measurements at k_tendency_cons_march, tendency_march_kernels.inc), the others two; fp32: three throughout.
constexpr int CONS_W3_MODES = (1 << 7) | (1 << 5) | (1 << 4) | (1 << 9) | (1 << 11);
constexpr int cons_minwaves(int mode, int elem_size) { return elem_size == 4 ? 3 : (((CONS_W3_MODES >> mode) & 1) ? 3 : 2); }

// Geometry of the marching tendency kernels.  Vector-invariant kernel: <= 168 VGPRs and 0.19 KB of LDS per lane -> 12 waves per
// CU, i.e. 3 / 6 workgroups of 256 / 128 threads.  Conservative kernel: 2 or 3 workgroups of 256 per CU (cons_minwaves).
// Knobs (read once): SWMHD_T_LY rows per segment, SWMHD_T_NT workgroup size (128 or 256), SWMHD_T_FOLD=0 no folded last strip (A/B).
// Folded last strip (fp64 vector-invariant kernel, 256 lanes, last strip <= 122 output columns; tendency_march_kernels.inc): 4096
// columns run 16 full workgroups and half a folded one per segment row instead of 17 -- LY 90 instead of 92 in one round.
// Packed-fp32 kernel (tendency_pk_kernels.inc): vector-invariant model, x read with periodic wrapping, even Nx.  256 lanes = 512
// columns per strip, 504 of them output; 3 workgroups per CU (<= 168 VGPRs, 46 KB LDS).
inline bool tendency_uses_packed_fp32(int Nx, int formulation, int wrap) {
    return formulation == 1 && (wrap & 1) && (Nx % 2 == 0) && Nx >= 8;
}
inline int tendency_force_ly() {
    static int cache = 0;
    return env_knob("SWMHD_T_LY", cache);
}
inline MarchGeometry packed_fp32_geometry(int Nx, int rows, int leave_room) {
    static const int cols[1] = {512}, wgs[1] = {3};   // in columns: 2 per lane, 4 halo columns a side -> 504 output columns per strip
    MarchGeometry g = march_geometry(Nx, rows, 4, cols, wgs, 1, 6, leave_room != 0, 0, tendency_force_ly());
    g.nt = 256;
    return g;
}
inline bool tendency_fold_enabled() {
    static const bool on = [] { const char *e = getenv("SWMHD_T_FOLD"); return !e || atoi(e) != 0; }();
    return on;
}
// fold_ok: the launch may fold its last strip (one row range: the slab driver's two-range launches keep full strips)
inline MarchGeometry tendency_march_geometry(int Nx, int rows, int formulation, int leave_room, int elem_size, int mode, bool fold_ok) {
    static int nt_cache = 0;
    const int force_ly = tendency_force_ly(), force_nt = env_knob("SWMHD_T_NT", nt_cache);
    if (formulation == 1) {
        // (384-thread workgroups cover 4096 columns with 3 % fewer lanes -- 11 strips instead of 17 -- but measured 37 % SLOWER on
        //  MI355X, 1.75 vs 1.275 ms per step: six waves per barrier leave each SIMD too little to overlap; removed after that measurement)
        static const int nts[2] = {256, 128}, wgs64[2] = {3, 6}, wgs32[2] = {4, 8};   // fp32: <= 128 VGPRs, 4 waves per SIMD
        const int fold_nt = elem_size == 8 && fold_ok && tendency_fold_enabled() ? 256 : 0;
        return march_geometry(Nx, rows, 3, nts, elem_size == 8 ? wgs64 : wgs32, 2, 6, leave_room != 0, force_nt, force_ly, fold_nt);
    }
    // (128-thread workgroups where they waste >= 5 % fewer lanes in the last strip: 1024 columns = 5 strips of 250 or 9 of 122)
    const int w = cons_minwaves(mode, elem_size);
    const int nts[2] = {256, 128}, wgs[2] = {w, 2 * w};
    return march_geometry(Nx, rows, 3, nts, wgs, 2, 6, leave_room != 0, force_nt, force_ly);
}

// ---- the plan of one tendency call ------------------------------------------------------------------------------------------------
constexpr long SW_MARCH_MIN_CELLS = 330000L;

// What the decision depends on: the fields of TendArgs of the same names, plus the build and, for an ensemble, the member count.
struct TendPlanIn {
    int Nx, Ny, Hy;
    long sy;              // 0: no parent known (the geometry query) -- taken to lie below 4 GiB
    int elem_size;
    int j0, j1, j0b, j1b;
    int formulation;
    bool strict;
    int kernel_variant, wrap, leave_room, topo_x, topo_y, edge_cols;
    int fuse, first, store_G, gm_prev, anchor;
    int members;          // > 0: an ensemble stage (LDS-tiled kernel, one row range, no frame); 0: a single grid
};
enum class TendKernel { TILE_RY1, TILE_RY2, TILE_BOUNDED, MARCH, MARCH_PACKED };   // 64 x 4 tiles | 64 x 8 | 64 x 8 wall kernel | row-marching | packed fp32
// One launch: the kernel family, its grid, and the arguments it runs with where they differ from the caller's.
struct TendLaunch {
    TendKernel kernel;
    int ntx, nty;             // tile kernels: tile columns, tile rows (both row ranges)
    MarchGeometry mg;         // marching kernels (mg.fold becomes TendArgs::fold_last)
    int mode, drop_G;         // marching kernels: compiled stage variant (MODE bits at k_tendency_vi_march); its G stores are to be dropped
    int j0, j1, j0b, j1b;     // row ranges of this launch
    int topo_x, topo_y;       // topology the kernel sees (0, 0 for the periodic body of a hybrid launch)
    int edge_cols;
    bool tile() const { return kernel != TendKernel::MARCH && kernel != TendKernel::MARCH_PACKED; }
};
struct TendPlan {
    int n = 0;
    TendLaunch e[3];
};

// Compiled stage variant of the marching kernels for a stage, and whether that variant stores a G the stage must not (drop_G: the
// stores are issued with an out-of-range offset).
inline int march_stage_mode(const TendPlanIn &a, int &drop_G) {
    int mode = (a.fuse ? 1 : 0) | ((a.fuse && !a.first) ? 2 : 0) | ((a.store_G || !a.fuse) ? 4 : 0) | (a.anchor ? 8 : 0);
    const bool cons64 = a.formulation == 0 && a.elem_size == 8;
    drop_G = 0;
    // The previous-state operand (gm_prev) lives in the stage-2 variant (coefficient form).  Conservative model: the last RK3 stage
    // (MODE 3) runs on the stage-2 variant (3 workgroups per CU, no scratch) with its G stores dropped by the hardware: 4096^2 step
    // 1.39-1.40 -> 1.36 ms.  (The same substitution bought nothing for the vector-invariant kernel, whose MODE 3 already has its third
    // workgroup: 398-403 vs 403-408 us.)
    if (mode == 3 && (a.gm_prev || (cons64 && cons_minwaves(7, 8) > cons_minwaves(3, 8)))) { mode = 7; drop_G = 1; }
    // ... and the first stage without a G store (MODE 1, two workgroups per CU) on the MODE-5 variant, likewise
    if (mode == 1 && cons64 && cons_minwaves(5, 8) > cons_minwaves(1, 8)) { mode = 5; drop_G = 1; }
    return mode;
}

inline TendLaunch tile_launch(TendKernel k, int ntx, int j0, int j1, int j0b, int j1b, int topo_x, int topo_y, int edge_cols) {
    const int ty = k == TendKernel::TILE_RY1 ? 4 : 8, rows_b = j1b > j0b ? j1b - j0b : 0;
    TendLaunch l{};
    l.kernel = k; l.ntx = ntx; l.nty = (j1 - j0 + ty - 1) / ty + (rows_b + ty - 1) / ty;
    l.j0 = j0; l.j1 = j1; l.j0b = j0b; l.j1b = j1b; l.topo_x = topo_x; l.topo_y = topo_y; l.edge_cols = edge_cols;
    return l;
}

// The launches of one tendency call, in order (none: nothing to compute).
// Kernel choice, fast builds: the row-marching kernels overtake the tile kernel between 512^2 and 640^2 cells for both formulations
// (tools/crossover.py: 640^2 82 vs 111 us/step, 1024^2 119 vs 184, 1280^2 161 vs 276; at 512^2 the tile kernel with its fused halo fill
// wins 60 : 80); small grids and the 3-row boundary strips of the overlapped multi-GPU step take the tile kernel.  kernel_variant 1 / 2
// force tile / marching.  Strict builds and ensembles have the tile kernel only.
inline TendPlan plan_tendency(TendPlanIn a) {
    TendPlan p;
    if (a.j1b <= a.j0b) a.j0b = a.j1b = 0;
    if (a.j1 <= a.j0 && a.j1b > a.j0b) { a.j0 = a.j0b; a.j1 = a.j1b; a.j0b = a.j1b = 0; }   // an empty first range: the second alone
    if (a.Nx <= 0 || a.j1 <= a.j0) return p;
    const bool two = a.j1b > a.j0b, bnd = is_bounded(a.topo_x, a.topo_y), fast = !a.strict && a.members <= 0;
    const int rows = a.j1 - a.j0 + (a.j1b - a.j0b);
    const bool big = (long)a.Nx * rows >= SW_MARCH_MIN_CELLS;
    const int ntx = a.edge_cols ? frame_tile_columns(a.Nx) : (a.Nx + TILE_X - 1) / TILE_X;
    // (the marching kernels address memory with 32-bit byte offsets: fields of 4 GiB or more stay on the tile kernel)
    const long parent_bytes = (long)(a.Ny + 2 * a.Hy) * a.sy * a.elem_size, row_bytes = a.sy * a.elem_size, lim32 = (1L << 32) - 64;
    const bool fits32 = parent_bytes < lim32;
    auto march = [&](int topo_x, int topo_y) {
        TendLaunch l{};
        const bool packed = a.elem_size == 4 && tendency_uses_packed_fp32(a.Nx, a.formulation, a.wrap);   // two columns per lane
        l.kernel = packed ? TendKernel::MARCH_PACKED : TendKernel::MARCH;
        l.mode = march_stage_mode(a, l.drop_G);
        // (a folded workgroup's rows without an output store one row beyond the parent: that offset must fit 32 bits too)
        const bool fold_ok = !two && parent_bytes + row_bytes < lim32;
        // Segments may be as short as 6 rows (as many warm-up rows as output rows): on mid-size grids filling the chip matters more
        // than the warm-up overhead (1024^2: 42 us/stage at LY = 7, 54 at 16).
        l.mg = packed ? packed_fp32_geometry(a.Nx, rows, a.leave_room)
                      : tendency_march_geometry(a.Nx, rows, a.formulation, a.leave_room, a.elem_size, l.mode, fold_ok);
        // (two ranges: the segments of the second range follow those of the first, same LY.  One 9-12-row segment per zone instead of
        //  two 6-row ones -- a single round of workgroups in the slots the interior launch leaves free -- measured slower: 4096 x 512
        //  ring-of-one step +22 % over plain instead of +11 %)
        if (two) l.mg.nseg = (a.j1 - a.j0 + l.mg.LY - 1) / l.mg.LY + (a.j1b - a.j0b + l.mg.LY - 1) / l.mg.LY;
        l.j0 = a.j0; l.j1 = a.j1; l.j0b = a.j0b; l.j1b = a.j1b; l.topo_x = topo_x; l.topo_y = topo_y; l.edge_cols = a.edge_cols;
        return l;
    };
    if (fast && !bnd && fits32 && (a.kernel_variant == 2 || (a.kernel_variant == 0 && big))) {
        p.e[p.n++] = march(0, 0);
        return p;
    }
    // Large Bounded grids: a cell further than a few cells from a wall has exactly the periodic formulas (every reconstruction at full
    // order, no wall branch of the Lorentz fluxes).  So the row-marching kernel computes ALL rows as if the grid were periodic, reading
    // the boundary-condition halos from memory, and the LDS-tiled Bounded kernel then overwrites the frame (bounded_frame; fused
    // substep included: all launches compute from the same old state).  A y-slab's cut side has no frame rows (TOPO_OPEN_*).
    // 4096^2 (Bounded, Bounded), RK3 step incl. the boundary-condition fills: 3.12 -> 1.49 ms (vector-invariant), 4.34 -> 1.67
    // (conservative); periodic 1.31 / 1.36 in the same call (tools/time_bounded.py).
    if (fast && bnd && !two && !a.edge_cols && fits32 && a.kernel_variant == 0 && big && a.Nx >= 4 * TILE_X && a.Ny >= 48) {
        p.e[p.n++] = march(0, 0);
        BoundedFrame f = bounded_frame(a.Ny, a.j0, a.j1, a.topo_x, a.topo_y);
        if (f.s1 <= f.s0) { f.s0 = f.n0; f.s1 = f.n1; f.n0 = f.n1 = 0; }
        if (f.n1 <= f.n0) f.n0 = f.n1 = 0;
        if (f.s1 > f.s0) p.e[p.n++] = tile_launch(TendKernel::TILE_BOUNDED, ntx, f.s0, f.s1, f.n0, f.n1, a.topo_x, a.topo_y, 0);
        if (f.x_walls) p.e[p.n++] = tile_launch(TendKernel::TILE_BOUNDED, frame_tile_columns(a.Nx), a.j0, a.j1, 0, 0, a.topo_x, a.topo_y, 1);
        return p;
    }
    // Tile height.  Bounded grids: the wall kernel, 64 x 8.  Small grids of fast builds (the reference's own 64^2 .. 128^2,
    // SWMHD_example.jl:11, up to where the marching kernels take over) and thin strips: there are at most a few tiles per CU, so the
    // launch lasts about as long as ONE tile takes; one output row per lane (64 x 4 tiles) instead of two halves the dependent
    // arithmetic of that tile (64^2 .. 256^2: 41 -> 27 us per RK3 step, 512^2: 60 -> 52).  Larger grids forced onto the tile kernel
    // keep 64 x 8 tiles (less halo per cell), as do strict builds.  An ensemble's members take the tile a single model of the member's
    // size would take; SWMHD_ENS_RY = 1 | 2 forces the height for periodic members (read once; measurement only).
    TendKernel k = bnd ? TendKernel::TILE_BOUNDED : (!a.strict && !big ? TendKernel::TILE_RY1 : TendKernel::TILE_RY2);
    if (a.members > 0 && !bnd) {
        static int ry_cache = 0;
        const int force_ry = env_knob("SWMHD_ENS_RY", ry_cache);
        if (force_ry == 1 || force_ry == 2) k = force_ry == 1 ? TendKernel::TILE_RY1 : TendKernel::TILE_RY2;
    }
    p.e[p.n++] = tile_launch(k, ntx, a.j0, a.j1, a.j0b, a.j1b, a.topo_x, a.topo_y, a.edge_cols);
    return p;
}

// How an ensemble stage maps members onto the grid (launch_ensemble_stage): folded into blockIdx.x (1, the default) or blockIdx.y (2).
// Knob (read once; measurement only): SWMHD_ENS_MAP = 1 | 2.
inline int ensemble_member_map() {
    static int cache = 0;
    return env_knob("SWMHD_ENS_MAP", cache) == 2 ? 2 : 1;
}
// swmhd_ensemble_launch_geometry: the launch of a fused ensemble stage over all Ny rows of `members` members, from the planner and
// the knob reader that launch_ensemble_stage asks.  out: kind (1 LDS-tiled), threads, tile columns, tile rows, rows per tile, member
// mapping (1 blockIdx.x, 2 blockIdx.y), grid.x, grid.y.  1: not one tile launch (nothing to do, or no plan).
inline int ensemble_launch_geometry(int Nx, int Ny, int formulation, int elem_size, bool strict, int wrap, int topo_x, int topo_y,
                                    int members, int out[8]) {
    TendPlanIn in{};
    in.Nx = Nx; in.Ny = Ny; in.elem_size = elem_size; in.j1 = Ny; in.formulation = formulation; in.strict = strict;
    in.kernel_variant = 1; in.wrap = wrap; in.topo_x = topo_x; in.topo_y = topo_y;
    in.fuse = 1; in.store_G = 1; in.members = members;
    const TendPlan p = plan_tendency(in);
    if (p.n != 1 || !p.e[0].tile()) return 1;
    const TendLaunch &l = p.e[0];
    const int map = ensemble_member_map();
    const long tiles = (long)l.ntx * l.nty, gx = map == 2 ? tiles : tiles * members;
    if (gx >= (1L << 31)) return 1;
    out[0] = 1; out[1] = 256; out[2] = l.ntx; out[3] = l.nty; out[4] = l.kernel == TendKernel::TILE_RY1 ? 4 : 8;
    out[5] = map; out[6] = (int)gx; out[7] = map == 2 ? members : 1;
    return 0;
}

// swmhd_tendency_launch_geometry: the first launch of the plan of a periodic single-range stage of MODE 7 (a fused middle stage that
// stores G) on a parent below 4 GiB.  out: kind (1 LDS-tiled, 2 row-marching, 3 packed fp32), threads, strips | tile columns, segments |
// tile rows, rows per segment | tile, workgroups per CU (0: tiles), halo lanes a side, CUs.
inline int tendency_launch_geometry(int Nx, int rows, int formulation, int elem_size, bool strict, int kernel_variant, int leave_room,
                                    int wrap, int out[8]) {
    TendPlanIn in{};
    in.Nx = Nx; in.Ny = rows; in.elem_size = elem_size; in.j1 = rows; in.formulation = formulation; in.strict = strict;
    in.kernel_variant = kernel_variant; in.wrap = wrap; in.leave_room = leave_room;
    in.fuse = 1; in.store_G = 1;
    const TendPlan p = plan_tendency(in);
    if (p.n < 1) return 1;
    const TendLaunch &l = p.e[0];
    if (l.tile()) {
        out[0] = 1; out[1] = 256; out[2] = l.ntx; out[3] = l.nty; out[4] = l.kernel == TendKernel::TILE_RY1 ? 4 : 8; out[5] = 0; out[6] = 3;
    } else {
        const bool packed = l.kernel == TendKernel::MARCH_PACKED;
        out[0] = packed ? 3 : 2; out[1] = l.mg.nt; out[2] = l.mg.nstrips; out[3] = l.mg.nseg; out[4] = l.mg.LY; out[5] = l.mg.wg_per_cu;
        out[6] = packed ? 2 : 3;
    }
    out[7] = device_cu_count();
    return 0;
}

// ---- the plan of one Lorentz operator call ------------------------------------------------------------------------------------------
// Marching operator kernels (lorentz_march_kernels.inc): 256 lanes, 2 (Jacobian form) / 3 (divergence form) halo lanes a side, 6 / 5
// workgroups per CU.  Their geometry is march_geometry's with other parameters than the tendency kernels', because these kernels do
// less: one workgroup size and no folded last strip (their kernels have neither variant), never a comm stream beside them (no
// leave_room), and segments of at least 8 rows, not 6 (4-6 warm-up rows per segment; divergence form at 1024^2: 17 us at 8 rows, 23 us
// at 16).  At most 16 rounds are tried, not 64: a grid taller than that takes 32-row segments.  SWMHD_OP_LY overrides the rows per
// segment (tuning; read once).
constexpr int OP_MARCH_NT = 256, OP_MARCH_MAX_ROUNDS = 16, OP_MARCH_LY_MIN = 8;
constexpr int OP_JAC_TILE_Y = 16, OP_DIV_TILE_Y = 8;   // tile kernels: TILE_X columns x this many rows
inline MarchGeometry lorentz_march_geometry(int Nx, int rows, bool divergence) {
    static int ly_cache = 0;
    const int nts[1] = {OP_MARCH_NT}, wgs[1] = {divergence ? 5 : 6};
    return march_geometry(Nx, rows, divergence ? 3 : 2, nts, wgs, 1, OP_MARCH_LY_MIN, false, 0, env_knob("SWMHD_OP_LY", ly_cache), 0,
                          OP_MARCH_MAX_ROUNDS);
}
// Cross-over of the tile and the marching kernels, fast builds: Jacobian form at ~2 Mcell; divergence form near 1000^2 (1024^2 17 vs
// 20 us, 1448^2 27 vs 41 us).
constexpr long OP_JAC_MARCH_MIN_CELLS = 2000000L, OP_DIV_MARCH_MIN_CELLS = 900000L;

// What the decision depends on: the fields of OpArgs of the same names, plus the form and the build.
struct OpPlanIn {
    int Nx, Ny, j0, j1;
    bool divergence, strict;
    int kernel_variant, topo_x, topo_y, edge_cols;
};
enum class OpKernel { TILE, MARCH };
struct OpLaunch {
    OpKernel kernel;
    int ntx, nty;         // tile kernel: tile columns, tile rows
    MarchGeometry mg;     // marching kernel
    int j0, j1;           // rows of this launch
    int topo_x, topo_y;   // topology the kernel sees (0, 0 for the periodic body of a hybrid launch)
    int edge_cols;
};
struct OpPlan {
    int n = 0;
    OpLaunch e[4];
};

// The launches of one operator call, in order (none: nothing to compute).  kernel_variant 1 / 2 force tile / marching; strict builds
// have the tile kernels only.  The Jacobian form has no wall branches: its kernels read neither the topology nor edge_cols.
inline OpPlan plan_lorentz(const OpPlanIn &a) {
    OpPlan p;
    const int rows = a.j1 - a.j0;
    if (a.Nx <= 0 || rows <= 0) return p;
    const bool bnd = a.divergence && is_bounded(a.topo_x, a.topo_y);
    const bool big = (long)a.Nx * rows >= (a.divergence ? OP_DIV_MARCH_MIN_CELLS : OP_JAC_MARCH_MIN_CELLS);
    auto launch = [&](OpKernel k, int j0, int j1, int topo_x, int topo_y, int edge_cols) {
        OpLaunch l{};
        l.kernel = k; l.j0 = j0; l.j1 = j1; l.topo_x = topo_x; l.topo_y = topo_y; l.edge_cols = edge_cols;
        if (k == OpKernel::MARCH) l.mg = lorentz_march_geometry(a.Nx, j1 - j0, a.divergence);
        else {
            const int ty = a.divergence ? OP_DIV_TILE_Y : OP_JAC_TILE_Y;
            l.ntx = a.divergence && edge_cols ? frame_tile_columns(a.Nx) : (a.Nx + TILE_X - 1) / TILE_X;
            l.nty = (j1 - j0 + ty - 1) / ty;
        }
        p.e[p.n++] = l;
    };
    // (the marching divergence kernel implements the periodic branch only)
    if (!a.strict && !bnd && (a.kernel_variant == 2 || (a.kernel_variant == 0 && big))) {
        launch(OpKernel::MARCH, a.j0, a.j1, a.topo_x, a.topo_y, a.edge_cols);
        return p;
    }
    // Large Bounded grids, divergence form: the marching kernel (periodic branch) over every row, then the tile kernel with the
    // reference's wall branches over the frame of cells near the walls (bounded_frame, as in plan_tendency).  The two y strips are two
    // launches: k_lorentz_divergence has one row range.
    if (!a.strict && bnd && !a.edge_cols && a.kernel_variant == 0 && big && a.Nx >= 4 * TILE_X && a.Ny >= 48) {
        const BoundedFrame f = bounded_frame(a.Ny, a.j0, a.j1, a.topo_x, a.topo_y);
        launch(OpKernel::MARCH, a.j0, a.j1, 0, 0, 0);
        if (f.s1 > f.s0) launch(OpKernel::TILE, f.s0, f.s1, a.topo_x, a.topo_y, 0);
        if (f.n1 > f.n0) launch(OpKernel::TILE, f.n0, f.n1, a.topo_x, a.topo_y, 0);
        if (f.x_walls) launch(OpKernel::TILE, a.j0, a.j1, a.topo_x, a.topo_y, 1);
        return p;
    }
    launch(OpKernel::TILE, a.j0, a.j1, a.topo_x, a.topo_y, a.edge_cols);
    return p;
}

// ---- the tiles of one tracer stage --------------------------------------------------------------------------------------------------
constexpr int TRACER_TILE_X = 64, TRACER_TILE_Y = 16;   // cells of a workgroup's tile (profiles/tracers/README.md)
struct TracerTiles {
    int ntx, nty;
    long blocks;      // ntx * nty * members: every tile of every member in one launch
    bool none;        // nothing to compute: no rows, no tracers or no members
    bool too_many;    // 2^31 blocks or more: beyond the grid of one launch
};
// members: 1 for a single grid
inline TracerTiles tracer_tiles(int Nx, int rows, int K, int members) {
    TracerTiles t{};
    t.none = rows <= 0 || K <= 0 || members <= 0;
    if (t.none) return t;
    t.ntx = (Nx + TRACER_TILE_X - 1) / TRACER_TILE_X;
    t.nty = (rows + TRACER_TILE_Y - 1) / TRACER_TILE_Y;
    t.blocks = (long)t.ntx * t.nty * members;
    t.too_many = t.blocks >= (1L << 31);
    return t;
}

// ---- the strips of one per-stage correction launch (strip_device.inc: coriolis.hip, diffusion.hip, biharmonic.hip, relaxation.hip,
// source.hip, stochastic.hip) ---------------------------------------------------------------------------------------------------------
// A wave owns a strip of STRIP_WAVE lanes x vec columns and marches down STRIP_WAVE_ROWS rows of it; the STRIP_WAVES waves of a
// workgroup are consecutive row segments of one strip.  vec = 16 bytes of elements where `phase` >= 0: the 16-byte phase (in elements)
// that the interior pointers of all parents share and the pitches keep (common_phase) -- then the vector groups start `lead` = phase
// columns left of x = 0, so that a group inside [0, Nx) is 16-byte aligned in every parent.  phase < 0: one element per lane.
// blockIdx.x = (l nsb + sb) nstrips + strip, l < launches: the member (Coriolis), member x field (the five others).
constexpr int STRIP_WAVE = 64, STRIP_WAVES = 4, STRIP_WAVE_ROWS = 16;   // STRIP_WAVES STRIP_WAVE_ROWS = SWMHD_CORIOLIS_ / SWMHD_DIFFUSION_ / SWMHD_RELAXATION_TILE_ROWS
struct StripPlan {
    int vec, lead;
    int nstrips, nsb; // strips of 64 vec columns x blocks of STRIP_WAVES row segments, of one of the launches
    long blocks;      // nstrips * nsb * launches (0 where too_many)
    bool none;        // nothing to compute: no columns, no rows or no launches
    bool too_many;    // 2^31 blocks or more: beyond the grid of one launch
};
// launches: 1 for one field of a single grid
inline StripPlan strip_plan(int Nx, int rows, int elem_size, int phase, int launches) {
    StripPlan p{};
    p.none = Nx <= 0 || rows <= 0 || launches <= 0;
    if (p.none) return p;
    p.vec = phase >= 0 ? 16 / elem_size : 1;
    p.lead = phase >= 0 ? phase : 0;
    const long cols = (long)STRIP_WAVE * p.vec, tile_rows = (long)STRIP_WAVES * STRIP_WAVE_ROWS;
    const long nstrips = ((long)Nx + p.lead + cols - 1) / cols, nsb = ((long)rows + tile_rows - 1) / tile_rows;
    p.nstrips = (int)nstrips; p.nsb = (int)nsb;
    p.too_many = nstrips * nsb >= (1L << 31) || nstrips * nsb * launches >= (1L << 31);   // (in this order: the product cannot overflow)
    if (!p.too_many) p.blocks = nstrips * nsb * launches;
    return p;
}
// The 16-byte phase (in elements) that the n pointers of ptrs share (null entries are skipped), or -1: where they differ, or where the
// row pitch sy or the member pitch stride_m (0: one grid) does not keep it.
inline int common_phase(int elem_size, long sy, long stride_m, const void *const *ptrs, int n) {
    const int V = 16 / elem_size;
    if (sy % V != 0 || stride_m % V != 0) return -1;
    int ph = -1;
    for (int k = 0; k < n; ++k) {
        if (!ptrs[k]) continue;
        const int q = (int)(((unsigned long)ptrs[k] / (unsigned long)elem_size) % (unsigned long)V);
        if (ph >= 0 && q != ph) return -1;
        ph = q;
    }
    return ph;
}
// The plan of one correction call: rows rows of Nx columns of every parent in ptrs (n entries, null ones skipped), per_member launches
// for each member (members <= 0: one grid, whose stride_m is not looked at).  The phase is common_phase's, kept by `further` too: the
// pitches of a kind beyond sy and stride_m (a mask's or a source's member pitch, the pitch of a table) -- 0: shared or not applicable,
// which keeps every phase.
inline StripPlan strip_call_plan(int Nx, int rows, int elem_size, const void *const *ptrs, int n, long sy, int members, long stride_m,
                                 int per_member, std::initializer_list<long> further = {}) {
    int phase = common_phase(elem_size, sy, members > 0 ? stride_m : 0, ptrs, n);
    for (const long pitch : further)
        if (pitch % (16 / elem_size) != 0) phase = -1;
    return strip_plan(Nx, rows, elem_size, phase, (members > 0 ? members : 1) * per_member);
}

// ---- the rows of one zonal-mean call (zonal.hip) -------------------------------------------------------------------------------------
// One wavefront reduces one row: lane l takes the 4-cell chunks l, l + 64, l + 128, ... of the row (ZONAL_TRIP = 256 cells per trip of
// the wave), adds their terms serially in x order, and a 6-level butterfly adds the 64 lane sums.  Four rows per 256-thread workgroup,
// the workgroups of member m after those of member m - 1 in blockIdx.x.  The summation order is zonal_depth's: a function of Nx alone.
constexpr int ZONAL_NT = 256, ZONAL_WAVE = 64, ZONAL_VEC = 4;
constexpr int ZONAL_ROWS = ZONAL_NT / ZONAL_WAVE, ZONAL_TRIP = ZONAL_WAVE * ZONAL_VEC;
struct ZonalPlan {
    int rows_per_block;
    long row_blocks;  // workgroups of one member
    long blocks;      // row_blocks * members: every row of every member in one launch
    bool none;        // nothing to compute: no rows or no members
    bool too_many;    // 2^31 blocks or more: beyond the grid of one launch
};
// members: 1 for a single grid
inline ZonalPlan zonal_plan(int rows, int members) {
    ZonalPlan p{};
    p.rows_per_block = ZONAL_ROWS;
    p.none = rows <= 0 || members <= 0;
    if (p.none) return p;
    p.row_blocks = ((long)rows + ZONAL_ROWS - 1) / ZONAL_ROWS;
    p.blocks = p.row_blocks * members;
    p.too_many = p.blocks >= (1L << 31);
    return p;
}
// Additions on the longest path from a term to the row sum: lane 0 has the most terms, 4 per full trip and min(4, cells left) of the
// ragged one, added one after the other (terms - 1 additions); then one butterfly level per bit of (lanes with terms - 1) -- a level
// whose partner lane has no term adds 0.0, which is exact.  The bound of tests/zonal_cases.py.
inline int zonal_depth(int Nx) {
    if (Nx <= 0) return 0;
    const int rem = Nx % ZONAL_TRIP, terms0 = ZONAL_VEC * (Nx / ZONAL_TRIP) + (rem < ZONAL_VEC ? rem : ZONAL_VEC);
    const int chunks = (Nx + ZONAL_VEC - 1) / ZONAL_VEC, lanes = chunks < ZONAL_WAVE ? chunks : ZONAL_WAVE;
    int levels = 0;
    while ((1 << levels) < lanes) ++levels;
    return terms0 - 1 + levels;
}

// ---- the two launches of one zonal-spectrum call (spectra.hip) -----------------------------------------------------------------------
// Pass 1: W units per (member, field); unit w transforms the rows w, w + W, w + 2W, ... of the range one after the other in LDS and adds
// their p_j[k] to per-thread accumulators in that order, then stores its partial spectrum of Nx/2 + 1 doubles to the workspace at
// ((member * nfields + field) * W + w) * (Nx/2 + 1).  W = min(rows, SPECTRA_WMAX): a function of the row count alone, never of the
// device, so the summation order depends on (Nx, rows) only.  A unit is a workgroup of SPECTRA_NT threads from Nx = 512 on; up to
// Nx = 256 a stage has at most 64 butterflies, a unit is one wave, and a workgroup holds SPECTRA_UNITS_SMALL units of consecutive w.
// Pass 2: one thread group per (member, field, k): SPECTRA_P2_G lanes, lane g adds the partials g, g + G, g + 2G, ... one after the
// other, a tree of log2(G) levels through LDS adds the lane sums, the result is divided by rows.  SPECTRA_P2_K values of k per workgroup.
// LDS of a unit: the row (Nx doubles = Nx/2 complex) and the twiddle quarter table (Nx/4 complex): 12 Nx bytes, 48 KiB at Nx = 4096,
// 12 KiB for the four units of a workgroup at Nx = 256.
constexpr int SPECTRA_NT = 256, SPECTRA_WMAX = 256, SPECTRA_MIN_LOG2 = 2, SPECTRA_MAX_LOG2 = 12;
constexpr int SPECTRA_P2_G = 16, SPECTRA_P2_K = 16;
constexpr int SPECTRA_SMALL_NX = 256, SPECTRA_UNITS_SMALL = 4;   // up to SMALL_NX: one wave per row, UNITS_SMALL rows per workgroup
constexpr int SPECTRA_ACC = ((1 << (SPECTRA_MAX_LOG2 - 1)) + SPECTRA_NT) / SPECTRA_NT;   // accumulators of a thread: ceil((Nx/2 + 1) / NT)
struct SpectraPlan {
    int log2n;        // Nx = 2^log2n; -1: Nx is not a supported size
    int W;            // units of pass 1 per (member, field)
    int units;        // units per workgroup: 1, or SPECTRA_UNITS_SMALL up to SPECTRA_SMALL_NX
    int nk;           // Nx/2 + 1
    long blocks1;     // ceil(W / units) * nfields * members
    long blocks2;     // ceil(nk / SPECTRA_P2_K) * nfields * members
    long lds_bytes;   // dynamic LDS of a pass-1 workgroup
    long workspace;   // doubles: W * nfields * members * nk
    int depth;        // D_rows (spectra_depth)
    bool none;        // nothing to compute: no rows, no fields or no members
    bool unsupported; // Nx is not 2^p with SPECTRA_MIN_LOG2 <= p <= SPECTRA_MAX_LOG2
    bool too_many;    // 2^31 workgroups or more in one of the launches
};
inline int spectra_log2(int Nx) {
    for (int p = SPECTRA_MIN_LOG2; p <= SPECTRA_MAX_LOG2; ++p)
        if (Nx == (1 << p)) return p;
    return -1;
}
inline int spectra_W(int rows) { return rows <= 0 ? 0 : (rows < SPECTRA_WMAX ? rows : SPECTRA_WMAX); }
// Rounded additions on the longest path from a p_j[k] to the row sum: workgroup 0 has ceil(rows / W) rows, added one after the other
// starting from 0.0 (the first addition is exact); lane 0 of pass 2 adds ceil(W / G) partials the same way; then one tree level per bit
// of (lanes with a partial - 1) -- a level whose partner holds no partial adds 0.0, which is exact.  The bound of tests/spectra_cases.py.
inline int spectra_depth(int rows) {
    if (rows <= 0) return 0;
    const int W = spectra_W(rows);
    const int serial1 = (int)(((long)rows + W - 1) / W) - 1, serial2 = (W + SPECTRA_P2_G - 1) / SPECTRA_P2_G - 1;
    const int lanes = W < SPECTRA_P2_G ? W : SPECTRA_P2_G;
    int levels = 0;
    while ((1 << levels) < lanes) ++levels;
    return serial1 + serial2 + levels;
}
// members: 1 for a single grid
inline SpectraPlan spectra_plan(int Nx, int rows, int nfields, int members) {
    SpectraPlan p{};
    p.log2n = spectra_log2(Nx);
    p.unsupported = p.log2n < 0;
    p.none = rows <= 0 || nfields <= 0 || members <= 0;
    if (p.unsupported || p.none) return p;
    p.W = spectra_W(rows);
    p.nk = Nx / 2 + 1;
    p.units = Nx <= SPECTRA_SMALL_NX ? SPECTRA_UNITS_SMALL : 1;
    p.blocks1 = (long)((p.W + p.units - 1) / p.units) * nfields * members;
    p.blocks2 = (long)((p.nk + SPECTRA_P2_K - 1) / SPECTRA_P2_K) * nfields * members;
    p.lds_bytes = 12L * Nx * p.units;
    p.workspace = (long)p.W * nfields * members * p.nk;
    p.depth = spectra_depth(rows);
    p.too_many = p.blocks1 >= (1L << 31) || p.blocks2 >= (1L << 31);
    return p;
}

// ---- the three launches of one 2-D / isotropic spectrum call (spectra2d.hip) ---------------------------------------------------------
// Workspace: the complex half-plane, (member, field, kx, j) with j contiguous (2 nkx Ny doubles per member and field, nkx = Nx/2 + 1),
// then, when shells are asked for, the column partials (member, field, kx, s) (nkx NS doubles per member and field).
// Pass 1 (rows): a workgroup of SPECTRA_NT threads takes R consecutive rows of one (member, field), transforms them as the zonal spectra
// do -- one row at a time from Nx = 512 on, SPECTRA_UNITS_SMALL rows side by side, a wave each, up to Nx = 256 -- keeps all R transformed
// rows in LDS and then stores the modes transposed, R x 16 B of one line per store.  R: the largest power of two <= min(S2D_RMAX, Ny)
// whose LDS -- R rows of 8 Nx bytes (+ 16 bytes of padding each where R > 2: the transposed read takes the same element of R rows) and
// one twiddle quarter table of 4 Nx bytes -- stays within min(lds_limit, S2D_ROWS_LDS): 16 rows up to Nx = 512, 8, 4, 2 at 1024, 2048,
// 4096 (80 KiB: two workgroups per CU).
// Pass 2 (columns): one unit per (member, field, kx): a wave up to Ny = 256 (SPECTRA_UNITS_SMALL to a workgroup; the last workgroup may
// hold idle units), a workgroup from Ny = 512 on.  LDS of a unit: the column (16 Ny bytes) and the twiddle quarter table (4 Ny bytes):
// 80 KiB at Ny = 4096.  Fallback, where the device admits less than that per workgroup (lds_limit: its attribute, asked once per
// process): no table, sincospi per butterfly -- the same values bit for bit -- and 16 Ny bytes = 64 KiB.
// Pass 3 (shells): as pass 2 of the zonal spectra: SPECTRA_P2_G lanes per (member, field, s), lane g adds the partials of kx = g, g + G,
// ... one after the other, then a tree; SPECTRA_P2_K shells per workgroup.  Not launched when no shells are asked for.
constexpr int S2D_RMAX = 16;
constexpr long S2D_ROWS_LDS = 80L * 1024, S2D_LDS_MAX = 160L * 1024;
struct Spectra2dPlan {
    int log2nx, log2ny;   // -1: not a supported size
    int nkx, NS;          // Nx/2 + 1; shells (spectra2d_shells)
    int R, pad;           // rows of a pass-1 workgroup; doubles of padding behind each of its rows in LDS
    int units1, units2;   // rows side by side in pass 1; units per workgroup of pass 2
    bool table;           // pass 2 holds a twiddle table in LDS
    long blocks1, blocks2, blocks3;
    long lds1, lds2;      // dynamic LDS of a workgroup of pass 1, pass 2
    long modes, partials; // doubles of the two parts of the workspace (partials: 0 without shells)
    long workspace;       // modes + partials
    bool none;            // nothing to compute: no fields or no members
    bool unsupported;     // Nx or Ny is not 2^p with SPECTRA_MIN_LOG2 <= p <= SPECTRA_MAX_LOG2
    bool too_many;        // 2^31 workgroups or more in one of the launches
};
// the shell of mode (mx, my): include/swmhd_spectra2d.h; two products, one sum, in this order, no contraction
inline int spectra2d_shell(int mx, int my, double wx, double wy) {
    const double a = wx * (double)(mx * mx);
    const double b = wy * (double)(my * my);
    const double r2 = a + b;
    return (int)__builtin_floor(__builtin_sqrt(r2) + 0.5);
}
// NS: one more than the shell of the corner mode (Nx/2, Ny/2); 0 for extents or metrics that are not positive and finite
inline int spectra2d_shells(int Nx, int Ny, double wx, double wy) {
    if (Nx <= 0 || Ny <= 0 || !(wx > 0.0) || !(wy > 0.0) || wx > 1.7e308 || wy > 1.7e308) return 0;
    const double a = wx * ((double)(Nx / 2) * (double)(Nx / 2));   // (as spectra2d_shell; the squares in double: any Nx)
    const double b = wy * ((double)(Ny / 2) * (double)(Ny / 2));
    const double r2 = a + b;
    const double r = __builtin_sqrt(r2) + 0.5;
    return r < 2147483646.0 ? (int)__builtin_floor(r) + 1 : 0;
}
// members: 1 for a single grid; lds_limit: bytes of LDS a workgroup may take on the device
inline Spectra2dPlan spectra2d_plan(int Nx, int Ny, int nfields, int members, double wx, double wy, bool shells, long lds_limit = S2D_LDS_MAX) {
    Spectra2dPlan p{};
    p.log2nx = spectra_log2(Nx);
    p.log2ny = spectra_log2(Ny);
    p.unsupported = p.log2nx < 0 || p.log2ny < 0;
    p.none = nfields <= 0 || members <= 0;
    if (p.unsupported || p.none) return p;
    p.nkx = Nx / 2 + 1;
    p.NS = spectra2d_shells(Nx, Ny, wx, wy);
    const long mf = (long)nfields * members;
    const long budget = lds_limit < S2D_ROWS_LDS ? lds_limit : S2D_ROWS_LDS;
    p.units1 = Nx <= SPECTRA_SMALL_NX ? SPECTRA_UNITS_SMALL : 1;
    for (p.R = S2D_RMAX < Ny ? S2D_RMAX : Ny; ; p.R >>= 1) {
        p.pad = p.R > 2 ? 2 : 0;
        p.lds1 = (long)p.R * 8 * (Nx + p.pad) + 4L * Nx;
        if (p.lds1 <= budget || p.R == 1) break;
    }
    p.blocks1 = (long)(Ny / p.R) * mf;
    p.units2 = Ny <= SPECTRA_SMALL_NX ? SPECTRA_UNITS_SMALL : 1;
    p.table = 20L * Ny * p.units2 <= lds_limit;
    p.lds2 = (p.table ? 20L : 16L) * Ny * p.units2;
    p.blocks2 = (p.nkx * mf + p.units2 - 1) / p.units2;
    p.blocks3 = shells ? (long)((p.NS + SPECTRA_P2_K - 1) / SPECTRA_P2_K) * mf : 0;
    p.modes = 2L * p.nkx * Ny * mf;
    p.partials = shells ? (long)p.nkx * p.NS * mf : 0;
    p.workspace = p.modes + p.partials;
    p.too_many = p.blocks1 >= (1L << 31) || p.blocks2 >= (1L << 31) || p.blocks3 >= (1L << 31);
    return p;
}

// ---- the chunks of one derived-frame call (derived.hip) -----------------------------------------------------------------------------
// One-shot workgroups in address order, as the output frames: a thread takes one 4-cell chunk of one row, a 256-thread workgroup 256
// consecutive chunks of the row-major list of (row, chunk); the member is blockIdx.y.
constexpr int DERIVED_NT = 256, DERIVED_VEC = 4;
struct DerivedPlan {
    int nchunk;       // chunks of one row: the last may be ragged
    long threads;     // rows * nchunk: chunks of one member
    long blocks;      // workgroups of one member (grid x); grid y = members
    int members;
    bool none;        // nothing to compute: no rows or no members
    bool too_many;    // 2^31 workgroups or more: beyond the grid of one launch
};
// members: 1 for a single grid
inline DerivedPlan derived_plan(int Nx, int rows, int members) {
    DerivedPlan p{};
    p.none = Nx <= 0 || rows <= 0 || members <= 0;
    if (p.none) return p;
    p.members = members;
    p.nchunk = (int)(((long)Nx + DERIVED_VEC - 1) / DERIVED_VEC);
    p.threads = (long)rows * p.nchunk;
    p.blocks = (p.threads + DERIVED_NT - 1) / DERIVED_NT;
    p.too_many = p.blocks >= (1L << 31) || p.blocks * members >= (1L << 31);   // (in this order: the product cannot overflow)
    return p;
}

}  // namespace swmhd
