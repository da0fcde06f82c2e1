// Host program: builds the launch plans of the tendency, Lorentz operator and tracer kernels (swmhd_amd/csrc/launch_plan.hpp) and
// checks the dispatch sequence of each case against what the launchers enqueued before the plans existed (read off those launchers; the
// same cases were traced on an MI355X, profiles/launch_plan/ and profiles/op_launch_plan/).  Launches nothing and allocates no device
// memory; without a device the CU count is taken as 256, which is the MI355X's, so the numbers hold either way.  Compiled and run by
// tests/test_launch_plan_cpu.py with the SWMHD_* knobs unset, and again as `launch_plan_check op_ly 5` with SWMHD_OP_LY=5 and `op_ly 13` with 13.
#include "launch_plan.hpp"
#include <stdio.h>
#include <string.h>

using namespace swmhd;
using K = TendKernel;

static int failures = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { ++failures; printf("FAILED line %d: %s\n", __LINE__, #cond); } \
    } while (0)

// a stage on an Nx x Ny grid (halo 3), rows [0, Ny), fast build, kernel by size
static TendPlanIn grid(int Nx, int Ny, int elem_size, int formulation) {
    TendPlanIn a{};
    a.Nx = Nx; a.Ny = Ny; a.Hy = 3; a.sy = Nx + 6; a.elem_size = elem_size; a.j1 = Ny; a.formulation = formulation;
    return a;
}
static TendPlanIn stage(TendPlanIn a, int fuse, int first, int store_G, int gm_prev = 0, int anchor = 0) {
    a.fuse = fuse; a.first = first; a.store_G = store_G; a.gm_prev = gm_prev; a.anchor = anchor;
    return a;
}
static bool rows_are(const TendLaunch &l, int j0, int j1, int j0b, int j1b) { return l.j0 == j0 && l.j1 == j1 && l.j0b == j0b && l.j1b == j1b; }
static bool topo_is(const TendLaunch &l, int tx, int ty, int edge) { return l.topo_x == tx && l.topo_y == ty && l.edge_cols == edge; }
static bool march_is(const TendLaunch &l, K k, int nt, int nstrips, int nseg, int LY, int wg, int fold) {
    return l.kernel == k && l.mg.nt == nt && l.mg.nstrips == nstrips && l.mg.nseg == nseg && l.mg.LY == LY && l.mg.wg_per_cu == wg &&
           l.mg.fold == fold;
}
static bool tile_is(const TendLaunch &l, K k, int ntx, int nty) { return l.kernel == k && l.ntx == ntx && l.nty == nty; }
// one marching launch over the whole periodic grid with this stage variant
static bool one_march(const TendPlan &p, K k, int mode, int drop_G) {
    return p.n == 1 && p.e[0].kernel == k && p.e[0].mode == mode && p.e[0].drop_G == drop_G && rows_are(p.e[0], 0, 4096, 0, 0) &&
           topo_is(p.e[0], 0, 0, 0);
}

static void periodic_4096() {
    for (int form = 0; form <= 1; ++form) {
        for (int es = 4; es <= 8; es += 4) {
            const TendPlanIn g = grid(4096, 4096, es, form);
            const bool cons64 = form == 0 && es == 8;
            // anchor form (fast periodic default): W out in stage 1, W in later
            CHECK(one_march(plan_tendency(stage(g, 1, 1, 0, 0, 1)), K::MARCH, 9, 0));
            CHECK(one_march(plan_tendency(stage(g, 1, 0, 0, 0, 1)), K::MARCH, 11, 0));
            // classic G- form: G stored in stages 1 and 2; the last stage of the fp64 conservative model runs the stage-2 variant
            CHECK(one_march(plan_tendency(stage(g, 1, 1, 1)), K::MARCH, 5, 0));
            CHECK(one_march(plan_tendency(stage(g, 1, 0, 1)), K::MARCH, 7, 0));
            CHECK(one_march(plan_tendency(stage(g, 1, 0, 0)), K::MARCH, cons64 ? 7 : 3, cons64 ? 1 : 0));
            // from-state form: no G store in stage 1 (fp64 conservative: on the MODE-5 variant), previous state as the operand later
            CHECK(one_march(plan_tendency(stage(g, 1, 1, 0)), K::MARCH, cons64 ? 5 : 1, cons64 ? 1 : 0));
            CHECK(one_march(plan_tendency(stage(g, 1, 0, 1, 1)), K::MARCH, 7, 0));
            CHECK(one_march(plan_tendency(stage(g, 1, 0, 0, 1)), K::MARCH, 7, 1));
            // tendencies alone
            CHECK(one_march(plan_tendency(stage(g, 0, 0, 0)), K::MARCH, 4, 0));
        }
    }
    // geometries: fp64 vector-invariant folds its 17th strip; fp32 has 4 workgroups per CU; conservative 3 in every RK3 stage variant
    CHECK(march_is(plan_tendency(stage(grid(4096, 4096, 8, 1), 1, 0, 1)).e[0], K::MARCH, 256, 17, 46, 90, 3, 1));
    CHECK(plan_tendency(stage(grid(4096, 4096, 8, 1), 1, 0, 1)).e[0].mg.blocks() == 16 * 46 + 23);
    CHECK(march_is(plan_tendency(stage(grid(4096, 4096, 4, 1), 1, 0, 1)).e[0], K::MARCH, 256, 17, 60, 69, 4, 0));
    CHECK(march_is(plan_tendency(stage(grid(4096, 4096, 8, 0), 1, 0, 1)).e[0], K::MARCH, 256, 17, 45, 92, 3, 0));
    CHECK(march_is(plan_tendency(stage(grid(4096, 4096, 4, 0), 1, 0, 1)).e[0], K::MARCH, 256, 17, 45, 92, 3, 0));
    TendPlanIn room = stage(grid(4096, 4096, 8, 1), 1, 0, 1);
    room.leave_room = 1;
    CHECK(march_is(plan_tendency(room).e[0], K::MARCH, 256, 17, 45, 92, 3, 1));
    // packed fp32: vector-invariant, x read with wrapping, even Nx -- and nothing else
    for (int form = 0; form <= 1; ++form) {
        for (int es = 4; es <= 8; es += 4) {
            for (int wrap = 0; wrap <= 3; ++wrap) {
                for (int Nx = 4095; Nx <= 4096; ++Nx) {
                    TendPlanIn a = stage(grid(Nx, 4096, es, form), 1, 0, 0, 0, 1);
                    a.wrap = wrap;
                    const TendPlan p = plan_tendency(a);
                    const bool packed = form == 1 && es == 4 && (wrap & 1) && Nx == 4096;
                    CHECK(p.n == 1 && p.e[0].kernel == (packed ? K::MARCH_PACKED : K::MARCH) && p.e[0].mode == 11);
                    if (packed) CHECK(march_is(p.e[0], K::MARCH_PACKED, 256, 9, 84, 49, 3, 0));
                }
            }
        }
    }
}

static void bounded_4096() {
    const int B = 1, S = TOPO_OPEN_SOUTH, N = TOPO_OPEN_NORTH;
    TendPlanIn a = stage(grid(4096, 4096, 8, 1), 1, 0, 1);
    a.topo_x = a.topo_y = B;
    TendPlan p = plan_tendency(a);
    CHECK(p.n == 3);
    // the body: the periodic plan's launch, periodic topology
    CHECK(march_is(p.e[0], K::MARCH, 256, 17, 46, 90, 3, 1) && p.e[0].mode == 7 && rows_are(p.e[0], 0, 4096, 0, 0) && topo_is(p.e[0], 0, 0, 0));
    // the y frame: 8 + 8 rows in one two-range launch of the wall kernel over all 64 tile columns
    CHECK(tile_is(p.e[1], K::TILE_BOUNDED, 64, 2) && rows_are(p.e[1], 0, 8, 4088, 4096) && topo_is(p.e[1], B, B, 0));
    // the x frame: tile columns 0 and 63 over all rows
    CHECK(tile_is(p.e[2], K::TILE_BOUNDED, 2, 512) && rows_are(p.e[2], 0, 4096, 0, 0) && topo_is(p.e[2], B, B, 1));
    // slabs of a chain: no frame rows along a cut
    a.topo_y = B | S;
    p = plan_tendency(a);
    CHECK(p.n == 3 && tile_is(p.e[1], K::TILE_BOUNDED, 64, 1) && rows_are(p.e[1], 4088, 4096, 0, 0) && topo_is(p.e[1], B, B | S, 0));
    CHECK(topo_is(p.e[0], 0, 0, 0) && tile_is(p.e[2], K::TILE_BOUNDED, 2, 512) && topo_is(p.e[2], B, B | S, 1));
    a.topo_y = B | N;
    p = plan_tendency(a);
    CHECK(p.n == 3 && tile_is(p.e[1], K::TILE_BOUNDED, 64, 1) && rows_are(p.e[1], 0, 8, 0, 0) && topo_is(p.e[1], B, B | N, 0));
    a.topo_y = B | S | N;
    p = plan_tendency(a);
    CHECK(p.n == 2 && p.e[0].kernel == K::MARCH && tile_is(p.e[1], K::TILE_BOUNDED, 2, 512) && topo_is(p.e[1], B, B | S | N, 1));
    a.topo_x = 0;
    p = plan_tendency(a);
    CHECK(p.n == 1 && march_is(p.e[0], K::MARCH, 256, 17, 46, 90, 3, 1) && topo_is(p.e[0], 0, 0, 0));
    // (Periodic, Bounded): body and y frame; (Bounded, Periodic): body and x frame; a narrow last tile column takes the last two
    a.topo_y = B;
    p = plan_tendency(a);
    CHECK(p.n == 2 && tile_is(p.e[1], K::TILE_BOUNDED, 64, 2) && rows_are(p.e[1], 0, 8, 4088, 4096) && topo_is(p.e[1], 0, B, 0));
    TendPlanIn w = stage(grid(4100, 4096, 8, 0), 1, 0, 1);
    w.topo_x = B;
    p = plan_tendency(w);
    CHECK(p.n == 2 && p.e[0].kernel == K::MARCH && p.e[0].mode == 7 && tile_is(p.e[1], K::TILE_BOUNDED, 3, 512) && topo_is(p.e[1], B, 0, 1));
    CHECK(frame_tile_columns(4096) == 2 && frame_tile_columns(4100) == 3 && frame_tile_columns(4104) == 2 && frame_tile_columns(64) == 1);
    // a slab further from the walls than the frame: nothing of the y frame is its own
    const BoundedFrame f = bounded_frame(4096, 1024, 2048, 0, B);
    CHECK(f.s1 <= f.s0 && f.n1 <= f.n0 && !f.x_walls);
    // below the thresholds of the hybrid launch, forced, strict or with a caller's own frame: the wall kernel alone
    TendPlanIn s = stage(grid(128, 4096, 8, 1), 1, 0, 1);
    s.topo_x = s.topo_y = B;
    p = plan_tendency(s);
    CHECK(p.n == 1 && tile_is(p.e[0], K::TILE_BOUNDED, 2, 512) && topo_is(p.e[0], B, B, 0));
    s = stage(grid(16384, 40, 8, 1), 1, 0, 1);
    s.topo_y = B;
    p = plan_tendency(s);
    CHECK(p.n == 1 && tile_is(p.e[0], K::TILE_BOUNDED, 256, 5));
    s = stage(grid(512, 512, 8, 0), 1, 0, 1);
    s.topo_x = B;
    p = plan_tendency(s);
    CHECK(p.n == 1 && tile_is(p.e[0], K::TILE_BOUNDED, 8, 64) && rows_are(p.e[0], 0, 512, 0, 0));
    a.topo_x = a.topo_y = B;
    a.kernel_variant = 1;
    p = plan_tendency(a);
    CHECK(p.n == 1 && tile_is(p.e[0], K::TILE_BOUNDED, 64, 512));
    a.kernel_variant = 2;   // (the marching kernels have no walls)
    CHECK(plan_tendency(a).n == 1 && plan_tendency(a).e[0].kernel == K::TILE_BOUNDED);
    a.kernel_variant = 0;
    a.strict = true;
    p = plan_tendency(a);
    CHECK(p.n == 1 && tile_is(p.e[0], K::TILE_BOUNDED, 64, 512));
    a.strict = false;
    a.edge_cols = 1;
    p = plan_tendency(a);
    CHECK(p.n == 1 && tile_is(p.e[0], K::TILE_BOUNDED, 2, 512) && topo_is(p.e[0], B, B, 1));
}

static void ranges_and_sizes() {
    // a slab's two zones in one marching launch: segments of both ranges, same LY, full strips
    TendPlanIn a = stage(grid(4096, 4096, 8, 1), 1, 0, 0, 0, 1);
    a.j0 = 0; a.j1 = 1024; a.j0b = 3072; a.j1b = 4096;
    TendPlan p = plan_tendency(a);
    CHECK(p.n == 1 && march_is(p.e[0], K::MARCH, 256, 17, 23 + 23, 46, 3, 0) && rows_are(p.e[0], 0, 1024, 3072, 4096));
    a.j1 = 1000;   // 22 segments of 46 rows = 1012 >= 1000, and 23 for the second range
    p = plan_tendency(a);
    CHECK(p.n == 1 && p.e[0].mg.fold == 0 && p.e[0].mg.nseg == (1000 + p.e[0].mg.LY - 1) / p.e[0].mg.LY + (1024 + p.e[0].mg.LY - 1) / p.e[0].mg.LY);
    // the thin boundary strips of a slab: one launch of 64 x 4 tiles, tile rows of the second range after those of the first
    a.j0 = 0; a.j1 = 6; a.j0b = 4090; a.j1b = 4096;
    p = plan_tendency(a);
    CHECK(p.n == 1 && tile_is(p.e[0], K::TILE_RY1, 64, 2 + 2) && rows_are(p.e[0], 0, 6, 4090, 4096));
    // an empty first range: the second alone, as a single range (so it may fold)
    a.j0 = 5; a.j1 = 5; a.j0b = 0; a.j1b = 4096;
    p = plan_tendency(a);
    CHECK(p.n == 1 && march_is(p.e[0], K::MARCH, 256, 17, 46, 90, 3, 1) && rows_are(p.e[0], 0, 4096, 0, 0));
    a.j0 = 7; a.j1 = 2;
    p = plan_tendency(a);
    CHECK(p.n == 1 && rows_are(p.e[0], 0, 4096, 0, 0) && p.e[0].mg.fold == 1);
    // nothing to do
    a.j0b = a.j1b = 0;
    CHECK(plan_tendency(a).n == 0);
    // a parent of 4 GiB or more stays on the tile kernel (32-bit byte offsets in the marching kernels), forced or not
    TendPlanIn big = stage(grid(32768, 16384, 8, 1), 1, 0, 1);
    p = plan_tendency(big);
    CHECK(p.n == 1 && tile_is(p.e[0], K::TILE_RY2, 512, 2048));
    big.kernel_variant = 2;
    CHECK(plan_tendency(big).e[0].kernel == K::TILE_RY2);
    // ... and one whose last row ends within 4 GiB but the row after does not keeps full strips
    TendPlanIn edge = stage(grid(4096, 130874, 8, 1), 1, 0, 1);   // (130874 + 6) rows x 4102 x 8 B = 2^32 - 9216 B; one more row of 32816 B passes 2^32 - 64
    p = plan_tendency(edge);
    CHECK(p.n == 1 && p.e[0].kernel == K::MARCH && p.e[0].mg.nstrips == 17 && p.e[0].mg.fold == 0);
    // by size: 64 x 4 tiles below 330000 cells, marching from there; forced either way
    TendPlanIn sm = stage(grid(128, 128, 8, 1), 1, 0, 1);
    p = plan_tendency(sm);
    CHECK(p.n == 1 && tile_is(p.e[0], K::TILE_RY1, 2, 32) && topo_is(p.e[0], 0, 0, 0));
    sm.kernel_variant = 1;   // forced tile on a small grid: still 64 x 4
    CHECK(tile_is(plan_tendency(sm).e[0], K::TILE_RY1, 2, 32));
    sm.kernel_variant = 2;
    CHECK(plan_tendency(sm).e[0].kernel == K::MARCH);
    sm.kernel_variant = 0;
    sm.strict = true;
    CHECK(tile_is(plan_tendency(sm).e[0], K::TILE_RY2, 2, 16));
    CHECK(plan_tendency(stage(grid(574, 574, 8, 0), 1, 0, 1)).e[0].kernel == K::TILE_RY1);   // 329476 cells
    CHECK(plan_tendency(stage(grid(575, 574, 8, 0), 1, 0, 1)).e[0].kernel == K::MARCH);      // 330050
    TendPlanIn t = stage(grid(4096, 4096, 8, 1), 1, 0, 1);
    t.kernel_variant = 1;
    CHECK(tile_is(plan_tendency(t).e[0], K::TILE_RY2, 64, 512));
    t.kernel_variant = 0;
    t.strict = true;
    CHECK(plan_tendency(t).n == 1 && tile_is(plan_tendency(t).e[0], K::TILE_RY2, 64, 512));
}

static void ensembles() {
    auto member = [](int N, bool strict, int topo) {
        TendPlanIn a = stage(grid(N, N, 8, 1), 1, 0, 1);
        a.strict = strict; a.topo_x = a.topo_y = topo; a.members = 256;
        return plan_tendency(a);
    };
    // the tile of a single model of the member's size; never the marching kernel, never a frame
    CHECK(member(64, false, 0).n == 1 && tile_is(member(64, false, 0).e[0], K::TILE_RY1, 1, 16));
    CHECK(member(64, true, 0).n == 1 && tile_is(member(64, true, 0).e[0], K::TILE_RY2, 1, 8));
    CHECK(member(1024, false, 0).n == 1 && tile_is(member(1024, false, 0).e[0], K::TILE_RY2, 16, 128));
    CHECK(member(1024, true, 0).n == 1 && tile_is(member(1024, true, 0).e[0], K::TILE_RY2, 16, 128));
    CHECK(member(64, false, 1).n == 1 && tile_is(member(64, false, 1).e[0], K::TILE_BOUNDED, 1, 8));
    CHECK(member(64, true, 1).n == 1 && tile_is(member(64, true, 1).e[0], K::TILE_BOUNDED, 1, 8));
    CHECK(member(1024, false, 1).n == 1 && tile_is(member(1024, false, 1).e[0], K::TILE_BOUNDED, 16, 128));
}

static void query() {
    int o[8];
    // the report is the plan's first launch: forced tile below 330000 cells is 64 x 4 in fast builds, 64 x 8 in strict ones
    CHECK(tendency_launch_geometry(128, 128, 1, 8, false, 1, 0, 0, o) == 0 && o[0] == 1 && o[2] == 2 && o[3] == 32 && o[4] == 4);
    CHECK(tendency_launch_geometry(128, 128, 1, 8, true, 0, 0, 0, o) == 0 && o[0] == 1 && o[2] == 2 && o[3] == 16 && o[4] == 8);
    CHECK(tendency_launch_geometry(4096, 4096, 1, 8, false, 0, 0, 0, o) == 0 && o[0] == 2 && o[1] == 256 && o[2] == 17 && o[3] == 46 &&
          o[4] == 90 && o[5] == 3 && o[6] == 3 && o[7] == 256);
    CHECK(tendency_launch_geometry(4096, 4096, 1, 4, false, 0, 0, 1, o) == 0 && o[0] == 3 && o[2] == 9 && o[6] == 2);
}

// ---- Lorentz operators (plan_lorentz) ------------------------------------------------------------------------------------------------
// an operator call on an Nx x Ny grid, rows [0, Ny), fast build, kernel by size, periodic
static OpPlanIn op(int Nx, int Ny, bool divergence, int topo_x = 0, int topo_y = 0) {
    OpPlanIn a{};
    a.Nx = Nx; a.Ny = Ny; a.j1 = Ny; a.divergence = divergence; a.topo_x = topo_x; a.topo_y = topo_y;
    return a;
}
// a marching launch: 256 lanes, no fold, 6 (Jacobian) / 5 (divergence) workgroups per CU
static bool op_march_is(const OpLaunch &l, int nstrips, int nseg, int LY, int wg) {
    return l.kernel == OpKernel::MARCH && l.mg.nt == 256 && l.mg.nstrips == nstrips && l.mg.nseg == nseg && l.mg.LY == LY &&
           l.mg.wg_per_cu == wg && l.mg.fold == 0 && l.mg.blocks() == nstrips * nseg;
}
static bool op_tile_is(const OpLaunch &l, int ntx, int nty) { return l.kernel == OpKernel::TILE && l.ntx == ntx && l.nty == nty; }
static bool op_args_are(const OpLaunch &l, int j0, int j1, int tx, int ty, int edge) {
    return l.j0 == j0 && l.j1 == j1 && l.topo_x == tx && l.topo_y == ty && l.edge_cols == edge;
}
// the wall tile kernel alone, over the caller's rows with the caller's topology
static bool wall_tile_alone(const OpPlanIn &a, int ntx) {
    const OpPlan p = plan_lorentz(a);
    return p.n == 1 && op_tile_is(p.e[0], ntx, (a.j1 - a.j0 + 7) / 8) && op_args_are(p.e[0], a.j0, a.j1, a.topo_x, a.topo_y, a.edge_cols);
}

static void operators_periodic() {
    OpPlan p = plan_lorentz(op(4096, 4096, false));
    CHECK(p.n == 1 && op_march_is(p.e[0], 17, 90, 46, 6) && op_args_are(p.e[0], 0, 4096, 0, 0, 0));
    p = plan_lorentz(op(4096, 4096, true));
    CHECK(p.n == 1 && op_march_is(p.e[0], 17, 75, 55, 5) && op_args_are(p.e[0], 0, 4096, 0, 0, 0));
    p = plan_lorentz(op(16384, 2048, false));
    CHECK(p.n == 1 && op_march_is(p.e[0], 66, 23, 90, 6));
    p = plan_lorentz(op(16384, 2048, true));
    CHECK(p.n == 1 && op_march_is(p.e[0], 66, 19, 108, 5));
    // the Jacobian form's cross-over, 2 000 000 cells: 64 x 16 tiles below it
    p = plan_lorentz(op(1415, 1414, false));   // 2 000 810
    CHECK(p.n == 1 && op_march_is(p.e[0], 6, 177, 8, 6));
    p = plan_lorentz(op(1414, 1414, false));   // 1 999 396
    CHECK(p.n == 1 && op_tile_is(p.e[0], 23, 89) && op_args_are(p.e[0], 0, 1414, 0, 0, 0));
    // the divergence form's, 900 000 cells: 64 x 8 tiles below it
    p = plan_lorentz(op(1000, 900, true));
    CHECK(p.n == 1 && op_march_is(p.e[0], 4, 113, 8, 5));
    p = plan_lorentz(op(999, 900, true));
    CHECK(p.n == 1 && op_tile_is(p.e[0], 16, 113));
    // the cells counted are those of the row range
    OpPlanIn r = op(4096, 4096, false);
    r.j0 = 100; r.j1 = 588;   // 488 rows: 1 998 848 cells
    p = plan_lorentz(r);
    CHECK(p.n == 1 && op_tile_is(p.e[0], 64, 31) && op_args_are(p.e[0], 100, 588, 0, 0, 0));
    r.j1 = 589;               // 2 002 944: one round of 90 segments, 6 rows each, raised to the minimum of 8
    p = plan_lorentz(r);
    CHECK(p.n == 1 && op_march_is(p.e[0], 17, 62, 8, 6) && op_args_are(p.e[0], 100, 589, 0, 0, 0));
    // forced either way; strict builds have the tile kernels only
    for (int div = 0; div <= 1; ++div) {
        OpPlanIn f = op(4096, 4096, div != 0);
        f.kernel_variant = 1;
        p = plan_lorentz(f);
        CHECK(p.n == 1 && op_tile_is(p.e[0], 64, div ? 512 : 256));
        f.kernel_variant = 0;
        f.strict = true;
        p = plan_lorentz(f);
        CHECK(p.n == 1 && op_tile_is(p.e[0], 64, div ? 512 : 256));
        f.kernel_variant = 2;
        CHECK(plan_lorentz(f).n == 1 && plan_lorentz(f).e[0].kernel == OpKernel::TILE);
        OpPlanIn s = op(128, 128, div != 0);
        s.kernel_variant = 2;   // 1 strip, 1536 | 1280 slots: 128 segments of 1 row, raised to 8
        p = plan_lorentz(s);
        CHECK(p.n == 1 && op_march_is(p.e[0], 1, 16, 8, div ? 5 : 6));
        s.kernel_variant = 0;
        p = plan_lorentz(s);
        CHECK(p.n == 1 && op_tile_is(p.e[0], 2, div ? 16 : 8));
    }
    // the Jacobian form has no walls: topology and edge_cols pass through and change nothing
    OpPlanIn j = op(4096, 4096, false, 1, 1);
    j.edge_cols = 1;
    p = plan_lorentz(j);
    CHECK(p.n == 1 && op_march_is(p.e[0], 17, 90, 46, 6) && op_args_are(p.e[0], 0, 4096, 1, 1, 1));
    j.kernel_variant = 1;
    p = plan_lorentz(j);
    CHECK(p.n == 1 && op_tile_is(p.e[0], 64, 256) && op_args_are(p.e[0], 0, 4096, 1, 1, 1));
    // at most 16 rounds of resident workgroups are tried: 2 strips, 1536 slots -> 768 k segments in round k.  1 600 000 rows need
    // 131 rows per segment in round 16 and 123 in round 17, so the fall-back of 32 rows holds; 1 572 864 = 16 x 768 x 128 still fits
    p = plan_lorentz(op(256, 1600000, false));
    CHECK(p.n == 1 && op_march_is(p.e[0], 2, 50000, 32, 6));
    p = plan_lorentz(op(256, 1572864, false));
    CHECK(p.n == 1 && op_march_is(p.e[0], 2, 12288, 128, 6));
    // nothing to do
    OpPlanIn e = op(4096, 4096, true);
    e.j0 = e.j1 = 7;
    CHECK(plan_lorentz(e).n == 0);
    e.j0 = 9;
    CHECK(plan_lorentz(e).n == 0);
    CHECK(plan_lorentz(op(0, 4096, true)).n == 0 && plan_lorentz(op(0, 4096, false)).n == 0 && plan_lorentz(op(64, 0, false)).n == 0);
}

static void operators_bounded() {
    const int B = 1;
    // the hybrid: periodic body, south strip, north strip, x frame (1300 = 20 x 64 + 20: two frame tile columns)
    OpPlan p = plan_lorentz(op(1300, 800, true, B, B));
    CHECK(p.n == 4);
    CHECK(op_march_is(p.e[0], 6, 100, 8, 5) && op_args_are(p.e[0], 0, 800, 0, 0, 0));
    CHECK(op_tile_is(p.e[1], 21, 1) && op_args_are(p.e[1], 0, 8, B, B, 0));
    CHECK(op_tile_is(p.e[2], 21, 1) && op_args_are(p.e[2], 792, 800, B, B, 0));
    CHECK(op_tile_is(p.e[3], 2, 100) && op_args_are(p.e[3], 0, 800, B, B, 1));
    p = plan_lorentz(op(1300, 800, true, 0, B));
    CHECK(p.n == 3 && op_march_is(p.e[0], 6, 100, 8, 5) && op_args_are(p.e[0], 0, 800, 0, 0, 0));
    CHECK(op_tile_is(p.e[1], 21, 1) && op_args_are(p.e[1], 0, 8, 0, B, 0) && op_tile_is(p.e[2], 21, 1) && op_args_are(p.e[2], 792, 800, 0, B, 0));
    p = plan_lorentz(op(1300, 800, true, B, 0));
    CHECK(p.n == 2 && op_march_is(p.e[0], 6, 100, 8, 5) && op_args_are(p.e[0], 0, 800, 0, 0, 0));
    CHECK(op_tile_is(p.e[1], 2, 100) && op_args_are(p.e[1], 0, 800, B, 0, 1));
    // a row range that ends below the north strip, on a grid whose last tile column is 4 wide: no north launch, three frame columns
    OpPlanIn a = op(1284, 800, true, B, B);
    a.j0 = 5; a.j1 = 790;
    p = plan_lorentz(a);
    CHECK(p.n == 3 && op_march_is(p.e[0], 6, 99, 8, 5) && op_args_are(p.e[0], 5, 790, 0, 0, 0));
    CHECK(op_tile_is(p.e[1], 21, 1) && op_args_are(p.e[1], 5, 8, B, B, 0));
    CHECK(op_tile_is(p.e[2], 3, 99) && op_args_are(p.e[2], 5, 790, B, B, 1));
    // at the edge of all three thresholds at once (>= 900 000 cells, Nx >= 256, Ny >= 48): 18752 x 48 = 900 096 cells
    p = plan_lorentz(op(18752, 48, true, B, B));
    CHECK(p.n == 4 && op_march_is(p.e[0], 76, 6, 8, 5) && op_tile_is(p.e[1], 293, 1) && op_args_are(p.e[1], 0, 8, B, B, 0) &&
          op_tile_is(p.e[2], 293, 1) && op_args_are(p.e[2], 40, 48, B, B, 0) && op_tile_is(p.e[3], 2, 6) && op_args_are(p.e[3], 0, 48, B, B, 1));
    p = plan_lorentz(op(18750, 48, true, B, B));              // 900 000 cells exactly
    CHECK(p.n == 4 && op_march_is(p.e[0], 75, 6, 8, 5) && op_tile_is(p.e[1], 293, 1) && op_tile_is(p.e[3], 2, 6));
    CHECK(plan_lorentz(op(18751, 48, true, B, B)).n == 4);    // 900 048
    CHECK(wall_tile_alone(op(18749, 48, true, B, B), 293));   // 899 952 cells
    CHECK(wall_tile_alone(op(18752, 47, true, B, B), 293));   // Ny < 48 (881 344 cells; 19149 x 47 = 900 003 below)
    CHECK(wall_tile_alone(op(19149, 47, true, B, B), 300));
    CHECK(wall_tile_alone(op(255, 4096, true, B, B), 4));     // Nx < 256 (1 044 480 cells)
    CHECK(wall_tile_alone(op(255, 4096, true, 0, B), 4) && wall_tile_alone(op(255, 4096, true, B, 0), 4));
    // forced, strict or with a caller's own frame: the wall tile kernel alone
    a = op(1300, 800, true, B, B);
    a.kernel_variant = 1;
    CHECK(wall_tile_alone(a, 21));
    a.kernel_variant = 2;   // (the marching kernel has no walls)
    CHECK(wall_tile_alone(a, 21));
    a.kernel_variant = 0;
    a.strict = true;
    CHECK(wall_tile_alone(a, 21));
    a.strict = false;
    a.edge_cols = 1;
    CHECK(wall_tile_alone(a, 2));
    a.Nx = 1284;
    CHECK(wall_tile_alone(a, 3));
    // a y-slab's open sides count as Bounded and have no frame rows
    p = plan_lorentz(op(1300, 800, true, 0, B | TOPO_OPEN_SOUTH));
    CHECK(p.n == 2 && p.e[0].kernel == OpKernel::MARCH && op_tile_is(p.e[1], 21, 1) && op_args_are(p.e[1], 792, 800, 0, B | TOPO_OPEN_SOUTH, 0));
}

// ---- the shapes of the operator call matrix (tests/operator_cases.py) -------------------------------------------------------------
// What every shape of the matrix lands on, so that "one column and one row below, at and above a workgroup" is a fact about the plan:
// strips of 252 | 250 output columns x segments of 8 rows on the march path (SWMHD_MARCH_KERNEL: kernel_variant 2), tiles of
// 64 x 16 | 64 x 8 on the tile, strict and wall paths.
struct MatrixShape { int Nx, Ny, nx, ny, ny_inner; };   // strips | tile columns, segments | tile rows over all rows and over rows [1, Ny - 1)
static OpPlanIn matrix_op(int Nx, int Ny, bool div, int variant, bool strict, int tx, int ty, int j0, int j1) {
    OpPlanIn a = op(Nx, Ny, div, tx, ty);
    a.kernel_variant = variant; a.strict = strict; a.j0 = j0; a.j1 = j1;
    return a;
}
static void operators_matrix() {
    CHECK(OP_MARCH_NT == 256 && OP_MARCH_LY_MIN == 8 && TILE_X == 64 && OP_JAC_TILE_Y == 16 && OP_DIV_TILE_Y == 8);
    // march: (1,1) (2,3) (5,4) (W-1,R-1) (W,R) (W+1,R+1) (2W+1,2R+1), W = 252 | 250, R = 8: a small grid forced onto the marching
    // kernels has segments of the minimum of 8 rows
    const MatrixShape jm[7] = {{1, 1, 1, 1, 0}, {2, 3, 1, 1, 1}, {5, 4, 1, 1, 1}, {251, 7, 1, 1, 1}, {252, 8, 1, 1, 1}, {253, 9, 2, 2, 1}, {505, 17, 3, 3, 2}};
    const MatrixShape dm[7] = {{1, 1, 1, 1, 0}, {2, 3, 1, 1, 1}, {5, 4, 1, 1, 1}, {249, 7, 1, 1, 1}, {250, 8, 1, 1, 1}, {251, 9, 2, 2, 1}, {501, 17, 3, 3, 2}};
    for (int div = 0; div <= 1; ++div) {
        for (int k = 0; k < 7; ++k) {
            const MatrixShape &m = div ? dm[k] : jm[k];
            OpPlan p = plan_lorentz(matrix_op(m.Nx, m.Ny, div != 0, 2, false, 0, 0, 0, m.Ny));
            CHECK(p.n == 1 && op_march_is(p.e[0], m.nx, m.ny, 8, div ? 5 : 6) && op_args_are(p.e[0], 0, m.Ny, 0, 0, 0));
            p = plan_lorentz(matrix_op(m.Nx, m.Ny, div != 0, 2, false, 0, 0, 1, m.Ny - 1 > 1 ? m.Ny - 1 : 1));
            CHECK(m.ny_inner ? p.n == 1 && op_march_is(p.e[0], m.nx, m.ny_inner, 8, div ? 5 : 6) : p.n == 0);
        }
        // the phase sweep: (W + 1, 21), rows [j0, j0 + 9): two strips, the second one column wide; a full segment and one of one row
        for (int j0 = 0; j0 < 12; ++j0) {
            const OpPlan p = plan_lorentz(matrix_op(div ? 251 : 253, 21, div != 0, 2, false, 0, 0, j0, j0 + 9));
            CHECK(p.n == 1 && op_march_is(p.e[0], 2, 2, 8, div ? 5 : 6) && op_args_are(p.e[0], j0, j0 + 9, 0, 0, 0));
        }
    }
    // tile and strict: the same seven around 64 x 16 | 64 x 8, and (129, 9)
    const MatrixShape jt[8] = {{1, 1, 1, 1, 0}, {2, 3, 1, 1, 1}, {5, 4, 1, 1, 1}, {63, 15, 1, 1, 1}, {64, 16, 1, 1, 1}, {65, 17, 2, 2, 1}, {129, 33, 3, 3, 2}, {129, 9, 3, 1, 1}};
    const MatrixShape dt[8] = {{1, 1, 1, 1, 0}, {2, 3, 1, 1, 1}, {5, 4, 1, 1, 1}, {63, 7, 1, 1, 1}, {64, 8, 1, 1, 1}, {65, 9, 2, 2, 1}, {129, 17, 3, 3, 2}, {129, 9, 3, 2, 1}};
    for (int div = 0; div <= 1; ++div) {
        for (int strict = 0; strict <= 1; ++strict) {
            for (int k = 0; k < 8; ++k) {
                const MatrixShape &m = div ? dt[k] : jt[k];
                OpPlan p = plan_lorentz(matrix_op(m.Nx, m.Ny, div != 0, strict ? 0 : 1, strict != 0, 0, 0, 0, m.Ny));
                CHECK(p.n == 1 && op_tile_is(p.e[0], m.nx, m.ny) && op_args_are(p.e[0], 0, m.Ny, 0, 0, 0));
                p = plan_lorentz(matrix_op(m.Nx, m.Ny, div != 0, strict ? 0 : 1, strict != 0, 0, 0, 1, m.Ny - 1 > 1 ? m.Ny - 1 : 1));
                CHECK(m.ny_inner ? p.n == 1 && op_tile_is(p.e[0], m.nx, m.ny_inner) : p.n == 0);
            }
        }
    }
    // wall and wall-strict: (4,3) and (7,9) in place of the three tiny shapes; the wall tile kernel alone with the caller's topology
    const MatrixShape dw[7] = {{4, 3, 1, 1, 1}, {7, 9, 1, 2, 1}, {63, 7, 1, 1, 1}, {64, 8, 1, 1, 1}, {65, 9, 2, 2, 1}, {129, 17, 3, 3, 2}, {129, 9, 3, 2, 1}};
    const int topos[3][2] = {{1, 1}, {1, 0}, {0, 1}};
    for (int t = 0; t < 3; ++t) {
        for (int strict = 0; strict <= 1; ++strict) {
            for (int k = 0; k < 7; ++k) {
                const MatrixShape &m = dw[k];
                const OpPlanIn a = matrix_op(m.Nx, m.Ny, true, strict ? 0 : 1, strict != 0, topos[t][0], topos[t][1], 0, m.Ny);
                CHECK(wall_tile_alone(a, m.nx) && plan_lorentz(a).e[0].nty == m.ny);
                const OpPlanIn b = matrix_op(m.Nx, m.Ny, true, strict ? 0 : 1, strict != 0, topos[t][0], topos[t][1], 1, m.Ny - 1);
                CHECK(wall_tile_alone(b, m.nx) && plan_lorentz(b).e[0].nty == m.ny_inner);
            }
        }
    }
}

// SWMHD_OP_LY = ly (a process of its own: the knob is read once): that many rows per segment, even below the minimum of 8 -- on a large
// grid and on the sweep grid of the operator matrix (all 21 rows and rows [j0, j0 + 9))
static void operators_forced_ly(int ly) {
    for (int div = 0; div <= 1; ++div) {
        OpPlan p = plan_lorentz(op(4096, 4096, div != 0));
        CHECK(p.n == 1 && op_march_is(p.e[0], 17, (4096 + ly - 1) / ly, ly, div ? 5 : 6));
        p = plan_lorentz(matrix_op(div ? 251 : 253, 21, div != 0, 2, false, 0, 0, 0, 21));
        CHECK(p.n == 1 && op_march_is(p.e[0], 2, (21 + ly - 1) / ly, ly, div ? 5 : 6));
        p = plan_lorentz(matrix_op(div ? 251 : 253, 21, div != 0, 2, false, 0, 0, 7, 16));
        CHECK(p.n == 1 && op_march_is(p.e[0], 2, (9 + ly - 1) / ly, ly, div ? 5 : 6));
    }
}

// ---- tracers (tracer_tiles) ------------------------------------------------------------------------------------------------------------
static bool tiles_are(const TracerTiles &t, int ntx, int nty, long blocks) {
    return !t.none && !t.too_many && t.ntx == ntx && t.nty == nty && t.blocks == blocks;
}
static void tracers() {
    CHECK(TRACER_TILE_X == 64 && TRACER_TILE_Y == 16);
    // one grid: both directions round up
    CHECK(tiles_are(tracer_tiles(65, 17, 3, 1), 2, 2, 4));
    CHECK(tiles_are(tracer_tiles(64, 16, 1, 1), 1, 1, 1));
    CHECK(tiles_are(tracer_tiles(63, 15, 1, 1), 1, 1, 1));
    CHECK(tiles_are(tracer_tiles(4096, 4095, 8, 1), 64, 256, 16384) && tiles_are(tracer_tiles(4096, 4097, 8, 1), 64, 257, 16448));
    // an ensemble: the tiles of every member
    CHECK(tiles_are(tracer_tiles(65, 17, 3, 3), 2, 2, 12));
    CHECK(tiles_are(tracer_tiles(4096, 8192, 1, 65535), 64, 512, 2147450880L));
    const TracerTiles big = tracer_tiles(4096, 8193, 1, 65535);   // 64 x 513 x 65535 = 2 151 645 120 >= 2^31
    CHECK(!big.none && big.too_many && big.blocks == 2151645120L);
    CHECK(tracer_tiles(64, 64, 1, 1 << 29).too_many && !tracer_tiles(64, 64, 1, (1 << 29) - 1).too_many);   // 4 tiles: 2^31 | 2^31 - 4
    // nothing to do: no tracers, no rows, no members
    CHECK(tracer_tiles(64, 64, 0, 4).none && tracer_tiles(64, 0, 2, 4).none && tracer_tiles(64, -3, 2, 1).none && tracer_tiles(64, 64, 2, 0).none);
}

int main(int argc, char **argv) {
    CHECK(device_cu_count() == 256);
    if (argc == 3 && !strcmp(argv[1], "op_ly")) {
        operators_forced_ly(atoi(argv[2]));
        printf(failures ? "%d plan checks FAILED\n" : "launch plans OK\n", failures);
        return failures ? 1 : 0;
    }
    CHECK(is_bounded(1, 0) && is_bounded(0, 1) && is_bounded(0, 1 | TOPO_OPEN_SOUTH | TOPO_OPEN_NORTH) && !is_bounded(0, 0));
    periodic_4096();
    bounded_4096();
    ranges_and_sizes();
    ensembles();
    query();
    operators_periodic();
    operators_bounded();
    operators_matrix();
    tracers();
    printf(failures ? "%d plan checks FAILED\n" : "launch plans OK\n", failures);
    return failures ? 1 : 0;
}
