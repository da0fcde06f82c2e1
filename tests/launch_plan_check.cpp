// Host program: builds tendency launch plans (swmhd_amd/csrc/launch_plan.hpp) and checks the dispatch sequence of each case against
// what the launcher enqueued before the plan existed (read off that launcher; the same cases were traced on an MI355X,
// profiles/launch_plan/).  Launches nothing and allocates no device memory; without a device the CU count is taken as 256, which is the
// MI355X's, so the numbers hold either way.  Compiled and run by tests/test_launch_plan_cpu.py with the SWMHD_* knobs unset.
#include "launch_plan.hpp"
#include <stdio.h>

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

int main() {
    CHECK(device_cu_count() == 256);
    CHECK(is_bounded(1, 0) && is_bounded(0, 1) && is_bounded(0, 1 | TOPO_OPEN_SOUTH | TOPO_OPEN_NORTH) && !is_bounded(0, 0));
    periodic_4096();
    bounded_4096();
    ranges_and_sizes();
    ensembles();
    query();
    printf(failures ? "%d plan checks FAILED\n" : "launch plans OK\n", failures);
    return failures ? 1 : 0;
}
