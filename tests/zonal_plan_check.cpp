// Host program: prints the launch plan of the zonal-mean kernel (zonal_plan, swmhd_amd/csrc/launch_plan.hpp) for the row counts and
// member counts given on the command line, and the depth of its summation tree (zonal_depth) for the row widths given.  Launches nothing
// and allocates no device memory.  Compiled and run by tests/test_zonal_plan_cpu.py, which compares the lines with what the shape of the
// kernel implies.
//   zonal_plan_check plan ROWS MEMBERS [ROWS MEMBERS ...]   ->  "plan ROWS MEMBERS rows_per_block row_blocks blocks none too_many"
//   zonal_plan_check depth NX [NX ...]                      ->  "depth NX D"
//   zonal_plan_check shape                                  ->  "shape NT WAVE VEC ROWS TRIP"
#include "launch_plan.hpp"
#include <stdio.h>
#include <string.h>

using namespace swmhd;

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "shape")) {
        printf("shape %d %d %d %d %d\n", ZONAL_NT, ZONAL_WAVE, ZONAL_VEC, ZONAL_ROWS, ZONAL_TRIP);
        return 0;
    }
    if (argc >= 4 && !strcmp(argv[1], "plan") && argc % 2 == 0) {
        for (int k = 2; k + 1 < argc; k += 2) {
            const int rows = atoi(argv[k]), members = atoi(argv[k + 1]);
            const ZonalPlan p = zonal_plan(rows, members);
            printf("plan %d %d %d %ld %ld %d %d\n", rows, members, p.rows_per_block, p.row_blocks, p.blocks, (int)p.none, (int)p.too_many);
        }
        return 0;
    }
    if (argc >= 3 && !strcmp(argv[1], "depth")) {
        for (int k = 2; k < argc; ++k) printf("depth %d %d\n", atoi(argv[k]), zonal_depth(atoi(argv[k])));
        return 0;
    }
    fprintf(stderr, "usage: zonal_plan_check shape | plan ROWS MEMBERS ... | depth NX ...\n");
    return 2;
}
