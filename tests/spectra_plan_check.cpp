// Host program: prints the launch plan of the zonal-spectrum kernels (spectra_plan, swmhd_amd/csrc/launch_plan.hpp) for the shapes
// given on the command line, with W and the depth D_rows of the row summation (spectra_depth).  Launches nothing and allocates no device
// memory.  Compiled and run by tests/test_spectra_plan_cpu.py, which compares the lines with what the shape of the kernels implies.
//   spectra_plan_check plan NX ROWS NFIELDS MEMBERS [...]  ->  "plan NX ROWS NFIELDS MEMBERS log2n W units nk blocks1 blocks2 lds_bytes workspace
//                                                               depth none unsupported too_many"
//   spectra_plan_check depth ROWS [ROWS ...]               ->  "depth ROWS W D"
//   spectra_plan_check shape                               ->  "shape NT WMAX P2_G P2_K ACC MIN_LOG2 MAX_LOG2 SMALL_NX UNITS_SMALL"
#include "launch_plan.hpp"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

using namespace swmhd;

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "shape")) {
        printf("shape %d %d %d %d %d %d %d %d %d\n", SPECTRA_NT, SPECTRA_WMAX, SPECTRA_P2_G, SPECTRA_P2_K, SPECTRA_ACC, SPECTRA_MIN_LOG2, SPECTRA_MAX_LOG2,
               SPECTRA_SMALL_NX, SPECTRA_UNITS_SMALL);
        return 0;
    }
    if (argc >= 6 && !strcmp(argv[1], "plan") && (argc - 2) % 4 == 0) {
        for (int k = 2; k + 3 < argc; k += 4) {
            const int Nx = atoi(argv[k]), rows = atoi(argv[k + 1]), nf = atoi(argv[k + 2]), members = atoi(argv[k + 3]);
            const SpectraPlan p = spectra_plan(Nx, rows, nf, members);
            printf("plan %d %d %d %d %d %d %d %d %ld %ld %ld %ld %d %d %d %d\n", Nx, rows, nf, members, p.log2n, p.W, p.units, p.nk, p.blocks1, p.blocks2,
                   p.lds_bytes, p.workspace, p.depth, (int)p.none, (int)p.unsupported, (int)p.too_many);
        }
        return 0;
    }
    if (argc >= 3 && !strcmp(argv[1], "depth")) {
        for (int k = 2; k < argc; ++k) printf("depth %d %d %d\n", atoi(argv[k]), spectra_W(atoi(argv[k])), spectra_depth(atoi(argv[k])));
        return 0;
    }
    fprintf(stderr, "usage: spectra_plan_check shape | plan NX ROWS NFIELDS MEMBERS ... | depth ROWS ...\n");
    return 2;
}
