// Host program: prints the launch plan of the 2-D / isotropic spectrum kernels (spectra2d_plan, swmhd_amd/csrc/launch_plan.hpp) for the
// shapes given on the command line.  Launches nothing and allocates no device memory.  Compiled and run by
// tests/test_spectra2d_plan_cpu.py, which compares the lines with what the shape of the kernels implies.
//   spectra2d_plan_check plan NX NY NFIELDS MEMBERS WX WY SHELLS LDS_LIMIT [...]
//       ->  "plan NX NY NFIELDS MEMBERS log2nx log2ny nkx NS R pad units1 units2 table blocks1 blocks2 blocks3 lds1 lds2 modes partials
//            workspace none unsupported too_many"
//   spectra2d_plan_check shell WX WY MX MY [MX MY ...]   ->  "shell MX MY S"
//   spectra2d_plan_check shape                           ->  "shape NT RMAX ROWS_LDS LDS_MAX P2_G P2_K SMALL UNITS_SMALL"
#include "launch_plan.hpp"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

using namespace swmhd;

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "shape")) {
        printf("shape %d %d %ld %ld %d %d %d %d\n", SPECTRA_NT, S2D_RMAX, S2D_ROWS_LDS, S2D_LDS_MAX, SPECTRA_P2_G, SPECTRA_P2_K, SPECTRA_SMALL_NX,
               SPECTRA_UNITS_SMALL);
        return 0;
    }
    if (argc >= 10 && !strcmp(argv[1], "plan") && (argc - 2) % 8 == 0) {
        for (int k = 2; k + 7 < argc; k += 8) {
            const int Nx = atoi(argv[k]), Ny = atoi(argv[k + 1]), nf = atoi(argv[k + 2]), members = atoi(argv[k + 3]);
            const double wx = atof(argv[k + 4]), wy = atof(argv[k + 5]);
            const Spectra2dPlan p = spectra2d_plan(Nx, Ny, nf, members, wx, wy, atoi(argv[k + 6]) != 0, atol(argv[k + 7]));
            printf("plan %d %d %d %d %d %d %d %d %d %d %d %d %d %ld %ld %ld %ld %ld %ld %ld %ld %d %d %d\n", Nx, Ny, nf, members, p.log2nx, p.log2ny, p.nkx,
                   p.NS, p.R, p.pad, p.units1, p.units2, (int)p.table, p.blocks1, p.blocks2, p.blocks3, p.lds1, p.lds2, p.modes, p.partials, p.workspace,
                   (int)p.none, (int)p.unsupported, (int)p.too_many);
        }
        return 0;
    }
    if (argc >= 6 && !strcmp(argv[1], "shell") && argc % 2 == 0) {
        const double wx = atof(argv[2]), wy = atof(argv[3]);
        for (int k = 4; k + 1 < argc; k += 2) printf("shell %d %d %d\n", atoi(argv[k]), atoi(argv[k + 1]), spectra2d_shell(atoi(argv[k]), atoi(argv[k + 1]), wx, wy));
        return 0;
    }
    fprintf(stderr, "usage: spectra2d_plan_check shape | plan NX NY NFIELDS MEMBERS WX WY SHELLS LDS_LIMIT ... | shell WX WY MX MY ...\n");
    return 2;
}
