// Host program: prints the launch plan of the six strip-march correction launches (strip_plan, swmhd_amd/csrc/launch_plan.hpp: Coriolis,
// diffusion, biharmonic, relaxation, source, stochastic) for the shapes given on the command line, the 16-byte phase a list of addresses
// shares (common_phase), and the plan of a whole call with the further pitches of its kind (strip_call_plan).
// Launches nothing and allocates no device memory.  Compiled and run by tests/test_strip_plan_cpu.py, which compares the lines with what
// the shape of the kernels implies.
//   strip_plan_check shape                                        ->  "shape WAVE WAVES WAVE_ROWS"
//   strip_plan_check plan NX ROWS ELEM_SIZE PHASE LAUNCHES ...    ->  "plan NX ROWS ELEM_SIZE PHASE LAUNCHES vec lead nstrips nsb blocks none too_many"
//   strip_plan_check phase ELEM_SIZE SY STRIDE_M ADDR [ADDR ...]  ->  "phase P"        (ADDR 0: a null entry)
//   strip_plan_check call NX ROWS ELEM_SIZE SY MEMBERS STRIDE_M PER_MEMBER NF PITCH_1 .. PITCH_NF ADDR [ADDR ...]
//                                                                 ->  "call vec lead nstrips nsb blocks none too_many"
#include "launch_plan.hpp"
#include <stdio.h>
#include <string.h>

using namespace swmhd;

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "shape")) {
        printf("shape %d %d %d\n", STRIP_WAVE, STRIP_WAVES, STRIP_WAVE_ROWS);
        return 0;
    }
    if (argc >= 7 && !strcmp(argv[1], "plan") && (argc - 2) % 5 == 0) {
        for (int k = 2; k + 4 < argc; k += 5) {
            const int Nx = atoi(argv[k]), rows = atoi(argv[k + 1]), es = atoi(argv[k + 2]), phase = atoi(argv[k + 3]), launches = atoi(argv[k + 4]);
            const StripPlan p = strip_plan(Nx, rows, es, phase, launches);
            printf("plan %d %d %d %d %d %d %d %d %d %ld %d %d\n", Nx, rows, es, phase, launches, p.vec, p.lead, p.nstrips, p.nsb, p.blocks,
                   (int)p.none, (int)p.too_many);
        }
        return 0;
    }
    if (argc >= 6 && !strcmp(argv[1], "phase") && argc - 5 <= 64) {
        const void *ptrs[64];
        for (int k = 5; k < argc; ++k) ptrs[k - 5] = (const void *)strtoul(argv[k], nullptr, 10);
        printf("phase %d\n", common_phase(atoi(argv[2]), atol(argv[3]), atol(argv[4]), ptrs, argc - 5));
        return 0;
    }
    if (argc >= 11 && !strcmp(argv[1], "call") && atoi(argv[9]) >= 0 && atoi(argv[9]) <= 3 && argc > 10 + atoi(argv[9]) &&
        argc - 10 - atoi(argv[9]) <= 64) {
        const int nf = atoi(argv[9]), n = argc - 10 - nf;
        long f[3] = {0, 0, 0};
        for (int k = 0; k < nf; ++k) f[k] = atol(argv[10 + k]);
        const void *ptrs[64];
        for (int k = 0; k < n; ++k) ptrs[k] = (const void *)strtoul(argv[10 + nf + k], nullptr, 10);
        const int Nx = atoi(argv[2]), rows = atoi(argv[3]), es = atoi(argv[4]), members = atoi(argv[6]), per = atoi(argv[8]);
        const long sy = atol(argv[5]), stride_m = atol(argv[7]);
        const StripPlan p = nf == 0   ? strip_call_plan(Nx, rows, es, ptrs, n, sy, members, stride_m, per)
                            : nf == 1 ? strip_call_plan(Nx, rows, es, ptrs, n, sy, members, stride_m, per, {f[0]})
                            : nf == 2 ? strip_call_plan(Nx, rows, es, ptrs, n, sy, members, stride_m, per, {f[0], f[1]})
                                      : strip_call_plan(Nx, rows, es, ptrs, n, sy, members, stride_m, per, {f[0], f[1], f[2]});
        printf("call %d %d %d %d %ld %d %d\n", p.vec, p.lead, p.nstrips, p.nsb, p.blocks, (int)p.none, (int)p.too_many);
        return 0;
    }
    fprintf(stderr, "usage: strip_plan_check shape | plan NX ROWS ELEM_SIZE PHASE LAUNCHES ... | phase ELEM_SIZE SY STRIDE_M ADDR ... | "
                    "call NX ROWS ELEM_SIZE SY MEMBERS STRIDE_M PER_MEMBER NF PITCH ... ADDR ...\n");
    return 2;
}
