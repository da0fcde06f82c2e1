// Host program: checks the launch plan of the derived-frame kernel (derived_plan, swmhd_amd/csrc/launch_plan.hpp) against what the
// shape of the kernel implies -- every chunk of every row has exactly one thread, nothing is planned without rows or members, and
// 2^31 workgroups and more are refused -- and prints the plans of the row widths, row counts and member counts given on the command
// line.  Launches nothing and allocates no device memory.  Compiled (with the address and undefined-behaviour sanitizers) and run by
// tests/test_derived_abi.py.
//   derived_plan_check                                  ->  "derived plans OK"
//   derived_plan_check plan NX ROWS MEMBERS [...]       ->  "plan NX ROWS MEMBERS nchunk threads blocks members none too_many"
#include "launch_plan.hpp"
#include <stdio.h>
#include <string.h>

using namespace swmhd;

static int failures = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            printf("FAILED line %d: %s\n", __LINE__, #cond);                    \
            ++failures;                                                         \
        }                                                                       \
    } while (0)

static void covers(int Nx, int rows, int members) {
    const DerivedPlan p = derived_plan(Nx, rows, members);
    CHECK(!p.none && !p.too_many);
    CHECK(p.nchunk >= 1 && (long)p.nchunk * DERIVED_VEC >= Nx && ((long)p.nchunk - 1) * DERIVED_VEC < Nx);
    CHECK(p.threads == (long)rows * p.nchunk);
    CHECK(p.blocks * DERIVED_NT >= p.threads && (p.blocks - 1) * DERIVED_NT < p.threads);
    CHECK(p.members == members);
    // the kernel's decoding of a thread number: the last planned thread is the last chunk of the last row
    const long t = p.threads - 1;
    CHECK((int)(t / p.nchunk) == rows - 1 && (int)(t - (long)(rows - 1) * p.nchunk) == p.nchunk - 1);
}

int main(int argc, char **argv) {
    if (argc >= 5 && !strcmp(argv[1], "plan") && (argc - 2) % 3 == 0) {
        for (int k = 2; k + 2 < argc; k += 3) {
            const int Nx = atoi(argv[k]), rows = atoi(argv[k + 1]), members = atoi(argv[k + 2]);
            const DerivedPlan p = derived_plan(Nx, rows, members);
            printf("plan %d %d %d %d %ld %ld %d %d %d\n", Nx, rows, members, p.nchunk, p.threads, p.blocks, p.members, (int)p.none, (int)p.too_many);
        }
        return 0;
    }
    if (argc != 1) {
        fprintf(stderr, "usage: derived_plan_check [plan NX ROWS MEMBERS ...]\n");
        return 2;
    }
    CHECK(DERIVED_NT == 256 && DERIVED_VEC == 4);
    const int widths[] = {1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 1023, 1024, 1025, 4096, 2147483647};
    const int heights[] = {1, 2, 3, 9, 64, 4096};
    const int counts[] = {1, 3, 256, 65535};
    for (int Nx : widths)
        for (int rows : heights)
            for (int members : counts)
                if ((((long)Nx + 3) / 4 * rows + 255) / 256 * members < (1L << 31)) covers(Nx, rows, members);
    // nothing to do: no launch is planned, whatever the other arguments are
    CHECK(derived_plan(64, 0, 1).none && derived_plan(64, 5, 0).none && derived_plan(64, -1, 3).none && derived_plan(0, 5, 1).none);
    CHECK(derived_plan(64, 0, 1).blocks == 0 && derived_plan(64, 5, 0).threads == 0);
    // one row of 64 cells is 16 threads of one workgroup; 65 cells take a 17th; 1025 cells cross into a second workgroup
    CHECK(derived_plan(64, 1, 1).threads == 16 && derived_plan(64, 1, 1).blocks == 1);
    CHECK(derived_plan(65, 1, 1).threads == 17 && derived_plan(1025, 1, 1).threads == 257 && derived_plan(1025, 1, 1).blocks == 2);
    CHECK(derived_plan(4096, 4096, 1).blocks == 4096 * 4 && derived_plan(64, 64, 256).blocks == 4);
    // the edge of one launch: 2^31 - 1 workgroups pass, 2^31 are refused (rows x chunks, and the members on top)
    CHECK(!derived_plan(1024, 2147483647, 1).too_many && derived_plan(1024, 2147483647, 1).blocks == 2147483647L);
    CHECK(derived_plan(1028, 2147483647, 1).too_many);
    CHECK(!derived_plan(4096, 32768, 16383).too_many && derived_plan(4096, 32768, 16384).too_many);
    CHECK(derived_plan(2147483647, 2147483647, 65535).too_many);      // (no overflow on the way: 2^29 chunks x 2^31 rows x 2^16)
    if (failures) return 1;
    printf("derived plans OK\n");
    return 0;
}
