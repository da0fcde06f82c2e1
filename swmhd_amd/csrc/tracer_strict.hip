// Strict build of the passive-tracer stage kernel (-ffp-contract=off, oracle expression order).
#include "common.hpp"
#include "launch_plan.hpp"
#define SWMHD_STRICT 1
#define LAUNCH_SFX strict
#include "tracer_kernels.inc"
