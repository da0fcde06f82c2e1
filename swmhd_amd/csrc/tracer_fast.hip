// Fast build of the passive-tracer stage kernel.
#include "common.hpp"
#include "launch_plan.hpp"
#define SWMHD_STRICT 0
#define LAUNCH_SFX fast
#include "tracer_kernels.inc"
