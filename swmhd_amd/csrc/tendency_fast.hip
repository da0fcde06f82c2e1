// Fast build of the fused tendency / RK3 kernels.
#include "common.hpp"
#include "launch_plan.hpp"
#define SWMHD_STRICT 0
#define LAUNCH_SFX fast
#include "tendency_tile_kernels.inc"
#include "tendency_launch.inc"
