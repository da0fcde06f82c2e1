// Fast build of the Lorentz operator kernels: reciprocal multiplies, FMA contraction on.
#include "common.hpp"
#include "launch_plan.hpp"
#define SWMHD_STRICT 0
#define LAUNCH_SFX fast
#include "lorentz_tile_kernels.inc"
#include "lorentz_launch.inc"
