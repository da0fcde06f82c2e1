"""The geometry of the stage matrices of the six strip-march correction launches (csrc/strip_device.inc: Coriolis, diffusion, biharmonic,
relaxation, source, stochastic), which their *_cases.py share, and which tests/strip_plan_check.cpp plans.
No numpy, no device."""
TILE_ROWS = 64                      # SWMHD_CORIOLIS_TILE_ROWS = SWMHD_DIFFUSION_TILE_ROWS = ...: four waves of 16 rows


def wave_columns(itemsize, aligned):
    """Columns of one wave of the kernel: 16 bytes per lane where all parents have the same 16-byte phase and the pitch keeps it."""
    return 64 * (16 // itemsize) if aligned else 64


def stage_shapes(itemsize, aligned):
    W = wave_columns(itemsize, aligned)
    return [(1, 1), (2, 3), (3, 3), (7, 9), (65, 17), (129, 9), (W - 1, TILE_ROWS - 1), (W, TILE_ROWS), (W + 1, TILE_ROWS + 1)]


def row_ranges(Ny):
    return [(0, Ny), (1, max(Ny - 1, 1)), (min(2, Ny), min(2, Ny))]      # all rows, the inner rows, an empty range
