"""ctypes binding of libswmhd.so (include/swmhd.h).  The product path: fails loudly if the HIP library is
missing -- there is no CPU fallback anywhere in this package."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libswmhd.so")
_LIB = None

STRICT = 1
FAST = 0
TILE_KERNEL = 2
MARCH_KERNEL = 4
WRAP_X, WRAP_Y = 16, 32
LEAVE_ROOM = 64
GM_IS_PREV_STATE = 1024
RK3_ANCHOR = 2048
BOUNDED_X, BOUNDED_Y = 256, 512
OPEN_SOUTH, OPEN_NORTH = 4096, 8192    # with BOUNDED_Y: that side of a y-slab of a Bounded-y chain is a cut, not a wall
KERNEL_FLAGS = {None: 0, "auto": 0, "tile": 2, "march": 4}
PERIODIC, BOUNDED = 0, 1
HALO_X, HALO_Y = 1, 2
DIAG_NOUT, DIAG_WORKSPACE = 7, 1024 * 7
# SWMHD_OUT_*: the output fields of swmhd_output_fields_*, by the names of the reference's writer, in bit (= frame) order
OUT_BITS = {"u": 1, "v": 2, "h": 4, "A": 8, "s": 16, "B_x": 32, "B_y": 64}
# SWMHD_ZM_*: the profiles of swmhd_zonal_means_*, in bit (= profile) order: the seven fields of OUT_BITS, then the second moments
ZM_BITS = {**OUT_BITS, "uu": 128, "vv": 256, "uv": 512, "B_xB_x": 1024, "B_yB_y": 2048, "B_xB_y": 4096, "vA": 8192}
# SWMHD_DRV_*: the fields of swmhd_derived_fields_* (include/swmhd_derived.h), in bit (= frame) order
DRV_BITS = {"vorticity": 1, "divergence": 2, "current": 4, "potential_vorticity": 8}
# SWMHD_ZS_*: the fields of swmhd_zonal_spectra_* (include/swmhd_spectra.h): those of OUT_BITS; Nx = 2^p, p = 2 .. 12
ZS_BITS = dict(OUT_BITS)
SPECTRA_MIN_NX, SPECTRA_MAX_NX = 4, 4096
ENSEMBLE_MAX_MEMBERS = 65535
ENSEMBLE_NPARAMS = 3    # SWMHD_ENSEMBLE_NPARAMS: (g, f, dt) per member in the table of the swmhd_ensemble_*_params calls
MAX_TRACERS = 8         # SWMHD_MAX_TRACERS: passive tracers per swmhd_tracers_rk3_* launch
DIFFUSION_MAX_FIELDS = 3 + MAX_TRACERS    # SWMHD_DIFFUSION_MAX_FIELDS: fields per swmhd_diffusion_rk3_* launch
DIFFUSION_TILE_ROWS = 64                  # SWMHD_DIFFUSION_TILE_ROWS: rows of a workgroup of the diffusion kernel (four waves)
CORIOLIS_TILE_ROWS = 64                   # SWMHD_CORIOLIS_TILE_ROWS: rows of a workgroup of the Coriolis kernel (four waves)
RELAXATION_MAX_FIELDS = 4 + MAX_TRACERS   # SWMHD_RELAXATION_MAX_FIELDS: fields per swmhd_relaxation_rk3_* launch
RELAXATION_TILE_ROWS = 64                 # SWMHD_RELAXATION_TILE_ROWS: rows of a workgroup of the relaxation kernel (four waves)
SOURCE_MAX_FIELDS = 4 + MAX_TRACERS       # SWMHD_SOURCE_MAX_FIELDS: fields per swmhd_source_rk3_* launch
SOURCE_TILE_ROWS = 64                     # SWMHD_SOURCE_TILE_ROWS: rows of a workgroup of the source kernel (four waves)
SOURCE_PLAIN, SOURCE_X_FACE, SOURCE_Y_FACE = 0, 1, 2    # SWMHD_SOURCE_*: the source as it is, times the thickness at the x / y face
STOCHASTIC_MAX_FIELDS = 4 + MAX_TRACERS   # SWMHD_STOCHASTIC_MAX_FIELDS: fields per swmhd_stochastic_rk3_* launch, groups per draw
STOCHASTIC_MAX_MODES = 256                # SWMHD_STOCHASTIC_MAX_MODES: Fourier modes of one field
STOCHASTIC_TILE_ROWS = 64                 # SWMHD_STOCHASTIC_TILE_ROWS: rows of a workgroup of the stochastic kernel (four waves)
STOCHASTIC_MODE_CHUNK = 4                 # SWMHD_STOCHASTIC_MODE_CHUNK: modes whose x tables a lane holds in registers at a time
PARTICLES_BLOCK = 256                     # SWMHD_PARTICLES_BLOCK: particles of a workgroup of the particle kernels (one lane each)
PARTICLES_MAX_FIELDS = 4 + MAX_TRACERS    # SWMHD_PARTICLES_MAX_FIELDS: fields per swmhd_particles_sample_* launch
PARTICLES_CENTER_X, PARTICLES_CENTER_Y = 1, 2    # SWMHD_PARTICLES_CENTER_*: a sampled field's nodes are cell centres in that direction


def ensemble_diag_workspace(members, Nx, Ny):
    """SWMHD_ENSEMBLE_DIAG_WORKSPACE(members, Nx, Ny): doubles of device workspace swmhd_ensemble_diagnostics_* needs."""
    cells = Nx * Ny
    return members * 7 * (1024 if cells >= 1024 * 256 else (cells + 255) // 256)
CONSERVATIVE, VECTOR_INVARIANT = 0, 1
LORENTZ_NONE, LORENTZ_JACOBIAN, LORENTZ_DIVERGENCE = 0, 1, 2


def ptr_array(ptrs):
    """Host array of device pointers (void*[n]) for the *_multi / rk3 entry points."""
    return (C.c_void_p * len(ptrs))(*ptrs)


class SwmhdError(RuntimeError):
    pass


def _declare(lib):
    p, i, i64 = C.c_void_p, C.c_int, C.c_int64
    lib.swmhd_version.restype = i
    lib.swmhd_strerror.restype = C.c_char_p
    lib.swmhd_strerror.argtypes = [i]
    lib.swmhd_event_create.argtypes = [C.POINTER(p)]
    lib.swmhd_event_record.argtypes = [p, p]
    lib.swmhd_event_elapsed_ms.argtypes = [p, p, C.POINTER(C.c_float)]
    lib.swmhd_event_destroy.argtypes = [p]
    for n in ("create", "record", "elapsed_ms", "destroy"):
        getattr(lib, "swmhd_event_" + n).restype = i
    lib.swmhd_probe_fp64_issue.argtypes = [p, C.POINTER(C.c_float), p]
    lib.swmhd_probe_fp64_issue.restype = i
    lib.swmhd_probe_copy.argtypes = [p, p, C.c_size_t, i, C.POINTER(C.c_float), p]
    lib.swmhd_probe_copy.restype = i
    for sfx, ft in (("f64", C.c_double), ("f32", C.c_float)):
        for form in ("jacobian", "divergence"):
            f = getattr(lib, f"swmhd_lorentz_{form}_{sfx}")
            f.argtypes = [p, p, p, p, i, i, i, i, i64, ft, ft, i, p]
            f.restype = i
        f = getattr(lib, f"swmhd_lorentz_jacobian_rows_{sfx}")
        f.argtypes = [p, p, p, p, i, i, i, i, i64, ft, ft, i, i, i, p]
        f.restype = i
        f = getattr(lib, f"swmhd_lorentz_divergence_rows_{sfx}")
        f.argtypes = [p, p, p, p, i, i, i, i, i64, ft, ft, i, i, i, i, i, p]
        f.restype = i
        f = getattr(lib, f"swmhd_fill_halo_periodic_{sfx}")
        f.argtypes = [p, i, i, i, i, i64, i, p]
        f.restype = i
        f = getattr(lib, f"swmhd_fill_halo_{sfx}")
        f.argtypes = [C.POINTER(p), i, i, i, i, i, i64, i, i, i, i, p, ft, ft, p]
        f.restype = i
        f = getattr(lib, f"swmhd_fill_halo_periodic_multi_{sfx}")
        f.argtypes = [C.POINTER(p), i, i, i, i, i, i64, i, p]
        f.restype = i
        f = getattr(lib, f"swmhd_tendencies_{sfx}")
        f.argtypes = [p] * 8 + [i, i, i, i, i64, ft, ft, ft, ft, i, i, i, i, i, p]
        f.restype = i
        f = getattr(lib, f"swmhd_tendencies_rk3_{sfx}")
        f.argtypes = [C.POINTER(p)] * 4 + [i, i, i, i, i64, ft, ft, ft, ft, i, i, ft, ft, ft, i, i, i, i, p]
        f.restype = i
        f = getattr(lib, f"swmhd_step_rk3_{sfx}")
        f.argtypes = [C.POINTER(p)] * 4 + [i, i, i, i, i64, ft, ft, ft, ft, i, i, ft, i, i, C.POINTER(i), p]
        f.restype = i
        f = getattr(lib, f"swmhd_tracers_rk3_{sfx}")
        f.argtypes = [p, p, p] + [C.POINTER(p)] * 4 + [i, i, i, i, i, i64, ft, ft, i, ft, ft, ft, i, i, i, i, p]
        f.restype = i
        f = getattr(lib, f"swmhd_diagnostics_{sfx}")
        f.argtypes = [p, p, p, p, i, i, i, i, i64, ft, ft, ft, ft, i, i, i, p, p, p]
        f.restype = i
        f = getattr(lib, f"swmhd_rk3_substep_{sfx}")
        f.argtypes = [C.POINTER(p), C.POINTER(p), C.POINTER(p), i, i, i, i, i64, ft, ft, ft, i, i, i, p]
        f.restype = i
        f = getattr(lib, f"swmhd_ensemble_tendencies_rk3_{sfx}")
        f.argtypes = [C.POINTER(p)] * 4 + [i, i64, i, i, i, i, i64, ft, ft, ft, ft, i, i, ft, ft, ft, i, i, p]
        f.restype = i
        f = getattr(lib, f"swmhd_ensemble_step_rk3_{sfx}")
        f.argtypes = [C.POINTER(p)] * 4 + [i, i64, i, i, i, i, i64, ft, ft, ft, ft, i, i, ft, i, i, C.POINTER(i), p]
        f.restype = i
        f = getattr(lib, f"swmhd_ensemble_fill_halo_periodic_{sfx}")
        f.argtypes = [C.POINTER(p), i, i, i64, i, i, i, i, i64, i, p]
        f.restype = i
        f = getattr(lib, f"swmhd_ensemble_diagnostics_{sfx}")
        f.argtypes = [p, p, p, p, i, i64, i, i, i, i, i64, ft, ft, ft, ft, i, p, p, p]
        f.restype = i
        f = getattr(lib, f"swmhd_ensemble_fill_halo_{sfx}")
        f.argtypes = [C.POINTER(p), i, i, i64, i, i, i, i, i64, i, i, i, i, p, ft, ft, p]
        f.restype = i
        f = getattr(lib, f"swmhd_ensemble_step_rk3_bc_{sfx}")
        f.argtypes = [C.POINTER(p)] * 4 + [i, i64, i, i, i, i, i64, ft, ft, ft, ft, i, i, ft, i, p, i, C.POINTER(i), p]
        f.restype = i
        # per-member (g, f, dt): the scalars replaced by a device table
        f = getattr(lib, f"swmhd_ensemble_tendencies_rk3_params_{sfx}")
        f.argtypes = [C.POINTER(p)] * 4 + [i, i64, i, i, i, i, i64, ft, ft, p, i, i, ft, ft, i, i, p]
        f.restype = i
        f = getattr(lib, f"swmhd_ensemble_step_rk3_params_{sfx}")
        f.argtypes = [C.POINTER(p)] * 4 + [i, i64, i, i, i, i, i64, ft, ft, p, i, i, i, i, C.POINTER(i), p]
        f.restype = i
        f = getattr(lib, f"swmhd_ensemble_step_rk3_bc_params_{sfx}")
        f.argtypes = [C.POINTER(p)] * 4 + [i, i64, i, i, i, i, i64, ft, ft, p, i, i, i, p, i, C.POINTER(i), p]
        f.restype = i
        f = getattr(lib, f"swmhd_ensemble_diagnostics_params_{sfx}")
        f.argtypes = [p, p, p, p, i, i64, i, i, i, i, i64, ft, ft, p, ft, i, p, p, p]
        f.restype = i
        # the tracers of a periodic ensemble: swmhd_tracers_rk3 without the row range, with members and stride_m (dt: scalar | table)
        f = getattr(lib, f"swmhd_ensemble_tracers_rk3_{sfx}")
        f.argtypes = [p, p, p] + [C.POINTER(p)] * 4 + [i, i, i64, i, i, i, i, i64, ft, ft, i, ft, ft, ft, i, i, p]
        f.restype = i
        f = getattr(lib, f"swmhd_ensemble_tracers_rk3_params_{sfx}")
        f.argtypes = [p, p, p] + [C.POINTER(p)] * 4 + [i, i, i64, i, i, i, i, i64, ft, ft, i, p, ft, ft, i, i, p]
        f.restype = i
        f = getattr(lib, f"swmhd_ring_exchange_y_{sfx}")
        f.argtypes = [p, C.POINTER(p), i, i, i, i, i, i64, p]
        f.restype = i
        f = getattr(lib, f"swmhd_ring_step_rk3_{sfx}")
        f.argtypes = [p] + [C.POINTER(p)] * 4 + [i, i, i, i, i64, ft, ft, ft, ft, i, i, ft, i, i, C.POINTER(i), p]
        f.restype = i
        f = getattr(lib, f"swmhd_ring_exchange_y_sides_{sfx}")
        f.argtypes = [p, C.POINTER(p), i, i, i, i, i, i64, i, p]
        f.restype = i
        f = getattr(lib, f"swmhd_ring_step_rk3_bc_{sfx}")
        f.argtypes = [p] + [C.POINTER(p)] * 4 + [i, i, i, i, i64, ft, ft, ft, ft, i, i, ft, i, p, i, C.POINTER(i), p]
        f.restype = i
        f = getattr(lib, f"swmhd_fill_halo_walls_{sfx}")
        f.argtypes = [C.POINTER(p), i, i, i, i, i, i64, i, i, i, i, p, ft, ft, p]
        f.restype = i
        f = getattr(lib, f"swmhd_output_fields_{sfx}")
        f.argtypes = [p, p, p, p, i, i, i, i, i64, ft, ft, i, i, i, i, p, i, i64, i64, i, p]
        f.restype = i
        f = getattr(lib, f"swmhd_ensemble_output_fields_{sfx}")
        f.argtypes = [p, p, p, p, i, i64, i, i, i, i, i64, ft, ft, i, i, i, i, p, i, i64, i64, i64, i, p]
        f.restype = i
        f = getattr(lib, f"swmhd_zonal_means_{sfx}")
        f.argtypes = [p, p, p, p, i, i, i, i, i64, ft, ft, i, i, i, i, p, i64, i, p]
        f.restype = i
        f = getattr(lib, f"swmhd_ensemble_zonal_means_{sfx}")
        f.argtypes = [p, p, p, p, i, i64, i, i, i, i, i64, ft, ft, i, i, i, i, p, i64, i64, i, p]
        f.restype = i
        # derived frames: the arguments of the output frames with coriolis_f (or the (g, f, dt) table) after the formulation
        f = getattr(lib, f"swmhd_derived_fields_{sfx}")
        f.argtypes = [p, p, p, p, i, i, i, i, i64, ft, ft, i, ft, i, i, i, p, i, i64, i64, i, p]
        f.restype = i
        f = getattr(lib, f"swmhd_ensemble_derived_fields_{sfx}")
        f.argtypes = [p, p, p, p, i, i64, i, i, i, i, i64, ft, ft, i, ft, i, i, i, p, i, i64, i64, i64, i, p]
        f.restype = i
        # zonal spectra: the arguments of the zonal means with the workspace in front of `out`
        f = getattr(lib, f"swmhd_zonal_spectra_{sfx}")
        f.argtypes = [p, p, p, p, i, i, i, i, i64, ft, ft, i, i, i, i, p, p, i64, i, p]
        f.restype = i
        f = getattr(lib, f"swmhd_ensemble_zonal_spectra_{sfx}")
        f.argtypes = [p, p, p, p, i, i64, i, i, i, i, i64, ft, ft, i, i, i, i, p, p, i64, i64, i, p]
        f.restype = i
        # 2-D and isotropic spectra: the zonal spectra without the rows; wx, wy; out_shell and out_2d with their strides
        f = getattr(lib, f"swmhd_spectra2d_{sfx}")
        f.argtypes = [p, p, p, p, i, i, i, i, i64, ft, ft, i, i, C.c_double, C.c_double, p, p, i64, p, i64, i64, i, p]
        f.restype = i
        f = getattr(lib, f"swmhd_ensemble_spectra2d_{sfx}")
        f.argtypes = [p, p, p, p, i, i64, i, i, i, i, i64, ft, ft, i, i, C.c_double, C.c_double, p, p, i64, i64, p, i64, i64, i64, i, p]
        f.restype = i
        f = getattr(lib, f"swmhd_ensemble_derived_fields_params_{sfx}")
        f.argtypes = [p, p, p, p, i, i64, i, i, i, i, i64, ft, ft, i, p, i, i, i, p, i, i64, i64, i64, i, p]
        f.restype = i
        # ScalarDiffusivity closure: old, new, acc, coef (host array | device table), nfields, ...
        f = getattr(lib, f"swmhd_diffusion_rk3_{sfx}")
        f.argtypes = [C.POINTER(p)] * 3 + [p, i, i, i, i, i, i64, ft, ft, ft, ft, i, i, i, p]
        f.restype = i
        f = getattr(lib, f"swmhd_ensemble_diffusion_rk3_{sfx}")
        f.argtypes = [C.POINTER(p)] * 3 + [p, i, i, i64, i, i, i, i, i64, ft, ft, p, ft, ft, i, i, i, p]
        f.restype = i
        # ScalarBiharmonicDiffusivity closure: the argument lists of the two diffusion calls
        f = getattr(lib, f"swmhd_biharmonic_rk3_{sfx}")
        f.argtypes = [C.POINTER(p)] * 3 + [p, i, i, i, i, i, i64, ft, ft, ft, ft, i, i, i, p]
        f.restype = i
        f = getattr(lib, f"swmhd_ensemble_biharmonic_rk3_{sfx}")
        f.argtypes = [C.POINTER(p)] * 3 + [p, i, i, i64, i, i, i, i, i64, ft, ft, p, ft, ft, i, i, i, p]
        f.restype = i
        # BetaPlane Coriolis: q1, q2 old, new, acc, frow (device table), ...
        f = getattr(lib, f"swmhd_coriolis_rk3_{sfx}")
        f.argtypes = [p] * 7 + [i, i, i, i, i64, ft, ft, i, i, i, p]
        f.restype = i
        f = getattr(lib, f"swmhd_ensemble_coriolis_rk3_{sfx}")
        f.argtypes = [p] * 7 + [i, i64, i, i, i, i, i64, p, ft, ft, i, i, i, p]
        f.restype = i
        # Relaxation forcing: old, new, acc, mask, target (host arrays of device pointers), rate, tval (host arrays | device tables), ...
        f = getattr(lib, f"swmhd_relaxation_rk3_{sfx}")
        f.argtypes = [C.POINTER(p)] * 5 + [p, p, i, i, i, i, i, i64, ft, ft, i, i, i, p]
        f.restype = i
        f = getattr(lib, f"swmhd_ensemble_relaxation_rk3_{sfx}")
        f.argtypes = [C.POINTER(p)] * 5 + [p, p, i, i, i64, i64, i64, i, i, i, i, i64, p, ft, ft, i, i, i, p]
        f.restype = i
        # Static sources: old, new, acc, source (host arrays of device pointers), kind (host array), nfields, thickness, ...
        f = getattr(lib, f"swmhd_source_rk3_{sfx}")
        f.argtypes = [C.POINTER(p)] * 4 + [C.POINTER(i), i, i, i, i, i, i, i64, ft, ft, i, i, i, p]
        f.restype = i
        f = getattr(lib, f"swmhd_ensemble_source_rk3_{sfx}")
        f.argtypes = [C.POINTER(p)] * 4 + [C.POINTER(i), i, i, i, i64, i64, i, i, i, i, i64, p, ft, ft, i, i, i, p]
        f.restype = i
        # Stochastic forcing, the draw: counter (device), coef, amp0, ktx, kty (host arrays of device pointers), nmodes, kind (host), ...
        f = getattr(lib, f"swmhd_stochastic_coefficients_{sfx}")
        f.argtypes = [p] + [C.POINTER(p)] * 4 + [C.POINTER(i), C.POINTER(i), i, C.c_uint64, C.c_uint32, C.c_double, p]
        f.restype = i
        f = getattr(lib, f"swmhd_ensemble_stochastic_coefficients_{sfx}")
        f.argtypes = [p] + [C.POINTER(p)] * 4 + [C.POINTER(i), C.POINTER(i), i, i, i64, i64, C.c_uint64, p, C.c_double, p]
        f.restype = i
        # the correction: old, new, acc, coef, xtab, ytab (host arrays of device pointers), nmodes (host), nfields, x_pitch, y_pitch, ...
        f = getattr(lib, f"swmhd_stochastic_rk3_{sfx}")
        f.argtypes = [C.POINTER(p)] * 6 + [C.POINTER(i), i, i64, i64, i, i, i, i, i64, ft, ft, i, i, i, p]
        f.restype = i
        f = getattr(lib, f"swmhd_ensemble_stochastic_rk3_{sfx}")
        f.argtypes = [C.POINTER(p)] * 6 + [C.POINTER(i), i, i64, i64, i, i64, i64, i, i, i, i, i64, p, ft, ft, i, i, i, p]
        f.restype = i
        # Lagrangian particles: q1, q2, h, x, y, gx, gy, P, [members, stride_m,] grid, x0, y0, dx, dy (doubles), form, [params,] dt, gamma, zeta
        d = C.c_double
        f = getattr(lib, f"swmhd_particles_rk3_{sfx}")
        f.argtypes = [p] * 7 + [i64, i, i, i, i, i64, d, d, d, d, i, d, d, d, i, p]
        f.restype = i
        f = getattr(lib, f"swmhd_ensemble_particles_rk3_{sfx}")
        f.argtypes = [p] * 7 + [i64, i, i64, i, i, i, i, i64, d, d, d, d, i, p, d, d, d, i, p]
        f.restype = i
        # the sampler: fields (host array of device pointers), loc (host array), nfields, x, y, out, P, [members, stride_m,] grid, ...
        f = getattr(lib, f"swmhd_particles_sample_{sfx}")
        f.argtypes = [C.POINTER(p), C.POINTER(i), i, p, p, p, i64, i, i, i, i, i64, d, d, d, d, i, p]
        f.restype = i
        f = getattr(lib, f"swmhd_ensemble_particles_sample_{sfx}")
        f.argtypes = [C.POINTER(p), C.POINTER(i), i, p, p, p, i64, i, i64, i, i, i, i, i64, d, d, d, d, i, p]
        f.restype = i
    lib.swmhd_zonal_spectra_workspace.argtypes = [i, i, i, i]
    lib.swmhd_zonal_spectra_workspace.restype = i64
    lib.swmhd_spectra2d_shells.argtypes = [i, i, C.c_double, C.c_double]
    lib.swmhd_spectra2d_shells.restype = i
    lib.swmhd_spectra2d_workspace.argtypes = [i, i, i, i, C.c_double, C.c_double]
    lib.swmhd_spectra2d_workspace.restype = i64
    lib.swmhd_tendency_launch_geometry.argtypes = [i, i, i, i, i, C.POINTER(i)]
    lib.swmhd_tendency_launch_geometry.restype = i
    lib.swmhd_ensemble_launch_geometry.argtypes = [i, i, i, i, i, i, C.POINTER(i)]
    lib.swmhd_ensemble_launch_geometry.restype = i
    lib.swmhd_ring_available.argtypes = [C.c_char_p]
    lib.swmhd_ring_available.restype = i
    lib.swmhd_ring_unique_id.argtypes = [C.c_char_p, p]
    lib.swmhd_ring_unique_id.restype = i
    lib.swmhd_ring_create.argtypes = [C.POINTER(p), C.c_char_p, i, i, p]
    lib.swmhd_ring_create.restype = i
    lib.swmhd_ring_create_loopback.argtypes = [C.POINTER(p), i, C.c_double]
    lib.swmhd_ring_create_loopback.restype = i
    lib.swmhd_ring_destroy.argtypes = [p]
    lib.swmhd_ring_destroy.restype = i
    lib.swmhd_ring_last_error.argtypes = [p]
    lib.swmhd_ring_last_error.restype = C.c_char_p
    lib.swmhd_ring_comm_stream.argtypes = [p]
    lib.swmhd_ring_comm_stream.restype = p
    lib.swmhd_ring_join.argtypes = [p, p]
    lib.swmhd_ring_join.restype = i
    lib.swmhd_ring_time_launches.argtypes = [p, i]
    lib.swmhd_ring_time_launches.restype = i
    lib.swmhd_ring_launch_times.argtypes = [p, C.POINTER(C.c_float), C.POINTER(i), i]
    lib.swmhd_ring_launch_times.restype = i


# every symbol include/swmhd.h declares (tests/test_abi.py checks the .so exports each of them)
EXPORTS = ["swmhd_version", "swmhd_strerror", "swmhd_tendency_launch_geometry", "swmhd_ensemble_launch_geometry", "swmhd_probe_fp64_issue", "swmhd_probe_copy"] + ["swmhd_event_" + n for n in ("create", "record", "elapsed_ms", "destroy")] + [
    f"swmhd_{name}_{sfx}" for sfx in ("f64", "f32") for name in (
        "lorentz_jacobian", "lorentz_jacobian_rows", "lorentz_divergence", "lorentz_divergence_rows",
        "fill_halo", "fill_halo_periodic", "fill_halo_periodic_multi", "tendencies", "tendencies_rk3", "rk3_substep", "step_rk3", "diagnostics",
        "ring_exchange_y", "ring_step_rk3", "ensemble_tendencies_rk3", "ensemble_step_rk3", "ensemble_fill_halo_periodic",
        "ensemble_diagnostics", "ensemble_fill_halo", "ensemble_step_rk3_bc", "fill_halo_walls", "ring_exchange_y_sides", "ring_step_rk3_bc",
        "output_fields", "ensemble_output_fields", "ensemble_tendencies_rk3_params", "ensemble_step_rk3_params",
        "ensemble_step_rk3_bc_params", "ensemble_diagnostics_params", "tracers_rk3", "ensemble_tracers_rk3",
        "ensemble_tracers_rk3_params")] + [
    "swmhd_ring_" + name for name in ("available", "unique_id", "create", "create_loopback", "destroy", "last_error", "comm_stream", "join", "time_launches",
                                      "launch_times")]
# the symbols include/swmhd_zonal.h declares (swmhd.h includes it; tests/test_zonal_abi.py checks the .so exports each of them)
ZONAL_EXPORTS = [f"swmhd_{name}_{sfx}" for sfx in ("f64", "f32") for name in ("zonal_means", "ensemble_zonal_means")]
# the symbols include/swmhd_derived.h declares (swmhd.h includes it; tests/test_derived_abi.py checks the .so exports each of them)
DERIVED_EXPORTS = [f"swmhd_{name}_{sfx}" for sfx in ("f64", "f32")
                   for name in ("derived_fields", "ensemble_derived_fields", "ensemble_derived_fields_params")]
# the symbols include/swmhd_spectra.h declares (swmhd.h includes it; tests/test_spectra_abi.py checks the .so exports each of them)
SPECTRA_EXPORTS = ["swmhd_zonal_spectra_workspace"] + [f"swmhd_{name}_{sfx}" for sfx in ("f64", "f32")
                                                       for name in ("zonal_spectra", "ensemble_zonal_spectra")]
# the symbols include/swmhd_spectra2d.h declares (swmhd.h includes it; tests/test_spectra2d_abi.py checks the .so exports each of them)
SPECTRA2D_EXPORTS = ["swmhd_spectra2d_shells", "swmhd_spectra2d_workspace"] + [f"swmhd_{name}_{sfx}" for sfx in ("f64", "f32")
                                                                               for name in ("spectra2d", "ensemble_spectra2d")]
# the symbols include/swmhd_diffusion.h declares (swmhd.h includes it; tests/test_diffusion_abi.py checks the .so exports each of them)
DIFFUSION_EXPORTS = [f"swmhd_{name}_{sfx}" for sfx in ("f64", "f32") for name in ("diffusion_rk3", "ensemble_diffusion_rk3")]
# the symbols include/swmhd_biharmonic.h declares (swmhd.h includes it; tests/test_biharmonic_abi.py checks the .so exports each of them)
BIHARMONIC_EXPORTS = [f"swmhd_{name}_{sfx}" for sfx in ("f64", "f32") for name in ("biharmonic_rk3", "ensemble_biharmonic_rk3")]
# the symbols include/swmhd_coriolis.h declares (swmhd.h includes it; tests/test_coriolis_abi.py checks the .so exports each of them)
CORIOLIS_EXPORTS = [f"swmhd_{name}_{sfx}" for sfx in ("f64", "f32") for name in ("coriolis_rk3", "ensemble_coriolis_rk3")]
# the symbols include/swmhd_relaxation.h declares (swmhd.h includes it; tests/test_relaxation_abi.py checks the .so exports each of them)
RELAXATION_EXPORTS = [f"swmhd_{name}_{sfx}" for sfx in ("f64", "f32") for name in ("relaxation_rk3", "ensemble_relaxation_rk3")]
# the symbols include/swmhd_stochastic.h declares (swmhd.h includes it; tests/test_stochastic_abi.py checks the .so exports each of them)
STOCHASTIC_EXPORTS = [f"swmhd_{name}_{sfx}" for sfx in ("f64", "f32")
                      for name in ("stochastic_coefficients", "ensemble_stochastic_coefficients", "stochastic_rk3", "ensemble_stochastic_rk3")]
# the symbols include/swmhd_source.h declares (swmhd.h includes it; tests/test_source_abi.py checks the .so exports each of them)
SOURCE_EXPORTS = [f"swmhd_{name}_{sfx}" for sfx in ("f64", "f32") for name in ("source_rk3", "ensemble_source_rk3")]
# the symbols include/swmhd_particles.h declares (swmhd.h includes it; tests/test_particles_abi.py checks the .so exports each of them)
PARTICLES_EXPORTS = [f"swmhd_{name}_{sfx}" for sfx in ("f64", "f32")
                     for name in ("particles_rk3", "ensemble_particles_rk3", "particles_sample", "ensemble_particles_sample")]
RING_ID_BYTES = 128


class TimingEvent:
    """A HIP timing event without the system-scope fence (swmhd_event_*), with the two methods of torch.cuda.Event that the
    benchmarks use.  `record` takes the raw stream handle (default: torch's current stream)."""

    def __init__(self):
        self._e = C.c_void_p()
        check(lib().swmhd_event_create(C.byref(self._e)), "swmhd_event_create")

    def record(self, stream=None):
        if stream is None:
            import torch
            stream = torch.cuda.current_stream().cuda_stream
        check(lib().swmhd_event_record(self._e, C.c_void_p(stream)), "swmhd_event_record")

    def elapsed_time(self, stop):
        ms = C.c_float()
        check(lib().swmhd_event_elapsed_ms(self._e, stop._e, C.byref(ms)), "swmhd_event_elapsed_ms")
        return ms.value

    def __del__(self):
        try:
            if self._e:
                lib().swmhd_event_destroy(self._e)
        except Exception:
            pass


def lib():
    """Load libswmhd.so (built in-tree by __graft_entry__.build() / swmhd_amd/csrc/Makefile)."""
    global _LIB
    if _LIB is None:
        path = os.environ.get("SWMHD_LIBRARY", LIB_PATH)     # A/B builds of the same library (tools/): never a different backend
        if not os.path.exists(path):
            raise SwmhdError(
                f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  swmhd_amd has no CPU fallback.")
        _LIB = C.CDLL(path)
        _declare(_LIB)
    return _LIB


def tendency_launch_geometry(Nx, rows, formulation, elem_size=8, flags=0):
    """dict(kind, threads, nstrips, nseg, rows_per_segment, wg_per_cu, halo_lanes, cus) of the fast tendency launch (swmhd.h)."""
    out = (C.c_int * 8)()
    check(lib().swmhd_tendency_launch_geometry(Nx, rows, formulation, elem_size, flags, out), "swmhd_tendency_launch_geometry")
    keys = ("kind", "threads", "nstrips", "nseg", "rows_per_segment", "wg_per_cu", "halo_lanes", "cus")
    return dict(zip(keys, list(out)))


def ensemble_launch_geometry(Nx, Ny, formulation, members, elem_size=8, flags=0):
    """dict(kind, threads, tile_columns, tile_rows, rows_per_tile, member_map, grid_x, grid_y) of a fused ensemble stage (swmhd.h)."""
    out = (C.c_int * 8)()
    check(lib().swmhd_ensemble_launch_geometry(Nx, Ny, formulation, elem_size, flags, members, out), "swmhd_ensemble_launch_geometry")
    keys = ("kind", "threads", "tile_columns", "tile_rows", "rows_per_tile", "member_map", "grid_x", "grid_y")
    return dict(zip(keys, list(out)))


def source_hash():
    """sha256 (first 16 hex digits) over the kernel sources libswmhd.so is built from: profiles/ files record it, so that bench.py
    can tell whether a committed counter value still describes the kernels that are running."""
    import glob, hashlib
    h = hashlib.sha256()
    src = os.path.join(_HERE, "csrc")
    for f in sorted(glob.glob(os.path.join(src, "*.hip")) + glob.glob(os.path.join(src, "*.inc")) + glob.glob(os.path.join(src, "*.hpp"))
                    + [os.path.join(src, "Makefile")]):
        h.update(os.path.basename(f).encode()); h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def check(rc, what=""):
    if rc != 0:
        raise SwmhdError(f"{what}: rc={rc}: {lib().swmhd_strerror(rc).decode()}")
