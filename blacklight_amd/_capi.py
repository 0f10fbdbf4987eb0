"""ctypes binding of the C-ABI in include/blacklight_amd.h (libblacklight_amd.so).

Plumbing only: the product is the HIP library. Loading fails loudly if the library has not been
built (python -c "import __graft_entry__ as g; g.build()"); there is no CPU fallback.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# BLACKLIGHT_AMD_LIB: another build of the same library (kernel A/B runs, tools/gpu_ab.sh)
LIB_PATH = os.environ.get("BLACKLIGHT_AMD_LIB") or os.path.join(_HERE, "libblacklight_amd.so")

BL_OK, BL_E_INPUT, BL_E_MISSING, BL_E_UNSUPPORTED, BL_E_DEVICE, BL_E_ARG, BL_E_STATE = range(7)


class GridDesc(C.Structure):
    _fields_ = [
        ("n_blocks", C.c_int32), ("n_i", C.c_int32), ("n_j", C.c_int32), ("n_k", C.c_int32),
        ("n_var", C.c_int32),
        ("prim", C.c_void_p),
        ("x1f", C.c_void_p), ("x2f", C.c_void_p), ("x3f", C.c_void_p),
        ("x1v", C.c_void_p), ("x2v", C.c_void_p), ("x3v", C.c_void_p),
        ("ind_rho", C.c_int32), ("ind_pgas", C.c_int32), ("ind_kappa", C.c_int32),
        ("ind_uu1", C.c_int32), ("ind_uu2", C.c_int32), ("ind_uu3", C.c_int32),
        ("ind_bb1", C.c_int32), ("ind_bb2", C.c_int32), ("ind_bb3", C.c_int32),
        ("plasma_gamma", C.c_double), ("plasma_gamma_i", C.c_double), ("plasma_gamma_e", C.c_double),
        ("levels", C.c_void_p), ("locations", C.c_void_p), ("n_3_root", C.c_int32),
        ("sks_map", C.c_void_p), ("sks_map_n1", C.c_int32), ("sks_map_n2", C.c_int32),
        ("sks_map_r_in", C.c_double), ("sks_map_dr", C.c_double), ("sks_map_dtheta", C.c_double),
        ("simulation_bounds", C.c_double * 6),
    ]


BL_CELLS_F32, BL_CELLS_F64 = 0, 1


class DeviceCells(C.Structure):
    """bl_device_cells: the caller's cells in device memory (bl_set_grid_device); strides and extent in elements."""
    _fields_ = [("prim", C.c_void_p), ("dtype", C.c_int32), ("wait", C.c_int32), ("var_stride", C.c_int64), ("block_stride", C.c_int64),
                ("n_elements", C.c_int64), ("stream", C.c_void_p)]


class HarmHeader(C.Structure):
    """bl_harm_header: what the reader takes from an iharm3d file's header (absent adiabatic index: NaN; absent variable: -1)."""
    _fields_ = [("n1", C.c_int32), ("n2", C.c_int32), ("n3", C.c_int32), ("n_prim", C.c_int32), ("startx", C.c_double * 3), ("dx", C.c_double * 3),
                ("a", C.c_double), ("hslope", C.c_double), ("metric", C.c_int32), ("reserved", C.c_int32),
                ("r_in", C.c_double), ("poly_xt", C.c_double), ("poly_alpha", C.c_double), ("mks_smooth", C.c_double),
                ("gam", C.c_double), ("gam_p", C.c_double), ("gam_e", C.c_double)] + \
               [(name, C.c_int32) for name in ("ind_rho", "ind_uu", "ind_u1", "ind_u2", "ind_u3", "ind_b1", "ind_b2", "ind_b3", "ind_kappa", "reserved2")]


BL_HARM_MKS, BL_HARM_FMKS = 0, 1


class HarmCells(C.Structure):
    """bl_harm_cells: a harm-family code's prims[n1][n2][n3][n_prim] in device memory (bl_set_grid_device_harm)."""
    _fields_ = [("prim", C.c_void_p), ("dtype", C.c_int32), ("wait", C.c_int32), ("n_elements", C.c_int64), ("stream", C.c_void_p)]


BL_MAX_SWEEP = 16


class Sweep(C.Structure):
    """bl_sweep: the sweep_rat_low / sweep_rat_high / sweep_rho_cgs lists of a .input file, kept beside the parameter block."""
    _fields_ = [("n_rat_low", C.c_int32), ("n_rat_high", C.c_int32), ("n_rho_cgs", C.c_int32), ("reserved", C.c_int32),
                ("rat_low", C.c_double * BL_MAX_SWEEP), ("rat_high", C.c_double * BL_MAX_SWEEP), ("rho_cgs", C.c_double * BL_MAX_SWEEP)]


class SweepCuts(C.Structure):
    """bl_sweep_cuts: the sweep_cut_sigma_max list of a .input file, beside bl_sweep (whose size is part of the ABI)."""
    _fields_ = [("n_sigma_max", C.c_int32), ("reserved", C.c_int32), ("sigma_max", C.c_double * BL_MAX_SWEEP)]


class SweepCameras(C.Structure):
    """bl_sweep_cameras: the sweep_camera_th / sweep_camera_ph lists of a .input file (degrees), beside bl_sweep and bl_sweep_cuts."""
    _fields_ = [("n_th", C.c_int32), ("n_ph", C.c_int32), ("th", C.c_double * BL_MAX_SWEEP), ("ph", C.c_double * BL_MAX_SWEEP)]


BL_MAX_CAMERAS = 16


class SweepElectrons(C.Structure):
    """bl_sweep_electrons: the seven electron lists of a .input file (sweep_power_frac ... sweep_w), beside the three structs above."""
    _fields_ = [("n_" + name, C.c_int32) for name in ("power_frac", "p", "gamma_min", "gamma_max", "kappa_frac", "kappa", "w")] + [("reserved", C.c_int32)] + \
               [(name, C.c_double * BL_MAX_SWEEP) for name in ("power_frac", "p", "gamma_min", "gamma_max", "kappa_frac", "kappa", "w")]


class SweepLists(C.Structure):
    """bl_sweep_lists: pointers to the four structs (NULL: that struct's keys are validated and dropped)."""
    _fields_ = [("sweep", C.POINTER(Sweep)), ("cuts", C.POINTER(SweepCuts)), ("cameras", C.POINTER(SweepCameras)), ("electrons", C.POINTER(SweepElectrons))]


class SweepFrequencies(C.Structure):
    """bl_sweep_frequencies: the sweep_frequency list of a .input file (Hz), in a struct of its own beside the four above."""
    _fields_ = [("n", C.c_int32), ("reserved", C.c_int32), ("hz", C.c_double * BL_MAX_SWEEP)]


class SweepAll(C.Structure):
    """bl_sweep_all: pointers to all five structs (NULL: that struct's keys are validated and dropped)."""
    _fields_ = [("sweep", C.POINTER(Sweep)), ("cuts", C.POINTER(SweepCuts)), ("cameras", C.POINTER(SweepCameras)), ("electrons", C.POINTER(SweepElectrons)),
                ("frequencies", C.POINTER(SweepFrequencies))]


BL_MAX_FREQUENCIES = 1024

ELECTRON_MIX_KEYS = ("power_frac", "p", "gamma_min", "gamma_max", "kappa_frac", "kappa", "w")


class ElectronMix(C.Structure):
    """bl_electron_mix: the seven plasma_* values of an electron distribution (bl_set_polarized_variants_electrons)."""
    _fields_ = [(name, C.c_double) for name in ELECTRON_MIX_KEYS + ("reserved",)]


class CameraFrame(C.Structure):
    _fields_ = [(name, C.c_double * 4) for name in
                ("cam_x", "u_con", "u_cov", "norm_con", "norm_con_c", "hor_con_c", "vert_con_c")] + \
               [(name, C.c_double) for name in ("bh_m", "bh_a", "r_horizon", "r_terminate", "mass_msun")]


class RenderDesc(C.Structure):
    _fields_ = [
        ("level", C.c_int32), ("n_blocks", C.c_int32), ("block_locs", C.c_void_p),
        ("n_rays", C.c_int64), ("pixel_map", C.c_void_p), ("outputs_on_device", C.c_int32),
        ("image", C.c_void_p), ("sample_num", C.c_void_p), ("sample_flags", C.c_void_p),
        ("camera_pos", C.c_void_p), ("camera_dir", C.c_void_p), ("render", C.c_void_p),
    ]


# BL_SWITCH_* of include/blacklight_amd.h: measurement switches (bl_stats.switches, bl_debug_set_switches)
SWITCHES = {"TENSOR_TRANSPORT": 1 << 0, "SPLIT_RECORDS": 1 << 1, "RECORD_EVERY_STEP": 1 << 2,
            "GENERAL_LOCATE": 1 << 4, "LANE_TRANSFER": 1 << 5, "NO_FUSED_LOCATE": 1 << 6, "SAMPLE_RECORDS": 1 << 8, "QUAD_EVERY_RAY": 1 << 11,
            "FLAT_ORDER": 1 << 12, "GLOBAL_ANGLES": 1 << 13, "GENERAL_CUTS": 1 << 14, "NO_MIRROR_PAIRS": 1 << 15,
            "EXACT_DISTANCE": 1 << 16, "WIDE_DISTANCE_BAND": 1 << 17}

BL_MAX_LEVELS = 16


class OutputLevel(C.Structure):
    _fields_ = [("n_blocks", C.c_int32), ("block_locs", C.c_void_p), ("image", C.c_void_p), ("camera", C.c_void_p),
                ("render", C.c_void_p)]


class OutputDesc(C.Structure):
    _fields_ = [("adaptive_num_levels", C.c_int32), ("level", OutputLevel * (BL_MAX_LEVELS + 1)),
                ("snapshot", C.c_int32)]


class Stats(C.Structure):
    _fields_ = [
        ("n_rays", C.c_int64), ("n_samples", C.c_int64), ("n_samples_emitted", C.c_int64),
        ("n_gathers", C.c_int64), ("n_flagged", C.c_int64), ("max_sample_num", C.c_int32),
        ("n_chunks", C.c_int32), ("algorithmic_bytes", C.c_double),
        ("ms_geodesic", C.c_float), ("ms_shade", C.c_float), ("ms_transfer", C.c_float),
        ("ms_total", C.c_float),
        ("launches_geodesic", C.c_int32), ("launches_shade", C.c_int32),
        ("launches_transfer", C.c_int32),
        ("ms_locate", C.c_float), ("ms_wall", C.c_float), ("launches_locate", C.c_int32),
        ("arithmetic", C.c_int32), ("mirror_pairs", C.c_int32), ("n_deferred", C.c_int64), ("n_undefined", C.c_int64),
        ("switches", C.c_uint32), ("fused_variant", C.c_int32), ("n_parked", C.c_int64),
        ("composed_maps", C.c_int32), ("tail_policy", C.c_int32), ("geodesics_reused", C.c_int32), ("sampling_reused", C.c_int32),
        ("xcd_order", C.c_int32), ("local_angles", C.c_int32), ("n_cameras", C.c_int32),
    ]

    @property
    def n_mixes(self):
        """bl_stats.n_mixes, the struct's last member: the int32 behind n_cameras, in what were the struct's four bytes of tail
        padding - so the field list above, whose last entry the cameras' host test pins, and the struct's size stay as they are."""
        return C.c_int32.from_buffer(self, Stats.N_MIXES_OFFSET).value


Stats.N_MIXES_OFFSET = Stats.n_cameras.offset + 4
assert Stats.N_MIXES_OFFSET + 4 <= C.sizeof(Stats)


_lib = None


def lib():
    """Load libblacklight_amd.so (once) and declare prototypes."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build the HIP library first "
            "(python -c 'import __graft_entry__ as g; g.build()'). There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    L.bl_params_clear.argtypes = [C.c_void_p]
    L.bl_params_sizeof.restype = C.c_size_t
    L.bl_params_set_line.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_size_t]
    L.bl_params_read_file.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int), C.c_char_p, C.c_size_t]
    L.bl_params_get.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]
    L.bl_params_get_string.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_size_t]
    L.bl_params_set_line_sweep.argtypes = [C.c_void_p, C.POINTER(Sweep), C.c_char_p, C.c_char_p, C.c_size_t]
    L.bl_params_read_file_sweep.argtypes = [C.c_void_p, C.POINTER(Sweep), C.c_char_p, C.POINTER(C.c_int), C.c_char_p, C.c_size_t]
    L.bl_sweep_resolve.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Sweep), C.POINTER(C.c_int), C.c_char_p, C.c_size_t]
    L.bl_apply_sweep.argtypes = [C.c_void_p, C.POINTER(Sweep)]
    L.bl_params_set_line_sweeps.argtypes = [C.c_void_p, C.POINTER(Sweep), C.POINTER(SweepCuts), C.c_char_p, C.c_char_p, C.c_size_t]
    L.bl_params_read_file_sweeps.argtypes = [C.c_void_p, C.POINTER(Sweep), C.POINTER(SweepCuts), C.c_char_p, C.POINTER(C.c_int), C.c_char_p, C.c_size_t]
    L.bl_apply_sweeps.argtypes = [C.c_void_p, C.POINTER(Sweep), C.POINTER(SweepCuts)]
    L.bl_params_set_line_sweeps_cameras.argtypes = [C.c_void_p, C.POINTER(Sweep), C.POINTER(SweepCuts), C.POINTER(SweepCameras), C.c_char_p, C.c_char_p,
                                                    C.c_size_t]
    L.bl_params_read_file_sweeps_cameras.argtypes = [C.c_void_p, C.POINTER(Sweep), C.POINTER(SweepCuts), C.POINTER(SweepCameras), C.c_char_p,
                                                     C.POINTER(C.c_int), C.c_char_p, C.c_size_t]
    L.bl_sweep_cameras_resolve.argtypes = [C.POINTER(SweepCameras), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                           C.c_char_p, C.c_size_t]
    L.bl_apply_sweeps_cameras.argtypes = [C.c_void_p, C.POINTER(Sweep), C.POINTER(SweepCuts), C.POINTER(SweepCameras)]
    L.bl_params_set_line_sweep_lists.argtypes = [C.c_void_p, C.POINTER(SweepLists), C.c_char_p, C.c_char_p, C.c_size_t]
    L.bl_params_read_file_sweep_lists.argtypes = [C.c_void_p, C.POINTER(SweepLists), C.c_char_p, C.POINTER(C.c_int), C.c_char_p, C.c_size_t]
    L.bl_sweep_electrons_resolve.argtypes = [C.POINTER(SweepElectrons), C.POINTER(Sweep), C.c_void_p, C.POINTER(C.c_int), C.POINTER(Sweep), C.c_void_p,
                                             C.c_char_p, C.c_size_t]
    L.bl_apply_sweep_lists.argtypes = [C.c_void_p, C.POINTER(SweepLists)]
    L.bl_params_set_line_sweep_all.argtypes = [C.c_void_p, C.POINTER(SweepAll), C.c_char_p, C.c_char_p, C.c_size_t]
    L.bl_params_read_file_sweep_all.argtypes = [C.c_void_p, C.POINTER(SweepAll), C.c_char_p, C.POINTER(C.c_int), C.c_char_p, C.c_size_t]
    L.bl_apply_sweep_all.argtypes = [C.c_void_p, C.POINTER(SweepAll)]
    L.bl_set_frequencies.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.bl_num_frequencies.argtypes = [C.c_void_p]
    L.bl_write_output_frequency.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(OutputDesc), C.c_int, C.c_int, C.c_int]
    L.bl_frequency_output_path.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t]
    L.bl_set_cameras.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.bl_num_cameras.argtypes = [C.c_void_p]
    L.bl_cameras_get.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.bl_camera_frame_get_camera.argtypes = [C.c_void_p, C.c_int, C.POINTER(CameraFrame)]
    L.bl_write_output_camera.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(OutputDesc), C.c_int, C.c_int]
    L.bl_camera_output_path.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t]
    L.bl_num_variants.argtypes = [C.c_void_p]
    L.bl_variants_get.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
    L.bl_write_output_variant.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(OutputDesc), C.c_int]
    L.bl_variant_output_path.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_size_t]
    L.bl_init.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    L.bl_set_grid.argtypes = [C.c_void_p, C.POINTER(GridDesc)]
    L.bl_set_grid_device.argtypes = [C.c_void_p, C.POINTER(GridDesc), C.POINTER(DeviceCells)]
    L.bl_set_grid_slice_device.argtypes = [C.c_void_p, C.c_int, C.POINTER(GridDesc), C.POINTER(DeviceCells), C.c_double]
    L.bl_device_cells_sizeof.restype = C.c_size_t
    L.bl_grid_host_bytes.argtypes = [C.c_void_p]
    L.bl_grid_host_bytes.restype = C.c_int64
    L.bl_context_device.argtypes = [C.c_void_p]
    L.bl_image_num_quantities.argtypes = [C.c_void_p]
    L.bl_camera_frame_get.argtypes = [C.c_void_p, C.POINTER(CameraFrame)]
    L.bl_frequencies.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int]
    L.bl_set_scratch_limit.argtypes = [C.c_void_p, C.c_uint64]
    L.bl_set_overlap.argtypes = [C.c_void_p, C.c_int]
    L.bl_set_arithmetic.argtypes = [C.c_void_p, C.c_int]
    L.bl_set_reproducible.argtypes = [C.c_void_p, C.c_int]
    L.bl_set_tail_policy.argtypes = [C.c_void_p, C.c_int]
    L.bl_set_geodesic_reuse.argtypes = [C.c_void_p, C.c_int]
    L.bl_set_electron_models.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.bl_num_electron_models.argtypes = [C.c_void_p]
    L.bl_set_density_units.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.bl_num_density_units.argtypes = [C.c_void_p]
    L.bl_set_polarized_variants.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bl_set_polarized_variants_sigma.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bl_num_polarized_variants.argtypes = [C.c_void_p]
    L.bl_set_polarized_variants_electrons.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bl_polarized_variant_electrons.argtypes = [C.c_void_p, C.c_int, C.POINTER(ElectronMix)]
    L.bl_set_sigma_cuts.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.bl_num_sigma_cuts.argtypes = [C.c_void_p]
    L.bl_set_electron_mixes.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.bl_num_electron_mixes.argtypes = [C.c_void_p]
    L.bl_electron_mix_get.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.bl_host_alloc.argtypes = [C.c_void_p, C.c_size_t]
    L.bl_host_alloc.restype = C.c_void_p
    L.bl_host_free.argtypes = [C.c_void_p, C.c_void_p]
    L.bl_set_caller_stream.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.bl_device_count.restype = C.c_int
    L.bl_set_undefined_policy.argtypes = [C.c_void_p, C.c_int]
    L.bl_debug_set_guard_band.argtypes = [C.c_void_p, C.c_double]
    L.bl_debug_set_switches.argtypes = [C.c_void_p, C.c_uint32]
    L.bl_debug_math.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bl_render.argtypes = [C.c_void_p, C.POINTER(RenderDesc)]
    L.bl_get_stats.argtypes = [C.c_void_p, C.POINTER(Stats)]
    L.bl_last_error.argtypes = [C.c_void_p]
    L.bl_last_error.restype = C.c_char_p
    L.bl_last_global_error.restype = C.c_char_p
    L.bl_warnings.argtypes = [C.c_void_p]
    L.bl_warnings.restype = C.c_char_p
    L.bl_adaptive_refine.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.POINTER(C.c_int32), C.c_void_p]
    L.bl_adaptive_refine_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.POINTER(C.c_int32), C.c_void_p]
    L.bl_write_output.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(OutputDesc)]
    L.bl_free.argtypes = [C.c_void_p]
    L.bl_snapshot_open.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t]
    L.bl_snapshot_grid.argtypes = [C.c_void_p]
    L.bl_snapshot_grid.restype = C.POINTER(GridDesc)
    L.bl_snapshot_time.argtypes = [C.c_void_p]
    L.bl_snapshot_time.restype = C.c_double
    L.bl_snapshot_warnings.argtypes = [C.c_void_p]
    L.bl_snapshot_warnings.restype = C.c_char_p
    L.bl_snapshot_file.argtypes = [C.c_void_p]
    L.bl_snapshot_file.restype = C.c_char_p
    L.bl_snapshot_blocks.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_int32)), C.POINTER(C.POINTER(C.c_int32))]
    L.bl_snapshot_close.argtypes = [C.c_void_p]
    L.bl_snapshot_open_number.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t]
    L.bl_snapshot_open_raw.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t]
    L.bl_snapshot_harm_header.argtypes = [C.c_void_p, C.POINTER(HarmHeader)]
    L.bl_snapshot_harm_prims.argtypes = [C.c_void_p]
    L.bl_snapshot_harm_prims.restype = C.c_void_p
    L.bl_harm_header_sizeof.restype = C.c_size_t
    L.bl_harm_cells_sizeof.restype = C.c_size_t
    L.bl_harm_grid_create.argtypes = [C.c_void_p, C.POINTER(HarmHeader), C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t]
    L.bl_harm_grid_desc.argtypes = [C.c_void_p, C.c_int]
    L.bl_harm_grid_desc.restype = C.POINTER(GridDesc)
    L.bl_harm_grid_warnings.argtypes = [C.c_void_p]
    L.bl_harm_grid_warnings.restype = C.c_char_p
    L.bl_harm_grid_planes.argtypes = [C.c_void_p]
    L.bl_harm_grid_free.argtypes = [C.c_void_p]
    L.bl_harm_convert_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.bl_set_grid_device_harm.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(HarmCells)]
    L.bl_set_grid_slice_device_harm.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(HarmCells), C.c_double]
    L.bl_harm_convert_device.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(HarmCells), C.c_void_p]
    L.bl_slow_light_read.argtypes = [C.c_void_p, C.c_int]
    L.bl_set_grid_slice.argtypes = [C.c_void_p, C.c_int, C.POINTER(GridDesc), C.c_double]
    L.bl_shift_grid_slices.argtypes = [C.c_void_p, C.c_int]
    L.bl_set_snapshot.argtypes = [C.c_void_p, C.c_int]
    L.bl_warnings_clear.argtypes = [C.c_void_p]
    L.bl_build_info.restype = C.c_char_p
    _lib = L
    return L


class BlacklightError(RuntimeError):
    """Raised with the reference-style 'Error: ...' text of a failed C-ABI call."""

    def __init__(self, code, message):
        super().__init__(message.strip() or f"blacklight_amd error code {code}")
        self.code = code
