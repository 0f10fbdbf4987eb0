/* blacklight_amd.h - C-ABI of the MI355X-native hot path of blacklight (c-white/blacklight).
 *
 * The reference has no plugin / FFI boundary: its hot path is entered by three C++ member calls
 * made from main() (reference src/blacklight.cpp:93-94, 203-204, 221):
 *
 *     double GeodesicIntegrator::Integrate()                      geodesic_integrator.cpp:194
 *     bool   RadiationIntegrator::Integrate(int, double*, ...)    radiation_integrator.cpp:676
 *     double GeodesicIntegrator::AddGeodesics(RadiationIntegrator*) geodesic_integrator.cpp:236
 *
 * with inputs = the InputReader fields copied in the two constructors
 * (geodesic_integrator.cpp:26-104, radiation_integrator.cpp:30-357) plus the read-only grid arrays
 * owned by SimulationReader (simulation_sampling.cpp:38-78), and outputs = image[level](n_q,n_pix),
 * sample_num, sample_flags, camera_pos/dir (output_writer.cpp:116-124, 172-246).
 *
 * This header is the drop-in replacement for exactly that surface, as plain C: a parameter block
 * that mirrors InputReader key-for-key (bl_params), a borrowed view of the grid (bl_grid_desc), and
 * one call per adaptive level (bl_render) that runs camera + geodesics + sampling + coefficients +
 * transfer on the GPU. No C++ or torch types cross the boundary; every function returns 0 on
 * success or a BL_E_* code, with the message text (identical to the reference's where the
 * reference has one) available from bl_last_error().
 */
#ifndef BLACKLIGHT_AMD_H_
#define BLACKLIGHT_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BL_API __attribute__((visibility("default")))

/* ------------------------------------------------------------------ error codes */
enum {
  BL_OK = 0,
  BL_E_INPUT = 1,      /* malformed .input file or bad value: message = reference text            */
  BL_E_MISSING = 2,    /* a required key is absent (reference: std::bad_optional_access)          */
  BL_E_UNSUPPORTED = 3,/* valid reference configuration outside the hot-path scope of this build  */
  BL_E_DEVICE = 4,     /* HIP runtime failure or no gfx950 device                                 */
  BL_E_ARG = 5,        /* bad argument to the C-ABI itself                                        */
  BL_E_STATE = 6       /* call out of order (e.g. simulation render before bl_set_grid)           */
};

/* ------------------------------------------------------------------ enumerations
 * Same members, same order as reference src/blacklight.hpp:36-46. */
enum { BL_MODEL_SIMULATION = 0, BL_MODEL_FORMULA = 1 };
enum { BL_OUTPUT_NPZ = 0, BL_OUTPUT_NPY = 1, BL_OUTPUT_RAW = 2 };
enum { BL_SIMFMT_ATHENA = 0, BL_SIMFMT_ATHENAK = 1, BL_SIMFMT_IHARM3D = 2, BL_SIMFMT_HARM3D = 3 };
enum { BL_COORD_CKS = 0, BL_COORD_SKS = 1, BL_COORD_FMKS = 2 };
enum { BL_CAMERA_PLANE = 0, BL_CAMERA_PINHOLE = 1 };
enum { BL_TERMINATE_PHOTON = 0, BL_TERMINATE_MULTIPLICATIVE = 1, BL_TERMINATE_ADDITIVE = 2 };
enum { BL_INTEGRATOR_DP = 0, BL_INTEGRATOR_RK4 = 1, BL_INTEGRATOR_RK2 = 2 };
enum { BL_SPACING_LIN_FREQ = 0, BL_SPACING_LIN_WAVE = 1, BL_SPACING_LOG = 2 };
enum { BL_NORM_CAMERA = 0, BL_NORM_INFINITY = 1 };
enum { BL_PLASMA_TI_TE_BETA = 0, BL_PLASMA_CODE_KAPPA = 1 };

#define BL_STR_LEN 512
#define BL_MAX_REGIONS 32

/* ------------------------------------------------------------------ parameter block
 * One entry per key of the reference's .input grammar (src/input_reader/input_reader.cpp:101-407),
 * in the same order. X(kind, name):
 *   B bool (int32 0/1)   I int32   D double   F float   S string   E enum (int32)
 *   G double given in degrees in the file, stored in radians as val * pi / 180
 *     (input_reader.cpp:185-201, 389)
 * camera_th additionally sets camera_pole when the written value is exactly 0 or 180
 * (input_reader.cpp:492-500).
 */
#define BL_PARAM_LIST(X) \
  X(E, model_type) X(I, num_threads) \
  X(E, output_format) X(S, output_file) X(B, output_camera) \
  X(B, checkpoint_geodesic_save) X(B, checkpoint_geodesic_load) X(S, checkpoint_geodesic_file) \
  X(B, checkpoint_sample_save) X(B, checkpoint_sample_load) X(S, checkpoint_sample_file) \
  X(E, simulation_format) X(S, simulation_file) X(B, simulation_multiple) X(I, simulation_start) \
  X(I, simulation_end) X(E, simulation_coord) X(D, simulation_a) X(D, simulation_m_msun) \
  X(D, simulation_rho_cgs) X(S, simulation_kappa_name) X(B, simulation_interp) \
  X(B, simulation_block_interp) \
  X(D, formula_mass) X(D, formula_spin) X(D, formula_r0) X(D, formula_h) X(D, formula_l0) \
  X(D, formula_q) X(D, formula_nup) X(D, formula_cn0) X(D, formula_alpha) X(D, formula_a) \
  X(D, formula_beta) \
  X(E, camera_type) X(D, camera_r) X(G, camera_th) X(G, camera_ph) X(D, camera_urn) \
  X(D, camera_uthn) X(D, camera_uphn) X(D, camera_k_r) X(D, camera_k_th) X(D, camera_k_ph) \
  X(G, camera_rotation) X(D, camera_width) X(I, camera_resolution) X(B, camera_pole) \
  X(B, ray_flat) X(E, ray_terminate) X(D, ray_factor) X(E, ray_integrator) X(D, ray_step) \
  X(I, ray_max_steps) X(I, ray_max_retries) X(D, ray_tol_abs) X(D, ray_tol_rel) \
  X(B, image_light) X(I, image_num_frequencies) X(D, image_frequency) X(D, image_frequency_start) \
  X(D, image_frequency_end) X(E, image_frequency_spacing) X(E, image_normalization) \
  X(B, image_polarization) X(B, image_rotation_split) X(B, image_time) X(B, image_length) \
  X(B, image_lambda) X(B, image_emission) X(B, image_tau) X(B, image_lambda_ave) \
  X(B, image_emission_ave) X(B, image_tau_int) X(B, image_crossings) \
  X(I, render_num_images) \
  X(B, slow_light_on) X(B, slow_interp) X(I, slow_chunk_size) X(D, slow_t_start) X(D, slow_dt) \
  X(I, slow_num_images) X(I, slow_offset) \
  X(I, adaptive_max_level) X(I, adaptive_block_size) X(I, adaptive_frequency_num) \
  X(D, adaptive_val_cut) X(D, adaptive_val_frac) X(D, adaptive_abs_grad_cut) \
  X(D, adaptive_abs_grad_frac) X(D, adaptive_rel_grad_cut) X(D, adaptive_rel_grad_frac) \
  X(D, adaptive_abs_lapl_cut) X(D, adaptive_abs_lapl_frac) X(D, adaptive_rel_lapl_cut) \
  X(D, adaptive_rel_lapl_frac) X(I, adaptive_num_regions) \
  X(D, plasma_mu) X(D, plasma_ne_ni) X(E, plasma_model) X(B, plasma_use_p) X(D, plasma_gamma) \
  X(D, plasma_gamma_i) X(D, plasma_gamma_e) X(D, plasma_rat_low) X(D, plasma_rat_high) \
  X(D, plasma_power_frac) X(D, plasma_p) X(D, plasma_gamma_min) X(D, plasma_gamma_max) \
  X(D, plasma_kappa_frac) X(D, plasma_kappa) X(D, plasma_w) \
  X(D, cut_rho_min) X(D, cut_rho_max) X(D, cut_n_e_min) X(D, cut_n_e_max) X(D, cut_p_gas_min) \
  X(D, cut_p_gas_max) X(D, cut_theta_e_min) X(D, cut_theta_e_max) X(D, cut_b_min) X(D, cut_b_max) \
  X(D, cut_sigma_min) X(D, cut_sigma_max) X(D, cut_beta_inverse_min) X(D, cut_beta_inverse_max) \
  X(B, cut_omit_near) X(B, cut_omit_far) X(D, cut_omit_in) X(D, cut_omit_out) \
  X(G, cut_midplane_theta) X(D, cut_midplane_z) X(B, cut_plane) \
  X(D, cut_plane_origin_x) X(D, cut_plane_origin_y) X(D, cut_plane_origin_z) \
  X(D, cut_plane_normal_x) X(D, cut_plane_normal_y) X(D, cut_plane_normal_z) \
  X(B, fallback_nan) X(F, fallback_rho) X(F, fallback_pgas) X(F, fallback_kappa)

typedef struct bl_str { char s[BL_STR_LEN]; } bl_str;

#define BL_PT_B int32_t
#define BL_PT_I int32_t
#define BL_PT_E int32_t
#define BL_PT_D double
#define BL_PT_G double
#define BL_PT_F float
#define BL_PT_S bl_str
#define BL_X_FIELD(kind, name) BL_PT_##kind name;
#define BL_X_INDEX(kind, name) BL_P_##name,

enum { BL_PARAM_LIST(BL_X_INDEX) BL_P_COUNT };

/* False-colour rendering (rendering.cpp): bounds of this build and enumerations */
#define BL_MAX_RENDER_IMAGES 4
#define BL_MAX_RENDER_FEATURES 16
enum { BL_RENDER_FILL = 0, BL_RENDER_THRESH = 1, BL_RENDER_RISE = 2, BL_RENDER_FALL = 3 };
enum { BL_RENDER_HAS_QUANTITY = 1, BL_RENDER_HAS_TYPE = 2, BL_RENDER_HAS_MIN = 4, BL_RENDER_HAS_MAX = 8,
       BL_RENDER_HAS_THRESH = 16, BL_RENDER_HAS_TAU_SCALE = 32, BL_RENDER_HAS_OPACITY = 64, BL_RENDER_HAS_XYZ = 128 };

typedef struct bl_params {
  /* has[i] != 0 iff field i (enum BL_P_*) was given: the std::optional of the reference */
  uint8_t has[((BL_P_COUNT + 7) / 8) * 8];
  BL_PARAM_LIST(BL_X_FIELD)
  /* adaptive_region_<n>_{level,x_min,x_max,y_min,y_max}  (src/input_reader/adaptive_reader.cpp) */
  int32_t adaptive_region_has[BL_MAX_REGIONS];     /* bit 0..4 = level, x_min, x_max, y_min, y_max */
  int32_t adaptive_region_level[BL_MAX_REGIONS];
  double adaptive_region_x_min[BL_MAX_REGIONS];
  double adaptive_region_x_max[BL_MAX_REGIONS];
  double adaptive_region_y_min[BL_MAX_REGIONS];
  double adaptive_region_y_max[BL_MAX_REGIONS];
  /* render_<i>_num_features, render_<i>_<f>_{quantity,type,min,max,thresh,tau_scale,opacity,rgb|xyz}
   * (src/input_reader/render_reader.cpp); indices beyond render_num_images / num_features are ignored
   * as there, indices beyond BL_MAX_RENDER_* are an error of this build */
  int32_t render_num_features_has[BL_MAX_RENDER_IMAGES];
  int32_t render_num_features[BL_MAX_RENDER_IMAGES];
  int32_t render_has[BL_MAX_RENDER_IMAGES][BL_MAX_RENDER_FEATURES];   /* BL_RENDER_HAS_* bits */
  int32_t render_quantity[BL_MAX_RENDER_IMAGES][BL_MAX_RENDER_FEATURES];   /* cell value index 0..6 */
  int32_t render_type[BL_MAX_RENDER_IMAGES][BL_MAX_RENDER_FEATURES];       /* BL_RENDER_* */
  double render_min[BL_MAX_RENDER_IMAGES][BL_MAX_RENDER_FEATURES];
  double render_max[BL_MAX_RENDER_IMAGES][BL_MAX_RENDER_FEATURES];
  double render_thresh[BL_MAX_RENDER_IMAGES][BL_MAX_RENDER_FEATURES];
  double render_tau_scale[BL_MAX_RENDER_IMAGES][BL_MAX_RENDER_FEATURES];
  double render_opacity[BL_MAX_RENDER_IMAGES][BL_MAX_RENDER_FEATURES];
  double render_x[BL_MAX_RENDER_IMAGES][BL_MAX_RENDER_FEATURES];      /* XYZ colour (D65), rgb keys converted */
  double render_y[BL_MAX_RENDER_IMAGES][BL_MAX_RENDER_FEATURES];
  double render_z[BL_MAX_RENDER_IMAGES][BL_MAX_RENDER_FEATURES];
} bl_params;

/* Zero a parameter block (nothing present). */
BL_API void bl_params_clear(bl_params *p);
BL_API size_t bl_params_sizeof(void);
/* Parse one "key = value" assignment exactly as a line of the .input file would be
 * (whitespace stripped, '#' comments removed); err receives "Error: ...\n" text on failure. */
BL_API int bl_params_set_line(bl_params *p, const char *line, char *err, size_t err_len);
/* Parse a whole .input file: replaces InputReader::Read() (input_reader.cpp:72-428).
 * *num_runs receives the run count (1 unless simulation_multiple). */
BL_API int bl_params_read_file(bl_params *p, const char *path, int *num_runs, char *err,
                               size_t err_len);
/* Typed read-back by key name (used by the Python host layer and the tests). */
BL_API int bl_params_get(const bl_params *p, const char *key, double *value, int *present);
BL_API int bl_params_get_string(const bl_params *p, const char *key, char *out, size_t out_len);

/* ------------------------------------------------------------------ sweeps written in the .input file
 * Four keys the reference does not have; a file without them parses exactly as before, and they never enter bl_params:
 *     sweep_rat_low  = 1, 1, 1          (R_low, R_high) pairs: two lists of equal length
 *     sweep_rat_high = 10, 40, 160
 *     sweep_rho_cgs  = 1e-16, 2e-16     density units (simulation_rho_cgs values), each finite and > 0
 * At most BL_MAX_SWEEP entries per list; an entry is a whole number text ("1e-16", not "1e-16g"), none is empty.
 * image_polarization = false: the pairs are electron models (bl_set_electron_models), the units density units
 *   (bl_set_density_units); the image is their product, model-major. Either list may be absent: the block's own value.
 * image_polarization = true: (R_low, R_high, unit) triples (bl_set_polarized_variants). sweep_rho_cgs has the pairs' length, or
 *   one entry (every pair at that unit), or is absent (every pair at the block's simulation_rho_cgs); units without pairs: the
 *   block's pair at each unit.
 * bl_params_set_line / bl_params_read_file accept and validate the keys and drop their values; the two calls below keep them.
 * n_* = 0: key absent. Errors (BL_E_INPUT, "Error: ...\n"): an empty entry, a text that is not a number, a unit that is not finite
 * and > 0, more than BL_MAX_SWEEP entries - when the line is read; lists whose lengths do not fit each other - at the end of
 * bl_params_read_file*, in bl_sweep_resolve and in bl_apply_sweep. What the setters refuse (formula mode, slow light, code_kappa
 * for pairs, adaptive runs, renderings a variant enters, a ratio that is not finite) is refused by them, in their words. */
#define BL_MAX_SWEEP 16
typedef struct bl_sweep {
  int32_t n_rat_low, n_rat_high, n_rho_cgs;
  int32_t reserved;
  double rat_low[BL_MAX_SWEEP], rat_high[BL_MAX_SWEEP], rho_cgs[BL_MAX_SWEEP];
} bl_sweep;
BL_API int bl_params_set_line_sweep(bl_params *p, bl_sweep *sweep, const char *line, char *err, size_t err_len);
BL_API int bl_params_read_file_sweep(bl_params *p, bl_sweep *sweep, const char *path, int *num_runs, char *err, size_t err_len);
/* The lists as the setters will receive them. Unpolarized block: *resolved = *sweep. Polarized block (*polarized = 1) with any
 * list given: all three lists of *resolved have the number of triples, filled by the rule above. resolved, polarized may be NULL. */
BL_API int bl_sweep_resolve(const bl_sweep *sweep, const bl_params *p, bl_sweep *resolved, int *polarized, char *err, size_t err_len);
/* The fourth key, beside bl_sweep (whose size is part of the ABI):
 *     sweep_cut_sigma_max = 1, 3, 10, -1     sigma cuts (cut_sigma_max values; negative: the cut off), each finite
 * The same list forms and error texts with the key's name, and one of its own: "Invalid sigma cut (<text>) in list
 * (sweep_cut_sigma_max) in input file: must be finite." The cuts are an axis of their own (bl_set_sigma_cuts): the image is
 * models x units x cuts. The calls above accept and validate the key and drop its value; the two below keep it (sweep, cuts may
 * be NULL: dropped). */
typedef struct bl_sweep_cuts {
  int32_t n_sigma_max, reserved;
  double sigma_max[BL_MAX_SWEEP];
} bl_sweep_cuts;
BL_API int bl_params_set_line_sweeps(bl_params *p, bl_sweep *sweep, bl_sweep_cuts *cuts, const char *line, char *err, size_t err_len);
BL_API int bl_params_read_file_sweeps(bl_params *p, bl_sweep *sweep, bl_sweep_cuts *cuts, const char *path, int *num_runs, char *err, size_t err_len);

/* The fifth and sixth key, in a third struct beside the two above (whose sizes are part of the ABI):
 *     sweep_camera_th = 17, 60, 163     cameras (bl_set_cameras): camera_th values in degrees - a list of (th, ph) pairs, not a product
 *     sweep_camera_ph = 0, 0, 90        camera_ph values: the same length, or one entry (every th at that ph), or absent (every th at
 *                                       the block's camera_ph); ph without th: the block's camera_th at each ph
 * The same list forms and error texts with the key's name, and two of their own: "Invalid angle (<text>) in list (<key>) in input
 * file: must be finite." and - at the end of bl_params_read_file*, in bl_sweep_cameras_resolve and in bl_apply_sweeps_cameras -
 * "sweep_camera_ph must have one entry or as many as sweep_camera_th (<n_ph> and <n_th>) in input file." Every call above accepts
 * and validates the keys and drops their values; the two below keep them (any of sweep, cuts, cameras may be NULL: dropped). */
typedef struct bl_sweep_cameras {
  int32_t n_th, n_ph;
  double th[BL_MAX_SWEEP], ph[BL_MAX_SWEEP];
} bl_sweep_cameras;
BL_API int bl_params_set_line_sweeps_cameras(bl_params *p, bl_sweep *sweep, bl_sweep_cuts *cuts, bl_sweep_cameras *cameras, const char *line,
                                             char *err, size_t err_len);
BL_API int bl_params_read_file_sweeps_cameras(bl_params *p, bl_sweep *sweep, bl_sweep_cuts *cuts, bl_sweep_cameras *cameras, const char *path,
                                              int *num_runs, char *err, size_t err_len);
/* The cameras the two lists mean: *n of them (0: neither key given), th_deg[c] and ph_deg[c] filled for the angles the lists give
 * (arrays of BL_MAX_SWEEP), *th_given / *ph_given = 0 where that angle is the parameter block's own for every camera. Any output may
 * be NULL. */
BL_API int bl_sweep_cameras_resolve(const bl_sweep_cameras *cameras, int *n, double *th_deg, double *ph_deg, int *th_given, int *ph_given,
                                    char *err, size_t err_len);

/* Seven more keys, in a fourth struct beside the three above (whose sizes are part of the ABI) - each is "sweep_" and a plasma_ key
 * without its prefix, the electron distribution of a polarized variant (bl_set_polarized_variants_electrons):
 *     sweep_power_frac = 0, 0.3, 0.2        plasma_power_frac      sweep_kappa_frac = 0.4, 0, 0.25     plasma_kappa_frac
 *     sweep_p          = 2.5                plasma_p               sweep_kappa      = 4, 4, 4.3        plasma_kappa
 *     sweep_gamma_min  = 2                  plasma_gamma_min       sweep_w          = 1.5, 1.5, 2.5    plasma_w
 *     sweep_gamma_max  = 1000               plasma_gamma_max
 * The same list forms and error texts with the key's name, and one of their own: "Invalid value (<text>) in list (<key>) in input
 * file: must be finite." Polarized blocks only; with sweep_rat_low, sweep_rat_high and sweep_rho_cgs they form a LIST OF TUPLES, not
 * a product. N is the number of triples those three keys give where pairs or units are written (the rule above), else the longest
 * electron list. Every electron list has N entries, or one (every variant at that value), or is absent (the block's value). Anything
 * else: "sweep_<key> must have one entry or as many as the other sweep lists (<n> and <N>) in input file."; an electron key in a
 * block that is not polarized: "sweep_<key> needs image_polarization = true in input file." - both BL_E_INPUT, raised at the end of
 * every bl_params_read_file*, in bl_sweep_electrons_resolve and in bl_apply_sweep_lists, as the camera lists' are. What the setter
 * checks (kappa within [3.5, 5], ...) it checks, in its words. n_* = 0: key absent.
 * Every parser call above accepts and validates the seven keys and drops their values; a file without them parses, applies and
 * renders exactly as before. The calls below keep every list, and are the ones a next key will be added to: bl_sweep_lists names
 * the structs (a NULL member: that struct's keys are validated and dropped). */
typedef struct bl_sweep_electrons {
  int32_t n_power_frac, n_p, n_gamma_min, n_gamma_max, n_kappa_frac, n_kappa, n_w;
  int32_t reserved;
  double power_frac[BL_MAX_SWEEP], p[BL_MAX_SWEEP], gamma_min[BL_MAX_SWEEP], gamma_max[BL_MAX_SWEEP];
  double kappa_frac[BL_MAX_SWEEP], kappa[BL_MAX_SWEEP], w[BL_MAX_SWEEP];
} bl_sweep_electrons;
typedef struct bl_sweep_lists {
  bl_sweep *sweep;
  bl_sweep_cuts *cuts;
  bl_sweep_cameras *cameras;
  bl_sweep_electrons *electrons;
} bl_sweep_lists;   /* NULL member: dropped */
BL_API int bl_params_set_line_sweep_lists(bl_params *p, const bl_sweep_lists *lists, const char *line, char *err, size_t err_len);
BL_API int bl_params_read_file_sweep_lists(bl_params *p, const bl_sweep_lists *lists, const char *path, int *num_runs, char *err, size_t err_len);
/* The tuples the electron lists and the three lists of `sweep` (NULL: none written) mean together: *n of them (0: no list of either
 * kind that makes variants), *resolved the N triples as bl_sweep_resolve gives them - the block's pair and unit N times where only
 * electron lists are written - and mix[v] variant v's distribution (an array of BL_MAX_SWEEP), the block's value where a list is
 * absent. Without an electron list this is bl_sweep_resolve with the block's mix N times. Any output may be NULL. */
struct bl_electron_mix;
BL_API int bl_sweep_electrons_resolve(const bl_sweep_electrons *e, const bl_sweep *sweep, const bl_params *p, int *n, bl_sweep *resolved,
                                      struct bl_electron_mix *mix, char *err, size_t err_len);

/* One key more, in a fifth struct beside the four above (whose sizes, and bl_sweep_lists' four members, are part of the ABI):
 *     sweep_frequency = 86e9, 230e9, 345e9     observing frequencies in Hz (bl_set_frequencies), each finite and > 0
 * The same list forms and error texts with the key's name, and one of its own: "Invalid frequency (<text>) in list
 * (sweep_frequency) in input file: must be finite and positive." The list replaces the block's frequencies for the run - the block
 * must still be valid on its own - and is an axis of its own: one render per snapshot covers every frequency beside whatever variants
 * and cameras the file also sweeps, and one file of the reference's layout is written per (camera, frequency, variant), tagged fFF
 * (bl_write_output_frequency). Every parser call above accepts and validates the key and drops its values. bl_sweep_all names all
 * five structs (a NULL member: that struct's keys are validated and dropped); the bl_sweep_lists calls forward to the calls below
 * with `frequencies` NULL. n = 0: key absent. */
typedef struct bl_sweep_frequencies {
  int32_t n, reserved;
  double hz[BL_MAX_SWEEP];
} bl_sweep_frequencies;
typedef struct bl_sweep_all {
  bl_sweep *sweep;
  bl_sweep_cuts *cuts;
  bl_sweep_cameras *cameras;
  bl_sweep_electrons *electrons;
  bl_sweep_frequencies *frequencies;
} bl_sweep_all;   /* NULL member: dropped */
BL_API int bl_params_set_line_sweep_all(bl_params *p, const bl_sweep_all *lists, const char *line, char *err, size_t err_len);
BL_API int bl_params_read_file_sweep_all(bl_params *p, const bl_sweep_all *lists, const char *path, int *num_runs, char *err, size_t err_len);

/* ------------------------------------------------------------------ grid view
 * What RadiationIntegrator::ObtainGridData() takes from SimulationReader
 * (simulation_sampling.cpp:26-95). All pointers are host pointers borrowed for the duration of
 * bl_set_grid(); layouts are the reference's Array<T> layouts (n1 fastest):
 *   prim  float  [n_var][n_blocks][n_k][n_j][n_i]     simulation_reader.cpp:767-780
 *   x1f   double [n_blocks][n_i+1], x1v double [n_blocks][n_i]  (x2*, x3* alike)
 * Coordinates are the values the reader hands over, i.e. file float32 promoted to double
 * (simulation_reader.cpp:615-620) after its angular-range fix (:724-758). */
typedef struct bl_grid_desc {
  int32_t n_blocks, n_i, n_j, n_k, n_var;
  const float *prim;
  const double *x1f, *x2f, *x3f, *x1v, *x2v, *x3v;
  int32_t ind_rho, ind_pgas, ind_kappa, ind_uu1, ind_uu2, ind_uu3, ind_bb1, ind_bb2, ind_bb3;
  double plasma_gamma, plasma_gamma_i, plasma_gamma_e; /* possibly modified by the reader */
  /* MeshBlock table, read only with simulation_block_interp = true (simulation_sampling.cpp:36-39, :84-93):
   * refinement level of each block, its logical location (i, j, k) on that level, and the number of cells
   * of the root grid in x^3 (RootGridSize[2]). NULL / 0 otherwise. */
  const int32_t *levels;      /* [n_blocks] */
  const int32_t *locations;   /* [n_blocks][3] */
  int32_t n_3_root;
  /* simulation_coord = fmks (iharm3d FMKS / MMKS grids; simulation_sampling.cpp:66-73, :190-198, :396-456): x1f ... x3v
   * stay in the file's native coordinates (x^1 = log r, x^2 in [0, 1], x^3 = phi, one block, uniform), and a sample's
   * position on them comes from the reader's look-up table from spherical Kerr-Schild (r, theta) to (x^1, x^2)
   * (SimulationReader::GenerateSKSMap, simulation_geometry.cpp:321-419) within the grid's bounds in (r, theta, phi)
   * (simulation_bounds, :46-57). NULL / 0 for every other coordinate system. */
  const double *sks_map;      /* [2][sks_map_n2][sks_map_n1]: x^1, then x^2 */
  int32_t sks_map_n1, sks_map_n2;
  double sks_map_r_in, sks_map_dr, sks_map_dtheta;
  double simulation_bounds[6];   /* r_min, r_max, theta_min, theta_max, phi_min, phi_max */
} bl_grid_desc;

/* ------------------------------------------------------------------ snapshot reader (host only)
 * SimulationReader for simulation_format = athena: constructor checks (simulation_reader.cpp:36-159),
 * Read() (:211-861: file name for `snapshot` via FormatFilename :870-904, Time, Levels, LogicalLocations,
 * coordinates with the angular-range fix :722-758, VerifyVariablesAthena :1141-1216, "prim" + "B" cell
 * data :761-781) over the subset of HDF5 the reference decodes by hand (hdf5_format_*.cpp: superblock 0,
 * version-1 B-trees / heaps / object headers / attributes, contiguous version-3 layouts). The snapshot
 * owns the arrays bl_snapshot_grid() points to; hand that view to bl_set_grid(), then close the snapshot.
 * err receives "Error: ...\n" (reference texts). Each call reads its file completely; the reference
 * re-uses block layout and coordinates of the first file for later files of a series.
 * simulation_format = athenak: the AthenaK binary dump reader (simulation_reader.cpp:915-1131, :434-589) behind the same calls.
 * simulation_format = iharm3d / harm3d: modified Kerr-Schild (MKS) dumps read with simulation_coord = sks (coordinates and
 * vector components converted like SimulationReader does); iharm3d FMKS / MMKS dumps read with simulation_coord = fmks
 * (native coordinates kept, bl_grid_desc::sks_map built). With slow_light_on use bl_slow_light_read(). */
typedef struct bl_snapshot bl_snapshot;
BL_API int bl_snapshot_open(const bl_params *p, int snapshot, bl_snapshot **out, char *err, size_t err_len);
BL_API const bl_grid_desc *bl_snapshot_grid(const bl_snapshot *s);
BL_API double bl_snapshot_time(const bl_snapshot *s);              /* file attribute "Time"           */
BL_API const char *bl_snapshot_warnings(const bl_snapshot *s);     /* "Warning: ...\n" lines           */
/* How many leading bytes of bl_snapshot_warnings() stem from SimulationReader's constructor checks (the reference
 * prints those before RadiationIntegrator's constructor warnings - bl_warnings() after bl_init() - and the file's
 * own warnings after them). */
BL_API size_t bl_snapshot_setup_warning_bytes(const bl_snapshot *s);
BL_API const char *bl_snapshot_file(const bl_snapshot *s);         /* file name actually opened       */
/* MeshBlock table: returns n_blocks; *levels -> [n_blocks], *locations -> [n_blocks][3] */
BL_API int bl_snapshot_blocks(const bl_snapshot *s, const int32_t **levels, const int32_t **locations);
BL_API void bl_snapshot_close(bl_snapshot *s);
/* Open file number `file_number` of the series (simulation_file with its {Nd} field filled in), whatever
 * simulation_multiple / slow_light_on say: the building block of bl_slow_light_read(). */
BL_API int bl_snapshot_open_number(const bl_params *p, int file_number, bl_snapshot **out, char *err, size_t err_len);

/* ------------------------------------------------------------------ iharm3d-family primitives (host side; no HIP call)
 * iharm3d, KHARMA and their kin hold prims[n1][n2][n3][n_prim]: density, internal energy UU, velocity U1..U3 and field B1..B3 on
 * the basis of their modified (MKS) or funky modified (FMKS / MMKS) Kerr-Schild coordinates. What the sampler reads is
 * [var][k][j][i] with pressure, normal-frame velocity and lab-frame field on the spherical Kerr-Schild basis: the reference's
 * ConvertCoordinates and ConvertPrimitives3 (simulation_geometry.cpp:29-230). The calls below do to a header and a cell array in
 * memory what the reader does to a file, with the reader's error and warning texts and cells equal to its cells bit for bit; the
 * device calls (bl_set_grid_device_harm, further down) run the same conversion on arrays in device memory.
 * bl_harm_header: the numbers the reader takes from the file. Absent adiabatic indices are NaN, an absent variable is index -1. */
#define BL_HARM_MKS 0    /* header/metric = MKS                                                        */
#define BL_HARM_FMKS 1   /* header/metric = FMKS or MMKS: r_in, poly_xt, poly_alpha, mks_smooth are read */
typedef struct bl_harm_header {
  int32_t n1, n2, n3, n_prim;
  double startx[3], dx[3];       /* header/geom/startx1..3, dx1..3                                  */
  double a, hslope;              /* header/geom/<metric>/a, hslope                                  */
  int32_t metric, reserved;      /* BL_HARM_MKS | BL_HARM_FMKS                                      */
  double r_in, poly_xt, poly_alpha, mks_smooth;
  double gam, gam_p, gam_e;      /* header/gam, gam_p, gam_e; NaN: not in the file                  */
  int32_t ind_rho, ind_uu, ind_u1, ind_u2, ind_u3, ind_b1, ind_b2, ind_b3;   /* "RHO", "UU", "U1" ... "B3" in header/prim_names */
  int32_t ind_kappa, reserved2;  /* simulation_kappa_name; read with plasma_model = code_kappa      */
} bl_harm_header;
BL_API size_t bl_harm_header_sizeof(void);
/* The grid of a header under the parameters `p` (simulation_coord = sks: coordinates converted to r, theta; fmks: kept native, with
 * bounds and look-up table; simulation_a, the plasma model and the adiabatic indices as the reader treats them), and the table of the
 * conversion's per-point factors. err receives "Error: ...\n" with the reader's texts ("Array dimension mismatch.", "Unable to locate
 * \"U1\" slice of \"prims\" in data file.", "simulation_coord = fmks needs a file whose header/metric is FMKS or MMKS.", ...);
 * bl_harm_grid_warnings the reader's "Warning: ...\n" lines (spin and adiabatic indices that differ from the input's). One refusal
 * is this call's own (BL_E_UNSUPPORTED): with plasma_model = code_kappa, an ind_kappa that names UU or a vector component - the
 * entropy plane is a copy of the variable as it lies, and the reader would hand over the converted one.
 * bl_harm_grid_desc(g, 0): the description for bl_set_grid_device_harm - prim NULL, n_var = n_prim, the header's indices; (g, 1): for
 * planes as bl_harm_convert_* write them - n_var 8 (9), indices 0 ... 7 (8) - which is what bl_set_grid / bl_set_grid_device take
 * with those planes. Both are owned by the grid. The 2048 x 2048 look-up table of simulation_coord = fmks is built when a
 * description is first asked for: a caller who only converts never pays for it. */
typedef struct bl_harm_grid bl_harm_grid;
BL_API int bl_harm_grid_create(const bl_params *p, const bl_harm_header *header, bl_harm_grid **out, char *err, size_t err_len);
BL_API const bl_grid_desc *bl_harm_grid_desc(bl_harm_grid *g, int converted);
BL_API const char *bl_harm_grid_warnings(const bl_harm_grid *g);
BL_API int bl_harm_grid_planes(const bl_harm_grid *g);   /* 8, or 9 with plasma_model = code_kappa (the entropy plane last) */
BL_API void bl_harm_grid_free(bl_harm_grid *g);
/* prims: float32 [n1][n2][n3][n_prim] -> out: float32 [planes][n3][n2][n1] in the order rho, pgas, uu1, uu2, uu3, bb1, bb2, bb3
 * (, kappa): p = (gamma - 1) u in float, the vectors converted in double and rounded, everything else copied. */
BL_API int bl_harm_convert_host(const bl_harm_grid *g, const float *prims, float *out);
/* The reader stopped before its transpose (simulation_format = iharm3d only): every check of bl_snapshot_open_number made, the header
 * as a struct, the file's prims as they lie - float32 [n1][n2][n3][n_prim], owned by the snapshot - and no look-up table built.
 * file_number = -1: simulation_file as it stands. bl_snapshot_grid()->prim is NULL for such a snapshot. */
BL_API int bl_snapshot_open_raw(const bl_params *p, int file_number, bl_snapshot **out, char *err, size_t err_len);
BL_API int bl_snapshot_harm_header(const bl_snapshot *s, bl_harm_header *out);   /* BL_E_STATE: not opened raw */
BL_API const float *bl_snapshot_harm_prims(const bl_snapshot *s);                /* NULL: not opened raw       */

/* ------------------------------------------------------------------ camera frame
 * The seven 4-vectors GeodesicIntegrator::InitializeCamera() derives (camera.cpp:61-380,
 * geodesic_integrator.hpp) and the frequency list (:30-50). Filled by bl_init. */
typedef struct bl_camera_frame {
  double cam_x[4], u_con[4], u_cov[4], norm_con[4], norm_con_c[4], hor_con_c[4], vert_con_c[4];
  double bh_m, bh_a, r_horizon, r_terminate, mass_msun;
} bl_camera_frame;

/* ------------------------------------------------------------------ one render call
 * Replaces, for one adaptive level, InitializeCamera/AugmentCamera + IntegrateGeodesics* +
 * ReverseGeodesics + CalculateSimulationSampling + SampleSimulation + Calculate*Coefficients +
 * IntegrateUnpolarizedRadiation / IntegratePolarizedRadiation (image rows 4 l + (I, Q, U, V) with
 * image_polarization). The refinement decision between levels
 * (radiation_adaptive.cpp) stays with the caller, as in blacklight.cpp:196-233. */
typedef struct bl_render_desc {
  int32_t level;              /* 0 = root camera; L>0 = refined blocks at res * 2^L              */
  int32_t n_blocks;           /* level>0: number of blocks                                        */
  const int32_t *block_locs;  /* level>0: host [n_blocks][2] = (block_v, block_u), camera.cpp:457  */
  int64_t n_rays;             /* rays to trace in this call                                       */
  const int32_t *pixel_map;   /* optional host [n_rays]: ray r is pixel pixel_map[r] of the level's
                                 pixel array (multi-GPU tiling); NULL = pixels 0..n_rays-1        */
  int32_t outputs_on_device;  /* 0: pointers below are host memory; 1: device memory (HBM)        */
  double *image;              /* [n_q][n_rays] f64, row order = reference image offsets            */
  int32_t *sample_num;        /* [n_rays] or NULL                                                  */
  uint8_t *sample_flags;      /* [n_rays] or NULL                                                  */
  double *camera_pos;         /* [n_rays][4] or NULL                                               */
  double *camera_dir;         /* [n_rays][4] or NULL                                               */
  double *render;             /* render_num_images > 0: [render_num_images][3][n_rays] XYZ, else NULL
                                 (RadiationIntegrator::Render, rendering.cpp:25-179)                  */
} bl_render_desc;

typedef struct bl_stats {
  int64_t n_rays;             /* rays traced by the last bl_render                                 */
  int64_t n_samples;          /* kept samples (sum of sample_num)                                  */
  int64_t n_samples_emitted;  /* sample records the geodesic kernel wrote (before truncation; a paired render's count twice: the
                                 whole frame's). The records themselves, the same from launch to launch - not the record slots its
                                 waves took, which count every wave's partly filled last block of 1 024 as well and which this
                                 field reported before mirror pairs (up to a block per wave more; still so where the records come
                                 from a geodesic checkpoint). A scratch limit sized from it wants that margin on top.             */
  int64_t n_gathers;          /* S_in: samples that read the grid (8 var x 8 corners, or x1)        */
  int64_t n_flagged;          /* rays with sample_flags set                                        */
  int32_t max_sample_num;     /* geodesic_num_steps                                                */
  int32_t n_chunks;
  double algorithmic_bytes;   /* 256 (or 32) * n_gathers + 13 * n_rays                */
  float ms_geodesic, ms_shade, ms_transfer, ms_total; /* HIP-event kernel time, last bl_render: geodesic,
                                 coefficient (bl_shade_kernel) and transfer kernels; ms_total = sum of all four    */
  int32_t launches_geodesic, launches_shade, launches_transfer;
  float ms_locate;            /* locate kernel (simulation mode)                                      */
  float ms_wall;              /* first kernel start to last kernel end; less than ms_total when the geodesic
                                 kernel of one chunk overlaps the shading of the previous one          */
  int32_t launches_locate;
  int32_t arithmetic;         /* BL_ARITH_EXACT or BL_ARITH_TOLERANT: the tier the last bl_render ran in          */
  int32_t mirror_pairs;       /* 1: only the left half of the frame was traced and every sample record shaded for its pixel and for the
                                 mirror pixel (zero spin, camera in the mirror plane; BL_SWITCH_NO_MIRROR_PAIRS: 0). In the four bytes
                                 that were padding in front of n_deferred: no other member moves, n_cameras stays the last one.       */
  int64_t n_deferred;         /* tolerant tier: samples whose cut decision was left to the exact kernel           */
  int64_t n_undefined;        /* BL_UNDEFINED_EDGE: samples where the reference reads past its arrays (edge cell used)     */
  uint32_t switches;          /* BL_SWITCH_* bits active in this context (measurement switches, below); 0 in production  */
  int32_t fused_variant;      /* the locate step inside the coefficient kernel: 2 = bl_shade_fused2_kernel (tolerant tier),
                                 3 = bl_shade_exact2_kernel (exact tier), 4 = bl_shade_polarized2_kernel (polarized runs),
                                 0 = a locate kernel of its own ran  */
  int64_t n_parked;           /* rays whose last steps ran with a ray per quad of lanes (bl_geodesic_quad_kernel)                 */
  int32_t composed_maps;      /* 1: the tolerant tier composed the affine transfer maps of neighbouring samples (intensities equal from
                                 run to run to rounding, ~1e-15, not bit for bit); 0: every image row of this render is bit-reproducible
                                 (always so in the exact tier and under bl_set_reproducible)                                         */
  int32_t tail_policy;        /* BL_TAIL_* the render ran with (after BL_TAIL_AUTO was resolved)                                     */
  int32_t geodesics_reused;   /* 1: the sample records of an earlier render of the same camera were shaded again - no ray was
                                 integrated (launches_geodesic = 0, ms_geodesic = 0); bl_set_geodesic_reuse                              */
  int32_t sampling_reused;    /* 1: ... and the located samples too (same grid geometry: no locate kernel ran, launches_locate = 0)     */
  int32_t xcd_order;          /* 1: the rays were traced and their records shaded in the trace order per XCD (BL_SWITCH_FLAT_ORDER: 0) */
  int32_t local_angles;       /* 1: bl_shade_fused2_kernel took theta and phi relative to the centre of the guessed cell; 0: acos / atan2
                                 (angular cells beyond the series' reach, a mesh with refinement, BL_SWITCH_GLOBAL_ANGLES, another kernel) */
  int32_t n_cameras;          /* cameras the last bl_render traced as one set of rays (bl_set_cameras): max(1, n) */
  /* Several electron models (bl_set_electron_models) where they cannot share one pass: launches_shade / launches_transfer count one
     shading pass per model and chunk; n_gathers, n_deferred and the sample counts are those of one pass (every pass has the same
     samples); ms_shade runs from the first coefficient kernel to the last one, ms_transfer is the last transfer kernel's. */
  /* ... and density units (bl_set_density_units) likewise: one shading pass per (model, unit) and chunk, n_chunks * M * U launches;
     where every variant shares one pass, n_chunks. */
  /* ... and sigma cuts (bl_set_sigma_cuts): one shading pass per (model, unit, cut) and chunk, n_chunks * M * U * S launches; where
     every variant shares one pass, n_chunks whatever S is. */
  int32_t n_mixes;            /* electron mixes the last bl_render rendered (bl_set_electron_mixes): max(1, n); one shading pass per
                                 (mix, model, unit, cut) and chunk, or where every variant shares one pass n_chunks whatever E is */
} bl_stats;

/* Measurement switches: environment variables BLACKLIGHT_AMD_<NAME>, read ONCE by bl_init (never during a render) and echoed in
 * bl_stats.switches, so that a benchmark line says which kernels it timed. They select an alternative kernel or layout with the
 * same results (A/B runs, tests of the general paths); none of them changes an image. */
#define BL_SWITCH_TENSOR_TRANSPORT (1u << 0)                /* polarized, tolerant tier: the exact tier's tensor transport      */
#define BL_SWITCH_SPLIT_RECORDS (1u << 1)                   /* sample records as two arrays of 32-byte halves                   */
#define BL_SWITCH_RECORD_EVERY_STEP (1u << 2)               /* steps in the empty shell around the grid leave records too       */
#define BL_SWITCH_GENERAL_LOCATE (1u << 4)                  /* bl_locate_kernel where bl_locate_plain_kernel applies; a refined
                                                               mesh's tables searched in HBM where they would be staged in LDS */
#define BL_SWITCH_LANE_TRANSFER (1u << 5)                   /* one lane per ray where bl_transfer_quad_kernel applies           */
#define BL_SWITCH_NO_FUSED_LOCATE (1u << 6)                 /* a locate kernel + bl_shade_fast_kernel / bl_shade_exact_kernel   */
#define BL_SWITCH_SAMPLE_RECORDS (1u << 8)                  /* tolerant tier: one transfer record per sample where composed maps apply */
#define BL_SWITCH_QUAD_EVERY_RAY (1u << 11)                 /* every ray parked before its first step: all stepping in bl_geodesic_quad_kernel */
#define BL_SWITCH_FLAT_ORDER (1u << 12)                     /* one ray queue, tile by tile, and the records in one grid-stride walk
                                                               where the trace order per XCD applies (bl_stats.xcd_order)           */
#define BL_SWITCH_GLOBAL_ANGLES (1u << 13)                  /* tolerant coefficient kernel: theta and phi by acos / atan2 where the
                                                               angles relative to the cell centre apply (bl_stats.local_angles)     */
#define BL_SWITCH_GENERAL_CUTS (1u << 14)                   /* tolerant coefficient kernel: the general block of cell cuts where
                                                               cut_sigma_max is the only active threshold (its short form)         */
#define BL_SWITCH_NO_MIRROR_PAIRS (1u << 15)                /* every ray of the frame traced where one ray per mirror pair applies
                                                               (bl_stats.mirror_pairs)                                              */
#define BL_SWITCH_EXACT_DISTANCE (1u << 16)                 /* Dormand-Prince stepper: the reference's proper-distance operations in
                                                               every stage where the closed form applies (`stepper:` debug line)    */
#define BL_SWITCH_WIDE_DISTANCE_BAND (1u << 17)             /* ... the closed form with a band of 0.25 in the sample count: nearly
                                                               every ray has an undecided step, so the frame is rendered a second
                                                               time with the reference's operations (exercises that path)           */
/* (Fourteen switches. Rounds 3 - 5 had eight more for experiments the measurements buried - a second pre-fused2 kernel, pre-gathered
 * cell bricks, the coefficient kernel beside a chunk's last rays, repacked tails - and for what bl_set_tail_policy now says; their
 * numbers are in docs/notebook.md, their code in the history.) */

typedef struct bl_ctx bl_ctx;

/* Validate parameters exactly like the two reference constructors, compute the camera frame and
 * frequency list on the host, select the device (device = -1: current device) and allocate
 * nothing large yet. device = BL_DEVICE_NONE gives a host-only context (parameter validation, camera
 * frame, bl_adaptive_refine, bl_write_output); bl_set_grid / bl_render on it fail with BL_E_DEVICE. */
#define BL_DEVICE_NONE (-2)
BL_API int bl_init(const bl_params *p, int device, bl_ctx **out);
/* HIP devices visible to this process (0: none). One context per device and one host thread per context is how one process
 * drives several GPUs: bl_render is thread-safe across contexts (bin/blacklight_amd with BLACKLIGHT_AMD_DEVICES does that). */
BL_API int bl_device_count(void);
/* The grid into its HBM layout; once per snapshot. Equal blocks of one level tiling a box are merged into one [k][j][i][8 floats]
 * array; other sets of non-overlapping equal-sized blocks (mesh refinement) stay [block][k][j][i][8] behind a lattice of block
 * boundaries. Overlapping blocks are refused. The variable planes are uploaded as they lie and interleaved on the device (a 256^3
 * snapshot: 33 ms, the PCIe copy of its 537 MB).
 * Beside a render: when the geometry handed over is, to the bit, the one in place (the next snapshot of a series) bl_set_grid may be
 * called on another host thread while bl_render of the same context runs: the cells go up on a stream of their own into a second
 * cell array, and the call returns once that render has ended and the arrays have changed places - the new cells are what the NEXT
 * bl_render reads. One bl_set_grid at a time per context; any other change of the grid waits for the render and excludes it. */
BL_API int bl_set_grid(bl_ctx *ctx, const bl_grid_desc *g);
/* The same call for cells that already lie in device memory (a GRMHD code in the same process, a torch pipeline, a series kept
 * resident): the staging kernel reads the caller's array where it lies - no copy through the host, none into a plane buffer.
 * `g` is what bl_set_grid takes with g->prim ignored (NULL is fine); the coordinate arrays, the MeshBlock table and sks_map stay host
 * pointers. The cells of one (variable, block) are contiguous [n_k][n_j][n_i]; variable v of block b starts at
 * prim + v * var_stride + b * block_stride (elements):
 *   [var][block][k][j][i] (the reference's)      var_stride = n_blocks * block_cells, block_stride = block_cells
 *   [block][var][k][j][i] (AthenaK-style codes)  var_stride = block_cells,            block_stride = n_var * block_cells
 * BL_CELLS_F64 cells are rounded to the nearest float (ties to even) on the device - what writing them to a float32 file and reading
 * it back does - so everything downstream sees the bytes of bl_set_grid with the array converted to float32.
 * Ordering: with wait != 0 the staging waits, on the device, for the work queued so far on `stream` (an event, no host wait); with
 * wait == 0 the caller has synchronised. The call returns once the cells are in place: the array may be overwritten then. Beside a
 * render, slow-light slices, refusals: as bl_set_grid / bl_set_grid_slice.
 * Checked before anything is launched (BL_E_ARG, a text each): cells / prim NULL, prim not aligned to its element, dtype, a stride
 * below 1, n_elements below what the strides reach (the eight variables read, ind_kappa with plasma_model = code_kappa); then, on the
 * device, that prim is device memory of the context's device and that n_elements elements from it lie within one allocation. Host
 * arrays, pinned or not, go through bl_set_grid. */
#define BL_CELLS_F32 0
#define BL_CELLS_F64 1
typedef struct bl_device_cells {
  const void *prim;       /* device memory of the context's device                                          */
  int32_t dtype;          /* BL_CELLS_F32 | BL_CELLS_F64                                                     */
  int32_t wait;           /* != 0: the staging first waits, on the device, for the work queued on `stream`  */
  int64_t var_stride;     /* elements between variable v and v + 1 of one block                              */
  int64_t block_stride;   /* elements between block b and b + 1 of one variable                              */
  int64_t n_elements;     /* extent of the caller's array from `prim`, in elements                           */
  void *stream;           /* hipStream_t (NULL: the NULL stream); read only with wait != 0                   */
} bl_device_cells;
BL_API int bl_set_grid_device(bl_ctx *ctx, const bl_grid_desc *g, const bl_device_cells *cells);
BL_API size_t bl_device_cells_sizeof(void);
/* Bytes the last bl_set_grid* call of this context copied from host memory: variable planes, tables, block origins. After a
 * device call: the tables only. */
BL_API int64_t bl_grid_host_bytes(const bl_ctx *ctx);
/* The HIP device of the context (what bl_init selected; BL_DEVICE_NONE for a host-only context): where bl_device_cells::prim must lie. */
BL_API int bl_context_device(const bl_ctx *ctx);
/* ---- slow light (slow_light_on = true): the reader keeps a window of slow_chunk_size files, latest first
 * (simulation_reader.cpp:211-303), all on the geometry of the first; every sample reads the slice(s) around
 * its own coordinate time (simulation_sampling.cpp:296-349, :736-786, :840-912).
 * bl_slow_light_read(ctx, snapshot): SimulationReader::Read(snapshot) for slow light - advances the window to
 *   cover camera time slow_t_start + snapshot * slow_dt, reading only new files (bl_snapshot_open_number),
 *   shifting the slices already in HBM, and selects `snapshot` for the next bl_render. Reference error and
 *   warning texts ("... would require significant extrapolation beyond file N.").
 * The three calls below are what it is made of, for callers with their own reader:
 * bl_set_grid_slice(ctx, n, g, time): slice n of the window (prim[n], time[n]).
 * bl_shift_grid_slices(ctx, count): slice n <- slice n - count for n >= count (device pointers move, no copy).
 * bl_set_snapshot(ctx, snapshot): image index; camera time and the texts of bl_render's extrapolation
 *   warnings / errors (simulation_sampling.cpp:577-617) follow from it. */
BL_API int bl_slow_light_read(bl_ctx *ctx, int snapshot);
BL_API int bl_set_grid_slice(bl_ctx *ctx, int slice, const bl_grid_desc *g, double time);
BL_API int bl_set_grid_slice_device(bl_ctx *ctx, int slice, const bl_grid_desc *g, const bl_device_cells *cells, double time);   /* (cells in device memory: bl_set_grid_device) */
BL_API int bl_shift_grid_slices(bl_ctx *ctx, int count);
BL_API int bl_set_snapshot(bl_ctx *ctx, int snapshot);
/* ---- iharm3d-family primitives in device memory: bl_set_grid_device / bl_set_grid_slice_device for the array a harm-family code
 * holds, prims[n1][n2][n3][n_prim] contiguous, float or double. The staging kernel transposes it and converts every cell as the
 * reader converts a file's (bl_harm_grid, above): F64 cells are rounded to float first, p = (gamma - 1) u in float, the vectors in
 * double from the grid's point table (uploaded once per grid and context), the result rounded to float - the cells in HBM are, bit
 * for bit, those of bl_set_grid with the snapshot the reader makes of the same data. prim, dtype, wait, stream and n_elements mean
 * what they mean in bl_device_cells, and the same is checked (BL_E_ARG, a text each): prim NULL or not aligned to its element, dtype,
 * n_elements below n1 n2 n3 n_prim, then on the device that prim is device memory of the context's device with n_elements elements
 * inside one allocation. Beside a render, the series' fast path, slow-light slices, bl_grid_host_bytes (tables only): as
 * bl_set_grid_device.
 * The grid and the context: spin, adiabatic indices and the choice of variables are the grid's, fixed by the parameters it was made
 * with - make it with the context's. A grid made with another plasma_model than the context's, where one of the two is code_kappa,
 * is refused (BL_E_ARG): the entropy plane would be missing or come from a variable nobody named.
 * Threads: these three calls are bl_set_grid calls - one at a time per context, bl_harm_convert_device included (the context keeps
 * one copy of a grid's point table on the device, replaced when another grid comes; a render of the same context may run beside
 * the setters as beside bl_set_grid, and bl_harm_convert_device waits for it).
 * bl_harm_convert_device writes the planes of bl_harm_convert_host - float32 [planes][n3][n2][n1], planes = bl_harm_grid_planes() -
 * into out_planes, caller-owned device memory of the context's device holding at least that many floats: with
 * bl_harm_grid_desc(g, 1) they are what bl_set_grid_device takes. Any n1, n2, n3 >= 1. Returns when the planes are written. */
typedef struct bl_harm_cells {
  const void *prim;       /* device memory of the context's device: [n1][n2][n3][n_prim], contiguous         */
  int32_t dtype;          /* BL_CELLS_F32 | BL_CELLS_F64                                                     */
  int32_t wait;           /* != 0: the staging first waits, on the device, for the work queued on `stream`  */
  int64_t n_elements;     /* extent of the caller's array from `prim`, in elements                           */
  void *stream;           /* hipStream_t (NULL: the NULL stream); read only with wait != 0                   */
} bl_harm_cells;
BL_API size_t bl_harm_cells_sizeof(void);
BL_API int bl_set_grid_device_harm(bl_ctx *ctx, bl_harm_grid *grid, const bl_harm_cells *cells);
BL_API int bl_set_grid_slice_device_harm(bl_ctx *ctx, int slice, bl_harm_grid *grid, const bl_harm_cells *cells, double time);
BL_API int bl_harm_convert_device(bl_ctx *ctx, const bl_harm_grid *grid, const bl_harm_cells *cells, float *out_planes);
/* Number of image rows n_q and their offsets (radiation_integrator.cpp:436-520). */
BL_API int bl_image_num_quantities(const bl_ctx *ctx);
/* Electron-temperature models (the R_high / R_low prescription: plasma_rat_high, plasma_rat_low) rendered by one bl_render.
 * n = 0 (what a context starts with): the parameter block's own pair. 1 <= n <= BL_MAX_ELECTRON_MODELS: n (R_low, R_high) pairs,
 * finite; bl_image_num_quantities is then n times the single-model count and image row m * n_q + q is row q of model m
 * (sample_num, sample_flags and renderings come out once). Geodesics and located samples do not depend on the model: changing the
 * models between renders keeps them (bl_set_geodesic_reuse). Refused (BL_E_UNSUPPORTED): formula mode, polarized runs,
 * plasma_model = code_kappa, slow light, and with n >= 2 adaptive_max_level > 0 and renderings that a model enters (a Theta_e
 * feature, or a Theta_e cut beside renderings) - as are bl_adaptive_refine and bl_write_output while n >= 2 (refinement reads one
 * image; the reference's files have no model axis). The tolerant tier's plain intensity images without a Theta_e cut render n >= 2
 * models in one pass: one gather and coefficient kernel, one transfer lane per (ray, model, frequency) - each model within the tier's
 * tolerance of its exact image. Everything else runs one shading pass per model over the shared samples: each model's image is what
 * a render with that pair in the parameter block gives (the same bits in the exact tier and under bl_set_reproducible). */
#define BL_MAX_ELECTRON_MODELS 16
BL_API int bl_set_electron_models(bl_ctx *ctx, int n, const double *rat_low, const double *rat_high);
BL_API int bl_num_electron_models(const bl_ctx *ctx);   /* 0 = unset: the parameter block's own model */
/* Density units (simulation_rho_cgs, the code density in g / cm^3; simulation_coefficients.cpp:237-239) rendered by one bl_render -
 * the normalisation a flux fit tunes. n = 0 (what a context starts with): the parameter block's own unit. 1 <= n <=
 * BL_MAX_DENSITY_UNITS: n absolute values of simulation_rho_cgs, each finite and > 0. With M = max(1, electron models) and
 * U = max(1, n), bl_image_num_quantities is M * U times the single-render count and image row (m * U + u) * n_q + q is row q of
 * model m at unit u (model-major; sample_num, sample_flags and renderings come out once). Geodesics and located samples do not
 * depend on the unit: changing the units between renders keeps them. Refused (BL_E_UNSUPPORTED): formula mode, polarized runs,
 * slow light, and with n >= 2 adaptive_max_level > 0 and renderings that a unit enters (a rho, n_e, p_gas or B feature, or a cut
 * on rho, n_e, p_gas or B beside renderings) - as are bl_adaptive_refine and bl_write_output while n >= 2. n = 1 renders that
 * value instead of the parameter block's. The tolerant tier's plain intensity images without a Theta_e cut - and, with n >= 2,
 * without a cut on rho, n_e, p_gas or B - render every (model, unit) in one pass: one gather and coefficient kernel, one transfer
 * lane per (ray, model, unit, frequency), each within the tier's tolerance of its exact image. Everything else runs one shading pass per (model, unit) over the shared samples: each variant's
 * image is what a render with that unit (and pair) in the parameter block gives (the same bits in the exact tier and under
 * bl_set_reproducible). */
#define BL_MAX_DENSITY_UNITS 16
BL_API int bl_set_density_units(bl_ctx *ctx, int n, const double *rho_cgs);
BL_API int bl_num_density_units(const bl_ctx *ctx);   /* 0 = unset: the parameter block's own unit; -1: no context */
/* Polarized variants: (R_low, R_high, simulation_rho_cgs) triples rendered by one bl_render of a polarized run - the door the two calls
 * above keep shut (they refuse image_polarization = true). A list of triples, not a product: after a flux fit every pair has a unit
 * of its own. n = 0 (what a context starts with): the parameter block's own pair and unit. 1 <= n <= BL_MAX_POLARIZED_VARIANTS:
 * bl_image_num_quantities is n times the single-render count and image row v * n_q + q is row q (rows 4 l + (I, Q, U, V), ...) of
 * variant v; sample_num, sample_flags and the camera outputs come out once. BL_E_ARG: n out of range, a null array with n > 0, a
 * non-finite R_low or R_high, a unit that is not finite and > 0. Refused (BL_E_UNSUPPORTED): a context that is not polarized (use
 * bl_set_electron_models / bl_set_density_units there), formula mode, slow light, and with n >= 2 adaptive_max_level > 0 and
 * render_num_images > 0 - as are bl_adaptive_refine and bl_write_output while n >= 2. A refused call changes nothing. With
 * plasma_model = code_kappa the pairs are unused, the units are not. Geodesics and located samples do not depend on the variants:
 * changing them between renders keeps what is resident (bl_stats.geodesics_reused).
 * Every variant's rows are the bits of a render with that triple in the parameter block, in the exact tier and - under
 * bl_set_reproducible, and wherever the polarized tolerant path repeats itself - in the tolerant one. n = 1 plans as that render does.
 * n >= 2 renders in ONE PASS where no decision differs between variants - Stokes rows and the optical-depth row only (no other
 * auxiliary row), Theta_e from R_high / R_low, a cut on rho, n_e, p_gas or B only if all units are equal, a Theta_e cut only if all triples are
 * equal: the gather, fluid frame and tetrad once per chunk (bl_stats.launches_shade = n_chunks), the transport matrices once, a
 * coefficient-kernel wave per (64 samples, variant) and a transfer lane per (ray, variant). Everything else: one shading pass per
 * variant over the shared samples (launches_shade = n_chunks * n).
 * bl_set_polarized_variants is bl_set_polarized_variants_sigma (below) with sigma_max = NULL: every variant is rendered under the
 * parameter block's own cut_sigma_max, and the cuts an earlier call of that function set are gone - as are, after either call, the
 * electron mixes an earlier bl_set_polarized_variants_electrons set. */
#define BL_MAX_POLARIZED_VARIANTS 16
BL_API int bl_set_polarized_variants(bl_ctx *ctx, int n, const double *rat_low, const double *rat_high, const double *rho_cgs);
/* ... with a sigma cut each: (R_low, R_high, simulation_rho_cgs, cut_sigma_max) quadruples, a list like the triples and not a
 * product. sigma_max[v] has the reference's meaning - a value >= 0 cuts cells with sigma = b.b / rho > value, a negative value
 * switches the cut off - and must be finite (BL_E_ARG, with the variant's index in the text; the call changes nothing).
 * sigma_max = NULL is exactly bl_set_polarized_variants. Everything else - the range of n, the other arrays, the refusals, image
 * rows, bl_num_variants, bl_num_polarized_variants, the .vNN tags of bl_write_output_variant - is as for the triples: a cut adds no
 * rows, it changes what variant v is. Every variant's rows are still the bits of a render with that quadruple in the parameter
 * block. Where the triples render in one pass the quadruples do too, whatever their cuts: with cuts that differ the shared
 * frame-and-inputs kernel runs with the sigma upper cut off and bl_polarized_coefficients_kernel, which has the cell's rho and
 * b.b in the sample's row, leaves a (sample, variant) with sigma above the variant's threshold without coefficients. Where the
 * render takes one shading pass per variant, each pass compares its own variant's cut. The cuts are no part of what the resident
 * geodesics depend on. */
BL_API int bl_set_polarized_variants_sigma(bl_ctx *ctx, int n, const double *rat_low, const double *rat_high, const double *rho_cgs,
                                           const double *sigma_max);
BL_API int bl_num_polarized_variants(const bl_ctx *ctx);   /* 0 = unset: the parameter block's own pair and unit; -1: no context */
/* ... with an electron distribution each: (R_low, R_high, simulation_rho_cgs, cut_sigma_max, mix) tuples, a list and not a product.
 * A mix is the seven plasma_* values that say which share of the electrons is a power law and which a kappa distribution (the rest
 * is thermal: 1 - (power_frac + kappa_frac), formed as bl_init forms it). sigma_max = NULL: the parameter block's cut_sigma_max for
 * every variant; mix = NULL: the parameter block's own seven values for every variant - the call is then exactly
 * bl_set_polarized_variants or bl_set_polarized_variants_sigma. n = 0 clears; n = 1 plans as a fresh render with that tuple in the
 * parameter block. The range of n, the refusals, image rows (row v * n_q + q is row q of variant v), bl_num_variants and the .vNN
 * tags are those of the triples: a mix adds no rows, it changes what variant v is. Variant v's rows are the bits of a render with
 * its R_low, R_high, unit, cut and seven plasma_* values in the parameter block - in the exact tier, and in the tolerant one under
 * the conditions stated for the triples above; sample_num, sample_flags and the camera outputs come out once.
 * Checked per variant when the call is made: every value that is read must be finite (BL_E_ARG, the variant's number in the text);
 * with kappa_frac != 0 a kappa outside [3.5, 5] is refused (BL_E_ARG: "Polarized transport only supports kappa in [3.5, 5]."); the
 * reference's warnings - a fraction of power-law, kappa-distribution or thermal electrons outside [0, 1], and "Polarized transport
 * will interpolate formulas based on kappa." for a kappa that is none of 3.5, 4, 4.5, 5 - go to bl_warnings, each at most once per
 * call. With power_frac == 0 (kappa_frac == 0) that distribution's shape values - p, gamma_min, gamma_max (kappa, w) - are neither
 * read nor checked, and bl_polarized_variant_electrons returns them as given. No other range is checked: the reference checks none.
 * A refused or failed call changes nothing. A later bl_set_polarized_variants or bl_set_polarized_variants_sigma drops the mixes.
 * No decision of a render depends on a mix - sample counts, flags, cells and cuts do not - except that Theta_e exists only where
 * the thermal fraction is non-zero: where the triples render in one pass the tuples do too (bl_stats.launches_shade = n_chunks),
 * unless a Theta_e cut is set and the mixes differ (one shading pass per variant then, launches_shade = n_chunks * n); every wave
 * of bl_polarized_coefficients_kernel reads its variant's electron constants from a device table. The mixes are no part of what the
 * resident geodesics depend on: changing them between renders of a camera reuses the records. */
typedef struct bl_electron_mix {
  double power_frac, p, gamma_min, gamma_max;   /* plasma_power_frac, plasma_p, plasma_gamma_min, plasma_gamma_max */
  double kappa_frac, kappa, w;                  /* plasma_kappa_frac, plasma_kappa, plasma_w */
  double reserved;                              /* 0 */
} bl_electron_mix;
BL_API int bl_set_polarized_variants_electrons(bl_ctx *ctx, int n, const double *rat_low, const double *rat_high,
                                               const double *rho_cgs, const double *sigma_max, const bl_electron_mix *mix);
/* The mix variant `variant` renders with - the parameter block's own where none was set. BL_E_ARG: variant outside
 * [0, max(1, bl_num_polarized_variants)). */
BL_API int bl_polarized_variant_electrons(const bl_ctx *ctx, int variant, bl_electron_mix *out);
/* Sigma cuts (cut_sigma_max, the magnetisation above which a cell is left out: sigma = b.b / rho in code units,
 * simulation_coefficients.cpp:361-375) rendered by one bl_render - the standard way to take the jet funnel out of an image. n = 0
 * (what a context starts with): the parameter block's own cut_sigma_max. 1 <= n <= BL_MAX_SIGMA_CUTS: n values with the reference's
 * meaning - a value >= 0 cuts cells with sigma > value, a negative value switches the cut off - each finite (BL_E_ARG otherwise).
 * With M = max(1, electron models), U = max(1, density units) and S = max(1, n), bl_image_num_quantities is M * U * S times the
 * single-render count and image row ((m * U + u) * S + s) * n_q + q is row q of model m at unit u under cut s; sample_num and
 * sample_flags come out once. Geodesics and located samples do not depend on the cut: changing the cuts between renders keeps
 * them. n = 1 renders that value instead of the parameter block's and plans as a fresh render with it. Refused
 * (BL_E_UNSUPPORTED): formula mode, polarized runs (the polarized axis is not built yet), slow light, and with n >= 2
 * adaptive_max_level > 0 and render_num_images > 0 (a cut cell drops out of a rendering) - as are bl_adaptive_refine and
 * bl_write_output while n >= 2. A refused call changes nothing. Where the tolerant tier renders models and units in one pass it
 * renders the cuts there too: the coefficient kernels run with the sigma upper cut off and leave every sample's sigma in its row,
 * and a transfer lane per (ray, model, unit, cut, frequency) compares it with the lane's threshold (bl_stats.launches_shade =
 * n_chunks whatever S is) - each variant within the tier's tolerance of its exact image. Everything else runs one shading pass per
 * variant over the shared samples: each variant's rows are the bits of a render with that value in the parameter block, in the
 * exact tier and under bl_set_reproducible. A polarized run takes its cuts with its variants, one per variant:
 * bl_set_polarized_variants_sigma. */
#define BL_MAX_SIGMA_CUTS 16
BL_API int bl_set_sigma_cuts(bl_ctx *ctx, int n, const double *sigma_max);
BL_API int bl_num_sigma_cuts(const bl_ctx *ctx);   /* 0 = unset: the parameter block's own cut_sigma_max; -1: no context */
/* Electron mixes of an UNPOLARIZED run (plasma_power_frac, plasma_p, plasma_gamma_min, plasma_gamma_max: which share of the electrons
 * is a power law, the rest thermal) rendered by one bl_render - a fourth product axis, outermost. n = 0 (what a context starts with)
 * clears the list: the parameter block's own four values apply. 1 <= n <= BL_MAX_ELECTRON_MIXES: with E = max(1, n) and M, U, S as
 * above, bl_image_num_quantities is E * M * U * S times the single-render count and image row
 * (((e * M + m) * U + u) * S + s) * n_q + q is row q of a render with mix e's four plasma_* values, model m, unit u and cut s in its
 * parameter block; sample_num, sample_flags and the camera outputs come out once. Geodesics and located samples do not depend on the
 * mix: changing the list between renders of a series keeps the records. n = 1 plans as a context with that mix in its block. Cameras
 * multiply rays and compose unchanged.
 * Checked when the call is made (BL_E_ARG, the mix's index in the text): power_frac must be finite, and p, gamma_min and gamma_max
 * where power_frac != 0 - where it is zero they are not read, and bl_electron_mix_get returns them as given. The reference's warnings
 * "Fraction of power-law electrons outside [0, 1]." and "Fraction of thermal electrons outside [0, 1]." go to bl_warnings, each at
 * most once per call. Refused (BL_E_UNSUPPORTED): formula mode, polarized runs (bl_set_polarized_variants_electrons is their list),
 * slow light, any mix with kappa_frac != 0 (the reference's unpolarized kappa absorptivity is undefined), and with n >= 2
 * adaptive_max_level > 0 and render_num_images > 0 - as are bl_adaptive_refine, bl_write_output and the two checkpoint saves while
 * n >= 2. A refused call changes nothing. Works on a BL_DEVICE_NONE context.
 * Where the tolerant tier renders models, units and cuts in one pass it renders two mixes or more there too, provided every mix has a
 * thermal part: the coefficient kernels write the sample's mix-free row with a thermal fraction of 1 (the kernels of a thermal run,
 * the one with the locate step inside included: bl_stats.fused_variant stays 2), and bl_transfer_freq_kernel runs a workgroup per
 * (256 rays, mix, model, unit, cut, frequency) that scales the thermal line by its mix's thermal fraction and adds its mix's power-law
 * emissivity and absorptivity, formed from the same row (bl_stats.launches_shade = launches_transfer = n_chunks whatever E is) - each
 * variant within the tier's tolerance of its exact image. Everything else runs one shading pass per variant over the shared samples
 * (launches_shade = n_chunks * E * M * U * S): each variant's rows are the bits of a render with that mix in the parameter block, in
 * the exact tier. The kernels of the passes are chosen once per render: a power law in any mix selects the ones that know power
 * laws, and a thermal mix passes through them with zero fractions - in the exact tier the same bits. The tolerant tier has no kernel
 * for a mix without a thermal part (power_frac = 1: the exact tier's render it, as they render a context with that mix in its block)
 * and other kernels for thermal electrons alone than for a power law beside them; so a list that holds a mix without a thermal part
 * beside others is rendered there run by run, a pass per variant - the neighbouring mixes of one of these three kinds as one render
 * into their rows, each kind exactly as a context with such a mix in its block plans it (under bl_set_reproducible: that context's
 * bits), the later runs from the resident geodesics where the record layout is the same. bl_stats then holds the last run's values
 * with the launches and kernel times summed over the runs, arithmetic = BL_ARITH_TOLERANT if any run was tolerant, and n_mixes = E. */
#define BL_MAX_ELECTRON_MIXES 16
BL_API int bl_set_electron_mixes(bl_ctx *ctx, int n, const bl_electron_mix *mix);
BL_API int bl_num_electron_mixes(const bl_ctx *ctx);             /* 0 = unset; -1: no context */
/* Mix e of the list, 0 <= e < max(1, n); with no list, mix 0 is the parameter block's own. */
BL_API int bl_electron_mix_get(const bl_ctx *ctx, int e, bl_electron_mix *out);
/* Cameras (viewing angles: camera_th, camera_ph) rendered by one bl_render - the third axis of a model library beside snapshots and
 * plasma variants. n = 0 (what a context starts with): the parameter block's own camera. 1 <= n <= BL_MAX_CAMERAS: n (th, ph) pairs in
 * DEGREES, as camera_th and camera_ph are written in the .input file, converted exactly as those two keys are (val * pi / 180;
 * camera_pole for a written th of exactly 0 or 180). Camera c's frame is the frame bl_init builds from the context's parameters with
 * those three fields replaced (bl_camera_frame_get_camera). bl_init refuses no value of camera_th or camera_ph, so neither does this call.
 * With C = max(1, n) a full root-level render has n_rays = C * res^2: ray, output index and "virtual pixel" v = c * res^2 + m are one
 * number, m the reference's pixel index within camera c. Every per-ray output is indexed by v - image[row][v], sample_num, sample_flags,
 * camera_pos / camera_dir, renderings, on the host or the device. bl_image_num_quantities does not change: cameras multiply rays, not
 * rows (rows stay variant-major under every variant setter). pixel_map entries are virtual pixels (BL_E_ARG outside 0 .. C * res^2 - 1,
 * checked while a camera list is set), and n_rays is checked against C * res^2. n = 1 renders that camera and plans exactly as a
 * context whose block holds those angles (bl_camera_frame_get then returns that camera's frame).
 * In the exact tier and under bl_set_reproducible the slice [:, c res^2 : (c + 1) res^2] of every output is bit for bit what a context
 * renders that bl_init made with camera c's angles in its block, whatever the chunking; with composed maps every integer output and
 * NaN mask is that render's and every finite pixel lies within the tier's per-pixel bound of it. The cameras are ONE set of rays:
 * bl_stats.launches_geodesic = n_chunks whatever C is, the rays are traced 8 x 8 tile by tile with the cameras interleaved (tile t of
 * every camera, then the next tile, each camera's tiles centre first). With n >= 2 the trace order per XCD stays off
 * (bl_stats.xcd_order = 0) and BL_TAIL_SPLIT resolves to BL_TAIL_WIDE (bl_stats.tail_policy) - both change speed only. The reference's
 * warning about geodesics that terminate unexpectedly is raised once per render and carries the totals over all cameras ("k out of
 * M", M = C * res^2). The camera list is part of what "the same camera" means for bl_set_geodesic_reuse: another list integrates
 * again, the same list after bl_set_grid shades the resident records (bl_stats.geodesics_reused = 1).
 * BL_E_ARG: a non-finite angle (with the camera's index), n outside 0 .. BL_MAX_CAMERAS, a null array with n > 0. Refused
 * (BL_E_UNSUPPORTED): with n >= 1 checkpoint_geodesic_load (the file carries its own camera); with n >= 2 adaptive_max_level > 0,
 * slow light, checkpoint_geodesic_save, checkpoint_sample_save, and the three settings whose kernels read the one camera position of
 * their argument block: cut_omit_near, cut_omit_far and image_crossings - as are bl_adaptive_refine, bl_write_output and
 * bl_write_output_variant while n >= 2 (the reference's file holds one camera). A refused call changes nothing. Works on a
 * BL_DEVICE_NONE context. */
#define BL_MAX_CAMERAS 16
BL_API int bl_set_cameras(bl_ctx *ctx, int n, const double *th_deg, const double *ph_deg);
BL_API int bl_num_cameras(const bl_ctx *ctx);   /* 0 = unset: the parameter block's own camera; -1: no context */
/* The frame of camera `camera` of the list (0 .. max(1, n) - 1; with no list, camera 0 is the parameter block's). */
BL_API int bl_camera_frame_get_camera(const bl_ctx *ctx, int camera, bl_camera_frame *out);
/* The sweep of a .input file onto a context, as one checked step - one rule for the command-line driver, a bound reference main()
 * and Python. Every list of `lists` (a NULL member: none) is resolved against the context's parameters (bl_sweep_cameras_resolve,
 * bl_sweep_resolve or, with an electron list, bl_sweep_electrons_resolve), then checked with the checks of the setter it belongs to -
 * bl_set_cameras, then bl_set_polarized_variants (polarized) or bl_set_electron_models and bl_set_density_units, then
 * bl_set_sigma_cuts; with an electron list the tuples are resolved first of all, and the cuts are checked before
 * bl_set_polarized_variants_electrons, which takes the tuples under the parameter block's cut_sigma_max. The first failure is the
 * call's: a list error (BL_E_INPUT, the resolver's text) or a setter's refusal in its words. All or nothing: only when every check
 * has passed are the lists stored, all under one hold of the lock bl_render holds, so a render on another thread sees the context
 * before the call or after it; a refused call leaves the context exactly as it was. A list the call does not carry leaves its axis
 * as it is, and an empty sweep changes nothing. */
BL_API int bl_apply_sweep_lists(bl_ctx *ctx, const bl_sweep_lists *lists);
/* ... with the frequency list (sweep_frequency) as a fifth: checked last, with bl_set_frequencies' checks, and stored under the same
 * hold of the lock as the others - the same rule, all or nothing. Two frequencies or more on a block with adaptive_max_level > 0 are
 * refused here (BL_E_UNSUPPORTED), as the other sweeps are on such blocks: the files of a sweep are one-frequency files, and a
 * one-frequency run refines by its own image. bl_apply_sweep_lists forwards to this call with `frequencies` NULL. */
BL_API int bl_apply_sweep_all(bl_ctx *ctx, const bl_sweep_all *lists);
/* Forwards to bl_apply_sweep_lists with the lists they name (cuts, cameras may be NULL), kept for their callers: BL_E_ARG without a
 * context or a sweep. */
BL_API int bl_apply_sweep(bl_ctx *ctx, const bl_sweep *sweep);
BL_API int bl_apply_sweeps(bl_ctx *ctx, const bl_sweep *sweep, const bl_sweep_cuts *cuts);
BL_API int bl_apply_sweeps_cameras(bl_ctx *ctx, const bl_sweep *sweep, const bl_sweep_cuts *cuts, const bl_sweep_cameras *cameras);
/* The angles of the camera list as given, in degrees (an angle taken from the parameter block: its radians x 180 / pi): the first
 * min(n, bl_num_cameras) entries of both arrays. */
BL_API int bl_cameras_get(const bl_ctx *ctx, int n, double *th_deg, double *ph_deg);
/* Images one bl_render produces: max(1, electron models) * max(1, density units) * max(1, sigma cuts) * max(1, polarized variants)
 * - a polarized variant's own sigma cut (bl_set_polarized_variants_sigma) is part of the variant and adds no image; -1: no context. */
BL_API int bl_num_variants(const bl_ctx *ctx);
/* What every image of a render is rendered with: the first min(n, bl_num_variants) rows, in image-row order - the triples, else
 * models x units x sigma cuts, model-major, then unit, then cut, with the parameter block's value where an axis is not set (the counts:
 * bl_num_electron_models, ...). *flags: whether the triples carry cuts and mixes of their own (bl_polarized_variant_electrons reads
 * the mixes). Any output may be NULL. */
#define BL_VARIANTS_TRIPLES_CUT 1
#define BL_VARIANTS_TRIPLES_MIX 2
BL_API int bl_variants_get(const bl_ctx *ctx, int n, double *rat_low, double *rat_high, double *rho_cgs, double *sigma_max, int *flags);
/* Number of false-colour renderings bl_render produces (render_num_images; 0 in formula mode). */
BL_API int bl_render_num_images(const bl_ctx *ctx);
BL_API int bl_camera_frame_get(const bl_ctx *ctx, bl_camera_frame *out);
BL_API int bl_frequencies(const bl_ctx *ctx, double *out, int n);
/* An explicit list of observing frequencies rendered by one bl_render - the frequency axis of a model library: 86, 230 and 345 GHz
 * over one set of geodesics, which no spacing of image_frequency_start .. image_frequency_end gives. n = 0 (what a context starts
 * with): the parameter block's own list, rebuilt exactly as bl_init built it. 1 <= n <= BL_MAX_FREQUENCIES: hz[0 .. n), each with the
 * meaning of image_frequency - it goes through the same image_normalization and nothing else; the values need not be ordered or
 * distinct. From then on n is the context's frequency count everywhere: bl_frequencies, bl_image_num_quantities and the auxiliary
 * rows' offsets (those of a block with image_num_frequencies = n: within a variant, frequency l of a quantity sits where it sits
 * there), the render's plan, the .npz / .npy / raw writer (bl_write_output writes one file with the reference's frequency axis of
 * length n) and a geodesic checkpoint that is saved. For bl_adaptive_refine adaptive_frequency_num - 1 indexes the list (n = 1: 0).
 * Row l of a list render is the row of a context with that one frequency in its block: bit for bit in the exact tier, within the
 * tier's per-pixel bound in the tolerant one. Formula mode, slow light, polarized runs, every variant setter and the camera list
 * compose with the list unchanged. The values are no part of what "the same camera" means for bl_set_geodesic_reuse: a render after
 * other values of the same length shades the resident records (bl_stats.geodesics_reused = 1), and another length does wherever the
 * plan chooses the same record layout (four frequencies or more leave the kernels as per-sample factors: another layout).
 * BL_E_ARG: a value that is not finite and > 0 (with the entry's index), n outside 0 .. BL_MAX_FREQUENCIES, a null array with n > 0;
 * adaptive_max_level > 0 with n >= 2 and adaptive_frequency_num absent or outside 1 .. n ("Must choose adaptive_frequency_num from 1
 * to image_num_frequencies."). BL_E_UNSUPPORTED: checkpoint_geodesic_load with n >= 1 (the file carries its own frequency list, which
 * replaces the context's). A refused call changes nothing. Works on a BL_DEVICE_NONE context. */
#define BL_MAX_FREQUENCIES 1024     /* the fast path's LDS table bound, bl_render.hip: job.n_nu <= 1024 */
BL_API int bl_set_frequencies(bl_ctx *ctx, int n, const double *hz);
BL_API int bl_num_frequencies(const bl_ctx *ctx);   /* 0 = unset: the parameter block's own list; -1: no context */
/* Arithmetic tier. BL_ARITH_TOLERANT (what a new context starts in, unless the environment says BLACKLIGHT_AMD_ARITHMETIC=exact): the
 * tolerance north_star grants for intensities ("within a stated fp64 tolerance", per-pixel L-infinity < 1e-6: every pixel relative to
 * its own intensity; measured 2e-14 per pixel - 6e-15 of the image maximum - on the benchmark frame's 1 048 576 pixels and against the
 * reference's own windows of it, asserted at 1e-10 per pixel: tests/test_gpu_window_1024.py, test_gpu_configs_at_size.py) is used between the sampled primitives and the transfer record of a sample -
 * fused multiply-adds, lighter exp / expm1 / cbrt, the fluid-frame angle and frequency as invariants instead of through the tetrad
 * of simulation_coefficients.cpp:398-455, transport matrices in polarized runs. Ray-step counts, flags, cell indices, NaN masks and
 * every cut decision are those of the exact tier. Where a pixel's accumulator I / nu^3 reaches the bottom of the normal range - its
 * samples' emission then passes through a subnormal exp(-x^(1/3)), whose unit 2^-1074 the exact tier carries as well - the bound is
 * absolute instead: |I - I_exact| <= max(1e-10 |I_exact|, 2^-1022 nu^3), and only there may one tier's pixel be zero where the
 * other's is a subnormal accumulator (tests/test_gpu_variant_edges.py). Configurations the tier has no kernel for run in exact arithmetic regardless -
 * bl_stats.arithmetic reports the tier that ran. BL_ARITH_EXACT: every operation in the reference's order with the pinned math
 * library - images equal the reference's bit for bit (tier-B goldens), at 0.57 of the tolerant tier's speed on the benchmark frame.
 * (Rounds 1 - 4 started contexts in the exact tier; the parity suite pins it through the environment variable, tests/conftest.py.) */
/* What to do with a sample for which the reference reads past the end of one of its arrays (no bounds checks in its Array):
 * inter-block interpolation at an upper edge of the file's last MeshBlock (simulation_sampling.cpp:520-522), FMKS sampling in
 * the last polar zone of the last azimuthal plane (:412-415 with :809-819). BL_UNDEFINED_REFUSE (default): bl_render fails with
 * BL_E_UNSUPPORTED - there is no defined result to reproduce. BL_UNDEFINED_EDGE: such samples use the edge of the data that
 * exists (block centre mirrored about the upper face; the zone's own row), and bl_render warns with their number. Every
 * sample the reference defines is unaffected by the choice. */
#define BL_UNDEFINED_REFUSE 0
#define BL_UNDEFINED_EDGE 1
/* BL_UNDEFINED_KAPPA (may be or-ed with BL_UNDEFINED_EDGE): kappa-distribution electrons (plasma_kappa_frac != 0) in an unpolarized
 * run. The reference's absorptivity reads kappa_aa_high_i (simulation_coefficients.cpp:652), which it sets for polarized runs only
 * (:108-121): whatever its allocator left there decides its image. Without this flag bl_render refuses such a run (BL_E_UNSUPPORTED);
 * with it the constant has its polarized definition, (3 / kappa)^4.75 + 0.6, and bl_render says so in a warning. No reference image
 * exists to compare with: the checker is the oracle under the same definition. */
#define BL_UNDEFINED_KAPPA 2
BL_API int bl_set_undefined_policy(bl_ctx *ctx, int policy);
#define BL_ARITH_EXACT 0
#define BL_ARITH_TOLERANT 1
BL_API int bl_set_arithmetic(bl_ctx *ctx, int mode);
/* Tolerant tier only (the exact tier is always bit-reproducible). on = 0 (default): the coefficient kernel composes the affine
 * transfer maps of a ray's neighbouring samples before they leave it (a quarter of the transfer records); which samples are
 * composed together follows the order in which the persistent geodesic waves emitted them, so two renders of one frame - or a
 * frame and its tiles - agree to rounding (~1e-15 of the image maximum), not bit for bit. on = 1: one transfer record per
 * sample, applied in ray order: tolerant images are then bit-identical from run to run and however a frame is cut into
 * bl_render calls, ranks or chunks, like the reference's are across thread counts (blacklight.cpp:196-233 is one deterministic
 * loop). Costs ~1.5 % of the benchmark frame. bl_stats.composed_maps says which way the last render went. */
BL_API int bl_set_reproducible(bl_ctx *ctx, int on);
/* Who steps the rays a chunk of geodesics waits for longest (per-ray independence, geodesics.cpp:109-324; the results are
 * bit-identical whichever way, only the time differs). BL_TAIL_WIDE: the persistent one-ray-per-lane stepper alone.
 * BL_TAIL_QUAD: it parks rays that outlive their neighbours and bl_geodesic_quad_kernel finishes them with a ray per quad of
 * lanes (1.5 - 1.65 x faster per ray; pays where a few rays run for thousands of steps - formula-mode frames - and costs where
 * they do not). BL_TAIL_SPLIT: the rays of a plane camera whose impact parameter lies within 0.12 M of the photon ring's
 * 3 sqrt(3) M - the longest of a frame by a factor of two - are given to bl_geodesic_quad_kernel before their first step, on a
 * stream whose CU mask keeps the other stepper off its compute units (hipExtStreamCreateWithCUMask); pays where the geodesic
 * stage waits for single rays - a rank's share of a tiled frame: an eighth of the benchmark frame 8.0 -> 7.2 ms - and needs a
 * non-rotating hole (the critical curve is a circle), the Dormand-Prince stepper and a call whose rays fit one chunk.
 * BL_TAIL_AUTO (default): QUAD in formula mode; SPLIT where it applies and the call has at most eight rays per lane of the
 * device (a share of a frame tiled over two or more GPUs); else WIDE. bl_stats.tail_policy says what the last render did. */
#define BL_TAIL_AUTO 0
#define BL_TAIL_WIDE 1
#define BL_TAIL_QUAD 2
#define BL_TAIL_SPLIT 3
BL_API int bl_set_tail_policy(bl_ctx *ctx, int policy);
/* Ordering against the caller's own GPU work. bl_render runs on streams of its own (non-blocking: the NULL stream does not order
 * them) and returns when its outputs are complete, so nothing the caller does AFTER the call needs ordering. What the caller
 * queued BEFORE it - a fill of the output buffers, an RCCL gather still reading the previous frame out of them - does:
 * with enabled != 0, every later bl_render first makes its streams wait (on the device, hipStreamWaitEvent: no host wait) for
 * all work queued on `stream` (a hipStream_t; NULL is the NULL stream) up to the moment of the call. */
BL_API int bl_set_caller_stream(bl_ctx *ctx, void *stream, int enabled);
/* Geodesics once per series. The reference integrates the root camera's geodesics ONCE, before its loop over snapshots
 * (blacklight.cpp:93-94 against :178-250), and - while the mesh does not change and slow light is off - locates the samples on the
 * grid once (`first_time`, radiation_integrator.cpp:693-704); per snapshot it only reads the cells, evaluates the coefficients and
 * integrates. on != 0 (default): a root-level bl_render whose rays fit one chunk leaves its sample records (64 B per sample: 48 GB
 * for the 1024^2 benchmark camera) and per-ray rows in HBM. A frame of more than one chunk (a 1024^2 full-Stokes frame, 64 frequencies,
 * 2048^2) keeps nothing the first time; the next render of that camera integrates again, with the scratch it already holds
 * re-partitioned (nothing allocated) into a record store for the whole frame beside shading arrays for one chunk, and the renders after
 * it shade the kept chunks one after another (bl_stats.n_chunks as that render had them) - reuse from the third frame on. Where no such
 * partition holds the frame's records, the frames integrate as before. Not kept there: located samples (located again every frame), anything under
 * bl_set_overlap(1), and no render that writes a geodesic or sample checkpoint integrates into the store. The next root-level
 * bl_render of this context with the SAME camera -
 * same parameters, pixel map, record layout, tail policy - after a new bl_set_grid / bl_slow_light_read shades those records again
 * instead of launching the stepper (bl_stats.geodesics_reused = 1, launches_geodesic = 0), and where a locate kernel of its own
 * ran, skips that too when the grid's geometry is bit for bit the one it located the samples on (bl_stats.sampling_reused).
 * Renders of refined levels in between (the adaptive loop of every snapshot) leave the root level's records alone: they work in
 * buffers of their own. The records go when the camera changes, when a render fails, when memory for another render cannot be
 * had otherwise, and with bl_free. Images are the same bits either way in the exact tier and under bl_set_reproducible (the records
 * ARE what the stepper would write again); with composed maps, equal to rounding like any two renders. The reference's warning
 * about geodesics that end unexpectedly is raised by the render that integrated them, once. on = 0: every render integrates its
 * rays (what a benchmark of the whole pipeline wants: bench.py's headline). */
BL_API int bl_set_geodesic_reuse(bl_ctx *ctx, int on);
/* Host memory the device copies into at the link's rate (pinned: hipHostMalloc). bl_render recognises such buffers among the pointers
 * of bl_render_desc - and any the caller pinned itself (hipHostRegister) - and downloads into them with one asynchronous-engine copy
 * (537 MB of image rows: ~10 ms) where pageable memory goes through the runtime's staging buffer (~16 GB/s: 34 ms; more host
 * threads bring nothing, the pages' first touch is what such a copy waits for). Large results in many rows (eight image rows or more, a quarter of a GiB or more)
 * leave chunk by chunk while the next chunk renders, whichever kind of memory receives them. NULL when the allocation fails or
 * the context is host-only: fall back to malloc. Free with bl_host_free (NULL is fine). */
BL_API void *bl_host_alloc(bl_ctx *ctx, size_t bytes);
BL_API void bl_host_free(bl_ctx *ctx, void *p);
/* Cap on scratch HBM (bytes) used for per-sample records; default four fifths of the device's memory (MI355X: 230 GB of 288). */
BL_API int bl_set_scratch_limit(bl_ctx *ctx, uint64_t bytes);
/* on != 0: when a render needs several chunks, run the geodesic kernel of chunk c + 1 on a second stream
 * beside the shading kernels of chunk c (two scratch sets of half the budget). Off by default: measured
 * on MI355X it changes the frame time by less than 1 %, and per-kernel times are cleaner off. */
BL_API int bl_set_overlap(bl_ctx *ctx, int on);
BL_API int bl_render(bl_ctx *ctx, const bl_render_desc *d);
/* Diagnostics (not part of the reference's interface): apply one device math function element-wise to
 * host arrays x (and y for two-argument functions; may be NULL otherwise) and return the results in out.
 * op: 0 exp, 1 expm1, 2 log, 3 cbrt, 4 sin, 5 cos, 6 acos, 7 atan, 8 atan2(x, y), 9 pow(x, y),
 * 10 hypot (blmath.h), 11 bl_hypot_g, 12 bl_sqrt_g, 13 bl_div_g(x, y) (bl_geometry.h), 14 sqrt, 15 x / y,
 * 16 sincos -> sin, 17 sincos -> cos; 38 bl_pow_neg_fifth (the step controller's x^(-1/5), blmath.h). Used by the tests to compare the
 * device arithmetic with the host's.
 * 40 (spin zero), 41 (any spin): not element-wise - the tolerant locate step's theta and phi of m points against an angular lattice,
 * relative to the centre of the guessed cell (what bl_shade_fused2_kernel computes where bl_stats.local_angles says so) and by acos /
 * atan2. x = [m, a, n_th, n_ph, xs[m], ys[m], zs[m]], y = [x2f[n_th + 1], x2v[n_th], x3f[n_ph + 1], x3v[n_ph]], both padded to n;
 * n >= 16 m and n >= 2 (n_th + n_ph) + 2; out = [16][m]: rows 0 - 7 relative to the centre - anchor cell in theta, in phi, fraction
 * in theta, in phi, smallest signed margin, undecided (margin <= 1e-12), guessed cell in theta, in phi - rows 8 - 15 the same from
 * acos / atan2. */
BL_API int bl_debug_math(bl_ctx *ctx, int op, int64_t n, const double *x, const double *y, double *out);
/* Tolerant tier, tests only: relative half-width of the band around an active cell cut threshold inside which the cut
 * decision of a sample is left to the exact kernel (default 1e-9; the tolerant arithmetic is good to ~1e-13). A wide band
 * defers many samples, which exercises the list and its overflow path. ops 20-27 of bl_debug_math are the tolerant
 * tier's exp, expm1, cbrt, reciprocal, reciprocal square root and K_0, K_1, K_2. */
BL_API int bl_debug_set_guard_band(bl_ctx *ctx, double relative_width);
/* The measurement switches of this context (BL_SWITCH_*, above) set by the program instead of the environment bl_init read:
 * what tests and A/B tools use between two renders of one context. */
BL_API int bl_debug_set_switches(bl_ctx *ctx, uint32_t switches);
BL_API int bl_get_stats(const bl_ctx *ctx, bl_stats *out);
/* Text of the last failure on this context ("Error: ...\n"), or "" */
BL_API const char *bl_last_error(const bl_ctx *ctx);
/* Text of the last failure of a call that has no context (bl_init) */
BL_API const char *bl_last_global_error(void);
/* Warnings raised by the last call, newline separated, reference wording ("Warning: ...\n") */
BL_API const char *bl_warnings(const bl_ctx *ctx);
BL_API void bl_warnings_clear(bl_ctx *ctx);   /* forget the warnings collected so far */
BL_API void bl_free(bl_ctx *ctx);

/* ------------------------------------------------------------------ steps between / after renders
 * The output writer runs on the host, as in the reference. The refinement decision exists twice with one result: bl_adaptive_refine
 * on the host (tiny, serial per block: the call for a level whose image is in host memory already, and the only one a host-only
 * context has) and bl_adaptive_refine_device on the GPU (one kernel launch over all blocks: the call for a level whose image lies in
 * HBM - bl_render_desc.outputs_on_device = 1, a de-tiled level of a distributed run - which then need not come down to be decided). */
#define BL_MAX_LEVELS 16

/* RadiationIntegrator::CheckAdaptiveRefinement + EvaluateBlock (radiation_adaptive.cpp:19-312) for the
 * level just rendered, followed by the block bookkeeping of GeodesicIntegrator::AugmentCamera
 * (camera.cpp:445-458): which blocks refine, and the (block_v, block_u) list of the next level in the
 * reference's order (parents in order, children (2v,2u), (2v,2u+1), (2v+1,2u), (2v+1,2u+1)).
 *   block_locs    [n_blocks][2] of this level; NULL at level 0 (root blocks, row-major)
 *   image         host [n_q][n_pix of this level] as filled by bl_render
 *   refine_flags  out [n_blocks]
 *   next_locs     out [4 * n_refined][2], may be NULL
 * Returns BL_OK; *n_refined = 0 means the adaptive loop is complete. */
BL_API int bl_adaptive_refine(const bl_ctx *ctx, int level, int n_blocks, const int32_t *block_locs,
                              const double *image, uint8_t *refine_flags, int32_t *n_refined,
                              int32_t *next_locs);

/* bl_adaptive_refine with the image in this context's HBM: the same meaning, the same flags and the same list, always (one source for
 * the criteria, csrc/bl_refine.h). block_locs, refine_flags and next_locs are host arrays as above; `image` is a device pointer to
 * [n_q][n_pix of this level], of which the one row the decision reads must lie inside one allocation of the context's device to its
 * end (the allocation as the runtime knows it, hipMemGetAddressRange: for memory handed out by a caching allocator that is the
 * allocator's segment, not the tensor carved from it - a tensor too short by less than its segment's slack passes this check, and
 * its extent is the caller's to get right, as Context.adaptive_refine_device does from the tensor's shape). One kernel launch decides every block and the flags (n_blocks bytes) come back with one copy; the list is built on the host
 * from them. adaptive_max_level <= 0 or level >= adaptive_max_level: all flags 0, nothing is launched. With bl_set_caller_stream
 * enabled the kernel starts behind the work queued so far on that stream (what fills `image`); the call returns when the flags are
 * on the host. Refused: what bl_adaptive_refine refuses, with its texts; a host-only context (BL_E_DEVICE); an `image` in host
 * memory, pinned or not, on another device, or too short (BL_E_ARG); adaptive_block_size = 1 with a gradient criterion on
 * (BL_E_UNSUPPORTED: the host reads past its one-pixel block there, as the reference does - no defined result). */
BL_API int bl_adaptive_refine_device(bl_ctx *ctx, int level, int n_blocks, const int32_t *block_locs /* host */,
                                     const double *image /* device: [n_q][n_pix of this level] */,
                                     uint8_t *refine_flags /* host out */, int32_t *n_refined, int32_t *next_locs /* host out, may be NULL */);

/* OutputWriter::Write (output_writer.cpp:169-274): npz / npy / raw exactly in the reference's layout
 * (numpy_format.cpp, zip_format.cpp, raw_format.cpp), format and array selection from the parameters. */
typedef struct bl_output_level {
  int32_t n_blocks;            /* levels > 0 */
  const int32_t *block_locs;   /* levels > 0: [n_blocks][2] */
  const double *image;         /* host [n_q][n_pix of the level] */
  const double *camera;        /* output_camera: positions (plane) or directions (pinhole) [n_pix][4] */
  const double *render;        /* render_num_images > 0: host [render_num_images][3][n_pix of the level] */
} bl_output_level;
typedef struct bl_output_desc {
  int32_t adaptive_num_levels; /* levels beyond the root that were rendered */
  bl_output_level level[BL_MAX_LEVELS + 1];
  int32_t snapshot;            /* run index, for output_file with {Nd} when simulation_multiple */
} bl_output_desc;
BL_API int bl_write_output(bl_ctx *ctx, const char *path_override, const bl_output_desc *d);
/* One variant of a sweep as a file of the reference's layout. d->level[0].image holds all V = bl_num_variants(ctx) images as
 * bl_render wrote them (V * n_q rows); `variant` counts in the image's own order: m * U + u for models x units, v for polarized
 * triples (BL_E_ARG outside 0 .. V - 1, and for adaptive levels, which a sweep cannot have). The file is what bl_write_output writes
 * from rows variant * n_q ... (variant + 1) * n_q - 1 in a context with that variant's plasma_rat_low, plasma_rat_high and
 * simulation_rho_cgs in its parameter block, byte for byte in all three formats, ZIP64 rules included: NO record of the reference's
 * files carries one of those three values (mass_msun, width, frequency, adaptive_*, positions / directions, the image rows and
 * renderings are all there is), so the files of a sweep differ in their image rows and nothing else; camera records and renderings
 * are the render's single copies, in every file. Rows are written from where the caller holds them. V = 1: variant must be 0 and
 * the call is bl_write_output. Works on a BL_DEVICE_NONE context.
 * Name: path_override if given, else bl_variant_output_path. */
BL_API int bl_write_output_variant(bl_ctx *ctx, const char *path_override, const bl_output_desc *d, int variant);
/* The name bl_write_output_variant gives the file of run `snapshot` and `variant`: output_file - with the file number where
 * bl_write_output formats one (simulation_multiple) - and, when V >= 2, a tag in front of the extension (the last '.' of the last path
 * component; appended where there is none):
 *     .mMMuUU   electron model MM (two digits, from 00) at density unit UU; both always present, 00 for a list that is not set
 *     .mMMuUUsSS  ... under sigma cut SS, where sigma cuts are set (bl_set_sigma_cuts): names without cuts are as above
 *     .eEEmMMuUU[sSS]  ... with electron mix EE, where mixes are set (bl_set_electron_mixes): names without mixes are as above
 *     .vVV      polarized triple VV
 * image.npz -> image.m00u00.npz, image.m00u01.npz, ... image.m02u01.npz: names sort in variant order. V = 1: no tag.
 * BL_E_ARG: variant outside 0 .. V - 1, or buf too short; BL_E_MISSING / BL_E_INPUT as bl_write_output. */
BL_API int bl_variant_output_path(bl_ctx *ctx, int snapshot, int variant, char *buf, size_t len);

/* One camera (and variant) of a render of several cameras as a file of the reference's layout. d->level[0] holds what bl_render
 * wrote for all C = max(1, bl_num_cameras) cameras: image [V * n_q][C * res^2], camera records [C * res^2][4], renderings
 * [render_num_images][3][C * res^2]. The file is, byte for byte in all three formats, what bl_write_output writes in a context with
 * that camera's angles (and that variant's values) in its parameter block from the camera's slice [c res^2, (c + 1) res^2) of every
 * row and record (a camera's rows are gathered into one block before they are written: they do not lie side by side in the
 * caller's arrays). BL_E_ARG: camera outside 0 .. C - 1, variant outside 0 .. V - 1, adaptive levels with C >= 2. C = 1: the call is
 * bl_write_output_variant. Works on a BL_DEVICE_NONE context. Name: path_override if given, else bl_camera_output_path. */
BL_API int bl_write_output_camera(bl_ctx *ctx, const char *path_override, const bl_output_desc *d, int camera, int variant);
/* The name bl_write_output_camera gives the file: bl_variant_output_path's, with - when C >= 2 - the camera's tag .cCC (two digits,
 * from 00) in front of the variant's tag inside the same dot group: image.c01.npz, image.c01m00u02.npz, image.c01m00u02s03.npz,
 * image.c01v03.npz; names sort in (camera, variant) order. C = 1: no camera tag. */
BL_API int bl_camera_output_path(bl_ctx *ctx, int snapshot, int camera, int variant, char *buf, size_t len);

/* ONE frequency (of one camera and variant) of a render as a file of the reference's layout. `frequency` indexes bl_frequencies -
 * the list bl_set_frequencies set, or the block's own spaced list. For every quantity with a frequency axis (I_nu ... V_nu, lambda,
 * emission, tau and the seven cell values of lambda_ave, emission_ave and tau_int) the file's rows are those of frequency `frequency`;
 * the rows without one (time, length, crossings), the renderings and the camera records are copied as they are; its `frequency`
 * record holds that one value. The file is, byte for byte in all three formats, what bl_write_output writes in a context whose block
 * has image_num_frequencies = 1 and image_frequency = that value (and that camera's angles and that variant's values) - the rows are
 * gathered into one block before they are written. BL_E_ARG: frequency outside the list, camera outside 0 .. C - 1, variant outside
 * 0 .. V - 1, adaptive levels with C >= 2 or V >= 2, and adaptive levels (adaptive_num_levels != 0) while the context has two
 * frequencies or more - a one-frequency run refines by its own image, so its file is not this one. Works on a BL_DEVICE_NONE
 * context. Name: path_override if given, else bl_frequency_output_path. */
BL_API int bl_write_output_frequency(bl_ctx *ctx, const char *path_override, const bl_output_desc *d, int frequency, int camera, int variant);
/* The name bl_write_output_frequency gives the file: bl_camera_output_path's, with the frequency's tag fFF (two digits and more,
 * from 00) inside the one dot group the other tags share, after the camera's and before the variant's: image.f02.npz,
 * image.c01f02m00u01.npz, image.f00v03.npz. The tag is there whatever the list's length - a list of one writes image.f00.npz - and
 * only in this call's names: every other name stays as it is. */
BL_API int bl_frequency_output_path(bl_ctx *ctx, int snapshot, int frequency, int camera, int variant, char *buf, size_t len);

/* Library self-description: "gfx950;hip" etc. Lets a loader verify the HIP path is the one built. */
BL_API const char *bl_build_info(void);

#ifdef __cplusplus
}
#endif
#endif /* BLACKLIGHT_AMD_H_ */
