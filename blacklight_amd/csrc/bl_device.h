// bl_device.h - data layout shared by the HIP kernels (bl_geodesic.hip, bl_shade.hip, bl_shade_fast.hip, bl_coefficients_freq.hip, bl_transfer.hip, bl_polarized.hip) and their host driver
// (bl_api.hip).
//
// HBM layout of one render chunk (all sizes for C rays, ray_max_steps = S, n_nu frequencies):
//
//   grid cells    float  [n_k][n_j][n_i][8]      32 B per cell: rho, pgas, uu1, uu2, uu3, bb1, bb2,
//                                                bb3 interleaved, i fastest, so the 8 corners of a
//                                                trilinear fetch are four 64-B segments
//   face / centre double x{1,2,3}f[n+1], x{1,2,3}v[n]  + per-axis bucket tables for the cell search
//   records       BlSampleHot, BlSampleCold [<= C*S]  2 x 32 B per emitted sample (position + id | momentum +
//                                                length), written by the geodesic kernel in wave-contiguous
//                                                runs; the locate kernel reads the first, the coefficient
//                                                kernel both (coalesced)
//   located       BlLocated [<= C*S] + tag [<= C*S]   32 + 8 B per sample: trilinear fractions + azimuth | first
//                                                cell + status, locate kernel -> coefficient kernel
//   transfer      double2 [C][S][n_nu]           (a, b) of the per-sample affine update
//                                                I <- a * (I + b), written by the shading kernel,
//                                                replayed far -> near by the transfer kernel
//   per ray       k_t, 1/nu_local, sample_num, flags, output index
#ifndef BLACKLIGHT_AMD_BL_DEVICE_H_
#define BLACKLIGHT_AMD_BL_DEVICE_H_

#include <stdint.h>

#include "bl_camera.h"
#include "bl_geometry.h"
#include "bl_kernel_plan.h"

// One emitted geodesic sample (geodesic_pos/dir/len entries of the reference, geodesics.cpp:250-293), before the
// per-sample momentum renormalisation of :352-371, in two 32-byte halves kept in two arrays: the locate kernel
// reads positions and ids only, and with the halves interleaved in one 64-byte record it fetched the whole line
// for half of it (24 GB instead of 12 GB per launch of the benchmark).
struct alignas(16) BlSampleHot {
  double x, y, z;     // position (CKS)
  uint32_t ray;       // chunk-local ray slot, 0xFFFFFFFF = dead slot (sample dropped by truncation)
  uint32_t n;         // sample index along the ray in integration order
};
struct alignas(16) BlSampleCold {
  double kx, ky, kz;  // covariant spatial momentum, not yet renormalised
  double len;         // affine step length as stored by the integrator (negative: camera -> source)
};
static_assert(sizeof(BlSampleHot) == 32 && sizeof(BlSampleCold) == 32, "record halves must be 32 bytes");

// One located sample, written by the locate kernel at the index of its sample record and read once by the
// coefficient kernel (simulation mode): where the sample sits on the grid. 32 bytes of fractions and azimuth
// (BlLocated) plus an 8-byte tag in its own array: bits 0..31 linear index of cell (k_m, j_m, i_m) resp. of the
// nearest cell, bits 32..39 SampleStatus, bits 40.. time slice (slow light). r^2, which the coefficient kernel
// needs again, is not handed over: with zero spin it is x^2 + y^2 + z^2, otherwise one hypot.
struct alignas(16) BlLocated {
  double f_i, f_j, f_k;   // trilinear fractions (kSampleInterp)
  double ph;              // unwrapped spherical Kerr-Schild azimuth (needed again by the Jacobian)
};
static_assert(sizeof(BlLocated) == 32, "located sample must be 32 bytes");

#define BL_DEAD_RAY 0xFFFFFFFFu
// Record slots a wave of the geodesic kernel reserves at a time (one global atomic per block); the
// record buffers hold one spare block per launched wave on top of chunk_rays * ray_max_steps.
#define BL_RECORD_BLOCK 1024
#define BL_XCD_QUEUES 8        // trace order per XCD (BlTraceArgs::xcd_state): one queue and one record list per XCD
#define BL_XCD_RUN 4096        // ... rays dealt to a queue at a time: a 64 x 64-pixel super-tile of the tile order
#define BL_XCD_BATCH 16        // ... groups of 64 records bl_shade_fused2_kernel claims from a list at a time
// Marker for "optically thick: I <- b" in the transfer record (exp(-dtau) is never negative)
#define BL_THICK_MARK (-1.0)
// ... and in the tolerant tier's affine records (a, c) of I <- a I + c: a = -0.0. An optically thick step's intensity REPLACES what lies
// behind it (unpolarized.cpp:103-104), a NaN included, so the transfer kernels must tell it from a thin step whose a = 1 + expm1(-tau)
// has rounded to +0 (tau > 37.4), behind which a NaN stays a NaN as in the exact tier (NaN x exp(-tau)). No other a is negative.
#define BL_AFFINE_THICK (-0.0)
#define BL_IS_AFFINE_THICK(a) (__double2hiint(a) < 0)
// A row of composed maps (BlShadeArgs::composed) that stands for per-sample records instead: a = -(number of samples) <= -1 (no
// map has such an a: a composed a lies in [0, 1], the thick mark is -0.0), c = the bit pattern of the first sample's record index;
// the transfer kernel replays transfer[first ... first + number) in its place.
#define BL_COMPOSED_EXPANDED(a) ((a) <= -1.0)

enum BlCounter {
  BL_CNT_NEXT_RAY = 0,      // work queue head of the geodesic kernel
  BL_CNT_RECORDS = 1,       // sample records allocated
  BL_CNT_GATHERS = 2,       // samples that read the grid (S_in)
  BL_CNT_OVERFLOW = 3,      // record buffer overflow flag
  BL_CNT_UNDEFINED = 4,     // inter-block interpolation: samples at an upper edge of the last MeshBlock
  BL_CNT_INTERP_FAILED = 5, // inter-block interpolation: samples for which no anchor block exists
  BL_CNT_REDO = 6,          // tolerant tier: samples left to the exact coefficient kernel (redo list entries)
  BL_CNT_COMMITTED = 7,     // geodesic kernel: record slots spoken for - ray_max_steps per ray in flight, what it emitted per finished ray
  BL_CNT_SAMPLES = 8,       // kept samples of the finished rays: where the next ray's per-sample rows start (BlTraceArgs::ray_offset)
  BL_CNT_PARKED = 9,        // rays bl_geodesic_kernel parked for bl_geodesic_quad_kernel (BlTraceArgs::parked)
  BL_CNT_COUNT = 10
};
// per scratch set: the counters above, four transfer statistics, eight debug counters (kernels built with -DBL_GEO_STATS)
#define BL_CNT_DEBUG (BL_CNT_COUNT + 4)
#define BL_CNT_QUAD_NEXT (BL_CNT_COUNT + 12)   // work queue head of the launch that finishes the parked rays: parked rays handed out
#define BL_CNT_UNDECIDED (BL_CNT_COUNT + 13)   // accepted steps whose sample count the closed-form distance did not decide (BlTraceArgs::distance_mode)
#define BL_CNT_PARKED_YOUNG (BL_CNT_COUNT + 14)  // parked rays with fewer than BlTraceArgs::park_age samples so far (BL_CNT_PARKED: the others)
#define BL_CNT_TOTAL (BL_CNT_COUNT + 15)

// dynamic LDS the refined instantiation of bl_shade_fused2_kernel may take (one 512-lane workgroup to a compute unit of 160 KiB)
#define BL_FUSED_REFINED_LDS (150 * 1024)
// ... and the tables of bl_locate_kernel<kRefined> (one 1 024-lane workgroup to a compute unit; 16 KiB more for its waves' lists)
#define BL_LOCATE_REFINED_LDS (136 * 1024)
// ... and of the exact second pass behind the fused kernel (256-lane workgroups, two to a compute unit, 8 KiB of anchor rows beside)
#define BL_REDO_TABLES_LDS (48 * 1024)

// Theta and phi relative to the centre of the guessed cell (bl_local_angles.h): how far a point of an angular cell may lie from the
// cell's centre for the arcsine's series to hold its bound - the plan's condition on BlGridDevice::angle_reach
constexpr double kLocalAngleReach = 1.0 / 16.0;

struct BlGridDevice {
  const float *cells;        // [n_k][n_j][n_i][8]
  const float *kappa;        // [n_k][n_j][n_i] electron entropy (plasma_model = code_kappa), else null
  const double *xf[3];       // faces  (r, theta, phi)
  const double *xv[3];       // centres
  const unsigned short *bucket[3];   // bucket -> first candidate cell
  double bucket_x0[3], bucket_inv_w[3];
  int n_bucket[3];
  // axes whose faces are evenly spaced to 1e-4 of a cell (bit a of uniform_mask): cell = floor((x - cell_x0) * cell_inv_w), which the
  // tolerant locate step takes as its guess and checks against the faces (locate_plain_from_angles)
  int uniform_mask;
  double cell_x0[3], cell_inv_w[3];
  // what bl_shade_fused2_kernel (bl_shade_fused.hip) asks of a grid: radial faces evenly spaced in log r to 1e-4 of a cell
  // (log_uniform; cell = floor((log2 r - log_l0) * log_inv_w), a guess the faces confirm), theta and phi covering the sphere
  // (full_sphere: no sample is off the grid in angle), and the first and last radial face
  int log_uniform, full_sphere;
  float log_l0, log_inv_w;
  double r_face_in, r_face_out;
  // ... and for theta and phi relative to the centre of the guessed cell (bl_local_angles.h): (cos, sin) of every theta and phi centre,
  // and the largest distance of a point of an angular cell from that cell's centre (the plan: at most local_angles::kAngleReach)
  const double *angle_trig[2];   // [n[1]][2], [n[2]][2]
  double angle_reach;
  float angle_guess[4];          // cell_x0[1], cell_inv_w[1], cell_x0[2], cell_inv_w[2] in single precision: the cell guess of those angles
  int n[3];                  // n_i, n_j, n_k of the (merged) global grid
  int nb[3];                 // cells per block along each axis (= n for a single block)
  int stride_row, stride_plane;   // cells between j- and k-neighbours in `cells` / `kappa`
  // Mesh refinement (blocks of several levels, simulation_sampling.cpp:352-394): `cells` is then
  // [block][n_k][n_j][n_i][8] with nb = block size, and the tables above are unused. n_blocks = 0: merged grid.
  int n_blocks;
  const double *edge[3];     // ascending distinct block boundaries per axis, n_edge[a] + 1 values
  int n_edge[3];
  const int *lattice;        // [n_edge[2]][n_edge[1]][n_edge[0]] -> block covering that box, -1: none
  // Coordinate rows of the blocks, each distinct row once (blocks at one level and position along an axis share theirs: a 256^3 mesh in
  // 64^3 blocks has 4 - 6 rows per axis, 36 - 64 blocks): small enough for the locate kernel to stage in LDS (refined_lds_bytes)
  const double *bxf[3];      // [n_rows[a]][nb[a] + 1] faces
  const double *bxv[3];      // [n_rows[a]][nb[a]] centres
  const int *block_row[3];   // [n_blocks]: a block's row along each axis
  const double *xv_next[3];  // [n_blocks]: first centre of the NEXT block of the file along the axis (what the reference's Array holds behind a
                             // block's last centre, simulation_sampling.cpp:520-522); unused for the last block
  const double *row_guess[3];   // [n_rows[a]][3]: where in a row to start the search for a coordinate s - kind (0: faces evenly spaced, 1: evenly
                                // spaced in log s), origin (the first face, or its log2), cells per unit (of s, or of log2 s); any start gives
                                // the same cell, a good one saves the walk
  int n_rows[3];
  double edge_first[3], edge_last[3];   // edge[a][0], edge[a][n_edge[a]]
  double box_guess[3][3];    // the same three numbers for the block boundaries along each axis
  int refined_lds_bytes;     // > 0: edges, lattice, rows, block table and hash fit the locate kernel's LDS budget (bl_locate_kernel<kRefined>)
  // The locate step inside bl_shade_fused2_kernel<..., kRefined> (bl_shade_fused.hip): a mesh whose boxes are evenly spaced in log r, theta
  // and phi, cover the sphere, and whose rows are evenly spaced likewise. Per box one descriptor: byte offset of the block's cells, LDS
  // offsets of the block's three row chunks (16-byte header with the row's cell guess, then 64 bytes per cell).
  const unsigned int *fused_desc;   // [n_edge[2]][n_edge[1]][n_edge[0]][4]
  int fused_lds_bytes;              // > 0: the kernel takes this mesh (cut table + row chunks + descriptors)
  float box_l0, box_linv;           // box along r = floor((log2 r - box_l0) * box_linv)
  double box_x0[2], box_inv_w[2];   // along theta and phi = floor((x - box_x0) * box_inv_w)
  // Inter-block interpolation (simulation_block_interp; simulation_sampling.cpp:505-546, :1068-1321): the MeshBlock
  // table and a hash from (level, location) to block - the reference scans all blocks for every such lookup
  int block_interp;
  const int *levels;             // [n_blocks]
  const int *locations;          // [n_blocks][3]
  const unsigned long long *hash_keys;   // open addressing, hash_mask + 1 slots, ~0ull = empty
  const int *hash_blocks;
  unsigned int hash_mask;
  int max_level, n_3_level0;     // n_3_level(level) = n_3_level0 << level (:84-93)
  // FMKS grids (simulation_coord = fmks; simulation_sampling.cpp:190-198, :396-456): one block in native coordinates
  // (tables above: only x^3 is searched in them), position in x^1, x^2 from the reader's look-up table
  int fmks;
  const double *sks_map;         // [2][sks_map_n2][sks_map_n1]
  int sks_map_n1, sks_map_n2;
  double sks_map_r_in, sks_map_dr, sks_map_dtheta;
  double fmks_bounds[6];         // r, theta, phi limits of the grid
  double fmks_x1_0, fmks_dx1, fmks_dx2;
};

struct BlPlasmaDevice {
  // units (simulation_coefficients.cpp:237-239)
  double d_unit, e_unit, b_unit;
  double plasma_mu, plasma_ne_ni, plasma_rat_low, plasma_rat_high, plasma_thermal_frac;
  int plasma_use_p;
  int simulation_interp;
  int simulation_coord;
  int fallback_nan;
  int any_cell_cut;          // some cell cut threshold (simulation_coefficients.cpp:361-375) is >= 0
  // power-law electrons (simulation_coefficients.cpp:54-66, :556-584); power_frac = 0: none
  double power_frac, plasma_p, power_jj, power_aa;
  int kappa_frac_zero;       // plasma_kappa_frac == 0 (BlShadeCold::kappa.frac lives in HBM; the launchers choose instantiations by this)
  int code_kappa;            // plasma_model = code_kappa: theta_e from the simulation's electron entropy (:351-358)
  int cut_mask;              // bit c set: cell cut threshold c (BlShadeCold::fast_cut order) is active
  int kappa_unpolarized;     // kappa-distribution electrons in an unpolarized run (BL_UNDEFINED_KAPPA): BlShadeCold::kappa's intensity terms
};

// Kappa-distribution electrons (simulation_coefficients.cpp:82-193; the reference's names without the prefix).
// frac = 0: none. The reference defines every constant in polarized runs only: an unpolarized run reads aa_high_i without ever
// setting it, and is rendered here only under bl_set_undefined_policy(BL_UNDEFINED_KAPPA), with the polarized definition.
struct BlKappaDevice {
  double frac, kappa, w;
  double jj_low, jj_high, jj_x_i, aa_low, aa_high, aa_x_i;
  double jj_low_q, jj_low_v, jj_high_q, jj_high_v, jj_x_q, jj_x_v;
  double aa_low_q, aa_low_v, aa_high_i, aa_high_q, aa_high_v, aa_x_q, aa_x_v;
  double rho_v, rho_frac;
  double rho_q_low[5], rho_q_high[5];   // a, b, c, d, e of the two fits that bracket kappa
  double rho_v_low[2], rho_v_high[2];   // a, b
};

// Rarely used parameters of the shading kernel (optional geometric cuts, cell cut thresholds,
// fallback primitives): kept in HBM behind one pointer and read under wave-uniform flags, so they do
// not occupy SGPRs in the common case where they are all disabled.
struct BlShadeCold {
  int omit_near, omit_far, plane;
  double omit_in, omit_out, midplane_theta, midplane_z;
  double plane_origin[3], plane_normal[3];
  double cam_x[4];
  double cut_rho_min, cut_rho_max, cut_n_e_min, cut_n_e_max, cut_p_gas_min, cut_p_gas_max;
  double cut_theta_e_min, cut_theta_e_max, cut_b_min, cut_b_max, cut_sigma_min, cut_sigma_max;
  double cut_beta_inverse_min, cut_beta_inverse_max;
  float fallback_rho, fallback_pgas, fallback_kappa;
  double plasma_gamma, plasma_gamma_i, plasma_gamma_e;
  BlKappaDevice kappa;
  // Tolerant tier: the active cell cut thresholds in the order rho, n_e, p_gas, theta_e, B, sigma, 1 / beta, each
  // (min, max), and the guard band around each (threshold * (1 -+ 1e-9)) inside which the decision is left to the
  // exact kernel
  double fast_cut[14], fast_cut_lo[14], fast_cut_hi[14];
};

struct BlFormulaDevice {
  double r0, h, l0, q, nup, cn0, alpha, a, beta;
};

struct BlCutsDevice {
  int any_optional;          // any cut besides r > camera_r is active (details in BlShadeCold)
  double camera_r;
};

// Per-sample inputs of the auxiliary images (unpolarized.cpp:113-173), stored [ray][n] like the transfer
// records. Only written and read when an auxiliary image is requested; in that mode the transfer buffer
// holds (j_nu, alpha_nu) per sample and frequency instead of (a, b).
#define BL_NUM_CELL_VALUES 7   // blacklight.hpp:30-33: rho, n_e, p_gas, theta_e, bb, sigma, beta_inv
struct alignas(16) BlAuxSample {
  double delta_lambda;               // sample_len in geometric units
  double length_term;                // sqrt(dl_dlambda_sq) * delta_lambda * x_unit (image_length)
  double t;                          // coordinate time of the sample (image_time)
  double plane;                      // camera_x . x (image_crossings compares its sign between samples)
  double cell[BL_NUM_CELL_VALUES];   // cell_values, NaN when not recorded
  double pad;
};
static_assert(sizeof(BlAuxSample) == 96, "aux sample must be 96 bytes");

// Which auxiliary images are requested, and where their rows start (radiation_integrator.cpp:436-520)
struct BlAuxImages {
  int any;
  int image_light, image_time, image_length, image_lambda, image_emission, image_tau;
  int image_lambda_ave, image_emission_ave, image_tau_int, image_crossings;
  int offset_time, offset_length, offset_lambda, offset_emission, offset_tau;
  int offset_lambda_ave, offset_emission_ave, offset_tau_int, offset_crossings;
  int n_q;
  int polarized;   // rows 4 l + (I, Q, U, V) written by the polarized transfer kernel instead of row l
  int polarized_rows_only;   // polarized run whose only other row is tau (or none), no rendering: the polarized transfer kernel
                             // accumulates tau beside the Stokes parameters, the auxiliary kernel keeps its bookkeeping only
                             // and the coefficient kernel writes no BlAuxSample
};

// False-colour rendering parameters (rendering.cpp; a device buffer, too large for kernel arguments)
struct BlRenderDevice {
  int n_images;
  int fill_present;
  int n_features[BL_MAX_RENDER_IMAGES];
  int quantity[BL_MAX_RENDER_IMAGES][BL_MAX_RENDER_FEATURES];
  int type[BL_MAX_RENDER_IMAGES][BL_MAX_RENDER_FEATURES];
  double min_val[BL_MAX_RENDER_IMAGES][BL_MAX_RENDER_FEATURES], max_val[BL_MAX_RENDER_IMAGES][BL_MAX_RENDER_FEATURES];
  double thresh[BL_MAX_RENDER_IMAGES][BL_MAX_RENDER_FEATURES], tau_scale[BL_MAX_RENDER_IMAGES][BL_MAX_RENDER_FEATURES];
  double opacity[BL_MAX_RENDER_IMAGES][BL_MAX_RENDER_FEATURES];
  double xyz[BL_MAX_RENDER_IMAGES][BL_MAX_RENDER_FEATURES][3];
};

// Kernel arguments: geodesic kernel
struct BlTraceArgs {
  BlSpacetime st;
  BlCameraDevice cam;
  double r_terminate, r_horizon, camera_r;
  double ray_step, ray_tol_abs, ray_tol_rel;
  int ray_max_steps, ray_max_retries;
  long long chunk_begin;      // first traversal index of this chunk
  int chunk_rays;
  long long n_rays_total;
  int swizzle_tiles;          // >0: traversal order walks 8x8 pixel tiles of a swizzle_tiles-wide image
  const int *tile_order;      // device [tiles of the image] or null: order in which the 8x8 tiles are traced
  const int *pixel_map;       // device, or null
  const int *block_locs;      // device, or null
  BlSampleHot *records_hot;
  BlSampleCold *records_cold;
  int record_stride;          // 1: the two halves of a record in arrays of their own; 2: interleaved, 64 bytes per record (records_cold = records_hot + 1)
  double *sample_t;           // optional [record capacity]: coordinate time of each sample (image_time)
  long long record_capacity;
  // The geodesic kernel hands a ray to a lane only while BL_CNT_COMMITTED + ray_max_steps <= record_gate (= capacity minus one
  // block per wave): a chunk is the rays that fit the record buffers as they turn out, not as the worst case would have them.
  // Rays it did not get to (BL_CNT_NEXT_RAY < chunk_rays at the end) are the next chunk's.
  long long record_gate;
  unsigned long long *counters;
  double2 *ray_constants;     // [chunk_rays]: (k_t, momentum factor), written once at ray start (read: bl_ray_constants and its two halves)
  int *ray_sample_num;
  unsigned char *ray_flags;
  long long *ray_out_index;
  long long *ray_offset;      // [chunk_rays]: first row of the ray's kept samples in the per-sample arrays (transfer records, ...)
  double *camera_pos, *camera_dir;  // optional [n_rays][4] indexed by output index
  // Start state of every ray of the chunk, written by bl_ray_init_kernel (one ray per lane, every lane busy) and read by the
  // persistent geodesic kernel when it hands a ray to an idle lane: BL_RAY_START_FIELDS rows of ray_start_stride doubles,
  // [field][chunk slot] - t, x, y, z, k_x, k_y, k_z | k_t | r | first-stage derivatives (Dormand-Prince only)
  double *ray_start;
  long long ray_start_stride;
  // Steps in the empty shell between the grid's outer edge and the camera's sphere leave no records (plain images of a spherical
  // Kerr-Schild simulation with fallback values: every sample there is off the grid, has no field and adds nothing, simulation_
  // sampling.cpp:352-394, simulation_coefficients.cpp:394). A step is skipped when the bound |p - y| <= sum_q |r_q| on its dense
  // output puts all its samples there: |y| - d > skip_low (= sqrt(r_out^2 (1 + 1e-9) + a^2); r_KS^2 >= R^2 - a^2) and
  // |y| + d < skip_high (= camera_r (1 - 1e-9); r_KS <= R). skip_low = +inf: every step is recorded. The samples still count
  // (sample_num, ray_max_steps); ray_skipped[slot] is how many of a ray's samples have no record.
  double skip_low, skip_high;
  int *ray_skipped;
  // Composed transfer maps (tolerant tier, bl_shade_fused2_kernel with one map per segment): records carry segment numbers instead
  // of sample numbers, ray_offset counts segments, ray_rows[slot] = the ray's segments (bl_geodesic_kernel's emission loop)
  int segment_rows;
  int *ray_rows;
  // Parked rays (Dormand-Prince, no sample times, no skipped shell; BL_SWITCH_QUAD_TAIL - a measured experiment, off by default).
  // A ray advances one step per pass of its wave through ~6 000 instructions however few of the wave's lanes still hold one, so
  // the last rays of a chunk - a wave with nothing left to refill its idle lanes from - set the kernel's time. Such a wave, once
  // park_below or fewer of its lanes hold a ray, writes those rays to parked[] (BL_PARK_DOUBLES doubles each, below; BL_CNT_PARKED
  // counts them) and ends; bl_geodesic_quad_kernel, launched behind it, finishes them with a ray per QUAD of lanes in two thirds
  // of the instructions per step - the same operations on the same operands, so the same bits (bl_geodesic_quad.hip: what it
  // gains and costs). park_always: every wave parks every ray it is handed before its first step (tests: the whole frame
  // goes through the quad kernel). parked == nullptr: no ray is parked.
  double *parked;
  int park_capacity;
  int park_below;
  int park_after;    // ... or, however many lanes hold one, park_after passes of the wave after it first had nothing to refill a lane from
  // Parked rays are taken up again oldest first: those with park_age samples or more fill parked[] from the front (BL_CNT_PARKED),
  // the others from the back (BL_CNT_PARKED_YOUNG) - a ray that is long so far is likely to be long, and the launch that finishes
  // them ends with its longest ray, which should not be the last to get a quad.
  int park_quiet;    // ... or park_quiet passes without a ray of the wave finishing (its rays are long ones)
  int park_age;
  int quad_first_round;   // bl_geodesic_quad_kernel: its first this many waves (one per SIMD) run at raised priority
  int park_always;
  // Rays predicted long, on compute units of their own from the first moment (BL_TAIL_SPLIT: docs/notebook.md section
  // 5k). bl_split_long_kernel parks - before either stepper starts - the rays of a plane camera whose impact parameter lies in
  // [split_b_lo, split_b_hi] (in units of M: the band around the photon ring's critical curve) and marks their start state (r < 0);
  // bl_geodesic_kernel passes a marked ray over, bl_geodesic_quad_kernel steps the parked ones on a stream whose CU mask the
  // other stream's excludes. split_b_hi = 0: no split.
  double split_b_lo, split_b_hi;
  // Trace order per XCD (off: BL_SWITCH_FLAT_ORDER; bl_render.hip: XcdOrderApplies). The chunk's traversal indices are dealt to BL_XCD_QUEUES queues in runs
  // of BL_XCD_RUN (a 64 x 64-pixel super-tile of the tile order): run m is queue m % BL_XCD_QUEUES's. A wave refills from the
  // queue of the XCD it runs on (HW_REG_XCC_ID) and from the others once that one is dry, and lists every block of record slots it
  // takes - as its aligned groups of 64 records - in that XCD's list, which bl_shade_fused2_kernel walks on the same XCD: the
  // records shaded side by side on one XCD are then those of neighbouring rays, whose gathers share cells in its L2. Placement
  // changes only speed. xcd_state: [0, 8) queue heads (rays handed out, by queue), [8, 16) list lengths (groups), [16, 24) the
  // coefficient kernel's cursors into the lists, [24] waves that have ended; xcd_lists: BL_XCD_QUEUES lists of xcd_list_capacity
  // group indices (record index / 64). Null: one queue, no lists - BL_CNT_NEXT_RAY is the head. With the queues BL_CNT_NEXT_RAY
  // is written by the last wave to end: the rays before the first one no queue handed out (a gate that closed leaves the others
  // to be traced again by the next chunk; only the rays before it are transferred).
  unsigned long long *xcd_state;
  unsigned int *xcd_lists;
  long long xcd_list_capacity;
  // Several cameras as one set of rays (bl_set_cameras with n >= 2): the level's pixels are "virtual pixels" v = c pixels_per_camera + m;
  // bl_ray_init_kernel starts ray v from cameras[c] at pixel m of that camera. Null: every ray is `cam`'s (pixels_per_camera unread).
  const BlCameraDevice *cameras;
  long long pixels_per_camera;
  // The proper distance of bl_geodesic_kernel's Dormand-Prince steps (bl_distance_closed.h; the plan's choice, KernelPlan::Geodesic::
  // distance). 0: the reference's operations in every stage, state component 7 its s. 1: the closed form; component 7 holds an upper
  // bound of |s|, a step's sample count is taken from the closed form where the bound on its distance from the reference's leaves
  // no integer in doubt, and every other accepted step adds one to BL_CNT_UNDECIDED - the host then discards the frame. 2: as 1 with
  // a band of 0.25 in the count (BL_SWITCH_WIDE_DISTANCE_BAND: exercises the host's second render).
  int distance_mode;
};
#define BL_RAY_START_FIELDS 17
// A parked ray (BlTraceArgs::parked): everything bl_geodesic_kernel holds of a ray between two steps, BL_PARK_DOUBLES doubles
//   0..7 the state t, x, y, z, k_x, k_y, k_z, s | 8..15 the first stage of the next step (FSAL) | 16 k_t | 17 the next step's
//   length | 18 r at the state | 19 r of the last sample | 20 (chunk slot, samples so far) | 21 (retries, index of the
//   truncating sample or -1) | 22 (segments so far, bit 0 previous step failed + bit 1 flagged) | 23 unused
#define BL_PARK_DOUBLES 24

// Kernel arguments: shading kernel
// Polarized transfer (image_polarization): what the polarized transfer kernel needs of every sample besides the
// eight coefficients - position (for the metric and the connection), affine length, k^mu = g^{mu nu} k_nu with the
// renormalised momentum, and rows 1 and 2 of the fluid tetrad (the only rows the Stokes projection and its inverse
// read: polarized.cpp:268-292, :793-813). The coefficient kernel has all of it at hand (simulation_coefficients.cpp:
// 398-431 builds the same tetrad from the same inputs as polarized.cpp:201-265). 128 bytes.
// Tolerant tier, per sample: the transport matrix (3 x 3 block of I, Q, U by rows, then the V number), the sample's length, a spare
#define BL_POL_MATRIX_DOUBLES 12
struct alignas(16) BlPolSample {
  double x[3];
  double delta_lambda;
  double kcon[4];
  double e1[4], e2[4];
};

// Tolerant tier with several frequencies (BlShadeArgs::freq_split): what is left of a sample once everything that does not
// depend on the frequency has been evaluated - the factors of bl_shade_fast_kernel's frequency loop. bl_transfer_freq_kernel
// (one lane per ray and frequency) turns them into the sample's (a, c) and applies it on the spot: no transfer records.
// flag: 0 nothing to add (cut sample, cut cell, no field), 1 coefficients follow, 2 NaN (off the grid with fallback_nan).
// A sample whose cut decision is deferred gets its factors from the exact second pass (bl_shade_kernel<..., kRedo>). 64 bytes.
struct alignas(16) BlFreqInputs {
  double flag;
  double s_1_2, s_1_3, s_1_6;   // x^(1/2), x^(1/3), x^(1/6) of x = nu / nu_s at unit frequency
  double s_planck;              // h nu / (k T_e) at unit frequency
  double s_j;                   // j_nu nu^2 e^(x^(1/3)) / var_c^2
  double s_length;              // delta lambda in cm at unit frequency
  double pad;
};
// ... and with several electron models in one pass (BlShadeArgs::freq_split = 2, BlTransferArgs::n_models): the same 64 bytes hold
// what no model enters - (flag, x at unit frequency and unit 1 / (k T_e)), (h s_nu, s_j), (s_length, 1 / beta^2), (K0 p / rho, sigma) -
// and bl_transfer_freq_kernel forms each model's 1 / (k T_e) = (K1_m + K2_m / beta^2 + K3 d) / (K0 (p / rho) d), d = 1 + 1 / beta^2.
#define BL_TRANSFER_MAX_MODELS 16
// ... and with density units (BlTransferArgs::n_units): the row is the unit the render folded (RenderJob::base_rho); unit u scales x at
// unit frequency (~ 1 / b_unit) by unit_x[u] and s_j (~ d_unit b_unit) by unit_j[u]. Nothing else in the row depends on the unit.
#define BL_TRANSFER_MAX_UNITS 16
// ... and with sigma cuts (BlTransferArgs::n_cuts): the coefficient kernels ran with the sigma upper cut off, the row's last double is
// the sample's sigma = b.b / rho in code units (every writer of the model-free row stores it), and cut s leaves out the samples with
// sigma > sigma_max[s]. The tolerant kernels leave a sample whose sigma lies in the guard band of any threshold to the exact pass
// (BlShadeArgs::sigma_band_lo / _hi), whose row holds the exact tier's sigma.
#define BL_TRANSFER_MAX_CUTS 16
// ... and with electron mixes (BlTransferArgs::n_mixes): the coefficient kernels folded a thermal fraction of 1 into s_j, and the lane
// applies its own mix - the thermal fraction on the thermal line, the power-law terms from the same row (bl_transfer_freq_kernel)
#define BL_TRANSFER_MAX_MIXES 16
#define BL_SHADE_MAX_SIGMA_CUTS 16

// Polarized runs: what the per-frequency coefficient formulas need of a sample (simulation_coefficients.cpp:458-698),
// left by the coefficient kernel for bl_polarized_coefficients_kernel, one per sample record. 64 bytes.
struct alignas(16) BlCoefInputs {
  double nu_fluid_over_nu;   // -k_mu u^mu
  double n_e_cgs, nu_c_cgs, theta_e, kb_tt_e_cgs;
  double cos2_theta_b;       // min(cos^2, 1) (:449-452)
  double cos_sign;           // +-1: sign of k.b in the fluid frame (:455)
  double have_coefficients;  // 1: the sample has coefficients; 0: j = alpha = rho = 0 at every frequency
};
#if defined(__HIPCC__) || defined(__HIP__)
// ... and in plain images with several frequencies (BlShadeArgs::coef_split) what the unpolarized formulas need, left by the
// coefficient kernel for bl_coefficients_freq_kernel. They take sin theta_B and neither the cosine nor its sign, and the transfer
// record takes the sample's length: such a row carries sin theta_B in cos2_theta_b and the length in cos_sign. This pair is the
// only code that knows. (Shade: SampleShade, bl_sampling.h. unpack returns the length.)
template <class Shade>
__device__ __forceinline__ BlCoefInputs bl_pack_plain_coef_inputs(const Shade &sh, double delta_lambda) {
  BlCoefInputs ci;
  ci.nu_fluid_over_nu = sh.nu_fluid_over_nu;
  ci.n_e_cgs = sh.n_e_cgs;
  ci.nu_c_cgs = sh.nu_c_cgs;
  ci.theta_e = sh.theta_e;
  ci.kb_tt_e_cgs = sh.kb_tt_e_cgs;
  ci.cos2_theta_b = sh.sin_theta_b;
  ci.cos_sign = delta_lambda;
  ci.have_coefficients = sh.have_coefficients ? 1.0 : 0.0;
  return ci;
}
template <class Shade>
__device__ __forceinline__ double bl_unpack_plain_coef_inputs(const BlCoefInputs &ci, Shade *sh) {
  sh->have_coefficients = ci.have_coefficients != 0.0;
  sh->nu_fluid_over_nu = ci.nu_fluid_over_nu;
  sh->n_e_cgs = ci.n_e_cgs;
  sh->nu_c_cgs = ci.nu_c_cgs;
  sh->theta_e = ci.theta_e;
  sh->kb_tt_e_cgs = ci.kb_tt_e_cgs;
  sh->sin_theta_b = ci.cos2_theta_b;
  return ci.cos_sign;
}
#endif

// ... and with several polarized variants in one pass (bl_set_polarized_variants, BlShadeArgs::pol_variants > 0) the row of a sample
// with coefficients holds what no variant enters: n_e_cgs = the cell's rho and p_gas (two floats), nu_c_cgs = b_mu b^mu in code units,
// theta_e = kb_tt_e_cgs = 0; bl_polarized_coefficients_kernel forms n_e, nu_c, Theta_e and k T_e of every variant from them and the
// variant's folded constants below (rows of samples without coefficients are as ever: bl_polarized_frame_kernel reads them) - and
// with a sigma cut per variant (bl_set_polarized_variants_sigma) decides each variant's cut from the same two values.
#define BL_POL_MAX_VARIANTS 16
struct alignas(16) BlPolVariant {
  double d_unit, e_unit, b_unit;   // FoldUnits of the variant's simulation_rho_cgs
  double rat_high, rat_low;
  double sigma_max;                // the variant's cut_sigma_max where the variants' cuts differ: no coefficients for a sample with
                                   // b.b / rho above it; +inf: no cut here (off, or equal for all and decided in the shared pass)
};

// Slow light (slow_light_on): the time slices the reader holds (simulation_reader.cpp:211-303), latest
// first, all on the geometry of BlGridDevice. n = 0: off.
struct BlSlowDevice {
  int n;                           // slow_chunk_size
  int interp;                      // slow_interp: linear in time between two slices, else the nearest slice
  double snapshot_time;            // camera time of this image
  const double *times;             // device [n], descending
  const float *const *cells;       // device [n]: cell array of every slice (layout of BlGridDevice::cells)
  const float *const *kappa;       // device [n] or null
  unsigned int *ray_extrap;        // [chunk rays]: bit e set = some sample needed extrapolation of kind e
  unsigned long long *extrap_max;  // [4]: bit pattern of the largest extrapolation of each kind (doubles >= 0)
  double *frac;                    // [record capacity]: t_frac of a located sample
};

struct BlShadeArgs {
  BlSpacetime st;
  BlCutsDevice cuts;
  BlPlasmaDevice plasma;
  BlFormulaDevice formula;
  BlGridDevice grid;
  BlSlowDevice slow;
  const BlShadeCold *cold;    // device pointer
  const BlSampleHot *records_hot;
  const BlSampleCold *records_cold;
  int record_stride;          // as in BlTraceArgs
  BlLocated *located;         // [record capacity], simulation mode
  unsigned long long *located_tag;   // [record capacity]: cell | status << 32 | time slice << 40
  BlFreqInputs *freq_inputs;         // [sample row] when freq_split
  int coef_split;                    // exact tier, plain images, n_nu >= 4: BlCoefInputs for bl_coefficients_freq_kernel instead of the frequency loop
  int freq_split;                    // tolerant tier, n_nu >= 4: per-sample factors instead of per-frequency transfer records;
                                     // 2: electron models in one pass - the factors' model-free layout (BlFreqInputs)
  int tag_in_record;                 // tolerant tier: the tag is written into BlLocated::ph instead (32 bytes per sample, one stream)
  int lds_table_bytes;        // size of the coordinate tables the locate kernel stages in LDS; 0: searched in HBM
  int samples_renormalised;   // records come from a geodesic checkpoint: momenta as stored, no renormalisation per sample
  int tolerant;               // bl_set_arithmetic(BL_ARITH_TOLERANT): kernels that have a tolerant instantiation use it
  // Composed transfer maps (bl_shade_fused2_kernel): one (a, c) per SEGMENT of a ray (BlTraceArgs::segment_rows) in row
  // ray_offset[ray] + segment of `composed`; `transfer` is then indexed by RECORD and written only for the samples of a wave that
  // holds a deferred sample or an optically thick step (the segment's row then says where they are: BL_COMPOSED_EXPANDED)
  double2 *composed;          // [segment row], or null: one transfer record per sample
  int general_locate;         // measurement switch (bl_stats.switches): the general locate kernel where the plain one applies; refined tables in HBM
  int undefined_edge;         // bl_set_undefined_policy(BL_UNDEFINED_EDGE): samples where the reference reads past its arrays use the edge
  int local_angles;           // bl_shade_fused2_kernel over one block: theta and phi relative to the centre of the guessed cell (bl_local_angles.h;
                              // the plan: angular cells within the series' reach, not BL_SWITCH_GLOBAL_ANGLES); 0: acos / atan2
  int general_cuts;           // measurement switch (bl_stats.switches): bl_shade_fused2_kernel's general cut block where cut_sigma_max is the only
                              // active threshold and its short form applies (fused2::cut_selection)
  const unsigned long long *counters_in;
  unsigned long long *counters;
  // bl_shade_fused2_kernel: the record lists of the geodesic kernel's trace order per XCD (BlTraceArgs::xcd_state), walked in
  // groups of 64 records from the list of the XCD a wave runs on and from the others once that one is done; the cursors
  // (xcd_state[16, 24)) are zero at the launch. Null: the records in one grid-stride walk.
  unsigned long long *xcd_state;
  const unsigned int *xcd_lists;
  long long xcd_list_capacity;
  // Mirror pairs (bl_render.hip: MirrorPairsApply; 0: off): only the left half of a frame whose camera lies in the mirror plane y = 0 of
  // a zero-spin spacetime was traced, and bl_shade_fused2_kernel, bl_shade_exact2_kernel and bl_shade_kernel<..., kRedo> walk the record
  // indices [0, 2 n) of the n = BL_CNT_RECORDS records (a multiple of 64): index i >= n is record i - n as the mirror pixel's ray - the sign
  // bits of y and k_y flipped, everything else the traced ray's - with its rows row_add (the rows the traced half may fill) beyond the
  // traced ray's in `composed` / `transfer`. What a kernel writes by record index (the per-sample records behind BL_COMPOSED_EXPANDED,
  // redo_list) it writes by the index walked.
  unsigned int row_add;
  const double2 *ray_constants;   // [chunk_rays]: (k_t, momentum factor) of BlTraceArgs::ray_constants
  const long long *ray_offset;   // [chunk_rays]: sample n of ray q has row ray_offset[q] + n in transfer, aux, pol_samples, freq_inputs, ...
  const double *frequencies;  // device [n_nu]
  int n_nu;
  int ray_max_steps;
  double x_unit;              // GM/c^2 in cm (unpolarized.cpp:42)
  double2 *transfer;          // [sample row][n_nu]; (a, b), or (j, alpha) in auxiliary mode
  double *tau_inc;            // tolerant tier with an optical-depth image: [sample row][n_nu] alpha x length of every sample, or null
  // auxiliary-image mode only
  BlAuxSample *aux;           // [sample row]
  const double *sample_t;     // [record capacity] or null
  const unsigned char *ray_flags;
  // polarized transfer only (runs in auxiliary-image mode): null otherwise
  BlPolSample *pol_samples;   // [sample row]
  double2 *pol_coeffs;        // [sample row][n_nu][4]: (j_I, alpha_I), (j_Q, j_V), (alpha_Q, alpha_V), (rho_Q, rho_V) - one 64-byte record, half a
                              // cache line, for the lane of the sequential kernels that walks the ray (polarized runs have no `transfer` array)
  BlCoefInputs *coef_inputs;  // [record capacity]: coefficient kernel -> polarized coefficient kernel
  int pol_variants;           // > 0: polarized variants in one pass - coef_inputs rows in their variant-free layout (BlPolVariant), and
                              // bl_polarized_coefficients_kernel with a wave per (64 records, variant): pol_coeffs[(sample row * pol_variants + v)][n_nu][4]
  const BlPolVariant *pol_variant_table;   // device [pol_variants]
  unsigned char *have_flags;  // [record capacity] or null: bl_shade_polarized2_kernel<..., kCoefficients> evaluates the coefficients itself and
                              // says here which records have them (bl_polarized_frame_kernel: the others' frames)
  unsigned int *anchors;      // inter-block interpolation: [record capacity][8] cells of the eight anchors, else null
  double power_pol[7];        // simulation_coefficients.cpp:67-80: jj_q, jj_v, aa_q, aa_v, rho, rho_q, rho_v
  double plasma_gamma_min;
  // tolerant arithmetic tier (bl_shade_fast_kernel) only
  // fast_shade_sample's constants, folded on the host (BuildShadeArgs): [0] k T_e = [0] p / rho x D / ([1] + [2] / beta^2 + [3] D) in code
  // units of p and rho; [4] x = nu / nu_s at unit frequency = s_nu / (|b| sin) / (k T_e)^2 x [4]; [5] j at unit frequency =
  // [5] rho |b| sin / s_nu^2; [6] n_e = [6] rho; [7] nu_c / |b|
  double fast_k[8];
  double fast_angle_band;     // tolerant locate step: theta / phi closer than this to a decision are the exact kernel's (1e-12; wider under bl_debug_set_guard_band)
  unsigned long long *redo_list;       // record indices left to the exact kernel, BL_CNT_REDO entries
  unsigned long long redo_capacity;    // entries the list holds; more than that: the exact kernel shades every record
  int aux_need_coefficients;  // image_light || image_emission || image_tau || image_emission_ave || image_tau_int (:389)
  int aux_need_length;
  int aux_record_unused;      // BlAuxImages::polarized_rows_only: nobody reads the BlAuxSample records
  double cam_x[4];
  // sigma cuts in one pass (freq_split = 2; 0: none): the guard band around each threshold - a sample of the tolerant kernels whose
  // sigma lies in one of them is the exact pass's. Read wave-uniform; an empty band (lo > hi) for a switched-off threshold.
  int n_sigma_bands;
  double sigma_band_lo[BL_SHADE_MAX_SIGMA_CUTS], sigma_band_hi[BL_SHADE_MAX_SIGMA_CUTS];
  // polarized variants in one pass with an electron mix each (bl_set_polarized_variants_electrons): device [pol_variants], every variant's
  // electron constants where bl_polarized_coefficients_kernel<*, false> reads them; null: the ones above, for every variant
  const struct BlPolVariantArgs *pol_variant_args;
};

// ... and with an electron mix per variant (BlShadeArgs::pol_variant_args): the electron constants of a variant in a copy of the
// argument block, so that the formulas of bl_coefficients.inc run on a reference to it as they run on the kernel's own arguments.
// Of `args` only what those formulas read of the electrons is filled - plasma (plasma_thermal_frac, power_frac, plasma_p, power_jj,
// power_aa), power_pol, plasma_gamma_min - and `cold`, which points at the `cold` member of the same element on the device (kappa
// alone is read there); everything else is zero. A wave's variant is uniform, and so is every address read here.
struct BlPolVariantArgs {
  BlShadeArgs args;
  BlShadeCold cold;
};

// Kernel arguments: transfer kernel
struct BlTransferArgs {
  // polarized transfer only
  const BlPolSample *pol_samples;
  const double2 *pol_coeffs;
  double *pol_matrix;                      // tolerant tier: [sample row][BL_POL_MATRIX_DOUBLES] (bl_polarized.hip)
  int pol_variants, pol_variant_rows;      // polarized variants in one pass: > 0, a lane per (ray, variant) in the polarized transfer kernels, variant v's
                                           // coefficients in pol_coeffs[(sample row * pol_variants + v)][n_nu][4], its image rows from v * pol_variant_rows
  const double *camera_pos, *camera_dir;   // [n_rays_total][4] by output index: initial position, momentum
  BlSpacetime st;
  int simulation_coord, rotation_split;
  double cam_u_con[4], cam_u_cov[4], cam_vert_con_c[4];
  // ... several cameras (BlTraceArgs::cameras): the ray with output index r is camera (pixel_map ? pixel_map[r] : r) / pixels_per_camera's,
  // whose three vectors take the place of the ones above. Null: one camera.
  const BlCameraDevice *cameras;
  const int *pixel_map;
  long long pixels_per_camera;
  const double2 *transfer;
  int ja_stride;                           // records between the (j, alpha) of consecutive (sample, frequency) pairs as bl_transfer_aux_kernel reads them:
                                           // 1, or 4 in polarized runs, where `transfer` is pol_coeffs
  const double *tau_inc;                   // bl_tau_kernel: [sample row][n_nu], rows summed into image row tau_row + l
  int tau_row;
  const unsigned long long *counters;      // BL_CNT_NEXT_RAY: rays of the chunk the geodesic kernel traced (bl_rays_done)
  const int *ray_sample_num;               // [chunk_rays]: kept samples with a record (= rows) of each ray
  const int *ray_skipped;                  // [chunk_rays] or null: its samples without a record (BlTraceArgs::skip_low)
  const unsigned char *ray_flags;
  const long long *ray_out_index;
  const long long *ray_offset;             // [chunk_rays]: first sample row of each ray
  const double *frequencies;
  int n_nu, ray_max_steps, chunk_rays;
  int fallback_nan, model_type;
  int affine;                 // tolerant tier: records are (a, c) of I <- a I + c instead of (a, b) of I <- a (I + b)
  int lane_transfer;          // measurement switch (bl_stats.switches): one lane per ray where four lanes per ray apply
  const double2 *composed;    // composed transfer maps (BlShadeArgs::composed): [ray_offset + segment], ray_rows[ray] of them per ray; `transfer` by record
  const int *ray_rows;
  // Mirror pairs (BlShadeArgs::row_add; mirror_rays = 0: off): bl_transfer_kernel, bl_transfer_quad_kernel and bl_transfer_composed_kernel
  // run over 2 mirror_rays slots; slot s >= mirror_rays is the mirror pixel of traced ray s - mirror_rays: that ray's per-ray values, its
  // rows row_add further on, its outputs at mirror_out_index[s - mirror_rays] (bl_mirror_slot)
  int mirror_rays;
  long long row_add;
  const long long *mirror_out_index;
  const BlFreqInputs *freq_inputs;            // bl_transfer_freq_kernel
  int n_models;                               // ... > 0: electron models in one pass, one lane per (ray, model, frequency), image row m n_nu + l
  double model_k1[BL_TRANSFER_MAX_MODELS], model_k2[BL_TRANSFER_MAX_MODELS], model_k3;   // ... R_high g1, R_low g1 of model m; n_e / n_i g2
  int n_units;                                // ... > 0 (with n_models > 0): density units too, a lane per (ray, model, unit, frequency), row (m n_units + u) n_nu + l
  double unit_x[BL_TRANSFER_MAX_UNITS], unit_j[BL_TRANSFER_MAX_UNITS];   // ... unit u's factors on x at unit frequency and on s_j
  int n_cuts;                                 // ... > 0 (with n_models > 0): sigma cuts too, a lane per (ray, model, unit, cut, frequency), row ((m n_units + u) n_cuts + s) n_nu + l
  double sigma_max[BL_TRANSFER_MAX_CUTS];     // ... cut s leaves out the samples whose row's sigma is > sigma_max[s] (+inf: off)
  long long n_rays_total;
  double *image;              // [n_q][n_rays_total]; rows 0..n_nu-1 = I_nu
  int *out_sample_num;        // [n_rays_total] or null
  unsigned char *out_flags;   // [n_rays_total] or null
  unsigned long long *stats;  // [0] sum sample_num, [1] flagged rays, [2] max sample_num
  // auxiliary-image mode only
  BlAuxImages aux_images;
  const BlAuxSample *aux;
  const double2 *ray_constants;
  double x_unit, t_unit;
  const BlRenderDevice *render_params;   // device, or null
  double *render;                        // [n_images][3][n_rays_total], or null
  // bl_transfer_freq_kernel, electron mixes in one pass (with n_models > 0; behind everything else: no older member moves). > 0: a lane
  // per ray in a workgroup per (256 rays, mix, model, unit, cut, frequency) - what the lane needs of its channel is the workgroup's -
  // row (((e n_models + m) n_units + u) n_cuts + s) n_nu + l; the rows hold a thermal fraction of 1. Mix e's tables, of what
  // FillElectronConstants gives of it and of fast_k at the base unit with a thermal fraction of 1 (the rows' constants):
  //   mix_thermal 1 - power_frac, mix_power_frac, mix_pw_e = -(p - 1) / 2,
  //   mix_pw_j = power_frac power_jj e^2 k6 k7 / (c k5), mix_pw_a = power_frac power_aa e^2 k6 k7 / (m_e c h k5)
  // (the last three 0 where power_frac == 0: p, power_jj and power_aa are not defined there), and power_k0 = 1 / (k4 k7).
  int n_mixes;
  double mix_thermal[BL_TRANSFER_MAX_MIXES], mix_power_frac[BL_TRANSFER_MAX_MIXES], mix_pw_e[BL_TRANSFER_MAX_MIXES];
  double mix_pw_j[BL_TRANSFER_MAX_MIXES], mix_pw_a[BL_TRANSFER_MAX_MIXES];
  double power_k0;
};

#if defined(__HIPCC__) || defined(__HIP__)
// A ray's constants (BlTraceArgs::ray_constants): both in one 16-byte read where a kernel wants both, or the one it wants
__device__ __forceinline__ double2 bl_ray_constants(const double2 *rays, size_t ray) { return rays[ray]; }
__device__ __forceinline__ double bl_ray_kt(const double2 *rays, size_t ray) { return rays[ray].x; }
__device__ __forceinline__ double bl_ray_factor(const double2 *rays, size_t ray) { return rays[ray].y; }
// Rays of a chunk the geodesic kernel traced: the rays after them did not fit the record buffers and go to the next chunk
__device__ __forceinline__ int bl_rays_done(const unsigned long long *counters, int chunk_rays) {
  const unsigned long long taken = counters[BL_CNT_NEXT_RAY];
  return taken < (unsigned long long)chunk_rays ? (int)taken : chunk_rays;
}
// Mirror pairs (BlTransferArgs::mirror_rays): the traced ray a transfer slot stands for, whether as its mirror pixel, and then where
// that pixel's rows start (relative to the traced ray's) and where its outputs go
__device__ __forceinline__ bool bl_mirror_slot(const BlTransferArgs &P, int *slot) {
  const bool mirror = P.mirror_rays > 0 && *slot >= P.mirror_rays;
  if (mirror) *slot -= P.mirror_rays;
  return mirror;
}
#endif

#endif  // BLACKLIGHT_AMD_BL_DEVICE_H_
