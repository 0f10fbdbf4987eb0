// bl_render.hip - bl_render(): the reference's GeodesicIntegrator::Integrate() + RadiationIntegrator::Integrate() for one
// level of rays (src/blacklight.cpp:93-94, 203-204) as a pipeline of HIP kernels over chunks of rays, and what hangs off
// it: when checkpoints are read and written and what of a chunk is copied for them (the files themselves: bl_checkpoint.cpp),
// statistics, the reference's warning texts.
//
// One call = plan (which kernels, what a sample costs in HBM) -> scratch -> kernel arguments -> chunks -> outputs.
// A chunk is not sized on the host: every scratch array has one entry per sample record (or per kept sample), a scratch set
// holds `record_capacity` of each, and the geodesic kernel hands out rays only while the records of the rays in flight
// are sure to fit (BlTraceArgs::record_gate). What it did not get to is the next chunk. The benchmark frame - 704 samples
// per ray where ray_max_steps allows 2 000 - is one chunk this way; sized for the worst case it was two.
#include <chrono>
#include <thread>

#include "bl_checkpoint.h"

namespace {

// geodesic start / end, locate start, coefficient start, transfer start, end, counters copied to the host; [7 ... 9] the split or
// geodesic stage; [10, 11] polarized runs: frames built / transport matrices built (on the second stream)
constexpr int kEventsPerChunk = 12;

// RadiationIntegrator::Hypergeometric (simulation_coefficients.cpp:740-773): 2F1 for z < 0 through its Pfaff
// transformation, ten terms of the series
double Hypergeometric(double alpha, double beta, double gamma, double z) {
  const double a = alpha, b = gamma - beta, c = gamma;
  const double x = z / (z - 1.0);
  double result = 1.0, a_k = 1.0, b_k = 1.0, c_k = 1.0, xk = 1.0, k_factorial = 1.0;
  for (int k = 1; k <= 10; k++) {
    a_k *= a + k - 1.0;
    b_k *= b + k - 1.0;
    c_k *= c + k - 1.0;
    xk *= x;
    k_factorial *= k;
    result += a_k * b_k * xk / (c_k * k_factorial);
  }
  result *= bl_pow(1.0 - z, -alpha);
  return result;
}

void EnsureRenderResources(bl_ctx *ctx) {
  const size_t need = 2 * kEventsPerChunk + 2;
  while (ctx->events.size() < need) {
    hipEvent_t e = nullptr;
    Check(hipEventCreate(&e), "hipEventCreate");
    ctx->events.push_back(e);
  }
  if (ctx->host_counters == nullptr)
    Check(hipHostMalloc(reinterpret_cast<void **>(&ctx->host_counters), 2 * BL_CNT_TOTAL * sizeof(unsigned long long), hipHostMallocDefault),
          "hipHostMalloc");
}

struct SplitIncomplete {};   // BL_TAIL_SPLIT: the chunk ended before its last ray (RunChunks)
struct DistanceUndecided {}; // closed-form proper distance: a step's sample count was left in doubt (CollectChunk; bl_distance_closed.h)
struct ReuseImpossible {};   // scratch for a render over the resident records could not be allocated beside them (EnsureScratch)

// Which of a scratch set's optional arrays (bl_ctx::ChunkSlot) a render uses: decided in one place (UsedArrays), read by the plan, the
// kept layout, the allocation and the binding. The first two rows: arrays with a fixed number of entries per record (ForEachRecordArray).
struct ArrayUse {
  bool located = false, freq_inputs = false, transfer = false, composed = false, tau_inc = false, aux = false, slow_frac = false;
  bool pol = false, pol_matrix = false, pol_coeffs = false, pol_variant_coeffs = false, coef_inputs = false, have_flags = false, anchors = false;
  bool sample_t = false, redo = false, xcd = false, parked = false;
  unsigned int Mask() const {   // (BLACKLIGHT_AMD_DEBUG_COUNTERS: bit 0 = located ... bit 17 = parked)
    unsigned int mask = 0, bit = 0;
    for (bool flag : {located, freq_inputs, transfer, composed, tau_inc, aux, slow_frac, pol, pol_matrix, pol_coeffs, pol_variant_coeffs, coef_inputs,
                      have_flags, anchors, sample_t, redo, xcd, parked}) mask |= (flag ? 1u : 0u) << bit++;
    return mask;
  }
};

// Everything one bl_render call decides before its first kernel, and what its chunks add up to
struct RenderJob {
  bl_ctx *ctx = nullptr;
  const bl_render_desc *d = nullptr;
  // which path
  bool simulation = false, aux = false, slow = false, geo_load = false, geo_save = false, need_time = false, block_interp = false;
  bool fast = false, tolerant_polarized = false, matrix_transport = false, freq_split = false, coef_split = false;
  bool rows_only = false, fill_present = false;
  bool interleaved = false;   // sample records as one 64-byte array instead of two of 32-byte halves
  bool fast_formula = false;   // tolerant tier in formula mode: bl_shade_formula_fast_kernel
  bool tau_row = false;   // tolerant tier: an optical-depth image beside the intensities on the plain path (bl_tau_kernel)
  bool skip_shell = false;   // steps between the grid's outer edge and the camera's sphere leave no records (BlTraceArgs::skip_low)
  bool fused2 = false;  // tolerant tier, the benchmark's grids: the locate step runs inside the coefficient kernel (bl_shade_fused2_kernel, bl_shade_fused.hip)
  bool composed = false;   // ... writing one affine transfer map per ray segment instead of one per sample (BlShadeArgs::composed)
  bool exact_fused = false;   // exact tier, the same grids, plain image at one frequency: bl_shade_exact2_kernel locates its samples itself
  bool pol_fused = false;     // polarized runs over the same grids (either tier): bl_shade_polarized2_kernel locates its samples itself
  bool pol_coefficients_inside = false;   // ... and, at one frequency with thermal electrons only, evaluates their polarized coefficients itself
  bool locate_inside = false; // fused2 || exact_fused || pol_fused: no locate kernel, no located samples in HBM
  bool park = false;          // BL_TAIL_QUAD: the last rays of a chunk go to bl_geodesic_quad_kernel (BlTraceArgs::parked)
  bool split_long = false;    // BL_TAIL_SPLIT: rays predicted long on compute units of their own (bl_split_long_kernel)
  bool allow_split = true;    // false: the call is being rendered again after its split chunk closed the reservation gate early
  bool allow_reuse = true;    // false: ... after memory for a render over the resident records could not be had
  bool allow_closed = true;   // false: ... after a step the closed-form distance did not decide, or this camera is remembered for one
  bool distance_retried = false;              // ... the former: this is the second render of the call
  unsigned long long undecided_before = 0;    // ... and the steps in doubt the discarded one had counted when it was given up
  float ms_discarded = 0.0f;                  // ... and the time it took (bl_stats.ms_wall covers both)
  bool keepable = false;      // root level, geodesics integrated here: what this render leaves may serve the next (bl_set_geodesic_reuse)
  bool reuse = false;         // the resident records of an earlier render of this camera are shaded again: no geodesic stage
  bool reuse_located = false; // ... and its located samples: no locate kernel
  bool reuse_chunks = false;  // ... and they are in the kept layout: the chunks of the render that integrated them, one after another
  bool kept = false;          // integrating in the kept layout: every chunk's records side by side in a store (bl_ctx::ResidentGeodesics)
  bool kept_spilled = false;  // ... the store ran out before the last ray: the remaining chunks overwrite it from its start, nothing is kept
  bool xcd_order = false;     // trace order per XCD (BlTraceArgs::xcd_state, XcdOrderApplies)
  bool mirror = false;        // mirror pairs (MirrorPairsApply): the left half of the frame is traced, both halves are shaded from its records
  long long n_traced = 0;     // rays the geodesic stage traces and the per-ray arrays hold: n_rays, or half of them with mirror pairs
  bool local_angles = false;  // fused2 over one block: theta and phi relative to the centre of the guessed cell (BlShadeArgs::local_angles)
  bool super_tiles = false;   // ... the tile order in super-tiles (BuildTraceArgs)
  bool raster = false;        // large host outputs (many image rows): rays in pixel order, so that a chunk is a range of columns of
                              // every row and goes to the caller's buffer while the next chunk renders (DownloadChunk)
  bool chunk_downloads = false;   // ... and this call does download chunk by chunk (more than one chunk, or a first chunk that left rays)
  std::vector<std::thread> downloads;   // blocking copies into pageable memory, one host thread per chunk in flight
  std::vector<hipError_t> download_status;
  RenderJob() { download_status.reserve(4096); }
  ~RenderJob() {
    for (std::thread &t : downloads)
      if (t.joinable()) t.join();
  }
  std::vector<unsigned char> geo_key, located_key;
  int split_cus = 0;          // ... how many compute units
  double split_b_lo = 0.0, split_b_hi = 0.0;   // ... and which impact parameters
  size_t park_capacity = 0;
  int quad_grid = 0;          // waves of bl_geodesic_quad_kernel
  int n_nu = 0, n_q = 0, max_steps = 0;
  // The render's variants (ResolveVariants: mixes x models x units x sigma cuts, or the triples of a polarized run), each with n_q_model image
  // rows (n_q = variants x n_q_model); the shading stage runs once per variant over the chunk's samples (variant_passes)
  MixRange mixes;                   // ... of these mixes of the context's list (bl_render: all of it, or one run of several)
  Variants variants;
  int n_q_model = 0, variant_passes = 1;
  bool variants_one_pass = false;   // ... or all of them in one pass: one gather, one lane per (ray, model, unit, cut, frequency) in the transfer kernel
  double base_rho = 0.0, base_rat_low = 0.0, base_rat_high = 0.0;   // what BuildShadeArgs folds (PlanJob; one pass: the rows' unit and pair)
  double base_sigma_max = -1.0;     // ... and its cut_sigma_max (one pass over cuts that differ: off - the transfer kernel compares each lane's, the
                                    // polarized coefficient kernel each variant's)
  // ... or pol_one_pass, the triples': the coefficient kernel and the transport matrices once per chunk,
  // bl_polarized_coefficients_kernel and the polarized transfer kernels with a variant axis
  bool pol_one_pass = false;
  int n_cold = 1;                   // BlShadeCold blocks on the device: one per (unit, sigma cut) where the passes' cut thresholds differ (BindVariant)
  int cold_units = 1, cold_cuts = 1;   // ... n_cold = cold_units x cold_cuts, an axis of one where the passes do not differ along it
                                       // (polarized variants with cuts or mixes that differ: cold_cuts = the variants, each with its own)
  bl_electron_mix base_mix{};       // the electron mix BuildShadeArgs folds: the first variant's (the parameter block's where none is set;
                                    // one pass: what the frame-and-inputs kernel sees of it decides nothing - PlanJob; BindVariant each pass's)
  bool all_thermal = false;         // the parameter block and every variant have thermal electrons only (PlanJob): the kernels chosen for that
  // What the plan asks of the electrons, over the render's variants where bl_set_electron_mixes set a list (PlanJob): some variant has
  // a power law (the kernels that know power laws - a thermal variant goes through them with zero fractions), some has kappa
  // electrons, every one has a thermal part. Without a list: the parameter block's plasma_power_frac != 0, plasma_kappa_frac != 0 and
  // the context's thermal fraction != 0, as ever.
  bool any_power = false, any_kappa = false, every_thermal = false;
  long long n_rays = 0, level_pixels = 0;
  int n_cameras = 1;          // cameras traced as one set of rays (bl_set_cameras): level_pixels = n_cameras x the camera's pixels
  bool camera_table = false;  // ... two or more: the ray-start kernel reads each ray's frame from BlTraceArgs::cameras
  size_t redo_capacity = 0;
  // scratch
  ArrayUse use;
  KernelPlan kernels;   // which instantiation every stage launches (PlanKernels)
  uint64_t bytes_per_record = 0;
  size_t record_capacity = 0;
  long long record_gate = 0;
  // kept layout: the chunk being bound - its segment of the store, where its records start there, its capacity and gate
  // (record_capacity is then the shading arrays' capacity)
  size_t chunk_base = 0, chunk_capacity = 0;
  int chunk_segment = 0;
  long long chunk_gate = 0, kept_least = 0;
  std::vector<bl_ctx::ResidentGeodesics::Segment> segments;   // kept layout: the store (PlanKeptLayout)
  std::vector<bl_ctx::ResidentGeodesics::Chunk> kept_chunks;
  int n_slots = 1, geo_grid = 1, geo_waves_per_cu = 1;
  // outputs (device pointers: the caller's, or staging)
  double *image = nullptr, *cam_pos = nullptr, *cam_dir = nullptr, *render_out = nullptr;
  int *out_num = nullptr;
  unsigned char *out_flags = nullptr;
  const int *d_pixel_map = nullptr, *d_block_locs = nullptr;
  double snapshot_time = 0.0;
  // kernel arguments common to all chunks
  BlTraceArgs ta{};
  BlShadeArgs sa{};
  BlTransferArgs xa{};
  int locate_grid_alone = 0, locate_grid_shared = 0, shade_grid = 0;
  // a chunk in flight on scratch set k
  struct InFlight {
    bool busy = false;
    long long begin = 0;
    int rays = 0;
    long long done = -1;   // rays the chunk covered, once known
  } in_flight[2];
  // totals
  int n_chunks = 0;
  float ms_geo = 0.0f, ms_locate = 0.0f, ms_shade = 0.0f, ms_transfer = 0.0f;
  unsigned long long total_samples = 0, total_flagged = 0, total_records = 0, total_emitted = 0, total_gathers = 0, total_redo = 0, total_undefined = 0, total_parked = 0, max_num = 0;
  unsigned long long total_undecided = 0;
  unsigned long long debug_counters[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  // (BLACKLIGHT_AMD_DEBUG_COUNTERS: the tables and launch of the locate kernel - the first chunk's and the last one's, which differ
  // when chunks overlap - of the coefficient kernel and of the exact second pass)
  TableLaunch tables_locate, tables_locate_last, tables_inside, tables_redo;
  // checkpoints (bl_checkpoint.h): the two files being assembled chunk by chunk
  bool sample_save = false;     // checkpoint_sample_save: where every kept sample of the level sits on the grid
  bool no_checkpoint = true;    // !geo_load && !geo_save && !sample_save: the chunks' records and located samples never meet the host
  CheckpointSave save;
  SampleSave sampling;
};

// BLACKLIGHT_AMD_DEBUG_COUNTERS: every stage's choice as family name and template arguments, on one line
std::string DescribeKernels(const KernelPlan &k) {
  auto args = [](std::initializer_list<int> values) {
    std::string text = "<";
    for (int v : values) text += (text.size() > 1 ? "," : "") + std::to_string(v);
    return text + ">";
  };
  const KernelPlan::Shade &c = k.shade;
  std::string shade;
  switch (c.family) {
    case KernelPlan::Shade::kShade: shade = "shade" + args({c.model, c.aux, c.extended, c.sks, c.polarized, 0}); break;
    case KernelPlan::Shade::kExact: shade = "exact" + args({c.spin_zero}); break;
    case KernelPlan::Shade::kFast: shade = "fast" + args({c.spin_zero, c.mode}); break;
    case KernelPlan::Shade::kFormulaFast: shade = "formula_fast"; break;
    case KernelPlan::Shade::kFused2: shade = "fused2" + args({c.spin_zero, c.composed, c.factors, c.refined}); break;
    case KernelPlan::Shade::kExact2: shade = "exact2" + args({c.spin_zero}); break;
    case KernelPlan::Shade::kPolarized2: shade = "polarized2" + args({c.spin_zero, c.records, c.coefficients}); break;
  }
  const KernelPlan::Geodesic &g = k.geodesic;
  static const char *const integrators[] = {"DP", "RK4", "RK2"};
  static_assert(BL_INTEGRATOR_DP == 0 && BL_INTEGRATOR_RK4 == 1 && BL_INTEGRATOR_RK2 == 2, "integrator names");
  std::string text = "shade=" + shade;
  text += " redo=" + (k.redo.run ? args({k.redo.model, k.redo.extended, k.redo.sks, k.redo.spin_zero}) + "+" + std::to_string(k.redo.table_bytes) : std::string("none"));
  if (k.freq.polarized_coefficients) text += " polarized_coefficients=" + args({0, k.freq.thermal_only});
  if (k.freq.polarized_frames) text += " polarized_frames";
  if (k.freq.coefficients_freq) text += " coefficients_freq=<1>";
  static const char *const transfers[] = {"aux", "freq", "composed", "quad", "lane"};
  text += std::string(" transfer=") + transfers[k.transfer.kind] + (k.transfer.kind == KernelPlan::Transfer::kLane ? args({k.transfer.affine}) : "") + (k.transfer.tau ? "+tau" : "");
  static const char *const routes[] = {"", " polarized=tensor", " polarized=matrix", " polarized=matrices_beside"};
  text += routes[k.polarized];
  const KernelPlan::Locate &l = k.locate;
  text += " locate=" + (l.kind == KernelPlan::Locate::kNone ? std::string("none")
                        : l.kind == KernelPlan::Locate::kPlain ? "plain" + args({l.spin_zero}) : "general" + args({l.refined, l.slow, 0, l.tables_in_hbm}));
  text += " geodesic=" + (g.source == KernelPlan::Geodesic::kResident ? std::string("none")
                          : g.source == KernelPlan::Geodesic::kCheckpoint ? std::string("checkpoint")
                          : std::string("<") + integrators[g.integrator > 2 || g.integrator < 0 ? 2 : g.integrator] + "," + std::to_string(g.with_time) + "," + std::to_string(g.spin_zero) + "," + std::to_string(g.shell) + ">");
  if (k.quad.park || k.quad.split) text += std::string(k.quad.split ? " split+quad=" : " quad=") + args({k.quad.spin_zero});
  return text;
}

// ... and where each stage that finds cells read the coordinate tables, with the launch that followed (the launch wrappers' own
// values: TableLaunch). lds:<bytes of tables>x<lanes>@<workgroups>/<256-lane workgroups asked for>, hbm, located or none; the locate
// kernel's last launch behind a comma where its workgroups differ from the first's (overlapping chunks)
std::string DescribeTables(const TableLaunch &locate, const TableLaunch &locate_last, const TableLaunch &inside, const TableLaunch &redo) {
  auto shape = [](const TableLaunch &t) { return "x" + std::to_string(t.lanes) + "@" + std::to_string(t.blocks) + "/" + std::to_string(t.grid); };
  auto stage = [&](const TableLaunch &t, bool with_shape) -> std::string {
    switch (t.where) {
      case TableLaunch::kNone: return "none";
      case TableLaunch::kLocated: return "located";
      case TableLaunch::kHbm: return "hbm" + (with_shape ? shape(t) : std::string());
      case TableLaunch::kLds: return "lds:" + std::to_string(t.table_bytes) + (with_shape ? shape(t) : std::string());
    }
    return "none";
  };
  const bool differs = locate_last.blocks != locate.blocks || locate_last.grid != locate.grid;
  return "locate=" + stage(locate, true) + (differs ? ",@" + std::to_string(locate_last.blocks) + "/" + std::to_string(locate_last.grid) : std::string())
      + " fused=" + stage(inside, true) + " redo=" + stage(redo, false);
}

hipEvent_t *SlotEvents(RenderJob &job, int k) { return job.ctx->events.data() + static_cast<size_t>(k) * kEventsPerChunk; }

// A density unit (simulation_rho_cgs) and the electron model in pl.plasma_rat_low / _high into what the coefficient kernels read:
// BlPlasmaDevice's units (simulation_coefficients.cpp:237-239) and the tolerant tier's constants fast_k. BuildShadeArgs folds the
// render's, BindVariant each variant's - one arithmetic, so that a variant has the bits of a fresh render with that unit and pair.
// (thermal_frac: the thermal fraction of the electron mix the constants are for - MixThermal below; only fast_k[5] reads it)
void FoldUnits(const bl_ctx *ctx, double rho_cgs, double thermal_frac, BlPlasmaDevice &pl, double (&fast_k)[8]) {
  const bl_params &p = ctx->params;
  pl.d_unit = rho_cgs;
  pl.e_unit = pl.d_unit * kC * kC;
  pl.b_unit = blm_sqrt(4.0 * kPi * pl.e_unit);
  const bool use_p = p.plasma_use_p != 0;
  const double g0 = use_p ? 1.0 : 1.0 / (ctx->grid.meta.plasma_gamma - 1.0);
  const double g1 = use_p ? 1.0 : 1.0 / (ctx->grid.meta.plasma_gamma_i - 1.0);
  const double g2 = use_p ? 1.0 : 1.0 / (ctx->grid.meta.plasma_gamma_e - 1.0);
  const double n_e_per_rho = pl.d_unit / (p.plasma_mu * kMp * (1.0 + 1.0 / p.plasma_ne_ni));
  const double nu_c_over_b = kE * pl.b_unit / (2.0 * kPi * kMe * kC);
  fast_k[0] = (1.0 + p.plasma_ne_ni) * p.plasma_mu * kMp * pl.e_unit / pl.d_unit * g0;
  fast_k[1] = pl.plasma_rat_high * g1;
  fast_k[2] = pl.plasma_rat_low * g1;
  fast_k[3] = p.plasma_ne_ni * g2;
  fast_k[4] = (kMe * kC * kC) * (kMe * kC * kC) * 4.5 / nu_c_over_b;
  fast_k[5] = thermal_frac * n_e_per_rho * kE * kE * nu_c_over_b / kC * (kSqrt2 * kPi / 27.0);
  fast_k[6] = n_e_per_rho;
  fast_k[7] = nu_c_over_b;
}

// ... and the tolerant tier's cell cut thresholds, which it compares in code units (rho, rho for n_e, p, k T_e for Theta_e, |b| in
// code units; sigma and 1 / beta have none): scaled once here by pl's units; the guard band is relative and scales with them
// (sigma_max: the pass's cut_sigma_max - the render's, or a variant's under bl_set_sigma_cuts)
void FoldFastCuts(const bl_ctx *ctx, const BlPlasmaDevice &pl, BlShadeCold &cold, double sigma_max) {
  const bl_params &p = ctx->params;
  const double cuts[14] = {p.cut_rho_min, p.cut_rho_max, p.cut_n_e_min, p.cut_n_e_max, p.cut_p_gas_min, p.cut_p_gas_max,
                           p.cut_theta_e_min, p.cut_theta_e_max, p.cut_b_min, p.cut_b_max, p.cut_sigma_min, sigma_max,
                           p.cut_beta_inverse_min, p.cut_beta_inverse_max};
  for (int c = 0; c < 14; c++) {
    const bool active = cuts[c] >= 0.0;
    const double n_e_per_rho = pl.d_unit / (p.plasma_mu * kMp * (1.0 + 1.0 / p.plasma_ne_ni));
    const double to_code[7] = {1.0 / pl.d_unit, 1.0 / n_e_per_rho, 1.0 / pl.e_unit, kMe * kC * kC, 1.0 / pl.b_unit, 1.0, 1.0};
    const double scaled = cuts[c] * to_code[c >> 1];
    cold.fast_cut[c] = active ? scaled : 0.0;
    cold.fast_cut_lo[c] = active ? scaled * (1.0 - ctx->guard_band) : 0.0;
    cold.fast_cut_hi[c] = active ? scaled * (1.0 + ctx->guard_band) : 0.0;
  }
}

// What the coefficient formulas read of an electron mix (FillElectronConstants below): BlPlasmaDevice's power-law constants and thermal
// fraction, BlShadeArgs::power_pol and plasma_gamma_min, BlShadeCold::kappa. The parameter block's own mix and a variant's go through
// the same function - the same calls on the same operands - which is where a variant's bits of a fresh render come from.
struct ElectronConstants {
  double thermal_frac;
  double power_frac, plasma_p, power_jj, power_aa;
  double power_pol[7];
  double plasma_gamma_min;
  BlKappaDevice kappa;
};
ElectronConstants FillElectronConstants(const bl_electron_mix &mix, bool polarized);
// ... into an argument block (the render's own, a pass's, a variant's copy): everything of `pl` and `sa` a mix enters
void BindElectronConstants(const ElectronConstants &ec, bool polarized, BlPlasmaDevice &pl, BlShadeArgs &sa) {
  pl.plasma_thermal_frac = ec.thermal_frac;
  pl.power_frac = ec.power_frac;
  pl.plasma_p = ec.plasma_p;
  pl.power_jj = ec.power_jj;
  pl.power_aa = ec.power_aa;
  pl.kappa_frac_zero = ec.kappa.frac == 0.0 ? 1 : 0;
  pl.kappa_unpolarized = (ec.kappa.frac != 0.0 && !polarized) ? 1 : 0;
  if (polarized) {
    for (int c = 0; c < 7; c++) sa.power_pol[c] = ec.power_pol[c];
    sa.plasma_gamma_min = ec.plasma_gamma_min;
  }
}
bool SameMix(const bl_electron_mix &a, const bl_electron_mix &b) { return std::memcmp(&a, &b, sizeof a) == 0; }   // (as bits, like the cuts)
bool ThermalOnly(const bl_electron_mix &mix) { return mix.power_frac == 0.0 && mix.kappa_frac == 0.0; }
// The thermal fraction FoldUnits folds for a variant: its mix's where bl_set_electron_mixes set a list (formed as bl_init forms the
// parameter block's, so that a variant has the constants of a context with that mix in its block), else the context's own as ever
double MixThermal(const RenderJob &job, const bl_electron_mix &mix) { return job.variants.n_mixes > 0 ? ThermalFraction(mix) : job.ctx->plasma_thermal_frac; }

// Variant v of the render into the argument blocks: its pair where the coefficient kernels read R_low / R_high, its unit folded as
// BuildShadeArgs folds the render's (FoldUnits), the cut thresholds of its unit and its sigma cut (its BlShadeCold, uploaded by
// BuildShadeArgs; the cut's bit of the mask, which a negative value switches off), and its rows of the image. Nothing to do with one
// variant - the one BuildShadeArgs folded - or where one pass has them all: the transfer kernel has every variant's constants
// (BuildTransferArgs), the polarized coefficient kernel its table (BuildShadeArgs).
void BindVariant(RenderJob &job, int v) {
  if (job.variants.list.size() == 1 || job.variants_one_pass || job.pol_one_pass) return;
  const Variant &variant = job.variants.list[v];
  BlPlasmaDevice &pl = job.sa.plasma;
  pl.plasma_rat_low = variant.rat_low;
  pl.plasma_rat_high = variant.rat_high;
  FoldUnits(job.ctx, variant.rho, MixThermal(job, variant.mix), pl, job.sa.fast_k);
  // (a polarized variant's electron mix: the constants in the argument block here, kappa in the pass's BlShadeCold below; an
  // unpolarized variant's likewise where bl_set_electron_mixes set a list - none of those has kappa electrons)
  if (job.variants.n_pol > 0 || job.variants.n_mixes > 0) BindElectronConstants(FillElectronConstants(variant.mix, job.ctx->polarized), job.ctx->polarized, pl, job.sa);
  const VariantPlace at = job.variants.At(v);   // (polarized variants: a cut each, PlanVariantCuts)
  job.sa.cold = job.ctx->d_shade_cold.ptr + ((job.cold_units > 1 ? at.u : 0) * job.cold_cuts + (job.cold_cuts > 1 ? at.s : 0));
  pl.cut_mask = (pl.cut_mask & ~(1 << 11)) | (variant.sigma_max >= 0.0 ? 1 << 11 : 0);   // (bit 11: cut_sigma_max, FoldFastCuts' order)
  pl.any_cell_cut = pl.cut_mask != 0 ? 1 : 0;
  job.xa.image = job.image + static_cast<size_t>(v) * job.n_q_model * static_cast<size_t>(job.n_rays);
}

bool GeometricCut(const bl_params &p) {   // an optional geometric cut is set
  return p.cut_omit_near || p.cut_omit_far || p.cut_omit_in >= 0.0 || p.cut_omit_out >= 0.0 || p.cut_midplane_theta != 0.0 || p.cut_midplane_z != 0.0 || p.cut_plane;
}
bool PerSampleRows(const BlAuxImages &rows) {   // an image row made of every sample's auxiliary record
  return rows.image_time || rows.image_length || rows.image_lambda || rows.image_emission || rows.image_lambda_ave || rows.image_emission_ave || rows.image_tau_int || rows.image_crossings;
}

// Where the variants' sigma cuts are compared, once the plan knows whether the variants share a pass (PlanJob; PlanScratch again where
// it takes the polarized one pass back).
void PlanVariantCuts(RenderJob &job) {
  const Variants &vs = job.variants;
  const Variant &first = vs.list[0];
  bool cuts_differ = false;   // (as bits: -1 and -2 both switch the cut off, and are still not "the same render")
  for (const Variant &v : vs.list) cuts_differ = cuts_differ || std::memcmp(&v.sigma_max, &first.sigma_max, sizeof(double)) != 0;
  // One cut: every variant's, in the shared pass or in every pass. Passes: BindVariant each variant's.
  job.base_sigma_max = first.sigma_max;
  // One pass over two sigma cuts or more: the coefficient kernels run with the sigma upper cut off and leave every sample's sigma in
  // its row; a transfer lane compares it with its own threshold (BuildTransferArgs), and the tolerant kernels leave a sample whose
  // sigma lies in the guard band of any of the thresholds to the exact pass (BuildShadeArgs: BlShadeArgs::sigma_band_lo / _hi)
  if (job.variants_one_pass && vs.n_cuts >= 2) job.base_sigma_max = -1.0;
  // Polarized variants in one pass whose cuts differ: the frame-and-inputs kernel runs with the sigma upper cut off - every other cut
  // is decided there as ever - and bl_polarized_coefficients_kernel compares b.b / rho of the sample's row with its variant's
  // threshold (BuildShadeArgs: BlPolVariant::sigma_max). That kernel is the exact tier's in both tiers, and the row's b.b and rho are
  // the exact tier's bits in both (no polarized frame-and-inputs kernel has tolerant arithmetic): no guard band. Equal cuts stay in
  // the shared pass.
  if (job.pol_one_pass && cuts_differ) job.base_sigma_max = -1.0;
  // (the passes of two units or more compare the cut thresholds of their own unit, those of two sigma cuts or more - or of polarized
  // variants whose cuts differ - their own cut_sigma_max: one BlShadeCold per (unit, cut))
  const bool cold_per_pass = job.simulation && job.variant_passes >= 2;
  job.cold_units = cold_per_pass && vs.n_units >= 2 ? vs.n_units : 1;
  job.cold_cuts = cold_per_pass && vs.n_cuts >= 2 ? vs.n_cuts : 1;
  // (... or whose electron mixes differ: kappa lives in that block)
  bool mixes_differ = false;
  for (const Variant &v : vs.list) mixes_differ = mixes_differ || !SameMix(v.mix, first.mix);
  if (cold_per_pass && vs.n_pol >= 2 && (cuts_differ || mixes_differ)) job.cold_cuts = vs.n_pol;
  job.n_cold = job.cold_units * job.cold_cuts;
}

// ---- plan: validation of the call, the path it takes
void PlanJob(RenderJob &job) {
  bl_ctx *ctx = job.ctx;
  const bl_render_desc *d = job.d;
  const bl_params &p = ctx->params;
  job.simulation = p.model_type == BL_MODEL_SIMULATION;
  if (ctx->device == BL_DEVICE_NONE) throw Failure{BL_E_DEVICE, "Host-only context: no HIP device selected (the hot path has no CPU fallback)."};
  if (job.simulation && !ctx->grid.have) throw Failure{BL_E_STATE, "bl_render called before bl_set_grid."};
  if (d->n_rays <= 0 || (d->image == nullptr && ctx->image_num_quantities > 0))
    throw Failure{BL_E_ARG, "bl_render needs n_rays > 0 and an image buffer."};
  if (ctx->render_num_images > 0 && d->render == nullptr) throw Failure{BL_E_ARG, "bl_render needs a render buffer when render_num_images > 0."};
  if (d->n_rays > 0x7fffffffll) throw Failure{BL_E_ARG, "Too many rays in one bl_render call."};
  if (d->level < 0 || d->level > p.adaptive_max_level) throw Failure{BL_E_ARG, "Adaptive level out of range."};
  if (d->level > 0 && (d->block_locs == nullptr || d->n_blocks <= 0)) throw Failure{BL_E_ARG, "Refined level needs block_locs."};
  job.variants = ResolveVariants(ctx, job.mixes);
  const Variants &vs = job.variants;
  job.any_power = p.plasma_power_frac != 0.0, job.any_kappa = p.plasma_kappa_frac != 0.0, job.every_thermal = ctx->plasma_thermal_frac != 0.0;
  if (vs.n_mixes > 0) {
    job.any_power = job.any_kappa = false, job.every_thermal = true;
    for (const Variant &v : vs.list) {
      job.any_power = job.any_power || v.mix.power_frac != 0.0;
      job.any_kappa = job.any_kappa || v.mix.kappa_frac != 0.0;
      job.every_thermal = job.every_thermal && ThermalFraction(v.mix) != 0.0;
    }
  }
  if (job.simulation && job.any_kappa && !ctx->polarized && vs.n_mixes == 0) {
    if (!(ctx->undefined_policy & BL_UNDEFINED_KAPPA))
      throw Failure{BL_E_UNSUPPORTED, "Kappa-distribution electrons (plasma_kappa_frac != 0) in an unpolarized run: the reference's absorptivity reads "
                                      "kappa_aa_high_i, which it only initialises for polarized runs - no defined result to reproduce. "
                                      "bl_set_undefined_policy(BL_UNDEFINED_KAPPA) uses the polarized definition instead."};
    if (!ctx->kappa_warned)
      Warn(ctx, "Unpolarized kappa-distribution electrons: kappa_aa_high_i, which the reference leaves uninitialised here, is (3 / kappa)^4.75 + 0.6.");
    ctx->kappa_warned = true;
  }
  if (const char *why = ElectronMixesRefusal(ctx, vs.n_mixes, ctx->mixes.data() + job.mixes.begin)) throw Failure{BL_E_UNSUPPORTED, why};
  if (const char *why = ElectronModelsRefusal(ctx, vs.n_models)) throw Failure{BL_E_UNSUPPORTED, why};
  if (const char *why = DensityUnitsRefusal(ctx, vs.n_units)) throw Failure{BL_E_UNSUPPORTED, why};
  if (const char *why = PolarizedVariantsRefusal(ctx, vs.n_pol)) throw Failure{BL_E_UNSUPPORTED, why};
  if (const char *why = SigmaCutsRefusal(ctx, vs.n_cuts)) throw Failure{BL_E_UNSUPPORTED, why};
  if (const char *why = CamerasRefusal(ctx, static_cast<int>(ctx->cameras.size()))) throw Failure{BL_E_UNSUPPORTED, why};
  if (const char *why = FrequenciesRefusal(ctx, ctx->frequencies_set)) throw Failure{BL_E_UNSUPPORTED, why};
  job.n_cameras = std::max<int>(1, static_cast<int>(ctx->cameras.size()));
  job.camera_table = job.n_cameras >= 2;
  // (two cameras or more render the root level only: adaptive_max_level is 0 with them, so the level check above has seen to it)
  // What BuildShadeArgs folds before a variant is bound: the first variant - one variant is a fresh render with it in the parameter
  // block, and the first triple's cut decisions are every triple's in one pass. But several (model, unit) variants keep the parameter
  // block's pair, and two or more units its unit too (so base_rho is the one set unit, the first triple's, else the parameter block's):
  // the one-pass rows are built with them - the exact second pass divides the pair out again, the transfer kernel rescales by unit_x and
  // unit_j - so another base changes roundings, and the unit the bytes of the BlShadeCold block that shade_cold_host is compared with.
  const Variant &first = vs.list[0];
  job.base_rho = first.rho, job.base_rat_low = first.rat_low, job.base_rat_high = first.rat_high;
  if (vs.n_pol == 0 && vs.list.size() >= 2) job.base_rat_low = p.plasma_rat_low, job.base_rat_high = p.plasma_rat_high;
  if (vs.n_units >= 2) job.base_rho = p.simulation_rho_cgs;
  // (the electron mix: the first variant's - the parameter block's own unless bl_set_polarized_variants_electrons set one)
  job.base_mix = first.mix;
  job.all_thermal = p.plasma_power_frac == 0.0 && p.plasma_kappa_frac == 0.0;
  for (const Variant &v : vs.list) job.all_thermal = job.all_thermal && ThermalOnly(v.mix);
  // (the context's frequencies, not the block's count: bl_set_frequencies' list where one is set, else what bl_init built of the block -
  // or a loaded checkpoint's, of the block's length. Everything below that reads n_nu - the d_freq upload, the LDS table's bound, the
  // freq_split and coef_split switches at four, the rows ctx->aux_images offsets - follows the list's length; its values enter no key.)
  job.n_nu = static_cast<int>(ctx->frequencies.size());
  job.n_q_model = ctx->image_num_quantities;
  job.variant_passes = static_cast<int>(vs.list.size());
  job.n_q = job.n_q_model * job.variant_passes;
  job.max_steps = p.ray_max_steps;
  job.n_rays = d->n_rays;
  job.aux = ctx->aux_images.any != 0;
  job.slow = job.simulation && p.slow_light_on;
  if (job.slow) {
    if (static_cast<int>(ctx->slow_slices.size()) != p.slow_chunk_size) throw Failure{BL_E_STATE, "Slow light: time slices not set."};
    for (const bl_ctx::SlowSlice &slice : ctx->slow_slices)
      if (!slice.set) throw Failure{BL_E_STATE, "Slow light: time slices not set."};
  }
  // geodesic checkpoints (root level only, like the reference's): load replaces the geodesic kernel by the file's
  // samples, save writes what the geodesic kernel produced in the reference's layout
  job.geo_load = p.checkpoint_geodesic_load && d->level == 0;
  job.geo_save = p.checkpoint_geodesic_save && d->level == 0;
  if (job.geo_load && !ctx->checkpoint) LoadGeodesicCheckpoint(ctx);
  job.need_time = (job.aux && ctx->aux_images.image_time) || job.slow || job.geo_load || job.geo_save;

  job.level_pixels = static_cast<long long>(p.camera_resolution) * p.camera_resolution;
  if (d->level > 0) job.level_pixels = static_cast<long long>(d->n_blocks) * p.adaptive_block_size * p.adaptive_block_size;
  else job.level_pixels *= job.n_cameras;   // (virtual pixels v = c res^2 + m)
  if (!ctx->cameras.empty() && d->pixel_map != nullptr)   // (a virtual pixel beyond the last camera would index past the camera table)
    for (long long ray = 0; ray < job.n_rays; ray++)
      if (d->pixel_map[ray] < 0 || d->pixel_map[ray] >= job.level_pixels)
        throw Failure{BL_E_ARG, "pixel_map names a pixel outside 0 .. " + std::to_string(job.level_pixels - 1) + " (cameras x camera_resolution^2)."};
  if (d->pixel_map == nullptr && job.n_rays > job.level_pixels) throw Failure{BL_E_ARG, "n_rays exceeds the pixels of this level."};
  if (job.geo_save && (d->pixel_map != nullptr || job.n_rays != job.level_pixels))
    throw Failure{BL_E_ARG, "checkpoint_geodesic_save needs the whole root camera in one bl_render call."};
  if (job.geo_load && d->pixel_map != nullptr) {   // a rank's tiles can be served from the one file; the map must stay inside it
    const size_t n_pix = ctx->checkpoint->sample_num.size();
    for (long long ray = 0; ray < job.n_rays; ray++)
      if (d->pixel_map[ray] < 0 || static_cast<size_t>(d->pixel_map[ray]) >= n_pix)
        throw Failure{BL_E_ARG, "pixel_map names a pixel the geodesic checkpoint does not hold."};
  }
  job.block_interp = job.simulation && ctx->grid.dev.block_interp != 0;
  // SaveSampling() (sample_checkpoint.cpp:22-46): with the first image of the root level only (radiation_integrator.cpp:693-704)
  job.sample_save = job.simulation && p.checkpoint_sample_save && d->level == 0 && !ctx->sample_checkpoint_saved;
  if (job.sample_save && (d->pixel_map != nullptr || job.n_rays != job.level_pixels))
    throw Failure{BL_E_ARG, "checkpoint_sample_save needs the whole root camera in one bl_render call."};
  job.no_checkpoint = !job.geo_load && !job.geo_save && !job.sample_save;
  // Tolerant tier: plain unpolarized images of a simulation with thermal (and power-law) electrons in a curved
  // spacetime have the fast coefficient kernel; every other configuration is rendered in exact arithmetic whatever
  // bl_set_arithmetic() asked for (bl_stats.arithmetic says which tier ran)
  // (an optical-depth image as the only auxiliary row is the plain path plus one sum per ray: not an auxiliary run below)
  const BlAuxImages &rows = ctx->aux_images;
  const bool tau_only = job.aux && !ctx->polarized && p.image_light && rows.image_tau && ctx->render_num_images == 0 && !job.geo_load && !job.geo_save
      && !PerSampleRows(rows);
  // (inter-block interpolation and slow light: bl_shade_fast_kernel behind their locate kernels, primitives by the exact tier's sampling)
  job.fast = ctx->arithmetic == BL_ARITH_TOLERANT && job.simulation && (!job.aux || tau_only) && !ctx->polarized && !(job.slow && job.block_interp)
      && !job.any_kappa && p.plasma_model != BL_PLASMA_CODE_KAPPA
      && !p.ray_flat && job.every_thermal
      && job.n_nu <= 1024;   // (its LDS table holds five numbers per frequency)
  if (job.fast && job.aux) {
    job.tau_row = true;
    job.aux = false;
  }
  // ... formula mode has a fast kernel of its own (plain images, no optional geometric cut)
  job.fast_formula = ctx->arithmetic == BL_ARITH_TOLERANT && !job.simulation && !job.aux
      && !GeometricCut(p);
  // ... and the per-frequency coefficient kernel of polarized runs (frame, transport and coupling stay exact)
  job.tolerant_polarized = ctx->arithmetic == BL_ARITH_TOLERANT && ctx->polarized;
  // ... and transport matrices (bl_transport_matrix_kernel) instead of the ray-sequential tensor transport, in curved spacetimes
  job.matrix_transport = job.tolerant_polarized && !p.ray_flat && !(ctx->switches & BL_SWITCH_TENSOR_TRANSPORT);
  // Several frequencies in the fast path: per-sample factors (BlFreqInputs) instead of per-frequency transfer records,
  // evaluated by bl_transfer_freq_kernel with one lane per ray and frequency
  job.freq_split = job.fast && job.n_nu >= 4 && !job.any_power && !job.tau_row;   // (the factors are the thermal formulas')
  // Electron models and density units in one pass: where the factors would apply, the image holds intensities only and no Theta_e cut
  // decides differently between models - nor, with two units or more, a rho, n_e, p_gas or B cut between units - a sample's row holds
  // what no model enters (BlFreqInputs, built with base_rho) and the transfer kernel forms each model's 1 / (k T_e) and scales the row
  // to each unit (everything else: one shading pass per variant over the shared samples, LaunchShadingStage)
  // (two electron mixes or more: the rows fold a thermal fraction of 1 and every transfer workgroup applies its own mix, power law
  // included - every mix has a thermal part, or job.fast is off. One mix is a context with it in its block. A run of a list rendered as
  // several - bl_render: it holds a mix without a thermal part - runs a pass per variant, whatever its own mixes could share.)
  const bool mixes_one_pass = vs.n_mixes >= 2;
  job.variants_one_pass = job.variant_passes >= 2 && job.fast && !job.mixes.pass_per_variant && (mixes_one_pass || (!job.any_power && vs.n_mixes < 2)) && !job.tau_row && !job.aux && ctx->render_num_images == 0
      && !ThetaECut(p) && !(vs.n_units >= 2 && UnitCut(p))
      && !((vs.n_units >= 2 || vs.n_cuts >= 2 || mixes_one_pass) && job.n_rays * job.n_nu * job.variant_passes >= (1ll << 31));   // (the transfer kernel's lanes of a chunk fit one grid)
  if (job.variants_one_pass) {
    job.freq_split = true;
    job.variant_passes = 1;
    // (mixes in one pass: no power law reaches the coefficient kernels, which write the mix-free row - the thermal kernels, the fused one
    // included, with a mix of thermal electrons alone, fraction 1, in their argument block)
    if (mixes_one_pass) {
      job.any_power = false;
      job.base_mix = bl_electron_mix{};
    }
  }
  // Plain images of a spherical Kerr-Schild simulation with fallback values beyond the grid: nothing is recorded of the steps that
  // lie in the empty shell between the grid's outer edge and the camera's sphere (both tiers; the samples count as ever)
  job.skip_shell = job.simulation && !job.aux && !ctx->polarized && !job.slow && job.no_checkpoint
      && !job.need_time && p.simulation_coord == BL_COORD_SKS && !ctx->grid.dev.fmks && !p.fallback_nan && ctx->grid.tables.outer_x1 > 0.0
      && p.ray_integrator == BL_INTEGRATOR_DP   // (the fixed-step steppers have no instantiation for it: bl_launch_geodesic)
      && ctx->grid.tables.outer_x1 < p.camera_r && !(ctx->switches & BL_SWITCH_RECORD_EVERY_STEP);
  // The fast path over one grid (or equal blocks merged into one) with its coordinate tables in LDS, trilinear sampling and no
  // optional geometric cut locates its samples inside the coefficient kernel: no located samples in HBM at all
  // (one frequency - with four or more it ends at the sample's factors, which no frequency enters: BlFreqInputs - over a single block
  // with evenly spaced faces, bl_fused2_applicable; everything else goes through a locate kernel and bl_shade_fast_kernel)
  // (a mesh with refinement whose blocks and rows are evenly spaced has an instantiation of that kernel too - one frequency, composed
  // maps: bl_fused2_refined_applicable and the conditions of job.composed below)
  const bool records_every_sample = ctx->reproducible || (ctx->switches & BL_SWITCH_SAMPLE_RECORDS) != 0;
  const bool fused2_grid = ctx->grid.dev.n_blocks == 0
      ? ctx->grid.tables.lds_table_bytes > 0 && bl_fused2_applicable(&ctx->grid.dev, job.freq_split ? 1 : job.n_nu, job.n_rays) != 0
      : !job.freq_split && !records_every_sample && !job.skip_shell && bl_fused2_refined_applicable(&ctx->grid.dev, job.n_nu, job.n_rays) != 0;
  // What the three kernels with the locate step inside ask for alike: a simulation on a spherical Kerr-Schild grid (their locate step is
  // the spherical one: Cartesian grids go through the locate kernel, FMKS grids too), trilinear sampling, one time slice, no optional
  // geometric cut, no geodesic checkpoint loaded or saved (interleaved records whose momenta are not renormalised yet), no sample
  // checkpoint (it is made of the located samples), neither measurement switch
  const bool locate_inside_possible = job.simulation && !job.slow && !ctx->grid.dev.fmks && p.simulation_interp && p.simulation_coord == BL_COORD_SKS
      && !GeometricCut(p) && job.no_checkpoint && !(ctx->switches & (BL_SWITCH_NO_FUSED_LOCATE | BL_SWITCH_SPLIT_RECORDS));
  // (its own: the tolerant tier's scope - only this one reads job.fast, which leaves it plain images and so no sample times - without
  // the optical-depth row and power-law electrons; it alone takes inter-block interpolation, which its grid predicate decides)
  job.fused2 = locate_inside_possible && job.fast && !job.tau_row && fused2_grid && !job.any_power;
  // ... with theta and phi relative to the centre of the guessed cell where the series behind them reaches every point of every angular
  // cell (bl_local_angles.h: 1 / 16 rad from the centre; one block - the mesh with refinement keeps acos / atan2)
  job.local_angles = job.fused2 && ctx->grid.dev.n_blocks == 0 && ctx->grid.dev.angle_trig[0] != nullptr && ctx->grid.dev.angle_reach <= kLocalAngleReach && !(ctx->switches & BL_SWITCH_GLOBAL_ANGLES);
  // The exact tier's plain image at one frequency over such a grid: the locate step inside bl_shade_exact2_kernel (bit-identical
  // to bl_locate_plain_kernel + bl_shade_exact_kernel, whose conditions these are: job.fast's electrons, restated because it is off)
  job.exact_fused = locate_inside_possible && !job.fast && !job.aux && !ctx->polarized && !job.block_interp && job.n_nu == 1
      && !job.any_kappa && !job.any_power && p.plasma_model != BL_PLASMA_CODE_KAPPA && !p.ray_flat
      && job.every_thermal
      && (ctx->grid.dev.n_blocks == 0 ? bl_fused2_applicable(&ctx->grid.dev, job.n_nu, job.n_rays) != 0 : bl_polarized2_refined_applicable(&ctx->grid.dev, job.n_rays) != 0);
  // Polarized runs over such a grid: the frame-and-inputs kernel with the locate step inside (bit-identical to bl_locate_plain_kernel +
  // bl_shade_kernel<polarized>, whose conditions these are; electron entropy from the grid is a ninth value it does not gather)
  // (... or a mesh with refinement whose tables the tolerant tier's fused kernel takes: the polarized kernel's locate step knows them too)
  // (only this one tests need_time: its runs may carry auxiliary rows - image_time - which the other two exclude altogether)
  job.pol_fused = locate_inside_possible && ctx->polarized && !job.block_interp && p.plasma_model != BL_PLASMA_CODE_KAPPA && !p.ray_flat && !job.need_time
      && (ctx->grid.dev.n_blocks == 0 ? bl_fused2_applicable(&ctx->grid.dev, 1, job.n_rays) != 0 : bl_polarized2_refined_applicable(&ctx->grid.dev, job.n_rays) != 0);
  job.interleaved = (job.fused2 || job.exact_fused || job.pol_fused || !job.simulation) && job.no_checkpoint && !(ctx->switches & BL_SWITCH_SPLIT_RECORDS);
  job.locate_inside = job.fused2 || job.exact_fused || job.pol_fused;
  // The benchmark's kernel also composes the affine maps of a ray's neighbouring samples before they leave it (the geodesic kernel
  // numbers the segments: BlTraceArgs::segment_rows)
  job.composed = job.fused2 && !job.freq_split && !records_every_sample;
  // (the geodesic kernel's instantiation that skips the shell has no register to number segments with: per-sample records there)
  if (job.skip_shell) job.composed = false;
  // The last rays of a chunk finished with a ray per quad of lanes (Dormand-Prince stepper without sample times; the instantiation
  // that skips the shell has no register for it): pays on frames whose last rays run for thousands of steps, costs the others
  const bool parkable = p.ray_integrator == BL_INTEGRATOR_DP && !job.need_time && !job.skip_shell && !job.geo_load;
  // (bl_set_tail_policy; BL_TAIL_AUTO: formula-mode frames - rays that circle for thousands of steps while the SIMDs around them idle,
  // configuration 2: 77 -> 67 ms - and not over a simulation grid, where the benchmark frame loses 6 ms to it. Bit-identical either way.)
  const bool quad_wanted = ctx->tail_policy == BL_TAIL_QUAD || (ctx->tail_policy == BL_TAIL_AUTO && !job.simulation && job.n_rays >= 64 * 64);
  job.park = parkable && (quad_wanted || (ctx->switches & BL_SWITCH_QUAD_EVERY_RAY) != 0);
  // BL_TAIL_SPLIT: the rays of a plane camera's root level whose impact parameter lies in a band around the photon ring's, stepped by
  // bl_geodesic_quad_kernel on compute units the other stepper is kept off
  const bool split_forced = ctx->tail_policy == BL_TAIL_SPLIT;
  // (BL_TAIL_AUTO: where the geodesic stage waits for single rays - up to eight rays per lane of a grid of one wave per SIMD: a share
  // of a frame tiled over two or more GPUs, measured 1.13 / 1.09 / 1.02 x at an eighth / a quarter / a half of the benchmark frame, 1.00 for
  // the whole - and the critical curve is the circle b = 3 sqrt(3) M: no spin)
  const bool split_auto = ctx->tail_policy == BL_TAIL_AUTO && !ctx->split_unavailable && ctx->st.bh_a == 0.0 && !p.ray_flat
      && job.n_rays >= 32768 && job.n_rays <= 8ll * 256 * ctx->num_cus;
  job.split_long = job.allow_split && parkable && !job.park && (split_forced || split_auto) && p.camera_type == BL_CAMERA_PLANE && d->level == 0
      && !job.camera_table;   // (several cameras: BL_TAIL_SPLIT resolves to BL_TAIL_WIDE - the split kernel knows one camera's pixels)
  // ... and in the exact coefficient kernel (plain images): the frequency loop as lanes of bl_coefficients_freq_kernel
  job.coef_split = !job.fast && job.simulation && !job.aux && !ctx->polarized && job.n_nu >= 4;
  // (polarized runs list the samples without coefficients there - cut samples, cut cells - which are many more)
  job.redo_capacity = ctx->polarized ? (1u << 24) : (1u << 20);
  // (inter-block interpolation with the locate step inside the coefficient kernel: the samples with an anchor beyond their own block -
  // up to a quarter of them, bl_fused2_refined_applicable - are the exact pass's; room for an eighth of the samples the rays may have)
  if (job.fused2 && job.block_interp)
    job.redo_capacity = static_cast<size_t>(std::min<long long>(1ll << 29, std::max<long long>(1ll << 20, job.n_rays * static_cast<long long>(p.ray_max_steps) / 8)));
  // polarized run with no per-sample row but tau and no rendering: tau is integrated by the polarized transfer kernel
  bool fill_present = false;
  for (int n_i = 0; n_i < ctx->render_num_images; n_i++)
    for (int n_f = 0; n_f < p.render_num_features[n_i]; n_f++)
      if (p.render_type[n_i][n_f] == BL_RENDER_FILL) fill_present = true;
  job.fill_present = fill_present;
  job.rows_only = ctx->polarized && ctx->render_num_images == 0 && !fill_present && !PerSampleRows(rows);
  // configuration 4's case: no BlCoefInputs through HBM, no bl_polarized_coefficients_kernel launch (bl_shade_fused.hip: kCoefficients)
  // (thermal electrons: the mix the single pass renders with - n = 1 through bl_set_polarized_variants_electrons is that tuple in the
  // block - and with a pass per variant every variant's, the kernel being chosen once)
  bool variants_thermal = true;
  for (const Variant &v : vs.list) variants_thermal = variants_thermal && ThermalOnly(v.mix);
  job.pol_coefficients_inside = job.pol_fused && job.n_nu == 1 && job.rows_only && variants_thermal && ctx->st.bh_a == 0.0;
  // Polarized variants in one pass: where no decision differs between them - a rho, n_e, p_gas or B cut only with one unit, a Theta_e
  // cut only with one unit and one pair (the units reach Theta_e through roundings), Stokes rows and the optical-depth row only (the
  // rows the polarized transfer kernels write), Theta_e from R_high / R_low (code_kappa: passes) - and the lanes of a chunk fit one grid
  if (vs.n_pol >= 2) {
    bool same_units = true, same_pairs = true, same_mixes = true;
    for (const Variant &v : vs.list) {
      same_units = same_units && v.rho == first.rho;
      same_pairs = same_pairs && v.rat_low == first.rat_low && v.rat_high == first.rat_high;
      same_mixes = same_mixes && SameMix(v.mix, first.mix);
    }
    // (an electron mix enters no decision but one: Theta_e exists only where the thermal fraction is non-zero, and a Theta_e cut
    // compares it - with such a cut, one pass asks for equal mixes as well)
    job.pol_one_pass = job.rows_only && p.plasma_model != BL_PLASMA_CODE_KAPPA && !(UnitCut(p) && !same_units)
        && !(ThetaECut(p) && !(same_units && same_pairs && same_mixes)) && job.n_rays * vs.n_pol < (1ll << 31);
    if (job.pol_one_pass) {
      job.variant_passes = 1;
      job.pol_coefficients_inside = false;   // (the samples go through the 64-byte row, which is where the variants part)
    }
  }
  PlanVariantCuts(job);
  // Host outputs of a quarter of a GiB and more in eight rows or more (configuration 5: 64 frequencies): the rays are traced in pixel
  // order - not the 8 x 8 tiles, centre first, that make chunks drain faster - so that what a chunk finishes is a range of columns,
  // downloaded while the next chunk renders (the image rows of a 4096^2 x 64 frame are 8.6 GB: 0.7 s of PCIe that used to follow the
  // last kernel)
  // (one variant's rows decide: the trace order is part of the resident geodesics' key, which the models and units must not change)
  job.raster = !d->outputs_on_device && d->level == 0 && d->pixel_map == nullptr && job.n_q_model >= 8
      && static_cast<uint64_t>(job.n_q_model) * static_cast<uint64_t>(job.n_rays) * sizeof(double) >= (256ull << 20) && job.no_checkpoint;
  job.n_traced = job.n_rays;   // (mirror pairs: halved once they are decided, bl_render)
}

// ---- geodesics once per series (bl_set_geodesic_reuse; reference: blacklight.cpp:93-94 against its run loop :178-250, and the
// `first_time` sampling of radiation_integrator.cpp:693-704)
struct KeyWriter {
  std::vector<unsigned char> *out;
  template <typename T>
  void Put(const T &value) {
    const unsigned char *p = reinterpret_cast<const unsigned char *>(&value);
    out->insert(out->end(), p, p + sizeof(T));
  }
};

unsigned long long HashWords(const int32_t *data, size_t count) {
  unsigned long long h = 1469598103934665603ull;
  size_t at = 0;
  for (; at + 2 <= count; at += 2) {
    unsigned long long word;
    std::memcpy(&word, data + at, 8);
    h = (h ^ word) * 1099511628211ull;
    h ^= h >> 29;
  }
  if (at < count) h = (h ^ static_cast<unsigned int>(data[at])) * 1099511628211ull;
  return h;
}

// Everything the sample records of a root-level render and their layout depend on, value by value (no struct padding): two
// renders with equal keys would write the same records. The located samples depend on the grid's geometry and the locate
// step's settings besides.
void BuildReuseKeys(RenderJob &job) {
  bl_ctx *ctx = job.ctx;
  const bl_render_desc *d = job.d;
  const bl_params &p = ctx->params;
  job.geo_key.clear();
  KeyWriter key{&job.geo_key};
  key.Put(ctx->st.bh_m); key.Put(ctx->st.bh_a); key.Put(ctx->st.ray_flat);
  const bl_camera_frame &f = ctx->frame;
  for (const double (*v)[4] : {&f.cam_x, &f.u_con, &f.u_cov, &f.norm_con, &f.norm_con_c, &f.hor_con_c, &f.vert_con_c})
    for (int mu = 0; mu < 4; mu++) key.Put((*v)[mu]);
  key.Put(f.r_horizon); key.Put(f.r_terminate);
  key.Put(job.n_cameras);
  if (job.camera_table)   // (the list is part of what "the same camera" means; a list of one is `frame` above)
    for (const bl_ctx::Camera &camera : ctx->cameras)
      for (const double (*v)[4] : {&camera.frame.cam_x, &camera.frame.u_con, &camera.frame.u_cov, &camera.frame.norm_con, &camera.frame.norm_con_c,
                                   &camera.frame.hor_con_c, &camera.frame.vert_con_c})
        for (int mu = 0; mu < 4; mu++) key.Put((*v)[mu]);
  key.Put(p.camera_type); key.Put(p.camera_width); key.Put(p.camera_r); key.Put(p.camera_resolution); key.Put(p.image_normalization);
  key.Put(p.ray_integrator); key.Put(p.ray_step); key.Put(p.ray_tol_abs); key.Put(p.ray_tol_rel); key.Put(p.ray_max_steps); key.Put(p.ray_max_retries);
  key.Put(d->level); key.Put(d->n_rays);
  const unsigned long long map_hash = d->pixel_map != nullptr ? HashWords(d->pixel_map, static_cast<size_t>(d->n_rays)) : 0ull;
  key.Put(d->pixel_map != nullptr ? 1 : 0); key.Put(map_hash);
  // the layout of the records and what the stepper leaves out of them
  key.Put(job.need_time ? 1 : 0); key.Put(job.interleaved ? 1 : 0); key.Put(job.composed ? 1 : 0); key.Put(job.skip_shell ? 1 : 0); key.Put(job.raster ? 1 : 0);
  key.Put(job.skip_shell ? ctx->grid.tables.outer_x1 : 0.0);
  // who steps which rays (the records' order; bl_stats says it)
  key.Put(ctx->tail_policy); key.Put(ctx->switches); key.Put(ctx->overlap_chunks); key.Put(ctx->num_cus);
  key.Put(ctx->scratch_limit);   // (a caller that lowers the cap wants the memory back: the records are integrated again, in as many chunks as it takes)
  job.located_key = job.geo_key;
  KeyWriter located{&job.located_key};
  located.Put(ctx->grid.tables.geometry); located.Put(ctx->undefined_policy); located.Put(job.fast ? 1 : 0); located.Put(job.block_interp ? 1 : 0);
  located.Put(ctx->guard_band); located.Put(p.simulation_interp); located.Put(p.simulation_coord);
}

// The root level's buffers and the other levels' change places (bl_ctx::ResidentGeodesics)
// (kept layout: the whole of scratch set 0 - its shading arrays hold part of the store)
void SwapResidentBuffers(bl_ctx *ctx) {
  bl_ctx::ResidentGeodesics::Buffers &st = ctx->resident.store;
  bl_ctx::ChunkSlot &sl = ctx->slot[0];
  if (!ctx->resident.chunks.empty()) {
    std::swap(st.slot, sl);
  } else {
    std::swap(st.records_hot, sl.d_records_hot);
    std::swap(st.records_cold, sl.d_records_cold);
    std::swap(st.sample_t, sl.d_sample_t);
    std::swap(st.located, sl.d_located);
    std::swap(st.located_tag, sl.d_located_tag);
    std::swap(st.anchors, sl.d_anchors);
  }
  std::swap(st.rays, ctx->rays);
  ctx->resident.parked = !ctx->resident.parked;
}

}  // namespace

void blhost::DropResident(bl_ctx *ctx) {
  bl_ctx::ResidentGeodesics &res = ctx->resident;
  if (res.valid && res.parked) {   // the buffers set aside are the root level's: back to the device
    res.store.Free();
    res.parked = false;
  }
  // (kept layout in place: the store is scratch set 0's own memory, which is scratch again)
  res.valid = res.located_valid = false;
  res.chunks.clear();
  res.segments.clear();
}

namespace {

// Which way this render goes: over the resident records (a root-level render of the same camera left them), or integrating its
// own - in scratch set 0 as ever, with the resident records of the root level, if any, set aside first
void DecideReuse(RenderJob &job) {
  bl_ctx *ctx = job.ctx;
  bl_ctx::ResidentGeodesics &res = ctx->resident;
  job.keepable = ctx->geodesic_reuse != 0 && job.d->level == 0 && !job.geo_load;
  if (job.keepable) BuildReuseKeys(job);
  // (resident records of mirror pairs serve a render that could be paired itself - MirrorPairsApply has said so in job.mirror; unpaired
  // records serve any render. Either way the render goes the way the records were traced.)
  // (the kept layout holds part of its store in the tails of the per-frequency shading arrays: a list of another length -
  // bl_set_frequencies - would shade into it, so such a render integrates again; in one chunk's layout the arrays simply grow)
  job.reuse = job.keepable && job.allow_reuse && res.valid && res.key == job.geo_key && (!res.mirror || job.mirror)
      && (res.chunks.empty() || res.kept_n_nu == job.n_nu);
  if (job.reuse) {
    job.mirror = res.mirror;
    if (res.parked) SwapResidentBuffers(ctx);
    job.reuse_chunks = !res.chunks.empty();
    // (kept layout: the located samples lived in one chunk's arrays and are gone)
    job.reuse_located = !job.reuse_chunks && job.simulation && !job.locate_inside && !job.slow && res.located_valid && res.located_key == job.located_key;
    job.geo_save = false;   // (the render that integrated them wrote the file: geodesic_checkpoint.cpp is called once per run of the program)
    job.no_checkpoint = !job.geo_load && !job.sample_save;
  } else if (res.valid) {
    if (job.keepable) DropResident(ctx);            // another camera: this render's records take their place
    else if (!res.parked) SwapResidentBuffers(ctx);   // another level: it works in buffers of its own
  }
  // The render after one of this camera that took several chunks and kept nothing: integrated in the kept layout (PlanScratch decides
  // whether it fits). Not with two scratch sets, nor where a checkpoint is written from the chunks' records.
  job.kept = job.keepable && !job.reuse && res.pending && res.pending_key == job.geo_key && ctx->overlap_chunks == 0 && !job.geo_save && !job.sample_save;
  if (job.kept) job.mirror = false;   // (more than one chunk: every ray is traced)
  job.n_traced = job.mirror ? job.n_rays / 2 : job.n_rays;
}

// What the shading stage adds to a chunk's counters: cleared, so that a render over the kept records counts it again
void ClearShadingCounters(unsigned long long *counters) {
  for (int c : {BL_CNT_GATHERS, BL_CNT_UNDEFINED, BL_CNT_INTERP_FAILED, BL_CNT_REDO}) counters[c] = 0ull;
  for (int c = BL_CNT_COUNT; c < BL_CNT_COUNT + 12; c++) counters[c] = 0ull;   // the transfer kernel's statistics, debug counters
}

// After a render that integrated the root level's geodesics in one chunk, or in the kept layout: what it left is the resident set.
// After one of several chunks that kept nothing: the pending entry that has the next render of this camera integrate in the kept layout.
void KeepResident(RenderJob &job) {
  bl_ctx *ctx = job.ctx;
  bl_ctx::ResidentGeodesics &res = ctx->resident;
  const bool located_here = job.simulation && !job.locate_inside && !job.slow;
  const unsigned long long *hc = ctx->host_counters;   // scratch set 0's, as CollectChunk read them
  if (ctx->debug_counters)
    std::fprintf(stderr, "scratch plan: bytes_per_record %llu, record_capacity %zu, record_gate %lld, geo_grid %d, n_slots %d, arrays 0x%05x\n", static_cast<unsigned long long>(job.bytes_per_record),
                 job.record_capacity, job.record_gate, job.geo_grid, job.n_slots, job.use.Mask());
  if (ctx->debug_counters) std::fprintf(stderr, "kernels: %s\n", DescribeKernels(job.kernels).c_str());
  if (ctx->debug_counters) std::fprintf(stderr, "tables: %s\n", DescribeTables(job.tables_locate, job.tables_locate_last, job.tables_inside, job.tables_redo).c_str());
  if (job.keepable && !job.reuse) {
    res.valid = false;
    res.super_tiles = job.super_tiles;
    res.mirror = job.mirror;
    if (job.kept && !job.kept_spilled) {
      res.valid = true;
      res.parked = false;
      res.pending = false;
      res.key = job.geo_key;
      res.record_capacity = job.record_capacity;
      res.kept_n_nu = job.n_nu;
      res.segments = job.segments;
      res.tail_policy = job.park ? BL_TAIL_QUAD : BL_TAIL_WIDE;
      res.n_parked = job.total_parked;
      res.n_flagged = job.total_flagged;
      res.chunks = job.kept_chunks;
      for (bl_ctx::ResidentGeodesics::Chunk &chunk : res.chunks) ClearShadingCounters(chunk.counters);
      if (ctx->debug_counters) {
        unsigned long long store = 0;
        for (const bl_ctx::ResidentGeodesics::Segment &seg : res.segments) store += seg.capacity;
        std::fprintf(stderr, "kept layout: %zu chunks, store %llu records in %zu segments, shading arrays %zu records\n", res.chunks.size(), store,
                     res.segments.size(), res.record_capacity);
      }
      res.located_valid = false;   // (located samples live in one chunk's arrays: located again every frame)
      return;
    }
    if (job.n_chunks != 1 || job.n_slots != 1) {   // (the chunks overwrote one another's records: recomputed next time)
      res.pending = ctx->overlap_chunks == 0 && !job.geo_save && !job.sample_save;
      if (res.pending) {
        // (a store that ran short: sized from what this render used, and larger than the last time)
        const unsigned long long grown = job.kept_spilled ? res.pending_records + res.pending_records / 8 : 0ull;
        res.pending_key = job.geo_key;
        res.pending_records = std::max<unsigned long long>(job.total_records, grown);
      }
      return;
    }
    res.pending = false;
    res.chunks.clear();
    res.segments.clear();
    res.valid = true;
    res.parked = false;
    res.key = job.geo_key;
    res.record_capacity = job.record_capacity;
    res.tail_policy = job.park ? BL_TAIL_QUAD : (job.split_long ? BL_TAIL_SPLIT : BL_TAIL_WIDE);
    res.n_parked = job.total_parked;
    res.n_flagged = job.total_flagged;
    std::memcpy(res.counters, hc, sizeof res.counters);
  } else if (!(job.reuse && !job.reuse_chunks && located_here && !job.reuse_located)) {
    return;
  }
  // (here: a render that integrated the geodesics, or one that located the resident samples on a new geometry)
  res.located_valid = located_here;
  res.located_key = job.located_key;
  for (int c : {BL_CNT_GATHERS, BL_CNT_UNDEFINED, BL_CNT_INTERP_FAILED}) res.counters[c] = located_here ? hc[c] : 0ull;
  res.counters[BL_CNT_REDO] = 0ull;
  for (int c = BL_CNT_COUNT; c < BL_CNT_COUNT + 12; c++) res.counters[c] = 0ull;   // the transfer kernel's statistics, debug counters
}

// ---- which arrays: decided where PlanScratch begins and again after whatever it and bl_render still drop
ArrayUse UsedArrays(const RenderJob &job) {
  ArrayUse use;
  const bool polarized = use.pol = job.ctx->polarized;
  use.located = job.simulation && !job.locate_inside;   // (locate step inside the coefficient kernel: no located samples in HBM)
  use.freq_inputs = job.freq_split;                     // ... instead of the transfer records
  use.transfer = !job.freq_split && !polarized;         // (polarized runs: the eight coefficients of a sample side by side, d_pol_coeffs)
  use.composed = job.composed;
  use.tau_inc = job.tau_row;
  use.aux = job.aux && !job.rows_only;                  // (rows_only: nobody writes or reads the 96-byte records)
  use.slow_frac = job.slow;
  use.pol_matrix = polarized && job.matrix_transport;
  use.pol_coeffs = polarized && !job.pol_one_pass;
  use.pol_variant_coeffs = polarized && job.pol_one_pass;   // polarized variants in one pass: every variant's coefficients, instead of d_pol_coeffs
  use.coef_inputs = polarized || job.coef_split;
  use.have_flags = polarized && job.pol_coefficients_inside;
  use.anchors = job.block_interp && !job.locate_inside;   // (locate step inside: the exact pass keeps a sample's anchors in registers)
  use.sample_t = job.need_time;
  use.redo = job.fast || job.fast_formula || polarized;   // (polarized runs: the samples whose frame bl_polarized_frame_kernel builds)
  use.xcd = job.xcd_order;
  use.parked = job.park || job.split_long;
  return use;
}

// The arrays of scratch set `sl` with a fixed number of entries per sample record that the render uses, in the order the kept layout lists
// their tails: visit(buffer, entries per record, whether its tail may hold part of the kept layout's store - not d_pol_variant_coeffs, so that
// a render over resident records may have more variants than the one that integrated them). The records and d_sample_t are the callers'.
template <typename Slot, typename Visitor>
void ForEachRecordArray(const RenderJob &job, Slot &sl, Visitor &&visit) {
  const ArrayUse &use = job.use;
  const size_t n_nu = static_cast<size_t>(job.n_nu);
  if (use.located) visit(sl.d_located, 1, true), visit(sl.d_located_tag, 1, true);
  if (use.freq_inputs) visit(sl.d_freq_inputs, 1, true);
  // (mirror pairs: the two arrays the shading stage fills hold the traced half's rows and, row_add = the record capacity further on,
  // the mirror half's)
  const size_t halves = job.mirror ? 2 : 1;
  if (use.transfer) visit(sl.d_transfer, n_nu * halves, true);
  if (use.composed) visit(sl.d_composed, halves, true);
  if (use.tau_inc) visit(sl.d_tau_inc, n_nu, true);
  if (use.aux) visit(sl.d_aux, 1, true);
  if (use.slow_frac) visit(sl.d_slow_frac, 1, true);
  if (use.pol) visit(sl.d_pol_samples, 1, true);
  if (use.pol_matrix) visit(sl.d_pol_matrix, BL_POL_MATRIX_DOUBLES, true);
  if (use.pol_coeffs) visit(sl.d_pol_coeffs, n_nu * 4, true);
  if (use.pol_variant_coeffs) visit(sl.d_pol_variant_coeffs, n_nu * 4 * static_cast<size_t>(job.variants.n_pol), false);
  if (use.coef_inputs) visit(sl.d_coef_inputs, 1, true);
  if (use.have_flags) visit(sl.d_have_flags, 1, true);
  if (use.anchors) visit(sl.d_anchors, 8, true);
}

// ---- kept layout (DecideReuse: the render after one of this camera that took several chunks). Scratch set 0 as the earlier render
// allocated it is re-partitioned - nothing is freed or allocated: its shading arrays take one chunk's `record_capacity` entries, and the
// store that takes every chunk's records is a list of segments, the record arrays and the tails of the shading arrays beyond those
// entries. The earlier render filled the same memory, so the scratch cap holds as it did then. The store has to hold:
//   - the records the earlier render used (ResidentGeodesics::pending_records: emitted records and the partly filled blocks of its chunks);
//   - the reservations of the rays in flight when the last chunk starts: ray_max_steps for every lane of the stepper's grid;
//   - a block of BL_RECORD_BLOCK per wave for every chunk (the part of each wave's last block the stepper leaves unfilled), and at the end
//     of every segment what is too little for one more chunk.
// Chunk c's records go to its segment + base_c, its gate is the smaller of the shading arrays' capacity and what is left of the segment,
// less a block per wave (PlaceKeptChunk, BindChunk): the stepper's reservations keep what it allocates under both, so neither can be
// overrun. A chunk starts in the next segment where what is left of this one cannot take the grid's first fill (a gate below that closes
// at once, a few rays long). Where no segment is left for a chunk, the kept layout ends for the render (kept_spilled: the rest overwrite segment 0 from its
// start, as every multi-chunk render did before; nothing is kept). The stepper's grid is held to lanes whose reservations are at most an
// sixteenth of the records: it runs in this render only, and a smaller in-flight reservation is a smaller store. False where no partition
// of what scratch set 0 holds gives the store beside a shading set that takes the grid's first fill within 16 chunks: the render is
// planned as any other.
bool PlanKeptLayout(RenderJob &job, long long max_grid, long long quad_waves, int waves_per_cu) {
  using Segment = bl_ctx::ResidentGeodesics::Segment;
  bl_ctx *ctx = job.ctx;
  bl_ctx::ChunkSlot &sl = ctx->slot[0];
  const uint64_t record_bytes = sizeof(BlSampleHot) + sizeof(BlSampleCold) + (job.need_time ? sizeof(double) : 0);
  // the record arrays as they are (segment 0)
  Segment first;
  first.hot = sl.d_records_hot.ptr;
  first.cold = job.interleaved ? nullptr : sl.d_records_cold.ptr;
  first.sample_t = job.need_time ? sl.d_sample_t.ptr : nullptr;
  first.capacity = job.interleaved ? sl.d_records_hot.count / 2 : std::min(sl.d_records_hot.count, sl.d_records_cold.count);
  if (job.need_time) first.capacity = std::min(first.capacity, sl.d_sample_t.count);
  // the shading arrays this render uses whose tails may hold the store: where they start, their bytes, their bytes per record
  struct Part {
    unsigned char *base;
    uint64_t bytes, per_record;
  };
  std::vector<Part> parts;
  uint64_t shading_cap = std::numeric_limits<uint64_t>::max();
  ForEachRecordArray(job, sl, [&](auto &buffer, size_t per_record, bool may_store) {
    if (!may_store) return;
    parts.push_back({reinterpret_cast<unsigned char *>(buffer.ptr), buffer.Bytes(), per_record * sizeof(*buffer.ptr)});
    shading_cap = std::min<uint64_t>(shading_cap, buffer.count / per_record);
  });
  shading_cap = std::min<uint64_t>(shading_cap, (1ull << 32) - (1ull << 22));   // (32-bit indices: PlanScratch)

  const uint64_t records = ctx->resident.pending_records;
  const uint64_t steps = static_cast<uint64_t>(job.max_steps);
  const uint64_t per_wave = BL_RECORD_BLOCK + 64ull * steps;
  const long long grid = std::max<long long>(1, std::min<long long>(max_grid, static_cast<long long>(records / 16 / (64ull * steps))));
  const uint64_t in_flight = static_cast<uint64_t>(grid) * 64ull * steps;
  const uint64_t blocks = static_cast<uint64_t>(grid + quad_waves) * BL_RECORD_BLOCK;
  const uint64_t least = static_cast<uint64_t>(grid) * per_wave + static_cast<uint64_t>(quad_waves) * BL_RECORD_BLOCK;   // the grid's first fill
  // (a chunk whose gate cannot take the grid's first fill closes at once, a few rays long: the rest of a segment below that is left
  // unused - PlaceKeptChunk - and a segment smaller than that is no segment)
  const uint64_t useful = least;
  if (first.hot == nullptr || first.capacity < least || shading_cap == std::numeric_limits<uint64_t>::max() || shading_cap < least) return false;
  // the segments with the shading arrays at `shading` entries (a multiple of 64: every tail starts 64-byte aligned)
  auto segments_for = [&](uint64_t shading) {
    std::vector<Segment> out{first};
    for (const Part &part : parts) {
      const uint64_t offset = shading * part.per_record;
      const uint64_t n = part.bytes > offset ? (part.bytes - offset) / record_bytes : 0;
      if (n < useful) continue;
      Segment seg;
      unsigned char *at = part.base + offset;
      seg.hot = reinterpret_cast<BlSampleHot *>(at);
      seg.cold = job.interleaved ? nullptr : reinterpret_cast<BlSampleCold *>(at + n * sizeof(BlSampleHot));
      seg.sample_t = job.need_time ? reinterpret_cast<double *>(at + n * (sizeof(BlSampleHot) + sizeof(BlSampleCold))) : nullptr;
      seg.capacity = static_cast<size_t>(n);
      out.push_back(seg);
    }
    return out;
  };
  auto room = [&](const std::vector<Segment> &segs) {   // records the segments take, less what the end of each may leave unused
    uint64_t total = 0;
    for (const Segment &seg : segs) total += seg.capacity - std::min<uint64_t>(seg.capacity, useful);
    return total;
  };
  for (uint64_t n_chunks = 2; n_chunks <= 16; n_chunks++) {
    // the largest shading capacity whose segments hold the store (fewer entries: longer tails)
    uint64_t lo = least, hi = shading_cap & ~63ull;
    if (hi < lo) return false;
    auto need = [&](const std::vector<Segment> &segs) { return records + in_flight + (n_chunks + 1 + segs.size()) * blocks; };
    if (room(segments_for(lo)) < need(segments_for(lo))) return false;
    while (hi - lo > 64) {
      const uint64_t mid = ((lo + hi) / 2) & ~63ull;
      const std::vector<Segment> segs = segments_for(mid);
      if (room(segs) >= need(segs)) lo = mid;
      else hi = mid;
    }
    {
      const std::vector<Segment> segs = segments_for(hi);
      if (room(segs) >= need(segs)) lo = hi;
    }
    const uint64_t shading = lo;
    // (a chunk closes its gate with the reservations of its rays in flight counted: it allocates at least its gate less those; a
    // segment's end can cut one chunk short)
    const std::vector<Segment> segs = segments_for(shading);
    const uint64_t per_chunk = shading - blocks - in_flight;
    if (per_chunk == 0 || (records + per_chunk - 1) / per_chunk + segs.size() - 1 > n_chunks) continue;
    job.n_slots = 1;
    job.segments = segs;
    job.record_capacity = static_cast<size_t>(shading);
    job.record_gate = static_cast<long long>(shading - blocks);
    job.chunk_capacity = job.record_capacity;
    job.chunk_gate = job.record_gate;
    job.geo_grid = static_cast<int>(grid);
    job.geo_waves_per_cu = waves_per_cu;
    job.quad_grid = static_cast<int>(quad_waves);
    job.park_capacity = job.park ? ((ctx->switches & BL_SWITCH_QUAD_EVERY_RAY) ? static_cast<size_t>(job.n_rays) : static_cast<size_t>(grid) * 64) : 0;
    job.split_long = false;   // (planned for calls one chunk is sure to take)
    job.kept_least = static_cast<long long>(least);
    return true;
  }
  return false;
}

// Where the next chunk of a kept-layout render goes: segment `segment` from `base` on, or the next segment with room for a ray
void PlaceKeptChunk(RenderJob &job, int segment, size_t base) {
  const long long blocks = static_cast<long long>(job.geo_grid + job.quad_grid) * BL_RECORD_BLOCK;
  while (!job.kept_spilled) {
    if (segment >= static_cast<int>(job.segments.size())) {
      job.kept_spilled = true;   // the store is full: this chunk and the rest overwrite segment 0 from the start, as without the kept layout
      break;
    }
    const size_t capacity = job.segments[segment].capacity;
    const size_t cap = std::min(job.record_capacity, capacity - std::min(base, capacity));
    if (static_cast<long long>(cap) >= job.kept_least) {   // (the grid's first fill: PlanKeptLayout)
      job.chunk_segment = segment;
      job.chunk_base = base;
      job.chunk_capacity = cap;
      job.chunk_gate = static_cast<long long>(cap) - blocks;
      return;
    }
    segment++;
    base = 0;
  }
  job.chunk_segment = 0;
  job.chunk_base = 0;
  job.chunk_capacity = std::min(job.record_capacity, job.segments[0].capacity);
  job.chunk_gate = static_cast<long long>(job.chunk_capacity) - blocks;
}

// Trace order per XCD (BlTraceArgs::xcd_state; BL_SWITCH_FLAT_ORDER turns it off, docs/notebook.md section 6: the coefficient
// kernel's L2 hits 21 -> 43 %, its fabric fetch -25 %, its time -1.65 ms): rays dealt to one queue per XCD in 64 x 64-pixel super-tiles, the records of an XCD's waves listed for the coefficient kernel's waves on the same XCD, whose
// gathers then share cells in that XCD's L2. For the kernel that walks the lists (bl_shade_fused2_kernel), a full root frame in
// tile order (the order swizzle_tiles gives), and geodesics integrated here into one scratch set by bl_geodesic_kernel alone - every
// other consumer of the records keeps the flat walk, and kept or loaded geodesics keep the one queue. (One scratch set: a chunk
// whose gate closed leaves rays that a queue did hand out to the next chunk, and these must not be written over while this chunk is
// still being shaded.)
bool XcdOrderApplies(const RenderJob &job) {
  const bl_ctx *ctx = job.ctx;
  const bl_params &p = ctx->params;
  return job.fused2 && !job.freq_split && !(ctx->switches & BL_SWITCH_FLAT_ORDER)
      && job.d->level == 0 && job.d->pixel_map == nullptr && p.camera_resolution % 8 == 0 && job.n_rays == job.level_pixels && !job.raster
      && !job.reuse && !job.reuse_chunks && !job.kept && job.no_checkpoint && !job.park && !job.split_long
      && !job.camera_table;   // (its super-tiles are one camera's: off for several cameras, which changes only speed)
}

// The geodesic stage's instantiation: decided here for PlanScratch - the persistent grid is sized by its occupancy - and for PlanKernels
KernelPlan::Geodesic PlanGeodesicKernel(const RenderJob &job) {
  const bl_ctx *ctx = job.ctx;
  KernelPlan::Geodesic g;
  g.source = job.reuse ? KernelPlan::Geodesic::kResident : (job.geo_load ? KernelPlan::Geodesic::kCheckpoint : KernelPlan::Geodesic::kStepper);
  g.integrator = ctx->params.ray_integrator;
  g.with_time = job.need_time;
  // (zero spin at compile time - also true for -0.0 - in the Dormand-Prince stepper only: the fixed-step steppers run it through the
  // general formulas, bit for bit the same; the empty shell: job.skip_shell asks for Dormand-Prince and no sample times)
  g.spin_zero = g.integrator == BL_INTEGRATOR_DP && ctx->st.bh_a == 0.0;
  g.shell = job.skip_shell;
  // The stages' proper distance (bl_distance_closed.h). The closed form where nothing needs the reference's s itself: the quad kernel
  // continues parked rays from it (parked or split rays), a checkpoint written or loaded goes with the exact stepper throughout.
  const bool stepper = g.source == KernelPlan::Geodesic::kStepper && g.integrator == BL_INTEGRATOR_DP;
  const bool closed = stepper && !job.park && !job.split_long && job.no_checkpoint && job.allow_closed && !(ctx->switches & BL_SWITCH_EXACT_DISTANCE);
  g.distance = !stepper ? KernelPlan::Geodesic::kNone : (closed ? KernelPlan::Geodesic::kClosed : KernelPlan::Geodesic::kExact);
  return g;
}

// Mirror pairs. With zero spin the Kerr-Schild geometry is symmetric under y -> -y, and a camera in that plane without roll or azimuthal
// velocity starts pixel (row, res - 1 - col) as the mirror image of pixel (row, col). The zero-spin Dormand-Prince stepper is equivariant
// under the reflection bit for bit (every quantity has a parity in y, every sum adds terms of one parity in a fixed order,
// correctly rounded operations commute with negation, the controller sees absolute values), so the right half's records would be the
// left half's with the sign bits of y and k_y flipped: only the left half is traced, and the shading stage walks its records twice
// (BlShadeArgs::row_add, BlTransferArgs::mirror_rays). That the start states are mirror images is not inferred from the parameters:
// bl_ray_init_kernel's own results are compared on the host, once per camera (the verdict is kept in the context with its inputs).
void BuildCameraArgs(const bl_ctx *ctx, const bl_render_desc *d, int max_steps, BlTraceArgs &ta);
bool MirrorCameraPasses(RenderJob &job) {
  bl_ctx *ctx = job.ctx;
  const bl_params &p = ctx->params;
  std::vector<unsigned char> inputs;
  KeyWriter key{&inputs};
  key.Put(ctx->st.bh_m); key.Put(ctx->st.bh_a); key.Put(ctx->st.ray_flat);
  const bl_camera_frame &f = ctx->frame;
  for (const double (*v)[4] : {&f.cam_x, &f.u_con, &f.u_cov, &f.norm_con, &f.norm_con_c, &f.hor_con_c, &f.vert_con_c})
    for (int mu = 0; mu < 4; mu++) key.Put((*v)[mu]);
  key.Put(p.camera_type); key.Put(p.camera_width); key.Put(p.camera_r); key.Put(p.camera_resolution); key.Put(p.image_normalization);
  key.Put(p.ray_integrator);
  if (ctx->mirror_key == inputs) return ctx->mirror_ok;
  const size_t n = static_cast<size_t>(job.n_rays), res = static_cast<size_t>(p.camera_resolution);
  DeviceBuffer<double2> d_constants;
  DeviceBuffer<long long> d_out_index;
  DeviceBuffer<double> d_start;
  d_constants.Ensure(n);
  d_out_index.Ensure(n);
  d_start.Ensure(n * BL_RAY_START_FIELDS);
  BlTraceArgs ta{};   // (no tile order, pixel map, block list, camera rows or camera table: slot = pixel of the one camera)
  BuildCameraArgs(ctx, job.d, job.max_steps, ta);
  ta.chunk_begin = 0;
  ta.chunk_rays = static_cast<int>(n);
  ta.ray_constants = d_constants.ptr;
  ta.ray_out_index = d_out_index.ptr;
  ta.ray_start = d_start.ptr;
  ta.ray_start_stride = static_cast<long long>(n);
  Check(bl_launch_ray_init(&ta, PlanGeodesicKernel(job), ctx->stream), "ray start kernel launch");
  Check(hipStreamSynchronize(ctx->stream), "kernel execution");
  std::vector<uint64_t> start(n * BL_RAY_START_FIELDS), constants(2 * n);
  Check(hipMemcpy(start.data(), d_start.ptr, start.size() * sizeof(uint64_t), hipMemcpyDeviceToHost), "start state download");
  Check(hipMemcpy(constants.data(), d_constants.ptr, constants.size() * sizeof(uint64_t), hipMemcpyDeviceToHost), "start state download");
  // rows of the start state: t x y z k_x k_y k_z | k_t | r | d/dlambda of (t x y z k_x k_y k_z s): odd in y are y, k_y, dy, dk_y
  constexpr uint64_t kSign = 1ull << 63;
  bool ok = true;
  for (size_t field = 0; field < BL_RAY_START_FIELDS && ok; field++) {
    const uint64_t flip = (field == 2 || field == 5 || field == 11 || field == 14) ? kSign : 0ull;
    const uint64_t *values = start.data() + field * n;
    for (size_t row = 0; row < res && ok; row++)
      for (size_t col = 0; col < res / 2; col++)
        // (an odd component may be a zero of either sign on both sides: a sum whose terms cancel exactly is +0 whatever their signs -
        // dy/dlambda of a plane camera's rays, whose directions have no y. A zero's sign changes no sum with a non-zero term and no
        // product's magnitude, and the stepper divides by nothing odd: the paths stay mirror images, the zeros may differ in sign.)
        // (The four odd components only: an even one must have the same bits on both sides, zeros included. DESIGN.md section 5.)
        if (values[row * res + col] != (values[row * res + res - 1 - col] ^ flip)
            && !(flip != 0ull && ((values[row * res + col] | values[row * res + res - 1 - col]) << 1) == 0ull)) {
          ok = false;
          if (ctx->debug_counters)
            std::fprintf(stderr, "mirror pairs: start field %zu of pixel (%zu, %zu) is %016llx, of its mirror pixel %016llx\n", field, row, col,
                         static_cast<unsigned long long>(values[row * res + col]), static_cast<unsigned long long>(values[row * res + res - 1 - col]));
          break;
        }
  }
  for (size_t row = 0; row < res && ok; row++)
    for (size_t col = 0; col < res / 2; col++) {
      const size_t a = row * res + col, b = row * res + res - 1 - col;
      if (constants[2 * a] != constants[2 * b] || constants[2 * a + 1] != constants[2 * b + 1]) {
        ok = false;
        break;
      }
    }
  ctx->mirror_key = inputs;
  ctx->mirror_ok = ok;
  return ok;
}

// Whether this render traces one ray per mirror pair: the plan's part (the paths whose kernels know the second walk - a full root frame of
// one camera in tile order, one frequency, one variant, unpolarized, no auxiliary row, no sample times, every step recorded, one block,
// nothing parked or split, no checkpoint, no camera rows - everything else takes the path it took), then the camera's. PlanScratch
// still drops it where one scratch set does not take the half frame's worst case in one chunk.
bool MirrorPairsApply(RenderJob &job) {
  const bl_ctx *ctx = job.ctx;
  const bl_params &p = ctx->params;
  const bl_render_desc *d = job.d;
  const Variants &vs = job.variants;
  const bool kernels = ((job.fused2 && !job.freq_split) || job.exact_fused) && ctx->grid.dev.n_blocks == 0;
  const bool plan = d->level == 0 && d->pixel_map == nullptr && job.n_rays == job.level_pixels && !job.camera_table && !job.raster
      && p.camera_resolution % 16 == 0 && ctx->st.bh_a == 0.0 && p.ray_integrator == BL_INTEGRATOR_DP
      && !ctx->polarized && job.n_nu == 1 && vs.list.size() == 1 && vs.n_models == 0 && vs.n_units == 0 && vs.n_cuts == 0 && vs.n_pol == 0
      && !job.aux && !job.tau_row && !job.need_time && !job.skip_shell && !job.park && !job.split_long
      && job.no_checkpoint && d->camera_pos == nullptr && d->camera_dir == nullptr
      && !(ctx->switches & BL_SWITCH_NO_MIRROR_PAIRS);
  const bool camera = kernels && plan && MirrorCameraPasses(job);
  if (ctx->debug_counters) std::fprintf(stderr, "mirror pairs: kernels %d, plan %d, camera %d\n", kernels ? 1 : 0, plan ? 1 : 0, camera ? 1 : 0);
  return camera;
}

// ---- scratch: what a sample record costs, how many fit, how many persistent waves trace rays into them
void PlanScratch(RenderJob &job) {
  bl_ctx *ctx = job.ctx;
  const bl_params &p = ctx->params;
  const int n_nu = job.n_nu;
  job.xcd_order = XcdOrderApplies(job);
  job.use = UsedArrays(job);
  // per sample record (the arrays indexed by record slot) and per kept sample (the arrays indexed by ray_offset + n: never more than records)
  job.bytes_per_record = sizeof(BlSampleHot) + sizeof(BlSampleCold);   // the two halves of a record
  ForEachRecordArray(job, ctx->slot[0], [&job](const auto &buffer, size_t per_record, bool) { job.bytes_per_record += per_record * sizeof(*buffer.ptr); });
  if (job.use.sample_t) job.bytes_per_record += sizeof(double);
  // (the record lists: BL_XCD_QUEUES x 4 bytes per 64 records; counted before the plan below can still drop the order - a chunk or more,
  // parked rays - which then leaves that byte unused)
  if (job.use.xcd) job.bytes_per_record += 1;
  if (job.reuse) {
    // over the resident records: the scratch set as the render that integrated them sized it, no stepper, nothing parked
    job.n_slots = 1;
    job.record_capacity = ctx->resident.record_capacity;
    // (polarized variants in one pass: the one array that grows with the number of variants must fit under the scratch limit beside
    // what the set holds - else one shading pass per variant over the resident records, which needs nothing more)
    if (job.pol_one_pass) {
      const bl_ctx::ChunkSlot &sl = ctx->slot[0];
      const uint64_t wanted = static_cast<uint64_t>(job.record_capacity) * n_nu * 4 * job.variants.n_pol * sizeof(double2);
      const uint64_t have = sl.d_pol_variant_coeffs.count * sizeof(double2);
      if (wanted > have && sl.Bytes() - have + wanted > ctx->scratch_limit) {
        job.pol_one_pass = false;
        job.variant_passes = job.variants.n_pol;
        PlanVariantCuts(job);   // (each pass its own variant's cut)
      }
    }
    job.record_gate = static_cast<long long>(job.record_capacity);
    if (job.reuse_chunks) job.segments = ctx->resident.segments;
    job.chunk_capacity = job.record_capacity;
    job.chunk_gate = job.record_gate;
    job.geo_grid = 1;
    job.park = job.split_long = false;
    job.park_capacity = 0;
    job.quad_grid = 0;
    return;
  }
  const uint64_t per_slot_fixed = (job.use.redo ? job.redo_capacity * sizeof(unsigned long long) : 0) + BL_CNT_TOTAL * sizeof(unsigned long long);   // d_redo, d_counters
  const bool park_every_ray = job.park && (ctx->switches & BL_SWITCH_QUAD_EVERY_RAY) != 0;
  const uint64_t per_ray = (2 + (job.geo_load ? 0 : BL_RAY_START_FIELDS) + (park_every_ray ? BL_PARK_DOUBLES : 0)) * sizeof(double) + (job.skip_shell ? 2 : 1) * sizeof(int) + 1 + 2 * sizeof(long long);
  // The budget is capped by what the device can actually give: 90 % of (free memory + what this context already holds
  // from earlier renders).
  uint64_t budget = ctx->scratch_limit;
  {
    size_t free_bytes = 0, total_bytes = 0;
    if (hipMemGetInfo(&free_bytes, &total_bytes) == hipSuccess) {
      // (the root level's resident records, set aside, are not this render's to use: they stay out of the budget)
      const uint64_t held = ctx->slot[0].Bytes() + ctx->slot[1].Bytes() + ctx->RayBytes();
      const uint64_t available = static_cast<uint64_t>(0.9 * static_cast<double>(free_bytes + held));
      if (available < budget) budget = available;
    }
  }
  const int waves_per_cu = bl_geodesic_occupancy(PlanGeodesicKernel(job));
  // No more lanes than half the rays: a lane that traces one ray only leaves its wave idling behind the longest of 64 rays, and
  // with fewer waves per SIMD each of them is faster - an eighth of the benchmark frame (131 072 rays) takes 4.3 ms on 1 024 waves,
  // 4.7 to 5.3 ms on 2 048 (and the coefficient kernel 5.0 instead of 5.2 ms over the more compact records)
  const long long max_grid = std::min<long long>(static_cast<long long>(ctx->num_cus) * waves_per_cu, std::max<long long>(1, (job.n_traced + 127) / 128));
  // (the waves of bl_geodesic_quad_kernel take blocks of record slots as well: a wave per SIMD)
  // (one to a SIMD: with three - as many as fit its registers - every ray runs at a third of the speed, the longest ones too, and
  // configuration 2 takes 94 ms instead of 67)
  const long long quad_waves = job.park ? static_cast<long long>(ctx->num_cus) * 4
      : (job.split_long ? 64ll * 4 : 0);   // (split: at most 64 compute units, sized below)
  const uint64_t worst_case = static_cast<uint64_t>(job.n_traced) * job.max_steps + static_cast<uint64_t>(max_grid + quad_waves) * BL_RECORD_BLOCK;
  const uint64_t fixed = per_ray * static_cast<uint64_t>(job.n_traced);
  if (job.kept && PlanKeptLayout(job, max_grid, quad_waves, waves_per_cu)) return;
  job.kept = false;   // (it does not fit: planned as any render, nothing kept)
  auto capacity_for = [&](int n_slots) -> uint64_t {
    const uint64_t overhead = fixed + n_slots * per_slot_fixed;
    if (budget <= overhead) return 0;
    return std::min<uint64_t>((budget - overhead) / (static_cast<uint64_t>(n_slots) * job.bytes_per_record), worst_case);
  };
  // One scratch set; two of half the size each under bl_set_overlap() when one set cannot be sure to take the whole call,
  // so that the geodesic kernel of chunk c + 1 runs while chunk c is being shaded.
  job.n_slots = 1;
  uint64_t capacity = capacity_for(1);
  if (ctx->overlap_chunks && capacity < worst_case) {
    job.n_slots = 2;
    capacity = capacity_for(2);
  }
  // Kernels index a scratch set's records with 32 bits, and a grid-stride loop runs a few strides past the last record: the
  // capacity stays 2^22 records below 2^32. Clamped BEFORE the persistent grid and the reservation gate are derived from it
  // (they were once computed from the unclamped value: a gate beyond the buffers EnsureScratch allocates).
  capacity = std::min<uint64_t>(capacity, (1ull << 32) - (1ull << 22));
  // Mirror pairs: the shading stage walks 2 n record indices with 32 bits, and the traced half must be sure to fit one chunk of one
  // scratch set. Where it is not, every ray is traced, as without pairs.
  if (job.mirror) {
    capacity = std::min<uint64_t>(capacity, ((1ull << 32) - (1ull << 22)) / 2);
    if (job.n_slots != 1 || capacity < worst_case) {
      job.mirror = false;
      job.n_traced = job.n_rays;
      PlanScratch(job);
      return;
    }
  }
  // Persistent waves: every lane in flight holds ray_max_steps record slots until its ray ends, so no more lanes than the
  // buffer can cover at once. (A chunk still takes about capacity / samples-per-ray rays: a finished ray gives back what it
  // did not emit and the lanes that were refused ask again. Fewer waves than that would only trace the same rays more
  // slowly - 500 instead of 2 048 waves took the 64-frequency exact frame's geodesic stage from 37 to 183 ms.)
  const uint64_t per_wave = BL_RECORD_BLOCK + 64ull * static_cast<uint64_t>(job.max_steps);
  const long long grid = std::max<long long>(1, std::min<long long>(max_grid, static_cast<long long>((capacity - std::min<uint64_t>(capacity, static_cast<uint64_t>(quad_waves) * BL_RECORD_BLOCK)) / per_wave)));
  const long long gate = static_cast<long long>(capacity) - (grid + quad_waves) * BL_RECORD_BLOCK;
  if (gate < job.max_steps)
    throw Failure{BL_E_ARG, "Scratch budget too small: the sample records of a single ray (ray_max_steps of them) do not fit (bl_set_scratch_limit)."};
  job.record_capacity = static_cast<size_t>(capacity);
  job.record_gate = gate;
  job.chunk_capacity = job.record_capacity;
  job.chunk_gate = gate;
  job.geo_grid = static_cast<int>(grid);
  job.geo_waves_per_cu = waves_per_cu;
  job.quad_grid = static_cast<int>(quad_waves);
  // a lane parks at most one ray (its wave ends), unless every ray is parked
  job.park_capacity = job.park ? (park_every_ray ? static_cast<size_t>(job.n_rays) : static_cast<size_t>(grid) * 64) : 0;
  // (the split is decided once for all rays of the call: only where one chunk is sure to take them all)
  if (job.split_long && (job.n_slots != 1 || capacity < worst_case)) job.split_long = false;
  // (... and so is the trace order per XCD: a gate that closed would leave rays some queue had handed out to the next chunk, to be
  // traced twice - correct, bl_rays_done, but the counts and the kept layout's sizes would include them)
  if (job.n_slots != 1 || capacity < worst_case) job.xcd_order = false;
  if (job.split_long) {
    // Which rays. Alone in a wave a ray of the benchmark camera takes 3.2 ms at b = 5.20 M, 2.3 ... 2.9 ms between 4.9 and 5.18, 2.3 ms
    // at 5.23 and 1.8 ms at 5.3 (tools/gpu_ray_length_by_radius.py): the band reaches 0.03 M beyond the critical curve and inwards
    // as far as the quad stepper's compute units hold it in ONE round of quads (a second round doubles its time) - a quad per ray,
    // 16 per wave, a wave per SIMD. The compute units: an eighth of the device, bits 0 ... num_cus / 8 - 1 of the mask - on MI355X
    // one CU of every shader engine of every XCD (tools/ubench/cu_mask_probe.hip), which leaves the other stepper's share of every
    // shader engine equal; other counts were measured and lose (uneven shader engines fill unevenly: docs/notebook.md section 5k).
    // How densely the call's rays cover the ring is counted on the host from every 1 / stride-th of them.
    const double centre = 5.196152422706632 * ctx->st.bh_m;
    const double scale = ctx->st.bh_m * p.camera_width / p.camera_resolution, half = 0.5 * p.camera_resolution - 0.5;
    const double ref_lo = centre - 0.3 * ctx->st.bh_m, ref_hi = centre + 0.1 * ctx->st.bh_m;
    const long long stride = std::max<long long>(1, job.n_rays / 32768);
    long long seen = 0, inside = 0;
    for (long long ray = 0; ray < job.n_rays; ray += stride, seen++) {
      const long long pixel = job.d->pixel_map != nullptr ? job.d->pixel_map[ray] : ray;
      const double u = (static_cast<double>(pixel % p.camera_resolution) - half) * scale, v = (static_cast<double>(pixel / p.camera_resolution) - half) * scale;
      const double b = std::sqrt(u * u + v * v);
      inside += (b >= ref_lo && b <= ref_hi) ? 1 : 0;
    }
    const double per_width = static_cast<double>(inside) * static_cast<double>(job.n_rays) / static_cast<double>(std::max<long long>(seen, 1)) / (ref_hi - ref_lo);
    job.split_cus = std::max(1, ctx->num_cus / 8);
    const double outer = 0.03 * ctx->st.bh_m;
    // (rounds of quads: one where the stage is a few rays per lane long - a second round would end after the other stepper -, more
    // where the other stepper has many rays per lane to get through and the quad stepper's compute units would stand idle meanwhile)
    const int rounds = job.n_rays > 2ll * 256 * ctx->num_cus ? 2 : 1;   // (a quarter of the frame: 14.0 ms with two, 14.6 with one, 14.5 with three)
    double width = per_width > 0.0 ? 0.9 * 64.0 * job.split_cus * rounds / per_width : 0.0;   // of the band
    width = std::min(width, 0.45 * ctx->st.bh_m);
    if (width >= 0.08 * ctx->st.bh_m) {
      job.split_b_lo = centre - (width - outer);
      job.split_b_hi = centre + outer;
    } else {
      job.split_long = false;   // no ring in these rays, or too many rays on it for an eighth of the device
    }
  }
  if (job.split_long) {
    job.park_capacity = static_cast<size_t>(job.n_rays);
    job.quad_grid = job.split_cus * 4;
  }
  if (job.n_slots != 1 || job.park || job.split_long) job.xcd_order = false;
}

// ---- which kernels: the one place where the plan's flags turn into template arguments (KernelPlan, bl_kernel_plan.h). Runs behind the
// plan, the scratch decision and UsedArrays, so that it sees what they dropped; reads flags and parameters, never the argument blocks'
// pointers - those follow from job.use, and the launch wrappers check that they agree with what is chosen here.
void PlanKernels(RenderJob &job) {
  const bl_ctx *ctx = job.ctx;
  const bl_params &p = ctx->params;
  const ArrayUse &use = job.use;
  KernelPlan &k = job.kernels;
  k = KernelPlan{};
  const bool spin_zero = ctx->st.bh_a == 0.0;
  const bool refined = job.simulation && ctx->grid.dev.n_blocks > 0;
  const bool slices = job.slow && p.slow_chunk_size > 0;
  const bool sks = p.simulation_coord != BL_COORD_CKS;   // (FMKS: everything but the cell search treats the grid as sks, BuildShadeArgs)
  const bool power_law = job.simulation && job.any_power;   // (some variant's: PlanJob)
  k.geodesic = PlanGeodesicKernel(job);
  k.quad.park = job.park;
  k.quad.split = job.split_long;
  k.quad.spin_zero = spin_zero;
  if (job.simulation && !job.locate_inside && !job.reuse_located) {
    // the common case has a kernel of its own: one grid with its tables in LDS, spherical, trilinear, no optional geometric cut
    const bool plain = !refined && !slices && ctx->grid.tables.lds_table_bytes > 0 && !ctx->grid.dev.fmks && p.simulation_interp && !GeometricCut(p) && sks
        && !use.anchors && !(ctx->switches & BL_SWITCH_GENERAL_LOCATE);
    k.locate.kind = plain ? KernelPlan::Locate::kPlain : KernelPlan::Locate::kGeneral;
    k.locate.spin_zero = plain && spin_zero;
    k.locate.refined = refined;
    k.locate.slow = slices;
    k.locate.tables_in_hbm = !plain && !refined && ctx->grid.tables.lds_table_bytes == 0;
  }
  KernelPlan::Shade &c = k.shade;
  c.model = p.model_type;
  if (job.fused2) {
    c.family = KernelPlan::Shade::kFused2;
    c.spin_zero = spin_zero;
    c.refined = refined;   // (a mesh: one frequency and composed maps, PlanJob - the wrapper refuses anything else)
    c.factors = job.freq_split;
    c.composed = job.composed;
  } else if (job.fast) {
    // power laws, Cartesian grids and an optical-depth image go through the general instantiation; inter-block interpolation and slow
    // light through the ones that also know anchor cells and time slices
    c.family = KernelPlan::Shade::kFast;
    c.mode = slices ? 3 : (use.anchors ? 2 : ((power_law || job.tau_row || !sks) ? 1 : 0));
    c.spin_zero = c.mode == 0 && spin_zero;
  } else if (job.fast_formula) {
    c.family = KernelPlan::Shade::kFormulaFast;
  } else if (job.exact_fused) {
    c.family = KernelPlan::Shade::kExact2;
    c.spin_zero = spin_zero;
  } else if (job.pol_fused) {
    c.family = KernelPlan::Shade::kPolarized2;
    c.spin_zero = spin_zero;
    c.records = !job.rows_only;
    c.coefficients = job.pol_coefficients_inside;
  } else if (!job.simulation) {
    c.aux = use.aux;
  } else {
    const bool sks_curved = sks && !ctx->st.ray_flat;
    c.polarized = ctx->polarized;
    c.aux = ctx->polarized || use.aux;   // (a polarized run is an auxiliary-image run whether or not it keeps BlAuxSample records)
    c.extended = ctx->polarized || power_law || p.plasma_model == BL_PLASMA_CODE_KAPPA || slices || use.anchors || job.any_kappa;
    c.sks = ctx->polarized && sks_curved;
    // plain image of a spherical Kerr-Schild simulation in a curved spacetime: the software-pipelined kernel
    if (!c.aux && !c.extended && sks_curved) {
      c.family = KernelPlan::Shade::kExact;
      c.spin_zero = spin_zero;
    }
  }
  if (job.fast || job.fast_formula) {   // the exact second pass over the records the tolerant kernel listed
    KernelPlan::Redo &r = k.redo;
    r.run = true;
    r.model = p.model_type;
    if (job.simulation) {
      // (behind the fused kernel the extended instantiation is the one that knows the anchor cells of inter-block interpolation)
      r.extended = job.fused2 ? job.block_interp : (!sks || power_law || job.tau_row || use.anchors || slices);
      r.sks = job.fused2 || sks;
      r.spin_zero = !r.extended && spin_zero;
      const int tables = ctx->grid.dev.refined_lds_bytes;   // (the mesh's tables in LDS, if they are small enough)
      r.table_bytes = (r.extended && job.fused2 && refined && tables > 0 && tables <= BL_REDO_TABLES_LDS) ? tables : 0;
    }
  }
  k.freq.polarized_frames = ctx->polarized;
  k.freq.polarized_coefficients = ctx->polarized && !job.pol_coefficients_inside;
  k.freq.thermal_only = ctx->polarized && job.all_thermal;   // (the parameter block and every variant)
  k.freq.coefficients_freq = job.coef_split;
  k.transfer.affine = job.fast || job.fast_formula;
  k.transfer.tau = job.tau_row;
  k.transfer.kind = job.aux ? KernelPlan::Transfer::kAux
      : job.freq_split ? KernelPlan::Transfer::kFreq
      : job.composed ? KernelPlan::Transfer::kComposed
      : (k.transfer.affine && job.n_nu == 1 && !(ctx->switches & BL_SWITCH_LANE_TRANSFER)) ? KernelPlan::Transfer::kQuad : KernelPlan::Transfer::kLane;
  // The transport matrices - memory - on the second stream beside the per-frequency coefficient kernel - arithmetic: both read what
  // the coefficient kernel left, neither reads the other. (The coefficient kernel's workgroups fill the device first, so the
  // matrices overlap its last quarter only: 276 -> 270 ms per 1024^2 frame, 1.10 -> 1.08 s at 2048^2 adaptive; a smaller grid for the
  // coefficient kernel or a priority stream for the matrices move the split, not the sum.)
  // (one scratch set: with two, the second stream carries the next chunk's geodesic stage, and the matrices would queue behind it)
  // (with the coefficients evaluated inside the coefficient kernel there is nothing left beside which to build them: in sequence)
  if (ctx->polarized)
    k.polarized = !job.matrix_transport ? KernelPlan::kTensor
        : (job.n_slots == 1 && !job.pol_coefficients_inside) ? KernelPlan::kMatricesBeside : KernelPlan::kMatrix;
}

void EnsureScratchOnce(RenderJob &job);
// The budget counts what the context already holds as available (PlanScratch); arrays of an earlier render in another mode - per-
// frequency transfer records where this one wants per-sample factors - are not among those this render grows. When an allocation
// fails, everything the scratch sets hold goes back to the device and the render's own arrays are allocated afresh.
void EnsureScratch(RenderJob &job) {
  try {
    EnsureScratchOnce(job);
  } catch (const Failure &) {
    (void)hipGetLastError();
    if (job.reuse) throw ReuseImpossible{};   // (scratch set 0 holds the resident records: the call is planned again without them)
    DropResident(job.ctx);                    // (... set aside: they make room)
    job.ctx->slot[0].Free();
    job.ctx->slot[1].Free();
    EnsureScratchOnce(job);
  }
}

void EnsureScratchOnce(RenderJob &job) {
  bl_ctx *ctx = job.ctx;
  const size_t cap = job.record_capacity;
  // kept layout: the record arrays and the tails of the others are the store, left as they are (PlanKeptLayout planned within what
  // scratch set 0 holds: none of the arrays below grows)
  const bool store = job.kept || job.reuse_chunks;
  for (int k = 0; k < job.n_slots; k++) {
    bl_ctx::ChunkSlot &sl = ctx->slot[k];
    if (!store) {
      sl.d_records_hot.Ensure(job.interleaved ? 2 * cap : cap);
      if (!job.interleaved) sl.d_records_cold.Ensure(cap);
      if (job.use.sample_t) sl.d_sample_t.Ensure(cap);
    }
    ForEachRecordArray(job, sl, [cap](auto &buffer, size_t per_record, bool) { buffer.Ensure(cap * per_record); });
    if (job.use.xcd) {
      sl.d_xcd_state.Ensure(4 * BL_XCD_QUEUES);
      sl.d_xcd_lists.Ensure(BL_XCD_QUEUES * (cap / 64 + 1));
    }
    if (job.use.parked) sl.d_parked.Ensure(job.park_capacity * BL_PARK_DOUBLES);
    sl.d_counters.Ensure(BL_CNT_TOTAL);
    if (job.use.redo) sl.d_redo.Ensure(job.redo_capacity);
  }
  const size_t n_rays = static_cast<size_t>(job.n_traced);
  auto ensure = [n_rays](auto &...buffer) { (buffer.Ensure(n_rays), ...); };
  ensure(ctx->rays.constants, ctx->rays.sample_num, ctx->rays.flags, ctx->rays.out_index, ctx->rays.offset);
  if (job.skip_shell) ctx->rays.skipped.Ensure(n_rays);
  if (job.composed) ctx->rays.rows.Ensure(n_rays);
  if (!job.geo_load) ctx->d_ray_start.Ensure(n_rays * BL_RAY_START_FIELDS);
  EnsureRenderResources(ctx);
}

// ---- inputs of the call that live in HBM: frequencies, pixel map, block list; output buffers (the caller's, or staging)
void StageInputsAndOutputs(RenderJob &job) {
  bl_ctx *ctx = job.ctx;
  const bl_render_desc *d = job.d;
  const bl_params &p = ctx->params;
  hipStream_t stream = ctx->stream;
  const long long n_rays = job.n_rays;
  if (ctx->caller_stream_set) {
    // bl_set_caller_stream: whatever the caller queued on its stream up to now (fills of the output buffers, a collective still
    // reading the previous frame out of them) is ahead of everything this call queues (both of its streams start behind `stream`) - a wait on the device, none on the host
    if (ctx->caller_event == nullptr) Check(hipEventCreateWithFlags(&ctx->caller_event, hipEventDisableTiming), "hipEventCreate");
    Check(hipEventRecord(ctx->caller_event, ctx->caller_stream), "event on the caller's stream");
    Check(hipStreamWaitEvent(stream, ctx->caller_event, 0), "stream wait");
  }
  ctx->d_freq.Ensure(job.n_nu);
  Check(hipMemcpyAsync(ctx->d_freq.ptr, ctx->frequencies.data(), job.n_nu * sizeof(double), hipMemcpyHostToDevice, stream), "freq upload");
  if (d->pixel_map != nullptr) {
    ctx->d_pixel_map.Ensure(n_rays);
    Check(hipMemcpyAsync(ctx->d_pixel_map.ptr, d->pixel_map, n_rays * sizeof(int), hipMemcpyHostToDevice, stream), "pixel_map upload");
    job.d_pixel_map = ctx->d_pixel_map.ptr;
  }
  if (d->level > 0) {
    ctx->d_block_locs.Ensure(static_cast<size_t>(d->n_blocks) * 2);
    Check(hipMemcpyAsync(ctx->d_block_locs.ptr, d->block_locs, static_cast<size_t>(d->n_blocks) * 2 * sizeof(int), hipMemcpyHostToDevice, stream), "block_locs upload");
    job.d_block_locs = ctx->d_block_locs.ptr;
  }
  job.image = d->image;
  job.cam_pos = d->camera_pos;
  job.cam_dir = d->camera_dir;
  job.out_num = d->sample_num;
  job.out_flags = d->sample_flags;
  if (!d->outputs_on_device) {
    ctx->d_image.Ensure(static_cast<size_t>(job.n_q) * n_rays);
    job.image = ctx->d_image.ptr;
    if (d->sample_num != nullptr) { ctx->d_out_sample_num.Ensure(n_rays); job.out_num = ctx->d_out_sample_num.ptr; }
    if (d->sample_flags != nullptr) { ctx->d_out_flags.Ensure(n_rays); job.out_flags = ctx->d_out_flags.ptr; }
    if (d->camera_pos != nullptr) { ctx->d_camera_pos.Ensure(static_cast<size_t>(n_rays) * 4); job.cam_pos = ctx->d_camera_pos.ptr; }
    if (d->camera_dir != nullptr) { ctx->d_camera_dir.Ensure(static_cast<size_t>(n_rays) * 4); job.cam_dir = ctx->d_camera_dir.ptr; }
  }
  if (ctx->polarized || job.geo_save) {   // the camera tetrad projection (and the checkpoint) need every ray's initial position and momentum
    if (job.cam_pos == nullptr) { ctx->d_camera_pos.Ensure(static_cast<size_t>(n_rays) * 4); job.cam_pos = ctx->d_camera_pos.ptr; }
    if (job.cam_dir == nullptr) { ctx->d_camera_dir.Ensure(static_cast<size_t>(n_rays) * 4); job.cam_dir = ctx->d_camera_dir.ptr; }
  }
  if (job.geo_load && (job.cam_pos != nullptr || job.cam_dir != nullptr)) {   // camera_pos / camera_dir come from the file as well
    if (ctx->caller_stream_set) Check(hipStreamSynchronize(ctx->caller_stream), "caller's stream");   // (blocking copies below: no stream orders them)
    for (int which = 0; which < 2; which++) {
      double *target = which == 0 ? job.cam_pos : job.cam_dir;
      if (target == nullptr) continue;
      const std::vector<double> rows = GatherCameraRows(which == 0 ? ctx->checkpoint->camera_pos : ctx->checkpoint->camera_dir, d->pixel_map, n_rays);
      Check(hipMemcpy(target, rows.data(), rows.size() * sizeof(double), hipMemcpyHostToDevice), "checkpoint upload");
    }
  }
  if (ctx->render_num_images > 0) {
    BlRenderDevice rp{};
    rp.n_images = ctx->render_num_images;
    for (int n_i = 0; n_i < rp.n_images; n_i++) {
      rp.n_features[n_i] = p.render_num_features[n_i];
      for (int n_f = 0; n_f < rp.n_features[n_i]; n_f++) {
        rp.quantity[n_i][n_f] = p.render_quantity[n_i][n_f];
        rp.type[n_i][n_f] = p.render_type[n_i][n_f];
        rp.min_val[n_i][n_f] = p.render_min[n_i][n_f];
        rp.max_val[n_i][n_f] = p.render_max[n_i][n_f];
        rp.thresh[n_i][n_f] = p.render_thresh[n_i][n_f];
        rp.tau_scale[n_i][n_f] = p.render_tau_scale[n_i][n_f];
        rp.opacity[n_i][n_f] = p.render_opacity[n_i][n_f];
        rp.xyz[n_i][n_f][0] = p.render_x[n_i][n_f];
        rp.xyz[n_i][n_f][1] = p.render_y[n_i][n_f];
        rp.xyz[n_i][n_f][2] = p.render_z[n_i][n_f];
      }
    }
    rp.fill_present = job.fill_present ? 1 : 0;
    ctx->d_render_params.Ensure(1);
    Check(hipMemcpyAsync(ctx->d_render_params.ptr, &rp, sizeof(BlRenderDevice), hipMemcpyHostToDevice, stream), "render parameter upload");
    Check(hipStreamSynchronize(stream), "render parameter upload");   // rp is a local
    job.render_out = d->render;
    if (!d->outputs_on_device) {
      ctx->d_render.Ensure(static_cast<size_t>(ctx->render_num_images) * 3 * n_rays);
      job.render_out = ctx->d_render.ptr;
    }
  }
}

// ---- kernel arguments common to all chunks: the geodesic kernel's. First what the context alone decides - spacetime, the camera's
// block, the stepper's settings: all bl_ray_init_kernel reads besides the arrays it is pointed at (MirrorCameraPasses launches it on
// these before the call is planned)
void BuildCameraArgs(const bl_ctx *ctx, const bl_render_desc *d, int max_steps, BlTraceArgs &ta) {
  const bl_params &p = ctx->params;
  ta.st = ctx->st;
  BlCameraDevice &cam = ta.cam;
  for (int mu = 0; mu < 4; mu++) {
    cam.cam_x[mu] = ctx->frame.cam_x[mu];
    cam.u_con[mu] = ctx->frame.u_con[mu];
    cam.u_cov[mu] = ctx->frame.u_cov[mu];
    cam.norm_con[mu] = ctx->frame.norm_con[mu];
    cam.norm_con_c[mu] = ctx->frame.norm_con_c[mu];
    cam.hor_con_c[mu] = ctx->frame.hor_con_c[mu];
    cam.vert_con_c[mu] = ctx->frame.vert_con_c[mu];
  }
  cam.camera_width = p.camera_width;
  cam.camera_r = p.camera_r;
  cam.camera_type = p.camera_type;
  cam.image_normalization = p.image_normalization;
  cam.camera_resolution = p.camera_resolution;
  cam.level = d->level;
  cam.block_size = p.adaptive_max_level > 0 ? p.adaptive_block_size : 1;
  cam.effective_resolution = p.camera_resolution;
  for (int l = 1; l <= d->level; l++) cam.effective_resolution *= 2;
  ta.r_terminate = ctx->frame.r_terminate;
  ta.r_horizon = ctx->frame.r_horizon;
  ta.camera_r = p.camera_r;
  ta.ray_step = p.ray_step;
  ta.ray_tol_abs = p.ray_integrator == BL_INTEGRATOR_DP ? p.ray_tol_abs : 0.0;
  ta.ray_tol_rel = p.ray_integrator == BL_INTEGRATOR_DP ? p.ray_tol_rel : 0.0;
  ta.ray_max_steps = max_steps;
  ta.ray_max_retries = p.ray_integrator == BL_INTEGRATOR_DP ? p.ray_max_retries : 0;
}

// ... then what the plan decides: which rays in which order, the skipped shell, the camera table
void BuildTraceArgs(RenderJob &job) {
  bl_ctx *ctx = job.ctx;
  const bl_render_desc *d = job.d;
  const bl_params &p = ctx->params;
  BlTraceArgs &ta = job.ta;
  BuildCameraArgs(ctx, d, job.max_steps, ta);
  const BlCameraDevice &cam = ta.cam;
  ta.skip_low = std::numeric_limits<double>::infinity();
  ta.skip_high = 0.0;
  if (job.skip_shell) {
    const double a = ctx->st.bh_a;
    ta.skip_low = std::sqrt(ctx->grid.tables.outer_x1 * ctx->grid.tables.outer_x1 * (1.0 + 1.0e-9) + a * a) * (1.0 + 1.0e-12);
    ta.skip_high = p.camera_r * (1.0 - 1.0e-9);
  }
  ta.n_rays_total = job.n_rays;
  ta.swizzle_tiles = (d->level == 0 && d->pixel_map == nullptr && p.camera_resolution % 8 == 0 && job.n_rays == job.level_pixels && !job.raster)
      ? p.camera_resolution : 0;
  // Order in which the 8x8 pixel tiles of a full frame are traced: centre of the image first. Rays near
  // the centre (photon ring, disc) are the long ones, the periphery is short; a chunk that ends on short
  // rays drains its persistent waves quickly (measured: geodesic kernel 33.9 -> 29.4 ms per frame at four
  // chunks), and waves of similar ray lengths also diverge less in the transfer kernel.
  // With the trace order per XCD (job.xcd_order) the unit of that order is a super-tile of 8 x 8 tiles (64 x 64 pixels, its tiles
  // row by row: BL_XCD_RUN rays), super-tiles centre first, dealt to its queues round-robin (BlTraceArgs::xcd_state), so that every
  // queue has its share of the long rays near the centre and of the short ones further out. A render over resident records
  // (job.reuse) uses the order of the render that integrated them: its ray slots must name the same pixels.
  ta.tile_order = nullptr;
  job.super_tiles = false;
  if (ta.swizzle_tiles > 0) {
    const bool super_tiles = job.reuse ? ctx->resident.super_tiles : job.xcd_order;
    job.super_tiles = super_tiles;
    if (ctx->tile_order_res != p.camera_resolution || ctx->tile_order_xcd != super_tiles || ctx->tile_order_cameras != job.n_cameras
        || ctx->tile_order_half != job.mirror) {
      const int tiles_per_row = p.camera_resolution / 8;
      const int n_tiles = tiles_per_row * tiles_per_row;
      const int unit = super_tiles ? 8 : 1;   // (tiles per side of the unit)
      // (mirror pairs: the tiles of the left half only, in the order they have in the whole frame's)
      std::vector<int> order;
      order.reserve(n_tiles);
      for (int t = 0; t < n_tiles; t++)
        if (!job.mirror || t % tiles_per_row < tiles_per_row / 2) order.push_back(t);
      const int units_per_row = (tiles_per_row + unit - 1) / unit;
      const double centre = 0.5 * (units_per_row - 1);
      auto unit_index = [&](int t) { return (t / tiles_per_row / unit) * units_per_row + t % tiles_per_row / unit; };
      auto unit_dist2 = [&](int t) {
        const int u = unit_index(t);
        const double dy = u / units_per_row - centre, dx = u % units_per_row - centre;
        return dx * dx + dy * dy;
      };
      std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
        const double da = unit_dist2(a), db = unit_dist2(b);
        return da != db ? da < db : unit_index(a) < unit_index(b);
      });
      // Several cameras: the ray set is an image of res x C res pixels, camera c's tiles are c n_tiles + t. Interleaved - tile t of
      // every camera, then the next tile of the one order - so that every camera's long rays near its centre come first and a chunk,
      // and the call, ends on every camera's short ones.
      if (job.n_cameras >= 2) {
        std::vector<int> stacked;
        stacked.reserve(static_cast<size_t>(n_tiles) * job.n_cameras);
#ifdef BL_CAMERAS_CONSECUTIVE   // (A/B builds: camera after camera, each centre first - profiles/cameras.json has both orders' times)
        for (int c = 0; c < job.n_cameras; c++)
          for (int t = 0; t < n_tiles; t++) stacked.push_back(c * n_tiles + order[t]);
#else
        for (int t = 0; t < n_tiles; t++)
          for (int c = 0; c < job.n_cameras; c++) stacked.push_back(c * n_tiles + order[t]);
#endif
        order.swap(stacked);
      }
      ctx->d_tile_order.Ensure(order.size());
      Check(hipMemcpy(ctx->d_tile_order.ptr, order.data(), order.size() * sizeof(int), hipMemcpyHostToDevice), "tile order upload");
      if (job.mirror) {   // where the mirror pixel of every traced slot goes (the geodesic kernel's traversal_to_ray, reflected)
        const long long res = p.camera_resolution;
        std::vector<long long> mirror_out(order.size() * 64);
        for (size_t q = 0; q < mirror_out.size(); q++) {
          const long long tile = order[q >> 6], within = static_cast<long long>(q & 63);
          const long long m2 = tile / tiles_per_row * 8 + (within >> 3), m1 = tile % tiles_per_row * 8 + (within & 7);
          mirror_out[q] = m2 * res + (res - 1 - m1);
        }
        ctx->d_mirror_out.Ensure(mirror_out.size());
        Check(hipMemcpy(ctx->d_mirror_out.ptr, mirror_out.data(), mirror_out.size() * sizeof(long long), hipMemcpyHostToDevice), "mirror pixel upload");
      }
      ctx->tile_order_res = p.camera_resolution;
      ctx->tile_order_xcd = super_tiles;
      ctx->tile_order_cameras = job.n_cameras;
      ctx->tile_order_half = job.mirror;
    }
    ta.tile_order = ctx->d_tile_order.ptr;
  }
  ta.pixel_map = job.d_pixel_map;
  ta.block_locs = job.d_block_locs;
  ta.camera_pos = job.cam_pos;
  ta.camera_dir = job.cam_dir;
  ta.ray_start_stride = job.n_traced;
  // Several cameras: every camera's block as `cam` above with its own seven vectors, in HBM (uploaded when the list changes)
  ta.cameras = nullptr;
  ta.pixels_per_camera = 0;
  if (job.camera_table) {
    if (!ctx->cameras_uploaded) {
      std::vector<BlCameraDevice> table(ctx->cameras.size(), cam);
      for (size_t c = 0; c < table.size(); c++) {
        const bl_camera_frame &f = ctx->cameras[c].frame;
        for (int mu = 0; mu < 4; mu++) {
          table[c].cam_x[mu] = f.cam_x[mu];
          table[c].u_con[mu] = f.u_con[mu];
          table[c].u_cov[mu] = f.u_cov[mu];
          table[c].norm_con[mu] = f.norm_con[mu];
          table[c].norm_con_c[mu] = f.norm_con_c[mu];
          table[c].hor_con_c[mu] = f.hor_con_c[mu];
          table[c].vert_con_c[mu] = f.vert_con_c[mu];
        }
      }
      ctx->d_cameras.Ensure(table.size());
      Check(hipMemcpy(ctx->d_cameras.ptr, table.data(), table.size() * sizeof(BlCameraDevice), hipMemcpyHostToDevice), "camera table upload");
      ctx->cameras_uploaded = true;
    }
    ta.cameras = ctx->d_cameras.ptr;
    ta.pixels_per_camera = static_cast<long long>(p.camera_resolution) * p.camera_resolution;
  }
}

// Power-law and kappa-distribution constants of the coefficient formulas (simulation_coefficients.cpp:54-193); pow / exp / log
// and K_nu are the pinned ones, tgamma the host libm's. A function of the mix alone (and of whether the run is polarized): the shape
// values of a distribution whose fraction is zero are not read.
ElectronConstants FillElectronConstants(const bl_electron_mix &mix, bool polarized) {
  ElectronConstants ec;
  std::memset(static_cast<void *>(&ec), 0, sizeof ec);
  ec.thermal_frac = ThermalFraction(mix);
  ec.power_frac = mix.power_frac;
  if (mix.power_frac != 0.0) {
    // simulation_coefficients.cpp:54-66 (unpolarized part)
    const double plasma_p = mix.p;
    const double var_a = bl_pow(3.0, plasma_p / 2.0) * (plasma_p - 1.0);
    const double var_b = 2.0 * (plasma_p + 1.0);
    const double var_c = bl_pow(mix.gamma_min, 1.0 - plasma_p) - bl_pow(mix.gamma_max, 1.0 - plasma_p);
    const double var_d = std::tgamma((3.0 * plasma_p - 1.0) / 12.0);
    const double var_e = std::tgamma((3.0 * plasma_p + 19.0) / 12.0);
    const double var_f = bl_pow(3.0, (plasma_p + 1.0) / 2.0) * (plasma_p - 1.0) / 4.0;
    const double var_g = std::tgamma((3.0 * plasma_p + 2.0) / 12.0);
    const double var_h = std::tgamma((3.0 * plasma_p + 22.0) / 12.0);
    ec.plasma_p = plasma_p;
    ec.plasma_gamma_min = mix.gamma_min;
    ec.power_jj = var_a / var_b / var_c * var_d * var_e;
    ec.power_aa = var_f / var_c * var_g * var_h;
    if (polarized) {   // simulation_coefficients.cpp:67-80
      const double var_i = 2.0 * (plasma_p + 2.0) / (plasma_p + 1.0);
      const double var_j = bl_pow(mix.gamma_min, -(plasma_p + 1.0));
      const double var_k = bl_log(mix.gamma_min);
      ec.power_pol[0] = -(plasma_p + 1.0) / (plasma_p + 7.0 / 3.0);
      ec.power_pol[1] = 0.684 * bl_pow(plasma_p, 0.49);
      ec.power_pol[2] = -bl_pow(0.034 * plasma_p - 0.0344, 0.086);
      ec.power_pol[3] = bl_pow(0.71 * plasma_p + 0.0352, 0.394);
      ec.power_pol[4] = (plasma_p - 1.0) / var_c;
      ec.power_pol[5] = -bl_pow(mix.gamma_min, 2.0 - plasma_p) / (plasma_p / 2.0 - 1.0);
      ec.power_pol[6] = var_i * var_j * var_k;
    }
  }
  if (mix.kappa_frac != 0.0) {
    // simulation_coefficients.cpp:82-193 for a polarized run
    BlKappaDevice &kk = ec.kappa;
    const double plasma_kappa = mix.kappa, plasma_w = mix.w;
    kk.frac = mix.kappa_frac;
    kk.kappa = plasma_kappa;
    kk.w = plasma_w;
    const double var_a = 4.0 * kPi * std::tgamma(plasma_kappa - 4.0 / 3.0);
    const double var_b = bl_pow(3.0, 7.0 / 3.0) * std::tgamma(plasma_kappa - 2.0);
    const double var_c = bl_pow(3.0, (plasma_kappa - 1.0) / 2.0);
    const double var_d = (plasma_kappa - 2.0) * (plasma_kappa - 1.0) / 4.0;
    const double var_e = std::tgamma(plasma_kappa / 4.0 - 1.0 / 3.0);
    const double var_f = std::tgamma(plasma_kappa / 4.0 + 4.0 / 3.0);
    const double var_g = bl_pow(3.0, 1.0 / 6.0) * 10.0 / 41.0;
    const double var_h = plasma_w * plasma_kappa;
    const double var_i = 2.0 * kPi * bl_pow(var_h, plasma_kappa - 10.0 / 3.0);
    const double var_j = (plasma_kappa - 2.0) * (plasma_kappa - 1.0) * plasma_kappa;
    const double var_k = 3.0 * plasma_kappa - 1.0;
    const double var_l = std::tgamma(5.0 / 3.0);
    const double var_m = Hypergeometric(plasma_kappa - 1.0 / 3.0, plasma_kappa + 1.0, plasma_kappa + 2.0 / 3.0, -var_h);
    const double var_n = bl_pow(kPi, 1.5) / 3.0;
    const double var_o = var_j / (var_h * var_h * var_h);
    const double var_p = 2.0 * std::tgamma(2.0 + plasma_kappa / 2.0) / (2.0 + plasma_kappa) - 1.0;
    kk.jj_low = var_a / var_b;
    kk.jj_high = var_c * var_d * var_e * var_f;
    kk.jj_x_i = 3.0 * bl_pow(plasma_kappa, -1.5);
    kk.aa_low = var_g * var_i * var_j / var_k * var_l * var_m;
    kk.aa_high = var_n * var_o * var_p;
    kk.aa_x_i = bl_pow(-1.75 + 1.6 * plasma_kappa, -0.86);
    const double var_q = 14.3 * bl_pow(plasma_w, -0.928);
    const double var_r = 169.0 * bl_pow(plasma_kappa, -8.0) + 0.0052 * plasma_kappa - 0.0526 + 47.0 / (200.0 * plasma_kappa);
    kk.jj_low_q = 0.5;
    kk.jj_low_v = 0.5625 * bl_pow(plasma_kappa, -0.528) / plasma_w;
    kk.jj_high_q = 0.64 + 0.02 * plasma_kappa;
    kk.jj_high_v = 0.765625 * bl_pow(plasma_kappa, -0.44) / plasma_w;
    kk.jj_x_q = 3.7 * bl_pow(plasma_kappa, -1.6);
    kk.jj_x_v = kk.jj_x_i;
    kk.aa_low_q = 25.0 / 48.0;
    kk.aa_low_v = 77.0 / (100.0 * plasma_w) * bl_pow(plasma_kappa, -0.7);
    kk.aa_high_i = bl_pow(3.0 / plasma_kappa, 4.75) + 0.6;
    kk.aa_high_q = 441.0 * bl_pow(plasma_kappa, -5.76) + 0.55;
    kk.aa_high_v = var_q * var_r;
    kk.aa_x_q = 1.4 * bl_pow(plasma_kappa, -1.15);
    kk.aa_x_v = 1.22 * bl_pow(plasma_kappa, -1.136) + 0.007;
    kk.rho_v = bl_cyl_bessel_k(0, 1.0 / plasma_w) / bl_cyl_bessel_k(2, 1.0 / plasma_w);
    // rotativity fits at kappa = 3.5, 4, 4.5, 5 (:128-192); kappa is bracketed by two of them
    const double sqrt_w = blm_sqrt(plasma_w), exp_w = bl_exp(-5.0 * plasma_w);
    const double fit_q[4][5] = {
        {17.0 * plasma_w + sqrt_w * (-3.0 + 7.0 * exp_w), -1.0 / 30.0, 0.1, -1.5, 0.471},
        {46.0 / 3.0 * plasma_w + sqrt_w * (-5.0 / 3.0 + 17.0 / 3.0 * exp_w), -1.0 / 18.0, 1.0 / 6.0, -1.75, 0.5},
        {14.0 * plasma_w + sqrt_w * (-1.625 + 4.5 * exp_w), -1.0 / 12.0, 0.25, -2.0, 0.525},
        {12.5 * plasma_w + sqrt_w * (-1.0 + 5.0 * exp_w), -0.125, 0.375, -2.25, 0.541}};
    const double fit_v[4][2] = {
        {(plasma_w * plasma_w + 2.0 * plasma_w + 1.0) / (3.125 * plasma_w * plasma_w + 4.0 * plasma_w + 1.0), 0.447},
        {(plasma_w * plasma_w + 54.0 * plasma_w + 50.0) / (30.0 / 11.0 * plasma_w * plasma_w + 134.0 * plasma_w + 50.0), 0.391},
        {(plasma_w * plasma_w + 43.0 * plasma_w + 38.0) / (7.0 / 3.0 * plasma_w * plasma_w + 92.5 * plasma_w + 38.0), 0.348},
        {(plasma_w + 13.0 / 14.0) / (2.0 * plasma_w + 13.0 / 14.0), 0.313}};
    const int lo = plasma_kappa < 4.0 ? 0 : (plasma_kappa < 4.5 ? 1 : 2);
    const double k_lo = 3.5 + 0.5 * lo, k_hi = 4.0 + 0.5 * lo;
    kk.rho_frac = (plasma_kappa - k_lo) / (k_hi - k_lo);
    for (int c = 0; c < 5; c++) {
      kk.rho_q_low[c] = fit_q[lo][c];
      kk.rho_q_high[c] = fit_q[lo + 1][c];
    }
    for (int c = 0; c < 2; c++) {
      kk.rho_v_low[c] = fit_v[lo][c];
      kk.rho_v_high[c] = fit_v[lo + 1][c];
    }
  }
  return ec;
}

// ---- the locate / coefficient kernels'
void BuildShadeArgs(RenderJob &job) {
  bl_ctx *ctx = job.ctx;
  const bl_params &p = ctx->params;
  hipStream_t stream = ctx->stream;
  BlShadeArgs &sa = job.sa;
  sa.st = ctx->st;
  BlShadeCold cold;
  std::memset(static_cast<void *>(&cold), 0, sizeof cold);   // (padding too: the block is compared byte for byte below)
  cold.omit_near = p.cut_omit_near;
  cold.omit_far = p.cut_omit_far;
  cold.plane = p.cut_plane;
  cold.omit_in = p.cut_omit_in;
  cold.omit_out = p.cut_omit_out;
  cold.midplane_theta = p.cut_midplane_theta;
  cold.midplane_z = p.cut_midplane_z;
  cold.plane_origin[0] = p.cut_plane_origin_x;
  cold.plane_origin[1] = p.cut_plane_origin_y;
  cold.plane_origin[2] = p.cut_plane_origin_z;
  cold.plane_normal[0] = p.cut_plane_normal_x;
  cold.plane_normal[1] = p.cut_plane_normal_y;
  cold.plane_normal[2] = p.cut_plane_normal_z;
  for (int mu = 0; mu < 4; mu++) cold.cam_x[mu] = ctx->frame.cam_x[mu];
  sa.cuts.camera_r = p.camera_r;
  sa.cuts.any_optional = GeometricCut(p) ? 1 : 0;
  sa.plasma.fallback_nan = p.fallback_nan;   // (formula mode too: a flagged ray's coefficients are NaN there as well, formula_coefficients.cpp:51-59)
  if (job.simulation) {
    BlPlasmaDevice &pl = sa.plasma;
    pl.plasma_mu = p.plasma_mu;
    pl.plasma_ne_ni = p.plasma_ne_ni;
    pl.plasma_rat_low = job.base_rat_low;     // (the render's base, PlanJob; BindVariant each variant's)
    pl.plasma_rat_high = job.base_rat_high;
    FoldUnits(ctx, job.base_rho, MixThermal(job, job.base_mix), pl, sa.fast_k);            // simulation_coefficients.cpp:237-239
    const ElectronConstants ec = FillElectronConstants(job.base_mix, ctx->polarized);   // (the render's: PlanJob; BindVariant each pass's)
    BindElectronConstants(ec, ctx->polarized, pl, sa);
    cold.kappa = ec.kappa;
    cold.plasma_gamma = ctx->grid.meta.plasma_gamma;
    cold.plasma_gamma_i = ctx->grid.meta.plasma_gamma_i;
    cold.plasma_gamma_e = ctx->grid.meta.plasma_gamma_e;
    pl.plasma_use_p = p.plasma_use_p;
    pl.simulation_interp = p.simulation_interp;
    // fmks: the reader has put vectors on the spherical Kerr-Schild basis; everything but the cell search treats the
    // grid as sks (radiation_geometry.cpp:39, :94, :460, :541)
    pl.simulation_coord = p.simulation_coord == BL_COORD_FMKS ? BL_COORD_SKS : p.simulation_coord;
    pl.fallback_nan = p.fallback_nan;
    cold.fallback_rho = p.fallback_nan ? 0.0f : p.fallback_rho;
    cold.fallback_pgas = p.fallback_nan ? 0.0f : p.fallback_pgas;
    cold.fallback_kappa = p.fallback_nan ? 0.0f : p.fallback_kappa;
    pl.code_kappa = p.plasma_model == BL_PLASMA_CODE_KAPPA ? 1 : 0;
    // cell cuts (simulation_coefficients.cpp:361-375): "cut >= 0 and value < cut". A disabled threshold goes to the
    // device as -inf (lower) / +inf (upper), against which no value - NaN included - compares true: same
    // decisions, one compare per threshold
    const double kInf = std::numeric_limits<double>::infinity();
    auto lower = [&](double cut) { return cut >= 0.0 ? cut : -kInf; };
    auto upper = [&](double cut) { return cut >= 0.0 ? cut : kInf; };
    cold.cut_rho_min = lower(p.cut_rho_min); cold.cut_rho_max = upper(p.cut_rho_max);
    cold.cut_n_e_min = lower(p.cut_n_e_min); cold.cut_n_e_max = upper(p.cut_n_e_max);
    cold.cut_p_gas_min = lower(p.cut_p_gas_min); cold.cut_p_gas_max = upper(p.cut_p_gas_max);
    cold.cut_theta_e_min = lower(p.cut_theta_e_min); cold.cut_theta_e_max = upper(p.cut_theta_e_max);
    cold.cut_b_min = lower(p.cut_b_min); cold.cut_b_max = upper(p.cut_b_max);
    cold.cut_sigma_min = lower(p.cut_sigma_min); cold.cut_sigma_max = upper(job.base_sigma_max);   // (the render's: PlanJob)
    cold.cut_beta_inverse_min = lower(p.cut_beta_inverse_min); cold.cut_beta_inverse_max = upper(p.cut_beta_inverse_max);
    {
      const double cuts[14] = {p.cut_rho_min, p.cut_rho_max, p.cut_n_e_min, p.cut_n_e_max, p.cut_p_gas_min, p.cut_p_gas_max,
                               p.cut_theta_e_min, p.cut_theta_e_max, p.cut_b_min, p.cut_b_max, p.cut_sigma_min, job.base_sigma_max,
                               p.cut_beta_inverse_min, p.cut_beta_inverse_max};
      pl.cut_mask = 0;
      pl.any_cell_cut = 0;
      for (int c = 0; c < 14; c++) {
        const bool active = cuts[c] >= 0.0;
        if (active) pl.cut_mask |= 1 << c;
        if (active) pl.any_cell_cut = 1;
      }
      FoldFastCuts(ctx, pl, cold, job.base_sigma_max);   // (the fast kernels' thresholds in code units)
      // Sigma cuts in one pass: the guard band of every threshold, folded as FoldFastCuts folds one (sigma has no unit); a
      // switched-off threshold has an empty band
      sa.n_sigma_bands = 0;
      if (job.variants_one_pass && job.variants.n_cuts >= 2) {
        static_assert(BL_SHADE_MAX_SIGMA_CUTS == BL_MAX_SIGMA_CUTS, "sigma cut bands");
        sa.n_sigma_bands = job.variants.n_cuts;
        for (int s = 0; s < job.variants.n_cuts; s++) {
          const double cut = job.variants.list[s].sigma_max;   // (the first (model, unit)'s variants are the cuts)
          sa.sigma_band_lo[s] = cut >= 0.0 ? cut * (1.0 - ctx->guard_band) : kInf;
          sa.sigma_band_hi[s] = cut >= 0.0 ? cut * (1.0 + ctx->guard_band) : -kInf;
        }
      }
      sa.fast_angle_band = std::max(1.0e-12, ctx->guard_band > 1.0e-8 ? ctx->guard_band : 0.0);   // (the debug switch widens both kinds of band)
    }
    sa.grid = ctx->grid.dev;
    sa.lds_table_bytes = ctx->grid.tables.lds_table_bytes;
    sa.undefined_edge = (ctx->undefined_policy & BL_UNDEFINED_EDGE) ? 1 : 0;
    // Polarized runs in the tolerant tier keep the exact tier's per-frequency coefficient kernel: the reference's polarized step
    // amplifies last-place differences of the coefficients by up to ten orders of magnitude in optically and Faraday thick
    // configurations (docs/notebook.md section 5h), so only bit-identical coefficients keep Stokes V within the tier's tolerance
    // everywhere. The tolerant coefficient kernel (106 -> 59 ms per 1024^2 frame) is there for the asking.
    sa.tolerant = job.fast ? 1 : 0;
  } else {
    BlFormulaDevice &fm = sa.formula;
    fm.r0 = p.formula_r0; fm.h = p.formula_h; fm.l0 = p.formula_l0; fm.q = p.formula_q; fm.nup = p.formula_nup;
    fm.cn0 = p.formula_cn0; fm.alpha = p.formula_alpha; fm.a = p.formula_a; fm.beta = p.formula_beta;
  }
  sa.samples_renormalised = job.geo_load ? 1 : 0;
  sa.general_locate = (ctx->switches & BL_SWITCH_GENERAL_LOCATE) ? 1 : 0;
  sa.local_angles = job.local_angles ? 1 : 0;
  sa.general_cuts = (ctx->switches & BL_SWITCH_GENERAL_CUTS) ? 1 : 0;
  // One block per (unit, sigma cut) where the passes of two units or more compare their own cut thresholds and those of two cuts or
  // more their own cut_sigma_max (job.n_cold; BindVariant points at its variant's): the render's block with the thresholds refolded,
  // byte for byte otherwise
  std::vector<unsigned char> colds(job.n_cold * sizeof(BlShadeCold));
  for (int b = 0; b < job.n_cold; b++) {
    std::memcpy(colds.data() + b * sizeof(BlShadeCold), &cold, sizeof(BlShadeCold));
    if (job.n_cold > 1) {
      // (the first mix's and model's variant of the block's unit and cut)
      const int u = job.cold_units > 1 ? b / job.cold_cuts : 0, s = job.cold_cuts > 1 ? b % job.cold_cuts : 0;
      const Variant &variant = job.variants.list[job.variants.Index(0, 0, u, s)];
      BlShadeCold unit_cold;
      std::memcpy(static_cast<void *>(&unit_cold), &cold, sizeof(BlShadeCold));
      BlPlasmaDevice unit_pl = sa.plasma;
      double unit_k[8];
      FoldUnits(ctx, job.cold_units > 1 ? variant.rho : job.base_rho, ctx->plasma_thermal_frac, unit_pl, unit_k);   // (unit_k is not read)
      const double sigma_max = job.cold_cuts > 1 ? variant.sigma_max : job.base_sigma_max;
      unit_cold.cut_sigma_max = sigma_max >= 0.0 ? sigma_max : std::numeric_limits<double>::infinity();
      FoldFastCuts(ctx, unit_pl, unit_cold, sigma_max);
      if (job.variants.n_pol > 0) unit_cold.kappa = FillElectronConstants(variant.mix, ctx->polarized).kappa;   // (polarized variants: the pass's mix)
      std::memcpy(colds.data() + b * sizeof(BlShadeCold), &unit_cold, sizeof(BlShadeCold));
    }
  }
  // (uploaded when it differs from what the device holds: a frame loop uploads it once and waits for nothing here)
  if (ctx->shade_cold_host != colds) {
    ctx->d_shade_cold.Ensure(job.n_cold);
    ctx->shade_cold_host.clear();   // (what the device holds is unknown until the copy has completed)
    Check(hipMemcpyAsync(ctx->d_shade_cold.ptr, colds.data(), colds.size(), hipMemcpyHostToDevice, stream), "shade parameter upload");
    Check(hipStreamSynchronize(stream), "shade parameter upload");
    ctx->shade_cold_host = colds;
  }
  sa.cold = ctx->d_shade_cold.ptr;
  // Polarized variants in one pass: every triple folded as the render's own is (FoldUnits), for bl_polarized_coefficients_kernel
  sa.pol_variants = 0;
  sa.pol_variant_table = nullptr;
  if (job.pol_one_pass) {
    static_assert(BL_POL_MAX_VARIANTS == BL_MAX_POLARIZED_VARIANTS, "variant constants");
    std::vector<BlPolVariant> table;
    for (const Variant &variant : job.variants.list) {
      BlPlasmaDevice variant_pl = sa.plasma;
      double variant_k[8];
      variant_pl.plasma_rat_low = variant.rat_low;
      variant_pl.plasma_rat_high = variant.rat_high;
      FoldUnits(ctx, variant.rho, ctx->plasma_thermal_frac, variant_pl, variant_k);
      // (the variant's threshold where the shared pass ran with the sigma upper cut off - PlanVariantCuts - else +inf: nothing to compare)
      const bool cut_here = job.base_sigma_max < 0.0 && variant.sigma_max >= 0.0;
      table.push_back(BlPolVariant{variant_pl.d_unit, variant_pl.e_unit, variant_pl.b_unit, variant_pl.plasma_rat_high, variant_pl.plasma_rat_low,
                                   cut_here ? variant.sigma_max : std::numeric_limits<double>::infinity()});
    }
    // (uploaded when it differs from what the device holds, as the cold block above: a fit's renders wait here only when their units change)
    std::vector<unsigned char> bytes(table.size() * sizeof(BlPolVariant));
    std::memcpy(bytes.data(), table.data(), bytes.size());
    if (ctx->pol_variant_host != bytes) {
      ctx->d_pol_variant_table.Ensure(BL_POL_MAX_VARIANTS);
      ctx->pol_variant_host.clear();
      Check(hipMemcpyAsync(ctx->d_pol_variant_table.ptr, bytes.data(), bytes.size(), hipMemcpyHostToDevice, stream), "variant table upload");
      Check(hipStreamSynchronize(stream), "variant table upload");
      ctx->pol_variant_host = bytes;
    }
    sa.pol_variants = job.variants.n_pol;
    sa.pol_variant_table = ctx->d_pol_variant_table.ptr;
  }
  // ... and, unless every electron is thermal, every variant's electron constants in a copy of the argument block with a BlShadeCold
  // of its own behind it (BlPolVariantArgs), uploaded like the table above when its bytes differ from what the device holds
  sa.pol_variant_args = nullptr;
  if (job.pol_one_pass && !job.all_thermal) {
    ctx->d_pol_variant_args.Ensure(BL_POL_MAX_VARIANTS);   // (before the elements are made: each holds the device address of its own `cold`)
    std::vector<unsigned char> bytes(job.variants.list.size() * sizeof(BlPolVariantArgs), 0);
    for (size_t v = 0; v < job.variants.list.size(); v++) {
      BlPolVariantArgs *at = reinterpret_cast<BlPolVariantArgs *>(bytes.data() + v * sizeof(BlPolVariantArgs));
      const ElectronConstants variant_ec = FillElectronConstants(job.variants.list[v].mix, ctx->polarized);
      at->args.plasma = sa.plasma;
      BindElectronConstants(variant_ec, ctx->polarized, at->args.plasma, at->args);
      at->cold.kappa = variant_ec.kappa;
      at->args.cold = &ctx->d_pol_variant_args.ptr[v].cold;
    }
    if (ctx->pol_variant_args_host != bytes) {
      ctx->pol_variant_args_host.clear();
      Check(hipMemcpyAsync(ctx->d_pol_variant_args.ptr, bytes.data(), bytes.size(), hipMemcpyHostToDevice, stream), "variant electron constants upload");
      Check(hipStreamSynchronize(stream), "variant electron constants upload");
      ctx->pol_variant_args_host = bytes;
    }
    sa.pol_variant_args = ctx->d_pol_variant_args.ptr;
  }
  sa.frequencies = ctx->d_freq.ptr;
  sa.n_nu = job.n_nu;
  sa.ray_max_steps = job.max_steps;
  sa.x_unit = kGGMsun * ctx->frame.mass_msun / (kC * kC);   // unpolarized.cpp:42
  sa.aux_need_coefficients = (p.image_light || p.image_emission || p.image_tau || ctx->aux_images.image_emission_ave
                              || ctx->aux_images.image_tau_int) ? 1 : 0;   // simulation_coefficients.cpp:389
  sa.aux_need_length = (ctx->aux_images.image_length || job.fill_present) ? 1 : 0;
  sa.aux_record_unused = job.rows_only ? 1 : 0;
  for (int mu = 0; mu < 4; mu++) sa.cam_x[mu] = ctx->frame.cam_x[mu];
  sa.tag_in_record = job.fast ? 1 : 0;
  sa.freq_split = job.freq_split ? (job.variants_one_pass ? 2 : 1) : 0;
  sa.coef_split = job.coef_split ? 1 : 0;
  sa.redo_capacity = job.use.redo ? job.redo_capacity : 0;
  sa.row_add = job.mirror ? static_cast<unsigned int>(job.record_capacity) : 0u;   // (at most 2^31: PlanScratch)

  job.snapshot_time = job.slow ? p.slow_t_start + p.slow_dt * ctx->snapshot : 0.0;   // simulation_reader.cpp:214
  if (job.slow) {
    const int chunk_size = p.slow_chunk_size;
    std::vector<unsigned long long> table(3 * static_cast<size_t>(chunk_size) + 4, 0ull);
    for (int n = 0; n < chunk_size; n++) {
      const bl_ctx::SlowSlice &slice = ctx->slow_slices[n];
      table[n] = reinterpret_cast<unsigned long long>(slice.cells.ptr);
      table[chunk_size + n] = reinterpret_cast<unsigned long long>(slice.kappa.ptr);
      std::memcpy(&table[2 * static_cast<size_t>(chunk_size) + n], &slice.time, sizeof(double));
    }
    ctx->d_slow_table.Ensure(table.size());
    Check(hipMemcpy(ctx->d_slow_table.ptr, table.data(), table.size() * sizeof(unsigned long long), hipMemcpyHostToDevice), "slow-light table upload");
    ctx->d_ray_extrap.Ensure(job.n_rays);
    Check(hipMemsetAsync(ctx->d_ray_extrap.ptr, 0, job.n_rays * sizeof(unsigned int), stream), "slow-light flags reset");
    sa.slow.n = chunk_size;
    sa.slow.interp = p.slow_interp ? 1 : 0;
    sa.slow.snapshot_time = job.snapshot_time;
    sa.slow.cells = reinterpret_cast<const float *const *>(ctx->d_slow_table.ptr);
    sa.slow.kappa = reinterpret_cast<const float *const *>(ctx->d_slow_table.ptr + chunk_size);
    sa.slow.times = reinterpret_cast<const double *>(ctx->d_slow_table.ptr + 2 * static_cast<size_t>(chunk_size));
    sa.slow.extrap_max = ctx->d_slow_table.ptr + 3 * static_cast<size_t>(chunk_size);
  }
  // Locate kernel: 256-thread workgroups. Alone it runs 4 waves per SIMD; beside the next chunk's geodesic kernel
  // (bl_set_overlap) one workgroup per CU, so that whichever of the two kernels is dispatched first cannot fill the
  // register file and lock the other out.
  job.locate_grid_alone = ctx->num_cus * 4 * 4;
  job.locate_grid_shared = ctx->num_cus;
  job.shade_grid = ctx->num_cus * 2 * 4;  // 256-thread workgroups, 2 waves per SIMD, x4 for tail balance
}

// ---- the transfer kernels'
void BuildTransferArgs(RenderJob &job) {
  bl_ctx *ctx = job.ctx;
  const bl_params &p = ctx->params;
  BlTransferArgs &xa = job.xa;
  xa.frequencies = ctx->d_freq.ptr;
  xa.n_nu = job.n_nu;
  xa.ray_max_steps = job.max_steps;
  xa.fallback_nan = p.fallback_nan;
  xa.model_type = p.model_type;
  xa.affine = (job.fast || job.fast_formula) ? 1 : 0;
  xa.lane_transfer = (ctx->switches & BL_SWITCH_LANE_TRANSFER) ? 1 : 0;
  xa.n_rays_total = job.n_rays;
  xa.mirror_rays = job.mirror ? static_cast<int>(job.n_traced) : 0;
  xa.row_add = job.mirror ? static_cast<long long>(job.record_capacity) : 0;
  xa.mirror_out_index = job.mirror ? ctx->d_mirror_out.ptr : nullptr;
  xa.image = job.image;
  xa.n_models = 0;
  xa.n_units = 0;
  xa.n_cuts = 0;
  xa.n_mixes = 0;
  xa.pol_variants = job.pol_one_pass ? job.variants.n_pol : 0;
  xa.pol_variant_rows = job.n_q_model;
  if (job.variants_one_pass) {   // every model's R_high / R_low folded as BuildShadeArgs folds the parameter block's (fast_k[1..3])
    static_assert(BL_TRANSFER_MAX_MODELS == BL_MAX_ELECTRON_MODELS, "model constants");
    static_assert(BL_TRANSFER_MAX_UNITS == BL_MAX_DENSITY_UNITS, "unit constants");
    const bool use_p = p.plasma_use_p != 0;
    const double g1 = use_p ? 1.0 : 1.0 / (ctx->grid.meta.plasma_gamma_i - 1.0);
    const double g2 = use_p ? 1.0 : 1.0 / (ctx->grid.meta.plasma_gamma_e - 1.0);
    const Variants &vs = job.variants;
    // (an axis' table: of the variants that lie at 0 on every other axis - Variants::Index)
    xa.n_models = vs.extent.m;   // (no models set: the parameter block's pair is model 0)
    for (int m = 0; m < xa.n_models; m++) {
      xa.model_k1[m] = vs.list[vs.Index(0, m, 0, 0)].rat_high * g1;
      xa.model_k2[m] = vs.list[vs.Index(0, m, 0, 0)].rat_low * g1;
    }
    xa.model_k3 = p.plasma_ne_ni * g2;
    // Two units or more: the rows hold base_rho's x at unit frequency (1 / b_unit: x = nu / nu_s, nu_s ~ nu_c ~ |b| b_unit) and s_j
    // (d_unit b_unit: n_e nu_c); unit u scales them by b_unit(base) / b_unit(u) and d_u b_unit(u) / (d_base b_unit(base)), with the
    // units of FoldUnits. (One unit is base_rho itself: the rows are that unit's.)
    if (vs.n_units >= 2) {
      BlPlasmaDevice base{}, unit{};
      double k[8];
      FoldUnits(ctx, job.base_rho, ctx->plasma_thermal_frac, base, k);   // (k is not read)
      xa.n_units = vs.n_units;
      for (int u = 0; u < vs.n_units; u++) {
        FoldUnits(ctx, vs.list[vs.Index(0, 0, u, 0)].rho, ctx->plasma_thermal_frac, unit, k);
        xa.unit_x[u] = base.b_unit / unit.b_unit;
        xa.unit_j[u] = (unit.d_unit * unit.b_unit) / (base.d_unit * base.b_unit);
      }
    }
    // Two sigma cuts or more: the rows carry every sample's sigma (the coefficient kernels ran with the upper cut off); cut s leaves
    // out the samples with sigma > sigma_max[s], +inf where it is switched off
    if (vs.n_cuts >= 2) {
      static_assert(BL_TRANSFER_MAX_CUTS == BL_MAX_SIGMA_CUTS, "sigma cut constants");
      xa.n_cuts = vs.n_cuts;
      for (int c = 0; c < vs.n_cuts; c++) {
        const double sigma_max = vs.list[vs.Index(0, 0, 0, c)].sigma_max;
        xa.sigma_max[c] = sigma_max >= 0.0 ? sigma_max : std::numeric_limits<double>::infinity();
      }
    }
    // Two electron mixes or more: the rows hold a thermal fraction of 1 (PlanJob); of mix e what FillElectronConstants gives of it,
    // folded with the products of fast_k - at base_rho, thermal fraction 1: the rows' - that turn a row into the power-law terms
    // (bl_transfer_freq_kernel has the algebra)
    if (vs.n_mixes >= 2) {
      static_assert(BL_TRANSFER_MAX_MIXES == BL_MAX_ELECTRON_MIXES, "mix constants");
      xa.n_mixes = vs.n_mixes;
      constexpr double kPlanck = 6.62607015e-27;   // (the kernels' kH, bl_kernel_util.h: the rows' q1.x is kH s_nu)
      BlPlasmaDevice base{};
      double k[8];
      FoldUnits(ctx, job.base_rho, 1.0, base, k);
      xa.power_k0 = 1.0 / (k[4] * k[7]);
      for (int e = 0; e < vs.n_mixes; e++) {
        const ElectronConstants ec = FillElectronConstants(vs.list[vs.Index(e, 0, 0, 0)].mix, false);
        const bool power = ec.power_frac != 0.0;   // (else p, power_jj and power_aa are not defined: zeros, which the kernel selects past)
        xa.mix_thermal[e] = ec.thermal_frac;
        xa.mix_power_frac[e] = ec.power_frac;
        xa.mix_pw_e[e] = power ? -(ec.plasma_p - 1.0) * 0.5 : 0.0;
        xa.mix_pw_j[e] = power ? ec.power_frac * ec.power_jj * (kE * kE * k[6] * k[7] / (kC * k[5])) : 0.0;
        xa.mix_pw_a[e] = power ? ec.power_frac * ec.power_aa * (kE * kE * k[6] * k[7] / (kMe * kC * kPlanck * k[5])) : 0.0;
      }
    }
  }
  xa.out_sample_num = job.out_num;
  xa.out_flags = job.out_flags;
  xa.aux_images = ctx->aux_images;
  xa.aux_images.polarized_rows_only = job.rows_only ? 1 : 0;
  xa.x_unit = kGGMsun * ctx->frame.mass_msun / (kC * kC);
  xa.t_unit = xa.x_unit / kC;   // unpolarized.cpp:43
  xa.render_params = ctx->render_num_images > 0 ? ctx->d_render_params.ptr : nullptr;
  xa.render = job.render_out;
  if (ctx->polarized) {
    xa.camera_pos = job.cam_pos;
    xa.camera_dir = job.cam_dir;
    xa.st = ctx->st;
    xa.simulation_coord = p.simulation_coord == BL_COORD_FMKS ? BL_COORD_SKS : p.simulation_coord;
    xa.rotation_split = p.image_rotation_split ? 1 : 0;
    for (int mu = 0; mu < 4; mu++) {
      xa.cam_u_con[mu] = ctx->frame.u_con[mu];
      xa.cam_u_cov[mu] = ctx->frame.u_cov[mu];
      xa.cam_vert_con_c[mu] = ctx->frame.vert_con_c[mu];
    }
    xa.cameras = job.ta.cameras;   // (several cameras: each ray's own - BuildTraceArgs made the table)
    xa.pixel_map = job.ta.pixel_map;
    xa.pixels_per_camera = job.ta.pixels_per_camera;
  }
}

// Point the three argument blocks at scratch set k and at the rays [begin, begin + rays)
void BindChunk(RenderJob &job, int k, long long begin, int rays) {
  bl_ctx *ctx = job.ctx;
  bl_ctx::ChunkSlot &sl = ctx->slot[k];
  const ArrayUse &use = job.use;
  BlTraceArgs &ta = job.ta;
  BlShadeArgs &sa = job.sa;
  BlTransferArgs &xa = job.xa;
  ta.chunk_begin = begin;
  ta.chunk_rays = rays;
  // The halves of a sample record (position + id | momentum + length): side by side in one array where every reader wants both
  // (the fused tolerant kernel: 64 contiguous bytes per lane for the geodesic kernel's scattered stores), in two arrays where
  // the locate kernel reads positions only
  // (kept layout: the chunk's records start at chunk_base in the store; every index the kernels see - record slots, ray_offset rows,
  // counters - stays relative to the chunk, so the shading arrays are the same one-chunk arrays for every chunk)
  ta.record_stride = job.interleaved ? 2 : 1;
  if (job.kept || job.reuse_chunks) {
    const bl_ctx::ResidentGeodesics::Segment &seg = job.segments[job.chunk_segment];
    const size_t base = job.chunk_base;
    ta.records_hot = seg.hot + base * ta.record_stride;
    ta.records_cold = job.interleaved ? reinterpret_cast<BlSampleCold *>(ta.records_hot + 1) : seg.cold + base;
    ta.sample_t = use.sample_t ? seg.sample_t + base : nullptr;
  } else {
    ta.records_hot = sl.d_records_hot.ptr;
    ta.records_cold = job.interleaved ? reinterpret_cast<BlSampleCold *>(sl.d_records_hot.ptr + 1) : sl.d_records_cold.ptr;
    ta.sample_t = use.sample_t ? sl.d_sample_t.ptr : nullptr;
  }
  ta.record_capacity = static_cast<long long>(job.chunk_capacity);
  ta.record_gate = job.chunk_gate;
  ta.counters = sl.d_counters.ptr;
  ta.ray_constants = ctx->rays.constants.ptr + begin;
  ta.ray_sample_num = ctx->rays.sample_num.ptr + begin;
  ta.ray_skipped = job.skip_shell ? ctx->rays.skipped.ptr + begin : nullptr;
  ta.segment_rows = job.composed ? 1 : 0;
  ta.ray_rows = job.composed ? ctx->rays.rows.ptr + begin : nullptr;
  ta.parked = use.parked ? sl.d_parked.ptr : nullptr;
  ta.split_b_lo = ta.split_b_hi = 0.0;
  if (job.split_long) {
    ta.split_b_lo = job.split_b_lo;
    ta.split_b_hi = job.split_b_hi;
  }
  ta.park_capacity = static_cast<int>(std::min<size_t>(job.park_capacity, 0x7fffffff));
  ta.park_below = 0;           // (a wave parks its rays once the queue is dry and none of its lanes holds ... see bl_geodesic.hip; the
  ta.park_after = 0;           //  other thresholds were measurement knobs of rounds 4 and 5, left at the values that won)
  ta.park_quiet = 1 << 30;
  ta.park_age = job.max_steps / 8;
  ta.quad_first_round = ctx->num_cus * 4;
  ta.park_always = (job.park && (ctx->switches & BL_SWITCH_QUAD_EVERY_RAY)) ? 1 : 0;
  ta.distance_mode = job.kernels.geodesic.distance != KernelPlan::Geodesic::kClosed ? 0 : ((ctx->switches & BL_SWITCH_WIDE_DISTANCE_BAND) ? 2 : 1);
  ta.xcd_state = use.xcd ? sl.d_xcd_state.ptr : nullptr;
  ta.xcd_lists = use.xcd ? sl.d_xcd_lists.ptr : nullptr;
  ta.xcd_list_capacity = use.xcd ? static_cast<long long>(job.record_capacity / 64 + 1) : 0;
  ta.ray_flags = ctx->rays.flags.ptr + begin;
  ta.ray_out_index = ctx->rays.out_index.ptr + begin;
  ta.ray_offset = ctx->rays.offset.ptr + begin;
  ta.ray_start = job.geo_load ? nullptr : ctx->d_ray_start.ptr + begin;
  sa.records_hot = ta.records_hot;
  sa.records_cold = ta.records_cold;
  sa.xcd_state = ta.xcd_state;
  sa.xcd_lists = ta.xcd_lists;
  sa.xcd_list_capacity = ta.xcd_list_capacity;
  sa.record_stride = ta.record_stride;
  sa.located = use.located ? sl.d_located.ptr : nullptr;
  sa.located_tag = use.located ? sl.d_located_tag.ptr : nullptr;
  sa.freq_inputs = use.freq_inputs ? sl.d_freq_inputs.ptr : nullptr;
  sa.counters_in = sl.d_counters.ptr;
  sa.counters = sl.d_counters.ptr;
  sa.ray_constants = ta.ray_constants;
  sa.ray_offset = ta.ray_offset;
  sa.ray_flags = ta.ray_flags;
  sa.transfer = use.pol ? nullptr : sl.d_transfer.ptr;   // (with per-sample factors instead: whatever an earlier render left, never read)
  sa.composed = use.composed ? sl.d_composed.ptr : nullptr;
  sa.tau_inc = use.tau_inc ? sl.d_tau_inc.ptr : nullptr;
  sa.aux = use.aux ? sl.d_aux.ptr : nullptr;
  sa.sample_t = ta.sample_t;
  sa.coef_inputs = use.coef_inputs ? sl.d_coef_inputs.ptr : nullptr;
  sa.have_flags = use.have_flags ? sl.d_have_flags.ptr : nullptr;
  sa.anchors = use.anchors ? sl.d_anchors.ptr : nullptr;
  sa.redo_list = use.redo ? sl.d_redo.ptr : nullptr;
  if (use.slow_frac) {
    sa.slow.frac = sl.d_slow_frac.ptr;
    sa.slow.ray_extrap = ctx->d_ray_extrap.ptr + begin;
  }
  xa.chunk_rays = rays;
  xa.counters = sl.d_counters.ptr;
  double2 *pol_coeffs = use.pol_variant_coeffs ? sl.d_pol_variant_coeffs.ptr : sl.d_pol_coeffs.ptr;
  xa.transfer = use.pol ? pol_coeffs : sl.d_transfer.ptr;   // (one pass: rows_only, never read)
  xa.ja_stride = use.pol ? 4 : 1;
  xa.composed = sa.composed;
  xa.ray_rows = ta.ray_rows;
  xa.tau_inc = sa.tau_inc;
  xa.tau_row = ctx->aux_images.offset_tau;
  xa.freq_inputs = sa.freq_inputs;
  xa.ray_sample_num = ta.ray_sample_num;
  xa.ray_skipped = ta.ray_skipped;
  xa.ray_flags = ta.ray_flags;
  xa.ray_out_index = ta.ray_out_index;
  xa.ray_offset = ta.ray_offset;
  xa.ray_constants = ta.ray_constants;
  xa.stats = sl.d_counters.ptr + BL_CNT_COUNT;
  xa.aux = sa.aux;
  if (use.pol) {
    xa.pol_samples = sa.pol_samples = sl.d_pol_samples.ptr;
    xa.pol_coeffs = sa.pol_coeffs = pol_coeffs;
    xa.pol_matrix = use.pol_matrix ? sl.d_pol_matrix.ptr : nullptr;
  }
}

// ---- checkpoints: what of a chunk crosses between device and host for them (the conversions and the files: bl_checkpoint.cpp)
// LoadGeodesics(): the chunk's sample records come from the file instead of the geodesic kernel - as many of the rays
// [begin, begin + rays) as the record buffers hold. Returns how many.
long long LoadChunkFromCheckpoint(RenderJob &job, int k, long long begin, int rays) {
  bl_ctx *ctx = job.ctx;
  bl_ctx::ChunkSlot &sl = ctx->slot[k];
  const HostChunk chunk = ChunkFromCheckpoint(*ctx->checkpoint, job.d->pixel_map, begin, rays, job.record_gate);
  const unsigned long long n_loaded = chunk.hot.size(), n_taken = chunk.sample_num.size();
  auto upload = [](auto *target, const auto &rows) {
    if (!rows.empty()) Check(hipMemcpy(target, rows.data(), rows.size() * sizeof rows[0], hipMemcpyHostToDevice), "checkpoint upload");
  };
  upload(sl.d_records_hot.ptr, chunk.hot);
  upload(sl.d_records_cold.ptr, chunk.cold);
  upload(sl.d_sample_t.ptr, chunk.sample_t);
  std::vector<double2> constants(chunk.kt.size());   // (the files keep k_t and the momentum factor as two arrays)
  for (size_t q = 0; q < constants.size(); q++) constants[q] = make_double2(chunk.kt[q], chunk.factor[q]);
  upload(ctx->rays.constants.ptr + begin, constants);
  upload(ctx->rays.sample_num.ptr + begin, chunk.sample_num);
  upload(ctx->rays.flags.ptr + begin, chunk.flags);
  upload(ctx->rays.out_index.ptr + begin, chunk.out_index);
  upload(ctx->rays.offset.ptr + begin, chunk.offset);
  Check(hipMemcpy(sl.d_counters.ptr + BL_CNT_RECORDS, &n_loaded, sizeof n_loaded, hipMemcpyHostToDevice), "checkpoint upload");
  Check(hipMemcpy(sl.d_counters.ptr + BL_CNT_NEXT_RAY, &n_taken, sizeof n_taken, hipMemcpyHostToDevice), "checkpoint upload");
  return static_cast<long long>(n_taken);
}

template <typename T>
void DownloadRows(std::vector<T> *rows, const T *source, size_t count) {
  rows->resize(count);
  if (count > 0) Check(hipMemcpy(rows->data(), source, count * sizeof(T), hipMemcpyDeviceToHost), "checkpoint download");
}

// SaveGeodesics() and SaveSampling(), first halves: what a finished chunk adds to the files, brought back while scratch set k holds it
void SaveChunk(RenderJob &job, int k, long long begin, long long done) {
  if (!job.geo_save && !job.sample_save) return;
  bl_ctx *ctx = job.ctx;
  bl_ctx::ChunkSlot &sl = ctx->slot[k];
  Check(hipStreamSynchronize(ctx->stream), "kernel execution");
  unsigned long long n_written = 0;
  Check(hipMemcpy(&n_written, sl.d_counters.ptr + BL_CNT_RECORDS, sizeof n_written, hipMemcpyDeviceToHost), "checkpoint download");
  HostChunk chunk;
  std::vector<double2> constants;   // (the files keep k_t and the momentum factor as two arrays)
  DownloadRows(&constants, ctx->rays.constants.ptr + begin, done);
  chunk.kt.resize(constants.size());
  chunk.factor.resize(constants.size());
  for (size_t q = 0; q < constants.size(); q++) {
    chunk.kt[q] = constants[q].x;
    chunk.factor[q] = constants[q].y;
  }
  DownloadRows(&chunk.sample_num, ctx->rays.sample_num.ptr + begin, done);
  DownloadRows(&chunk.flags, ctx->rays.flags.ptr + begin, done);
  DownloadRows(&chunk.out_index, ctx->rays.out_index.ptr + begin, done);
  if (job.geo_save) {
    DownloadRows(&chunk.hot, sl.d_records_hot.ptr, n_written);
    DownloadRows(&chunk.cold, sl.d_records_cold.ptr, n_written);
    DownloadRows(&chunk.sample_t, sl.d_sample_t.ptr, n_written);
    AddChunkToCheckpoint(chunk, ctx->st, job.n_rays, &job.save);
  }
  if (job.sample_save) {
    std::vector<BlLocated> located;
    std::vector<unsigned long long> tags(n_written);
    std::vector<unsigned int> anchors;
    DownloadRows(&chunk.hot, job.ta.records_hot, n_written * (job.interleaved ? 2 : 1));
    DownloadRows(&located, sl.d_located.ptr, n_written);
    if (!job.fast) DownloadRows(&tags, sl.d_located_tag.ptr, n_written);
    if (job.block_interp) DownloadRows(&anchors, sl.d_anchors.ptr, n_written * 8);
    AddChunkToSampleSave(chunk, located, tags, anchors, job.interleaved, job.fast, job.block_interp, ctx->params, ctx->grid.dev, ctx->grid.tables.merged_blocks,
                         ctx->grid.tables.merged_block_at, job.n_rays, &job.sampling);
  }
}

// ... second halves, behind the last chunk
void WriteCheckpoints(RenderJob &job) {
  bl_ctx *ctx = job.ctx;
  const bl_params &p = ctx->params;
  if (job.geo_save) {
    std::vector<double> camera_pos, camera_dir;
    DownloadRows(&camera_pos, job.cam_pos, static_cast<size_t>(job.n_rays) * 4);
    DownloadRows(&camera_dir, job.cam_dir, static_cast<size_t>(job.n_rays) * 4);
    WriteGeodesicCheckpoint(p.checkpoint_geodesic_file.s, ctx->frame, ctx->frequencies.data(), job.n_nu, camera_pos, camera_dir, job.save);
  }
  if (job.sample_save) {
    WriteSampleCheckpoint(p.checkpoint_sample_file.s, job.sampling, job.block_interp, p.simulation_interp != 0);
    ctx->sample_checkpoint_saved = true;
  }
}

// ---- a chunk, first half: the geodesic stage on stream_geo into scratch set k (the set must be free)
void LaunchGeodesicStage(RenderJob &job, int k, long long begin, int rays, hipStream_t stream_geo) {
  bl_ctx *ctx = job.ctx;
  bl_ctx::ChunkSlot &sl = ctx->slot[k];
  hipEvent_t *e = SlotEvents(job, k);
  BindChunk(job, k, begin, rays);
  Check(hipMemsetAsync(sl.d_counters.ptr, 0, BL_CNT_TOTAL * sizeof(unsigned long long), stream_geo), "counter reset");
  if (job.xcd_order) Check(hipMemsetAsync(sl.d_xcd_state.ptr, 0, 4 * BL_XCD_QUEUES * sizeof(unsigned long long), stream_geo), "counter reset");
  Check(hipEventRecord(e[0], stream_geo), "event");
  job.in_flight[k].busy = true;
  job.in_flight[k].begin = begin;
  job.in_flight[k].rays = rays;
  job.in_flight[k].done = -1;
  if (job.kernels.geodesic.source == KernelPlan::Geodesic::kCheckpoint) {
    Check(hipStreamSynchronize(stream_geo), "kernel execution");   // the counters are reset before the host writes two of them
    job.in_flight[k].done = LoadChunkFromCheckpoint(job, k, begin, rays);
  } else {
    if (job.kernels.quad.split) {
      // the band's rays parked; then the two steppers side by side on disjoint compute units, and the stage ends with both
      hipEvent_t *ev = SlotEvents(job, k);
      Check(bl_launch_split_long(&job.ta, stream_geo), "split kernel launch");
      Check(hipEventRecord(ev[7], stream_geo), "event");
      Check(hipStreamWaitEvent(ctx->stream_most, ev[7], 0), "stream wait");
      Check(hipStreamWaitEvent(ctx->stream_few, ev[7], 0), "stream wait");
      // (as many waves per SIMD as the unsplit launch would have had: a wave that shares its SIMD steps its rays more slowly)
      const int per_simd = std::max(1, (std::min(job.geo_grid, (rays + 63) / 64) + ctx->num_cus * 4 - 1) / (ctx->num_cus * 4));
      const int wide_grid = std::min(std::min(job.geo_grid, (rays + 63) / 64), (ctx->num_cus - job.split_cus) * 4 * per_simd);
      const int pad = per_simd == 1 ? ctx->split_lds_pad : 0;
      Check(bl_launch_geodesic(&job.ta, job.kernels.geodesic, std::max(wide_grid, 1), ctx->stream_most, pad), "geodesic kernel launch");
      Check(bl_launch_geodesic_quad(&job.ta, job.kernels.quad, job.quad_grid, ctx->stream_few, ctx->split_lds_pad), "geodesic quad kernel launch");
      Check(hipEventRecord(ev[8], ctx->stream_most), "event");
      Check(hipEventRecord(ev[9], ctx->stream_few), "event");
      Check(hipStreamWaitEvent(stream_geo, ev[8], 0), "stream wait");
      Check(hipStreamWaitEvent(stream_geo, ev[9], 0), "stream wait");
    } else
    Check(bl_launch_geodesic(&job.ta, job.kernels.geodesic, std::min(job.geo_grid, (rays + 63) / 64), stream_geo, 0), "geodesic kernel launch");
    // the rays it parked, sixteen to a wave, a wave per SIMD (waves that find none end at once)
    if (job.kernels.quad.park) Check(bl_launch_geodesic_quad(&job.ta, job.kernels.quad, job.quad_grid, stream_geo, 0), "geodesic quad kernel launch");
  }
  Check(hipEventRecord(e[1], stream_geo), "event");
}

// ---- second half: locate, coefficients, transfer on the shading stream, counters to the host
void LaunchShadingStage(RenderJob &job, int k, bool geodesic_beside, hipStream_t stream) {
  bl_ctx *ctx = job.ctx;
  const bl_params &p = ctx->params;
  bl_ctx::ChunkSlot &sl = ctx->slot[k];
  hipEvent_t *e = SlotEvents(job, k);
  BindChunk(job, k, job.in_flight[k].begin, job.in_flight[k].rays);
  BlShadeArgs &sa = job.sa;
  BlTransferArgs &xa = job.xa;
  const KernelPlan &plan = job.kernels;
  auto coefficient_kernel = [&]() {
    // (the list walk's cursors: every pass of the coefficient kernel walks the lists from their starts)
    if (sa.xcd_state != nullptr) Check(hipMemsetAsync(sa.xcd_state + 2 * BL_XCD_QUEUES, 0, BL_XCD_QUEUES * sizeof(unsigned long long), stream), "counter reset");
    hipError_t err = hipErrorInvalidValue;
    switch (plan.shade.family) {
      case KernelPlan::Shade::kShade:
      case KernelPlan::Shade::kExact: err = bl_launch_shade(&sa, plan.shade, job.shade_grid, stream); break;
      case KernelPlan::Shade::kFast: err = bl_launch_shade_fast(&sa, plan.shade, job.shade_grid, stream); break;
      case KernelPlan::Shade::kFormulaFast: err = bl_launch_shade_formula_fast(&sa, ctx->num_cus * 4 * 4, stream); break;
      case KernelPlan::Shade::kFused2: err = bl_launch_shade_fused2(&sa, plan.shade, job.shade_grid, stream); break;
      case KernelPlan::Shade::kExact2: err = bl_launch_shade_exact2(&sa, plan.shade, job.shade_grid, stream); break;
      case KernelPlan::Shade::kPolarized2: err = bl_launch_shade_polarized2(&sa, plan.shade, job.shade_grid, stream); break;
    }
    Check(err, "coefficient kernel launch");
    if (ctx->debug_counters && job.locate_inside) bl_shade_inside_tables(&sa, plan.shade, job.shade_grid, &job.tables_inside);
    // (the exact tier's kernel over the records the tolerant kernel deferred)
    if (plan.redo.run) {
      const int redo_grid = plan.shade.family == KernelPlan::Shade::kFormulaFast ? ctx->num_cus * 4 * 4 : job.shade_grid;
      Check(bl_launch_shade_redo(&sa, plan.redo, redo_grid, stream), "coefficient kernel launch");
      if (ctx->debug_counters) bl_shade_redo_tables(&sa, plan.redo, redo_grid, &job.tables_redo);
    }
  };
  Check(hipStreamWaitEvent(stream, e[1], 0), "stream wait");
  Check(hipEventRecord(e[2], stream), "event");
  if (plan.locate.kind != KernelPlan::Locate::kNone) {
    const int locate_grid = geodesic_beside ? job.locate_grid_shared : job.locate_grid_alone;
    Check(bl_launch_locate(&sa, plan.locate, locate_grid, ctx->grid.tables.lds_table_bytes, stream), "locate kernel launch");
    if (ctx->debug_counters) {
      bl_locate_tables(&sa, plan.locate, locate_grid, ctx->grid.tables.lds_table_bytes, &job.tables_locate_last);
      if (job.tables_locate.where == TableLaunch::kNone) job.tables_locate = job.tables_locate_last;
    }
  }
  Check(hipEventRecord(e[3], stream), "event");
  for (int v = 0; v < job.variant_passes; v++) {
    if (v > 0) {   // what the shading stage adds to the chunk's counters starts again from zero (ClearShadingCounters)
      unsigned long long *c = sl.d_counters.ptr;
      Check(hipMemsetAsync(c + BL_CNT_GATHERS, 0, sizeof *c, stream), "counter reset");
      Check(hipMemsetAsync(c + BL_CNT_UNDEFINED, 0, 3 * sizeof *c, stream), "counter reset");   // (UNDEFINED, INTERP_FAILED, REDO)
      Check(hipMemsetAsync(c + BL_CNT_COUNT, 0, 12 * sizeof *c, stream), "counter reset");
    }
    BindVariant(job, v);
    coefficient_kernel();
    // (the shading stream is never the context's second one: KernelPlan::kMatricesBeside builds the matrices there, PlanKernels)
    const bool matrices_beside = plan.polarized == KernelPlan::kMatricesBeside;
    const int polcoef_grid = ctx->num_cus * 20;
    if (matrices_beside) {
      // (the frames of the samples without coefficients first: the matrices read them)
      Check(bl_launch_polarized_frames(&sa, polcoef_grid, stream), "polarized frame kernel launch");
      Check(hipEventRecord(e[10], stream), "event");
      Check(hipStreamWaitEvent(ctx->stream_geo, e[10], 0), "stream wait");
      Check(bl_launch_transport_matrices(&xa, ctx->num_cus, ctx->stream_geo), "transport matrix kernel launch");
      Check(hipEventRecord(e[11], ctx->stream_geo), "event");
    }
    if (plan.freq.polarized_coefficients) Check(bl_launch_polarized_coefficients(&sa, plan.freq, polcoef_grid, stream), "polarized coefficient kernel launch");
    if (plan.freq.polarized_frames && !matrices_beside) Check(bl_launch_polarized_frames(&sa, polcoef_grid, stream), "polarized frame kernel launch");
    if (plan.freq.coefficients_freq) Check(bl_launch_coefficients_freq(&sa, ctx->num_cus * 16, stream), "per-frequency coefficient kernel launch");
    Check(hipEventRecord(e[4], stream), "event");
    Check(bl_launch_transfer(&xa, plan.transfer, stream), "transfer kernel launch");
    if (plan.transfer.tau) Check(bl_launch_tau(&xa, stream), "optical-depth kernel launch");
    switch (plan.polarized) {
      case KernelPlan::kUnpolarized: break;
      case KernelPlan::kTensor: Check(bl_launch_transfer_polarized(&xa, stream), "polarized transfer kernel launch"); break;
      case KernelPlan::kMatrix: Check(bl_launch_transport_matrices(&xa, ctx->num_cus, stream), "polarized transfer kernel launch");   // fall through
      case KernelPlan::kMatricesBeside:
        if (matrices_beside) Check(hipStreamWaitEvent(stream, e[11], 0), "stream wait");
        Check(bl_launch_transfer_polarized_rays(&xa, stream), "polarized transfer kernel launch");
        break;
    }
  }
  Check(hipEventRecord(e[5], stream), "event");
  Check(hipMemcpyAsync(ctx->host_counters + static_cast<size_t>(k) * BL_CNT_TOTAL, sl.d_counters.ptr, BL_CNT_TOTAL * sizeof(unsigned long long),
                       hipMemcpyDeviceToHost, stream), "counter download");
  Check(hipEventRecord(e[6], stream), "event");
}

// Rays of the chunk on scratch set k that the geodesic stage covered (waits for that stage)
long long WaitGeodesicStage(RenderJob &job, int k, hipStream_t stream_geo) {
  RenderJob::InFlight &fl = job.in_flight[k];
  if (fl.done >= 0) return fl.done;
  Check(hipStreamSynchronize(stream_geo), "kernel execution");
  unsigned long long taken = 0;
  Check(hipMemcpy(&taken, job.ctx->slot[k].d_counters.ptr + BL_CNT_NEXT_RAY, sizeof taken, hipMemcpyDeviceToHost), "counter download");
  fl.done = static_cast<long long>(std::min<unsigned long long>(taken, static_cast<unsigned long long>(fl.rays)));
  return fl.done;
}

// ---- wait for the chunk on scratch set k, add its counters and times to the totals, free the set
void CollectChunk(RenderJob &job, int k) {
  bl_ctx *ctx = job.ctx;
  const bl_params &p = ctx->params;
  RenderJob::InFlight &fl = job.in_flight[k];
  if (!fl.busy) return;
  hipEvent_t *e = SlotEvents(job, k);
  Check(hipEventSynchronize(e[6]), "kernel execution");
  const unsigned long long *hc = ctx->host_counters + static_cast<size_t>(k) * BL_CNT_TOTAL;
  float ms = 0.0f;
  Check(hipEventElapsedTime(&ms, e[0], e[1]), "event time"); job.ms_geo += ms;
  Check(hipEventElapsedTime(&ms, e[2], e[3]), "event time"); job.ms_locate += ms;
  if (job.split_long && ctx->debug_counters) {
    float a = 0, b = 0, c = 0;
    (void)hipEventElapsedTime(&a, e[0], e[7]);
    (void)hipEventElapsedTime(&b, e[0], e[8]);
    (void)hipEventElapsedTime(&c, e[0], e[9]);
    std::fprintf(stderr, "split long: rays parked by %.3f ms, wide stepper done at %.3f ms, quad stepper at %.3f ms; %llu rays with b in [%.3f, %.3f] M on %d CUs\n", a, b, c, hc[BL_CNT_PARKED],
                 job.split_b_lo, job.split_b_hi, job.split_cus);
  }
  Check(hipEventElapsedTime(&ms, e[3], e[4]), "event time"); job.ms_shade += ms;
  Check(hipEventElapsedTime(&ms, e[4], e[5]), "event time"); job.ms_transfer += ms;
  fl.busy = false;
  if (fl.done < 0) fl.done = static_cast<long long>(std::min<unsigned long long>(hc[BL_CNT_NEXT_RAY], static_cast<unsigned long long>(fl.rays)));
  if (hc[BL_CNT_OVERFLOW] != 0) throw Failure{BL_E_DEVICE, "Sample record buffer overflow."};
  // (closed-form distance: a step in doubt may have emitted another number of samples than the reference's - the frame is discarded)
  job.total_undecided += job.kernels.geodesic.distance == KernelPlan::Geodesic::kClosed ? hc[BL_CNT_UNDECIDED] : 0ull;
  if (job.total_undecided != 0) throw DistanceUndecided{};
  if (hc[BL_CNT_INTERP_FAILED] != 0) throw Failure{BL_E_INPUT, "Grid interpolation failed."};   // simulation_sampling.cpp:1319
  if (hc[BL_CNT_UNDEFINED] != 0 && !(ctx->undefined_policy & BL_UNDEFINED_EDGE)) {
    if (p.simulation_coord == BL_COORD_FMKS)
      throw Failure{BL_E_UNSUPPORTED, "FMKS sampling reached the last polar zone of the last azimuthal plane (or the last entry of the "
                                      "coordinate table), where the reference reads past its arrays (simulation_sampling.cpp:405-415, "
                                      ":809-819): no defined result to reproduce. bl_set_undefined_policy(BL_UNDEFINED_EDGE) uses the edge cell instead."};
    throw Failure{BL_E_UNSUPPORTED, "Inter-block interpolation reached an upper edge of the last MeshBlock, where the reference reads past the end "
                                    "of its cell-centre arrays (simulation_sampling.cpp:520-522): no defined result to reproduce. "
                                    "bl_set_undefined_policy(BL_UNDEFINED_EDGE) mirrors the last cell centre about the block's face instead."};
  }
  job.total_undefined += hc[BL_CNT_UNDEFINED];
  job.total_records += hc[BL_CNT_RECORDS];
  // (records the rays emitted: what is left of the steppers' reservations once every ray has given back what it did not emit - less the
  // gate's mark, kGateClosed = 2^46 per refusal. The record slots above also count each wave's partly filled last block, which differs
  // from launch to launch; this does not. Zero where the records came from a checkpoint: the slots are the records there.)
  job.total_emitted += hc[BL_CNT_COMMITTED] & ((1ull << 46) - 1ull);
  job.total_gathers += hc[BL_CNT_GATHERS];
  job.total_parked += std::min<unsigned long long>(hc[BL_CNT_PARKED] + hc[BL_CNT_PARKED_YOUNG], job.park_capacity);
  if (job.fast || job.fast_formula) job.total_redo += hc[BL_CNT_REDO];   // (polarized runs use the list for something else: bl_polarized_frame_kernel)
  job.total_samples += hc[BL_CNT_COUNT + 0];
  job.total_flagged += hc[BL_CNT_COUNT + 1];
  job.max_num = std::max<unsigned long long>(job.max_num, hc[BL_CNT_COUNT + 2]);
  for (int c = 0; c < 8; c++) job.debug_counters[c] += hc[BL_CNT_DEBUG + c];
  job.n_chunks++;
}

void DownloadChunk(RenderJob &job, long long begin, long long count);
hipError_t DownloadColumns(const RenderJob &job, long long begin, long long count);

// A chunk of the rays [begin, begin + done) is complete (CollectChunk has waited for its kernels): large host outputs leave now
void ChunkOutputs(RenderJob &job, long long begin, long long done) {
  if (job.raster && job.n_slots == 1 && (job.chunk_downloads || begin + done < job.n_rays) && job.download_status.size() < 4000) {
    job.chunk_downloads = true;
    DownloadChunk(job, begin, done);
  } else if (job.chunk_downloads) {
    Check(DownloadColumns(job, begin, done), "download of a chunk's outputs");
  }
}

// ---- all chunks of the call
void RunChunks(RenderJob &job) {
  bl_ctx *ctx = job.ctx;
  hipStream_t stream = ctx->stream;
  // one scratch set: one stream, chunks back to back
  hipStream_t stream_geo = job.n_slots == 2 ? ctx->stream_geo : stream;
  hipEvent_t ev_begin = ctx->events[2 * kEventsPerChunk], ev_end = ctx->events[2 * kEventsPerChunk + 1];
  Check(hipEventRecord(ev_begin, stream), "event");                // the uploads above were queued on `stream`
  if (stream_geo != stream) Check(hipStreamWaitEvent(stream_geo, ev_begin, 0), "stream wait");
  if (job.reuse) {
    // Shade the resident records again: the per-ray rows and the records are where the stepper left them; the counters go back to
    // what they were when it ended (and when the locate kernel ended, if its samples are kept too). The caller's camera_pos /
    // camera_dir - a pure function of the pixel - are written again by the kernel that wrote them then. Kept layout: chunk by chunk,
    // each at its place in the store with its own counters, through the one-chunk shading arrays.
    bl_ctx::ChunkSlot &sl = ctx->slot[0];
    const bl_ctx::ResidentGeodesics &res = ctx->resident;
    hipEvent_t *e = SlotEvents(job, 0);
    job.chunk_segment = 0;
    job.chunk_base = 0;
    BindChunk(job, 0, 0, static_cast<int>(job.n_traced));
    if (job.cam_pos != nullptr || job.cam_dir != nullptr) Check(bl_launch_ray_init(&job.ta, job.kernels.geodesic, stream), "ray start kernel launch");
    const size_t n_kept = job.reuse_chunks ? res.chunks.size() : 1;
    for (size_t c = 0; c < n_kept; c++) {
      const long long begin = job.reuse_chunks ? res.chunks[c].begin : 0;
      const int rays = static_cast<int>(job.n_traced - begin);
      const unsigned long long *counters = job.reuse_chunks ? res.chunks[c].counters : res.counters;
      job.chunk_segment = job.reuse_chunks ? res.chunks[c].segment : 0;
      job.chunk_base = job.reuse_chunks ? res.chunks[c].record_base : 0;
      // (pinned; the second set's half: a reuse render has one set. The previous chunk's upload from it has completed: CollectChunk below.)
      unsigned long long *staged = ctx->host_counters + BL_CNT_TOTAL;
      std::memcpy(staged, counters, BL_CNT_TOTAL * sizeof(unsigned long long));
      if (!job.reuse_located)
        for (int n : {BL_CNT_GATHERS, BL_CNT_UNDEFINED, BL_CNT_INTERP_FAILED}) staged[n] = 0ull;
      Check(hipMemcpyAsync(sl.d_counters.ptr, staged, BL_CNT_TOTAL * sizeof(unsigned long long), hipMemcpyHostToDevice, stream), "counter upload");
      Check(hipEventRecord(e[0], stream), "event");
      Check(hipEventRecord(e[1], stream), "event");
      job.in_flight[0].busy = true;
      job.in_flight[0].begin = begin;
      job.in_flight[0].rays = rays;
      job.in_flight[0].done = job.reuse_chunks ? static_cast<long long>(std::min<unsigned long long>(counters[BL_CNT_NEXT_RAY], static_cast<unsigned long long>(rays)))
                                               : job.n_traced;
      const long long done = job.in_flight[0].done;
      LaunchShadingStage(job, 0, false, stream);
      SaveChunk(job, 0, begin, done);
      CollectChunk(job, 0);
      ChunkOutputs(job, begin, done);
    }
    Check(hipEventRecord(ev_end, stream), "event");
    Check(hipStreamSynchronize(stream), "kernel execution");
    return;
  }
  if (!job.geo_load) {
    // start states of every ray of the call, once (bl_ray_init_kernel; the geodesic kernel of each chunk reads its share)
    BindChunk(job, 0, 0, static_cast<int>(job.n_traced));
    Check(bl_launch_ray_init(&job.ta, job.kernels.geodesic, stream_geo), "ray start kernel launch");
  }
  const long long n_rays = job.n_traced;
  auto no_progress = []() {
    return Failure{BL_E_ARG, "Scratch budget too small: no ray fits the sample record buffers (bl_set_scratch_limit)."};
  };
  long long begin = 0;
  int kept_segment = 0;   // kept layout: where the next chunk's records start in the store
  size_t kept_base = 0;
  for (int c = 0; begin < n_rays; c++) {
    const int k = c % job.n_slots;
    const int rays = static_cast<int>(n_rays - begin);
    CollectChunk(job, k);   // the chunk that used this scratch set before (two chunks back when there are two sets)
    if (job.kept) PlaceKeptChunk(job, kept_segment, kept_base);
    LaunchGeodesicStage(job, k, begin, rays, stream_geo);
    long long done;
    if (job.n_slots == 2) {
      // Two sets: chunk c + 1's geodesic kernel is to run beside chunk c's shading, so this chunk's extent is fetched as
      // soon as its geodesic kernel ends, and its shading goes to the other stream without waiting for anything else.
      done = WaitGeodesicStage(job, k, stream_geo);
      LaunchShadingStage(job, k, begin + done < n_rays, stream);
      SaveChunk(job, k, begin, done);
    } else {
      LaunchShadingStage(job, k, false, stream);
      if (job.geo_save || job.sample_save) SaveChunk(job, k, begin, WaitGeodesicStage(job, k, stream_geo));
      CollectChunk(job, k);
      done = job.in_flight[k].done;
      if (job.kept && !job.kept_spilled) {   // (one scratch set: the counters CollectChunk read are this chunk's as its kernels left them)
        bl_ctx::ResidentGeodesics::Chunk chunk;
        chunk.begin = begin;
        chunk.segment = job.chunk_segment;
        chunk.record_base = job.chunk_base;
        std::memcpy(chunk.counters, ctx->host_counters, sizeof chunk.counters);
        job.kept_chunks.push_back(chunk);
        kept_segment = job.chunk_segment;
        kept_base = job.chunk_base + static_cast<size_t>(ctx->host_counters[BL_CNT_RECORDS]);
      }
    }
    if (done <= 0) throw no_progress();
    // (the split is planned for calls one chunk is sure to take - PlanScratch - but the band's reservations are counted twice for a
    // moment, and a frame whose rays all use every step they may can see the gate close on that: the marked rays of a second chunk
    // would be lost. Rendered again with one stepper instead.)
    if (job.split_long && done < rays) throw SplitIncomplete{};
    ChunkOutputs(job, begin, done);
    begin += done;
  }
  const int oldest = job.n_chunks % job.n_slots;   // chunks are collected in order: the next one to collect sits on this set
  for (int k = 0; k < job.n_slots; k++) CollectChunk(job, (oldest + k) % job.n_slots);
  Check(hipEventRecord(ev_end, stream), "event");
  Check(hipStreamSynchronize(stream_geo), "kernel execution");
  Check(hipStreamSynchronize(stream), "kernel execution");
}

// ---- results to the caller's host memory
// The outputs of the rays [begin, begin + count) of the call: columns of every row, device -> host, both sides with a pitch. A pinned
// destination takes the copy at the link's rate; into pageable memory the runtime stages it through a buffer of its own (~16 GB/s;
// several host threads brought nothing - measured, 4 threads 41.6 ms against 33.7 for 537 MB: the pages' first touch is what it waits for)
hipError_t DownloadColumns(const RenderJob &job, long long begin, long long count) {
  bl_ctx *ctx = job.ctx;
  const bl_render_desc *d = job.d;
  const size_t n_rays = static_cast<size_t>(job.n_rays), first = static_cast<size_t>(begin), n = static_cast<size_t>(count);
  hipError_t err = hipSuccess;
  auto rows = [&](void *dst, const void *src, size_t element, size_t n_rows) {   // [n_rows][n_rays] arrays of `element` bytes
    if (dst == nullptr || err != hipSuccess || n == 0 || n_rows == 0) return;
    size_t width = n * element, pitch = n_rays * element;
    if (width == pitch) width *= n_rows, n_rows = 1, pitch = width;   // contiguous: one long row
    err = hipMemcpy2D(static_cast<char *>(dst) + first * element, pitch, static_cast<const char *>(src) + first * element, pitch, width, n_rows, hipMemcpyDeviceToHost);
  };
  if (job.n_q > 0) rows(d->image, job.image, sizeof(double), static_cast<size_t>(job.n_q));
  rows(d->sample_num, job.out_num, sizeof(int), 1);
  rows(d->sample_flags, job.out_flags, 1, 1);
  rows(d->camera_pos, job.cam_pos, 32, 1);   // [n_rays][4]
  rows(d->camera_dir, job.cam_dir, 32, 1);
  if (ctx->render_num_images > 0) rows(d->render, job.render_out, sizeof(double), static_cast<size_t>(ctx->render_num_images) * 3);
  return err;
}

// A finished chunk's columns on their way while the next chunk renders (RenderJob::raster): a host thread of its own, since a copy into
// pageable memory blocks the thread that asks for it
void DownloadChunk(RenderJob &job, long long begin, long long count) {
  job.download_status.push_back(hipSuccess);
  hipError_t *status = &job.download_status.back();
  const RenderJob *const_job = &job;
  const int device = job.ctx->device;
  job.downloads.emplace_back([=]() {
    *status = hipSetDevice(device);
    if (*status == hipSuccess) *status = DownloadColumns(*const_job, begin, count);
  });
}

void DownloadOutputs(RenderJob &job) {
  const bl_render_desc *d = job.d;
  if (d->outputs_on_device) return;
  if (job.chunk_downloads) {   // every chunk went as it finished
    for (std::thread &t : job.downloads)
      if (t.joinable()) t.join();
    for (hipError_t e : job.download_status) Check(e, "download of a chunk's outputs");
    return;
  }
  Check(DownloadColumns(job, 0, job.n_rays), "download of the outputs");
}

// bl_stats of the call, and the reference's warning about rays that ended unexpectedly (geodesics.cpp:389-394)
void FinishStats(RenderJob &job) {
  bl_ctx *ctx = job.ctx;
  const bl_params &p = ctx->params;
  bl_stats st{};
  st.n_rays = job.n_rays;
  st.n_chunks = job.n_chunks;
  const KernelPlan &plan = job.kernels;
  st.launches_geodesic = plan.geodesic.source == KernelPlan::Geodesic::kResident ? 0 : job.n_chunks;
  st.launches_locate = plan.locate.kind != KernelPlan::Locate::kNone ? job.n_chunks : 0;
  st.geodesics_reused = job.reuse ? 1 : 0;
  st.sampling_reused = job.reuse_located ? 1 : 0;
  st.launches_shade = job.n_chunks * job.variant_passes;   // (polarized variants in one pass: the coefficient kernel once per chunk)
  st.launches_transfer = job.n_chunks * job.variant_passes;
  st.n_samples = static_cast<int64_t>(job.total_samples);
  // (mirror pairs: every record stands for two)
  st.n_samples_emitted = static_cast<int64_t>(job.total_emitted != 0 ? job.total_emitted : job.total_records) * (job.mirror ? 2 : 1);
  st.n_gathers = static_cast<int64_t>(job.total_gathers);
  st.n_flagged = static_cast<int64_t>(job.total_flagged);
  st.max_sample_num = static_cast<int32_t>(job.max_num);
  const double bytes_per_gather = (job.simulation && !p.simulation_interp) ? 32.0 : 256.0;
  st.algorithmic_bytes = bytes_per_gather * static_cast<double>(job.total_gathers) + 13.0 * static_cast<double>(job.n_rays);
  st.ms_geodesic = (job.geo_load || job.reuse) ? 0.0f : job.ms_geo;   // nothing was integrated
  st.ms_locate = job.ms_locate;
  st.ms_shade = job.ms_shade;
  st.ms_transfer = job.ms_transfer;
  st.ms_total = job.ms_geo + job.ms_locate + job.ms_shade + job.ms_transfer;
  float ms_wall = 0.0f;
  Check(hipEventElapsedTime(&ms_wall, ctx->events[2 * kEventsPerChunk], ctx->events[2 * kEventsPerChunk + 1]), "event time");
  st.ms_wall = ms_wall + job.ms_discarded;   // (a render given up for an undecided step: both)
  st.arithmetic = (job.fast || job.fast_formula || job.tolerant_polarized) ? BL_ARITH_TOLERANT : BL_ARITH_EXACT;
  st.n_deferred = static_cast<int64_t>(job.total_redo);
  st.n_undefined = static_cast<int64_t>(job.total_undefined);
  st.switches = ctx->switches;
  st.fused_variant = plan.shade.family == KernelPlan::Shade::kFused2 ? 2 : (plan.shade.family == KernelPlan::Shade::kExact2 ? 3 : (plan.shade.family == KernelPlan::Shade::kPolarized2 ? 4 : 0));
  st.n_parked = static_cast<int64_t>(job.reuse ? ctx->resident.n_parked : job.total_parked);
  st.composed_maps = job.composed ? 1 : 0;
  st.xcd_order = job.xcd_order ? 1 : 0;
  st.mirror_pairs = job.mirror ? 1 : 0;
  st.local_angles = job.local_angles ? 1 : 0;
  st.n_cameras = job.n_cameras;
  st.n_mixes = ResolveVariants(ctx).extent.e;   // (the whole list's, whichever of its mixes this render covers)
  st.tail_policy = job.reuse ? ctx->resident.tail_policy : (job.park ? BL_TAIL_QUAD : (job.split_long ? BL_TAIL_SPLIT : BL_TAIL_WIDE));
  ctx->stats = st;
  if (ctx->debug_counters) {
    static const char *const distances[] = {"none", "exact", "closed"};
    std::fprintf(stderr, "stepper: distance=%s undecided=%llu retried=%d\n", distances[plan.geodesic.distance], job.undecided_before, job.distance_retried ? 1 : 0);
  }
  if (ctx->debug_counters) {   // kernels built with -DBL_GEO_STATS fill these
    std::fprintf(stderr, "debug counters:");
    for (int k = 0; k < 8; k++) std::fprintf(stderr, " %llu", job.debug_counters[k]);
    std::fprintf(stderr, "\n");
  }
  if (job.total_flagged > 0 && !job.reuse)   // (geodesics.cpp:389-394: raised where the geodesics are integrated - once per series)
    Warn(ctx, std::to_string(job.total_flagged) + " out of " + std::to_string(job.n_rays) + " geodesics terminate unexpectedly.");
  if (job.total_undefined > 0)   // BL_UNDEFINED_EDGE (this text has no counterpart in the reference)
    Warn(ctx, std::to_string(job.total_undefined) + " samples lie where the reference reads past its arrays; the edge cell was used for them.");
}

// Slow light (simulation_sampling.cpp:553-617): pixels whose samples fall outside the window of files
void SlowLightMessages(RenderJob &job) {
  bl_ctx *ctx = job.ctx;
  const bl_params &p = ctx->params;
  const long long n_rays = job.n_rays;
  std::vector<unsigned int> flags(n_rays);
  unsigned long long maxima[4];
  Check(hipMemcpy(flags.data(), ctx->d_ray_extrap.ptr, n_rays * sizeof(unsigned int), hipMemcpyDeviceToHost), "slow-light flags download");
  Check(hipMemcpy(maxima, ctx->d_slow_table.ptr + 3 * static_cast<size_t>(p.slow_chunk_size), sizeof maxima, hipMemcpyDeviceToHost), "slow-light maxima download");
  long long count[4] = {0, 0, 0, 0};
  for (unsigned int f : flags)
    for (int e = 0; e < 4; e++) count[e] += (f >> e) & 1u;
  auto text = [&](int kind, const char *degree, const char *direction) {
    double by;
    std::memcpy(&by, &maxima[kind], sizeof(double));
    std::ostringstream message;
    message << "Snapshot " << ctx->snapshot << " at time " << job.snapshot_time << " requires " << degree << " extrapolation "
            << direction << " in time (" << count[kind] << "/" << n_rays << " pixels, by up to " << by << " gravitational times).";
    return message.str();
  };
  for (int e = 0; e < 4; e++) {
    ctx->stats_slow_count[e] = count[e];
    std::memcpy(&ctx->stats_slow_val[e], &maxima[e], sizeof(double));
  }
  if (count[1] > 0) throw Failure{BL_E_INPUT, text(1, "significant", "forward")};
  if (count[3] > 0) throw Failure{BL_E_INPUT, text(3, "significant", "backward")};
  if (count[0] > 0) Warn(ctx, text(0, "moderate", "forward"));
  if (count[2] > 0) Warn(ctx, text(2, "moderate", "backward"));
}

}  // namespace

namespace {
// BL_TAIL_SPLIT: two streams whose CU masks partition the device - bit c of a mask = compute unit c may run the stream's kernels -
// `cus` compute units for bl_geodesic_quad_kernel, the rest for bl_geodesic_kernel. False when the runtime refuses.
// The pair belongs to the PROCESS, one per (device, cus), and is never destroyed: contexts borrow it. (Destroying a CU-masked
// stream leaves its queue in the runtime's list - ROCr 7.0 as torch ships it: the next device allocation that has to trim scratch,
// GpuAgent::Trim -> AqlQueue::AsyncReclaimMainScratch, walks into it. Found by the -m gpu suite, 300 contexts into the run. Two
// contexts of one device that render at once share the pair; their kernels queue behind each other there, which orders nothing
// that the events of each call do not order already.)
bool EnsureSplitStreams(bl_ctx *ctx, int cus) {
  if (ctx->stream_few != nullptr && ctx->split_cus_made == cus) return true;
  static std::mutex table_lock;
  static std::map<std::pair<int, int>, std::pair<hipStream_t, hipStream_t>> table;
  std::lock_guard<std::mutex> guard(table_lock);
  auto found = table.find({ctx->device, cus});
  if (found == table.end()) {
    const int words = (ctx->num_cus + 31) / 32;
    std::vector<uint32_t> few(words, 0u), most(words, 0u);
    for (int c = 0; c < ctx->num_cus; c++) (c < cus ? few : most)[c / 32] |= 1u << (c % 32);
    hipStream_t stream_few = nullptr, stream_most = nullptr;
    if (hipExtStreamCreateWithCUMask(&stream_few, static_cast<uint32_t>(words), few.data()) != hipSuccess
        || hipExtStreamCreateWithCUMask(&stream_most, static_cast<uint32_t>(words), most.data()) != hipSuccess) {
      (void)hipGetLastError();
      return false;   // (a first stream that was made stays: see above)
    }
    found = table.emplace(std::make_pair(ctx->device, cus), std::make_pair(stream_few, stream_most)).first;
  }
  ctx->stream_few = found->second.first;
  ctx->stream_most = found->second.second;
  ctx->split_cus_made = cus;
  return true;
}
}  // namespace

namespace blhost {
void EnsureStreams(bl_ctx *ctx) {
  if (ctx->stream == nullptr) Check(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking), "hipStreamCreate");
  if (ctx->stream_geo == nullptr) Check(hipStreamCreateWithFlags(&ctx->stream_geo, hipStreamNonBlocking), "hipStreamCreate");
}
}  // namespace blhost

namespace {
// One render of the context as it stands, over the mixes of `mixes`, render_lock held (bl_render below)
int RenderLocked(bl_ctx *ctx, const bl_render_desc *d, MixRange mixes) {
  auto drain = [ctx]() {   // leave no chunk half collected behind: a later call starts from idle streams
    if (ctx->stream_few != nullptr) (void)hipStreamSynchronize(ctx->stream_few);
    if (ctx->stream_most != nullptr) (void)hipStreamSynchronize(ctx->stream_most);
    if (ctx->stream_geo != nullptr) (void)hipStreamSynchronize(ctx->stream_geo);
    if (ctx->stream != nullptr) (void)hipStreamSynchronize(ctx->stream);
  };
  try {
    // (planned again at most twice: without the split stepper after a chunk that closed its gate early, without the resident
    // records after scratch beside them could not be had)
    // (... and once more with the reference's proper distance after a step the closed form did not decide - a failure of its own kind)
    bool allow_split = true, allow_reuse = true, allow_closed = true;
    unsigned long long undecided_before = 0;
    float ms_discarded = 0.0f;
    for (int attempt = 0;; attempt++) {
      RenderJob job;
      job.ctx = ctx;
      job.d = d;
      job.mixes = mixes;
      job.allow_split = allow_split;
      job.allow_reuse = allow_reuse;
      job.distance_retried = !allow_closed;
      job.undecided_before = undecided_before;
      job.ms_discarded = ms_discarded;
      const auto attempt_begin = std::chrono::steady_clock::now();
      try {
        PlanJob(job);
        Check(hipSetDevice(ctx->device), "hipSetDevice");
        EnsureStreams(ctx);
        job.mirror = MirrorPairsApply(job);
        DecideReuse(job);
        if (!job.keepable) BuildReuseKeys(job);   // (the camera's key for the memory below, whether or not its records may be kept)
        job.allow_closed = allow_closed && std::find(ctx->distance_exact_keys.begin(), ctx->distance_exact_keys.end(), job.geo_key) == ctx->distance_exact_keys.end();
        PlanScratch(job);
        if (job.split_long && !EnsureSplitStreams(ctx, job.split_cus)) {
          if (ctx->tail_policy == BL_TAIL_SPLIT) throw Failure{BL_E_DEVICE, "BL_TAIL_SPLIT: the runtime gave no stream with a CU mask (hipExtStreamCreateWithCUMask)."};
          ctx->split_unavailable = true;   // BL_TAIL_AUTO: the one-stepper path, from now on
          job.split_long = false;
          job.park_capacity = 0;
          job.quad_grid = 0;
        }
        job.use = UsedArrays(job);   // (less what the plan dropped: one pass over the polarized variants, the order per XCD, parked rays)
        PlanKernels(job);
        EnsureScratch(job);
        StageInputsAndOutputs(job);
        BuildTraceArgs(job);
        BuildShadeArgs(job);
        BuildTransferArgs(job);
        RunChunks(job);
        WriteCheckpoints(job);
        DownloadOutputs(job);
        FinishStats(job);
        KeepResident(job);
        if (job.slow) SlowLightMessages(job);
        break;
      } catch (const SplitIncomplete &) {
        drain();
        if (job.keepable) DropResident(ctx);
        if (!allow_split || attempt >= 2) throw Failure{BL_E_DEVICE, "A chunk of rays ended early twice."};
        allow_split = false;
      } catch (const DistanceUndecided &) {
        // Nothing of this attempt is kept: its job's totals go with it, a closed-mode render writes no checkpoint, what its chunks
        // sent to the caller's buffers is written again, and resident records it may have left half replaced are dropped.
        drain();
        if (job.keepable) DropResident(ctx);
        if (!allow_closed) throw Failure{BL_E_DEVICE, "The exact proper distance reported an undecided step."};   // (it counts none)
        allow_closed = false;
        undecided_before = job.total_undecided;
        ms_discarded += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - attempt_begin).count();
        if (ctx->distance_exact_keys.size() >= 64) ctx->distance_exact_keys.erase(ctx->distance_exact_keys.begin());
        ctx->distance_exact_keys.push_back(job.geo_key);
      } catch (const ReuseImpossible &) {
        drain();
        (void)hipGetLastError();
        DropResident(ctx);
        if (!allow_reuse || attempt >= 2) throw Failure{BL_E_DEVICE, "Scratch memory for the render could not be allocated."};
        allow_reuse = false;
      } catch (const Failure &) {
        // (what scratch set 0 holds is no longer known to be a whole set of records)
        if (job.keepable) DropResident(ctx);
        throw;
      }
    }
  } catch (const Failure &failure) {
    drain();
    return Fail(ctx, failure);
  }
  return BL_OK;
}

// What kind of electrons a mix has, as far as the tolerant tier's choice of kernels goes: no thermal part (no tolerant kernel: the exact
// tier's), thermal electrons alone, thermal electrons and a power law
int MixKind(const bl_electron_mix &mix) { return ThermalFraction(mix) == 0.0 ? 0 : (mix.power_frac == 0.0 ? 1 : 2); }

// The renders that one bl_render call is made of: one over the whole mix list, but for the one case below.
// Electron mixes in the tolerant tier: a render chooses its kernels once, and a mix without a thermal part has none in that tier (the
// exact tier's render it, as they render a context with that mix in its block), so a list that holds such a mix beside others cannot
// share the one pass, and a mix of thermal electrons alone has other kernels (the locate step inside, the factors of several
// frequencies) than one with a power law. So that every mix's rows are then what a context with that mix in its block renders in this
// tier, such a list is split into the runs of neighbouring mixes of one kind, each a render of its own with a pass per variant.
// (The exact tier has one set of kernels for all, and a list whose mixes all have a thermal part one pass or one choice: one render.)
std::vector<MixRange> MixRuns(const bl_ctx *ctx, const bl_render_desc *d) {
  const std::vector<bl_electron_mix> &all = ctx->mixes;
  bool one_kind = true, every_thermal = true;
  for (const bl_electron_mix &mix : all) one_kind = one_kind && MixKind(mix) == MixKind(all[0]), every_thermal = every_thermal && MixKind(mix) != 0;
  if (ctx->arithmetic != BL_ARITH_TOLERANT || one_kind || every_thermal || d->image == nullptr) return {MixRange{}};
  std::vector<MixRange> runs;
  const int n = static_cast<int>(all.size());
  for (int begin = 0, end = 0; begin < n; begin = end) {
    for (end = begin + 1; end < n && MixKind(all[end]) == MixKind(all[begin]);) end++;
    runs.push_back({begin, end, true});
  }
  return runs;
}

// A run's statistics into the render's (zeros before the first run): the launches and kernel times summed over the runs, the
// tolerant tier if any run ran in it, everything else the last run's
void FoldRunStats(bl_stats &render, const bl_stats &run) {
  const bl_stats before = render;
  render = run;
  for (int32_t bl_stats::*launches : {&bl_stats::launches_geodesic, &bl_stats::launches_locate, &bl_stats::launches_shade, &bl_stats::launches_transfer})
    render.*launches += before.*launches;
  for (float bl_stats::*ms : {&bl_stats::ms_geodesic, &bl_stats::ms_locate, &bl_stats::ms_shade, &bl_stats::ms_transfer, &bl_stats::ms_total, &bl_stats::ms_wall})
    render.*ms += before.*ms;
  if (before.arithmetic == BL_ARITH_TOLERANT) render.arithmetic = BL_ARITH_TOLERANT;
}
}  // namespace

// A render is its runs (MixRuns: one, as a rule), each over its mixes of the context's list - which no render changes - into its rows
// of the image (the mixes are the outermost axis: a run's rows lie together), a later run from the resident geodesics where its
// record layout is the earlier one's. bl_stats is the runs' folded (FoldRunStats). A run that fails ends the call with its code.
extern "C" int bl_render(bl_ctx *ctx, const bl_render_desc *d) {
  if (ctx == nullptr || d == nullptr) return BL_E_ARG;
  std::lock_guard<std::mutex> render_guard(ctx->render_lock);   // (bl_set_grid on another host thread stages the next snapshot meanwhile: bl_api.hip)
  const Variants whole = ResolveVariants(ctx);
  bl_stats stats{};
  for (const MixRange &run : MixRuns(ctx, d)) {
    bl_render_desc part = *d;
    part.image = d->image + static_cast<size_t>(whole.Index(run.begin, 0, 0, 0)) * ctx->image_num_quantities * static_cast<size_t>(d->n_rays);
    if (const int rc = RenderLocked(ctx, &part, run)) return rc;
    FoldRunStats(stats, ctx->stats);
  }
  ctx->stats = stats;
  return BL_OK;
}
