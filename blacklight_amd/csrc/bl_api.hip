// bl_api.hip - C-ABI of the MI355X hot path (include/blacklight_amd.h): context, parameter
// validation in the reference's words, grid repack + upload, settings (bl_render: bl_render.hip).
//
// Host-side counterpart of the reference's GeodesicIntegrator / RadiationIntegrator constructors
// (src/geodesic_integrator/geodesic_integrator.cpp:23-157, src/radiation_integrator/
// radiation_integrator.cpp:26-541) and of their Integrate() drivers, for the configurations in the
// hot-path scope. Configurations outside it are rejected loudly (BL_E_UNSUPPORTED); nothing falls
// back to a CPU path.
#include "bl_ctx.h"
#include "bl_harm.h"

#include <optional>

namespace {

thread_local std::string g_global_error;

bool Has(const bl_params &p, int index) { return p.has[index] != 0; }

// std::optional::value() of the reference: a missing key surfaces as bad_optional_access, which
// main() reports per stage (blacklight.cpp:100-104, 147-151)
void Require(const bl_params &p, std::initializer_list<int> keys, const char *stage_message) {
  for (int key : keys)
    if (!Has(p, key)) throw Failure{BL_E_MISSING, stage_message};
}

constexpr const char *kGeoMissing = "GeodesicIntegrator unable to find all needed values in input file.";
constexpr const char *kRadMissing = "RadiationIntegrator unable to find all needed values in input file.";

// GeodesicIntegrator::GeodesicIntegrator (geodesic_integrator.cpp:23-157)
void ValidateGeodesic(bl_ctx *ctx) {
  const bl_params &p = ctx->params;
  Require(p, {BL_P_model_type, BL_P_checkpoint_geodesic_save, BL_P_checkpoint_geodesic_load}, kGeoMissing);
  if (p.checkpoint_geodesic_save && p.checkpoint_geodesic_load)
    throw Failure{BL_E_INPUT, "Cannot both save and load a geodesic checkpoint."};
  if (p.checkpoint_geodesic_save || p.checkpoint_geodesic_load) Require(p, {BL_P_checkpoint_geodesic_file}, kGeoMissing);
  Require(p, {BL_P_camera_type, BL_P_camera_r, BL_P_camera_th, BL_P_camera_ph, BL_P_camera_urn, BL_P_camera_uthn,
              BL_P_camera_uphn, BL_P_camera_k_r, BL_P_camera_k_th, BL_P_camera_k_ph, BL_P_camera_rotation,
              BL_P_camera_width, BL_P_camera_resolution, BL_P_camera_pole},
          kGeoMissing);
  if (p.camera_resolution <= 0) throw Failure{BL_E_INPUT, "Must have positive camera_resolution."};
  Require(p, {BL_P_ray_flat, BL_P_ray_terminate}, kGeoMissing);
  if (p.ray_terminate != BL_TERMINATE_PHOTON) Require(p, {BL_P_ray_factor}, kGeoMissing);
  Require(p, {BL_P_ray_integrator, BL_P_ray_step, BL_P_ray_max_steps}, kGeoMissing);
  if (p.ray_max_steps <= 0) throw Failure{BL_E_INPUT, "Must have positive ray_max_steps."};
  if (p.ray_integrator == BL_INTEGRATOR_DP) {
    Require(p, {BL_P_ray_max_retries}, kGeoMissing);
    if (p.ray_max_retries <= 0) throw Failure{BL_E_INPUT, "Must have nonnegative ray_max_retries."};
    Require(p, {BL_P_ray_tol_abs, BL_P_ray_tol_rel}, kGeoMissing);
  }
  Require(p, {BL_P_image_num_frequencies}, kGeoMissing);
  if (p.image_num_frequencies == 1) {
    Require(p, {BL_P_image_frequency}, kGeoMissing);
    if (p.image_frequency <= 0.0) throw Failure{BL_E_INPUT, "Must choose positive image_frequency."};
  } else if (p.image_num_frequencies > 1) {
    Require(p, {BL_P_image_frequency_start}, kGeoMissing);
    if (p.image_frequency_start <= 0.0) throw Failure{BL_E_INPUT, "Must choose positive image_frequency_start."};
    Require(p, {BL_P_image_frequency_end}, kGeoMissing);
    if (p.image_frequency_end <= 0.0) throw Failure{BL_E_INPUT, "Must choose positive image_frequency_end."};
    Require(p, {BL_P_image_frequency_spacing}, kGeoMissing);
  } else {
    throw Failure{BL_E_INPUT, "Must have positive image_num_frequencies."};
  }
  Require(p, {BL_P_image_normalization, BL_P_adaptive_max_level}, kGeoMissing);
  if (p.adaptive_max_level > 0) {
    Require(p, {BL_P_adaptive_block_size}, kGeoMissing);
    if (p.adaptive_block_size <= 0) throw Failure{BL_E_INPUT, "Must have positive adaptive_block_size."};
    if (p.camera_resolution % p.adaptive_block_size != 0)
      throw Failure{BL_E_INPUT, "Must have adaptive_block_size divide camera_resolution."};
  }
  // geometry (:107-123)
  ctx->st.bh_m = 1.0;
  if (p.model_type == BL_MODEL_SIMULATION) {
    Require(p, {BL_P_simulation_a}, kGeoMissing);
    ctx->st.bh_a = p.simulation_a;
  } else {
    Require(p, {BL_P_formula_spin}, kGeoMissing);
    ctx->st.bh_a = p.formula_spin;
  }
  ctx->st.ray_flat = p.ray_flat;
  bl_camera_frame &f = ctx->frame;
  f.bh_m = ctx->st.bh_m;
  f.bh_a = ctx->st.bh_a;
  f.r_horizon = f.bh_m + blm_sqrt(f.bh_m * f.bh_m - f.bh_a * f.bh_a);
  if (p.ray_terminate == BL_TERMINATE_PHOTON)
    f.r_terminate = 2.0 * f.bh_m * (1.0 + bl_cos(2.0 / 3.0 * bl_acos(-blm_abs(f.bh_a) / f.bh_m)));
  else if (p.ray_terminate == BL_TERMINATE_MULTIPLICATIVE)
    f.r_terminate = f.r_horizon * p.ray_factor;
  else
    f.r_terminate = f.r_horizon + p.ray_factor;
}

// InitializeCamera frequency list (camera.cpp:30-50)
void BuildFrequencies(bl_ctx *ctx) {
  const bl_params &p = ctx->params;
  int nf = p.image_num_frequencies;
  ctx->frequencies.assign(nf, 0.0);
  if (nf == 1) {
    ctx->frequencies[0] = p.image_frequency;
    return;
  }
  ctx->frequencies[0] = p.image_frequency_start;
  ctx->frequencies[nf - 1] = p.image_frequency_end;
  for (int l = 1; l < nf - 1; l++) {
    double frac = static_cast<double>(l) / static_cast<double>(nf - 1);
    if (p.image_frequency_spacing == BL_SPACING_LIN_FREQ)
      ctx->frequencies[l] = p.image_frequency_start + frac * (p.image_frequency_end - p.image_frequency_start);
    else if (p.image_frequency_spacing == BL_SPACING_LIN_WAVE)
      ctx->frequencies[l] = 1.0 / (1.0 / p.image_frequency_start
          + frac * (1.0 / p.image_frequency_end - 1.0 / p.image_frequency_start));
    else
      ctx->frequencies[l] = bl_exp(bl_log(p.image_frequency_start) + frac * bl_log(p.image_frequency_end / p.image_frequency_start));
  }
}

// RadiationIntegrator::RadiationIntegrator (radiation_integrator.cpp:26-541), hot-path subset
void ValidateRadiation(bl_ctx *ctx) {
  bl_params &p = ctx->params;
  const bool simulation = p.model_type == BL_MODEL_SIMULATION;
  Require(p, {BL_P_num_threads}, kRadMissing);
  if (simulation) {
    Require(p, {BL_P_checkpoint_sample_save, BL_P_checkpoint_sample_load}, kRadMissing);
    if (p.checkpoint_sample_save && p.checkpoint_sample_load)
      throw Failure{BL_E_INPUT, "Cannot both save and load a sample checkpoint."};
    if (p.checkpoint_sample_save || p.checkpoint_sample_load) Require(p, {BL_P_checkpoint_sample_file}, kRadMissing);
    if (p.checkpoint_sample_load)
      // The reference cannot read these files itself: LoadSampling() (sample_checkpoint.cpp:49-63) restores sample_inds,
      // sample_fracs, sample_nan and sample_fallback but not sample_cut, which only CalculateSimulationSampling() allocates
      // (simulation_sampling.cpp:155) and SampleSimulation() reads for every sample (:691) - the reference binary built
      // from /root/reference ends in a segmentation fault on checkpoint_sample_load = true. Loading has no defined result to
      // match and is refused; saving writes the reference's file (bl_render.hip, WriteSampleCheckpoint).
      throw Failure{BL_E_UNSUPPORTED, "checkpoint_sample_load is not offered: the reference cannot load its own sample checkpoints (its "
                                      "LoadSampling() leaves sample_cut unallocated); use geodesic checkpoints."};
    Require(p, {BL_P_simulation_format, BL_P_simulation_coord, BL_P_simulation_m_msun, BL_P_simulation_rho_cgs,
                BL_P_simulation_interp},
            kRadMissing);
    if ((p.simulation_format == BL_SIMFMT_ATHENA || p.simulation_format == BL_SIMFMT_ATHENAK) && p.simulation_interp) {
      Require(p, {BL_P_simulation_block_interp}, kRadMissing);
    } else if (Has(p, BL_P_simulation_block_interp)) {
      Warn(ctx, "Ignoring simulation_block_interp selection.");
    }
  } else {
    if (Has(p, BL_P_checkpoint_sample_save) && p.checkpoint_sample_save) Warn(ctx, "Ignoring checkpoint_sample_save selection.");
    if (Has(p, BL_P_checkpoint_sample_load) && p.checkpoint_sample_load) Warn(ctx, "Ignoring checkpoint_sample_load selection.");
    Require(p, {BL_P_formula_mass, BL_P_formula_r0, BL_P_formula_h, BL_P_formula_l0, BL_P_formula_q, BL_P_formula_nup,
                BL_P_formula_cn0, BL_P_formula_alpha, BL_P_formula_a, BL_P_formula_beta},
            kRadMissing);
  }
  Require(p, {BL_P_image_light}, kRadMissing);
  bool polarization = false;
  if (p.image_light) {
    if (simulation) {
      Require(p, {BL_P_image_polarization}, kRadMissing);
      polarization = p.image_polarization != 0;
    } else if (Has(p, BL_P_image_polarization) && p.image_polarization) {
      Warn(ctx, "Ignoring image_polarization selection.");
    }
    if (polarization) Require(p, {BL_P_image_rotation_split}, kRadMissing);
  } else if (Has(p, BL_P_image_polarization) && p.image_polarization) {
    Warn(ctx, "Ignoring image_polarization selection.");
  }
  Require(p, {BL_P_image_time, BL_P_image_length, BL_P_image_lambda, BL_P_image_emission, BL_P_image_tau}, kRadMissing);
  if (simulation) {
    Require(p, {BL_P_image_lambda_ave, BL_P_image_emission_ave, BL_P_image_tau_int}, kRadMissing);
  } else {
    if (Has(p, BL_P_image_lambda_ave) && p.image_lambda_ave) Warn(ctx, "Ignoring image_lambda_ave selection.");
    if (Has(p, BL_P_image_emission_ave) && p.image_emission_ave) Warn(ctx, "Ignoring image_emission_ave selection.");
    if (Has(p, BL_P_image_tau_int) && p.image_tau_int) Warn(ctx, "Ignoring image_tau_int selection.");
    p.image_lambda_ave = p.image_emission_ave = p.image_tau_int = 0;
  }
  Require(p, {BL_P_image_crossings}, kRadMissing);
  int render_num_images = 0;
  if (simulation) {
    Require(p, {BL_P_render_num_images}, kRadMissing);
    render_num_images = p.render_num_images;
  } else if (Has(p, BL_P_render_num_images) && p.render_num_images > 0) {
    Warn(ctx, "Ignoring request for rendering.");
  }
  if (!(p.image_light || p.image_time || p.image_length || p.image_lambda || p.image_emission || p.image_tau
        || p.image_lambda_ave || p.image_emission_ave || p.image_tau_int || p.image_crossings || render_num_images > 0))
    throw Failure{BL_E_INPUT, "No image or rendering selected."};
  // rendering parameters (radiation_integrator.cpp:146-197): every value the features need must be present
  ctx->render_num_images = render_num_images;
  for (int n_i = 0; n_i < render_num_images; n_i++) {
    if (!p.render_num_features_has[n_i]) throw Failure{BL_E_MISSING, kRadMissing};
    const int num_features = p.render_num_features[n_i];
    if (num_features <= 0) throw Failure{BL_E_INPUT, "Must have positive number of features for each rendered image."};
    for (int n_f = 0; n_f < num_features; n_f++) {
      const int has = p.render_has[n_i][n_f];
      int need = BL_RENDER_HAS_QUANTITY | BL_RENDER_HAS_TYPE | BL_RENDER_HAS_XYZ;
      if ((has & BL_RENDER_HAS_TYPE) != 0) {
        if (p.render_type[n_i][n_f] == BL_RENDER_FILL)
          need |= BL_RENDER_HAS_MIN | BL_RENDER_HAS_MAX | BL_RENDER_HAS_TAU_SCALE;
        else
          need |= BL_RENDER_HAS_THRESH | BL_RENDER_HAS_OPACITY;
      }
      if ((has & need) != need) throw Failure{BL_E_MISSING, kRadMissing};
    }
  }
  ctx->polarized = polarization;
  if (simulation) {
    Require(p, {BL_P_slow_light_on}, kRadMissing);
    if (p.slow_light_on) {   // radiation_integrator.cpp:206-215
      if ((p.has[BL_P_checkpoint_sample_save] && p.checkpoint_sample_save) || (p.has[BL_P_checkpoint_sample_load] && p.checkpoint_sample_load))
        throw Failure{BL_E_INPUT, "Cannot use sample checkpoints with slow light."};
      Require(p, {BL_P_slow_interp, BL_P_slow_chunk_size, BL_P_slow_t_start, BL_P_slow_dt}, kRadMissing);
      if (p.slow_chunk_size < 2) throw Failure{BL_E_INPUT, "Must have slow_chunk_size be at least 2."};   // simulation_reader.cpp:77
    }
  }
  if (p.adaptive_max_level > 0) {   // radiation_integrator.cpp:218-270
    if (!p.image_light) throw Failure{BL_E_INPUT, "Adaptive ray tracing requires image_light."};
    if (p.adaptive_max_level > BL_MAX_LEVELS) throw Failure{BL_E_UNSUPPORTED, "adaptive_max_level exceeds BL_MAX_LEVELS."};
    if (p.image_num_frequencies > 1) {
      Require(p, {BL_P_adaptive_frequency_num}, kRadMissing);
      if (p.adaptive_frequency_num - 1 < 0 || p.adaptive_frequency_num - 1 >= p.image_num_frequencies)
        throw Failure{BL_E_INPUT, "Must choose adaptive_frequency_num from 1 to image_num_frequencies."};
    }
    Require(p, {BL_P_adaptive_val_frac}, kRadMissing);
    if (p.adaptive_val_frac >= 0.0) Require(p, {BL_P_adaptive_val_cut}, kRadMissing);
    Require(p, {BL_P_adaptive_abs_grad_frac}, kRadMissing);
    if (p.adaptive_abs_grad_frac >= 0.0) Require(p, {BL_P_adaptive_abs_grad_cut}, kRadMissing);
    Require(p, {BL_P_adaptive_rel_grad_frac}, kRadMissing);
    if (p.adaptive_rel_grad_frac >= 0.0) Require(p, {BL_P_adaptive_rel_grad_cut}, kRadMissing);
    Require(p, {BL_P_adaptive_abs_lapl_frac}, kRadMissing);
    if (p.adaptive_abs_lapl_frac >= 0.0) Require(p, {BL_P_adaptive_abs_lapl_cut}, kRadMissing);
    Require(p, {BL_P_adaptive_rel_lapl_frac}, kRadMissing);
    if (p.adaptive_rel_lapl_frac >= 0.0) Require(p, {BL_P_adaptive_rel_lapl_cut}, kRadMissing);
    Require(p, {BL_P_adaptive_num_regions}, kRadMissing);
    for (int r = 0; r < p.adaptive_num_regions; r++)
      if (p.adaptive_region_has[r] != 31) throw Failure{BL_E_MISSING, kRadMissing};
  }
  if (simulation) {
    Require(p, {BL_P_plasma_mu, BL_P_plasma_ne_ni, BL_P_plasma_model}, kRadMissing);
    if (p.plasma_model == BL_PLASMA_TI_TE_BETA)
      Require(p, {BL_P_plasma_use_p, BL_P_plasma_rat_low, BL_P_plasma_rat_high}, kRadMissing);
    Require(p, {BL_P_plasma_power_frac}, kRadMissing);
    if (p.plasma_power_frac < 0.0 || p.plasma_power_frac > 1.0) Warn(ctx, "Fraction of power-law electrons outside [0, 1].");
    Require(p, {BL_P_plasma_kappa_frac}, kRadMissing);
    if (p.plasma_kappa_frac < 0.0 || p.plasma_kappa_frac > 1.0) Warn(ctx, "Fraction of kappa-distribution electrons outside [0, 1].");
    if (p.plasma_power_frac != 0.0) Require(p, {BL_P_plasma_p, BL_P_plasma_gamma_min, BL_P_plasma_gamma_max}, kRadMissing);
    if (p.plasma_kappa_frac != 0.0) {   // radiation_integrator.cpp:296-308
      Require(p, {BL_P_plasma_kappa}, kRadMissing);
      if (p.image_light && p.image_polarization) {
        if (p.plasma_kappa < 3.5 || p.plasma_kappa > 5.0) throw Failure{BL_E_INPUT, "Polarized transport only supports kappa in [3.5, 5]."};
        if (p.plasma_kappa != 3.5 && p.plasma_kappa != 4.0 && p.plasma_kappa != 4.5 && p.plasma_kappa != 5.0)
          Warn(ctx, "Polarized transport will interpolate formulas based on kappa.");
      }
      Require(p, {BL_P_plasma_w}, kRadMissing);
      // (an unpolarized run with such electrons: bl_render refuses it unless bl_set_undefined_policy(BL_UNDEFINED_KAPPA) was called)
    }
    ctx->plasma_thermal_frac = 1.0 - (p.plasma_power_frac + p.plasma_kappa_frac);
    if (ctx->plasma_thermal_frac < 0.0 || ctx->plasma_thermal_frac > 1.0) Warn(ctx, "Fraction of thermal electrons outside [0, 1].");
    Require(p, {BL_P_cut_rho_min, BL_P_cut_rho_max, BL_P_cut_n_e_min, BL_P_cut_n_e_max, BL_P_cut_p_gas_min,
                BL_P_cut_p_gas_max, BL_P_cut_theta_e_min, BL_P_cut_theta_e_max, BL_P_cut_b_min, BL_P_cut_b_max,
                BL_P_cut_sigma_min, BL_P_cut_sigma_max, BL_P_cut_beta_inverse_min, BL_P_cut_beta_inverse_max},
            kRadMissing);
  }
  Require(p, {BL_P_cut_omit_near, BL_P_cut_omit_far, BL_P_cut_omit_in, BL_P_cut_omit_out, BL_P_cut_midplane_theta,
              BL_P_cut_midplane_z, BL_P_cut_plane},
          kRadMissing);
  if (p.cut_plane)
    Require(p, {BL_P_cut_plane_origin_x, BL_P_cut_plane_origin_y, BL_P_cut_plane_origin_z, BL_P_cut_plane_normal_x,
                BL_P_cut_plane_normal_y, BL_P_cut_plane_normal_z},
            kRadMissing);
  Require(p, {BL_P_fallback_nan}, kRadMissing);
  if (simulation && !p.fallback_nan) Require(p, {BL_P_fallback_rho, BL_P_fallback_pgas}, kRadMissing);
  if (simulation && !p.fallback_nan && p.plasma_model == BL_PLASMA_CODE_KAPPA) Require(p, {BL_P_fallback_kappa}, kRadMissing);

  // geometry data and image rows (:419-520)
  ctx->frame.mass_msun = simulation ? p.simulation_m_msun : p.formula_mass * kC * kC / kGGMsun;
}

// Image rows and their offsets (radiation_integrator.cpp:436-520) for nf frequencies: the parameter block's image_num_frequencies in
// bl_init, the length of bl_set_frequencies' list once one is set. Reads what ValidateRadiation left (polarized, render_num_images).
void BuildImageRows(bl_ctx *ctx, int nf) {
  const bl_params &p = ctx->params;
  const bool simulation = p.model_type == BL_MODEL_SIMULATION;
  BlAuxImages &A = ctx->aux_images;
  A = BlAuxImages{};
  A.image_light = p.image_light;
  A.image_time = p.image_time;
  A.image_length = p.image_length;
  A.image_lambda = p.image_lambda;
  A.image_emission = p.image_emission;
  A.image_tau = p.image_tau;
  A.image_lambda_ave = simulation && p.image_lambda_ave;
  A.image_emission_ave = simulation && p.image_emission_ave;
  A.image_tau_int = simulation && p.image_tau_int;
  A.image_crossings = p.image_crossings;
  int n_q = 0;
  A.polarized = ctx->polarized ? 1 : 0;
  if (A.image_light) n_q += nf * (ctx->polarized ? 4 : 1);
  A.offset_time = n_q;
  if (A.image_time) n_q += 1;
  A.offset_length = n_q;
  if (A.image_length) n_q += 1;
  A.offset_lambda = n_q;
  if (A.image_lambda) n_q += nf;
  A.offset_emission = n_q;
  if (A.image_emission) n_q += nf;
  A.offset_tau = n_q;
  if (A.image_tau) n_q += nf;
  A.offset_lambda_ave = n_q;
  if (A.image_lambda_ave) n_q += nf * kNumCellValues;
  A.offset_emission_ave = n_q;
  if (A.image_emission_ave) n_q += nf * kNumCellValues;
  A.offset_tau_int = n_q;
  if (A.image_tau_int) n_q += nf * kNumCellValues;
  A.offset_crossings = n_q;
  if (A.image_crossings) n_q += 1;
  A.n_q = n_q;
  A.any = (A.image_time || A.image_length || A.image_lambda || A.image_emission || A.image_tau || A.image_lambda_ave
           || A.image_emission_ave || A.image_tau_int || A.image_crossings || ctx->render_num_images > 0
           || ctx->polarized) ? 1 : 0;   // polarized transfer runs in auxiliary-image mode
  ctx->image_num_quantities = n_q;
}

}  // namespace

namespace blhost {
int Fail(bl_ctx *ctx, const Failure &failure) {
  std::string text = "Error: " + failure.message + "\n";
  if (ctx != nullptr)
    ctx->last_error = text;
  else
    g_global_error = text;
  return failure.code;
}

// Why n electron models cannot be rendered by this context (nullptr: they can). bl_set_electron_models and bl_render's plan both ask.
const char *ElectronModelsRefusal(const bl_ctx *ctx, int n) {
  const bl_params &p = ctx->params;
  if (n <= 0) return nullptr;
  if (p.model_type != BL_MODEL_SIMULATION) return "Electron models: formula mode has no electron temperature (model_type = formula).";
  if (ctx->polarized) return "Electron models: polarized runs render one electron model (image_polarization = true).";
  if (p.plasma_model == BL_PLASMA_CODE_KAPPA) return "Electron models: plasma_model = code_kappa takes the electron temperature from the grid, not from R_high / R_low.";
  if (p.slow_light_on) return "Electron models: slow light renders one electron model (slow_light_on = true).";
  if (n >= 2 && p.adaptive_max_level > 0)
    return "Electron models: adaptive refinement reads one image; n >= 2 models need adaptive_max_level = 0.";
  if (n >= 2 && ctx->render_num_images > 0) {   // (renderings come out once: only those no model enters)
    bool theta_e = ThetaECut(p);
    for (int i = 0; i < ctx->render_num_images; i++)
      for (int f = 0; f < p.render_num_features[i]; f++)
        if (p.render_quantity[i][f] == 3) theta_e = true;
    if (theta_e)
      return "Electron models: a rendering that reads Theta_e, or a Theta_e cut beside renderings, differs between models; n >= 2 "
             "models render renderings that no model enters only.";
  }
  return nullptr;
}

// Why n density units cannot be rendered by this context (nullptr: they can). bl_set_density_units and bl_render's plan both ask.
// (The unit scales rho, n_e, p_gas and B in cgs - simulation_coefficients.cpp:237-239, :361-375 - and nothing else a rendering reads.)
const char *DensityUnitsRefusal(const bl_ctx *ctx, int n) {
  const bl_params &p = ctx->params;
  if (n <= 0) return nullptr;
  if (p.model_type != BL_MODEL_SIMULATION) return "Density units: formula mode has no density (model_type = formula).";
  if (ctx->polarized) return "Density units: polarized runs render one density unit (image_polarization = true).";
  if (p.slow_light_on) return "Density units: slow light renders one density unit (slow_light_on = true).";
  if (n >= 2 && p.adaptive_max_level > 0)
    return "Density units: adaptive refinement reads one image; n >= 2 units need adaptive_max_level = 0.";
  if (n >= 2 && ctx->render_num_images > 0) {   // (renderings come out once: only those no unit enters)
    bool unit_cut = UnitCut(p);
    for (int i = 0; i < ctx->render_num_images; i++)
      for (int f = 0; f < p.render_num_features[i]; f++) {
        const int q = p.render_quantity[i][f];   // (bl_params.cpp: rho, n_e, p_gas, Theta_e, B, sigma, beta_inverse)
        if (q == 0 || q == 1 || q == 2 || q == 4) unit_cut = true;
      }
    if (unit_cut)
      return "Density units: a rendering that reads rho, n_e, p_gas or B, or a rho, n_e, p_gas or B cut beside renderings, differs "
             "between units; n >= 2 units render renderings that no unit enters only.";
  }
  return nullptr;
}

// Why n polarized variants cannot be rendered by this context (nullptr: they can). bl_set_polarized_variants and bl_render's plan both ask.
const char *PolarizedVariantsRefusal(const bl_ctx *ctx, int n) {
  const bl_params &p = ctx->params;
  if (n <= 0) return nullptr;
  if (p.model_type != BL_MODEL_SIMULATION)
    return "Polarized variants: formula mode has neither an electron temperature nor a density (model_type = formula).";
  if (!ctx->polarized)
    return "Polarized variants: the context is not polarized (image_polarization = false); bl_set_electron_models and "
           "bl_set_density_units render the variants of an unpolarized run.";
  if (p.slow_light_on) return "Polarized variants: slow light renders one variant (slow_light_on = true).";
  if (n >= 2 && p.adaptive_max_level > 0)
    return "Polarized variants: adaptive refinement reads one image; n >= 2 variants need adaptive_max_level = 0.";
  if (n >= 2 && ctx->render_num_images > 0)
    return "Polarized variants: renderings come out once; n >= 2 variants need render_num_images = 0.";
  return nullptr;
}

// Why n sigma cuts cannot be rendered by this context (nullptr: they can). bl_set_sigma_cuts and bl_render's plan both ask.
// (A cell the cut removes has no coefficients and no cell values: it drops out of a rendering, which comes out once.)
const char *SigmaCutsRefusal(const bl_ctx *ctx, int n) {
  const bl_params &p = ctx->params;
  if (n <= 0) return nullptr;
  if (p.model_type != BL_MODEL_SIMULATION) return "Sigma cuts: formula mode has no magnetisation (model_type = formula).";
  if (ctx->polarized) return "Sigma cuts: the polarized axis is not built yet; polarized runs render one sigma cut (image_polarization = true).";
  if (p.slow_light_on) return "Sigma cuts: slow light renders one sigma cut (slow_light_on = true).";
  if (n >= 2 && p.adaptive_max_level > 0)
    return "Sigma cuts: adaptive refinement reads one image; n >= 2 cuts need adaptive_max_level = 0.";
  if (n >= 2 && ctx->render_num_images > 0)
    return "Sigma cuts: a cut cell drops out of a rendering, and renderings come out once; n >= 2 cuts need render_num_images = 0.";
  return nullptr;
}

// Why n cameras cannot be rendered by this context (nullptr: they can). bl_set_cameras and bl_render's plan both ask.
const char *CamerasRefusal(const bl_ctx *ctx, int n) {
  const bl_params &p = ctx->params;
  if (n <= 0) return nullptr;
  if (p.checkpoint_geodesic_load) return "Cameras: a geodesic checkpoint carries its own camera (checkpoint_geodesic_load = true).";
  if (n < 2) return nullptr;
  if (p.adaptive_max_level > 0) return "Cameras: adaptive refinement reads one image; n >= 2 cameras need adaptive_max_level = 0.";
  if (p.model_type == BL_MODEL_SIMULATION && p.slow_light_on) return "Cameras: slow light renders one camera (slow_light_on = true).";
  if (p.checkpoint_geodesic_save) return "Cameras: a geodesic checkpoint holds one camera; n >= 2 cameras need checkpoint_geodesic_save = false.";
  if (p.model_type == BL_MODEL_SIMULATION && p.checkpoint_sample_save)
    return "Cameras: a sample checkpoint holds one camera; n >= 2 cameras need checkpoint_sample_save = false.";
  if (p.cut_omit_near || p.cut_omit_far) return "Cameras: cut_omit_near and cut_omit_far compare with one camera position; n >= 2 cameras need both off.";
  if (p.image_crossings) return "Cameras: image_crossings counts crossings of one camera's plane; n >= 2 cameras need image_crossings = false.";
  return nullptr;
}

// Why n electron mixes cannot be rendered by this context (nullptr: they can). bl_set_electron_mixes and bl_render's plan both ask.
const char *ElectronMixesRefusal(const bl_ctx *ctx, int n, const bl_electron_mix *mix) {
  const bl_params &p = ctx->params;
  if (n <= 0) return nullptr;
  if (p.model_type != BL_MODEL_SIMULATION) return "Electron mixes: formula mode has no electron distribution (model_type = formula).";
  if (ctx->polarized)
    return "Electron mixes: a polarized run takes its electron distributions with its variants (image_polarization = true): "
           "bl_set_polarized_variants_electrons.";
  if (p.slow_light_on) return "Electron mixes: slow light renders one electron mix (slow_light_on = true).";
  for (int e = 0; e < n; e++)
    if (mix[e].kappa_frac != 0.0)
      return "Electron mixes: kappa-distribution electrons (kappa_frac != 0) in an unpolarized run - the reference's absorptivity reads "
             "kappa_aa_high_i, which it only initialises for polarized runs: no defined result to reproduce.";
  if (n >= 2 && p.adaptive_max_level > 0)
    return "Electron mixes: adaptive refinement reads one image; n >= 2 mixes need adaptive_max_level = 0.";
  if (n >= 2 && ctx->render_num_images > 0) return "Electron mixes: renderings come out once; n >= 2 mixes need render_num_images = 0.";
  if (n >= 2 && p.checkpoint_geodesic_save) return "Electron mixes: a geodesic checkpoint is saved by a render of one image; n >= 2 mixes need checkpoint_geodesic_save = false.";
  if (n >= 2 && p.checkpoint_sample_save) return "Electron mixes: a sample checkpoint is saved by a render of one image; n >= 2 mixes need checkpoint_sample_save = false.";
  return nullptr;
}

// Why a list of n frequencies cannot be rendered by this context (nullptr: it can). bl_set_frequencies and bl_render's plan both ask.
const char *FrequenciesRefusal(const bl_ctx *ctx, int n) {
  if (n <= 0) return nullptr;
  if (ctx->params.checkpoint_geodesic_load)
    return "Frequencies: a geodesic checkpoint carries its own frequency list, which replaces the context's (checkpoint_geodesic_load = true).";
  return nullptr;
}

// The variants of a render, in image-row order: the triples (each with its own cut_sigma_max where bl_set_polarized_variants_sigma gave
// one, and its own electron mix where bl_set_polarized_variants_electrons gave one), else the mixes of `mixes` x models x units x
// sigma cuts - mix-major, then model, then unit, then cut (Variants::Index) - with the parameter block's mix, pair, unit and
// cut_sigma_max where an axis is not set. The one reader of what the five setters stored.
Variants ResolveVariants(const bl_ctx *ctx, MixRange mixes) {
  const bl_params &p = ctx->params;
  const std::vector<Variant> own = {{p.plasma_rat_low, p.plasma_rat_high, p.simulation_rho_cgs, p.cut_sigma_max, BlockMix(p)}};
  const std::vector<double> own_cut = {p.cut_sigma_max};
  const int mix_end = std::min(mixes.end, static_cast<int>(ctx->mixes.size()));
  const std::vector<bl_electron_mix> some_mixes(ctx->mixes.begin() + std::min(mixes.begin, mix_end), ctx->mixes.begin() + mix_end), own_mix = {BlockMix(p)};
  Variants v{ctx->triples, static_cast<int>(ctx->models.size()), static_cast<int>(ctx->units.size()), static_cast<int>(ctx->triples.size()),
             static_cast<int>(ctx->sigma_cuts.size()), static_cast<int>(some_mixes.size()), {}};
  if (!ctx->triples_cut)
    for (Variant &triple : v.list) triple.sigma_max = p.cut_sigma_max;
  if (!ctx->triples_mix)
    for (Variant &triple : v.list) triple.mix = BlockMix(p);
  if (v.n_pol == 0)
    for (const bl_electron_mix &mix : v.n_mixes > 0 ? some_mixes : own_mix)
      for (const Variant &model : v.n_models > 0 ? ctx->models : own)
        for (const Variant &unit : v.n_units > 0 ? ctx->units : own)
          for (const double sigma_max : v.n_cuts > 0 ? ctx->sigma_cuts : own_cut) v.list.push_back({model.rat_low, model.rat_high, unit.rho, sigma_max, mix});
  const auto extent = [](int n_set) { return n_set > 0 ? n_set : 1; };   // (0, not set: the parameter block's one)
  v.extent = {extent(v.n_mixes), extent(v.n_models), extent(v.n_units), extent(v.n_pol > 0 ? v.n_pol : v.n_cuts)};
  return v;
}

// The five lists a context holds, each as a check and a store. A check reads the parameter block and the call's arguments and nothing a
// setter stored, and gives the Failure the setter reports - nothing when the call can go through. A store needs render_lock held
// (between renders; geodesics and located samples stay: no model, unit, cut or triple enters them) and cannot fail. A setter is
// check, store; bl_apply_sweep_lists checks every list it carries, then stores them all.
namespace {
using Refused = std::optional<Failure>;

Refused CheckElectronModels(const bl_ctx *ctx, int n, const double *rat_low, const double *rat_high) {
  if (n < 0 || n > BL_MAX_ELECTRON_MODELS || (n > 0 && (rat_low == nullptr || rat_high == nullptr)))
    return Failure{BL_E_ARG, "bl_set_electron_models needs 0 <= n <= " + std::to_string(BL_MAX_ELECTRON_MODELS) + " and both ratio arrays."};
  for (int m = 0; m < n; m++)
    if (!std::isfinite(rat_low[m]) || !std::isfinite(rat_high[m]))
      return Failure{BL_E_ARG, "bl_set_electron_models: model " + std::to_string(m) + " has a ratio that is not finite."};
  if (const char *why = ElectronModelsRefusal(ctx, n)) return Failure{BL_E_UNSUPPORTED, why};
  return std::nullopt;
}
void StoreElectronModels(bl_ctx *ctx, int n, const double *rat_low, const double *rat_high) {
  ctx->models.resize(n);
  for (int m = 0; m < n; m++) ctx->models[m] = {rat_low[m], rat_high[m], 0.0, 0.0};
}

Refused CheckDensityUnits(const bl_ctx *ctx, int n, const double *rho_cgs) {
  if (n < 0 || n > BL_MAX_DENSITY_UNITS || (n > 0 && rho_cgs == nullptr))
    return Failure{BL_E_ARG, "bl_set_density_units needs 0 <= n <= " + std::to_string(BL_MAX_DENSITY_UNITS) + " and the array of units."};
  for (int u = 0; u < n; u++)
    if (!std::isfinite(rho_cgs[u]) || !(rho_cgs[u] > 0.0))
      return Failure{BL_E_ARG, "bl_set_density_units: unit " + std::to_string(u) + " is not a finite value > 0."};
  if (const char *why = DensityUnitsRefusal(ctx, n)) return Failure{BL_E_UNSUPPORTED, why};
  return std::nullopt;
}
void StoreDensityUnits(bl_ctx *ctx, int n, const double *rho_cgs) {
  ctx->units.resize(n);
  for (int u = 0; u < n; u++) ctx->units[u] = {0.0, 0.0, rho_cgs[u], 0.0};
}

// ... the triples, with a cut and a mix each where the arrays are given; *warnings: the reference's, for a call that goes through
Refused CheckPolarizedVariants(const bl_ctx *ctx, int n, const double *rat_low, const double *rat_high, const double *rho_cgs, const double *sigma_max,
                               const bl_electron_mix *mix, std::vector<const char *> *warnings) {
  if (n < 0 || n > BL_MAX_POLARIZED_VARIANTS || (n > 0 && (rat_low == nullptr || rat_high == nullptr || rho_cgs == nullptr)))
    return Failure{BL_E_ARG, "bl_set_polarized_variants needs 0 <= n <= " + std::to_string(BL_MAX_POLARIZED_VARIANTS) + " and the three arrays."};
  for (int v = 0; v < n; v++) {
    if (!std::isfinite(rat_low[v]) || !std::isfinite(rat_high[v]))
      return Failure{BL_E_ARG, "bl_set_polarized_variants: variant " + std::to_string(v) + " has a non-finite R_low or R_high."};
    if (!std::isfinite(rho_cgs[v]) || !(rho_cgs[v] > 0.0))
      return Failure{BL_E_ARG, "bl_set_polarized_variants: the unit of variant " + std::to_string(v) + " is not a finite value > 0."};
    if (sigma_max != nullptr && !std::isfinite(sigma_max[v]))
      return Failure{BL_E_ARG, "bl_set_polarized_variants_sigma: the sigma cut of variant " + std::to_string(v) + " is not finite."};
  }
  if (const char *why = PolarizedVariantsRefusal(ctx, n)) return Failure{BL_E_UNSUPPORTED, why};
  // The mixes, as bl_init checks the parameter block's (radiation_integrator.cpp:283-311): what is read must be finite - the shape values
  // of a distribution whose fraction is zero are not read - kappa within the range of the polarized fits, and the reference's warnings,
  // each once per call
  bool warn_power = false, warn_kappa = false, warn_thermal = false, warn_interpolate = false;
  for (int v = 0; mix != nullptr && v < n; v++) {
    const bl_electron_mix &m = mix[v];
    const std::string which = "bl_set_polarized_variants_electrons: variant " + std::to_string(v);
    if (!std::isfinite(m.power_frac)) return Failure{BL_E_ARG, which + " has a power_frac that is not finite."};
    if (!std::isfinite(m.kappa_frac)) return Failure{BL_E_ARG, which + " has a kappa_frac that is not finite."};
    if (m.power_frac != 0.0) {
      if (!std::isfinite(m.p)) return Failure{BL_E_ARG, which + " has a p that is not finite."};
      if (!std::isfinite(m.gamma_min)) return Failure{BL_E_ARG, which + " has a gamma_min that is not finite."};
      if (!std::isfinite(m.gamma_max)) return Failure{BL_E_ARG, which + " has a gamma_max that is not finite."};
    }
    if (m.kappa_frac != 0.0) {
      if (!std::isfinite(m.kappa)) return Failure{BL_E_ARG, which + " has a kappa that is not finite."};
      if (!std::isfinite(m.w)) return Failure{BL_E_ARG, which + " has a w that is not finite."};
      if (m.kappa < 3.5 || m.kappa > 5.0) return Failure{BL_E_ARG, which + ": Polarized transport only supports kappa in [3.5, 5]."};
      warn_interpolate = warn_interpolate || (m.kappa != 3.5 && m.kappa != 4.0 && m.kappa != 4.5 && m.kappa != 5.0);
    }
    warn_power = warn_power || m.power_frac < 0.0 || m.power_frac > 1.0;
    warn_kappa = warn_kappa || m.kappa_frac < 0.0 || m.kappa_frac > 1.0;
    const double thermal_frac = ThermalFraction(m);
    warn_thermal = warn_thermal || thermal_frac < 0.0 || thermal_frac > 1.0;
  }
  if (warn_power) warnings->push_back("Fraction of power-law electrons outside [0, 1].");
  if (warn_kappa) warnings->push_back("Fraction of kappa-distribution electrons outside [0, 1].");
  if (warn_interpolate) warnings->push_back("Polarized transport will interpolate formulas based on kappa.");
  if (warn_thermal) warnings->push_back("Fraction of thermal electrons outside [0, 1].");
  return std::nullopt;
}
void StorePolarizedVariants(bl_ctx *ctx, int n, const double *rat_low, const double *rat_high, const double *rho_cgs, const double *sigma_max,
                            const bl_electron_mix *mix) {
  ctx->triples.resize(n);
  for (int v = 0; v < n; v++)
    ctx->triples[v] = {rat_low[v], rat_high[v], rho_cgs[v], sigma_max != nullptr ? sigma_max[v] : 0.0, mix != nullptr ? mix[v] : bl_electron_mix{}};
  ctx->triples_cut = n > 0 && sigma_max != nullptr;
  ctx->triples_mix = n > 0 && mix != nullptr;
}

Refused CheckSigmaCuts(const bl_ctx *ctx, int n, const double *sigma_max) {
  if (n < 0 || n > BL_MAX_SIGMA_CUTS || (n > 0 && sigma_max == nullptr))
    return Failure{BL_E_ARG, "bl_set_sigma_cuts needs 0 <= n <= " + std::to_string(BL_MAX_SIGMA_CUTS) + " and the array of cuts."};
  for (int s = 0; s < n; s++)
    if (!std::isfinite(sigma_max[s])) return Failure{BL_E_ARG, "bl_set_sigma_cuts: cut " + std::to_string(s) + " is not finite."};
  if (const char *why = SigmaCutsRefusal(ctx, n)) return Failure{BL_E_UNSUPPORTED, why};
  return std::nullopt;
}
void StoreSigmaCuts(bl_ctx *ctx, int n, const double *sigma_max) { ctx->sigma_cuts.assign(sigma_max, sigma_max + n); }

// ... the electron mixes of an unpolarized run, checked as CheckPolarizedVariants checks a variant's mix (what is read must be finite; the
// reference's two warnings, each once per call); a mix with kappa electrons is refused, not checked
Refused CheckElectronMixes(const bl_ctx *ctx, int n, const bl_electron_mix *mix, std::vector<const char *> *warnings) {
  if (n < 0 || n > BL_MAX_ELECTRON_MIXES || (n > 0 && mix == nullptr))
    return Failure{BL_E_ARG, "bl_set_electron_mixes needs 0 <= n <= " + std::to_string(BL_MAX_ELECTRON_MIXES) + " and the array of mixes."};
  bool warn_power = false, warn_thermal = false;
  for (int e = 0; e < n; e++) {
    const bl_electron_mix &m = mix[e];
    const std::string which = "bl_set_electron_mixes: mix " + std::to_string(e);
    if (!std::isfinite(m.power_frac)) return Failure{BL_E_ARG, which + " has a power_frac that is not finite."};
    if (m.power_frac != 0.0) {
      if (!std::isfinite(m.p)) return Failure{BL_E_ARG, which + " has a p that is not finite."};
      if (!std::isfinite(m.gamma_min)) return Failure{BL_E_ARG, which + " has a gamma_min that is not finite."};
      if (!std::isfinite(m.gamma_max)) return Failure{BL_E_ARG, which + " has a gamma_max that is not finite."};
    }
  }
  if (const char *why = ElectronMixesRefusal(ctx, n, mix)) return Failure{BL_E_UNSUPPORTED, why};
  for (int e = 0; e < n; e++) {
    warn_power = warn_power || mix[e].power_frac < 0.0 || mix[e].power_frac > 1.0;
    const double thermal_frac = ThermalFraction(mix[e]);
    warn_thermal = warn_thermal || thermal_frac < 0.0 || thermal_frac > 1.0;
  }
  if (warn_power) warnings->push_back("Fraction of power-law electrons outside [0, 1].");
  if (warn_thermal) warnings->push_back("Fraction of thermal electrons outside [0, 1].");
  return std::nullopt;
}
void StoreElectronMixes(bl_ctx *ctx, int n, const bl_electron_mix *mix) { ctx->mixes.assign(mix, mix + n); }

// ... the cameras, 0 <= n <= BL_MAX_CAMERAS; *list: the cameras with their frames. th_deg == nullptr: every camera at the parameter
// block's own camera_th (its radians and its camera_pole, which no degree value need give back); ph_deg == nullptr: at the block's
// camera_ph - what an absent sweep_camera_th or sweep_camera_ph means.
Refused CheckCameras(const bl_ctx *ctx, int n, const double *th_deg, const double *ph_deg, std::vector<bl_ctx::Camera> *list) {
  for (int c = 0; c < n; c++)
    if ((th_deg != nullptr && !std::isfinite(th_deg[c])) || (ph_deg != nullptr && !std::isfinite(ph_deg[c])))
      return Failure{BL_E_ARG, "bl_set_cameras: camera " + std::to_string(c) + " has an angle that is not finite."};
  if (const char *why = CamerasRefusal(ctx, n)) return Failure{BL_E_UNSUPPORTED, why};
  // Each camera's frame: what bl_init builds from the parameters with the three fields a written camera_th and camera_ph set
  // (bl_params.cpp: degrees * pi / 180; camera_pole for a written th of exactly 0 or 180)
  list->resize(n);
  for (int c = 0; c < n; c++) {
    bl_params p = ctx->params;
    (*list)[c] = {p.camera_th * 180.0 / kPi, p.camera_ph * 180.0 / kPi, ctx->block_frame};
    if (th_deg != nullptr) {
      p.camera_th = th_deg[c] * kPi / 180.0;
      p.camera_pole = (th_deg[c] == 0.0 || th_deg[c] == 180.0) ? 1 : 0;
      (*list)[c].th_deg = th_deg[c];
    }
    if (ph_deg != nullptr) {
      p.camera_ph = ph_deg[c] * kPi / 180.0;
      (*list)[c].ph_deg = ph_deg[c];
    }
    bl_camera_frame_build(p, ctx->st, &(*list)[c].frame);
  }
  return std::nullopt;
}
void StoreCameras(bl_ctx *ctx, std::vector<bl_ctx::Camera> list) {   // (the resident geodesics' key holds the list: another list integrates again)
  ctx->cameras = std::move(list);
  ctx->cameras_uploaded = false;
  ctx->frame = ctx->cameras.size() == 1 ? ctx->cameras[0].frame : ctx->block_frame;
}

// ... the frequencies, 0 <= n <= BL_MAX_FREQUENCIES (n = 0: the parameter block's own list again)
Refused CheckFrequencies(const bl_ctx *ctx, int n, const double *hz) {
  const bl_params &p = ctx->params;
  if (n < 0 || n > BL_MAX_FREQUENCIES || (n > 0 && hz == nullptr))
    return Failure{BL_E_ARG, "bl_set_frequencies needs 0 <= n <= " + std::to_string(BL_MAX_FREQUENCIES) + " and the array of frequencies."};
  for (int l = 0; l < n; l++)
    if (!std::isfinite(hz[l]) || !(hz[l] > 0.0))
      return Failure{BL_E_ARG, "bl_set_frequencies: frequency " + std::to_string(l) + " is not a finite value > 0."};
  if (const char *why = FrequenciesRefusal(ctx, n)) return Failure{BL_E_UNSUPPORTED, why};
  // (bl_init's check of the block, radiation_integrator.cpp:231-236, with the list's length for image_num_frequencies)
  if (p.adaptive_max_level > 0 && n >= 2 && (!Has(p, BL_P_adaptive_frequency_num) || p.adaptive_frequency_num < 1 || p.adaptive_frequency_num > n))
    return Failure{BL_E_ARG, "Must choose adaptive_frequency_num from 1 to image_num_frequencies."};
  return std::nullopt;
}
// (geodesics and located samples stay: no frequency enters them. The rows and their offsets follow the list's length through the code
// bl_init built them with.)
void StoreFrequencies(bl_ctx *ctx, int n, const double *hz) {
  if (n == 0 && ctx->frequencies_set == 0) return;   // (nothing set: the list is bl_init's - or a loaded checkpoint's - as it stands)
  if (n > 0) ctx->frequencies.assign(hz, hz + n);
  else BuildFrequencies(ctx);
  ctx->frequencies_set = n;
  BuildImageRows(ctx, static_cast<int>(ctx->frequencies.size()));
}
}  // namespace
}  // namespace blhost

extern "C" {

int bl_init(const bl_params *p, int device, bl_ctx **out) {
  if (p == nullptr || out == nullptr) return BL_E_ARG;
  *out = nullptr;
  bl_ctx *ctx = new bl_ctx();
  ctx->params = *p;
  {   // measurement switches: the environment is read here and nowhere else (getenv is not safe beside a setenv in another thread)
    const struct { const char *name; unsigned int bit; } kSwitches[] = {
        {"BLACKLIGHT_AMD_TENSOR_TRANSPORT", BL_SWITCH_TENSOR_TRANSPORT}, {"BLACKLIGHT_AMD_SPLIT_RECORDS", BL_SWITCH_SPLIT_RECORDS},
        {"BLACKLIGHT_AMD_RECORD_EVERY_STEP", BL_SWITCH_RECORD_EVERY_STEP},
        {"BLACKLIGHT_AMD_GENERAL_LOCATE", BL_SWITCH_GENERAL_LOCATE}, {"BLACKLIGHT_AMD_LANE_TRANSFER", BL_SWITCH_LANE_TRANSFER},
        {"BLACKLIGHT_AMD_NO_FUSED_LOCATE", BL_SWITCH_NO_FUSED_LOCATE}, {"BLACKLIGHT_AMD_SAMPLE_RECORDS", BL_SWITCH_SAMPLE_RECORDS},
        {"BLACKLIGHT_AMD_QUAD_EVERY_RAY", BL_SWITCH_QUAD_EVERY_RAY}, {"BLACKLIGHT_AMD_FLAT_ORDER", BL_SWITCH_FLAT_ORDER},
        {"BLACKLIGHT_AMD_GLOBAL_ANGLES", BL_SWITCH_GLOBAL_ANGLES}, {"BLACKLIGHT_AMD_GENERAL_CUTS", BL_SWITCH_GENERAL_CUTS},
        {"BLACKLIGHT_AMD_NO_MIRROR_PAIRS", BL_SWITCH_NO_MIRROR_PAIRS}, {"BLACKLIGHT_AMD_EXACT_DISTANCE", BL_SWITCH_EXACT_DISTANCE},
        {"BLACKLIGHT_AMD_WIDE_DISTANCE_BAND", BL_SWITCH_WIDE_DISTANCE_BAND}};
    for (const auto &sw : kSwitches)
      if (std::getenv(sw.name) != nullptr) ctx->switches |= sw.bit;
    ctx->debug_counters = std::getenv("BLACKLIGHT_AMD_DEBUG_COUNTERS") != nullptr;
    // the arithmetic tier a context starts in: tolerant (north_star's tolerance), or what the deployment says
    // (exact | tolerant, in any case; anything else is an error of bl_init - a typo must not silently select a tier)
    if (const char *tier = std::getenv("BLACKLIGHT_AMD_ARITHMETIC")) {
      std::string name = tier;
      for (char &c : name) c = static_cast<char>(std::tolower(static_cast<unsigned char>(c)));
      if (name == "exact") ctx->arithmetic = BL_ARITH_EXACT;
      else if (name == "tolerant") ctx->arithmetic = BL_ARITH_TOLERANT;
      else {
        g_global_error = "Error: BLACKLIGHT_AMD_ARITHMETIC must be exact or tolerant, not \"" + std::string(tier) + "\".\n";
        delete ctx;
        return BL_E_INPUT;
      }
    }
    if (const char *policy = std::getenv("BLACKLIGHT_AMD_TAIL_POLICY")) {   // (A/B runs: bl_set_tail_policy from the environment)
      const std::string name = policy;
      if (name != "auto" && name != "wide" && name != "quad" && name != "split") {
        g_global_error = "Error: BLACKLIGHT_AMD_TAIL_POLICY must be auto, wide, quad or split, not \"" + name + "\".\n";
        delete ctx;
        return BL_E_INPUT;
      }
      ctx->tail_policy = name == "wide" ? BL_TAIL_WIDE : (name == "quad" ? BL_TAIL_QUAD : (name == "split" ? BL_TAIL_SPLIT : BL_TAIL_AUTO));
    }
  }
  try {
    ValidateGeodesic(ctx);
    ValidateRadiation(ctx);
    BuildFrequencies(ctx);
    BuildImageRows(ctx, static_cast<int>(ctx->frequencies.size()));
    bl_camera_frame_build(ctx->params, ctx->st, &ctx->frame);
    ctx->block_frame = ctx->frame;
    if (device == BL_DEVICE_NONE) {   // host-only context: validation, camera frame, refinement, writer
      ctx->device = BL_DEVICE_NONE;
      *out = ctx;
      return BL_OK;
    }
    int count = 0;
    hipError_t err = hipGetDeviceCount(&count);
    if (err != hipSuccess || count <= 0)
      throw Failure{BL_E_DEVICE, "No HIP device available: the MI355X hot path has no CPU fallback."};
    if (device < 0) Check(hipGetDevice(&device), "hipGetDevice");
    if (device >= count) throw Failure{BL_E_DEVICE, "Requested device index out of range."};
    Check(hipSetDevice(device), "hipSetDevice");
    ctx->device = device;
    hipDeviceProp_t prop;
    Check(hipGetDeviceProperties(&prop, device), "hipGetDeviceProperties");
    ctx->num_cus = prop.multiProcessorCount;
    // scratch for sample records: four fifths of the device's memory unless bl_set_scratch_limit says otherwise (MI355X: 230 of
    // 288 GB - a 1024^2 full-Stokes frame in two chunks; whatever a render plans is capped by what is actually free)
    ctx->scratch_limit = static_cast<uint64_t>(0.8 * static_cast<double>(prop.totalGlobalMem));
    EnsureStreams(ctx);
  } catch (const Failure &failure) {
    int code = Fail(nullptr, failure);
    delete ctx;
    return code;
  }
  *out = ctx;
  return BL_OK;
}

namespace {

// The cells into their HBM layout on the device. The caller's arrays are [variable][block][k][j][i] (simulation_reader.cpp:767-780);
// the kernels read [cell][8 variables]. Eight planes are uploaded as they lie (a copy each, no pass over them on the host) and
// one kernel interleaves them - a lane per cell: eight coalesced reads, 32 contiguous bytes written - placing a block's cells at the
// block's position in the merged array where there is one (block_origin: first target cell of every block, and the target's row
// and plane strides; null: the blocks stay one behind the other). On the host this repack was 0.3 s per 256^3 snapshot, ten times
// the render of a series' frame over resident geodesics.
// The planes are wherever `src` says: the upload buffer above (block_stride == block_cells: plane q's cell c at base[q] + c, the
// addresses this kernel always read), or the caller's own device array (bl_set_grid_device) with its block stride and element type -
// float, or double rounded to the nearest float as a conversion on the host rounds it. count == 1 places one plane instead of
// eight: `cells` is then a [k][j][i] float array with the same targets (the electron entropy of plasma_model = code_kappa).
// Everything but the cell index is wave-uniform.
struct BlCellPlanes {
  const void *base[8];                            // first element of each plane (count of them), already at its variable
  unsigned long long block_stride, block_cells;   // elements from a block to the next in the source; cells of a block
  int f64, count;                                 // elements are doubles; planes: 8 or 1
};
__device__ __forceinline__ float bl_plane_cell(const void *base, unsigned long long at, int f64) {
  return f64 ? static_cast<float>(static_cast<const double *>(base)[at]) : static_cast<const float *>(base)[at];
}

// The harm form of the same kernel (bl_set_grid_device_harm, bl_harm_convert_device): the source is one array [n1][n2][n3][n_prim] of a
// harm-family code, the target the same cells transposed to [k][j][i] and converted as the reader converts a file's (bl_harm.h). The
// source is contiguous along (k, variable) for fixed (i, j), the target along i: a workgroup takes a tile of kHarmTileI i's by
// kHarmTileK k's at one j through LDS - the reads run along k * n_prim (256 bytes and more per i), a lane then converts one cell and
// the stores run along i (whole 32-byte cells, 1 KB per half wave; plane by plane for bl_harm_convert_device) - and up to
// kHarmChunkTiles such tiles one after the other in k, so that the point structs of its i's are read once, into LDS, for all of them.
// A row of the tile (one i) is kHarmTileK * 9 + 1 words: the odd stride puts the lanes of a half wave, which read the same word of
// 32 different rows, into 32 different banks. No atomics; every address is formed from i < n1, j < n2, k < n3 and an index < n_prim.
struct BlHarmSource {
  const void *prims;                  // null: the plain form (and nothing else of this struct is read)
  const double *points;               // [n2][n1][BL_HARM_POINT_DOUBLES]: BlHarmPoint
  float *kappa;                       // the entropy plane [k][j][i] (variable index[8]); null: none
  unsigned long long plane_stride;    // 0: `cells` is [cell][8]; else eight planes, this many floats apart
  int n1, n2, n3, n_prim;
  int index[9];                       // rho, UU, U1..3, B1..3, entropy: where they lie in a cell's n_prim values
  int f64;
  float gamma_minus_one;
  unsigned int i_tiles;               // tiles along i: block = (k_chunk * n2 + j) * i_tiles + i_tile
};
constexpr int kHarmTileI = 32, kHarmTileK = 8, kHarmSlots = 9, kHarmRow = kHarmTileK * kHarmSlots + 1, kHarmChunkTiles = 8;
constexpr int kHarmPointRow = BL_HARM_POINT_DOUBLES + 1;   // a point's doubles and one of padding: the lanes of a half wave read one member of 32 points
constexpr size_t kHarmLdsBytes = static_cast<size_t>(kHarmPointRow) * kHarmTileI * sizeof(double) + static_cast<size_t>(kHarmTileI) * kHarmRow * sizeof(float);
static_assert(kHarmTileI * kHarmTileK == 256, "a lane per cell of the tile");

__device__ __forceinline__ void bl_harm_stage(const BlHarmSource &h, float *cells) {
  extern __shared__ double bl_stage_lds[];
  double *points = bl_stage_lds;                                                    // [i of the tile][kHarmPointRow]
  float *tile = reinterpret_cast<float *>(bl_stage_lds + kHarmPointRow * kHarmTileI);   // [i of the tile][kHarmRow]
  const int t = threadIdx.x;
  const unsigned int i_tile = blockIdx.x % h.i_tiles, rest = blockIdx.x / h.i_tiles;
  const int j = static_cast<int>(rest % static_cast<unsigned int>(h.n2)), k_chunk = static_cast<int>(rest / static_cast<unsigned int>(h.n2));
  const int i0 = static_cast<int>(i_tile) * kHarmTileI;
  const int n_i = min(kHarmTileI, h.n1 - i0);
  const int k_begin = k_chunk * (kHarmTileK * kHarmChunkTiles), k_end = min(h.n3, k_begin + kHarmTileK * kHarmChunkTiles);
  const double *point_row = h.points + (static_cast<unsigned long long>(j) * h.n1 + i0) * BL_HARM_POINT_DOUBLES;
  for (int e = t; e < n_i * BL_HARM_POINT_DOUBLES; e += 256) points[e + e / BL_HARM_POINT_DOUBLES] = point_row[e];
  // reading: lane t takes variable t % 8 of the cell at k0 + (t / 8) % 8 of the tile's rows t / 64, t / 64 + 4, ... - the eight variables of
  // a cell side by side, the cells of an i along k
  const int q = t % 8, lk = (t / 8) % kHarmTileK, li0 = t / 64;
  int variable = h.index[0];
#pragma unroll
  for (int s = 1; s < 8; s++) variable = q == s ? h.index[s] : variable;
  const unsigned long long row_elements = static_cast<unsigned long long>(h.n2) * h.n3 * h.n_prim;   // from an i to the next
  const unsigned long long read0 = (static_cast<unsigned long long>(i0 + li0) * h.n2 + j) * h.n3 * h.n_prim + variable;
  const unsigned long long kappa0 = (static_cast<unsigned long long>(i0 + t / kHarmTileK) * h.n2 + j) * h.n3 * h.n_prim + h.index[8];
  // converting: lane t takes the cell at row t % 32, k0 + t / 32
  const int ii = t % kHarmTileI, kk = t / kHarmTileI;
  const int i = i0 + ii;
  const BlHarmPoint &pt = *reinterpret_cast<const BlHarmPoint *>(points + ii * kHarmPointRow);
  for (int k0 = k_begin; k0 < k_end; k0 += kHarmTileK) {
    __syncthreads();   // (the tile's previous cells have been read; the first time: the points are in place after the next one)
    if (cells != nullptr && k0 + lk < k_end) {   // (cells null: the entropy plane alone is wanted, and read)
      const unsigned long long at = read0 + static_cast<unsigned long long>(k0 + lk) * h.n_prim;
#pragma unroll 2   // (two reads in flight per lane: unrolled further, the harm form needs more than the 64 registers that keep eight waves per SIMD)
      for (int pass = 0; pass < 8; pass++) {
        const int li = li0 + 4 * pass;
        if (i0 + li < h.n1) tile[li * kHarmRow + lk * kHarmSlots + q] = bl_plane_cell(h.prims, at + 4 * pass * row_elements, h.f64);
      }
    }
    if (h.kappa != nullptr && i0 + t / kHarmTileK < h.n1 && k0 + t % kHarmTileK < k_end)
      tile[(t / kHarmTileK) * kHarmRow + (t % kHarmTileK) * kHarmSlots + 8] =
          bl_plane_cell(h.prims, kappa0 + static_cast<unsigned long long>(k0 + t % kHarmTileK) * h.n_prim, h.f64);
    __syncthreads();
    const int k = k0 + kk;
    if (i >= h.n1 || k >= k_end) continue;
    const float *mine = tile + ii * kHarmRow + kk * kHarmSlots;
    const unsigned long long target = (static_cast<unsigned long long>(k) * h.n2 + j) * h.n1 + i;
    if (h.kappa != nullptr) h.kappa[target] = mine[8];
    if (cells == nullptr) continue;   // (the entropy plane alone)
    float in[6], converted[6];
#pragma unroll
    for (int s = 0; s < 6; s++) in[s] = mine[2 + s];
    bl_harm_cell(pt, in, converted);
    const float rho = mine[0], pgas = mine[1] * h.gamma_minus_one;   // internal energy to pressure, in float as the reader has it
    if (h.plane_stride == 0) {
      float4 *out = reinterpret_cast<float4 *>(cells + target * 8);
      out[0] = make_float4(rho, pgas, converted[0], converted[1]);
      out[1] = make_float4(converted[2], converted[3], converted[4], converted[5]);
    } else {
      cells[target] = rho;
      cells[h.plane_stride + target] = pgas;
#pragma unroll
      for (int s = 0; s < 6; s++) cells[(2 + s) * h.plane_stride + target] = converted[s];
    }
  }
}

__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) bl_interleave_cells_kernel(BlCellPlanes src, float *cells, unsigned long long n_cells, int nb_i, int nb_j, int nb_k,
                                                                  const unsigned long long *block_origin, unsigned long long row_stride,
                                                                  unsigned long long plane_stride, BlHarmSource harm) {
  if (harm.prims != nullptr) {   // (wave-uniform: the form is the launch's)
    bl_harm_stage(harm, cells);
    return;
  }
  const unsigned long long c = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_cells) return;
  unsigned long long target = c, from = c;
  if (block_origin != nullptr || src.block_stride != src.block_cells) {
    const unsigned long long blk = c / src.block_cells, rest = c - blk * src.block_cells;
    from = blk * src.block_stride + rest;
    if (block_origin != nullptr) {
      const unsigned long long k = rest / ((unsigned long long)nb_i * nb_j), j = (rest / nb_i) % nb_j, i = rest % nb_i;
      target = block_origin[blk] + k * plane_stride + j * row_stride + i;
    }
  }
  if (src.count == 1) {
    cells[target] = bl_plane_cell(src.base[0], from, src.f64);
    return;
  }
  float v[8];
  if (src.f64) {   // (one branch around the eight loads, so that either kind is issued back to back)
    double wide[8];
#pragma unroll
    for (int q = 0; q < 8; q++) wide[q] = static_cast<const double *>(src.base[q])[from];
#pragma unroll
    for (int q = 0; q < 8; q++) v[q] = static_cast<float>(wide[q]);
  } else {
#pragma unroll
    for (int q = 0; q < 8; q++) v[q] = static_cast<const float *>(src.base[q])[from];
  }
  float4 *out = reinterpret_cast<float4 *>(cells + target * 8);
  out[0] = make_float4(v[0], v[1], v[2], v[3]);
  out[1] = make_float4(v[4], v[5], v[6], v[7]);
}

// bl_set_grid_device's array on the device's side, before anything reads it: device memory of this context's device, and n_elements
// elements from prim inside one allocation (CheckDeviceCells has held the strides to n_elements)
void CheckDevicePointer(bl_ctx *ctx, const bl_device_cells &cells, const char *text = nullptr) {
  const Failure refusal{BL_E_ARG, text != nullptr ? text
                                                  : "bl_device_cells: prim must be device memory of the context's device, with n_elements elements inside one allocation; "
                                                    "host arrays go through bl_set_grid."};
  const size_t element = cells.dtype == BL_CELLS_F64 ? sizeof(double) : sizeof(float);
  if (cells.n_elements < 1 || static_cast<unsigned long long>(cells.n_elements) > (~0ull >> 1) / element) throw refusal;
  hipPointerAttribute_t attributes{};
  if (hipPointerGetAttributes(&attributes, cells.prim) != hipSuccess) {
    (void)hipGetLastError();   // (an address the runtime does not know: not an error of this context's)
    throw refusal;
  }
  if (attributes.type != hipMemoryTypeDevice || attributes.device != ctx->device) throw refusal;
  hipDeviceptr_t first = nullptr;
  size_t bytes = 0;
  if (hipMemGetAddressRange(&first, &bytes, const_cast<void *>(cells.prim)) != hipSuccess) {
    (void)hipGetLastError();
    throw refusal;
  }
  const unsigned long long lo = reinterpret_cast<unsigned long long>(first), at = reinterpret_cast<unsigned long long>(cells.prim);
  if (at < lo || at - lo > bytes || static_cast<unsigned long long>(cells.n_elements) * element > bytes - (at - lo)) throw refusal;
}

// One launch of the staging kernel on `stream`: `count` planes of `src` (8: into the cell array; 1: into a [k][j][i] plane) at the
// grid's placement
void LaunchCellStaging(bl_ctx *ctx, BlCellPlanes src, int count, float *target, hipStream_t stream) {
  const CellPlacement &pl = ctx->grid.tables.placement;
  src.block_cells = static_cast<unsigned long long>(pl.nb[0]) * pl.nb[1] * pl.nb[2];
  src.count = count;
  hipLaunchKernelGGL(bl_interleave_cells_kernel, dim3(static_cast<unsigned int>((pl.n_cells + 255) / 256)), dim3(256), 0, stream, src, target,
                     static_cast<unsigned long long>(pl.n_cells), pl.nb[0], pl.nb[1], pl.nb[2], pl.has_origin ? ctx->grid.d_block_origin.ptr : nullptr, pl.row_stride,
                     pl.plane_stride, BlHarmSource{});
  Check(hipGetLastError(), "cell interleave kernel launch");
}

// bl_set_grid_device_harm and its kin: the grid the cells belong to, and the caller's array
struct HarmCells {
  const bl_harm_grid *grid;
  const bl_harm_cells *cells;
};

// What bl_device_cells' checks ask of a harm array before anything is launched (CheckDeviceCells)
void CheckHarmCells(const bl_harm_grid *grid, const bl_harm_cells *cells) {
  if (grid == nullptr) throw Failure{BL_E_ARG, "bl_harm_cells: the grid is NULL."};
  if (cells == nullptr) throw Failure{BL_E_ARG, "bl_harm_cells: the description is NULL."};
  if (cells->prim == nullptr) throw Failure{BL_E_ARG, "bl_harm_cells: prim is NULL."};
  if (cells->dtype != BL_CELLS_F32 && cells->dtype != BL_CELLS_F64) throw Failure{BL_E_ARG, "bl_harm_cells: dtype must be BL_CELLS_F32 or BL_CELLS_F64."};
  if (reinterpret_cast<uintptr_t>(cells->prim) % (cells->dtype == BL_CELLS_F64 ? sizeof(double) : sizeof(float)) != 0)
    throw Failure{BL_E_ARG, "bl_harm_cells: prim is not aligned to its element type."};
  const bl_harm_header &h = grid->header;   // (counts within 1 ... 65536 and indices within n_prim: bl_harm_grid_create)
  int64_t needed = 0;
  const bool overflow = __builtin_mul_overflow(static_cast<int64_t>(h.n1) * h.n2, static_cast<int64_t>(h.n3) * h.n_prim, &needed);
  if (overflow || cells->n_elements < needed) throw Failure{BL_E_ARG, "bl_harm_cells: n_elements is smaller than n1 * n2 * n3 * n_prim."};
}

// The caller's array as bl_device_cells, for the checks and the ordering that read nothing but prim, dtype, n_elements, wait and stream
bl_device_cells HarmAsDeviceCells(const bl_harm_cells &cells) {
  bl_device_cells as{};
  as.prim = cells.prim;
  as.dtype = cells.dtype;
  as.wait = cells.wait;
  as.var_stride = as.block_stride = 1;
  as.n_elements = cells.n_elements;
  as.stream = cells.stream;
  return as;
}
constexpr const char *kHarmPointerRefusal = "bl_harm_cells: prim must be device memory of the context's device, with n_elements elements inside one allocation.";

// The grid's point table on the device: uploaded when this context sees the grid for the first time, kept for the cell arrays that follow
const double *HarmPointsOnDevice(bl_ctx *ctx, const bl_harm_grid &grid, hipStream_t stream) {
  bl_ctx::Grid &G = ctx->grid;
  if (G.harm_points_serial != grid.serial) {
    const size_t count = grid.points.size() * BL_HARM_POINT_DOUBLES;
    G.harm_points_serial = 0;
    G.d_harm_points.Ensure(count);
    Check(hipMemcpyAsync(G.d_harm_points.ptr, grid.points.data(), count * sizeof(double), hipMemcpyHostToDevice, stream), "point table upload");
    Check(hipStreamSynchronize(stream), "point table upload");
    G.host_bytes += static_cast<int64_t>(count * sizeof(double));
    G.harm_points_serial = grid.serial;
  }
  return G.d_harm_points.ptr;
}

// One launch of the staging kernel's harm form on `stream`: the eight variables into `cells` ([cell][8], or with plane_stride eight
// planes; null: none) and the entropy into `kappa` (null: none)
void LaunchHarmStaging(bl_ctx *ctx, const HarmCells &harm, float *cells, unsigned long long plane_stride, float *kappa, hipStream_t stream) {
  const bl_harm_grid &grid = *harm.grid;
  const bl_harm_header &h = grid.header;
  const bl_grid_desc &d = grid.desc;
  BlHarmSource src{};
  src.points = HarmPointsOnDevice(ctx, grid, stream);
  src.prims = harm.cells->prim;
  src.kappa = kappa;
  src.plane_stride = plane_stride;
  src.n1 = h.n1; src.n2 = h.n2; src.n3 = h.n3; src.n_prim = h.n_prim;
  const int index[9] = {d.ind_rho, d.ind_pgas, d.ind_uu1, d.ind_uu2, d.ind_uu3, d.ind_bb1, d.ind_bb2, d.ind_bb3, kappa != nullptr ? d.ind_kappa : 0};
  for (int q = 0; q < 9; q++) {
    if (index[q] < 0 || index[q] >= h.n_prim) throw Failure{BL_E_ARG, "bl_harm_cells: a variable index of the grid lies outside n_prim."};
    src.index[q] = index[q];
  }
  src.f64 = harm.cells->dtype == BL_CELLS_F64 ? 1 : 0;
  src.gamma_minus_one = static_cast<float>(d.plasma_gamma - 1.0);
  src.i_tiles = static_cast<unsigned int>((h.n1 + kHarmTileI - 1) / kHarmTileI);
  const unsigned long long k_chunks = (static_cast<unsigned long long>(h.n3) + kHarmTileK * kHarmChunkTiles - 1) / (kHarmTileK * kHarmChunkTiles);
  const unsigned long long blocks = k_chunks * static_cast<unsigned long long>(h.n2) * src.i_tiles;
  if (blocks >= (1ull << 24)) throw Failure{BL_E_ARG, "bl_harm_cells: the array has more tiles than one launch takes."};
  hipLaunchKernelGGL(bl_interleave_cells_kernel, dim3(static_cast<unsigned int>(blocks)), dim3(256), kHarmLdsBytes, stream, BlCellPlanes{}, cells, 0ull, 0, 0, 0,
                     static_cast<const unsigned long long *>(nullptr), 0ull, 0ull, src);
  Check(hipGetLastError(), "cell interleave kernel launch");
}

// The variables `order` of the caller's device array as the staging kernel's planes
BlCellPlanes DevicePlanes(const bl_device_cells &cells, const int *order, int count) {
  BlCellPlanes src{};
  const size_t element = cells.dtype == BL_CELLS_F64 ? sizeof(double) : sizeof(float);
  for (int v = 0; v < count; v++)
    src.base[v] = static_cast<const char *>(cells.prim) + static_cast<unsigned long long>(order[v]) * static_cast<unsigned long long>(cells.var_stride) * element;
  src.block_stride = static_cast<unsigned long long>(cells.block_stride);
  src.f64 = cells.dtype == BL_CELLS_F64 ? 1 : 0;
  return src;
}

// The staging on `stream` starts behind the work queued so far on the caller's stream (bl_device_cells::wait): an event, no host wait
void WaitForCallerCells(bl_ctx *ctx, const bl_device_cells &cells, hipStream_t stream) {
  if (cells.wait == 0) return;
  bl_ctx::Grid &G = ctx->grid;
  if (G.source_event == nullptr) Check(hipEventCreateWithFlags(&G.source_event, hipEventDisableTiming), "hipEventCreate");
  Check(hipEventRecord(G.source_event, static_cast<hipStream_t>(cells.stream)), "hipEventRecord");
  Check(hipStreamWaitEvent(stream, G.source_event, 0), "hipStreamWaitEvent");
}

// The planes of `g` - or, with `device_cells`, of the caller's device array - into `d_cells` as the grid's placement says, on `stream`;
// returns when the cells are in place (the caller's arrays are borrowed for the duration of bl_set_grid)
void UploadCellsAs(bl_ctx *ctx, const bl_grid_desc *g, const bl_device_cells *device_cells, const HarmCells *harm, DeviceBuffer<float> &d_cells, hipStream_t stream,
                   bool upload_origin) {
  bl_ctx::Grid &G = ctx->grid;
  const CellPlacement &pl = G.tables.placement;
  const size_t n_cells = pl.n_cells;
  d_cells.Ensure(n_cells * 8);
  BlCellPlanes src{};
  if (harm != nullptr) {   // (one block: the cells lie [k][j][i], no origins)
    if (pl.has_origin || n_cells != static_cast<size_t>(g->n_i) * g->n_j * g->n_k) throw Failure{BL_E_ARG, "Bad grid description."};
    WaitForCallerCells(ctx, *device_cells, stream);
    LaunchHarmStaging(ctx, *harm, d_cells.ptr, 0, nullptr, stream);
    Check(hipStreamSynchronize(stream), "grid upload");
    return;
  }
  if (device_cells != nullptr) {
    src = DevicePlanes(*device_cells, pl.order, 8);
    WaitForCallerCells(ctx, *device_cells, stream);
  } else {
    G.d_cell_planes.Ensure(n_cells * 8);
    for (int v = 0; v < 8; v++) {
      Check(hipMemcpyAsync(G.d_cell_planes.ptr + static_cast<size_t>(v) * n_cells, g->prim + static_cast<size_t>(pl.order[v]) * n_cells, n_cells * sizeof(float),
                           hipMemcpyHostToDevice, stream), "grid upload");
      src.base[v] = G.d_cell_planes.ptr + static_cast<size_t>(v) * n_cells;
    }
    src.block_stride = static_cast<unsigned long long>(pl.nb[0]) * pl.nb[1] * pl.nb[2];
    G.host_bytes += static_cast<int64_t>(n_cells * 8 * sizeof(float));
  }
  if (pl.has_origin && upload_origin) {
    G.d_block_origin.Ensure(pl.origin.size());
    Check(hipMemcpyAsync(G.d_block_origin.ptr, pl.origin.data(), pl.origin.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, stream), "grid upload");
    G.host_bytes += static_cast<int64_t>(pl.origin.size() * sizeof(unsigned long long));
  }
  LaunchCellStaging(ctx, src, 8, d_cells.ptr, stream);
  Check(hipStreamSynchronize(stream), "grid upload");
}

// The one upload step: each table of ctx->grid.tables into its buffer, once; the cells (into the time slice where there is one); then
// every pointer of BlGridDevice, from buffer base plus offset (BindGridTables)
void UploadGrid(bl_ctx *ctx, const bl_grid_desc *g, const bl_device_cells *device_cells, const HarmCells *harm, bl_ctx::SlowSlice *slice) {
  bl_ctx::Grid &G = ctx->grid;
  const GridTables &t = G.tables;
  DeviceBuffer<float> &d_cells = slice != nullptr ? slice->cells : G.d_cells;
  DeviceBuffer<float> &d_kappa = slice != nullptr ? slice->kappa : G.d_kappa;
  auto put = [&G](auto &buffer, const auto *data, size_t count, const char *what) {
    if (count == 0) return;
    buffer.Ensure(count);
    Check(hipMemcpy(buffer.ptr, data, count * sizeof(*data), hipMemcpyHostToDevice), what);
    G.host_bytes += static_cast<int64_t>(count * sizeof(*data));
  };
  EnsureStreams(ctx);
  UploadCellsAs(ctx, g, device_cells, harm, d_cells, ctx->stream, true);
  if (t.code_kappa && harm != nullptr) {   // the entropy where the harm array has it, through the same transpose
    d_kappa.Ensure(t.placement.n_cells);
    LaunchHarmStaging(ctx, *harm, nullptr, 0, d_kappa.ptr, ctx->stream);
    Check(hipStreamSynchronize(ctx->stream), "grid upload");
  } else if (t.code_kappa && device_cells != nullptr) {
    // the caller's plane where it lies, through the staging kernel: to the blocks' places in a merged array, else cell by cell
    d_kappa.Ensure(t.placement.n_cells);
    LaunchCellStaging(ctx, DevicePlanes(*device_cells, &g->ind_kappa, 1), 1, d_kappa.ptr, ctx->stream);
    Check(hipStreamSynchronize(ctx->stream), "grid upload");
  } else if (t.code_kappa) {   // (its own [k][j][i] array; block by block it lies in the caller's plane as the kernels read it)
    put(d_kappa, t.kappa.empty() ? g->prim + static_cast<size_t>(g->ind_kappa) * t.placement.n_cells : t.kappa.data(), t.placement.n_cells, "grid upload");
  }
  put(G.d_coords, t.coords.data(), t.coords.size(), "coordinate upload");
  put(G.d_buckets, t.buckets.data(), t.buckets.size(), "bucket upload");
  put(G.d_lattice, t.lattice.data(), t.lattice.size(), "lattice upload");
  put(G.d_fused_desc, t.fused_desc.data(), t.fused_desc.size(), "lattice upload");
  put(G.d_block_table, t.block_table.data(), t.block_table.size(), "block table upload");
  put(G.d_block_keys, t.block_keys.data(), t.block_keys.size(), "block table upload");
  if (t.dev.fmks) put(G.d_sks_map, g->sks_map, static_cast<size_t>(2) * g->sks_map_n1 * g->sks_map_n2, "sks_map upload");
  G.dev = BindGridTables(t, GridBases{d_cells.ptr, d_kappa.ptr, G.d_coords.ptr, G.d_buckets.ptr, G.d_lattice.ptr, G.d_fused_desc.ptr, G.d_block_table.ptr,
                                      G.d_block_keys.ptr, G.d_sks_map.ptr});
}

int FailBetweenRenders(bl_ctx *ctx, const Failure &failure) {   // (last_error is the render's to write while it runs)
  std::lock_guard<std::mutex> guard(ctx->render_lock);
  return Fail(ctx, failure);
}

// bl_set_grid, and bl_set_grid_slice with the time slice the cells go to. The cells come from the host planes g->prim, or with
// `device_cells` from the caller's device array (bl_set_grid_device, bl_set_grid_slice_device): everything else is one path.
int SetGrid(bl_ctx *ctx, const bl_grid_desc *g, const bl_device_cells *device_cells, bl_ctx::SlowSlice *slice, const HarmCells *harm = nullptr) {
  bl_ctx::Grid &G = ctx->grid;
  try {
    G.host_bytes = 0;
    if (harm != nullptr) {
      CheckHarmCells(harm->grid, harm->cells);
      // (the grid chose its variables, the entropy among them or not, under its own parameters: they must be this context's)
      if (harm->grid->code_kappa != (ctx->params.plasma_model == BL_PLASMA_CODE_KAPPA))
        throw Failure{BL_E_ARG, "bl_harm_grid: made with another plasma_model than the context's (one of them reads the electron entropy, plasma_model = code_kappa)."};
    } else if (device_cells != nullptr) CheckDeviceCells(*g, ctx->params.plasma_model == BL_PLASMA_CODE_KAPPA, device_cells);
    if (ctx->device == BL_DEVICE_NONE) throw Failure{BL_E_DEVICE, "Host-only context: no HIP device selected (the hot path has no CPU fallback)."};
    if (ctx->params.model_type != BL_MODEL_SIMULATION) throw Failure{BL_E_STATE, "bl_set_grid called in formula mode."};
    if (ctx->params.slow_light_on && slice == nullptr)
      throw Failure{BL_E_STATE, "slow_light_on = true: hand the time slices over with bl_set_grid_slice (or bl_slow_light_read)."};
    ValidateGridDescription(*g);
    if (device_cells == nullptr && g->prim == nullptr) throw Failure{BL_E_ARG, "Bad grid description."};
    Check(hipSetDevice(ctx->device), "hipSetDevice");
    if (device_cells != nullptr) CheckDevicePointer(ctx, *device_cells, harm != nullptr ? kHarmPointerRefusal : nullptr);
    // The next snapshot of a series - the geometry in place, to the bit, and the same variables: only the cells are new. They go up on
    // a stream of their own into the second cell array while a render of this context may be running on another host thread, and the
    // arrays change places once that render has ended. (With electron entropy from the grid there is a second array to double: the
    // long way.)
    const bool code_kappa = ctx->params.plasma_model == BL_PLASMA_CODE_KAPPA;
    int order_now[8];
    if (G.have && slice == nullptr && G.swappable && !code_kappa && SameGeometry(G.tables, *g) && GridVariableOrder(*g, false, order_now)
        && std::equal(order_now, order_now + 8, G.tables.placement.order) && g->n_var == G.meta.n_var
        && g->plasma_gamma == G.meta.plasma_gamma && g->plasma_gamma_i == G.meta.plasma_gamma_i && g->plasma_gamma_e == G.meta.plasma_gamma_e) {
      if (G.stream_upload == nullptr) Check(hipStreamCreateWithFlags(&G.stream_upload, hipStreamNonBlocking), "hipStreamCreate");
      UploadCellsAs(ctx, g, device_cells, harm, G.d_cells_back, G.stream_upload, false);
      std::lock_guard<std::mutex> guard(ctx->render_lock);
      std::swap(G.d_cells, G.d_cells_back);
      G.dev.cells = G.d_cells.ptr;
      G.meta = *g;
      return BL_OK;
    }
    std::lock_guard<std::mutex> guard(ctx->render_lock);   // (everything about the grid changes: not beside a render)
    G.have = false;   // a refused or failed grid leaves no grid behind (the previous one may be half overwritten)
    G.swappable = false;
    G.tables.geometry = 0;
    bl_grid_desc described = *g;
    if (device_cells != nullptr) described.prim = nullptr;   // (no host planes: the electron entropy plane is placed on the device)
    GridTables tables = BuildGridTables(ctx->params, described);
    const unsigned long long geometry = slice == nullptr ? tables.geometry : 0;   // (slow light locates per snapshot: no located samples are kept)
    tables.geometry = 0;
    G.tables = std::move(tables);
    UploadGrid(ctx, g, device_cells, harm, slice);
    G.tables.kappa = std::vector<float>();   // (as large as a cell plane, and on the device now)
    G.tables.geometry = geometry;
    G.meta = *g;
    G.swappable = slice == nullptr;   // (the time slices of slow light have no second array to change places with)
    G.have = true;
  } catch (const Failure &failure) {
    return FailBetweenRenders(ctx, failure);
  }
  return BL_OK;
}

int RefuseNoCells(bl_ctx *ctx, const bl_grid_desc *g) {   // (SetGrid reads a null description as "host planes")
  try {
    CheckDeviceCells(*g, false, nullptr);
  } catch (const Failure &failure) {
    return FailBetweenRenders(ctx, failure);
  }
  return BL_E_ARG;
}
}  // namespace

int bl_set_grid(bl_ctx *ctx, const bl_grid_desc *g) {
  if (ctx == nullptr || g == nullptr) return BL_E_ARG;
  return SetGrid(ctx, g, nullptr, nullptr);
}

int bl_set_grid_device(bl_ctx *ctx, const bl_grid_desc *g, const bl_device_cells *cells) {
  if (ctx == nullptr || g == nullptr) return BL_E_ARG;
  if (cells == nullptr) return RefuseNoCells(ctx, g);
  return SetGrid(ctx, g, cells, nullptr);
}

size_t bl_device_cells_sizeof(void) { return sizeof(bl_device_cells); }

int64_t bl_grid_host_bytes(const bl_ctx *ctx) { return ctx != nullptr ? ctx->grid.host_bytes : 0; }

int bl_context_device(const bl_ctx *ctx) { return ctx != nullptr ? ctx->device : BL_DEVICE_NONE; }

namespace {
int SetGridSlice(bl_ctx *ctx, int slice, const bl_grid_desc *g, const bl_device_cells *device_cells, double time, const HarmCells *harm = nullptr) {
  const bl_params &p = ctx->params;
  if (p.model_type != BL_MODEL_SIMULATION || !p.slow_light_on) return FailBetweenRenders(ctx, Failure{BL_E_STATE, "bl_set_grid_slice needs slow_light_on = true."});
  if (slice < 0 || slice >= p.slow_chunk_size) return FailBetweenRenders(ctx, Failure{BL_E_ARG, "Time slice index outside slow_chunk_size."});
  ctx->slow_slices.resize(p.slow_chunk_size);
  bl_ctx::SlowSlice &target = ctx->slow_slices[slice];
  const int rc = SetGrid(ctx, g, device_cells, &target, harm);
  if (rc != BL_OK) return rc;
  target.time = time;
  target.set = true;
  return BL_OK;
}
}  // namespace

int bl_set_grid_slice(bl_ctx *ctx, int slice, const bl_grid_desc *g, double time) {
  if (ctx == nullptr || g == nullptr) return BL_E_ARG;
  return SetGridSlice(ctx, slice, g, nullptr, time);
}

int bl_set_grid_slice_device(bl_ctx *ctx, int slice, const bl_grid_desc *g, const bl_device_cells *cells, double time) {
  if (ctx == nullptr || g == nullptr) return BL_E_ARG;
  if (cells == nullptr) return RefuseNoCells(ctx, g);
  return SetGridSlice(ctx, slice, g, cells, time);
}

// The harm calls: the grid's own description (for simulation_coord = fmks with its look-up table built), the caller's array in place of planes
int bl_set_grid_device_harm(bl_ctx *ctx, bl_harm_grid *grid, const bl_harm_cells *cells) {
  if (ctx == nullptr) return BL_E_ARG;
  try {
    CheckHarmCells(grid, cells);
  } catch (const Failure &failure) {
    return FailBetweenRenders(ctx, failure);
  }
  const bl_device_cells as = HarmAsDeviceCells(*cells);
  const HarmCells harm{grid, cells};
  return SetGrid(ctx, bl_harm_grid_desc(grid, 0), &as, nullptr, &harm);
}

int bl_set_grid_slice_device_harm(bl_ctx *ctx, int slice, bl_harm_grid *grid, const bl_harm_cells *cells, double time) {
  if (ctx == nullptr) return BL_E_ARG;
  try {
    CheckHarmCells(grid, cells);
  } catch (const Failure &failure) {
    return FailBetweenRenders(ctx, failure);
  }
  const bl_device_cells as = HarmAsDeviceCells(*cells);
  const HarmCells harm{grid, cells};
  return SetGridSlice(ctx, slice, bl_harm_grid_desc(grid, 0), &as, time, &harm);
}

int bl_harm_convert_device(bl_ctx *ctx, const bl_harm_grid *grid, const bl_harm_cells *cells, float *out_planes) {
  if (ctx == nullptr) return BL_E_ARG;
  try {
    CheckHarmCells(grid, cells);
    if (out_planes == nullptr || reinterpret_cast<uintptr_t>(out_planes) % sizeof(float) != 0)
      throw Failure{BL_E_ARG, "bl_harm_convert_device: out_planes is NULL or not aligned to float."};
    if (ctx->device == BL_DEVICE_NONE) throw Failure{BL_E_DEVICE, "Host-only context: no HIP device selected (the hot path has no CPU fallback)."};
    Check(hipSetDevice(ctx->device), "hipSetDevice");
    const bl_device_cells as = HarmAsDeviceCells(*cells);
    CheckDevicePointer(ctx, as, kHarmPointerRefusal);
    const bl_harm_header &h = grid->header;
    const unsigned long long n_cells = static_cast<unsigned long long>(h.n1) * h.n2 * h.n3;
    bl_device_cells target{};
    target.prim = out_planes;
    target.dtype = BL_CELLS_F32;
    target.n_elements = static_cast<int64_t>(n_cells * (grid->code_kappa ? 9 : 8));
    CheckDevicePointer(ctx, target, "bl_harm_convert_device: out_planes must be device memory of the context's device holding every plane inside one allocation.");
    EnsureStreams(ctx);
    std::lock_guard<std::mutex> guard(ctx->render_lock);   // (the point table is the context's: not beside a render or another staging)
    WaitForCallerCells(ctx, as, ctx->stream);
    const HarmCells harm{grid, cells};
    LaunchHarmStaging(ctx, harm, out_planes, n_cells, grid->code_kappa ? out_planes + 8 * n_cells : nullptr, ctx->stream);
    Check(hipStreamSynchronize(ctx->stream), "primitive conversion");
  } catch (const Failure &failure) {
    return FailBetweenRenders(ctx, failure);
  }
  return BL_OK;
}

size_t bl_harm_cells_sizeof(void) { return sizeof(bl_harm_cells); }

int bl_shift_grid_slices(bl_ctx *ctx, int count) {
  if (ctx == nullptr) return BL_E_ARG;
  const int chunk = static_cast<int>(ctx->slow_slices.size());
  if (count < 0 || count > chunk) return Fail(ctx, Failure{BL_E_ARG, "Bad slice shift."});
  // prim[n].Swap(prim[n - count]) for n = chunk - 1 ... count (simulation_reader.cpp:289-296)
  for (int n = chunk - 1; n >= count && count > 0; n--) std::swap(ctx->slow_slices[n], ctx->slow_slices[n - count]);
  return BL_OK;
}

int bl_set_snapshot(bl_ctx *ctx, int snapshot) {
  if (ctx == nullptr || snapshot < 0) return BL_E_ARG;
  ctx->snapshot = snapshot;
  return BL_OK;
}

int bl_render_num_images(const bl_ctx *ctx) { return ctx != nullptr ? ctx->render_num_images : 0; }

int bl_image_num_quantities(const bl_ctx *ctx) {
  return ctx != nullptr ? ctx->image_num_quantities * bl_num_variants(ctx) : -1;
}

int bl_num_variants(const bl_ctx *ctx) { return ctx != nullptr ? static_cast<int>(ResolveVariants(ctx).list.size()) : -1; }

int bl_set_electron_models(bl_ctx *ctx, int n, const double *rat_low, const double *rat_high) {
  if (ctx == nullptr) return BL_E_ARG;
  if (const Refused refused = CheckElectronModels(ctx, n, rat_low, rat_high)) return Fail(ctx, *refused);
  std::lock_guard<std::mutex> guard(ctx->render_lock);
  StoreElectronModels(ctx, n, rat_low, rat_high);
  return BL_OK;
}

int bl_num_electron_models(const bl_ctx *ctx) { return ctx != nullptr ? static_cast<int>(ctx->models.size()) : -1; }

int bl_set_density_units(bl_ctx *ctx, int n, const double *rho_cgs) {
  if (ctx == nullptr) return BL_E_ARG;
  if (const Refused refused = CheckDensityUnits(ctx, n, rho_cgs)) return Fail(ctx, *refused);
  std::lock_guard<std::mutex> guard(ctx->render_lock);
  StoreDensityUnits(ctx, n, rho_cgs);
  return BL_OK;
}

int bl_num_density_units(const bl_ctx *ctx) { return ctx != nullptr ? static_cast<int>(ctx->units.size()) : -1; }

int bl_set_polarized_variants_electrons(bl_ctx *ctx, int n, const double *rat_low, const double *rat_high, const double *rho_cgs, const double *sigma_max,
                                        const bl_electron_mix *mix) {
  if (ctx == nullptr) return BL_E_ARG;
  std::vector<const char *> warnings;
  if (const Refused refused = CheckPolarizedVariants(ctx, n, rat_low, rat_high, rho_cgs, sigma_max, mix, &warnings)) return Fail(ctx, *refused);
  for (const char *warning : warnings) Warn(ctx, warning);
  std::lock_guard<std::mutex> guard(ctx->render_lock);
  StorePolarizedVariants(ctx, n, rat_low, rat_high, rho_cgs, sigma_max, mix);
  return BL_OK;
}

int bl_set_polarized_variants_sigma(bl_ctx *ctx, int n, const double *rat_low, const double *rat_high, const double *rho_cgs, const double *sigma_max) {
  return bl_set_polarized_variants_electrons(ctx, n, rat_low, rat_high, rho_cgs, sigma_max, nullptr);
}

int bl_polarized_variant_electrons(const bl_ctx *ctx, int variant, bl_electron_mix *out) {
  if (ctx == nullptr || out == nullptr) return BL_E_ARG;
  const int n = static_cast<int>(ctx->triples.size());
  if (variant < 0 || variant >= std::max(1, n)) return BL_E_ARG;
  *out = (n > 0 && ctx->triples_mix) ? ctx->triples[variant].mix : BlockMix(ctx->params);
  return BL_OK;
}

int bl_set_polarized_variants(bl_ctx *ctx, int n, const double *rat_low, const double *rat_high, const double *rho_cgs) {
  return bl_set_polarized_variants_sigma(ctx, n, rat_low, rat_high, rho_cgs, nullptr);
}

int bl_num_polarized_variants(const bl_ctx *ctx) { return ctx != nullptr ? static_cast<int>(ctx->triples.size()) : -1; }

int bl_set_sigma_cuts(bl_ctx *ctx, int n, const double *sigma_max) {
  if (ctx == nullptr) return BL_E_ARG;
  if (const Refused refused = CheckSigmaCuts(ctx, n, sigma_max)) return Fail(ctx, *refused);
  std::lock_guard<std::mutex> guard(ctx->render_lock);
  StoreSigmaCuts(ctx, n, sigma_max);
  return BL_OK;
}

int bl_num_sigma_cuts(const bl_ctx *ctx) { return ctx != nullptr ? static_cast<int>(ctx->sigma_cuts.size()) : -1; }

int bl_set_electron_mixes(bl_ctx *ctx, int n, const bl_electron_mix *mix) {
  if (ctx == nullptr) return BL_E_ARG;
  std::vector<const char *> warnings;
  if (const Refused refused = CheckElectronMixes(ctx, n, mix, &warnings)) return Fail(ctx, *refused);
  for (const char *warning : warnings) Warn(ctx, warning);
  std::lock_guard<std::mutex> guard(ctx->render_lock);
  StoreElectronMixes(ctx, n, mix);
  return BL_OK;
}

int bl_num_electron_mixes(const bl_ctx *ctx) { return ctx != nullptr ? static_cast<int>(ctx->mixes.size()) : -1; }

int bl_electron_mix_get(const bl_ctx *ctx, int e, bl_electron_mix *out) {
  if (ctx == nullptr || out == nullptr) return BL_E_ARG;
  const int n = static_cast<int>(ctx->mixes.size());
  if (e < 0 || e >= std::max(1, n)) return BL_E_ARG;
  *out = n > 0 ? ctx->mixes[e] : BlockMix(ctx->params);
  return BL_OK;
}

int bl_set_cameras(bl_ctx *ctx, int n, const double *th_deg, const double *ph_deg) {
  if (ctx == nullptr) return BL_E_ARG;
  if (n < 0 || n > BL_MAX_CAMERAS || (n > 0 && (th_deg == nullptr || ph_deg == nullptr)))
    return Fail(ctx, Failure{BL_E_ARG, "bl_set_cameras needs 0 <= n <= " + std::to_string(BL_MAX_CAMERAS) + " and both arrays of angles."});
  std::vector<bl_ctx::Camera> list;
  if (const Refused refused = CheckCameras(ctx, n, th_deg, ph_deg, &list)) return Fail(ctx, *refused);
  std::lock_guard<std::mutex> guard(ctx->render_lock);
  StoreCameras(ctx, std::move(list));
  return BL_OK;
}

int bl_num_cameras(const bl_ctx *ctx) { return ctx != nullptr ? static_cast<int>(ctx->cameras.size()) : -1; }

int bl_camera_frame_get_camera(const bl_ctx *ctx, int camera, bl_camera_frame *out) {
  if (ctx == nullptr || out == nullptr) return BL_E_ARG;
  const int n = static_cast<int>(ctx->cameras.size());
  if (camera < 0 || camera >= std::max(1, n)) return BL_E_ARG;
  *out = n == 0 ? ctx->block_frame : ctx->cameras[camera].frame;
  return BL_OK;
}

int bl_cameras_get(const bl_ctx *ctx, int n, double *th_deg, double *ph_deg) {
  if (ctx == nullptr || n < 0 || (n > 0 && (th_deg == nullptr || ph_deg == nullptr))) return BL_E_ARG;
  for (int c = 0; c < n && c < static_cast<int>(ctx->cameras.size()); c++) th_deg[c] = ctx->cameras[c].th_deg, ph_deg[c] = ctx->cameras[c].ph_deg;
  return BL_OK;
}

int bl_variants_get(const bl_ctx *ctx, int n, double *rat_low, double *rat_high, double *rho_cgs, double *sigma_max, int *flags) {
  if (ctx == nullptr || n < 0) return BL_E_ARG;
  const Variants variants = ResolveVariants(ctx);
  for (int v = 0; v < n && v < static_cast<int>(variants.list.size()); v++) {
    if (rat_low != nullptr) rat_low[v] = variants.list[v].rat_low;
    if (rat_high != nullptr) rat_high[v] = variants.list[v].rat_high;
    if (rho_cgs != nullptr) rho_cgs[v] = variants.list[v].rho;
    if (sigma_max != nullptr) sigma_max[v] = variants.list[v].sigma_max;
  }
  if (flags != nullptr) *flags = (ctx->triples_cut ? BL_VARIANTS_TRIPLES_CUT : 0) | (ctx->triples_mix ? BL_VARIANTS_TRIPLES_MIX : 0);
  return BL_OK;
}

int bl_set_frequencies(bl_ctx *ctx, int n, const double *hz) {
  if (ctx == nullptr) return BL_E_ARG;
  if (const Refused refused = CheckFrequencies(ctx, n, hz)) return Fail(ctx, *refused);
  std::lock_guard<std::mutex> guard(ctx->render_lock);
  StoreFrequencies(ctx, n, hz);
  return BL_OK;
}

int bl_num_frequencies(const bl_ctx *ctx) { return ctx != nullptr ? ctx->frequencies_set : -1; }

int bl_apply_sweep_lists(bl_ctx *ctx, const bl_sweep_lists *lists) {
  if (ctx == nullptr || lists == nullptr) return BL_E_ARG;
  const bl_sweep_all all = {lists->sweep, lists->cuts, lists->cameras, lists->electrons, nullptr};
  return bl_apply_sweep_all(ctx, &all);
}

int bl_apply_sweep_all(bl_ctx *ctx, const bl_sweep_all *lists) {
  if (ctx == nullptr || lists == nullptr) return BL_E_ARG;
  const bl_sweep none = {};
  const bl_sweep *sweep = lists->sweep != nullptr ? lists->sweep : &none;
  const bl_sweep_cuts *cuts = lists->cuts;
  const bl_sweep_electrons *e = lists->electrons;
  const bool electrons = e != nullptr && (e->n_power_frac != 0 || e->n_p != 0 || e->n_gamma_min != 0 || e->n_gamma_max != 0 || e->n_kappa_frac != 0
                                          || e->n_kappa != 0 || e->n_w != 0);
  // 1. What the lists mean (bl_params.cpp; a list error is BL_E_INPUT in the resolver's words). With an electron list the tuples come
  // first: triples with a mix each, all three lists of `s` of their number. Without one the three lists wait behind the cut-count bound.
  char err[512] = "";
  const auto list_error = [&]() {   // (err is in Fail's form already)
    ctx->last_error = err;
    return BL_E_INPUT;
  };
  bl_sweep s;
  bl_electron_mix mix[BL_MAX_SWEEP];
  int polarized = 0, n_cameras = 0, th_given = 0, ph_given = 0;
  double th[BL_MAX_SWEEP], ph[BL_MAX_SWEEP];
  if (electrons && bl_sweep_electrons_resolve(e, sweep, &ctx->params, nullptr, &s, mix, err, sizeof err) != BL_OK) return list_error();
  if (lists->cameras != nullptr && bl_sweep_cameras_resolve(lists->cameras, &n_cameras, th, ph, &th_given, &ph_given, err, sizeof err) != BL_OK)
    return list_error();
  // 2. Every check, in the order the calls of the older entry points made them; the first failure is the call's, and nothing is stored
  std::vector<bl_ctx::Camera> cameras;
  Refused refused;
  if (n_cameras > 0) refused = CheckCameras(ctx, n_cameras, th_given ? th : nullptr, ph_given ? ph : nullptr, &cameras);
  if (refused) return Fail(ctx, *refused);
  if (cuts != nullptr && (cuts->n_sigma_max < 0 || cuts->n_sigma_max > BL_MAX_SWEEP))
    return Fail(ctx, Failure{BL_E_INPUT, "Too many entries in a sweep list: at most " + std::to_string(BL_MAX_SWEEP) + " for this build."});
  if (!electrons && bl_sweep_resolve(sweep, &ctx->params, &s, &polarized, err, sizeof err) != BL_OK) return list_error();
  const bool has_triples = electrons || (polarized && (s.n_rat_low > 0 || s.n_rho_cgs > 0)), has_cuts = cuts != nullptr && cuts->n_sigma_max > 0;
  const bool has_models = !has_triples && s.n_rat_low > 0, has_units = !has_triples && s.n_rho_cgs > 0;
  std::vector<const char *> warnings;
  if (electrons && has_cuts) refused = CheckSigmaCuts(ctx, cuts->n_sigma_max, cuts->sigma_max);   // (with tuples the cuts come first)
  if (!refused && has_triples)
    refused = CheckPolarizedVariants(ctx, s.n_rho_cgs, s.rat_low, s.rat_high, s.rho_cgs, nullptr, electrons ? mix : nullptr, &warnings);
  if (!refused && has_models) refused = CheckElectronModels(ctx, s.n_rat_low, s.rat_low, s.rat_high);
  if (!refused && has_units) refused = CheckDensityUnits(ctx, s.n_rho_cgs, s.rho_cgs);
  if (!refused && !electrons && has_cuts) refused = CheckSigmaCuts(ctx, cuts->n_sigma_max, cuts->sigma_max);
  // ... and the frequencies, last: the list's own bound (a struct the parser did not fill), the setter's checks, and the sweep's own
  // refusal - its files are one-frequency files, and a one-frequency run refines by its own image
  const bl_sweep_frequencies *freq = lists->frequencies;
  const bool has_frequencies = freq != nullptr && freq->n != 0;
  if (!refused && has_frequencies) {
    if (freq->n < 0 || freq->n > BL_MAX_SWEEP)
      refused = Failure{BL_E_INPUT, "Too many entries in a sweep list: at most " + std::to_string(BL_MAX_SWEEP) + " for this build."};
    else if (freq->n >= 2 && ctx->params.adaptive_max_level > 0)
      refused = Failure{BL_E_UNSUPPORTED, "Frequencies: adaptive refinement reads one image; a sweep of n >= 2 frequencies needs adaptive_max_level = 0."};
    else
      refused = CheckFrequencies(ctx, freq->n, freq->hz);
  }
  if (refused) return Fail(ctx, *refused);
  // 3. Every list the call carries, under one hold of the lock: no render sees half a sweep. A list it does not carry stays.
  {
    std::lock_guard<std::mutex> guard(ctx->render_lock);
    if (n_cameras > 0) StoreCameras(ctx, std::move(cameras));
    if (has_triples) StorePolarizedVariants(ctx, s.n_rho_cgs, s.rat_low, s.rat_high, s.rho_cgs, nullptr, electrons ? mix : nullptr);
    if (has_models) StoreElectronModels(ctx, s.n_rat_low, s.rat_low, s.rat_high);
    if (has_units) StoreDensityUnits(ctx, s.n_rho_cgs, s.rho_cgs);
    if (has_cuts) StoreSigmaCuts(ctx, cuts->n_sigma_max, cuts->sigma_max);
    if (has_frequencies) StoreFrequencies(ctx, freq->n, freq->hz);
  }
  for (const char *warning : warnings) Warn(ctx, warning);
  return BL_OK;
}

// The three older entry points: forwards
int bl_apply_sweeps_cameras(bl_ctx *ctx, const bl_sweep *sweep, const bl_sweep_cuts *cuts, const bl_sweep_cameras *cameras) {
  if (ctx == nullptr || sweep == nullptr) return BL_E_ARG;
  const bl_sweep_lists lists = {const_cast<bl_sweep *>(sweep), const_cast<bl_sweep_cuts *>(cuts), const_cast<bl_sweep_cameras *>(cameras), nullptr};
  return bl_apply_sweep_lists(ctx, &lists);
}

int bl_apply_sweeps(bl_ctx *ctx, const bl_sweep *sweep, const bl_sweep_cuts *cuts) { return bl_apply_sweeps_cameras(ctx, sweep, cuts, nullptr); }

int bl_apply_sweep(bl_ctx *ctx, const bl_sweep *sweep) { return bl_apply_sweeps_cameras(ctx, sweep, nullptr, nullptr); }

int bl_camera_frame_get(const bl_ctx *ctx, bl_camera_frame *out) {
  if (ctx == nullptr || out == nullptr) return BL_E_ARG;
  *out = ctx->frame;
  return BL_OK;
}

int bl_frequencies(const bl_ctx *ctx, double *out, int n) {
  if (ctx == nullptr || out == nullptr) return BL_E_ARG;
  for (int l = 0; l < n && l < static_cast<int>(ctx->frequencies.size()); l++) out[l] = ctx->frequencies[l];
  return BL_OK;
}

void *bl_host_alloc(bl_ctx *ctx, size_t bytes) {
  if (ctx == nullptr || ctx->device == BL_DEVICE_NONE || bytes == 0) return nullptr;
  void *p = nullptr;
  if (hipSetDevice(ctx->device) != hipSuccess || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  return p;
}

void bl_host_free(bl_ctx *ctx, void *p) {
  if (ctx == nullptr || p == nullptr || ctx->device == BL_DEVICE_NONE) return;
  (void)hipSetDevice(ctx->device);
  (void)hipHostFree(p);
}

int bl_set_geodesic_reuse(bl_ctx *ctx, int on) {
  if (ctx == nullptr) return BL_E_ARG;
  std::lock_guard<std::mutex> guard(ctx->render_lock);   // (not beside a render of this context)
  ctx->geodesic_reuse = on ? 1 : 0;
  if (!on && ctx->device != BL_DEVICE_NONE) {   // what was kept goes back to the device
    (void)hipSetDevice(ctx->device);
    DropResident(ctx);
    ctx->resident.parked = false;
    ctx->resident.store.Free();
    ctx->resident.pending = false;
  }
  return BL_OK;
}

int bl_set_overlap(bl_ctx *ctx, int on) {
  if (ctx == nullptr) return BL_E_ARG;
  ctx->overlap_chunks = on ? 1 : 0;
  return BL_OK;
}

int bl_debug_set_guard_band(bl_ctx *ctx, double relative_width) {
  if (ctx == nullptr || !(relative_width >= 0.0)) return BL_E_ARG;
  ctx->guard_band = relative_width;
  return BL_OK;
}

int bl_device_count(void) {
  int count = 0;
  return hipGetDeviceCount(&count) == hipSuccess ? count : 0;
}

int bl_set_undefined_policy(bl_ctx *ctx, int policy) {
  if (ctx == nullptr || policy < 0 || policy > (BL_UNDEFINED_EDGE | BL_UNDEFINED_KAPPA)) return BL_E_ARG;
  ctx->undefined_policy = policy;
  return BL_OK;
}

int bl_set_arithmetic(bl_ctx *ctx, int mode) {
  if (ctx == nullptr || (mode != BL_ARITH_EXACT && mode != BL_ARITH_TOLERANT)) return BL_E_ARG;
  ctx->arithmetic = mode;
  return BL_OK;
}

int bl_set_reproducible(bl_ctx *ctx, int on) {
  if (ctx == nullptr) return BL_E_ARG;
  ctx->reproducible = on ? 1 : 0;
  return BL_OK;
}

int bl_set_tail_policy(bl_ctx *ctx, int policy) {
  if (ctx == nullptr || policy < BL_TAIL_AUTO || policy > BL_TAIL_SPLIT) return BL_E_ARG;
  ctx->tail_policy = policy;
  return BL_OK;
}

int bl_set_caller_stream(bl_ctx *ctx, void *stream, int enabled) {
  if (ctx == nullptr) return BL_E_ARG;
  ctx->caller_stream = static_cast<hipStream_t>(stream);
  ctx->caller_stream_set = enabled != 0;
  return BL_OK;
}

namespace {
// bl_adaptive_refine_device's image on the device's side, before the kernel reads it: device memory of this context's device, and
// `bytes_needed` bytes from `image` inside one allocation (what CheckDevicePointer asks of bl_set_grid_device's cells)
void CheckDeviceImage(bl_ctx *ctx, const double *image, unsigned long long bytes_needed) {
  const Failure refusal{BL_E_ARG, "bl_adaptive_refine_device: image must be device memory of the context's device that holds the examined row to its end inside one "
                                  "allocation; an image in host memory goes through bl_adaptive_refine."};
  hipPointerAttribute_t attributes{};
  if (hipPointerGetAttributes(&attributes, image) != hipSuccess) {
    (void)hipGetLastError();   // (an address the runtime does not know: not an error of this context's)
    throw refusal;
  }
  if (attributes.type != hipMemoryTypeDevice || attributes.device != ctx->device) throw refusal;
  hipDeviceptr_t first = nullptr;
  size_t bytes = 0;
  if (hipMemGetAddressRange(&first, &bytes, const_cast<double *>(image)) != hipSuccess) {
    (void)hipGetLastError();
    throw refusal;
  }
  const unsigned long long lo = reinterpret_cast<unsigned long long>(first), at = reinterpret_cast<unsigned long long>(image);
  if (at < lo || at - lo > bytes || bytes_needed > bytes - (at - lo)) throw refusal;
}
}  // namespace

int bl_adaptive_refine_device(bl_ctx *ctx, int level, int n_blocks, const int32_t *block_locs, const double *image, uint8_t *refine_flags,
                              int32_t *n_refined, int32_t *next_locs) {
  if (ctx == nullptr || image == nullptr || refine_flags == nullptr || n_refined == nullptr || n_blocks < 0) return BL_E_ARG;
  std::lock_guard<std::mutex> guard(ctx->render_lock);   // (the context's stream and scratch: not beside a render of it)
  try {
    if (ctx->device == BL_DEVICE_NONE)
      throw Failure{BL_E_DEVICE, "Host-only context: no HIP device selected (bl_adaptive_refine_device reads the image in device memory; bl_adaptive_refine decides on the host)."};
    BlRefinePlan plan;
    if (int rc = bl_refine_plan(ctx, level, n_blocks, block_locs, n_refined, &plan)) return rc;
    if (!plan.decide || n_blocks == 0) {   // (no block refines: nothing to launch)
      for (int b = 0; b < n_blocks; b++) refine_flags[b] = 0;
      return BL_OK;
    }
    if (plan.bs == 1 && (plan.cuts.frac[BL_REFINE_ABS_GRAD] >= 0.0 || plan.cuts.frac[BL_REFINE_REL_GRAD] >= 0.0))
      throw Failure{BL_E_UNSUPPORTED, "bl_adaptive_refine_device: with adaptive_block_size = 1 a gradient criterion reads the pixel beside its one-pixel block, outside "
                                      "the block (as bl_adaptive_refine and the reference do): there is no defined result to reproduce."};
    Check(hipSetDevice(ctx->device), "hipSetDevice");
    const unsigned long long row_pixels = static_cast<unsigned long long>(plan.n_pix);
    CheckDeviceImage(ctx, image, (static_cast<unsigned long long>(plan.row) + 1ull) * row_pixels * sizeof(double));
    EnsureStreams(ctx);
    hipStream_t stream = ctx->stream;
    if (ctx->caller_stream_set) {   // bl_set_caller_stream: what the caller queued there so far (the fill of `image`) is ahead of the kernel
      if (ctx->caller_event == nullptr) Check(hipEventCreateWithFlags(&ctx->caller_event, hipEventDisableTiming), "hipEventCreate");
      Check(hipEventRecord(ctx->caller_event, ctx->caller_stream), "event on the caller's stream");
      Check(hipStreamWaitEvent(stream, ctx->caller_event, 0), "stream wait");
    }
    BlRefineArgs args{};
    args.row = image + plan.row * static_cast<size_t>(row_pixels);
    if (level > 0) {
      ctx->d_refine_locs.Ensure(static_cast<size_t>(n_blocks) * 2);
      Check(hipMemcpyAsync(ctx->d_refine_locs.ptr, block_locs, static_cast<size_t>(n_blocks) * 2 * sizeof(int), hipMemcpyHostToDevice, stream), "block_locs upload");
      args.block_locs = ctx->d_refine_locs.ptr;
    }
    ctx->d_refine_flags.Ensure(static_cast<size_t>(n_blocks));
    args.flags = ctx->d_refine_flags.ptr;
    args.n_blocks = n_blocks;
    args.level = level;
    args.bs = plan.bs;
    args.res = plan.res;
    args.root = plan.root;
    args.linear_num_blocks = plan.linear_num_blocks;
    args.camera_width = plan.camera_width;
    args.cuts = plan.cuts;
    args.regions = plan.regions;
    Check(bl_launch_refine(&args, stream), "refinement kernel launch");
    Check(hipMemcpyAsync(refine_flags, ctx->d_refine_flags.ptr, static_cast<size_t>(n_blocks), hipMemcpyDeviceToHost, stream), "refinement flags download");
    Check(hipStreamSynchronize(stream), "kernel execution");
    *n_refined = bl_refine_children(plan, level, n_blocks, block_locs, refine_flags, next_locs);
  } catch (const Failure &failure) {
    return Fail(ctx, failure);
  }
  return BL_OK;
}

int bl_debug_set_switches(bl_ctx *ctx, uint32_t switches) {
  if (ctx == nullptr) return BL_E_ARG;
  ctx->switches = switches;
  return BL_OK;
}

int bl_set_scratch_limit(bl_ctx *ctx, uint64_t bytes) {
  if (ctx == nullptr || bytes < (1ull << 20)) return BL_E_ARG;
  ctx->scratch_limit = bytes;
  return BL_OK;
}

int bl_debug_math(bl_ctx *ctx, int op, int64_t n, const double *x, const double *y, double *out) {
  if (ctx == nullptr || x == nullptr || out == nullptr || n <= 0) return BL_E_ARG;
  try {
    if (op == 40 || op == 41) {   // the locate step's angles of m points against a lattice: the arrays must hold the layout the header gives
      if (y == nullptr || n < 4) throw Failure{BL_E_ARG, "bl_debug_math: ops 40 and 41 take the lattice in y."};
      const double m = x[0], n_th = x[2], n_ph = x[3];
      if (!(m >= 1.0 && n_th >= 2.0 && n_ph >= 2.0 && n_th <= 65535.0 && n_ph <= 65535.0) || m != std::floor(m) || n_th != std::floor(n_th) || n_ph != std::floor(n_ph)
          || 16.0 * m > static_cast<double>(n) || 2.0 * (n_th + n_ph) + 2.0 > static_cast<double>(n))
        throw Failure{BL_E_ARG, "bl_debug_math: ops 40 and 41 need n >= 16 m and n >= 2 (n_th + n_ph) + 2."};
    }
    if (ctx->device == BL_DEVICE_NONE) throw Failure{BL_E_DEVICE, "Host-only context: no HIP device selected."};
    Check(hipSetDevice(ctx->device), "hipSetDevice");
    EnsureStreams(ctx);
    DeviceBuffer<double> dx, dy, dout;
    dx.Ensure(n);
    dout.Ensure(n);
    Check(hipMemcpy(dx.ptr, x, n * sizeof(double), hipMemcpyHostToDevice), "upload");
    if (y != nullptr) {
      dy.Ensure(n);
      Check(hipMemcpy(dy.ptr, y, n * sizeof(double), hipMemcpyHostToDevice), "upload");
    }
    hipError_t err = bl_launch_debug_math(op, n, dx.ptr, y != nullptr ? dy.ptr : nullptr, dout.ptr, ctx->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(ctx->stream);
    if (err == hipSuccess) err = hipMemcpy(out, dout.ptr, n * sizeof(double), hipMemcpyDeviceToHost);
    dx.Free(); dy.Free(); dout.Free();
    Check(err, "bl_debug_math");
  } catch (const Failure &failure) {
    return Fail(ctx, failure);
  }
  return BL_OK;
}

int bl_get_stats(const bl_ctx *ctx, bl_stats *out) {
  if (ctx == nullptr || out == nullptr) return BL_E_ARG;
  *out = ctx->stats;
  return BL_OK;
}

const char *bl_last_error(const bl_ctx *ctx) { return ctx != nullptr ? ctx->last_error.c_str() : ""; }
const char *bl_last_global_error(void) { return g_global_error.c_str(); }
const char *bl_warnings(const bl_ctx *ctx) { return ctx != nullptr ? ctx->warnings.c_str() : ""; }

void bl_warnings_clear(bl_ctx *ctx) {
  if (ctx != nullptr) ctx->warnings.clear();
}

void bl_free(bl_ctx *ctx) {
  if (ctx == nullptr) return;
  if (ctx->device == BL_DEVICE_NONE) {
    delete ctx;
    return;
  }
  (void)hipSetDevice(ctx->device);
  ctx->grid.d_cells.Free(); ctx->grid.d_kappa.Free(); ctx->grid.d_coords.Free(); ctx->grid.d_buckets.Free(); ctx->slot[0].Free(); ctx->slot[1].Free();
  ctx->d_freq.Free(); ctx->d_pixel_map.Free();
  ctx->d_block_locs.Free(); ctx->d_refine_locs.Free(); ctx->d_refine_flags.Free(); ctx->d_tile_order.Free(); ctx->d_mirror_out.Free(); ctx->d_cameras.Free(); ctx->d_render_params.Free(); ctx->d_render.Free(); ctx->d_shade_cold.Free(); ctx->d_pol_variant_table.Free(); ctx->d_pol_variant_args.Free(); ctx->d_image.Free(); ctx->d_camera_pos.Free(); ctx->d_camera_dir.Free();
  ctx->d_out_sample_num.Free(); ctx->d_out_flags.Free();
  for (auto &e : ctx->events)
    if (e != nullptr) (void)hipEventDestroy(e);
  if (ctx->host_counters != nullptr) (void)hipHostFree(ctx->host_counters);
  if (ctx->caller_event != nullptr) (void)hipEventDestroy(ctx->caller_event);
  if (ctx->stream != nullptr) (void)hipStreamDestroy(ctx->stream);
  if (ctx->stream_geo != nullptr) (void)hipStreamDestroy(ctx->stream_geo);
  if (ctx->grid.stream_upload != nullptr) (void)hipStreamDestroy(ctx->grid.stream_upload);
  if (ctx->grid.source_event != nullptr) (void)hipEventDestroy(ctx->grid.source_event);
  // (stream_few / stream_most are the process's, borrowed: EnsureSplitStreams)
  delete ctx;
}

const char *bl_build_info(void) { return "blacklight_amd;hip;gfx950;fp-contract=off"; }

}  // extern "C"

const bl_params *bl_internal_params(const bl_ctx *ctx) { return &ctx->params; }
bl_slow_state *bl_internal_slow_state(bl_ctx *ctx) { return &ctx->slow_state; }
void bl_internal_warn(bl_ctx *ctx, const char *message) { Warn(ctx, message); }
const bl_camera_frame *bl_internal_frame(const bl_ctx *ctx) { return &ctx->frame; }
const double *bl_internal_frequencies(const bl_ctx *ctx, int *count) {
  *count = static_cast<int>(ctx->frequencies.size());
  return ctx->frequencies.data();
}
bl_variant_place bl_internal_variant_place(const bl_ctx *ctx, int variant) {
  const Variants vs = ResolveVariants(ctx);
  const VariantPlace at = vs.At(variant);
  return {at.e, at.m, at.u, at.s, vs.n_mixes > 0, vs.n_cuts > 0, vs.n_pol > 0};
}
int bl_internal_fail(bl_ctx *ctx, int code, const char *message) {
  ctx->last_error = std::string("Error: ") + message + "\n";
  return code;
}
