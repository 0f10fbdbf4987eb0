// bl_coefficients_freq.hip - per-frequency coefficient kernels behind the coefficient kernel proper (gfx950): the polarized
// coefficients of a sample (both tiers), the frame of a polarized sample, the per-frequency factors of many-frequency renders in
// the tolerant tier; and the element-wise diagnostics kernel the math tests use.
#include "bl_sampling_fast.h"

// =================================================================================================
// Polarized coefficient kernel: the per-frequency part of CalculateSimulationCoefficients (simulation_coefficients.cpp:
// 458-698) for polarized runs, one sample record per lane from the scalars the coefficient kernel left
// (BlCoefInputs). Writes (j_I, alpha_I) and the three polarized pairs, [ray][n][frequency]: polarized_sample_prelude() once and
// polarized_sample_coefficients() per frequency (bl_sampling_fast.h; bl_shade_polarized2_kernel<.., kCoefficients> calls the same two).
// =================================================================================================
// kTolerant: the tolerant arithmetic tier's functions and fused multiply-adds in the formulas (bl_coefficients.inc,
// second inclusion) - the kernel is almost entirely the double-double pow / log of the pinned library otherwise.
#ifndef BL_POLCOEF_WAVES
#define BL_POLCOEF_WAVES 2
#endif
// kThermalOnly: no power-law and no kappa-distribution electrons (the host knows): without their formulas the exact kernel fits three
// waves per SIMD instead of two (168 registers), which is worth 8 ms of a 1024^2 frame's 106.
// Polarized variants with an electron mix each (BlShadeArgs::pol_variant_args): the block whose electron constants - thermal fraction,
// power-law constants, BlShadeCold::kappa behind its `cold` - variant v's formulas read. The table is written before the launch and
// read-only during it, and v is uniform over the wave: read through the constant address space, as the kernel's own arguments are, its
// fields are scalar loads where they are used. The thermal-only instantiation reads no electron constant but the thermal fraction,
// which is then the same for every variant: its own arguments.
template <bool kThermalOnly>
__device__ __forceinline__ const BlShadeArgs &variant_electrons(const BlShadeArgs &P, unsigned int v) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (!kThermalOnly) {
    // (one pointer in that address space behind the barrier kernel_arguments_in_place uses: the optimiser sees neither of its two
    // origins, so the reads through it stay scalar loads and the reads through P stay what they were)
    typedef const __attribute__((address_space(4))) BlShadeArgs *InConstant;
    const BlPolVariantArgs *table = P.pol_variant_args;
    InConstant e = table != nullptr ? (InConstant)&table[v].args : (InConstant)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(e));
    return *(const BlShadeArgs *)e;
  }
#endif
  return P;
}

template <bool kTolerant, bool kThermalOnly>
__global__ void __launch_bounds__(256, (kThermalOnly && !kTolerant) ? 3 : BL_POLCOEF_WAVES) bl_polarized_coefficients_kernel(const BlShadeArgs P_at_entry) {
  // (with power-law or kappa electrons the kernel holds ~45 more scalars than there are registers for: it reads its arguments where it uses them)
  const BlShadeArgs &P = kThermalOnly ? P_at_entry : kernel_arguments_in_place<BlShadeArgs>();
  const unsigned long long n_records = P.counters_in[BL_CNT_RECORDS];
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  // Polarized variants in one pass (P.pol_variants > 0, uniform per launch): a wave per (64 records, variant), the variants of a group
  // of records in consecutive waves - a wave's lanes share their variant, so its five constants are scalar operands, and the waves
  // of a group read the same 64 rows (4 KiB, from L2 after the first). Otherwise a lane per record, as ever.
  const unsigned int n_var = P.pol_variants > 0 ? (unsigned int)P.pol_variants : 1u;
  const unsigned long long n_items = n_var > 1u ? ((n_records + 63ull) >> 6) * 64ull * n_var : n_records;
  for (unsigned long long item = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; item < n_items; item += stride) {
    unsigned long long idx = item;
    unsigned int v = 0u;
    if (n_var > 1u) {
      const unsigned long long wave = item >> 6;
      v = (unsigned int)__builtin_amdgcn_readfirstlane((int)(wave % n_var));
      idx = (wave / n_var) * 64ull + (item & 63ull);
      if (idx >= n_records) continue;
    }
    const unsigned long long tag = reinterpret_cast<const unsigned long long *>(P.records_hot + (idx) * P.record_stride)[3];   // (ray, n)
    const uint32_t ray = (uint32_t)tag;
    if (ray == BL_DEAD_RAY) continue;
    const uint32_t n = (uint32_t)(tag >> 32);
    const BlCoefInputs ci = P.coef_inputs[idx];
    const double momentum_factor = bl_ray_factor(P.ray_constants, (size_t)ray);
    // the electron constants of the wave's variant (a mix per variant: its copy of the block; else the render's own, for every variant)
    const BlShadeArgs &E = variant_electrons<kThermalOnly>(P, v);
    SampleShade sh;   // (empty, then what the row holds)
    sh.have_coefficients = ci.have_coefficients != 0.0;
    sh.nu_fluid_over_nu = ci.nu_fluid_over_nu;
    sh.n_e_cgs = ci.n_e_cgs;
    sh.nu_c_cgs = ci.nu_c_cgs;
    sh.theta_e = ci.theta_e;
    sh.kb_tt_e_cgs = ci.kb_tt_e_cgs;
    if (P.pol_variants > 0 && sh.have_coefficients) {
      // the row holds (rho, p_gas) and b_mu b^mu: this variant's scalars by the functions sample_finish_simulation() forms them with
      const BlPolVariant &pv = P.pol_variant_table[v];
      const double rho = (double)__int_as_float(__double2loint(ci.n_e_cgs)), pgas = (double)__int_as_float(__double2hiint(ci.n_e_cgs));
      const double b_sq = ci.nu_c_cgs;
      // the variant's sigma cut (simulation_coefficients.cpp:361-375; wave-uniform threshold, +inf where there is none to compare):
      // sample_finish_simulation()'s quotient of its operands, and a cut cell's zeros at every frequency
      if (pv.sigma_max != __longlong_as_double(0x7ff0000000000000ll) && b_sq / rho > pv.sigma_max) sh.have_coefficients = false;
      const PlasmaCgs cgs = plasma_density_cgs(P.plasma, pv.d_unit, pv.e_unit, rho, pgas);
      sh.n_e_cgs = cgs.n_e_cgs;
      sh.nu_c_cgs = plasma_cyclotron_frequency(plasma_field_cgs(b_sq, pv.b_unit));
      sh.theta_e = sh.kb_tt_e_cgs = __longlong_as_double(0x7ff8000000000000ll);
      if (E.plasma.plasma_thermal_frac != 0.0)
        plasma_electron_temperature(P, pv.rat_high, pv.rat_low, plasma_beta_inverse(b_sq, pgas), cgs, &sh.theta_e, &sh.kb_tt_e_cgs);
    }
    sh.cos2_theta_b = ci.cos2_theta_b;
    sh.cos_sign = ci.cos_sign;
    polarized_sample_prelude<kTolerant>(E, &sh);
    const size_t at = (((size_t)P.ray_offset[ray] + n) * n_var + v) * P.n_nu;
    for (int l = 0; l < P.n_nu; l++) {
      const double freq = P.frequencies[l];
      double2 *out = P.pol_coeffs + (at + l) * 4;
      polarized_sample_coefficients<kTolerant, !kThermalOnly>(E, sh, momentum_factor, freq, out);
#ifdef BL_POL_CONDITION_STATS
      // (a measurement build, tools/build_variant.sh -DBL_POL_CONDITION_STATS: how many samples' joint coupling step - polarized.cpp:
      // 657-778 - loses more than 2, 3, 4, 6 digits to the cancellations in lambda_1, lambda_2 = sqrt(lambda_a +- lambda_b) and in
      // 1 / (alpha_I^2 - lambda_1^2); BL_CNT_DEBUG + 0 ... 3, samples with coefficients in + 4, with rho and alpha_P both non-zero in + 5)
      if (sh.have_coefficients) {
        const double alpha_val = out[0].y;
        const double2 pc[3] = {out[1], out[2], out[3]};
        const double a_sq = pc[1].x * pc[1].x + pc[1].y * pc[1].y, r_sq = pc[2].x * pc[2].x + pc[2].y * pc[2].y;
        const double a_r = pc[1].x * pc[2].x + pc[1].y * pc[2].y;
        const double lb = 0.5 * (a_sq - r_sq), la = sqrt(lb * lb + a_r * a_r);
        const double l1_sq = la + lb, l2_sq = la - lb;
        double kappa = 1.0;
        if (a_sq > 0.0 && r_sq > 0.0) {
          kappa = fmax(kappa, la / fabs(l1_sq));
          kappa = fmax(kappa, la / fabs(l2_sq));
          kappa = fmax(kappa, alpha_val * alpha_val / fabs(alpha_val * alpha_val - l1_sq));
        }
        atomicAdd(&P.counters[BL_CNT_DEBUG + 4], 1ull);
        if (a_sq > 0.0 && r_sq > 0.0) atomicAdd(&P.counters[BL_CNT_DEBUG + 5], 1ull);
        if (!(kappa < 1e2)) atomicAdd(&P.counters[BL_CNT_DEBUG + 0], 1ull);
        if (!(kappa < 1e3)) atomicAdd(&P.counters[BL_CNT_DEBUG + 1], 1ull);
        if (!(kappa < 1e4)) atomicAdd(&P.counters[BL_CNT_DEBUG + 2], 1ull);
        if (!(kappa < 1e6)) atomicAdd(&P.counters[BL_CNT_DEBUG + 3], 1ull);
      }
#endif
    }
  }
}

// Exact tier, plain images with several frequencies: one lane per (sample record, frequency). The coefficient kernel's frequency
// loop (simulation_coefficients.cpp:464-523, :556-584; unpolarized.cpp:74-110) with the loop turned into lanes: the lanes of a
// record read the same 64 bytes of inputs (bl_unpack_plain_coef_inputs), evaluate the pinned formulas at their own frequency - the
// loop's own body, write_transfer_records() at one frequency - and write the record's transfer records side by side (one contiguous
// kilobyte per sample at 64 frequencies instead of 64 scattered 16-byte stores per lane), at four waves per SIMD.
template <bool kExtended>
__global__ void __launch_bounds__(256, 4) bl_coefficients_freq_kernel(const BlShadeArgs P) {
  const unsigned long long n_records = P.counters_in[BL_CNT_RECORDS];
  const unsigned long long total = n_records * (unsigned long long)P.n_nu;
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  for (unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    const unsigned long long idx = t / (unsigned long long)P.n_nu;
    const int l = (int)(t - idx * (unsigned long long)P.n_nu);
    const unsigned long long tag = reinterpret_cast<const unsigned long long *>(P.records_hot + (idx) * P.record_stride)[3];   // (ray, n)
    const uint32_t ray = (uint32_t)tag;
    if (ray == BL_DEAD_RAY) continue;
    const uint32_t n = (uint32_t)(tag >> 32);
    const BlCoefInputs ci = P.coef_inputs[idx];
    const double momentum_factor = bl_ray_factor(P.ray_constants, (size_t)ray);
    SampleShade sh;
    const double delta_lambda = bl_unpack_plain_coef_inputs(ci, &sh);
    write_transfer_records<kExtended>(P, sh, P.frequencies[l], momentum_factor, delta_lambda, P.transfer + ((size_t)P.ray_offset[ray] + n) * P.n_nu + l);
  }
}

// The fluid frame of the samples without coefficients (polarized.cpp:163-265 at cut samples and cut or field-free cells):
// k^mu and tetrad rows 1, 2 into their BlPolSample, from what the coefficient kernel parked in BlCoefInputs.
__global__ void __launch_bounds__(256) bl_polarized_frame_kernel(const BlShadeArgs P) {
  const unsigned long long n_all = P.counters_in[BL_CNT_RECORDS];
  const unsigned long long n_listed = P.redo_list != nullptr ? P.counters_in[BL_CNT_REDO] : ~0ull;
  const bool listed = n_listed <= P.redo_capacity;   // else: more such samples than the list holds - look at every record
  const unsigned long long n_items = listed ? n_listed : n_all;
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  for (unsigned long long pos = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; pos < n_items; pos += stride) {
    const unsigned long long idx = listed ? P.redo_list[pos] : pos;
    const double2 *hot = reinterpret_cast<const double2 *>(P.records_hot + (idx) * P.record_stride);
    const double2 q1 = hot[1];
    const unsigned long long tag = (unsigned long long)__double_as_longlong(q1.y);   // (ray, n)
    const uint32_t ray = (uint32_t)tag;
    if (ray == BL_DEAD_RAY) continue;
    const double2 *in = reinterpret_cast<const double2 *>(P.coef_inputs + idx);
    const double2 c3 = in[3];
    // have_coefficients: the coefficient kernel wrote the frame (where it evaluated the coefficients itself it left no inputs: a flag)
    if (P.have_flags != nullptr ? P.have_flags[idx] != 0 : c3.y != 0.0) continue;
    const uint32_t n = (uint32_t)(tag >> 32);
    const double2 q0 = hot[0], c0 = in[0], c1 = in[1], c2 = in[2];
    const double kcov[4] = {c0.x, c0.y, c1.x, c1.y};
    const float uu[3] = {__int_as_float(__double2loint(c2.x)), __int_as_float(__double2hiint(c2.x)), __int_as_float(__double2loint(c2.y))};
    const float bb[3] = {__int_as_float(__double2hiint(c2.y)), __int_as_float(__double2loint(c3.x)), __int_as_float(__double2hiint(c3.x))};
    bl_pol::sample_frame(P.st, P.plasma.simulation_coord, q0.x, q0.y, q1.x, kcov, uu, bb, P.pol_samples + ((size_t)P.ray_offset[ray] + n));
  }
}



// Diagnostics (bl_debug_math op 40 / 41: spin zero / any spin): the locate step's theta and phi of given points against a given angular
// lattice, both ways - relative to the centre of the guessed cell (bl_local_angles.h: the functions bl_shade_fused2_kernel calls) and by the
// tier's acos / atan2 with the face and centre comparisons of fused2::axis_lookup.
// What this runs of the kernel: direction, angle_guess, make_row, offset_from_centre and lookup of bl_local_angles.h, with the centre's sine
// and cosine from the device's bl_sincos (the pinned library: the host table's bits) and the guess-to-cell step restated. The host-made table,
// the rows' place in LDS and fused2::read_angle_row are exercised by the frame tests only. The "global" half is a restatement too -
// fastmath::acos / atan2, which the kernel's acos_k / atan2_k restate, with axis_lookup's margins and anchor rule - not fused2::locate itself.
//   x = [m, a, n_th, n_ph, xs[m], ys[m], zs[m]],  y = [xf_th[n_th + 1], xv_th[n_th], xf_ph[n_ph + 1], xv_ph[n_ph]],  out = [16][m]:
//   rows 0 - 7 local: anchor cell in theta, in phi, fraction in theta, in phi, smallest margin, undecided (margin <= 1e-12), guessed cell in
//   theta, in phi;  rows 8 - 15 the same from the global angles.
#pragma clang fp contract(fast)
#include "bl_local_angles.h"
template <bool kSpinZero>
__device__ void debug_locate_angles(long long i, long long m, double a, int n_th, int n_ph, const double *x, const double *y, double *out) {
  const double *xf[2] = {y, y + 2 * n_th + 1}, *xv[2] = {y + n_th + 1, y + 2 * n_th + 1 + n_ph + 1};
  const int n[2] = {n_th, n_ph};
  const double px = x[4 + i], py = x[4 + m + i], pz = x[4 + 2 * m + i], band = 1.0e-12;
  BlSpacetime st{};
  st.bh_a = a;
  double r2;
  const double r = bl_radial_coordinate2<kSpinZero>(st, px, py, pz, &r2);
  const double r_inv = 1.0 / r;
  {   // relative to the cell centre
    const local_angles::Direction u = local_angles::direction<kSpinZero>(a, r, r_inv, px, py, pz);
    const float guess[2] = {local_angles::angle_guess<false>((float)u.sin_th, (float)u.cos_th), local_angles::angle_guess<true>((float)u.sin_ph, (float)u.cos_ph)};
    const double sines[2] = {u.sin_th, u.sin_ph}, cosines[2] = {u.cos_th, u.cos_ph};
    double margin = 1.0;
    for (int q = 0; q < 2; q++) {
      const float x0 = (float)xf[q][0], inv_w = (float)((double)n[q] / (xf[q][n[q]] - xf[q][0]));
      int c = (int)((guess[q] - x0) * inv_w);
      c = c < 0 ? 0 : (c > n[q] - 1 ? n[q] - 1 : c);
      double sin_c, cos_c;
      bl_sincos(xv[q][c], &sin_c, &cos_c);
      const local_angles::AngleRow at_c = local_angles::make_row(xf[q], xv[q], cos_c, sin_c, c, n[q], q == 0 ? kPi : 2.0 * kPi);
      double frac, mq;
      uint32_t shift;
      local_angles::lookup(at_c, local_angles::offset_from_centre(sines[q], cosines[q], at_c.cos_c, at_c.sin_c), &frac, &shift, &mq);
      margin = q == 0 ? mq : (margin < mq ? margin : mq);   // (as the kernel takes it: a NaN - phi on the polar axis - stays)
      out[(0 + q) * m + i] = (double)(c - (int)shift);
      out[(2 + q) * m + i] = frac;
      out[(6 + q) * m + i] = (double)c;
    }
    out[4 * m + i] = margin;
    out[5 * m + i] = margin > band ? 0.0 : 1.0;
  }
  {   // global angles
    double cth = pz * r_inv;
    cth = __builtin_fma(__builtin_fma(-r, cth, pz), r_inv, cth);
    const double th = fastmath::acos(cth);
    const double ph_unwrapped = kSpinZero ? fastmath::atan2(py, px) : fastmath::atan2(py, px) - fastmath::atan2(a, r);
    const double two_pi = 2.0 * kPi;
    double ph = ph_unwrapped + (ph_unwrapped < 0.0 ? two_pi : 0.0);
    const double ph_once = ph;
    ph -= ph >= two_pi ? two_pi : 0.0;
    const double angle[2] = {th, ph};
    double margin = __builtin_fabs(ph_unwrapped);
    const double e1 = __builtin_fabs(ph_once - two_pi);
    margin = margin < e1 ? margin : e1;
    for (int q = 0; q < 2; q++) {
      int c = (int)((angle[q] - xf[q][0]) * ((double)n[q] / (xf[q][n[q]] - xf[q][0])));
      c = c < 0 ? 0 : (c > n[q] - 1 ? n[q] - 1 : c);
      const bool ge = angle[q] >= xv[q][c];
      const int anchor = ge ? (c == n[q] - 1 ? c - 1 : c) : (c == 0 ? 0 : c - 1);
      const double frac = (angle[q] - xv[q][anchor]) * (1.0 / (xv[q][anchor + 1] - xv[q][anchor]));
      const double d_lo = angle[q] - xf[q][c], d_hi = xf[q][c + 1] - angle[q], d_c = __builtin_fabs(angle[q] - xv[q][c]);
      double mq = d_lo < d_hi ? d_lo : d_hi;
      mq = mq < d_c ? mq : d_c;
      margin = mq < margin ? mq : margin;
      margin = mq == mq ? margin : -1.0;
      out[(8 + q) * m + i] = (double)anchor;
      out[(10 + q) * m + i] = frac;
      out[(14 + q) * m + i] = (double)c;
    }
    out[12 * m + i] = margin;
    out[13 * m + i] = margin > band ? 0.0 : 1.0;
  }
}
#pragma clang fp contract(off)

// Diagnostics: apply one device math function element-wise (bl_debug_math). Lets the tests compare the
// device build of blmath.h and the exact-arithmetic devices of bl_geometry.h with the host, bit for bit.
__global__ void bl_debug_math_kernel(int op, long long n, const double *x, const double *y, double *out) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (op == 40 || op == 41) {   // (the layout above: the caller - bl_debug_math - has checked that x, y and out hold it)
    const long long m = (long long)x[0];
    if (i >= m) return;
    if (op == 40) debug_locate_angles<true>(i, m, 0.0, (int)x[2], (int)x[3], x, y, out);
    else debug_locate_angles<false>(i, m, x[1], (int)x[2], (int)x[3], x, y, out);
    return;
  }
  const double a = x[i], b = y != nullptr ? y[i] : 0.0;
  double r = 0.0, s_unused, c_unused;
  switch (op) {
    case 0: r = bl_exp(a); break;
    case 1: r = bl_expm1(a); break;
    case 2: r = bl_log(a); break;
    case 3: r = bl_cbrt(a); break;
    case 4: r = bl_sin(a); break;
    case 5: r = bl_cos(a); break;
    case 6: r = bl_acos(a); break;
    case 7: r = bl_atan(a); break;
    case 8: r = bl_atan2(a, b); break;
    case 9: r = bl_pow(a, b); break;
    case 10: r = bl_hypot(a, b); break;
    case 11: r = bl_hypot_g(a, b); break;
    case 12: r = bl_sqrt_g(a); break;
    case 13: r = bl_div_g(a, b); break;
    case 14: r = blm_sqrt(a); break;
    case 15: r = a / b; break;
    case 16: bl_sincos(a, &r, &c_unused); break;
    case 17: bl_sincos(a, &s_unused, &r); break;
    // tolerant tier's functions (not bit-reproducible by contract; accuracy is what the tests check)
    case 25: case 26: case 27: {
      double k0, k1, k2;
      fastmath::bessel_k012(a, &k0, &k1, &k2);
      r = op == 25 ? k0 : (op == 26 ? k1 : k2);
      break;
    }
    case 20: r = fastmath::exp(a); break;
    case 21: r = fastmath::expm1(a); break;
    case 22: r = fastmath::cbrt(a); break;
    case 23: r = fastmath::rcp(a); break;
    case 24: r = fastmath::rsqrt(a); break;
    case 28: r = fastmath::acos(a); break;
    case 29: r = fastmath::atan2(a, b); break;
    case 30: case 31: case 32: {   // the tolerant tier's Bessel functions K_0, K_1, K_2
      double k[3];
      fastmath::bessel_k012(a, &k[0], &k[1], &k[2]);
      r = k[op - 30];
      break;
    }
    case 33: case 34: case 35: {   // the exact tier's
      double k[3];
      bl_cyl_bessel_k012(a, &k[0], &k[1], &k[2]);
      r = k[op - 33];
      break;
    }
    case 36: r = fastmath::log(a); break;
    case 38: r = bl_pow_neg_fifth(a); break;
    case 37: r = fastmath::pow(a, b); break;
    default: break;
  }
  out[i] = r;
}


// The per-frequency coefficients of a polarized run's samples (simulation_coefficients<kExtended> also holds the unpolarized kappa
// terms: never in a polarized run), and the frames of its samples without coefficients
// (the exact tier's formulas in either tier: the polarized step amplifies last-place differences of the coefficients by orders of
// magnitude in optically and Faraday thick cells - docs/notebook.md - so a tolerant kernel here moved rows with the reference's own
// conditioning; it was a measurement switch until round 6)
extern "C" hipError_t bl_launch_polarized_coefficients(const BlShadeArgs *args, const KernelPlan::PerFrequency &plan, int grid, hipStream_t stream) {
  // (the thermal-only kernel needs thermal electrons in the block it reads - and no table of mixes, which it does not read; the
  // all-electrons kernel renders thermal ones to the same bits: a pass of a variant without a power law or kappa electrons among others with)
  const bool thermal_only = args->plasma.power_frac == 0.0 && args->plasma.kappa_unpolarized == 0 && args->plasma.kappa_frac_zero != 0;
  if (!plan.polarized_coefficients || (plan.thermal_only && (!thermal_only || args->pol_variant_args != nullptr)) || args->pol_samples == nullptr)
    return hipErrorInvalidValue;
  if (args->pol_variant_args != nullptr && args->pol_variants < 2) return hipErrorInvalidValue;
  void (*kernel)(BlShadeArgs) = plan.thermal_only ? bl_polarized_coefficients_kernel<false, true> : bl_polarized_coefficients_kernel<false, false>;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, stream, *args);
  return hipGetLastError();
}
extern "C" hipError_t bl_launch_polarized_frames(const BlShadeArgs *args, int grid, hipStream_t stream) {
  if (args->pol_samples == nullptr) return hipErrorInvalidValue;
  hipLaunchKernelGGL(bl_polarized_frame_kernel, dim3(grid), dim3(256), 0, stream, *args);
  return hipGetLastError();
}

extern "C" hipError_t bl_launch_debug_math(int op, long long n, const double *x, const double *y, double *out, hipStream_t stream) {
  int grid = (int)((n + 255) / 256);
  hipLaunchKernelGGL(bl_debug_math_kernel, dim3(grid), dim3(256), 0, stream, op, n, x, y, out);
  return hipGetLastError();
}

// (one instantiation: the extended formulas evaluate to the plain ones' bits where no power law or entropy is asked for)
extern "C" hipError_t bl_launch_coefficients_freq(const BlShadeArgs *args, int grid, hipStream_t stream) {
  if (args->coef_inputs == nullptr || !args->coef_split) return hipErrorInvalidValue;
  hipLaunchKernelGGL(bl_coefficients_freq_kernel<true>, dim3(grid), dim3(256), 0, stream, *args);
  return hipGetLastError();
}
