// bl_transfer.hip - the transfer stage of the hot path (gfx950).
//
//   bl_transfer_kernel       one lane per (ray, frequency): replays the per-sample records far -> near in the reference's
//                            order and scales by nu^3.   (unpolarized.cpp:71-110, :200-208)
//   bl_transfer_quad_kernel  tolerant tier, one frequency: four lanes per ray, affine maps composed by a DPP scan
//   bl_transfer_freq_kernel  tolerant tier, several frequencies - or electron models and density units in one pass: records
//                            built from per-sample factors on the fly
//   bl_transfer_aux_kernel   image_light and the nine auxiliary images.   (unpolarized.cpp:113-196)
//   bl_tau_kernel            optical depth beside the intensities in the tolerant tier
#include <type_traits>

#include "bl_kernel_util.h"

#pragma clang fp contract(fast)
#include "bl_fastmath.h"

// Several frequencies in the tolerant tier: one lane per (ray, frequency) walks the ray far -> near, builds each sample's
// (a, c) from the sample's factors (BlFreqInputs; the lanes of one ray read the same 64 bytes) and the lane's own frequency,
// and applies I <- a I + c at once. The per-frequency transfer records (16 bytes per sample and frequency: 1.5 TB written
// and read per 1024^2 x 64-frequency frame) do not exist on this path; the exact second pass leaves the same factors.
// With electron models in one pass (P.n_models > 0, wave-uniform) a lane is a (ray, model, frequency): the rows hold what no model
// enters (BlFreqInputs), and the lane forms its model's 1 / (k T_e) per sample before the same step. With density units as well
// (P.n_units > 0) a lane is a (ray, model, unit, frequency), and its unit scales the row's x at unit frequency and s_j (unit_x,
// unit_j), folded into the lane's frequency terms once: no work per sample. (Without units the factors are 1.0: the same bits.)
// With sigma cuts as well (P.n_cuts > 0) a lane is a (ray, model, unit, cut, frequency): the rows carry the sample's sigma, and the
// lane leaves out the samples above its own threshold - one compare per sample. (Without cuts the threshold is +inf, against which no
// sigma compares greater - NaN included, as in the reference: the same decisions.)
// With electron mixes as well (P.n_mixes > 0) a lane is a ray and a workgroup a (256 rays, mix, model, unit, cut, frequency): everything
// the walk needs of its channel is the workgroup's, computed once into LDS and read where it is used, which costs the walk no vector
// register across its loop - as lane constants they take 18, and the power-law terms on top of them 76 where 64 keep eight waves per
// SIMD. (Consecutive workgroups are the channels of the same rays: the rows they all read come from L2.) The rows were
// written with the thermal fraction folded as 1; the lane scales the thermal line by its mix's thermal fraction and adds its mix's
// power-law emissivity and absorptivity (bl_shade_fast_kernel's terms, simulation_coefficients.cpp:556-584), which follow from the same
// row: with k4, k5, k6, k7 of BlShadeArgs::fast_k at the base unit and a thermal fraction of 1, ratio = nu / (nu_c sin theta_B) =
// q0.y f / (k4 k7), rho |b| sin theta_B / s_nu^2 = q1.y / k5 and rho = q1.y (q1.x / h) q0.y / (k4 k5), so that
//   j     = power_frac power_jj (e^2 k6 k7 / (c k5)) q1.y f^-2 ratio^(-(p - 1) / 2)
//   alpha = power_frac power_aa (e^2 k6 / (m_e c h k4 k5)) q1.y q1.x q0.y ratio^(-(p + 2) / 2)
//         = power_frac power_aa (e^2 k6 k7 / (m_e c h k5)) q1.y q1.x f^-1 ratio^(-(p - 1) / 2) ratio^(-1/2)
// (q0.y = ratio k4 k7 / f): one logarithm, one exponential and one reciprocal square root per sample and lane. Unit u: n_e ~ unit and
// |b| ~ sqrt(unit) - ratio takes unit_x with f as x does, j's f^-2 is the lane's f_inv2 (unit_j in it), and alpha's f^-1 becomes
// f_inv2 f, which carries unit_j / unit_x x unit_x = n_e's factor.
// (what a workgroup with mixes keeps in LDS: f, its roots and reciprocals with the unit's factors, the cut's threshold, the model's
// constants, and of the mix the thermal fraction, -(p - 1) / 2, the folded factors of j and alpha, and 1 / (k4 k7))
enum { kGroupF, kGroupF12, kGroupF13, kGroupF16, kGroupFInv, kGroupFInv2, kGroupSigma, kGroupMk1, kGroupMk2, kGroupMk3, kGroupThermal, kGroupPwE, kGroupPwJ,
       kGroupPwA, kGroupK0, kGroupConstants };
// (the kernel's body twice, chosen by the wave-uniform P.n_mixes > 0 at its very top: without mixes it is, statement for statement, the
// kernel as it was before the axis existed - kGroup folds everything else away)
template <bool kGroup>
__device__ __forceinline__ void bl_transfer_freq_body(const BlTransferArgs &P, double *group_k) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool models = P.n_models > 0;
  const int n_units = P.n_units > 0 ? P.n_units : 1;
  const int n_cuts = P.n_cuts > 0 ? P.n_cuts : 1;
  const int channels = models ? P.n_models * n_units * n_cuts * P.n_nu : P.n_nu;
  int slot = (int)(t / channels);
  int channel = (int)(t % channels);   // ((m n_units + u) n_cuts + s) n_nu + l: the image row (with mixes: within the mix's rows)
  int mix = 0;
  if (kGroup) {   // a workgroup per (256 rays, mix, channel): both scalars, a lane per ray
    const unsigned int all = (unsigned int)(P.n_mixes * channels), group = blockIdx.x / all, c = blockIdx.x - group * all;
    mix = (int)(c / (unsigned int)channels);
    channel = (int)(c - (unsigned int)(mix * channels));
    slot = (int)(group * blockDim.x + threadIdx.x);
  }
  const int l = channel % P.n_nu;
  // With mixes the lane's constants are the workgroup's. They wait in LDS and are read where they are used, so that the power-law terms
  // fit the vector registers of eight waves per SIMD (as lane constants they take 18 registers across the loop).
  if (kGroup) {
    if (threadIdx.x == 0) {
      const int variant = channel / P.n_nu, pair = variant / n_cuts, m = pair / n_units, u = pair - m * n_units;
      const double ux = P.n_units > 0 ? P.unit_x[u] : 1.0, uj = P.n_units > 0 ? P.unit_j[u] : 1.0;
      const double f = P.frequencies[l], f_x = f * ux, f_1_3 = fastmath::cbrt(f_x), f_inv = fastmath::rcp(f);
      group_k[kGroupF] = f, group_k[kGroupF12] = bl_sqrt_g(f_x), group_k[kGroupF13] = f_1_3, group_k[kGroupF16] = bl_sqrt_g(f_1_3);
      group_k[kGroupFInv] = f_inv, group_k[kGroupFInv2] = f_inv * f_inv * uj;
      group_k[kGroupSigma] = P.n_cuts > 0 ? P.sigma_max[variant - pair * n_cuts] : __builtin_inf();
      group_k[kGroupMk1] = P.model_k1[m], group_k[kGroupMk2] = P.model_k2[m], group_k[kGroupMk3] = P.model_k3;
      // (the mix's, as the host folded them - BuildTransferArgs; zeros where it has no power law)
      group_k[kGroupThermal] = P.mix_thermal[mix], group_k[kGroupPwE] = P.mix_pw_e[mix], group_k[kGroupPwJ] = P.mix_pw_j[mix];
      group_k[kGroupPwA] = P.mix_pw_a[mix], group_k[kGroupK0] = P.power_k0;
    }
    __syncthreads();
  }
  unsigned long long samples = 0ull, flagged = 0ull;
  int max_num = 0;
  if (slot < bl_rays_done(P.counters, P.chunk_rays)) {
    const int num = P.ray_sample_num[slot];
    const bool flag = P.ray_flags[slot] != 0;
    const long long out_index = P.ray_out_index[slot];
    if (channel == 0 && (!kGroup || mix == 0)) {
      const int all = num + (P.ray_skipped != nullptr ? P.ray_skipped[slot] : 0);
      samples = (unsigned long long)all;
      flagged = flag ? 1ull : 0ull;
      max_num = all;
      if (P.out_sample_num != nullptr) P.out_sample_num[out_index] = all;
      if (P.out_flags != nullptr) P.out_flags[out_index] = flag ? 1 : 0;
    }
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const double f_given = P.frequencies[l];
    double intensity = 0.0;
    if (P.fallback_nan && flag) {
      intensity = num > 0 ? nan : 0.0;   // every sample of a flagged ray carries NaN primitives (simulation_sampling.cpp:211-216)
    } else {
      // (the ray's walk twice, behind a wave-uniform branch: the one without sigma cuts is the code it was - a render that does not use
      // the axis does not pay for it - the other holds the lane's threshold and one compare more per sample; a third, with electron mixes,
      // the mix's power-law terms per sample - it always compares, against +inf where no cuts are set)
      auto walk = [&](auto with_cuts, auto with_mixes) {
        constexpr bool kCuts = decltype(with_cuts)::value, kMixes = decltype(with_mixes)::value;
        const int variant = channel / P.n_nu, pair = kCuts ? variant / (kMixes ? n_cuts : P.n_cuts) : variant, m = pair / n_units, u = pair - m * n_units;
        const double f = f_given;
        const double sigma_max = (!kCuts || kMixes) ? 0.0 : P.sigma_max[variant - pair * P.n_cuts];
        // (with mixes: the workgroup's copy, read afresh at every use - K(i, lane's) is the lane's value in the two older forms)
        const volatile double *group = kMixes ? group_k : nullptr;
        auto K = [group](int i, double lanes) {
          if constexpr (kMixes) return (double)group[i];
          else return lanes;
        };
        // Unit u's factors where no sample register holds them: x at unit frequency enters only as x f, so unit_x is a factor on the
        // frequency of the x terms (f_1_2, f_1_3, f_1_6), and s_j only as s_j f^-2, so unit_j is one on f_inv2 (without units: 1.0)
        const double ux = P.n_units > 0 ? P.unit_x[u] : 1.0, uj = P.n_units > 0 ? P.unit_j[u] : 1.0;
        const double f_x = f * ux;
        const double f_1_2 = kMixes ? 0.0 : bl_sqrt_g(f_x), f_1_3 = kMixes ? 0.0 : fastmath::cbrt(f_x);
        const double f_1_6 = kMixes ? 0.0 : bl_sqrt_g(f_1_3), f_inv = kMixes ? 0.0 : fastmath::rcp(f);
        const double f_inv2 = kMixes ? 0.0 : f_inv * f_inv * uj;
        // A mix without a power law (power_frac == 0: its p, power_jj and power_aa are not defined, the host leaves zeros in the tables)
        // selects zeros below and never multiplies by them, so no 0 x inf forms; its thermal line is the row's times the thermal fraction.
        const bool power = kMixes && P.mix_power_frac[mix] != 0.0;
        // (one exponential per sample and frequency is most of this loop: its constants stay in scalar registers across it)
        double exp_c[15];
  #pragma unroll
        for (int i = 0; i < 15; i++) exp_c[i] = fastmath::resident_constant(fastmath::kExpConstants[i]);
        const double2 *in = reinterpret_cast<const double2 *>(P.freq_inputs + (size_t)P.ray_offset[slot]);
        const double kThird = fastmath::resident_constant(1.0 / 3.0), kInvPlanck = fastmath::resident_constant(kC * kC / (2.0 * kH));
        const double kRoot = fastmath::resident_constant(kPow2_11_12), kThin = fastmath::resident_constant(0x1p-10);
        const double mk1 = (models && !kMixes) ? P.model_k1[m] : 0.0, mk2 = (models && !kMixes) ? P.model_k2[m] : 0.0, mk3 = kMixes ? 0.0 : P.model_k3;
        for (int n = num - 1; n >= 0; n--) {   // reference sample order is reversed integration order (geodesics.cpp:832-840)
          const double2 q0 = in[4 * (size_t)n], q1 = in[4 * (size_t)n + 1], q2 = in[4 * (size_t)n + 2], q3 = in[4 * (size_t)n + 3];
          // bl_shade_fast_kernel's frequency loop (simulation_coefficients.cpp:464-523, unpolarized.cpp:74-110) as one straight line for
          // the sample that has coefficients, a thin step and h nu << k T_e - nearly every one: no expm1, no division, no branch; the
          // rest is selected or, where it needs an exponential of its own, redone behind a branch
          bool have = q0.x == 1.0;
          double s_1_3 = q1.x, s_1_6 = q1.y, s_1_2 = q0.y, s_planck = q2.x, s_j = q2.y, s_length = q3.x;
          if (models) {   // this model's 1 / (k T_e) (the fused kernel's kte_inv), then the sample's roots at unit frequency
            const double bi2 = q2.y, dd = 1.0 + bi2;
            const double kte_inv = (K(kGroupMk1, mk1) + K(kGroupMk2, mk2) * bi2 + K(kGroupMk3, mk3) * dd) * fastmath::rcp(q3.x * dd);
            s_1_3 = fastmath::cbrt(q0.y * (kte_inv * kte_inv));
            s_1_6 = bl_sqrt_g(s_1_3);
            s_1_2 = s_1_6 * s_1_3;
            s_planck = q1.x * kte_inv;
            s_j = q1.y;
            s_length = q2.x;
            if (kCuts) have = have && !(q3.y > K(kGroupSigma, sigma_max));   // (the row's sigma)
          }
          const double xx_1_3 = s_1_3 * K(kGroupF13, f_1_3);
          const double var_c = s_1_2 * K(kGroupF12, f_1_2) + kRoot * (s_1_6 * K(kGroupF16, f_1_6));
          double j_val = s_j * K(kGroupFInv2, f_inv2) * fastmath::exp(-xx_1_3, exp_c) * var_c * var_c;
          if (kMixes) j_val *= group[kGroupThermal];
          const double xp = s_planck * K(kGroupF, f);
          double planck = xp * (1.0 + 0.5 * xp * (1.0 + kThird * xp * (1.0 + 0.25 * xp)));
          if (__builtin_expect(have && !(xp < kThin), 0)) planck = fastmath::expm1(xp);
          double alpha_val = j_val * (planck * kInvPlanck);
          if (alpha_val * alpha_val <= 0x1p-1024) alpha_val = 0.0;
          double j_total = j_val;
          if (kMixes) {
            // the mix's power-law terms. Selected, not multiplied, where the mix has no power law and where the sample lies along the
            // field (q0.y = inf: sin theta_B = 0, both terms are zero there as in bl_shade_fast_kernel, and rho would form inf x 0). A row
            // without coefficients (q0.x != 1: nothing to add, or the NaN row) may hold anything here: `have` selects a and c below.
            __builtin_amdgcn_sched_barrier(0);   // (the thermal line first, then this: interleaved, the two exponentials' temporaries cost a wave of occupancy)
            const double root = K(kGroupF12, f_1_2), ratio = q0.y * (root * root) * group[kGroupK0];
            const double to_e = fastmath::exp(group[kGroupPwE] * fastmath::log(ratio), exp_c) * q1.y;
            const bool add = power && q0.y < __builtin_inf();
            j_total += add ? group[kGroupPwJ] * K(kGroupFInv2, f_inv2) * to_e : 0.0;
            alpha_val += add ? group[kGroupPwA] * (K(kGroupFInv2, f_inv2) * K(kGroupF, f)) * (q1.x * to_e) * fastmath::rsqrt(ratio) : 0.0;
          }
          const double delta_lambda_cgs = s_length * K(kGroupFInv, f_inv);
          const double delta_tau = alpha_val * delta_lambda_cgs;
          // optically thin step: expm1(-t) = -t p(t), p = 1 - t/2 (1 - t/3 (1 - t/4)) to 2^-53: a = 1 - t p, c = j dl p
          const double p = 1.0 - 0.5 * delta_tau * (1.0 - kThird * delta_tau * (1.0 - 0.25 * delta_tau));
          const bool absorbing = alpha_val > 0.0;
          double a = absorbing ? 1.0 - delta_tau * p : 1.0, c = j_total * delta_lambda_cgs * (absorbing ? p : 1.0);
          if (__builtin_expect(have && absorbing && !(delta_tau < kThin), 0)) {
            const double ss = j_total * fastmath::rcp(alpha_val);
            if (delta_tau <= kDeltaTauMax) {
              const double e1 = fastmath::expm1(-delta_tau);
              a = 1.0 + e1;
              c = -ss * e1;
            } else {
              a = 0.0;
              c = ss;
              intensity = 0.0;   // the thick step's intensity replaces what lies behind it, a NaN included (unpolarized.cpp:103-104)
            }
          }
          a = have ? a : 1.0;
          c = have ? c : (q0.x == 2.0 ? nan : 0.0);   // (2: NaN primitives off the grid, simulation_sampling.cpp:377-384; 0: nothing to add)
          intensity = __builtin_fma(a, intensity, c);
        }
      };
      if (kGroup) walk(std::true_type{}, std::true_type{});
      else if (P.n_cuts > 0) walk(std::true_type{}, std::false_type{});
      else walk(std::false_type{}, std::false_type{});
    }
    P.image[(kGroup ? (size_t)mix * channels + (size_t)channel : (size_t)channel) * P.n_rays_total + out_index] = intensity * (f_given * f_given * f_given);   // unpolarized.cpp:206-207
  }
  // statistics: wave reduce, one atomic per wave
  for (int offset = 32; offset > 0; offset >>= 1) {
    samples += __shfl_xor(samples, offset, 64);
    flagged += __shfl_xor(flagged, offset, 64);
    int other = __shfl_xor(max_num, offset, 64);
    max_num = other > max_num ? other : max_num;
  }
  if ((threadIdx.x & 63) == 0) {
    if (samples) atomicAdd(&P.stats[0], samples);
    if (flagged) atomicAdd(&P.stats[1], flagged);
    atomicMax(&P.stats[2], (unsigned long long)max_num);
  }
}
__global__ void __launch_bounds__(256) bl_transfer_freq_kernel(BlTransferArgs P) {
  __shared__ double group_k[kGroupConstants];
  if (P.n_mixes > 0) bl_transfer_freq_body<true>(P, group_k);
  else bl_transfer_freq_body<false>(P, group_k);
}
#pragma clang fp contract(off)

// =================================================================================================
// Transfer kernel
// =================================================================================================
// kAffine: tolerant tier, records are (a, c) of I <- a I + c
template <bool kAffine>
__global__ void __launch_bounds__(256) bl_transfer_kernel(BlTransferArgs P) {
  // One lane per (ray, frequency): consecutive lanes are the frequencies of one ray, whose records of a
  // sample are contiguous, so multi-frequency loads coalesce and the parallelism grows with n_nu.
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  int slot = (int)(t / P.n_nu);
  const int l = (int)(t % P.n_nu);
  const bool mirror = bl_mirror_slot(P, &slot);
  unsigned long long samples = 0ull, flagged = 0ull;
  int max_num = 0;
  if (slot < bl_rays_done(P.counters, P.chunk_rays)) {
    int num = P.ray_sample_num[slot];
    bool flag = P.ray_flags[slot] != 0;
    long long out_index = mirror ? P.mirror_out_index[slot] : P.ray_out_index[slot];
    if (l == 0) {
      const int all = num + (P.ray_skipped != nullptr ? P.ray_skipped[slot] : 0);   // the ray's samples, with or without a record
      samples = (unsigned long long)all;
      flagged = flag ? 1ull : 0ull;
      max_num = all;
      if (P.out_sample_num != nullptr) P.out_sample_num[out_index] = all;
      if (P.out_flags != nullptr) P.out_flags[out_index] = flag ? 1 : 0;
    }
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    {
      double intensity = 0.0;
      if (P.fallback_nan && flag) {
        // simulation: every sample of a flagged ray carries NaN primitives
        // (simulation_sampling.cpp:211-216); formula: only frequency index 0 is NaN-filled
        // (formula_coefficients.cpp:51-59 indexes a 3-D array with two indices)
        bool nan_row = P.model_type == BL_MODEL_SIMULATION || l == 0;
        intensity = (num > 0 && nan_row) ? nan : 0.0;
      } else {
        const double2 *rec = P.transfer + (size_t)(P.ray_offset[slot] + (mirror ? P.row_add : 0ll)) * P.n_nu + l;
        // reference sample order is reversed integration order (geodesics.cpp:832-840). The
        // recurrence is sequential but the loads are not: fetch 8 records (one 128-byte line of
        // this ray's row when n_nu = 1) at a time so 8 loads are in flight per lane.
        int n = num - 1;
        for (; n >= 7; n -= 8) {
          double2 ab[8];
#pragma unroll
          for (int u = 0; u < 8; u++) ab[u] = rec[(size_t)(n - u) * P.n_nu];
#pragma unroll
          for (int u = 0; u < 8; u++) {
            if (kAffine) intensity = BL_IS_AFFINE_THICK(ab[u].x) ? ab[u].y : __builtin_fma(ab[u].x, intensity, ab[u].y);   // (the thick step, see below)
            else intensity = (ab[u].x == BL_THICK_MARK) ? ab[u].y : ab[u].x * (intensity + ab[u].y);
          }
        }
        for (; n >= 0; n--) {
          double2 ab = rec[(size_t)n * P.n_nu];
          // (a = -0.0 marks an optically thick step, whose intensity replaces what lies behind it - a NaN included,
          // unpolarized.cpp:103-104; behind a thin step a NaN stays one, BL_AFFINE_THICK in bl_device.h)
          if (kAffine) intensity = BL_IS_AFFINE_THICK(ab.x) ? ab.y : __builtin_fma(ab.x, intensity, ab.y);
          else intensity = (ab.x == BL_THICK_MARK) ? ab.y : ab.x * (intensity + ab.y);
        }
      }
      double freq = P.frequencies[l];
      double nu_cu = freq * freq * freq;   // unpolarized.cpp:206-207
      P.image[(size_t)l * P.n_rays_total + out_index] = intensity * nu_cu;
    }
  }
  // statistics: wave reduce, one atomic per wave
  for (int offset = 32; offset > 0; offset >>= 1) {
    samples += __shfl_xor(samples, offset, 64);
    flagged += __shfl_xor(flagged, offset, 64);
    int other = __shfl_xor(max_num, offset, 64);
    max_num = other > max_num ? other : max_num;
  }
  if ((threadIdx.x & 63) == 0) {
    if (samples) atomicAdd(&P.stats[0], samples);
    if (flagged) atomicAdd(&P.stats[1], flagged);
    atomicMax(&P.stats[2], (unsigned long long)max_num);
  }
}

// Auxiliary-image transfer kernel (unpolarized.cpp:53-196 for one pixel per lane): integrates image_light
// and every requested auxiliary image from the (j, alpha) pairs and the BlAuxSample records, far -> near,
// in the reference's order. Not on the benchmark path.
__global__ void __launch_bounds__(64) bl_transfer_aux_kernel(BlTransferArgs P) {
  int slot = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long samples = 0ull, flagged = 0ull;
  int max_num = 0;
  if (slot < bl_rays_done(P.counters, P.chunk_rays)) {
    const BlAuxImages &A = P.aux_images;
    const int num = P.ray_sample_num[slot];
    const bool flag = P.ray_flags[slot] != 0;
    const long long out_index = P.ray_out_index[slot];
    samples = (unsigned long long)num;
    flagged = flag ? 1ull : 0ull;
    max_num = num;
    if (P.out_sample_num != nullptr) P.out_sample_num[out_index] = num;
    if (P.out_flags != nullptr) P.out_flags[out_index] = flag ? 1 : 0;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const double momentum_factor = bl_ray_factor(P.ray_constants, (size_t)slot);
    const size_t row = (size_t)P.n_rays_total;
    double *img = P.image + out_index;   // img[q * row] = image(q, pixel)
    for (int q = 0; q < A.n_q; q++) img[(size_t)q * row] = 0.0;
    const BlAuxSample *aux = P.aux + (size_t)P.ray_offset[slot];
    const double2 *ja = P.transfer + (size_t)P.ray_offset[slot] * P.n_nu * P.ja_stride;
    const bool use_j = A.image_light || A.image_emission || A.image_emission_ave;
    const bool use_alpha = A.image_light || A.image_tau || A.image_tau_int;
    if (P.render_params != nullptr) {
      // RadiationIntegrator::Render (rendering.cpp:25-179): false-colour composition along the ray from the
      // recorded cell values, far -> near
      const BlRenderDevice &R = *P.render_params;
      double rgb[BL_MAX_RENDER_IMAGES][3];
      for (int n_i = 0; n_i < BL_MAX_RENDER_IMAGES; n_i++) rgb[n_i][0] = rgb[n_i][1] = rgb[n_i][2] = 0.0;
      double previous_values[BL_NUM_CELL_VALUES];
      for (int a = 0; a < BL_NUM_CELL_VALUES; a++) previous_values[a] = nan;
      for (int n = num - 1; n >= 0; n--) {
        const BlAuxSample s = aux[n];
        const double delta_length = s.length_term;   // 0 unless a fill feature is present
        for (int n_i = 0; n_i < R.n_images; n_i++) {
          for (int n_f = 0; n_f < R.n_features[n_i]; n_f++) {
            const int n_v = R.quantity[n_i][n_f];
            const int type = R.type[n_i][n_f];
            double previous_value = 0.0, current_value = 0.0;
            for (int a = 0; a < BL_NUM_CELL_VALUES; a++)   // register arrays: select instead of indexing
              if (a == n_v) {
                previous_value = previous_values[a];
                current_value = s.cell[a];
              }
            const double cx = R.xyz[n_i][n_f][0], cy = R.xyz[n_i][n_f][1], cz = R.xyz[n_i][n_f][2];
            if (type == BL_RENDER_FILL && current_value >= R.min_val[n_i][n_f] && current_value <= R.max_val[n_i][n_f]) {
              const double delta_tau = delta_length / R.tau_scale[n_i][n_f];
              if (delta_tau <= kDeltaTauMax) {
                const double exp_neg = bl_exp(-delta_tau);
                const double expm1 = bl_expm1(delta_tau);
                rgb[n_i][0] = exp_neg * (rgb[n_i][0] + cx * expm1);
                rgb[n_i][1] = exp_neg * (rgb[n_i][1] + cy * expm1);
                rgb[n_i][2] = exp_neg * (rgb[n_i][2] + cz * expm1);
              } else {
                rgb[n_i][0] = cx;
                rgb[n_i][1] = cy;
                rgb[n_i][2] = cz;
              }
            }
            bool threshold_crossed = false;
            const bool rise_search = type == BL_RENDER_THRESH || type == BL_RENDER_RISE;
            if (rise_search && previous_value < R.thresh[n_i][n_f] && current_value >= R.thresh[n_i][n_f]) threshold_crossed = true;
            const bool fall_search = type == BL_RENDER_THRESH || type == BL_RENDER_FALL;
            if (fall_search && previous_value > R.thresh[n_i][n_f] && current_value <= R.thresh[n_i][n_f]) threshold_crossed = true;
            if (threshold_crossed) {
              const double opacity = R.opacity[n_i][n_f];
              rgb[n_i][0] = (1.0 - opacity) * rgb[n_i][0] + opacity * cx;
              rgb[n_i][1] = (1.0 - opacity) * rgb[n_i][1] + opacity * cy;
              rgb[n_i][2] = (1.0 - opacity) * rgb[n_i][2] + opacity * cz;
            }
          }
        }
        for (int a = 0; a < BL_NUM_CELL_VALUES; a++) previous_values[a] = s.cell[a];
      }
      for (int n_i = 0; n_i < R.n_images; n_i++)
        for (int c = 0; c < 3; c++) P.render[(size_t)(n_i * 3 + c) * row + out_index] = rgb[n_i][c];
    }
    for (int l = 0; l < ((A.n_q > 0 && !A.polarized_rows_only) ? P.n_nu : 0); l++) {
      const double freq = P.frequencies[l];
      double intensity = 0.0, integrated_lambda = 0.0, integrated_emission = 0.0, tau = 0.0;
      double time_min = 0.0, length = 0.0;
      double lambda_ave[BL_NUM_CELL_VALUES], emission_ave[BL_NUM_CELL_VALUES], tau_int[BL_NUM_CELL_VALUES];
      for (int a = 0; a < BL_NUM_CELL_VALUES; a++) lambda_ave[a] = emission_ave[a] = tau_int[a] = 0.0;
      bool plane_sign = num > 0 ? aux[num - 1].plane > 0.0 : false;   // first (farthest) sample, :63-67
      int crossings = 0;
      // reference sample order is reversed integration order (geodesics.cpp:832-840)
      for (int n = num - 1; n >= 0; n--) {
        const BlAuxSample s = aux[n];
        const double2 c = ja[((size_t)n * P.n_nu + l) * P.ja_stride];
        const double delta_lambda = s.delta_lambda;
        const double delta_lambda_cgs = delta_lambda * P.x_unit / (freq * momentum_factor);
        const double t_cgs = s.t * P.t_unit;
        const double j = use_j ? c.x : nan;
        const double alpha = use_alpha ? c.y : nan;
        const double ss = j / alpha;
        const double delta_tau = alpha * delta_lambda_cgs;
        // (consumers: the intensity of an unpolarized run and tau_int; a polarized run integrates its Stokes rows elsewhere)
        const bool need_exp = (A.image_light && !A.polarized) || A.image_tau_int;
        const double exp_neg = need_exp ? bl_exp(-delta_tau) : 0.0;
        const double expm1 = need_exp ? bl_expm1(delta_tau) : 0.0;
        const bool optically_thin = delta_tau <= kDeltaTauMax;
        if (A.image_light && !A.polarized) {
          if (alpha > 0.0) {
            if (optically_thin)
              intensity = exp_neg * (intensity + ss * expm1);
            else
              intensity = ss;
          } else {
            intensity += j * delta_lambda_cgs;
          }
        }
        if (A.image_time && l == 0) time_min = std_min(time_min, t_cgs);
        if (A.image_length && l == 0) length += s.length_term;
        if (A.image_lambda || A.image_lambda_ave) integrated_lambda += delta_lambda_cgs;
        if (A.image_emission || A.image_emission_ave) integrated_emission += j * delta_lambda_cgs;
        if (A.image_tau) tau += delta_tau;
        const bool have_cell = !(s.cell[0] != s.cell[0]);
        if (A.image_lambda_ave && have_cell)
          for (int a = 0; a < BL_NUM_CELL_VALUES; a++) lambda_ave[a] += s.cell[a] * delta_lambda_cgs;
        if (A.image_emission_ave && have_cell)
          for (int a = 0; a < BL_NUM_CELL_VALUES; a++) emission_ave[a] += s.cell[a] * j * delta_lambda_cgs;
        if (A.image_tau_int && have_cell) {
          if (optically_thin)
            for (int a = 0; a < BL_NUM_CELL_VALUES; a++) tau_int[a] = exp_neg * (tau_int[a] + s.cell[a] * expm1);
          else
            for (int a = 0; a < BL_NUM_CELL_VALUES; a++) tau_int[a] = s.cell[a];
        }
        if (A.image_crossings && l == 0) {
          const bool plane_sign_new = s.plane > 0.0;
          if (plane_sign_new != plane_sign) crossings++;
          plane_sign = plane_sign_new;
        }
      }
      if (A.image_light && !A.polarized) img[(size_t)l * row] = intensity * (freq * freq * freq);   // :200-208
      if (A.image_time && l == 0) img[(size_t)A.offset_time * row] = time_min;
      if (A.image_length && l == 0) img[(size_t)A.offset_length * row] = length;
      if (A.image_lambda) img[(size_t)(A.offset_lambda + l) * row] = integrated_lambda;
      if (A.image_emission) img[(size_t)(A.offset_emission + l) * row] = integrated_emission;
      if (A.image_tau) img[(size_t)(A.offset_tau + l) * row] = tau;
      if (A.image_crossings && l == 0) img[(size_t)A.offset_crossings * row] = (double)crossings;
      for (int a = 0; a < BL_NUM_CELL_VALUES; a++) {
        if (A.image_lambda_ave) img[(size_t)(A.offset_lambda_ave + l * BL_NUM_CELL_VALUES + a) * row] = lambda_ave[a] / integrated_lambda;
        if (A.image_emission_ave) img[(size_t)(A.offset_emission_ave + l * BL_NUM_CELL_VALUES + a) * row] = emission_ave[a] / integrated_emission;
        if (A.image_tau_int) img[(size_t)(A.offset_tau_int + l * BL_NUM_CELL_VALUES + a) * row] = tau_int[a];
      }
    }
  }
  for (int offset = 32; offset > 0; offset >>= 1) {
    samples += __shfl_xor(samples, offset, 64);
    flagged += __shfl_xor(flagged, offset, 64);
    int other = __shfl_xor(max_num, offset, 64);
    max_num = other > max_num ? other : max_num;
  }
  if ((threadIdx.x & 63) == 0) {
    if (samples) atomicAdd(&P.stats[0], samples);
    if (flagged) atomicAdd(&P.stats[1], flagged);
    atomicMax(&P.stats[2], (unsigned long long)max_num);
  }
}

// Optical depth beside the intensities in the tolerant tier: tau(ray, frequency) = sum of alpha x length over the ray's samples, far
// -> near as the reference adds them (unpolarized.cpp:63-151), from the increments the fast coefficient kernel left
__global__ void __launch_bounds__(256) bl_tau_kernel(BlTransferArgs P) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int slot = (int)(t / P.n_nu);
  const int l = (int)(t % P.n_nu);
  if (slot >= bl_rays_done(P.counters, P.chunk_rays)) return;
  const int num = P.ray_sample_num[slot];
  const double *inc = P.tau_inc + (size_t)P.ray_offset[slot] * P.n_nu + l;
  double tau = 0.0;
  int n = num - 1;
  if (P.fallback_nan && P.ray_flags[slot] != 0) {   // every sample of a flagged ray carries NaN primitives (simulation_sampling.cpp:211-216)
    tau = num > 0 ? __longlong_as_double(0x7ff8000000000000ll) : 0.0;
    n = -1;
  }
  for (; n >= 7; n -= 8) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; u++) v[u] = inc[(size_t)(n - u) * P.n_nu];
#pragma unroll
    for (int u = 0; u < 8; u++) tau += v[u];
  }
  for (; n >= 0; n--) tau += inc[(size_t)n * P.n_nu];
  P.image[(size_t)(P.tau_row + l) * P.n_rays_total + P.ray_out_index[slot]] = tau;
}

extern "C" hipError_t bl_launch_tau(const BlTransferArgs *args, hipStream_t stream) {
  const int grid = (int)(((long long)args->chunk_rays * args->n_nu + 255) / 256);
  hipLaunchKernelGGL(bl_tau_kernel, dim3(grid), dim3(256), 0, stream, *args);
  return hipGetLastError();
}

// Tolerant tier, one frequency: four lanes per ray. I <- a I + c is an affine map and maps compose - (a2, c2) after (a1, c1) is
// (a2 a1, a2 c1 + c2) - so the four lanes of a quad take four consecutive records (64 contiguous bytes where a lane per ray reads
// 16 from each of 64 different lines), compose them in order by two steps of a scan inside the quad, and the quad's map is applied to
// the running intensity. Same records, same order of application; the association differs (rounding level: the tier's tolerance).
// (Measured on the benchmark frame: 2.4 ms against the lane-per-ray kernel's 2.9; two lanes per ray 2.8, eight 3.6, sixteen 6.7 - beyond
// a quad the scan's moves go through the LDS crossbar instead of DPP; 4, 8 or 16 records per lane in flight make no difference.)
__global__ void __launch_bounds__(256) bl_transfer_quad_kernel(BlTransferArgs P) {
  constexpr int kLanes = 4, kShift = 2;
  constexpr int kBatch = 8;   // records per lane in flight
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  int slot = (int)(t >> kShift);
  const int q = (int)(t & (kLanes - 1));
  const bool mirror = bl_mirror_slot(P, &slot);
  unsigned long long samples = 0ull, flagged = 0ull;
  int max_num = 0;
  if (slot < bl_rays_done(P.counters, P.chunk_rays)) {
    const int num = P.ray_sample_num[slot];
    const bool flag = P.ray_flags[slot] != 0;
    const long long out_index = mirror ? P.mirror_out_index[slot] : P.ray_out_index[slot];
    const int all = num + (P.ray_skipped != nullptr ? P.ray_skipped[slot] : 0);
    if (q == 0) {
      samples = (unsigned long long)all;
      flagged = flag ? 1ull : 0ull;
      max_num = all;
      if (P.out_sample_num != nullptr) P.out_sample_num[out_index] = all;
      if (P.out_flags != nullptr) P.out_flags[out_index] = flag ? 1 : 0;
    }
    double intensity = 0.0;
    if (P.fallback_nan && flag) {
      intensity = num > 0 ? __longlong_as_double(0x7ff8000000000000ll) : 0.0;   // simulation_sampling.cpp:211-216
    } else {
      const double2 *rec = P.transfer + (size_t)(P.ray_offset[slot] + (mirror ? P.row_add : 0ll));
      for (int top = num - 1; top >= 0; top -= kLanes * kBatch) {   // far -> near (geodesics.cpp:832-840)
        double2 m[kBatch];
#pragma unroll
        for (int u = 0; u < kBatch; u++) {
          const int n = top - kLanes * u - q;
          m[u] = n >= 0 ? rec[n] : make_double2(1.0, 0.0);
        }
#pragma unroll
        for (int u = 0; u < kBatch; u++) {
          double a = m[u].x, c = m[u].y;
          // a = -0.0 marks an optically thick step, whose intensity replaces whatever lies behind it - a NaN included (unpolarized.cpp:
          // 103-104, BL_AFFINE_THICK; a thin step's a may round to +0 and a product of them underflow, behind which a NaN stays a
          // NaN). A segment that holds a thick step keeps its map; the sign of a product carries the mark of what a segment without
          // one is composed with (every other a is positive or +0), so the sign bit of a is the flag at every stage of the scan.
#pragma unroll
          for (int d = 1; d < kLanes; d <<= 1) {
            const double pa = __shfl_up(a, d, kLanes), pc = __shfl_up(c, d, kLanes);   // the map of the d records before this lane's segment
            if (q >= d && !BL_IS_AFFINE_THICK(a)) {
              c = __builtin_fma(a, pc, c);
              a *= pa;
            }
          }
          const double block_a = __shfl(a, kLanes - 1, kLanes), block_c = __shfl(c, kLanes - 1, kLanes);
          intensity = BL_IS_AFFINE_THICK(block_a) ? block_c : __builtin_fma(block_a, intensity, block_c);
        }
      }
    }
    if (q == 0) {
      const double freq = P.frequencies[0];
      P.image[out_index] = intensity * (freq * freq * freq);   // unpolarized.cpp:206-207
    }
  }
  for (int offset = 32; offset > 0; offset >>= 1) {
    samples += __shfl_xor(samples, offset, 64);
    flagged += __shfl_xor(flagged, offset, 64);
    const int other = __shfl_xor(max_num, offset, 64);
    max_num = other > max_num ? other : max_num;
  }
  if ((threadIdx.x & 63) == 0) {
    if (samples) atomicAdd(&P.stats[0], samples);
    if (flagged) atomicAdd(&P.stats[1], flagged);
    atomicMax(&P.stats[2], (unsigned long long)max_num);
  }
}

// Tolerant tier, composed maps (BlShadeArgs::composed; one frequency): one lane per ray applies the ray's segment maps far -> near -
// about a seventh of the per-sample records, already composed by the coefficient kernel. A row that stands for per-sample
// records (BL_COMPOSED_EXPANDED: its wave held a sample for the exact kernel or a thick step) is replayed from those.
__global__ void __launch_bounds__(256) bl_transfer_composed_kernel(BlTransferArgs P) {
  int slot = blockIdx.x * blockDim.x + threadIdx.x;
  const bool mirror = bl_mirror_slot(P, &slot);
  unsigned long long samples = 0ull, flagged = 0ull;
  int max_num = 0;
  if (slot < bl_rays_done(P.counters, P.chunk_rays)) {
    const int num = P.ray_sample_num[slot];
    const bool flag = P.ray_flags[slot] != 0;
    const long long out_index = mirror ? P.mirror_out_index[slot] : P.ray_out_index[slot];
    const int all = num + (P.ray_skipped != nullptr ? P.ray_skipped[slot] : 0);   // the ray's samples, with or without a record
    samples = (unsigned long long)all;
    flagged = flag ? 1ull : 0ull;
    max_num = all;
    if (P.out_sample_num != nullptr) P.out_sample_num[out_index] = all;
    if (P.out_flags != nullptr) P.out_flags[out_index] = flag ? 1 : 0;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double intensity = 0.0;
    if (P.fallback_nan && flag) {
      intensity = num > 0 ? nan : 0.0;   // every sample of a flagged ray carries NaN primitives (simulation_sampling.cpp:211-216)
    } else {
      const double2 *rows = P.composed + (size_t)(P.ray_offset[slot] + (mirror ? P.row_add : 0ll));
      auto apply = [&](const double2 map) {
        if (__builtin_expect(BL_COMPOSED_EXPANDED(map.x), 0)) {
          const int length = (int)(-map.x);
          const double2 *rec = P.transfer + (size_t)(unsigned long long)__double_as_longlong(map.y);
          for (int i = length - 1; i >= 0; i--) {
            const double2 ac = rec[i];
            intensity = BL_IS_AFFINE_THICK(ac.x) ? ac.y : __builtin_fma(ac.x, intensity, ac.y);   // (unpolarized.cpp:103-104: see bl_transfer_kernel)
          }
        } else {
          intensity = BL_IS_AFFINE_THICK(map.x) ? map.y : __builtin_fma(map.x, intensity, map.y);
        }
      };
      int s = P.ray_rows[slot] - 1;
      for (; s >= 7; s -= 8) {   // eight loads in flight per lane
        double2 maps[8];
#pragma unroll
        for (int u = 0; u < 8; u++) maps[u] = rows[s - u];
#pragma unroll
        for (int u = 0; u < 8; u++) apply(maps[u]);
      }
      for (; s >= 0; s--) apply(rows[s]);
    }
    const double freq = P.frequencies[0];
    P.image[out_index] = intensity * (freq * freq * freq);   // unpolarized.cpp:206-207
  }
  for (int offset = 32; offset > 0; offset >>= 1) {
    samples += __shfl_xor(samples, offset, 64);
    flagged += __shfl_xor(flagged, offset, 64);
    int other = __shfl_xor(max_num, offset, 64);
    max_num = other > max_num ? other : max_num;
  }
  if ((threadIdx.x & 63) == 0) {
    if (samples) atomicAdd(&P.stats[0], samples);
    if (flagged) atomicAdd(&P.stats[1], flagged);
    atomicMax(&P.stats[2], (unsigned long long)max_num);
  }
}

// The transfer kernel of the plan: grid, workgroup and kernel per kind (no dynamic LDS)
extern "C" hipError_t bl_launch_transfer(const BlTransferArgs *args, const KernelPlan::Transfer &plan, hipStream_t stream) {
  using Transfer = KernelPlan::Transfer;
  const long long rays = args->chunk_rays;
  void (*kernel)(BlTransferArgs) = nullptr;
  long long lanes = rays * args->n_nu;   // a lane per ray and frequency
  int block = 256;
  switch (plan.kind) {
    case Transfer::kAux:
      if (args->aux == nullptr && !args->aux_images.polarized_rows_only) return hipErrorInvalidValue;
      kernel = bl_transfer_aux_kernel, lanes = rays, block = 64;
      break;
    case Transfer::kFreq:   // ... and model and unit
      if (args->freq_inputs == nullptr) return hipErrorInvalidValue;
      kernel = bl_transfer_freq_kernel, lanes *= args->n_models > 0 ? args->n_models * (args->n_units > 0 ? args->n_units : 1) * (args->n_cuts > 0 ? args->n_cuts : 1) : 1;
      if (args->n_mixes > 0) {   // a workgroup per (256 rays, mix, channel): the lane's constants are scalars in the kernel
        // (the mixes ride on the model-free row; no mirror pairs here, as below)
        if (args->n_models <= 0 || args->n_mixes > BL_TRANSFER_MAX_MIXES || plan.affine != (args->affine != 0) || args->mirror_rays > 0) return hipErrorInvalidValue;
        const long long groups = (rays + block - 1) / block, per_group = lanes / (rays > 0 ? rays : 1) * args->n_mixes;
        if (groups * per_group >= (1ll << 31)) return hipErrorInvalidValue;
        hipLaunchKernelGGL(kernel, dim3((unsigned int)(groups * per_group)), dim3(block), 0, stream, *args);
        return hipGetLastError();
      }
      break;
    case Transfer::kComposed:
      if (args->composed == nullptr || !plan.affine) return hipErrorInvalidValue;
      kernel = bl_transfer_composed_kernel, lanes = rays;
      break;
    case Transfer::kQuad:   // four lanes per ray
      if (!plan.affine || args->n_nu != 1 || args->lane_transfer) return hipErrorInvalidValue;
      kernel = bl_transfer_quad_kernel, lanes = rays * 4;
      break;
    case Transfer::kLane:
      kernel = plan.affine ? bl_transfer_kernel<true> : bl_transfer_kernel<false>;
      break;
  }
  if (plan.affine != (args->affine != 0)) return hipErrorInvalidValue;
  if (args->mirror_rays > 0) {   // mirror pairs: the three kernels that know them, a second set of lanes for the mirror pixels
    if ((plan.kind != Transfer::kComposed && plan.kind != Transfer::kQuad && plan.kind != Transfer::kLane) || args->mirror_rays != args->chunk_rays
        || args->mirror_out_index == nullptr) return hipErrorInvalidValue;
    lanes *= 2;
  }
  hipLaunchKernelGGL(kernel, dim3((unsigned int)((lanes + block - 1) / block)), dim3(block), 0, stream, *args);
  return hipGetLastError();
}
