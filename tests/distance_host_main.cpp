// distance_host_main.cpp - the closed-form proper distance (blacklight_amd/csrc/bl_distance_closed.h) against the reference's, on the
// CPU: rays integrated with bl_geodesic_rhs<true> and the Dormand-Prince tableau and controller of bl_geodesic.hip, carrying the
// reference's s and the closed mode's quantities (increment, sum of absolute terms, S_hi, Q, band) side by side along one trajectory
// (the proper distance enters no right-hand side and no error norm, so both modes walk the same points). tests/test_distance_host.py
// builds it with -ffp-contract=off, reads the figures below and holds them to the bounds of the header.
//
//   distance_host_main <set>      set = a0 | ring | a09 | a05 | flat | a0_loose | a09_loose | a0_tight
// (the last three: the controller away from tolerances of 1e-8 - 1e-3 with ray_step = 0.3, where an accepted step is long and its stages lie
// far from the accepted path, and 1e-12, where nearly every step's error is near 1)
// prints one `name value` line per figure; exit code 0 unless a ray set is unknown. What the header assumes of a stage's point is counted
// for the stages of accepted steps - the ones whose d s / d lambda enter a count - and, under rejected_*, for those of rejected steps.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "bl_distance_closed.h"

namespace {

// Dormand-Prince RK5(4)7M (bl_geodesic_common.h, which names device types and cannot be included here)
constexpr double kA[7][6] = {
    {0.0, 0.0, 0.0, 0.0, 0.0, 0.0},
    {1.0 / 5.0, 0.0, 0.0, 0.0, 0.0, 0.0},
    {3.0 / 40.0, 9.0 / 40.0, 0.0, 0.0, 0.0, 0.0},
    {44.0 / 45.0, -56.0 / 15.0, 32.0 / 9.0, 0.0, 0.0, 0.0},
    {19372.0 / 6561.0, -25360.0 / 2187.0, 64448.0 / 6561.0, -212.0 / 729.0, 0.0, 0.0},
    {9017.0 / 3168.0, -355.0 / 33.0, 46732.0 / 5247.0, 49.0 / 176.0, -5103.0 / 18656.0, 0.0},
    {35.0 / 384.0, 0.0, 500.0 / 1113.0, 125.0 / 192.0, -2187.0 / 6784.0, 11.0 / 84.0}};
constexpr double kB5[7] = {35.0 / 384.0, 0.0, 500.0 / 1113.0, 125.0 / 192.0, -2187.0 / 6784.0, 11.0 / 84.0, 0.0};
constexpr double kB4[7] = {5179.0 / 57600.0, 0.0, 7571.0 / 16695.0, 393.0 / 640.0, -92097.0 / 339200.0, 187.0 / 2100.0, 1.0 / 40.0};
constexpr double kB4m[7] = {6025192743.0 / 30085553152.0, 0.0, 51252292925.0 / 65400821598.0, -2691868925.0 / 45128329728.0,
                            187940372067.0 / 1594534317056.0, -1776094331.0 / 19743644256.0, 11237099.0 / 235043384.0};

constexpr double kU = 0x1p-53;
// the relative distance of the two derivatives the header's table allows: the closed form's, the reference's, the l.l term
constexpr double kDerivativeBound = (30.0 + 1591.0 + 102.0) * kU;

struct Setup {
  BlSpacetime st;
  double camera_r, inclination, width;
  double ray_step = 0.01, tol_abs = 1.0e-8, tol_rel = 1.0e-8, ray_factor = 1.005;
  int max_steps = 2000, max_retries = 20;
};

struct Figures {
  long long rays = 0, steps = 0, undecided = 0, ceil_mismatch = 0, stages = 0, assumption_failures = 0, flagged = 0;
  double max_ratio = 0.0, max_derivative = 0.0, max_eps_l = 0.0, max_kt_over_k = 0.0, max_f = 0.0, max_s = 0.0, max_band = 0.0;
  // the same of the stages of rejected steps, which enter no count: kept apart (a step of 0.3 r near the hole is rejected for what its
  // stages look like)
  long long rejected_assumption_failures = 0;
  double rejected_max_eps_l = 0.0, rejected_max_kt_over_k = 0.0, rejected_max_f = 0.0;
};

// one stage: the derivatives of (t, x, y, z, k_x, k_y, k_z), the reference's d s / d lambda and the closed form's, r
template <bool kSpinZero>
void Stage(const Setup &su, const double y[8], double kt, double k[8], double *ds_closed, double *r, Figures *fig) {
  const double pos[3] = {y[1], y[2], y[3]}, kcov[4] = {kt, y[4], y[5], y[6]};
  double dpos[4], dk[3], ds = 0.0, dpos_c[4], dk_c[3], r_c = 0.0;
  *ds_closed = 0.0;
  bl_geodesic_rhs<true, kSpinZero>(su.st, pos, kcov, dpos, dk, &ds, r, BL_DISTANCE_EXACT);
  bl_geodesic_rhs<true, kSpinZero>(su.st, pos, kcov, dpos_c, dk_c, ds_closed, &r_c, BL_DISTANCE_CLOSED);
  for (int p = 0; p < 4; p++) k[p] = dpos[p];
  for (int p = 0; p < 3; p++) k[4 + p] = dk[p];
  k[7] = ds;
  const double r_horizon = su.st.bh_m + std::sqrt(su.st.bh_m * su.st.bh_m - su.st.bh_a * su.st.bh_a);
  if (su.st.ray_flat || !(*r >= 0.5 * r_horizon)) return;   // (flat: both forms are the same operations; below: the step is not decided)
  fig->stages++;
  const double distance = std::fabs(*ds_closed - ds) / std::fabs(ds);
  if (!(distance <= fig->max_derivative)) fig->max_derivative = distance;
  // what the header assumes of a stage's point
  BlKerrSchild ks;
  bl_kerr_schild<kSpinZero>(su.st, pos[0], pos[1], pos[2], &ks);
  const double eps = std::fabs(ks.l[0] * ks.l[0] + ks.l[1] * ks.l[1] + ks.l[2] * ks.l[2] - 1.0);
  const double kt_over_k = std::fabs(kt) / std::sqrt(kcov[1] * kcov[1] + kcov[2] * kcov[2] + kcov[3] * kcov[3]);
  if (!(eps <= fig->max_eps_l)) fig->max_eps_l = eps;
  if (!(kt_over_k <= fig->max_kt_over_k)) fig->max_kt_over_k = kt_over_k;
  if (!(ks.f <= fig->max_f)) fig->max_f = ks.f;
  if (!(eps <= 64.0 * kU && kt_over_k <= 2.0 && ks.f <= 4.0)) fig->assumption_failures++;
}

// The start of a plane camera's ray at (u, v) M in the image plane: a photon that moves along the camera's normal, away from the hole
void StartRay(const Setup &su, double u, double v, double y[8], double *kt) {
  const double th = su.inclination * (3.14159265358979323846 / 180.0);
  const double n[3] = {std::sin(th), 0.0, std::cos(th)};
  const double e_u[3] = {0.0, 1.0, 0.0}, e_v[3] = {n[1] * e_u[2] - n[2] * e_u[1], n[2] * e_u[0] - n[0] * e_u[2], n[0] * e_u[1] - n[1] * e_u[0]};
  double x[3];
  for (int i = 0; i < 3; i++) x[i] = su.camera_r * n[i] + u * e_u[i] + v * e_v[i];
  double g[4][4];
  bl_gcov(su.st, x[0], x[1], x[2], g);
  // g_tt (k^t)^2 + 2 g_ti n^i k^t + g_ij n^i n^j = 0, the future-directed root
  double b = 0.0, c = 0.0;
  for (int i = 0; i < 3; i++) {
    b += g[0][i + 1] * n[i];
    for (int j = 0; j < 3; j++) c += g[i + 1][j + 1] * n[i] * n[j];
  }
  const double a = g[0][0];
  const double k_up[4] = {(-b - std::sqrt(b * b - a * c)) / a, n[0], n[1], n[2]};
  double k_cov[4];
  for (int mu = 0; mu < 4; mu++) {
    k_cov[mu] = 0.0;
    for (int nu = 0; nu < 4; nu++) k_cov[mu] += g[mu][nu] * k_up[nu];
  }
  y[0] = 0.0;
  for (int i = 0; i < 3; i++) y[1 + i] = x[i], y[4 + i] = k_cov[1 + i];
  y[7] = 0.0;
  *kt = k_cov[0];
}

template <bool kSpinZero>
void TraceRay(const Setup &su, double u, double v, Figures *fig) {
  const BlSpacetime &st = su.st;
  const double r_horizon = st.bh_m + std::sqrt(st.bh_m * st.bh_m - st.bh_a * st.bh_a), r_terminate = r_horizon * su.ray_factor;
  double y[8], kt, k[7][8], kc[7];   // kc: the closed form's d s / d lambda per stage
  StartRay(su, u, v, y, &kt);
  double r_cur = bl_radial_coordinate<kSpinZero>(st, y[1], y[2], y[3]);
  const double camera_r = r_cur;
  double unused;
  Stage<kSpinZero>(su, y, kt, k[0], &unused, &unused, fig);
  kc[0] = k[0][7];   // (the ray-start kernel's: the reference's form)
  double s_hi = 0.0, h_new = -su.ray_step * r_cur;
  int num_retry = 0, sample_num = 0;
  bool previous_fail = false;
  fig->rays++;
  while (true) {
    if (num_retry > su.max_retries) {
      fig->flagged++;
      return;
    }
    const double h = h_new;
    const Figures before = *fig;   // (of the assumptions' figures: a rejected step gives its stages' back below)
    fig->max_eps_l = fig->max_kt_over_k = fig->max_f = 0.0;
    double r_stage = r_cur, r_low = r_cur;
    for (int s = 1; s < 7; s++) {
      double yt[8];
      for (int p = 1; p < 7; p++) {
        double acc = y[p];
        for (int q = 0; q < s; q++) acc += kA[s][q] * h * k[q][p];
        yt[p] = acc;
      }
      yt[0] = yt[7] = 0.0;
      Stage<kSpinZero>(su, yt, kt, k[s], &kc[s], &r_stage, fig);
      if (r_stage < r_low) r_low = r_stage;
    }
    double y5[8], error = 0.0;
    for (int p = 0; p < 8; p++) {
      double a5 = y[p], a4 = y[p];
      for (int q = 0; q < 7; q++) {
        a5 += kB5[q] * h * k[q][p];
        a4 += kB4[q] * h * k[q][p];
      }
      y5[p] = a5;   // (component 7: the reference's s5, terms added in stage order as BL_FOLD adds them)
      if (p < 7) {
        const double scale = su.tol_abs + su.tol_rel * std::fmax(std::fabs(y[p]), std::fabs(a5));
        error = std::fmax(error, std::fabs(a5 - a4) / scale);
      }
    }
    const double r_new = r_stage;
    const Figures step = *fig;
    fig->max_eps_l = before.max_eps_l, fig->max_kt_over_k = before.max_kt_over_k, fig->max_f = before.max_f;
    if (!(error <= 1.0)) {
      fig->rejected_assumption_failures += step.assumption_failures - before.assumption_failures;
      fig->assumption_failures = before.assumption_failures;
      if (!(step.max_eps_l <= fig->rejected_max_eps_l)) fig->rejected_max_eps_l = step.max_eps_l;
      if (!(step.max_kt_over_k <= fig->rejected_max_kt_over_k)) fig->rejected_max_kt_over_k = step.max_kt_over_k;
      if (!(step.max_f <= fig->rejected_max_f)) fig->rejected_max_f = step.max_f;
      h_new = h * (std::isfinite(error) ? std::fmax(0.9 * std::pow(error, -0.2), 0.2) : 0.2);
      num_retry++;
      previous_fail = true;
      continue;
    }
    if (!(step.max_eps_l <= fig->max_eps_l)) fig->max_eps_l = step.max_eps_l;
    if (!(step.max_kt_over_k <= fig->max_kt_over_k)) fig->max_kt_over_k = step.max_kt_over_k;
    if (!(step.max_f <= fig->max_f)) fig->max_f = step.max_f;
    double h_factor = 10.0;
    if (error > 0.0) h_factor = std::fmin(std::fmax(0.9 * std::pow(error, -0.2), 0.2), 10.0);
    if (previous_fail) h_factor = std::fmin(h_factor, 1.0);
    h_new = h * h_factor;
    num_retry = 0;
    previous_fail = false;
    double y4m[4];
    for (int p = 1; p < 4; p++) {
      double acc = y[p];
      for (int q = 0; q < 7; q++) acc += kB4m[q] * h * k[q][p];
      y4m[p] = acc;
    }
    const double delta_s_step = su.ray_step * bl_radial_coordinate<kSpinZero>(st, y4m[1], y4m[2], y4m[3]);
    // the reference's count
    const double q_ref = (y5[7] - y[7]) / delta_s_step;
    const int n_ref = static_cast<int>(std::ceil(q_ref));
    // the closed mode's, with the kernel's operations
    double delta = 0.0, abs_sum = 0.0;
    for (int q = 0; q < 7; q++) {
      if (kB5[q] == 0.0) continue;
      const double term = kB5[q] * h * kc[q];
      delta += term;
      abs_sum += std::fabs(term);
    }
    s_hi = (s_hi + abs_sum) * kDistanceInflate;
    const BlRecip rc_step = bl_recip(delta_s_step);
    const double q_closed = bl_div_r(delta, rc_step);
    const double bound = bl_div_r(bl_distance_bound_numerator(abs_sum, s_hi), rc_step);
    const double band = kDistanceBandFactor * bound, n_closed = std::ceil(q_closed);
    const bool decided = bl_distance_decided(q_closed, n_closed, band, st.ray_flat ? r_horizon : r_low, r_horizon);
    fig->steps++;
    if (r_low >= 0.5 * r_horizon || st.ray_flat) {   // (the bound is claimed where the header's assumptions hold)
      const double ratio = std::fabs(q_ref - q_closed) / bound;
      if (!(ratio <= fig->max_ratio)) fig->max_ratio = ratio;
      if (!(band <= fig->max_band)) fig->max_band = band;
    }
    if (!decided) fig->undecided++;
    else if (static_cast<int>(n_closed) != n_ref) fig->ceil_mismatch++;
    if (!(std::fabs(y5[7]) <= fig->max_s)) fig->max_s = std::fabs(y5[7]);
    // finish the step as the kernel does, with the reference's count
    sample_num += std::min(n_ref, su.max_steps - sample_num);
    const double factor = bl_renormalization_factor<kSpinZero>(st, y5[1], y5[2], y5[3], kt, y5[4], y5[5], y5[6]);
    for (int p = 4; p < 7; p++) y5[p] *= factor;
    const bool finish = (r_new > camera_r && r_new > r_cur) || r_new < r_terminate || sample_num >= su.max_steps;
    if (sample_num >= su.max_steps && !(r_new < r_terminate) && !(r_new > camera_r)) fig->flagged++;
    std::memcpy(y, y5, sizeof y5);
    std::memcpy(k[0], k[6], sizeof k[0]);
    kc[0] = kc[6];
    r_cur = r_new;
    if (finish) return;
  }
}

void Trace(const Setup &su, double u, double v, Figures *fig) {
  if (su.st.bh_a == 0.0) TraceRay<true>(su, u, v, fig);
  else TraceRay<false>(su, u, v, fig);
}

void Lattice(const Setup &su, int n, Figures *fig) {
  for (int j = 0; j < n; j++)
    for (int i = 0; i < n; i++) Trace(su, su.width * ((i + 0.5) / n - 0.5), su.width * ((j + 0.5) / n - 0.5), fig);
}

}  // namespace

int main(int argc, char **argv) {
  const std::string set = argc > 1 ? argv[1] : "";
  Setup su{};
  su.st = BlSpacetime{1.0, 0.0, 0};
  su.camera_r = 50.0;
  su.inclination = 45.0;
  su.width = 24.0;
  Figures fig;
  if (set == "a0") {
    Lattice(su, 64, &fig);
  } else if (set == "ring") {   // 200 impact parameters within 1e-3 of the photon ring's 3 sqrt(3) M
    for (int n = 0; n < 200; n++) Trace(su, 3.0 * std::sqrt(3.0) * (1.0 + 1.0e-3 * ((n + 0.5) / 100.0 - 1.0)), 0.0, &fig);
  } else if (set == "a09") {    // the formula case's spin and distance: large s
    su.st.bh_a = 0.9;
    su.camera_r = 1000.0;
    su.inclination = 60.0;
    su.max_steps = 20000;
    Lattice(su, 64, &fig);
  } else if (set == "a0_loose") {
    su.tol_abs = su.tol_rel = 1.0e-3;
    su.ray_step = 0.3;
    Lattice(su, 64, &fig);
  } else if (set == "a09_loose") {
    su.st.bh_a = 0.9;
    su.camera_r = 1000.0;
    su.inclination = 60.0;
    su.max_steps = 20000;
    su.tol_abs = su.tol_rel = 1.0e-3;
    su.ray_step = 0.3;
    Lattice(su, 64, &fig);
  } else if (set == "a0_tight") {
    su.tol_abs = su.tol_rel = 1.0e-12;
    Lattice(su, 64, &fig);
  } else if (set == "a05") {
    su.st.bh_a = 0.5;
    su.inclination = 80.0;
    Lattice(su, 64, &fig);
  } else if (set == "flat") {
    su.st.ray_flat = 1;
    Lattice(su, 64, &fig);
  } else {
    std::fprintf(stderr, "usage: distance_host_main a0|ring|a09|a05|flat|a0_loose|a09_loose|a0_tight\n");
    return 2;
  }
  std::printf("rays %lld\nsteps %lld\nstages %lld\nundecided %lld\nceil_mismatch %lld\nassumption_failures %lld\nflagged %lld\n", fig.rays, fig.steps, fig.stages,
              fig.undecided, fig.ceil_mismatch, fig.assumption_failures, fig.flagged);
  std::printf("max_ratio %.6e\nmax_derivative %.6e\nderivative_bound %.6e\nmax_eps_l_in_u %.3f\nmax_kt_over_k %.6f\nmax_f %.6f\nmax_s %.6e\nmax_band %.6e\n",
              fig.max_ratio, fig.max_derivative, kDerivativeBound, fig.max_eps_l / kU, fig.max_kt_over_k, fig.max_f, fig.max_s, fig.max_band);
  std::printf("rejected_assumption_failures %lld\nrejected_max_eps_l_in_u %.3f\nrejected_max_kt_over_k %.6f\nrejected_max_f %.6f\n", fig.rejected_assumption_failures,
              fig.rejected_max_eps_l / kU, fig.rejected_max_kt_over_k, fig.rejected_max_f);
  return 0;
}
