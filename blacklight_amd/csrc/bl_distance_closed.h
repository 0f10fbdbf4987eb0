// bl_distance_closed.h - when the Dormand-Prince stepper may count a step's samples from the closed-form proper distance
// (bl_distance_closed, bl_geometry.h) instead of the reference's. Host and device; tests/distance_host_main.cpp runs the same functions.
//
// What the reference computes per accepted step (geodesics.cpp:162-245, bl_geodesic.hip):
//   s5 = s; s5 += fl(fl(b_q h) K_q) for q = 0 ... 6;  delta_s_full = fl(s5 - s);  Q_ref = fl(delta_s_full / delta_s_step);
//   num_steps_ideal = ceil(Q_ref)
// with K_q the stage's d s / d lambda. Nothing else reads s. The closed mode computes
//   delta = sum over q in {0, 2, 3, 4, 5} of fl(fl(b_q h) K'_q),  A = the same sum of absolute values,  Q = fl(delta / delta_s_step)
// (b_1 = b_6 = 0: those terms are exact zeros in the reference), K'_q from bl_distance_closed - K'_0 of a ray's first step from the
// ray-start kernel's exact form -, and keeps S_hi >= |every partial sum of s5| instead of s: S_hi <- (S_hi + A)(1 + 2^-40).
//
// |Q_ref - Q| <= bound = kDistanceCRel A / delta_s_step + kDistanceCAbs ulp(S_hi) / delta_s_step. u = 2^-53. Assumed, and why:
//   f <= 4         every stage point has r >= half the horizon's r >= M / 2, and f <= 2 M / r: the kernel checks the stages' r (the last
//                  step of a ray that falls in ends below r_terminate, a little above the horizon; its stages may lie a little below)
//   |k_t| <= 2 |k| the null condition gives |k_t| <= |k| (f + sqrt(1 + f)) / (1 + f) <= 1.25 |k|; the momentum is renormalised to it
//                  after every step and drifts by ray_tol within one. Needed of the stages of ACCEPTED steps only (a rejected step's
//                  enter no count): at ray_tol = 1e-3 with ray_step = 0.3 the stages of accepted steps reach 1.81, those of the
//                  rejected first tries near the hole 10.7 (the sets a0_loose, a09_loose of tests/distance_host_main.cpp)
//   |l.l - 1| = |eps| <= 64 u   the computed l (a = 0: x_i r / r^2 with r^2 the rounded sum of squares, 9 u; the general formulas
//                  through the rounded root of the quartic); tests/distance_host_main.cpp checks all three at every stage it evaluates,
//                  apart for accepted and for rejected steps
//
//   source                                         relative to A, in u     how
//   ---------------------------------------------  ----------------------  -----------------------------------------------------
//   products fl(b_q h) K, both forms               2                       one rounding each; fl(b_q h) is the same number
//   the four additions of delta                    4                       each <= u |partial sum| <= u A
//   the two quotients by delta_s_step              2                       one rounding each
//   K', closed form                                30                      k.k: 3; (l.k)^2 f / (1 + f): 3 + 3 + 1 for the square of
//                                                                          the sum, 2 for the quotient, 1 for the product = 10 f /
//                                                                          (1 + f) of k.k; the difference: 1; over K'^2 >= k.k /
//                                                                          (1 + f): 4 + 13 f <= 56, eps in the bound: 58; halved by
//                                                                          the root, + 1 for its rounding
//   K, the reference's form                        1591                    a coefficient gamma^{aj}: 2 f (f l_a, then (f l_a) l_j)
//                                                                          + (1 + f) (the + 1) + 5 f^2 / (1 + f) (the product of two
//                                                                          rounded f l over a rounded g^00, two roundings) + (1 + f)
//                                                                          (the difference) <= 34; a row: 34 sqrt(3) |k| + (1 + 3) |k|
//                                                                          (products, additions; a row of gamma^-1 has norm <= 1)
//                                                                          + 4 f |k| (the residue (g0a - fl(fl(g0a g00) / g00)) k_t,
//                                                                          <= 2 u f |k_t|) <= 79 |k|; the vector: 137 |k|; through
//                                                                          the form gamma_ab (norm 1 + f) with |temp| <= K and |k| <=
//                                                                          sqrt(1 + f) K: 2 (1 + f)^1.5 137 = 3064 of K^2; the form's
//                                                                          entries (2 f + 1 + f), two products and eight additions of
//                                                                          nine terms: 23 (1 + f) = 115; halved by the root, + 1
//   l.l = 1 + eps: the two forms differ exactly    102                     d/dL of the reference's bracket -2c + c^2 L + f (1 - c L)^2,
//                                                                          c = f / (1 + f), is -c^2 at L = 1: c^2 (1 + f) eps = 3.2 eps
//                                                                          of K^2, 1.6 eps of K
//   ---------------------------------------------  ----------------------
//   sum                                            1731  ->  kDistanceCRel = 2048 u = 2^-42
//
//   the reference's accumulation                   absolute, in ulp(S_hi)
//   five additions of non-zero terms into s5       5 / 2                   each <= half an ulp of a partial sum, all <= S_hi
//   the difference s5 - s                          1 / 2
//   ---------------------------------------------  ----------------------
//   sum                                            3  =  kDistanceCAbs     (ulp(S_hi) <= 2^-52 S_hi is what is evaluated)
//
// These are worst cases added up, not estimates: the largest |Q_ref - Q| / bound the host program has seen is in
// profiles/closed_distance.md. The band is kDistanceBandFactor = 16 times the bound, for what a hand analysis may have missed. A step
// is DECIDED when no integer lies within the band of Q; then ceil(Q) = ceil(Q_ref). Expected share of undecided steps: twice the band,
// ~7e-12 A / delta_s_step per step.
#ifndef BLACKLIGHT_AMD_BL_DISTANCE_CLOSED_H_
#define BLACKLIGHT_AMD_BL_DISTANCE_CLOSED_H_

#include "bl_geometry.h"

constexpr double kDistanceCRel = 0x1p-42;          // 2048 u
constexpr double kDistanceCAbs = 3.0;              // ulps of S_hi
constexpr double kDistanceBandFactor = 16.0;
constexpr double kDistanceInflate = 1.0 + 0x1p-40; // S_hi's growth per step: covers the roundings of its own two operations
constexpr double kDistanceWideBand = 0.25;         // BL_SWITCH_WIDE_DISTANCE_BAND: nearly every ray has an undecided step
constexpr double kDistanceMaxQ = 0x1p30;           // above this (int)ceil(Q) is not trusted to fit

// The bound on |Q_ref - Q| in units of delta_s_step: what is divided by delta_s_step to give the bound in Q
BL_HD double bl_distance_bound_numerator(double abs_sum, double s_hi) {
  return kDistanceCRel * abs_sum + kDistanceCAbs * (0x1p-52 * s_hi);
}

// Whether ceil(Q) is ceil(Q_ref) for every Q_ref within `band` of Q: n = ceil(Q) as a double, r_low the least r of the step's stages
BL_HD bool bl_distance_decided(double q, double n, double band, double r_low, double r_horizon) {
  return q - q == 0.0 && q > band && q < kDistanceMaxQ && n - q > band && q - (n - 1.0) > band && r_low >= 0.5 * r_horizon;
}

#endif  // BLACKLIGHT_AMD_BL_DISTANCE_CLOSED_H_
