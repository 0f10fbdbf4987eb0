// bl_geometry.h - Kerr geometry in Cartesian Kerr-Schild coordinates for host and gfx950 device.
//
// Arithmetic contract: every value produced here is bit-identical to what the reference computes
// in src/geodesic_integrator/geodesic_geometry.cpp (and its duplicate in
// src/radiation_integrator/radiation_geometry.cpp) when both use the same hypot. The reference
// evaluates the same scalars (r, f, l_i) three times per right-hand side (once each in
// Covariant/Contravariant/...Derivative); here they are evaluated once and the 16 + 16 + 48 tensor
// components are never materialised. That is exact, not approximate, because
//   * identical operations on identical inputs give identical bits (common subexpressions),
//   * multiplying by l_0 = +-1 and negating are exact, fl(-a - b) = -fl(a + b),
//   * terms with the vanishing derivative d(l_0) = 0 contribute +-0, and x + (+-0) = x for x != 0
//     (the reference itself is built with -fno-signed-zeros).
// Everything else keeps the reference's operand order, e.g. g_ij = (f*l_i)*l_j is NOT symmetrised.
// The translation unit must be compiled with -ffp-contract=off.
#ifndef BLACKLIGHT_AMD_BL_GEOMETRY_H_
#define BLACKLIGHT_AMD_BL_GEOMETRY_H_

#include "blmath.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define BL_HD __host__ __device__ __forceinline__
#else
#define BL_HD inline
#endif

// ---- division by a shared denominator ----------------------------------------------------------
// IEEE-754 division a / b, correctly rounded, organised so that several numerators over the same
// denominator share the reciprocal. On gfx950 the compiler expands every fp64 `/` into
//   v_div_scale x2, v_rcp, 2 Newton steps (4 fma), mul, fma, v_div_fmas, v_div_fixup
// where the two v_div_scale and the scaling half of v_div_fmas only act when an exponent is close to
// the edge of the fp64 range. bl_recip()/bl_div_r() issue the same rcp + Newton + residual sequence
// without the scaling (5 instructions per denominator + 4 per numerator instead of 11 per quotient)
// and keep v_div_fixup, which restores the exact IEEE result for zeros, infinities and NaNs.
// Bit-identical to `/` whenever no scaling would have happened, i.e. for
//   2^-1000 < |b| < 2^1000,  a == 0 or 2^-900 < |a| < 2^1000,  2^-1000 < |a / b| < 2^1000.
// Used ONLY where both operands are built from coordinates, metric components and O(1) velocities /
// field components (all within 2^+-200 for any ray the reference itself can integrate); quantities in
// cgs units that can under- or overflow (emissivities, optical depths) keep the plain `/`.
// On the host both functions are a plain division.
struct BlRecip {
  double d;   // the denominator
  double y;   // its reciprocal after two Newton steps (device only)
};
BL_HD BlRecip bl_recip(double b) {
  BlRecip rc;
  rc.d = b;
#if defined(__HIP_DEVICE_COMPILE__)
  double y = __builtin_amdgcn_rcp(b);
  double e = __builtin_fma(-b, y, 1.0);
  y = __builtin_fma(y, e, y);
  e = __builtin_fma(-b, y, 1.0);
  y = __builtin_fma(y, e, y);
  rc.y = y;
#else
  rc.y = 0.0;
#endif
  return rc;
}
BL_HD double bl_div_r(double a, const BlRecip &rc) {
#if defined(__HIP_DEVICE_COMPILE__)
  double q = a * rc.y;
  double r = __builtin_fma(-rc.d, q, a);
  q = __builtin_fma(r, rc.y, q);
  return __builtin_amdgcn_div_fixup(q, rc.d, a);
#else
  return a / rc.d;
#endif
}
BL_HD double bl_div_g(double a, double b) { return bl_div_r(a, bl_recip(b)); }

// ---- square root and hypot for geometric operands -----------------------------------------------
// bl_sqrt_g: the compiler's correctly rounded fp64 square root (v_rsq + two coupled Newton steps)
// without the 2^256 pre-scaling it applies to arguments below 2^-767; zeros and +inf pass through,
// negative arguments and NaN give NaN. Bit-identical to sqrt() for x >= 2^-767.
// bl_hypot_g: bl_hypot() of blmath.h - same operations in the same order - without its range
// scaling and its infinity tests: bit-identical for finite arguments with max <= 2^510 and
// min >= 2^-450 (or zero); NaN in, NaN out. Host builds call the general functions.
BL_HD double bl_sqrt_g(double x) { return blm_sqrt_n(x); }
BL_HD double bl_hypot_g(double x, double y) {
#if defined(__HIP_DEVICE_COMPILE__)
  double ax = blm_abs(x), ay = blm_abs(y);
  const bool swap = ax < ay;
  const double big = swap ? ay : ax, small = swap ? ax : ay;
  double p = big * big, pe = __builtin_fma(big, big, -p);
  double q = small * small, qe = __builtin_fma(small, small, -q);
  double hi = p + q;
  double lo = (q - (hi - p)) + (pe + qe);
  double h = bl_sqrt_g(hi);
  double r = __builtin_fma(-h, h, hi) + lo;
  h = h + bl_div_g(r, h + h);
  return (small == 0.0 || small < big * 0x1p-54) ? big : h;
#else
  return bl_hypot(x, y);
#endif
}

struct BlSpacetime {
  double bh_m;
  double bh_a;
  int ray_flat;
};

// Scalars shared by all metric functions (geodesic_geometry.cpp:63-73, :131-141, :187-197)
struct BlKerrSchild {
  double r2, r, f;
  double l[3];    // l_1, l_2, l_3 (same for the covariant and contravariant null vector)
  double fl[3];   // f * l_i
  double a2, rr2;
};
// Reciprocals of the two denominators that the metric shares with its derivatives
struct BlKerrSchildRecip {
  BlRecip r, ra;  // 1 / r, 1 / (r^2 + a^2)
};

// ---- zero spin -------------------------------------------------------------------------------------
// kSpinZero instantiations (selected by the host when bh_a == 0.0, which the benchmark and every a = 0 input use)
// drop the operations whose result is fixed by a = 0. Bit-identical to the general code evaluated at a = 0:
//   a^2 = 0 * 0 = +0, and every product with it (a^2 z, a^2 z^2, 2 a z, a x, a y, 2 a^2 r z) is +-0 for the finite
//   coordinates of a ray; x + (+-0) = x and x - (+-0) = x for x != 0 (the reference is built with
//   -fno-signed-zeros, so the sign of a zero sum is not part of its contract either);
//   hypot(R^2 - 0, +-0) = |R^2| = R^2 (bl_hypot_g returns the larger argument when the smaller is zero), so
//   r^2 = 0.5 * (R^2 + R^2) = R^2 exactly, and 2 r^2 - R^2 + 0 = r^2 exactly: the denominators 2 r^2 - R^2 + a^2 and
//   r^2 + a^2 of geodesic_geometry.cpp:199-214 are both r^2 and share one reciprocal;
//   quotients keep their operands: f = (2 m r^2 r) / (r^2 r^2), l_1 = (r x) / r^2 - not 2 m / r, x / r.
// tests/test_gpu_math.py compares both instantiations on random points through bl_debug_geometry.

// geodesic_geometry.cpp:19-26; bl_radial_coordinate2 also returns r^2
template <bool kSpinZero = false>
BL_HD double bl_radial_coordinate2(const BlSpacetime &st, double x, double y, double z, double *r2_out) {
  double rr2 = x * x + y * y + z * z;
  if (kSpinZero) {
    *r2_out = rr2;
    return bl_sqrt_g(rr2);
  }
  double a2 = st.bh_a * st.bh_a;
  double r2 = 0.5 * (rr2 - a2 + bl_hypot_g(rr2 - a2, 2.0 * st.bh_a * z));
  *r2_out = r2;
  return bl_sqrt_g(r2);
}
template <bool kSpinZero = false>
BL_HD double bl_radial_coordinate(const BlSpacetime &st, double x, double y, double z) {
  double r2;
  return bl_radial_coordinate2<kSpinZero>(st, x, y, z, &r2);
}

// The Kerr-Schild scalars given r^2 = the value bl_radial_coordinate2() returned for the same point
template <bool kSpinZero = false>
BL_HD void bl_kerr_schild_r2(const BlSpacetime &st, double x, double y, double z, double r2, BlKerrSchild *ks,
                             BlKerrSchildRecip *rc) {
  double bh_a = st.bh_a;
  double a2 = kSpinZero ? 0.0 : bh_a * bh_a;
  double rr2 = x * x + y * y + z * z;
  double r = bl_sqrt_g(r2);
  double f = kSpinZero ? bl_div_g(2.0 * st.bh_m * r2 * r, r2 * r2) : bl_div_g(2.0 * st.bh_m * r2 * r, r2 * r2 + a2 * z * z);
  rc->r = bl_recip(r);
  rc->ra = kSpinZero ? bl_recip(r2) : bl_recip(r2 + a2);
  ks->a2 = a2;
  ks->rr2 = rr2;
  ks->r2 = r2;
  ks->r = r;
  ks->f = f;
  ks->l[0] = kSpinZero ? bl_div_r(r * x, rc->ra) : bl_div_r(r * x + bh_a * y, rc->ra);
  ks->l[1] = kSpinZero ? bl_div_r(r * y, rc->ra) : bl_div_r(r * y - bh_a * x, rc->ra);
  ks->l[2] = bl_div_r(z, rc->r);
  for (int i = 0; i < 3; i++) ks->fl[i] = f * ks->l[i];
}
template <bool kSpinZero = false>
BL_HD void bl_kerr_schild_r(const BlSpacetime &st, double x, double y, double z, BlKerrSchild *ks,
                            BlKerrSchildRecip *rc) {
  double rr2 = x * x + y * y + z * z;
  if (kSpinZero) {
    bl_kerr_schild_r2<true>(st, x, y, z, rr2, ks, rc);
    return;
  }
  double a2 = st.bh_a * st.bh_a;
  double r2 = 0.5 * (rr2 - a2 + bl_hypot_g(rr2 - a2, 2.0 * st.bh_a * z));
  bl_kerr_schild_r2<false>(st, x, y, z, r2, ks, rc);
}
template <bool kSpinZero = false>
BL_HD void bl_kerr_schild(const BlSpacetime &st, double x, double y, double z, BlKerrSchild *ks) {
  BlKerrSchildRecip rc;
  bl_kerr_schild_r<kSpinZero>(st, x, y, z, ks, &rc);
}

// Full covariant metric g_{mu nu} (geodesic_geometry.cpp:38-93). Used by the camera set-up and
// by the coefficient kernels where all 16 components are contracted.
BL_HD void bl_gcov(const BlSpacetime &st, double x, double y, double z, double g[4][4]) {
  if (st.ray_flat) {
    for (int mu = 0; mu < 4; mu++)
      for (int nu = 0; nu < 4; nu++) g[mu][nu] = mu == nu ? (mu == 0 ? -1.0 : 1.0) : 0.0;
    return;
  }
  BlKerrSchild ks;
  bl_kerr_schild(st, x, y, z, &ks);
  g[0][0] = ks.f - 1.0;                       // f * l_0 * l_0 - 1, l_0 = 1
  for (int i = 0; i < 3; i++) {
    g[0][i + 1] = ks.fl[i];                   // f * l_0 * l_i
    g[i + 1][0] = ks.fl[i];                   // f * l_i * l_0
    for (int j = 0; j < 3; j++) g[i + 1][j + 1] = ks.fl[i] * ks.l[j];
    g[i + 1][i + 1] = ks.fl[i] * ks.l[i] + 1.0;
  }
}

// Full contravariant metric g^{mu nu} (geodesic_geometry.cpp:105-161), l^0 = -1
BL_HD void bl_gcon(const BlSpacetime &st, double x, double y, double z, double g[4][4]) {
  if (st.ray_flat) {
    for (int mu = 0; mu < 4; mu++)
      for (int nu = 0; nu < 4; nu++) g[mu][nu] = mu == nu ? (mu == 0 ? -1.0 : 1.0) : 0.0;
    return;
  }
  BlKerrSchild ks;
  bl_kerr_schild(st, x, y, z, &ks);
  g[0][0] = -ks.f - 1.0;                      // -f * l0 * l0 - 1
  for (int i = 0; i < 3; i++) {
    g[0][i + 1] = ks.fl[i];                   // -f * l0 * l_i = f * l_i
    g[i + 1][0] = ks.fl[i];                   // -f * l_i * l0
    for (int j = 0; j < 3; j++) g[i + 1][j + 1] = -(ks.fl[i] * ks.l[j]);
    g[i + 1][i + 1] = -(ks.fl[i] * ks.l[i]) + 1.0;
  }
}

// Metric components from already-computed Kerr-Schild scalars (same values as bl_gcov / bl_gcon;
// lets a caller evaluate bl_kerr_schild once per point instead of once per tensor).
BL_HD void bl_gcov_ks(const BlKerrSchild &ks, double g[4][4]) {
  g[0][0] = ks.f - 1.0;
  for (int i = 0; i < 3; i++) {
    g[0][i + 1] = ks.fl[i];
    g[i + 1][0] = ks.fl[i];
    for (int j = 0; j < 3; j++) g[i + 1][j + 1] = ks.fl[i] * ks.l[j];
    g[i + 1][i + 1] = ks.fl[i] * ks.l[i] + 1.0;
  }
}
BL_HD void bl_gcon_ks(const BlKerrSchild &ks, double g[4][4]) {
  g[0][0] = -ks.f - 1.0;
  for (int i = 0; i < 3; i++) {
    g[0][i + 1] = ks.fl[i];
    g[i + 1][0] = ks.fl[i];
    for (int j = 0; j < 3; j++) g[i + 1][j + 1] = -(ks.fl[i] * ks.l[j]);
    g[i + 1][i + 1] = -(ks.fl[i] * ks.l[i]) + 1.0;
  }
}
BL_HD void bl_minkowski(double g[4][4]) {
  for (int mu = 0; mu < 4; mu++)
    for (int nu = 0; nu < 4; nu++) g[mu][nu] = mu == nu ? (mu == 0 ? -1.0 : 1.0) : 0.0;
}

// bl_renormalization_factor with the contravariant metric supplied by the caller
BL_HD double bl_renormalization_factor_g(const double gcon[4][4], double k0, double k1, double k2, double k3) {
  double k[4] = {k0, k1, k2, k3};
  double temp_a = 0.0;
  for (int a = 1; a < 4; a++)
    for (int b = 1; b < 4; b++) temp_a += gcon[a][b] * k[a] * k[b];
  double temp_b = 0.0;
  for (int a = 1; a < 4; a++) temp_b += 2.0 * gcon[0][a] * k[0] * k[a];
  double temp_c = gcon[0][0] * k[0] * k[0];
  double temp_d = bl_sqrt_g(temp_b * temp_b - 4.0 * temp_a * temp_c);
  return temp_b < 0.0 ? bl_div_g(temp_d - temp_b, 2.0 * temp_a) : bl_div_g(-2.0 * temp_c, temp_b + temp_d);
}

// Null-condition renormalisation factor for the spatial covariant momentum
// (geodesics.cpp:296-309 and :352-371): solves g^{mu nu} k_mu k_nu = 0 for a common factor on k_i.
template <bool kSpinZero = false>
BL_HD double bl_renormalization_factor(const BlSpacetime &st, double x, double y, double z,
                                       double k0, double k1, double k2, double k3) {
  double gcon[4][4];
  if (kSpinZero && !st.ray_flat) {
    BlKerrSchild ks;
    bl_kerr_schild<true>(st, x, y, z, &ks);
    bl_gcon_ks(ks, gcon);
  } else {
    bl_gcon(st, x, y, z, gcon);
  }
  double k[4] = {k0, k1, k2, k3};
  double temp_a = 0.0;
  for (int a = 1; a < 4; a++)
    for (int b = 1; b < 4; b++) temp_a += gcon[a][b] * k[a] * k[b];
  double temp_b = 0.0;
  for (int a = 1; a < 4; a++) temp_b += 2.0 * gcon[0][a] * k[0] * k[a];
  double temp_c = gcon[0][0] * k[0] * k[0];
  double temp_d = bl_sqrt_g(temp_b * temp_b - 4.0 * temp_a * temp_c);
  return temp_b < 0.0 ? bl_div_g(temp_d - temp_b, 2.0 * temp_a) : bl_div_g(-2.0 * temp_c, temp_b + temp_d);
}

// d k_a / d lambda = -1/2 d_a g^{mu nu} k_mu k_nu from the derivatives along x^a, df = d_a f and dl[i] = d_a l_{i+1}:
// k[4+a] -= 0.5 * dgcon[a-1][mu][nu] * y[4+mu] * y[4+nu], (mu, nu) row-major (geodesics.cpp:880-883), with
// dgcon[a][mu][nu] = -(df_a l_mu l_nu + f dl_mu,a l_nu + f l_mu dl_nu,a) (geodesic_geometry.cpp:223-274)
//   [0][0] = -df_a ; [0][j] = [j][0] = df_a l_j + f dl_j,a ; [i][j] as written.
// (One function for the kernel with a ray per lane, which calls it three times, and the one with a ray per quad of lanes,
// whose lanes call it once each: the same operations in the same order either way.)
BL_HD double bl_momentum_rhs(double df, const double dl[3], double f, const double l[3], const double fl[3], const double kcov[4]) {
  double dfl[3], fdl[3];
  for (int i = 0; i < 3; i++) {
    dfl[i] = df * l[i];
    fdl[i] = f * dl[i];
  }
  // Every term of the reference's sum carries the factor 0.5 as its first multiplication. Scaling
  // by a power of two commutes with rounding (nothing here is near the underflow threshold), so
  // summing the unscaled terms in the same order and halving once gives the same bits.
  double acc = 0.0;
  acc -= (-df) * kcov[0] * kcov[0];
  for (int j = 0; j < 3; j++) acc -= (dfl[j] + fdl[j]) * kcov[0] * kcov[j + 1];
  for (int i = 0; i < 3; i++) {
    acc -= (dfl[i] + fdl[i]) * kcov[i + 1] * kcov[0];
    for (int j = 0; j < 3; j++) {
      double dg = -(dfl[i] * l[j] + fdl[i] * l[j] + fl[i] * dl[j]);
      acc -= dg * kcov[i + 1] * kcov[j + 1];
    }
  }
  return 0.5 * acc;
}

// The proper-distance derivative (geodesics.cpp:884-891), in the two pieces the kernel with a ray per quad of lanes needs:
//   temp_a[a] += (gcon[a][mu] - gcon[0][a] * gcon[0][mu] / gcon[0][0]) * y[4+mu] (:884-887), from row a of g^{ij}
BL_HD double bl_distance_row(double g0a, const double gia[3], const double fl[3], double g00, const BlRecip &rc_g00, const double kcov[4]) {
  double acc = (g0a - bl_div_r(g0a * g00, rc_g00)) * kcov[0];
  for (int j = 0; j < 3; j++) acc += (gia[j] - bl_div_r(g0a * fl[j], rc_g00)) * kcov[j + 1];
  return acc;
}
//   k[8] += gcov[a][b] * temp_a[a] * temp_a[b] (:888-891); gcov[i][j] = (f l_i) l_j (+1 diag); k[8] = -sqrt of this
BL_HD double bl_distance_norm(const double fl[3], const double l[3], const double temp_a[3]) {
  double acc = 0.0;
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) {
      double gab = a == b ? fl[a] * l[b] + 1.0 : fl[a] * l[b];
      acc += gab * temp_a[a] * temp_a[b];
    }
  return acc;
}

// The same derivative in closed form. With g^{ij} = delta_ij - f l_i l_j, g^{0i} = f l_i, g^{00} = -(1 + f) the bracket of
// bl_distance_row is gamma^{aj} = delta_aj - l_a l_j f / (1 + f), the inverse of the spatial metric (its k_t column is identically
// zero), and bl_distance_norm contracts gamma_ab gamma^{ai} gamma^{bj} k_i k_j = gamma^{ij} k_i k_j:
//   d s / d lambda = -sqrt(k.k - (l.k)^2 f / (1 + f))
// for any spin, without the null condition. NOT the reference's bits: bl_distance_closed.h states how far the two may lie apart
// and where the stepper may use this one. No cancellation beyond a factor 1 + f: f / (1 + f) < 1 and (l.k)^2 <= (l.l) (k.k).
BL_HD double bl_distance_closed(double f, const double l[3], const double kcov[4]) {
  const double kk = kcov[1] * kcov[1] + kcov[2] * kcov[2] + kcov[3] * kcov[3];
  const double lk = l[0] * kcov[1] + l[1] * kcov[2] + l[2] * kcov[3];
  return -bl_sqrt_g(kk - lk * lk * bl_div_g(f, 1.0 + f));
}

// bl_geodesic_rhs's distance argument (kWithDistance only): the reference's operations, the closed form, or no *ds at all
enum { BL_DISTANCE_EXACT = 0, BL_DISTANCE_CLOSED = 1, BL_DISTANCE_NONE = 2 };

// Right-hand side of the geodesic equations (geodesics.cpp:867-893 with distance, :909-925
// without). State: pos = (x, y, z); kcov = (k_t, k_x, k_y, k_z).
//   dpos[0..3] = d(t, x, y, z)/d lambda = g^{mu nu} k_nu
//   dk[0..2]   = d(k_x, k_y, k_z)/d lambda = -1/2 d_i g^{mu nu} k_mu k_nu      (d k_t = 0)
//   *ds        = d s / d lambda (proper distance), only if kWithDistance; `distance` (BL_DISTANCE_*, uniform across a wave where a
//                kernel passes anything but the default) chooses the reference's operations or bl_distance_closed
// Returns r at the evaluation point through *r_out.
template <bool kWithDistance, bool kSpinZero = false>
BL_HD void bl_geodesic_rhs(const BlSpacetime &st, const double pos[3], const double kcov[4],
                           double dpos[4], double dk[3], double *ds, double *r_out, int distance = BL_DISTANCE_EXACT) {
  if (st.ray_flat) {
    // Minkowski: g = diag(-1,1,1,1), all derivatives zero (geodesic_geometry.cpp:41-60, :177-184)
    dpos[0] = -kcov[0];
    for (int i = 0; i < 3; i++) dpos[i + 1] = kcov[i + 1];
    // k[4+a] = 0 - 0.5*0*k*k ... stays (+-)0
    for (int i = 0; i < 3; i++) dk[i] = 0.0;
    if (kWithDistance) {
      // temp_a[a] = sum_mu (g^{a mu} - g^{0a} g^{0 mu}/g^{00}) k_mu = k_a ; k[8] = -sqrt(sum k_a^2)
      double acc = 0.0;
      for (int a = 1; a < 4; a++) acc += kcov[a] * kcov[a];
      *ds = -bl_sqrt_g(acc);
    }
    // RadialGeodesicCoordinate ignores ray_flat (geodesic_geometry.cpp:19-26)
    *r_out = bl_radial_coordinate<kSpinZero>(st, pos[0], pos[1], pos[2]);
    return;
  }
  double x = pos[0], y = pos[1], z = pos[2];
  double bh_a = st.bh_a;
  BlKerrSchild ks;
  BlKerrSchildRecip rc;
  bl_kerr_schild_r<kSpinZero>(st, x, y, z, &ks, &rc);
  double r = ks.r, r2 = ks.r2, f = ks.f, a2 = ks.a2, rr2 = ks.rr2;
  const double *l = ks.l;
  const double *fl = ks.fl;
  *r_out = r;

  // g^{mu nu} rows needed below. gcon[0][0] = -f - 1; gcon[0][i] = gcon[i][0] = f l_i;
  // gcon[i][j] = -(f l_i) l_j (+1 on the diagonal)
  double g00 = -f - 1.0;
  double gij[3][3];
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) gij[i][j] = -(fl[i] * l[j]);
    gij[i][i] = -(fl[i] * l[i]) + 1.0;
  }

  // k[mu] += gcon[mu][nu] * y[4+nu], nu = 0..3 in order, starting from 0 (:877-879)
  {
    double acc = g00 * kcov[0];
    for (int j = 0; j < 3; j++) acc += fl[j] * kcov[j + 1];
    dpos[0] = acc;
    for (int i = 0; i < 3; i++) {
      double a = fl[i] * kcov[0];
      for (int j = 0; j < 3; j++) a += gij[i][j] * kcov[j + 1];
      dpos[i + 1] = a;
    }
  }

  // Scalar and vector derivatives (geodesic_geometry.cpp:199-220)
  double dr[3], df[3], dl[3][3];  // dl[i][a] = d l_{i+1} / d x^a
  // all quotients below are over four denominators (denom, den_f, r^2 + a^2, r), each inverted once
  if (kSpinZero) {
    // 2 r^2 - R^2 + a^2 = r^2 = r^2 + a^2 exactly (see "zero spin" above): one reciprocal serves both
    const BlRecip &rc_denom = rc.ra;
    dr[0] = bl_div_r(r * x, rc_denom);
    dr[1] = bl_div_r(r * y, rc_denom);
    dr[2] = bl_div_r(r * z, rc_denom);
    double num_f = r2 * r2;
    const BlRecip rc_den_f = bl_recip(r * (r2 * r2));
    df[0] = bl_div_r(-num_f * dr[0], rc_den_f) * f;
    df[1] = bl_div_r(-num_f * dr[1], rc_den_f) * f;
    df[2] = bl_div_r(-(num_f * dr[2]), rc_den_f) * f;
    double xl = x - 2.0 * r * l[0];
    double yl = y - 2.0 * r * l[1];
    dl[0][0] = bl_div_r(xl * dr[0] + r, rc.ra);
    dl[0][1] = bl_div_r(xl * dr[1], rc.ra);
    dl[0][2] = bl_div_r(xl * dr[2], rc.ra);
    dl[1][0] = bl_div_r(yl * dr[0], rc.ra);
    dl[1][1] = bl_div_r(yl * dr[1] + r, rc.ra);
    dl[1][2] = bl_div_r(yl * dr[2], rc.ra);
    double mz_r2 = bl_div_r(-z, rc.ra);   // -z / r^2
    dl[2][0] = mz_r2 * dr[0];
    dl[2][1] = mz_r2 * dr[1];
    dl[2][2] = mz_r2 * dr[2] + bl_div_r(1.0, rc.r);
  } else {
    const BlRecip rc_denom = bl_recip(2.0 * r2 - rr2 + a2);
    dr[0] = bl_div_r(r * x, rc_denom);
    dr[1] = bl_div_r(r * y, rc_denom);
    dr[2] = bl_div_r(r * z + bl_div_r(a2 * z, rc.r), rc_denom);
    double num_f = r2 * r2 - 3.0 * a2 * z * z;
    const BlRecip rc_den_f = bl_recip(r * (r2 * r2 + a2 * z * z));
    df[0] = bl_div_r(-num_f * dr[0], rc_den_f) * f;
    df[1] = bl_div_r(-num_f * dr[1], rc_den_f) * f;
    df[2] = bl_div_r(-(num_f * dr[2] + 2.0 * a2 * r * z), rc_den_f) * f;
    double xl = x - 2.0 * r * l[0];
    double yl = y - 2.0 * r * l[1];
    dl[0][0] = bl_div_r(xl * dr[0] + r, rc.ra);
    dl[0][1] = bl_div_r(xl * dr[1] + bh_a, rc.ra);
    dl[0][2] = bl_div_r(xl * dr[2], rc.ra);
    dl[1][0] = bl_div_r(yl * dr[0] - bh_a, rc.ra);
    dl[1][1] = bl_div_r(yl * dr[1] + r, rc.ra);
    dl[1][2] = bl_div_r(yl * dr[2], rc.ra);
    double mz_r2 = bl_div_g(-z, r2);
    dl[2][0] = mz_r2 * dr[0];
    dl[2][1] = mz_r2 * dr[1];
    dl[2][2] = mz_r2 * dr[2] + bl_div_r(1.0, rc.r);
  }

  for (int a = 0; a < 3; a++) {
    const double dla[3] = {dl[0][a], dl[1][a], dl[2][a]};
    dk[a] = bl_momentum_rhs(df[a], dla, f, l, fl, kcov);
  }

  if (kWithDistance) {
    if (distance == BL_DISTANCE_EXACT) {
      double temp_a[3];
      const BlRecip rc_g00 = bl_recip(g00);   // twelve quotients over g^{00}
      for (int a = 0; a < 3; a++) temp_a[a] = bl_distance_row(fl[a], gij[a], fl, g00, rc_g00, kcov);
      const double acc = bl_distance_norm(fl, l, temp_a);
      *ds = -bl_sqrt_g(acc);
    } else if (distance == BL_DISTANCE_CLOSED) {
      *ds = bl_distance_closed(f, l, kcov);
    }
  }
}

#endif  // BLACKLIGHT_AMD_BL_GEOMETRY_H_
