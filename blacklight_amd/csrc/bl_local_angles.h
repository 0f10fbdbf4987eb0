/* bl_local_angles.h - theta and phi of a sample relative to the centre of a guessed cell (tolerant tier, the locate step of
 * bl_shade_fused2_kernel over one block; bl_debug_math ops 40 and 41 run the same functions on given points).
 *
 * What the locate step takes from an angle is a cell, the signed distances to that cell's faces and centre (compared with
 * fast_angle_band = 1e-12) and the interpolation fraction. All of them are functions of d = angle - centre of the cell, which is
 * small, and d needs neither an arccosine nor an arctangent to 1e-16:
 *
 *   cos theta = z / r,  sin theta = sqrt((1 - |cos theta|) (1 + |cos theta|))
 *   phi = atan2(y, x) - atan2(a, r):  sin phi = (y r - x a) / (rho R),  cos phi = (x r + y a) / (rho R)
 *                                     (rho^2 = x^2 + y^2, R^2 = r^2 + a^2: x^2 + y^2 = R^2 sin^2 theta)
 *   sin(d) = sin(angle) cos(centre) - cos(angle) sin(centre),   d = asin(sin d) by its series through s^9
 *
 * with the centre's cosine and sine from a table (BlGridDevice::angle_trig, made once on the host). The cell itself is guessed in
 * single precision from the same four numbers; a guess that is off by a cell shows as a negative face margin and the sample goes to
 * the exact pass like every other undecided one.
 *
 * theta is the exact tier's theta = acos(z / r) of the ROUNDED r, not the true polar angle (rho / R would give that one): the two
 * differ by (relative error of z / r) x cot theta, which passes the band below theta = 1e-3. So cos theta is the correctly rounded
 * quotient, as on the global path, and the sine is taken from it - 1 - |cos theta| is exact from 1 / 2 on, as inside an arccosine.
 *
 * Rounding bound of d (kAngleOffsetError, what tests/test_gpu_local_angles.py holds the fraction to, times 1 / width):
 *   8e-16   two reciprocal square roots of one Newton step (4e-16 each: rsqrt1), one in sin theta, one in both of sin / cos phi
 *   1e-15   in phi: r, which is the exact tier's (correctly rounded root of a sum of a few rounded terms: at most 9 units of 1.1e-16)
 *   9e-16   eight roundings of the products, the table's two entries (below one unit each) among them
 *   1.3e-15 the series' first omitted term, 945 / 42240 s^11, at |d| = 1 / 16 - the plan takes this path only where no point of an
 *           angular cell is further than that from the cell's centre (kLocalAngleReach, BlGridDevice::angle_reach)
 * together 4e-15, 250 times below the band.
 *
 * On the polar axis rho = 0 and phi's sine and cosine are NaN, and so are d and its margin: the caller's comparisons leave such a
 * sample undecided (with spin the exact tier's theta is not even zero there: r is a rounding error above |z|).
 *
 * Device only; to be included inside a `#pragma clang fp contract(fast)` region, after bl_fastmath.h. */
#ifndef BLACKLIGHT_AMD_BL_LOCAL_ANGLES_H_
#define BLACKLIGHT_AMD_BL_LOCAL_ANGLES_H_

#include <stdint.h>

#include "bl_fastmath.h"

namespace local_angles {

constexpr double kAngleOffsetError = 4.0e-15;   // the bound above

// One angular cell as the search wants it (LDS, 64 bytes: the size of fused2::AxisRow, whose place in the tables it takes)
struct alignas(16) AngleRow {
  double cos_c, sin_c;          // of the cell's centre xv[c]
  double lo, hi;                // faces relative to the centre: xf[c] - xv[c] < 0 < xf[c + 1] - xv[c] (make_row)
  double inv_w_ge, inv_w_lt;    // 1 / (distance between the anchor's centre and the next) when d >= 0 / when d < 0
  uint32_t shift_ge, shift_lt;  // anchor = c - shift and fraction = d * inv_w + shift: (0, 1), (1, 1) in the last cell, (0, 0) in the first
  uint32_t unused[2];
};
static_assert(sizeof(AngleRow) == 64, "angle row must be 64 bytes");

// Row c of an axis of n cells from its faces and centres and the cosine and sine of xv[c]. `turn`: where the angle's range ends (pi for
// theta, 2 pi for phi). The exact tier's angles lie in [0, turn] - its phi is wrapped there - so an outer face beyond that range (the
// mock's last faces are pi and 2 pi rounded up to single precision) gives way to the end of the range: the seam of phi at 0 / 2 pi is
// then the outer face of the first and of the last phi cell.
__device__ __forceinline__ AngleRow make_row(const double *xf, const double *xv, double cos_c, double sin_c, int c, int n, double turn) {
  const int c_ge = c == n - 1 ? c - 1 : c, c_lt = c == 0 ? 0 : c - 1;
  AngleRow row;
  row.cos_c = cos_c;
  row.sin_c = sin_c;
  row.lo = (xf[c] > 0.0 ? xf[c] : 0.0) - xv[c];
  row.hi = (xf[c + 1] < turn ? xf[c + 1] : turn) - xv[c];
  row.inv_w_ge = 1.0 / (xv[c_ge + 1] - xv[c_ge]);
  row.inv_w_lt = 1.0 / (xv[c_lt + 1] - xv[c_lt]);
  row.shift_ge = (uint32_t)(c - c_ge);
  row.shift_lt = (uint32_t)(c - c_lt);
  row.unused[0] = row.unused[1] = 0u;
  return row;
}

// 1 / sqrt(x) for finite x > 0: v_rsq_f64 and one Newton step, 4e-16
__device__ __forceinline__ double rsqrt1(double x) {
  const double y = __builtin_amdgcn_rsq(x);
  const double e = __builtin_fma(-0.5 * x * y, y, 0.5);
  return __builtin_fma(y, e, y);
}

// Cosine and sine of a sample's theta and phi (r: the exact tier's radius, r_inv its reciprocal to 2e-16)
struct Direction {
  double cos_th, sin_th, cos_ph, sin_ph;
};
// (phi's half alone: with zero spin it takes nothing but x and y, and under y -> -y its cosine keeps its bits and its sine changes
// the sign bit - rho2's y * y does not see the sign, and neither does the rounding of y * rho_inv)
template <bool kSpinZero>
__device__ __forceinline__ void direction_phi(double a, double r, double x, double y, double *sin_ph, double *cos_ph) {
  const double rho2 = __builtin_fma(x, x, y * y);
  if (kSpinZero) {
    const double rho_inv = rsqrt1(rho2);
    *sin_ph = y * rho_inv;
    *cos_ph = x * rho_inv;
  } else {
    const double q = rsqrt1(rho2 * __builtin_fma(r, r, a * a));
    *sin_ph = __builtin_fma(y, r, -(x * a)) * q;
    *cos_ph = __builtin_fma(x, r, y * a) * q;
  }
}
template <bool kSpinZero>
__device__ __forceinline__ Direction direction(double a, double r, double r_inv, double x, double y, double z) {
  Direction u;
  // (the product with the reciprocal, corrected once by its residual, is the correctly rounded quotient - the exact tier's argument of
  // its arccosine bit for bit - in all but a few cases in a million)
  double c = z * r_inv;
  c = __builtin_fma(__builtin_fma(-r, c, z), r_inv, c);
  u.cos_th = c;
  const double ac = __builtin_fabs(c);
  const double w = __builtin_fmax((1.0 - ac) * (1.0 + ac), 0x1p-1000);   // (on the axis: theta = 1e-151, closer to the face than any band)
  u.sin_th = w * rsqrt1(w);
  direction_phi<kSpinZero>(a, r, x, y, &u.sin_ph, &u.cos_ph);
  return u;
}

// atan2(s, c) of a unit vector in single precision, 4e-7 (polynomial 3e-7, rounding): [0, pi] for s >= 0, else (with kFullTurn)
// in (pi, 2 pi)
template <bool kFullTurn>
__device__ __forceinline__ float angle_guess(float s, float c) {
  const float as = __builtin_fabsf(s), ac = __builtin_fabsf(c);
  const float mx = as > ac ? as : ac, mn = as > ac ? ac : as;
  const float u = mn * __builtin_amdgcn_rcpf(mx), w = u * u;
  float p = __builtin_fmaf(0x1.be6a4p-8f, w, -0x1.1348e4p-5f);
  p = __builtin_fmaf(p, w, 0x1.46234ep-4f);
  p = __builtin_fmaf(p, w, -0x1.0f04c6p-3f);
  p = __builtin_fmaf(p, w, 0x1.95a9fcp-3f);
  p = __builtin_fmaf(p, w, -0x1.552b7cp-2f);
  p = __builtin_fmaf(p, w, 0x1.ffff7ep-1f);
  float t = p * u;                                  // atan(mn / mx)
  t = as > ac ? 0x1.921fb6p+0f - t : t;
  t = c < 0.0f ? 0x1.921fb6p+1f - t : t;
  if (kFullTurn) t = s < 0.0f ? 0x1.921fb6p+2f - t : t;
  return t;
}

// d = asin(s) for |s| <= sin(1 / 16): s + s^3 / 6 + 3 s^5 / 40 + 15 s^7 / 336 + 105 s^9 / 3456
__device__ __forceinline__ double small_asin(double s) {
  const double w = s * s;
  double q = fastmath::add_k(w * BLM_K(105.0 / 3456.0), 15.0 / 336.0);
  q = fastmath::fma_k(q, w, 3.0 / 40.0);
  q = fastmath::fma_k(q, w, 1.0 / 6.0);
  return __builtin_fma(s * w, q, s);
}
__device__ __forceinline__ double offset_from_centre(double sin_angle, double cos_angle, double cos_c, double sin_c) {
  return small_asin(__builtin_fma(sin_angle, cos_c, -(cos_angle * sin_c)));
}

// One axis from d and the guessed cell's row: anchor shift, fraction, smallest of the signed distances to the faces (negative: the
// guess is wrong) and the distance to the centre
__device__ __forceinline__ void lookup(const AngleRow &row, double d, double *frac, uint32_t *shift, double *margin) {
  const bool ge = d >= 0.0;
  *shift = ge ? row.shift_ge : row.shift_lt;
  *frac = __builtin_fma(d, ge ? row.inv_w_ge : row.inv_w_lt, (double)*shift);
  *margin = __builtin_fmin(__builtin_fmin(d - row.lo, row.hi - d), __builtin_fabs(d));   // (NaN for a NaN d: all three are)
}

}  // namespace local_angles

#endif  // BLACKLIGHT_AMD_BL_LOCAL_ANGLES_H_
