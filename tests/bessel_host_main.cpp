// bl_bessel.h's claim, on the host: bl_cyl_bessel_k(n, x) is libstdc++'s std::cyl_bessel_k(n, x) operation for operation. The pinned
// math library's object (oracle/blmath_preload.c) is linked into this program, so that libstdc++'s template runs over the same log, exp,
// cosh and sinh as the header; built without builtins and without contraction (oracle/Makefile, bessel_check). Prints the number of
// arguments tried and of (n, x) pairs whose bits differ; tests/test_blmath.py asserts 0.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "bl_bessel.h"

static uint64_t bits(double v) {
  uint64_t u;
  std::memcpy(&u, &v, sizeof u);
  return u;
}

int main() {
  std::mt19937_64 engine(20261020);
  auto uniform = [&](double lo, double hi) { return lo + (hi - lo) * (static_cast<double>(engine() >> 11) * 0x1p-53); };
  std::vector<double> xs;
  const double lo = -300.0, hi = std::log10(745.0);   // (libstdc++ itself throws below: 2 n / x overflows, and for subnormal x)
  for (int i = 0; i < 150000; i++) xs.push_back(std::pow(10.0, uniform(lo, hi)));
  for (int i = 0; i < 100000; i++) xs.push_back(std::pow(10.0, uniform(-6.0, std::log10(500.0))));
  for (int i = 0; i < 100000; i++) xs.push_back(1.0 / std::pow(10.0, uniform(-2.0, 4.0)));   // 1 / Theta_e, Theta_e in [0.01, 1e4]
  for (int i = 0; i < 50000; i++) xs.push_back(uniform(1.9, 2.1));                           // the series / continued-fraction switch
  double below = 2.0, above = 2.0;
  xs.push_back(2.0);
  for (int i = 0; i < 64; i++) {
    below = std::nextafter(below, 0.0);
    above = std::nextafter(above, 3.0);
    xs.push_back(below);
    xs.push_back(above);
  }
  for (double x : {1.0e-300, 0.01, 100.0, 1.0e-4, 500.0, 700.0, 745.0, 0.0, std::numeric_limits<double>::quiet_NaN()}) xs.push_back(x);
  long mismatches = 0;
  for (double x : xs)
    for (int n = 0; n <= 2; n++) {
      const double want = std::cyl_bessel_k(static_cast<double>(n), x);
      const double got = bl_cyl_bessel_k(n, x);
      if (bits(want) != bits(got) && !(want != want && got != got)) {
        if (mismatches < 5) std::printf("K_%d(%.17g): std %.17g, bl %.17g\n", n, x, want, got);
        mismatches++;
      }
    }
  double k0, k1, k2;   // ... and one k012 call is the three single calls
  for (double x : xs) {
    bl_cyl_bessel_k012(x, &k0, &k1, &k2);
    const double single[3] = {bl_cyl_bessel_k(0, x), bl_cyl_bessel_k(1, x), bl_cyl_bessel_k(2, x)};
    const double triple[3] = {k0, k1, k2};
    for (int n = 0; n <= 2; n++)
      if (bits(single[n]) != bits(triple[n]) && !(single[n] != single[n] && triple[n] != triple[n])) mismatches++;
  }
  std::printf("arguments %zu mismatches %ld\n", xs.size(), mismatches);
  return 0;
}
