// bl_harm.h - iharm3d-family primitives (prims[n1][n2][n3][n_prim]: internal energy, velocity and field components on the MKS / FMKS
// coordinate basis) to what the sampler reads (pressure, normal-frame velocity and lab-frame field on the spherical Kerr-Schild
// basis), written once for the file reader (ReadIharm3d, bl_snapshot.cpp), the host call (bl_harm_convert_host, bl_harm.cpp) and the
// staging kernel (bl_interleave_cells_kernel's harm form, bl_api.hip).
//   SimulationReader::ConvertPrimitives3                      src/simulation_reader/simulation_geometry.cpp:95-230
//   ::ConvertCoordinates, ::GenerateSKSMap, ::GetSKSCoordinates, ::SetJacobianFactors   :29-83, :321-483
//   ::Read (Harm header, VerifyVariablesHarm)                 src/simulation_reader/simulation_reader.cpp:354-428, :598-657, :1302-1413
// The conversion has two parts. What depends on the point (i, j) alone - r, theta, the Jacobian of the coordinate map, the metric on
// both bases - holds every elementary function; it is evaluated on the host, once per point, with the reader's operations in the
// reader's order (BlHarmPoint, bl_harm.cpp). What depends on the cell is IEEE add, multiply, divide and square root (bl_harm_cell,
// below): both builds have -ffp-contract=off, so the host loops and the kernel produce the same bits.
#ifndef BLACKLIGHT_AMD_BL_HARM_H_
#define BLACKLIGHT_AMD_BL_HARM_H_

#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../include/blacklight_amd.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define BL_HARM_FN static inline __host__ __device__
#else
#define BL_HARM_FN static inline
#endif

// One point (i, j) of the grid: the Jacobian dr/dx1, dtheta/dx1, dtheta/dx2, the covariant metric on the file's basis (g_01 ... g_33),
// the contravariant time row on it (g01 ... g03), the lapse on either basis and the contravariant time row of spherical Kerr-Schild.
// (Members that are zero for every Kerr-Schild point are kept: they meet the cell's values in products, where a zero and an infinity
// or a NaN make what the reader makes.)
struct BlHarmPoint {
  double dr_dx1, dth_dx1, dth_dx2;
  double g_01, g_02, g_03, g_11, g_12, g_13, g_22, g_23, g_33;
  double g01, g02, g03;
  double alpha, alpha_mod;
  double gtr, gtth, gtph;
};
enum { BL_HARM_POINT_DOUBLES = 20 };
static_assert(sizeof(BlHarmPoint) == BL_HARM_POINT_DOUBLES * sizeof(double), "BlHarmPoint is an array of doubles to the staging kernel");

// One cell (simulation_geometry.cpp:160-227): velocity uu1..3 and field bb1..3 as the file has them, rounded to float; out: the six
// values the reader stores, in that order. The operand order is the reference's.
BL_HARM_FN void bl_harm_cell(const BlHarmPoint &pt, const float in[6], float out[6]) {
#pragma clang fp contract(off)
  const double uu1 = in[0], uu2 = in[1], uu3 = in[2];
  const double bb1 = in[3], bb2 = in[4], bb3 = in[5];
  const double uu0 = sqrt(1.0 + pt.g_11 * uu1 * uu1 + 2.0 * pt.g_12 * uu1 * uu2 + 2.0 * pt.g_13 * uu1 * uu3 + pt.g_22 * uu2 * uu2
                          + 2.0 * pt.g_23 * uu2 * uu3 + pt.g_33 * uu3 * uu3);
  const double u0 = uu0 / pt.alpha_mod;
  const double u1 = uu1 - pt.alpha_mod * pt.g01 * uu0;
  const double u2 = uu2 - pt.alpha_mod * pt.g02 * uu0;
  const double u3 = uu3 - pt.alpha_mod * pt.g03 * uu0;
  const double u_1 = pt.g_01 * u0 + pt.g_11 * u1 + pt.g_12 * u2 + pt.g_13 * u3;
  const double u_2 = pt.g_02 * u0 + pt.g_12 * u1 + pt.g_22 * u2 + pt.g_23 * u3;
  const double u_3 = pt.g_03 * u0 + pt.g_13 * u1 + pt.g_23 * u2 + pt.g_33 * u3;
  const double ut = u0;
  const double ur = pt.dr_dx1 * u1;
  const double uth = pt.dth_dx1 * u1 + pt.dth_dx2 * u2;
  const double uph = u3;
  const double uur = ur + pt.alpha * pt.alpha * pt.gtr * ut;
  const double uuth = uth + pt.alpha * pt.alpha * pt.gtth * ut;
  const double uuph = uph + pt.alpha * pt.alpha * pt.gtph * ut;
  const double b0 = u_1 * bb1 + u_2 * bb2 + u_3 * bb3;
  const double b1 = (bb1 + b0 * u1) / u0;
  const double b2 = (bb2 + b0 * u2) / u0;
  const double b3 = (bb3 + b0 * u3) / u0;
  const double bt = b0;
  const double br = pt.dr_dx1 * b1;
  const double bth = pt.dth_dx1 * b1 + pt.dth_dx2 * b2;
  const double bph = b3;
  out[0] = static_cast<float>(uur);
  out[1] = static_cast<float>(uuth);
  out[2] = static_cast<float>(uuph);
  out[3] = static_cast<float>(br * ut - bt * ur);
  out[4] = static_cast<float>(bth * ut - bt * uth);
  out[5] = static_cast<float>(bph * ut - bt * uph);
}

// ------------------------------------------------------------------------------------------------ host only
// bl_harm_grid: what the reader makes of a header, kept for as many cell arrays as follow on the same geometry
struct bl_harm_grid {
  bl_params params{};
  bl_harm_header header{};
  std::vector<double> coords[6];     // x1f x2f x3f x1v x2v x3v as the sampler takes them (fmks: native; else r, theta, phi)
  std::vector<double> x2v_native;    // x^2 of the cell centres as the file has it
  double poly_norm = 0.0;            // FMKS: the derived normalisation of the polynomial term
  std::vector<double> sks_map;       // fmks: built when the description is first asked for (BuildSksMap)
  std::vector<BlHarmPoint> points;   // [n2][n1]
  std::vector<int32_t> levels, locations;
  bl_grid_desc desc{};               // prim = NULL; the header's variable indices
  bl_grid_desc converted{};          // ... and for planes in the internal order (bl_harm_convert_*): indices 0 ... 7 (8)
  std::string warnings;
  bool fmks = false, code_kappa = false, map_built = false;
  unsigned long long serial = 0;     // one per grid made in this process: what a context keys its copy of `points` by
};

namespace blharm {
struct Refusal {
  int code;
  std::string message;
};
// The steps of ReadIharm3d between its reads of the file, in its order; each throws Refusal with the reader's text.
void CheckMetric(bl_harm_grid *g);        // simulation_coord, the spin warning, fmks asked of an MKS header
void BuildCoordinates(bl_harm_grid *g);   // the counts, the six coordinate arrays and their conversion (fmks: bounds)
void CheckVariables(bl_harm_grid *g);     // the nine indices, the adiabatic indices; the description's scalars
void BuildSksMap(bl_harm_grid *g);        // fmks: the 2048 x 2048 look-up table (or the copy of the last one built from the same numbers)
void BuildPoints(bl_harm_grid *g);        // the point table
void FinishDescription(bl_harm_grid *g);  // the description's pointers
// prims [n1][n2][n3][n_prim] float -> planes [8 (9 with code_kappa)][n3][n2][n1] in the order rho, pgas, uu1..3, bb1..3 (, kappa)
void ConvertHost(const bl_harm_grid &g, const float *prims, float *out);
// The FMKS map (r, theta) of native (x1, x2) and its Jacobian
void SksCoordinates(const bl_harm_grid &g, double x1, double x2, double *r, double *theta);
}  // namespace blharm

#endif  // BLACKLIGHT_AMD_BL_HARM_H_
