// bl_harm.cpp - host side of bl_harm.h: from an iharm3d header to the grid the sampler takes (coordinates, FMKS look-up table and
// bounds, variable and adiabatic indices), the point table of the primitive conversion, and the conversion of a cell array on the
// host. No HIP call: everything here works on a machine without a device. ReadIharm3d (bl_snapshot.cpp) runs these steps between its
// reads of the file, bl_harm_grid_create runs them on a header the caller filled in; the texts are the reader's.
#include "bl_harm.h"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <sstream>
#include <thread>

#include "bl_internal.h"
#include "blmath.h"

namespace {
constexpr double kPi = 3.141592653589793;   // blacklight.hpp Math::pi

// The last FMKS look-up table built in this process and what it was built from
std::mutex g_sks_map_mutex;
std::vector<double> g_sks_map_key, g_sks_map;
std::atomic<unsigned long long> g_serial{0};

[[noreturn]] void Refuse(const char *message, int code = BL_E_INPUT) { throw blharm::Refusal{code, message}; }
void Warn(bl_harm_grid *g, const std::string &text) { g->warnings += "Warning: " + text + "\n"; }

// SimulationReader::SetJacobianFactors (simulation_geometry.cpp:451-483), FMKS branch
void FmksJacobian(const bl_harm_grid &g, double x1, double x2, double *dr_dx1, double *dth_dx1, double *dth_dx2) {
  const bl_harm_header &h = g.header;
  *dr_dx1 = bl_exp(x1);
  const double var_a = bl_exp(h.mks_smooth * (bl_log(h.r_in) - x1));
  const double var_b = kPi * (0.5 - x2);
  const double var_c = bl_pow((2.0 * x2 - 1.0) / h.poly_xt, h.poly_alpha);
  const double var_d = 1.0 + h.poly_alpha;
  const double var_e = g.poly_norm * (1.0 + var_c / var_d);
  const double var_f = var_e * (2.0 * x2 - 1.0);
  const double var_g = -0.5 * (1.0 - h.hslope) * bl_sin(2.0 * kPi * x2);
  *dth_dx1 = -h.mks_smooth * var_a * (var_b + var_f + var_g);
  const double var_h = kPi + (1.0 - h.hslope) * kPi * bl_cos(2.0 * kPi * x2);
  const double var_i = -kPi + 2.0 * var_e;
  const double var_j = 2.0 * g.poly_norm * h.poly_alpha * var_c / var_d;
  const double var_k = -(1.0 - h.hslope) * kPi * bl_cos(2.0 * kPi * x2);
  *dth_dx2 = var_h + var_a * (var_i + var_j + var_k);
}
}  // namespace

namespace blharm {

// SimulationReader::GetSKSCoordinates (simulation_geometry.cpp:427-443), FMKS branch
void SksCoordinates(const bl_harm_grid &g, double x1, double x2, double *r, double *theta) {
  const bl_harm_header &h = g.header;
  *r = bl_exp(x1);
  const double y = 2.0 * x2 - 1.0;
  const double theta_g = kPi * x2 + (1.0 - h.hslope) / 2.0 * bl_sin(2.0 * kPi * x2);
  const double theta_j = 0.5 * kPi + g.poly_norm * y * (1.0 + bl_pow(y / h.poly_xt, h.poly_alpha) / (h.poly_alpha + 1.0));
  *theta = theta_g + bl_exp(h.mks_smooth * (bl_log(h.r_in) - x1)) * (theta_j - theta_g);
}

void CheckMetric(bl_harm_grid *g) {
  const bl_params &p = g->params;
  const bl_harm_header &h = g->header;
  if (p.simulation_coord != BL_COORD_SKS && p.simulation_coord != BL_COORD_FMKS) Refuse("Invalid simulation_coord for Harm format.");
  if (h.a != p.simulation_a) {
    std::ostringstream message;
    message << "Given spin of " << p.simulation_a << " does not match file value of " << h.a << "; ignoring the latter.";
    Warn(g, message.str());
  }
  g->fmks = p.simulation_coord == BL_COORD_FMKS;
  g->code_kappa = p.plasma_model == BL_PLASMA_CODE_KAPPA;
  if (g->fmks && h.metric != BL_HARM_FMKS)   // the reference would build its map from uninitialised parameters
    Refuse("simulation_coord = fmks needs a file whose header/metric is FMKS or MMKS.", BL_E_UNSUPPORTED);
}

// coordinates (simulation_reader.cpp:622-656) and their conversion to r, theta (simulation_geometry.cpp:36-81)
void BuildCoordinates(bl_harm_grid *g) {
  const bl_harm_header &h = g->header;
  g->poly_norm = 0.0;
  if (h.metric == BL_HARM_FMKS) {   // (simulation_reader.cpp:396-427)
    g->poly_norm = (h.poly_alpha + 1.0) * bl_pow(h.poly_xt, h.poly_alpha);
    g->poly_norm = 0.5 * kPi * g->poly_norm / (g->poly_norm + 1.0);
  }
  const long n[3] = {h.n1, h.n2, h.n3};
  for (int a = 0; a < 3; a++) {
    if (n[a] < 1 || n[a] > 65536) Refuse("Array dimension mismatch.");
    const double start = h.startx[a], dx = h.dx[a];
    std::vector<double> &xf = g->coords[a], &xv = g->coords[3 + a];
    xf.assign(n[a] + 1, 0.0);
    xv.assign(n[a], 0.0);
    xf[0] = start;
    for (long i = 0; i < n[a]; i++) {
      xf[i + 1] = start + static_cast<double>(i + 1) * dx;
      xv[i] = 0.5 * (xf[i] + xf[i + 1]);
    }
  }
  g->x2v_native = g->coords[4];
  bl_grid_desc &gd = g->desc;
  if (g->fmks) {
    // the coordinates stay native; the map from (r, theta) to (x^1, x^2) (BuildSksMap) and the grid's bounds in (r, theta, phi)
    // are what the sampler works with
    const int map_n1 = 2048, map_n2 = 2048;
    const double r_in = bl_exp(g->coords[0][0]), r_out = bl_exp(g->coords[0][n[0]]);
    gd.sks_map = nullptr;
    gd.sks_map_n1 = map_n1;
    gd.sks_map_n2 = map_n2;
    gd.sks_map_r_in = r_in;
    gd.sks_map_dr = (r_out - r_in) / (map_n1 - 1);
    gd.sks_map_dtheta = kPi / (map_n2 - 1);
    double r_val, theta_val;
    SksCoordinates(*g, g->coords[0][0], 0.0, &r_val, &theta_val);
    gd.simulation_bounds[0] = r_val;
    gd.simulation_bounds[2] = theta_val;
    gd.simulation_bounds[4] = 0.0;
    SksCoordinates(*g, g->coords[0][n[0]], 1.0, &r_val, &theta_val);
    gd.simulation_bounds[1] = r_val;
    gd.simulation_bounds[3] = theta_val;
    gd.simulation_bounds[5] = 2.0 * kPi;
  } else {
    for (double &x : g->coords[0]) x = bl_exp(x);
    for (double &x : g->coords[3]) x = bl_exp(x);
    for (double &x : g->coords[1]) x = kPi * x + (1.0 - h.hslope) / 2.0 * bl_sin(2.0 * kPi * x);
    for (double &x : g->coords[4]) x = kPi * x + (1.0 - h.hslope) / 2.0 * bl_sin(2.0 * kPi * x);
  }
}

// GenerateSKSMap (simulation_geometry.cpp:321-419): 2048 x 2048 points, x^2 by bisection on theta(x^1, x^2) to 1e-8.
// (The files of a series share their geometry - slow light opens a window of them - and the map is 4 million bisections: the last map
// built in this process is kept with everything it was built from, and copied when those numbers come again.)
void BuildSksMap(bl_harm_grid *g) {
  if (!g->fmks || g->map_built) return;
  const bl_harm_header &h = g->header;
  bl_grid_desc &gd = g->desc;
  const int map_n1 = gd.sks_map_n1, map_n2 = gd.sks_map_n2, max_iter = 1000;
  const double tol = 1.0e-8;
  const double r_in = gd.sks_map_r_in, r_out = bl_exp(g->coords[0][h.n1]);
  const double dr = gd.sks_map_dr, dtheta = gd.sks_map_dtheta;
  const std::vector<double> map_key = {r_in, r_out, h.hslope, h.r_in, h.poly_xt, h.poly_alpha, h.mks_smooth};
  bool map_cached = false;
  {
    std::lock_guard<std::mutex> lock(g_sks_map_mutex);
    if (g_sks_map_key == map_key && !g_sks_map.empty()) {
      g->sks_map = g_sks_map;
      map_cached = true;
    }
  }
  if (!map_cached) g->sks_map.assign(static_cast<size_t>(2) * map_n2 * map_n1, 0.0);
  double *map_x1 = g->sks_map.data(), *map_x2 = g->sks_map.data() + static_cast<size_t>(map_n2) * map_n1;
  // (columns are independent: spread over the host's threads; the reference fills the map serially)
  auto fill_columns = [&](int i_begin, int i_end) {
    for (int i = i_begin; i < i_end; ++i) {
      const double r = r_in + i * dr;
      const double x1 = bl_log(r);
      for (int j = 0; j < map_n2; ++j) {
        const double theta = std::min(j * dtheta, kPi);
        double x2 = 0.5;
        if (theta > tol && std::abs(kPi - theta) > tol) {
          double x2_a = 0.0, x2_b = 1.0;
          x2 = (x2_b + x2_a) / 2.0;
          double temp_r, theta_a = 0.0, theta_b = kPi, theta_c = kPi / 2.0;
          SksCoordinates(*g, x1, x2_a, &temp_r, &theta_a);
          SksCoordinates(*g, x1, x2_b, &temp_r, &theta_b);
          for (int iter = 0; iter < max_iter; iter++) {
            SksCoordinates(*g, x1, x2, &temp_r, &theta_c);
            if ((theta_c - theta) * (theta_b - theta) < 0.0) {
              theta_a = theta_c;
              x2_a = x2;
            } else {
              theta_b = theta_c;
              x2_b = x2;
            }
            x2 = (x2_a + x2_b) / 2.0;
            if (std::abs(theta - theta_c) < tol) break;
          }
          (void)theta_a;
        } else if (theta < tol) {
          x2 = 0.0;
        } else if (theta > kPi - tol) {
          x2 = 1.0;
        }
        map_x1[static_cast<size_t>(j) * map_n1 + i] = x1;
        map_x2[static_cast<size_t>(j) * map_n1 + i] = x2;
      }
    }
  };
  if (!map_cached) {
    const int n_threads = std::max(1, std::min(64, static_cast<int>(std::thread::hardware_concurrency())));
    std::vector<std::thread> workers;
    for (int t = 0; t < n_threads; t++)
      workers.emplace_back(fill_columns, static_cast<int>(static_cast<long>(map_n1) * t / n_threads),
                           static_cast<int>(static_cast<long>(map_n1) * (t + 1) / n_threads));
    for (std::thread &w : workers) w.join();
    std::lock_guard<std::mutex> lock(g_sks_map_mutex);
    g_sks_map_key = map_key;
    g_sks_map = g->sks_map;
  }
  g->map_built = true;
  gd.sks_map = g->sks_map.data();
}

// VerifyVariablesHarm (simulation_reader.cpp:1302-1413): an index of -1 is a name the file does not have
void CheckVariables(bl_harm_grid *g) {
  const bl_params &p = g->params;
  const bl_harm_header &h = g->header;
  auto locate = [&](int index, const char *message) {
    if (index < 0 || index >= h.n_prim) Refuse(message);
    return index;
  };
  bl_grid_desc &d = g->desc;
  d.ind_rho = locate(h.ind_rho, "Unable to locate \"RHO\" slice of \"prims\" in data file.");
  d.ind_pgas = locate(h.ind_uu, "Unable to locate \"UU\" slice of \"prims\" in data file.");
  d.ind_kappa = 0;
  if (g->code_kappa) d.ind_kappa = locate(h.ind_kappa, "Unable to locate electron entropy slice of \"prims\" in data file.");
  d.ind_uu1 = locate(h.ind_u1, "Unable to locate \"U1\" slice of \"prims\" in data file.");
  d.ind_uu2 = locate(h.ind_u2, "Unable to locate \"U2\" slice of \"prims\" in data file.");
  d.ind_uu3 = locate(h.ind_u3, "Unable to locate \"U3\" slice of \"prims\" in data file.");
  d.ind_bb1 = locate(h.ind_b1, "Unable to locate \"B1\" slice of \"prims\" in data file.");
  d.ind_bb2 = locate(h.ind_b2, "Unable to locate \"B2\" slice of \"prims\" in data file.");
  d.ind_bb3 = locate(h.ind_b3, "Unable to locate \"B3\" slice of \"prims\" in data file.");
  auto adiabatic_index = [&](double in_file, bool given, double *value, const char *what, const char *missing) {
    if (in_file != in_file) {   // absent
      if (!given) Refuse(missing);
      return;
    }
    if (!given) {
      *value = in_file;
    } else if (*value != in_file) {
      std::ostringstream message;
      message << "Given " << what << " adiabatic index of " << *value << " does not match file value of " << in_file << "; ignoring the latter.";
      Warn(g, message.str());
    }
  };
  adiabatic_index(h.gam, p.has[BL_P_plasma_gamma] != 0, &d.plasma_gamma, "total", "Could not find total adiabatic index in input or data file.");
  if (p.plasma_model == BL_PLASMA_TI_TE_BETA && !p.plasma_use_p) {
    adiabatic_index(h.gam_p, p.has[BL_P_plasma_gamma_i] != 0, &d.plasma_gamma_i, "ion", "Could not find ion adiabatic index in input or data file.");
    adiabatic_index(h.gam_e, p.has[BL_P_plasma_gamma_e] != 0, &d.plasma_gamma_e, "electron", "Could not find electron adiabatic index in input or data file.");
  }
}

// The part of ConvertPrimitives3 (simulation_geometry.cpp:95-158) that a cell's values do not enter. For modified Kerr-Schild
// coordinates the Jacobian is dr/dx1 = exp(x1), dtheta/dx1 = 0, dtheta/dx2 = pi + (1 - h) pi cos(2 pi x2) (:440-468), with x1 = log r
// of the converted centre, as the reference has it.
void BuildPoints(bl_harm_grid *g) {
  const bl_harm_header &h = g->header;
  const double a = g->params.simulation_a;
  g->points.assign(static_cast<size_t>(h.n1) * h.n2, BlHarmPoint{});
  for (long j = 0; j < h.n2; j++)
    for (long i = 0; i < h.n1; i++) {
      double r = g->coords[3][i], th = g->coords[4][j];
      double x1, x2, dr_dx1, dth_dx1, dth_dx2;
      if (g->fmks) {   // the cell centres are native coordinates (:118-124); Jacobian of the FMKS map (:463-475)
        x1 = r;
        x2 = th;
        SksCoordinates(*g, x1, x2, &r, &th);
        FmksJacobian(*g, x1, x2, &dr_dx1, &dth_dx1, &dth_dx2);
      } else {
        x1 = bl_log(r);
        x2 = g->x2v_native[j];
        dr_dx1 = bl_exp(x1);
        dth_dx1 = 0.0;
        dth_dx2 = kPi + (1.0 - h.hslope) * kPi * bl_cos(2.0 * kPi * x2);
      }
      const double sth = bl_sin(th), cth = bl_cos(th);
      const double sigma = r * r + a * a * cth * cth;
      const double f = 2.0 * r / sigma;
      const double g_tr = f, g_tth = 0.0, g_tph = -a * f * sth * sth;
      const double g_rr = 1.0 + f, g_rth = 0.0, g_rph = -a * (1.0 + f) * sth * sth;
      const double g_thth = sigma, g_thph = 0.0;
      const double g_phph = (r * r + a * a + a * a * f * sth * sth) * sth * sth;
      const double gtt = -(1.0 + f), gtr = f, gtth = 0.0, gtph = 0.0;
      BlHarmPoint &pt = g->points[static_cast<size_t>(j) * h.n1 + i];
      pt.dr_dx1 = dr_dx1;
      pt.dth_dx1 = dth_dx1;
      pt.dth_dx2 = dth_dx2;
      pt.alpha = 1.0 / std::sqrt(-gtt);
      pt.g_01 = dr_dx1 * g_tr + dth_dx1 * g_tth;
      pt.g_02 = dth_dx2 * g_tth;
      pt.g_03 = g_tph;
      pt.g_11 = dr_dx1 * dr_dx1 * g_rr + 2.0 * dr_dx1 * dth_dx1 * g_rth + dth_dx1 * dth_dx1 * g_thth;
      pt.g_12 = dr_dx1 * dth_dx2 * g_rth + dth_dx1 * dth_dx2 * g_thth;
      pt.g_13 = dr_dx1 * g_rph + dth_dx1 * g_thph;
      pt.g_22 = dth_dx2 * dth_dx2 * g_thth;
      pt.g_23 = dth_dx2 * g_thph;
      pt.g_33 = g_phph;
      const double g00 = gtt;
      pt.g01 = gtr / dr_dx1;
      pt.g02 = g_tth / dth_dx2 - dth_dx1 * g_tr / (dr_dx1 * dth_dx2);
      pt.g03 = gtph;
      pt.alpha_mod = 1.0 / std::sqrt(-g00);
      pt.gtr = gtr;
      pt.gtth = gtth;
      pt.gtph = gtph;
    }
}

void FinishDescription(bl_harm_grid *g) {
  const bl_harm_header &h = g->header;
  g->levels.assign(1, 0);
  g->locations.assign(3, 0);
  bl_grid_desc &d = g->desc;
  d.n_blocks = 1;
  d.n_i = h.n1;
  d.n_j = h.n2;
  d.n_k = h.n3;
  d.n_var = h.n_prim;
  d.prim = nullptr;
  d.x1f = g->coords[0].data(); d.x2f = g->coords[1].data(); d.x3f = g->coords[2].data();
  d.x1v = g->coords[3].data(); d.x2v = g->coords[4].data(); d.x3v = g->coords[5].data();
  d.levels = g->levels.data();
  d.locations = g->locations.data();
  d.n_3_root = 0;
  g->converted = d;
  g->converted.n_var = g->code_kappa ? 9 : 8;
  g->converted.ind_rho = 0; g->converted.ind_pgas = 1; g->converted.ind_uu1 = 2; g->converted.ind_uu2 = 3; g->converted.ind_uu3 = 4;
  g->converted.ind_bb1 = 5; g->converted.ind_bb2 = 6; g->converted.ind_bb3 = 7; g->converted.ind_kappa = g->code_kappa ? 8 : 0;
}

// What ReadIharm3d does to a file's cells (simulation_reader.cpp:792-805, simulation_geometry.cpp:95-230), for the variables read
void ConvertHost(const bl_harm_grid &g, const float *prims, float *out) {
  const bl_harm_header &h = g.header;
  const bl_grid_desc &d = g.desc;
  const size_t n1 = h.n1, n2 = h.n2, n3 = h.n3, n_prim = h.n_prim, cells = n1 * n2 * n3;
  const float gamma_minus_one = static_cast<float>(d.plasma_gamma - 1.0);
  const int vector_index[6] = {d.ind_uu1, d.ind_uu2, d.ind_uu3, d.ind_bb1, d.ind_bb2, d.ind_bb3};
  for (size_t i = 0; i < n1; i++)
    for (size_t j = 0; j < n2; j++) {
      const BlHarmPoint &pt = g.points[j * n1 + i];
      for (size_t k = 0; k < n3; k++) {
        const float *cell = prims + ((i * n2 + j) * n3 + k) * n_prim;
        float *to = out + (k * n2 + j) * n1 + i;
        float in[6], converted[6];
        for (int q = 0; q < 6; q++) in[q] = cell[vector_index[q]];
        bl_harm_cell(pt, in, converted);
        to[0] = cell[d.ind_rho];
        to[cells] = cell[d.ind_pgas] * gamma_minus_one;
        for (int q = 0; q < 6; q++) to[(2 + q) * cells] = converted[q];
        if (g.code_kappa) to[8 * cells] = cell[d.ind_kappa];
      }
    }
}

}  // namespace blharm

namespace {
void SetError(char *err, size_t err_len, const std::string &message) {
  if (err != nullptr && err_len > 0) std::snprintf(err, err_len, "Error: %s\n", message.c_str());
}
}  // namespace

extern "C" {

int bl_harm_grid_create(const bl_params *p, const bl_harm_header *header, bl_harm_grid **out, char *err, size_t err_len) {
  if (p == nullptr || header == nullptr || out == nullptr) {
    SetError(err, err_len, "bl_harm_grid_create: bad argument.");
    return BL_E_ARG;
  }
  *out = nullptr;
  bl_harm_grid *g = nullptr;
  try {
    g = new bl_harm_grid;
    g->params = *p;
    g->header = *header;
    g->serial = ++g_serial;
    // the adiabatic indices the input gives (SimulationReader's constructor, simulation_reader.cpp:84-151, Harm formats)
    const bool ion_electron = p->plasma_model == BL_PLASMA_TI_TE_BETA && !p->plasma_use_p;
    g->desc.plasma_gamma = p->has[BL_P_plasma_gamma] ? p->plasma_gamma : 0.0;
    g->desc.plasma_gamma_i = ion_electron && p->has[BL_P_plasma_gamma_i] ? p->plasma_gamma_i : 0.0;
    g->desc.plasma_gamma_e = ion_electron && p->has[BL_P_plasma_gamma_e] ? p->plasma_gamma_e : 0.0;
    if (header->n_prim < 1) throw blharm::Refusal{BL_E_INPUT, "Inconsistency in number of primitive variables."};
    blharm::CheckMetric(g);
    blharm::BuildCoordinates(g);
    blharm::CheckVariables(g);
    if (g->code_kappa) {   // (the reader hands such an entropy over as converted in place; the calls on arrays copy the variable as it lies)
      const bl_grid_desc &d = g->desc;
      for (int index : {d.ind_pgas, d.ind_uu1, d.ind_uu2, d.ind_uu3, d.ind_bb1, d.ind_bb2, d.ind_bb3})
        if (d.ind_kappa == index)
          throw blharm::Refusal{BL_E_UNSUPPORTED, "bl_harm_header: ind_kappa names the internal energy or a vector component, which the conversion changes."};
    }
    blharm::BuildPoints(g);
    blharm::FinishDescription(g);
    *out = g;
    return BL_OK;
  } catch (const blharm::Refusal &refusal) {
    delete g;
    SetError(err, err_len, refusal.message);
    return refusal.code;
  } catch (const std::exception &e) {
    delete g;
    SetError(err, err_len, std::string("Could not build the grid (") + e.what() + ").");
    return BL_E_INPUT;
  }
}

const bl_grid_desc *bl_harm_grid_desc(bl_harm_grid *g, int converted) {
  if (g == nullptr) return nullptr;
  if (g->fmks && !g->map_built) {
    blharm::BuildSksMap(g);
    g->converted.sks_map = g->desc.sks_map;
  }
  return converted != 0 ? &g->converted : &g->desc;
}

const char *bl_harm_grid_warnings(const bl_harm_grid *g) { return g != nullptr ? g->warnings.c_str() : ""; }

int bl_harm_grid_planes(const bl_harm_grid *g) { return g == nullptr ? 0 : (g->code_kappa ? 9 : 8); }

int bl_harm_convert_host(const bl_harm_grid *g, const float *prims, float *out) {
  if (g == nullptr || prims == nullptr || out == nullptr) return BL_E_ARG;
  blharm::ConvertHost(*g, prims, out);
  return BL_OK;
}

void bl_harm_grid_free(bl_harm_grid *g) { delete g; }

size_t bl_harm_header_sizeof(void) { return sizeof(bl_harm_header); }

}  // extern "C"
