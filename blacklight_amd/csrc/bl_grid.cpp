// bl_grid.cpp - a grid's tables on the host (bl_grid.h). Host code only: nothing here calls the GPU. Every expression whose value a
// kernel reads - bucket tables, search guesses, the float conversions, the byte budgets, the hash - is the one bl_set_grid always used.
#include "bl_grid.h"

#include "bl_ctx.h"

namespace blhost {
namespace {

const char *const kBadGrid = "Bad grid description.";
const char *const kBadMesh = "Multi-block grid has blocks that overlap or faces that do not ascend.";
const char *const kBadIndex = "Grid variable index out of range.";

// The parts of a description that decide where a sample lies, in the order the hash takes them
template <typename F>
void ForEachGeometryPart(const bl_grid_desc &g, F &&part) {
  const int32_t dims[5] = {g.n_blocks, g.n_i, g.n_j, g.n_k, g.n_3_root};
  part(dims, sizeof dims);
  const size_t n_b = static_cast<size_t>(g.n_blocks);
  part(g.x1f, n_b * (g.n_i + 1) * sizeof(double)); part(g.x1v, n_b * g.n_i * sizeof(double));
  part(g.x2f, n_b * (g.n_j + 1) * sizeof(double)); part(g.x2v, n_b * g.n_j * sizeof(double));
  part(g.x3f, n_b * (g.n_k + 1) * sizeof(double)); part(g.x3v, n_b * g.n_k * sizeof(double));
  if (g.levels != nullptr) part(g.levels, n_b * sizeof(int32_t));
  if (g.locations != nullptr) part(g.locations, n_b * 3 * sizeof(int32_t));
  if (g.sks_map != nullptr) {
    const int32_t map_dims[2] = {g.sks_map_n1, g.sks_map_n2};
    part(map_dims, sizeof map_dims);
    part(g.sks_map, 2 * static_cast<size_t>(g.sks_map_n1) * g.sks_map_n2 * sizeof(double));
    const double scalars[3] = {g.sks_map_r_in, g.sks_map_dr, g.sks_map_dtheta};
    part(scalars, sizeof scalars);
    part(g.simulation_bounds, sizeof g.simulation_bounds);
  }
}
int GivenTables(const bl_grid_desc &g) { return (g.levels != nullptr ? 1 : 0) | (g.locations != nullptr ? 2 : 0) | (g.sks_map != nullptr ? 4 : 0); }

void BuildBuckets(const double *xf, int n, int n_bucket, std::vector<int> *table, double *x0, double *inv_w) {
  // bucket b covers [x0 + b w, x0 + (b+1) w); table[b] = first cell c with xf[c+1] >= x0 + (b-1) w,
  // i.e. a start index that is never beyond the reference's linear-scan result for any x whose
  // bucket index evaluates to b (one bucket of slack covers rounding of the index computation)
  double lo = xf[0], hi = xf[n];
  double w = (hi - lo) / n_bucket;
  *x0 = lo;
  *inv_w = 1.0 / w;
  table->resize(n_bucket);
  int c = 0;
  for (int b = 0; b < n_bucket; b++) {
    double edge = lo + (b - 1) * w;
    while (c < n - 1 && !(xf[c + 1] >= edge)) c++;
    (*table)[b] = c;
  }
}

// Every face within 1e-4 of a cell of first + c width, in log2 where `logarithmic` (a NaN anywhere: no)
bool FacesOnSteps(const double *f, int n, bool logarithmic, double first, double width) {
  for (int c = 0; c <= n; c++)
    if (!(std::abs((logarithmic ? std::log2(f[c]) : f[c]) - (first + c * width)) <= 1.0e-4 * width)) return false;
  return true;
}
// "Evenly spaced to 1e-4 of a cell", linear or in log2: a positive width and every face on its step. *first and *width are what was
// computed, whatever the answer. The one decision of the merged grid's cell guess (linear) and of the fused kernels' boxes and rows.
// (The merged grid's log r test does not enter here: it asks for f[n] > f[0] in r, not for a positive width in log2 r, and the two
// part where distinct faces share a log2 - there it goes on to say "even" with a width of zero. It keeps its entry conditions and
// shares FacesOnSteps.)
bool EvenlySpaced(const double *f, int n, bool logarithmic, double *first, double *width) {
  if (n < 1 || (logarithmic && !(f[0] > 0.0))) return false;
  *first = logarithmic ? std::log2(f[0]) : f[0];
  const double last = logarithmic ? std::log2(f[n]) : f[n];
  *width = (last - *first) / n;
  return *width > 0.0 && FacesOnSteps(f, n, logarithmic, *first, *width);
}

// Where the search along n ascending faces starts (BlGridDevice::row_guess, box_guess): kind (1: logarithmic), origin, cells per unit.
// Logarithmic where every face is positive and the ratios of neighbouring faces agree better than their differences do.
void SearchGuess(const double *f, int n, double guess[3]) {
  bool positive = f[0] > 0.0;
  double ratio_lo = 1.0e300, ratio_hi = 0.0, step_lo = 1.0e300, step_hi = 0.0;
  for (int i = 0; i < n && positive; i++) {
    ratio_lo = std::min(ratio_lo, f[i + 1] / f[i]); ratio_hi = std::max(ratio_hi, f[i + 1] / f[i]);
    step_lo = std::min(step_lo, f[i + 1] - f[i]); step_hi = std::max(step_hi, f[i + 1] - f[i]);
  }
  const bool logarithmic = positive && n > 1 && (ratio_hi / ratio_lo - 1.0) < 0.5 * (step_hi / step_lo - 1.0);
  if (logarithmic) {
    guess[0] = 1.0;
    guess[1] = std::log2(f[0]);
    guess[2] = n / (std::log2(f[n]) - std::log2(f[0]));
  } else {
    guess[0] = 0.0;
    guess[1] = f[0];
    guess[2] = n / (f[n] - f[0]);
  }
}

void SetVariableOrder(const bl_params &p, const bl_grid_desc &g, GridTables *t) {
  t->code_kappa = p.plasma_model == BL_PLASMA_CODE_KAPPA;
  if (!GridVariableOrder(g, t->code_kappa, t->placement.order)) throw Failure{BL_E_ARG, kBadIndex};
}

// Equal blocks at one refinement level tiling a box, in any order (simulation_sampling.cpp:352-394 searches the blocks per sample):
// merged into one global array at upload; the locate kernel keeps the reference's per-block anchor rules through the block size.
// false: the blocks are not such a tiling, and nothing of *t counts.
bool BuildMergedTables(const bl_params &p, const bl_grid_desc &g, GridTables *t) {
  const int nb_cells[3] = {g.n_i, g.n_j, g.n_k};
  const double *block_xf[3] = {g.x1f, g.x2f, g.x3f};
  const double *block_xv[3] = {g.x1v, g.x2v, g.x3v};
  const int n_b = g.n_blocks;
  std::vector<double> starts[3];          // distinct first faces along each axis, ascending
  std::vector<int> block_pos[3];          // position of every block along each axis
  for (int a = 0; a < 3; a++) {
    for (int blk = 0; blk < n_b; blk++) starts[a].push_back(block_xf[a][static_cast<size_t>(blk) * (nb_cells[a] + 1)]);
    std::sort(starts[a].begin(), starts[a].end());
    starts[a].erase(std::unique(starts[a].begin(), starts[a].end()), starts[a].end());
    block_pos[a].resize(n_b);
    for (int blk = 0; blk < n_b; blk++) {
      const double first = block_xf[a][static_cast<size_t>(blk) * (nb_cells[a] + 1)];
      block_pos[a][blk] = static_cast<int>(std::lower_bound(starts[a].begin(), starts[a].end(), first) - starts[a].begin());
    }
  }
  const int nbl[3] = {static_cast<int>(starts[0].size()), static_cast<int>(starts[1].size()), static_cast<int>(starts[2].size())};
  if (static_cast<long long>(nbl[0]) * nbl[1] * nbl[2] != n_b) return false;
  std::vector<int> block_at(n_b, -1);     // lattice position -> block
  for (int blk = 0; blk < n_b; blk++) {
    const int at = (block_pos[2][blk] * nbl[1] + block_pos[1][blk]) * nbl[0] + block_pos[0][blk];
    if (block_at[at] != -1) return false;
    block_at[at] = blk;
  }
  // global coordinate tables; every block at the same position along an axis must carry the same rows,
  // and neighbouring rows must meet bit for bit (no gaps, no overlaps)
  const int n_i = nbl[0] * nb_cells[0], n_j = nbl[1] * nb_cells[1], n_k = nbl[2] * nb_cells[2];
  const int n[3] = {n_i, n_j, n_k};
  std::vector<double> global_xf[3], global_xv[3];
  for (int a = 0; a < 3; a++) {
    global_xf[a].assign(n[a] + 1, 0.0);
    global_xv[a].assign(n[a], 0.0);
    std::vector<char> seen(nbl[a], 0);
    for (int blk = 0; blk < n_b; blk++) {
      const int pos = block_pos[a][blk];
      const double *f = block_xf[a] + static_cast<size_t>(blk) * (nb_cells[a] + 1);
      const double *v = block_xv[a] + static_cast<size_t>(blk) * nb_cells[a];
      double *gf = global_xf[a].data() + static_cast<size_t>(pos) * nb_cells[a];
      double *gv = global_xv[a].data() + static_cast<size_t>(pos) * nb_cells[a];
      if (!seen[pos]) {
        if (pos > 0 && seen[pos - 1] && std::memcmp(gf, f, sizeof(double)) != 0) return false;
        std::memcpy(gf, f, sizeof(double) * (nb_cells[a] + 1));
        std::memcpy(gv, v, sizeof(double) * nb_cells[a]);
        seen[pos] = 1;
      } else if (std::memcmp(gf, f, sizeof(double) * (nb_cells[a] + 1)) != 0 || std::memcmp(gv, v, sizeof(double) * nb_cells[a]) != 0) {
        return false;
      }
    }
    // joins written by a later block: the first face of block pos must equal the last face of pos - 1
    for (int blk = 0; blk < n_b; blk++) {
      const int pos = block_pos[a][blk];
      const double *f = block_xf[a] + static_cast<size_t>(blk) * (nb_cells[a] + 1);
      if (std::memcmp(global_xf[a].data() + static_cast<size_t>(pos) * nb_cells[a], f, sizeof(double)) != 0
          || std::memcmp(global_xf[a].data() + static_cast<size_t>(pos + 1) * nb_cells[a], f + nb_cells[a], sizeof(double)) != 0)
        return false;
    }
  }
  // ---- a tiling: from here on a fault is a refusal
  t->merged_block_at = block_at;        // (sample checkpoints name cells by MeshBlock and block-local indices)
  for (int a = 0; a < 3; a++) t->merged_blocks[a] = nbl[a];
  const size_t n_cells = static_cast<size_t>(n_i) * n_j * n_k;
  const size_t block_cells = static_cast<size_t>(nb_cells[0]) * nb_cells[1] * nb_cells[2];
  // [var][block][k][j][i] -> global [k][j][i][8]: rho, pgas, uu1, uu2, uu3, bb1, bb2, bb3
  SetVariableOrder(p, g, t);
  CellPlacement &pl = t->placement;
  pl.n_cells = n_cells;
  for (int a = 0; a < 3; a++) pl.nb[a] = nb_cells[a];
  pl.has_origin = n_b > 1;
  pl.row_stride = static_cast<unsigned long long>(n_i);
  pl.plane_stride = static_cast<unsigned long long>(n_i) * n_j;
  if (pl.has_origin) {
    pl.origin.resize(n_b);   // first cell of every block in the merged array
    for (int blk = 0; blk < n_b; blk++)
      pl.origin[blk] = (static_cast<unsigned long long>(block_pos[2][blk]) * nb_cells[2] * n_j + static_cast<unsigned long long>(block_pos[1][blk]) * nb_cells[1]) * n_i
          + static_cast<unsigned long long>(block_pos[0][blk]) * nb_cells[0];
  }
  if (t->code_kappa && n_b > 1 && g.prim != nullptr) {
    // the ninth value of a cell (simulation_reader.cpp:1164-1172) in its own [k][j][i] array: only the
    // extended coefficient kernel reads it (cells in device memory: the staging kernel places the plane at pl.origin)
    t->kappa.resize(n_cells);
    for (int blk = 0; blk < n_b; blk++) {
      const int pi = block_pos[0][blk], pj = block_pos[1][blk], pk = block_pos[2][blk];
      const float *src = g.prim + (static_cast<size_t>(g.ind_kappa) * n_b + blk) * block_cells;
      for (int k = 0; k < nb_cells[2]; k++)
        for (int j = 0; j < nb_cells[1]; j++) {
          const size_t row = (static_cast<size_t>(pk * nb_cells[2] + k) * n_j + (pj * nb_cells[1] + j)) * n_i + static_cast<size_t>(pi) * nb_cells[0];
          std::memcpy(t->kappa.data() + row, src + (static_cast<size_t>(k) * nb_cells[1] + j) * nb_cells[0], sizeof(float) * nb_cells[0]);
        }
    }
  }
  // coordinates
  const double *xf[3] = {global_xf[0].data(), global_xf[1].data(), global_xf[2].data()};
  const double *xv[3] = {global_xv[0].data(), global_xv[1].data(), global_xv[2].data()};
  std::vector<double> &coords = t->coords;
  for (int a = 0; a < 3; a++) {
    t->at.xf[a] = coords.size();
    coords.insert(coords.end(), xf[a], xf[a] + n[a] + 1);
    t->at.xv[a] = coords.size();
    coords.insert(coords.end(), xv[a], xv[a] + n[a]);
  }
  // cosine and sine of every theta and phi centre, and how far a cell reaches from its centre: what the tolerant coefficient kernel's
  // angles relative to the cell centre ask for (bl_local_angles.h)
  double angle_reach = 0.0;
  for (int a = 1; a < 3; a++) {
    t->at.angle_trig[a - 1] = coords.size();
    for (int c = 0; c < n[a]; c++) {
      double sine, cosine;
      bl_sincos(xv[a][c], &sine, &cosine);
      coords.push_back(cosine);
      coords.push_back(sine);
      angle_reach = std::max(angle_reach, std::max(xv[a][c] - xf[a][c], xf[a][c + 1] - xv[a][c]));
    }
  }
  // bucket tables for the cell search
  if (n_i > 65535 || n_j > 65535 || n_k > 65535)
    throw Failure{BL_E_UNSUPPORTED, "More than 65535 cells along an axis of the merged grid."};
  BlGridDevice &dev = t->dev;
  for (int a = 0; a < 3; a++) {
    int n_bucket = std::max(512, 8 * n[a]);
    std::vector<int> table;
    BuildBuckets(xf[a], n[a], n_bucket, &table, &dev.bucket_x0[a], &dev.bucket_inv_w[a]);
    {   // evenly spaced faces?
      double first, width = 0.0;
      const bool even = EvenlySpaced(xf[a], n[a], false, &first, &width);
      dev.cell_x0[a] = xf[a][0];
      dev.cell_inv_w[a] = even ? 1.0 / width : 0.0;
      if (even) dev.uniform_mask |= 1 << a;
    }
    if (a == 0) {   // radial faces evenly spaced in log r? (bl_shade_fused2_kernel guesses the cell from log2 r and confirms it by the faces)
      dev.r_face_in = xf[0][0];
      dev.r_face_out = xf[0][n[0]];
      bool even = xf[0][0] > 0.0 && xf[0][n[0]] > xf[0][0];
      const double l0 = even ? std::log2(xf[0][0]) : 0.0, width = even ? (std::log2(xf[0][n[0]]) - l0) / n[0] : 1.0;
      even = even && FacesOnSteps(xf[0], n[0], true, l0, width);
      dev.log_uniform = even ? 1 : 0;
      dev.log_l0 = static_cast<float>(l0);
      dev.log_inv_w = static_cast<float>(1.0 / width);
    }
    dev.n_bucket[a] = n_bucket;
    t->at.bucket[a] = t->buckets.size();
    t->buckets.insert(t->buckets.end(), table.begin(), table.end());
  }
  // theta from pole to pole and phi all the way round: no sample is off the grid in angle
  dev.full_sphere = (xf[1][0] <= 0.0 && xf[1][n[1]] >= kPi && xf[2][0] <= 0.0 && xf[2][n[2]] >= 2.0 * kPi) ? 1 : 0;
  dev.n_blocks = 0;
  dev.stride_row = n_i;
  dev.stride_plane = n_i * n_j;
  for (int a = 0; a < 3; a++) {
    dev.n[a] = n[a];
    dev.nb[a] = nb_cells[a];
  }
  dev.angle_reach = angle_reach;
  for (int a = 1; a < 3; a++) {
    dev.angle_guess[2 * a - 2] = static_cast<float>(dev.cell_x0[a]);
    dev.angle_guess[2 * a - 1] = static_cast<float>(dev.cell_inv_w[a]);
  }
  if (p.simulation_coord == BL_COORD_FMKS) {
    // FMKS grid (simulation_sampling.cpp:66-73): native coordinates above, plus the reader's map and bounds
    if (n_b != 1 || g.sks_map == nullptr || g.sks_map_n1 < 2 || g.sks_map_n2 < 2)
      throw Failure{BL_E_ARG, "simulation_coord = fmks needs a single block and the reader's sks_map in bl_grid_desc."};
    dev.fmks = 1;
    dev.sks_map_n1 = g.sks_map_n1;
    dev.sks_map_n2 = g.sks_map_n2;
    dev.sks_map_r_in = g.sks_map_r_in;
    dev.sks_map_dr = g.sks_map_dr;
    dev.sks_map_dtheta = g.sks_map_dtheta;
    for (int c = 0; c < 6; c++) dev.fmks_bounds[c] = g.simulation_bounds[c];
    dev.fmks_x1_0 = xf[0][0];
    dev.fmks_dx1 = xf[0][1] - xf[0][0];
    dev.fmks_dx2 = xf[1][1] - xf[1][0];
  }
  // The locate kernel stages the tables in LDS when they fit 60 KiB: faces and centres as doubles and max(512, 8 n) 16-bit buckets
  // per axis, 32 n + 8 bytes for an axis of 64 cells or more - about 640 cells on each of three axes, or 1 847 on one beside two
  // of eight. (The kernels with the locate step inside have a budget of their own: 1 018 cells summed over the axes,
  // bl_fused2_applicable.) Larger grids are searched in the same tables where they lie in HBM (lds_table_bytes = 0).
  size_t bytes = 0;
  for (int a = 0; a < 3; a++) bytes += (2 * static_cast<size_t>(n[a]) + 1) * sizeof(double) + static_cast<size_t>(dev.n_bucket[a]) * sizeof(unsigned short);
  t->lds_table_bytes = bytes > 60 * 1024 ? 0 : static_cast<int>((bytes + 15) / 16 * 16);
  if (t->lds_table_bytes == 0 && p.slow_light_on)
    throw Failure{BL_E_UNSUPPORTED, "Slow light on a grid whose coordinate tables exceed the 60 KiB LDS budget is not built."};
  return true;
}

// Mesh with refinement (blocks of several levels), or any other set of non-overlapping equal-sized blocks:
// cells stay block by block; the distinct block boundaries along each axis span a lattice of boxes, each
// covered by at most one block, from which the locate kernel finds the block of a sample (the reference
// scans all blocks per sample, simulation_sampling.cpp:352-394), then the cell from the block's own rows.
void BuildLatticeTables(const bl_params &p, const bl_grid_desc &g, GridTables *t) {
  const int nb[3] = {g.n_i, g.n_j, g.n_k};
  const double *block_xf[3] = {g.x1f, g.x2f, g.x3f};
  const double *block_xv[3] = {g.x1v, g.x2v, g.x3v};
  const int n_b = g.n_blocks;
  std::vector<double> edge[3];
  for (int a = 0; a < 3; a++) {
    for (int blk = 0; blk < n_b; blk++) {
      const double *f = block_xf[a] + static_cast<size_t>(blk) * (nb[a] + 1);
      for (int i = 0; i < nb[a]; i++)
        if (!(f[i] < f[i + 1])) throw Failure{BL_E_UNSUPPORTED, kBadMesh};
      edge[a].push_back(f[0]);
      edge[a].push_back(f[nb[a]]);
    }
    std::sort(edge[a].begin(), edge[a].end());
    edge[a].erase(std::unique(edge[a].begin(), edge[a].end()), edge[a].end());
  }
  const int n_edge[3] = {static_cast<int>(edge[0].size()) - 1, static_cast<int>(edge[1].size()) - 1,
                         static_cast<int>(edge[2].size()) - 1};
  const size_t n_boxes = static_cast<size_t>(n_edge[0]) * n_edge[1] * n_edge[2];
  const size_t block_cells = static_cast<size_t>(nb[0]) * nb[1] * nb[2];
  const size_t n_cells = block_cells * n_b;
  if (n_boxes > (1ull << 28) || n_cells >= (1ull << 32))
    throw Failure{BL_E_UNSUPPORTED, "Multi-block grid too large for the block lattice of this build."};
  std::vector<int> &lattice = t->lattice;
  lattice.assign(n_boxes, -1);
  for (int blk = 0; blk < n_b; blk++) {
    int lo[3], hi[3];
    for (int a = 0; a < 3; a++) {
      const double *f = block_xf[a] + static_cast<size_t>(blk) * (nb[a] + 1);
      lo[a] = static_cast<int>(std::lower_bound(edge[a].begin(), edge[a].end(), f[0]) - edge[a].begin());
      hi[a] = static_cast<int>(std::lower_bound(edge[a].begin(), edge[a].end(), f[nb[a]]) - edge[a].begin());
    }
    for (int kk = lo[2]; kk < hi[2]; kk++)
      for (int jj = lo[1]; jj < hi[1]; jj++)
        for (int ii = lo[0]; ii < hi[0]; ii++) {
          int &slot = lattice[(static_cast<size_t>(kk) * n_edge[1] + jj) * n_edge[0] + ii];
          if (slot != -1) throw Failure{BL_E_UNSUPPORTED, kBadMesh};
          slot = blk;
        }
  }
  // cells: [var][block][k][j][i] -> [block][k][j][i][8] (the blocks stay one behind the other: the caller's order)
  SetVariableOrder(p, g, t);
  t->placement.n_cells = n_cells;
  for (int a = 0; a < 3; a++) t->placement.nb[a] = nb[a];
  // Coordinate rows, each distinct one once (faces and centres of a block along an axis, compared bit for bit: blocks of one level at
  // one position share them), which row every block uses, the first centre of the next block of the file (what the reference reads one
  // past a block's last centre), then the block boundaries
  std::vector<double> &coords = t->coords;
  std::vector<int> block_row(static_cast<size_t>(n_b) * 3);
  int n_rows[3];
  for (int a = 0; a < 3; a++) {
    const size_t row_len = static_cast<size_t>(nb[a]) * 2 + 1;
    std::map<std::vector<unsigned long long>, int> seen;   // (rows compared word for word: the same bits, not merely equal values)
    std::vector<const double *> row_f, row_v;
    for (int blk = 0; blk < n_b; blk++) {
      const double *f = block_xf[a] + static_cast<size_t>(blk) * (nb[a] + 1), *v = block_xv[a] + static_cast<size_t>(blk) * nb[a];
      std::vector<unsigned long long> key(row_len);
      std::memcpy(key.data(), f, (static_cast<size_t>(nb[a]) + 1) * sizeof(double));
      std::memcpy(key.data() + nb[a] + 1, v, static_cast<size_t>(nb[a]) * sizeof(double));
      auto found = seen.find(key);
      if (found == seen.end()) {
        found = seen.emplace(std::move(key), static_cast<int>(row_f.size())).first;
        row_f.push_back(f);
        row_v.push_back(v);
      }
      block_row[static_cast<size_t>(a) * n_b + blk] = found->second;
    }
    n_rows[a] = static_cast<int>(row_f.size());
    t->at.bxf[a] = coords.size();
    for (const double *f : row_f) coords.insert(coords.end(), f, f + nb[a] + 1);
    t->at.bxv[a] = coords.size();
    for (const double *v : row_v) coords.insert(coords.end(), v, v + nb[a]);
    t->at.xv_next[a] = coords.size();
    for (int blk = 0; blk < n_b; blk++)
      coords.push_back(blk + 1 < n_b ? block_xv[a][static_cast<size_t>(blk + 1) * nb[a]] : std::numeric_limits<double>::quiet_NaN());
    t->at.row_guess[a] = coords.size();
    for (const double *f : row_f) {
      double guess[3];
      SearchGuess(f, nb[a], guess);
      coords.insert(coords.end(), guess, guess + 3);
    }
    t->at.edge[a] = coords.size();
    coords.insert(coords.end(), edge[a].begin(), edge[a].end());
  }
  // (the lattice, then the blocks' rows)
  const size_t lattice_ints = lattice.size();
  lattice.insert(lattice.end(), block_row.begin(), block_row.end());
  BlGridDevice &dev = t->dev;
  dev.n_blocks = n_b;
  t->at.lattice = 0;
  dev.stride_row = nb[0];
  dev.stride_plane = nb[0] * nb[1];
  for (int a = 0; a < 3; a++) {
    t->at.block_row[a] = lattice_ints + static_cast<size_t>(a) * n_b;
    dev.n_rows[a] = n_rows[a];
    dev.n_edge[a] = n_edge[a];
    dev.edge_first[a] = edge[a].front();
    dev.edge_last[a] = edge[a].back();
    SearchGuess(edge[a].data(), n_edge[a], dev.box_guess[a]);
    dev.n[a] = nb[a];
    dev.nb[a] = nb[a];
  }
  if (p.simulation_interp && p.simulation_block_interp) {
    // MeshBlock table for FindNearbyInds (simulation_sampling.cpp:36-39, :84-93) and a hash from (level, location)
    // to block in place of its scans over all blocks
    // n_3_root only enters through the periodic seam of spherical coordinates (simulation_sampling.cpp:1181-1219)
    if (g.levels == nullptr || g.locations == nullptr || (g.n_3_root <= 0 && p.simulation_coord == BL_COORD_SKS))
      throw Failure{BL_E_ARG, "simulation_block_interp = true needs the MeshBlock table (levels, locations, n_3_root) in bl_grid_desc."};
    int max_level = 0;
    for (int blk = 0; blk < n_b; blk++) {
      if (g.levels[blk] < 0 || g.levels[blk] > 30) throw Failure{BL_E_ARG, "Bad MeshBlock level."};
      max_level = std::max(max_level, g.levels[blk]);
      for (int a = 0; a < 3; a++)
        if (g.locations[3 * blk + a] < 0 || g.locations[3 * blk + a] >= (1 << 19)) throw Failure{BL_E_UNSUPPORTED, "MeshBlock location outside the range of this build."};
    }
    unsigned int slots = 16;
    while (slots < 2u * static_cast<unsigned int>(n_b)) slots *= 2;
    std::vector<unsigned long long> &keys = t->block_keys;
    std::vector<int> &table = t->block_table;
    keys.assign(slots, ~0ull);
    table.assign(static_cast<size_t>(n_b) * 4 + slots, -1);
    for (int blk = 0; blk < n_b; blk++) {
      table[blk] = g.levels[blk];
      for (int a = 0; a < 3; a++) table[n_b + 3 * blk + a] = g.locations[3 * blk + a];
      const unsigned long long key = (static_cast<unsigned long long>(g.levels[blk]) << 57) | (static_cast<unsigned long long>(g.locations[3 * blk]) << 38)
          | (static_cast<unsigned long long>(g.locations[3 * blk + 1]) << 19) | static_cast<unsigned long long>(g.locations[3 * blk + 2]);
      unsigned int slot = static_cast<unsigned int>((key * 0x9e3779b97f4a7c15ull) >> 32) & (slots - 1);
      while (keys[slot] != ~0ull) {
        if (keys[slot] == key) throw Failure{BL_E_UNSUPPORTED, kBadMesh};   // two blocks at one place
        slot = (slot + 1) & (slots - 1);
      }
      keys[slot] = key;
      table[static_cast<size_t>(n_b) * 4 + slot] = blk;
    }
    dev.block_interp = 1;
    t->at.levels = 0;
    t->at.locations = n_b;
    t->at.hash_blocks = static_cast<size_t>(n_b) * 4;
    dev.hash_mask = slots - 1;
    dev.max_level = max_level;
    dev.n_3_level0 = g.n_3_root / nb[2];
  }
  {
    // what bl_locate_kernel<kRefined> stages in LDS when it fits (four workgroups to a compute unit up to 36 KiB, one of 1 024 lanes beyond): block boundaries,
    // lattice, rows, the blocks' rows and next centres, and with inter-block interpolation the MeshBlock table and its hash
    size_t doubles = 0, ints = lattice_ints + static_cast<size_t>(n_b) * 3;
    for (int a = 0; a < 3; a++) doubles += static_cast<size_t>(n_edge[a]) + 1 + static_cast<size_t>(n_rows[a]) * (2 * nb[a] + 1 + 3) + n_b;
    if (dev.block_interp) {
      doubles += dev.hash_mask + 1;                                        // (the keys: 8 bytes each)
      ints += static_cast<size_t>(n_b) * 4 + dev.hash_mask + 1;
    }
    const size_t bytes = doubles * sizeof(double) + (ints + 3) / 4 * 4 * sizeof(int);
    dev.refined_lds_bytes = bytes <= static_cast<size_t>(BL_LOCATE_REFINED_LDS) ? static_cast<int>(bytes) : 0;
  }
  {
    // what bl_shade_fused2_kernel<..., kRefined> asks of a mesh (bl_shade_fused.hip): boxes and rows evenly spaced in log r / theta / phi to
    // 1e-4 of a cell (its guesses are then right wherever its margins let it decide), the sphere covered without a hole, 32-bit byte
    // offsets into the cell array, room in LDS for the row chunks and one descriptor per box (one 512-lane workgroup to a compute unit)
    bool ok = nb[0] >= 2 && nb[1] >= 2 && nb[2] >= 2 && n_cells * 32ull < (1ull << 32) && static_cast<unsigned long long>(nb[1]) * nb[2] < (1ull << 24);
    for (size_t box = 0; box < n_boxes && ok; box++) ok = lattice[box] >= 0;
    ok = ok && edge[1].front() <= 0.0 && edge[1].back() >= kPi && edge[2].front() <= 0.0 && edge[2].back() >= 2.0 * kPi;
    double origin[3] = {0.0, 0.0, 0.0}, width[3] = {0.0, 0.0, 0.0};
    for (int a = 0; a < 3 && ok; a++) ok = EvenlySpaced(edge[a].data(), n_edge[a], a == 0, &origin[a], &width[a]);
    size_t chunk_at[3] = {0, 0, 0}, bytes = 48 * sizeof(double);
    for (int a = 0; a < 3 && ok; a++) {
      chunk_at[a] = bytes - 48 * sizeof(double);   // (relative to the first chunk: the kernel adds where that lies)
      for (int q = 0; q < n_rows[a] && ok; q++) {
        const double *guess = coords.data() + t->at.row_guess[a] + 3 * static_cast<size_t>(q);
        double row_origin, row_width;
        ok = (guess[0] != 0.0) == (a == 0) && EvenlySpaced(coords.data() + t->at.bxf[a] + static_cast<size_t>(q) * (nb[a] + 1), nb[a], a == 0, &row_origin, &row_width);
      }
      bytes += static_cast<size_t>(n_rows[a]) * (16 + 64 * static_cast<size_t>(nb[a]));
    }
    bytes += 16 * n_boxes;
    ok = ok && bytes <= static_cast<size_t>(BL_FUSED_REFINED_LDS);
    if (ok) {
      std::vector<unsigned int> &desc = t->fused_desc;
      desc.resize(4 * n_boxes);
      for (size_t box = 0; box < n_boxes; box++) {
        const int blk = lattice[box];
        desc[4 * box] = static_cast<unsigned int>(static_cast<size_t>(blk) * block_cells * 32);
        for (int a = 0; a < 3; a++)
          desc[4 * box + 1 + a] = static_cast<unsigned int>(chunk_at[a] + static_cast<size_t>(block_row[static_cast<size_t>(a) * n_b + blk]) * (16 + 64 * static_cast<size_t>(nb[a])));
      }
      dev.fused_lds_bytes = static_cast<int>(bytes);
      dev.box_l0 = static_cast<float>(origin[0]);
      dev.box_linv = static_cast<float>(1.0 / width[0]);
      for (int a = 1; a < 3; a++) {
        dev.box_x0[a - 1] = origin[a];
        dev.box_inv_w[a - 1] = 1.0 / width[a];
      }
      dev.r_face_in = edge[0].front();
      dev.r_face_out = edge[0].back();
    }
  }
  t->lds_table_bytes = 0;
}

}  // namespace

// Hash (FNV-1a, 64 bits) of everything about a grid that decides WHERE a sample lies on it: the block table, the coordinate arrays,
// the FMKS look-up table. Two bl_set_grid calls with the same hash very likely hand over the same geometry (the cells may differ);
// SameGeometry settles it. Located samples of the first then stay valid for the second (the reference's `first_time`,
// radiation_integrator.cpp:693-704).
unsigned long long GridGeometryHash(const bl_grid_desc &g) {
  unsigned long long h = 1469598103934665603ull;
  ForEachGeometryPart(g, [&h](const void *data, size_t bytes) {
    const unsigned char *p = static_cast<const unsigned char *>(data);
    // (eight bytes a step where they are there: coordinate arrays are doubles)
    size_t at = 0;
    for (; at + 8 <= bytes; at += 8) {
      unsigned long long word;
      std::memcpy(&word, p + at, 8);
      h = (h ^ word) * 1099511628211ull;
      h ^= h >> 29;
    }
    for (; at < bytes; at++) h = (h ^ p[at]) * 1099511628211ull;
  });
  return h != 0 ? h : 1;
}

bool SameGeometry(const GridTables &t, const bl_grid_desc &g) {
  if (t.geometry == 0 || GridGeometryHash(g) != t.geometry || GivenTables(g) != t.given_tables) return false;
  size_t at = 0;
  bool same = true;
  ForEachGeometryPart(g, [&](const void *data, size_t bytes) {
    same = same && at + bytes <= t.given.size() && std::memcmp(t.given.data() + at, data, bytes) == 0;
    at += bytes;
  });
  return same && at == t.given.size();
}

BlGridDevice BindGridTables(const GridTables &t, const GridBases &base) {
  BlGridDevice dev = t.dev;
  const GridOffsets &at = t.at;
  auto bind = [](auto *&pointer, auto *table, size_t offset) { pointer = offset == GridOffsets::kNone ? nullptr : table + offset; };
  dev.cells = base.cells;
  dev.kappa = t.code_kappa ? base.kappa : nullptr;
  for (int a = 0; a < 3; a++) {
    bind(dev.xf[a], base.coords, at.xf[a]);
    bind(dev.xv[a], base.coords, at.xv[a]);
    bind(dev.bucket[a], base.buckets, at.bucket[a]);
    bind(dev.bxf[a], base.coords, at.bxf[a]);
    bind(dev.bxv[a], base.coords, at.bxv[a]);
    bind(dev.xv_next[a], base.coords, at.xv_next[a]);
    bind(dev.row_guess[a], base.coords, at.row_guess[a]);
    bind(dev.edge[a], base.coords, at.edge[a]);
    bind(dev.block_row[a], base.lattice, at.block_row[a]);
  }
  for (int a = 0; a < 2; a++) bind(dev.angle_trig[a], base.coords, at.angle_trig[a]);
  bind(dev.lattice, base.lattice, at.lattice);
  bind(dev.levels, base.block_table, at.levels);
  bind(dev.locations, base.block_table, at.locations);
  bind(dev.hash_blocks, base.block_table, at.hash_blocks);
  dev.hash_keys = t.block_keys.empty() ? nullptr : base.block_keys;
  dev.fused_desc = t.fused_desc.empty() ? nullptr : base.fused_desc;
  dev.sks_map = t.dev.fmks ? base.sks_map : nullptr;
  return dev;
}

bool GridVariableOrder(const bl_grid_desc &g, bool code_kappa, int order[8]) {
  const int given[8] = {g.ind_rho, g.ind_pgas, g.ind_uu1, g.ind_uu2, g.ind_uu3, g.ind_bb1, g.ind_bb2, g.ind_bb3};
  bool in_range = !code_kappa || (g.ind_kappa >= 0 && g.ind_kappa < g.n_var);
  for (int v = 0; v < 8; v++) {
    order[v] = given[v];
    in_range = in_range && given[v] >= 0 && given[v] < g.n_var;
  }
  return in_range;
}

void CheckDeviceCells(const bl_grid_desc &g, bool code_kappa, const bl_device_cells *cells) {
  if (cells == nullptr) throw Failure{BL_E_ARG, "bl_device_cells: the description is NULL."};
  if (cells->prim == nullptr) throw Failure{BL_E_ARG, "bl_device_cells: prim is NULL."};
  if (cells->dtype != BL_CELLS_F32 && cells->dtype != BL_CELLS_F64) throw Failure{BL_E_ARG, "bl_device_cells: dtype must be BL_CELLS_F32 or BL_CELLS_F64."};
  if (reinterpret_cast<uintptr_t>(cells->prim) % (cells->dtype == BL_CELLS_F64 ? sizeof(double) : sizeof(float)) != 0)
    throw Failure{BL_E_ARG, "bl_device_cells: prim is not aligned to its element type."};
  if (cells->var_stride < 1) throw Failure{BL_E_ARG, "bl_device_cells: var_stride must be at least 1."};
  if (cells->block_stride < 1) throw Failure{BL_E_ARG, "bl_device_cells: block_stride must be at least 1."};
  int order[8];
  if (g.n_blocks < 1 || g.n_i < 1 || g.n_j < 1 || g.n_k < 1 || !GridVariableOrder(g, code_kappa, order)) return;   // (refused further on)
  int last_var = code_kappa ? g.ind_kappa : 0;
  for (int v = 0; v < 8; v++) last_var = std::max(last_var, order[v]);
  // last_var * var_stride + (n_blocks - 1) * block_stride + n_i * n_j * n_k - 1, the index of the furthest element read
  int64_t reach = 0, term = 0;
  bool overflow = __builtin_mul_overflow(static_cast<int64_t>(g.n_i), static_cast<int64_t>(g.n_j), &reach) || __builtin_mul_overflow(reach, static_cast<int64_t>(g.n_k), &reach);
  reach -= 1;
  overflow = overflow || __builtin_mul_overflow(static_cast<int64_t>(g.n_blocks) - 1, cells->block_stride, &term) || __builtin_add_overflow(reach, term, &reach);
  overflow = overflow || __builtin_mul_overflow(static_cast<int64_t>(last_var), cells->var_stride, &term) || __builtin_add_overflow(reach, term, &reach);
  if (overflow || reach >= cells->n_elements) throw Failure{BL_E_ARG, "bl_device_cells: n_elements is smaller than what the strides and the grid's extents reach."};
}

void ValidateGridDescription(const bl_grid_desc &g) {
  if (g.n_blocks < 1) throw Failure{BL_E_ARG, kBadGrid};
  if (g.n_i < 2 || g.n_j < 2 || g.n_k < 2) throw Failure{BL_E_ARG, kBadGrid};
  for (const double *array : {g.x1f, g.x2f, g.x3f, g.x1v, g.x2v, g.x3v})
    if (array == nullptr) throw Failure{BL_E_ARG, kBadGrid};
}

GridTables BuildGridTables(const bl_params &p, const bl_grid_desc &g) {
  ValidateGridDescription(g);
  GridTables t;
  // inter-block interpolation works on the MeshBlocks as they are; else the lattice takes blocks of several levels, or a tiling with holes
  if ((p.simulation_interp && p.simulation_block_interp) || !BuildMergedTables(p, g, &t)) {
    t = GridTables{};
    BuildLatticeTables(p, g, &t);
  }
  t.geometry = GridGeometryHash(g);
  t.given_tables = GivenTables(g);
  size_t given_bytes = 0;
  ForEachGeometryPart(g, [&given_bytes](const void *, size_t bytes) { given_bytes += bytes; });
  t.given.reserve(given_bytes);
  ForEachGeometryPart(g, [&t](const void *data, size_t bytes) {
    const unsigned char *first = static_cast<const unsigned char *>(data);
    t.given.insert(t.given.end(), first, first + bytes);
  });
  t.outer_x1 = g.x1f[g.n_i];
  for (int blk = 1; blk < g.n_blocks; blk++) t.outer_x1 = std::max(t.outer_x1, g.x1f[static_cast<size_t>(blk) * (g.n_i + 1) + g.n_i]);
  return t;
}

}  // namespace blhost
