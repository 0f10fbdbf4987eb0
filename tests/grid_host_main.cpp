// grid_host_main.cpp - the grid set-up of blacklight_amd/csrc/bl_grid.cpp without a GPU (tests/test_grid_host.py builds this file with
// it, once plainly and once under the host sanitizers).
//
//   grid_host_main <description> [<out>]
//       reads a grid description from a flat file (layout: ReadDescription below, written by test_grid_host.py), calls BuildGridTables
//       and prints either "refused <code> <text>" (exit 2) or "ok" and a dump (exit 0): every table that a pointer of BlGridDevice
//       names with its element count and FNV-1a digest, every scalar of BlGridDevice (doubles and floats as hex bits), the budgets,
//       extents, placement and hash. With <out>, the tables themselves go to <out>.<table> as raw arrays.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "bl_ctx.h"
#include "bl_grid.h"

namespace {

struct Description {
  bl_params params{};
  bl_grid_desc g{};
  std::vector<double> coords[6], sks_map;
  std::vector<int32_t> levels, locations;
  std::vector<float> prim;
};

template <typename T>
void ReadArray(std::FILE *f, std::vector<T> *into, size_t count) {
  into->resize(count);
  if (count > 0 && std::fread(into->data(), sizeof(T), count, f) != count) {
    std::fprintf(stderr, "description cut short\n");
    std::exit(1);
  }
}

// int32 head[32]; double scalars[12]; then the arrays that `head` announces, in the order read here
void ReadDescription(const char *path, Description *d) {
  std::FILE *f = std::fopen(path, "rb");
  if (f == nullptr) {
    std::fprintf(stderr, "cannot open %s\n", path);
    std::exit(1);
  }
  std::vector<int32_t> head;
  std::vector<double> scalars;
  ReadArray(f, &head, 32);
  ReadArray(f, &scalars, 12);
  bl_grid_desc &g = d->g;
  g.n_blocks = head[0]; g.n_i = head[1]; g.n_j = head[2]; g.n_k = head[3]; g.n_var = head[4];
  g.ind_rho = head[5]; g.ind_pgas = head[6]; g.ind_kappa = head[7]; g.ind_uu1 = head[8]; g.ind_uu2 = head[9]; g.ind_uu3 = head[10];
  g.ind_bb1 = head[11]; g.ind_bb2 = head[12]; g.ind_bb3 = head[13];
  g.n_3_root = head[14];
  g.sks_map_n1 = head[15]; g.sks_map_n2 = head[16];
  const int present = head[17];   // bits 0-5: x1f x2f x3f x1v x2v x3v; 6: levels; 7: locations; 8: sks_map; 9: prim
  d->params.simulation_interp = head[18];
  d->params.simulation_block_interp = head[19];
  d->params.simulation_coord = head[20];
  d->params.plasma_model = head[21];
  d->params.slow_light_on = head[22];
  g.plasma_gamma = scalars[0]; g.plasma_gamma_i = scalars[1]; g.plasma_gamma_e = scalars[2];
  g.sks_map_r_in = scalars[3]; g.sks_map_dr = scalars[4]; g.sks_map_dtheta = scalars[5];
  for (int c = 0; c < 6; c++) g.simulation_bounds[c] = scalars[6 + c];
  const size_t n_b = g.n_blocks > 0 ? g.n_blocks : 0;
  const size_t per_block[6] = {size_t(g.n_i) + 1, size_t(g.n_j) + 1, size_t(g.n_k) + 1, size_t(g.n_i), size_t(g.n_j), size_t(g.n_k)};
  const double **into[6] = {&g.x1f, &g.x2f, &g.x3f, &g.x1v, &g.x2v, &g.x3v};
  for (int a = 0; a < 6; a++)
    if (present & (1 << a)) {
      ReadArray(f, &d->coords[a], n_b * per_block[a]);
      *into[a] = d->coords[a].data();
    }
  if (present & 64) { ReadArray(f, &d->levels, n_b); g.levels = d->levels.data(); }
  if (present & 128) { ReadArray(f, &d->locations, 3 * n_b); g.locations = d->locations.data(); }
  if (present & 256) { ReadArray(f, &d->sks_map, size_t(2) * g.sks_map_n1 * g.sks_map_n2); g.sks_map = d->sks_map.data(); }
  if (present & 512) { ReadArray(f, &d->prim, size_t(g.n_var) * n_b * g.n_i * g.n_j * g.n_k); g.prim = d->prim.data(); }
  std::fclose(f);
}

template <typename T>
void Table(const char *name, int axis, const T *data, size_t count, const char *out) {
  if (data == nullptr) return;
  unsigned long long h = 1469598103934665603ull;
  const unsigned char *bytes = reinterpret_cast<const unsigned char *>(data);
  for (size_t at = 0; at < count * sizeof(T); at++) h = (h ^ bytes[at]) * 1099511628211ull;
  char label[64];
  if (axis >= 0) std::snprintf(label, sizeof label, "%s%d", name, axis);
  else std::snprintf(label, sizeof label, "%s", name);
  std::printf("table %s %zu %016llx\n", label, count, h);
  if (out != nullptr) {
    const std::string path = std::string(out) + "." + label;
    std::FILE *f = std::fopen(path.c_str(), "wb");
    if (f == nullptr || std::fwrite(data, sizeof(T), count, f) != count) {
      std::fprintf(stderr, "cannot write %s\n", path.c_str());
      std::exit(1);
    }
    std::fclose(f);
  }
}

unsigned long long Bits(double x) { unsigned long long u; std::memcpy(&u, &x, 8); return u; }
unsigned int Bits(float x) { unsigned int u; std::memcpy(&u, &x, 4); return u; }
void Ints(const char *name, const int *v, int n) {
  std::printf("dev %s", name);
  for (int i = 0; i < n; i++) std::printf(" %d", v[i]);
  std::printf("\n");
}
void Doubles(const char *name, const double *v, int n) {
  std::printf("dev %s", name);
  for (int i = 0; i < n; i++) std::printf(" %016llx", Bits(v[i]));
  std::printf("\n");
}
void Floats(const char *name, const float *v, int n) {
  std::printf("dev %s", name);
  for (int i = 0; i < n; i++) std::printf(" %08x", Bits(v[i]));
  std::printf("\n");
}

// Every table a pointer of `d` names (host memory), then every scalar
void DumpDevice(const BlGridDevice &d, size_t n_cells, const char *out) {
  const size_t n_b = d.n_blocks;
  const size_t n_boxes = size_t(d.n_edge[0]) * d.n_edge[1] * d.n_edge[2];
  Table("kappa", -1, d.kappa, n_cells, out);
  for (int a = 0; a < 3; a++) {
    Table("xf", a, d.xf[a], size_t(d.n[a]) + 1, out);
    Table("xv", a, d.xv[a], size_t(d.n[a]), out);
    Table("bucket", a, d.bucket[a], size_t(d.n_bucket[a]), out);
    Table("bxf", a, d.bxf[a], size_t(d.n_rows[a]) * (d.nb[a] + 1), out);
    Table("bxv", a, d.bxv[a], size_t(d.n_rows[a]) * d.nb[a], out);
    Table("xv_next", a, d.xv_next[a], n_b, out);
    Table("row_guess", a, d.row_guess[a], size_t(d.n_rows[a]) * 3, out);
    Table("edge", a, d.edge[a], size_t(d.n_edge[a]) + 1, out);
    Table("block_row", a, d.block_row[a], n_b, out);
  }
  for (int a = 0; a < 2; a++) Table("angle_trig", a, d.angle_trig[a], size_t(d.n[a + 1]) * 2, out);
  Table("lattice", -1, d.lattice, n_boxes, out);
  Table("fused_desc", -1, d.fused_desc, 4 * n_boxes, out);
  Table("levels", -1, d.levels, n_b, out);
  Table("locations", -1, d.locations, 3 * n_b, out);
  Table("hash_keys", -1, d.hash_keys, size_t(d.hash_mask) + 1, out);
  Table("hash_blocks", -1, d.hash_blocks, size_t(d.hash_mask) + 1, out);
  Table("sks_map", -1, d.sks_map, size_t(2) * d.sks_map_n1 * d.sks_map_n2, out);
  Doubles("bucket_x0", d.bucket_x0, 3); Doubles("bucket_inv_w", d.bucket_inv_w, 3); Ints("n_bucket", d.n_bucket, 3);
  Ints("uniform_mask", &d.uniform_mask, 1); Doubles("cell_x0", d.cell_x0, 3); Doubles("cell_inv_w", d.cell_inv_w, 3);
  Ints("log_uniform", &d.log_uniform, 1); Ints("full_sphere", &d.full_sphere, 1); Floats("log_l0", &d.log_l0, 1); Floats("log_inv_w", &d.log_inv_w, 1);
  Doubles("r_face_in", &d.r_face_in, 1); Doubles("r_face_out", &d.r_face_out, 1);
  Doubles("angle_reach", &d.angle_reach, 1); Floats("angle_guess", d.angle_guess, 4);
  Ints("n", d.n, 3); Ints("nb", d.nb, 3); Ints("stride_row", &d.stride_row, 1); Ints("stride_plane", &d.stride_plane, 1);
  Ints("n_blocks", &d.n_blocks, 1); Ints("n_edge", d.n_edge, 3); Ints("n_rows", d.n_rows, 3);
  Doubles("edge_first", d.edge_first, 3); Doubles("edge_last", d.edge_last, 3);
  for (int a = 0; a < 3; a++) Doubles(a == 0 ? "box_guess0" : (a == 1 ? "box_guess1" : "box_guess2"), d.box_guess[a], 3);
  Ints("refined_lds_bytes", &d.refined_lds_bytes, 1); Ints("fused_lds_bytes", &d.fused_lds_bytes, 1);
  Floats("box_l0", &d.box_l0, 1); Floats("box_linv", &d.box_linv, 1); Doubles("box_x0", d.box_x0, 2); Doubles("box_inv_w", d.box_inv_w, 2);
  const int hash_mask = static_cast<int>(d.hash_mask);
  Ints("block_interp", &d.block_interp, 1); Ints("hash_mask", &hash_mask, 1); Ints("max_level", &d.max_level, 1); Ints("n_3_level0", &d.n_3_level0, 1);
  Ints("fmks", &d.fmks, 1); Ints("sks_map_n1", &d.sks_map_n1, 1); Ints("sks_map_n2", &d.sks_map_n2, 1);
  Doubles("sks_map_r_in", &d.sks_map_r_in, 1); Doubles("sks_map_dr", &d.sks_map_dr, 1); Doubles("sks_map_dtheta", &d.sks_map_dtheta, 1);
  Doubles("fmks_bounds", d.fmks_bounds, 6); Doubles("fmks_x1_0", &d.fmks_x1_0, 1); Doubles("fmks_dx1", &d.fmks_dx1, 1); Doubles("fmks_dx2", &d.fmks_dx2, 1);
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 2 && argc != 3) {
    std::fprintf(stderr, "usage: grid_host_main <description> [<out>]\n");
    return 1;
  }
  const char *out = argc == 3 ? argv[2] : nullptr;
  Description d;
  ReadDescription(argv[1], &d);
  try {
    const GridTables t = BuildGridTables(d.params, d.g);
    // the tables as a kernel sees them: BlGridDevice's pointers into the host vectors (kappa: the repacked plane, else where it lies in prim)
    const float *kappa = !t.kappa.empty() ? t.kappa.data() : (d.g.prim != nullptr ? d.g.prim + size_t(d.g.ind_kappa) * t.placement.n_cells : nullptr);
    const BlGridDevice dev = BindGridTables(t, GridBases{nullptr, kappa, t.coords.data(), t.buckets.data(), t.lattice.data(), t.fused_desc.data(),
                                                         t.block_table.data(), t.block_keys.data(), d.g.sks_map});
    std::printf("ok\n");
    DumpDevice(dev, t.placement.n_cells, out);
    const CellPlacement &pl = t.placement;
    Table("merged_block_at", -1, t.merged_block_at.data(), t.merged_block_at.size(), out);
    Table("origin", -1, pl.has_origin ? pl.origin.data() : nullptr, pl.origin.size(), out);
    std::printf("lds_table_bytes %d\n", t.lds_table_bytes);
    std::printf("merged_blocks %d %d %d\n", t.merged_blocks[0], t.merged_blocks[1], t.merged_blocks[2]);
    std::printf("placement n_cells %zu nb %d %d %d order", pl.n_cells, pl.nb[0], pl.nb[1], pl.nb[2]);
    for (int v = 0; v < 8; v++) std::printf(" %d", pl.order[v]);
    std::printf(" has_origin %d row_stride %llu plane_stride %llu\n", pl.has_origin ? 1 : 0, pl.row_stride, pl.plane_stride);
    std::printf("outer_x1 %016llx\n", Bits(t.outer_x1));
    std::printf("geometry %016llx\n", t.geometry);
    std::printf("same_geometry %d\n", SameGeometry(t, d.g) ? 1 : 0);
  } catch (const Failure &failure) {
    std::printf("refused %d %s\n", failure.code, failure.message.c_str());
    return 2;
  }
  return 0;
}
