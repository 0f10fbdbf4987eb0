// bl_checkpoint.cpp - the reference's checkpoint files (geodesic_checkpoint.cpp:28-108, sample_checkpoint.cpp:22-46, file_io.cpp:65-127)
// and what turns them into a chunk's sample records and back. Host code only: byte layout and index reversal.
#include "bl_checkpoint.h"

#include <sys/stat.h>

#include <initializer_list>

namespace blhost {
namespace {

// ---- an Array of the reference (file_io.cpp:65-127): five int32 extents n1 ... n5, fastest first, followed by the data
template <typename T>
void ReadArray(std::istream &in, std::vector<T> *data) {
  int dims[5];
  in.read(reinterpret_cast<char *>(dims), sizeof dims);
  const size_t cap = (1ull << 36) / sizeof(T);
  size_t count = 1;
  bool fits = static_cast<bool>(in);
  for (int a = 0; a < 5 && fits; a++) {   // (the product is compared before it is formed: no five extents wrap it back under the cap)
    const size_t extent = static_cast<size_t>(std::max(dims[a], 1));
    fits = count <= cap / extent;
    count *= extent;
  }
  if (!fits) throw Failure{BL_E_INPUT, "Geodesic checkpoint file is damaged."};
  data->resize(count);
  in.read(reinterpret_cast<char *>(data->data()), static_cast<std::streamsize>(count * sizeof(T)));
  if (!in) throw Failure{BL_E_INPUT, "Geodesic checkpoint file is damaged."};
}

void WriteHeader(std::ostream &out, std::initializer_list<int> extents) {
  int dims[5] = {1, 1, 1, 1, 1};
  std::copy(extents.begin(), extents.end(), dims);
  out.write(reinterpret_cast<const char *>(dims), sizeof dims);
}

template <typename T>
void WriteArray(std::ostream &out, std::initializer_list<int> extents, const T *data) {
  WriteHeader(out, extents);
  size_t count = 1;
  for (int extent : extents) count *= static_cast<size_t>(extent);
  out.write(reinterpret_cast<const char *>(data), static_cast<std::streamsize>(count * sizeof(T)));
}

// An Array (n_pix, num_steps, per_sample) from packed samples: a pixel's samples, then zeros. (The reference leaves what lies
// beyond a pixel's samples - and samples it cut or found off the grid - as allocated; nothing reads it.)
template <typename T>
void WritePaddedRows(std::ostream &out, std::initializer_list<int> extents, const std::vector<T> &packed, const std::vector<size_t> &offset,
                     const std::vector<int32_t> &sample_num, int num_steps, int per_sample) {
  WriteHeader(out, extents);
  std::vector<T> row(static_cast<size_t>(num_steps) * per_sample);
  for (size_t m = 0; m < sample_num.size(); m++) {
    std::fill(row.begin(), row.end(), T(0));
    const size_t first = offset[m] * per_sample, count = static_cast<size_t>(sample_num[m]) * per_sample;
    std::copy(packed.begin() + first, packed.begin() + first + count, row.begin());
    out.write(reinterpret_cast<const char *>(row.data()), static_cast<std::streamsize>(row.size() * sizeof(T)));
  }
}

int MostSamples(const std::vector<int32_t> &sample_num) {
  return sample_num.empty() ? 0 : std::max(0, static_cast<int>(*std::max_element(sample_num.begin(), sample_num.end())));
}

// A chunk's rays behind the `packed` samples the file being assembled holds already: each ray's first entry there (HostChunk::offset),
// and by pixel its sample_num and offset. Returns what the file holds with them.
size_t PlaceRays(HostChunk &chunk, size_t packed, long long n_rays, std::vector<int32_t> *sample_num, std::vector<size_t> *offset) {
  sample_num->resize(n_rays);   // (zeros, with the first chunk)
  offset->resize(n_rays);
  chunk.offset.resize(chunk.sample_num.size());
  for (size_t q = 0; q < chunk.sample_num.size(); q++) {
    const size_t m = static_cast<size_t>(chunk.out_index[q]);
    (*sample_num)[m] = chunk.sample_num[q];
    (*offset)[m] = chunk.offset[q] = packed;
    packed += static_cast<size_t>(chunk.sample_num[q]);
  }
  return packed;
}

}  // namespace

// ---- geodesic checkpoints (geodesic_checkpoint.cpp:28-108): 7 x 4 doubles of camera frame, then Arrays of camera_pos (n_pix, 4),
// camera_dir (n_pix, 4), image_frequencies, momentum_factors (n_pix), the int geodesic_num_steps, sample_flags (n_pix, bool),
// sample_num (n_pix, int), sample_pos (n_pix, n_steps, 4), sample_dir (n_pix, n_steps, 4), sample_len (n_pix, n_steps); root level only.
std::shared_ptr<const bl_ctx::Checkpoint> ReadGeodesicCheckpoint(const bl_params &p) {
  std::ifstream in(p.checkpoint_geodesic_file.s, std::ios_base::in | std::ios_base::binary);
  if (!in.is_open()) throw Failure{BL_E_INPUT, "Could not open geodesic checkpoint file."};
  auto loaded = std::make_shared<bl_ctx::Checkpoint>();
  bl_ctx::Checkpoint &c = *loaded;
  for (double (&v)[4] : c.frame) in.read(reinterpret_cast<char *>(v), 4 * sizeof(double));
  const size_t n_pix = static_cast<size_t>(p.camera_resolution) * p.camera_resolution;
  ReadArray(in, &c.camera_pos);
  ReadArray(in, &c.camera_dir);
  ReadArray(in, &c.frequencies);
  ReadArray(in, &c.factors);
  in.read(reinterpret_cast<char *>(&c.num_steps), sizeof(int));
  ReadArray(in, &c.flags);
  ReadArray(in, &c.sample_num);
  ReadArray(in, &c.pos);
  ReadArray(in, &c.dir);
  ReadArray(in, &c.len);
  const size_t steps = static_cast<size_t>(std::max(c.num_steps, 0));
  if (c.camera_pos.size() != 4 * n_pix || c.camera_dir.size() != 4 * n_pix || c.factors.size() != n_pix || c.flags.size() != n_pix
      || c.sample_num.size() != n_pix || c.pos.size() != n_pix * steps * 4 || c.dir.size() != n_pix * steps * 4
      || c.len.size() != n_pix * steps || static_cast<int>(c.frequencies.size()) != p.image_num_frequencies || c.num_steps > p.ray_max_steps)
    throw Failure{BL_E_INPUT, "Geodesic checkpoint does not match this camera (resolution, frequencies or ray_max_steps)."};
  for (size_t m = 0; m < n_pix; m++)
    if (c.sample_num[m] < 0 || c.sample_num[m] > c.num_steps) throw Failure{BL_E_INPUT, "Geodesic checkpoint file is damaged."};
  return loaded;
}

// LoadGeodesics() for this context. The file's contents are shared between the contexts of a process that load the same file for the
// same camera (path, size, modification time, resolution, frequencies, ray_max_steps): the table holds weak references, so the
// memory goes when the last context that uses it does.
void LoadGeodesicCheckpoint(bl_ctx *ctx) {
  static std::mutex table_lock;
  static std::map<std::string, std::weak_ptr<const bl_ctx::Checkpoint>> table;
  const bl_params &p = ctx->params;
  struct stat info {};
  std::string key = p.checkpoint_geodesic_file.s;
  if (stat(p.checkpoint_geodesic_file.s, &info) == 0)
    key += "|" + std::to_string(static_cast<long long>(info.st_size)) + "|" + std::to_string(static_cast<long long>(info.st_mtim.tv_sec)) + "."
        + std::to_string(static_cast<long long>(info.st_mtim.tv_nsec)) + "|" + std::to_string(static_cast<long long>(info.st_ctim.tv_sec)) + "."
        + std::to_string(static_cast<long long>(info.st_ctim.tv_nsec)) + "|" + std::to_string(static_cast<long long>(info.st_ino));   // (a file rewritten in place within a second is another file)
  key += "|" + std::to_string(p.camera_resolution) + "|" + std::to_string(p.image_num_frequencies) + "|" + std::to_string(p.ray_max_steps);
  // (The table's lock covers the look-up only. Two contexts that ask for the same file for the first time at the same moment both read
  // it - tens of GB at 1024^2 - and the second keeps the first one's copy; a context that loads another file never waits behind them.)
  std::shared_ptr<const bl_ctx::Checkpoint> loaded;
  {
    std::lock_guard<std::mutex> guard(table_lock);
    loaded = table[key].lock();
  }
  if (!loaded) {
    std::shared_ptr<const bl_ctx::Checkpoint> mine = ReadGeodesicCheckpoint(p);
    std::lock_guard<std::mutex> guard(table_lock);
    loaded = table[key].lock();
    if (!loaded) {
      loaded = mine;
      table[key] = loaded;
    }
  }
  bl_camera_frame &f = ctx->frame;
  double *vectors[7] = {f.cam_x, f.u_con, f.u_cov, f.norm_con, f.norm_con_c, f.hor_con_c, f.vert_con_c};
  for (int v = 0; v < 7; v++) std::memcpy(vectors[v], loaded->frame[v], 4 * sizeof(double));
  ctx->block_frame = ctx->frame;   // (no camera list beside a loaded checkpoint: bl_set_cameras)
  ctx->frequencies = loaded->frequencies;   // LoadGeodesics() replaces what InitializeCamera() would have computed
  ctx->checkpoint = loaded;
}

// SaveGeodesics(), second half (geodesic_checkpoint.cpp:28-59)
void WriteGeodesicCheckpoint(const char *path, const bl_camera_frame &f, const double *frequencies, int n_nu, const std::vector<double> &camera_pos,
                             const std::vector<double> &camera_dir, const CheckpointSave &save) {
  std::ofstream out(path, std::ios_base::out | std::ios_base::binary);
  if (!out.is_open()) throw Failure{BL_E_INPUT, "Could not open geodesic checkpoint file."};
  const double *vectors[7] = {f.cam_x, f.u_con, f.u_cov, f.norm_con, f.norm_con_c, f.hor_con_c, f.vert_con_c};
  for (const double *v : vectors) out.write(reinterpret_cast<const char *>(v), 4 * sizeof(double));
  const int n_pix = static_cast<int>(save.sample_num.size());
  const int num_steps = MostSamples(save.sample_num);
  WriteArray(out, {4, n_pix}, camera_pos.data());
  WriteArray(out, {4, n_pix}, camera_dir.data());
  WriteArray(out, {n_nu}, frequencies);
  WriteArray(out, {n_pix}, save.factors.data());
  out.write(reinterpret_cast<const char *>(&num_steps), sizeof(int));
  WriteArray(out, {n_pix}, save.flags.data());
  WriteArray(out, {n_pix}, save.sample_num.data());
  WritePaddedRows(out, {4, num_steps, n_pix}, save.pos, save.offset, save.sample_num, num_steps, 4);
  WritePaddedRows(out, {4, num_steps, n_pix}, save.dir, save.offset, save.sample_num, num_steps, 4);
  WritePaddedRows(out, {num_steps, n_pix}, save.len, save.offset, save.sample_num, num_steps, 1);
  if (!out) throw Failure{BL_E_INPUT, "Could not write geodesic checkpoint file."};
}

// SaveSampling(), second half (sample_checkpoint.cpp:22-46): four Arrays
void WriteSampleCheckpoint(const char *path, const SampleSave &sv, bool block_interp, bool interp) {
  std::ofstream out(path, std::ios_base::out | std::ios_base::binary);
  if (!out.is_open()) throw Failure{BL_E_INPUT, "Could not open sample checkpoint file."};
  const int n_pix = static_cast<int>(sv.sample_num.size());
  const int num_steps = MostSamples(sv.sample_num);
  if (block_interp) WritePaddedRows(out, {4, 8, num_steps, n_pix}, sv.inds, sv.offset, sv.sample_num, num_steps, sv.per_sample);
  else WritePaddedRows(out, {4, num_steps, n_pix}, sv.inds, sv.offset, sv.sample_num, num_steps, sv.per_sample);
  if (interp) WritePaddedRows(out, {3, num_steps, n_pix}, sv.fracs, sv.offset, sv.sample_num, num_steps, 3);
  WritePaddedRows(out, {num_steps, n_pix}, sv.nan, sv.offset, sv.sample_num, num_steps, 1);
  WritePaddedRows(out, {num_steps, n_pix}, sv.fallback, sv.offset, sv.sample_num, num_steps, 1);
  if (!out) throw Failure{BL_E_INPUT, "Could not write sample checkpoint file."};
}

std::vector<double> GatherCameraRows(const std::vector<double> &source, const int *pixel_map, long long n_rays) {
  std::vector<double> rows(static_cast<size_t>(n_rays) * 4);
  for (long long ray = 0; ray < n_rays; ray++) {
    const size_t m = pixel_map != nullptr ? static_cast<size_t>(pixel_map[ray]) : static_cast<size_t>(ray);
    for (int mu = 0; mu < 4; mu++) rows[4 * ray + mu] = source[4 * m + mu];
  }
  return rows;
}

// LoadGeodesics(): the chunk's sample records come from the file instead of the geodesic kernel. The file holds them
// far -> near (ReverseGeodesics) with the renormalised momentum; records are near -> far, so sample n of a ray is entry
// num - 1 - n, and len = -sample_len.
HostChunk ChunkFromCheckpoint(const bl_ctx::Checkpoint &ck, const int *pixel_map, long long begin, int rays, long long record_gate) {
  const size_t steps = static_cast<size_t>(ck.num_steps);
  size_t total = 0;
  int taken = 0;
  for (; taken < rays; taken++) {
    const long long ray = begin + taken;
    const size_t m = pixel_map != nullptr ? static_cast<size_t>(pixel_map[ray]) : static_cast<size_t>(ray);
    const size_t num = static_cast<size_t>(ck.sample_num[m]);
    if (total + num > static_cast<size_t>(record_gate)) break;
    total += num;
  }
  if (taken == 0) throw Failure{BL_E_ARG, "Scratch budget too small for the samples of one checkpointed ray (bl_set_scratch_limit)."};
  HostChunk chunk;
  chunk.hot.reserve(total);
  chunk.cold.reserve(total);
  chunk.sample_t.reserve(total);
  for (int q = 0; q < taken; q++) {
    const long long ray = begin + q;
    const size_t m = pixel_map != nullptr ? static_cast<size_t>(pixel_map[ray]) : static_cast<size_t>(ray);
    const int num = ck.sample_num[m];
    chunk.kt.push_back(ck.camera_dir[4 * m]);
    chunk.factor.push_back(ck.factors[m]);
    chunk.sample_num.push_back(num);
    chunk.flags.push_back(ck.flags[m]);
    chunk.out_index.push_back(ray);
    chunk.offset.push_back(static_cast<long long>(chunk.hot.size()));
    for (int n = 0; n < num; n++) {
      const size_t at = m * steps + static_cast<size_t>(num - 1 - n);
      BlSampleHot h;
      h.x = ck.pos[4 * at + 1]; h.y = ck.pos[4 * at + 2]; h.z = ck.pos[4 * at + 3];
      h.ray = static_cast<uint32_t>(q);
      h.n = static_cast<uint32_t>(n);
      BlSampleCold c;
      c.kx = ck.dir[4 * at + 1]; c.ky = ck.dir[4 * at + 2]; c.kz = ck.dir[4 * at + 3];
      c.len = -ck.len[at];
      chunk.hot.push_back(h);
      chunk.cold.push_back(c);
      chunk.sample_t.push_back(ck.pos[4 * at]);
    }
  }
  return chunk;
}

// SaveGeodesics(), first half: a chunk's records, in the order its kernel wrote them, into the file's
void AddChunkToCheckpoint(HostChunk &chunk, const BlSpacetime &st, long long n_rays, CheckpointSave *out) {
  CheckpointSave &save = *out;
  save.flags.resize(n_rays);
  save.factors.resize(n_rays);
  const size_t packed = PlaceRays(chunk, save.len.size(), n_rays, &save.sample_num, &save.offset);
  for (size_t q = 0; q < chunk.sample_num.size(); q++) {
    const size_t m = static_cast<size_t>(chunk.out_index[q]);
    save.flags[m] = chunk.flags[q];
    save.factors[m] = chunk.factor[q];
  }
  save.pos.resize(4 * packed);
  save.dir.resize(4 * packed);
  save.len.resize(packed);
  for (size_t r = 0; r < chunk.hot.size(); r++) {
    const BlSampleHot &h = chunk.hot[r];
    if (h.ray == BL_DEAD_RAY) continue;
    const int num = chunk.sample_num[h.ray];
    if (static_cast<int>(h.n) >= num) continue;
    const BlSampleCold &c = chunk.cold[r];
    // ReverseGeodesics (geodesics.cpp:820-842) behind the per-sample renormalisation (:352-371)
    const size_t at = static_cast<size_t>(chunk.offset[h.ray]) + static_cast<size_t>(num - 1 - static_cast<int>(h.n));
    const double kt = chunk.kt[h.ray];
    const double factor = bl_renormalization_factor(st, h.x, h.y, h.z, kt, c.kx, c.ky, c.kz);
    save.pos[4 * at] = chunk.sample_t[r]; save.pos[4 * at + 1] = h.x; save.pos[4 * at + 2] = h.y; save.pos[4 * at + 3] = h.z;
    save.dir[4 * at] = kt; save.dir[4 * at + 1] = c.kx * factor; save.dir[4 * at + 2] = c.ky * factor; save.dir[4 * at + 3] = c.kz * factor;
    save.len[at] = -c.len;
  }
}

// SaveSampling(), first half: a chunk's located samples as the reference keeps them - sample_inds (MeshBlock, k, j, i of the nearest
// cell or of the lower corner; eight of them with inter-block interpolation), sample_fracs (f_k, f_j, f_i), sample_nan, sample_fallback
// (simulation_sampling.cpp:205-216, :377-384, :427-549) - by pixel and by the reversed sample index of ReverseGeodesics.
void AddChunkToSampleSave(HostChunk &chunk, const std::vector<BlLocated> &located, const std::vector<unsigned long long> &tags,
                          const std::vector<unsigned int> &anchors, bool interleaved, bool fast, bool block_interp, const bl_params &p,
                          const BlGridDevice &g, const int *merged_blocks, const std::vector<int> &merged_block_at, long long n_rays, SampleSave *sampling) {
  SampleSave &out = *sampling;
  const size_t stride = static_cast<size_t>(interleaved ? 2 : 1);
  out.per_sample = block_interp ? 32 : 4;
  const size_t packed = PlaceRays(chunk, out.nan.size(), n_rays, &out.sample_num, &out.offset);
  out.inds.resize(packed * out.per_sample, 0);
  if (p.simulation_interp) out.fracs.resize(packed * 3, 0.0);
  out.nan.resize(packed, 0);
  out.fallback.resize(packed, 0);
  // a cell of the HBM arrays as the reference names it: MeshBlock of the file, then k, j, i inside the block
  const size_t block_cells = static_cast<size_t>(g.nb[0]) * g.nb[1] * g.nb[2];
  auto name_cell = [&](unsigned int cell, int32_t *dst) {
    if (g.n_blocks > 0) {   // cells kept by MeshBlock
      const size_t b = cell / block_cells, rest = cell % block_cells;
      dst[0] = static_cast<int32_t>(b);
      dst[1] = static_cast<int32_t>(rest / g.stride_plane);
      dst[2] = static_cast<int32_t>(rest % g.stride_plane / g.stride_row);
      dst[3] = static_cast<int32_t>(rest % g.stride_row);
    } else {                // equal blocks merged into one array (one block: itself)
      const int i = static_cast<int>(cell % g.n[0]), j = static_cast<int>(cell / g.n[0] % g.n[1]), kk = static_cast<int>(cell / (static_cast<size_t>(g.n[0]) * g.n[1]));
      const int at = ((kk / g.nb[2]) * merged_blocks[1] + j / g.nb[1]) * merged_blocks[0] + i / g.nb[0];
      dst[0] = merged_block_at.empty() ? 0 : merged_block_at[at];
      dst[1] = kk % g.nb[2];
      dst[2] = j % g.nb[1];
      dst[3] = i % g.nb[0];
    }
  };
  for (size_t r = 0; r < located.size(); r++) {
    const BlSampleHot &h = chunk.hot[r * stride];
    if (h.ray == BL_DEAD_RAY) continue;
    const int num = chunk.sample_num[h.ray];
    if (static_cast<int>(h.n) >= num) continue;
    const size_t at = static_cast<size_t>(chunk.offset[h.ray]) + static_cast<size_t>(num - 1 - static_cast<int>(h.n));
    if (p.fallback_nan && chunk.flags[h.ray] != 0) {   // a poorly terminated geodesic samples NaN everywhere (:211-216)
      out.nan[at] = 1;
      continue;
    }
    unsigned long long tag = tags[r];
    if (fast) std::memcpy(&tag, &located[r].ph, sizeof tag);   // tolerant tier: the tag rides in the azimuth's slot
    const int status = static_cast<int>(tag >> 32) & 0xff;
    if (status == 2) {                 // off the grid (:377-384)
      (p.fallback_nan ? out.nan : out.fallback)[at] = 1;
    } else if (status == 3 || status == 4) {   // nearest cell | lower corner of the trilinear stencil
      name_cell(static_cast<unsigned int>(tag), &out.inds[at * out.per_sample]);
    } else if (status == 6) {          // inter-block interpolation: the eight anchors (:541)
      for (int c = 0; c < 8; c++) name_cell(anchors[r * 8 + c], &out.inds[at * out.per_sample + 4 * c]);
    }
    if (p.simulation_interp && (status == 4 || status == 6)) {
      out.fracs[3 * at] = located[r].f_k;
      out.fracs[3 * at + 1] = located[r].f_j;
      out.fracs[3 * at + 2] = located[r].f_i;
    }
  }
}

}  // namespace blhost
