// bl_host.cpp - the two host-side steps that sit between and after GPU renders, kept on the host as
// in the reference: the adaptive refinement decision (src/radiation_integrator/
// radiation_adaptive.cpp:19-312 + the block bookkeeping of camera.cpp:445-458) and the output writer
// (src/output_writer/output_writer.cpp:169-316, numpy_format.cpp, zip_format.cpp, raw_format.cpp).
// The .npy / ZIP byte layout is the reference's (NumPy .npy v1.0 with a 128-byte header, ZIP 2.0
// stored entries with CRC-32), so its plotting scripts read the files unchanged.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <ctime>
#include <fcntl.h>
#include <unistd.h>

#include <fstream>
#include <thread>
#include <string>
#include <vector>

#include "bl_internal.h"
#include "bl_refine.h"
#include "blmath.h"

namespace {

// ------------------------------------------------------------------ adaptive refinement
// EvaluateBlock (radiation_adaptive.cpp:163-312). q(row, col) = intensity of the block. The criteria's arithmetic is bl_refine.h's,
// which the device call (bl_refine.hip) shares.
bool EvaluateBlock(const BlRefineCuts &cuts, const double *block, int bs) {
  auto q_at = [&](int i, int j) { return block[i * bs + j]; };
  for (int c = 0; c < BL_REFINE_CRITERIA; c++) {
    if (!(cuts.frac[c] >= 0.0)) continue;
    const int margin = bl_refine_margin(c);
    int num_examined = 0, num_exceeded = 0;
    for (int i = margin; i < bs - margin; i++)
      for (int j = margin; j < bs - margin; j++) {
        double q = bl_refine_examined(c, q_at, i, j, bs);
        if (!bl_refine_counts(q)) continue;
        num_examined++;
        if (q > cuts.cut[c]) num_exceeded++;
      }
    if (bl_refine_verdict(num_exceeded, num_examined, cuts.frac[c])) return true;
  }
  return false;
}

// ------------------------------------------------------------------ .npy / ZIP
using Bytes = std::vector<uint8_t>;

// NumPy .npy v1.0 with the reference's fixed 128-byte header (numpy_format.cpp:604-664); empty if the shape does not fit
Bytes MakeNpyHeader(const char *descr, const std::vector<int> &shape) {
  const size_t header_length = 128;
  Bytes out(header_length);
  std::memcpy(out.data(), "\x93NUMPY\x01\x00", 8);
  uint16_t header_len = static_cast<uint16_t>(header_length - 10);
  std::memcpy(out.data() + 8, &header_len, 2);
  std::string dict = std::string("{'descr': '") + descr + "', 'fortran_order': False, 'shape': (";
  for (size_t i = 0; i < shape.size(); i++) {
    dict += std::to_string(shape[i]);
    if (shape.size() == 1) dict += ",";
    else if (i + 1 < shape.size()) dict += ", ";
  }
  dict += ")}";
  if (dict.size() > header_length - 11) return Bytes();
  std::memset(out.data() + 10, ' ', header_length - 11);
  std::memcpy(out.data() + 10, dict.data(), dict.size());
  out[header_length - 1] = '\n';
  return out;
}

// One array on its way into a file: the .npy header and the data where they lie (the caller's image rows) or, where the
// reference reorders them (Stokes components, cell averages) or they are locals, a copy. Nothing is assembled in memory:
// a 4096^2 x 64-frequency I_nu record (8.6 GB) is checksummed and written straight from the image.
struct NpyRecord {
  std::string name;
  Bytes head;
  const uint8_t *data = nullptr;
  size_t data_bytes = 0;
  Bytes owned;
  size_t size() const { return head.size() + data_bytes; }
};

// Standard CRC-32 (what zip_format.cpp:284-360 computes with its bit-reversed tables), eight bytes per step
uint32_t Crc32Update(uint32_t crc, const uint8_t *data, size_t n) {
  static uint32_t table[8][256];
  static bool ready = false;
  if (!ready) {
    for (uint32_t i = 0; i < 256; i++) {
      uint32_t c = i;
      for (int k = 0; k < 8; k++) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
      table[0][i] = c;
    }
    for (uint32_t i = 0; i < 256; i++)
      for (int t = 1; t < 8; t++) table[t][i] = table[0][table[t - 1][i] & 0xFFu] ^ (table[t - 1][i] >> 8);
    ready = true;
  }
  crc ^= 0xFFFFFFFFu;
  size_t i = 0;
  for (; i + 8 <= n; i += 8) {
    uint32_t lo, hi;
    std::memcpy(&lo, data + i, 4);
    std::memcpy(&hi, data + i + 4, 4);
    lo ^= crc;
    crc = table[7][lo & 0xFFu] ^ table[6][(lo >> 8) & 0xFFu] ^ table[5][(lo >> 16) & 0xFFu] ^ table[4][lo >> 24]
        ^ table[3][hi & 0xFFu] ^ table[2][(hi >> 8) & 0xFFu] ^ table[1][(hi >> 16) & 0xFFu] ^ table[0][hi >> 24];
  }
  for (; i < n; i++) crc = table[0][(crc ^ data[i]) & 0xFFu] ^ (crc >> 8);
  return crc ^ 0xFFFFFFFFu;
}

// CRC-32 of the concatenation A | B from crc(A), crc(B) and the length of B: the CRC register is linear over GF(2), so appending
// len_b zero bytes to A is a 32 x 32 bit matrix applied to crc(A) - the matrix for one zero byte squared up along the bits of len_b -
// and crc(A | B) = that ^ crc(B). (The construction zlib's crc32_combine uses; written out here from the algebra.)
uint32_t Gf2Times(const uint32_t *matrix, uint32_t vec) {
  uint32_t sum = 0;
  for (int bit = 0; vec != 0; vec >>= 1, bit++)
    if (vec & 1u) sum ^= matrix[bit];
  return sum;
}
void Gf2Square(uint32_t *square, const uint32_t *matrix) {
  for (int n = 0; n < 32; n++) square[n] = Gf2Times(matrix, matrix[n]);
}
uint32_t Crc32Combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) {
  if (len_b == 0) return crc_a;
  uint32_t even[32], odd[32];
  odd[0] = 0xEDB88320u;   // the register's shift by one zero BIT: the polynomial, then the identity shifted
  for (int n = 1; n < 32; n++) odd[n] = 1u << (n - 1);
  Gf2Square(even, odd);   // two bits
  Gf2Square(odd, even);   // four bits
  do {                     // eight bits = one byte on the first pass, then squared per bit of len_b
    Gf2Square(even, odd);
    if (len_b & 1u) crc_a = Gf2Times(even, crc_a);
    len_b >>= 1;
    if (len_b == 0) break;
    Gf2Square(odd, even);
    if (len_b & 1u) crc_a = Gf2Times(odd, crc_a);
    len_b >>= 1;
  } while (len_b != 0);
  return crc_a ^ crc_b;
}

// Host threads for the byte work on large records (a 4096^2 x 64 image is 8.6 GB: one thread took 3.9 s for its CRC, round 5)
int ByteWorkers(size_t bytes) {
  if (bytes < (32u << 20)) return 1;
  const unsigned int cores = std::thread::hardware_concurrency();
  return static_cast<int>(std::min<size_t>(std::min<unsigned int>(cores == 0 ? 4 : cores, 16), bytes >> 24));
}

// ... of a large array: slices in parallel, combined in order
uint32_t Crc32Large(uint32_t crc, const uint8_t *data, size_t n) {
  const int workers = ByteWorkers(n);
  if (workers <= 1) return Crc32Update(crc, data, n);
  (void)Crc32Update(0, data, 0);   // (the tables, before the threads race to build them)
  const size_t share = (n + workers - 1) / workers;
  std::vector<uint32_t> part(workers, 0);
  std::vector<std::thread> pool;
  for (int t = 0; t < workers; t++)
    pool.emplace_back([&, t]() {
      const size_t first = std::min(n, share * t), last = std::min(n, share * (t + 1));
      part[t] = Crc32Update(0, data + first, last - first);
    });
  for (std::thread &t : pool) t.join();
  for (int t = 0; t < workers; t++) {
    const size_t first = std::min(n, share * t), last = std::min(n, share * (t + 1));
    crc = Crc32Combine(crc, part[t], last - first);
  }
  return crc;
}

uint32_t Crc32(const NpyRecord &r) { return Crc32Large(Crc32Update(0, r.head.data(), r.head.size()), r.data, r.data_bytes); }

template <typename T>
void Put(Bytes *b, T v) {
  const uint8_t *p = reinterpret_cast<const uint8_t *>(&v);
  b->insert(b->end(), p, p + sizeof(T));
}

// zip_format.cpp:26-110
// zip64: the record carries its sizes in a ZIP64 extended-information field (APPNOTE 4.5.3) - beyond the reference, which
// stops at 4 GiB (numpy_format.cpp:44-45); used only where 32 bits do not hold the size (or when forced, for the tests)
bool MakeLocalHeader(const std::string &name, const NpyRecord &record, bool zip64, Bytes *header) {
  if (record.size() > UINT32_MAX && !zip64) return false;
  std::string full = name + ".npy";
  header->clear();
  header->insert(header->end(), {0x50, 0x4b, 0x03, 0x04});
  Put<uint8_t>(header, zip64 ? 45 : 20);   // version needed 2.0 (4.5 with ZIP64 fields)
  Put<uint8_t>(header, 0);
  Put<uint16_t>(header, 0);   // flags
  Put<uint16_t>(header, 0);   // stored
  std::time_t now = std::time(nullptr);
  std::tm *lt = std::localtime(&now);
  uint16_t time = static_cast<uint16_t>(lt->tm_hour << 11);
  time |= static_cast<uint16_t>((lt->tm_min & 0x1F) << 5);
  time |= static_cast<uint16_t>(lt->tm_sec / 2 & 0x1F);
  uint16_t date = static_cast<uint16_t>((lt->tm_year - 80) << 9);
  date |= static_cast<uint16_t>(((lt->tm_mon + 1) & 0xF) << 5);
  date |= static_cast<uint16_t>(lt->tm_mday & 0x1F);
  Put<uint16_t>(header, time);
  Put<uint16_t>(header, date);
  Put<uint32_t>(header, Crc32(record));
  Put<uint32_t>(header, zip64 ? 0xFFFFFFFFu : static_cast<uint32_t>(record.size()));
  Put<uint32_t>(header, zip64 ? 0xFFFFFFFFu : static_cast<uint32_t>(record.size()));
  Put<uint16_t>(header, static_cast<uint16_t>(full.size()));
  Put<uint16_t>(header, zip64 ? 20 : 0);
  header->insert(header->end(), full.begin(), full.end());
  if (zip64) {
    Put<uint16_t>(header, 0x0001);
    Put<uint16_t>(header, 16);
    Put<uint64_t>(header, record.size());   // uncompressed, then compressed
    Put<uint64_t>(header, record.size());
  }
  return true;
}

// zip_format.cpp:122-190
Bytes MakeCentralHeader(const Bytes &local, size_t offset, bool zip64, size_t record_size) {
  Bytes out = {0x50, 0x4b, 0x01, 0x02};
  Put<uint8_t>(&out, zip64 ? 45 : 20);   // version made by 2.0 (4.5 with ZIP64 fields)
  Put<uint8_t>(&out, 3);    // unix
  if (!zip64) {
    out.insert(out.end(), local.begin() + 4, local.begin() + 30);
  } else {
    out.insert(out.end(), local.begin() + 4, local.begin() + 28);   // ... up to the name length
    Put<uint16_t>(&out, 28);                                           // extra: sizes and the offset of the local header
  }
  Put<uint16_t>(&out, 0);   // comment length
  Put<uint16_t>(&out, 0);   // disk number
  Put<uint16_t>(&out, 0);   // internal attributes
  Put<uint32_t>(&out, 0x81800000u);
  Put<uint32_t>(&out, zip64 ? 0xFFFFFFFFu : static_cast<uint32_t>(offset));
  uint16_t name_length;
  std::memcpy(&name_length, local.data() + 26, 2);
  out.insert(out.end(), local.begin() + 30, local.begin() + 30 + name_length);
  if (zip64) {
    Put<uint16_t>(&out, 0x0001);
    Put<uint16_t>(&out, 24);
    Put<uint64_t>(&out, record_size);
    Put<uint64_t>(&out, record_size);
    Put<uint64_t>(&out, offset);
  }
  return out;
}

// output_writer.cpp:283-316
bool FormatFilename(const std::string &pattern, int file_number, std::string *out) {
  std::string::size_type open = pattern.find_first_of('{');
  if (open == std::string::npos) return false;
  std::string::size_type close = pattern.find_first_of('}', open);
  if (close == std::string::npos) return false;
  if (pattern[close - 1] != 'd') return false;
  int field_length = 0;
  if (close - open > 2) field_length = std::atoi(pattern.substr(open + 1, close - open - 2).c_str());
  std::string number = std::to_string(file_number);
  std::string zeros;
  if (static_cast<int>(number.size()) < field_length) zeros.assign(field_length - number.size(), '0');
  *out = pattern.substr(0, open) + zeros + number + pattern.substr(close + 1);
  return true;
}

}  // namespace

// ------------------------------------------------------------------ what bl_adaptive_refine and bl_adaptive_refine_device share (bl_refine.h)
// The refusals and checks of both entry points, with the texts of bl_adaptive_refine. BL_OK: *plan is filled.
int bl_refine_plan(bl_ctx *ctx, int level, int n_blocks, const int32_t *block_locs, int32_t *n_refined, BlRefinePlan *plan) {
  if (bl_num_electron_models(ctx) >= 2)
    return bl_internal_fail(ctx, BL_E_UNSUPPORTED, "bl_adaptive_refine reads one image: not with two or more electron models (bl_set_electron_models).");
  if (bl_num_density_units(ctx) >= 2)
    return bl_internal_fail(ctx, BL_E_UNSUPPORTED, "bl_adaptive_refine reads one image: not with two or more density units (bl_set_density_units).");
  if (bl_num_polarized_variants(ctx) >= 2)
    return bl_internal_fail(ctx, BL_E_UNSUPPORTED, "bl_adaptive_refine reads one image: not with two or more polarized variants (bl_set_polarized_variants).");
  if (bl_num_sigma_cuts(ctx) >= 2)
    return bl_internal_fail(ctx, BL_E_UNSUPPORTED, "bl_adaptive_refine reads one image: not with two or more sigma cuts (bl_set_sigma_cuts).");
  if (bl_num_cameras(ctx) >= 2)
    return bl_internal_fail(ctx, BL_E_UNSUPPORTED, "bl_adaptive_refine reads one image: not with two or more cameras (bl_set_cameras).");
  if (bl_num_electron_mixes(ctx) >= 2)
    return bl_internal_fail(ctx, BL_E_UNSUPPORTED, "bl_adaptive_refine reads one image: not with two or more electron mixes (bl_set_electron_mixes).");
  const bl_params &p = *bl_internal_params(ctx);
  *n_refined = 0;
  *plan = BlRefinePlan{};
  if (p.adaptive_max_level <= 0 || level >= p.adaptive_max_level) return BL_OK;
  plan->decide = true;
  plan->bs = p.adaptive_block_size;
  plan->res = p.camera_resolution;
  plan->root = p.camera_resolution / plan->bs;
  if (level == 0 && n_blocks != plan->root * plan->root)
    return bl_internal_fail(ctx, BL_E_ARG, "Level 0 must be evaluated with all root blocks.");
  if (level > 0 && block_locs == nullptr) return bl_internal_fail(ctx, BL_E_ARG, "Refined levels need block_locs.");
  plan->linear_num_blocks = plan->root;
  for (int n = 1; n <= level; n++) plan->linear_num_blocks *= 2;
  plan->n_pix = level == 0 ? static_cast<long long>(p.camera_resolution) * p.camera_resolution
                           : static_cast<long long>(n_blocks) * plan->bs * plan->bs;
  // row of I_nu at the chosen frequency (radiation_adaptive.cpp:166-167): rows 4 l + (I, Q, U, V) when polarized
  // (of the context's frequencies: bl_set_frequencies' list where one is set, whose length the setter held adaptive_frequency_num to)
  int n_nu = 0;
  (void)bl_internal_frequencies(ctx, &n_nu);
  const int freq_index = n_nu > 1 ? p.adaptive_frequency_num - 1 : 0;
  const bool polarized = p.model_type == BL_MODEL_SIMULATION && p.image_light && p.has[BL_P_image_polarization] && p.image_polarization;
  plan->row = static_cast<size_t>(freq_index) * (polarized ? 4 : 1);
  plan->camera_width = p.camera_width;
  const double cut[BL_REFINE_CRITERIA] = {p.adaptive_val_cut, p.adaptive_abs_grad_cut, p.adaptive_rel_grad_cut, p.adaptive_abs_lapl_cut, p.adaptive_rel_lapl_cut};
  const double frac[BL_REFINE_CRITERIA] = {p.adaptive_val_frac, p.adaptive_abs_grad_frac, p.adaptive_rel_grad_frac, p.adaptive_abs_lapl_frac, p.adaptive_rel_lapl_frac};
  for (int c = 0; c < BL_REFINE_CRITERIA; c++) {
    plan->cuts.cut[c] = cut[c];
    plan->cuts.frac[c] = frac[c];
  }
  plan->regions.count = p.adaptive_num_regions > 0 ? p.adaptive_num_regions : 0;
  for (int r = 0; r < plan->regions.count; r++) {
    plan->regions.level[r] = p.adaptive_region_level[r];
    plan->regions.x_min[r] = p.adaptive_region_x_min[r];
    plan->regions.x_max[r] = p.adaptive_region_x_max[r];
    plan->regions.y_min[r] = p.adaptive_region_y_min[r];
    plan->regions.y_max[r] = p.adaptive_region_y_max[r];
  }
  return BL_OK;
}

// The next level's list from the flags (camera.cpp:453-458): parents in order, each with its four children; returns the parents' count
int bl_refine_children(const BlRefinePlan &plan, int level, int n_blocks, const int32_t *block_locs, const uint8_t *refine_flags,
                              int32_t *next_locs) {
  int count = 0;
  for (int b = 0; b < n_blocks; b++) {
    if (!refine_flags[b]) continue;
    if (next_locs != nullptr) {
      int loc_v, loc_u;
      bl_refine_block_loc(plan, level, b, block_locs, &loc_v, &loc_u);
      int32_t *dst = next_locs + static_cast<size_t>(count) * 8;
      int k = 0;
      for (int v = 2 * loc_v; v <= 2 * loc_v + 1; v++)
        for (int u = 2 * loc_u; u <= 2 * loc_u + 1; u++) {
          dst[2 * k + 0] = v;
          dst[2 * k + 1] = u;
          k++;
        }
    }
    count++;
  }
  return count;
}

extern "C" {

int bl_adaptive_refine(const bl_ctx *ctx_const, int level, int n_blocks, const int32_t *block_locs,
                       const double *image, uint8_t *refine_flags, int32_t *n_refined, int32_t *next_locs) {
  bl_ctx *ctx = const_cast<bl_ctx *>(ctx_const);
  if (ctx == nullptr || image == nullptr || refine_flags == nullptr || n_refined == nullptr) return BL_E_ARG;
  BlRefinePlan plan;
  if (int rc = bl_refine_plan(ctx, level, n_blocks, block_locs, n_refined, &plan)) return rc;
  if (!plan.decide) {
    for (int b = 0; b < n_blocks; b++) refine_flags[b] = 0;
    return BL_OK;
  }
  const int bs = plan.bs;
  const int block_num_pix = bs * bs;
  const double *row = image + plan.row * static_cast<size_t>(plan.n_pix);
  std::vector<double> block(block_num_pix);
  for (int b = 0; b < n_blocks; b++) {
    int loc_v, loc_u;
    bl_refine_block_loc(plan, level, b, block_locs, &loc_v, &loc_u);
    bool flag = bl_refine_forced(plan.regions, level, loc_v, loc_u, plan.linear_num_blocks, plan.camera_width);
    if (!flag) {
      if (level == 0) {
        const int j0 = loc_v * bs, i0 = loc_u * bs;
        for (int j = 0; j < bs; j++)
          for (int i = 0; i < bs; i++) block[j * bs + i] = row[static_cast<size_t>(j0 + j) * plan.res + i0 + i];
      } else {
        std::memcpy(block.data(), row + static_cast<size_t>(b) * block_num_pix, sizeof(double) * block_num_pix);
      }
      flag = EvaluateBlock(plan.cuts, block.data(), bs);
    }
    refine_flags[b] = flag ? 1 : 0;
  }
  const int count = bl_refine_children(plan, level, n_blocks, block_locs, refine_flags, next_locs);
  *n_refined = count;
  return BL_OK;
}

}  // extern "C"

namespace {

// The file's name (output_writer.cpp:283-316 for a series) and, for one image of several, its tag (include/blacklight_amd.h)
// (frequency >= 0: the file of one frequency, bl_write_output_frequency - its tag fFF whatever the list's length)
int OutputPath(bl_ctx *ctx, int snapshot, int variant, int n_variants, int camera, int n_cameras, std::string *path, int frequency = -1) {
  const bl_params &p = *bl_internal_params(ctx);
  if (!p.has[BL_P_output_file]) return bl_internal_fail(ctx, BL_E_MISSING, "OutputWriter unable to find all needed values in input file.");
  *path = p.output_file.s;
  if (p.model_type == BL_MODEL_SIMULATION && p.simulation_multiple) {
    int file_number = snapshot + (p.slow_light_on ? p.slow_offset : p.simulation_start);
    if (!FormatFilename(p.output_file.s, file_number, path))
      return bl_internal_fail(ctx, BL_E_INPUT, "Invalid output_file for multiple runs.");
  }
  if (n_variants < 2 && n_cameras < 2 && frequency < 0) return BL_OK;
  // (the camera's tag in front of the frequency's, that in front of the variant's, inside one dot group: .c01m00u02, .c01f02m00u02)
  char camera_tag[32] = "", tag[32] = "";
  if (n_cameras >= 2) std::snprintf(camera_tag, sizeof camera_tag, "c%02d", camera);
  if (frequency >= 0) std::snprintf(camera_tag + std::strlen(camera_tag), sizeof camera_tag - std::strlen(camera_tag), "f%02d", frequency);
  const bl_variant_place at = bl_internal_variant_place(ctx, variant);
  if (n_variants < 2) {
  } else if (at.polarized) {
    std::snprintf(tag, sizeof tag, "v%02d", variant);
  } else {
    // (the cut's tag only where cuts are set, the mix's - in front - only where mixes are: names without either are as ever)
    char mix_tag[8] = "", cut_tag[8] = "";
    if (at.mixes_set) std::snprintf(mix_tag, sizeof mix_tag, "e%02d", at.e);
    if (at.cuts_set) std::snprintf(cut_tag, sizeof cut_tag, "s%02d", at.s);
    std::snprintf(tag, sizeof tag, "%sm%02du%02d%s", mix_tag, at.m, at.u, cut_tag);
  }
  const std::string group = std::string(".") + camera_tag + tag;
  const std::string::size_type slash = path->find_last_of('/');
  const std::string::size_type dot = path->find_last_of('.');
  if (dot == std::string::npos || (slash != std::string::npos && dot < slash)) path->append(group);
  else path->insert(dot, group);
  return BL_OK;
}

// bl_write_output, bl_write_output_variant and bl_write_output_camera: image `variant` of the n_variants the root level's rows hold, and
// of every row and record the slice of `camera` of the n_cameras that lie side by side in it
// (frequency >= 0: the one-frequency file of that entry of the context's frequencies - bl_write_output_frequency, which has held the index
// to the list and refused adaptive levels beside two frequencies or more)
int WriteOutput(bl_ctx *ctx, const char *path_override, const bl_output_desc *d_given, int variant, int n_variants, int camera = 0, int n_cameras = 1,
                int frequency = -1) {
  const bl_output_desc *d = d_given;
  if (d->level[0].image == nullptr && bl_image_num_quantities(ctx) > 0) return bl_internal_fail(ctx, BL_E_ARG, "bl_write_output needs the root image.");
  // Several cameras: the camera's share of the variant's rows, of the renderings and of the camera records, as the one-camera
  // arrays everything below expects (rows of C res^2 entries -> rows of res^2; the records of a camera lie together already)
  bl_output_desc sliced;
  std::vector<double> camera_image, camera_render;
  if (n_cameras >= 2) {
    const bl_params &pp = *bl_internal_params(ctx);
    const size_t pixels = static_cast<size_t>(pp.camera_resolution) * pp.camera_resolution, stride = pixels * n_cameras;
    const size_t rows = static_cast<size_t>(bl_image_num_quantities(ctx) / n_variants), render_rows = static_cast<size_t>(bl_render_num_images(ctx)) * 3;
    sliced = *d;
    if (d->level[0].image != nullptr) {
      camera_image.resize(rows * pixels);
      const double *from = d->level[0].image + static_cast<size_t>(variant) * rows * stride + camera * pixels;
      for (size_t q = 0; q < rows; q++) std::memcpy(camera_image.data() + q * pixels, from + q * stride, pixels * sizeof(double));
      sliced.level[0].image = camera_image.data();
    }
    if (d->level[0].render != nullptr) {
      camera_render.resize(render_rows * pixels);
      for (size_t q = 0; q < render_rows; q++)
        std::memcpy(camera_render.data() + q * pixels, d->level[0].render + q * stride + camera * pixels, pixels * sizeof(double));
      sliced.level[0].render = camera_render.data();
    }
    if (d->level[0].camera != nullptr) sliced.level[0].camera = d->level[0].camera + static_cast<size_t>(camera) * pixels * 4;
    d = &sliced;
  }
  int row_variant = n_cameras >= 2 ? 0 : variant;   // (a camera's slice holds the one variant's rows alone)
  const bl_params &p = *bl_internal_params(ctx);
  const bl_camera_frame &frame = *bl_internal_frame(ctx);
  int n_nu = 0;
  const double *frequencies = bl_internal_frequencies(ctx, &n_nu);
  const int res = p.camera_resolution;
  int n_q = bl_image_num_quantities(ctx) / n_variants;
  const size_t n_pix = static_cast<size_t>(res) * res;
  // One frequency of several: the variant's rows of that frequency, in the order of a block with image_num_frequencies = 1
  // (radiation_integrator.cpp:436-520: Stokes rows 4 l + a, then time, length, lambda, emission, tau by frequency, the cell values
  // 7 l + n, crossings), gathered into one block; everything below then writes a one-frequency context's file
  std::vector<double> frequency_image;
  if (frequency >= 0 && n_nu >= 2) {
    const bool sim = p.model_type == BL_MODEL_SIMULATION;
    const int stride = (sim && p.image_light && p.has[BL_P_image_polarization] && p.image_polarization) ? 4 : 1;
    std::vector<int> rows;
    int at = 0;
    const auto take = [&](bool on, int per_frequency, bool has_axis) {   // a quantity's rows: per_frequency for every frequency, or that many in all
      if (!on) return;
      for (int k = 0; k < per_frequency; k++) rows.push_back(at + (has_axis ? frequency * per_frequency : 0) + k);
      at += has_axis ? n_nu * per_frequency : per_frequency;
    };
    take(p.image_light, stride, true);
    take(p.image_time, 1, false);
    take(p.image_length, 1, false);
    take(p.image_lambda, 1, true);
    take(p.image_emission, 1, true);
    take(p.image_tau, 1, true);
    take(sim && p.image_lambda_ave, 7, true);
    take(sim && p.image_emission_ave, 7, true);
    take(sim && p.image_tau_int, 7, true);
    take(p.image_crossings, 1, false);
    if (at != n_q) return bl_internal_fail(ctx, BL_E_STATE, "bl_write_output_frequency: the image rows do not add up to bl_image_num_quantities.");
    if (d->level[0].image != nullptr) {
      const double *from = d->level[0].image + static_cast<size_t>(row_variant) * n_q * n_pix;
      frequency_image.resize(rows.size() * n_pix);
      for (size_t q = 0; q < rows.size(); q++) std::memcpy(frequency_image.data() + q * n_pix, from + static_cast<size_t>(rows[q]) * n_pix, n_pix * sizeof(double));
      if (d != &sliced) sliced = *d;
      sliced.level[0].image = frequency_image.data();
      d = &sliced;
    }
    row_variant = 0;
    n_q = static_cast<int>(rows.size());
    frequencies += frequency;
    n_nu = 1;
  }

  std::string path;
  if (path_override != nullptr && path_override[0] != '\0') {
    path = path_override;
  } else {
    const int rc = OutputPath(ctx, d->snapshot, variant, n_variants, camera, n_cameras, &path, frequency);
    if (rc != BL_OK) return rc;
  }
  std::ofstream stream(path, std::ios_base::out | std::ios_base::binary);
  if (!stream.is_open()) return bl_internal_fail(ctx, BL_E_INPUT, "Could not open output file.");

  if (bl_render_num_images(ctx) > 0 && p.output_format != BL_OUTPUT_NPZ)
    return bl_internal_fail(ctx, BL_E_INPUT, "Only npz outputs support rendering.");
  const double *image0 = d->level[0].image == nullptr ? nullptr : d->level[0].image + static_cast<size_t>(row_variant) * n_q * n_pix;
  if (p.output_format == BL_OUTPUT_RAW && p.model_type == BL_MODEL_SIMULATION && p.image_light && p.has[BL_P_image_polarization]
      && p.image_polarization)   // output_writer.cpp:64-70
    return bl_internal_fail(ctx, BL_E_INPUT, "Only npz or npy outputs support polarization.");
  if (p.output_format == BL_OUTPUT_RAW) {   // raw_format.cpp: the bytes of image[0]
    stream.write(reinterpret_cast<const char *>(image0), static_cast<std::streamsize>(sizeof(double) * n_q * n_pix));
    return BL_OK;
  }
  if (p.output_format == BL_OUTPUT_NPY) {   // numpy_format.cpp:19-32: image[0] as (n_q, res, res)
    Bytes head = MakeNpyHeader("<f8", {n_q, res, res});
    stream.write(reinterpret_cast<const char *>(head.data()), static_cast<std::streamsize>(head.size()));
    stream.write(reinterpret_cast<const char *>(image0), static_cast<std::streamsize>(sizeof(double) * n_q * n_pix));
    return BL_OK;
  }

  // npz (numpy_format.cpp:46-584), records in the reference's order
  std::vector<NpyRecord> records;
  // copy: the data are a local or a reordered temporary; otherwise they stay where the caller holds them
  auto add = [&](const std::string &name, const char *descr, const std::vector<int> &shape, const void *data, size_t bytes, bool copy) {
    NpyRecord r;
    r.name = name;
    r.head = MakeNpyHeader(descr, shape);
    r.data_bytes = bytes;
    if (copy) r.owned.assign(static_cast<const uint8_t *>(data), static_cast<const uint8_t *>(data) + bytes);
    else r.data = static_cast<const uint8_t *>(data);
    records.push_back(std::move(r));
  };
  double mass_msun = frame.mass_msun;
  double width = p.camera_width;
  int32_t num_levels = d->adaptive_num_levels;
  add("mass_msun", "<f8", {1}, &mass_msun, 8, true);
  add("width", "<f8", {1}, &width, 8, true);
  add("frequency", "<f8", {n_nu}, frequencies, sizeof(double) * n_nu, true);
  add("adaptive_num_levels", "<i4", {1}, &num_levels, 4, true);
  if (p.adaptive_max_level > 0) {
    std::vector<int32_t> counts(num_levels + 1);
    counts[0] = (res / p.adaptive_block_size) * (res / p.adaptive_block_size);
    for (int l = 1; l <= num_levels; l++) counts[l] = d->level[l].n_blocks;
    add("adaptive_num_blocks", "<i4", {num_levels + 1}, counts.data(), 4 * counts.size(), true);
  }
  const char *camera_name = p.camera_type == BL_CAMERA_PLANE ? "positions" : "directions";
  if (p.output_camera) {
    if (d->level[0].camera == nullptr) return bl_internal_fail(ctx, BL_E_ARG, "output_camera needs camera data.");
    add(camera_name, "<f8", {res, res, 4}, d->level[0].camera, sizeof(double) * n_pix * 4, false);
  }
  // Stokes rows (numpy_format.cpp:128-165): row (l * stride + a) of the image -> record a, slice l
  const bool polarized = p.model_type == BL_MODEL_SIMULATION && p.image_light && p.has[BL_P_image_polarization] && p.image_polarization;
  const int stokes_stride = polarized ? 4 : 1;
  static const char *const kStokesNames[4] = {"I_nu", "Q_nu", "U_nu", "V_nu"};
  std::vector<double> stokes;
  auto add_stokes = [&](const double *image, size_t pixels, const std::vector<int> &pixel_shape, const std::string &prefix,
                        const std::string &suffix) {
    std::vector<int> shape = pixel_shape;
    if (n_nu > 1) shape.insert(shape.begin(), n_nu);
    if (stokes_stride == 1) {   // unpolarized: the rows are the record
      add(prefix + kStokesNames[0] + suffix, "<f8", shape, image, sizeof(double) * n_nu * pixels, false);
      return;
    }
    for (int a = 0; a < stokes_stride; a++) {
      stokes.resize(static_cast<size_t>(n_nu) * pixels);
      for (int l = 0; l < n_nu; l++)
        std::memcpy(stokes.data() + static_cast<size_t>(l) * pixels, image + static_cast<size_t>(l * stokes_stride + a) * pixels,
                    sizeof(double) * pixels);
      add(prefix + kStokesNames[a] + suffix, "<f8", shape, stokes.data(), sizeof(double) * n_nu * pixels, true);
    }
  };
  if (p.image_light) add_stokes(image0, n_pix, {res, res}, "", "");
  // alternate images (numpy_format.cpp:167-281) and renderings (:282-289), root level
  const bool simulation = p.model_type == BL_MODEL_SIMULATION;
  const int n_render = bl_render_num_images(ctx);
  struct RowSet { const char *name; bool on; int offset; bool per_frequency; bool per_cell; };
  int row = p.image_light ? n_nu * stokes_stride : 0;
  auto take = [&](bool on, int count) { int at = row; if (on) row += count; return at; };
  const int off_time = take(p.image_time, 1), off_length = take(p.image_length, 1), off_lambda = take(p.image_lambda, n_nu);
  const int off_emission = take(p.image_emission, n_nu), off_tau = take(p.image_tau, n_nu);
  const int off_lambda_ave = take(simulation && p.image_lambda_ave, 7 * n_nu);
  const int off_emission_ave = take(simulation && p.image_emission_ave, 7 * n_nu);
  const int off_tau_int = take(simulation && p.image_tau_int, 7 * n_nu);
  const int off_crossings = take(p.image_crossings, 1);
  static const char *const cell_names[7] = {"rho", "n_e", "p_gas", "Theta_e", "B", "sigma", "beta_inverse"};
  // level_shape: the trailing dimensions of one image of the level ({res, res} or {n_blocks, bs, bs})
  auto add_alternates = [&](const double *image, size_t level_pix, const std::vector<int> &level_shape, const std::string &prefix,
                            const std::string &suffix, const double *render) {
    auto shaped = [&](bool per_frequency) {
      std::vector<int> shape;
      if (per_frequency && n_nu > 1) shape.push_back(n_nu);
      shape.insert(shape.end(), level_shape.begin(), level_shape.end());
      return shape;
    };
    auto rows = [&](const std::string &name, int offset, int count, bool per_frequency) {
      add(prefix + name + suffix, "<f8", shaped(per_frequency), image + static_cast<size_t>(offset) * level_pix, sizeof(double) * count * level_pix, false);
    };
    auto cells = [&](const char *stem, int offset) {
      std::vector<double> copy(static_cast<size_t>(n_nu) * level_pix);
      for (int n = 0; n < 7; n++) {
        for (int l = 0; l < n_nu; l++)
          std::memcpy(&copy[static_cast<size_t>(l) * level_pix], image + static_cast<size_t>(offset + l * 7 + n) * level_pix, sizeof(double) * level_pix);
        add(prefix + stem + cell_names[n] + suffix, "<f8", shaped(true), copy.data(), sizeof(double) * copy.size(), true);
      }
    };
    if (p.image_time) rows("time", off_time, 1, false);
    if (p.image_length) rows("length", off_length, 1, false);
    if (p.image_lambda) rows("lambda", off_lambda, n_nu, true);
    if (p.image_emission) rows("emission", off_emission, n_nu, true);
    if (p.image_tau) rows("tau", off_tau, n_nu, true);
    if (simulation && p.image_lambda_ave) cells("lambda_ave_", off_lambda_ave);
    if (simulation && p.image_emission_ave) cells("emission_ave_", off_emission_ave);
    if (simulation && p.image_tau_int) cells("tau_int_", off_tau_int);
    if (p.image_crossings) rows("crossings", off_crossings, 1, false);
    if (n_render > 0) {
      std::vector<int> shape = {n_render, 3};
      shape.insert(shape.end(), level_shape.begin(), level_shape.end());
      add(prefix + "rendering" + suffix, "<f8", shape, render, sizeof(double) * n_render * 3 * level_pix, false);
    }
  };
  if (n_render > 0 && d->level[0].render == nullptr) return bl_internal_fail(ctx, BL_E_ARG, "render_num_images > 0 needs render data.");
  add_alternates(image0, n_pix, {res, res}, "", "", d->level[0].render);
  const int bs = p.adaptive_max_level > 0 ? p.adaptive_block_size : 1;
  for (int l = 1; l <= num_levels; l++) {
    const bl_output_level &lv = d->level[l];
    if (lv.image == nullptr || lv.block_locs == nullptr) return bl_internal_fail(ctx, BL_E_ARG, "Missing adaptive level data.");
    const std::string suffix = "_" + std::to_string(l);
    const size_t level_pix = static_cast<size_t>(lv.n_blocks) * bs * bs;
    add("adaptive_block_locs" + suffix, "<i4", {lv.n_blocks, 2}, lv.block_locs, 8 * static_cast<size_t>(lv.n_blocks), false);
    if (p.output_camera) {
      if (lv.camera == nullptr) return bl_internal_fail(ctx, BL_E_ARG, "output_camera needs camera data.");
      add(std::string("adaptive_") + camera_name + suffix, "<f8", {lv.n_blocks, bs, bs, 4}, lv.camera, sizeof(double) * level_pix * 4, false);
    }
    if (p.image_light) add_stokes(lv.image, level_pix, {lv.n_blocks, bs, bs}, "adaptive_", suffix);
    if (n_render > 0 && lv.render == nullptr) return bl_internal_fail(ctx, BL_E_ARG, "render_num_images > 0 needs render data.");
    add_alternates(lv.image, level_pix, {lv.n_blocks, bs, bs}, "adaptive_", suffix, lv.render);
  }

  // ZIP64 (beyond the reference, whose writer ends with "too large for ZIP" there - numpy_format.cpp:44-45,
  // zip_format.cpp:83-85): records of 4 GiB and more, and records behind the first 4 GiB of the file, carry 64-bit sizes
  // and offsets, and the file ends with the ZIP64 end-of-central-directory record and locator (APPNOTE 4.3.14-15), which
  // numpy.load reads. Files within the 32-bit limits are byte for byte what the reference writes.
  // BLACKLIGHT_AMD_ZIP64 = never keeps the reference's error, = always writes the 64-bit fields whatever the size.
  const char *zip64_env = std::getenv("BLACKLIGHT_AMD_ZIP64");
  const bool zip64_never = zip64_env != nullptr && std::strcmp(zip64_env, "never") == 0;
  const bool zip64_always = zip64_env != nullptr && std::strcmp(zip64_env, "always") == 0;
  std::vector<Bytes> local_headers(records.size()), central_headers(records.size());
  size_t offset = 0;
  bool any_zip64 = zip64_always;
  for (NpyRecord &r : records)
    if (!r.owned.empty()) r.data = r.owned.data();   // (set here: the vector of records has stopped moving)
  for (size_t n = 0; n < records.size(); n++) {
    const size_t size = records[n].size();
    const bool zip64 = !zip64_never && (zip64_always || size > UINT32_MAX || offset > UINT32_MAX);
    if (records[n].head.empty() || !MakeLocalHeader(records[n].name, records[n], zip64, &local_headers[n]))
      return bl_internal_fail(ctx, BL_E_INPUT, "Array and metadata too large for ZIP record.");
    central_headers[n] = MakeCentralHeader(local_headers[n], offset, zip64, size);
    any_zip64 = any_zip64 || zip64;
    offset += local_headers[n].size() + size;
  }
  size_t central_length = 0;
  for (const Bytes &h : central_headers) central_length += h.size();
  const bool end_zip64 = !zip64_never && (any_zip64 || offset > UINT32_MAX || central_length > UINT32_MAX || records.size() > 0xFFFE);
  if (!end_zip64 && (offset > UINT32_MAX || central_length > UINT32_MAX))
    return bl_internal_fail(ctx, BL_E_INPUT, "File contents too large for ZIP format.");
  Bytes end;
  if (end_zip64) {
    end = {0x50, 0x4b, 0x06, 0x06};
    Put<uint64_t>(&end, 44);             // size of the rest of this record
    Put<uint16_t>(&end, 45 | (3 << 8));  // made by 4.5, unix
    Put<uint16_t>(&end, 45);
    Put<uint32_t>(&end, 0);
    Put<uint32_t>(&end, 0);
    Put<uint64_t>(&end, records.size());
    Put<uint64_t>(&end, records.size());
    Put<uint64_t>(&end, central_length);
    Put<uint64_t>(&end, offset);
    end.insert(end.end(), {0x50, 0x4b, 0x06, 0x07});   // locator
    Put<uint32_t>(&end, 0);
    Put<uint64_t>(&end, offset + central_length);
    Put<uint32_t>(&end, 1);
  }
  end.insert(end.end(), {0x50, 0x4b, 0x05, 0x06});
  Put<uint16_t>(&end, 0);
  Put<uint16_t>(&end, 0);
  Put<uint16_t>(&end, static_cast<uint16_t>(std::min<size_t>(records.size(), 0xFFFF)));
  Put<uint16_t>(&end, static_cast<uint16_t>(std::min<size_t>(records.size(), 0xFFFF)));
  Put<uint32_t>(&end, static_cast<uint32_t>(std::min<size_t>(central_length, UINT32_MAX)));
  Put<uint32_t>(&end, static_cast<uint32_t>(std::min<size_t>(offset, UINT32_MAX)));
  Put<uint16_t>(&end, 0);
  // Small pieces through the stream; the data of a large record straight to its place in the file from several host threads (pwrite:
  // the copy into the page cache is what a write costs, and it parallelises) - the same bytes at the same offsets.
  bool written = true;
  size_t position = 0;
  auto put = [&](const uint8_t *bytes, size_t count) {
    stream.write(reinterpret_cast<const char *>(bytes), static_cast<std::streamsize>(count));
    position += count;
  };
  for (size_t n = 0; n < records.size() && written; n++) {
    put(local_headers[n].data(), local_headers[n].size());
    put(records[n].head.data(), records[n].head.size());
    const size_t bytes = records[n].data_bytes;
    const int workers = ByteWorkers(bytes);
    if (workers <= 1) {
      put(records[n].data, bytes);
      continue;
    }
    stream.flush();
    const int fd = ::open(path.c_str(), O_WRONLY);
    if (fd < 0 || !stream.good()) {
      if (fd >= 0) ::close(fd);
      put(records[n].data, bytes);   // (no second descriptor: the plain way)
      continue;
    }
    const size_t share = ((bytes + workers - 1) / workers + 4095) / 4096 * 4096;
    std::vector<char> ok(workers, 1);
    std::vector<std::thread> pool;
    const uint8_t *data = records[n].data;
    for (int t = 0; t < workers; t++)
      pool.emplace_back([&, t]() {
        size_t first = std::min(bytes, share * t);
        const size_t last = std::min(bytes, share * (t + 1));
        while (first < last) {
          const ssize_t did = ::pwrite(fd, data + first, std::min<size_t>(last - first, 256u << 20), static_cast<off_t>(position + first));
          if (did <= 0) {
            ok[t] = 0;
            return;
          }
          first += static_cast<size_t>(did);
        }
      });
    for (std::thread &t : pool) t.join();
    ::close(fd);
    for (char good : ok) written = written && good != 0;
    position += bytes;
    stream.seekp(static_cast<std::streamoff>(position));
  }
  for (const Bytes &h : central_headers) put(h.data(), h.size());
  put(end.data(), end.size());
  return (written && stream.good()) ? BL_OK : bl_internal_fail(ctx, BL_E_INPUT, "Could not write output file.");
}

}  // namespace

extern "C" {

int bl_write_output(bl_ctx *ctx, const char *path_override, const bl_output_desc *d) {
  if (ctx == nullptr || d == nullptr) return BL_E_ARG;
  if (bl_num_electron_models(ctx) >= 2)
    return bl_internal_fail(ctx, BL_E_UNSUPPORTED, "bl_write_output: the reference's file layout has no electron-model axis (bl_set_electron_models with n >= 2).");
  if (bl_num_density_units(ctx) >= 2)
    return bl_internal_fail(ctx, BL_E_UNSUPPORTED, "bl_write_output: the reference's file layout has no density-unit axis (bl_set_density_units with n >= 2).");
  if (bl_num_polarized_variants(ctx) >= 2)
    return bl_internal_fail(ctx, BL_E_UNSUPPORTED, "bl_write_output: the reference's file layout has no variant axis (bl_set_polarized_variants with n >= 2).");
  if (bl_num_sigma_cuts(ctx) >= 2)
    return bl_internal_fail(ctx, BL_E_UNSUPPORTED, "bl_write_output: the reference's file layout has no sigma-cut axis (bl_set_sigma_cuts with n >= 2).");
  if (bl_num_electron_mixes(ctx) >= 2)
    return bl_internal_fail(ctx, BL_E_UNSUPPORTED, "bl_write_output: the reference's file layout has no electron-mix axis (bl_set_electron_mixes with n >= 2).");
  if (bl_num_cameras(ctx) >= 2)
    return bl_internal_fail(ctx, BL_E_UNSUPPORTED, "bl_write_output: the reference's file holds one camera (bl_set_cameras with n >= 2; bl_write_output_camera).");
  return WriteOutput(ctx, path_override, d, 0, 1);
}

int bl_write_output_variant(bl_ctx *ctx, const char *path_override, const bl_output_desc *d, int variant) {
  if (ctx == nullptr || d == nullptr) return BL_E_ARG;
  const int n_variants = bl_num_variants(ctx);
  if (variant < 0 || variant >= n_variants)
    return bl_internal_fail(ctx, BL_E_ARG, ("bl_write_output_variant: variant " + std::to_string(variant) + " outside 0 .. " + std::to_string(n_variants - 1) + ".").c_str());
  if (n_variants >= 2 && d->adaptive_num_levels != 0)
    return bl_internal_fail(ctx, BL_E_ARG, "bl_write_output_variant: a render of several variants has no adaptive levels.");
  if (bl_num_cameras(ctx) >= 2)
    return bl_internal_fail(ctx, BL_E_UNSUPPORTED, "bl_write_output_variant: the reference's file holds one camera (bl_set_cameras with n >= 2; bl_write_output_camera).");
  return WriteOutput(ctx, path_override, d, variant, n_variants);
}

int bl_write_output_camera(bl_ctx *ctx, const char *path_override, const bl_output_desc *d, int camera, int variant) {
  if (ctx == nullptr || d == nullptr) return BL_E_ARG;
  const int n_variants = bl_num_variants(ctx), n_cameras = std::max(1, bl_num_cameras(ctx));
  if (camera < 0 || camera >= n_cameras)
    return bl_internal_fail(ctx, BL_E_ARG, ("bl_write_output_camera: camera " + std::to_string(camera) + " outside 0 .. " + std::to_string(n_cameras - 1) + ".").c_str());
  if (variant < 0 || variant >= n_variants)
    return bl_internal_fail(ctx, BL_E_ARG, ("bl_write_output_camera: variant " + std::to_string(variant) + " outside 0 .. " + std::to_string(n_variants - 1) + ".").c_str());
  if ((n_variants >= 2 || n_cameras >= 2) && d->adaptive_num_levels != 0)
    return bl_internal_fail(ctx, BL_E_ARG, "bl_write_output_camera: a render of several cameras or variants has no adaptive levels.");
  return WriteOutput(ctx, path_override, d, variant, n_variants, camera, n_cameras);
}

int bl_camera_output_path(bl_ctx *ctx, int snapshot, int camera, int variant, char *buf, size_t len) {
  if (ctx == nullptr || buf == nullptr) return BL_E_ARG;
  const int n_variants = bl_num_variants(ctx), n_cameras = std::max(1, bl_num_cameras(ctx));
  if (camera < 0 || camera >= n_cameras)
    return bl_internal_fail(ctx, BL_E_ARG, ("bl_camera_output_path: camera " + std::to_string(camera) + " outside 0 .. " + std::to_string(n_cameras - 1) + ".").c_str());
  if (variant < 0 || variant >= n_variants)
    return bl_internal_fail(ctx, BL_E_ARG, ("bl_camera_output_path: variant " + std::to_string(variant) + " outside 0 .. " + std::to_string(n_variants - 1) + ".").c_str());
  std::string path;
  const int rc = OutputPath(ctx, snapshot, variant, n_variants, camera, n_cameras, &path);
  if (rc != BL_OK) return rc;
  if (path.size() + 1 > len) return bl_internal_fail(ctx, BL_E_ARG, "bl_camera_output_path: the buffer is too short for the name.");
  std::memcpy(buf, path.c_str(), path.size() + 1);
  return BL_OK;
}

namespace {
// What bl_write_output_frequency and bl_frequency_output_path check alike: the three indices
int CheckFrequencyFile(bl_ctx *ctx, const char *who, int frequency, int camera, int variant) {
  int n_nu = 0;
  (void)bl_internal_frequencies(ctx, &n_nu);
  const int n_variants = bl_num_variants(ctx), n_cameras = std::max(1, bl_num_cameras(ctx));
  const auto outside = [&](const char *what, int index, int n) {
    return bl_internal_fail(ctx, BL_E_ARG, (std::string(who) + ": " + what + " " + std::to_string(index) + " outside 0 .. " + std::to_string(n - 1) + ".").c_str());
  };
  if (frequency < 0 || frequency >= n_nu) return outside("frequency", frequency, n_nu);
  if (camera < 0 || camera >= n_cameras) return outside("camera", camera, n_cameras);
  if (variant < 0 || variant >= n_variants) return outside("variant", variant, n_variants);
  return BL_OK;
}
}  // namespace

int bl_write_output_frequency(bl_ctx *ctx, const char *path_override, const bl_output_desc *d, int frequency, int camera, int variant) {
  if (ctx == nullptr || d == nullptr) return BL_E_ARG;
  if (const int rc = CheckFrequencyFile(ctx, "bl_write_output_frequency", frequency, camera, variant)) return rc;
  int n_nu = 0;
  (void)bl_internal_frequencies(ctx, &n_nu);
  const int n_variants = bl_num_variants(ctx), n_cameras = std::max(1, bl_num_cameras(ctx));
  if (n_nu >= 2 && d->adaptive_num_levels != 0)
    return bl_internal_fail(ctx, BL_E_ARG, "bl_write_output_frequency: a one-frequency run refines by its own image; the file of one frequency of several has no adaptive levels.");
  if ((n_variants >= 2 || n_cameras >= 2) && d->adaptive_num_levels != 0)
    return bl_internal_fail(ctx, BL_E_ARG, "bl_write_output_frequency: a render of several cameras or variants has no adaptive levels.");
  return WriteOutput(ctx, path_override, d, variant, n_variants, camera, n_cameras, frequency);
}

int bl_frequency_output_path(bl_ctx *ctx, int snapshot, int frequency, int camera, int variant, char *buf, size_t len) {
  if (ctx == nullptr || buf == nullptr) return BL_E_ARG;
  if (const int rc = CheckFrequencyFile(ctx, "bl_frequency_output_path", frequency, camera, variant)) return rc;
  std::string path;
  const int rc = OutputPath(ctx, snapshot, variant, bl_num_variants(ctx), camera, std::max(1, bl_num_cameras(ctx)), &path, frequency);
  if (rc != BL_OK) return rc;
  if (path.size() + 1 > len) return bl_internal_fail(ctx, BL_E_ARG, "bl_frequency_output_path: the buffer is too short for the name.");
  std::memcpy(buf, path.c_str(), path.size() + 1);
  return BL_OK;
}

int bl_variant_output_path(bl_ctx *ctx, int snapshot, int variant, char *buf, size_t len) {
  if (ctx == nullptr || buf == nullptr) return BL_E_ARG;
  const int n_variants = bl_num_variants(ctx);
  if (variant < 0 || variant >= n_variants)
    return bl_internal_fail(ctx, BL_E_ARG, ("bl_variant_output_path: variant " + std::to_string(variant) + " outside 0 .. " + std::to_string(n_variants - 1) + ".").c_str());
  std::string path;
  const int rc = OutputPath(ctx, snapshot, variant, n_variants, 0, 1, &path);
  if (rc != BL_OK) return rc;
  if (path.size() + 1 > len) return bl_internal_fail(ctx, BL_E_ARG, "bl_variant_output_path: the buffer is too short for the name.");
  std::memcpy(buf, path.c_str(), path.size() + 1);
  return BL_OK;
}

}  // extern "C"
