// bl_checkpoint.h - the reference's checkpoint files on the host (bl_checkpoint.cpp): its Array format, the geodesic checkpoint both
// ways, the sample checkpoint it writes, and the conversions between a file's order (by pixel, far -> near) and a chunk's sample records
// (near -> far). No GPU call: bl_render.hip copies a chunk between device and host and decides when; tests/checkpoint_host_main.cpp
// runs everything here on any machine.
#ifndef BLACKLIGHT_AMD_BL_CHECKPOINT_H_
#define BLACKLIGHT_AMD_BL_CHECKPOINT_H_
#include "bl_ctx.h"

namespace blhost {

// A geodesic checkpoint being assembled: samples of every pixel, far -> near, packed
struct CheckpointSave {
  std::vector<int32_t> sample_num;
  std::vector<uint8_t> flags;
  std::vector<double> factors, pos, dir, len;
  std::vector<size_t> offset;
};
// checkpoint_sample_save: where every kept sample of the level sits on the grid, by pixel and reversed sample index
struct SampleSave {
  int per_sample = 4;                     // indices per sample: 4, or 8 x 4 with inter-block interpolation
  std::vector<int32_t> sample_num;        // [pixel]
  std::vector<size_t> offset;             // [pixel]: first entry of the pixel in the packed arrays below
  std::vector<int32_t> inds;              // [sample][per_sample]
  std::vector<double> fracs;              // [sample][3] (trilinear sampling)
  std::vector<uint8_t> nan, fallback;     // [sample]
};
// A chunk on the host: its sample records as a scratch set holds them, and its rays' rows of bl_ctx::RayArrays
struct HostChunk {
  std::vector<BlSampleHot> hot;           // (interleaved records: every second entry, the cold halves between them)
  std::vector<BlSampleCold> cold;
  std::vector<double> sample_t, kt, factor;
  std::vector<int> sample_num;
  std::vector<unsigned char> flags;
  std::vector<long long> out_index;
  std::vector<long long> offset;          // a ray's first record (loading), its first entry in the file being assembled (saving)
};

// ---- the files
std::shared_ptr<const bl_ctx::Checkpoint> ReadGeodesicCheckpoint(const bl_params &p);
void LoadGeodesicCheckpoint(bl_ctx *ctx);
void WriteGeodesicCheckpoint(const char *path, const bl_camera_frame &frame, const double *frequencies, int n_nu, const std::vector<double> &camera_pos,
                             const std::vector<double> &camera_dir, const CheckpointSave &save);
void WriteSampleCheckpoint(const char *path, const SampleSave &sampling, bool block_interp, bool interp);

// ---- the conversions
// A file's camera_pos or camera_dir rows for the rays of a call (pixel_map null: ray = pixel)
std::vector<double> GatherCameraRows(const std::vector<double> &source, const int *pixel_map, long long n_rays);
// File -> chunk: as many of the rays [begin, begin + rays) as `record_gate` records hold
HostChunk ChunkFromCheckpoint(const bl_ctx::Checkpoint &ck, const int *pixel_map, long long begin, int rays, long long record_gate);
// Chunk -> the file being assembled, whose pixels the chunk's out_index names (`n_rays` of them)
void AddChunkToCheckpoint(HostChunk &chunk, const BlSpacetime &st, long long n_rays, CheckpointSave *save);
// Chunk and its located samples (tags: the exact tier's; anchors: inter-block interpolation, eight cells per record) -> sample checkpoint
void AddChunkToSampleSave(HostChunk &chunk, const std::vector<BlLocated> &located, const std::vector<unsigned long long> &tags,
                          const std::vector<unsigned int> &anchors, bool interleaved, bool fast, bool block_interp, const bl_params &p,
                          const BlGridDevice &g, const int *merged_blocks, const std::vector<int> &merged_block_at, long long n_rays, SampleSave *sampling);

}  // namespace blhost
#endif  // BLACKLIGHT_AMD_BL_CHECKPOINT_H_
