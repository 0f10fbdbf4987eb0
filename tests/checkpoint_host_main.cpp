// checkpoint_host_main.cpp - the checkpoint code of blacklight_amd/csrc/bl_checkpoint.cpp without a GPU (tests/test_checkpoint_host.py
// builds this file with it, once plainly and once under the host sanitizers).
//
//   checkpoint_host_main read <file> <resolution> <frequencies> <ray_max_steps>
//       reads a geodesic checkpoint: "ok", exit 0 - or the failure's text, exit 2; then the most memory the run ever held (KiB)
//   checkpoint_host_main roundtrip <file> <resolution> <frequencies> <ray_max_steps> <out>
//       file -> chunks -> file, twice: the rays in pixel order (<out>.ordered) and through a shuffled pixel map (<out>.shuffled), with a
//       record gate that makes at least three chunks of the pixels; reads both files back; then asks for a chunk behind a gate
//       one record short of the longest ray and prints what that failure says
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>

#include "bl_checkpoint.h"

namespace {

bl_params Params(char **argv) {
  bl_params p{};
  std::snprintf(p.checkpoint_geodesic_file.s, sizeof p.checkpoint_geodesic_file.s, "%s", argv[2]);
  p.camera_resolution = std::atoi(argv[3]);
  p.image_num_frequencies = std::atoi(argv[4]);
  p.ray_max_steps = std::atoi(argv[5]);
  return p;
}

// The file's geodesics through chunks of at most `gate` records into a new file. map: ray -> pixel, every pixel once.
int RoundTrip(const bl_ctx::Checkpoint &ck, const std::vector<int> &map, long long gate, const std::string &path) {
  const long long n_pix = static_cast<long long>(ck.sample_num.size());
  const BlSpacetime st{1.0, 0.9375, 0};   // (enters sample_dir only, which a save renormalises again: not compared)
  CheckpointSave save;
  int chunks = 0;
  for (long long begin = 0; begin < n_pix; chunks++) {
    HostChunk chunk = ChunkFromCheckpoint(ck, map.data(), begin, static_cast<int>(n_pix - begin), gate);
    begin += static_cast<long long>(chunk.sample_num.size());
    for (long long &ray : chunk.out_index) ray = map[ray];   // (a save names pixels: it is refused with a pixel map)
    AddChunkToCheckpoint(chunk, st, n_pix, &save);
  }
  // the camera's rows as a render through this map would get them, put back by pixel
  std::vector<double> camera[2] = {GatherCameraRows(ck.camera_pos, map.data(), n_pix), GatherCameraRows(ck.camera_dir, map.data(), n_pix)};
  for (std::vector<double> &rows : camera) {
    const std::vector<double> by_ray = rows;
    for (long long ray = 0; ray < n_pix; ray++) std::copy(&by_ray[4 * ray], &by_ray[4 * ray] + 4, &rows[4 * map[ray]]);
  }
  bl_camera_frame frame{};
  double *vectors[7] = {frame.cam_x, frame.u_con, frame.u_cov, frame.norm_con, frame.norm_con_c, frame.hor_con_c, frame.vert_con_c};
  for (int v = 0; v < 7; v++) std::copy(ck.frame[v], ck.frame[v] + 4, vectors[v]);
  WriteGeodesicCheckpoint(path.c_str(), frame, ck.frequencies.data(), static_cast<int>(ck.frequencies.size()), camera[0], camera[1], save);
  return chunks;
}

}  // namespace

int main(int argc, char **argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (!((mode == "read" && argc == 6) || (mode == "roundtrip" && argc == 7))) {
    std::fprintf(stderr, "usage: checkpoint_host_main read|roundtrip <file> <resolution> <frequencies> <ray_max_steps> [<out>]\n");
    return 1;
  }
  int status = 0;
  try {
    bl_params p = Params(argv);
    const std::shared_ptr<const bl_ctx::Checkpoint> ck = ReadGeodesicCheckpoint(p);
    if (mode == "roundtrip") {
      const int n_pix = static_cast<int>(ck->sample_num.size());
      const long long most = *std::max_element(ck->sample_num.begin(), ck->sample_num.end());
      const long long total = std::accumulate(ck->sample_num.begin(), ck->sample_num.end(), 0ll);
      const long long gate = std::max(most, total / 4);   // (never below the longest ray: every ray fits a chunk of its own)
      std::vector<int> map(n_pix);
      std::iota(map.begin(), map.end(), 0);
      const int ordered = RoundTrip(*ck, map, gate, std::string(argv[6]) + ".ordered");
      std::mt19937 draw(7);
      for (int m = n_pix - 1; m > 0; m--) std::swap(map[m], map[draw() % static_cast<unsigned int>(m + 1)]);
      const int shuffled = RoundTrip(*ck, map, gate, std::string(argv[6]) + ".shuffled");
      for (const char *suffix : {".ordered", ".shuffled"}) {
        std::snprintf(p.checkpoint_geodesic_file.s, sizeof p.checkpoint_geodesic_file.s, "%s%s", argv[6], suffix);
        ReadGeodesicCheckpoint(p);
      }
      std::printf("most=%lld total=%lld gate=%lld chunks_ordered=%d chunks_shuffled=%d\n", most, total, gate, ordered, shuffled);
      const long long longest = std::max_element(ck->sample_num.begin(), ck->sample_num.end()) - ck->sample_num.begin();
      try {
        ChunkFromCheckpoint(*ck, nullptr, longest, 1, most - 1);
        std::printf("small gate: no failure\n");
      } catch (const Failure &failure) {
        std::printf("small gate: %s\n", failure.message.c_str());
      }
    } else {
      std::printf("ok\n");
    }
  } catch (const Failure &failure) {
    std::printf("failure: %s\n", failure.message.c_str());
    status = 2;
  }
  // (VmHWM of this program's own address space: getrusage's ru_maxrss starts from the parent process's)
  std::ifstream self("/proc/self/status");
  for (std::string line; std::getline(self, line);)
    if (line.compare(0, 6, "VmHWM:") == 0) std::printf("peak_rss_kib=%ld\n", std::atol(line.c_str() + 6));
  return status;
}
