// bl_refine.hip - the adaptive refinement decision on the device (bl_adaptive_refine_device, bl_api.hip): one launch of
// bl_refine_kernel per call leaves one flag per block of the level. The criteria, their order, the verdict and the forced regions are
// bl_refine.h's, which the host call (bl_host.cpp) runs too: equal flags, always. The next level's block list is built on the host
// from the flags.
//   blocks of at most 64 pixels   one wave per block, one pixel per lane; a 256-lane workgroup takes four blocks. The two counts of a
//                                 criterion are popcounts of ballots: no LDS, no atomics, no barrier.
//   larger blocks                 one workgroup per block; its lanes stride over the pixels, every wave sums its ballots' popcounts,
//                                 and the four waves' sums meet in a few words of LDS (one barrier per criterion that is on).
//                                 A block of 65 to 255 pixels (block sizes 9 to 15) has a 256-lane workgroup to itself too, part of
//                                 whose lanes count nothing: the price of two mappings instead of one per block size.
// Neighbours are read from global memory: a block is a few KiB, its stencils hit in the vector L1.
#include <hip/hip_runtime.h>

#include "bl_refine.h"

__global__ void __launch_bounds__(256) bl_refine_kernel(BlRefineArgs A) {
  const int bs = A.bs, num_pix = bs * bs;
  const bool wave_per_block = num_pix <= 64;
  const int wave = threadIdx.x >> 6;
  const long long b = wave_per_block ? (long long)blockIdx.x * 4 + wave : (long long)blockIdx.x;
  if (b >= (long long)A.n_blocks) return;   // (a whole wave with one block each, or a whole workgroup: nobody is left waiting at a barrier)
  const bool writer = wave_per_block ? (threadIdx.x & 63) == 0 : threadIdx.x == 0;
  const int loc_v = A.level == 0 ? (int)(b / A.root) : A.block_locs[2 * b + 0];
  const int loc_u = A.level == 0 ? (int)(b % A.root) : A.block_locs[2 * b + 1];
  if (bl_refine_forced(A.regions, A.level, loc_v, loc_u, A.linear_num_blocks, A.camera_width)) {   // (before any pixel is read)
    if (writer) A.flags[b] = 1;
    return;
  }
  // level 0: the block's pixels lie in the res x res frame; refined levels: block b is the run [b bs^2, (b + 1) bs^2) of the row
  const double *first = A.level == 0 ? A.row + ((long long)loc_v * bs) * A.res + (long long)loc_u * bs : A.row + b * num_pix;
  const long long pitch = A.level == 0 ? A.res : bs;
  auto q_at = [&](int i, int j) { return first[i * pitch + j]; };
  __shared__ int counts[BL_REFINE_CRITERIA][4][2];
  bool flag = false;
  for (int c = 0; c < BL_REFINE_CRITERIA && !flag; c++) {
    if (!(A.cuts.frac[c] >= 0.0)) continue;   // (wave-uniform, as is `flag`: it comes from the block's counts)
    const int margin = bl_refine_margin(c);
    const double cut = A.cuts.cut[c];
    int num_examined = 0, num_exceeded = 0;
    // (every lane makes every pass, so that the ballots see whole waves; a lane past the block's pixels or in the margin counts nothing)
    for (int pass = 0; pass < num_pix; pass += wave_per_block ? 64 : 256) {
      const int pixel = pass + (wave_per_block ? (int)(threadIdx.x & 63) : (int)threadIdx.x);
      const int i = pixel / bs, j = pixel - i * bs;
      bool counted = false, exceeds = false;
      if (pixel < num_pix && i >= margin && i < bs - margin && j >= margin && j < bs - margin) {
        const double q = bl_refine_examined(c, q_at, i, j, bs);
        counted = bl_refine_counts(q);
        exceeds = counted && q > cut;
      }
      num_examined += __popcll(__ballot(counted));
      num_exceeded += __popcll(__ballot(exceeds));
    }
    if (!wave_per_block) {
      if ((threadIdx.x & 63) == 0) {
        counts[c][wave][0] = num_examined;
        counts[c][wave][1] = num_exceeded;
      }
      __syncthreads();   // (criterion c's own words: the next criterion writes others, so one barrier is enough)
      num_examined = counts[c][0][0] + counts[c][1][0] + counts[c][2][0] + counts[c][3][0];
      num_exceeded = counts[c][0][1] + counts[c][1][1] + counts[c][2][1] + counts[c][3][1];
    }
    flag = bl_refine_verdict(num_exceeded, num_examined, A.cuts.frac[c]);
  }
  if (writer) A.flags[b] = flag ? 1 : 0;
}

extern "C" hipError_t bl_launch_refine(const BlRefineArgs *args, hipStream_t stream) {
  if (args->row == nullptr || args->flags == nullptr || args->n_blocks < 1 || args->bs < 1 || args->root < 1
      || (args->level > 0 && args->block_locs == nullptr))
    return hipErrorInvalidValue;
  const bool wave_per_block = args->bs * args->bs <= 64;
  const unsigned int grid = wave_per_block ? (static_cast<unsigned int>(args->n_blocks) + 3u) / 4u : static_cast<unsigned int>(args->n_blocks);
  hipLaunchKernelGGL(bl_refine_kernel, dim3(grid), dim3(256), 0, stream, *args);
  return hipGetLastError();
}
