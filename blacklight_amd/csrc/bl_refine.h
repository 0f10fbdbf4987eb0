// bl_refine.h - the adaptive refinement decision, written once for the host call (bl_adaptive_refine, bl_host.cpp) and the device call
// (bl_adaptive_refine_device: bl_refine_kernel in bl_refine.hip, its entry point in bl_api.hip).
//   RadiationIntegrator::CheckAdaptiveRefinement, ::EvaluateBlock   src/radiation_integrator/radiation_adaptive.cpp:19-312
//   the children's order of GeodesicIntegrator::AugmentCamera        src/geodesic_integrator/camera.cpp:445-458
// First part, host and device: the value each of the five criteria examines at pixel (i, j) of a block of bs x bs pixels read through an
// accessor q_at(i, j) (i: the block's row, j: its column), the verdict of one criterion from its two counts, and the forced regions.
// The operand order is the reference's, and both builds have -ffp-contract=off, IEEE fp64 division and the pinned bl_hypot (blmath.h):
// the host loop and the kernel examine the same bits. Second part, host only: the plan of a call and the declarations of what the two entry points share around
// the blocks' verdicts - refusals, the checks of level and block count, the choice of image row, the next level's block list (bl_host.cpp).
#ifndef BLACKLIGHT_AMD_BL_REFINE_H_
#define BLACKLIGHT_AMD_BL_REFINE_H_

#include <stddef.h>
#include <stdint.h>

#include "bl_internal.h"
#include "blmath.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define BL_REFINE_FN static inline __host__ __device__
#else
#define BL_REFINE_FN static inline
#endif

// The criteria in the order EvaluateBlock runs them
enum { BL_REFINE_VAL = 0, BL_REFINE_ABS_GRAD, BL_REFINE_REL_GRAD, BL_REFINE_ABS_LAPL, BL_REFINE_REL_LAPL, BL_REFINE_CRITERIA };

// cut and frac of every criterion (frac < 0: the criterion is off), and the forced regions: what a block's verdict reads of the parameters
struct BlRefineCuts {
  double cut[BL_REFINE_CRITERIA], frac[BL_REFINE_CRITERIA];
};
struct BlRefineRegions {
  int count;
  int level[BL_MAX_REGIONS];
  double x_min[BL_MAX_REGIONS], x_max[BL_MAX_REGIONS], y_min[BL_MAX_REGIONS], y_max[BL_MAX_REGIONS];
};

// bl_refine_kernel's argument block (bl_refine.hip)
struct BlRefineArgs {
  const double *row;        // device: the image row examined, n_pix of the level
  const int *block_locs;    // device: [n_blocks][2] (block_v, block_u); null at level 0 (root blocks, row-major)
  unsigned char *flags;     // device out: [n_blocks]
  int n_blocks, level;
  int bs, res, root, linear_num_blocks;   // BlRefinePlan's
  double camera_width;
  BlRefineCuts cuts;
  BlRefineRegions regions;
};

// Pixels (i, j) with margin <= i, j < bs - margin are examined: every pixel by the value and the gradients, the interior by the Laplacians
BL_REFINE_FN int bl_refine_margin(int criterion) { return criterion >= BL_REFINE_ABS_LAPL ? 1 : 0; }

// The value itself
template <typename Q>
BL_REFINE_FN double bl_refine_value(const Q &q_at, int i, int j, int bs) {
  (void)bs;
  return __builtin_fabs(q_at(i, j));
}

// The absolute gradient (one-sided at the block's edges, centred inside; bs = 1 reads past the block, as the reference does)
template <typename Q>
BL_REFINE_FN double bl_refine_abs_gradient(const Q &q_at, int i, int j, int bs) {
  double q_x = j == 0 ? q_at(i, j + 1) - q_at(i, j)
      : (j == bs - 1 ? q_at(i, j) - q_at(i, j - 1) : 0.5 * (q_at(i, j + 1) - q_at(i, j - 1)));
  double q_y = i == 0 ? q_at(i + 1, j) - q_at(i, j)
      : (i == bs - 1 ? q_at(i, j) - q_at(i - 1, j) : 0.5 * (q_at(i + 1, j) - q_at(i - 1, j)));
  return bl_hypot(q_x, q_y);
}

// The relative gradient: each difference over the mean of the values it spans
template <typename Q>
BL_REFINE_FN double bl_refine_rel_gradient(const Q &q_at, int i, int j, int bs) {
  double q_x;
  if (j == 0)
    q_x = 2.0 * (q_at(i, j + 1) - q_at(i, j)) / (q_at(i, j) + q_at(i, j + 1));
  else if (j == bs - 1)
    q_x = 2.0 * (q_at(i, j) - q_at(i, j - 1)) / (q_at(i, j - 1) + q_at(i, j));
  else
    q_x = 2.0 * (q_at(i, j + 1) - q_at(i, j - 1)) / (q_at(i, j - 1) + 2.0 * q_at(i, j) + q_at(i, j + 1));
  double q_y;
  if (i == 0)
    q_y = 2.0 * (q_at(i + 1, j) - q_at(i, j)) / (q_at(i, j) + q_at(i + 1, j));
  else if (i == bs - 1)
    q_y = 2.0 * (q_at(i, j) - q_at(i - 1, j)) / (q_at(i - 1, j) + q_at(i, j));
  else
    q_y = 2.0 * (q_at(i + 1, j) - q_at(i - 1, j)) / (q_at(i - 1, j) + 2.0 * q_at(i, j) + q_at(i + 1, j));
  return bl_hypot(q_x, q_y);
}

// The absolute Laplacian (interior pixels only)
template <typename Q>
BL_REFINE_FN double bl_refine_abs_laplacian(const Q &q_at, int i, int j, int bs) {
  (void)bs;
  double q_x = q_at(i, j - 1) - 2.0 * q_at(i, j) + q_at(i, j + 1);
  double q_y = q_at(i - 1, j) - 2.0 * q_at(i, j) + q_at(i + 1, j);
  return __builtin_fabs(q_x + q_y);
}

// The relative Laplacian (interior pixels only)
template <typename Q>
BL_REFINE_FN double bl_refine_rel_laplacian(const Q &q_at, int i, int j, int bs) {
  (void)bs;
  double q_x = 4.0 * (q_at(i, j - 1) - 2.0 * q_at(i, j) + q_at(i, j + 1))
      / (q_at(i, j - 1) + 2.0 * q_at(i, j) + q_at(i, j + 1));
  double q_y = 4.0 * (q_at(i - 1, j) - 2.0 * q_at(i, j) + q_at(i + 1, j))
      / (q_at(i - 1, j) + 2.0 * q_at(i, j) + q_at(i + 1, j));
  return __builtin_fabs(q_x + q_y);
}

// ... by number
template <typename Q>
BL_REFINE_FN double bl_refine_examined(int criterion, const Q &q_at, int i, int j, int bs) {
  switch (criterion) {
    case BL_REFINE_VAL: return bl_refine_value(q_at, i, j, bs);
    case BL_REFINE_ABS_GRAD: return bl_refine_abs_gradient(q_at, i, j, bs);
    case BL_REFINE_REL_GRAD: return bl_refine_rel_gradient(q_at, i, j, bs);
    case BL_REFINE_ABS_LAPL: return bl_refine_abs_laplacian(q_at, i, j, bs);
    default: return bl_refine_rel_laplacian(q_at, i, j, bs);
  }
}

// A pixel counts as examined when its value is finite (NaN and infinite values drop out of both counts)
BL_REFINE_FN bool bl_refine_counts(double examined_value) { return __builtin_isfinite(examined_value); }

// One criterion's verdict from its counts. A block without a finite value gives 0 / 0 = NaN, which exceeds nothing.
BL_REFINE_FN bool bl_refine_verdict(int num_exceeded, int num_examined, double frac_cut) {
  double frac = static_cast<double>(num_exceeded) / static_cast<double>(num_examined);
  return frac > frac_cut;
}

// Forced regions (:52-69, :96-113): a block of a level below a region's whose centre lies inside it refines whatever its pixels say
BL_REFINE_FN bool bl_refine_forced(const BlRefineRegions &regions, int level, int loc_v, int loc_u, int linear_num_blocks, double camera_width) {
  if (regions.count <= 0) return false;
  double y = ((loc_v + 0.5) / linear_num_blocks - 0.5) * camera_width;
  double x = ((loc_u + 0.5) / linear_num_blocks - 0.5) * camera_width;
  for (int r = 0; r < regions.count; r++)
    if (level < regions.level[r] && x > regions.x_min[r] && x < regions.x_max[r] && y > regions.y_min[r] && y < regions.y_max[r]) return true;
  return false;
}

// ------------------------------------------------------------------ host only: around the blocks' verdicts (declarations; bl_host.cpp)

// What a call decides over, from the context and the call's level and block count
struct BlRefinePlan {
  bool decide = false;          // false: adaptive_max_level <= 0 or level >= adaptive_max_level - no block refines (radiation_adaptive.cpp:22-23)
  int bs = 0;                   // adaptive_block_size
  int res = 0;                  // camera_resolution
  int root = 0;                 // root blocks per side
  int linear_num_blocks = 0;    // blocks per side of the camera at this level
  long long n_pix = 0;          // pixels of one image row of this level
  size_t row = 0;               // the image row examined: I_nu at the chosen frequency
  double camera_width = 0.0;
  BlRefineCuts cuts{};
  BlRefineRegions regions{};
};

// The refusals and checks of both entry points, with the texts of bl_adaptive_refine. BL_OK: *plan is filled. (*n_refined is zero
// once the context's variants are found to be one image, as ever.) Defined in bl_host.cpp, as is bl_refine_children.
int bl_refine_plan(bl_ctx *ctx, int level, int n_blocks, const int32_t *block_locs, int32_t *n_refined, BlRefinePlan *plan);

// Block b's place (block_v, block_u) among the blocks of its level
inline void bl_refine_block_loc(const BlRefinePlan &plan, int level, int b, const int32_t *block_locs, int *loc_v, int *loc_u) {
  *loc_v = level == 0 ? b / plan.root : block_locs[2 * b + 0];
  *loc_u = level == 0 ? b % plan.root : block_locs[2 * b + 1];
}

// The next level's list from the flags (camera.cpp:453-458): parents in order, each with its four children; returns the parents' count
int bl_refine_children(const BlRefinePlan &plan, int level, int n_blocks, const int32_t *block_locs, const uint8_t *refine_flags, int32_t *next_locs);

#endif  // BLACKLIGHT_AMD_BL_REFINE_H_
