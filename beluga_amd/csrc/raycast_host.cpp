// raycast_host.cpp — the host rule of mcl_cast_rays* (raycast_host.h).  Plain C++17, no HIP.
#include "raycast_host.h"

#include <algorithm>
#include <cmath>

namespace mcl {

const char* cast_check_range(double max_range, double resolution) {
  if (!std::isfinite(max_range) || !(max_range > 0.0)) return "max_range is not a finite positive number";
  // the walks keep 16 * span in an int (walk_blocks): the bound mcl_reweight enforces on a beam context's beam_max_range
  if (!(max_range / resolution < kCastMaxReachCells)) return "max_range / resolution must stay below 2^27 - 2 cells";
  return nullptr;
}

mcl_status cast_check_call(const double* poses, bool check_poses, bool have_poses, uint64_t n, const double* bearings_cs, uint64_t num_bearings,
                           double max_range, double resolution, bool have_ranges_out, const char** what) {
  if (const char* wrong = cast_check_range(max_range, resolution)) {
    *what = wrong;
    return MCL_ERR_INVALID_ARGUMENT;
  }
  if (n == 0 || num_bearings == 0) return MCL_OK;
  if (!have_poses || !bearings_cs || !have_ranges_out) {
    *what = "null argument";
    return MCL_ERR_INVALID_ARGUMENT;
  }
  if (n > kCastMaxPoses || num_bearings > kCastMaxBearings || n > kCastMaxRays / num_bearings) {
    *what = "more rays than memory can hold";
    return MCL_ERR_OUT_OF_MEMORY;
  }
  for (uint64_t i = 0; i < 2 * num_bearings; ++i)
    if (!std::isfinite(bearings_cs[i])) {
      *what = "a bearing has a value that is not finite";
      return MCL_ERR_INVALID_ARGUMENT;
    }
  if (check_poses)
    for (uint64_t i = 0; i < 4 * n; ++i)
      if (!std::isfinite(poses[i])) {
        *what = "a pose has a value that is not finite";
        return MCL_ERR_INVALID_ARGUMENT;
      }
  return MCL_OK;
}

CastPlan cast_plan(uint64_t n, uint64_t num_bearings, uint64_t chunk_rays) {
  CastPlan plan{};
  plan.rays = n * num_bearings;
  plan.chunk_rays = std::clamp<uint64_t>(chunk_rays, static_cast<uint64_t>(kCastChunkMin), kCastLaunchRays);
  plan.chunks = (plan.rays + plan.chunk_rays - 1) / plan.chunk_rays;
  // a range of r rays of the order i * B + b touches at most (r + B - 2) / B + 1 poses (it may start at a pose's last bearing)
  if (plan.rays) plan.chunk_poses = std::min<uint64_t>(n, (std::min(plan.chunk_rays, plan.rays) + num_bearings - 2) / num_bearings + 1);
  return plan;
}

CastChunk cast_chunk_at(const CastPlan& plan, uint64_t num_bearings, uint64_t c) {
  CastChunk k{};
  k.first_ray = c * plan.chunk_rays;
  k.rays = std::min<uint64_t>(plan.chunk_rays, plan.rays - k.first_ray);
  k.first_pose = k.first_ray / num_bearings;
  k.first_bearing = k.first_ray % num_bearings;
  k.poses = (k.first_ray + k.rays - 1) / num_bearings - k.first_pose + 1;
  k.blocks = (k.rays + kCastBlock - 1) / kCastBlock;
  return k;
}

}  // namespace mcl
