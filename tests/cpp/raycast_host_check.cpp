// raycast_host_check.cpp — the host rule of mcl_cast_rays* (beluga_amd/csrc/raycast_host.cpp) as a stand-alone program, for a CPU build
// under the sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ibeluga_amd/csrc
//       tests/cpp/raycast_host_check.cpp beluga_amd/csrc/raycast_host.cpp -o raycast_host_check && ./raycast_host_check
// Exercises every function of the file at its edges; exits 0 and prints "raycast_host_check OK" if every expectation holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "raycast_host.h"

#define EXPECT(cond)                                                       \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

using namespace mcl;

static mcl_status check(const std::vector<double>& poses, bool look, const std::vector<double>& bearings, double max_range, double resolution,
                        bool ranges = true) {
  const char* what = nullptr;
  const mcl_status s = cast_check_call(poses.data(), look, true, poses.size() / 4, bearings.data(), bearings.size() / 2, max_range, resolution, ranges,
                                       &what);
  EXPECT((s == MCL_OK) == (what == nullptr));
  return s;
}

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  // max_range: finite, positive, and below the walks' reach, one step either side of the bound (a resolution with an exact reciprocal)
  const double res = 0.0625, bound = kCastMaxReachCells * res;
  EXPECT(cast_check_range(1.0, res) == nullptr);
  EXPECT(cast_check_range(std::nextafter(bound, 0.0), res) == nullptr);
  EXPECT(cast_check_range(bound, res) != nullptr);
  EXPECT(cast_check_range(std::nextafter(bound, inf), res) != nullptr);
  EXPECT(cast_check_range((kCastMaxReachCells - 1.0) * res, res) == nullptr);
  for (const double bad : {0.0, -1.0, inf, -inf, nan, -0.0}) EXPECT(cast_check_range(bad, res) != nullptr);
  EXPECT(cast_check_range(std::numeric_limits<double>::denorm_min(), res) == nullptr);

  const std::vector<double> poses{1.0, 0.0, 0.5, 0.5, 0.0, 1.0, -3.0, 2.0}, bearings{1.0, 0.0, 0.6, 0.8, 0.0, -1.0};
  EXPECT(check(poses, true, bearings, 2.0, res) == MCL_OK);
  EXPECT(check(poses, true, bearings, bound, res) == MCL_ERR_INVALID_ARGUMENT);
  EXPECT(check(poses, true, bearings, 2.0, res, /*ranges=*/false) == MCL_ERR_INVALID_ARGUMENT);
  for (size_t k = 0; k < poses.size(); ++k)
    for (const double bad : {inf, nan}) {
      std::vector<double> p = poses;
      p[k] = bad;
      EXPECT(check(p, true, bearings, 2.0, res) == MCL_ERR_INVALID_ARGUMENT);
      EXPECT(check(p, false, bearings, 2.0, res) == MCL_OK);  // the device form does not look
    }
  for (size_t k = 0; k < bearings.size(); ++k) {
    std::vector<double> b = bearings;
    b[k] = nan;
    EXPECT(check(poses, true, b, 2.0, res) == MCL_ERR_INVALID_ARGUMENT);
    EXPECT(check(poses, false, b, 2.0, res) == MCL_ERR_INVALID_ARGUMENT);
  }
  const char* what = nullptr;
  // zero counts: nothing is dereferenced, max_range is checked all the same
  EXPECT(cast_check_call(nullptr, true, false, 0, nullptr, 0, 2.0, res, false, &what) == MCL_OK);
  EXPECT(cast_check_call(nullptr, true, false, 5, nullptr, 0, 2.0, res, false, &what) == MCL_OK);
  EXPECT(cast_check_call(nullptr, true, false, 0, nullptr, 5, 2.0, res, false, &what) == MCL_OK);
  EXPECT(cast_check_call(nullptr, true, false, 0, nullptr, 0, -2.0, res, false, &what) == MCL_ERR_INVALID_ARGUMENT);
  // null arguments with both counts non-zero
  EXPECT(cast_check_call(nullptr, true, false, 2, bearings.data(), 3, 2.0, res, true, &what) == MCL_ERR_INVALID_ARGUMENT);
  EXPECT(cast_check_call(poses.data(), true, true, 2, nullptr, 3, 2.0, res, true, &what) == MCL_ERR_INVALID_ARGUMENT);
  // counts no memory holds are refused before anything is multiplied or read
  EXPECT(cast_check_call(nullptr, false, true, kCastMaxPoses + 1, bearings.data(), 1, 2.0, res, true, &what) == MCL_ERR_OUT_OF_MEMORY);
  EXPECT(cast_check_call(nullptr, false, true, 1, bearings.data(), kCastMaxBearings + 1, 2.0, res, true, &what) == MCL_ERR_OUT_OF_MEMORY);
  EXPECT(cast_check_call(nullptr, false, true, 1ull << 40, bearings.data(), 1ull << 30, 2.0, res, true, &what) == MCL_ERR_OUT_OF_MEMORY);
  EXPECT(cast_check_call(nullptr, false, true, ~0ull, bearings.data(), ~0ull, 2.0, res, true, &what) == MCL_ERR_OUT_OF_MEMORY);

  // the plan: every ray once, in order, whatever the chunk; the pose area holds what a chunk touches
  const uint64_t shapes[][3] = {{1, 1, 64},   {3, 129, 64},  {65, 7, 100},     {1, 4097, 4096},   {5, 1, 64},        {2000, 180, 1 << 22},
                                {7, 64, 64},  {7, 64, 65},   {7, 64, 63},      {1000, 360, 4097}, {3, 5, 1ull << 40}, {4, 256, 0}};
  for (const auto& shape : shapes) {
    const uint64_t n = shape[0], B = shape[1];
    const CastPlan plan = cast_plan(n, B, shape[2]);
    EXPECT(plan.rays == n * B && plan.chunk_rays >= static_cast<uint64_t>(kCastChunkMin) && plan.chunk_rays <= kCastLaunchRays);
    EXPECT(plan.chunks == (plan.rays + plan.chunk_rays - 1) / plan.chunk_rays);
    uint64_t next = 0;
    for (uint64_t c = 0; c < plan.chunks; ++c) {
      const CastChunk k = cast_chunk_at(plan, B, c);
      EXPECT(k.first_ray == next && k.rays >= 1 && k.rays <= plan.chunk_rays);
      EXPECT(k.first_pose * B + k.first_bearing == k.first_ray && k.first_bearing < B);
      EXPECT(k.poses >= 1 && k.poses <= plan.chunk_poses && k.first_pose + k.poses <= n);
      EXPECT((k.first_ray + k.rays - 1) / B == k.first_pose + k.poses - 1);
      EXPECT(k.blocks == (k.rays + kCastBlock - 1) / kCastBlock && k.blocks <= kCastMaxBlocks);
      next += k.rays;
    }
    EXPECT(next == plan.rays);
  }
  // around the grid limit: one launch holds 2^30 workgroups of 256 rays, one ray more is a second launch of one workgroup
  for (const uint64_t extra : {0ull, 1ull}) {
    const uint64_t B = 1ull << 19, n = (kCastLaunchRays >> 19) + extra;
    const CastPlan plan = cast_plan(n, B, kCastLaunchRays);
    EXPECT(plan.chunks == 1 + extra);
    EXPECT(cast_chunk_at(plan, B, 0).blocks == kCastMaxBlocks);
    if (extra) EXPECT(cast_chunk_at(plan, B, 1).rays == B && cast_chunk_at(plan, B, 1).first_pose == n - 1);
  }
  {
    const CastPlan plan = cast_plan(kCastLaunchRays + 1, 1, ~0ull);  // a chunk above the launch's size is the launch's size
    EXPECT(plan.chunk_rays == kCastLaunchRays && plan.chunks == 2 && cast_chunk_at(plan, 1, 1).rays == 1 && cast_chunk_at(plan, 1, 1).blocks == 1);
  }
  EXPECT(cast_plan(0, 5, 64).chunks == 0 && cast_plan(5, 0, 64).chunks == 0 && cast_plan(0, 0, 64).chunk_poses == 0);
  std::puts("raycast_host_check OK");
  return 0;
}
