// raycast_host.h — the host rule of mcl_cast_rays* (include/beluga_mcl.h "Ray casting as a function"): the checks of the call's
// arguments and the chunk plan.  Plain C++17, no HIP: tests/test_raycast_host_cpu.py holds it on the CPU, tests/cpp/raycast_host_check.cpp
// runs it under the sanitizers.
#pragma once

#include <cstdint>

#include "beluga_mcl.h"

namespace mcl {

// Option cast_chunk: the rays a chunk of the host form holds - what bounds the call's device memory.  The result does not depend on it.
constexpr int64_t kCastChunkMin = 64, kCastChunkMax = 1ll << 28, kCastChunkDefault = 1ll << 22;
constexpr uint32_t kCastBlock = 256;                                   // rays of a workgroup of k_cast_rays (kBlock)
constexpr uint64_t kCastMaxBlocks = 1ull << 30;                        // workgroups of one launch: below a grid dimension's 2^31 - 1
constexpr uint64_t kCastLaunchRays = kCastMaxBlocks * kCastBlock;      // the most rays of one launch (the device form's chunk)
// Counts beyond these cannot lie in memory (2^40 poses are 32 TB, 2^36 bearings 1 TB, 2^62 ranges more than any address space): refused
// as out of memory before anything is multiplied.
constexpr uint64_t kCastMaxPoses = 1ull << 40, kCastMaxBearings = 1ull << 36, kCastMaxRays = 1ull << 62;
// The walks' own bound on max_range / resolution (kernels.h restates it as kBeamMaxReachCells and asserts the two equal).
constexpr double kCastMaxReachCells = 134217726.0;  // 2^27 - 2

// What is wrong with max_range on a grid of this resolution, or nullptr.
const char* cast_check_range(double max_range, double resolution);
// What mcl_cast_rays* check of their arguments once the context has passed, in this order: max_range, the counts, (both counts non-zero:)
// the null pointers and the finite values.  poses == nullptr with check_poses == false: the device form, whose poses are device memory.
// MCL_OK, or the status with *what set.
mcl_status cast_check_call(const double* poses, bool check_poses, bool have_poses, uint64_t n, const double* bearings_cs, uint64_t num_bearings,
                           double max_range, double resolution, bool have_ranges_out, const char** what);

// The n * B rays in the flattened order i * B + b, cut into chunks of `chunk_rays` (the last one shorter).
struct CastPlan {
  uint64_t rays;         // n * B
  uint64_t chunk_rays;   // rays of a full chunk, 1 .. kCastLaunchRays
  uint64_t chunks;
  uint64_t chunk_poses;  // the most poses a chunk touches: what the chunk's pose area holds
};
struct CastChunk {
  uint64_t first_ray, rays;  // the chunk's range of the flattened order
  uint64_t first_pose;       // first_ray / B
  uint64_t first_bearing;    // first_ray % B
  uint64_t poses;            // poses the chunk touches
  uint64_t blocks;           // workgroups of its launch
};
// chunk_rays: the option's value for the host form (clamped to kCastChunkMin .. kCastChunkMax here), kCastLaunchRays for the device form.
CastPlan cast_plan(uint64_t n, uint64_t num_bearings, uint64_t chunk_rays);
CastChunk cast_chunk_at(const CastPlan& plan, uint64_t num_bearings, uint64_t c);

}  // namespace mcl
