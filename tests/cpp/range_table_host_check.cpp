// range_table_host_check.cpp - the host rule of the beam model's range table (beluga_amd/csrc/range_table_host.cpp) as a program of its
// own, meant to be built with -fsanitize=address,undefined: the checks at their edges, products that would overflow, every launch of
// plans small and huge, and the bearing table written into buffers of exactly its size.  Prints "range_table_host_check OK".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "range_table_host.h"

namespace {

int failures = 0;
#define EXPECT(cond)                                            \
  do {                                                          \
    if (!(cond)) {                                              \
      std::printf("line %d: %s\n", __LINE__, #cond);            \
      ++failures;                                               \
    }                                                           \
  } while (0)

mcl_status check(uint32_t A, uint64_t W, uint64_t H, int64_t cap, uint64_t* bytes, double max_range = 3.0, double resolution = 0.05,
                 int32_t kind = MCL_SENSOR_BEAM) {
  const char* what = nullptr;
  *bytes = 0;
  const mcl_status s = mcl::range_table_check(kind, A, W, H, max_range, resolution, cap, bytes, &what);
  EXPECT((s == MCL_OK) == (what == nullptr));
  return s;
}

}  // namespace

int main() {
  constexpr int64_t kCap = mcl::kRangeTableMaxBytesDefault;
  constexpr uint64_t kMax = std::numeric_limits<uint64_t>::max();
  uint64_t bytes = 0;
  EXPECT(check(0, 10, 10, kCap, &bytes) == MCL_ERR_INVALID_ARGUMENT);
  EXPECT(check(1, 10, 10, kCap, &bytes) == MCL_OK && bytes == 400);
  EXPECT(check(4096, 10, 10, kCap, &bytes) == MCL_OK && bytes == 100ull * 4096 * 4);
  EXPECT(check(4097, 10, 10, kCap, &bytes) == MCL_ERR_INVALID_ARGUMENT);
  EXPECT(check(360, 10, 10, kCap, &bytes, 3.0, 0.05, MCL_SENSOR_LIKELIHOOD_FIELD) == MCL_ERR_INVALID_ARGUMENT);
  EXPECT(check(65, 257, 130, 257 * 130 * 65 * 4, &bytes) == MCL_OK);
  EXPECT(check(65, 257, 130, 257 * 130 * 65 * 4 - 1, &bytes) == MCL_ERR_OUT_OF_MEMORY && bytes == 0);
  EXPECT(check(64, 4096, 4096, kCap, &bytes) == MCL_OK && bytes == static_cast<uint64_t>(kCap));
  EXPECT(check(65, 4096, 4096, kCap, &bytes) == MCL_ERR_OUT_OF_MEMORY);
  EXPECT(check(1, 10, 10, 0, &bytes) == MCL_ERR_OUT_OF_MEMORY);
  EXPECT(check(1, 10, 10, std::numeric_limits<int64_t>::min(), &bytes) == MCL_ERR_OUT_OF_MEMORY);
  const int64_t huge = std::numeric_limits<int64_t>::max();
  EXPECT(check(1, kMax, kMax, huge, &bytes) == MCL_ERR_OUT_OF_MEMORY);
  EXPECT(check(4096, kMax, 1, huge, &bytes) == MCL_ERR_OUT_OF_MEMORY);
  EXPECT(check(1, 1ull << 32, 1ull << 32, huge, &bytes) == MCL_ERR_OUT_OF_MEMORY);
  EXPECT(check(4, 1ull << 31, 1ull << 31, huge, &bytes) == MCL_ERR_OUT_OF_MEMORY);
  EXPECT(check(1, 1ull << 30, 1ull << 30, huge, &bytes) == MCL_OK && bytes == 1ull << 62);
  EXPECT(check(8, 10, 10, kCap, &bytes, (mcl::kRangeTableMaxReachCells - 1.0) * 0.0625, 0.0625) == MCL_OK);
  EXPECT(check(8, 10, 10, kCap, &bytes, mcl::kRangeTableMaxReachCells * 0.0625, 0.0625) == MCL_ERR_INVALID_ARGUMENT);
  EXPECT(check(8, 10, 10, kCap, &bytes, std::nan(""), 0.05) == MCL_ERR_INVALID_ARGUMENT);
  EXPECT(check(8, 10, 10, kCap, &bytes, INFINITY, 0.05) == MCL_ERR_INVALID_ARGUMENT);
  EXPECT(check(8, 0, 10, kCap, &bytes) == MCL_ERR_INVALID_ARGUMENT);

  // every launch of a plan covers its entries once, in whole workgroups but for the last
  const uint64_t launch_sizes[] = {0, 1, 255, 256, 257, 1000, 25600, 1ull << 30, (1ull << 30) + 1, kMax};
  const uint64_t shapes[][2] = {{1, 1}, {1, 4096}, {257 * 130, 65}, {31 * 33, 63}, {7, 64}, {1000, 360}};
  for (const auto& shape : shapes)
    for (const uint64_t size : launch_sizes) {
      const mcl::RangeTablePlan plan = mcl::range_table_plan(shape[0], static_cast<uint32_t>(shape[1]), size);
      EXPECT(plan.entries == shape[0] * shape[1]);
      EXPECT(plan.launch_entries % mcl::kRangeTableBlock == 0 && plan.launch_entries >= mcl::kRangeTableBlock &&
             plan.launch_entries <= mcl::kRangeTableLaunchEntries);
      if (plan.launches > 100000) continue;
      uint64_t next = 0;
      for (uint64_t c = 0; c < plan.launches; ++c) {
        const mcl::RangeTableLaunch l = mcl::range_table_launch_at(plan, c);
        EXPECT(l.first_entry == next && l.entries >= 1 && l.entries <= plan.launch_entries);
        EXPECT(l.blocks == (l.entries + mcl::kRangeTableBlock - 1) / mcl::kRangeTableBlock && l.blocks <= mcl::kRangeTableMaxBlocks);
        EXPECT(c + 1 == plan.launches || l.entries == plan.launch_entries);
        next += l.entries;
      }
      EXPECT(next == plan.entries);
    }
  {
    const mcl::RangeTablePlan plan = mcl::range_table_plan((1ull << 32) - 2, 4096);  // the largest table a grid can ask for
    EXPECT(plan.entries == ((1ull << 32) - 2) * 4096);
    const mcl::RangeTableLaunch last = mcl::range_table_launch_at(plan, plan.launches - 1);
    EXPECT(last.first_entry + last.entries == plan.entries && last.blocks <= mcl::kRangeTableMaxBlocks);
  }

  // the bearing table, written into a buffer of exactly 2 A doubles
  for (const uint32_t A : {1u, 2u, 63u, 64u, 65u, 360u, 4096u}) {
    std::vector<double> cs(2 * static_cast<size_t>(A));
    mcl::range_table_bearings(A, cs.data());
    EXPECT(cs[0] == 1.0 && cs[1] == 0.0);
    for (uint32_t k = 0; k < A; ++k) {
      const double norm = cs[2 * k] * cs[2 * k] + cs[2 * k + 1] * cs[2 * k + 1];
      EXPECT(std::fabs(norm - 1.0) < 1e-15);
    }
    if (A % 4 == 0) EXPECT(std::fabs(cs[2 * (A / 4)]) < 1e-15 && std::fabs(cs[2 * (A / 4) + 1] - 1.0) < 1e-15);
  }
  if (failures) return 1;
  std::printf("range_table_host_check OK\n");
  return 0;
}
