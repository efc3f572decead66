// range_table_host.h — the host rule of the beam model's range table (include/beluga_mcl.h "Range table for the beam model"): the checks
// of mcl_build_range_table, the chunk plan of the build and the bearing table.  Plain C++17, no HIP: tests/test_range_table_host_cpu.py
// holds it on the CPU, tests/cpp/range_table_host_check.cpp runs it under the sanitizers.
//
// The table holds, per cell (x, y) of the grid and heading bin k of A, the squared cell distance between the cell and the cell the exact
// rule's cast from it hits - the cast from the cell's CENTRE to the far end along the bin's bearing (cos, sin)(k * 2 pi / A), all in the
// grid frame - or kRangeTableNoHit.  What it discards of the exact rule: the source's position inside its cell, and the heading within a
// bin.
#pragma once

#include <cstdint>

#include "beluga_mcl.h"

namespace mcl {

constexpr uint32_t kRangeTableMaxAngles = 4096;
constexpr uint32_t kRangeTableNoHit = 0xFFFFFFFFu;                              // the entry of a cast that hits nothing
constexpr uint32_t kRangeTableFarthest = 0xFFFFFFFEu;                           // squared distances saturate here (a hit 65 536 cells away or more)
constexpr int64_t kRangeTableMaxBytesDefault = 4ll << 30;                       // option range_table_max_bytes
constexpr uint32_t kRangeTableBlock = 256;                                      // entries of a workgroup of k_build_range_table (kBlock)
constexpr uint64_t kRangeTableMaxBlocks = 1ull << 22;                           // workgroups of one launch: far below a grid dimension's 2^31 - 1
constexpr uint64_t kRangeTableLaunchEntries = kRangeTableMaxBlocks * kRangeTableBlock;  // 2^30 entries, 4 GiB of table, per launch
// The walks' own bound on max_range / resolution (kernels.h restates it as kBeamMaxReachCells and asserts the two equal).
constexpr double kRangeTableMaxReachCells = 134217726.0;  // 2^27 - 2

// What mcl_build_range_table checks before anything is allocated, in this order: the sensor model (only the beam model's cycle reads a
// table), num_angles in 1 .. 4096, the reach max_range / resolution below 2^27 - 2 cells, and width * height * num_angles * 4 bytes -
// formed without overflow - against max_bytes (MCL_ERR_OUT_OF_MEMORY above it).  MCL_OK with *bytes set, or the status with *what set.
mcl_status range_table_check(int32_t sensor_kind, uint32_t num_angles, uint64_t width, uint64_t height, double max_range, double resolution,
                             int64_t max_bytes, uint64_t* bytes, const char** what);

// The entries cell * A + k of the build, cut into launches of at most `launch_entries` (a multiple of kRangeTableBlock; the last one shorter).
struct RangeTablePlan {
  uint64_t entries;         // cells * A
  uint64_t launch_entries;  // entries of a full launch
  uint64_t launches;
};
struct RangeTableLaunch {
  uint64_t first_entry, entries;
  uint64_t blocks;  // workgroups of the launch
};
RangeTablePlan range_table_plan(uint64_t cells, uint32_t num_angles, uint64_t launch_entries = kRangeTableLaunchEntries);
RangeTableLaunch range_table_launch_at(const RangeTablePlan& plan, uint64_t c);

// cs_out[2 k], [2 k + 1] = std::cos, std::sin of double(k) * (2 pi / A): the bearings of the bins, computed here and nowhere else - the
// device and mcl_range_table_bearings read this table.
void range_table_bearings(uint32_t num_angles, double* cs_out);

}  // namespace mcl
