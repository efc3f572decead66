// range_table_host.cpp — the host rule of the beam model's range table (range_table_host.h).  Plain C++17, no HIP.
#include "range_table_host.h"

#include <algorithm>
#include <cmath>

namespace mcl {

mcl_status range_table_check(int32_t sensor_kind, uint32_t num_angles, uint64_t width, uint64_t height, double max_range, double resolution,
                             int64_t max_bytes, uint64_t* bytes, const char** what) {
  if (sensor_kind != MCL_SENSOR_BEAM) {
    *what = "only a beam context reads a range table";
    return MCL_ERR_INVALID_ARGUMENT;
  }
  if (num_angles < 1 || num_angles > kRangeTableMaxAngles) {
    *what = "num_angles must be 1 .. 4096";
    return MCL_ERR_INVALID_ARGUMENT;
  }
  if (width == 0 || height == 0 || !(resolution > 0.0) || !std::isfinite(max_range) || !(max_range > 0.0)) {
    *what = "no grid, or a max_range that is not a finite positive number";
    return MCL_ERR_INVALID_ARGUMENT;
  }
  if (!(max_range / resolution < kRangeTableMaxReachCells)) {
    *what = "max_range / resolution must stay below 2^27 - 2 cells";
    return MCL_ERR_INVALID_ARGUMENT;
  }
  // width * height * num_angles * 4, every product checked against what is left of 64 bits before it is formed
  const uint64_t cap = max_bytes > 0 ? static_cast<uint64_t>(max_bytes) : 0;
  const uint64_t row = static_cast<uint64_t>(num_angles) * sizeof(uint32_t);  // <= 16 384
  bool fits = width <= UINT64_MAX / height;
  const uint64_t cells = fits ? width * height : 0;
  fits = fits && cells <= UINT64_MAX / row;
  if (!fits || cells * row > cap) {
    *what = "the table would be larger than range_table_max_bytes";
    return MCL_ERR_OUT_OF_MEMORY;
  }
  *bytes = cells * row;
  return MCL_OK;
}

RangeTablePlan range_table_plan(uint64_t cells, uint32_t num_angles, uint64_t launch_entries) {
  RangeTablePlan plan{};
  plan.entries = cells * num_angles;  // (range_table_check has bounded the product)
  plan.launch_entries = std::clamp<uint64_t>(launch_entries, kRangeTableBlock, kRangeTableLaunchEntries) / kRangeTableBlock * kRangeTableBlock;
  plan.launches = (plan.entries + plan.launch_entries - 1) / plan.launch_entries;
  return plan;
}

RangeTableLaunch range_table_launch_at(const RangeTablePlan& plan, uint64_t c) {
  RangeTableLaunch l{};
  l.first_entry = c * plan.launch_entries;
  l.entries = std::min<uint64_t>(plan.launch_entries, plan.entries - l.first_entry);
  l.blocks = (l.entries + kRangeTableBlock - 1) / kRangeTableBlock;
  return l;
}

void range_table_bearings(uint32_t num_angles, double* cs_out) {
  const double step = 2.0 * 3.14159265358979323846264338327950288 / static_cast<double>(num_angles);
  for (uint32_t k = 0; k < num_angles; ++k) {
    const double a = static_cast<double>(k) * step;
    cs_out[2 * k] = std::cos(a);
    cs_out[2 * k + 1] = std::sin(a);
  }
}

}  // namespace mcl
