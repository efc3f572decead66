// range_table_demo.cpp - the range table of the beam model through the header-only facade: beluga_amd::Amcl::build_range_table,
// range_table_info, range_table_bearings, range_table and drop_range_table (ros_amcl.hpp forwards its calls of the same names to
// these).  Prints the grid ("grid W H resolution", "origin ...", one "row ..." line per row), "angles A",
// the bearings ("bearing c s"), the table ("entry cell k r2", every entry), the states ("state cos sin x y"), the points ("point x y")
// and the likelihoods over the table ("table_likelihood v") and, after the drop, on the exact walk ("exact_likelihood v"), so that a test
// can hold them to the reference and to the Python facade.  Exit code 3: no usable GPU (the library has no CPU fallback).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <utility>
#include <vector>

#include "beluga_amd/amcl.hpp"

namespace {
constexpr std::uint32_t kW = 37, kH = 29, kAngles = 24;
constexpr double kResolution = 0.1, kMaxRange = 2.5;
}  // namespace

int main() {
  std::vector<std::int8_t> cells(kW * kH, 0);
  for (std::uint32_t y = 0; y < kH; ++y)
    for (std::uint32_t x = 0; x < kW; ++x) {
      if (x == 0 || y == 0 || x == kW - 1 || y == kH - 1) cells[y * kW + x] = 100;   // the walls
      if (x >= 20 && x < 23 && y >= 11 && y < 15) cells[y * kW + x] = 100;           // a pillar
      if (x >= 8 && x < 10 && y >= 20 && y < 22) cells[y * kW + x] = -1;             // a patch nobody has seen
    }
  beluga_amd::OccupancyGridView grid;
  grid.cells = cells.data();
  grid.width = kW;
  grid.height = kH;
  grid.resolution = kResolution;
  grid.origin = beluga_amd::SE2d{0.3, -1.0, 0.5};
  std::printf("grid %u %u %.17g\n", kW, kH, kResolution);
  std::printf("origin %.17g %.17g %.17g %.17g\n", grid.origin.data()[0], grid.origin.data()[1], grid.origin.data()[2], grid.origin.data()[3]);
  for (std::uint32_t y = 0; y < kH; ++y) {
    std::printf("row");
    for (std::uint32_t x = 0; x < kW; ++x) std::printf(" %d", cells[y * kW + x]);
    std::printf("\n");
  }
  std::vector<beluga_amd::SE2d> states;
  for (int k = 0; k < 5; ++k) states.push_back(beluga_amd::SE2d{0.4 * k - 0.5, -0.4 + 0.35 * k, 1.1 + 0.3 * k});
  states.push_back(beluga_amd::SE2d{0.0, 30.0, 30.0});  // far off the map: nothing is hit
  std::vector<std::pair<double, double>> points;
  for (int b = 0; b < 16; ++b) points.emplace_back((0.4 + 0.11 * b) * std::cos(0.07 + b * M_PI / 8), (0.4 + 0.11 * b) * std::sin(0.07 + b * M_PI / 8));
  try {
    beluga_amd::AmclParams params;
    params.min_particles = 100;
    params.max_particles = 100;
    beluga_amd::BeamModelParam beam;
    beam.beam_max_range = kMaxRange;
    beluga_amd::Amcl amcl{grid, beluga_amd::DifferentialDriveModelParam{0.1, 0.05, 0.1, 0.05}, beam, params, 7};
    if (amcl.range_table_info().built != 0) return 2;
    amcl.build_range_table(kAngles);
    const mcl_range_table_info info = amcl.range_table_info();
    if (info.built != 1 || info.num_angles != kAngles || info.width != kW || info.height != kH ||
        info.bytes != static_cast<std::uint64_t>(kW) * kH * kAngles * 4 || info.builds != 1 || info.lut_launches != 0)
      return 2;
    const std::vector<std::pair<double, double>> bearings = amcl.range_table_bearings();
    if (bearings.size() != kAngles) return 2;
    std::printf("angles %u\n", kAngles);
    for (const auto& b : bearings) std::printf("bearing %.17g %.17g\n", b.first, b.second);
    const std::vector<std::uint32_t> table = amcl.range_table(0, static_cast<std::uint64_t>(kW) * kH);
    if (table.size() != static_cast<std::size_t>(kW) * kH * kAngles) return 2;
    for (std::size_t e = 0; e < table.size(); ++e) std::printf("entry %zu %zu %u\n", e / kAngles, e % kAngles, table[e]);
    if (amcl.range_table(5 * kW + 3, 2) != std::vector<std::uint32_t>(table.begin() + (5 * kW + 3) * kAngles, table.begin() + (5 * kW + 5) * kAngles)) return 2;
    for (const auto& s : states) std::printf("state %.17g %.17g %.17g %.17g\n", s.data()[0], s.data()[1], s.data()[2], s.data()[3]);
    for (const auto& p : points) std::printf("point %.17g %.17g\n", p.first, p.second);
    for (const double v : amcl.likelihoods(states, points)) std::printf("table_likelihood %.17g\n", v);
    amcl.drop_range_table();
    if (amcl.range_table_info().built != 0 || amcl.range_table_info().builds != 1) return 2;
    for (const double v : amcl.likelihoods(states, points)) std::printf("exact_likelihood %.17g\n", v);
    bool threw = false;
    try {
      amcl.build_range_table(0);
    } catch (const std::runtime_error&) {
      threw = true;
    }
    if (!threw) return 2;
  } catch (const std::runtime_error& e) {
    std::printf("runtime_error: %s\n", e.what());
    return 3;
  }
  return 0;
}
