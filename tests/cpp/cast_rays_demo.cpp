// cast_rays_demo.cpp - ray casting as a function through the header-only facade: Amcl::cast_rays(states, bearings, max_range) on a
// likelihood-field and on a beam filter over a small room with a pillar.  Prints the grid ("grid W H resolution", then one "row ..." line
// per row), the states ("state cos sin x y"), the bearings ("bearing c s") and, per filter, "visited N" and one line per ray
// ("ray range hit_cell"), so that a test can cast the same rays through the Python facade.  Exit code 3: no usable GPU (the library has no
// CPU fallback).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <utility>
#include <vector>

#include "beluga_amd/amcl.hpp"

namespace {

constexpr std::uint32_t kW = 37, kH = 29;
constexpr double kResolution = 0.1, kMaxRange = 2.5;

template <class Sensor>
int run(const beluga_amd::OccupancyGridView& grid, const Sensor& sensor, const std::vector<beluga_amd::SE2d>& states,
        const std::vector<std::pair<double, double>>& bearings) {
  beluga_amd::AmclParams params;
  params.min_particles = 100;
  params.max_particles = 100;
  beluga_amd::Amcl amcl{grid, beluga_amd::DifferentialDriveModelParam{0.1, 0.05, 0.1, 0.05}, sensor, params, 7};
  std::vector<std::int64_t> hits;
  std::uint64_t visited = 0;
  const std::vector<double> ranges = amcl.cast_rays(states, bearings, kMaxRange, &hits, &visited);
  if (ranges.size() != states.size() * bearings.size() || hits.size() != ranges.size()) return 2;
  std::printf("visited %llu\n", static_cast<unsigned long long>(visited));
  for (std::size_t k = 0; k < ranges.size(); ++k) std::printf("ray %.17g %lld\n", ranges[k], static_cast<long long>(hits[k]));
  if (amcl.cast_rays(states, bearings, kMaxRange) != ranges) return 2;  // the ranges alone
  return amcl.cast_rays({}, bearings, kMaxRange).empty() ? 0 : 2;
}

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
  std::vector<std::pair<double, double>> bearings;
  for (int b = 0; b < 24; ++b) bearings.emplace_back(std::cos(b * M_PI / 12), std::sin(b * M_PI / 12));
  for (const auto& s : states) std::printf("state %.17g %.17g %.17g %.17g\n", s.data()[0], s.data()[1], s.data()[2], s.data()[3]);
  for (const auto& b : bearings) std::printf("bearing %.17g %.17g\n", b.first, b.second);
  try {
    beluga_amd::LikelihoodFieldModelParam lf;
    lf.max_obstacle_distance = 1.0;
    if (const int rc = run(grid, lf, states, bearings)) return rc;
    beluga_amd::BeamModelParam beam;
    beam.beam_max_range = kMaxRange;
    if (const int rc = run(grid, beam, states, bearings)) return rc;
  } catch (const std::runtime_error& e) {
    std::printf("runtime_error: %s\n", e.what());
    return 3;
  }
  return 0;
}
