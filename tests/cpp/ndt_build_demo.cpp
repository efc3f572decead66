// ndt_build_demo.cpp - the NDT map built on the device through the header-only facade: a filter that starts from an occupancy grid
// builds its own map (Amcl::build_ndt_map), reads it back (Amcl::ndt_map) and finds the cells NDTMap2d::from_occupancy_grid fits on
// the host, bit for bit; the same for a point cloud.
// Exit code 0: equal; 1: a difference; 3: no usable GPU (the library has no CPU fallback).
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <utility>
#include <vector>

#include "beluga_amd/amcl.hpp"

namespace {
bool same(const beluga_amd::NDTMap2d& a, const beluga_amd::NDTMap2d& b) {
  if (a.size() != b.size() || a.resolution() != b.resolution()) return false;
  for (std::size_t i = 0; i < a.size(); ++i)
    if (a.keys()[i] != b.keys()[i] || a.cells()[i].mean != b.cells()[i].mean || a.cells()[i].covariance != b.cells()[i].covariance) return false;
  return true;
}
}  // namespace

int main() {
  // a room of 8 m x 6 m at 0.05 m cells, walls two cells thick, around the origin
  const std::uint32_t W = 160, H = 120;
  std::vector<std::int8_t> cells(static_cast<std::size_t>(W) * H, 0);
  for (std::uint32_t y = 0; y < H; ++y)
    for (std::uint32_t x = 0; x < W; ++x)
      if (x < 2 || y < 2 || x >= W - 2 || y >= H - 2) cells[static_cast<std::size_t>(y) * W + x] = 100;
  beluga_amd::OccupancyGridView grid;
  grid.cells = cells.data();
  grid.width = W;
  grid.height = H;
  grid.resolution = 0.05;
  grid.origin = beluga_amd::SE2d{0.0, -4.0, -3.0};
  const beluga_amd::NDTMap2d host = beluga_amd::NDTMap2d::from_occupancy_grid(grid, 0.5);
  if (host.size() < 20) return 1;
  std::vector<std::pair<double, double>> cloud;
  for (int i = 0; i < 4000; ++i) cloud.emplace_back(-3.0 + 0.0015 * i, 0.3 * ((i * 7919) % 1000) / 1000.0 + 0.001 * (i % 13));
  const beluga_amd::NDTMap2d host_cloud = beluga_amd::NDTMap2d::from_points(cloud, 0.5);
  beluga_amd::NDTModelParam2d sensor;
  sensor.minimum_likelihood = 0.01;
  sensor.d2 = 0.6;
  beluga_amd::AmclParams params;
  params.min_particles = 500;
  params.max_particles = 500;
  try {
    beluga_amd::Amcl amcl{host_cloud, beluga_amd::DifferentialDriveModelParam{0.1, 0.05, 0.1, 0.05}, sensor, params, 7};
    if (!same(amcl.ndt_map(), host_cloud)) return 1;
    amcl.build_ndt_map(grid, 0.5);
    const beluga_amd::NDTMap2d built = amcl.ndt_map();
    if (!same(built, host)) return 1;
    amcl.build_ndt_map(cloud, 0.5);
    if (!same(amcl.ndt_map(), host_cloud)) return 1;
    std::printf("%zu cells from the grid, %zu from the cloud\n", built.size(), host_cloud.size());
  } catch (const std::runtime_error& e) {
    std::printf("runtime_error: %s\n", e.what());
    return 3;
  }
  return 0;
}
