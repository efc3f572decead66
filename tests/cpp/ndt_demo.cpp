// ndt_demo.cpp - the NDT filter of ndt_amcl_node through the header-only facade: code written for
// beluga_amcl's `NdtAmcl<Motion, Policy>` (ndt_amcl_node.hpp:77-84) switches by the alias below.
// Prints one line per update ("x y theta"), so that a test can compare it with the Python facade on the same inputs.
// Exit code 3: no usable GPU (the library has no CPU fallback).
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "beluga_amd/amcl.hpp"

using NdtAmcl = beluga_amd::Amcl;

int main() {
  // a square room of NDT cells, one metre each, walls along x = +-4 and y = +-4
  std::vector<beluga_amd::NDTMap2d::key_type> keys;
  std::vector<beluga_amd::NDTCell2d> cells;
  for (int k = -4; k < 4; ++k) {
    const double c = k + 0.5;
    keys.push_back({k, -4});
    cells.push_back({{c, -3.9}, {0.08, 0.0, 0.0, 0.002}});
    keys.push_back({k, 3});
    cells.push_back({{c, 3.9}, {0.08, 0.0, 0.0, 0.002}});
    keys.push_back({-4, k});
    cells.push_back({{-3.9, c}, {0.002, 0.0, 0.0, 0.08}});
    keys.push_back({3, k});
    cells.push_back({{3.9, c}, {0.002, 0.0, 0.0, 0.08}});
  }
  // (the corner keys appear twice above: keep the first)
  std::vector<beluga_amd::NDTMap2d::key_type> k2;
  std::vector<beluga_amd::NDTCell2d> c2;
  for (std::size_t i = 0; i < keys.size(); ++i) {
    bool seen = false;
    for (const auto& k : k2) seen = seen || k == keys[i];
    if (!seen) {
      k2.push_back(keys[i]);
      c2.push_back(cells[i]);
    }
  }
  const beluga_amd::NDTMap2d map{k2, c2, 1.0};
  beluga_amd::NDTModelParam2d sensor;
  sensor.minimum_likelihood = 0.01;
  sensor.d1 = 1.0;
  sensor.d2 = 0.6;
  beluga_amd::AmclParams params;
  params.min_particles = 2000;
  params.max_particles = 2000;
  try {
    NdtAmcl amcl{map, beluga_amd::DifferentialDriveModelParam{0.1, 0.05, 0.1, 0.05}, sensor, params, 7};
    if (map.size() != k2.size() || !map.data_at({0, 3}) || map.data_at({0, 0})) return 1;
    amcl.initialize(beluga_amd::SE2d{0.0, 0.0, 0.0}, beluga_amd::Matrix3d{0.04, 0, 0, 0, 0.04, 0, 0, 0, 0.01});
    for (int c = 0; c < 4; ++c) {
      // points on the walls as seen from the origin, every 2 degrees
      std::vector<std::pair<double, double>> scan;
      for (int b = 0; b < 180; ++b) {
        const double a = b * 2.0 * M_PI / 180.0, ca = std::cos(a), sa = std::sin(a);
        const double t = 3.9 / std::max(std::abs(ca), std::abs(sa));
        scan.emplace_back(t * ca, t * sa);
      }
      amcl.force_update();
      const auto est = amcl.update(beluga_amd::SE2d{0.0, 0.0, 0.0}, scan);
      if (!est) return 2;
      std::printf("%.17g %.17g %.17g\n", est->first.x, est->first.y, est->first.angle());
    }
  } catch (const std::runtime_error& e) {
    std::printf("runtime_error: %s\n", e.what());
    return 3;
  }
  return 0;
}
