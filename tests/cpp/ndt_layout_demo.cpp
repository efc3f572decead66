// ndt_layout_demo.cpp - the NDT map layout mode through the header-only facade: the defaulted trailing argument of the NDT
// constructor, Amcl::set_ndt_map_layout and Amcl::ndt_map_layout.  A map of two clusters 20000 keys apart is refused by the default
// (dense) layout and taken under mode 1 into the hashed table; a map that fits stays dense under mode 1 and goes into the table under
// mode 2 at the next update_map, not before.
// Exit code 0: as expected; 1: a difference (the line is printed); 3: no usable GPU (the library has no CPU fallback).
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "beluga_amd/amcl.hpp"

#define EXPECT(cond)                                   \
  do {                                                 \
    if (!(cond)) {                                     \
      std::printf("line %d: %s\n", __LINE__, #cond); \
      return 1;                                        \
    }                                                  \
  } while (0)

int main() {
  using layout = std::pair<std::int32_t, std::int32_t>;
  std::vector<std::pair<double, double>> near_cloud, both_clouds;
  for (int i = 0; i < 600; ++i) near_cloud.emplace_back(1.0 + 0.01 * i, 1.0 + 5.0 * ((i * 7919) % 1000) / 1000.0);
  both_clouds = near_cloud;
  for (const auto& p : near_cloud) both_clouds.emplace_back(p.first + 20000.0, p.second + 20000.0);
  const beluga_amd::NDTMap2d near_map = beluga_amd::NDTMap2d::from_points(near_cloud, 1.0);
  const beluga_amd::NDTMap2d far_map = beluga_amd::NDTMap2d::from_points(both_clouds, 1.0);
  EXPECT(near_map.size() >= 10 && far_map.size() > near_map.size() + 10);
  const beluga_amd::DifferentialDriveModelParam motion{0.1, 0.05, 0.1, 0.05};
  beluga_amd::NDTModelParam2d sensor;
  sensor.minimum_likelihood = 0.01;
  sensor.d2 = 0.6;
  beluga_amd::AmclParams params;
  params.min_particles = 64;
  params.max_particles = 64;
  try {
    beluga_amd::Amcl dense{near_map, motion, sensor, params, 7};  // the argument left out: mode 0
    EXPECT(dense.ndt_map_layout() == (layout{0, 0}));
    bool refused = false;
    try {
      beluga_amd::Amcl too_large{far_map, motion, sensor, params, 7};
    } catch (const std::runtime_error& e) {
      refused = std::string(e.what()).find("2^26") != std::string::npos;
    }
    EXPECT(refused);
    beluga_amd::Amcl sparse{far_map, motion, sensor, params, 7, 0, {}, 1};  // the trailing argument, in front of the first install
    EXPECT(sparse.ndt_map_layout() == (layout{1, 1}));
    EXPECT(sparse.ndt_map().size() == far_map.size());
    beluga_amd::Amcl automatic{near_map, motion, sensor, params, 7, 0, {}, 1};
    EXPECT(automatic.ndt_map_layout() == (layout{1, 0}));
    dense.set_ndt_map_layout(2);
    EXPECT(dense.ndt_map_layout() == (layout{2, 0}));  // the installed map stays as it is
    dense.update_map(near_map);
    EXPECT(dense.ndt_map_layout() == (layout{2, 1}));
    dense.set_ndt_map_layout(1);
    dense.build_ndt_map(both_clouds, 1.0);
    EXPECT(dense.ndt_map_layout() == (layout{1, 1}) && dense.ndt_map().size() == far_map.size());
    bool invalid = false;
    try {
      dense.set_ndt_map_layout(3);
    } catch (const std::exception&) {
      invalid = true;
    }
    EXPECT(invalid && dense.ndt_map_layout() == (layout{1, 1}));
    std::printf("%zu cells dense, %zu cells hashed\n", near_map.size(), far_map.size());
  } catch (const std::runtime_error& e) {
    std::printf("runtime_error: %s\n", e.what());
    return 3;
  }
  return 0;
}
