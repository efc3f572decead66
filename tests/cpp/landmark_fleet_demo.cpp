// landmark_fleet_demo.cpp - a fleet of three landmark filters through the header-only facade: beluga_amd::AmclBatch over
// AmclLandmarkBatchSpec members with the small cycle on, update() with one vector of detections per member (mcl_landmark_batch_update).
// Prints one line per member and update ("x y theta", members in order within a cycle), then "launches <kernel_launches> fused
// <members_landmark_fused>", so that a test can compare them with the Python facade on the same inputs.  Exit code 3: no usable GPU.
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "beluga_amd/amcl.hpp"

int main() {
  // 12 landmarks on a circle of 5 m at heights 0.5 / 1.0 / 1.5, categories 0 .. 3; the robots stand at the origin
  std::vector<beluga_amd::LandmarkPositionDetection> landmarks;
  for (int k = 0; k < 12; ++k)
    landmarks.push_back({{5.0 * std::cos(k * M_PI / 6), 5.0 * std::sin(k * M_PI / 6), 0.5 * (1 + k % 3)}, static_cast<std::uint32_t>(k % 4)});
  const beluga_amd::LandmarkMap map{beluga_amd::LandmarkMapBoundaries{{-6.0, -6.0, 0.0}, {6.0, 6.0, 2.0}}, landmarks};
  beluga_amd::LandmarkModelParam sensor;
  sensor.sigma_range = 0.2;
  sensor.sigma_bearing = 0.1;
  sensor.random_prob = 1e-3;
  const std::size_t sizes[3] = {2000, 1000, 500};
  std::vector<beluga_amd::AmclLandmarkBatchSpec> specs;
  std::vector<std::vector<beluga_amd::LandmarkPositionDetection>> detections(3);
  for (std::size_t i = 0; i < 3; ++i) {
    beluga_amd::AmclParams params;
    params.min_particles = sizes[i];
    params.max_particles = sizes[i];
    specs.push_back({map, beluga_amd::DifferentialDriveModelParam{0.1, 0.05, 0.1, 0.05}, sensor, params, 7 + i, true, {}});
    for (std::size_t k = i; k < landmarks.size(); k += 2 + i) detections[i].push_back(landmarks[k]);  // member i sees every (2 + i)-th one
  }
  try {
    beluga_amd::AmclBatch batch{specs};
    for (auto& member : batch.members()) {
      if (!member.landmark_small_cycle()) return 1;
      member.initialize(beluga_amd::SE2d{0.0, 0.0, 0.0}, beluga_amd::Matrix3d{0.04, 0, 0, 0, 0.04, 0, 0, 0, 0.01});
    }
    const std::vector<beluga_amd::SE2d> controls(3, beluga_amd::SE2d{0.0, 0.0, 0.0});
    for (int c = 0; c < 4; ++c) {
      for (auto& member : batch.members()) member.force_update();
      const auto estimates = batch.update(controls, detections);
      for (const auto& est : estimates) {
        if (!est) return 2;
        std::printf("%.17g %.17g %.17g\n", est->first.x, est->first.y, est->first.angle());
      }
    }
    std::printf("launches %llu fused %llu\n", static_cast<unsigned long long>(batch.counter("kernel_launches")),
                static_cast<unsigned long long>(batch.counter("members_landmark_fused")));
  } catch (const std::runtime_error& e) {
    std::printf("runtime_error: %s\n", e.what());
    return 3;
  }
  return 0;
}
