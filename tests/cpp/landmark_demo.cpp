// landmark_demo.cpp - the landmark and the bearing sensor model through the header-only facade: beluga::Amcl over a LandmarkMap with
// LandmarkModelParam / BearingModelParam, update() with a vector of detections.
// Prints one line per update ("x y theta"), first the landmark filter's four, then the bearing filter's four, so that a test can
// compare them with the Python facade on the same inputs.  Exit code 3: no usable GPU (the library has no CPU fallback).
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "beluga_amd/amcl.hpp"

namespace {

template <class Sensor, class Detection>
int run(const beluga_amd::LandmarkMap& map, const Sensor& sensor, const std::vector<Detection>& detections) {
  beluga_amd::AmclParams params;
  params.min_particles = 2000;
  params.max_particles = 2000;
  beluga_amd::Amcl amcl{map, beluga_amd::DifferentialDriveModelParam{0.1, 0.05, 0.1, 0.05}, sensor, params, 7};
  amcl.initialize(beluga_amd::SE2d{0.0, 0.0, 0.0}, beluga_amd::Matrix3d{0.04, 0, 0, 0, 0.04, 0, 0, 0, 0.01});
  for (int c = 0; c < 4; ++c) {
    amcl.force_update();
    const auto est = amcl.update(beluga_amd::SE2d{0.0, 0.0, 0.0}, detections);
    if (!est) return 2;
    std::printf("%.17g %.17g %.17g\n", est->first.x, est->first.y, est->first.angle());
  }
  return 0;
}

}  // namespace

int main() {
  // 12 landmarks on a circle of 5 m at heights 0.5 / 1.0 / 1.5, categories 0 .. 3; the robot stands at the origin and sees every other one
  std::vector<beluga_amd::LandmarkPositionDetection> landmarks;
  for (int k = 0; k < 12; ++k)
    landmarks.push_back({{5.0 * std::cos(k * M_PI / 6), 5.0 * std::sin(k * M_PI / 6), 0.5 * (1 + k % 3)}, static_cast<std::uint32_t>(k % 4)});
  const beluga_amd::LandmarkMap map{beluga_amd::LandmarkMapBoundaries{{-6.0, -6.0, 0.0}, {6.0, 6.0, 2.0}}, landmarks};
  const beluga_amd::LandmarkMap implicit{landmarks};
  if (implicit.map_limits().min()[0] != -5.0 || implicit.map_limits().max()[2] != 1.5 || map.map_limits().max()[0] != 6.0) return 1;
  std::vector<beluga_amd::LandmarkPositionDetection> positions;
  std::vector<beluga_amd::LandmarkBearingDetection> bearings;
  const double height = 0.5;  // of the bearing sensor above the robot's origin
  for (std::size_t k = 0; k < landmarks.size(); k += 2) {
    const auto& p = landmarks[k].detection_position_in_robot;
    positions.push_back({p, landmarks[k].category});
    bearings.push_back({{p[0], p[1], p[2] - height}, landmarks[k].category});
  }
  try {
    beluga_amd::LandmarkModelParam landmark_sensor;
    landmark_sensor.sigma_range = 0.2;
    landmark_sensor.sigma_bearing = 0.1;
    landmark_sensor.random_prob = 1e-3;
    if (const int rc = run(map, landmark_sensor, positions)) return rc;
    beluga_amd::BearingModelParam bearing_sensor;
    bearing_sensor.sigma_bearing = 0.1;
    bearing_sensor.sensor_pose_in_robot = {0.0, 0.0, 0.0, 1.0, 0.0, 0.0, height};
    if (const int rc = run(map, bearing_sensor, bearings)) return rc;
  } catch (const std::runtime_error& e) {
    std::printf("runtime_error: %s\n", e.what());
    return 3;
  }
  return 0;
}
