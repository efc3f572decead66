// likelihoods_demo.cpp - the sensor model as a function through the header-only facade: Amcl::likelihoods(states, detections) on a
// landmark and on a bearing filter, for a lattice of candidate states around the origin, then initialize(pose, cov) at the best one.
// Prints one line per candidate ("cos sin x y score", first the landmark filter's, then the bearing filter's) so that a test can score
// the same states through the Python facade, and "best x y theta" after each lattice.  Exit code 3: no usable GPU (the library has
// no CPU fallback).
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "beluga_amd/amcl.hpp"

namespace {

template <class Sensor, class Detection>
int run(const beluga_amd::LandmarkMap& map, const Sensor& sensor, const std::vector<Detection>& detections) {
  beluga_amd::AmclParams params;
  params.min_particles = 500;
  params.max_particles = 500;
  beluga_amd::Amcl amcl{map, beluga_amd::DifferentialDriveModelParam{0.1, 0.05, 0.1, 0.05}, sensor, params, 7};
  amcl.initialize(beluga_amd::SE2d{1.0, -1.0, 0.5}, beluga_amd::Matrix3d{0.04, 0, 0, 0, 0.04, 0, 0, 0, 0.01});
  std::vector<beluga_amd::SE2d> states;
  for (int ix = -2; ix <= 2; ++ix)
    for (int iy = -2; iy <= 2; ++iy)
      for (int it = -1; it <= 1; ++it) states.push_back(beluga_amd::SE2d{0.25 * ix, 0.25 * iy, 0.2 * it});
  const std::vector<double> scores = amcl.likelihoods(states, detections);
  if (scores.size() != states.size()) return 2;
  std::size_t best = 0;
  for (std::size_t i = 0; i < states.size(); ++i) {
    const double* d = states[i].data();
    std::printf("%.17g %.17g %.17g %.17g %.17g\n", d[0], d[1], d[2], d[3], scores[i]);
    if (scores[i] > scores[best]) best = i;
  }
  std::printf("best %.17g %.17g %.17g\n", states[best].x, states[best].y, states[best].angle());
  amcl.initialize(states[best], beluga_amd::Matrix3d{0.01, 0, 0, 0, 0.01, 0, 0, 0, 0.0025});  // relocalise at the best candidate
  return amcl.likelihoods({}, detections).empty() ? 0 : 2;
}

}  // namespace

int main() {
  // 12 landmarks on a circle of 5 m at heights 0.5 / 1.0 / 1.5, categories 0 .. 3; the robot stands at the origin and sees every other one
  std::vector<beluga_amd::LandmarkPositionDetection> landmarks;
  for (int k = 0; k < 12; ++k)
    landmarks.push_back({{5.0 * std::cos(k * M_PI / 6), 5.0 * std::sin(k * M_PI / 6), 0.5 * (1 + k % 3)}, static_cast<std::uint32_t>(k % 4)});
  const beluga_amd::LandmarkMap map{beluga_amd::LandmarkMapBoundaries{{-6.0, -6.0, 0.0}, {6.0, 6.0, 2.0}}, landmarks};
  std::vector<beluga_amd::LandmarkPositionDetection> positions;
  std::vector<beluga_amd::LandmarkBearingDetection> bearings;
  const double height = 0.5;  // of the bearing sensor above the robot's origin
  for (std::size_t k = 0; k < landmarks.size(); k += 2) {
    const auto& p = landmarks[k].detection_position_in_robot;
    positions.push_back({p, landmarks[k].category});
    bearings.push_back({{p[0], p[1], p[2] - height}, landmarks[k].category});
  }
  for (const auto& l : landmarks) {
    const auto& p = l.detection_position_in_robot;
    std::printf("landmark %.17g %.17g %.17g %u\n", p[0], p[1], p[2], l.category);
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
