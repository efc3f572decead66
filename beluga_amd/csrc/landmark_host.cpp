// landmark_host.cpp — see landmark_host.h.  Also the two models' default parameters (C ABI, no context).
#include "landmark_host.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace mcl {

#define LANDMARK_REQUIRE(cond, msg) \
  do { if (!(cond)) { if (error) *error = (msg); return MCL_ERR_INVALID_ARGUMENT; } } while (0)

mcl_status landmark_layout_map(int32_t kind, const double* positions_xyz, const uint32_t* categories, uint64_t n, const double boundaries[6],
                               const void* params, LandmarkMapLayout* out, std::string* error) {
  LANDMARK_REQUIRE(n == 0 || (positions_xyz && categories), "mcl_set_landmark_map: null argument");
  LANDMARK_REQUIRE(n < (1ull << 31), "mcl_set_landmark_map: too many landmarks");
  LANDMARK_REQUIRE(n > 0 || boundaries, "mcl_set_landmark_map: an empty map needs explicit boundaries");
  for (uint64_t i = 0; i < 3 * n; ++i)
    LANDMARK_REQUIRE(std::isfinite(positions_xyz[i]), "mcl_set_landmark_map: landmark " + std::to_string(i / 3) + " has a value that is not finite");
  LandmarkMapLayout& v = *out;
  if (kind == MCL_SENSOR_LANDMARK) {
    mcl_landmark_params prm;
    if (params) prm = *static_cast<const mcl_landmark_params*>(params);
    else mcl_default_landmark_params(&prm);
    LANDMARK_REQUIRE(std::isfinite(prm.sigma_range) && prm.sigma_range > 0.0 && std::isfinite(prm.sigma_bearing) && prm.sigma_bearing > 0.0,
                     "mcl_set_landmark_map: sigma_range and sigma_bearing must be positive and finite");
    LANDMARK_REQUIRE(std::isfinite(prm.random_prob), "mcl_set_landmark_map: random_prob must be finite");
    v.den_range = (2. * prm.sigma_range) * prm.sigma_range;  // landmark_sensor_model.hpp:147
    v.den_bearing = (2. * prm.sigma_bearing) * prm.sigma_bearing;
    // (a sigma whose (2 sigma) sigma leaves the finite positive range would divide an exact zero error by zero, or inf by inf: NaN weights)
    LANDMARK_REQUIRE(v.den_range > 0.0 && std::isfinite(v.den_range) && v.den_bearing > 0.0 && std::isfinite(v.den_bearing),
                     "mcl_set_landmark_map: (2 sigma) sigma must be positive and finite for sigma_range and sigma_bearing");
    v.random_prob = prm.random_prob;
  } else {
    mcl_bearing_params prm;
    if (params) prm = *static_cast<const mcl_bearing_params*>(params);
    else mcl_default_bearing_params(&prm);
    LANDMARK_REQUIRE(std::isfinite(prm.sigma_bearing) && prm.sigma_bearing > 0.0, "mcl_set_landmark_map: sigma_bearing must be positive and finite");
    const double* q = prm.sensor_pose_in_robot;
    for (int k = 0; k < 7; ++k) LANDMARK_REQUIRE(std::isfinite(q[k]), "mcl_set_landmark_map: sensor_pose_in_robot must be finite");
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    LANDMARK_REQUIRE(std::abs(std::sqrt(x * x + y * y + z * z + w * w) - 1.0) <= 1e-9,
                     "mcl_set_landmark_map: sensor_pose_in_robot's quaternion is not of unit length");
    v.den_bearing = (2. * prm.sigma_bearing) * prm.sigma_bearing;  // bearing_sensor_model.hpp:134
    LANDMARK_REQUIRE(v.den_bearing > 0.0 && std::isfinite(v.den_bearing), "mcl_set_landmark_map: (2 sigma) sigma must be positive and finite for sigma_bearing");
    // Eigen's Quaternion::toRotationMatrix
    const double tx = 2. * x, ty = 2. * y, tz = 2. * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    const double R[9] = {1. - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1. - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1. - (txx + tyy)};
    std::copy(R, R + 9, v.Rs);
    std::copy(q + 4, q + 7, v.ts);
  }
  double* lo = v.lo;
  double* hi = v.hi;
  if (boundaries) {
    for (int k = 0; k < 6; ++k) LANDMARK_REQUIRE(std::isfinite(boundaries[k]), "mcl_set_landmark_map: the boundaries must be finite");
    std::copy(boundaries, boundaries + 3, lo);
    std::copy(boundaries + 3, boundaries + 6, hi);
    LANDMARK_REQUIRE(lo[0] <= hi[0] && lo[1] <= hi[1], "mcl_set_landmark_map: boundaries with min > max");
  } else {
    for (int k = 0; k < 3; ++k) lo[k] = hi[k] = positions_xyz[k];
    for (uint64_t i = 1; i < n; ++i)
      for (int k = 0; k < 3; ++k) {
        lo[k] = std::min(lo[k], positions_xyz[3 * i + k]);
        hi[k] = std::max(hi[k], positions_xyz[3 * i + k]);
      }
  }
  std::vector<uint32_t> order(n);
  for (uint64_t i = 0; i < n; ++i) order[i] = static_cast<uint32_t>(i);
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return categories[a] < categories[b]; });
  v.landmarks.assign(static_cast<size_t>(n) * 4, 0.0);
  v.ranges.clear();
  for (uint64_t i = 0; i < n; ++i) {
    std::copy(positions_xyz + 3 * order[i], positions_xyz + 3 * order[i] + 3, v.landmarks.begin() + static_cast<ptrdiff_t>(4 * i));
    auto it = v.ranges.find(categories[order[i]]);
    if (it == v.ranges.end()) v.ranges[categories[order[i]]] = {static_cast<uint32_t>(i), 1u};
    else it->second.second += 1;
  }
  return MCL_OK;
}

mcl_status landmark_records(const char* who, int32_t kind, const double* xyz, const uint32_t* categories, uint64_t n,
                            const LandmarkRanges* ranges, std::vector<double>& out, std::string* error) {
  LANDMARK_REQUIRE(n == 0 || (xyz && categories), std::string(who) + ": null argument");
  LANDMARK_REQUIRE(n <= MCL_LANDMARK_MAX_DETECTIONS, std::string(who) + ": more than MCL_LANDMARK_MAX_DETECTIONS detections");
  for (uint64_t i = 0; i < 3 * n; ++i) LANDMARK_REQUIRE(std::isfinite(xyz[i]), std::string(who) + ": a detection has a value that is not finite");
  if (!ranges) {
    if (error) *error = std::string(who) + ": no landmark map set (mcl_set_landmark_map)";
    return MCL_ERR_NOT_READY;
  }
  std::vector<uint32_t> order(n);
  for (uint64_t i = 0; i < n; ++i) order[i] = static_cast<uint32_t>(i);
  if (kind == MCL_SENSOR_BEARING) std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return categories[a] < categories[b]; });
  out.assign(static_cast<size_t>(n) * kLandmarkRecord, 0.0);
  for (uint64_t i = 0; i < n; ++i) {
    const double* d = xyz + 3 * order[i];
    double* r = out.data() + i * kLandmarkRecord;
    const double n2 = d[0] * d[0] + (d[1] * d[1] + d[2] * d[2]);
    const double norm = std::sqrt(n2);
    r[0] = d[0], r[1] = d[1], r[2] = d[2], r[3] = norm;
    for (int k = 0; k < 3; ++k) r[4 + k] = n2 > 0.0 ? d[k] / norm : d[k];  // Eigen's normalized()
    const auto it = ranges->find(categories[order[i]]);
    const uint32_t packed[4] = {it == ranges->end() ? 0xFFFFFFFFu : it->second.first, it == ranges->end() ? 0u : it->second.second, order[i], 0u};
    std::memcpy(r + 7, packed, sizeof(packed));
  }
  return MCL_OK;
}

}  // namespace mcl

extern "C" {

void mcl_default_landmark_params(mcl_landmark_params* params) {
  if (!params) return;
  *params = mcl_landmark_params{1.0, 1.0, 1e-4};  // LandmarkModelParam (landmark_sensor_model.hpp:44-48)
}

void mcl_default_bearing_params(mcl_bearing_params* params) {
  if (!params) return;
  *params = mcl_bearing_params{1.0, {0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0}};  // BearingModelParam (bearing_sensor_model.hpp:42-45)
}

}  // extern "C"
