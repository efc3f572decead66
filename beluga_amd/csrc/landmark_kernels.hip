// landmark_kernels.hip — the landmark and bearing sensor models' reweight on gfx950: beluga::LandmarkSensorModel2d and
// beluga::BearingSensorModel2d over a LandmarkMap (sensor/landmark_sensor_model.hpp:92-157, sensor/bearing_sensor_model.hpp:89-141,
// sensor/data/landmark_map.hpp:81-161).
//
// A lane per particle, f64 throughout.  The detections (kernels.h: kLandmarkRecord doubles each) and the landmarks (4 doubles each,
// grouped by category) are the same for every lane and are read at wave-uniform addresses (scalar loads); a few KB, they stay in the
// scalar cache.  The reference searches the whole map per detection and filters by category on the way; here a detection carries the
// range of its category's landmarks, resolved on the host, and the scan covers that range only - in map order, replacing the match on a
// strictly better candidate, so the landmark selected is the one std::min_element selects, the first of equal ones included.
//
// A particle (c, s, x, y) stands for the pose Rz(theta), (x, y, 0); the rotation is applied from (c, s) (the reference goes through
// SO3::rotZ(so2.log()) and a quaternion product: the last bits differ).  Sums of three terms associate as v0 + (v1 + v2): that is how
// Eigen 3.4's unrolled reduction of a 3-vector reads in its header (Redux.h, the unroller splits the range in halves) - taken from
// reading the header, not from a run of the reference.  It moves last bits only.
#include <hip/hip_runtime.h>

#include "device_common.hpp"

namespace mcl {
namespace {

struct Vec3 {
  double x, y, z;
};

__device__ __forceinline__ double squared_norm(const Vec3& v) { return v.x * v.x + (v.y * v.y + v.z * v.z); }
__device__ __forceinline__ double dot(const Vec3& a, const Vec3& b) { return a.x * b.x + (a.y * b.y + a.z * b.z); }
// Eigen's normalized(): v / sqrt(squaredNorm), v itself where that is zero
__device__ __forceinline__ Vec3 normalized(const Vec3& v) {
  const double n2 = squared_norm(v);
  if (!(n2 > 0.0)) return v;
  const double n = sqrt(n2);
  return Vec3{v.x / n, v.y / n, v.z / n};
}
// atan2(|a x b|, a . b)
__device__ __forceinline__ double aperture(const Vec3& a, const Vec3& b) {
  const Vec3 cross{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
  return atan2(sqrt(squared_norm(cross)), dot(a, b));
}

struct Detection {
  Vec3 d;        // as given
  double range;  // |d|
  Vec3 unit;     // normalized(d)
  uint32_t first, count, place;
};
__device__ __forceinline__ Detection load_detection(const double* __restrict__ r) {
  const uint32_t* u = reinterpret_cast<const uint32_t*>(r + 7);
  return Detection{Vec3{r[0], r[1], r[2]}, r[3], Vec3{r[4], r[5], r[6]}, u[0], u[1], u[2]};
}
// What the bearing search reads of a detection: the vector as given and the detection's place in the caller's order.
__device__ __forceinline__ Vec3 load_detection_vector(const double* __restrict__ r) { return Vec3{r[0], r[1], r[2]}; }
__device__ __forceinline__ uint32_t load_detection_first(const double* __restrict__ r) { return reinterpret_cast<const uint32_t*>(r + 7)[0]; }
__device__ __forceinline__ uint32_t load_detection_place(const double* __restrict__ r) { return reinterpret_cast<const uint32_t*>(r + 7)[2]; }
__device__ __forceinline__ Vec3 load_landmark(const double* __restrict__ landmarks, uint32_t at) {
  const double2* l = reinterpret_cast<const double2*>(landmarks + static_cast<size_t>(at) * 4);
  const double2 xy = l[0], z = l[1];
  return Vec3{xy.x, xy.y, z.x};
}

// detection_weight of landmark_sensor_model.hpp:109-153 for the pose s
__device__ __forceinline__ double landmark_term(const LandmarkMapView& m, const double* __restrict__ r, const Pose2& s) {
  const Detection q = load_detection(r);
  if (q.count == 0) return m.random_prob;  // :126-128
  const double rc = s.r.c, rs = s.r.s;
  // robot_pose_in_world * detection (:119)
  const Vec3 p{(rc * q.d.x - rs * q.d.y) + s.x, (rs * q.d.x + rc * q.d.y) + s.y, q.d.z};
  // find_nearest_landmark (landmark_map.hpp:81-110)
  Vec3 match = load_landmark(m.landmarks, q.first);
  double best = squared_norm(Vec3{match.x - p.x, match.y - p.y, match.z - p.z});
  for (uint32_t t = 1; t < q.count; ++t) {
    const Vec3 l = load_landmark(m.landmarks, q.first + t);
    const double d2 = squared_norm(Vec3{l.x - p.x, l.y - p.y, l.z - p.z});
    if (d2 < best) {
      best = d2;
      match = l;
    }
  }
  // the landmark in the robot frame, R^T (l - t) (:133)
  const double vx = match.x - s.x, vy = match.y - s.y;
  const Vec3 in_robot{rc * vx + rs * vy, rc * vy - rs * vx, match.z};
  const double landmark_range = sqrt(squared_norm(in_robot));
  const double bearing_error = aperture(normalized(in_robot), q.unit);  // :139-141
  const double range_error = q.range - landmark_range;
  return exp(-range_error * range_error / m.den_range) * exp(-bearing_error * bearing_error / m.den_bearing) + m.random_prob;
}

__global__ __launch_bounds__(kBlock) void k_reweight_landmarks(Particles p, uint64_t n, LandmarkMapView m, const double* __restrict__ det,
                                                               uint32_t k) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n) return;
  const Pose2 s = load_pose(p, i);
  // std::transform_reduce(detections, 1.0, multiplies, ...) (:155) as libstdc++ multiplies it: blocks of four, the rest one by one
  double acc = 1.0;
  uint32_t j = 0;
  for (; j + 4 <= k; j += 4) {
    const double t0 = landmark_term(m, det + (j + 0) * kLandmarkRecord, s);
    const double t1 = landmark_term(m, det + (j + 1) * kLandmarkRecord, s);
    const double t2 = landmark_term(m, det + (j + 2) * kLandmarkRecord, s);
    const double t3 = landmark_term(m, det + (j + 3) * kLandmarkRecord, s);
    acc = acc * ((t0 * t1) * (t2 * t3));
  }
  for (; j < k; ++j) acc = acc * landmark_term(m, det + j * kLandmarkRecord, s);
  p.w[i] *= acc;  // actions::reweight (actions/reweight.hpp:53-60)
}

// The bearing model.  sensor_pose_in_world = robot * sensor_pose_in_robot (bearing_sensor_model.hpp:107): rotation Rz Rs, translation
// Rz ts + t; a landmark's bearing in the sensor frame is normalized(Rw^T (l - tw)) (landmark_map.hpp:128,140).
struct SensorFrame {
  double r[9];  // Rw, row-major
  Vec3 t;
};
__device__ __forceinline__ Vec3 bearing_of(const SensorFrame& f, const Vec3& l) {
  const Vec3 v{l.x - f.t.x, l.y - f.t.y, l.z - f.t.z};
  return normalized(Vec3{f.r[0] * v.x + (f.r[3] * v.y + f.r[6] * v.z), f.r[1] * v.x + (f.r[4] * v.y + f.r[7] * v.z),
                         f.r[2] * v.x + (f.r[5] * v.y + f.r[8] * v.z)});
}

// One wave per workgroup, a lane per particle.  The detections arrive sorted by category; for each run of one category the landmarks of
// that category are visited ONCE: the landmark's bearing is normalised once and every detection of the run is compared against it (the
// reference normalises it again for every detection).  The state of a detection's search - the best dot product so far and the place
// of its landmark in the category - lives in LDS, k slots per lane, [slot][lane] (each lane touches its own column only: no barrier,
// no bank conflict); the slot is the detection's place in the caller's order, and once the run is searched it holds the detection's
// term, so that the product at the end follows the caller's order in blocks of four.
__global__ __launch_bounds__(kWave) void k_reweight_bearings(Particles p, uint64_t n, LandmarkMapView m, const double* __restrict__ det,
                                                             uint32_t k) {
  extern __shared__ double s_value[];                                      // [k][kWave]
  uint32_t* s_pick = reinterpret_cast<uint32_t*>(s_value + k * kWave);     // [k][kWave]
  const uint32_t lane = threadIdx.x;
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kWave + lane;
  if (i >= n) return;
  const Pose2 s = load_pose(p, i);
  const double rc = s.r.c, rs = s.r.s;
  SensorFrame f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    f.r[c] = rc * m.Rs[c] - rs * m.Rs[3 + c];
    f.r[3 + c] = rs * m.Rs[c] + rc * m.Rs[3 + c];
    f.r[6 + c] = m.Rs[6 + c];
  }
  f.t = Vec3{(rc * m.ts[0] - rs * m.ts[1]) + s.x, (rs * m.ts[0] + rc * m.ts[1]) + s.y, m.ts[2]};
  for (uint32_t j = 0; j < k;) {
    const Detection head = load_detection(det + j * kLandmarkRecord);
    if (head.count == 0) {  // no landmark of that category: 0.0 (bearing_sensor_model.hpp:115-117)
      s_value[head.place * kWave + lane] = 0.0;
      ++j;
      continue;
    }
    uint32_t end = j + 1;
    while (end < k && load_detection_first(det + end * kLandmarkRecord) == head.first) ++end;
    // find_closest_bearing_landmark (landmark_map.hpp:117-161): the largest dot product with the detection as given, the first of equal
    for (uint32_t t = 0; t < head.count; ++t) {
      const Vec3 b = bearing_of(f, load_landmark(m.landmarks, head.first + t));
      for (uint32_t q = j; q < end; ++q) {
        const double v = dot(b, load_detection_vector(det + q * kLandmarkRecord));
        const uint32_t at = load_detection_place(det + q * kLandmarkRecord) * kWave + lane;
        if (t == 0 || v > s_value[at]) {
          s_value[at] = v;
          s_pick[at] = t;
        }
      }
    }
    for (uint32_t q = j; q < end; ++q) {
      const Detection d = load_detection(det + q * kLandmarkRecord);
      const uint32_t at = d.place * kWave + lane;
      const Vec3 b = bearing_of(f, load_landmark(m.landmarks, head.first + s_pick[at]));  // (the same bits as in the search)
      const double e = aperture(d.unit, b);  // :120-130
      s_value[at] = exp(-e * e / m.den_bearing);
    }
    j = end;
  }
  double acc = 1.0;  // std::transform_reduce(detections, 1.0, multiplies, ...) (:139), libstdc++'s order
  uint32_t j = 0;
  for (; j + 4 <= k; j += 4) {
    const double t0 = s_value[(j + 0) * kWave + lane], t1 = s_value[(j + 1) * kWave + lane];
    const double t2 = s_value[(j + 2) * kWave + lane], t3 = s_value[(j + 3) * kWave + lane];
    acc = acc * ((t0 * t1) * (t2 * t3));
  }
  for (; j < k; ++j) acc = acc * s_value[j * kWave + lane];
  p.w[i] *= acc;
}

}  // namespace

void launch_reweight_landmarks(hipStream_t st, Particles p, uint64_t n, const LandmarkMapView& m, const double* detections, uint32_t k) {
  if (n == 0 || k == 0) return;  // (no detection: the product is 1.0)
  hipLaunchKernelGGL(k_reweight_landmarks, dim3(blocks_for(n)), dim3(kBlock), 0, st, p, n, m, detections, k);
}

void launch_reweight_bearings(hipStream_t st, Particles p, uint64_t n, const LandmarkMapView& m, const double* detections, uint32_t k) {
  if (n == 0 || k == 0) return;
  const size_t lds = static_cast<size_t>(k) * kWave * (sizeof(double) + sizeof(uint32_t));  // <= 48 KB at kLandmarkMaxDetections
  hipLaunchKernelGGL(k_reweight_bearings, dim3(static_cast<unsigned>((n + kWave - 1) / kWave)), dim3(kWave), lds, st, p, n, m, detections, k);
}

}  // namespace mcl
