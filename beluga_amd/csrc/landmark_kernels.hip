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

#include "batch_host.h"
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

// The pieces of detection_weight (landmark_sensor_model.hpp:109-153) that the lane-per-particle and the wave-per-particle kernel share:
// the same expressions in both, so the same bits (-ffp-contract=off).
// robot_pose_in_world * detection (:119)
__device__ __forceinline__ Vec3 detection_in_world(const Pose2& s, const Vec3& d) {
  const double rc = s.r.c, rs = s.r.s;
  return Vec3{(rc * d.x - rs * d.y) + s.x, (rs * d.x + rc * d.y) + s.y, d.z};
}
// what find_nearest_landmark minimises (landmark_map.hpp:81-110)
__device__ __forceinline__ double squared_distance(const Vec3& l, const Vec3& p) { return squared_norm(Vec3{l.x - p.x, l.y - p.y, l.z - p.z}); }
// the term of a detection against the landmark `match` that the search picked (:133-153)
__device__ __forceinline__ double landmark_match_term(const LandmarkMapView& m, const Detection& q, const Pose2& s, const Vec3& match) {
  const double rc = s.r.c, rs = s.r.s;
  // the landmark in the robot frame, R^T (l - t) (:133)
  const double vx = match.x - s.x, vy = match.y - s.y;
  const Vec3 in_robot{rc * vx + rs * vy, rc * vy - rs * vx, match.z};
  const double landmark_range = sqrt(squared_norm(in_robot));
  const double bearing_error = aperture(normalized(in_robot), q.unit);  // :139-141
  const double range_error = q.range - landmark_range;
  return exp(-range_error * range_error / m.den_range) * exp(-bearing_error * bearing_error / m.den_bearing) + m.random_prob;
}

// detection_weight of landmark_sensor_model.hpp:109-153 for the pose s
__device__ __forceinline__ double landmark_term(const LandmarkMapView& m, const double* __restrict__ r, const Pose2& s) {
  const Detection q = load_detection(r);
  if (q.count == 0) return m.random_prob;  // :126-128
  const Vec3 p = detection_in_world(s, q.d);
  // find_nearest_landmark (landmark_map.hpp:81-110)
  Vec3 match = load_landmark(m.landmarks, q.first);
  double best = squared_distance(match, p);
  for (uint32_t t = 1; t < q.count; ++t) {
    const Vec3 l = load_landmark(m.landmarks, q.first + t);
    const double d2 = squared_distance(l, p);
    if (d2 < best) {
      best = d2;
      match = l;
    }
  }
  return landmark_match_term(m, q, s, match);
}

// the product over the k detections for the pose s, as a lane multiplies it: what a particle's weight is multiplied by
__device__ __forceinline__ double landmark_lane_product(const LandmarkMapView& m, const double* __restrict__ det, uint32_t k, const Pose2& s) {
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
  return acc;
}
__global__ __launch_bounds__(kBlock) void k_reweight_landmarks(Particles p, uint64_t n, LandmarkMapView m, const double* __restrict__ det,
                                                               uint32_t k) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n) return;
  p.w[i] *= landmark_lane_product(m, det, k, load_pose(p, i));  // actions::reweight (actions/reweight.hpp:53-60)
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

// sensor_pose_in_world for the pose s (:107)
__device__ __forceinline__ SensorFrame sensor_frame(const LandmarkMapView& m, const Pose2& s) {
  const double rc = s.r.c, rs = s.r.s;
  SensorFrame f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    f.r[c] = rc * m.Rs[c] - rs * m.Rs[3 + c];
    f.r[3 + c] = rs * m.Rs[c] + rc * m.Rs[3 + c];
    f.r[6 + c] = m.Rs[6 + c];
  }
  f.t = Vec3{(rc * m.ts[0] - rs * m.ts[1]) + s.x, (rs * m.ts[0] + rc * m.ts[1]) + s.y, m.ts[2]};
  return f;
}
// the term of a detection (its normalized() vector `unit`) against the bearing `b` of the landmark that the search picked (:120-130)
__device__ __forceinline__ double bearing_match_term(const LandmarkMapView& m, const Vec3& unit, const Vec3& b) {
  const double e = aperture(unit, b);
  return exp(-e * e / m.den_bearing);
}

// One wave per workgroup, a lane per particle.  The detections arrive sorted by category; for each run of one category the landmarks of
// that category are visited ONCE: the landmark's bearing is normalised once and every detection of the run is compared against it (the
// reference normalises it again for every detection).  The state of a detection's search - the best dot product so far and the place
// of its landmark in the category - lives in LDS, k slots per lane, [slot][lane] (each lane touches its own column only: no barrier,
// no bank conflict); the slot is the detection's place in the caller's order, and once the run is searched it holds the detection's
// term, so that the product at the end follows the caller's order in blocks of four.
// (the product itself for the pose s, by the lane `lane` of a one-wave workgroup: s_value and s_pick are its [k][kWave] columns)
__device__ __forceinline__ double bearings_lane_product(const LandmarkMapView& m, const double* __restrict__ det, uint32_t k, const Pose2& s,
                                                        uint32_t lane, double* s_value, uint32_t* s_pick) {
  const SensorFrame f = sensor_frame(m, s);
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
      s_value[at] = bearing_match_term(m, d.unit, b);
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
  return acc;
}
__global__ __launch_bounds__(kWave) void k_reweight_bearings(Particles p, uint64_t n, LandmarkMapView m, const double* __restrict__ det,
                                                             uint32_t k) {
  extern __shared__ double s_value[];                                      // [k][kWave]
  uint32_t* s_pick = reinterpret_cast<uint32_t*>(s_value + k * kWave);     // [k][kWave]
  const uint32_t lane = threadIdx.x;
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kWave + lane;
  if (i >= n) return;
  p.w[i] *= bearings_lane_product(m, det, k, load_pose(p, i), lane, s_value, s_pick);
}

// ---- a wave per particle (small sets: mcl_set_landmark_small_cycle) -------------------------------------------------------------------
// At 2000 particles a lane per particle is 32 waves on 256 CUs, each lane walking k detections x L landmarks in a row.  Here a wave
// takes one particle (kBlock threads, four particles per workgroup, as k_reweight_ndt_wave) and its lanes take the detections: with P
// the smallest power of two >= k and g = 64 / P, record j owns the aligned lanes [j g, (j + 1) g), and lane r of that group scans the
// landmarks first + r, first + r + g, ... of the record's category in ascending order, replacing its candidate on a strictly better
// value - the lane kernel's rule.  The group then reduces in log2 g xor steps, which stay inside the aligned group: the better value
// wins, an equal value goes to the smaller landmark index, a lane that scanned nothing (r >= count) carries the index 0xFFFFFFFF
// and the worst value, so it loses to every lane that scanned.  (value, index) in this order is a total order on finite inputs, so
// the result is its minimum over the category whatever the shape of the reduction: the landmark the sequential scan picks, the first of
// equal ones.  The group's first lane forms the term from the pick with the lane kernel's own functions; the product is then chained
// through v_readlane in the lane kernel's order and association, every lane carrying the same running product.
struct GroupShape {
  uint32_t shift;  // log2 g
  uint32_t g;      // lanes of a record's group
};
__device__ __forceinline__ GroupShape group_shape(uint32_t k) {  // 1 <= k <= kWave
  uint32_t shift = 6;
  while ((static_cast<uint32_t>(kWave) >> shift) < k) --shift;  // the largest g = 2^shift with 64 / g >= k
  return GroupShape{shift, 1u << shift};
}
constexpr uint32_t kNoPick = 0xFFFFFFFFu;
// kLarger = false: the smaller value is the better one (squared distances); true: the larger one (dot products)
template <bool kLarger>
__device__ __forceinline__ bool pick_beats(double v, uint32_t at, double other_v, uint32_t other_at) {
  if (other_at == kNoPick) return true;   // (the other lane scanned nothing; two such lanes are alike)
  if (at == kNoPick) return false;
  if (v == other_v) return at < other_at;
  return kLarger ? v > other_v : v < other_v;
}
template <bool kLarger>
__device__ __forceinline__ void group_reduce(uint32_t g, double* v, uint32_t* at) {  // every lane of the wave takes part
  for (uint32_t step = g >> 1; step >= 1; step >>= 1) {
    const double other_v = __shfl_xor(*v, static_cast<int>(step));
    const uint32_t other_at = __shfl_xor(*at, static_cast<int>(step));
    if (!pick_beats<kLarger>(*v, *at, other_v, other_at)) {
      *v = other_v;
      *at = other_at;
    }
  }
}
// terms 0 .. k-1 are held by the lanes 0, stride, 2 stride, ...: the product as libstdc++ multiplies it, blocks of four, the rest one by one
__device__ __forceinline__ double chained_product(double term, uint32_t k, uint32_t shift) {
  double acc = 1.0;
  uint32_t j = 0;
  for (; j + 4 <= k; j += 4) {
    const double t0 = readlane_f64(term, static_cast<int>((j + 0) << shift)), t1 = readlane_f64(term, static_cast<int>((j + 1) << shift));
    const double t2 = readlane_f64(term, static_cast<int>((j + 2) << shift)), t3 = readlane_f64(term, static_cast<int>((j + 3) << shift));
    acc = acc * ((t0 * t1) * (t2 * t3));
  }
  for (; j < k; ++j) acc = acc * readlane_f64(term, static_cast<int>(j << shift));
  return acc;
}

// (the products themselves, for the pose s and 1 <= k <= kWave detections: every lane of the wave returns the product)
__device__ __forceinline__ double landmarks_wave_product(uint32_t lane, const Pose2& s, const LandmarkMapView& m, const double* __restrict__ det,
                                                         uint32_t k) {
  const GroupShape shape = group_shape(k);
  const uint32_t j = lane >> shape.shift, r = lane & (shape.g - 1);
  const bool mine = j < k;
  Detection q{};
  double best = 0.0;
  uint32_t at = kNoPick;
  if (mine) {
    q = load_detection(det + j * kLandmarkRecord);
    const Vec3 w = detection_in_world(s, q.d);
    for (uint32_t t = r; t < q.count; t += shape.g) {
      const double d2 = squared_distance(load_landmark(m.landmarks, q.first + t), w);
      if (t == r || d2 < best) {
        best = d2;
        at = t;
      }
    }
  }
  group_reduce<false>(shape.g, &best, &at);
  double term = 1.0;
  if (mine && r == 0) term = q.count == 0 ? m.random_prob : landmark_match_term(m, q, s, load_landmark(m.landmarks, q.first + at));
  return chained_product(term, k, shape.shift);  // record order
}
// The bearing model.  A record's term goes to the slot of its `place` in the wave's row of workgroup memory (the records arrive sorted
// by category, the product follows the caller's order); lane t then takes slot t back and the chain runs over the lanes 0 .. k-1.
__device__ __forceinline__ double bearings_wave_product(uint32_t lane, const Pose2& s, const LandmarkMapView& m, const double* __restrict__ det,
                                                        uint32_t k, double* s_terms /* [kBlock] */) {
  const SensorFrame f = sensor_frame(m, s);
  const GroupShape shape = group_shape(k);
  const uint32_t j = lane >> shape.shift, r = lane & (shape.g - 1);
  const bool mine = j < k;
  Detection q{};
  double best = 0.0;
  uint32_t at = kNoPick;
  if (mine) {
    q = load_detection(det + j * kLandmarkRecord);
    // find_closest_bearing_landmark (landmark_map.hpp:117-161): the largest dot product with the detection as given
    for (uint32_t t = r; t < q.count; t += shape.g) {
      const double v = dot(bearing_of(f, load_landmark(m.landmarks, q.first + t)), q.d);
      if (t == r || v > best) {
        best = v;
        at = t;
      }
    }
  }
  group_reduce<true>(shape.g, &best, &at);
  double* row = s_terms + (threadIdx.x & ~63u);
  if (mine && r == 0)  // no landmark of that category: 0.0 (bearing_sensor_model.hpp:115-117); q.place < k: the places are a permutation
    row[q.place & 63u] = q.count == 0 ? 0.0 : bearing_match_term(m, q.unit, bearing_of(f, load_landmark(m.landmarks, q.first + at)));
  // (one wave wrote, the same wave reads: its LDS operations complete in order)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const double term = lane < k ? row[lane] : 1.0;
  return chained_product(term, k, 0);  // the caller's order
}

// (the bodies: block `block` of ONE set - blockIdx.x in the lone kernels, a member's local block in k_batch_reweight_landmarks)
__device__ __forceinline__ void reweight_landmarks_wave_block(uint32_t block, const Particles& p, uint64_t n, const LandmarkMapView& m,
                                                              const double* __restrict__ det, uint32_t k) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t i = static_cast<uint64_t>(block) * (kBlock / kWave) + (threadIdx.x >> 6);
  if (i >= n || k == 0 || k > static_cast<uint32_t>(kWave)) return;  // (the whole wave)
  const double acc = landmarks_wave_product(lane, load_pose(p, i), m, det, k);
  if (lane == 0) p.w[i] *= acc;  // actions::reweight (actions/reweight.hpp:53-60)
}
__device__ __forceinline__ void reweight_bearings_wave_block(uint32_t block, const Particles& p, uint64_t n, const LandmarkMapView& m,
                                                             const double* __restrict__ det, uint32_t k, double* s_terms /* [kBlock] */) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t i = static_cast<uint64_t>(block) * (kBlock / kWave) + (threadIdx.x >> 6);
  if (i >= n || k == 0 || k > static_cast<uint32_t>(kWave)) return;  // (the whole wave)
  const double acc = bearings_wave_product(lane, load_pose(p, i), m, det, k, s_terms);
  if (lane == 0) p.w[i] *= acc;
}

__global__ __launch_bounds__(kBlock) void k_reweight_landmarks_wave(Particles p, uint64_t n, LandmarkMapView m, const double* __restrict__ det,
                                                                    uint32_t k) {
  reweight_landmarks_wave_block(blockIdx.x, p, n, m, det, k);
}
__global__ __launch_bounds__(kBlock) void k_reweight_bearings_wave(Particles p, uint64_t n, LandmarkMapView m, const double* __restrict__ det,
                                                                   uint32_t k) {
  __shared__ double s_terms[kBlock];
  reweight_bearings_wave_block(blockIdx.x, p, n, m, det, k, s_terms);
}

// The sensor models as functions (mcl_likelihoods_landmarks, mcl_likelihoods_bearings): out[i] = the product for the caller's pose i - the
// factor the reweight kernels above multiply a particle at that pose by, from their own products (the same bits from the lane and the
// wave form).  A plain array of poses (cos, sin, x, y) in, a plain array out; nothing of a filter is read or written.
__device__ __forceinline__ Pose2 pose_at(const double4* __restrict__ poses, uint64_t i) {
  const double4 v = poses[i];
  return Pose2{Rot2{v.x, v.y}, v.z, v.w};
}
__global__ __launch_bounds__(kBlock) void k_likelihoods_landmarks(const double4* __restrict__ poses, uint64_t n, LandmarkMapView m,
                                                                  const double* __restrict__ det, uint32_t k, double* __restrict__ out) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n) return;
  out[i] = landmark_lane_product(m, det, k, pose_at(poses, i));
}
__global__ __launch_bounds__(kWave) void k_likelihoods_bearings(const double4* __restrict__ poses, uint64_t n, LandmarkMapView m,
                                                                const double* __restrict__ det, uint32_t k, double* __restrict__ out) {
  extern __shared__ double s_value[];                                      // [k][kWave]
  uint32_t* s_pick = reinterpret_cast<uint32_t*>(s_value + k * kWave);     // [k][kWave]
  const uint32_t lane = threadIdx.x;
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kWave + lane;
  if (i >= n) return;
  out[i] = bearings_lane_product(m, det, k, pose_at(poses, i), lane, s_value, s_pick);
}
template <bool kBearing>
__global__ __launch_bounds__(kBlock) void k_likelihoods_landmarks_wave(const double4* __restrict__ poses, uint64_t n, LandmarkMapView m,
                                                                       const double* __restrict__ det, uint32_t k, double* __restrict__ out) {
  __shared__ double s_terms[kBearing ? kBlock : 1];
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * (kBlock / kWave) + (threadIdx.x >> 6);
  if (i >= n || k == 0 || k > static_cast<uint32_t>(kWave)) return;  // (the whole wave)
  double acc;
  if constexpr (kBearing) acc = bearings_wave_product(lane, pose_at(poses, i), m, det, k, s_terms);
  else acc = landmarks_wave_product(lane, pose_at(poses, i), m, det, k);
  if (lane == 0) out[i] = acc;
}

// The same over a fleet's landmark and bearing members (mcl_landmark_batch_update; the pattern is k_batch_reweight_ndt): a workgroup finds
// its member over the first_landmark_block prefix - a member without a block (no particle, no detection, another family's member) is
// never found - and runs the body of the member's kind, a workgroup-uniform branch, with its LOCAL block number on the member's own map
// and staged records.
static_assert(kBatchLandmarkThreads == kBlock && kBatchLandmarkBlock == kBlock / kWave, "batch_host.h restates the wave-per-particle landmark kernels' launch geometry");
__global__ __launch_bounds__(kBlock) void k_batch_reweight_landmarks(const BatchItem* __restrict__ items, uint32_t count) {
  __shared__ double s_terms[kBlock];
  const BatchItem& it = items[batch_member_of(count, blockIdx.x, [items](uint32_t m) { return items[m].first_landmark_block; })];
  const uint32_t block = blockIdx.x - it.first_landmark_block;
  if (it.landmark_bearing) reweight_bearings_wave_block(block, it.p, it.n, it.landmark, it.scan_dst, it.landmark_k, s_terms);
  else reweight_landmarks_wave_block(block, it.p, it.n, it.landmark, it.scan_dst, it.landmark_k);
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

void launch_reweight_landmarks_wave(hipStream_t st, Particles p, uint64_t n, const LandmarkMapView& m, const double* detections, uint32_t k) {
  if (n == 0 || k == 0) return;
  hipLaunchKernelGGL(k_reweight_landmarks_wave, dim3(batch_landmark_blocks(n, k)), dim3(kBlock), 0, st, p, n, m, detections, k);
}
void launch_reweight_bearings_wave(hipStream_t st, Particles p, uint64_t n, const LandmarkMapView& m, const double* detections, uint32_t k) {
  if (n == 0 || k == 0) return;
  hipLaunchKernelGGL(k_reweight_bearings_wave, dim3(batch_landmark_blocks(n, k)), dim3(kBlock), 0, st, p, n, m, detections, k);
}

void launch_likelihoods_landmarks(hipStream_t st, const double4* poses, uint64_t n, const LandmarkMapView& m, const double* detections, uint32_t k,
                                  bool bearing, double* out) {
  if (n == 0) return;
  if (k == 0) {  // (no detection: the product is 1.0)
    launch_fill(st, out, n, 1.0);
    return;
  }
  if (n <= kLikelihoodsWaveMax) {
    const dim3 grid(batch_landmark_blocks(n, k));
    if (bearing) hipLaunchKernelGGL(k_likelihoods_landmarks_wave<true>, grid, dim3(kBlock), 0, st, poses, n, m, detections, k, out);
    else hipLaunchKernelGGL(k_likelihoods_landmarks_wave<false>, grid, dim3(kBlock), 0, st, poses, n, m, detections, k, out);
    return;
  }
  if (bearing) {
    const size_t lds = static_cast<size_t>(k) * kWave * (sizeof(double) + sizeof(uint32_t));  // <= 48 KB at kLandmarkMaxDetections
    constexpr uint64_t chunk = kLikelihoodsLaneChunk / (kBlock / kWave);  // (a one-wave workgroup: 2^30 blocks of 64)
    for (uint64_t at = 0; at < n; at += chunk) {
      const uint64_t count = std::min<uint64_t>(chunk, n - at);
      hipLaunchKernelGGL(k_likelihoods_bearings, dim3(static_cast<unsigned>((count + kWave - 1) / kWave)), dim3(kWave), lds, st, poses + at, count, m,
                         detections, k, out + at);
    }
    return;
  }
  for (uint64_t at = 0; at < n; at += kLikelihoodsLaneChunk) {
    const uint64_t count = std::min<uint64_t>(kLikelihoodsLaneChunk, n - at);
    hipLaunchKernelGGL(k_likelihoods_landmarks, dim3(blocks_for(count)), dim3(kBlock), 0, st, poses + at, count, m, detections, k, out + at);
  }
}

void launch_batch_reweight_landmarks(hipStream_t st, const BatchItem* d_items, uint32_t members, uint32_t blocks) {
  if (blocks == 0) return;
  hipLaunchKernelGGL(k_batch_reweight_landmarks, dim3(blocks), dim3(kBlock), 0, st, d_items, members);
}

}  // namespace mcl
