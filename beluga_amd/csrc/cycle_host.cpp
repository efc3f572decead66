// cycle_host.cpp — the update cycle's host decisions (cycle_host.h).  Plain C++17, no HIP.
#include "cycle_host.h"

#include <algorithm>
#include <cmath>
#include <limits>

namespace mcl {

namespace {

// motion/differential_drive_model.hpp:129-154,167-173
double rotation_variance(const Rot2& r) {
  const Rot2 flipped = rot_mul(r, rot_exp(kPi));
  const double delta = std::min(std::abs(rot_log(r)), std::abs(rot_log(flipped)));
  return delta * delta;
}

bool off_grid(int sensor_kind) {
  return sensor_kind == MCL_SENSOR_NDT || sensor_kind == MCL_SENSOR_LANDMARK || sensor_kind == MCL_SENSOR_BEARING;
}

}  // namespace

SensorFamily sensor_family(int sensor_kind) {
  switch (sensor_kind) {
    case MCL_SENSOR_BEAM: return SensorFamily::kBeam;
    case MCL_SENSOR_NDT: return SensorFamily::kNdt;
    case MCL_SENSOR_LANDMARK:
    case MCL_SENSOR_BEARING: return SensorFamily::kLandmark;
    default: return SensorFamily::kLikelihoodField;  // MCL_SENSOR_LIKELIHOOD_FIELD, MCL_SENSOR_LIKELIHOOD_FIELD_PROB
  }
}

// ---- motion --------------------------------------------------------------------------------------------------------------------------

DiffDriveSampler make_sampler(const Pose2& pose, const Pose2& prev, const mcl_diffdrive_params& a, int kind, double alpha5) {
  const double tx = pose.x - prev.x, ty = pose.y - prev.y;
  const double distance = std::sqrt(tx * tx + ty * ty);
  const double distance_variance = distance * distance;
  const Rot2 heading = rot_exp(std::atan2(ty, tx));
  const Rot2 first = distance > a.distance_threshold ? rot_mul(heading, rot_inverse(prev.r)) : Rot2{1.0, 0.0};
  DiffDriveSampler s{};
  s.kind = kind;
  s.first_c = first.c;
  s.first_s = first.s;
  if (kind == MCL_MOTION_STATIONARY) return s;  // stationary_model.hpp:53-61 ignores the control action
  if (kind == MCL_MOTION_OMNIDIRECTIONAL) {     // omnidirectional_drive_model.hpp:102-131
    const Rot2 rotation = rot_mul(pose.r, rot_inverse(prev.r));
    s.m1 = rot_log(rotation);
    s.s1 = std::sqrt(a.rotation_noise_from_rotation * rotation_variance(rotation) + a.rotation_noise_from_translation * distance_variance);
    s.mt = distance;
    s.st = std::sqrt(a.translation_noise_from_translation * distance_variance + a.translation_noise_from_rotation * rotation_variance(rotation));
    s.m2 = 0.0;
    s.s2 = std::sqrt(alpha5 * distance_variance + a.translation_noise_from_rotation * rotation_variance(rotation));
    return s;
  }
  const Rot2 second = rot_mul(rot_mul(pose.r, rot_inverse(prev.r)), rot_inverse(first));
  s.m1 = rot_log(first);
  s.s1 = std::sqrt(a.rotation_noise_from_rotation * rotation_variance(first) + a.rotation_noise_from_translation * distance_variance);
  s.mt = distance;
  s.st = std::sqrt(a.translation_noise_from_translation * distance_variance +
                   a.translation_noise_from_rotation * (rotation_variance(first) + rotation_variance(second)));
  s.m2 = rot_log(second);
  s.s2 = std::sqrt(a.rotation_noise_from_rotation * rotation_variance(second) + a.rotation_noise_from_translation * distance_variance);
  return s;
}

bool samplers_close(const DiffDriveSampler& now, const DiffDriveSampler& predicted) {
  if (now.kind != predicted.kind) return false;
  auto ratio_ok = [](double a, double b) { return a <= 1.5 * b + 1e-3 && b <= 1.5 * a + 1e-3; };
  if (!ratio_ok(now.s1, predicted.s1) || !ratio_ok(now.st, predicted.st) || !ratio_ok(now.s2, predicted.s2)) return false;
  if (std::abs(now.mt - predicted.mt) > 0.3 * std::max(std::abs(predicted.mt), 0.02)) return false;
  const double turn_now = now.kind == MCL_MOTION_DIFFERENTIAL ? now.m1 + now.m2 : now.m1;
  const double turn_predicted = predicted.kind == MCL_MOTION_DIFFERENTIAL ? predicted.m1 + predicted.m2 : predicted.m1;
  if (std::abs(turn_now - turn_predicted) > 0.15) return false;
  // the direction of the translation in the robot's frame (differential: the first rotation; omnidirectional: `first`)
  const double heading_now = now.kind == MCL_MOTION_DIFFERENTIAL ? now.m1 : std::atan2(now.first_s, now.first_c);
  const double heading_predicted = predicted.kind == MCL_MOTION_DIFFERENTIAL ? predicted.m1 : std::atan2(predicted.first_s, predicted.first_c);
  const double apart = std::abs(std::remainder(heading_now - heading_predicted, 2.0 * kPi));
  return apart * std::max(std::abs(now.mt), std::abs(predicted.mt)) <= 0.05;  // (metres of lateral disagreement)
}

bool covariance_to_transform(const double cov[9], double T[9]) {
  double a[3][3], v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) a[i][j] = cov[3 * i + j];
  for (int i = 0; i < 3; ++i)
    for (int j = i + 1; j < 3; ++j) {
      const double scale = std::max(std::abs(a[i][j]), std::abs(a[j][i]));
      if (std::abs(a[i][j] - a[j][i]) > 1e-12 * scale) return false;  // "not symmetric"
      if (!std::isfinite(a[i][j])) return false;
    }
  for (int sweep = 0; sweep < 64; ++sweep) {
    const double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2];
    if (off < 1e-300) break;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        if (a[p][q] == 0.0) continue;
        const double theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (std::abs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 3; ++k) {
          const double akp = a[k][p], akq = a[k][q];
          a[k][p] = c * akp - s * akq;
          a[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 3; ++k) {
          const double apk = a[p][k], aqk = a[q][k];
          a[p][k] = c * apk - s * aqk;
          a[q][k] = s * apk + c * aqk;
        }
        for (int k = 0; k < 3; ++k) {
          const double vkp = v[k][p], vkq = v[k][q];
          v[k][p] = c * vkp - s * vkq;
          v[k][q] = s * vkp + c * vkq;
        }
      }
  }
  for (int j = 0; j < 3; ++j) {
    if (!std::isfinite(a[j][j])) return false;
    if (a[j][j] < 0.0) {
      if (a[j][j] > -1e-14) a[j][j] = 0.0;
      else return false;  // "negative eigenvalues"
    }
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) T[3 * i + j] = v[i][j] * std::sqrt(a[j][j]);
  return true;
}

// ---- where the set is ----------------------------------------------------------------------------------------------------------------

void CloudEstimate::remember(const mcl_estimate& est) {
  const double vx = est.covariance[0], vy = est.covariance[4], vt = est.covariance[8];
  mean_[0] = est.pose[2];
  mean_[1] = est.pose[3];
  mean_[2] = std::atan2(est.pose[1], est.pose[0]);
  sigma_[0] = vx > 0.0 ? std::sqrt(vx) : 0.0;
  sigma_[1] = vy > 0.0 ? std::sqrt(vy) : 0.0;
  sigma_[2] = std::isfinite(vt) ? (vt > 0.0 ? std::sqrt(vt) : 0.0) : kPi;  // infinite circular variance: all headings
  valid_ = std::isfinite(mean_[0]) && std::isfinite(mean_[1]) && std::isfinite(mean_[2]) && std::isfinite(sigma_[0]) && std::isfinite(sigma_[1]);
}

void CloudEstimate::set(const double mean[3], const double sigma[3]) {
  for (int k = 0; k < 3; ++k) {
    mean_[k] = mean[k];
    sigma_[k] = sigma[k];
  }
  valid_ = true;
}

bool predict_key_frame(const CloudEstimate& cloud, const DiffDriveSampler* motion, int moves, uint32_t layout, const KeyFrameInputs& in,
                       KeyFrame* out) {
  out->layout = layout;
  if (!cloud.valid()) return false;
  double x = cloud.mean()[0], y = cloud.mean()[1], t = cloud.mean()[2];
  double sx = cloud.sigma()[0], sy = cloud.sigma()[1], st = cloud.sigma()[2];
  if (motion && motion->kind != MCL_MOTION_STATIONARY) {
    for (int move = 1; move < moves; ++move) {  // (the centre alone)
      const double heading = t + (motion->kind == MCL_MOTION_DIFFERENTIAL ? motion->m1 : std::atan2(motion->first_s, motion->first_c));
      x += motion->mt * std::exp(-0.5 * st * st) * std::cos(heading);
      y += motion->mt * std::exp(-0.5 * st * st) * std::sin(heading);
      t += motion->kind == MCL_MOTION_DIFFERENTIAL ? motion->m1 + motion->m2 : motion->m1;
    }
    const double heading = t + (motion->kind == MCL_MOTION_DIFFERENTIAL ? motion->m1 : std::atan2(motion->first_s, motion->first_c));
    // every pose moves along ITS heading: the set's mean moves by the translation times the mean resultant length of the headings
    // (next to nothing for a set that points everywhere), and a heading error turns into a lateral one over the translation -
    // mt * sigma_theta for a narrow set, at most mt / sqrt(2) per axis for headings all around
    const double resultant = std::exp(-0.5 * st * st);
    x += motion->mt * resultant * std::cos(heading);
    y += motion->mt * resultant * std::sin(heading);
    t += motion->kind == MCL_MOTION_DIFFERENTIAL ? motion->m1 + motion->m2 : motion->m1;
    const double lateral = motion->mt * std::min(st, std::sqrt(0.5));
    const double noise2 = motion->st * motion->st + lateral * lateral + (motion->kind == MCL_MOTION_OMNIDIRECTIONAL ? motion->s2 * motion->s2 : 0.0);
    sx = std::sqrt(sx * sx + noise2);
    sy = std::sqrt(sy * sy + noise2);
    st = std::sqrt(st * st + motion->s1 * motion->s1 + (motion->kind == MCL_MOTION_DIFFERENTIAL ? motion->s2 * motion->s2 : 0.0));
  } else if (motion) {
    sx = std::sqrt(sx * sx + 0.02 * 0.02);
    sy = std::sqrt(sy * sy + 0.02 * 0.02);
    st = std::sqrt(st * st + 0.02 * 0.02);
  }
  if (!(std::isfinite(x) && std::isfinite(y) && std::isfinite(t) && std::isfinite(sx) && std::isfinite(sy) && std::isfinite(st))) return false;
  // +- 4 sigma; a set reported as dispersed is closer to uniform than to normal: +- 2 sigma hold all of a uniform one
  const double spans = in.patch_useful ? 8.0 : 4.0;
  auto inverse_span = [spans](double sigma) { return sigma > 0.0 ? static_cast<float>(1.0 / (spans * sigma)) : 0.f; };
  auto sigma_span_t = [](double sigma) { return sigma > 0.0 ? static_cast<float>(1.0 / (8.0 * sigma)) : 0.f; };
  out->cx = x;
  out->cy = y;
  out->c0 = std::cos(t);
  out->s0 = std::sin(t);
  out->inv_x = inverse_span(sx);
  out->inv_y = inverse_span(sy);
  out->inv_t = sigma_span_t(std::min(st, kPi / 4.0));  // the heading bins never span more than the circle
  out->t_off = 0.f;
  if (in.key_warp && !(out->layout & 1u) && spans == 8.0) out->layout |= 4u;  // bins of equal mass over the +-4 sigma
  // How the 20 bits are split: a run of the curve is roughly a cube of bins, and what a workgroup's LDS patch has to absorb is
  // its extent in x (or y) PLUS its extent in heading times the scan's reach - so the split that minimises the sum of the two
  // bin sizes, in cells: 8 sigma_xy / res / 2^b  +  8 sigma_theta reach / res / 2^(20 - 2 b), b = 4 .. 6.
  out->bits_xy = 6;
  if (in.key_bits_xy >= 4 && in.key_bits_xy <= 6) {
    out->bits_xy = static_cast<uint32_t>(in.key_bits_xy);
  } else if (in.key_bits_xy == 0 && in.resolution > 0.0 && std::isfinite(in.scan_extent)) {
    const double reach = 0.5 * in.scan_extent / in.resolution;  // cells; scan_extent = max |x| + |y| of the scan, ~ sqrt 2 the longest beam
    const double span_xy = spans * std::max(sx, sy) / in.resolution, span_t = 8.0 * std::min(st, kPi / 4.0) * reach;
    double best = std::numeric_limits<double>::infinity();
    for (uint32_t b = 4; b <= 6; ++b) {
      const double cost = std::ldexp(span_xy, -static_cast<int>(b)) + std::ldexp(span_t, -static_cast<int>(20 - 2 * b));
      if (cost < best) {
        best = cost;
        out->bits_xy = b;
      }
    }
  }
  return true;
}

// ---- which likelihood-field kernel a cycle takes -------------------------------------------------------------------------------------

bool LfPlanner::hopelessly_sparse(const LfSite& site, const CloudEstimate& cloud) {
  if (!cloud.valid()) return false;
  const double side = 40.0 * site.resolution;
  const double area = 12.0 * cloud.sigma()[0] * cloud.sigma()[1];
  const double arc = std::min(2.0 * kPi, std::sqrt(12.0) * cloud.sigma()[2]);
  const double volume = std::max(area, side * side) * std::max(arc, 0.05);
  const double poses = static_cast<double>(site.n) * (side * side * 0.05) / volume;
  return poses < 448.0 / 8.0;
}

// Whether the next LF launch goes to the LDS-patch kernel (where its other preconditions hold): by the verdict of the last launch
// that has reported.  A dispersed set (global localisation) has no group that fits a patch, and the patch kernel's workgroups carry
// a wave that would then do nothing.
bool LfPlanner::wants_patches(const LfSite& site, const CloudEstimate& cloud, uint64_t planned, uint64_t through) {
  if (site.tuning.lf_patch == 0) return false;
  if (site.tuning.lf_patch != 1) return true;
  if (planned != seen_planned_) {  // a launch has reported since the last look
    const uint64_t dp = (planned - seen_planned_) & 0xFFFFFFFFull, dt = (through - seen_through_) & 0xFFFFFFFFull;
    seen_planned_ = planned;
    seen_through_ = through;
    patch_useful_ = 4 * dt >= dp;
    if (!patch_useful_) probe_in_ = 16;
  }
  if (patch_useful_) return true;
  if (--probe_in_ <= 0) {
    probe_in_ = 16;
    return !hopelessly_sparse(site, cloud);  // a probe (3.7 ms instead of 1.1 on 1M dispersed particles: not where it cannot succeed)
  }
  return false;
}

LfPlanner::Mode LfPlanner::decide(const LfSite& site, const CloudEstimate& cloud, uint64_t planned, uint64_t through) {
  if (decided_) return mode_;
  decided_ = true;
  mode_ = Mode{false, false};
  if (site.sensor_kind == MCL_SENSOR_BEAM || off_grid(site.sensor_kind)) return mode_;
  const Tuning& t = site.tuning;
  const bool palette = site.palette && t.lf_table == 0;
  if (t.lf_variant == kLfBeamLanes) {
    mode_.beams = palette;
    return mode_;
  }
  if (t.lf_variant != kLfSortedLanes) return mode_;
  mode_.patches = wants_patches(site, cloud, planned, through);
  mode_.beams = !mode_.patches && t.lf_patch == 1 && t.lf_dispersed == 1 && !patch_useful_ && palette && !lf_set_is_small(site.n, t);
  return mode_;
}

void LfPlanner::set_installed(Installed how, uint64_t planned, uint64_t through) {
  if (how == Installed::kKept) return;
  seen_planned_ = planned;
  seen_through_ = through;
  patch_useful_ = how == Installed::kFresh;
  if (how == Installed::kDispersed) probe_in_ = 16;
}

bool LfPlanner::wants_ordering(const LfSite& site) const {
  const Tuning& t = site.tuning;
  if (site.n >= (1ull << 32)) return false;
  if (off_grid(site.sensor_kind)) return false;  // (a lane per particle in index order: these maps live in L2 or the scalar cache, locality buys nothing)
  if (site.sensor_kind == MCL_SENSOR_BEAM) return site.n >= static_cast<uint64_t>(t.beam_sort_min_particles);
  if (site.n < static_cast<uint64_t>(t.sort_min_particles)) return false;
  if (decided_ && mode_.beams) return false;
  return t.lf_variant == kLfSortedLanes && !(lf_set_is_small(site.n, t) && site.palette && t.lf_table == 0);
}

uint32_t LfPlanner::key_layout(const LfSite& site) const {
  const Tuning& t = site.tuning;
  const uint32_t curve = t.key_curve ? 0u : 2u;  // heading-major keys: Hilbert curve (default) / Morton order
  if (t.key_layout >= 0) return (t.key_layout ? 1u : 0u) | curve;
  return (site.sensor_kind != MCL_SENSOR_BEAM && !off_grid(site.sensor_kind) && t.lf_patch == 1 && !patch_useful_ && t.lf_far_tiles != 0 && site.far_tiles
              ? 1u
              : 0u) |
         curve;
}

bool LfPlanner::gathers_dispersed(const Tuning& tuning) const {
  return !mode_.patches && (tuning.lf_far_tiles == 2 || (tuning.lf_patch == 1 && !patch_useful_));
}

// ---- policies ------------------------------------------------------------------------------------------------------------------------

bool moved_enough(const Pose2& latest, const Pose2& pose, double min_d, double min_a) {
  const Pose2 delta = pose_mul(pose_inverse(latest), pose);
  return std::sqrt(delta.x * delta.x + delta.y * delta.y) > min_d || std::abs(rot_log(delta.r)) > min_a;
}

HostPolicy host_policy(ExponentialFilter& slow, ExponentialFilter& fast, bool selective_resampling, bool fires, double norm_sum,
                       double norm_sumsq, uint64_t n) {
  HostPolicy r;
  const double average = norm_sum / static_cast<double>(n);
  const double fast_average = fast(average), slow_average = slow(average);
  if (std::abs(slow_average) >= std::numeric_limits<double>::epsilon())
    r.random_state_probability = std::clamp(1.0 - fast_average / slow_average, 0.0, 1.0);
  r.resample = fires;
  if (fires && selective_resampling) {
    r.ess = norm_sum == 0.0 ? 0.0 : (norm_sum * norm_sum) / norm_sumsq;
    r.resample = r.ess < static_cast<double>(n) * 0.5;
  }
  return r;
}

// ---- particle shards -----------------------------------------------------------------------------------------------------------------

bool grid_cycle_is_small(const GridCycleFacts& f) {
  return f.small_fused && f.n <= kSmallCycleMaxParticles && f.max_particles <= kSmallCycleMaxParticles;
}

bool ndt_cycle_is_small(const NdtCycleFacts& f) {
  return f.small_cycle && f.small_fused && !f.profiling && f.n >= 1 && f.n <= kSmallCycleMaxParticles && f.max_particles >= 1 &&
         f.max_particles <= kSmallCycleMaxParticles;
}

bool landmark_cycle_is_small(const LandmarkCycleFacts& f) {
  return f.small_cycle && f.small_fused && !f.profiling && f.n >= 1 && f.n <= kSmallCycleMaxParticles && f.max_particles >= 1 &&
         f.max_particles <= kSmallCycleMaxParticles;
}

void ndt_hand_back_taken(const NdtHandBack& h, ExponentialFilter& slow, ExponentialFilter& fast) {
  slow.output = h.slow;
  fast.output = h.fast;
}

void ndt_hand_back_resamples(const NdtHandBack& h, ExponentialFilter& slow, ExponentialFilter& fast, bool* force_update) {
  if (h.p > 0.0) {  // :184-186
    slow.reset();
    fast.reset();
  }
  *force_update = false;  // :199
}

void shard_bounds(uint64_t n_total, uint32_t world, uint32_t rank, uint64_t* first, uint64_t* count) {
  const uint64_t base = n_total / world, rem = n_total % world;
  *first = rank * base + std::min<uint64_t>(rank, rem);
  *count = base + (rank < rem ? 1 : 0);
}

uint64_t padded_capacity(uint64_t n_total, uint32_t world, uint32_t permille) {
  const uint64_t m_max = (n_total + world - 1) / world;
  const double mean = static_cast<double>(m_max) / world;
  const double cap = mean * (permille / 1000.0) + 8.0 * std::sqrt(mean) + 64.0;
  return (static_cast<uint64_t>(cap) + 63u) & ~63ull;
}

uint64_t rebalance_block(uint64_t pos, uint64_t cnt, uint64_t n_out, uint32_t world, uint32_t rank, uint64_t* send, uint64_t* recv) {
  auto overlap = [](uint64_t a0, uint64_t a1, uint64_t b0, uint64_t b1) {
    const uint64_t lo = std::max(a0, b0), hi = std::min(a1, b1);
    return hi > lo ? hi - lo : 0;
  };
  uint64_t new_first, new_n, my_lo, my_m;
  shard_bounds(n_out, world, rank, &new_first, &new_n);
  shard_bounds(cnt, world, rank, &my_lo, &my_m);
  for (uint32_t q = 0; q < world; ++q) {
    uint64_t q_lo, q_m, span_first, span_n;
    shard_bounds(cnt, world, q, &q_lo, &q_m);
    shard_bounds(n_out, world, q, &span_first, &span_n);
    send[q] = overlap(pos + my_lo, std::min(pos + my_lo + my_m, n_out), span_first, span_first + span_n) * 4 * sizeof(double);
    recv[q] = overlap(pos + q_lo, std::min(pos + q_lo + q_m, n_out), new_first, new_first + new_n) * 4 * sizeof(double);
  }
  return std::min(std::max(pos, new_first) - new_first, new_n);
}

bool estimate_needs_repivot(const double sums[12]) {
  const double w = sums[0];
  if (!(w > 0.0)) return false;
  const double mx = sums[4] / w, my = sums[5] / w;
  const double m2 = mx * mx + my * my, second = (sums[6] + sums[8]) / w;
  if (!(m2 - m2 == 0.0 && second - second == 0.0)) return false;
  return (1.0 + kRepivotMultiple) * m2 > kRepivotMultiple * second;
}

bool propagation_writes_field_poses(const Tuning& tuning, bool have_buffer, bool have_map) {
  return tuning.lf_pose_ahead != 0 && have_buffer && have_map;
}

FieldPosePlan field_pose_plan(const Tuning& tuning, bool have_buffer, const SetFacts& facts, uint64_t map_generation) {
  if (tuning.lf_pose_ahead == 0 || !have_buffer) return FieldPosePlan{false, false};
  return FieldPosePlan{true, !facts.field_poses_current(map_generation)};
}

}  // namespace mcl
