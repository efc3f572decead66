// beam_skip_host.cpp - see beam_skip_host.h.
#include "beam_skip_host.h"

#include <cmath>

namespace mcl {

const char* beam_skip_check_params(const mcl_beam_skip_params& p) {
  if (p.enabled != 0 && p.enabled != 1) return "beam skip: enabled must be 0 or 1";
  if (!(std::isfinite(p.distance) && p.distance > 0.0)) return "beam skip: distance must be positive and finite";
  if (!(p.threshold >= 0.0 && p.threshold <= 1.0)) return "beam skip: threshold must lie in [0, 1]";
  if (!(p.error_threshold >= 0.0 && p.error_threshold <= 1.0)) return "beam skip: error_threshold must lie in [0, 1]";
  return nullptr;
}

float beam_skip_level(const mcl_lf_params& lf, double distance) {
  constexpr double kPiD = 3.14159265358979323846;
  const double two_squared_sigma = 2 * lf.sigma_hit * lf.sigma_hit;
  const double amplitude = lf.z_hit / (lf.sigma_hit * std::sqrt(2 * kPiD));
  const double offset = lf.z_random / lf.max_laser_distance;
  const float squared = static_cast<float>(distance * distance);  // the builder's distances are floats
  return static_cast<float>(amplitude * std::exp(-static_cast<double>(squared) / two_squared_sigma) + offset);
}

BeamSkipDecision beam_skip_decide(const uint32_t* counts, uint64_t B, uint64_t n, double threshold, double error_threshold, uint8_t* kept) {
  uint64_t kept_count = 0;
  for (uint64_t b = 0; b < B; ++b) {
    const bool keep = static_cast<double>(counts[b]) / static_cast<double>(n) > threshold;
    if (kept) kept[b] = keep ? 1 : 0;
    kept_count += keep ? 1 : 0;
  }
  const uint64_t skipped = B - kept_count;
  const bool used_all = B > 0 && static_cast<double>(skipped) / static_cast<double>(B) >= error_threshold;
  return BeamSkipDecision{skipped, used_all};
}

}  // namespace mcl
