// local_search_host.cpp — the host rule of the local pose search (local_search_host.h).  Plain C++17, no HIP.
#include "local_search_host.h"

#include <algorithm>
#include <cmath>

namespace mcl {

namespace {
constexpr int64_t kChunkMin = 64, kChunkMax = 1ll << 22;  // option search_chunk's range (search_host.h: kSearchChunkMin, kSearchChunkMax)
}

const char* local_check_params(const mcl_local_search_params& p) {
  if (p.half_steps_xy > kLocalMaxHalfXY) return "half_steps_xy above 32";
  if (p.half_steps_theta > kLocalMaxHalfTheta) return "half_steps_theta above 64";
  if (!std::isfinite(p.step_xy) || !std::isfinite(p.step_theta)) return "a step is not finite";
  if (!(p.step_xy >= 0.0)) return "step_xy is negative";
  if (!(p.step_theta > 0.0)) return "step_theta is not above 0";
  if (!(static_cast<double>(p.half_steps_theta) * p.step_theta < kPi)) return "half_steps_theta * step_theta is not below pi";
  return nullptr;
}

void local_offsets(uint32_t Kx, double step_xy, std::vector<double>& off) {
  off.resize(local_side(Kx));
  for (int32_t i = -static_cast<int32_t>(Kx); i <= static_cast<int32_t>(Kx); ++i) off[i + static_cast<int32_t>(Kx)] = static_cast<double>(i) * step_xy;
}

void local_rotations(const double* seeds, uint64_t n, uint32_t Kt, double step_theta, std::vector<double>& cos_sin) {
  const uint32_t nt = local_side(Kt);
  cos_sin.resize(2 * static_cast<size_t>(n) * nt);
  for (uint64_t s = 0; s < n; ++s) {
    const Rot2 seed{seeds[4 * s], seeds[4 * s + 1]};
    for (int32_t k = -static_cast<int32_t>(Kt); k <= static_cast<int32_t>(Kt); ++k) {
      const Rot2 r = k == 0 ? seed : rot_mul(seed, rot_exp(static_cast<double>(k) * step_theta));
      const size_t at = 2 * (static_cast<size_t>(s) * nt + static_cast<size_t>(k + static_cast<int32_t>(Kt)));
      cos_sin[at] = r.c;
      cos_sin[at + 1] = r.s;
    }
  }
}

LocalPlan local_plan(uint64_t n, uint64_t L, int64_t search_chunk) {
  const uint64_t chunk = static_cast<uint64_t>(std::clamp<int64_t>(search_chunk, kChunkMin, kChunkMax));
  LocalPlan plan{};
  plan.seeds_per_pass = std::max<uint64_t>(1, chunk / L);
  plan.pass_candidates = plan.seeds_per_pass * L;
  plan.passes = static_cast<uint32_t>((n + plan.seeds_per_pass - 1) / plan.seeds_per_pass);
  return plan;
}

int32_t local_finish(const double sums[10], double step_xy, double step_theta, const double seed[4], double mean_pose[4], double cov[9]) {
  const double S0 = sums[0];
  if (!(S0 != 0.0) || !std::isfinite(S0)) {
    std::copy(seed, seed + 4, mean_pose);
    std::fill(cov, cov + 9, 0.0);
    return 0;
  }
  const double m[3] = {sums[1] / S0, sums[2] / S0, sums[3] / S0};
  const double step[3] = {step_xy, step_xy, step_theta};
  const Rot2 r = rot_mul(Rot2{seed[0], seed[1]}, rot_exp(step_theta * m[2]));
  mean_pose[0] = r.c;
  mean_pose[1] = r.s;
  mean_pose[2] = seed[2] + step_xy * m[0];
  mean_pose[3] = seed[3] + step_xy * m[1];
  static const int second[3][3] = {{4, 5, 6}, {5, 7, 8}, {6, 8, 9}};
  for (int a = 0; a < 3; ++a)
    for (int b = a; b < 3; ++b) cov[3 * a + b] = cov[3 * b + a] = ((sums[second[a][b]] / S0 - m[a] * m[b]) * step[a]) * step[b];
  return 1;
}

}  // namespace mcl

extern "C" {

void mcl_default_local_search_params(mcl_local_search_params* params) {
  if (params) *params = mcl::local_default_params();
}

mcl_status mcl_local_search_finish(const double sums[10], const mcl_local_search_params* params, const double seed[4], double mean_pose[4],
                                   double cov[9], int32_t* moments_valid) {
  const mcl_local_search_params p = params ? *params : mcl::local_default_params();
  if (!sums || !seed || !mean_pose || !cov || !moments_valid || mcl::local_check_params(p)) return MCL_ERR_INVALID_ARGUMENT;
  for (int c = 0; c < 4; ++c)
    if (!std::isfinite(seed[c])) return MCL_ERR_INVALID_ARGUMENT;
  *moments_valid = mcl::local_finish(sums, p.step_xy, p.step_theta, seed, mean_pose, cov);
  return MCL_OK;
}

}  // extern "C"
