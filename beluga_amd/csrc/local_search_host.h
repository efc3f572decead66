// local_search_host.h — the host rule of the local pose search (mcl_local_search*, include/beluga_mcl.h): the parameter checks, the
// offset and rotation tables, the lattice arithmetic (ids, their inverse, the pass plan), the order key and the moments' finish.
// Plain C++17, no HIP: tests/test_local_search_host_cpu.py holds it to tests/local_search_reference.py on the CPU,
// tests/cpp/local_search_host_check.cpp runs it under the sanitizers.
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

#include "beluga_mcl.h"
#include "se2.h"

namespace mcl {

constexpr uint32_t kLocalMaxHalfXY = 32, kLocalMaxHalfTheta = 64;
constexpr uint32_t kLocalSums = 10;  // S0 | i j k | ii ij ik jj jk kk

inline mcl_local_search_params local_default_params() { return mcl_local_search_params{4, 5, 0.0, kPi / 360.0}; }
// nullptr, or what is wrong with the parameters (step_xy == 0 passes: whether a cell size stands behind it is the context's question).
const char* local_check_params(const mcl_local_search_params& p);

inline uint32_t local_side(uint32_t half_steps) { return 2 * half_steps + 1; }
inline uint64_t local_candidates(const mcl_local_search_params& p) {
  return static_cast<uint64_t>(local_side(p.half_steps_xy)) * local_side(p.half_steps_xy) * local_side(p.half_steps_theta);
}
inline uint32_t local_id(uint32_t Kx, uint32_t Kt, int32_t i, int32_t j, int32_t k) {
  const uint32_t nx = local_side(Kx);
  return (static_cast<uint32_t>(k + static_cast<int32_t>(Kt)) * nx + static_cast<uint32_t>(j + static_cast<int32_t>(Kx))) * nx +
         static_cast<uint32_t>(i + static_cast<int32_t>(Kx));
}
inline void local_offsets_of(uint32_t Kx, uint32_t Kt, uint32_t id, int32_t& i, int32_t& j, int32_t& k) {
  const uint32_t nx = local_side(Kx);
  i = static_cast<int32_t>(id % nx) - static_cast<int32_t>(Kx);
  j = static_cast<int32_t>(id / nx % nx) - static_cast<int32_t>(Kx);
  k = static_cast<int32_t>(id / nx / nx) - static_cast<int32_t>(Kt);
}
// off[i + Kx] = double(i) * step_xy: 2 Kx + 1 doubles.
void local_offsets(uint32_t Kx, double step_xy, std::vector<double>& off);
// (cos, sin) of seed s at step k at [(s * (2 Kt + 1) + k + Kt) * 2]: rot_mul(seed.r, rot_exp(double(k) * step_theta)), and the seed's
// rotation as given for k == 0.  seeds: n x (cos, sin, x, y).
void local_rotations(const double* seeds, uint64_t n, uint32_t Kt, double step_theta, std::vector<double>& cos_sin);
// The pose of candidate `id` of a seed, by the expressions the device uses (off and rot are this seed's tables).
inline void local_pose(const double seed[4], const double* off, const double* rot, uint32_t Kx, uint32_t Kt, uint32_t id, double pose[4]) {
  int32_t i, j, k;
  local_offsets_of(Kx, Kt, id, i, j, k);
  pose[0] = rot[2 * (k + static_cast<int32_t>(Kt))];
  pose[1] = rot[2 * (k + static_cast<int32_t>(Kt)) + 1];
  pose[2] = seed[2] + off[i + static_cast<int32_t>(Kx)];
  pose[3] = seed[3] + off[j + static_cast<int32_t>(Kx)];
}

// A pass takes max(1, search_chunk / L) whole seeds; its buffers hold seeds_per_pass * L <= max(search_chunk, L) candidates.
struct LocalPlan {
  uint64_t seeds_per_pass;
  uint64_t pass_candidates;
  uint32_t passes;
};
LocalPlan local_plan(uint64_t n, uint64_t L, int64_t search_chunk);

// The integer keys behind the score in one word, lower first: i*i + j*j (at most 2048: 12 bits) | |k| (at most 64: 7 bits) | id (below
// 2^20).  With search_key(score) (search_host.h) in front, `a` comes before `b` when its score key is higher, or equal and its tie key lower.
inline uint64_t local_tie_key(uint32_t Kx, uint32_t Kt, uint32_t id) {
  int32_t i, j, k;
  local_offsets_of(Kx, Kt, id, i, j, k);
  return (static_cast<uint64_t>(i * i + j * j) << 27) | (static_cast<uint64_t>(k < 0 ? -k : k) << 20) | id;
}
inline uint32_t local_id_of_tie_key(uint64_t tie) { return static_cast<uint32_t>(tie & 0xFFFFFu); }
inline uint64_t local_score_key(double score) {  // search_key's image (search_host.h), restated so that this file stands alone
  if (score != score) return 0;
  uint64_t bits;
  std::memcpy(&bits, &score, sizeof bits);
  return (bits >> 63) ? ~bits : (bits | (1ull << 63));
}
inline bool local_before(uint64_t score_key_a, uint64_t tie_a, uint64_t score_key_b, uint64_t tie_b) {
  return score_key_a > score_key_b || (score_key_a == score_key_b && tie_a < tie_b);
}

// The header's finish: 3 divisions for the means; per covariance entry a division, a product, a difference and two products by the steps.
// Returns moments_valid.
int32_t local_finish(const double sums[10], double step_xy, double step_theta, const double seed[4], double mean_pose[4], double cov[9]);

}  // namespace mcl
