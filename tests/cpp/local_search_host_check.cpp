// local_search_host_check.cpp — the local pose search's host rule (beluga_amd/csrc/local_search_host.cpp) as a stand-alone program, for
// a CPU build under the sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ibeluga_amd/csrc
//       tests/cpp/local_search_host_check.cpp beluga_amd/csrc/local_search_host.cpp -o local_search_host_check && ./local_search_host_check
// Exercises every function of the file at its edges; exits 0 and prints "local_search_host_check OK" if every expectation holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "local_search_host.h"

#define EXPECT(cond)                                                       \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

using namespace mcl;

int main() {
  mcl_local_search_params p{};
  mcl_default_local_search_params(&p);
  mcl_default_local_search_params(nullptr);
  EXPECT(p.half_steps_xy == 4 && p.half_steps_theta == 5 && p.step_xy == 0.0 && p.step_theta == kPi / 360.0);
  EXPECT(local_check_params(p) == nullptr && local_candidates(p) == 81 * 11);
  const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
  for (const mcl_local_search_params bad : {mcl_local_search_params{33, 5, 0.1, 0.01}, {4, 65, 0.1, 0.01}, {4, 5, -0.1, 0.01}, {4, 5, 0.1, 0.0},
                                            {4, 5, 0.1, -0.01}, {4, 5, inf, 0.01}, {4, 5, 0.1, inf}, {4, 5, nan, 0.01}, {4, 5, 0.1, nan},
                                            {4, 64, 0.1, kPi / 64.0}, {4, 1, 0.1, kPi}})
    EXPECT(local_check_params(bad) != nullptr);
  EXPECT(local_check_params(mcl_local_search_params{32, 64, 0.0, 0.04}) == nullptr);
  EXPECT(local_check_params(mcl_local_search_params{0, 0, 1e300, 1e300}) == nullptr);

  // the lattice at both ends of its range: every id and its inverse, the tie key's fields, the poses of the whole lattice
  for (const mcl_local_search_params q : {mcl_local_search_params{0, 0, 0.0125, 0.01}, {1, 1, 0.0125, 0.01}, {2, 3, 0.05, 0.02}, {32, 64, 0.01, 0.04},
                                          {0, 64, 0.01, 0.04}, {32, 0, 0.01, 0.04}}) {
    const uint32_t Kx = q.half_steps_xy, Kt = q.half_steps_theta;
    const uint64_t L = local_candidates(q);
    EXPECT(L == static_cast<uint64_t>(2 * Kx + 1) * (2 * Kx + 1) * (2 * Kt + 1) && L <= 545025);
    std::vector<double> off, rot;
    local_offsets(Kx, q.step_xy, off);
    EXPECT(off.size() == 2 * Kx + 1 && off[Kx] == 0.0 && off[0] == -static_cast<double>(Kx) * q.step_xy);
    const double seeds[8] = {std::cos(0.3), std::sin(0.3), 4.0, -2.5, -1.0, 0.0, 1e6, -1e6};
    local_rotations(seeds, 2, Kt, q.step_theta, rot);
    EXPECT(rot.size() == 4 * static_cast<size_t>(2 * Kt + 1));
    for (int s = 0; s < 2; ++s) {
      const double* r = rot.data() + 2 * static_cast<size_t>(s) * (2 * Kt + 1);
      EXPECT(r[2 * Kt] == seeds[4 * s] && r[2 * Kt + 1] == seeds[4 * s + 1]);
      for (uint32_t k = 0; k < 2 * Kt + 1; ++k) EXPECT(std::fabs(std::hypot(r[2 * k], r[2 * k + 1]) - 1.0) < 1e-15);
    }
    for (uint64_t id = 0; id < L; ++id) {
      int32_t i, j, k;
      local_offsets_of(Kx, Kt, static_cast<uint32_t>(id), i, j, k);
      EXPECT(std::abs(i) <= static_cast<int32_t>(Kx) && std::abs(j) <= static_cast<int32_t>(Kx) && std::abs(k) <= static_cast<int32_t>(Kt));
      EXPECT(local_id(Kx, Kt, i, j, k) == id);
      const uint64_t tie = local_tie_key(Kx, Kt, static_cast<uint32_t>(id));
      EXPECT(local_id_of_tie_key(tie) == id && (tie >> 27) == static_cast<uint64_t>(i * i + j * j) && ((tie >> 20) & 0x7F) == static_cast<uint64_t>(std::abs(k)));
      double pose[4];
      local_pose(seeds + 4, off.data(), rot.data() + 2 * (2 * Kt + 1), Kx, Kt, static_cast<uint32_t>(id), pose);
      EXPECT(pose[2] == 1e6 + off[i + static_cast<int32_t>(Kx)] && pose[3] == -1e6 + off[j + static_cast<int32_t>(Kx)]);
      if (i == 0 && j == 0 && k == 0) EXPECT(pose[0] == -1.0 && pose[1] == 0.0 && pose[2] == 1e6 && pose[3] == -1e6);
    }
  }
  std::vector<double> none;
  local_rotations(nullptr, 0, 64, 0.01, none);
  EXPECT(none.empty());

  // the pass plan: clamped chunks, a lattice larger than the chunk, no seed
  LocalPlan plan = local_plan(5, 27, 64);
  EXPECT(plan.seeds_per_pass == 2 && plan.pass_candidates == 54 && plan.passes == 3);
  plan = local_plan(5, 175, 64);
  EXPECT(plan.seeds_per_pass == 1 && plan.pass_candidates == 175 && plan.passes == 5);
  plan = local_plan(3, 545025, 1);
  EXPECT(plan.seeds_per_pass == 1 && plan.pass_candidates == 545025 && plan.passes == 3);
  plan = local_plan(0, 1, 1ll << 40);
  EXPECT(plan.seeds_per_pass == (1u << 22) && plan.passes == 0);
  plan = local_plan((1ull << 30) + 1, 1, 64);
  EXPECT(plan.seeds_per_pass == 64 && plan.passes == (1u << 24) + 1);

  // the order: the score first, then the radius, |k|, the id; NaN behind everything
  const double values[] = {-inf, -1.0, -0.0, 0.0, 5e-324, 1.0, 1.0000000000000002, inf};
  for (size_t i = 0; i + 1 < sizeof values / sizeof values[0]; ++i) EXPECT(local_score_key(values[i]) < local_score_key(values[i + 1]));
  EXPECT(local_score_key(nan) == 0 && local_score_key(-nan) == 0 && local_score_key(-inf) > 0);
  const auto tie = [](int32_t i, int32_t j, int32_t k) { return local_tie_key(2, 3, local_id(2, 3, i, j, k)); };
  const uint64_t hi = local_score_key(0.7), lo = local_score_key(0.6);
  EXPECT(local_before(hi, tie(2, 2, 3), lo, tie(0, 0, 0)) && !local_before(lo, tie(0, 0, 0), hi, tie(2, 2, 3)));
  EXPECT(local_before(hi, tie(1, 0, 3), hi, tie(1, 1, 0)) && local_before(hi, tie(1, 0, 0), hi, tie(1, 0, -1)) && local_before(hi, tie(1, 0, -1), hi, tie(1, 0, 1)));
  EXPECT(!local_before(hi, tie(1, 0, 1), hi, tie(1, 0, 1)) && local_before(local_score_key(-inf), tie(2, 2, 3), local_score_key(nan), tie(0, 0, 0)));

  // the finish: a uniform response over Kx = 1, Kt = 1 (27 candidates): the means 0, the variances 2/3 step^2
  const double uniform[10] = {27.0, 0.0, 0.0, 0.0, 18.0, 0.0, 0.0, 18.0, 0.0, 18.0};
  const double seed[4] = {0.6, 0.8, 3.0, -4.0};
  double mean[4], cov[9];
  int32_t valid = 7;
  mcl_local_search_params q{1, 1, 0.5, 0.25};
  EXPECT(mcl_local_search_finish(uniform, &q, seed, mean, cov, &valid) == MCL_OK && valid == 1);
  EXPECT(mean[2] == 3.0 && mean[3] == -4.0 && std::fabs(mean[0] - 0.6) < 1e-15 && std::fabs(mean[1] - 0.8) < 1e-15);
  EXPECT(std::fabs(cov[0] - 0.25 * 2.0 / 3.0) < 1e-16 && cov[0] == cov[4] && std::fabs(cov[8] - 0.0625 * 2.0 / 3.0) < 1e-17);
  EXPECT(cov[1] == 0.0 && cov[2] == 0.0 && cov[3] == 0.0 && cov[5] == 0.0 && cov[6] == 0.0 && cov[7] == 0.0);
  for (const double S0 : {0.0, -0.0, inf, -inf, nan}) {
    double sums[10] = {S0, 1, 2, 3, 4, 5, 6, 7, 8, 9};
    EXPECT(mcl_local_search_finish(sums, &q, seed, mean, cov, &valid) == MCL_OK && valid == 0);
    for (int c = 0; c < 4; ++c) EXPECT(mean[c] == seed[c]);
    for (int c = 0; c < 9; ++c) EXPECT(cov[c] == 0.0);
  }
  EXPECT(mcl_local_search_finish(uniform, nullptr, seed, mean, cov, &valid) == MCL_OK && valid == 1);
  valid = 7;
  EXPECT(mcl_local_search_finish(nullptr, &q, seed, mean, cov, &valid) == MCL_ERR_INVALID_ARGUMENT);
  EXPECT(mcl_local_search_finish(uniform, &q, nullptr, mean, cov, &valid) == MCL_ERR_INVALID_ARGUMENT);
  EXPECT(mcl_local_search_finish(uniform, &q, seed, nullptr, cov, &valid) == MCL_ERR_INVALID_ARGUMENT);
  EXPECT(mcl_local_search_finish(uniform, &q, seed, mean, nullptr, &valid) == MCL_ERR_INVALID_ARGUMENT);
  EXPECT(mcl_local_search_finish(uniform, &q, seed, mean, cov, nullptr) == MCL_ERR_INVALID_ARGUMENT);
  const double bad_seed[4] = {0.6, nan, 3.0, -4.0};
  EXPECT(mcl_local_search_finish(uniform, &q, bad_seed, mean, cov, &valid) == MCL_ERR_INVALID_ARGUMENT);
  q.half_steps_xy = 33;
  EXPECT(mcl_local_search_finish(uniform, &q, seed, mean, cov, &valid) == MCL_ERR_INVALID_ARGUMENT && valid == 7);
  std::puts("local_search_host_check OK");
  return 0;
}
