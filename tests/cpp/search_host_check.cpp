// search_host_check.cpp — the global pose search's host rule (beluga_amd/csrc/search_host.cpp) as a stand-alone program, for a CPU build
// under the sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ibeluga_amd/csrc
//       tests/cpp/search_host_check.cpp beluga_amd/csrc/search_host.cpp -o search_host_check && ./search_host_check
// Exercises every function of the file at its edges; exits 0 and prints "search_host_check OK" if every expectation holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "search_host.h"

#define EXPECT(cond)                                                       \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

using namespace mcl;

int main() {
  mcl_search_params p{};
  mcl_default_search_params(&p);
  mcl_default_search_params(nullptr);
  EXPECT(p.cell_stride == 2 && p.headings == 72 && p.pool == 1024 && p.max_results == 16 && p.separation_cells == 10 && p.separation_headings == 6);
  EXPECT(search_check_params(p) == nullptr);
  for (const mcl_search_params bad : {mcl_search_params{0, 8, 16, 4, 0, 0}, {1, 0, 16, 4, 0, 0}, {1, 4097, 16, 4, 0, 0}, {1, 8, 0, 1, 0, 0},
                                      {1, 8, 4097, 4, 0, 0}, {1, 8, 16, 0, 0, 0}, {1, 8, 16, 17, 0, 0}})
    EXPECT(search_check_params(bad) != nullptr);

  // the heading table: unit rotations, the first one at -pi, both ends of the range of headings
  for (const uint32_t headings : {1u, 2u, 72u, 4096u}) {
    std::vector<double> table;
    search_heading_table(headings, table);
    EXPECT(table.size() == 2 * static_cast<size_t>(headings));
    EXPECT(std::fabs(table[0] + 1.0) < 1e-15 && std::fabs(table[1]) < 1e-15);
    for (uint32_t h = 0; h < headings; ++h) {
      const double theta = -kPi + h * (2.0 * kPi / headings);
      EXPECT(std::fabs(table[2 * h] - std::cos(theta)) <= 0x1p-52 && std::fabs(table[2 * h + 1] - std::sin(theta)) <= 0x1p-52);
    }
  }

  // the chunk plan: clamped chunk sizes, more headings than the chunk holds, an empty free list
  SearchPlan plan = search_plan(6899, 16, 64);
  EXPECT(plan.cells_per_chunk == 4 && plan.chunk_candidates == 64 && plan.chunks == 1725 && plan.tiles == 1);
  plan = search_plan(6899, 4096, 1);
  EXPECT(plan.cells_per_chunk == 1 && plan.chunk_candidates == 4096 && plan.chunks == 6899 && plan.tiles == 1);
  plan = search_plan(0, 72, 1ll << 40);
  EXPECT(plan.cells_per_chunk == (1u << 22) / 72 && plan.chunks == 0 && plan.tiles == (plan.chunk_candidates + 4095) / 4096);
  plan = search_plan(0xFFFFFFFFull, 1, 1ll << 20);
  EXPECT(plan.chunks == 4096 && plan.tiles == 256);
  EXPECT(search_merge_levels(0) == 0 && search_merge_levels(4096) == 0 && search_merge_levels(4097) == 1 && search_merge_levels(1u << 20) == 8 &&
         search_merge_levels(3 * 4096) == 2);

  // ids, the stride test, the cell's position
  EXPECT(search_id(0xFFFFFFFFu, 4096, 4095) == 0xFFFFFFFFull * 4096 + 4095);
  EXPECT(search_cell_selected(0, 7, 3) && !search_cell_selected(1, 7, 3) && search_cell_selected(3 * 7 + 6, 7, 3) && !search_cell_selected(2 * 7 + 6, 7, 3));
  double x = 0, y = 0;
  search_cell_position(2 * 10 + 3, 10, 0.5, Pose2{Rot2{0.0, 1.0}, 100.0, -50.0}, x, y);
  EXPECT(x == 100.0 - 1.25 && y == -50.0 + 1.75);

  // the key: order-preserving, NaN lowest, inverted exactly
  const double inf = std::numeric_limits<double>::infinity();
  const double values[] = {-inf, -1e300, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, 1.0000000000000002, 1e300, inf};
  for (size_t i = 0; i + 1 < sizeof values / sizeof values[0]; ++i) EXPECT(search_key(values[i]) < search_key(values[i + 1]));
  for (const double v : values) {
    const double back = search_score(search_key(v));
    EXPECT(back == v && std::signbit(back) == std::signbit(v));
  }
  EXPECT(search_key(std::nan("")) == 0 && search_key(-std::nan("")) == 0 && search_key(-inf) > 0 && std::isnan(search_score(0)));

  // the suppression, through the C entry: at the bound and one beyond, the heading wrap, max_results, refusals
  std::vector<mcl_search_hit> pool;
  const auto add = [&](uint32_t cx, uint32_t cy, uint32_t h) {
    mcl_search_hit hit{};
    hit.cell = cy * 50 + cx;
    hit.heading = h;
    pool.push_back(hit);
  };
  add(10, 10, 71), add(13, 14, 0), add(13, 15, 0), add(10, 10, 2), add(10, 10, 69), add(49, 49, 36);
  std::vector<uint32_t> kept(4096, 0xFFFFFFFFu);
  uint64_t n = 99;
  mcl_search_params q{1, 72, 4096, 4096, 5, 1};
  EXPECT(mcl_search_suppress(pool.data(), pool.size(), 50, &q, kept.data(), &n) == MCL_OK);
  EXPECT(n == 5 && kept[0] == 0 && kept[1] == 2 && kept[2] == 3 && kept[3] == 4 && kept[4] == 5);
  q.max_results = 2;
  EXPECT(mcl_search_suppress(pool.data(), pool.size(), 50, &q, kept.data(), &n) == MCL_OK && n == 2);
  q.separation_cells = 0xFFFFFFFFu;  // the square does not overflow an int64
  q.separation_headings = 0xFFFFFFFFu;
  q.max_results = 4096;
  EXPECT(mcl_search_suppress(pool.data(), pool.size(), 50, &q, kept.data(), &n) == MCL_OK && n == 1);
  EXPECT(mcl_search_suppress(pool.data(), 0, 50, &q, kept.data(), &n) == MCL_OK && n == 0);
  EXPECT(mcl_search_suppress(nullptr, 0, 50, nullptr, kept.data(), &n) == MCL_OK && n == 0);
  n = 99;
  EXPECT(mcl_search_suppress(pool.data(), pool.size(), 0, &q, kept.data(), &n) == MCL_ERR_INVALID_ARGUMENT);
  EXPECT(mcl_search_suppress(nullptr, 3, 50, &q, kept.data(), &n) == MCL_ERR_INVALID_ARGUMENT);
  EXPECT(mcl_search_suppress(pool.data(), pool.size(), 50, &q, nullptr, &n) == MCL_ERR_INVALID_ARGUMENT);
  EXPECT(mcl_search_suppress(pool.data(), pool.size(), 50, &q, kept.data(), nullptr) == MCL_ERR_INVALID_ARGUMENT);
  q.headings = 71;  // pool[0].heading is 71
  EXPECT(mcl_search_suppress(pool.data(), pool.size(), 50, &q, kept.data(), &n) == MCL_ERR_INVALID_ARGUMENT && n == 99);
  std::puts("search_host_check OK");
  return 0;
}
