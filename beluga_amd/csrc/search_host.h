// search_host.h — the host rule of the global pose search (mcl_global_search*, include/beluga_mcl.h): the parameter checks, the heading
// table, the enumeration arithmetic (ids, counts, the chunk plan), the order-preserving image of a score, and the greedy suppression.
// Plain C++17, no HIP: tests/test_search_host_cpu.py holds it to tests/search_reference.py on the CPU, tests/cpp/search_host_check.cpp
// runs it under the sanitizers.
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

#include "beluga_mcl.h"
#include "se2.h"

namespace mcl {

constexpr uint32_t kSearchMaxHeadings = 4096, kSearchMaxPool = 4096;
constexpr uint32_t kSearchTile = 4096;  // candidates a workgroup of the selection sorts in LDS (k_search_sort_tiles): 64 KB of (key, id)
constexpr int64_t kSearchChunkMin = 64, kSearchChunkMax = 1ll << 22, kSearchChunkDefault = 1ll << 20;

inline mcl_search_params search_default_params() { return mcl_search_params{2, 72, 1024, 16, 10, 6}; }
// nullptr, or what is wrong with the parameters.
const char* search_check_params(const mcl_search_params& p);
// (cos, sin) of theta_h = -pi + h * (2 pi / headings), h < headings, as rot_exp gives them: 2 * headings doubles.
void search_heading_table(uint32_t headings, std::vector<double>& cos_sin);

// A chunk is a range of the map's free-cell list, before the stride test: cells_per_chunk = max(1, search_chunk / headings) cells, so a
// chunk holds at most max(search_chunk, headings) candidates (and on an open map about 1 / cell_stride^2 of that).
struct SearchPlan {
  uint64_t cells_per_chunk;
  uint64_t chunk_candidates;  // cells_per_chunk * headings: what the chunk's buffers hold
  uint32_t chunks;            // ranges of the free list
  uint32_t tiles;             // sort tiles of a full chunk
};
SearchPlan search_plan(uint64_t free_cells, uint32_t headings, int64_t search_chunk);
// Merge levels behind the tile sort of a chunk of n candidates: the runs are halved until one is left.
uint32_t search_merge_levels(uint64_t n);

inline bool search_cell_selected(uint32_t cell, uint32_t width, uint32_t stride) { return (cell % width) % stride == 0 && (cell / width) % stride == 0; }
inline uint64_t search_id(uint32_t cell, uint32_t headings, uint32_t heading) { return static_cast<uint64_t>(cell) * headings + heading; }
// The centre of a cell in the world: random_free_state's expressions (kernels.hip), operation by operation.
inline void search_cell_position(uint32_t cell, uint32_t width, double resolution, const Pose2& origin, double& x, double& y) {
  const double lx = (static_cast<double>(static_cast<int>(cell % width)) + 0.5) * resolution;
  const double ly = (static_cast<double>(static_cast<int>(cell / width)) + 0.5) * resolution;
  double gx, gy;
  rot_apply(origin.r, lx, ly, gx, gy);
  x = gx + origin.x;
  y = gy + origin.y;
}

// The u64 image of a score whose unsigned order is the scores' order; NaN is the lowest (0).  search_score inverts it (NaN for 0).
inline uint64_t search_key(double score) {
  if (score != score) return 0;
  uint64_t bits;
  std::memcpy(&bits, &score, sizeof bits);
  return (bits >> 63) ? ~bits : (bits | (1ull << 63));
}
inline double search_score(uint64_t key) {
  uint64_t bits = (key >> 63) ? (key & ~(1ull << 63)) : ~key;
  if (key == 0) bits = 0x7ff8000000000000ull;
  double score;
  std::memcpy(&score, &bits, sizeof score);
  return score;
}

// Greedy suppression in pool order (the header's rule): kept_index[k] = the pool index of the k-th kept hit; returns how many were kept
// (at most p.max_results).  Integers only.
uint64_t search_suppress(const mcl_search_hit* pool, uint64_t n, uint32_t grid_width, const mcl_search_params& p, uint32_t* kept_index);

}  // namespace mcl
