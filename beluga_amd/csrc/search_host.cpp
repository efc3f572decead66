// search_host.cpp — the host rule of the global pose search (search_host.h).  Plain C++17, no HIP.
#include "search_host.h"

#include <algorithm>

namespace mcl {

const char* search_check_params(const mcl_search_params& p) {
  if (p.cell_stride == 0) return "cell_stride is 0";
  if (p.headings < 1 || p.headings > kSearchMaxHeadings) return "headings outside 1 .. 4096";
  if (p.pool < 1 || p.pool > kSearchMaxPool) return "pool outside 1 .. 4096";
  if (p.max_results < 1 || p.max_results > p.pool) return "max_results outside 1 .. pool";
  return nullptr;
}

void search_heading_table(uint32_t headings, std::vector<double>& cos_sin) {
  cos_sin.resize(2 * static_cast<size_t>(headings));
  const double step = 2.0 * kPi / static_cast<double>(headings);
  for (uint32_t h = 0; h < headings; ++h) {
    const Rot2 r = rot_exp(-kPi + static_cast<double>(h) * step);
    cos_sin[2 * h] = r.c;
    cos_sin[2 * h + 1] = r.s;
  }
}

SearchPlan search_plan(uint64_t free_cells, uint32_t headings, int64_t search_chunk) {
  const uint64_t chunk = static_cast<uint64_t>(std::clamp<int64_t>(search_chunk, kSearchChunkMin, kSearchChunkMax));
  SearchPlan plan{};
  plan.cells_per_chunk = std::max<uint64_t>(1, chunk / headings);
  plan.chunk_candidates = plan.cells_per_chunk * headings;
  plan.chunks = static_cast<uint32_t>((free_cells + plan.cells_per_chunk - 1) / plan.cells_per_chunk);
  plan.tiles = static_cast<uint32_t>((plan.chunk_candidates + kSearchTile - 1) / kSearchTile);
  return plan;
}

uint32_t search_merge_levels(uint64_t n) {
  uint32_t levels = 0;
  for (uint64_t runs = (n + kSearchTile - 1) / kSearchTile; runs > 1; runs = (runs + 1) / 2) ++levels;
  return levels;
}

uint64_t search_suppress(const mcl_search_hit* pool, uint64_t n, uint32_t grid_width, const mcl_search_params& p, uint32_t* kept_index) {
  // unsigned 64-bit: the square of a 32-bit separation or coordinate difference fits; the sum of two squares may wrap, and is then
  // beyond every reach
  const uint64_t reach = static_cast<uint64_t>(p.separation_cells) * p.separation_cells;
  const int64_t headings = p.headings;
  uint64_t kept = 0;
  for (uint64_t i = 0; i < n && kept < p.max_results; ++i) {
    const int64_t x = pool[i].cell % grid_width, y = pool[i].cell / grid_width, h = pool[i].heading;
    bool near = false;
    for (uint64_t k = 0; k < kept && !near; ++k) {
      const mcl_search_hit& other = pool[kept_index[k]];
      const int64_t dx = x - static_cast<int64_t>(other.cell % grid_width), dy = y - static_cast<int64_t>(other.cell / grid_width);
      const int64_t dh = h > other.heading ? h - other.heading : other.heading - h;
      const uint64_t ax = static_cast<uint64_t>(dx < 0 ? -dx : dx), ay = static_cast<uint64_t>(dy < 0 ? -dy : dy);
      const uint64_t dx2 = ax * ax, d2 = dx2 + ay * ay;
      near = d2 >= dx2 && d2 <= reach && std::min(dh, headings - dh) <= static_cast<int64_t>(p.separation_headings);
    }
    if (!near) kept_index[kept++] = static_cast<uint32_t>(i);
  }
  return kept;
}

}  // namespace mcl

extern "C" {

void mcl_default_search_params(mcl_search_params* params) {
  if (params) *params = mcl::search_default_params();
}

mcl_status mcl_search_suppress(const mcl_search_hit* pool, uint64_t n, uint32_t grid_width, const mcl_search_params* params, uint32_t* kept_index,
                               uint64_t* kept) {
  const mcl_search_params p = params ? *params : mcl::search_default_params();
  if (!kept_index || !kept || (n != 0 && !pool) || grid_width == 0 || mcl::search_check_params(p)) return MCL_ERR_INVALID_ARGUMENT;
  for (uint64_t i = 0; i < n; ++i)
    if (pool[i].heading >= p.headings) return MCL_ERR_INVALID_ARGUMENT;
  *kept = mcl::search_suppress(pool, n, grid_width, p, kept_index);
  return MCL_OK;
}

}  // extern "C"
