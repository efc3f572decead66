// cluster_host.cpp — see cluster_host.h.
// The cluster assignment runs over the reference's own standard containers, fed in the reference's order: which cell a tie
// goes to is decided by the containers' iteration order, so none of it may be rearranged.
#include "cluster_host.h"

#include <algorithm>
#include <cmath>
#include <queue>
#include <unordered_map>

namespace mcl {

uint64_t host_floor_and_fibo_hash(double value, unsigned shift) {
  const int64_t sv = static_cast<int64_t>(std::floor(value));
  const uint64_t h = 11400714819323198485ull * static_cast<uint64_t>(sv);
  return shift ? ((h << shift) | (h >> (64 - shift))) : h;
}
uint64_t host_spatial_hash(const Pose2& s, double res_xy, double res_theta) {
  return host_floor_and_fibo_hash(s.x / res_xy, 0) ^ host_floor_and_fibo_hash(s.y / res_xy, 21) ^
         host_floor_and_fibo_hash(rot_log(s.r) / res_theta, 42);
}
uint64_t host_cell_key(const Pose2& s, double res_xy, double res_theta) {
  uint64_t hash = host_spatial_hash(s, res_xy, res_theta);
  if (hash == ~0ull) hash -= 1;  // the device table's reserved key
  return hash;
}

std::vector<ClusterCell> merge_cluster_cells(const ClusterCell* gathered, size_t stride, const uint64_t* count_of, uint32_t world,
                                             uint32_t rank, std::vector<uint32_t>* index_of_rank) {
  std::vector<ClusterCell> cells;
  if (index_of_rank) index_of_rank->clear();
  std::unordered_map<unsigned long long, size_t> seen;
  for (uint32_t r = 0; r < world; ++r) {
    for (uint64_t j = 0; j < count_of[r]; ++j) {
      const ClusterCell& rec = gathered[static_cast<size_t>(r) * stride + j];
      const auto [it, fresh] = seen.try_emplace(rec.key, cells.size());
      if (fresh) {
        cells.push_back(rec);
      } else {
        cells[it->second].weight_sum += rec.weight_sum;
        cells[it->second].count += rec.count;
      }
      if (index_of_rank && r == rank) index_of_rank->push_back(static_cast<uint32_t>(it->second));
    }
  }
  return cells;
}

ClusterAssignment assign_clusters(const std::vector<ClusterCell>& g, double linear_hash_resolution, double angular_hash_resolution,
                                  double weight_cap_percentile) {
  const size_t cells = g.size();
  uint64_t n_global = 0;
  for (const ClusterCell& c : g) n_global += c.count;

  // make_cluster_map :137-157
  struct Cell {
    Pose2 representative_state;
    double weight;
    size_t num_particles;
    std::optional<size_t> cluster_id;
    size_t k;
  };
  std::unordered_map<size_t, Cell> map;
  map.reserve(n_global / 5);
  for (size_t k = 0; k < cells; ++k) {
    map.try_emplace(static_cast<size_t>(g[k].key), Cell{g[k].state, g[k].weight_sum, static_cast<size_t>(g[k].count), std::nullopt, k});
  }
  // normalize_and_cap_weights :173-189 (+ calculate_percentile_threshold :103-109)
  for (auto& kv : map) kv.second.weight /= static_cast<double>(kv.second.num_particles);
  {
    std::vector<double> values;
    values.reserve(map.size());
    for (auto& kv : map) values.push_back(kv.second.weight);
    const auto nth = static_cast<std::ptrdiff_t>(static_cast<double>(values.size()) * weight_cap_percentile);
    std::nth_element(values.begin(), values.begin() + nth, values.end());
    const double max_weight = values[static_cast<size_t>(nth)];
    for (auto& kv : map) kv.second.weight = std::min(kv.second.weight, max_weight);
  }
  // assign_clusters :203-238
  struct KeyWithPriority {
    double priority;
    size_t key;
    bool operator<(const KeyWithPriority& other) const { return priority < other.priority; }
  };
  std::vector<KeyWithPriority> init;
  init.reserve(map.size());
  for (auto& kv : map) init.push_back(KeyWithPriority{kv.second.weight, kv.first});
  std::priority_queue<KeyWithPriority> queue(init.begin(), init.end());
  const double max_priority = queue.top().priority;
  const double lin = linear_hash_resolution, ang = angular_hash_resolution;
  const Pose2 adjacent[6] = {Pose2{rot_exp(0.0), +lin, 0.0}, Pose2{rot_exp(0.0), -lin, 0.0}, Pose2{rot_exp(0.0), 0.0, +lin},
                             Pose2{rot_exp(0.0), 0.0, -lin}, Pose2{rot_exp(+ang), 0.0, 0.0}, Pose2{rot_exp(-ang), 0.0, 0.0}};
  size_t next_cluster_id = 0;
  while (!queue.empty()) {
    const size_t hash = queue.top().key;
    queue.pop();
    Cell& cell = map[hash];
    if (!cell.cluster_id.has_value()) cell.cluster_id = next_cluster_id++;
    for (const Pose2& adj : adjacent) {
      const uint64_t neighbor_hash = host_cell_key(pose_mul(cell.representative_state, adj), lin, ang);
      auto it = map.find(static_cast<size_t>(neighbor_hash));
      if (it == map.end() || it->second.cluster_id.has_value() || !(it->second.weight <= cell.weight)) continue;
      it->second.cluster_id = cell.cluster_id;
      queue.push(KeyWithPriority{max_priority + it->second.weight, static_cast<size_t>(neighbor_hash)});
    }
  }
  // estimate_clusters :345-411: clusters with more than one particle, the first one of maximum total weight
  std::vector<double> total_w(next_cluster_id, 0.0);
  std::vector<uint64_t> total_n(next_cluster_id, 0);
  ClusterAssignment out;
  out.cluster_of_cell.resize(cells);
  for (auto& kv : map) out.cluster_of_cell[kv.second.k] = static_cast<unsigned int>(kv.second.cluster_id.value());
  for (size_t k = 0; k < cells; ++k) {  // particle-order accumulation is not reproducible from cell sums; cell order is fixed
    total_w[out.cluster_of_cell[k]] += g[k].weight_sum;
    total_n[out.cluster_of_cell[k]] += g[k].count;
  }
  long best = -1;
  for (size_t c = 0; c < next_cluster_id; ++c)
    if (total_n[c] > 1 && (best < 0 || total_w[static_cast<size_t>(best)] < total_w[c])) best = static_cast<long>(c);
  if (best >= 0) out.winner = static_cast<unsigned int>(best);
  out.weight = std::move(total_w);
  out.count = std::move(total_n);
  return out;
}

ClusterSelection select_heaviest_clusters(const std::vector<double>& weight, const std::vector<uint64_t>& count, size_t k) {
  ClusterSelection out;
  out.rank_of_cluster.assign(weight.size(), kClusterNotSelected);
  for (size_t c = 0; c < weight.size(); ++c)
    if (count[c] > 1) out.selected.push_back(static_cast<unsigned int>(c));  // :382-389 one sample gives no covariance
  out.eligible = out.selected.size();
  const size_t keep = std::min(k, out.selected.size());
  std::partial_sort(out.selected.begin(), out.selected.begin() + static_cast<std::ptrdiff_t>(keep), out.selected.end(),
                    [&weight](unsigned int a, unsigned int b) { return weight[a] > weight[b] || (weight[a] == weight[b] && a < b); });
  out.selected.resize(keep);
  for (size_t r = 0; r < keep; ++r) out.rank_of_cluster[out.selected[r]] = static_cast<unsigned int>(r);
  return out;
}

}  // namespace mcl
