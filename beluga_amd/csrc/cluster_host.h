// cluster_host.h — the host pass of cluster_based_estimate (algorithm/cluster_based_estimation.hpp) and the merge of the
// shards' cell lists.  Host only: se2.h and the standard library, no HIP and no mcl_ctx, so that a plain C++ compiler can
// build and check it (like map_build.cpp).  The device side - hashing, per-cell aggregation, masked sums - is in kernels.hip.
#pragma once
#include <cstddef>
#include <cstdint>
#include <optional>
#include <type_traits>
#include <vector>

#include "se2.h"

namespace mcl {

// algorithm/spatial_hash.hpp:45-75,87-94,190-193 on the host.
uint64_t host_floor_and_fibo_hash(double value, unsigned shift);
uint64_t host_spatial_hash(const Pose2& s, double res_xy, double res_theta);
// The key a state's cell has in the device's tables: the hash, with the tables' reserved key ~0 ("empty") moved to ~0 - 1.
uint64_t host_cell_key(const Pose2& s, double res_xy, double res_theta);

// One occupied cell.  A list of them is in global first-occurrence order: the order in which the cells' first particles
// appear in the set, which is the order make_cluster_map (:137-157) inserts them in.
// It is also the record the shards exchange, as it stands: 7 doubles (key and count travel as bit patterns).
struct ClusterCell {
  unsigned long long key;
  double weight_sum;
  unsigned long long count;  // particles
  Pose2 state;               // the state of the cell's first particle (cos, sin, x, y)
};
constexpr size_t kCellRecordDoubles = 7;
static_assert(sizeof(ClusterCell) == kCellRecordDoubles * sizeof(double) && std::is_trivially_copyable<ClusterCell>::value,
              "the exchanged record is the struct itself");

// The ranks' records, rank r's first count_of[r] of `stride`, merged in rank order: shards are contiguous pieces of the
// global index space, so rank order followed by local order IS the global first-occurrence order; a cell seen by several
// ranks keeps the state of its first particle and adds up weights and counts.  index_of_rank (optional): where each of
// `rank`'s records went in the result.
std::vector<ClusterCell> merge_cluster_cells(const ClusterCell* gathered, size_t stride, const uint64_t* count_of, uint32_t world,
                                             uint32_t rank = 0, std::vector<uint32_t>* index_of_rank = nullptr);

struct ClusterAssignment {
  std::vector<unsigned int> cluster_of_cell;  // per cell, in the list's order
  std::optional<unsigned int> winner;         // none: no cluster holds more than one particle
  std::vector<double> weight;                 // per cluster id: the sum of its cells' weight sums, added in the list's order
  std::vector<uint64_t> count;                // per cluster id: its particles
};
// make_cluster_map, normalize_and_cap_weights, assign_clusters (:137-238) and the choice of estimate_clusters (:345-411):
// among the clusters with more than one particle, the first one of maximum total weight.  `cells` is not empty.
ClusterAssignment assign_clusters(const std::vector<ClusterCell>& cells, double linear_hash_resolution, double angular_hash_resolution,
                                  double weight_cap_percentile);

// The clusters estimate_clusters (:337-399) reports - those of more than one particle - and the `k` heaviest of them by `weight`,
// ties to the smaller id.
constexpr unsigned int kClusterNotSelected = 0xFFFFFFFFu;
struct ClusterSelection {
  uint64_t eligible = 0;                       // clusters of more than one particle: the size of the reference's vector
  std::vector<unsigned int> selected;          // min(k, eligible) cluster ids, by descending weight, then ascending id
  std::vector<unsigned int> rank_of_cluster;   // per cluster id: its index in `selected`, or kClusterNotSelected
};
ClusterSelection select_heaviest_clusters(const std::vector<double>& weight, const std::vector<uint64_t>& count, size_t k);

}  // namespace mcl
