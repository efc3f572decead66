// estimate_clusters() and cluster_labels() of include/beluga_amd/amcl.hpp on the fine multicluster set of the reference's
// HeaviestClusterSelectionTest (beluga/test/beluga/algorithm/test_cluster_based_estimation.cpp:67-94,357-386): four peaks, one per
// quadrant of [-2, 2]^2.  Prints "key value" lines that tests/test_cpp_cluster_modes.py checks.
#include <cmath>
#include <cstdio>
#include <vector>

#include "beluga_amd/amcl.hpp"

int main() {
  using namespace beluga_amd;
  const std::uint32_t W = 64, H = 64;
  std::vector<std::int8_t> cells(W * H, 0);
  OccupancyGridView map;
  map.cells = cells.data();
  map.width = W;
  map.height = H;
  map.resolution = 0.1;
  map.origin = SE2d{0.0, -3.2, -3.2};

  const double side = 4.0, step = 0.025, pi = 3.14159265358979323846;
  std::vector<SE2d> states;
  std::vector<double> weights;
  for (double x = step / 2.0; x <= side; x += step) {
    for (double y = step / 2.0; y <= side; y += step) {
      const double k = (2 * x < side ? 0.0 : 1.0) + (2 * y < side ? 0.0 : 2.0) + 1.0;
      const double w = std::abs(std::sin(2.0 * pi * x / side)) * std::abs(std::sin(2.0 * pi * y / side)) * k;
      states.emplace_back(0.0, x - 2.0, y - 2.0);
      weights.push_back(std::max(0.0, w - k / 2.0));
    }
  }

  AmclParams params;
  params.min_particles = states.size();
  params.max_particles = states.size();
  LikelihoodFieldModelParam lf;
  lf.max_obstacle_distance = 2.0;
  lf.max_laser_distance = 100.0;
  try {
    Amcl filter{map, DifferentialDriveModelParam{0.1, 0.05, 0.1, 0.05}, lf, params, /*seed=*/123};
    // (initialize(states) gives every particle weight 1; the peaks are in the weights)
    if (mcl_set_particles(filter.native_handle(), states.data()->data(), weights.data(), states.size()) != MCL_OK) {
      std::printf("set_particles %s\n", mcl_last_error(filter.native_handle()));
      return 2;
    }
    const std::vector<ClusterEstimate> found = filter.estimate_clusters();
    std::printf("particles %zu\n", states.size());
    std::printf("clusters %zu\n", found.size());
    for (const ClusterEstimate& e : found)
      std::printf("entry %u %llu %.17g %.17g %.17g %.17g %.17g\n", e.id, static_cast<unsigned long long>(e.count), e.weight, e.mean.x, e.mean.y,
                  e.covariance[0], e.covariance[4]);
    std::printf("two %zu\n", filter.estimate_clusters(ParticleClusterizerParam{}, 2).size());
    const std::vector<std::uint32_t> labels = filter.cluster_labels();
    std::vector<unsigned long long> per_label(found.size(), 0);
    std::size_t out_of_range = 0;
    for (const std::uint32_t l : labels) {
      if (l < per_label.size()) per_label[l] += 1; else out_of_range += 1;
    }
    std::printf("labels %zu %zu\n", labels.size(), out_of_range);
    for (std::size_t l = 0; l < per_label.size(); ++l) std::printf("label_count %zu %llu\n", l, per_label[l]);
    const Amcl::estimation_type best = filter.cluster_based_estimate();
    std::printf("cluster_based_estimate %.17g %.17g\n", best.first.x, best.first.y);
  } catch (const std::runtime_error& e) {
    std::printf("runtime_error %s\n", e.what());
    return 3;
  }
  return 0;
}
