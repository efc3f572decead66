// AmclBatch of include/beluga_amd/amcl.hpp with four members that return the cluster-based estimate - use_cluster_based_estimate(true),
// which is what beluga_amd::ros::Amcl sets on its filter (ros_amcl.hpp, beluga_ros/src/amcl.cpp:125) - beside four lone filters made the
// same way, four update cycles.  (The lone filters are beluga_amd::Amcl objects, not ros::Amcl ones: the ROS facade seeds its filter from
// the system's entropy source, as the reference does, so no two of its filters can be compared bit for bit.)  Prints "key value" lines
// that tests/test_cpp_batch_cluster.py checks: every estimate, `equal 1` where each of them and every particle equals the lone filter's
// bit for bit, the shared cluster launches and the members that went through them; then a fifth cycle with the members' option
// batch_cluster_fused off, which must not move those counters and must still equal the lone filters.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "beluga_amd/amcl.hpp"

int main() {
  using namespace beluga_amd;
  const std::uint32_t W = 96, H = 64;
  std::vector<std::int8_t> cells(W * H, 0);
  for (std::uint32_t x = 0; x < W; ++x) cells[x] = cells[(H - 1) * W + x] = 100;
  for (std::uint32_t y = 0; y < H; ++y) cells[y * W] = cells[y * W + W - 1] = 100;
  for (std::uint32_t y = 20; y < 44; ++y) cells[y * W + 60] = 100;
  OccupancyGridView map;
  map.cells = cells.data();
  map.width = W;
  map.height = H;
  map.resolution = 0.05;
  map.origin = SE2d{0.0, -2.4, -1.6};

  LikelihoodFieldModelParam lf;
  lf.max_obstacle_distance = 2.0;
  lf.max_laser_distance = 100.0;
  const DifferentialDriveModelParam motion{0.1, 0.05, 0.1, 0.05};
  constexpr std::size_t kMembers = 4;
  const std::size_t sizes[kMembers][2] = {{300, 300}, {200, 900}, {1025, 1025}, {64, 64}};
  const std::size_t beams[kMembers] = {61, 180, 259, 16};
  try {
    std::vector<AmclBatchSpec> specs;
    std::vector<std::unique_ptr<Amcl>> twins;
    for (std::size_t i = 0; i < kMembers; ++i) {
      AmclParams params;
      params.min_particles = sizes[i][0];
      params.max_particles = sizes[i][1];
      specs.push_back(AmclBatchSpec{map, motion, lf, params, /*seed=*/200u + static_cast<unsigned>(i), {}});
      twins.push_back(std::make_unique<Amcl>(map, motion, lf, params, 200u + static_cast<unsigned>(i)));
    }
    AmclBatch batch{specs};
    const Matrix3d covariance{0.04, 0, 0, 0, 0.04, 0, 0, 0, 0.01};
    for (std::size_t i = 0; i < kMembers; ++i) {
      batch.member(i).use_cluster_based_estimate(true);
      twins[i]->use_cluster_based_estimate(true);
      batch.member(i).initialize(SE2d{0.0, -1.0, 0.0}, covariance);
      twins[i]->initialize(SE2d{0.0, -1.0, 0.0}, covariance);
    }
    bool equal = true;
    auto cycle_once = [&](int cycle, bool print) {
      std::vector<SE2d> controls(kMembers, SE2d{0.1 * cycle, 0.3 * cycle, 0.0});
      std::vector<Amcl::measurement_type> scans(kMembers);
      for (std::size_t i = 0; i < kMembers; ++i)
        for (std::size_t b = 0; b < beams[i]; ++b) {
          const double a = -2.0 + 4.0 * static_cast<double>(b) / static_cast<double>(beams[i]);
          scans[i].emplace_back(1.5 * std::cos(a), 1.5 * std::sin(a));
        }
      const auto got = batch.update(controls, scans);
      for (std::size_t i = 0; i < kMembers; ++i) {
        const auto want = twins[i]->update(controls[i], scans[i]);
        equal = equal && got[i].has_value() && want.has_value() && std::memcmp(&got[i]->first, &want->first, sizeof(SE2d)) == 0 &&
                std::memcmp(got[i]->second.data(), want->second.data(), 9 * sizeof(double)) == 0;
        const ParticleSet& a = batch.member(i).particles();
        const ParticleSet& b = twins[i]->particles();
        equal = equal && a.states.size() == b.states.size() &&
                std::memcmp(a.states.data(), b.states.data(), a.states.size() * sizeof(SE2d)) == 0 &&
                std::memcmp(a.weights.data(), b.weights.data(), a.weights.size() * sizeof(double)) == 0;
        if (print && got[i].has_value()) {
          const double* p = got[i]->first.data();
          std::printf("estimate %d %zu %.17g %.17g %.17g %.17g\n", cycle, i, p[0], p[1], p[2], p[3]);
        }
      }
    };
    for (int cycle = 1; cycle <= 4; ++cycle) cycle_once(cycle, true);
    std::printf("members %zu\n", batch.size());
    std::printf("equal %d\n", equal ? 1 : 0);
    std::printf("kernel_launches %llu\n", static_cast<unsigned long long>(batch.counter("kernel_launches")));
    std::printf("cluster_launches %llu\n", static_cast<unsigned long long>(batch.counter("cluster_launches")));
    std::printf("members_cluster_fused %llu\n", static_cast<unsigned long long>(batch.counter("members_cluster_fused")));
    // the switch: every member through its own kernels
    batch.set_option("batch_cluster_fused", 0);
    cycle_once(5, false);
    std::printf("equal_switched_off %d\n", equal ? 1 : 0);
    std::printf("cluster_launches_switched_off %llu\n", static_cast<unsigned long long>(batch.counter("cluster_launches")));
    std::printf("members_fused %llu\n", static_cast<unsigned long long>(batch.counter("members_fused")));
    bool refused = false;
    try {
      batch.set_option("batch_cluster_fusion", 1);
    } catch (const std::runtime_error&) {
      refused = true;
    }
    std::printf("unknown_option_refused %d\n", refused ? 1 : 0);
  } catch (const std::runtime_error& e) {
    std::printf("runtime_error %s\n", e.what());
    return 3;
  }
  return 0;
}
