// SharedMap of include/beluga_amd/amcl.hpp: three small filters in one AmclBatch that read ONE map on the device (AmclBatch::use_map)
// beside three lone Amcl twins that each hold the same grid privately, four update cycles; the SharedMap object goes out of scope
// before the batch does.  Prints "key value" lines that tests/test_cpp_shared_map.py checks; `equal 1` says that every estimate and
// every particle of the members equals its twin's, bit for bit.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "beluga_amd/amcl.hpp"

int main() {
  using namespace beluga_amd;
  const std::uint32_t W = 101, H = 75;  // (off the 8 x 8 tile on both axes)
  std::vector<std::int8_t> cells(W * H, 0);
  for (std::uint32_t x = 0; x < W; ++x) cells[x] = cells[(H - 1) * W + x] = 100;
  for (std::uint32_t y = 0; y < H; ++y) cells[y * W] = cells[y * W + W - 1] = 100;
  for (std::uint32_t y = 20; y < 51; ++y) cells[y * W + 60] = 100;
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
  const std::size_t sizes[3][2] = {{300, 300}, {200, 900}, {1025, 1025}};
  const std::size_t beams[3] = {61, 180, 259};
  try {
    std::vector<AmclBatchSpec> specs;
    std::vector<std::unique_ptr<Amcl>> twins;
    for (int i = 0; i < 3; ++i) {
      AmclParams params;
      params.min_particles = sizes[i][0];
      params.max_particles = sizes[i][1];
      specs.push_back(AmclBatchSpec{OccupancyGridView{}, motion, lf, params, /*seed=*/100u + static_cast<unsigned>(i), {}});  // (no map yet)
      twins.push_back(std::make_unique<Amcl>(map, motion, lf, params, 100u + static_cast<unsigned>(i)));
    }
    AmclBatch batch{specs};
    std::uint32_t users_attached = 0, users_one_swapped = 0;
    std::uint64_t map_bytes = 0;
    {
      SharedMap shared{map, lf};
      SharedMap moved{std::move(shared)};
      batch.use_map(moved);
      users_attached = moved.info().users;
      map_bytes = moved.info().device_bytes;
      batch.use_map(1, moved);  // (the map it reads already: counted once)
      users_one_swapped = moved.info().users;
    }  // the caller's reference goes here; the members keep the map
    const Matrix3d covariance{0.04, 0, 0, 0, 0.04, 0, 0, 0, 0.01};
    for (int i = 0; i < 3; ++i) {
      batch.member(static_cast<std::size_t>(i)).initialize(SE2d{0.0, -1.0, 0.0}, covariance);
      twins[static_cast<std::size_t>(i)]->initialize(SE2d{0.0, -1.0, 0.0}, covariance);
    }
    bool equal = true;
    for (int cycle = 1; cycle <= 4; ++cycle) {
      std::vector<SE2d> controls(3, SE2d{0.1 * cycle, 0.3 * cycle, 0.0});
      std::vector<Amcl::measurement_type> scans(3);
      for (int i = 0; i < 3; ++i)
        for (std::size_t b = 0; b < beams[i]; ++b) {
          const double a = -2.0 + 4.0 * static_cast<double>(b) / static_cast<double>(beams[i]);
          scans[static_cast<std::size_t>(i)].emplace_back(1.5 * std::cos(a), 1.5 * std::sin(a));
        }
      const auto got = batch.update(controls, scans);
      for (std::size_t i = 0; i < 3; ++i) {
        const auto want = twins[i]->update(controls[i], scans[i]);
        equal = equal && got[i].has_value() && want.has_value() && std::memcmp(&got[i]->first, &want->first, sizeof(SE2d)) == 0 &&
                std::memcmp(got[i]->second.data(), want->second.data(), 9 * sizeof(double)) == 0;
        const ParticleSet& a = batch.member(i).particles();
        const ParticleSet& b = twins[i]->particles();
        equal = equal && a.states.size() == b.states.size() &&
                std::memcmp(a.states.data(), b.states.data(), a.states.size() * sizeof(SE2d)) == 0 &&
                std::memcmp(a.weights.data(), b.weights.data(), a.weights.size() * sizeof(double)) == 0;
      }
    }
    std::uint64_t shared_members = 0, owned_bytes = 0;
    for (std::size_t i = 0; i < 3; ++i) {
      std::uint64_t value = 0;
      if (mcl_get_counter(batch.member(i).native_handle(), "map_shared", &value) == MCL_OK) shared_members += value;
      if (mcl_get_counter(batch.member(i).native_handle(), "map_device_bytes", &value) == MCL_OK) owned_bytes += value;
    }
    std::printf("members %zu\n", batch.size());
    std::printf("users %u %u\n", users_attached, users_one_swapped);
    std::printf("map_bytes %llu\n", static_cast<unsigned long long>(map_bytes));
    std::printf("shared_members %llu\n", static_cast<unsigned long long>(shared_members));
    std::printf("owned_bytes %llu\n", static_cast<unsigned long long>(owned_bytes));
    std::printf("equal %d\n", equal ? 1 : 0);
    std::printf("cycles %llu\n", static_cast<unsigned long long>(batch.counter("cycles")));
    std::printf("kernel_launches %llu\n", static_cast<unsigned long long>(batch.counter("kernel_launches")));
    std::printf("members_fused %llu\n", static_cast<unsigned long long>(batch.counter("members_fused")));
    std::printf("members_alone %llu\n", static_cast<unsigned long long>(batch.counter("members_alone")));
    for (std::size_t i = 0; i < 3; ++i) std::printf("particles %zu %zu\n", i, batch.member(i).particles().states.size());
  } catch (const std::runtime_error& e) {
    std::printf("runtime_error %s\n", e.what());
    return 3;
  }
  return 0;
}
