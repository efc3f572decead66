// local_search_demo.cpp - the local pose search through the header-only facades on the small asymmetric map of search_demo.cpp:
// beluga_amd::Amcl::global_search, then local_search about its hits and relocalize with refinement, with points in the base frame; then
// beluga_amd::ros::Amcl::local_search with a laser scan whose sensor sits 0.25 m ahead of the base (the same points, so the same hits).
// Prints "hit <di> <dj> <dk> <plateau> <score> <seed_score> <x> <y> <cos> <sin> <mean x> <mean y> <cov xx> <cov yy> <cov tt>" per seed
// of the plain facade, "refined ..." per hit of relocalize (ordered by refined score), "estimate x y theta" after it, and "ros_hit ..."
// per seed of the ROS facade.  Exit code 3: no usable GPU (no CPU fallback).
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "beluga_amd/ros_amcl.hpp"

namespace {
// The least a grid, a laser scan and their transforms have to offer the ROS facade (beluga_ros::OccupancyGrid, beluga_ros::LaserScan).
struct Origin2 {
  double v[4];  // cos, sin, x, y
  [[nodiscard]] int so2() const { return 0; }
  [[nodiscard]] const double* data() const { return v; }
};
struct Grid {
  std::vector<std::int8_t> cells;
  std::size_t w, h;
  double res;
  Origin2 at;
  [[nodiscard]] const std::vector<std::int8_t>& data() const { return cells; }
  [[nodiscard]] std::size_t width() const { return w; }
  [[nodiscard]] std::size_t height() const { return h; }
  [[nodiscard]] double resolution() const { return res; }
  [[nodiscard]] const Origin2& origin() const { return at; }
};
struct Point2 {
  double px, py;
  [[nodiscard]] double x() const { return px; }
  [[nodiscard]] double y() const { return py; }
};
struct Origin3 {
  double v[7];  // qx qy qz qw tx ty tz
  [[nodiscard]] const double* data() const { return v; }
};
struct Scan {
  std::vector<Point2> points;
  Origin3 sensor;
  [[nodiscard]] const std::vector<Point2>& points_in_cartesian_coordinates() const { return points; }
  [[nodiscard]] const Origin3& origin() const { return sensor; }
};

template <class Hit>
void print_hit(const char* tag, const Hit& h) {
  std::printf("%s %d %d %d %llu %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", tag, h.di, h.dj, h.dk,
              static_cast<unsigned long long>(h.plateau), h.score, h.seed_score, h.pose.x, h.pose.y, h.pose.c, h.pose.s, h.mean_pose.x, h.mean_pose.y,
              h.cov[0], h.cov[4], h.cov[8]);
}
}  // namespace

int main() {
  using namespace beluga_amd;
  const std::uint32_t W = 64, H = 48;
  std::vector<std::int8_t> cells(W * H, 0);
  for (std::uint32_t x = 0; x < W; ++x) cells[x] = cells[(H - 1) * W + x] = 100;
  for (std::uint32_t y = 0; y < H; ++y) cells[y * W] = cells[y * W + W - 1] = 100;
  for (std::uint32_t x = 0; x < W; ++x)
    if (x < 12 || x > 18) cells[30 * W + x] = 100;
  for (std::uint32_t y = 0; y < 30; ++y) cells[y * W + 40] = 100;
  OccupancyGridView map;
  map.cells = cells.data();
  map.width = W;
  map.height = H;
  map.resolution = 0.1;
  map.origin = SE2d{0.0, -1.0, -1.0};
  AmclParams params;
  params.min_particles = 300;
  params.max_particles = 1500;
  params.update_min_d = 0.0;
  params.update_min_a = 0.0;
  LikelihoodFieldModelParam lf;
  lf.max_obstacle_distance = 2.0;
  lf.max_laser_distance = 100.0;
  const Amcl::measurement_type scan{{3.0, 0.0}, {0.0, 2.0}, {-1.0, 0.0}, {0.0, -1.0}, {3.0, 1.0}, {3.0, -1.0}, {1.0, 2.0}, {-1.0, 1.0}};
  try {
    Amcl filter{map, DifferentialDriveModelParam{0.1, 0.05, 0.1, 0.05}, lf, params, /*seed=*/5};
    Amcl::SearchParams search;
    search.headings = 36;
    search.max_results = 5;
    const std::vector<Amcl::SearchHit> coarse = filter.global_search(scan, search);
    if (coarse.empty() || coarse.size() > 5) return 2;
    std::vector<SE2d> seeds;
    for (const Amcl::SearchHit& h : coarse) seeds.push_back(h.pose);
    const Amcl::LocalSearchParams refine;  // the defaults
    const std::vector<Amcl::LocalHit> hits = filter.local_search(seeds, scan, refine);
    if (hits.size() != seeds.size()) return 2;
    for (const Amcl::LocalHit& h : hits) {
      print_hit("hit", h);
      if (h.score < h.seed_score || !h.moments_valid) return 2;
    }
    std::printf("candidates_per_seed %llu step_xy %.17g\n", static_cast<unsigned long long>(filter.last_local_search_info().candidates_per_seed),
                filter.last_local_search_info().step_xy);
    const std::vector<Amcl::LocalHit> refined = filter.relocalize(scan, search, refine);
    for (const Amcl::LocalHit& h : refined) print_hit("refined", h);
    for (std::size_t i = 1; i < refined.size(); ++i)
      if (refined[i].score > refined[i - 1].score) return 2;
    const auto estimate = filter.update(SE2d{}, Amcl::measurement_type{scan});
    if (!estimate) return 2;
    std::printf("estimate %.17g %.17g %.17g\n", estimate->first.x, estimate->first.y, estimate->first.angle());
    // the ROS facade over its own scan type: the sensor 0.25 m ahead of the base, the points given in the sensor's frame
    using RosAmcl = ros::Amcl<Grid>;
    const Grid grid{cells, W, H, 0.1, Origin2{{1.0, 0.0, -1.0, -1.0}}};
    Scan laser{{}, Origin3{{0.0, 0.0, 0.0, 1.0, 0.25, 0.0, 0.0}}};
    for (const auto& p : scan) laser.points.push_back(Point2{p.first - 0.25, p.second});
    RosAmcl node_filter{grid, models::DifferentialDriveModel{DifferentialDriveModelParam{0.1, 0.05, 0.1, 0.05}}, models::LikelihoodFieldModel<Grid>{lf, grid},
                        params};
    const std::vector<RosAmcl::LocalHit> ros_hits = node_filter.local_search(seeds, laser, refine);
    for (const RosAmcl::LocalHit& h : ros_hits) print_hit("ros_hit", h);
    if (ros_hits.size() != hits.size()) return 2;
    if (node_filter.relocalize(laser, search, refine).size() != refined.size()) return 2;
  } catch (const std::runtime_error& e) {
    std::printf("runtime_error: %s\n", e.what());
    return 3;
  }
  return 0;
}
