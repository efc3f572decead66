// search_demo.cpp - the global pose search through the header-only facades on a small asymmetric map: beluga_amd::Amcl::global_search and
// relocalize with points in the base frame, then beluga_amd::ros::Amcl::global_search with a laser scan whose sensor sits 0.25 m ahead
// of the base (the same points, so the same hits).  Prints "hit <cell> <heading> <score> <x> <y> <theta>" per hit of the plain facade,
// best first, "estimate x y theta" after relocalize and one update, and "ros_hit ..." per hit of the ROS facade.  Exit code 3: no
// usable GPU (no CPU fallback).
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
}  // namespace

int main() {
  using namespace beluga_amd;
  // 64 x 48 cells of 0.1 m inside a border, a wall along x at row 30 with a door, one along y at column 40: no symmetry.
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
  // what a robot at cell (10, 10), heading 0, sees of the walls around it, in its own frame
  const Amcl::measurement_type scan{{3.0, 0.0}, {0.0, 2.0}, {-1.0, 0.0}, {0.0, -1.0}, {3.0, 1.0}, {3.0, -1.0}, {1.0, 2.0}, {-1.0, 1.0}};
  try {
    Amcl filter{map, DifferentialDriveModelParam{0.1, 0.05, 0.1, 0.05}, lf, params, /*seed=*/5};
    Amcl::SearchParams search;
    search.headings = 36;
    search.max_results = 5;
    const std::vector<Amcl::SearchHit> hits = filter.global_search(scan, search);
    for (const Amcl::SearchHit& h : hits)
      std::printf("hit %u %u %.17g %.17g %.17g %.17g\n", h.cell, h.heading, h.score, h.pose.x, h.pose.y, h.pose.angle());
    std::printf("candidates %llu\n", static_cast<unsigned long long>(filter.last_search_info().candidates));
    if (hits.empty() || hits.size() > 5) return 2;
    for (std::size_t i = 1; i < hits.size(); ++i)
      if (hits[i].score > hits[i - 1].score) return 2;
    filter.relocalize(scan, search, Matrix3d{0.01, 0, 0, 0, 0.01, 0, 0, 0, 0.0025});
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
    const std::vector<RosAmcl::SearchHit> ros_hits = node_filter.global_search(laser, search);
    for (const RosAmcl::SearchHit& h : ros_hits)
      std::printf("ros_hit %u %u %.17g %.17g %.17g %.17g\n", h.cell, h.heading, h.score, h.pose.x, h.pose.y, h.pose.angle());
    if (ros_hits.size() != hits.size()) return 2;
  } catch (const std::runtime_error& e) {
    std::printf("runtime_error: %s\n", e.what());
    return 3;
  }
  return 0;
}
