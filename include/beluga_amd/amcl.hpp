// beluga_amd/amcl.hpp — header-only C++17 facade over the C ABI (include/beluga_mcl.h).
//
// Same public surface as `beluga::Amcl` (beluga/include/beluga/algorithm/amcl_core.hpp:81-233) for the
// SE(2) / DifferentialDriveModel / LikelihoodFieldModel|BeamSensorModel instantiation that
// `beluga_ros::Amcl` uses (beluga_ros/include/beluga_ros/amcl.hpp:102-282):
//   ctor(map, motion params, sensor params, AmclParams) ; particles() ; initialize(pose, covariance) ;
//   initialize(states) ; update_map(map) ; update(control_action, measurement) -> optional<pair<pose, cov>> ;
//   force_update() ; likelihood_field().
// Error behaviour follows the reference: `initialize` throws std::runtime_error on an invalid covariance
// (random/multivariate_normal_distribution.hpp:114-124), `update` returns std::nullopt when no update ran
// (amcl_core.hpp:166-172).  Any other failure of the device library throws std::runtime_error with its text.
//
// The reference's value types are Sophus::SE2d / Eigen::Matrix3d; neither library is required here.  `SE2d`
// below has Sophus' memory layout (cos, sin, x, y) and, when <sophus/se2.hpp> is available, converts both ways.
#ifndef BELUGA_AMD_AMCL_HPP
#define BELUGA_AMD_AMCL_HPP

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <execution>
#include <iterator>
#include <optional>
#include <random>
#include <stdexcept>
#include <string>
#include <tuple>
#include <type_traits>
#include <utility>
#include <variant>
#include <vector>

#include "beluga_mcl.h"

#if defined(__has_include)
#if __has_include(<sophus/se2.hpp>)
#include <sophus/se2.hpp>
#define BELUGA_AMD_HAS_SOPHUS 1
#endif
#endif

namespace beluga_amd {

/// SE(2) pose with Sophus::SE2d's data() layout: unit complex (cos, sin) then translation (x, y).
struct SE2d {
  double c{1.0}, s{0.0}, x{0.0}, y{0.0};
  SE2d() = default;
  SE2d(double theta, double tx, double ty) : c(std::cos(theta)), s(std::sin(theta)), x(tx), y(ty) {}
  /// From any SE(2) type with Sophus::SE2d's interface (so2() + data() = cos, sin, x, y).
  template <class T, class = decltype(std::declval<const T&>().so2()), class = decltype(std::declval<const T&>().data())>
  SE2d(const T& other) : c(other.data()[0]), s(other.data()[1]), x(other.data()[2]), y(other.data()[3]) {}  // NOLINT
  [[nodiscard]] double angle() const { return std::atan2(s, c); }
  [[nodiscard]] const double* data() const { return &c; }
  [[nodiscard]] double* data() { return &c; }
#ifdef BELUGA_AMD_HAS_SOPHUS
  operator Sophus::SE2d() const {                                                                    // NOLINT
    Sophus::SE2d out;
    out.so2().data()[0] = c;
    out.so2().data()[1] = s;
    out.translation() = Eigen::Vector2d{x, y};
    return out;
  }
#endif
};
static_assert(sizeof(SE2d) == 4 * sizeof(double), "SE2d must be four packed doubles");

using Matrix3d = std::array<double, 9>;  ///< row-major 3x3

/// beluga::AmclParams (amcl_core.hpp:34-55) + the spatial hash resolutions of beluga_ros::AmclParams.
struct AmclParams {
  double update_min_d = 0.25;
  double update_min_a = 0.2;
  std::size_t resample_interval = 1UL;
  bool selective_resampling = false;
  std::size_t min_particles = 500UL;
  std::size_t max_particles = 2000UL;
  double alpha_slow = 0.001;
  double alpha_fast = 0.1;
  double kld_epsilon = 0.05;
  double kld_z = 3.0;
  double spatial_resolution_x = 0.5;
  double spatial_resolution_y = 0.5;
  double spatial_resolution_theta = 10.0 * 3.14159265358979323846 / 180.0;
};

/// beluga::DifferentialDriveModelParam (motion/differential_drive_model.hpp:40-68).
struct DifferentialDriveModelParam {
  double rotation_noise_from_rotation;
  double rotation_noise_from_translation;
  double translation_noise_from_translation;
  double translation_noise_from_rotation;
  double distance_threshold = 0.01;
};

/// beluga::OmnidirectionalDriveModelParam (motion/omnidirectional_drive_model.hpp:36-73).
struct OmnidirectionalDriveModelParam {
  double rotation_noise_from_rotation;
  double rotation_noise_from_translation;
  double translation_noise_from_translation;
  double translation_noise_from_rotation;
  double strafe_noise_from_translation;
  double distance_threshold = 0.01;
};

/// beluga::StationaryModel (motion/stationary_model.hpp:40-62) has no parameters.
struct StationaryModelParam {};

using MotionModelParam = std::variant<DifferentialDriveModelParam, OmnidirectionalDriveModelParam, StationaryModelParam>;

/// beluga::LikelihoodFieldModelParam (sensor/likelihood_field_model_base.hpp:42-64).
struct LikelihoodFieldModelParam {
  double max_obstacle_distance = 100.0;
  double max_laser_distance = 2.0;
  double z_hit = 0.5;
  double z_random = 0.5;
  double sigma_hit = 0.2;
  bool model_unknown_space = false;
  bool only_obstacle_boundaries = false;
};

/// beluga::BeamModelParam (sensor/beam_model.hpp:43-58).
struct BeamModelParam {
  double z_hit{0.5};
  double z_short{0.5};
  double z_max{0.05};
  double z_rand{0.05};
  double sigma_hit{0.2};
  double lambda_short{0.1};
  double beam_max_range{60};
};

/// beluga::LikelihoodFieldProbModelParam (sensor/likelihood_field_prob_model.hpp:34): same fields, other weighting.
struct LikelihoodFieldProbModelParam : LikelihoodFieldModelParam {};

/// beluga::NDTModelParam2d (sensor/ndt_sensor_model.hpp:153-166): the reference's defaults; ndt_amcl_node's are 0.01 / 1.0 / 0.6.
struct NDTModelParam2d {
  double minimum_likelihood = 0.0;
  double d1 = 1.0;
  double d2 = 1.0;
  std::vector<std::array<int, 2>> neighbors_kernel = {{-1, -1}, {-1, 0}, {-1, 1}, {0, -1}, {0, 0}, {0, 1}, {1, -1}, {1, 0}, {1, 1}};
};

using SensorModelParam = std::variant<LikelihoodFieldModelParam, BeamModelParam, LikelihoodFieldProbModelParam, NDTModelParam2d>;

/// One NDTCell2d (sensor/data/ndt_cell.hpp): mean and 2 x 2 covariance (row-major).
struct NDTCell2d {
  std::array<double, 2> mean{};
  std::array<double, 4> covariance{};
};

/// beluga::LandmarkModelParam (sensor/landmark_sensor_model.hpp:44-48).
struct LandmarkModelParam {
  double sigma_range = 1.0;
  double sigma_bearing = 1.0;
  double random_prob = 1e-4;
};
/// beluga::BearingModelParam (sensor/bearing_sensor_model.hpp:42-45); the pose in Sophus::SE3d::data() order: quaternion x, y, z, w,
/// translation x, y, z.
struct BearingModelParam {
  double sigma_bearing = 1.0;
  std::array<double, 7> sensor_pose_in_robot{0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0};
};
/// types/landmark_detection_types.hpp:32-48, with plain arrays in the place of Eigen's vectors.
using LandmarkCategory = std::uint32_t;
using LandmarkPosition3 = std::array<double, 3>;
using LandmarkBearing3 = std::array<double, 3>;
struct LandmarkPositionDetection {
  LandmarkPosition3 detection_position_in_robot;
  LandmarkCategory category;
};
struct LandmarkBearingDetection {
  LandmarkBearing3 detection_bearing_in_sensor;
  LandmarkCategory category;
};
/// Eigen::AlignedBox3d's two corners.
struct LandmarkMapBoundaries {
  std::array<double, 3> min_corner{0.0, 0.0, 0.0}, max_corner{0.0, 0.0, 0.0};
  [[nodiscard]] const std::array<double, 3>& min() const { return min_corner; }
  [[nodiscard]] const std::array<double, 3>& max() const { return max_corner; }
};
/// beluga::LandmarkMap (sensor/data/landmark_map.hpp:40-75): both constructors and map_limits().  Built from the landmarks alone, its
/// limits are their bounding box; an empty map built that way has no limits and is refused by the filter.
class LandmarkMap {
 public:
  using landmarks_set_position_data = std::vector<LandmarkPositionDetection>;
  LandmarkMap(const LandmarkMapBoundaries& boundaries, landmarks_set_position_data landmarks)
      : landmarks_(std::move(landmarks)), boundaries_(boundaries), has_boundaries_(true) {}
  explicit LandmarkMap(landmarks_set_position_data landmarks) : landmarks_(std::move(landmarks)) {
    if (landmarks_.empty()) return;
    has_boundaries_ = true;
    boundaries_.min_corner = boundaries_.max_corner = landmarks_[0].detection_position_in_robot;
    for (const auto& l : landmarks_)
      for (std::size_t k = 0; k < 3; ++k) {
        boundaries_.min_corner[k] = std::min(boundaries_.min_corner[k], l.detection_position_in_robot[k]);
        boundaries_.max_corner[k] = std::max(boundaries_.max_corner[k], l.detection_position_in_robot[k]);
      }
  }
  [[nodiscard]] LandmarkMapBoundaries map_limits() const { return boundaries_; }
  [[nodiscard]] bool has_limits() const { return has_boundaries_; }
  [[nodiscard]] const landmarks_set_position_data& landmarks() const { return landmarks_; }

 private:
  landmarks_set_position_data landmarks_;
  LandmarkMapBoundaries boundaries_{};
  bool has_boundaries_{false};
};

/// The NDT sensor model's map with the accessors of beluga::SparseValueGrid2 (sensor/data/sparse_value_grid.hpp) that code written
/// against it reads: resolution(), size(), data_at(key) (std::nullopt where no cell is present), cell_near(point).  The cells are
/// kept in the load_from_hdf5 layout, which is what the device map is built from.
class NDTMap2d {
 public:
  using key_type = std::array<int, 2>;
  NDTMap2d() = default;
  NDTMap2d(std::vector<key_type> cells, std::vector<NDTCell2d> data, double resolution)
      : cells_(std::move(cells)), data_(std::move(data)), resolution_(resolution) {
    if (cells_.size() != data_.size()) throw std::invalid_argument("NDTMap2d: keys and cells differ in number");
  }
  [[nodiscard]] double resolution() const { return resolution_; }
  [[nodiscard]] std::size_t size() const { return cells_.size(); }
  [[nodiscard]] const std::vector<key_type>& keys() const { return cells_; }
  [[nodiscard]] const std::vector<NDTCell2d>& cells() const { return data_; }
  [[nodiscard]] std::optional<NDTCell2d> data_at(const key_type& key) const {
    for (std::size_t i = 0; i < cells_.size(); ++i)
      if (cells_[i] == key) return data_[i];
    return std::nullopt;
  }
  [[nodiscard]] key_type cell_near(double x, double y) const {  // regular_grid.hpp:75-78
    const double inv = 1. / resolution_;
    return {static_cast<int>(std::floor(x * inv)), static_cast<int>(std::floor(y * inv))};
  }
  /// The map of a point cloud (world frame) by the rule of detail::to_cells (ndt_sensor_model.hpp:88-110), on the host: keys by
  /// (p / resolution) truncated toward zero, cells of 5 points or more, in ascending key order (mcl_ndt_measurement_cells).
  /// Amcl::build_ndt_map builds the same cells on the device.
  static NDTMap2d from_points(const std::vector<std::pair<double, double>>& points, double resolution) {
    std::vector<double> xy;
    xy.reserve(2 * points.size());
    std::vector<std::pair<key_type, std::size_t>> counts;  // ascending keys
    for (const auto& p : points) {
      xy.push_back(p.first);
      xy.push_back(p.second);
      const double qx = p.first / resolution, qy = p.second / resolution;
      if (!(std::abs(qx) < 2147483647.0 && std::abs(qy) < 2147483647.0)) continue;
      counts.push_back({key_type{static_cast<int>(qx), static_cast<int>(qy)}, 1});
    }
    std::sort(counts.begin(), counts.end());
    std::vector<key_type> keys;
    for (std::size_t a = 0; a < counts.size();) {
      std::size_t b = a;
      while (b < counts.size() && counts[b].first == counts[a].first) ++b;
      if (b - a >= 5) keys.push_back(counts[a].first);
      a = b;
    }
    std::vector<double> means(2 * (points.size() / 5 + 1)), covs(4 * (points.size() / 5 + 1));
    std::uint64_t k = 0;
    if (mcl_ndt_measurement_cells(xy.data(), points.size(), resolution, means.data(), covs.data(), &k) != MCL_OK || k != keys.size())
      throw std::invalid_argument("NDTMap2d::from_points: the resolution must be positive and finite");
    std::vector<NDTCell2d> data(k);
    for (std::size_t j = 0; j < k; ++j) data[j] = NDTCell2d{{means[2 * j], means[2 * j + 1]}, {covs[4 * j], covs[4 * j + 1], covs[4 * j + 2], covs[4 * j + 3]}};
    return NDTMap2d{std::move(keys), std::move(data), resolution};
  }
  /// The same from the centres of a grid's occupied cells, row-major, origin * (resolution * (index + 0.5)); `Grid` is an
  /// OccupancyGridView.
  template <class Grid>
  static NDTMap2d from_occupancy_grid(const Grid& grid, double resolution) {
    std::vector<std::pair<double, double>> points;
    const double* o = grid.origin.data();
    for (std::uint32_t yi = 0; yi < grid.height; ++yi)
      for (std::uint32_t xi = 0; xi < grid.width; ++xi) {
        if (grid.cells[static_cast<std::size_t>(yi) * grid.width + xi] != grid.occupied_value) continue;
        const double lx = (static_cast<double>(xi) + 0.5) * grid.resolution, ly = (static_cast<double>(yi) + 0.5) * grid.resolution;
        points.emplace_back((o[0] * lx - o[1] * ly) + o[2], (o[1] * lx + o[0] * ly) + o[3]);
      }
    return from_points(points, resolution);
  }

 private:
  std::vector<key_type> cells_;
  std::vector<NDTCell2d> data_;
  double resolution_{1.0};
};

/// A non-owning view of anything satisfying OccupancyGrid2 (sensor/data/occupancy_grid.hpp:39-75).
struct OccupancyGridView {
  const std::int8_t* cells{nullptr};  ///< row-major, height x width
  std::uint32_t width{0}, height{0};
  double resolution{0.0};
  SE2d origin{};
  std::int8_t free_value{0}, unknown_value{-1}, occupied_value{100};  ///< beluga_ros::OccupancyGrid::ValueTraits

  /// Adapts a grid type with width()/height()/resolution()/origin()/data() whose cell type is int8.  The value traits are
  /// the grid's own (`Grid::ValueTraits::kFreeValue / kUnknownValue / kOccupiedValue`, beluga_ros/occupancy_grid.hpp:48-64)
  /// when it declares them, the ROS trinary interpretation 0 / -1 / 100 otherwise.
  template <class Grid>
  static OccupancyGridView from(const Grid& grid) {
    OccupancyGridView v;
    v.cells = reinterpret_cast<const std::int8_t*>(&*std::begin(grid.data()));
    v.width = static_cast<std::uint32_t>(grid.width());
    v.height = static_cast<std::uint32_t>(grid.height());
    v.resolution = grid.resolution();
    v.origin = SE2d{grid.origin()};
    read_traits<Grid>(v, 0);
    return v;
  }

 private:
  template <class Grid>
  static auto read_traits(OccupancyGridView& v, int) -> decltype(Grid::ValueTraits::kFreeValue, void()) {
    v.free_value = static_cast<std::int8_t>(Grid::ValueTraits::kFreeValue);
    v.unknown_value = static_cast<std::int8_t>(Grid::ValueTraits::kUnknownValue);
    v.occupied_value = static_cast<std::int8_t>(Grid::ValueTraits::kOccupiedValue);
  }
  template <class Grid>
  static void read_traits(OccupancyGridView&, long) {}
};

/// What beluga_ros::LaserScan wraps (beluga_ros/include/beluga_ros/laser_scan.hpp:46-66): the sensor_msgs/LaserScan
/// fields, the laser origin in the base frame and the decimation / range limits.
struct LaserScan {
  std::vector<float> ranges;
  float angle_min{0.F}, angle_increment{0.F};
  float range_min{0.F}, range_max{0.F};
  std::array<double, 7> origin{0, 0, 0, 1, 0, 0, 0};  ///< Sophus::SE3d::data(): qx qy qz qw tx ty tz
  std::size_t max_beams{static_cast<std::size_t>(-1)};
  double min_range{2.2250738585072014e-308};
  double max_range{1.7976931348623157e308};
};

/// Host mirror of the particle set: what `beluga::TupleVector<std::tuple<SE2d, Weight>>` holds.  A sized random-access range
/// of (state, weight) tuples — `std::get<0>(p)` / `std::get<1>(p)` are what `beluga::state(p)` / `beluga::weight(p)` read
/// (type_traits/particle_traits.hpp) — plus the two component ranges `beluga::views::states / weights` project.
struct ParticleSet {
  using value_type = std::tuple<SE2d, double>;
  using reference = std::tuple<const SE2d&, const double&>;
  std::vector<SE2d> states;
  std::vector<double> weights;

  class const_iterator {
   public:
    using iterator_category = std::random_access_iterator_tag;
    using value_type = ParticleSet::value_type;
    using difference_type = std::ptrdiff_t;
    using pointer = void;
    using reference = ParticleSet::reference;
    const_iterator() = default;
    const_iterator(const ParticleSet* set, std::size_t index) : set_(set), index_(index) {}
    reference operator*() const { return reference{set_->states[index_], set_->weights[index_]}; }
    reference operator[](difference_type k) const { return *(*this + k); }
    const_iterator& operator++() { ++index_; return *this; }
    const_iterator operator++(int) { auto old = *this; ++index_; return old; }
    const_iterator& operator--() { --index_; return *this; }
    const_iterator operator--(int) { auto old = *this; --index_; return old; }
    const_iterator& operator+=(difference_type k) { index_ = static_cast<std::size_t>(static_cast<difference_type>(index_) + k); return *this; }
    const_iterator& operator-=(difference_type k) { return *this += -k; }
    friend const_iterator operator+(const_iterator it, difference_type k) { return it += k; }
    friend const_iterator operator+(difference_type k, const_iterator it) { return it += k; }
    friend const_iterator operator-(const_iterator it, difference_type k) { return it -= k; }
    friend difference_type operator-(const const_iterator& a, const const_iterator& b) {
      return static_cast<difference_type>(a.index_) - static_cast<difference_type>(b.index_);
    }
    friend bool operator==(const const_iterator& a, const const_iterator& b) { return a.index_ == b.index_; }
    friend bool operator!=(const const_iterator& a, const const_iterator& b) { return a.index_ != b.index_; }
    friend bool operator<(const const_iterator& a, const const_iterator& b) { return a.index_ < b.index_; }
    friend bool operator>(const const_iterator& a, const const_iterator& b) { return a.index_ > b.index_; }
    friend bool operator<=(const const_iterator& a, const const_iterator& b) { return a.index_ <= b.index_; }
    friend bool operator>=(const const_iterator& a, const const_iterator& b) { return a.index_ >= b.index_; }

   private:
    const ParticleSet* set_{nullptr};
    std::size_t index_{0};
  };
  using iterator = const_iterator;

  [[nodiscard]] std::size_t size() const { return weights.size(); }
  [[nodiscard]] bool empty() const { return weights.empty(); }
  [[nodiscard]] const_iterator begin() const { return {this, 0}; }
  [[nodiscard]] const_iterator end() const { return {this, size()}; }
  [[nodiscard]] reference operator[](std::size_t i) const { return reference{states[i], weights[i]}; }
};

/// `beluga::views::states(particles)` / `beluga::views::weights(particles)` for the host mirror (views/particles.hpp).
namespace views {
inline const std::vector<SE2d>& states(const ParticleSet& particles) { return particles.states; }
inline const std::vector<double>& weights(const ParticleSet& particles) { return particles.weights; }
}  // namespace views

/// What `likelihood_field()` returns: the accessors of `beluga::ValueGrid2<float>` (sensor/data/value_grid.hpp:36-69) that
/// `beluga_ros::assign_likelihood_field` reads (beluga_ros/include/beluga_ros/likelihood_field.hpp:31-66).
template <class T>
class ValueGrid2 {
 public:
  ValueGrid2() = default;
  ValueGrid2(std::vector<T> data, std::size_t width, double resolution) : data_(std::move(data)), width_(width), resolution_(resolution) {}
  [[nodiscard]] std::size_t size() const { return data_.size(); }
  [[nodiscard]] const std::vector<T>& data() const { return data_; }
  [[nodiscard]] std::size_t width() const { return width_; }
  [[nodiscard]] std::size_t height() const { return width_ ? data_.size() / width_ : 0; }
  [[nodiscard]] double resolution() const { return resolution_; }
  [[nodiscard]] const T& operator[](std::size_t i) const { return data_[i]; }

 private:
  std::vector<T> data_;
  std::size_t width_{0};
  double resolution_{1.0};
};

/// A contiguous shard of one logical filter's particles (include/beluga_mcl.h, "Particle shards"): one `Amcl` per GPU, every
/// instance with its shard, the same map, control actions and scans; after `attach` / `attach_rccl`, `update()` runs the cycle
/// over all shards (fixed-size and KLD-adaptive) and every instance returns the same estimate.  `particles()` is the shard.
struct Shard {
  std::uint64_t offset{0};    ///< global index of the shard's first particle
  std::uint64_t capacity{0};  ///< particles the shard can hold (its share of max_particles); 0: not sharded
  /// The balanced split the library itself uses when it re-balances: rank `rank` of `world`.
  static Shard of(std::uint64_t max_particles, unsigned rank, unsigned world) {
    const std::uint64_t base = max_particles / world, rem = max_particles % world;
    return Shard{rank * base + (rank < rem ? rank : rem), base + (rank < rem ? 1u : 0u)};
  }
};

/// beluga::ParticleClusterizerParam (algorithm/cluster_based_estimation.hpp:243-259).
struct ParticleClusterizerParam {
  double linear_hash_resolution = 0.20;    ///< cell size of the clustering's spatial hash, metres
  double angular_hash_resolution = 0.524;  ///< ... and radians
  double weight_cap_percentile = 0.90;     ///< the cells' mean weights are capped at this percentile of theirs
};

/// One entry of beluga::estimate_clusters' result (:356-360: weight, mean, covariance) and, beside the reference's fields, the cluster's id
/// (what cluster_labels() gives its particles) and its number of particles.
struct ClusterEstimate {
  double weight{0};
  SE2d mean;
  Matrix3d covariance{};
  std::uint32_t id{0};
  std::uint64_t count{0};
};

class AmclBatch;

/// One map on the device for any number of filters (mcl_shared_map_*): built once - for the device and the sensor model given, which
/// every filter that uses it must share (the likelihood-field models: the same model and equal parameters) - and never changed.
/// Amcl::use_map / AmclBatch::use_map attach filters to it; the object holds the caller's reference only and may go out of scope while
/// filters still use the map, which lives until the last of them has left it.  The constructor touches no filter: it may run on another
/// thread while filters update.
class SharedMap {
 public:
  /// `device_field_build`: the likelihood field by the device's exact distance transform instead of the reference's wavefront on the host.
  inline SharedMap(const OccupancyGridView& map, const SensorModelParam& sensor, int device = 0, bool device_field_build = false);
  SharedMap(const SharedMap&) = delete;
  SharedMap& operator=(const SharedMap&) = delete;
  SharedMap(SharedMap&& other) noexcept : map_(other.map_) { other.map_ = nullptr; }
  SharedMap& operator=(SharedMap&& other) noexcept {
    if (this != &other) {
      mcl_shared_map_release(map_);
      map_ = other.map_;
      other.map_ = nullptr;
    }
    return *this;
  }
  ~SharedMap() { mcl_shared_map_release(map_); }
  /// Size, sensor kind, device, the bytes the map holds and the filters attached now.
  [[nodiscard]] mcl_shared_map_info info() const {
    mcl_shared_map_info out{};
    if (mcl_shared_map_get_info(map_, &out) != MCL_OK) throw std::runtime_error("beluga_amd::SharedMap: no map (moved from)");
    return out;
  }
  [[nodiscard]] mcl_shared_map* native_handle() const { return map_; }

 private:
  mcl_shared_map* map_{nullptr};
};

class Amcl {
 public:
  using state_type = SE2d;
  using measurement_type = std::vector<std::pair<double, double>>;
  using estimation_type = std::pair<SE2d, Matrix3d>;

  /// `options`: library switches applied before the map is installed (mcl_set_option), e.g. {{"field_build", 1}} to build
  /// the likelihood field with the device's exact distance transform instead of the reference's wavefront on the host.
  Amcl(const OccupancyGridView& map, const MotionModelParam& motion, const SensorModelParam& sensor,
       const AmclParams& params = AmclParams{}, std::uint64_t seed = 0, int device = 0,
       const std::vector<std::pair<std::string, std::int64_t>>& options = {}, const Shard& shard = Shard{}) {
    if (std::holds_alternative<NDTModelParam2d>(sensor)) throw std::invalid_argument("beluga_amd::Amcl: the NDT sensor model takes an NDTMap2d");
    create(make_config(motion, sensor, params, seed, device, shard), params, options);
    try {
      update_map(map);
    } catch (...) {
      mcl_destroy(ctx_);
      ctx_ = nullptr;
      throw;
    }
  }
  /// The filter of ndt_amcl_node (beluga_amcl/include/beluga_amcl/ndt_amcl_node.hpp:77-84): beluga::Amcl with the NDT sensor model.
  /// Code written for `NdtAmcl<Motion, Policy>` switches by a type alias: construction from (map, motion, NDTModelParam2d, params).
  /// `ndt_map_layout`: set_ndt_map_layout before `map` is installed (0 dense, 1 hashed where the dense grid does not fit, 2 hashed).
  Amcl(const NDTMap2d& map, const MotionModelParam& motion, const NDTModelParam2d& sensor, const AmclParams& params = AmclParams{},
       std::uint64_t seed = 0, int device = 0, const std::vector<std::pair<std::string, std::int64_t>>& options = {},
       std::int32_t ndt_map_layout = 0)
      : ndt_params_(sensor) {
    create(make_config(motion, SensorModelParam{sensor}, params, seed, device, Shard{}), params, options);
    try {
      if (ndt_map_layout != 0) set_ndt_map_layout(ndt_map_layout);
      update_map(map);
    } catch (...) {
      mcl_destroy(ctx_);
      ctx_ = nullptr;
      throw;
    }
  }
  /// beluga::Amcl with LandmarkSensorModel2d<LandmarkMap> / BearingSensorModel2d<LandmarkMap> (the reference has no node for them).
  Amcl(const LandmarkMap& map, const MotionModelParam& motion, const LandmarkModelParam& sensor, const AmclParams& params = AmclParams{},
       std::uint64_t seed = 0, int device = 0, const std::vector<std::pair<std::string, std::int64_t>>& options = {})
      : landmark_params_(sensor) {
    create_landmark(MCL_SENSOR_LANDMARK, map, motion, params, seed, device, options);
  }
  Amcl(const LandmarkMap& map, const MotionModelParam& motion, const BearingModelParam& sensor, const AmclParams& params = AmclParams{},
       std::uint64_t seed = 0, int device = 0, const std::vector<std::pair<std::string, std::int64_t>>& options = {})
      : bearing_params_(sensor) {
    create_landmark(MCL_SENSOR_BEARING, map, motion, params, seed, device, options);
  }

 private:
  void create_landmark(int kind, const LandmarkMap& map, const MotionModelParam& motion, const AmclParams& params, std::uint64_t seed, int device,
                       const std::vector<std::pair<std::string, std::int64_t>>& options) {
    mcl_config cfg = base_config(motion, params, seed, device, Shard{});
    cfg.sensor_kind = kind;  // (its parameters travel with the map: mcl_set_landmark_map)
    landmark_kind_ = kind;
    create(cfg, params, options);
    try {
      update_map(map);
    } catch (...) {
      mcl_destroy(ctx_);
      ctx_ = nullptr;
      throw;
    }
  }
  template <class Detection, class Get>
  static void flatten(const std::vector<Detection>& detections, Get get, std::vector<double>& xyz, std::vector<std::uint32_t>& categories) {
    xyz.clear();
    categories.clear();
    for (const auto& d : detections) {
      const std::array<double, 3>& v = get(d);
      xyz.insert(xyz.end(), v.begin(), v.end());
      categories.push_back(d.category);
    }
  }
  auto finish_update(const mcl_estimate& est, const mcl_update_info& info) -> std::optional<std::pair<SE2d, Matrix3d>> {
    last_info_ = info;
    if (!info.updated) return std::nullopt;
    dirty_ = true;
    std::pair<SE2d, Matrix3d> out;
    out.first.c = est.pose[0];
    out.first.s = est.pose[1];
    out.first.x = est.pose[2];
    out.first.y = est.pose[3];
    for (int i = 0; i < 9; ++i) out.second[static_cast<std::size_t>(i)] = est.covariance[i];
    return out;
  }
  /// Everything of the configuration but the sensor model.
  static mcl_config base_config(const MotionModelParam& motion, const AmclParams& params, std::uint64_t seed, int device, const Shard& shard) {
    mcl_config cfg;
    mcl_default_config(&cfg);
    cfg.device_id = device;
    cfg.seed = seed;
    cfg.shard_offset = shard.offset;
    cfg.shard_capacity = shard.capacity;
    cfg.amcl.update_min_d = params.update_min_d;
    cfg.amcl.update_min_a = params.update_min_a;
    cfg.amcl.resample_interval = params.resample_interval;
    cfg.amcl.selective_resampling = params.selective_resampling ? 1 : 0;
    cfg.amcl.min_particles = params.min_particles;
    cfg.amcl.max_particles = params.max_particles;
    cfg.amcl.alpha_slow = params.alpha_slow;
    cfg.amcl.alpha_fast = params.alpha_fast;
    cfg.amcl.kld_epsilon = params.kld_epsilon;
    cfg.amcl.kld_z = params.kld_z;
    cfg.amcl.spatial_resolution_x = params.spatial_resolution_x;
    cfg.amcl.spatial_resolution_y = params.spatial_resolution_y;
    cfg.amcl.spatial_resolution_theta = params.spatial_resolution_theta;
    if (const auto* dd = std::get_if<DifferentialDriveModelParam>(&motion)) {
      cfg.motion_kind = MCL_MOTION_DIFFERENTIAL;
      cfg.motion = mcl_diffdrive_params{dd->rotation_noise_from_rotation, dd->rotation_noise_from_translation,
                                        dd->translation_noise_from_translation, dd->translation_noise_from_rotation,
                                        dd->distance_threshold};
    } else if (const auto* om = std::get_if<OmnidirectionalDriveModelParam>(&motion)) {
      cfg.motion_kind = MCL_MOTION_OMNIDIRECTIONAL;
      cfg.motion = mcl_diffdrive_params{om->rotation_noise_from_rotation, om->rotation_noise_from_translation,
                                        om->translation_noise_from_translation, om->translation_noise_from_rotation,
                                        om->distance_threshold};
      cfg.strafe_noise_from_translation = om->strafe_noise_from_translation;
    } else {
      cfg.motion_kind = MCL_MOTION_STATIONARY;
    }
    return cfg;
  }
  static mcl_config make_config(const MotionModelParam& motion, const SensorModelParam& sensor, const AmclParams& params, std::uint64_t seed,
                                int device, const Shard& shard) {
    mcl_config cfg = base_config(motion, params, seed, device, shard);
    const LikelihoodFieldModelParam* lf = std::get_if<LikelihoodFieldModelParam>(&sensor);
    if (!lf) lf = std::get_if<LikelihoodFieldProbModelParam>(&sensor);
    if (lf) {
      cfg.sensor_kind = std::holds_alternative<LikelihoodFieldProbModelParam>(sensor) ? MCL_SENSOR_LIKELIHOOD_FIELD_PROB
                                                                                     : MCL_SENSOR_LIKELIHOOD_FIELD;
      cfg.lf = mcl_lf_params{lf->max_obstacle_distance, lf->max_laser_distance, lf->z_hit, lf->z_random, lf->sigma_hit,
                             lf->model_unknown_space ? 1 : 0, lf->only_obstacle_boundaries ? 1 : 0};
    } else if (const auto* b = std::get_if<BeamModelParam>(&sensor)) {
      cfg.sensor_kind = MCL_SENSOR_BEAM;
      cfg.beam = mcl_beam_params{b->z_hit, b->z_short, b->z_max, b->z_rand, b->sigma_hit, b->lambda_short, b->beam_max_range};
    } else {
      cfg.sensor_kind = MCL_SENSOR_NDT;
    }
    return cfg;
  }
  void create(const mcl_config& cfg, const AmclParams& params, const std::vector<std::pair<std::string, std::int64_t>>& options) {
    max_particles_ = params.max_particles;
    const mcl_status st = mcl_create(&cfg, &ctx_);
    if (st != MCL_OK) throw std::runtime_error(std::string("beluga_amd::Amcl: ") + mcl_last_error(nullptr));
    try {
      for (const auto& [name, value] : options) check(mcl_set_option(ctx_, name.c_str(), value));
    } catch (...) {
      mcl_destroy(ctx_);
      ctx_ = nullptr;
      throw;
    }
  }

 public:
  Amcl(const Amcl&) = delete;
  Amcl& operator=(const Amcl&) = delete;
  Amcl(Amcl&& other) noexcept
      : ctx_(other.ctx_),
        width_(other.width_),
        height_(other.height_),
        max_particles_(other.max_particles_),
        resolution_(other.resolution_),
        has_field_(other.has_field_),
        ndt_params_(std::move(other.ndt_params_)),
        ndt_resolution_(other.ndt_resolution_),
        landmark_params_(other.landmark_params_),
        bearing_params_(other.bearing_params_),
        landmark_kind_(other.landmark_kind_) {
    other.ctx_ = nullptr;
  }
  ~Amcl() { mcl_destroy(ctx_); }

  /// Returns a reference to the current set of particles (amcl_core.hpp:127). Downloaded lazily.
  [[nodiscard]] const ParticleSet& particles() const {
    if (dirty_) {
      std::uint64_t n = 0;
      check(mcl_num_particles(ctx_, &n));
      mirror_.states.resize(n);
      mirror_.weights.resize(n);
      if (n) check(mcl_get_particles(ctx_, mirror_.states.data()->data(), mirror_.weights.data(), n, &n));
      dirty_ = false;
    }
    return mirror_;
  }

  /// Initialize particles with a given pose and covariance (amcl_core.hpp:145-147).
  /// \throw std::runtime_error If the provided covariance is invalid.
  void initialize(const SE2d& pose, const Matrix3d& covariance) {
    const double mean[3] = {pose.x, pose.y, pose.angle()};
    const mcl_status st = mcl_initialize_normal(ctx_, mean, covariance.data());
    if (st == MCL_ERR_BAD_COVARIANCE) throw std::runtime_error("Invalid covariance matrix");
    check(st);
    dirty_ = true;
  }

  /// Initialize particles from caller-drawn states, weight 1 each (amcl_core.hpp:131-137).
  void initialize(const std::vector<SE2d>& states) {
    const std::vector<double> ones(states.size(), 1.0);
    check(mcl_set_particles(ctx_, states.empty() ? nullptr : states.data()->data(), ones.data(), states.size()));
    dirty_ = true;
  }

  /// Update the landmark map (LandmarkSensorModel::update_map, BearingSensorModel::update_map).
  void update_map(const LandmarkMap& map) {
    std::vector<double> xyz;
    std::vector<std::uint32_t> categories;
    flatten(map.landmarks(), [](const LandmarkPositionDetection& d) -> const std::array<double, 3>& { return d.detection_position_in_robot; }, xyz,
            categories);
    const LandmarkMapBoundaries limits = map.map_limits();
    const double box[6] = {limits.min_corner[0], limits.min_corner[1], limits.min_corner[2],
                           limits.max_corner[0], limits.max_corner[1], limits.max_corner[2]};
    const mcl_landmark_params lp{landmark_params_.sigma_range, landmark_params_.sigma_bearing, landmark_params_.random_prob};
    mcl_bearing_params bp{bearing_params_.sigma_bearing, {}};
    for (std::size_t k = 0; k < 7; ++k) bp.sensor_pose_in_robot[k] = bearing_params_.sensor_pose_in_robot[k];
    const void* prm = landmark_kind_ == MCL_SENSOR_BEARING ? static_cast<const void*>(&bp) : static_cast<const void*>(&lp);
    check(mcl_set_landmark_map(ctx_, xyz.data(), categories.data(), categories.size(), map.has_limits() ? box : nullptr, prm));
  }
  /// update(control_action, std::vector<LandmarkPositionDetection>): the landmark sensor model's measurement.
  auto update(const SE2d& control_action, const std::vector<LandmarkPositionDetection>& detections) -> std::optional<estimation_type> {
    std::vector<double> xyz;
    std::vector<std::uint32_t> categories;
    flatten(detections, [](const LandmarkPositionDetection& d) -> const std::array<double, 3>& { return d.detection_position_in_robot; }, xyz,
            categories);
    mcl_estimate est;
    mcl_update_info info;
    check(mcl_update_landmarks(ctx_, control_action.data(), xyz.data(), categories.data(), categories.size(), &est, &info));
    return finish_update(est, info);
  }
  /// update(control_action, std::vector<LandmarkBearingDetection>): the bearing sensor model's measurement.
  auto update(const SE2d& control_action, const std::vector<LandmarkBearingDetection>& detections) -> std::optional<estimation_type> {
    std::vector<double> xyz;
    std::vector<std::uint32_t> categories;
    flatten(detections, [](const LandmarkBearingDetection& d) -> const std::array<double, 3>& { return d.detection_bearing_in_sensor; }, xyz,
            categories);
    mcl_estimate est;
    mcl_update_info info;
    check(mcl_update_bearings(ctx_, control_action.data(), xyz.data(), categories.data(), categories.size(), &est, &info));
    return finish_update(est, info);
  }
  /// Extension: the global pose search (mcl_global_search): every free cell of the map whose x and y are multiples of cell_stride,
  /// at `headings` headings each, scored with the sensor model on the device as likelihoods() would score it; of the best `pool`
  /// those not within separation_xy (metres) and separation_theta (radians) of a better kept one, best first, at most max_results.
  /// The filter is untouched.  Likelihood-field and beam filters (throws on another); points in the base frame.  The separations are
  /// handed over as round(separation_xy / the map's resolution) cells and round(separation_theta / (2 pi / headings)) heading steps;
  /// the resolution is that of the map the filter holds (a map given by update_map_async counts from its swap on).
  /// \throw std::invalid_argument for a separation that is negative or not finite.
  struct SearchParams {
    std::uint32_t cell_stride = 2, headings = 72, pool = 1024, max_results = 16;
    double separation_xy = 0.5, separation_theta = 0.5235987755982988;  // 30 degrees
  };
  struct SearchHit {
    SE2d pose;
    double score = 0.0;
    std::uint64_t id = 0;
    std::uint32_t cell = 0, heading = 0;
  };
  [[nodiscard]] std::vector<SearchHit> global_search(const std::vector<std::pair<double, double>>& measurement, const SearchParams& search) {
    static_assert(sizeof(std::pair<double, double>) == 2 * sizeof(double), "points are handed over as (x, y) doubles");
    if (!(search.separation_xy >= 0.0 && std::isfinite(search.separation_xy) && search.separation_theta >= 0.0 && std::isfinite(search.separation_theta)))
      throw std::invalid_argument("global_search: a separation is negative or not finite");
    (void)map_pending();  // (a swap inside an update() may have changed the map, and with it the resolution)
    const double step = search.headings ? 2.0 * 3.14159265358979323846 / search.headings : 1.0;
    const auto steps_of = [](double separation, double unit) {  // beyond 2^32 - 1 units: everything is within reach anyway
      return unit > 0.0 ? static_cast<std::uint32_t>(std::min(std::round(separation / unit), 4294967295.0)) : 0u;
    };
    const mcl_search_params p{search.cell_stride, search.headings, search.pool, search.max_results, steps_of(search.separation_xy, resolution_),
                              steps_of(search.separation_theta, step)};
    std::vector<mcl_search_hit> raw(std::max<std::uint32_t>(p.max_results, 1));
    std::uint64_t count = 0;
    check(mcl_global_search(ctx_, measurement.empty() ? nullptr : &measurement.data()->first, measurement.size(), &p, raw.data(), raw.size(), &count,
                            &last_search_info_));
    std::vector<SearchHit> hits(count);
    for (std::uint64_t i = 0; i < count; ++i) {
      hits[i].pose.c = raw[i].pose[0], hits[i].pose.s = raw[i].pose[1], hits[i].pose.x = raw[i].pose[2], hits[i].pose.y = raw[i].pose[3];
      hits[i].score = raw[i].score, hits[i].id = raw[i].id, hits[i].cell = raw[i].cell, hits[i].heading = raw[i].heading;
    }
    return hits;
  }
  [[nodiscard]] std::vector<SearchHit> global_search(const std::vector<std::pair<double, double>>& measurement) {
    return global_search(measurement, SearchParams{});
  }
  /// The counts of the last global_search (mcl_search_info).
  [[nodiscard]] const mcl_search_info& last_search_info() const { return last_search_info_; }
  /// global_search, then initialize(best pose, covariance): host glue.  With no hit (a map without a candidate cell) the filter is
  /// left as it was.  Returns the hits.
  std::vector<SearchHit> relocalize(const std::vector<std::pair<double, double>>& measurement, const SearchParams& search, const Matrix3d& covariance) {
    std::vector<SearchHit> hits = global_search(measurement, search);
    if (!hits.empty()) initialize(hits.front().pose, covariance);
    return hits;
  }

  /// Extension: the local pose search (mcl_local_search): about each of `states` the lattice of (2 half_steps_xy + 1)^2
  /// (2 half_steps_theta + 1) poses at offsets of step_xy (0: a quarter of the map's cell size) in world x and y and of step_theta in
  /// heading is scored on the device as likelihoods() would score it.  Per state a LocalHit: the best lattice pose (ties go to the one
  /// nearest the state), its score, the state's own, and the score-weighted mean pose and covariance of the lattice.  The filter is
  /// untouched.  Every sensor model; the measurement as likelihoods() takes it.
  struct LocalSearchParams {
    std::uint32_t half_steps_xy = 4, half_steps_theta = 5;
    double step_xy = 0.0, step_theta = 3.14159265358979323846 / 360.0;
  };
  struct LocalHit {
    SE2d pose;
    double score = 0.0, seed_score = 0.0;
    std::int32_t di = 0, dj = 0, dk = 0;
    std::uint64_t plateau = 0;
    SE2d mean_pose;
    Matrix3d cov{};
    std::array<double, 10> sums{};
    bool moments_valid = false;
  };
  [[nodiscard]] std::vector<LocalHit> local_search(const std::vector<SE2d>& states, const std::vector<std::pair<double, double>>& measurement,
                                                   const LocalSearchParams& search) {
    static_assert(sizeof(std::pair<double, double>) == 2 * sizeof(double), "points are handed over as (x, y) doubles");
    const mcl_local_search_params p{search.half_steps_xy, search.half_steps_theta, search.step_xy, search.step_theta};
    std::vector<mcl_local_hit> raw(std::max<std::size_t>(states.size(), 1));
    check(mcl_local_search(ctx_, states.empty() ? nullptr : states.data()->data(), states.size(), measurement.empty() ? nullptr : &measurement.data()->first,
                           measurement.size(), &p, raw.data(), &last_local_search_info_));
    return local_hits(raw, states.size());
  }
  [[nodiscard]] std::vector<LocalHit> local_search(const std::vector<SE2d>& states, const std::vector<LandmarkPositionDetection>& detections,
                                                   const LocalSearchParams& search) {
    std::vector<double> xyz;
    std::vector<std::uint32_t> categories;
    flatten(detections, [](const LandmarkPositionDetection& d) -> const std::array<double, 3>& { return d.detection_position_in_robot; }, xyz,
            categories);
    const mcl_local_search_params p{search.half_steps_xy, search.half_steps_theta, search.step_xy, search.step_theta};
    std::vector<mcl_local_hit> raw(std::max<std::size_t>(states.size(), 1));
    check(mcl_local_search_landmarks(ctx_, states.empty() ? nullptr : states.data()->data(), states.size(), xyz.data(), categories.data(), categories.size(),
                                     &p, raw.data(), &last_local_search_info_));
    return local_hits(raw, states.size());
  }
  [[nodiscard]] std::vector<LocalHit> local_search(const std::vector<SE2d>& states, const std::vector<LandmarkBearingDetection>& detections,
                                                   const LocalSearchParams& search) {
    std::vector<double> xyz;
    std::vector<std::uint32_t> categories;
    flatten(detections, [](const LandmarkBearingDetection& d) -> const std::array<double, 3>& { return d.detection_bearing_in_sensor; }, xyz,
            categories);
    const mcl_local_search_params p{search.half_steps_xy, search.half_steps_theta, search.step_xy, search.step_theta};
    std::vector<mcl_local_hit> raw(std::max<std::size_t>(states.size(), 1));
    check(mcl_local_search_bearings(ctx_, states.empty() ? nullptr : states.data()->data(), states.size(), xyz.data(), categories.data(), categories.size(),
                                    &p, raw.data(), &last_local_search_info_));
    return local_hits(raw, states.size());
  }
  /// local_search with the default parameters, whatever the measurement's type.
  template <class Measurement>
  [[nodiscard]] std::vector<LocalHit> local_search(const std::vector<SE2d>& states, const Measurement& measurement) {
    return local_search(states, measurement, LocalSearchParams{});
  }
  /// The counts and the step of the last local_search (mcl_local_search_info).
  [[nodiscard]] const mcl_local_search_info& last_local_search_info() const { return last_local_search_info_; }
  /// relocalize with refinement: the kept hits of global_search are refined by local_search and ordered by their refined score (stable
  /// for ties); the filter is initialised at the best one's mean_pose with its cov + diag(step_xy^2, step_xy^2, step_theta^2) / 12 - the
  /// variance of a uniform error inside one lattice step, which keeps the matrix positive definite on a plateau or with no steps at all.
  /// Where the best hit's moments are not valid, `covariance` is used (and must be given).  Returns the refined hits.
  std::vector<LocalHit> relocalize(const std::vector<std::pair<double, double>>& measurement, const SearchParams& search, const LocalSearchParams& refine,
                                   const Matrix3d* covariance = nullptr) {
    const std::vector<SearchHit> hits = global_search(measurement, search);
    if (hits.empty()) return {};
    std::vector<SE2d> seeds;
    for (const SearchHit& h : hits) seeds.push_back(h.pose);
    std::vector<LocalHit> refined = local_search(seeds, measurement, refine);
    std::stable_sort(refined.begin(), refined.end(), [](const LocalHit& a, const LocalHit& b) { return a.score > b.score; });
    const LocalHit& best = refined.front();
    if (best.moments_valid) {
      const double sx = last_local_search_info_.step_xy, st = refine.step_theta;
      Matrix3d cov = best.cov;
      cov[0] += sx * sx / 12.0, cov[4] += sx * sx / 12.0, cov[8] += st * st / 12.0;
      initialize(best.mean_pose, cov);
    } else {
      if (!covariance) throw std::invalid_argument("relocalize: the best hit's moments are not valid and no covariance was given");
      initialize(best.mean_pose, *covariance);
    }
    return refined;
  }

  /// Extension: states | views::likelihoods(sensor_model(measurement)) (views/likelihoods.hpp:44-59) on the device - for each of
  /// `states`, in their order, the factor by which a reweight with `measurement` would multiply the weight of a particle there
  /// (mcl_likelihoods).  The filter is untouched: particles, weights, random stream, policies and counters stay as they are.
  /// Points in the base frame on a likelihood-field, beam or NDT filter; detections on a landmark or bearing filter (throws on a
  /// filter of another sensor model).
  [[nodiscard]] std::vector<double> likelihoods(const std::vector<SE2d>& states, const std::vector<std::pair<double, double>>& measurement) {
    static_assert(sizeof(std::pair<double, double>) == 2 * sizeof(double), "points are handed over as (x, y) doubles");
    std::vector<double> out(states.size());
    check(mcl_likelihoods(ctx_, states.empty() ? nullptr : states.data()->data(), states.size(),
                          measurement.empty() ? nullptr : &measurement.data()->first, measurement.size(), out.data()));
    return out;
  }
  [[nodiscard]] std::vector<double> likelihoods(const std::vector<SE2d>& states, const std::vector<LandmarkPositionDetection>& detections) {
    std::vector<double> xyz;
    std::vector<std::uint32_t> categories;
    flatten(detections, [](const LandmarkPositionDetection& d) -> const std::array<double, 3>& { return d.detection_position_in_robot; }, xyz,
            categories);
    std::vector<double> out(states.size());
    check(mcl_likelihoods_landmarks(ctx_, states.empty() ? nullptr : states.data()->data(), states.size(), xyz.data(), categories.data(),
                                    categories.size(), out.data()));
    return out;
  }
  [[nodiscard]] std::vector<double> likelihoods(const std::vector<SE2d>& states, const std::vector<LandmarkBearingDetection>& detections) {
    std::vector<double> xyz;
    std::vector<std::uint32_t> categories;
    flatten(detections, [](const LandmarkBearingDetection& d) -> const std::array<double, 3>& { return d.detection_bearing_in_sensor; }, xyz,
            categories);
    std::vector<double> out(states.size());
    check(mcl_likelihoods_bearings(ctx_, states.empty() ? nullptr : states.data()->data(), states.size(), xyz.data(), categories.data(),
                                   categories.size(), out.data()));
    return out;
  }
  /// Extension: Ray2d::cast (algorithm/raycasting.hpp:97-107) on the device for caller-given states and bearings (mcl_cast_rays): the
  /// range the map predicts from states[i] along bearings[b] = (cos, sin) of the beam's angle in the state's frame - unit vectors, used
  /// as they are - at [i * bearings.size() + b]; max_range where the ray hits nothing.  hit_cells (optional): y * width + x of each
  /// hit cell, -1 without one; cells_visited (optional): the cells the walks looked at.  The filter is untouched.  Likelihood-field
  /// and beam filters (throws on another).
  [[nodiscard]] std::vector<double> cast_rays(const std::vector<SE2d>& states, const std::vector<std::pair<double, double>>& bearings, double max_range,
                                              std::vector<std::int64_t>* hit_cells = nullptr, std::uint64_t* cells_visited = nullptr) {
    static_assert(sizeof(std::pair<double, double>) == 2 * sizeof(double), "bearings are handed over as (cos, sin) doubles");
    std::vector<double> ranges(states.size() * bearings.size());
    if (hit_cells) hit_cells->assign(ranges.size(), -1);
    check(mcl_cast_rays(ctx_, states.empty() ? nullptr : states.data()->data(), states.size(), bearings.empty() ? nullptr : &bearings.data()->first,
                        bearings.size(), max_range, ranges.data(), hit_cells ? hit_cells->data() : nullptr, cells_visited));
    return ranges;
  }
  /// Extension: the range table of the beam model (mcl_build_range_table; what MIT's rangelibc calls a look-up table): per cell and
  /// heading bin of num_angles, the squared cell distance to the cell the exact cast from the cell's centre hits.  From the next
  /// reweight on update(), reweight() and likelihoods() read it - one look-up per beam in place of a walk.  An approximation (the
  /// source's position inside its cell and the heading within a bin are discarded), hence opt-in.  Whatever installs a map afterwards
  /// rebuilds the table.  Beam filters only (throws on another); cast_rays() and global_search() stay exact.
  void build_range_table(std::uint32_t num_angles = 360) { check(mcl_build_range_table(ctx_, num_angles)); }
  /// Back to the exact walk; the table's memory is freed.
  void drop_range_table() { check(mcl_drop_range_table(ctx_)); }
  [[nodiscard]] mcl_range_table_info range_table_info() const {
    mcl_range_table_info info{};
    check(mcl_range_table_get_info(ctx_, &info));
    return info;
  }
  /// The bins' bearings (cos, sin) the table was built with.
  [[nodiscard]] std::vector<std::pair<double, double>> range_table_bearings() const {
    static_assert(sizeof(std::pair<double, double>) == 2 * sizeof(double), "bearings are handed over as (cos, sin) doubles");
    std::vector<std::pair<double, double>> out(range_table_info().num_angles);
    check(mcl_range_table_bearings(ctx_, out.empty() ? nullptr : &out.data()->first));
    return out;
  }
  /// The entries of cells first_cell .. first_cell + num_cells - 1 (cell = y * width + x), num_angles each; 0xFFFFFFFF: no hit.
  [[nodiscard]] std::vector<std::uint32_t> range_table(std::uint64_t first_cell, std::uint64_t num_cells) const {
    std::vector<std::uint32_t> out(num_cells * range_table_info().num_angles);
    check(mcl_range_table_read(ctx_, first_cell, num_cells, out.data()));
    return out;
  }
  /// Extension: beam skipping (mcl_set_beam_skip; Nav2 AMCL's do_beamskip, beam_skip_distance, beam_skip_threshold,
  /// beam_skip_error_threshold).  Before every reweight the cloud votes on each beam; beams that too few particles can explain are
  /// left out of that update, unless so much of the scan would go that all of it is used.  Likelihood-field sensor models only.
  void set_beam_skip(bool enabled, double distance = 0.5, double threshold = 0.3, double error_threshold = 0.9) {
    const mcl_beam_skip_params p{enabled ? 1 : 0, 0, distance, threshold, error_threshold};
    check(mcl_set_beam_skip(ctx_, &p));
  }
  /// The decision of the last update with beam skipping on (mcl_get_beam_skip_result), counts and mask by the points of that scan.
  struct BeamSkipResult {
    mcl_beam_skip_result summary{};
    std::vector<std::uint32_t> counts;
    std::vector<std::uint8_t> kept;
  };
  [[nodiscard]] BeamSkipResult beam_skip_result() {
    BeamSkipResult r;
    check(mcl_get_beam_skip_result(ctx_, &r.summary, nullptr, nullptr, 0));
    if (!r.summary.valid) return r;
    r.counts.resize(r.summary.num_beams);
    r.kept.resize(r.summary.num_beams);
    check(mcl_get_beam_skip_result(ctx_, &r.summary, r.counts.data(), r.kept.data(), r.summary.num_beams));
    return r;
  }
  /// For each point of `measurement` (base frame), the particles of the current set it agrees with (mcl_beam_agreement).  The filter
  /// is untouched: particles, weights, random stream, policies and counters stay as they are.
  [[nodiscard]] std::vector<std::uint32_t> beam_agreement(const std::vector<std::pair<double, double>>& measurement) {
    static_assert(sizeof(std::pair<double, double>) == 2 * sizeof(double), "points are handed over as (x, y) doubles");
    std::vector<std::uint32_t> counts(measurement.size());
    check(mcl_beam_agreement(ctx_, measurement.empty() ? nullptr : &measurement.data()->first, measurement.size(), counts.data()));
    return counts;
  }
  /// Extension (the landmark and bearing constructor forms only; throws on another sensor model): the small cycle of a landmark or
  /// bearing filter, mcl_set_landmark_small_cycle.  Sets of up to 4096 particles take a wave-per-particle reweight (bit for bit the
  /// lane-per-particle kernels' weights) and the one-launch tail with one host synchronisation.  Off by default.
  void set_landmark_small_cycle(bool on) { check(mcl_set_landmark_small_cycle(ctx_, on ? 1 : 0)); }
  [[nodiscard]] bool landmark_small_cycle() const {
    std::int32_t on = 0;
    check(mcl_get_landmark_small_cycle(ctx_, &on));
    return on != 0;
  }
  /// Update the NDT map used for localization (amcl_core.hpp:150 on the NDT filter).
  void update_map(const NDTMap2d& map) {
    if (ndt_params_.neighbors_kernel.empty() || ndt_params_.neighbors_kernel.size() > MCL_NDT_MAX_OFFSETS) throw std::invalid_argument("beluga_amd::Amcl: the neighbours kernel takes 1 .. 32 offsets");
    std::vector<std::int32_t> keys;
    std::vector<double> means, covs;
    keys.reserve(2 * map.size());
    means.reserve(2 * map.size());
    covs.reserve(4 * map.size());
    for (std::size_t i = 0; i < map.size(); ++i) {
      keys.push_back(map.keys()[i][0]);
      keys.push_back(map.keys()[i][1]);
      means.insert(means.end(), map.cells()[i].mean.begin(), map.cells()[i].mean.end());
      covs.insert(covs.end(), map.cells()[i].covariance.begin(), map.cells()[i].covariance.end());
    }
    mcl_ndt_params p;
    mcl_default_ndt_params(&p);
    p.minimum_likelihood = ndt_params_.minimum_likelihood;
    p.d1 = ndt_params_.d1;
    p.d2 = ndt_params_.d2;
    p.num_offsets = static_cast<std::uint32_t>(ndt_params_.neighbors_kernel.size());
    for (std::size_t k = 0; k < ndt_params_.neighbors_kernel.size(); ++k) {
      p.offsets[2 * k] = ndt_params_.neighbors_kernel[k][0];
      p.offsets[2 * k + 1] = ndt_params_.neighbors_kernel[k][1];
    }
    check(mcl_set_ndt_map(ctx_, keys.data(), means.data(), covs.data(), map.size(), map.resolution(), &p));
    ndt_resolution_ = map.resolution();
    has_field_ = false;
    field_.reset();
  }

  /// Extension (the NDT constructor form only; throws on another sensor model): the small cycle of an NDT filter,
  /// mcl_set_ndt_small_cycle.  Sets of up to 4096 particles take a wave-per-particle reweight and the one-launch tail with one host
  /// synchronisation; a cycle that would inject random states is handed back to the host behind the policies.  Off by default.
  void set_ndt_small_cycle(bool on) { check(mcl_set_ndt_small_cycle(ctx_, on ? 1 : 0)); }
  [[nodiscard]] bool ndt_small_cycle() const {
    std::int32_t on = 0;
    check(mcl_get_ndt_small_cycle(ctx_, &on));
    return on != 0;
  }
  /// {small cycles that ended inside the one-launch tail, small cycles the tail handed back}: running totals.
  [[nodiscard]] std::pair<std::uint64_t, std::uint64_t> ndt_small_cycle_counts() const {
    std::uint64_t completed = 0, handed_back = 0;
    check(mcl_get_ndt_small_cycle_counts(ctx_, &completed, &handed_back));
    return {completed, handed_back};
  }

  /// Extension (the NDT constructor form only; throws on another sensor model or another value): mcl_set_ndt_map_layout, how the NEXT
  /// update_map / build_ndt_map lays the map out on the device.  0: the dense index grid over the keys' bounding box, the default (a box
  /// beyond 2^26 cells is refused); 1: the hashed table where that grid does not fit; 2: the hashed table always.  The same weights, bit
  /// for bit, on every map both layouts hold; the installed map stays as it is.
  void set_ndt_map_layout(std::int32_t mode) { check(mcl_set_ndt_map_layout(ctx_, mode)); }
  /// {the mode as set, what the installed map uses: 0 dense, 1 hashed, -1 no map}.
  [[nodiscard]] std::pair<std::int32_t, std::int32_t> ndt_map_layout() const {
    std::int32_t mode = 0, in_use = 0;
    check(mcl_get_ndt_map_layout(ctx_, &mode, &in_use));
    return {mode, in_use};
  }

  /// Extension: the NDT map built on the device from a point cloud in the world frame, by the rule of NDTMap2d::from_points (the same
  /// cells, bit for bit), and installed in place; the sensor model's parameters stay.
  void build_ndt_map(const std::vector<std::pair<double, double>>& points, double resolution) {
    std::vector<double> xy;
    xy.reserve(2 * points.size());
    for (const auto& p : points) {
      xy.push_back(p.first);
      xy.push_back(p.second);
    }
    check(mcl_build_ndt_map_from_points(ctx_, xy.data(), points.size(), resolution));
    ndt_resolution_ = resolution;
  }
  /// ... from the occupied cells (value 100) of an occupancy grid.
  void build_ndt_map(const OccupancyGridView& grid, double resolution) {
    check(mcl_build_ndt_map_from_grid(ctx_, grid.cells, grid.width, grid.height, grid.resolution, grid.origin.data(), resolution));
    ndt_resolution_ = resolution;
  }
  /// The NDT map the filter holds, however it was set.
  [[nodiscard]] NDTMap2d ndt_map() const {
    std::uint64_t n = 0;
    check(mcl_get_ndt_map(ctx_, nullptr, nullptr, nullptr, 0, &n));
    std::vector<std::int32_t> keys(2 * n);
    std::vector<double> means(2 * n), covs(4 * n);
    check(mcl_get_ndt_map(ctx_, keys.data(), means.data(), covs.data(), n, &n));
    std::vector<NDTMap2d::key_type> k(n);
    std::vector<NDTCell2d> data(n);
    for (std::size_t j = 0; j < n; ++j) {
      k[j] = {keys[2 * j], keys[2 * j + 1]};
      data[j] = NDTCell2d{{means[2 * j], means[2 * j + 1]}, {covs[4 * j], covs[4 * j + 1], covs[4 * j + 2], covs[4 * j + 3]}};
    }
    return NDTMap2d{std::move(k), std::move(data), ndt_resolution_};
  }

  /// Update the map used for localization (amcl_core.hpp:150).
  void update_map(const OccupancyGridView& map) {
    const std::int8_t traits[3] = {map.free_value, map.unknown_value, map.occupied_value};
    check(mcl_set_map(ctx_, map.cells, map.width, map.height, map.resolution, map.origin.data(), traits));
    have_pending_ = false;  // (a map given now replaces one that was still on its way)
    width_ = map.width;
    height_ = map.height;
    resolution_ = map.resolution;
    std::int32_t has = 0;
    check(mcl_has_likelihood_field(ctx_, &has));
    has_field_ = has != 0;
    field_.reset();
  }

  /// update_map with a map that other filters read as well (mcl_use_shared_map): nothing is built or uploaded, and the filter's results
  /// are those of update_map with the same grid, bit for bit.  \throw std::runtime_error if the map was built for another device or
  /// sensor model (the filter is unchanged).
  void use_map(const SharedMap& map) {
    const mcl_shared_map_info info = map.info();
    check(mcl_use_shared_map(ctx_, map.native_handle()));
    have_pending_ = false;  // (a map given now replaces one that was still on its way)
    width_ = info.width;
    height_ = info.height;
    resolution_ = info.resolution;
    std::int32_t has = 0;
    check(mcl_has_likelihood_field(ctx_, &has));
    has_field_ = has != 0;
    field_.reset();
  }

  /// Extension (mcl_set_map_async): the new map's likelihood field is built on a worker thread - the reference's update_map blocks the
  /// caller for the build, seconds at 16 M cells - while the filter keeps running on the map it has; the swap happens at the start of the
  /// first update() after the build is done, or in map_commit().  `map` is copied before the call returns.
  void update_map_async(const OccupancyGridView& map) {
    const std::int8_t traits[3] = {map.free_value, map.unknown_value, map.occupied_value};
    check(mcl_set_map_async(ctx_, map.cells, map.width, map.height, map.resolution, map.origin.data(), traits));
    pending_ = {map.width, map.height, map.resolution};
    have_pending_ = true;
  }
  /// 0: no map on its way, 1: its field is being built, 2: built, waiting for the swap.
  int map_pending() {
    std::int32_t state = 0;
    check(mcl_map_pending(ctx_, &state));
    if (state == 0 && have_pending_) {  // the swap has happened (inside an update, or in map_commit)
      width_ = pending_.width;
      height_ = pending_.height;
      resolution_ = pending_.resolution;
      have_pending_ = false;
      field_.reset();
    }
    return state;
  }
  void map_commit(bool wait = true) {
    check(mcl_map_commit(ctx_, wait ? 1 : 0));
    (void)map_pending();
  }

  /// The C ABI writes points as a flat double[2 m]; the measurement type is a vector of pairs (no aliasing between the two).
  static measurement_type pairs_from(const std::vector<double>& flat, std::size_t m) {
    measurement_type points;
    points.reserve(m);
    for (std::size_t i = 0; i < m; ++i) points.emplace_back(flat[2 * i], flat[2 * i + 1]);
    return points;
  }

  /// Update particles based on motion and sensor information (amcl_core.hpp:165-201).  An empty particle set returns
  /// std::nullopt before the motion policy sees the control action (:166-168; mcl_update checks it first).
  auto update(const SE2d& control_action, const measurement_type& measurement) -> std::optional<estimation_type> {
    static_assert(sizeof(std::pair<double, double>) == 2 * sizeof(double), "measurement points must be packed pairs");
    mcl_estimate est;
    mcl_update_info info;
    check(mcl_update(ctx_, control_action.data(), measurement.empty() ? nullptr : &measurement.front().first, measurement.size(),
                     &est, &info));
    last_info_ = info;
    if (have_pending_) (void)map_pending();  // (a map given to update_map_async may have taken over inside this call)
    if (!info.updated) return std::nullopt;
    dirty_ = true;
    estimation_type out;
    out.first.c = est.pose[0];
    out.first.s = est.pose[1];
    out.first.x = est.pose[2];
    out.first.y = est.pose[3];
    for (int i = 0; i < 9; ++i) out.second[static_cast<std::size_t>(i)] = est.covariance[i];
    return out;
  }

  /// beluga_ros::Amcl::update(base_pose_in_odom, laser_scan) (beluga_ros/src/amcl.cpp:54-63).
  auto update(const SE2d& base_pose_in_odom, const LaserScan& laser_scan) -> std::optional<estimation_type> {
    mcl_laser_scan scan;
    scan.ranges = laser_scan.ranges.data();
    scan.num_ranges = laser_scan.ranges.size();
    scan.angle_min = laser_scan.angle_min;
    scan.angle_increment = laser_scan.angle_increment;
    scan.range_min = laser_scan.range_min;
    scan.range_max = laser_scan.range_max;
    for (std::size_t i = 0; i < 7; ++i) scan.origin_se3[i] = laser_scan.origin[i];
    scan.max_beams = laser_scan.max_beams;
    scan.min_range = laser_scan.min_range;
    scan.max_range = laser_scan.max_range;
    std::vector<double> flat(2 * (std::min<std::size_t>(laser_scan.ranges.size(), laser_scan.max_beams) + 1));
    std::uint64_t m = 0;
    check(mcl_prepare_laser_scan(&scan, flat.data(), &m));
    return update(base_pose_in_odom, pairs_from(flat, m));
  }

  /// Force a manual update of the particles on the next iteration of the filter (amcl_core.hpp:204).
  void force_update() { check(mcl_force_update(ctx_)); }

  /// Joins the communicator of a sharded filter (this instance was constructed with its `Shard`).  `transport`: the two
  /// collectives of the exchange over device buffers (MPI, threads of one process, ...); copied, its `user` must outlive this.
  /// A COLLECTIVE call for world > 1 (the ranks exchange a word of their configuration): every rank attaches, concurrently.
  void attach(unsigned rank, unsigned world, const mcl_transport& transport) { check(mcl_comm_attach(ctx_, rank, world, &transport)); }
  /// The same over RCCL / xGMI (librccl.so is loaded at run time): rank 0 calls rccl_unique_id() and hands the 128 bytes to
  /// the other ranks by whatever means the host has.
  void attach_rccl(const std::array<std::uint8_t, 128>& id, unsigned rank, unsigned world) {
    check(mcl_comm_attach_rccl(ctx_, id.data(), rank, world));
  }
  [[nodiscard]] static std::array<std::uint8_t, 128> rccl_unique_id() {
    std::array<std::uint8_t, 128> id{};
    if (mcl_comm_unique_id(id.data()) != MCL_OK) throw std::runtime_error(std::string("beluga_amd::Amcl: ") + mcl_last_error(nullptr));
    return id;
  }

  /// The pose sample behind beluga_ros::assign_particle_cloud(particles, size, PoseArray&)
  /// (beluga_ros/include/beluga_ros/particle_cloud.hpp:131-149): `size` states drawn with probability proportional to the
  /// weights (`views::sample | take_exactly(size)`); the set is not modified.  Pass a new draw_id per publication.
  [[nodiscard]] std::vector<SE2d> sample_particle_cloud(std::size_t size, std::uint32_t draw_id = 0) const {
    std::uint64_t n = 0;
    check(mcl_num_particles(ctx_, &n));
    std::vector<SE2d> out(n ? size : 0);
    if (!out.empty()) check(mcl_sample_particle_cloud(ctx_, out.size(), draw_id, reinterpret_cast<double*>(out.data())));
    return out;
  }

  /// beluga::cluster_based_estimate (algorithm/cluster_based_estimation.hpp:415-433) of the current particle set.
  [[nodiscard]] estimation_type cluster_based_estimate(double linear_hash_resolution = 0.20, double angular_hash_resolution = 0.524,
                                                       double weight_cap_percentile = 0.90) const {
    const mcl_cluster_params cp{linear_hash_resolution, angular_hash_resolution, weight_cap_percentile};
    mcl_estimate est;
    check(mcl_cluster_based_estimate(ctx_, &cp, &est));
    estimation_type out;
    out.first.c = est.pose[0];
    out.first.s = est.pose[1];
    out.first.x = est.pose[2];
    out.first.y = est.pose[3];
    for (int i = 0; i < 9; ++i) out.second[static_cast<std::size_t>(i)] = est.covariance[i];
    return out;
  }

  /// beluga::estimate_clusters (algorithm/cluster_based_estimation.hpp:337-399) over the clusters of ParticleClusterizer (:269-304):
  /// the weight, mean and covariance of the clusters of more than one particle - every hypothesis of the set, where
  /// cluster_based_estimate returns the heaviest alone.  The heaviest min(max_clusters, 64) of them, by descending weight (ties by
  /// ascending id); the first one is cluster_based_estimate's.  Not on a sharded filter.
  [[nodiscard]] std::vector<ClusterEstimate> estimate_clusters(const ParticleClusterizerParam& param = {}, std::size_t max_clusters = 64) const {
    const mcl_cluster_params cp{param.linear_hash_resolution, param.angular_hash_resolution, param.weight_cap_percentile};
    std::vector<mcl_cluster_estimate> raw(std::min<std::size_t>(max_clusters, MCL_MAX_CLUSTER_ESTIMATES));
    std::uint64_t total = 0;
    check(mcl_estimate_clusters(ctx_, &cp, raw.empty() ? nullptr : raw.data(), raw.size(), &total));
    raw.resize(std::min<std::size_t>(raw.size(), total));
    std::vector<ClusterEstimate> out(raw.size());
    for (std::size_t k = 0; k < raw.size(); ++k) {
      const mcl_estimate& est = raw[k].estimate;
      out[k].weight = raw[k].weight;
      out[k].mean.c = est.pose[0];
      out[k].mean.s = est.pose[1];
      out[k].mean.x = est.pose[2];
      out[k].mean.y = est.pose[3];
      for (int i = 0; i < 9; ++i) out[k].covariance[static_cast<std::size_t>(i)] = est.covariance[i];
      out[k].id = raw[k].id;
      out[k].count = raw[k].count;
    }
    return out;
  }

  /// ParticleClusterizer::operator() (:269-304): the cluster id of every particle, in particles()' order.  Not on a sharded filter.
  [[nodiscard]] std::vector<std::uint32_t> cluster_labels(const ParticleClusterizerParam& param = {}) const {
    const mcl_cluster_params cp{param.linear_hash_resolution, param.angular_hash_resolution, param.weight_cap_percentile};
    std::uint64_t n = 0;
    check(mcl_num_particles(ctx_, &n));
    std::vector<std::uint32_t> labels(n);
    if (n) check(mcl_cluster_labels(ctx_, &cp, labels.data()));
    return labels;
  }

  /// Makes update() return cluster_based_estimate, as beluga_ros::Amcl does (beluga_ros/src/amcl.cpp:125), instead of
  /// beluga::estimate, as beluga::Amcl does (amcl_core.hpp:200).  On a sharded filter (attach) a COLLECTIVE call: every rank, concurrently, alike.
  void use_cluster_based_estimate(bool enable) { check(mcl_set_estimate_kind(ctx_, enable ? 1 : 0, nullptr)); }

  /// beluga_ros::Amcl::likelihood_field() (beluga_ros/include/beluga_ros/amcl.hpp:141-158;
  /// LikelihoodFieldModelBase::likelihood_field(), likelihood_field_model_base.hpp:102), row-major height x width.
  /// \throw std::runtime_error If the sensor model has no likelihood field (the beam model).
  [[nodiscard]] const ValueGrid2<float>& likelihood_field() const {
    if (!has_field_) throw std::runtime_error("The current sensor model does not support likelihood field");
    if (!field_) {
      std::vector<float> data(static_cast<std::size_t>(width_) * height_);
      check(mcl_get_likelihood_field(ctx_, data.data()));
      field_.emplace(std::move(data), width_, resolution_);
    }
    return *field_;
  }

  /// beluga_ros::Amcl::likelihood_field_origin() (beluga_ros/include/beluga_ros/amcl.hpp:161-178).
  /// \throw std::runtime_error If the sensor model has no likelihood field.
  [[nodiscard]] SE2d likelihood_field_origin() const {
    SE2d origin;
    const mcl_status st = mcl_get_likelihood_field_origin(ctx_, origin.data());
    if (st == MCL_ERR_UNSUPPORTED) throw std::runtime_error("The current sensor model does not support likelihood field");
    check(st);
    return origin;
  }

  /// beluga_ros::Amcl::has_likelihood_field() (beluga_ros/include/beluga_ros/amcl.hpp:181-188).
  [[nodiscard]] bool has_likelihood_field() const { return has_field_; }

  /// beluga_ros::Amcl::initialize_from_map() (beluga_ros/include/beluga_ros/amcl.hpp:209): max_particles states drawn
  /// uniformly over the free cells of the map (random/multivariate_uniform_distribution.hpp:126-161).
  void initialize_from_map() {
    check(mcl_initialize_from_map(ctx_));
    dirty_ = true;
  }

  /// beluga_ros::Amcl::update(base_pose_in_odom, point_cloud) (beluga_ros/src/amcl.cpp:67-81): `points_xyz` are the cloud's
  /// points (3 floats each) in the sensor frame, `origin` the sensor pose in the base frame as Sophus::SE3d::data().
  auto update(const SE2d& base_pose_in_odom, const std::vector<float>& points_xyz, const std::array<double, 7>& origin)
      -> std::optional<estimation_type> {
    std::vector<double> flat(2 * (points_xyz.size() / 3 + 1));
    check(mcl_project_point_cloud(points_xyz.data(), points_xyz.size() / 3, origin.data(), flat.data()));
    return update(base_pose_in_odom, pairs_from(flat, points_xyz.size() / 3));
  }

  [[nodiscard]] const mcl_update_info& last_update_info() const { return last_info_; }
  [[nodiscard]] std::size_t max_particles() const { return max_particles_; }
  [[nodiscard]] mcl_ctx* native_handle() const { return ctx_; }

 private:
  void check(mcl_status st) const {
    if (st != MCL_OK) throw std::runtime_error(std::string("beluga_amd::Amcl: ") + mcl_last_error(ctx_));
  }
  static std::vector<LocalHit> local_hits(const std::vector<mcl_local_hit>& raw, std::size_t n) {
    std::vector<LocalHit> hits(n);
    for (std::size_t i = 0; i < n; ++i) {
      const mcl_local_hit& r = raw[i];
      LocalHit& h = hits[i];
      h.pose.c = r.pose[0], h.pose.s = r.pose[1], h.pose.x = r.pose[2], h.pose.y = r.pose[3];
      h.mean_pose.c = r.mean_pose[0], h.mean_pose.s = r.mean_pose[1], h.mean_pose.x = r.mean_pose[2], h.mean_pose.y = r.mean_pose[3];
      h.score = r.score, h.seed_score = r.seed_score, h.di = r.di, h.dj = r.dj, h.dk = r.dk, h.plateau = r.plateau;
      std::copy(r.cov, r.cov + 9, h.cov.begin());
      std::copy(r.sums, r.sums + 10, h.sums.begin());
      h.moments_valid = r.moments_valid != 0;
    }
    return hits;
  }
  mcl_ctx* ctx_{nullptr};
  mcl_search_info last_search_info_{};
  mcl_local_search_info last_local_search_info_{};
  struct PendingShape {
    std::uint32_t width{0}, height{0};
    double resolution{0.0};
  };
  PendingShape pending_{};  ///< of the map given to update_map_async, until its swap
  bool have_pending_{false};
  std::uint32_t width_{0}, height_{0};
  std::size_t max_particles_{0};
  double resolution_{0.0};
  bool has_field_{false};
  NDTModelParam2d ndt_params_{};
  double ndt_resolution_{0.0};  // of the NDT map the context holds
  LandmarkModelParam landmark_params_{};
  BearingModelParam bearing_params_{};
  int landmark_kind_{0};
  mutable ParticleSet mirror_;
  mutable bool dirty_{true};
  mutable std::optional<ValueGrid2<float>> field_;
  mcl_update_info last_info_{};

  friend class AmclBatch;
  friend class SharedMap;
  /// A member of an AmclBatch: bound to a context the batch owns (mcl_destroy does nothing on it).
  struct Adopted {};
  Amcl(Adopted, mcl_ctx* ctx, const AmclParams& params) : ctx_(ctx), max_particles_(params.max_particles) {}
};

/// One member of an AmclBatch: the arguments of Amcl's constructor for an occupancy grid (the likelihood-field, likelihood-field-prob and
/// beam sensor models).  The map is installed by the batch's constructor; `map.cells == nullptr`: the member gets its map later
/// (update_map on the member).
struct AmclBatchSpec {
  OccupancyGridView map;
  MotionModelParam motion;
  SensorModelParam sensor;
  AmclParams params{};
  std::uint64_t seed{0};
  std::vector<std::pair<std::string, std::int64_t>> options{};
};

/// One member of an AmclBatch of landmark or bearing filters: the arguments of Amcl's constructor over a LandmarkMap.  `small_cycle`:
/// set_landmark_small_cycle(true) on the member, so that it shares the fleet's launches (at most 4096 particles).
struct AmclLandmarkBatchSpec {
  LandmarkMap map;
  MotionModelParam motion;
  std::variant<LandmarkModelParam, BearingModelParam> sensor;
  AmclParams params{};
  std::uint64_t seed{0};
  bool small_cycle{false};
  std::vector<std::pair<std::string, std::int64_t>> options{};
};

/// A fleet of small filters that share their launches (mcl_batch_*): one update call, three kernel launches for all members whose cycle
/// is the small one (likelihood-field models, at most 4096 particles), one synchronisation; every other member runs its ordinary cycle
/// inside the same call.  member(i) is a beluga_amd::Amcl bound to the batch's i-th context: every method of Amcl works on it between
/// batch updates, all filter state lives in it, and for every member update() below does, bit for bit, what member(i).update(...) does.
class AmclBatch {
 public:
  using measurement_type = Amcl::measurement_type;
  using estimation_type = Amcl::estimation_type;

  explicit AmclBatch(const std::vector<AmclBatchSpec>& specs, int device = 0) {
    std::vector<mcl_config> cfgs;
    for (const AmclBatchSpec& s : specs) {
      if (std::holds_alternative<NDTModelParam2d>(s.sensor)) throw std::invalid_argument("beluga_amd::AmclBatch: an occupancy-grid sensor model");
      cfgs.push_back(Amcl::make_config(s.motion, s.sensor, s.params, s.seed, device, Shard{}));
    }
    const mcl_status st = mcl_batch_create(cfgs.data(), static_cast<std::uint32_t>(cfgs.size()), &batch_);
    if (st != MCL_OK) throw std::runtime_error(std::string("beluga_amd::AmclBatch: ") + mcl_batch_last_error(nullptr));
    try {
      members_.reserve(specs.size());
      for (std::size_t i = 0; i < specs.size(); ++i) {
        mcl_ctx* ctx = nullptr;
        check(mcl_batch_member(batch_, static_cast<std::uint32_t>(i), &ctx));
        members_.push_back(Amcl(Amcl::Adopted{}, ctx, specs[i].params));
        for (const auto& [name, value] : specs[i].options) members_.back().check(mcl_set_option(ctx, name.c_str(), value));
        if (specs[i].map.cells) members_.back().update_map(specs[i].map);
      }
    } catch (...) {
      release();
      throw;
    }
    estimates_.resize(specs.size());
    infos_.resize(specs.size());
    statuses_.assign(specs.size(), MCL_OK);
  }
  /// A fleet of landmark and bearing filters (mcl_landmark_batch_update): update() over one vector of detections per member.
  explicit AmclBatch(const std::vector<AmclLandmarkBatchSpec>& specs, int device = 0) {
    std::vector<mcl_config> cfgs;
    for (const AmclLandmarkBatchSpec& s : specs) {
      mcl_config cfg = Amcl::base_config(s.motion, s.params, s.seed, device, Shard{});
      cfg.sensor_kind = std::holds_alternative<BearingModelParam>(s.sensor) ? MCL_SENSOR_BEARING : MCL_SENSOR_LANDMARK;
      cfgs.push_back(cfg);
    }
    const mcl_status st = mcl_batch_create(cfgs.data(), static_cast<std::uint32_t>(cfgs.size()), &batch_);
    if (st != MCL_OK) throw std::runtime_error(std::string("beluga_amd::AmclBatch: ") + mcl_batch_last_error(nullptr));
    try {
      members_.reserve(specs.size());
      for (std::size_t i = 0; i < specs.size(); ++i) {
        mcl_ctx* ctx = nullptr;
        check(mcl_batch_member(batch_, static_cast<std::uint32_t>(i), &ctx));
        members_.push_back(Amcl(Amcl::Adopted{}, ctx, specs[i].params));
        Amcl& m = members_.back();
        m.landmark_kind_ = cfgs[i].sensor_kind;
        if (const auto* bearing = std::get_if<BearingModelParam>(&specs[i].sensor)) m.bearing_params_ = *bearing;
        else m.landmark_params_ = std::get<LandmarkModelParam>(specs[i].sensor);
        for (const auto& [name, value] : specs[i].options) m.check(mcl_set_option(ctx, name.c_str(), value));
        if (specs[i].small_cycle) m.set_landmark_small_cycle(true);
        m.update_map(specs[i].map);
      }
    } catch (...) {
      release();
      throw;
    }
    estimates_.resize(specs.size());
    infos_.resize(specs.size());
    statuses_.assign(specs.size(), MCL_OK);
  }
  AmclBatch(const AmclBatch&) = delete;
  AmclBatch& operator=(const AmclBatch&) = delete;
  ~AmclBatch() { release(); }

  [[nodiscard]] std::size_t size() const { return members_.size(); }
  [[nodiscard]] Amcl& member(std::size_t i) { return members_.at(i); }
  [[nodiscard]] std::vector<Amcl>& members() { return members_; }

  /// Amcl::update on every member (amcl_core.hpp:165-201): control_actions[i] and measurements[i] are member i's.  An entry is
  /// std::nullopt where the member did not update (no motion, no particles).  \throw std::runtime_error where a member fails;
  /// statuses() then tells which, and the other members have updated.
  auto update(const std::vector<SE2d>& control_actions, const std::vector<measurement_type>& measurements)
      -> std::vector<std::optional<estimation_type>> {
    static_assert(sizeof(std::pair<double, double>) == 2 * sizeof(double), "measurement points must be packed pairs");
    static_assert(sizeof(SE2d) == 4 * sizeof(double), "control actions must be packed (cos, sin, x, y) records");
    if (control_actions.size() != size() || measurements.size() != size())
      throw std::invalid_argument("beluga_amd::AmclBatch: one control action and one measurement per member");
    offsets_.assign(size() + 1, 0);
    points_.clear();
    for (std::size_t i = 0; i < size(); ++i) {
      for (const auto& p : measurements[i]) {
        points_.push_back(p.first);
        points_.push_back(p.second);
      }
      offsets_[i + 1] = points_.size() / 2;
    }
    const mcl_status st = mcl_batch_update(batch_, size() ? control_actions.front().data() : nullptr, points_.data(), offsets_.data(),
                                           estimates_.data(), infos_.data(), statuses_.data());
    std::vector<std::optional<estimation_type>> out(size());
    for (std::size_t i = 0; i < size(); ++i)
      if (statuses_[i] == MCL_OK) out[i] = members_[i].finish_update(estimates_[i], infos_[i]);
    check(st);
    return out;
  }

  /// Amcl::update on every member of a fleet of landmark filters / of bearing filters (mcl_landmark_batch_update): control_actions[i] and
  /// detections[i] are member i's; for every member, bit for bit, what member(i).update(control_actions[i], detections[i]) does.  Members
  /// with set_landmark_small_cycle(true) share three launches; every other one runs its own cycle inside the call.  Throws as above.
  auto update(const std::vector<SE2d>& control_actions, const std::vector<std::vector<LandmarkPositionDetection>>& detections)
      -> std::vector<std::optional<estimation_type>> {
    return update_detections(control_actions, detections,
                             [](const LandmarkPositionDetection& d) -> const std::array<double, 3>& { return d.detection_position_in_robot; });
  }
  auto update(const std::vector<SE2d>& control_actions, const std::vector<std::vector<LandmarkBearingDetection>>& detections)
      -> std::vector<std::optional<estimation_type>> {
    return update_detections(control_actions, detections,
                             [](const LandmarkBearingDetection& d) -> const std::array<double, 3>& { return d.detection_bearing_in_sensor; });
  }

  /// Every member, or member `index`, reads the shared map from now on (Amcl::use_map): a fleet on one building's map holds it once.
  void use_map(const SharedMap& map) {
    for (Amcl& m : members_) m.use_map(map);
  }
  void use_map(std::size_t index, const SharedMap& map) { members_.at(index).use_map(map); }

  [[nodiscard]] const std::vector<mcl_update_info>& last_infos() const { return infos_; }
  [[nodiscard]] const std::vector<mcl_status>& statuses() const { return statuses_; }
  /// mcl_set_option on every member, e.g. batch_cluster_fused (default 1; 0: the member's cluster-based estimate through its own kernels
  /// instead of the fleet's two shared launches).
  void set_option(const std::string& name, std::int64_t value) {
    for (Amcl& m : members_) m.check(mcl_set_option(m.ctx_, name.c_str(), value));
  }
  /// cycles, kernel_launches, members_fused, members_alone, cluster_launches, members_cluster_fused, cluster_host_ns, beam_launches, members_beam_fused,
  /// landmark_launches, members_landmark_fused (mcl_batch_get_counter).
  [[nodiscard]] std::uint64_t counter(const std::string& name) const {
    std::uint64_t value = 0;
    check(mcl_batch_get_counter(batch_, name.c_str(), &value));
    return value;
  }
  [[nodiscard]] mcl_batch* native_handle() const { return batch_; }

 private:
  void check(mcl_status st) const {
    if (st != MCL_OK) throw std::runtime_error(std::string("beluga_amd::AmclBatch: ") + mcl_batch_last_error(batch_));
  }
  template <class Detection, class Get>
  auto update_detections(const std::vector<SE2d>& control_actions, const std::vector<std::vector<Detection>>& detections, Get get)
      -> std::vector<std::optional<estimation_type>> {
    static_assert(sizeof(SE2d) == 4 * sizeof(double), "control actions must be packed (cos, sin, x, y) records");
    if (control_actions.size() != size() || detections.size() != size())
      throw std::invalid_argument("beluga_amd::AmclBatch: one control action and one vector of detections per member");
    offsets_.assign(size() + 1, 0);
    points_.clear();
    categories_.clear();
    for (std::size_t i = 0; i < size(); ++i) {
      for (const Detection& d : detections[i]) {
        const std::array<double, 3>& v = get(d);
        points_.insert(points_.end(), v.begin(), v.end());
        categories_.push_back(d.category);
      }
      offsets_[i + 1] = categories_.size();
    }
    const mcl_status st = mcl_landmark_batch_update(batch_, size() ? control_actions.front().data() : nullptr, points_.data(), categories_.data(),
                                                    offsets_.data(), estimates_.data(), infos_.data(), statuses_.data());
    std::vector<std::optional<estimation_type>> out(size());
    for (std::size_t i = 0; i < size(); ++i)
      if (statuses_[i] == MCL_OK) out[i] = members_[i].finish_update(estimates_[i], infos_[i]);
    check(st);
    return out;
  }
  void release() {
    for (Amcl& m : members_) m.ctx_ = nullptr;  // (the batch destroys the contexts)
    members_.clear();
    mcl_batch_destroy(batch_);
    batch_ = nullptr;
  }
  mcl_batch* batch_{nullptr};
  std::vector<Amcl> members_;
  std::vector<double> points_;
  std::vector<std::uint32_t> categories_;
  std::vector<std::uint64_t> offsets_;
  std::vector<mcl_estimate> estimates_;
  std::vector<mcl_update_info> infos_;
  std::vector<mcl_status> statuses_;
};

inline SharedMap::SharedMap(const OccupancyGridView& map, const SensorModelParam& sensor, int device, bool device_field_build) {
  if (std::holds_alternative<NDTModelParam2d>(sensor)) throw std::invalid_argument("beluga_amd::SharedMap: an occupancy-grid sensor model");
  const mcl_config cfg = Amcl::make_config(StationaryModelParam{}, sensor, AmclParams{}, 0, device, Shard{});
  const std::int8_t traits[3] = {map.free_value, map.unknown_value, map.occupied_value};
  const mcl_status st = mcl_shared_map_create(&cfg, map.cells, map.width, map.height, map.resolution, map.origin.data(), traits,
                                              device_field_build ? 1 : 0, &map_);
  if (st != MCL_OK) throw std::runtime_error(std::string("beluga_amd::SharedMap: ") + mcl_shared_map_last_error(nullptr));
}

}  // namespace beluga_amd

#endif  // BELUGA_AMD_AMCL_HPP
