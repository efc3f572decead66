/* beluga_mcl.h — C ABI of libbeluga_mcl.so: the MI355X-native MCL particle-filter update.
 *
 * This is the drop-in boundary for ONE hot path of Ekumen-OS/beluga: `beluga::Amcl::update`
 * (beluga/include/beluga/algorithm/amcl_core.hpp:165-201) with DifferentialDriveModel +
 * LikelihoodFieldModel | BeamSensorModel, multinomial / KLD-adaptive resampling and the SE2
 * estimate.  The reference has no FFI for this path (it is header-only C++17 templates); these
 * entry points are what a binding for the path binds: one per reference call named below.
 * Plain pointers and sizes only, no C++/torch types, no exceptions across the boundary.
 *
 * Conventions
 *   - An SE2 pose is 4 doubles (cos, sin, x, y) = Sophus::SE2d::data() order, the layout of the
 *     reference's particle states (beluga/containers/tuple_vector.hpp:198 over Sophus::SE2d).
 *   - Particle sets cross the boundary as `states[n*4]` + `weights[n]` (host memory, caller owned).
 *     On the device the poses live as the same 4-double records (plus a weight array), owned by the context.
 *   - A measurement is `points_xy[B*2]` doubles: lidar hits in the robot base frame
 *     (`std::vector<std::pair<double,double>>`, sensor/likelihood_field_model.hpp:48).
 *   - Every call returns mcl_status (0 = OK, <0 = error; mcl_last_error() has the text).  Calls on
 *     one context must be serialised by the caller (the reference filter is not thread-safe either:
 *     beluga_amcl/src/ros2_common.cpp:407-409 uses one mutually exclusive callback group).
 *   - All work is enqueued on the context's HIP stream; calls that return host data synchronise it.
 *   - There is NO CPU fallback: mcl_create fails with MCL_ERR_NO_DEVICE when no gfx950 GPU is usable.
 */
#ifndef BELUGA_MCL_H
#define BELUGA_MCL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mcl_ctx mcl_ctx;
typedef struct mcl_batch mcl_batch; /* a fleet of contexts that share their launches ("Batches of small filters" below) */
typedef int32_t mcl_status;

enum {
  MCL_OK = 0,
  MCL_ERR_INVALID_ARGUMENT = -1,
  MCL_ERR_HIP = -2,
  MCL_ERR_OUT_OF_MEMORY = -3,
  MCL_ERR_NOT_READY = -4,      /* no map / no particles yet */
  MCL_ERR_BAD_COVARIANCE = -5, /* std::runtime_error of multivariate_normal_distribution.hpp:114-124 */
  MCL_ERR_NO_DEVICE = -6,
  MCL_ERR_UNSUPPORTED = -7     /* std::runtime_error "The current sensor model does not support likelihood field" (beluga_ros/amcl.hpp:154,174) */
};

/* LikelihoodFieldModel (sensor/likelihood_field_model.hpp), BeamSensorModel (sensor/beam_model.hpp),
 * LikelihoodFieldProbModel (sensor/likelihood_field_prob_model.hpp): beluga_ros::Amcl's sensor variants.
 * NDTSensorModel over a SparseValueGrid2 of NDTCell2d (sensor/ndt_sensor_model.hpp): the filter of beluga_amcl's ndt_amcl_node
 * (its map comes from mcl_set_ndt_map, see "2D NDT sensor model" below).
 * LandmarkSensorModel2d and BearingSensorModel2d over a LandmarkMap (sensor/landmark_sensor_model.hpp, sensor/bearing_sensor_model.hpp):
 * their map comes from mcl_set_landmark_map, their measurement through mcl_update_landmarks / mcl_update_bearings (see "Landmark and
 * bearing sensor models" below). */
enum {
  MCL_SENSOR_LIKELIHOOD_FIELD = 0,
  MCL_SENSOR_BEAM = 1,
  MCL_SENSOR_LIKELIHOOD_FIELD_PROB = 2,
  MCL_SENSOR_NDT = 3,
  MCL_SENSOR_LANDMARK = 4,
  MCL_SENSOR_BEARING = 5
};
/* DifferentialDriveModel, OmnidirectionalDriveModel (motion/omnidirectional_drive_model.hpp:102-146),
 * StationaryModel (motion/stationary_model.hpp:55-61): beluga_ros::Amcl's motion variants. */
enum { MCL_MOTION_DIFFERENTIAL = 0, MCL_MOTION_OMNIDIRECTIONAL = 1, MCL_MOTION_STATIONARY = 2 };

/* beluga::AmclParams (algorithm/amcl_core.hpp:34-55) + the spatial-hash resolutions that
 * beluga_ros::AmclParams adds (beluga_ros/include/beluga_ros/amcl.hpp:90-97). Same defaults. */
typedef struct mcl_amcl_params {
  double update_min_d;          /* 0.25 */
  double update_min_a;          /* 0.2 */
  uint64_t resample_interval;   /* 1 */
  int32_t selective_resampling; /* 0 */
  int32_t reserved0;
  uint64_t min_particles; /* 500 */
  uint64_t max_particles; /* 2000 */
  double alpha_slow;      /* 0.001 */
  double alpha_fast;      /* 0.1 */
  double kld_epsilon;     /* 0.05 */
  double kld_z;           /* 3.0 */
  double spatial_resolution_x;     /* 0.5 */
  double spatial_resolution_y;     /* 0.5 */
  double spatial_resolution_theta; /* 10 deg in rad */
} mcl_amcl_params;

/* beluga::DifferentialDriveModelParam (motion/differential_drive_model.hpp:40-68). */
typedef struct mcl_diffdrive_params {
  double rotation_noise_from_rotation;       /* alpha1 */
  double rotation_noise_from_translation;    /* alpha2 */
  double translation_noise_from_translation; /* alpha3 */
  double translation_noise_from_rotation;    /* alpha4 */
  double distance_threshold;                 /* 0.01 */
} mcl_diffdrive_params;

/* beluga::LikelihoodFieldModelBaseParam (sensor/likelihood_field_model_base.hpp:42-64). */
typedef struct mcl_lf_params {
  double max_obstacle_distance; /* 100.0 */
  double max_laser_distance;    /* 2.0 */
  double z_hit;                 /* 0.5 */
  double z_random;              /* 0.5 */
  double sigma_hit;             /* 0.2 */
  int32_t model_unknown_space;      /* 0 */
  int32_t only_obstacle_boundaries; /* 0 */
} mcl_lf_params;

/* beluga::BeamModelParam (sensor/beam_model.hpp:43-58). */
/* beam_max_range / (the map's resolution) must stay below 2^27 - 2 cells (6 700 km at 5 cm): the ray walks keep 16 x the line's span in
 * an int.  mcl_reweight, mcl_update and a batch member's update return MCL_ERR_INVALID_ARGUMENT otherwise, the set untouched. */
typedef struct mcl_beam_params {
  double z_hit, z_short, z_max, z_rand, sigma_hit, lambda_short, beam_max_range;
} mcl_beam_params;

typedef struct mcl_config {
  int32_t device_id;   /* HIP device ordinal */
  int32_t sensor_kind; /* MCL_SENSOR_* */
  uint64_t seed;       /* key of the counter-based Philox4x32-10 stream (DESIGN.md "RNG stream") */
  mcl_amcl_params amcl;
  mcl_diffdrive_params motion;
  mcl_lf_params lf;
  mcl_beam_params beam;
  /* Particle sharding across processes (one context per GPU).  A single-GPU filter uses
   * shard_offset = 0, shard_count = max_particles.  Random draws are addressed by GLOBAL index. */
  uint64_t shard_offset;
  uint64_t shard_capacity; /* 0 => amcl.max_particles */
  void* hip_stream;        /* optional external hipStream_t (e.g. torch's current stream); NULL => own stream */
  int32_t motion_kind;     /* MCL_MOTION_*; the four alphas in `motion` are shared by the differential and omni models */
  int32_t reserved1;
  double strafe_noise_from_translation; /* OmnidirectionalDriveModelParam alpha5 (omnidirectional_drive_model.hpp:64-70) */
} mcl_config;

/* Fills `cfg` with the reference defaults listed above. */
void mcl_default_config(mcl_config* cfg);

/* beluga::Amcl ctor (amcl_core.hpp:105-124). */
mcl_status mcl_create(const mcl_config* cfg, mcl_ctx** out);
void mcl_destroy(mcl_ctx* ctx); /* does nothing on a member of a batch: mcl_batch_destroy is its owner */
const char* mcl_last_error(const mcl_ctx* ctx); /* ctx may be NULL: error of the last failed mcl_create */

/* Sensor-model ctor / Amcl::update_map (amcl_core.hpp:150; likelihood_field_model_base.hpp:96-99,113-116,
 * 130-185; beam_model.hpp:152-156).  `cells` is row-major H x W int8 with value traits
 * {free, unknown, occupied} (beluga_ros/occupancy_grid.hpp:48-64 uses {0,-1,100}).
 * Builds the likelihood field with the reference's algorithm and uploads grid, field and the
 * free-cell list used by the random-state generator (random/multivariate_uniform_distribution.hpp:126-161). */
mcl_status mcl_set_map(mcl_ctx* ctx, const int8_t* cells, uint32_t width, uint32_t height, double resolution,
                       const double origin[4], const int8_t value_traits[3]);
/* Extension beside mcl_set_map (the reference has no such call: Amcl::update_map, amcl_core.hpp:150, builds the new sensor model on the
 * caller's thread, which at 16 M cells is 1 - 3 s of priority-queue wavefront, distance_map.hpp:55-98, during which no update runs):
 * the arguments are copied, the likelihood field of the new grid is built on a WORKER thread - the same host wavefront, the same bits -
 * while the filter keeps running on the map it has, and the swap (uploads, derived tables: a few milliseconds) happens at the start of
 * the first mcl_update after the build is done, or in mcl_map_commit.  A second call, or mcl_set_map, replaces a pending one.
 * mcl_map_pending: *state = 0 nothing pending, 1 building, 2 built and waiting for its swap.
 * mcl_map_commit: swaps now if the build is done (wait = 0: otherwise returns with nothing changed; wait = 1: waits for it first).
 * Not on a filter with a communicator of several ranks (MCL_ERR_UNSUPPORTED): the ranks would swap in different cycles. */
mcl_status mcl_set_map_async(mcl_ctx* ctx, const int8_t* cells, uint32_t width, uint32_t height, double resolution,
                             const double origin[4], const int8_t value_traits[3]);
mcl_status mcl_map_pending(mcl_ctx* ctx, int32_t* state);
mcl_status mcl_map_commit(mcl_ctx* ctx, int32_t wait);
/* LikelihoodFieldModelBase::likelihood_field() (likelihood_field_model_base.hpp:102). out: H*W floats. */
mcl_status mcl_get_likelihood_field(mcl_ctx* ctx, float* out);
/* beluga_ros::Amcl::has_likelihood_field() (beluga_ros/include/beluga_ros/amcl.hpp:181-188): 1 for the two likelihood-field
 * models, 0 for the beam model. */
mcl_status mcl_has_likelihood_field(const mcl_ctx* ctx, int32_t* has);
/* beluga_ros::Amcl::likelihood_field_origin() (amcl.hpp:161-178; likelihood_field_model_base.hpp:105): the field's origin
 * in world coordinates as (cos, sin, x, y).  MCL_ERR_UNSUPPORTED for the beam model (the reference throws). */
mcl_status mcl_get_likelihood_field_origin(mcl_ctx* ctx, double origin[4]);
/* Replace the device field with a caller-built one (same W,H as the current map). */
mcl_status mcl_set_likelihood_field(mcl_ctx* ctx, const float* field);

/* Amcl::initialize(pose, covariance) (amcl_core.hpp:145-147): max_particles samples of
 * N(mean_xytheta, cov[3x3 row-major]) with weight 1; sets force_update. */
mcl_status mcl_initialize_normal(mcl_ctx* ctx, const double mean_xytheta[3], const double cov[9]);
/* beluga_ros::Amcl::initialize_from_map() (beluga_ros/include/beluga_ros/amcl.hpp:209, called at
 * beluga_amcl/src/amcl_node.cpp:716): max_particles draws of MultivariateUniformDistribution<SE2d, OccupancyGrid>
 * (random/multivariate_uniform_distribution.hpp:126-161: the centre of a uniformly chosen free cell in the world frame,
 * uniform heading), weight 1; sets force_update.  Drawn on the device from the counter-based stream (step 0). */
mcl_status mcl_initialize_from_map(mcl_ctx* ctx);
/* Amcl::initialize(distribution) with caller-drawn states (amcl_core.hpp:131-137); n <= capacity. */
mcl_status mcl_set_particles(mcl_ctx* ctx, const double* states, const double* weights, uint64_t n);
/* Amcl::particles() (amcl_core.hpp:127). */
mcl_status mcl_num_particles(mcl_ctx* ctx, uint64_t* n);
mcl_status mcl_get_particles(mcl_ctx* ctx, double* states, double* weights, uint64_t capacity, uint64_t* n);
/* Amcl::force_update() (amcl_core.hpp:204). */
mcl_status mcl_force_update(mcl_ctx* ctx);

typedef struct mcl_estimate {
  double pose[4];        /* (cos, sin, x, y) */
  double covariance[9];  /* row-major 3x3: xy block + circular variance at [8] */
} mcl_estimate;

typedef struct mcl_update_info {
  int32_t updated;    /* 0 <=> the reference returns std::nullopt (amcl_core.hpp:166-172) */
  int32_t resampled;  /* resample_policy_ fired (amcl_core.hpp:181) */
  uint64_t num_particles;          /* after the update */
  double weight_sum;               /* sum of weights before normalisation */
  double effective_sample_size;    /* -1 when the policy did not evaluate it */
  double random_state_probability; /* ThrunRecoveryProbabilityEstimator output (amcl_core.hpp:179) */
} mcl_update_info;

/* Amcl::update(control_action, measurement) (amcl_core.hpp:165-201): the whole cycle. */
mcl_status mcl_update(mcl_ctx* ctx, const double control_pose[4], const double* points_xy, uint64_t num_points,
                      mcl_estimate* estimate, mcl_update_info* info);

/* Caller-side scan preparation, i.e. what beluga_ros::Amcl::update(pose, LaserScan) does before the filter sees the
 * measurement (beluga_ros/src/amcl.cpp:54-63; beluga_ros/include/beluga_ros/laser_scan.hpp:46-100;
 * beluga/sensor/data/laser_scan.hpp:64-90; beluga/views/take_evenly.hpp:126-148): decimate to `max_beams` evenly
 * spaced beams, drop NaN and out-of-range readings, polar -> cartesian, move into the base frame with the laser origin
 * `origin_se3` = Sophus::SE3d::data() = (qx, qy, qz, qw, tx, ty, tz).  sensor_msgs/LaserScan fields are float32.
 * Pure host arithmetic (O(beams)); `points_xy` must hold 2 * min(n, max_beams) doubles. */
typedef struct mcl_laser_scan {
  const float* ranges;
  uint64_t num_ranges;
  float angle_min, angle_increment;
  float range_min, range_max; /* from the message */
  double origin_se3[7];
  uint64_t max_beams;         /* SIZE_MAX: all */
  double min_range, max_range; /* caller limits (laser_min_range / laser_max_range); combined with the message's */
} mcl_laser_scan;
mcl_status mcl_prepare_laser_scan(const mcl_laser_scan* scan, double* points_xy, uint64_t* num_points);
/* mcl_prepare_laser_scan followed by mcl_update: beluga_ros::Amcl::update(base_pose_in_odom, laser_scan). */
mcl_status mcl_update_laser_scan(mcl_ctx* ctx, const double control_pose[4], const mcl_laser_scan* scan, mcl_estimate* estimate,
                                 mcl_update_info* info);

/* beluga_ros::Amcl::update(base_pose_in_odom, SparsePointCloud3f) (beluga_ros/src/amcl.cpp:67-81): every point of the
 * cloud (float x, y, z in the sensor frame) is moved into the base frame with the sensor origin `origin_se3` =
 * Sophus::SE3d::data() = (qx, qy, qz, qw, tx, ty, tz) in double precision and projected onto z = 0. */
mcl_status mcl_project_point_cloud(const float* points_xyz, uint64_t num_points, const double origin_se3[7], double* points_xy);
mcl_status mcl_update_point_cloud(mcl_ctx* ctx, const double control_pose[4], const float* points_xyz, uint64_t num_points,
                                  const double origin_se3[7], mcl_estimate* estimate, mcl_update_info* info);

/* ---- 2D NDT sensor model (sensor/ndt_sensor_model.hpp; beluga_amcl/src/ndt_amcl_node.cpp) ----------------------------------
 * A context created with sensor_kind = MCL_SENSOR_NDT takes its map from mcl_set_ndt_map instead of mcl_set_map: a sparse grid of
 * NDT cells (SparseValueGrid2<unordered_map<Vector2i, NDTCell2d>>) at one resolution, no origin.  mcl_update (and _laser_scan,
 * _point_cloud) then fits the measurement cells of the scan on the host (detail::to_cells, ndt_sensor_model.hpp:88-110) and weighs
 * every particle on the device: w *= 1 + sum over the measurement cells of
 *   max(sum over the kernel's offsets of the map cells present at cell_near(mu') + offset of d1 exp(-d2/2 e^T (S' + S_map)^-1 e),
 *       minimum_likelihood)
 * (operator() :216-226, likelihood_at :229-239, NDTCell::likelihood_at and SE2 * NDTCell: sensor/data/ndt_cell.hpp:49-68).
 * random_intersperse's random states are drawn from N(estimate of the normalised set) instead of uniformly over free cells
 * (ndt_amcl_node.cpp:248-254): estimated just before the draw, in cycles whose random state probability is > 0; a covariance the
 * normal distribution rejects returns MCL_ERR_BAD_COVARIANCE before the draw: as where the reference throws (amcl_core.hpp:182), the set
 * has then been propagated, reweighted and normalised and the recovery estimator and resample policy have advanced, but no particle
 * has been replaced and the estimator has not been reset.
 * Not on an NDT context (MCL_ERR_UNSUPPORTED): mcl_set_map[_async], mcl_initialize_from_map, mcl_get_likelihood_field_origin,
 * mcl_set_likelihood_field, comm attach and the sharded resampling steps (mcl_resample_targets, mcl_commit_routed,
 * mcl_finish_candidates); mcl_get_likelihood_field returns MCL_ERR_UNSUPPORTED and mcl_has_likelihood_field 0. */
#define MCL_NDT_MAX_OFFSETS 32
/* beluga::NDTModelParam2d (ndt_sensor_model.hpp:153-166). */
typedef struct mcl_ndt_params {
  double minimum_likelihood; /* 0 */
  double d1;                 /* 1 */
  double d2;                 /* 1 */
  uint32_t num_offsets;      /* 9: the 3 x 3 block of kDefaultNeighborKernel2d (:113-123), in its order */
  int32_t offsets[2 * MCL_NDT_MAX_OFFSETS]; /* (dx, dy) pairs */
} mcl_ndt_params;
/* Fills `params` with the reference struct's defaults (the node's are 0.01 / 1.0 / 0.6: ndt_amcl_node.cpp:87-107). */
void mcl_default_ndt_params(mcl_ndt_params* params);
/* NDTSensorModel's map (io::load_from_hdf5 layout): n cells with integer keys cells[n*2] (x, y), means[n*2] and covariances[n*4]
 * (2 x 2 row-major), at `resolution` metres per cell; params NULL = mcl_default_ndt_params.  Replaces the map between updates
 * (Amcl::update_map).  MCL_ERR_INVALID_ARGUMENT on a context of another sensor model, duplicate keys, no cells, a resolution that is
 * not positive and finite, values that are not finite, an asymmetric covariance, more than MCL_NDT_MAX_OFFSETS offsets or an offset
 * beyond 64 cells; MCL_ERR_UNSUPPORTED where the keys' bounding box (with a border of twice the kernel's reach) exceeds 2^26 cells
 * and the context's map layout is the dense one, the default: mcl_set_ndt_map_layout(ctx, 1) beforehand takes such a map as well. */
mcl_status mcl_set_ndt_map(mcl_ctx* ctx, const int32_t* cells, const double* means, const double* covariances, uint64_t n,
                           double resolution, const mcl_ndt_params* params);
/* detail::to_cells (ndt_sensor_model.hpp:66-110) of a scan in the base frame: points grouped by (p / resolution) truncated toward
 * zero, groups of fewer than 5 points dropped, each other group's mean and sample covariance (divided by n - 1, diagonal clamped to
 * >= 1e-5).  Cells in ascending (x, y) key order.  Pure host arithmetic.  means_out / covs_out hold B / 5 cells (2 and 4 doubles each). */
mcl_status mcl_ndt_measurement_cells(const double* points_xy, uint64_t num_points, double resolution, double* means_out,
                                     double* covs_out, uint64_t* num_cells);
/* Stage-level reweight from measurement cells fitted by the caller (means[k*2], covs[k*4] 2 x 2 row-major, base frame): w *= 1 +
 * sum over the cells of likelihood_at(state * cell).  mcl_reweight on an NDT context fits the cells of its points first. */
mcl_status mcl_reweight_ndt_cells(mcl_ctx* ctx, const double* means, const double* covs, uint64_t num_cells);
/* The small cycle of an NDT context, off by default.  on = 1: a cycle whose set and min(max_particles, capacity) are both at most 4096,
 * with the option small_fused on and stage profiling off, runs three launches and ONE host synchronisation, as a likelihood-field
 * filter of that size does - the propagation, a reweight with a wave per particle and its lanes over the measurement cells (every
 * weight bit for bit that of the lane-per-particle kernel), and the one-launch tail (normalisation, policies, resampling, estimate
 * sums).  One kind of cycle does not end inside the tail: one that resamples with a random state probability > 0.  The generator of
 * its random states, N(estimate of the normalised set), is the host's to build (amcl_core.hpp:182), so the tail stores the normalised
 * weights and the policies' scalars, draws nothing and hands the cycle back; the host then takes the steps of the ordinary cycle from
 * there on - the generator, the recovery filters' reset, the draw, the estimate.  The recovery filters, the every_n counter, the step
 * number and force_update end up where the ordinary cycle leaves them, a generator that is refused (MCL_ERR_BAD_COVARIANCE) included:
 * set propagated, reweighted and normalised, estimator and policy advanced, no particle replaced, estimator not reset.  Results agree
 * with the ordinary cycle's within the rounding of the tail's sums (as the likelihood-field small cycle's do).  mcl_reweight and
 * mcl_reweight_ndt_cells take the wave-per-particle kernel for sets of up to 4096 particles.  on = 0: everything as without the call.
 * MCL_ERR_UNSUPPORTED on a context of another sensor model, MCL_ERR_INVALID_ARGUMENT for a value other than 0 or 1.
 * mcl_get_ndt_small_cycle_counts: running totals of the small cycles that ended inside the tail and of those it handed back (either
 * pointer may be NULL).  In a batch (mcl_batch_update) a member with the switch on rides the fleet's shared launches: see there. */
mcl_status mcl_set_ndt_small_cycle(mcl_ctx* ctx, int32_t on);
mcl_status mcl_get_ndt_small_cycle(mcl_ctx* ctx, int32_t* on);
mcl_status mcl_get_ndt_small_cycle_counts(mcl_ctx* ctx, uint64_t* completed, uint64_t* handed_back);
/* How the NEXT map install (mcl_set_ndt_map, mcl_build_ndt_map_from_points / _from_grid) lays the map out on the device.
 *   0  dense, the default: an int32 index grid over the keys' bounding box; a box beyond 2^26 cells is MCL_ERR_UNSUPPORTED.
 *   1  automatic: the dense grid where the box fits 2^26 cells, the hashed table where it does not.
 *   2  hashed always.
 * The hashed table maps a key (int32 x, int32 y) to its cell by open addressing (a power of two of slots, load at most 1/2, linear
 * probing bounded by the longest probe of any stored key): memory in proportion to the cells, keys anywhere in the int32 range, as the
 * reference's SparseValueGrid2 over an unordered_map.  On every map that both layouts hold the weights are the same bits, and so is
 * everything that follows from them; mcl_get_ndt_map does not depend on the layout.  The installed map is never laid out again by this
 * call: the mode waits for the next install.  In a batch a member whose installed map is hashed runs its own cycle inside
 * mcl_batch_update and is not counted by mcl_ndt_batch_counts.
 * mcl_get_ndt_map_layout: *mode as set, *in_use what the installed map uses - 0 dense, 1 hashed, -1 no map (either pointer may be NULL).
 * MCL_ERR_UNSUPPORTED on a context of another sensor model, MCL_ERR_INVALID_ARGUMENT for any other mode. */
mcl_status mcl_set_ndt_map_layout(mcl_ctx* ctx, int32_t mode);
mcl_status mcl_get_ndt_map_layout(mcl_ctx* ctx, int32_t* mode, int32_t* in_use);

/* The map built on the device from what a user has at a cold start, a point cloud or an occupancy grid: detail::to_cells with
 * fit_points over the n points (world frame), the rule of mcl_ndt_measurement_cells - keys by (p / resolution) truncated toward zero,
 * cells of 5 points or more, mean and sample covariance with the diagonal clamped to >= 1e-5, cells in ascending (x, y) key order, a
 * cell's sums taken in input order: the cells equal mcl_ndt_measurement_cells' bit for bit.  The result becomes the context's map as if
 * passed to mcl_set_ndt_map, without a visit to the host; the model parameters are those of the last mcl_set_ndt_map on the context,
 * mcl_default_ndt_params if there was none.  MCL_ERR_UNSUPPORTED on a context of another sensor model, or where the kept cells' bounding
 * box (with its border) exceeds 2^26 cells under the dense map layout (the default; not under mcl_set_ndt_map_layout's modes 1 and 2,
 * where the kept cells' keys go into the hashed table on the device); MCL_ERR_INVALID_ARGUMENT for no points, a point that is not finite or whose key does not
 * fit an int32, a resolution that is not positive and finite, or an input without any cell of 5 points: the map is then kept as it was. */
mcl_status mcl_build_ndt_map_from_points(mcl_ctx* ctx, const double* points_xy, uint64_t n, double resolution);
/* The same from an occupancy grid (row-major int8 cells, grid_resolution metres per cell, origin as SE2 (cos, sin, x, y)): the points
 * are the centres of the occupied cells - value 100, the default value traits' occupied_value - in row-major order,
 * origin * (grid_resolution * (index + 0.5)). */
mcl_status mcl_build_ndt_map_from_grid(mcl_ctx* ctx, const int8_t* cells, uint32_t width, uint32_t height, double grid_resolution,
                                       const double origin[4], double ndt_resolution);
/* The context's map, however it was set, in mcl_set_ndt_map's formats (cells_out[n*2], means_out[n*2], covariances_out[n*4]); *n = its
 * cells.  The three arrays hold `capacity` cells each (MCL_ERR_INVALID_ARGUMENT if fewer than the map's); all three NULL: *n alone.
 * MCL_ERR_NOT_READY without a map. */
mcl_status mcl_get_ndt_map(mcl_ctx* ctx, int32_t* cells_out, double* means_out, double* covariances_out, uint64_t capacity, uint64_t* n);

/* ---- Landmark and bearing sensor models (sensor/landmark_sensor_model.hpp, sensor/bearing_sensor_model.hpp) -------------------
 * A context created with sensor_kind = MCL_SENSOR_LANDMARK or MCL_SENSOR_BEARING takes its map from mcl_set_landmark_map: a
 * beluga::LandmarkMap (sensor/data/landmark_map.hpp), 3D landmark positions with a category each, plus the map's boundaries.  The
 * measurement is a list of detections with a category each: positions in the robot frame (mcl_update_landmarks) or bearing vectors
 * in the sensor frame (mcl_update_bearings).  A particle (cos, sin, x, y) stands for the pose Rz(theta), (x, y, 0).  Per particle:
 *   landmark: w *= product over the detections of exp(-range_error^2 / (2 sigma_range^2)) exp(-bearing_error^2 / (2 sigma_bearing^2))
 *             + random_prob against the landmark of the detection's category nearest to the detection moved into the world
 *             (random_prob alone where the map has none of that category);
 *   bearing:  w *= product over the detections of exp(-e^2 / (2 sigma_bearing^2)), e the angle between the detection and the bearing,
 *             in the sensor frame, of the landmark of its category that maximises the dot product with the detection as given (0
 *             where the map has none of that category: the weight becomes 0).
 * Equal candidates resolve to the first in the map's order, as std::min_element does.  No detections leave the weights unchanged.
 * The reference has no node for these models; the library draws their random states (random_intersperse) and
 * mcl_initialize_from_map's states uniformly over the x-y extent of the map's boundaries with a uniform heading
 * (MultivariateUniformDistribution<SE2d, AlignedBox2d>): global localisation.
 * Not on these contexts (MCL_ERR_UNSUPPORTED): mcl_update, mcl_update_laser_scan, mcl_update_point_cloud, mcl_reweight, the entry
 * points of the other of the two kinds, mcl_set_map[_async], mcl_set_ndt_map, mcl_get_likelihood_field[_origin],
 * mcl_set_likelihood_field, comm attach and the sharded resampling steps; mcl_has_likelihood_field says 0.  The four entry points
 * below return MCL_ERR_UNSUPPORTED on a context of any other sensor model.  Every argument is checked before the device is used. */
/* Most detections one call takes (the bearing kernel keeps 12 bytes of LDS per detection and lane); more: MCL_ERR_INVALID_ARGUMENT. */
#define MCL_LANDMARK_MAX_DETECTIONS 64
/* beluga::LandmarkModelParam (landmark_sensor_model.hpp:44-48). */
typedef struct mcl_landmark_params {
  double sigma_range;   /* 1.0 */
  double sigma_bearing; /* 1.0 */
  double random_prob;   /* 1e-4 */
} mcl_landmark_params;
/* beluga::BearingModelParam (bearing_sensor_model.hpp:42-45). */
typedef struct mcl_bearing_params {
  double sigma_bearing;           /* 1.0 */
  double sensor_pose_in_robot[7]; /* identity; Sophus::SE3d::data() order: quaternion x, y, z, w, translation x, y, z */
} mcl_bearing_params;
void mcl_default_landmark_params(mcl_landmark_params* params);
void mcl_default_bearing_params(mcl_bearing_params* params);
/* The LandmarkMap: n landmarks positions_xyz[n*3] with categories[n]; boundaries = min x, y, z, max x, y, z (LandmarkMapBoundaries),
 * NULL = the landmarks' bounding box (the reference's second constructor).  params points at the struct of the context's kind
 * (mcl_landmark_params or mcl_bearing_params), NULL = its defaults.  Replaces the map between updates (update_map).  n = 0 with
 * explicit boundaries is a valid, empty map.  MCL_ERR_INVALID_ARGUMENT: n = 0 with NULL boundaries (the reference keeps Eigen's empty
 * box there, from which nothing can be drawn), values that are not finite, min > max in x or y, a sigma that is not positive and
 * finite or whose (2 sigma) sigma, the exponents' denominator, underflows to 0 or overflows (about sigma < 1.1e-162 or > 9.4e153: an
 * exact error of 0 would give 0 / 0, a NaN weight from finite inputs), a quaternion that is not finite or not of unit length within
 * 1e-9. */
mcl_status mcl_set_landmark_map(mcl_ctx* ctx, const double* positions_xyz, const uint32_t* categories, uint64_t n,
                                const double boundaries[6], const void* params);
/* Amcl::update with a std::vector<LandmarkPositionDetection> / <LandmarkBearingDetection>: n detections vectors_xyz[n*3] with
 * categories[n]; otherwise as mcl_update.  MCL_ERR_INVALID_ARGUMENT for more than MCL_LANDMARK_MAX_DETECTIONS detections or values
 * that are not finite. */
mcl_status mcl_update_landmarks(mcl_ctx* ctx, const double control_pose[4], const double* positions_xyz, const uint32_t* categories,
                                uint64_t n, mcl_estimate* estimate, mcl_update_info* info);
mcl_status mcl_update_bearings(mcl_ctx* ctx, const double control_pose[4], const double* bearings_xyz, const uint32_t* categories,
                               uint64_t n, mcl_estimate* estimate, mcl_update_info* info);

/* The small cycle of a landmark or bearing context, off by default.  on = 1: a cycle whose set and min(max_particles, capacity) are both
 * 1 .. 4096, with the option small_fused on and stage profiling off, runs three launches and ONE host synchronisation, as a
 * likelihood-field filter of that size does - the propagation (it pulls the staged detection records), a reweight with a wave per
 * particle (no launch where there is no detection), and the one-launch tail (normalisation, policies, resampling with the random states
 * drawn from the map's boundaries, estimate sums).  Nothing is handed back to the host.  The wave-per-particle kernels spread the
 * detections over the lanes: with P the smallest power of two >= k and g = 64 / P, detection j owns lanes [j g, (j + 1) g), lane r of
 * them scans the landmarks r, r + g, ... of the detection's category in ascending order (replacing on a strictly nearer landmark, or a
 * strictly larger dot product for the bearing model), and the group reduces with ties going to the smaller landmark index: the landmark
 * picked is the sequential scan's, the first of equal ones, and every weight is bit for bit that of the lane-per-particle kernels.  The
 * recovery filters, the every_n counter, the step number and force_update end up where the ordinary cycle leaves them; results agree
 * with the ordinary cycle's within the rounding of the tail's sums (as the likelihood-field small cycle's do).  The counter
 * small_tail_launches advances as on a likelihood-field context, landmark_wave_launches with every wave-per-particle reweight.
 * mcl_reweight_landmarks and mcl_reweight_bearings take the wave-per-particle kernels for sets of up to 4096 particles, and so does
 * the reweight of an update that is NOT the small cycle while the switch is on (small_fused off, stage profiling on, or
 * min(max_particles, capacity) above 4096 with a set of at most 4096): the same bits from the other kernel, inside the ordinary cycle;
 * landmark_wave_launches counts those launches too.  on = 0:
 * everything as without the call.  MCL_ERR_UNSUPPORTED on a context of another sensor model, MCL_ERR_INVALID_ARGUMENT for a value other
 * than 0 or 1.  In a batch (mcl_landmark_batch_update) a member with the switch on rides the fleet's shared launches: see there. */
mcl_status mcl_set_landmark_small_cycle(mcl_ctx* ctx, int32_t on);
mcl_status mcl_get_landmark_small_cycle(mcl_ctx* ctx, int32_t* on);
/* Stage-level reweight of the two models (what the two updates compose with the other stages below). */
mcl_status mcl_reweight_landmarks(mcl_ctx* ctx, const double* positions_xyz, const uint32_t* categories, uint64_t n);
mcl_status mcl_reweight_bearings(mcl_ctx* ctx, const double* bearings_xyz, const uint32_t* categories, uint64_t n);

/* ---- Stage-level entry points (what update() composes; used by parity tests and by the
 * multi-GPU driver, which interleaves collectives between them). -------------------------------- */

/* actions::propagate with DifferentialDriveModel::operator() (actions/propagate.hpp:57-79;
 * motion/differential_drive_model.hpp:129-164). `step` is the cycle counter word of the RNG stream. */
mcl_status mcl_propagate(mcl_ctx* ctx, const double pose[4], const double previous_pose[4], uint32_t step);
/* actions::reweight with the configured sensor model (actions/reweight.hpp:53-60;
 * likelihood_field_model.hpp:68-91 or beam_model.hpp:104-150): w[i] *= model(state[i]). */
mcl_status mcl_reweight(mcl_ctx* ctx, const double* points_xy, uint64_t num_points);

/* ---- The sensor model as a function: sensor_model(measurement)(state) at caller-given poses -------------------------------------
 * The reference's sensor models are functions - sensor_model(measurement) returns state -> weight, and states | views::likelihoods(model)
 * applies it to any range of states (views/likelihoods.hpp:44-59).  These entries are that: out[i] = the factor by which the matching
 * mcl_reweight* would multiply the weight of a particle at poses[i], for n poses (cos, sin, x, y) - mcl_set_particles' layout - in the
 * caller's order, anywhere on or off the map.  Scoring a list of candidate poses to relocalise, the current estimate as a quality
 * signal, a pose from another source before mcl_initialize_normal, a new map against a recorded scan.
 *
 * THE FILTER IS UNTOUCHED.  Particles, weights and count, step number and random stream, recovery filters, every_n counter,
 * force_update, control window, cached set facts, spatial order, the work the cycle keeps in flight and every counter of
 * mcl_get_counter are what they are on a context on which the call was never made.  The call has buffers of its own, runs on the
 * context's stream behind whatever is in flight, and reads the map the context reads NOW: a shared map, a hashed NDT map; a map
 * given by mcl_set_map_async counts from its swap on.  Allowed between the updates of a batch on its members, and on a sharded
 * context (the map is whole on every rank: no collective, every rank may ask on its own).
 *
 * mcl_likelihoods: likelihood-field, likelihood-field-prob, beam and NDT contexts (an NDT context fits the measurement cells of the
 * points first, as its mcl_reweight does); a beam context takes at most 4096 points here, whatever n is.  The other entries are the
 * counterparts of mcl_reweight_ndt_cells, mcl_reweight_landmarks and mcl_reweight_bearings.  poses and out are host memory, n doubles
 * out.  An empty measurement scores 1.0 where the reweight leaves the weights as they are.  The kernels are the reweight kernels' own
 * per-pose functions: NDT, landmark and bearing scores equal the reweight's factor bit for bit, likelihood-field and beam scores
 * within the rounding of the sum over the scan (the reweight picks among several kernel forms by the set it has).
 * Checks, all before the device is used; on any error out is not written: MCL_ERR_UNSUPPORTED on a context of another sensor model,
 * MCL_ERR_NOT_READY without a map, MCL_ERR_INVALID_ARGUMENT for a null argument, a pose with a value that is not finite, and whatever
 * the matching mcl_reweight* refuses of the measurement.  n == 0 is MCL_OK and does nothing.  n is limited by memory only. */
mcl_status mcl_likelihoods(mcl_ctx* ctx, const double* poses, uint64_t n, const double* points_xy, uint64_t num_points, double* out);
mcl_status mcl_likelihoods_ndt_cells(mcl_ctx* ctx, const double* poses, uint64_t n, const double* means, const double* covs, uint64_t num_cells,
                                     double* out);
mcl_status mcl_likelihoods_landmarks(mcl_ctx* ctx, const double* poses, uint64_t n, const double* positions_xyz, const uint32_t* categories,
                                     uint64_t k, double* out);
mcl_status mcl_likelihoods_bearings(mcl_ctx* ctx, const double* poses, uint64_t n, const double* bearings_xyz, const uint32_t* categories,
                                    uint64_t k, double* out);
/* mcl_likelihoods with d_poses and d_out in device memory of the context's device (points_xy stays host memory): enqueued on the
 * context's stream, no host synchronisation beyond the measurement's upload (the call waits for the PREVIOUS call's upload before it
 * stages its own) - synchronise the stream, or order your own work behind it, before reading d_out.  The poses are not looked at on
 * the host: a pose that is not finite scores whatever the arithmetic gives. */
mcl_status mcl_likelihoods_device(mcl_ctx* ctx, const double* d_poses, uint64_t n, const double* points_xy, uint64_t num_points, double* d_out);

/* ---- Global pose search: score every free cell and heading with the sensor model, keep the best -------------------------------------
 * Localising without an initial guess (a kidnapped robot, a start without a pose, "is there a better place than where the filter
 * sits"): the candidates are made on the device, scored there by mcl_likelihoods' kernels, and only the winners come back.  Contexts of
 * a grid sensor model (likelihood field, likelihood-field prob, beam) with a map.  tests/search_reference.py restates all of this.
 *
 * Candidate cells: the map's free cells (those mcl_initialize_from_map draws from) whose x % cell_stride == 0 && y % cell_stride == 0.
 * Headings: theta_h = -pi + h * (2 pi / headings), h < headings <= 4096; the rotation (cos, sin) of each heading is computed once per
 *   call on the host and uploaded as a table: every candidate of heading h carries the same bits.
 * Position: the centre of the cell in the world, by the expressions the random states of mcl_initialize_from_map use:
 *   (x + 0.5) * resolution, rotated by the origin, + the origin.
 * Candidate id: linear_cell_index * headings + h.  Every order and every tie below is decided by the id: the result does not depend on
 *   the chunking (option search_chunk), on the order of the compaction or on the launch geometry.
 * Score: score(id) is what mcl_likelihoods returns for that pose and that measurement, bit for bit (the same kernels, the same order
 *   of the sum over the scan).  The measurement's checks and staging are mcl_likelihoods' own: at most 4096 points on a beam context,
 *   a point that is not finite has no cell for any pose.
 * Pool: the `pool` (1 .. 4096) candidates that come first by (score descending, id ascending).  A NaN score cannot arise from finite
 *   poses; it is defined as the lowest, so that the order is total.
 * Suppression: greedy, in pool order, on the host.  A candidate is kept unless an already kept one lies within separation_cells of it
 *   AND within separation_headings of it: dx*dx + dy*dy <= separation_cells * separation_cells in integer cell coordinates, and
 *   min(|dh|, headings - |dh|) <= separation_headings.  Integers only, so the rule is exact.  With both separations 0 only a candidate
 *   identical to a kept one would be dropped, which cannot happen: nothing is dropped.  It stops after max_results (1 .. pool) kept.
 *
 * The filter is untouched, by mcl_likelihoods' own contract: the call has buffers of its own, runs on the context's stream and reads the
 * map the filter holds through the views the reweight reads, as they are now - a shared map (mcl_use_shared_map) as well; a map given
 * by mcl_set_map_async counts from its swap on.  Allowed between the updates of a batch on its members, and on a sharded context on
 * each rank by itself (the map is whole on every rank: no collective).
 *
 * Device memory is bounded by the chunk (option search_chunk: 64 .. 2^22 candidates, default 2^20), not by the number of candidates.
 * At most one host synchronisation per chunk, and one at the end.
 *
 * Checks, all before the device is used; on any error no output is written: MCL_ERR_UNSUPPORTED on NDT, landmark and bearing contexts,
 * MCL_ERR_NOT_READY without a map, MCL_ERR_INVALID_ARGUMENT for a null argument, cell_stride == 0, headings or pool outside 1 .. 4096,
 * max_results outside 1 .. pool, capacity < max_results (mcl_global_search_pool: < pool), and whatever mcl_likelihoods refuses of the
 * measurement.  A map with no candidate cell is MCL_OK with count == 0. */
typedef struct mcl_search_params {
  uint32_t cell_stride, headings, pool, max_results, separation_cells, separation_headings;
} mcl_search_params;
typedef struct mcl_search_hit {
  double pose[4]; /* cos, sin, x, y: mcl_set_particles' layout */
  double score;
  uint64_t id;
  uint32_t cell, heading; /* id = cell * headings + heading; cell = y * width + x */
} mcl_search_hit;
typedef struct mcl_search_info {
  uint64_t cells;       /* candidate cells */
  uint64_t candidates;  /* cells * headings */
  uint64_t pool_filled; /* min(pool, candidates) */
  uint32_t chunks;      /* ranges of the free-cell list the call went through: ceil(free cells / max(1, search_chunk / headings)) */
  uint32_t launches;    /* kernel launches of the call: its own kernels, and one per chunk for the scoring (a chunk's candidates are one
                           launch of mcl_likelihoods_device's kernel); copies and fills of the stream are not counted */
} mcl_search_info;
/* cell_stride 2, headings 72 (5 degrees), pool 1024, max_results 16, separation_cells 10, separation_headings 6 (30 degrees): choices
 * of a reasonable start, not measurements. */
void mcl_default_search_params(mcl_search_params* params);
/* The hits that survive the suppression, best first; params NULL: the defaults; info may be NULL. */
mcl_status mcl_global_search(mcl_ctx* ctx, const double* points_xy, uint64_t num_points, const mcl_search_params* params, mcl_search_hit* hits,
                             uint64_t capacity, uint64_t* count, mcl_search_info* info);
/* The pool before the suppression, in pool order (capacity >= pool). */
mcl_status mcl_global_search_pool(mcl_ctx* ctx, const double* points_xy, uint64_t num_points, const mcl_search_params* params, mcl_search_hit* hits,
                                  uint64_t capacity, uint64_t* count, mcl_search_info* info);
/* The candidates themselves, as the device makes them, in id order: those of rank first_id_rank .. first_id_rank + count - 1 (fewer
 * where the list ends) into ids_out and poses_out (4 doubles each; host memory; either may be NULL with count == 0); *total = the
 * number of candidates.  Only cell_stride and headings of the parameters matter, all are checked. */
mcl_status mcl_global_search_candidates(mcl_ctx* ctx, const mcl_search_params* params, uint64_t first_id_rank, uint64_t count, uint64_t* ids_out,
                                        double* poses_out, uint64_t* total);
/* The suppression alone, on the host: needs no device and no context.  pool: n hits in pool order (cell and heading are read),
 * grid_width: the map's width in cells; kept_index (room for max_results): the pool indices of the kept hits, *kept their number.
 * MCL_ERR_INVALID_ARGUMENT: a null argument, grid_width == 0, parameters mcl_global_search refuses, a heading >= headings. */
mcl_status mcl_search_suppress(const mcl_search_hit* pool, uint64_t n, uint32_t grid_width, const mcl_search_params* params, uint32_t* kept_index,
                               uint64_t* kept);

/* ---- Local pose search: a lattice of offsets about each seed pose, the best of it and the response's moments ---------------------------
 * The correlative scan matcher: refine a hit of mcl_global_search below its quantisation, "look around the current estimate for a
 * better pose", and learn how well the measurement pins the pose there (tight across a corridor, loose along it).  It needs no map
 * cells, only seeds: every sensor model has it.  tests/local_search_reference.py restates all of this.
 *
 * Parameters: half_steps_xy (Kx) <= 32, half_steps_theta (Kt) <= 64, both steps finite, step_theta > 0, step_xy >= 0, Kt * step_theta
 *   < pi.  step_xy == 0 stands for a quarter of the map's cell size - the grid's resolution on grid contexts, the NDT map's on NDT
 *   contexts; a landmark or bearing context has no cell size and refuses it.
 * Lattice: a seed has L = (2 Kx + 1)^2 (2 Kt + 1) candidates (at most 545 025), the integer triples (i, j, k), |i|, |j| <= Kx, |k| <= Kt;
 *   the local id of one is ((k + Kt) (2 Kx + 1) + (j + Kx)) (2 Kx + 1) + (i + Kx).
 * Position: x = seed.x + off[i], y = seed.y + off[j] in world axes; off[i] = double(i) * step_xy is computed once per call on the
 *   host and uploaded: the device does one addition per coordinate.
 * Rotation: from a table of n (2 Kt + 1) entries computed on the host and uploaded; the entry for k is the seed's rotation times
 *   exp(double(k) * step_theta) by SO(2)'s product as the library forms it everywhere (renormalised, then normalised with hypot); the
 *   entry for k == 0 is the seed's rotation as given.  Every candidate's bits are the host's, and the centre candidate is the seed bit
 *   for bit.
 * Score: score(seed, id) is what mcl_likelihoods* returns for that pose and that measurement, bit for bit (the same kernels, as the
 *   global search's; a beam context with a range table walks all the same).
 * Best: the candidate that comes first by (score descending, i*i + j*j ascending, |k| ascending, id ascending) - integers only behind
 *   the score, whose order is that of its bits' order-preserving image (a NaN, which finite poses cannot give, is the lowest).  A
 *   likelihood field is constant over a cell, so plateaus of equal scores are the normal case: the rule pulls towards the seed, not
 *   towards a corner.  plateau = the candidates whose score equals the best's bit for bit.
 * Moments: ten f64 sums per seed with w = score, in integer offset coordinates: S0 = sum w; sum w i, sum w j, sum w k; sum w ii, w ij,
 *   w ik, w jj, w jk, w kk (sums[0 .. 9] in this order); a term is the score times the integer product, rounded once.  The order of the summation is fixed by L and the launch geometry alone: the
 *   same call gives the same bits, whatever option search_chunk is.
 * Finish (on the host; mcl_local_search_finish is this alone): m_a = S_a / S0; mean_dx = step_xy * m_i, mean_dy = step_xy * m_j,
 *   mean_dtheta = step_theta * m_k; cov[a][b] = ((S_ab / S0 - m_a * m_b) * step_a) * step_b, symmetric, (x, y, theta) order; mean_pose =
 *   (seed.x + mean_dx, seed.y + mean_dy, seed rotation times exp(mean_dtheta)).  moments_valid = 0 where S0 is 0 or not finite: the
 *   mean is then the seed as given and the covariance zero.
 * pose of a hit: formed on the host from the id by the expressions above, as the global search forms its hits.
 *
 * The filter is untouched, by mcl_likelihoods' own contract: the call has buffers of its own, runs on the context's stream and reads
 * the map the context reads now.  Allowed on batch members, on contexts attached to a shared map, and per rank on a sharded context.
 * Device memory: a pass takes max(1, search_chunk / L) whole seeds, its buffers hold max(search_chunk, L) candidates; a seed is never
 * split and the result does not depend on search_chunk.  Per seed the call keeps its table entries and 14 words of results.  One host
 * synchronisation, at the end of the call.
 *
 * Checks, all before the device is used; on any error nothing is written: MCL_ERR_NOT_READY without a map; MCL_ERR_INVALID_ARGUMENT
 * for a null argument, a seed value that is not finite, parameters outside the limits above and whatever mcl_likelihoods* refuses of
 * the measurement; MCL_ERR_UNSUPPORTED for the entry of another sensor model, as mcl_likelihoods*.  n == 0 is MCL_OK. */
typedef struct mcl_local_search_params {
  uint32_t half_steps_xy, half_steps_theta;
  double step_xy, step_theta;
} mcl_local_search_params;
typedef struct mcl_local_hit {
  double pose[4];      /* the best candidate: cos, sin, x, y */
  double score;        /* its score */
  double seed_score;   /* the centre candidate's: mcl_likelihoods at the seed */
  int32_t di, dj, dk;  /* its integer offsets */
  int32_t moments_valid;
  uint64_t plateau;    /* candidates whose score equals `score` bit for bit */
  double mean_pose[4];
  double cov[9];       /* row-major, (x, y, theta) */
  double sums[10];
} mcl_local_hit;
typedef struct mcl_local_search_info {
  uint64_t candidates_per_seed; /* L */
  uint64_t seeds_per_pass;      /* max(1, search_chunk / L) */
  uint32_t passes;              /* ceil(n / seeds_per_pass) */
  uint32_t launches;            /* kernel launches: per pass one generation, one scoring (mcl_likelihoods_device's kernel), one reduction */
  double step_xy;               /* the step used: the parameter, or a quarter of the map's cell size */
} mcl_local_search_info;
/* half_steps_xy 4, half_steps_theta 5, step_xy 0 (a quarter of a cell), step_theta pi / 360: plus or minus one cell and plus or minus
 * 2.5 degrees, half of the global search's default quantisation in each axis.  Choices of a reasonable start, not measurements. */
void mcl_default_local_search_params(mcl_local_search_params* params);
/* seeds: n poses (cos, sin, x, y); hits: room for n; params NULL: the defaults; info may be NULL.  Likelihood-field,
 * likelihood-field-prob, beam and NDT contexts. */
mcl_status mcl_local_search(mcl_ctx* ctx, const double* seeds, uint64_t n, const double* points_xy, uint64_t num_points,
                            const mcl_local_search_params* params, mcl_local_hit* hits, mcl_local_search_info* info);
/* The same on landmark and bearing contexts, with the measurement of mcl_likelihoods_landmarks / mcl_likelihoods_bearings. */
mcl_status mcl_local_search_landmarks(mcl_ctx* ctx, const double* seeds, uint64_t n, const double* positions_xyz, const uint32_t* categories,
                                      uint64_t k, const mcl_local_search_params* params, mcl_local_hit* hits, mcl_local_search_info* info);
mcl_status mcl_local_search_bearings(mcl_ctx* ctx, const double* seeds, uint64_t n, const double* bearings_xyz, const uint32_t* categories,
                                     uint64_t k, const mcl_local_search_params* params, mcl_local_hit* hits, mcl_local_search_info* info);
/* The lattice of one seed as the device makes it, in id order: the candidates first .. first + count - 1 (fewer where the lattice
 * ends) into poses_out (4 doubles each; host memory; may be NULL with count == 0); *total = L.  Every sensor model. */
mcl_status mcl_local_search_candidates(mcl_ctx* ctx, const double seed[4], const mcl_local_search_params* params, uint64_t first, uint64_t count,
                                       double* poses_out, uint64_t* total);
/* The moments' finish alone, on the host: needs no device and no context.  params NULL: the defaults; its step_xy is used as given (0
 * is a step of no length, not a quarter of a cell: there is no map here).  MCL_ERR_INVALID_ARGUMENT: a null argument, a seed value that
 * is not finite, parameters mcl_local_search refuses. */
mcl_status mcl_local_search_finish(const double sums[10], const mcl_local_search_params* params, const double seed[4], double mean_pose[4],
                                   double cov[9], int32_t* moments_valid);

/* ---- Ray casting as a function: the range the map predicts along a bearing from a pose (Ray2d::cast, algorithm/raycasting.hpp:97-107) ----
 * An expected scan to draw over the measured one, per-beam residuals against a stale map or a moving obstacle, a synthetic scan for a
 * simulated robot, a range table.  The walk is the beam model's own (the kernels mcl_reweight runs on a beam context), opened to
 * caller-given poses and bearings.  Likelihood-field, likelihood-field-prob and beam contexts with a map.  tests/raycast_reference.py
 * restates all of this.
 *
 * For pose i (cos, sin, x, y: mcl_set_particles' layout), bearing b = (c, s) of bearings_cs[2 b], [2 b + 1] - a unit vector as the caller
 * gives it, never normalised here - and max_range:
 *   T = origin^-1 * pose, as the beam model forms it.
 *   source cell: floor(T.x * (1 / resolution)), floor(T.y * (1 / resolution)).
 *   far end: T * (c * max_range, s * max_range), every product and sum rounded on its own; its cell likewise.
 *   trace: the standard Bresenham line from the source cell to the far-end cell (bresenham.hpp:84-160).  It stops at the first cell outside
 *     the grid (no hit), at the first cell that is not free (hit: an unknown cell is not free), or behind the far-end cell (no hit).
 *   ranges_out[i * B + b] = fmin(the distance of the two cells' centres (xi + 0.5) * resolution, max_range); max_range without a hit.
 *   hit_cells_out[i * B + b] = y * width + x of the hit cell, or -1.  May be NULL.
 *   *cells_visited = the cells looked at, summed over all rays: those of a trace inside the grid, up to and including the hit.  May be NULL.
 *   Out of reach: a ray whose source cell is at or beyond 2^30 in magnitude along an axis is no hit and visits no cell (no grid that fits
 *     in memory has such a cell, so this is the rule above); so is a ray whose line spans 2^27 cells or more along an axis, which takes a
 *     bearing or a pose rotation that is no unit vector.  Both are decided on the doubles, before any conversion to an integer: no input
 *     forms an address outside a buffer.
 * With bearings (px / z, py / z), z = sqrt(px^2 + py^2), of scan points and the model's beam_max_range, ranges_out is the expected range
 * the beam model compares each measured range with, bit for bit.  A beam context walks its packed bit maps, a likelihood-field context
 * the cells themselves: the three outputs are the same.
 *
 * THE FILTER IS UNTOUCHED, by mcl_likelihoods' own contract: the call has buffers of its own, runs on the context's stream behind
 * whatever is in flight, writes nothing the cycle reads and moves no counter of mcl_get_counter (mcl_beam_cells_visited included: the
 * count above is the call's own).  It reads the map the context reads NOW - a shared map as well; a map given by mcl_set_map_async counts
 * from its swap on.  Allowed between the updates of a batch on its members, and on a sharded context on each rank by itself.
 *
 * n and num_bearings are limited by memory only (the 4096 points of mcl_likelihoods on a beam context do not apply).  The host form's
 * device memory is the bearing table (16 bytes per bearing) and one chunk of rays: option cast_chunk, 64 .. 2^28 rays, default 2^22 -
 * 16 bytes per ray and up to 32 per ray for the poses of a table shorter than a chunk.  The result does not depend on it.  The host form
 * synchronises once per chunk.
 *
 * Checks, all before the device is used; on any error no output is written: MCL_ERR_UNSUPPORTED on NDT, landmark and bearing contexts;
 * MCL_ERR_NOT_READY without a map; MCL_ERR_INVALID_ARGUMENT for a max_range that is not finite or not positive, max_range / resolution
 * at or above 2^27 - 2 cells (the bound of mcl_reweight on a beam context), a null poses, bearings_cs or ranges_out, a pose or bearing
 * value that is not finite; MCL_ERR_OUT_OF_MEMORY for counts no memory holds (n above 2^40, num_bearings above 2^36, n * num_bearings
 * above 2^62).  n == 0 or num_bearings == 0 is MCL_OK and writes nothing but *cells_visited = 0 (the context and max_range are checked
 * all the same). */
mcl_status mcl_cast_rays(mcl_ctx* ctx, const double* poses, uint64_t n, const double* bearings_cs, uint64_t num_bearings, double max_range,
                         double* ranges_out, int64_t* hit_cells_out /* NULL ok */, uint64_t* cells_visited /* NULL ok */);
/* mcl_cast_rays with d_poses, d_ranges_out and d_hit_cells_out (NULL ok) in device memory of the context's device; bearings_cs and
 * cells_visited stay host memory.  Enqueued on the context's stream; the call waits for the PREVIOUS call's upload of the bearings before
 * it stages its own, and synchronises the stream only where cells_visited is given - otherwise synchronise, or order your own work behind
 * it, before reading the outputs.  The poses are not looked at on the host: one that is not finite is out of reach.  cast_chunk does not
 * apply (the outputs are the caller's); a launch holds 2^38 rays. */
mcl_status mcl_cast_rays_device(mcl_ctx* ctx, const double* d_poses, uint64_t n, const double* bearings_cs, uint64_t num_bearings, double max_range,
                                double* d_ranges_out, int64_t* d_hit_cells_out /* NULL ok */, uint64_t* cells_visited /* NULL ok */);

/* ---- Range table for the beam model: the expected range as one look-up per beam in place of a walk ---------------------------------
 * The exact rule's expected range depends on the source cell and the far-end cell alone.  With the ray's heading in the GRID frame
 * quantised to A bins it becomes a table over (cell, bin) - what MIT's rangelibc calls a look-up table.  An APPROXIMATION, hence opt-in:
 * a context without a table is byte for byte what it was.  tests/range_table_reference.py restates all of this.
 *
 * The table (the context's own, one per map x beam_max_range x A - even on a shared map): uint32 table[(y * width + x) * A + k] = the
 * squared cell distance (hx - x)^2 + (hy - y)^2 between cell (x, y) and the cell the exact rule's cast from it hits, 0xFFFFFFFF without a
 * hit (a distance of 65 536 cells or more is stored as 0xFFFFFFFE).  The cast of entry (x, y, k), all in the grid frame:
 *   far end ((x + 0.5) * resolution + c_k * max_range, (y + 0.5) * resolution + s_k * max_range), every product and sum rounded on its
 *     own; its cell floor(v * (1 / resolution)); source cell (x, y); max_range = the context's beam_max_range;
 *   the walk of mcl_cast_rays (standard Bresenham; stops at the first cell outside the grid, not free, or behind the far end).
 *   (c_k, s_k) = std::cos, std::sin of double(k) * (2 pi / A), computed on the host, uploaded, kept: mcl_range_table_bearings.
 * WHAT IT DISCARDS of the exact rule: the source's position inside its cell (the cast starts at the centre), and the heading within a bin.
 *
 * The bin of a beam (the reweight's rule).  Per particle: src = origin^-1 * pose and its cell (sx, sy) as the exact path forms them,
 * theta = atan2(src.r.s, src.r.c).  Per scan point: beta = atan2(py, px).  u = (theta + beta) * (A / (2 pi)); k = floor(u + 0.5) reduced
 * into [0, A).  The entry is table[(sy * width + sx) * A + k], or "no hit" for a source cell outside the grid (exact: the walk's first
 * cell is outside).  The expected range is fmin(sqrt(r2) * resolution, max_range), max_range without a hit; the mixture from there on is
 * the beam model's, with `measured < expected` decided on that value (the exact path's re-derivation of a tie from the two cell centres
 * has no hit cell to work with here).
 *
 * With a table built: mcl_update, mcl_reweight, mcl_likelihoods and mcl_likelihoods_device of the context read it (mcl_likelihoods stays
 * "the factor a reweight would apply"); one kernel serves every set size, for scans of up to 4096 points (a larger one is
 * MCL_ERR_INVALID_ARGUMENT while a table is built).  mcl_cast_rays* stays the exact caster and mcl_global_search*
 * stays on the exact walk.  mcl_beam_cells_visited does not move: nothing is walked.  A member of a batch with a table runs its own
 * cycle inside mcl_batch_update, whatever batch_beam_fused says.  On a sharded context the build is a LOCAL call that every rank makes
 * for itself; the library does not compare it across ranks.
 *
 * mcl_build_range_table builds the table of the current map on the device (synchronises the stream) and switches the cycle over from
 * the next reweight on; called again it replaces the table (another A).  Whatever installs a map afterwards - mcl_set_map, the swap of a
 * map given by mcl_set_map_async (inside mcl_update or mcl_map_commit), mcl_use_shared_map - REBUILDS the table inside that call, so a
 * context with a table never walks silently; a rebuild that fails drops the table (built == 0, the exact walk again) and its status is
 * that call's.  Memory: width * height * A * 4 bytes, refused with MCL_ERR_OUT_OF_MEMORY before anything is allocated above option
 * range_table_max_bytes (default 4 GiB).  Other refusals, MCL_ERR_INVALID_ARGUMENT: a context that is no beam context (a
 * likelihood-field cycle would never read the table), num_angles outside 1 .. 4096, beam_max_range / resolution at or above 2^27 - 2
 * cells; MCL_ERR_NOT_READY without a map.  Every refusal leaves the filter and a table it already has as they were. */
typedef struct mcl_range_table_info {
  int32_t built;         /* 1: the cycle reads a table */
  uint32_t num_angles;   /* A */
  uint32_t width, height;
  uint64_t bytes;        /* of the table in device memory */
  uint64_t builds;       /* tables built on this context since mcl_create, rebuilds included */
  uint64_t lut_launches; /* reweights of the cycle that read a table: one per reweight */
} mcl_range_table_info;
mcl_status mcl_build_range_table(mcl_ctx* ctx, uint32_t num_angles);
/* Back to the exact walk; the memory is freed.  MCL_OK without a table. */
mcl_status mcl_drop_range_table(mcl_ctx* ctx);
mcl_status mcl_range_table_get_info(mcl_ctx* ctx, mcl_range_table_info* info);
/* cs_out[2 k], [2 k + 1] = (c_k, s_k), 2 * A doubles: the bearings the table was built with.  MCL_ERR_NOT_READY without a table. */
mcl_status mcl_range_table_bearings(mcl_ctx* ctx, double* cs_out);
/* out[(c - first_cell) * A + k] = the entries of cells first_cell .. first_cell + num_cells - 1 (cell = y * width + x); synchronises the
 * stream.  MCL_ERR_NOT_READY without a table, MCL_ERR_INVALID_ARGUMENT for cells beyond the grid. */
mcl_status mcl_range_table_read(mcl_ctx* ctx, uint64_t first_cell, uint64_t num_cells, uint32_t* out);

/* ---- Beam skipping (Nav2 AMCL's do_beamskip) for the likelihood-field models ----------------------------------------------------
 * A beam that hits something the map does not know - a person, a pallet, an open door - pulls the weight of EVERY particle down
 * together and flattens the posterior.  With beam skipping the cloud votes on each beam before the reweight: beams that too few
 * particles can explain are left out of this update.  The vote is per beam over ALL live particles, unweighted - which a sensor
 * model that is a function of one state cannot express (the reference has none) and a device that visits the (particle x beam)
 * grid anyway takes as one integer reduction.  MCL_SENSOR_LIKELIHOOD_FIELD and MCL_SENSOR_LIKELIHOOD_FIELD_PROB only.
 *
 * level: the value the field builder gives a cell at squared distance float(distance * distance) from the nearest obstacle,
 *   float(amplitude * exp(-double(float(distance^2)) / (2 sigma_hit^2)) + z_random / max_laser_distance), from the context's
 *   mcl_lf_params - parameters only, never the map.
 * agreement: a point of the scan AGREES with a pose iff its end-point's cell - the cell the reweight reads, mcl_reweight's exact
 *   rule - is inside the grid and field[cell] > level, strictly, on the field mcl_get_likelihood_field returns NOW: host-built,
 *   device-built, given by mcl_set_likelihood_field, shared, swapped in by mcl_set_map_async.  Off the grid: no.  A point with a
 *   NaN or infinite coordinate agrees with no pose.
 * count[b]: the live particles beam b agrees with, taken behind the propagation and in front of the reweight.
 * decision (n live particles, B points): kept[b] = double(count[b]) / double(n) > threshold; skipped = B - sum kept;
 *   used_all = B > 0 && double(skipped) / double(B) >= error_threshold.  used_all: too much of the scan disagrees with the cloud, the
 *   cloud is probably wrong, and the whole scan is used (Nav2's rule).
 * reweight: with used_all, or disabled, everything is as without the feature.  Otherwise the weights are those mcl_reweight gives for
 *   the kept points alone, in the caller's order, bit for bit (the same staging, kernel choice and order of the sum).
 * Applies to mcl_update, mcl_update_laser_scan, mcl_update_point_cloud, mcl_reweight and to a member's cycle in mcl_batch_update
 * (such a member runs its own cycle: it counts in members_alone; the results are its lone mcl_update's).  mcl_likelihoods* ignore
 * it.  An enabled cycle costs one launch and ONE more host synchronisation between the propagation and the reweight; a disabled one
 * nothing at all. */
typedef struct mcl_beam_skip_params {
  int32_t enabled;        /* 0 (do_beamskip) */
  int32_t reserved0;
  double distance;        /* 0.5 m (beam_skip_distance): how far from an obstacle an end-point may land and still agree */
  double threshold;       /* 0.3 (beam_skip_threshold): share of the particles a kept beam must agree with, exceeded strictly */
  double error_threshold; /* 0.9 (beam_skip_error_threshold): share of skipped beams from which on the whole scan is used */
} mcl_beam_skip_params;
void mcl_default_beam_skip_params(mcl_beam_skip_params* params);
/* Allowed between updates, on batch members and on contexts attached to a shared map.  MCL_ERR_UNSUPPORTED on a beam, NDT, landmark
 * or bearing context, and for enabled = 1 on a context attached to a communicator of several ranks (the counts are not exchanged
 * yet: mcl_comm_attach* with world > 1 on an enabled context is refused likewise, before any collective);
 * MCL_ERR_INVALID_ARGUMENT for a value outside its range or not finite.  A refused call leaves the old parameters in place. */
mcl_status mcl_set_beam_skip(mcl_ctx* ctx, const mcl_beam_skip_params* params);
mcl_status mcl_get_beam_skip(mcl_ctx* ctx, mcl_beam_skip_params* params);
typedef struct mcl_beam_skip_result {
  int32_t valid;          /* an enabled update or reweight has taken a decision (cleared by mcl_set_beam_skip) */
  int32_t used_all;       /* the whole scan was used after all */
  uint64_t num_beams;     /* B: the caller's points */
  uint64_t num_particles; /* n: the live particles that voted */
  uint64_t num_skipped;   /* beams the vote skipped (with used_all they were used all the same) */
  double level;           /* the level, widened */
} mcl_beam_skip_result;
/* The last decision taken by an update or a reweight of this context; counts[b] and kept[b] (1 / 0) by the caller's points, capacity
 * entries each, either may be NULL.  MCL_ERR_INVALID_ARGUMENT if capacity < num_beams with an array given.  Without a decision yet:
 * valid = 0, level filled in, nothing written to the arrays. */
mcl_status mcl_get_beam_skip_result(mcl_ctx* ctx, mcl_beam_skip_result* result, uint32_t* counts, uint8_t* kept, uint64_t capacity);
/* The function form: counts[b], b < num_points, of the CURRENT set for a scan - which beams of this scan does the filter think are
 * not the map?  A dynamic-obstacle mask, a filtered scan for a costmap.  Uses the context's distance whether enabled or not.
 * THE FILTER IS UNTOUCHED.  Particles, weights and count, step number and random stream, recovery filters, every_n counter,
 * force_update, control window, cached set facts, spatial order, the work the cycle keeps in flight and every counter of
 * mcl_get_counter are what they are on a context on which the call was never made.  The call has buffers of its own, runs on the
 * context's stream behind whatever is in flight, and reads the map the context reads NOW.  (Its own counter, beam_agreement_calls,
 * apart.)  MCL_ERR_NOT_READY without a map or without particles; num_points == 0 is MCL_OK and does nothing. */
mcl_status mcl_beam_agreement(mcl_ctx* ctx, const double* points_xy, uint64_t num_points, uint32_t* counts);

typedef struct mcl_weight_stats {
  double sum;        /* sum of weights before normalisation (actions/normalize.hpp:70) */
  double norm_sum;   /* sum of the normalised weights (the Thrun estimator's total, Q1) */
  double norm_sumsq; /* sum of squared normalised weights: ESS = norm_sum^2 / norm_sumsq */
} mcl_weight_stats;
/* Local sums of this shard's weights, no normalisation (multi-GPU: all-reduce `sum` first). */
mcl_status mcl_weight_sum(mcl_ctx* ctx, double* sum);
/* actions::normalize (actions/normalize.hpp:54-85) by `factor` (NaN => this shard's own sum) and
 * the statistics the policies consume (effective_sample_size.hpp:46-59, thrun_..._estimator.hpp:79-80). */
mcl_status mcl_normalize(mcl_ctx* ctx, double factor, mcl_weight_stats* stats);

/* views::sample | random_intersperse | take_while_kld | actions::assign (amcl_core.hpp:188-196).
 * New weights are 1 (type_traits/particle_traits.hpp:105). */
mcl_status mcl_resample(mcl_ctx* ctx, double random_state_probability, uint32_t step, uint64_t* n_out);

/* Sufficient statistics of beluga::estimate (algorithm/estimation.hpp:436-475) for this shard:
 * {Sw, Sw2, Sw*c, Sw*s, Sw*dx, Sw*dy, Sw*dx*dx, Sw*dx*dy, Sw*dy*dy, pivot_x, pivot_y, 0} with
 * dx = x - pivot_x.  Sums over shards are additive when every shard uses the same pivot. */
mcl_status mcl_estimate_sums(mcl_ctx* ctx, const double pivot_xy[2], double sums[12]);
/* Finishes the estimate from (all-reduced) sums. Pure host arithmetic. */
mcl_status mcl_estimate_from_sums(const double sums[12], mcl_estimate* out);
/* Convenience: single-shard estimate (estimation.hpp:436-475). */
mcl_status mcl_estimate_pose(mcl_ctx* ctx, mcl_estimate* out);

/* beluga::cluster_based_estimate (algorithm/cluster_based_estimation.hpp:415-433) — what beluga_ros::Amcl::update
 * returns (beluga_ros/src/amcl.cpp:125): particles are grouped into clusters around local maxima of the cell-averaged
 * weight; the mean and covariance of the cluster with the highest total weight are returned, or the overall estimate
 * if no cluster has more than one particle.  ParticleClusterizerParam :243-259 defaults: 0.20 m, 0.524 rad, 0.90. */
typedef struct mcl_cluster_params {
  double linear_hash_resolution;
  double angular_hash_resolution;
  double weight_cap_percentile;
} mcl_cluster_params;
mcl_status mcl_cluster_based_estimate(mcl_ctx* ctx, const mcl_cluster_params* params /* NULL: defaults */, mcl_estimate* out);
/* Selects what mcl_update returns: 0 = beluga::estimate (beluga::Amcl), 1 = cluster_based_estimate (beluga_ros::Amcl). */
mcl_status mcl_set_estimate_kind(mcl_ctx* ctx, int32_t kind, const mcl_cluster_params* params /* NULL: defaults */);

/* beluga::estimate_clusters (algorithm/cluster_based_estimation.hpp:337-399) over the clusters of ParticleClusterizer (:269-304):
 * the weight, mean and covariance of EVERY cluster of more than one particle - the hypotheses of a filter that has not converged
 * (global localisation, a symmetric building, a kidnapped robot), of which mcl_cluster_based_estimate returns the heaviest alone.
 * *num_clusters: how many such clusters there are (the size of the reference's vector).  out receives the heaviest
 * min(capacity, MCL_MAX_CLUSTER_ESTIMATES, *num_clusters) of them, by descending weight, ties by ascending id: out[0] is
 * mcl_cluster_based_estimate's cluster.  No such cluster: MCL_OK, *num_clusters = 0, nothing written (the reference returns an empty
 * vector; the fallback to the overall estimate is mcl_cluster_based_estimate's).  capacity = 0 with out = NULL: the count alone, without
 * a pass over the particles.  The clusters are selected by the per-cell weight sums; the reported weight is the sum of the same pass over
 * the particles that gives the estimate beside it, and the order is taken over the reported weights.  One pass over the set for all
 * clusters, fixed-order sums: two calls on an unchanged set return the same bits.  The set is not modified.
 * MCL_ERR_NOT_READY without particles; MCL_ERR_INVALID_ARGUMENT for bad parameters; any sensor model.
 * Not on a context with a communicator of several ranks (MCL_ERR_UNSUPPORTED): the shards' sums are not exchanged yet. */
#define MCL_MAX_CLUSTER_ESTIMATES 64
typedef struct mcl_cluster_estimate {
  uint32_t id;           /* the cluster id ParticleClusterizer assigns (what mcl_cluster_labels writes) */
  uint32_t reserved;
  uint64_t count;        /* particles in the cluster, > 1 */
  double weight;         /* sum of the cluster's particle weights (estimate_clusters' Estimate::weight) */
  mcl_estimate estimate; /* beluga::estimate over the cluster's particles alone */
} mcl_cluster_estimate;
mcl_status mcl_estimate_clusters(mcl_ctx* ctx, const mcl_cluster_params* params /* NULL: defaults */, mcl_cluster_estimate* out,
                                 uint64_t capacity, uint64_t* num_clusters);
/* ParticleClusterizer::operator() (:269-304): the cluster id of every particle, in the order mcl_get_particles returns the particles.
 * labels: host memory, mcl_num_particles entries.  Errors as mcl_estimate_clusters, MCL_ERR_UNSUPPORTED over several ranks included. */
mcl_status mcl_cluster_labels(mcl_ctx* ctx, const mcl_cluster_params* params /* NULL: defaults */, uint32_t* labels);

/* beluga_ros::assign_particle_cloud(particles, size, PoseArray&) (beluga_ros/include/beluga_ros/particle_cloud.hpp:131-149):
 * `particles | views::sample | take_exactly(size)` — a weighted sample of `size` states of the current set, for
 * publication; the set itself is not modified.  states: size x 4 doubles (cos, sin, x, y), host memory.  The draws come
 * from the counter-based stream (seed; index, 0x80000000 | draw_id): pass a different draw_id per publication. */
mcl_status mcl_sample_particle_cloud(mcl_ctx* ctx, uint64_t size, uint32_t draw_id, double* states);

/* ---- Batches of small filters: many beluga::Amcl objects, one update call, three launches for the fleet ---------------------
 * A fleet server, a simulation farm or a multi-hypothesis tracker runs tens to hundreds of filters of the reference's own sizes (500 ..
 * 2000 particles).  One such update is three kernels around nanoseconds of work; a batch runs those three kernels ONCE for all its
 * members, with the members' blocks side by side in one grid, behind one synchronisation.
 *
 * mcl_batch_create stands for `count` beluga::Amcl constructors (amcl_core.hpp:105-124): member i is a full mcl_ctx made from cfgs[i],
 * all on ONE device and ONE stream - every device_id equal; every hip_stream NULL (the batch creates a stream and owns it) or all the
 * same non-NULL stream; anything else is MCL_ERR_INVALID_ARGUMENT.  count is 1 .. 1024.  Members may differ in every other
 * parameter: map, seed, particle bounds, motion model, sensor kind, scan size.  ALL filter state lives in the members, none in the
 * batch: mcl_batch_member hands member `index` out, and every call of this header works on it - mcl_set_map, mcl_initialize_*,
 * mcl_set_particles, mcl_get_particles, mcl_set_option, mcl_set_estimate_kind, mcl_update itself - between batch updates, from the
 * thread that drives the batch.  mcl_destroy on a member does nothing; mcl_batch_destroy destroys the members too.
 *
 * mcl_batch_update stands for Amcl::update (amcl_core.hpp:165-201) on every member: member i takes the control action
 * control_poses[4 i .. 4 i + 4) and the scan points_xy[2 point_offsets[i] .. 2 point_offsets[i + 1]) (point_offsets: count + 1 entries
 * that do not decrease).  For every member the call's effect and outputs - estimates[i], infos[i], the particle set, the recovery
 * filters, the every_n counter, the step number, force_update - are those of
 *   mcl_update(member_i, control_i, scan_i, points_i, &estimates[i], &infos[i])
 * BIT FOR BIT, and statuses[i] is that call's status: a member that fails its preconditions (no map, ...) is left as its own failing
 * mcl_update leaves it, one whose control has not moved far enough reports updated = 0, and the others proceed.  Returns the first
 * non-zero member status in index order, or MCL_ERR_INVALID_ARGUMENT of its own for null control_poses / point_offsets or offsets that
 * decrease (then no member has moved).  estimates, infos and statuses may each be NULL.
 *
 * Which members share the launches is decided per member and cycle: those whose own mcl_update would run exactly the small cycle -
 * likelihood-field or likelihood-field-prob model, not sharded, option small_fused on, the set and min(max_particles, capacity) both at
 * most 4096, the field's palette table usable, stage profiling off.  A beam-model member shares them too where its option
 * batch_beam_fused is on (default 0) and its own mcl_update would run the small cycle with the beam model's wave-per-particle kernel:
 * not sharded, option small_fused on, the set and min(max_particles, capacity) both 1 .. 4096, the set below the option
 * beam_sort_min_particles (from there on the member wants the ordered kernel), stage profiling off.  The beam members' reweight is one
 * more shared launch, between the propagation and the tail: a fleet of one family takes three launches per cycle, a fleet of both
 * takes four.  A scan of more than 4096 points is refused for such a member as by its own mcl_update (the kernel stages the scan in 64 KB
 * of workgroup memory): its status is its own, its state untouched, the others proceed.  An NDT member shares the launches where its
 * switch mcl_set_ndt_small_cycle is on and its own mcl_update would run the small cycle: not sharded, option small_fused on, the set
 * and min(max_particles, capacity) both 1 .. 4096, an NDT map installed, stage profiling off.  Its scan is fitted on the host and
 * staged per member as in its lone cycle; the NDT members' reweight is one more shared launch (a member without a measurement cell has
 * no block in it).  A fleet of all three families takes five launches per cycle.  An NDT member whose tail hands its cycle back
 * (mcl_set_ndt_small_cycle) finishes it inside the call, behind the shared synchronisation, with its own launches: its status - that
 * of a refused generator, MCL_ERR_BAD_COVARIANCE, included -, estimate and info are its lone mcl_update's, and the others are not
 * disturbed.  Every other member (larger sets, beam members with the option off or of the ordered kernel's size, NDT members with
 * the switch off, the landmark models, profiling on) runs its ordinary cycle inside the same call; a pending mcl_set_map_async map is
 * swapped in where mcl_update would.
 *
 * Counters (mcl_batch_get_counter): cycles = calls that updated at least one member; kernel_launches = kernels the shared cycle has
 * enqueued, a running total (per cycle with a fused member, however many members there are: 3 where the fused members are of one family,
 * 4 where likelihood-field and beam members are both present; the beam launch is left out where no fused beam member has a scan point);
 * members_fused / members_alone = running totals of members that updated through the shared launches / through their ordinary cycle;
 * beam_launches = shared beam reweight kernels enqueued, a running total; members_beam_fused = running total of beam members that updated
 * through the shared launches (they count in members_fused as well).  A fused member's own counters (small_tail_launches,
 * lf_beams_launches, the cells of mcl_beam_cells_visited) advance as in a lone cycle.  kernel_launches counts the NDT members' shared
 * reweight as well (one more per cycle in which a fused NDT member has a measurement cell); mcl_ndt_batch_counts reads the running
 * totals of those launches and of the NDT members that updated through the shared launches (they count in members_fused as well;
 * either pointer may be NULL).
 *
 * The cluster-based estimate (mcl_set_estimate_kind 1: what beluga_ros::Amcl::update returns) of the fused members is batched as well:
 * behind the cycle's synchronisation, TWO shared launches of one workgroup per member - the occupied cells of every member into its own
 * mapped list, then, behind each member's own host pass (assign_clusters), the sums of every member's winning cluster - with one
 * synchronisation each, in place of two launches and two synchronisations per member.  A member takes them if its cycle was fused, its
 * estimate kind is 1, its option batch_cluster_fused is on, its live set holds 1 .. 4096 particles and its cluster parameters are valid; every other member calls its own
 * mcl_cluster_based_estimate as before.  Two rare cases run that member's own kernels behind the shared ones: no cluster of more than
 * one particle (the overall estimate, cluster_based_estimation.hpp:424-427) and a cluster far from the pivot (a second pass of its sums,
 * counted in the member's estimate_repivots as in a lone cycle).  A member whose cell list fails its bounds check gets MCL_ERR_HIP as its
 * own status and the others proceed.  kernel_launches does not count these launches.  Further counters: cluster_launches = shared
 * cluster kernels enqueued, a running total (2 per cycle in which a member took the shared cluster path, 1 if none of them had a
 * winner, 0 if there was none); members_cluster_fused = running total of members whose estimate came through them; cluster_host_ns =
 * host time between the two launches (every member's cells ordered and assigned, one member after the other).
 *
 * The switch is a member's option: mcl_set_option(member, "batch_cluster_fused", 0) sends that member through its own
 * mcl_cluster_based_estimate (default 1; the batch has no entry point of its own for it). */
mcl_status mcl_batch_create(const mcl_config* cfgs, uint32_t count, mcl_batch** out);
void mcl_batch_destroy(mcl_batch* batch);
mcl_status mcl_batch_size(const mcl_batch* batch, uint32_t* count);
mcl_status mcl_batch_member(mcl_batch* batch, uint32_t index, mcl_ctx** ctx);
mcl_status mcl_batch_update(mcl_batch* batch, const double* control_poses, const double* points_xy, const uint64_t* point_offsets,
                            mcl_estimate* estimates, mcl_update_info* infos, mcl_status* statuses);
mcl_status mcl_batch_get_counter(mcl_batch* batch, const char* name, uint64_t* value);
mcl_status mcl_ndt_batch_counts(mcl_batch* batch, uint64_t* launches, uint64_t* members);
/* The fleet's update for landmark and bearing members: mcl_batch_update's contract with detections in the place of scans.  Member i
 * takes the detections [detection_offsets[i], detection_offsets[i + 1]) of vectors_xyz (3 doubles each) and categories: positions in
 * the robot frame for a landmark member, bearings in the sensor frame for a bearing member.  Every member's effect and outputs are bit
 * for bit those of its own mcl_update_landmarks / mcl_update_bearings, and statuses[i] is that call's status: more than
 * MCL_LANDMARK_MAX_DETECTIONS detections or a value that is not finite is the member's own MCL_ERR_INVALID_ARGUMENT, its state untouched,
 * the others proceed.  A member of any other sensor model gets MCL_ERR_UNSUPPORTED and is untouched (a fleet of scan and detection
 * members takes two calls; mcl_batch_update keeps refusing landmark and bearing members).  Offsets that decrease, or a null table, are
 * refused with no member moved.  A member shares the launches where its switch mcl_set_landmark_small_cycle is on and its own update
 * would run the small cycle: not sharded, option small_fused on, the set and min(max_particles, capacity) both 1 .. 4096, stage
 * profiling off.  Those members take k_batch_propagate, ONE shared reweight launch for both kinds (a workgroup finds its member and
 * branches on the member's kind; a member without a particle or a detection has no block in it) and k_batch_small_tail: three launches
 * per cycle for the fleet, one synchronisation.  Every other landmark or bearing member runs its own cycle inside the call.  The
 * cluster-based estimate of fused members goes through the two shared cluster launches as in mcl_batch_update.  Counters
 * (mcl_batch_get_counter): landmark_launches = shared landmark reweight kernels enqueued, members_landmark_fused = members that updated
 * through the shared launches (running totals; kernel_launches and members_fused count them as well). */
mcl_status mcl_landmark_batch_update(mcl_batch* batch, const double* control_poses, const double* vectors_xyz, const uint32_t* categories,
                                     const uint64_t* detection_offsets, mcl_estimate* estimates, mcl_update_info* infos, mcl_status* statuses);
const char* mcl_batch_last_error(const mcl_batch* batch); /* batch may be NULL: error of the last failed mcl_batch_create */

/* ---- Shared maps: one uploaded map, many filters ------------------------------------------------------------------------------
 * A fleet on one building's map needs that map on the device once.  mcl_shared_map_create builds, for the device, sensor_kind and lf
 * of `cfg`, everything mcl_set_map would build for a context made from that config - the occupancy, the free-cell list, and for the
 * likelihood-field kinds the field (field_build 0: the reference's wavefront on the host, 1: the exact distance transform on the
 * device), its pz^3 table, the palette and the far-tile bitmaps; for the beam model the packed occupancy - on a stream of its own,
 * synchronised before it returns.  It touches no context, so it may run on any thread while filters update.  NDT, landmark and bearing
 * kinds have maps of their own: MCL_ERR_UNSUPPORTED.  A shared map never changes.
 *
 * mcl_use_shared_map stands for update_map on the context, wherever mcl_set_map is allowed (a batch member between two batch updates
 * included): it leaves the context as mcl_set_map with the same grid leaves it - a pending mcl_set_map_async map is dropped - except
 * that the context owns nothing of the map.  Every result of an attached context equals, bit for bit, that of a context given the same
 * grid through mcl_set_map.  It is accepted if the map is on the context's device and was built for its sensor family: the beam model
 * for a beam context; for the likelihood-field kinds the same sensor_kind and an mcl_lf_params equal field for field.  Otherwise
 * MCL_ERR_INVALID_ARGUMENT, mcl_last_error names the mismatch, and the context is unchanged.  A shared map holds every table a
 * private one holds, so no option of an attached context is refused.
 *
 * While attached, every read and every update entry point works as before; mcl_set_likelihood_field answers MCL_ERR_UNSUPPORTED and
 * changes nothing; mcl_set_map / mcl_set_map_async (at its swap) detach the context and give it a map of its own.
 * mcl_shared_map_release gives up the caller's reference only: the map lives until the last context that reads it has left it or is
 * destroyed.  Thread rules: create, release and get_info from any thread; mcl_use_shared_map from the thread that drives the context.
 *
 * mcl_shared_map_info: device_bytes / host_bytes = what the map holds; users = contexts attached now.  Counters of a context
 * (mcl_get_counter): map_device_bytes = device bytes the context itself owns for its map (0 while attached), map_shared = 0 / 1. */
typedef struct mcl_shared_map mcl_shared_map;
typedef struct mcl_shared_map_info {
  uint32_t width, height;
  double resolution;
  int32_t sensor_kind;
  int32_t device_id;
  uint64_t device_bytes, host_bytes;
  uint32_t users;
} mcl_shared_map_info;
mcl_status mcl_shared_map_create(const mcl_config* cfg, const int8_t* cells, uint32_t width, uint32_t height, double resolution,
                                 const double origin[4], const int8_t value_traits[3], int32_t field_build, mcl_shared_map** out);
void mcl_shared_map_release(mcl_shared_map* map);
mcl_status mcl_shared_map_get_info(const mcl_shared_map* map, mcl_shared_map_info* info);
const char* mcl_shared_map_last_error(const mcl_shared_map* map); /* map may be NULL: error of the last failed mcl_shared_map_create */
mcl_status mcl_use_shared_map(mcl_ctx* ctx, mcl_shared_map* map);

/* ---- Particle shards across the GPUs of one node (one context per GPU, one process or thread per context) -------------
 * The logical filter's particles are split into contiguous shards of the global index space (mcl_config.shard_offset /
 * shard_capacity); the map is replicated and every rank passes the same control action and scan to mcl_update.  With a
 * communicator attached, mcl_update runs the whole cycle over the sharded set: propagation and reweight are local; the weight
 * normaliser is the sum of the gathered shard sums; the shard totals of the normalised weights are gathered into the
 * intervals of the global CDF; every output slot's draw u_j * total (same counter-based stream as on one GPU) is routed to the
 * shard that owns it, which answers with the ancestor's state (views::sample | random_intersperse | actions::assign,
 * amcl_core.hpp:188-196); the estimate's nine sums are gathered and added in rank order.  Results do not depend on the
 * number of ranks beyond the rounding of these sums.  With min_particles < max_particles the resampling is KLD-adaptive over
 * the shards as well (views::take_while_kld over the GLOBAL candidate stream, take_while_kld.hpp:72-88,112-137): candidates are
 * drawn block by block through the same exchange, the spatial hashes of every block are all-gathered, every rank takes the same
 * cut, and the kept candidates are re-balanced into contiguous shards - each context's shard_capacity must hold its share of
 * max_particles; mcl_update_info.num_particles is the count over all shards.  (The same steps are available one by one through
 * the stage-level entry points below: beluga_amd/sharded.py drives them over torch.distributed.)
 *
 * The collectives go through a transport: RCCL over xGMI (mcl_comm_attach_rccl; librccl.so is loaded at run time, the
 * library has no link-time dependency on it), or caller-supplied functions (mcl_comm_attach: MPI, a shared-memory exchange
 * between the threads of one process, ...).  All buffers are DEVICE pointers; calls are made in the same order on all ranks
 * and must be complete (or stream-ordered on `hip_stream`) when they return. */
typedef struct mcl_transport {
  void* user;
  /* every rank contributes `bytes` bytes at d_send; d_recv receives world * bytes, in rank order */
  int32_t (*all_gather)(void* user, const void* d_send, void* d_recv, uint64_t bytes, void* hip_stream);
  /* this rank sends send_bytes[q] bytes to rank q (consecutive blocks of d_send, in rank order) and receives recv_bytes[q]
   * bytes from rank q (consecutive blocks of d_recv, in rank order) */
  int32_t (*all_to_all)(void* user, const void* d_send, const uint64_t* send_bytes, void* d_recv, const uint64_t* recv_bytes,
                        void* hip_stream);
} mcl_transport;
/* Attaches a communicator of `world` ranks to a context created with this rank's shard_offset / shard_capacity.  The transport
 * struct is copied; `user` must outlive the context.  world == 1 is allowed (the cycle then needs no exchange).
 * COLLECTIVE for world > 1: the attach all-gathers a word of the configuration that selects a cycle's collectives (particle bounds,
 * resampling policy, thresholds, recovery alphas, KLD parameters, models, seed, device_policy, estimate kind, shard_pad_permille) and blocks until every
 * rank has attached - the ranks attach CONCURRENTLY (one thread or process per rank; a host that attaches its ranks one after the
 * other from one thread through a rendezvous transport deadlocks) - and every rank fails alike on a mismatch.  On an attached
 * filter mcl_set_option("device_policy" | "shard_pad_permille", ...) and mcl_set_estimate_kind are collective in the same way: every rank calls them, concurrently,
 * with the same arguments, whatever its own previous value was; on a mismatch they return an error and leave the value unchanged. */
mcl_status mcl_comm_attach(mcl_ctx* ctx, uint32_t rank, uint32_t world, const mcl_transport* transport);
/* RCCL: rank 0 obtains an id (ncclGetUniqueId), hands its 128 bytes to the other ranks by any means, every rank attaches. */
mcl_status mcl_comm_unique_id(uint8_t id[128]);
mcl_status mcl_comm_attach_rccl(mcl_ctx* ctx, const uint8_t id[128], uint32_t rank, uint32_t world);

/* ---- Device access for zero-copy interop (torch / RCCL hand-off) -------------------------------- */
typedef struct mcl_device_view {
  double* states;     /* n records of 4 doubles (cos, sin, x, y) */
  double* w;
  double* cdf;        /* inclusive scan of the normalised weights (valid after mcl_build_cdf): non-decreasing, flat across weights of zero */
  uint64_t n;         /* live particles in this shard */
  uint64_t capacity;
  void* hip_stream;
} mcl_device_view;
mcl_status mcl_get_device_view(mcl_ctx* ctx, mcl_device_view* view);
mcl_status mcl_set_num_particles(mcl_ctx* ctx, uint64_t n);
/* Inclusive scan of the (normalised) weights into the cdf buffer; returns the shard total. */
mcl_status mcl_build_cdf(mcl_ctx* ctx, double* total);
/* Sharded views::sample | random_intersperse (views/sample.hpp:102,133-135; random_intersperse.hpp:90-115) for the
 * `count` output slots [first_slot, first_slot+count) of the GLOBAL particle index space:
 * d_targets[t] = u_j * total (a point of the global CDF, total = sum of all shards' weights), or NaN where the
 * slot receives an injected random state.  u_j comes from the same Philox stream as the single-GPU path. */
mcl_status mcl_resample_targets(mcl_ctx* ctx, uint32_t step, double random_state_probability, double total,
                                uint64_t first_slot, uint64_t count, double* d_targets);
/* Routing for the ancestor exchange (device pointers throughout, nothing synchronises):
 * groups the `count` targets of mcl_resample_targets by the shard that owns them. `d_ends[r]` / `d_offsets[r]` are the
 * inclusive end / exclusive start of shard r's interval of the global CDF (world <= 64).  Outputs: d_send_targets =
 * shard-local targets ordered by destination rank, d_order[k] = output slot answered by the k-th request,
 * d_counts[r] (int64) = requests for rank r.  NaN targets (injected slots) are routed to `self_rank`. */
mcl_status mcl_route_targets(mcl_ctx* ctx, const double* d_targets, uint64_t count, const double* d_ends, const double* d_offsets,
                             uint32_t world, uint32_t self_rank, double* d_send_targets, uint32_t* d_order, int64_t* d_counts);
/* The owning shard's side of the exchange: for each of the `m` requests t[j] (values in this shard's cdf range
 * [0, total]) the state of the first particle i with cdf[i] >= t[j] — std::discrete_distribution's lower_bound
 * (views/sample.hpp:133-135) — as one (x, y, cos, sin) record of 4 doubles. */
mcl_status mcl_serve_requests(mcl_ctx* ctx, const double* d_requests, uint64_t m, double* d_replies);
/* actions::assign (actions/assign.hpp:56-64) of the exchanged ancestors, replies in request order plus the d_order of
 * mcl_route_targets: slot d_order[k] takes reply k, or a random free-space state where its target is NaN; weights become
 * 1 (particle_traits.hpp:105); the shard then holds `count` particles. */
mcl_status mcl_commit_routed(mcl_ctx* ctx, uint32_t step, uint64_t first_slot, uint64_t count, const double* d_replies,
                             const uint32_t* d_order, const double* d_targets);
/* KLD-adaptive resampling across shards (views/take_while_kld.hpp:72-88,112-137 over the GLOBAL candidate stream).
 * The driver draws candidates block by block: each shard draws its slice of the block (mcl_resample_targets, routing,
 * mcl_serve_requests as above), then mcl_finish_candidates writes the slice's states (4 doubles cos, sin, x, y per
 * candidate, slot order) and spatial hashes (algorithm/spatial_hash.hpp:190-193) to caller buffers without touching the
 * live set.  Every shard is fed the hashes of the whole block in global candidate order (all-gather) through
 * mcl_kld_feed, which returns in *first_fail the global index of the first candidate failing kld_condition (it and
 * everything after it is dropped), or ~0 if the block passes; mcl_kld_begin starts a pass.  After the cut the driver
 * re-balances the kept candidates and installs each shard's slice with mcl_load_shard (weights 1,
 * particle_traits.hpp:105); shard_offset is the global index of its first particle (used by the RNG addressing). */
mcl_status mcl_finish_candidates(mcl_ctx* ctx, uint32_t step, uint64_t first_slot, uint64_t count, const double* d_replies,
                                 const uint32_t* d_order, const double* d_targets, double* d_states, uint64_t* d_hashes);
mcl_status mcl_kld_begin(mcl_ctx* ctx);
mcl_status mcl_kld_feed(mcl_ctx* ctx, const uint64_t* d_hashes, uint64_t count, uint64_t* first_fail);
mcl_status mcl_load_shard(mcl_ctx* ctx, const double* d_states, uint64_t n, uint64_t shard_offset);
/* Device-side variants for callers that keep scalars on the GPU (e.g. to feed RCCL collectives without a host
 * round trip).  All pointers are DEVICE pointers; nothing synchronises; work is enqueued on the context's stream. */
mcl_status mcl_weight_sum_device(mcl_ctx* ctx, double* d_sum);
/* d_factor: the (global) normalisation factor; d_stats[0] = sum of the new weights, d_stats[1] = sum of squares. */
mcl_status mcl_normalize_device(mcl_ctx* ctx, const double* d_factor, double* d_stats);
mcl_status mcl_build_cdf_device(mcl_ctx* ctx, double* d_total);
/* d_sums[0..8] = the nine sums of mcl_estimate_sums for the given pivot. */
mcl_status mcl_estimate_sums_device(mcl_ctx* ctx, const double pivot_xy[2], double* d_sums);
mcl_status mcl_sync(mcl_ctx* ctx);

/* ---- Measurement hooks (bench.py): HIP-event timing of each stage on the context's stream. ------ */
enum {
  MCL_STAGE_PROPAGATE = 0,
  MCL_STAGE_REWEIGHT = 1,
  MCL_STAGE_NORMALIZE = 2,
  MCL_STAGE_RESAMPLE = 3,
  MCL_STAGE_ESTIMATE = 4,
  MCL_STAGE_SENSOR_KERNEL = 5, /* the sensor-model kernel alone (inside MCL_STAGE_REWEIGHT) */
  MCL_NUM_STAGES = 6
};
/* on: 0 = off, 1 = the sensor kernel of every 4th cycle only, 2 = every stage of every cycle (each event record costs ~5 us
 * of stream time, so timed runs use 1). */
mcl_status mcl_profile_enable(mcl_ctx* ctx, int32_t on);
/* Accumulated milliseconds and launch counts per stage since the last reset. */
mcl_status mcl_profile_read(mcl_ctx* ctx, double ms[MCL_NUM_STAGES], uint64_t counts[MCL_NUM_STAGES], int32_t reset);

/* Beam model only: grid cells visited by the ray walks since the last reset (cells/s).  It does not move while the
 * cycle reads a range table (mcl_build_range_table): nothing is walked there, and the table's build is not counted. */
mcl_status mcl_beam_cells_visited(mcl_ctx* ctx, uint64_t* cells, int32_t reset);

/* ---- Switches and hooks for A/B measurements and tests.  No option but field_build changes a result beyond the rounding of a
 * particle's sum over the scan: the likelihood-field kernels with a lane per particle add the beams as libstdc++'s
 * std::transform_reduce does (blocks of four; the reference's call, likelihood_field_model.hpp:76), the kernels with a wave per
 * particle (lf_variant 3, small sets, lf_dispersed) in a fixed tree - 1e-16 relative. ------------------------------------
 * Options (defaults in parentheses; BELUGA_MCL_<NAME> in the environment sets the default at mcl_create):
 *   lf_variant (2)  likelihood-field kernel family: 2 = spatially ordered lanes (small sets: see lf_small_particles), 1 (and 0) = a lane
 *                   per particle in index order over the f32 field (no ordering pass), 3 = wave per particle over the palette table
 *   lf_fast (-1)    FMA variant with exact fallback: nonzero = whenever its preconditions hold, 0 = never
 *   lf_table (0)    1 = force the 8-byte table instead of the palette
 *   lf_patch (1)    index table through per-workgroup LDS patches (dense sets): 1 = where the last launch found them useful
 *                   (a dispersed set - global localisation - has none, and is sent to the per-lane gathers, with a probe every
 *                   16th launch), 0 = never, 2 = always
 *   lf_loose_below (224)  LDS-patch kernel: a workgroup with fewer than this many 256ths of its beam groups fitting a patch
 *                   gathers every look-up (a gathered group inside a patched workgroup costs twice one of an all-gathering one)
 *   lf_dispersed (2)  a set reported as dispersed: 2 = the lanes of a wave over the beams of one pose, the poses in the position-major
 *                   order, the far-tile bitmap in LDS (where the bitmap takes at most 32 KB and the scan fits beside it, else as 0),
 *                   0 = the ordered-lanes gather kernel (a lane per particle; 15 % slower at 1M x 1080), 1 = a wave per particle, lanes
 *                   over the beams, no ordering pass (slower still).  2 and 1 add a pose's terms as a tree over 64 lane sums: the
 *                   weights of 0 up to rounding (1e-13 relative).  lf_far_beams_per_wave (0 = 32): poses per wave of 2.
 *   lf_far_tiles (1)  the per-lane gather kernel keeps a bitmap of the table's far tiles in LDS (8x8 cells uniformly at the
 *                   field's most common value: free space beyond max_obstacle_distance of anything) and skips the memory access
 *                   of a look-up into one: 1 = for sets reported as dispersed, 0 = never, 2 = whenever that kernel runs.  Same
 *                   values, same sums (1M x 1080 dispersed over the 4000^2 map: 3.7 -> 1.9 ms per launch)
 *   key_layout (-1)  spatial ordering key: -1 = position-major (y, x Morton-interleaved, heading last) for likelihood-field sets
 *                   reported as dispersed - the far-tile gather kernel hands each XCD one contiguous eighth of that order, so an
 *                   XCD's L2 serves the neighbourhood of one block of the map at a time - and heading-major otherwise; 0 / 1 force
 *   lf_small_particles (65536)  likelihood-field sets below this size: a wave per 1..16 particles, lanes over the beams, no
 *                   ordering pass (the measured crossover to the ordered kernels)
 *   beam_table (1)  beam model, ordered kernel: what depends on a beam's EXPECTED range alone (the range itself, the hit normaliser
 *                   with its two erf, the short-return normaliser with its exp) comes from a table over the squared cell distance
 *                   between the hit and the source, built on the device at mcl_set_map with the same expressions; 0 = per beam
 *   lf_weight_sums (1)  the whole cycle's normalisation factor is added up from the likelihood-field kernel's workgroup sums of the
 *                   new weights (fixed order: the spatial order is the sort by (key, index), the same in every run); 0 = a pass of
 *                   its own over the weights (k_chunk_sum)
 *   device_policy (1)  recovery estimator on the device when the cycle takes no host-side decision
 *   sort_min_particles (16384)  below this many particles the spatial ordering is skipped (likelihood-field models)
 *   beam_sort_min_particles (16384)  beam model: the ordered kernel from this size on; below it a wave per particle over the
 *                   whole-grid bit maps (both skip empty space by the block distance map)
 *   key_curve (1)   heading-major ordering key: 1 = along the Hilbert curve through the (heading, y, x) bins - any run of the
 *                   order is a compact, connected set of bins -, 0 = Morton order (round 2: a run that crosses a high-level boundary
 *                   of the Z curve is two pieces far apart, and its workgroup fits no LDS patch)
 *   key_warp (1)    heading-major ordering key over bins of equal MASS of a normal set (the key frame's +-4 sigma mapped through the
 *                   normal distribution function) instead of equal width: the ordering's 1024 first-pass buckets then hold about the
 *                   same number of particles; 0 = equal width (round 2)
 *   key_bits_xy (0) bits of the x and of the y bins of that key (the heading gets the other 20 - 2 b): 0 = chosen every cycle from
 *                   the cloud's spread and the scan's reach (4 .. 6), 4 / 5 / 6 = forced (round 2: 6)
 *   lf_queue (1)    LDS-patch kernel, launches with more blocks than the device keeps workgroups resident (three per CU): 1 = that many
 *                   workgroups, each taking blocks from a counter until none is left (an XCD that is ahead takes more:
 *                   2 - 4 % off the kernel at 1M particles), 0 = one workgroup per block.  Which workgroup computes a block changes
 *                   nothing in it.  lf_queue_grid (0): the number of resident workgroups, 0 = three per CU (tests: a few workgroups)
 *   shard_pad_permille (1063)  sharded fixed-size cycle (mcl_comm_attach): the ancestor exchange moves a FIXED number of entries per pair of
 *                   ranks - mean * permille / 1000 + 8 * sqrt(mean) + 64, mean = what a shard's output slots ask of one other shard on
 *                   average - so that no count has to be read by the host in the middle of the cycle (one host synchronisation per cycle);
 *                   a cycle whose requests do not fit runs the exchange again with exact counts (mcl_get_counter "comm_overflows").
 *                   0 = always exact counts (two host synchronisations per cycle).  Part of the configuration the ranks compare at
 *                   mcl_comm_attach; on an attached filter setting it is a COLLECTIVE call like device_policy (every rank, same value).
 *   lf_ends_first (1)  LDS-patch kernel: the blocks are taken from both ends of the spatial order inwards (0, N - 1, 1, N - 2, ...): the ends
 *                   are the cloud's fringe, whose blocks gather every look-up and take twice as long - taken first they are not the launch's
 *                   last; 0 = in order
 *   beam_sectors (1)  beam model, ordered kernel, scanners that reach beyond half the 1024-cell LDS window (448 .. 896 cells): the scan is taken
 *                   in four sectors, each with a window that holds its rays; 0 = one centred window, rays that leave it go on over the
 *                   whole-grid maps in global memory (same cells visited either way)
 *   beam_free_ahead (1)  beam model, ordered kernel: per workgroup and beam, the cells the middle particle's ray clearance proves free for
 *                   every lane are passed in one closed-form step before a lane's own walk (same cells visited, same weights)
 *   cycle_spin (-1)  fixed-size cycles (resample every cycle, mean / covariance estimate): 1 = the host waits for a completion word the
 *                   cycle's last kernel stores to mapped host memory instead of the stream's completion signal (the calling thread spins
 *                   for the length of the cycle); 0 = hipStreamSynchronize; -1 = the word for sets of 256K particles and more.
 *                   Measured: + 1 % at 1M particles, 4 us per cycle slower at 2000.  Never while stage profiling is enabled.
 *   scan_fused (1)  fixed-size cycle that resamples: normalisation, totals of the normalised weights, recovery estimator and CDF in ONE
 *                   launch (the chunk sums travel between the workgroups inside it): 1 = for sets of up to 64K particles, where the cycle
 *                   is bound by the host's launches; 2 = up to 2M particles (measured at 1M: no faster than the two launches); 0 = never.
 *                   Bit-identical.
 *   draw_fold (1)   the draw kernel's last workgroup to finish adds up the estimate sums instead of a launch of its own behind it: 1 = for
 *                   sets of up to 64K particles, 2 = up to 4M (measured at 1M: 2.6 us slower), 0 = never.  Bit-identical.
 *   lf_unit_weights (1)  LDS-patch kernel on a set whose weights are all 1.0 - fresh from a resampling or an initialisation
 *                   (particle_traits.hpp:105), which the library keeps track of -: the old weight is not loaded (1.0 x = x); 0 = always
 *                   loaded.  Bit-identical; 9 us of a 1M-particle cycle.
 *   noise_ahead (1)  fixed-size cycles, sets of 64K .. 2M particles: the NEXT cycle's propagation normals - a function of (seed, step, particle
 *                   index) alone - are drawn a cycle ahead: 1 = by the draw kernel (whose vector units wait for memory), 2 = by a kernel of its
 *                   own behind the cycle's last one, while the host is away (cycles that end on the completion word); 0 = by the propagation
 *                   kernel itself.  Bit-identical; counter noise_ahead_used.
 *   order_ahead (1)  fixed-size cycles that end on the completion word (cycle_spin), sets of 64K .. 2M particles: the draw kernel also leaves the
 *                   ordering key of where each particle will be after the NEXT propagation - with the control action of this cycle as the
 *                   prediction, first order, single precision -, the ordering passes run behind the cycle's last kernel while the host is
 *                   away, and the next cycle goes from its propagation straight into the reweight if the action it gets is close to the
 *                   predicted one (else it orders as before).  Only locality depends on the order.  0 = the ordering inside the cycle.
 *                   Counters order_ahead_used / order_ahead_missed.
 *   draw_key_hist (1)  with order_ahead: the draw kernel counts the high digits of the ordering keys it predicts, per workgroup, and the ordering's
 *                   row scan adds those counts up - no pass of its own over the keys; 0 = a kernel reads the keys back.  Bit-identical.
 *   rows_merged (1)  with draw_key_hist: the estimate sums' last additions and that row scan in one launch; 0 = two.  Bit-identical.
 *                   Both measured at 1M particles: + 1.6 % once the cloud has settled, nothing shown before.
 *   lf_pose_ahead (1)  likelihood-field models: world_to_field * pose of every particle - what each of their kernels starts from - is
 *                   stored beside the pose by the propagation that writes it (by a kernel of its own, k_field_pose, in front of a reweight
 *                   of a set that nothing has propagated under the current map: after mcl_set_particles, an initialisation, a
 *                   resampling, a map given since) and the kernels load it; 32 bytes per particle of capacity.  0 = every kernel forms
 *                   the product itself, per particle and launch.  Bit-identical; counter field_pose_rebuilds (launches of k_field_pose).
 *                   Set through mcl_set_option alone: it has no BELUGA_MCL_* variable.
 *   norm_store (0)  fixed-size cycle that resamples at once: 0 = the normalisation kernel does not store the normalised weights (nothing reads
 *                   them), the CDF kernel divides again; 1 = stored.  Bit-identical.
 *   batch_cluster_fused (1)  a member of a batch that returns the cluster-based estimate: 1 = through the batch's two shared launches
 *                   ("Batches of small filters"), 0 = through its own mcl_cluster_based_estimate.  The same bits either way.
 *   batch_beam_fused (0)  a beam-model member of a batch whose cycle is the small one with the wave-per-particle kernel: 1 = its kernels
 *                   ride on the fleet's shared launches, the reweight on one launch for all such members ("Batches of small filters"),
 *                   0 = it runs its own cycle inside mcl_batch_update.  The same bits either way.  Off until the path has been measured.
 *   range_table_max_bytes (4 GiB)  mcl_build_range_table refuses a table larger than this (0 .. 2^62) before anything is allocated
 *   range_table_launch (2^30)  entries one launch of the table's build covers (256 .. 2^30, whole workgroups of 256); the same table
 *   small_fused (1)  sets of up to 4096 particles: everything behind the reweight - normalise, policies, fixed-size or KLD resampling, estimate
 *                   sums - in one launch of one workgroup and one host synchronisation (and two one-workgroup kernels around the host's pass of
 *                   cluster_based_estimate); 0 = the kernels of the large path
 *   lf_split (3)    LDS-patch planner: a group of 8 beams that fits no whole 64 x 64-cell patch (its end-points straddle a range
 *                   discontinuity: 3 - 5 % of the groups of an indoor scan, whatever the cloud) goes through two half patches -
 *                   beams [0, k) and [k, 8), 32 x 64 (bit 0) or 64 x 32 (bit 1) cells each, in the buffer of one whole patch; 0 = such
 *                   groups are gathered
 *   lf_margin (1)   LDS-patch planner, the rotation part of the bound on a workgroup's end-points: 1 = per axis
 *                   ((1 - cos d) |q'x| + |sin d| |q'y| in x, the transpose in y), 0 = |R_p - R_ref| |q| on both axes (round 2)
 *   field_build (0)  how the NEXT mcl_set_map builds the likelihood field: 0 = the reference's priority-queue wavefront on the
 *                    host (bit-identical field, seconds at 16 M cells), 1 = exact Euclidean distance transform on the device
 *                    (milliseconds; equal at all but the few cells where the wavefront does not find the nearest obstacle,
 *                    never farther from the truth; falls back to 0 when max_obstacle_distance spans more than 1024 cells).
 *                    This one DOES change the field where the two algorithms differ; everything downstream follows the field.
 * Counters: lf_beams_launches = launches of the wave-per-particle LF kernel (small sets, lf_dispersed, lf_variant 3);
 *   lf_far_launches = those of the gather kernels with the far-tile bitmap (lf_far_beams_launches of them: the lanes-over-beams form,
 *   lf_dispersed 2), lf_far_tiles = tiles in the bitmap (0 = none built);
 *   lf_fast_launches = launches of the FMA variant so far; lf_patch_launches = those of them sent to the LDS-patch
 *   kernel; lf_patch_groups_planned / lf_patch_groups_through = groups of 8 beams (per workgroup) that kernel has looked at /
 *   has read through a patch, running totals over a sample of the workgroups; lf_queue_launches = launches of the
 *   LDS-patch kernel with the queue of blocks; field_built_on_device, field_build_us = the last mcl_set_map;
 *   small_tail_launches = cycles that ran their tail in the one launch of option small_fused;
 *   beam_wave_launches / beam_ordered_launches = a beam context's own reweight launches of the wave-per-particle kernel / of the
 *   ordered-lanes kernel (beam_sort_min_particles decides; no launch for an empty set or scan; a fleet's shared launch counts in the
 *   batch's beam_launches instead);
 *   ndt_lane_launches / ndt_wave_launches = an NDT context's own reweight launches of the lane-per-particle kernel / of the
 *   wave-per-particle kernel, in either map layout (mcl_set_ndt_small_cycle and the size of the set decide; not counted for an empty set
 *   or a scan without a measurement cell; a fleet's shared launch counts in mcl_ndt_batch_counts instead);
 *   landmark_lane_launches / landmark_wave_launches = a landmark or bearing context's reweight launches of the lane-per-particle kernel /
 *   of the wave-per-particle kernel (mcl_set_landmark_small_cycle and the size of the set decide; not counted for an empty set or a call
 *   without detections; a fleet's shared launch counts in the member's landmark_wave_launches);
 *   beam_skip_launches = count launches of enabled cycles and reweights ("Beam skipping": one per pass of 4096 beams; none for an
 *   empty set or scan), beam_skip_used_all = those decisions that fell back to the whole scan, beam_agreement_calls = calls of
 *   mcl_beam_agreement that reached the device;
 *   cluster_cells = occupied cells of the last cluster_based_estimate; comm_ranks_seen (ncclCommCount of the library's communicator, 0
 *   without one), comm_collectives, comm_bytes_out (running totals of this rank), comm_backend (0 = none, 1 = the caller's transport, 2 = RCCL inside the library). */
mcl_status mcl_set_option(mcl_ctx* ctx, const char* name, int64_t value);
mcl_status mcl_get_counter(mcl_ctx* ctx, const char* name, uint64_t* value);
/* Runs the spatial ordering on the current set and returns it: perm[t] = particle at position t, keys[i] = ordering key
 * of particle i (n entries each, host memory).  keys[perm[t]] is non-decreasing in t. */
mcl_status mcl_debug_order(mcl_ctx* ctx, uint32_t* perm, uint32_t* keys);

/* Test hook: sets the outputs of the two exponential filters of ThrunRecoveryProbabilityEstimator
 * (thrun_recovery_probability_estimator.hpp:69-89, exponential_filter.hpp:32-44) on the host and on the device.  With a fixed particle
 * count the estimator sees the average of NORMALISED weights - 1 / N in every cycle - and never leaves p = 0 by itself (amcl_core.hpp:177-179,
 * as in the reference); a test that wants a cycle with injected random states (random_intersperse over shards) puts the filters apart first.
 * On an attached filter every rank has to make the same call. */
mcl_status mcl_debug_set_recovery_filters(mcl_ctx* ctx, double slow, double fast);

/* Test hook, read-only: the motion sampler the last propagation (mcl_propagate, or the propagation of an update) handed to its kernel, bit
 * for bit - out = {m1, s1, mt, st, m2, s2, kind (MCL_MOTION_*), first_c, first_s}: the means and standard deviations of the first rotation,
 * the translation and the second rotation (omnidirectional: rotation, translation, strafe; first_c / first_s = the rotation to the direction
 * of travel).  MCL_ERR_INVALID_ARGUMENT before the first propagation.  No device work. */
mcl_status mcl_debug_last_sampler(mcl_ctx* ctx, double out[9]);

/* Position of the cell (heading, y, x), `bits` bits each, along the 3-D Hilbert curve the heading-major ordering key follows
 * (kernels.h hilbert_index_3; pure host arithmetic, no device needed): consecutive positions are face neighbours. */
uint32_t mcl_debug_curve_index(uint32_t heading_bin, uint32_t y_bin, uint32_t x_bin, uint32_t bits /* per axis, 1 .. 6 */);

const char* mcl_version(void);
/* Nonzero for a measurement build of the kernels (tools/build_variant.sh: ablations compute nonsense by design, timing builds distort):
 * beluga_amd/capi.py refuses to load one as the product library unless BELUGA_MCL_ALLOW_MEASUREMENT_BUILD=1. */
int mcl_measurement_build(void);

#ifdef __cplusplus
}
#endif
#endif /* BELUGA_MCL_H */
