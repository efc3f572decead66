// kernels.h — launchers of the gfx950 kernels behind the C ABI (include/beluga_mcl.h).
// Data layout in HBM (all owned by mcl_ctx):
//   particles : pose records of 4 f64 (cos, sin, x, y) + w[cap]   (two sets: live + resample target)
//   field     : f32 row-major H x W likelihood field (likelihood_field_model_base.hpp:120), 64 MB at 4000^2
//   cells     : int8 row-major H x W occupancy grid (beam model + free-space sampling), 16 MB at 4000^2
//   points    : f64 (x,y) pairs of the current scan, 17 KB at 1080 beams
//   cdf       : f64 inclusive scan of the normalised weights
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "batch_host.h"
#include "cycle_types.h"
#include "ndt_hash.h"
#include "scratch_layout.h"
#include "se2.h"
#include "search_host.h"
#include "raycast_host.h"
#include "range_table_host.h"
#include "sensor_records.h"

namespace mcl {

// One particle set: poses as records of 4 doubles (cos, sin, x, y) — Sophus::SE2d::data() order, the order of the C ABI —
// and the weights as a separate array.  Records, not one array per component: the multinomial draw and the spatial
// ordering gather poses of random particles, and a record is one 32-byte access instead of four cache lines.
struct Particles {
  double4* pose;
  double* w;
};

// Where a kernel that writes poses into the live set also leaves their field-frame form, world_to_field * pose as (cos, sin, x, y) with
// the host's bits (se2.h pose_mul_ieee), indexed like Particles::pose - what every likelihood-field kernel starts from (option
// lf_pose_ahead).  pose == nullptr: nowhere (another sensor model, or the option is off).
struct FieldPoseOut {
  double4* pose;
  Pose2 world_to_field;  // FieldView::world_to_field of the map the poses will be read against
};

struct FieldView {
  const float* data;
  uint32_t W, H;
  double inv_resolution;  // 1. / resolution (regular_grid.hpp:76)
  Pose2 world_to_field;   // grid.origin().inverse() (likelihood_field_model_base.hpp:99)
  float unknown_value;    // float(1 / max_laser_distance) (likelihood_field_model.hpp:75)
  // Derived table for the hot kernel: cube[i] = pz*pz*pz with pz = double(data[i]) — exactly the per-beam
  // term of likelihood_field_model.hpp:84-88 — and cube[W*H] = the same for unknown_value.  8 B per cell.
  const double* cube;
  int prob;  // LikelihoodFieldProbModel: the table holds log(pz) and the weight is exp(sum) (likelihood_field_prob_model.hpp:76-88)
  // Palette form of the same table (used when the field has few distinct values, which a quantised distance map always
  // has): pal_val[k] = the cube / log term of the k-th distinct field value; pal_idx = one uint16 per cell, stored in
  // 8x8-cell tiles of 128 bytes (see palette_offset) with a border of one tile of "unknown" cells all around, so that
  // clamping a cell coordinate to [-1, W] x [-1, H] replaces the in-grid test.  The uint16 is the LDS byte address of the
  // cell's palette entry inside k_reweight_lf_palette's workgroup memory: pal_base + 8 * k.
  // 2 B per cell instead of 8 and square tiles: a wave's gather touches ~4x fewer cache lines.
  const uint16_t* pal_idx;
  const double* pal_val;
  uint32_t pal_count;  // 0 = no palette
  uint32_t pal_pitch;  // bytes per row of tiles (border included)
  uint32_t pal_base;   // LDS byte offset of the palette (after the row-offset table of H + 2 words)
  uint32_t pal_bytes;  // size of pal_idx in bytes
  // Far tiles: one bit per 8x8 tile of pal_idx (border tiles included), set where all 64 cells hold the table's most common
  // entry far_entry (free space beyond max_obstacle_distance of anything: more than half of a typical map).  Rows of
  // far_row_bytes bytes, bit (tx & 7) of byte tx >> 3.  A look-up into such a tile needs no memory access at all; the gather
  // kernel of DISPERSED sets keeps the bitmap in LDS (k_reweight_lf_palette<true, true>).  nullptr = none.
  const uint8_t* far_bits;
  uint32_t far_row_bytes;
  uint32_t far_bytes;  // size of far_bits, a multiple of 16
  uint32_t far_entry;  // LDS byte address of the common entry (as stored in pal_idx)
  // The same bits by the tile's LINEAR index (ty * tiles_x + tx = a cell's byte offset in pal_idx >> 7): bit (index & 7) of byte
  // index >> 3 - the test then starts from the offset a look-up has computed anyway (k_reweight_lf_far_beams).  nullptr = none.
  const uint8_t* far_linear;
  uint32_t far_linear_bytes;  // a multiple of 16
  // Where a particle's sum over the scan starts: 1 (likelihood_field_model.hpp:76) or 0 (the prob model's sum of logs), plus the terms
  // of the scan points that have no cell for ANY pose - NaN or infinite coordinates, taken out where the scan is staged
  // (stage_points): their count times the unknown-space term.  No kernel ever sees such a point.
  double acc0;
};

constexpr uint32_t kMaxPalette = 2048;
// Byte offset of cell (x, y), -8 <= x < W + 8, -8 <= y < H + 8, in the tiled uint16 table: tiles are 8x8 cells,
// column-major inside a tile, so x contributes a plain shift and y = (row of tiles) * pitch + (y & 7) * 2.
__host__ __device__ inline uint32_t palette_row_offset(int32_t y, uint32_t pitch) {
  const uint32_t py = static_cast<uint32_t>(y + 8);
  return (py >> 3) * pitch + ((py & 7u) << 1) + 128u;  // + 128: the x border tile
}
__host__ __device__ inline uint32_t palette_offset(int32_t x, int32_t y, uint32_t pitch) {
  return palette_row_offset(y, pitch) + (static_cast<uint32_t>(x) << 4);
}

struct GridView {
  const int8_t* cells;
  uint32_t W, H;
  double resolution;
  Pose2 origin;          // grid frame in the world
  Pose2 origin_inverse;  // world -> grid
  int8_t free_value;
};

struct BeamModel {
  double z_hit, z_short, z_max, z_rand, sigma_hit, lambda_short, beam_max_range;
};

// Where random_intersperse's random states come from (random_free_state, kernels.hip).  Likelihood-field and beam models: uniformly
// over the free cells of the occupancy grid (multivariate_uniform_distribution.hpp:126-161).  NDT model (normal != 0): N(mean, T T^T)
// as mean + T z (ndt_amcl_node.cpp:248-254; multivariate_normal_distribution.hpp:109-126), count = 1 so that the Bernoulli stream
// selects the same slots; the host fills mean / T from the estimate of the normalised set just before the draw.  Landmark and bearing
// models (box != 0): uniformly over the x-y extent of LandmarkMap::map_limits() with a uniform heading
// (MultivariateUniformDistribution<SE2d, AlignedBox2d>, multivariate_uniform_distribution.hpp:77-113), count = 1 as well.
struct FreeCells {
  const uint32_t* index;  // linear indices of free cells
  uint64_t count;
  int normal{0};
  double mean[3]{0.0, 0.0, 0.0};  // x, y, theta
  double T[9]{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // row-major
  int box{0};
  double box_min[2]{0.0, 0.0};     // x, y
  double box_extent[2]{0.0, 0.0};  // max - min
};

// The NDT model's map (ndt_kernels.hip): a dense int32 index grid over the bounding box of the map's keys with a border of 2 * reach
// cells (reach = the largest |component| of a kernel offset, at least 1), -1 where no cell is present, plus the cell records.  A
// measurement cell whose centre key lies farther than `reach` from the keys' box has no neighbour in the map (one test); any other
// centre key's offsets stay inside the grid (no per-offset test).
constexpr int kNdtMaxOffsets = 32;
struct NdtMapView {
  const int32_t* grid;  // gw x gh, row-major
  const double* cells;  // kNdtRecord doubles per map cell
  uint32_t gw;
  double inv_resolution;           // 1. / resolution (regular_grid.hpp:76)
  double key_x0, key_y0;           // key of the centre box's first cell = (smallest key) - reach
  double box_w, box_h;             // size of the centre box (key span + 2 reach)
  int32_t reach;                   // grid index of centre-box cell (0, 0) = reach * gw + reach
  double d1, d2, minimum_likelihood;
  uint32_t num_offsets;
  int32_t delta[kNdtMaxOffsets];   // dy * gw + dx of each kernel offset, in the kernel's order
};
// NDTSensorModel::operator() (ndt_sensor_model.hpp:216-239): w[i] *= 1 + sum over the k measurement cells (kNdtRecord doubles each,
// base frame) of max(sum of the present neighbours' d1 exp(-d2/2 e^T (S' + S_map)^-1 e), minimum_likelihood).  A lane per particle.
void launch_reweight_ndt(hipStream_t st, Particles p, uint64_t n, const NdtMapView& m, const double* meas, uint32_t k);
// The same weights, bit for bit, from a wave per particle with the lanes over the measurement cells (k_reweight_ndt_wave): small sets.
void launch_reweight_ndt_wave(hipStream_t st, Particles p, uint64_t n, const NdtMapView& m, const double* meas, uint32_t k);

// The same map in the hashed layout (mcl_set_ndt_map_layout; ndt_hash.h has the table, its hash and the bound on the probe): no index
// grid, so the keys' box may be of any extent.  The centre box is tested first, in doubles, exactly as with NdtMapView; inside it the
// centre key is an integer, every neighbour key is centre + (dx, dy) in 64 bits, and only a neighbour that fits an int32 is probed.
// A view of its own, not fields of NdtMapView: the three kernels that take that one (BatchItem included) stay as they are.
struct NdtHashView {
  NdtHashTable table;
  const double* cells;             // kNdtRecord doubles per map cell
  double inv_resolution;
  double key_x0, key_y0;           // as NdtMapView's ...
  double box_w, box_h;
  long long centre_x0, centre_y0;  // ... and key_x0, key_y0 as integers
  double d1, d2, minimum_likelihood;
  uint32_t num_offsets;
  int32_t offsets[2 * kNdtMaxOffsets];  // (dx, dy) of each kernel offset, in the kernel's order
};
// launch_reweight_ndt and launch_reweight_ndt_wave on such a map: the same weights, bit for bit, on every map both layouts hold.
void launch_reweight_ndt_hashed(hipStream_t st, Particles p, uint64_t n, const NdtHashView& m, const double* meas, uint32_t k);
void launch_reweight_ndt_wave_hashed(hipStream_t st, Particles p, uint64_t n, const NdtHashView& m, const double* meas, uint32_t k);

// The NDT map built on the device (ndt_build_kernels.hip): detail::to_cells with fit_points over n points, as ndt_fit_cells (ndt_host.cpp)
// does on the host - keys by truncation toward zero, cells of 5 points or more in ascending (x, y) key order, a cell's sums taken in
// input order.  Every launcher takes n > 0 points (n < 2^31), x and y interleaved.
struct NdtBuildScratch {
  unsigned long long* words[2];  // [n] each: the points' keys relative to their box, (x << 32) | y; ping-pong of the sort
  uint32_t* idx[2];              // [n] each: the point indices that travel with them
  uint32_t* table;               // [ndt_radix_table_words(n)] chunk histograms of a pass
  uint32_t* flags;               // [n] cell starts, then their exclusive scan
  uint32_t* chunk_tmp;           // [num_chunks(max(n, ndt_radix_table_words(n)))] chunk sums of the scans
  uint32_t* starts;              // [n / 5] first sorted position of every kept cell
  uint32_t* counters;            // [kNdtCounters], see below
};
enum NdtBuildCounter : int {
  kNdtCountCells = 0,    // cells kept (launch_ndt_group_points)
  kNdtCountKeptBox = 1,  // [1..5): min x, max x, min y, max y of the kept cells' relative keys; the caller sets UINT_MAX, 0, UINT_MAX, 0
  kNdtCountScratch = 5,
  kNdtCountLongestProbe = 6,  // launch_ndt_hash_insert: the most slots any key needed; the caller sets 0
  kNdtCounters = kNdtBuildCounters  // (scratch_layout.h sizes the area)
};
struct NdtBuildLayout {
  long long x0, y0;            // the key the relative keys count from
  long long grid_x0, grid_y0;  // key of the index grid's cell (0, 0)
  long long gw;
};
size_t ndt_radix_table_words(uint32_t n);
// d_box[5] = {min x, max x, min y, max y} of the points' keys and a flag: != 0 if some point is not finite or its key does not fit an
// int32.  The caller sets {INT_MAX, INT_MIN, INT_MAX, INT_MIN, 0} first.
void launch_ndt_key_box(hipStream_t st, const double* pts, uint32_t n, double resolution, int32_t* d_box);
// Stable sort of the points by key, relative to (x0, y0), over the low bits_x / bits_y bits the box's spans need; then the kept cells'
// starts marked and scanned into s.flags, their number and box into s.counters.  Returns which of the scratch's two lists is sorted.
int launch_ndt_group_points(hipStream_t st, const double* pts, uint32_t n, double resolution, int32_t x0, int32_t y0, uint32_t bits_x,
                            uint32_t bits_y, const NdtBuildScratch& s);
// The `cells` kept cells (s.counters[kNdtCountCells]) -> records (kNdtRecord doubles each), keys (x, y) and their entries in the index
// grid (set to -1 by the caller), laid out as NdtMapView wants them.  grid == nullptr (the hashed layout): no entries.
void launch_ndt_fit_cells(hipStream_t st, const double* pts, uint32_t n, const NdtBuildScratch& s, int sorted, uint32_t cells,
                          const NdtBuildLayout& lay, double* records, int32_t* keys, int32_t* grid);
// The hashed layout's table over `cells` distinct keys (x, y pairs, as launch_ndt_fit_cells leaves them): slots[0 .. mask] set to 0xFF
// bytes by the caller (every record kNdtNoRecord), mask and shift as NdtHashTable's.  Which slot a key lands in depends on the race
// between the lanes; what ndt_hash_find returns does not.  *d_longest takes the most slots any key needed (atomic max).
void launch_ndt_hash_insert(hipStream_t st, const int32_t* keys, uint32_t cells, NdtSlot* slots, uint32_t mask, uint32_t shift, uint32_t* d_longest);
// Occupancy grid -> points: offsets[i] = occupied cells before cell i in row-major order, *d_total = their number; then the centres of
// the occupied cells, origin * (resolution * (index + 0.5)), in that order.
void launch_ndt_grid_offsets(hipStream_t st, const int8_t* cells, uint32_t count, int8_t occupied, uint32_t* offsets, uint32_t* chunk_tmp,
                             uint32_t* d_total);
void launch_ndt_grid_points(hipStream_t st, const int8_t* cells, uint32_t W, uint32_t H, int8_t occupied, const uint32_t* offsets,
                            double resolution, Pose2 origin, double* pts);

// The landmark and bearing models' map and measurement (landmark_kernels.hip).  The landmarks are grouped by category on the host with
// a stable sort (map order inside a category: std::min_element's "first of equal" holds), 4 doubles each (x, y, z, 0).  A detection is
// kLandmarkRecord (10) doubles: the vector as given (x, y, z), its norm, its normalized() (x, y, z), then three uint32 in the place of
// doubles 7 and 8: first and count of its category's landmarks (count 0 = no landmark of that category, first = 0xFFFFFFFF) and the
// detection's place in the caller's order.
constexpr int kLandmarkMaxDetections = 64;  // MCL_LANDMARK_MAX_DETECTIONS
struct LandmarkMapView {
  const double* landmarks;  // 4 doubles per landmark, grouped by category
  uint32_t count;
  double den_range, den_bearing;  // (2. * sigma) * sigma
  double random_prob;
  double Rs[9];  // bearing model: sensor_pose_in_robot's rotation (row-major, Eigen's toRotationMatrix) and translation
  double ts[3];
};
// LandmarkSensorModel2d::operator() (landmark_sensor_model.hpp:92-157): w[i] *= product over the k detections of
// exp(-range_error^2 / den_range) exp(-bearing_error^2 / den_bearing) + random_prob against the nearest landmark of the detection's
// category (random_prob alone where there is none).  A lane per particle; detections in the caller's order.
void launch_reweight_landmarks(hipStream_t st, Particles p, uint64_t n, const LandmarkMapView& m, const double* detections, uint32_t k);
// BearingSensorModel2d::operator() (bearing_sensor_model.hpp:89-141): w[i] *= product over the k detections of exp(-e^2 / den_bearing), e
// the aperture between the detection and the bearing of the landmark of its category whose bearing is closest (0 where there is
// none).  `detections` are sorted by category (their record says where they stand in the caller's order, which the product follows):
// a landmark's bearing in the sensor frame is computed once per particle and serves every detection of its category.
void launch_reweight_bearings(hipStream_t st, Particles p, uint64_t n, const LandmarkMapView& m, const double* detections, uint32_t k);
// The same weights, bit for bit, from a wave per particle: the lanes over the detections, the search of a detection split over the lanes
// of its group (k_reweight_landmarks_wave, k_reweight_bearings_wave): small sets, mcl_set_landmark_small_cycle.  k <= 64.
void launch_reweight_landmarks_wave(hipStream_t st, Particles p, uint64_t n, const LandmarkMapView& m, const double* detections, uint32_t k);
void launch_reweight_bearings_wave(hipStream_t st, Particles p, uint64_t n, const LandmarkMapView& m, const double* detections, uint32_t k);

// ---- the sensor model as a function (mcl_likelihoods*): out[i] = sensor_model(measurement)(poses[i]) -------------------------------------
// The factor a reweight kernel multiplies the weight of a particle at poses[i] by, computed by that kernel's own per-pose functions, for
// n caller-given poses (cos, sin, x, y) in the caller's order.  Plain arrays in device memory: no particle set, no order, no weight.
// A launcher chunks its launches where a grid dimension would overflow; n is limited by memory alone.
constexpr uint64_t kLikelihoodsWaveMax = 4096;               // NDT, landmark, bearing: a wave per pose up to here, a lane per pose above
constexpr uint64_t kLikelihoodsLaneChunk = 1ull << 38;       // poses per launch of a lane-per-pose kernel (2^30 blocks of 256)
constexpr uint64_t kLikelihoodsWaveChunk = 1ull << 32;       // ... of a wave-per-pose kernel (2^30 blocks of four waves)
// Likelihood-field models (kernels.hip): a wave per pose, the lanes over the beams, the scan staged in LDS where it fits beside the
// palette (else read from memory); a field without a palette: a lane per pose over the f32 field.  f.acc0 as stage_points would set it.
void launch_likelihoods_lf(hipStream_t st, const double4* poses, uint64_t n, const FieldView& f, const double* d_points, uint32_t B,
                           const Tuning& tuning, double* out);
// Beam model (beam_kernels.hip): k_reweight_beam's form, a wave per pose over the scan staged in LDS (B <= 4096 points); no cell count.
// B == 0: 1.0, as launch_reweight_beam leaves the weights.
void launch_likelihoods_beam(hipStream_t st, const double4* poses, uint64_t n, GridView g, BeamModel m, const double* d_points, uint32_t B,
                             const uint32_t* nonfree_bits, double* out);
void launch_likelihoods_ndt(hipStream_t st, const double4* poses, uint64_t n, const NdtMapView& m, const double* meas, uint32_t k, double* out);
void launch_likelihoods_ndt_hashed(hipStream_t st, const double4* poses, uint64_t n, const NdtHashView& m, const double* meas, uint32_t k, double* out);
// k <= kLandmarkMaxDetections; k == 0: 1.0.  bearing: the records sorted by category, as launch_reweight_bearings takes them.
void launch_likelihoods_landmarks(hipStream_t st, const double4* poses, uint64_t n, const LandmarkMapView& m, const double* detections, uint32_t k,
                                  bool bearing, double* out);

// ---- ray casting as a function (mcl_cast_rays*; DESIGN.md "Ray casting as a function"; the host rule: raycast_host.h) --------------------
// table: B bearings (c, s) in device memory, made into the far-end vectors (c * max_range, s * max_range) in place.
void launch_cast_far_ends(hipStream_t st, double* table, uint64_t B, double max_range);
// One chunk of the flattened order i * B + b (CastChunk): poses points at the chunk's first pose, ranges / hit_cells (may be null) at its
// first ray; far_ends is the whole table.  nonfree_bits: the packed bit maps of a beam context's map (cast_ray_grid's walk), or null: the
// plain walk over g.cells (cast_ray's).  *d_steps (may be null) += the cells looked at.
void launch_cast_rays(hipStream_t st, const double4* poses, const double* far_ends, uint64_t B, const CastChunk& chunk, GridView g,
                      const uint32_t* nonfree_bits, double max_range, double* ranges, int64_t* hit_cells, unsigned long long* d_steps);

// ---- beam skipping: the cloud's vote on every beam (mcl_beam_agreement, the enabled cycle; DESIGN.md "Beam skipping") ---------------------
// count[b] = the poses i < n whose end-point of scan point b has a cell inside the grid with f.data[cell] > level - the exact cell of
// lf_beam, the f32 field itself (whatever field the view reads: nothing derived, nothing to rebuild).  pose: the particles' poses, or
// (pose_ahead) their field-frame form as FieldPoseOut left it.  d_points: B finite points (stage_points' rule: the others agree with
// no pose and are never sent).  A lane per pose, a bounded grid striding over the set, the beam uniform across the wave: a ballot and
// a popcount per beam into the workgroup's LDS counters, one vector atomicAdd per counter and workgroup at the end - integer adds, so
// the result does not depend on the geometry.  A scan of more than kBeamSkipPass beams takes a launch per pass.  Zeroes count first.
// Returns the kernel launches (0 for n == 0 or B == 0: count is not touched).
constexpr uint32_t kBeamSkipPass = 4096;  // beams of one launch: its LDS counters (16 KB)
uint32_t launch_beam_agreement(hipStream_t st, const double4* pose, bool pose_ahead, uint64_t n, const FieldView& f, float level,
                               const double* d_points, uint32_t B, uint32_t* count);

// ---- global pose search (mcl_global_search*; DESIGN.md "Global pose search"; the host rule: search_host.h) -------------------------------
struct SearchGrid {
  uint32_t W;
  double resolution;
  Pose2 origin;
};
// The selection's device arrays (SearchLayout, scratch_layout.h): two sets of sorted runs, the pool twice.
struct SearchScratch {
  unsigned long long *run_keys[2], *run_ids[2], *pool_keys[2], *pool_ids[2];
};
// Zeroes *selected_count, then compacts the cells of free_cells[0, count) that pass the stride test into `selected` (room for count; any
// order) and counts them.  Each launcher returns its kernel launches.
uint32_t launch_search_select(hipStream_t st, const uint32_t* free_cells, uint32_t count, uint32_t W, uint32_t stride, uint32_t* selected,
                              uint32_t* selected_count);
// poses[c * headings + h] = (table[h], the centre of cell selected[c] in the world), ids[...] = selected[c] * headings + h.
uint32_t launch_search_poses(hipStream_t st, const uint32_t* selected, uint32_t cells, uint32_t headings, const double* table, const SearchGrid& g,
                             double4* poses, unsigned long long* ids);
// The pool (pool_len entries in set *pool_at, sorted) becomes the best `pool` of itself and the chunk's n (score, id), sorted, in the
// other set; *pool_at is flipped.  By (key descending, id ascending), exact whatever ties there are.  n == 0: nothing.
uint32_t launch_search_pool(hipStream_t st, const double* scores, const unsigned long long* ids, uint64_t n, const SearchScratch& s, uint32_t pool,
                            uint32_t pool_len, int* pool_at);

// ---- local pose search (mcl_local_search*; DESIGN.md "Local pose search"; the host rule: local_search_host.h) ---------------------------
struct LocalLattice {
  uint32_t Kx, Kt;  // half steps
  uint32_t nx, nt;  // 2 K + 1
  uint32_t L;       // nx * nx * nt candidates per seed
};
constexpr int kLocalReduceBlock = 256;
constexpr uint32_t kLocalResultDoubles = 12;  // per seed: the ten sums | the best score | the seed's score
constexpr uint32_t kLocalResultWords = 2;     // per seed: the best candidate's tie key (its id in the low 20 bits) | plateau
// poses[s * L + id] for the `seeds` seeds of a pass, a lane per candidate: (rot[s * nt + k + Kt], seed_xy[s] + (off[i + Kx], off[j + Kx])).
// seed_xy and rot start at the pass's first seed.
uint32_t launch_local_generate(hipStream_t st, const double* seed_xy, const double* rot, const double* off, uint32_t seeds, const LocalLattice& lat,
                               double4* poses);
// One workgroup per seed of the pass over its L scores (scores + s * L): the best by (score key descending, tie key ascending), the ten
// sums by a fixed tree (a lane's candidates in ascending order, the wave's lanes by wave_sum_f64, the waves in order), the plateau
// count in a second sweep.  out_f64 + s * kLocalResultDoubles, out_u64 + s * kLocalResultWords.
uint32_t launch_local_reduce(hipStream_t st, const double* scores, uint32_t seeds, const LocalLattice& lat, double* out_f64,
                             unsigned long long* out_u64);

struct HashParams {
  double res_x, res_y, res_theta;
};

struct ResampleArgs {
  uint64_t seed;
  uint32_t step;
  double random_state_probability;
  const double* d_random_state_probability;  // if set, read the probability from device memory instead (the recovery estimator's output, see RecoveryPolicy)
  uint64_t n_in;            // live particles of the source set
  uint64_t first_candidate; // global index of candidate 0 of this launch
  uint64_t count;           // candidates in this launch
  uint64_t out_offset;      // where candidate `first_candidate` lands in the output set
};

// Position of the cell (a0, a1, a2), `bits` bits each (bits <= 6), along the 3-D Hilbert curve through the (2^bits)^3 cells
// (Skilling's transpose form, "Programming the Hilbert curve", 2004: undo the excess work, Gray-encode, interleave with a0 most
// significant).  Consecutive positions are face neighbours, so ANY run of the order is a connected, compact set of cells - a run
// of the Morton order that crosses a high-level boundary of the Z curve is two pieces far apart, and the workgroup that holds it
// (448 consecutive particles of the order, k_reweight_lf_patch) fits no LDS patch.  The curve enters at (0, 0, 0) and leaves at
// (2^bits - 1, 0, 0): with the heading on axis 0, the slabs of the key's top heading bits chain into one continuous curve.
template <uint32_t bits>
__host__ __device__ inline uint32_t hilbert_index_3_fixed(uint32_t a0, uint32_t a1, uint32_t a2) {
  const uint32_t mask = (1u << bits) - 1u;
  uint32_t x0 = a0 & mask, x1 = a1 & mask, x2 = a2 & mask;
#pragma unroll
  for (uint32_t q = 1u << (bits - 1); q > 1; q >>= 1) {
    const uint32_t p = q - 1;
    x0 ^= (x0 & q) ? p : 0u;  // axis 0 against itself: invert or nothing
    {
      const uint32_t t = (x0 ^ x1) & p;
      const bool inv = (x1 & q) != 0;
      x0 ^= inv ? p : t;
      x1 ^= inv ? 0u : t;
    }
    {
      const uint32_t t = (x0 ^ x2) & p;
      const bool inv = (x2 & q) != 0;
      x0 ^= inv ? p : t;
      x2 ^= inv ? 0u : t;
    }
  }
  x1 ^= x0;
  x2 ^= x1;
  uint32_t t = 0;
#pragma unroll
  for (uint32_t q = 1u << (bits - 1); q > 1; q >>= 1) t ^= (x2 & q) ? q - 1 : 0u;
  x0 ^= t;
  x1 ^= t;
  x2 ^= t;
  auto spread = [](uint32_t v) {  // ..fedcba -> f00e00d00c00b00a
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
  };
  return (spread(x0) << 2) | (spread(x1) << 1) | spread(x2);
}
__host__ __device__ inline uint32_t hilbert_index_3(uint32_t a0, uint32_t a1, uint32_t a2, uint32_t bits) {  // straight-line code per width
  switch (bits) {
    case 1: return hilbert_index_3_fixed<1>(a0, a1, a2);
    case 2: return hilbert_index_3_fixed<2>(a0, a1, a2);
    case 3: return hilbert_index_3_fixed<3>(a0, a1, a2);
    case 4: return hilbert_index_3_fixed<4>(a0, a1, a2);
    case 5: return hilbert_index_3_fixed<5>(a0, a1, a2);
    default: return hilbert_index_3_fixed<6>(a0, a1, a2);
  }
}
struct SortScratch {
  uint32_t* keys;                // [n] key of particle i
  uint32_t* perm;                // [n] sorted position -> particle index
  uint32_t* table;               // [kSortDigits][nblocks] block histograms -> exclusive offsets (reused by both passes)
  uint32_t* totals;              // [kSortDigits] digit totals
  uint32_t* bases;               // [kSortDigits] their exclusive scan (the buckets' first positions), then [16] flags ([0]: some bucket
                                 // is beyond kSortHugeBucket) - written by the first pass's first workgroup
  unsigned long long* keyidx;    // [n] (high digit << 32 | index) after the first pass
  double* bbox;                  // [8] min/max of x, y, relative heading
  double* bbox_partials;         // [6][nblocks] their per-chunk partials
  KeyFrame* frame;               // key frame derived from the bounding box (device-resident fallback)
  double* partial;               // [kLfMaxSegments][min(n, 262144)] scan-segment sums (medium particle counts); may be null
};

// K1  actions/propagate.hpp:57-79 + differential_drive_model.hpp:156-163
// scan_src / scan_dst (optional): the cycle's scan, copied by the kernel from mapped pinned host memory into HBM (no
// copy-engine hand-off on the stream).  sort + frame (optional): the kernel also emits the ordering keys and the first
// pass's block histograms (launch_order_particles then skips its own key pass).
void launch_propagate(hipStream_t st, Particles p, uint64_t n, DiffDriveSampler smp, uint64_t seed, uint32_t step,
                      uint64_t index_offset, const double* scan_src = nullptr, double* scan_dst = nullptr, uint32_t scan_doubles = 0,
                      const SortScratch* sort = nullptr, const KeyFrame* frame = nullptr, const double* normals_ahead = nullptr,
                      uint64_t normals_stride = 0, FieldPoseOut field = FieldPoseOut{nullptr, Pose2{Rot2{1.0, 0.0}, 0.0, 0.0}});
// field.pose[i] = world_to_field * pose[i], i < n, as a propagation with `field` leaves it: the rebuild for a set whose poses something
// else has written (k_field_pose; cycle_host.h field_pose_plan says when).
void launch_field_pose(hipStream_t st, const double4* pose, uint64_t n, const FieldPoseOut& field);
// The propagation's standard normals per particle for `step`, drawn ahead of the cycle that uses them (k_noise_ahead: the three the motion
// models use, as three arrays of n doubles): launch_propagate(..., normals_ahead, stride = that n) then reads them instead of drawing (not the
// small-set kernel).  Same bits.
void launch_noise_ahead(hipStream_t st, uint64_t seed, uint32_t step, uint64_t index_offset, uint64_t n, double* d_normals);
void launch_pull_scan(hipStream_t st, const double* scan_src, double* scan_dst, uint32_t scan_doubles);
// Full sort of the particles by the ordering key -> sort->perm.  frame == nullptr: bounding-box pass + device-resident frame.
// keys_ready: launch_propagate already wrote sort->keys and the first pass's block histograms.
// layout: KeyFrame::layout of the device-resident frame (a host frame carries its own).
void launch_order_particles(hipStream_t st, Particles p, uint64_t n, const SortScratch* sort, const KeyFrame* frame, bool keys_ready,
                            uint32_t layout = 0);
// The same order a cycle AHEAD: sort->keys hold the keys the draw kernel predicted for the next cycle (launch_resample_draw_and_estimate,
// keys_ahead) - their block histograms and the three ordering kernels -> sort->perm.  `done`: how much of that the draw's launcher has
// enqueued already (its return value); the rest follows here.
enum OrderAheadDone : int {
  kOrderAheadKeys = 0,         // the keys alone: k_key_hist, k_row_scan and the two sorting kernels follow
  kOrderAheadHalfColumns = 1,  // the draw kernel counted its keys (half-column histograms in the words of sort->keyidx): from k_row_scan on
  kOrderAheadTable = 2         // and the row scan ran in k_final_rows' launch: the two sorting kernels follow
};
void launch_order_ahead(hipStream_t st, uint64_t n, const SortScratch* sort, OrderAheadDone done = kOrderAheadKeys);
// K2  actions/reweight.hpp:53-60 + likelihood_field_model.hpp:68-91
// The LDS-patch kernel's running totals and scratch (LfReweightArgs::stats).
struct PatchStats {
  unsigned long long* device;  // [3]: groups planned, groups through a patch, workgroups reported (never reset)
  unsigned long long* mirror;  // [3]: mapped host copy of the first two, written by the last workgroup of a launch, and their
                               // low halves packed into one word (planned | through << 32: one store, read without synchronisation)
  uint32_t loose_below;        // a workgroup with fewer than loose_below / 256 of its groups fitting a patch gathers them all
  uint32_t isotropic_margin;   // 1: the rotation part of the bound as |R_p - R_ref| |q| on both axes (Tuning::lf_margin = 0)
  uint32_t split_patches;      // 1: a group that fits no whole patch may go through two half patches (Tuning::lf_split)
  double* weight_sums;         // optional: [workgroups] sums of the new weights, one per workgroup of the patch kernel (the
                               // normalisation's input: launch_sum_and_normalize); only written by single-segment launches
  unsigned int* arrivals;      // the queue of blocks (k_reweight_lf_patch<true>): the next block to take; wraps to 0 behind a launch's last fetch
};
// A cycle's inputs to the LF reweight.
struct LfReweightArgs {
  Particles p;
  uint64_t n;
  FieldView f;
  const double* d_points;
  uint32_t B;
  const SortScratch* sort;  // the set is ordered (sort->perm, launch_order_particles): the ordered kernels; nullptr: not ordered
  bool patches, beams;  // the cycle's mode: the LDS-patch kernel where it fits (dense sets); k_reweight_lf_beams (dispersed sets)
  bool dispersed;       // the set is reported as dispersed: the far-tile bitmap where it applies
  double scan_cells;    // max |x| + |y| of the scan points in cells (NaN: unknown); the FMA variant needs fewer than 8192
  bool unit_weights;    // every old weight is 1.0 (the patch and far-beams kernels do not load them)
  PatchStats stats;
  const double4* field_pose;  // the field-frame poses of p, current (FieldPoseOut): the kernels load them; nullptr: they form the product
};
// The kernel that ran: k_reweight_lf_patch<false> / <true>, _far_beams, _palette<true, true> / <true> / <false>, _sorted<true> /
// <false> over the order, _beams, _sorted<false> in index order.  The first five are the FMA variant.
enum class LfKernel { kNone, kPatch, kPatchQueue, kFarBeams, kPaletteFar, kPaletteFast, kPaletteExact, kSortedCube, kSortedField, kBeams, kIndexOrder };
// kernel: kNone where n == 0; weight_sums: workgroup sums of the new weights left in stats.weight_sums (0: another kernel, or segments)
struct LfLaunch { LfKernel kernel; uint32_t weight_sums; };
// The one place that chooses the LF kernel (from the arguments and `tuning`); launches it.
LfLaunch launch_reweight_lf(hipStream_t st, const LfReweightArgs& a, const Tuning& tuning);
// Its answer where that is k_reweight_lf_beams (LfKernel::kBeams), without launching; lf_palette_lds: that kernel's workgroup memory.
bool lf_takes_beams(const LfReweightArgs& a, const Tuning& tuning);
inline size_t lf_palette_lds(const FieldView& f) { return static_cast<size_t>(f.pal_base) + static_cast<size_t>(f.pal_count) * sizeof(double); }
// K2' beam_model.hpp:104-150 + raycasting.hpp:62-107 + bresenham.hpp:84-160
// `sorted` != nullptr: lane-per-ordered-particle variant (needs launch_order_particles first).
// d_beam_points: scratch of kBeamPointDoubles * B doubles (per-beam terms shared by all particles; ordered variant only).
constexpr uint32_t kBeamPointDoubles = 5;
// d_beam_table (optional, ordered variant): launch_beam_table's output, beam_table_count entries of 4 doubles
// w[perm[t]] *= the sum of a scan's segment sums partial[s][t] (mode 0: 1 + sum, 1: exp(sum), 2: sum - the beam model), segments in order
void launch_lf_combine(hipStream_t st, double* w, uint64_t n, const uint32_t* perm, const double* partial, uint32_t segments, int mode);
void launch_reweight_beam(hipStream_t st, Particles p, uint64_t n, GridView g, BeamModel m, const double* d_points, uint32_t B,
                          unsigned long long* d_steps, const SortScratch* sorted, const uint32_t* nonfree_bits, double* d_beam_points,
                          const double* d_beam_table = nullptr, uint32_t beam_table_count = 0, bool free_ahead = true, bool sectors = true);
// The beam model's terms that depend on the expected range alone, tabulated over the squared cell distance of the hit (beam_kernels.hip
// BeamTable): entries = beam_table_entries(...) (0: the range spans too many cells for a table), 4 doubles each.
constexpr double kBeamTableMaxCells = 2046.0;
// The longest line the beam kernels walk, in cells between the source and the far end (beam_max_range / resolution, + a cell for the
// roundings): below 2^27, so that 16 * span - walk_blocks' 8 * dminor and q * dmajor - stays an int.  mcl_reweight / mcl_update refuse more.
constexpr double kBeamMaxReachCells = 134217726.0;  // 2^27 - 2
uint32_t beam_table_entries(double beam_max_range, double resolution);
void launch_beam_table(hipStream_t st, BeamModel m, double resolution, uint32_t entries, double* table);
// The occupancy the ray walks read, in one buffer of nonfree_words(W, H) words: one bit per cell (1 = not free), ceil(W/32)
// words per row, followed by two coarse bitmaps — one bit per 8 x 8-cell block, "any cell not free" — row-major and column-major —
// and the block distance map (one byte per block).
struct NonFreeBits {
  const uint32_t* fine;
  const uint32_t* rows;     // [ceil(H/8)][row_words]
  const uint32_t* columns;  // [ceil(W/8)][column_words]
  const uint8_t* dist;      // [ceil(H/8)][dist_stride]: Chebyshev distance, in blocks, to the nearest block with a bit in `rows`
                            // (0 = the block itself), capped at 17
  uint32_t words_per_row, row_words, column_words, dist_stride;
};
NonFreeBits nonfree_layout(uint32_t W, uint32_t H, uint32_t* base);
size_t nonfree_words(uint32_t W, uint32_t H);
void launch_pack_nonfree(hipStream_t st, const int8_t* cells, uint32_t W, uint32_t H, int8_t free_value, uint32_t* bits);
// The dynamic-LDS opt-ins of the kernels that need one (configure_beam_kernels: the ordered beam kernel's).  They are per device:
// mcl_create calls this for every context, after hipSetDevice.
hipError_t configure_device_kernels();
hipError_t configure_beam_kernels();

// ---- the range table of the beam model (mcl_build_range_table; DESIGN.md "Range table for the beam model"; the host rule:
// range_table_host.h) ---------------------------------------------------------------------------------------------------------------------
// table[(y * W + x) * A + k]: the squared cell distance from cell (x, y) to the cell the exact rule's cast hits along bin k's bearing
// from the cell's centre, in the grid frame; kRangeTableNoHit without a hit.
struct RangeTableView {
  const uint32_t* entries;
  uint32_t A;
};
// One launch of the build (RangeTableLaunch): entries first_entry .. + entries of `table`.  bearings_cs: the A bearings (cos, sin) in
// device memory.  nonfree_bits: the packed bit maps of a beam context's map, or null: the plain walk over g.cells.
void launch_build_range_table(hipStream_t st, GridView g, const uint32_t* nonfree_bits, const double* bearings_cs, uint32_t A,
                              const RangeTableLaunch& launch, double max_range, uint32_t* table);
// The table reweight's per-beam entries (z, exp(-lambda_short z), the tail, beta = atan2(py, px)): kBeamLutPointDoubles * B doubles.
constexpr uint32_t kBeamLutPointDoubles = 4;
constexpr uint32_t kBeamLutMaxPoints = 4096;     // the points a beam context takes (reweight_preconditions, likelihoods_points)
constexpr size_t kBeamLutLds = 128 * 1024;       // ... staged in workgroup memory
void launch_beam_lut_points(hipStream_t st, const double* d_points, uint32_t B, BeamModel m, double* d_lut_points);
// p.w[i] *= the beam model's sum over the scan with the expected ranges read from the table; serves every set size, orders nothing,
// counts no cells.  d_beam_table / beam_table_count: launch_beam_table's output, or null / 0: a lane evaluates the entry itself.
void launch_reweight_beam_lut(hipStream_t st, Particles p, uint64_t n, GridView g, BeamModel m, RangeTableView t, const double* d_beam_table,
                              uint32_t beam_table_count, const double* d_lut_points, uint32_t B);
// out[i] = that sum for the caller's pose i.  B == 0: 1.0.
void launch_likelihoods_beam_lut(hipStream_t st, const double4* poses, uint64_t n, GridView g, BeamModel m, RangeTableView t,
                                 const double* d_beam_table, uint32_t beam_table_count, const double* d_lut_points, uint32_t B, double* out);

// Deterministic chunked reductions / scans: kChunk consecutive elements per workgroup, num_chunks(n) of them (scratch_layout.h).

// K3a: partial[b] = sum of w over chunk b ; then d_out[0] = sum of partials (fixed order).
// host_mirror (here and below, optional): mapped pinned-host memory that also receives the result
void launch_weight_sum(hipStream_t st, const double* w, uint64_t n, double* d_partials, double* d_out, double* host_mirror = nullptr);
// K3b: w[i] /= *d_factor unless |factor-1| < eps (normalize.hpp:73-82); chunk sums of the new w and w^2;
//      d_out[0] = total of new w, d_out[1] = total of squares.
void launch_normalize(hipStream_t st, double* w, uint64_t n, const double* d_factor, double* d_chunk_sum, double* d_chunk_sumsq,
                      double* d_out, double* host_mirror = nullptr);
// known_partials (optional): `known_count` sums whose total is the normalisation factor (PatchStats::weight_sums) - k_chunk_sum is skipped
void launch_sum_and_normalize(hipStream_t st, double* w, uint64_t n, double* d_partials, double* d_chunk_sum, double* d_chunk_sumsq,
                              double* d_sums, double* host_mirror, bool finalize = true, const double* known_partials = nullptr,
                              uint32_t known_count = 0, bool store_weights = true);
// ThrunRecoveryProbabilityEstimator (thrun_recovery_probability_estimator.hpp:69-89, exponential_filter.hpp:32-44) evaluated
// on the device so that a cycle without host-side decisions needs no mid-cycle read-back: d_policy = {slow, fast, p}.
// It rides on the workgroup that adds up the totals of the normalised weights (launch_cdf / launch_norm_finalize).
struct RecoveryPolicy {
  double alpha_slow, alpha_fast;
  int resampling;       // this cycle resamples: reset the filters when p > 0 (amcl_core.hpp:184-186)
  double* d_policy;     // {slow, fast, p}
  double* host_mirror;  // optional: p at [2]
};
// d_sums[0] = sum, d_sums[1] = sum of squares of the normalised weights (from k_normalize's chunk rows) + optional policy step.
void launch_norm_finalize(hipStream_t st, const double* d_chunk_sum, const double* d_chunk_sumsq, uint64_t n, double* d_sums,
                          double* sums_mirror, const RecoveryPolicy* policy);
// K5: cdf[i] = inclusive scan of w; d_chunk_sum is recomputed; d_total[0] = cdf[n-1].
// 16-ary search tree over the cdf: level l (l = 1 .. depth) keeps every 16^l-th cumulative sum (the last of each group
// of 16 entries of the level below, one 128-byte line per group), so that std::lower_bound touches one line per level.
// Pure comparisons: the result is exactly cdf_lower_bound's.
// A launch's own completion word (k_final_rows): d_ticket counts its workgroups (never reset), host_flag is a word of mapped host
// memory that receives seq when the last of them is done, behind everything the launch mirrored to the host.
struct Completion {
  unsigned long long* d_ticket{nullptr};
  unsigned long long* host_flag{nullptr};
  unsigned long long seq{0};
};
constexpr int kCdfTreeMaxDepth = 8;
struct CdfTree {
  const double* cdf;
  const double* levels;                   // level 1 first
  uint32_t offset[kCdfTreeMaxDepth];      // of level l + 1 inside `levels`
  uint32_t size[kCdfTreeMaxDepth];
  int depth;                              // number of sampled levels (0 for n <= 16)
  uint64_t n;
};
inline uint64_t cdf_tree_doubles(uint64_t n) { return n / 15 + 32 * kCdfTreeMaxDepth; }
inline CdfTree make_cdf_tree(const double* cdf, const double* levels, uint64_t n) {
  CdfTree t{};
  t.cdf = cdf;
  t.levels = levels;
  t.n = n;
  uint64_t size = n, off = 0;
  while (size > 16 && t.depth < kCdfTreeMaxDepth) {
    size = (size + 15) / 16;
    t.offset[t.depth] = static_cast<uint32_t>(off);
    t.size[t.depth] = static_cast<uint32_t>(size);
    off += (size + 15) & ~15ull;  // every group of 16 entries in a 128-byte line of its own
    ++t.depth;
  }
  return t;
}
// launch_cdf also fills the tree levels when `tree_levels` is given (cdf_tree_doubles(n) doubles).
// finalize_*: the first workgroup also leaves the totals of known_chunk_sum / finalize_sumsq in finalize_sums[0..1] and runs
// the recovery estimator (see launch_norm_finalize) — for the cycle that goes straight from k_normalize into a resample.
void launch_cdf(hipStream_t st, const double* w, uint64_t n, double* d_chunk_sum, double* d_chunk_offset, double* cdf,
                double* d_total, double* tree_levels, const double* known_chunk_sum = nullptr, const double* finalize_sumsq = nullptr,
                double* finalize_sums = nullptr, double* finalize_mirror = nullptr, const RecoveryPolicy* policy = nullptr,
                const double* d_factor = nullptr);
// Normalisation by the set's own total + totals of the normalised weights (+ recovery estimator) + CDF and its search tree in one launch
// (k_normalize_cdf): what launch_sum_and_normalize(finalize = false) followed by launch_cdf(known chunk sums, finalize arguments) leave,
// bit for bit.  known_partials as in launch_sum_and_normalize (nullptr: k_chunk_sum into d_partials first).  scan_state: kScanStateWords
// words of 8 bytes, zero when allocated, owned by the context; epoch: nonzero, another one than the previous launch's on that state.
// write_weights = false: the normalised weights themselves are not stored (a cycle that resamples at once never reads them).
// Returns false, nothing launched, where the set is beyond what the kernel takes (more than 2M particles).
constexpr size_t kScanStateWords = 8 + 4 * 1024;
bool launch_normalize_cdf(hipStream_t st, double* w, uint64_t n, double* d_partials, const double* known_partials, uint32_t known_count,
                          double* d_sums, double* sums_mirror, double* d_chunk_sum, double* d_chunk_sumsq, bool write_weights, double* cdf,
                          double* d_total, double* tree_levels, const RecoveryPolicy* policy, unsigned long long* scan_state, uint32_t epoch);
// The context's block of kScalarSlots doubles, held twice: d_scalars in device memory and its mirror h_scalars in mapped host memory
// (kernels see it as hd_scalars).  "mirrored": a kernel stores the value into both and the host reads the mirror behind a
// synchronisation; "device": only the device block holds it; "host": only the mirror does.  A range names its first slot.
enum ScalarSlot : int {
  kSlotWeightSum = 0,     // mirrored: the total of the weights before the normalisation
  kSlotNormSum = 1,       // mirrored: sum of the normalised weights
  kSlotNormSumSq = 2,     // mirrored: sum of their squares
  kSlotFactor = 3,        // device: the normalisation's factor when the caller gives one (uploaded through the same host slot)
  kSlotCdfTotal = 4,      // device: the CDF's total (mcl_cdf_total copies it to the same host slot)
  kSlotResampled = 5,     // mirrored, k_small_tail: 1 if the cycle resampled, else 0
  kSlotParticles = 6,     // mirrored, k_small_tail: particles after the cycle
  kSlotEss = 7,           // mirrored, k_small_tail: effective sample size (-1: not evaluated)
  kSlotEstimate = 8,      // mirrored: [8..17) the nine sums of the estimate (estimation.hpp:436-475)
  kSlotOverflow = 17,     // mirrored, sharded cycle: the ranks' overflow flags of the fixed-capacity exchange, summed with the estimate's
  kSlotSlow = 18,         // mirrored, k_small_tail: the recovery filters' new outputs
  kSlotFast = 19,
  kSlotPolicy = 20,       // [20..23) the device-side recovery estimator (RecoveryPolicy::d_policy): {slow, fast, p}; p is mirrored
  kSlotPolicyFast = 21,
  kSlotPolicyP = 22,      // the random state probability
  kSlotHandBack = 23,     // mirrored, k_small_tail on an NDT context: 1 if the tail handed the cycle back behind the policies, else 0
  kSlotPatchTotals = 24,  // device: [24..27) the LDS-patch kernel's running totals (PatchStats::device, 64-bit words)
  kSlotDoneTicket = 27,   // device: the completion ticket (Completion::d_ticket, a 64-bit word)
  kSlotPatchMirror = 28,  // host: [28..31) the patch totals as the kernel copies them (PatchStats::mirror, 64-bit words)
  kSlotPatchQueue = 30,   // device: the patch kernel's queue of blocks (PatchStats::arrivals, a 32-bit word)
  kSlotDoneWord = 31,     // host: the completion word (Completion::host_flag, a 64-bit word)
  kScalarSlots = 32
};
static_assert(kSlotEstimate + 9 == kSlotOverflow && kSlotPolicyP < kSlotHandBack && kSlotHandBack < kSlotPatchTotals && kSlotPatchTotals + 3 == kSlotDoneTicket &&
                  kSlotDoneWord < kScalarSlots,
              "the scalar block's ranges overlap or do not fit in kScalarSlots doubles");
// The whole tail of a small set's cycle - normalise, policies, resample (fixed size or KLD-adaptive), estimate sums - in one launch of one
// workgroup (k_small_tail; sets and candidate streams of up to 4096 particles).  Results through `mirror` (the mapped host block) and
// d_scalars: the slots marked k_small_tail above, kSlotWeightSum .. kSlotNormSumSq, kSlotEstimate and kSlotPolicy's three.  fires: every_n
// says so this cycle.  Returns false, nothing launched, where the set does not fit.
// hand_back (an NDT context, mcl_set_ndt_small_cycle): a cycle that resamples with a random state probability > 0 ends behind the
// policies - the normalised weights stored, the scalars mirrored with the recovery filters NOT reset, kSlotResampled 0, kSlotHandBack 1 -
// and draws nothing: the host builds the generator of the random states and finishes the cycle.  Every other cycle as without it.
struct SmallTail {
  Particles src, dst;
  uint32_t n, min_particles, max_particles;
  uint64_t seed;
  uint32_t step;
  bool fires, selective;
  double alpha_slow, alpha_fast, slow, fast, kld_epsilon, kld_z;
  HashParams hp;
  GridView g;
  FreeCells fc;
  double pivot_x, pivot_y;
  double* mirror;
  double* d_scalars;
  unsigned long long* done_flag{nullptr};  // completion word in mapped host memory (optional) and the value it takes
  unsigned long long done_seq{0};
  bool hand_back{false};
};
bool launch_small_tail(hipStream_t st, const SmallTail& t);
// The kernel's own argument record (k_small_tail takes it by value, k_batch_small_tail from its member's BatchItem).
struct SmallTailArgs {
  Particles src, dst;
  uint32_t n;               // live particles
  uint32_t min_particles, max_particles;
  uint64_t seed;
  uint32_t step;
  int fires;                // every_n says so
  int selective;            // && on_effective_size_drop
  int adaptive;             // min < max: take_while_kld
  double alpha_slow, alpha_fast, slow, fast;  // the recovery estimator's filters (the host keeps their state)
  double two_epsilon, z;
  HashParams hp;
  GridView g;
  FreeCells fc;
  double pivot_x, pivot_y;
  double* out;              // [kScalarSlots] mirror in mapped host memory (the context's h_scalars): see the stores below
  double* d_out;            // the same values in device memory (d_scalars)
  unsigned long long* done_flag;  // optional: a word of mapped host memory that takes done_seq behind everything mirrored (cycle_spin)
  unsigned long long done_seq;
  int hand_back;            // NDT: end behind the policies where the cycle resamples with p > 0 (SmallTail::hand_back)
};
SmallTailArgs small_tail_args(const SmallTail& t);
bool small_tail_fits(uint64_t n, uint64_t max_particles);  // launch_small_tail's own test: both 1 .. 4096

// ---- a batch of small filters (mcl_batch_update): the small cycle's three kernels over many sets in one launch each ----------------------
// One member's cycle, as k_propagate_small, its reweight kernel - k_reweight_lf_beams (a wave per particle) for the likelihood-field
// kinds, k_reweight_beam for the beam model - and k_small_tail take it.  The host fills one record per fused member and cycle; every
// kernel of the cycle gets the device table.
// k_reweight_beam's arguments beyond the set and the scan (batch_beam_record fills it as launch_reweight_beam fills the lone launch).
struct BatchBeam {
  GridView g;
  BeamModel m;
  NonFreeBits bits;             // all zero: no packed occupancy, the walk reads the cells
  unsigned long long* d_steps;  // the member's count of cells visited (mcl_beam_cells_visited)
};
BatchBeam batch_beam_record(GridView g, BeamModel m, const uint32_t* nonfree_bits, unsigned long long* d_steps);
struct BatchItem {
  Particles p;  // the live set
  uint64_t n;
  DiffDriveSampler smp;  // k_propagate_small's arguments
  uint64_t seed;
  uint32_t step;
  uint64_t index_offset;
  const double* scan_src;  // the member's staged scan in mapped host memory (nullptr: an empty scan, nothing pulled)
  double* scan_dst;        // ... and where the reweight reads it
  uint32_t scan_doubles;
  FieldPoseOut field_out;      // ... and where it leaves the field-frame poses (a likelihood-field member with lf_pose_ahead; else null)
  const double4* field_pose;   // k_reweight_lf_beams' field-frame poses (nullptr: it forms them)
  FieldView f;  // k_reweight_lf_beams' arguments (its points are scan_dst); a beam member's stays zero
  uint32_t B;   // the scan's points, of either family
  SmallTailArgs tail;
  uint32_t first_propagate_block, first_reweight_block;  // batch_layout (a beam member has no block in the second)
  BatchBeam beam;             // a beam member's k_reweight_beam arguments; a likelihood-field member's stays zero
  uint32_t first_beam_block;  // batch_beam_layout (a likelihood-field member has no block)
  NdtMapView ndt;             // an NDT member's k_reweight_ndt_wave arguments (its measurement cells are scan_dst); another member's stays zero
  uint32_t ndt_cells;         // ... the staged measurement cells, kNdtRecord doubles each
  uint32_t first_ndt_block;   // batch_ndt_layout (a member of another family has no block)
  LandmarkMapView landmark;   // a landmark or bearing member's wave kernel arguments (its detection records are scan_dst); else zero
  uint32_t landmark_k;        // ... the staged detection records, kLandmarkRecord doubles each
  uint32_t landmark_bearing;  // ... 1: the bearing model's body, 0: the landmark model's
  uint32_t first_landmark_block;  // batch_landmark_layout (a member of another family has no block)
};
// k_batch_propagate, k_batch_reweight_lf_beams (if grid.reweight_blocks), k_batch_reweight_beam (if beam.blocks), k_batch_reweight_ndt (if
// ndt_blocks), k_batch_reweight_landmarks (if landmark_blocks), k_batch_small_tail over d_items[0 .. grid.members), in this order on `st`.
// Returns the kernels enqueued.
uint32_t launch_batch_cycle(hipStream_t st, const BatchItem* d_items, const BatchGrid& grid, const BatchBeamGrid& beam, uint32_t ndt_blocks = 0,
                            uint32_t landmark_blocks = 0);
void launch_batch_reweight_landmarks(hipStream_t st, const BatchItem* d_items, uint32_t members, uint32_t blocks);  // (landmark_kernels.hip)
void launch_batch_reweight_ndt(hipStream_t st, const BatchItem* d_items, uint32_t members, uint32_t blocks);  // (ndt_kernels.hip)
void launch_batch_reweight_beam(hipStream_t st, const BatchItem* d_items, uint32_t members, const BatchBeamGrid& grid);  // (beam_kernels.hip)
// K6: one thread per candidate (views/sample.hpp:102,133-135; random_intersperse.hpp:90-115; particle_traits.hpp:105).
void launch_resample_draw(hipStream_t st, Particles src, CdfTree cdf, const double* d_total, Particles dst,
                          ResampleArgs a, GridView g, FreeCells fc, HashParams hp, unsigned long long* d_hashes);
// hist_sort (with keys_ahead = hist_sort->keys; Tuning::draw_key_hist): the draw kernel also counts the high digits of the keys it stores, the
// ordering's first-pass histograms; rows_merged (Tuning::rows_merged): the row scan over them runs in the launch of k_final_rows.  Returns how
// far the ordering of the keys got (launch_order_ahead's `done`).
OrderAheadDone launch_resample_draw_and_estimate(hipStream_t st, Particles src, CdfTree cdf, const double* d_total, Particles dst, ResampleArgs a,
                                                 GridView g, FreeCells fc, HashParams hp, double pivot_x, double pivot_y, double* d_partials,
                                                 double* d_sums, double* host_mirror, const Completion* done = nullptr,
                                                 unsigned int* fold_ticket = nullptr, double* normals_ahead = nullptr,
                                                 uint64_t normals_stride = 0, uint64_t normals_index_offset = 0, uint32_t normals_step = 0,
                                                 uint32_t* keys_ahead = nullptr, const DiffDriveSampler* predicted = nullptr,
                                                 const KeyFrame* frame_ahead = nullptr, const SortScratch* hist_sort = nullptr,
                                                 bool rows_merged = false);
// Sharded variant: targets given, no RNG (mcl_gather_by_cdf).
// Sharded resampling helpers (mcl_resample_targets / mcl_commit_resampled).
void launch_resample_targets(hipStream_t st, uint64_t seed, uint32_t step, double p, double total, uint64_t first_slot,
                             uint64_t count, uint64_t n_free, double* d_targets, const double* d_plan = nullptr);
// Sharded fixed-size cycle: CDF intervals, global total, totals of the normalised weights and the recovery estimator from the
// gathered shard statistics, on the device (d_plan = {total, random state probability}; d_intervals = ends[world], offsets[world]).
struct RecoveryPolicy;
void launch_shard_plan(hipStream_t st, const double* d_stats, uint32_t world, uint64_t n_total, double* d_sums, double* sums_mirror,
                       const RecoveryPolicy& policy, double* d_intervals, double* d_plan);
// Counting sort of resample targets by owning shard; d_block_hist needs world * num_chunks(count) words.
void launch_route_targets(hipStream_t st, const double* d_targets, uint64_t count, const double* d_ends, const double* d_offsets,
                          uint32_t world, uint32_t self_rank, uint8_t* d_dest, uint32_t* d_block_hist, uint32_t* d_chunk_sum,
                          uint32_t* d_chunk_off, double* d_send_targets, uint32_t* d_order, long long* d_counts, uint32_t pad_capacity = 0,
                          double* d_overflow = nullptr);
void launch_gather_by_cdf_aos(hipStream_t st, Particles src, CdfTree cdf, const double* d_targets, uint64_t m,
                              double* d_out);
void launch_commit_routed(hipStream_t st, Particles dst, uint64_t seed, uint32_t step, uint64_t first_slot, uint64_t count,
                          const double* d_replies, const uint32_t* d_order, const double* d_targets, GridView g, FreeCells fc);
// The fixed-capacity exchange keeps injected slots (NaN targets) out of its request lists: their random states, straight from d_targets.
void launch_commit_injected(hipStream_t st, Particles dst, uint64_t seed, uint32_t step, uint64_t first_slot, uint64_t count,
                            const double* d_targets, GridView g, FreeCells fc);
// K7: exact parallel take_while_kld (take_while_kld.hpp:72-88).
void launch_finish_candidates(hipStream_t st, uint64_t seed, uint32_t step, uint64_t first_slot, uint64_t count, const double* d_replies,
                              const uint32_t* d_order, const double* d_targets, GridView g, FreeCells fc, HashParams hp,
                              double* d_states, unsigned long long* d_hashes);
struct KldTable {
  unsigned long long* keys;  // 0 = empty (hash 0 is remapped)
  unsigned int* first;       // smallest candidate index that produced the key
  uint64_t capacity;         // power of two
};
void launch_kld_insert(hipStream_t st, const unsigned long long* d_hashes, uint64_t first, uint64_t count, KldTable t);
// flags[j] = 1 if candidate j is the first with its hash; inclusive scan -> d_k[j]; then the first j
// violating (j+1 <= min || j+1 <= target(k_base + k[j])) is atomically minimised into *d_first_fail.
void launch_kld_scan(hipStream_t st, const unsigned long long* d_hashes, uint64_t first, uint64_t count, KldTable t,
                     uint32_t* d_flags_scan, uint32_t* d_chunk_sum, uint32_t* d_chunk_offset, const uint32_t* d_k_base,
                     uint32_t* d_k_total, uint64_t min_particles, double epsilon, double z, unsigned long long* d_first_fail);
// K8: estimation.hpp:436-475 sufficient statistics; d_out[9].
void launch_estimate_sums(hipStream_t st, Particles p, uint64_t n, double pivot_x, double pivot_y, double* d_partials,
                          double* d_out, double* host_mirror = nullptr);
// cluster_based_estimate (algorithm/cluster_based_estimation.hpp): hash + per-cell aggregation + compaction of the occupied
// cells (for the host's cluster assignment), the write-back of the cells' cluster ids and the masked estimate sums.
struct CellTable {  // the open-addressing table of the occupied cells
  unsigned long long* keys;
  unsigned int* first;
  double* wsum;
  unsigned int* count;
  unsigned int* cluster;  // written by the host pass
  uint64_t capacity;      // power of two
  // What the masked sums read of a table: the keys and the cells' clusters, nothing else.
  static CellTable keys_and_clusters(const CellTable& t) { return CellTable{t.keys, nullptr, nullptr, nullptr, t.cluster, t.capacity}; }
};
struct CellList {  // compacted occupied cells, arbitrary order (the host sorts by `first`)
  unsigned long long* key;
  unsigned int* first;
  unsigned int* count;
  unsigned int* slot;
  double* wsum;
  double4* state;  // representative state = state of particle `first` as (c, s, x, y)
  unsigned int* size;
};
// (table_ready: only the compaction again, into a larger list)
void launch_cluster_cells(hipStream_t st, Particles p, uint64_t n, HashParams hp, unsigned long long* d_hashes, const CellTable& t,
                          const CellList& out, unsigned int list_capacity, bool table_ready = false);
// The same for a set of up to 4096 particles: one workgroup each (k_small_cluster_cells: straight into the caller's list - the mapped host
// list - and its size into size_mirror as well; false = the set does not fit; k_small_cluster_sums: the cells' keys and cluster ids back
// in, the sums of the particles of cluster `wanted` out).
bool launch_small_cluster_cells(hipStream_t st, Particles p, uint64_t n, HashParams hp, const CellList& out, unsigned int* size_mirror);
void launch_small_cluster_sums(hipStream_t st, Particles p, uint64_t n, HashParams hp, const unsigned long long* d_keys,
                               const unsigned int* d_cluster, uint32_t cells, unsigned int wanted, double pivot_x, double pivot_y, double* d_out,
                               double* host_mirror);
// The two kernels over a fleet (mcl_batch_update): one workgroup per record, every record one member's arguments of the lone kernel.  The
// host fills a table per launch (the sums' table holds only the members whose assignment has a winner).
struct BatchClusterCells {
  Particles p;  // the live set
  uint32_t n;   // 1 .. 4096
  HashParams hp;
  CellList out;               // the member's own mapped list, out.size its size word in device memory
  unsigned int* size_mirror;  // ... and the list's size word in the mapped memory
};
struct BatchClusterSums {
  Particles p;
  uint32_t n;
  HashParams hp;
  const unsigned long long* keys;  // the list's keys and the host's cluster ids, `cells` of each
  const unsigned int* cluster;
  uint32_t cells;
  unsigned int wanted;
  double pivot_x, pivot_y;
  double* d_out;   // the member's d_scalars + kSlotEstimate
  double* mirror;  // ... and hd_scalars + kSlotEstimate
};
void launch_batch_small_cluster_cells(hipStream_t st, const BatchClusterCells* d_items, uint32_t members);
void launch_batch_small_cluster_sums(hipStream_t st, const BatchClusterSums* d_items, uint32_t members);
// t.cluster[cells.slot[k]] = d_cluster[k], k < m
void launch_cell_set_cluster(hipStream_t st, const CellList& cells, const unsigned int* d_cluster, uint32_t m, const CellTable& t);
void launch_estimate_sums_cluster(hipStream_t st, Particles p, uint64_t n, const unsigned long long* d_hashes, const CellTable& t,
                                  unsigned int wanted, double pivot_x, double pivot_y, double* d_partials, double* d_out,
                                  double* host_mirror = nullptr);
// estimate_clusters (:337-399): t.cluster holds, per cell, the rank in [0, ranks) of its cluster among the selected ones (anything else:
// not selected); d_out[ranks][9]: the nine sums of estimation.hpp:436-475 per rank.  d_partials: ranks * 9 * num_chunks(n) doubles.
// ranks <= kMaxClusterRanks (the kernel keeps ranks * 288 bytes of LDS; more: nothing is launched).  Fixed-order reductions only.
constexpr uint32_t kMaxClusterRanks = 64;  // = MCL_MAX_CLUSTER_ESTIMATES
void launch_estimate_sums_clusters(hipStream_t st, Particles p, uint64_t n, const unsigned long long* d_hashes, const CellTable& t,
                                   uint32_t ranks, double pivot_x, double pivot_y, double* d_partials, double* d_out);
// ParticleClusterizer::operator() (:269-304): d_labels[i] = t.cluster of particle i's cell (d_hashes as launch_cluster_cells left them)
void launch_cluster_labels(hipStream_t st, uint64_t n, const unsigned long long* d_hashes, const CellTable& t, unsigned int* d_labels);
// init: multivariate_normal_distribution.hpp:96-126 with T = V sqrt(L)
void launch_init_normal(hipStream_t st, Particles p, uint64_t n, const double mean[3], const double T[9], uint64_t seed,
                        uint64_t index_offset);
// initialize_from_map: multivariate_uniform_distribution.hpp:126-161 over the free cells, weight 1
void launch_init_from_map(hipStream_t st, Particles p, uint64_t n, uint64_t seed, uint64_t index_offset, GridView g, FreeCells fc);
void launch_fill(hipStream_t st, double* p, uint64_t n, double v);
// d_out[k] = sum over r < rows (in order) of d_gathered[r * columns + k], columns <= 64 (gathered per-shard scalars)
void launch_sum_rows(hipStream_t st, const double* d_gathered, uint32_t rows, uint32_t columns, double* d_out, double* host_mirror);
// Likelihood field built on the device: exact Euclidean distance transform + the reference's Gaussian map, unknown-space
// overlay and edge mask (likelihood_field_model_base.hpp:130-185).  Scratch: W * H uint16 and int16.  Returns false (nothing
// launched) when max_obstacle_distance spans more than kFieldBuildMaxReach cells: the caller then builds on the host.
constexpr double kFieldBuildMaxReach = 1024.0;
struct FieldBuildParams {
  double max_obstacle_distance, max_laser_distance, z_hit, z_random, sigma_hit;
  int model_unknown_space, only_obstacle_boundaries;
};
bool launch_build_field(hipStream_t st, const int8_t* d_cells, uint32_t W, uint32_t H, double resolution, int8_t free_value,
                        int8_t unknown_value, int8_t occupied_value, const FieldBuildParams& fp, uint16_t* d_column_distance,
                        int16_t* d_column_offset, float* d_field);
// cube[i] = double(field[i])^3 (or log(double(field[i])) for the prob model) for i < cells, cube[cells] = same for `unknown`
void launch_cube_table(hipStream_t st, const float* field, uint64_t cells, float unknown_value, double* cube, int prob);
// keys: the sorted bit patterns of the distinct field values (count entries, unknown_value among them)
void launch_palette_table(hipStream_t st, const float* field, uint32_t W, uint32_t H, float unknown_value, const uint32_t* keys,
                          uint32_t count, int prob, uint16_t* idx, double* val, uint32_t pal_base);
// Far tiles of a palette table (FieldView::far_bits).  votes[k] (count entries, zeroed here) = number of tiles uniformly equal
// to entry k; the caller picks the entry and has launch_far_tile_bits write the bitmap (far_bytes bytes).
void launch_far_tile_votes(hipStream_t st, const uint16_t* idx, uint32_t tiles, uint32_t pal_base, uint32_t count, uint32_t* votes);
void launch_far_tile_bits_linear(hipStream_t st, const uint16_t* idx, uint32_t tiles, uint32_t entry, uint32_t bytes, uint8_t* bits);
void launch_far_tile_bits(hipStream_t st, const uint16_t* idx, uint32_t tiles_x, uint32_t tiles_y, uint32_t entry, uint32_t row_bytes,
                          uint32_t far_bytes, uint8_t* bits);
// AoS (c,s,x,y) host layout <-> SoA device layout

}  // namespace mcl
