// cycle_host.h — the host decisions of the update cycle that touch no device memory: the motion model's per-cycle constants, where the
// set is (the frame of the ordering keys), which likelihood-field kernel a cycle takes, the resampling policies, and the arithmetic of
// the particle shards.  context.hip calls them between its launches.  Plain C++17, no HIP.
#pragma once

#include <cstdint>

#include "beluga_mcl.h"
#include "cycle_types.h"
#include "se2.h"
#include "set_facts.h"

namespace mcl {

// ---- motion --------------------------------------------------------------------------------------------------------------------------
// motion/differential_drive_model.hpp:129-154,167-173, omnidirectional_drive_model.hpp:102-131, stationary_model.hpp:53-61
DiffDriveSampler make_sampler(const Pose2& pose, const Pose2& prev, const mcl_diffdrive_params& a, int kind, double alpha5);
// Is the control action that came close enough to the one the order was predicted with (launch_order_ahead)?  What matters is that the
// particles end up in the same ARRANGEMENT: a common shift does not change it, different noise scales or a translation along another
// heading do.  Generous bounds: a miss costs look-ups that fit no LDS patch, a fallback costs the ordering passes on the critical path.
bool samplers_close(const DiffDriveSampler& now, const DiffDriveSampler& predicted);
// Symmetric 3x3 eigen-decomposition (cyclic Jacobi): T = V sqrt(L)  (multivariate_normal_distribution.hpp:109-126).  False: the matrix
// is not symmetric, not finite, or has a negative eigenvalue.
bool covariance_to_transform(const double cov[9], double T[9]);

// ---- where the set is ----------------------------------------------------------------------------------------------------------------
// The last estimate of the set, when the host has one: where the ordering keys of the next cycle are centred (KeyFrame), and how
// thinly the set is spread (LfPlanner::hopelessly_sparse).
class CloudEstimate {
 public:
  bool valid() const { return valid_; }
  const double* mean() const { return mean_; }    // x, y, theta
  const double* sigma() const { return sigma_; }  // standard deviations of x, y, theta
  void remember(const mcl_estimate& est);         // a cycle's estimate; not valid where its mean or spread is not finite
  void set(const double mean[3], const double sigma[3]);  // an entry point that wrote the set knows where it put it
  void forget() { valid_ = false; }               // ... or does not: a bounding-box pass until the next estimate

 private:
  bool valid_{false};
  double mean_[3]{0, 0, 0}, sigma_[3]{0, 0, 0};
};

// What predict_key_frame reads of the context beside the cloud.
struct KeyFrameInputs {
  bool patch_useful;    // LfPlanner::patch_useful(): a set reported as dispersed takes +- 2 sigma and bins of equal width
  double resolution;    // of the map (0: none)
  double scan_extent;   // max |x| + |y| of the staged scan points (NaN if the beam model's scan holds a NaN)
  int key_warp, key_bits_xy;  // Tuning
};
// The frame of the ordering keys for the set as it will be AFTER this propagation: the last estimate moved by the mean motion, spans
// widened by the motion noise.  Only the balance of the key's bins depends on it.  out->layout = layout (LfPlanner::key_layout) in
// every case; false: the host does not know where the set is.  motion: nullptr = the set as it stands.
// moves: how often the set's centre is moved by `motion` (2: the frame of the cycle AFTER the one that is running - launch_order_ahead -, whose
// set is the remembered one moved twice; its spread grows once: the resampling in between takes it back to where it was).
bool predict_key_frame(const CloudEstimate& cloud, const DiffDriveSampler* motion, int moves, uint32_t layout, const KeyFrameInputs& in,
                       KeyFrame* out);

// ---- is the pivot of the estimate sums still inside the set? -----------------------------------------------------------------------------
// sums: the twelve of mcl_estimate_from_sums.  With m = (S w dx, S w dy) / W the offset of the mean from the pivot and
// M = (S w dx^2 + S w dy^2) / W the second moment about the pivot (a sum of positive terms: well conditioned whatever the pivot), the
// biased variance is T = M - |m|^2.  A sum's rounding error is a count of roundings times u M; the estimate is held to the same count
// times u D^2, D the diagonal of the set's bounding box, so the sums serve while M <= D^2.  The host does not know D, but each axis'
// variance is at most a quarter of its extent squared (Popoviciu), so T <= D^2 / 4 and M = T + |m|^2 <= D^2 wherever |m|^2 <= 3 T:
// the multiple is kRepivotMultiple = 3, and written on the well-conditioned quantities the test is |m|^2 > 3/4 M.  True: take the
// sums once more about the mean just computed (then m is a rounding of zero and M = T).  False for sums that are not finite.
// A set with no spread at all (one particle, a set collapsed onto one state, one particle holding all the weight: T = 0) answers true
// for any m != 0: its covariance is exact only about the state itself.  Such a filter pays the second pass on every cycle whose carried
// pivot is not bit-equal to that state; a filter with any spread does not (the carried pivot lands within it).
constexpr double kRepivotMultiple = 3.0;
bool estimate_needs_repivot(const double sums[12]);

// ---- which likelihood-field kernel a cycle takes -------------------------------------------------------------------------------------
// What the planner reads of the context.
struct LfSite {
  int sensor_kind;    // MCL_SENSOR_*
  uint64_t n;         // particles of the live set
  bool palette;       // the field has a palette table (pal_count != 0)
  bool far_tiles;     // ... and a far-tile bitmap (far_tiles != 0)
  double resolution;  // of the map
  const Tuning& tuning;
};

// The LDS-patch kernel reports how many beam groups it planned and how many went through a patch (running totals, mirrored into host
// memory); a launch that found few sends the next ones to the kernels for dispersed sets, with a probe every 16th decision (option
// lf_patch = 1).  The planner owns what the host remembers of those reports and this cycle's decision.  A stale value is a silently
// different kernel (and different last ulps of a weight), not an error: every write is one of the events below.
//
//   seen      the mirrored totals (planned, through) at the last look
//   useful    the last launch that reported put a quarter of its groups or more through a patch
//   probe in  decisions until a set reported as dispersed tries the patch kernel again
//   mode      this cycle's decision: {patches, beams}, and whether it has been taken
//
//   event                               seen        useful              probe in             mode
//   cycle_begins                        .           .                   .                    undecided
//   decide(site, cloud, totals)         (a decided cycle: nothing; beam, NDT, landmark kinds and lf_variant != sorted lanes: mode alone)
//     lf_patch 0 / 2                    .           .                   .                    = patches never / always
//     lf_patch 1, totals moved          = totals    = 4 dt >= dp        16 if not useful     .
//     lf_patch 1, useful                .           .                   .                    = patches
//     lf_patch 1, not useful            .           .                   - 1; at 0: 16        = patches on the probe unless hopelessly_sparse,
//                                                                                              else beams where lf_dispersed = 1
//   mode_consumed                       .           .                   .                    undecided
//   set_installed(kKept, totals)        .           .                   .                    .
//   set_installed(kFresh, totals)       = totals    true                .                    .
//   set_installed(kDispersed, totals)   = totals    false               16                   .
//
// The totals are the low 32 bits of each running total, as the kernel packs them into one word: differences are taken modulo 2^32.
// cycle_begins: the top of the update cycle (whatever an earlier, failed cycle left behind); mode_consumed: the reweight, once it has
// asked everything that depends on the mode.  wants_ordering, key_layout and gathers_dispersed only read.
class LfPlanner {
 public:
  // patches = the LDS-patch kernel; beams = a dispersed set goes to k_reweight_lf_beams (wave per particle, no ordering).
  struct Mode { bool patches, beams; };
  // An entry point installed a set.  kKept: the statistics as they were; kFresh: earlier launches' reports are history, the next LF
  // launch finds out; kDispersed: history, and the set is what the patch kernel would report as dispersed - the first cycle already
  // takes the kernel for dispersed sets.
  enum class Installed { kKept, kFresh, kDispersed };

  bool patch_useful() const { return patch_useful_; }
  bool decided() const { return decided_; }

  void cycle_begins() { decided_ = false; }
  // The LF launch of this cycle: the patch kernel, the gather kernel, or - for a set the patch kernel has reported as dispersed (no
  // probe due) - the wave-per-particle kernel, which needs no ordering pass.  Decided once per cycle, before the propagation kernel
  // (which emits the ordering keys): a second call returns the first one's answer.
  Mode decide(const LfSite& site, const CloudEstimate& cloud, uint64_t planned, uint64_t through);
  void mode_consumed() { decided_ = false; }
  void set_installed(Installed how, uint64_t planned, uint64_t through);

  // Is the set spatially ordered before the reweight?  The one answer for k_propagate's keys, the order ahead and the LF kernel.
  bool wants_ordering(const LfSite& site) const;
  // KeyFrame::layout of the next ordering: position-major for likelihood-field sets reported as dispersed (their gather kernel walks
  // the order region by region, kernels.hip: k_reweight_lf_palette<true, true>), heading-major otherwise.
  uint32_t key_layout(const LfSite& site) const;
  // LfReweightArgs::dispersed of the decided mode: the far-tile bitmap where the launch gathers.
  bool gathers_dispersed(const Tuning& tuning) const;
  // A workgroup of the patch kernel needs its 448 poses within a patch (64 x 64 cells less the margins) and within a few hundredths
  // of a radian.  From the last estimate's spread, taken as uniform (12 sigma_x sigma_y of area, sqrt(12) sigma_theta of heading, at
  // most the circle): the number of poses in such a volume.  Below an eighth of a workgroup no probe is worth it.
  static bool hopelessly_sparse(const LfSite& site, const CloudEstimate& cloud);

 private:
  bool wants_patches(const LfSite& site, const CloudEstimate& cloud, uint64_t planned, uint64_t through);

  uint64_t seen_planned_{0}, seen_through_{0};
  bool patch_useful_{true};
  int probe_in_{0};
  bool decided_{false};
  Mode mode_{false, false};
};

// ---- the field-frame poses of the live set (option lf_pose_ahead) --------------------------------------------------------------------
// world_to_field * pose, what every likelihood-field kernel starts from, is kept per particle in a buffer of the context (FieldPoseOut,
// kernels.h; likelihood-field contexts alone have one) and SetFacts knows whether it describes the live set under the current map.
// Does a propagation store them beside the poses it writes?  With the option on, where there is a buffer and a map whose frame they are
// taken in.  It then reports field_poses_written(generation), otherwise poses_moved.
bool propagation_writes_field_poses(const Tuning& tuning, bool have_buffer, bool have_map);
// What a likelihood-field launch does: `load` - its kernel reads the buffer instead of forming the product; `rebuild_first` - and
// k_field_pose fills it before (the set's poses were written by something that stores none - a resampling, an exchange,
// mcl_set_particles, an initialisation - or the map has changed since).  The steady propagate -> reweight cycle never rebuilds.
struct FieldPosePlan { bool load, rebuild_first; };
FieldPosePlan field_pose_plan(const Tuning& tuning, bool have_buffer, const SetFacts& facts, uint64_t map_generation);

// ---- policies (amcl_core.hpp:170-186) ------------------------------------------------------------------------------------------------
// algorithm/exponential_filter.hpp:32-44
struct ExponentialFilter {
  double alpha{0.}, output{0.};
  void reset() { output = 0.; }
  double operator()(double input) {
    output += (output == 0.) ? input : alpha * (input - output);
    return output;
  }
};
// update_policy_ = on_motion (policies/on_motion.hpp:63-67,121-133): has the control pose moved by more than min_d or turned by more than min_a?
bool moved_enough(const Pose2& latest, const Pose2& pose, double min_d, double min_a);
// every_n (every_n.hpp:47-50, :181): the counter as this cycle leaves it; the policy fires where it is 0.
inline uint64_t next_every_n(uint64_t current, uint64_t interval) { return (current + 1) % interval; }

// Where a particle's sum over the scan starts in the likelihood-field kernels (FieldView::acc0): the model's own start - 1
// (likelihood_field_model.hpp:76) or 0 (the prob model's sum of logs, likelihood_field_prob_model.hpp:77) - plus the terms of the
// `no_cell` scan points taken out where the scan was staged (NaN or infinite: outside every grid for every pose), each the
// unknown-space term pz^3 or log(pz) of pz = double(unknown_value) (likelihood_field_model.hpp:75,84-88).  Exactly the model's start
// for a scan without such points.
inline double lf_acc0(bool prob, float unknown_value, uint64_t no_cell) {
  const double pz = static_cast<double>(unknown_value);
  if (no_cell == 0) return prob ? 0.0 : 1.0;
  return prob ? static_cast<double>(no_cell) * std::log(pz) : 1.0 + static_cast<double>(no_cell) * (pz * pz * pz);
}
// The resampling decision on the host from the totals of the normalised weights of n particles: :179 ThrunRecoveryProbabilityEstimator
// (thrun_recovery_probability_estimator.hpp:69-89), :181 every_n's verdict `fires` [&& on_effective_size_drop] (on_effective_size_drop.hpp:45-49,
// effective_sample_size.hpp:46-59).  The filters' reset (:184-186) is the caller's.
struct HostPolicy {
  double random_state_probability{0.0}, ess{-1.0};  // (ess -1: not evaluated)
  bool resample{false};
};
HostPolicy host_policy(ExponentialFilter& slow, ExponentialFilter& fast, bool selective_resampling, bool fires, double norm_sum,
                       double norm_sumsq, uint64_t n);

// ---- the small cycle of a likelihood-field or beam context ---------------------------------------------------------------------------
// Does everything behind the reweight run in one launch of one workgroup and one synchronisation (k_small_tail, option small_fused)?
// One workgroup holds the set and the candidates of a resampling: the size rule the other families' small cycles share.  (A cycle
// reaches the question with n >= 1; where k_small_tail refuses its record - no particle may be kept - the large path takes over.)
struct GridCycleFacts {
  bool small_fused;        // option small_fused
  uint64_t n;              // particles of the live set
  uint64_t max_particles;  // min(max_particles, capacity)
};
constexpr uint64_t kSmallCycleMaxParticles = 4096;
bool grid_cycle_is_small(const GridCycleFacts& f);

// ---- the small cycle of an NDT context (mcl_set_ndt_small_cycle) ----------------------------------------------------------------------
// Does this NDT cycle run k_propagate_small, k_reweight_ndt_wave, k_small_tail with one synchronisation?  The size rule is the
// likelihood-field small cycle's.
struct NdtCycleFacts {
  bool small_cycle;        // the context's switch
  bool small_fused;        // option small_fused
  bool profiling;          // stage profiling on
  uint64_t n;              // particles of the live set
  uint64_t max_particles;  // min(max_particles, capacity)
};
bool ndt_cycle_is_small(const NdtCycleFacts& f);
// The wave-per-particle kernel for a stage-level reweight (mcl_reweight, mcl_reweight_ndt_cells)?
inline bool ndt_reweight_takes_waves(bool small_cycle, uint64_t n) { return small_cycle && n <= kSmallCycleMaxParticles; }
// The tail ends an NDT cycle that resamples with a random state probability > 0 behind the policies, without drawing: the generator of
// the random states is N(estimate of the normalised set), which the host forms (amcl_core.hpp:182).  What it leaves in the mirror:
struct NdtHandBack {
  double slow, fast;  // the recovery filters' outputs as :179 leaves them - NOT reset (:184-186 comes behind :182, which may throw)
  double p, ess, weight_sum;
};
// The host's side of such a cycle, in the reference's order of events (:179-199).  every_n was stored when the tail was launched
// (:181 has run on the device) and the step number when the cycle began: neither moves here.
// taken: :179 - the filters take the tail's outputs.  A generator that is refused (MCL_ERR_BAD_COVARIANCE) ends the cycle here: estimator
// and policy advanced, no reset, no particle replaced, force_update as it was.
void ndt_hand_back_taken(const NdtHandBack& h, ExponentialFilter& slow, ExponentialFilter& fast);
// resamples: the generator stands - :184-186 the filters' reset (p > 0, as in every handed-back cycle), :199 force_update cleared.
void ndt_hand_back_resamples(const NdtHandBack& h, ExponentialFilter& slow, ExponentialFilter& fast, bool* force_update);

// ---- the small cycle of a landmark or bearing context (mcl_set_landmark_small_cycle) --------------------------------------------------
// Does this cycle run k_propagate_small, the wave-per-particle kernel of the context's kind, k_small_tail with one synchronisation?  The
// size rule is the likelihood-field small cycle's.  Nothing is handed back: the random states come from the map's box, inside the tail.
struct LandmarkCycleFacts {
  bool small_cycle;        // the context's switch
  bool small_fused;        // option small_fused
  bool profiling;          // stage profiling on
  uint64_t n;              // particles of the live set
  uint64_t max_particles;  // min(max_particles, capacity)
};
bool landmark_cycle_is_small(const LandmarkCycleFacts& f);
// The wave-per-particle kernels for a stage-level reweight (mcl_reweight_landmarks, mcl_reweight_bearings)?
inline bool landmark_reweight_takes_waves(bool small_cycle, uint64_t n) { return small_cycle && n <= kSmallCycleMaxParticles; }

// ---- particle shards -----------------------------------------------------------------------------------------------------------------
// Contiguous, balanced split of [0, n_total) over the ranks.
void shard_bounds(uint64_t n_total, uint32_t world, uint32_t rank, uint64_t* first, uint64_t* count);
// Entries per pair of ranks in the fixed-capacity exchange: what a shard's m output slots ask of one other shard - m / world on average,
// the shards' weight sums being those of equal random samples of one set - plus `permille` / 1000 - 1 of it, eight standard deviations
// of the binomial count and 64.  Every rank derives the same number from the same arguments.
uint64_t padded_capacity(uint64_t n_total, uint32_t world, uint32_t permille);
// Re-balancing the kept candidates [0, n_out) into contiguous shards of the new set, one candidate block [pos, pos + cnt) at a time (every
// rank holds its shard_bounds slice of the block): the bytes (32 per state) this rank sends to every rank q, send[world], and expects
// from it, recv[world].  What a rank receives from a block is one contiguous run of its new shard: returns where it starts, in
// particles from the new shard's first.
uint64_t rebalance_block(uint64_t pos, uint64_t cnt, uint64_t n_out, uint32_t world, uint32_t rank, uint64_t* send, uint64_t* recv);

}  // namespace mcl
