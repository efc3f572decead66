// cycle_types.h — the plain types that the cycle's host code (cycle_host.cpp) shares with the kernel launchers (kernels.h): the motion
// sampler, the frame of the ordering keys, and the per-context switches.  Plain C++17, no HIP.
#pragma once

#include <algorithm>
#include <cstdint>

namespace mcl {

// The sensor models by what their update cycle runs: one family, one arm at every place that asks which model a context has
// ("Adding a sensor family").  Every MCL_SENSOR_* value (sensor_kind) has exactly one; a value outside them, which
// mcl_create refuses, answers kLikelihoodField, the arm such a kind has always fallen to.  (cycle_host.cpp)
enum class SensorFamily : uint8_t { kLikelihoodField, kBeam, kNdt, kLandmark };
SensorFamily sensor_family(int sensor_kind);

// Per-cycle constants of the motion model's sampling function (computed on the host from the control action).
//   differential   : three (mean, stddev) pairs: first rotation, translation, second rotation
//   omnidirectional: (mean, stddev) of the rotation and of the translation, stddev of the strafe, first rotation
//   stationary     : nothing (N(0, 0.02) on heading, x, y)
struct DiffDriveSampler {
  int kind;  // MCL_MOTION_*
  double m1, s1, mt, st, m2, s2;
  double first_c, first_s;
};

enum LfVariant : int {
  kLfWavePerParticle = 0,  // (rounds 1 - 4: a wave per particle over the f32 field; now the same kernel as 1)
  kLfLanePerParticle = 1,  // a lane per particle in index order over the f32 field (no ordering pass, no palette)
  kLfSortedLanes = 2,      // default: lanes = spatial neighbours (ordering pass), palette table, LDS patches
  kLfBeamLanes = 3         // wave per particle, lanes = beams, palette table: dispersed sets (chosen by the cycle, or forced)
};

// Per-context switches for A/B measurements and tests (mcl_set_option); no switch changes a result beyond the rounding of a
// particle's sum over the scan (libstdc++'s transform_reduce order with a lane per particle, a fixed tree with a wave per particle).
struct Tuning {
  int lf_variant = kLfSortedLanes;  // kernel family of the likelihood-field reweight
  int lf_fast = -1;                 // FMA variant with exact fallback: -1 / 1 = whenever its preconditions hold, 0 = never
  int lf_table = 0;                 // 0 = palette table when the field allows it, 1 = force the 8-byte cube table
  int lf_patch = 1;                 // index table through per-workgroup LDS patches: 1 = where the last launch found them useful,
                                    // 0 = never (per-lane gathers only), 2 = always
  int lf_loose_below = 224;         // LF patch kernel: a workgroup with fewer than this many 256ths of its beam groups fitting a patch
                                    // drops the patches (no producer, no barriers) and gathers every look-up
  int lf_dispersed = 2;             // a set the patch kernel reports as dispersed (lf_patch = 1): 2 = lanes over the beams of a pose, the poses
                                    // in the position-major order, far-tile bitmap (k_reweight_lf_far_beams; where its tables fit LDS, else
                                    // as 0), 0 = the ordered-lanes gather kernel (a lane per particle; rounds 2 - 5), 1 = wave per particle /
                                    // lane per beam without any order (k_reweight_lf_beams; 20 % slower than 0: profiles/r02_dispersed_study.txt)
  int lf_far_beams_per_wave = 0;    // particles a wave of k_reweight_lf_far_beams takes (0 = 32)
  int device_policy = 1;            // recovery estimator on the device when the cycle has no host-side decision
  int sort_min_particles = 16384;   // below this the ordering passes cost more than they save (likelihood-field models)
  int beam_sort_min_particles = 16384;  // beam model: the ordered kernel (LDS bit window, scan segments) from here on; below, a wave per
                                       // particle over the whole-grid maps (measured crossover: 12K particles at 180 beams, 28K at 1080)
  int lf_far_tiles = 1;             // the gather kernel skips look-ups into far tiles (FieldView::far_bits): 1 = for sets reported as
                                    // dispersed (lf_patch = 1), 0 = never, 2 = whenever it gathers
  int key_layout = -1;              // ordering key: -1 = position-major for dispersed likelihood-field sets, heading-major otherwise; 0 / 1 force
  int lf_small_particles = 65536;   // likelihood-field sets below this: a wave per particle with the lanes over the beams, no ordering
                                    // (measured: 25 % faster than the ordered kernels at 20K particles, 10 % at 50K, 12 % slower at 100K)
  int field_build = 0;              // mcl_set_map: 0 = host wavefront (bit-identical to the reference), 1 = exact EDT on the device
  int key_curve = 1;                // heading-major ordering key: 1 = Hilbert curve through (heading, y, x), 0 = Morton order
  int key_warp = 1;                 // heading-major key: 1 = bins of equal mass (the frame's +-4 sigma mapped through the normal distribution
                                    // function) when the frame comes from an estimate of the set, 0 = bins of equal width
  int key_bits_xy = 0;              // bits of the x / y bins of that key: 0 = chosen per cycle from the cloud's spread and the scan's
                                    // reach (4 .. 6), otherwise forced; round 2: 6 (8 heading bits)
  int cycle_spin = -1;              // fixed-size cycles: 1 = the host waits for the cycle's own completion word (written to mapped host memory
                                    // by the last kernel, Completion) instead of the stream's completion signal; 0 = hipStreamSynchronize;
                                    // -1 = the word for sets of 256K particles and more.  Measured (round 6, three alternating runs of 65
                                    // cycles each): 1749 against 1731 cycles/s in the driver's window at 1M particles, 1933 against 1901 once
                                    // the cloud has settled; round 3 at 2000 particles: 4 us per cycle SLOWER (the launches behind an
                                    // unsynchronised stream cost the host more) - hence the threshold.  The waiting thread spins.
  int beam_table = 1;               // beam model, ordered kernel: the terms that depend on the expected range alone from a table over the hit's
                                    // squared cell distance (built at mcl_set_map); 0 = evaluated per beam
  int lf_weight_sums = 1;           // fixed-size cycle: the normalisation factor is added up from the LF patch kernel's workgroup sums of the
                                    // new weights (no k_chunk_sum pass); 0 = from chunk sums of the weights
  int lf_split = 3;                 // LDS-patch planner: a group of 8 beams that fits no whole 64 x 64 patch (a range discontinuity inside
                                    // it) may go through two half patches (beams [0, k) and [k, 8): 32 x 64 or 64 x 32 cells each); 0 = never
  int lf_margin = 1;                // LDS-patch planner, rotation part of the bound: 1 = per axis (|sin d| |q'y| + (1 - cos d) |q'x|),
                                    // 0 = round 2's |R_p - R_ref| |q| on both axes
  int beam_free_ahead = 1;          // beam model, ordered kernel: a workgroup's lanes pass the cells its middle ray's clearance proves free in one
                                    // closed-form step (per beam and workgroup); 0 = block-distance skips only
  int lf_queue_grid = 0;            // workgroups of the queue form (lf_queue): 0 = three per CU, otherwise this many (tests: few workgroups, many
                                    // blocks each)
  int device_cus = 0;               // compute units of the context's device (filled in by mcl_create; 0 = assume 256)
  int shard_pad_permille = 1063;    // sharded fixed-size cycle: the ancestor exchange moves a FIXED number of entries per pair of ranks - this many
                                    // thousandths of a shard's share of another shard's draws, plus eight standard deviations - so that no count
                                    // is read by the host before the cycle's end; 0 = exact counts (one more host synchronisation per cycle)
  int lf_ends_first = 1;            // LDS-patch kernel: the blocks are taken from both ends of the order inwards (the fringe's slow blocks first)
  int beam_sectors = 1;             // beam model, ordered kernel, scanners that reach beyond half the LDS window: the scan in four sectors, each with
                                    // a window of its own that holds its rays (0 = one centred window; the rays that leave it go on in global memory)
  int lf_queue = 1;                 // LDS-patch kernel: 1 = as many workgroups as stay resident (lf_queue_grid) take the blocks from a queue where
                                    // there are more blocks than that (k_reweight_lf_patch<true>), 0 = one workgroup per block.  Bit-identical.
  int scan_fused = 1;               // fixed-size cycle that resamples: normalisation, totals, recovery estimator and CDF in ONE launch
                                    // (k_normalize_cdf): 1 = for sets of up to 64K particles (where the cycle is bound by the host's launches:
                                    // one less), 2 = wherever the kernel takes the set (up to 2M particles; measured at 1M: 18.6 us against
                                    // 10.3 + 7.2 - a hand-off inside a launch costs what the kernel boundary did), 0 = k_normalize + k_cdf.
                                    // Bit-identical.
  int draw_fold = 1;                // the draw kernel's last workgroup to finish adds up the estimate sums (no k_final_rows launch behind it):
                                    // 1 = for sets of up to 64K particles, 2 = up to 4M (measured at 1M: 56.2 us against 49.2 + 4.4 - every
                                    // workgroup ends on the ticket's round trip), 0 = k_final_rows.  Bit-identical.
  int noise_ahead = 1;              // fixed-size cycles, sets of more than 64K particles: the next cycle's propagation normals are drawn a cycle AHEAD:
                                    // 1 = by the draw kernel, whose vector units wait for the fabric (draw + 7.4 us, k_propagate - 12 at 1M); 2 = by a
                                    // kernel of its own behind the cycle's last one, while the host is away (k_noise_ahead, 17 us: cycles that end
                                    // on the completion word); both up to 2M particles (at 10M the draw is at the HBM's limit: measured a loss);
                                    // 0 = by k_propagate itself.  Bit-identical.
  int order_ahead = 1;              // with noise_ahead = 1: the NEXT cycle's spatial order is computed behind a cycle's last kernel, while the host is
                                    // away, from the predicted control action (the one of the cycle that ends); the next cycle uses it if the action it
                                    // gets is close to the prediction, else it orders by the real poses as before.  Only locality depends on the order.
  int draw_key_hist = 1;            // with order_ahead: the draw kernel counts the high digit of every predicted key it stores (an LDS counter per
                                    // digit and workgroup) and stores its 1024 counts side by side - a half column of the ordering's table, a draw
                                    // workgroup covering half a chunk - which k_row_scan adds in pairs on its way: no k_key_hist pass over the keys.
                                    // 0 = k_key_hist.  Measured at 1M: the draw 62.0 -> 62.9 us, k_key_hist's 7.4 us gone; alone (its row scan a
                                    // launch of its own: unmeasured) above every parent run only once the cloud has settled, + 0.9 %.  Digit-major
                                    // half columns - a 4-byte store per line - cost the draw 7.4 us, all that k_key_hist took.  Integer counts
                                    // only: bit-identical.
  int rows_merged = 1;              // with draw_key_hist: the nine workgroups of k_final_rows and the workgroups of k_row_scan - both read the draw's
                                    // output alone, neither the other's - in ONE launch, roles by blockIdx.x (k_final_rows_row_scan; nothing is handed
                                    // over inside it).  0 = two launches.  Measured at 1M: 9.8 us against k_final_rows' 5.2 + k_row_scan's 6.1 (from
                                    // whole columns).  Both options against the parent, three alternating runs of 65 cycles: 1924 against 1889 and
                                    // 1941 against 1911 cycles/s in the two settled windows (every run above every parent run), 1774 against 1744
                                    // in the driver's window (above the parent in every round, but inside the parent's own spread of 30: no gain
                                    // shown there).  Bit-identical.
  int norm_store = 0;               // fixed-size cycle that resamples at once: 0 = k_normalize leaves the chunk sums of the normalised weights
                                    // but does not store them - the CDF kernel divides again (same division, same bits), nothing else reads them;
                                    // 1 = stored
  int batch_cluster_fused = 1;      // a member of a batch (mcl_batch_update) whose cycle was fused and which returns the cluster-based estimate: 1 = that
                                    // estimate through the batch's two shared launches, 0 = through its own mcl_cluster_based_estimate
  int batch_beam_fused = 0;         // a beam-model member of a batch (mcl_batch_update) whose cycle is the small one with the wave-per-particle
                                    // kernel: 1 = its three kernels ride on the fleet's shared launches, the reweight on one launch for all such
                                    // members (k_batch_reweight_beam); 0 = it runs its own cycle inside the call.  Bit-identical.  Off until the
                                    // path has been measured ("Batched small filters").
  int small_fused = 1;              // sets of up to 4096 particles (plain estimate, one context): everything behind the reweight - normalise,
                                    // policies, fixed-size or KLD resampling, estimate sums - in one launch of one workgroup and one host
                                    // synchronisation (k_small_tail); 0 = the kernels of the large path
  int lf_pose_ahead = 1;            // likelihood-field models: world_to_field * pose of every particle is stored by the propagation that writes the
                                    // pose (k_field_pose for a set nothing has propagated) and the LF kernels load it; 0 = every LF kernel forms
                                    // the product itself, per particle and launch.  The same expression on the same values: bit-identical.
                                    // Measured: profiles/field_pose_ab.txt.
  int lf_unit_weights = 1;          // LF patch kernel on a set whose weights are all 1.0 (fresh from a resampling or an initialisation):
                                    // the old weight is not loaded (1.0 x = x: bit-identical); 0 = always loaded
  int search_chunk = 1 << 20;       // mcl_global_search*: candidates a chunk holds (64 .. 2^22) - what bounds the call's device memory; the result
                                    // does not depend on it
  int cast_chunk = 1 << 22;         // mcl_cast_rays: rays a chunk of the host form holds (64 .. 2^28) - what bounds the call's device memory; the
                                    // result does not depend on it
  int range_table_launch = 1 << 30; // mcl_build_range_table: entries one launch of the build covers (256 .. 2^30, in whole workgroups of 256); the
                                    // table does not depend on it
  int64_t range_table_max_bytes = 4ll << 30;  // mcl_build_range_table: a table larger than this is refused (MCL_ERR_OUT_OF_MEMORY) before
                                              // anything is allocated; 0 .. 2^62.  The one option that is no int: set_tuning stores it itself
};

// Spatial ordering of the particles (kLfSortedLanes, ordered beam kernel): the 64 lanes of a wave should hold neighbouring
// poses, so that their look-ups for a given beam fall into the same few table lines.  Order = full sort by a 20-bit key:
// bins of x, y (6 bits each) and heading (8 bits) over +-4 sigma around the cloud's centre, the two extra heading bits on
// top, the rest Morton-interleaved.  The frame of the bins comes from the previous cycle's estimate moved by the control
// action (host, no pass over the particles), or from a bounding-box pass when the host has no estimate of the set.
struct KeyFrame {
  double cx, cy;          // centre of the x / y bins
  double c0, s0;          // heading of the centre of the heading bins
  float inv_x, inv_y;     // 1 / span of the x / y bins (span = 8 sigma)
  float inv_t, t_off;     // heading bins: u = (delta - t_off) * inv_t + 0.5
  uint32_t layout;        // 0: heading-major key (dense sets: a workgroup's poses fit an LDS patch), 1: position-major key
                          // (dispersed sets: neighbours in the order share a region of the map, whatever their heading);
                          // | 2: the heading-major key follows the Z (Morton) curve instead of the Hilbert curve (option key_curve)
                          // | 4: heading-major key over bins of equal mass of a normal set instead of equal width (option key_warp)
  uint32_t bits_xy;       // heading-major key: bits of the x and of the y bins (4 .. 6; 0 = 6); the heading takes the other 20 - 2 bits_xy
};

// Likelihood-field sets below the threshold of the ordered kernels (the larger of the two options: the ordering itself and
// the LF kernels' own crossover).
inline bool lf_set_is_small(uint64_t n, const Tuning& t) {
  return n < static_cast<uint64_t>(std::max(t.sort_min_particles, t.lf_small_particles));
}

}  // namespace mcl
