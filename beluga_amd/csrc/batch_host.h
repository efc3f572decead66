// batch_host.h — the arithmetic of a batch of small filters (mcl_batch_*) that touches no device memory: which members of a cycle share
// the cycle's launches (likelihood-field and beam-model members, a reweight launch per family), where each member's blocks lie in the gridded launches, how a block finds its member, how much workgroup memory
// the shared reweight needs, which members share the cluster-based estimate's two launches, and the validation of mcl_batch_create's configs and mcl_batch_update's scan offsets.  context.hip calls
// them between its launches; batch_member_of is also what the batched kernels run (kernels.hip).  Plain C++17, no HIP.
#pragma once

#include <cstddef>
#include <cstdint>

#include "beluga_mcl.h"
#include "se2.h"  // MCL_HD

namespace mcl {

constexpr uint32_t kBatchMaxMembers = 1024;   // mcl_batch_create's count
constexpr uint64_t kBatchMaxParticles = 4096;  // of a fused member: one workgroup of k_small_tail holds the set (kSmallMax)
constexpr uint32_t kBatchPropagateBlock = 256;  // particles of a block of k_propagate_small (kBlock)
constexpr uint32_t kBatchReweightBlock = 4;     // ... of k_reweight_lf_beams with a wave per particle (kBeamsBlock / kWave)
constexpr uint32_t kBatchBeamThreads = 256;     // threads of a block of k_reweight_beam (kBlock)
constexpr uint32_t kBatchBeamBlock = 4;         // ... and its particles, a wave each (kBlock / kWave)
constexpr uint32_t kBatchBeamPointBytes = 16;   // a scan point staged in its workgroup memory (double2)
constexpr uint32_t kBatchBeamMaxPoints = 4096;  // 64 KB of it: the lone kernel's own limit (reweight_preconditions)
constexpr uint32_t kBatchNdtThreads = 256;      // threads of a block of k_reweight_ndt_wave (kBlock)
constexpr uint32_t kBatchNdtBlock = 4;          // ... and its particles, a wave each (kBlock / kWave)
constexpr uint32_t kBatchLandmarkThreads = 256;  // threads of a block of k_reweight_landmarks_wave / k_reweight_bearings_wave (kBlock)
constexpr uint32_t kBatchLandmarkBlock = 4;      // ... and its particles, a wave each (kBlock / kWave)
constexpr uint32_t kBatchLandmarkMaxDetections = 64;  // MCL_LANDMARK_MAX_DETECTIONS: a wave's lanes

// ---- which members share the launches ------------------------------------------------------------------------------------------------
// What the predicate reads of a member in the cycle that is being prepared.
struct BatchMemberFacts {
  int sensor_kind;         // MCL_SENSOR_*
  bool sharded;            // the context is one rank of a sharded filter
  bool small_fused;        // option small_fused
  uint64_t n;              // particles of the live set
  uint64_t max_particles;  // min(max_particles, capacity): the candidates of a resampling
  bool palette_beams;      // the cycle's reweight is k_reweight_lf_beams over the palette table, no ordering pass (lf_takes_beams)
  bool profiling;          // stage profiling on: the member's own events bracket its own launches
  bool beam_skip;          // beam skipping enabled (mcl_set_beam_skip): a count and a synchronisation stand between its propagation and its reweight
};
// The member's own mcl_update would run exactly k_propagate_small, k_reweight_lf_beams with a wave per particle, k_small_tail.
bool batch_member_fused(const BatchMemberFacts& m);

// The same for a beam-model member (batch_member_fused answers 0 for it): what k_batch_reweight_beam's members must satisfy.
struct BatchBeamFacts {
  int sensor_kind;                   // MCL_SENSOR_*
  bool sharded;                      // the context is one rank of a sharded filter
  bool small_fused;                  // option small_fused
  bool beam_fused;                   // option batch_beam_fused
  uint64_t n;                        // particles of the live set
  uint64_t max_particles;            // min(max_particles, capacity)
  uint64_t beam_sort_min_particles;  // option beam_sort_min_particles: from this size on the member wants the ordering and the ordered kernel
  bool profiling;                    // stage profiling on
};
// The member's own mcl_update would run exactly k_propagate_small, k_reweight_beam (a wave per particle), k_small_tail.
bool batch_beam_member_fused(const BatchBeamFacts& m);

// The same for an NDT member (mcl_set_ndt_small_cycle): what k_batch_reweight_ndt's members must satisfy.
struct BatchNdtFacts {
  int sensor_kind;         // MCL_SENSOR_*
  bool small_cycle;        // the context's switch (mcl_set_ndt_small_cycle)
  bool sharded;            // the context is one rank of a sharded filter
  bool small_fused;        // option small_fused
  uint64_t n;              // particles of the live set
  uint64_t max_particles;  // min(max_particles, capacity)
  bool have_map;           // an NDT map is installed, in the dense layout (k_batch_reweight_ndt reads the index grid; a member on a
                           // hashed map, mcl_set_ndt_map_layout, runs its own cycle)
  bool profiling;          // stage profiling on
};
// The member's own mcl_update would run exactly k_propagate_small, k_reweight_ndt_wave, k_small_tail.
bool batch_ndt_member_fused(const BatchNdtFacts& m);

// The same for a landmark or bearing member (mcl_set_landmark_small_cycle): what k_batch_reweight_landmarks' members must satisfy.
struct BatchLandmarkFacts {
  int sensor_kind;         // MCL_SENSOR_*
  bool small_cycle;        // the context's switch (mcl_set_landmark_small_cycle)
  bool sharded;            // the context is one rank of a sharded filter
  bool small_fused;        // option small_fused
  uint64_t n;              // particles of the live set
  uint64_t max_particles;  // min(max_particles, capacity)
  bool profiling;          // stage profiling on
};
// The member's own mcl_update_landmarks / mcl_update_bearings would run exactly k_propagate_small, the wave kernel of its kind, k_small_tail.
bool batch_landmark_member_fused(const BatchLandmarkFacts& m);

// ---- which fused members share the cluster-based estimate's two launches ------------------------------------------------------------------
// What cluster_front checks of cluster parameters before anything is launched.
inline bool cluster_params_ok(double linear_hash_resolution, double angular_hash_resolution, double weight_cap_percentile) {
  return linear_hash_resolution > 0 && angular_hash_resolution > 0 && weight_cap_percentile >= 0 && weight_cap_percentile < 1.0;
}
// A fused member behind the state half of its cycle (the live set is the one the estimate is taken of).
struct BatchClusterFacts {
  int status;         // of the state half: MCL_OK, or the member has left the cycle
  int estimate_kind;  // 0: beluga::estimate, 1: cluster_based_estimate
  bool cluster_fused; // the member's option batch_cluster_fused
  uint64_t n;         // particles of the live set
  double linear_hash_resolution, angular_hash_resolution, weight_cap_percentile;  // the member's mcl_cluster_params
};
// The member's estimate goes through k_batch_small_cluster_cells / k_batch_small_cluster_sums: the small path of its own
// mcl_cluster_based_estimate would take it, and nothing about it is refused.
bool batch_cluster_member(const BatchClusterFacts& m);
// picked[0 .. returned count): the indices m < members with batch_cluster_member, in order.
uint32_t batch_cluster_select(const BatchClusterFacts* m, uint32_t members, uint32_t* picked);
// Shared cluster launches of a cycle: `cells_members` records went to the first kernel, `sums_members` of them - those whose assignment
// has a winner - to the second.  0, 1 or 2.
uint32_t batch_cluster_launches(uint32_t cells_members, uint32_t sums_members);

// ---- where the members' blocks are ---------------------------------------------------------------------------------------------------
MCL_HD uint32_t batch_propagate_blocks(uint64_t n) { return static_cast<uint32_t>((n + kBatchPropagateBlock - 1) / kBatchPropagateBlock); }
MCL_HD uint32_t batch_reweight_blocks(uint64_t n) { return static_cast<uint32_t>((n + kBatchReweightBlock - 1) / kBatchReweightBlock); }
// The launch geometry of a cycle's fused members.
struct BatchGrid {
  uint32_t members;           // = workgroups of k_batch_small_tail
  uint32_t propagate_blocks;  // grid of k_batch_propagate
  uint32_t reweight_blocks;   // grid of k_batch_reweight_lf_beams
  uint32_t reweight_lds;      // its dynamic workgroup memory: the largest palette layout of the members
};
// n[m], lds[m] (lf_palette_lds of the member's field) for m < members  ->  first_propagate[m], first_reweight[m]: the member's first
// block in each gridded launch (running sums; a member with n = 0 has no block and is never found), and the grids.
BatchGrid batch_layout(const uint64_t* n, const uint32_t* lds, uint32_t members, uint32_t* first_propagate, uint32_t* first_reweight);
// The beam members' launch (k_batch_reweight_beam).  A member with n = 0 or B = 0 has no block: the lone launch returns at once there.
MCL_HD uint32_t batch_beam_blocks(uint64_t n, uint32_t B) {
  return (n == 0 || B == 0) ? 0u : static_cast<uint32_t>((n + kBatchBeamBlock - 1) / kBatchBeamBlock);
}
struct BatchBeamGrid {
  uint32_t blocks;  // grid of k_batch_reweight_beam (0: nothing to launch)
  uint32_t lds;     // its dynamic workgroup memory: the largest staged scan of the members that have a block
};
// n[m], B[m] (scan points) for m < members  ->  first_beam[m]: the member's first block (a running sum; a member that is no beam member
// of the cycle comes with n = 0 or B = 0, has no block and is never found), and the grid.
BatchBeamGrid batch_beam_layout(const uint64_t* n, const uint32_t* B, uint32_t members, uint32_t* first_beam);
// The NDT members' launch (k_batch_reweight_ndt).  A member with n = 0 or K = 0 measurement cells has no block: its weights stay (x 1.0).
MCL_HD uint32_t batch_ndt_blocks(uint64_t n, uint32_t K) {
  return (n == 0 || K == 0) ? 0u : static_cast<uint32_t>((n + kBatchNdtBlock - 1) / kBatchNdtBlock);
}
// n[m], K[m] for m < members  ->  first_ndt[m]: the member's first block (a running sum; a member that is no NDT member of the cycle
// comes with n = 0 or K = 0, has no block and is never found).  Returns the grid (0: nothing to launch).
uint32_t batch_ndt_layout(const uint64_t* n, const uint32_t* K, uint32_t members, uint32_t* first_ndt);
// The landmark and bearing members' launch (k_batch_reweight_landmarks).  A member with n = 0 or k = 0 detections has no block: its
// weights stay (x 1.0).
MCL_HD uint32_t batch_landmark_blocks(uint64_t n, uint32_t k) {
  return (n == 0 || k == 0) ? 0u : static_cast<uint32_t>((n + kBatchLandmarkBlock - 1) / kBatchLandmarkBlock);
}
// n[m], k[m] for m < members  ->  first_landmark[m]: the member's first block (a running sum; a member that is no landmark member of the
// cycle comes with n = 0 or k = 0, has no block and is never found).  Returns the grid (0: nothing to launch).
uint32_t batch_landmark_layout(const uint64_t* n, const uint32_t* k, uint32_t members, uint32_t* first_landmark);
// The member whose blocks include `block`: the LAST m with first_of(m) <= block (members without a block share their successor's first
// block and are skipped).  Needs first_of(0) == 0 and block < the grid.  ceil(log2(members)) steps, each one read.
template <class FirstOf>
MCL_HD uint32_t batch_member_of(uint32_t members, uint32_t block, FirstOf first_of) {
  uint32_t lo = 0, hi = members;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (first_of(mid) <= block) lo = mid;
    else hi = mid;
  }
  return lo;
}

// ---- validation ----------------------------------------------------------------------------------------------------------------------
// mcl_batch_create: 1 .. kBatchMaxMembers configs on one device, their hip_stream all NULL or all the same stream.  nullptr: fine;
// otherwise what is wrong.
const char* batch_check_configs(const mcl_config* cfgs, uint32_t count);
// mcl_batch_update: offsets[0 .. members] do not decrease.  nullptr: fine.
const char* batch_check_offsets(const uint64_t* offsets, uint32_t members);

}  // namespace mcl
