// batch_host.cpp — see batch_host.h.
#include "batch_host.h"

#include <algorithm>

namespace mcl {

bool batch_member_fused(const BatchMemberFacts& m) {
  const bool likelihood_field = m.sensor_kind == MCL_SENSOR_LIKELIHOOD_FIELD || m.sensor_kind == MCL_SENSOR_LIKELIHOOD_FIELD_PROB;
  return likelihood_field && !m.sharded && m.small_fused && m.n >= 1 && m.n <= kBatchMaxParticles && m.max_particles >= 1 &&
         m.max_particles <= kBatchMaxParticles && m.palette_beams && !m.profiling && !m.beam_skip;
}

bool batch_beam_member_fused(const BatchBeamFacts& m) {
  return m.sensor_kind == MCL_SENSOR_BEAM && !m.sharded && m.small_fused && m.beam_fused && m.n >= 1 && m.n <= kBatchMaxParticles &&
         m.max_particles >= 1 && m.max_particles <= kBatchMaxParticles && m.n < m.beam_sort_min_particles && !m.profiling;
}

bool batch_ndt_member_fused(const BatchNdtFacts& m) {
  return m.sensor_kind == MCL_SENSOR_NDT && m.small_cycle && !m.sharded && m.small_fused && m.n >= 1 && m.n <= kBatchMaxParticles &&
         m.max_particles >= 1 && m.max_particles <= kBatchMaxParticles && m.have_map && !m.profiling;
}

bool batch_landmark_member_fused(const BatchLandmarkFacts& m) {
  return (m.sensor_kind == MCL_SENSOR_LANDMARK || m.sensor_kind == MCL_SENSOR_BEARING) && m.small_cycle && !m.sharded && m.small_fused &&
         m.n >= 1 && m.n <= kBatchMaxParticles && m.max_particles >= 1 && m.max_particles <= kBatchMaxParticles && !m.profiling;
}

bool batch_cluster_member(const BatchClusterFacts& m) {
  return m.status == MCL_OK && m.estimate_kind == 1 && m.cluster_fused && m.n >= 1 && m.n <= kBatchMaxParticles &&
         cluster_params_ok(m.linear_hash_resolution, m.angular_hash_resolution, m.weight_cap_percentile);
}

uint32_t batch_cluster_select(const BatchClusterFacts* m, uint32_t members, uint32_t* picked) {
  uint32_t count = 0;
  for (uint32_t i = 0; i < members; ++i)
    if (batch_cluster_member(m[i])) picked[count++] = i;
  return count;
}

uint32_t batch_cluster_launches(uint32_t cells_members, uint32_t sums_members) {
  if (cells_members == 0) return 0;
  return sums_members ? 2 : 1;
}

BatchGrid batch_layout(const uint64_t* n, const uint32_t* lds, uint32_t members, uint32_t* first_propagate, uint32_t* first_reweight) {
  BatchGrid g{members, 0, 0, 0};
  for (uint32_t m = 0; m < members; ++m) {
    first_propagate[m] = g.propagate_blocks;
    first_reweight[m] = g.reweight_blocks;
    g.propagate_blocks += batch_propagate_blocks(n[m]);
    g.reweight_blocks += batch_reweight_blocks(n[m]);
    g.reweight_lds = std::max(g.reweight_lds, lds[m]);
  }
  return g;
}

BatchBeamGrid batch_beam_layout(const uint64_t* n, const uint32_t* B, uint32_t members, uint32_t* first_beam) {
  BatchBeamGrid g{0, 0};
  for (uint32_t m = 0; m < members; ++m) {
    first_beam[m] = g.blocks;
    const uint32_t blocks = batch_beam_blocks(n[m], B[m]);
    g.blocks += blocks;
    if (blocks) g.lds = std::max(g.lds, B[m] * kBatchBeamPointBytes);
  }
  return g;
}

uint32_t batch_ndt_layout(const uint64_t* n, const uint32_t* K, uint32_t members, uint32_t* first_ndt) {
  uint32_t blocks = 0;
  for (uint32_t m = 0; m < members; ++m) {
    first_ndt[m] = blocks;
    blocks += batch_ndt_blocks(n[m], K[m]);
  }
  return blocks;
}

uint32_t batch_landmark_layout(const uint64_t* n, const uint32_t* k, uint32_t members, uint32_t* first_landmark) {
  uint32_t blocks = 0;
  for (uint32_t m = 0; m < members; ++m) {
    first_landmark[m] = blocks;
    blocks += batch_landmark_blocks(n[m], k[m]);
  }
  return blocks;
}

const char* batch_check_configs(const mcl_config* cfgs, uint32_t count) {
  if (!cfgs) return "mcl_batch_create: null configs";
  if (count < 1 || count > kBatchMaxMembers) return "mcl_batch_create: count must be 1 .. 1024";
  for (uint32_t i = 1; i < count; ++i) {
    if (cfgs[i].device_id != cfgs[0].device_id) return "mcl_batch_create: every member must be on the same device";
    if (cfgs[i].hip_stream != cfgs[0].hip_stream) return "mcl_batch_create: hip_stream must be NULL for every member or the same stream for all";
  }
  return nullptr;
}

const char* batch_check_offsets(const uint64_t* offsets, uint32_t members) {
  if (!offsets) return "mcl_batch_update: null point_offsets";
  for (uint32_t i = 0; i < members; ++i)
    if (offsets[i + 1] < offsets[i]) return "mcl_batch_update: point_offsets decrease";
  return nullptr;
}

}  // namespace mcl
