// ndt_kernels.hip — the 2D NDT sensor model's reweight on gfx950: beluga::NDTSensorModel<SparseValueGrid2<...NDTCell2d...>>
// (sensor/ndt_sensor_model.hpp:216-239; sensor/data/ndt_cell.hpp:49-68).
//
// A lane per particle, f64 throughout.  The measurement cells of the scan (a few hundred at most: one per 5 points) are the same for
// every lane and are read at wave-uniform addresses (scalar loads).  Per (particle, measurement cell): the cell moved into the world
// by the pose, its centre key, then for each offset of the neighbour kernel one int32 look-up in the index grid (kernels.h
// NdtMapView) and, where a map cell is present, one record of 48 bytes and one f64 exponential.  The grid and the records are a
// few hundred KB for a building-sized map at 1 m: they stay in L2.
//
// A map in the hashed layout (NdtHashView, ndt_hash.h) runs the same source: the arithmetic below is a template over the view, and only
// the neighbour look-up differs - a bounded probe of the table instead of one load from the grid.  The offsets are visited in the same
// order and the present cells added in it, so the two layouts give the same bits on every map that both can hold.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "batch_host.h"
#include "device_common.hpp"

namespace mcl {
namespace {

// The one place where the layouts differ, written inside the arithmetic (if constexpr): the dense layout's statements are the ones the
// kernels had before the hashed layout existed, in their places, so that its three kernels keep their registers and occupancy (with
// the look-up in a helper of its own the lane kernel came out with other figures; DESIGN.md "Hashed map layout").
template <class View>
constexpr bool kNdtDense = std::is_same<View, NdtMapView>::value;

// likelihood_at(state * measurement) (ndt_sensor_model.hpp:229-239) of measurement cell `c` for the pose (c, s, x, y).
template <class View>
__device__ __forceinline__ double ndt_cell_likelihood(const View& m, const double* __restrict__ c, const Pose2& p) {
  const double mx = c[0], my = c[1], sa = c[2], sb = c[3], sd = c[4];
  const double rc = p.r.c, rs = p.r.s;
  // SE2 * NDTCell (ndt_cell.hpp:61-66): mean = so2 * mean + t (Sophus: real * x - imag * y, imag * x + real * y),
  // covariance = R S R^T, evaluated as (R S) R^T with R = [[c, -s], [s, c]]
  const double ux = (rc * mx - rs * my) + p.x;
  const double uy = (rs * mx + rc * my) + p.y;
  const double t00 = rc * sa - rs * sb, t01 = rc * sb - rs * sd;
  const double t10 = rs * sa + rc * sb, t11 = rs * sb + rc * sd;
  const double c00 = t00 * rc - t01 * rs, c01 = t00 * rs + t01 * rc;
  const double c10 = t10 * rc - t11 * rs, c11 = t10 * rs + t11 * rc;
  // cell_near (regular_grid.hpp:75-78): floor(p * (1 / resolution)), relative to the centre box; outside it no offset reaches a key
  const double fx = floor(ux * m.inv_resolution) - m.key_x0;
  const double fy = floor(uy * m.inv_resolution) - m.key_y0;
  double likelihood = 0.0;
  if (fx >= 0.0 && fx < m.box_w && fy >= 0.0 && fy < m.box_h) {
    // the centre: its index in the grid, or (hashed) the key itself = box position + the box's first key, |.| < 2^33
    const auto centre = [&] {
      if constexpr (kNdtDense<View>) return (static_cast<int32_t>(fy) + m.reach) * static_cast<int32_t>(m.gw) + static_cast<int32_t>(fx) + m.reach;
      else return longlong2{static_cast<long long>(fx) + m.centre_x0, static_cast<long long>(fy) + m.centre_y0};
    }();
    const double scale = -m.d2 / 2.0;
    for (uint32_t o = 0; o < m.num_offsets; ++o) {
      int32_t idx;
      if constexpr (kNdtDense<View>) idx = m.grid[centre + m.delta[o]];
      else idx = ndt_hash_find_neighbour(m.table, centre.x, centre.y, m.offsets[2 * o], m.offsets[2 * o + 1]);
      if (idx < 0) continue;
      const double2* rec = reinterpret_cast<const double2*>(m.cells + static_cast<size_t>(idx) * kNdtRecord);
      const double2 mean = rec[0], ab = rec[1], d_ = rec[2];
      // NDTCell::likelihood_at (ndt_cell.hpp:49-54): d1 exp((-d2 / 2) e^T (S' + S_map)^-1 e); Eigen's 2 x 2 inverse: adjugate / det
      const double e0 = ux - mean.x, e1 = uy - mean.y;
      const double s00 = c00 + ab.x, s01 = c01 + ab.y, s10 = c10 + ab.y, s11 = c11 + d_.x;
      const double inv_det = 1.0 / (s00 * s11 - s10 * s01);
      const double i00 = s11 * inv_det, i01 = -s01 * inv_det, i10 = -s10 * inv_det, i11 = s00 * inv_det;
      const double v0 = scale * e0, v1 = scale * e1;
      const double r0 = v0 * i00 + v1 * i10, r1 = v0 * i01 + v1 * i11;
      likelihood += m.d1 * exp(r0 * e0 + r1 * e1);
    }
  }
  return likelihood > m.minimum_likelihood ? likelihood : m.minimum_likelihood;  // std::max(likelihood, minimum_likelihood)
}

// 1 + the sum over the k measurement cells for the pose s, as a lane adds it: what a particle's weight is multiplied by.
template <class View>
__device__ __forceinline__ double ndt_lane_sum(const Pose2& s, const View& m, const double* __restrict__ meas, uint32_t k) {
  // std::transform_reduce(cells, 1.0, plus, ...) (ndt_sensor_model.hpp:219-224) as libstdc++ adds it: blocks of four, the rest one by one
  double acc = 1.0;
  uint32_t j = 0;
  for (; j + 4 <= k; j += 4) {
    const double l0 = ndt_cell_likelihood(m, meas + (j + 0) * kNdtRecord, s);
    const double l1 = ndt_cell_likelihood(m, meas + (j + 1) * kNdtRecord, s);
    const double l2 = ndt_cell_likelihood(m, meas + (j + 2) * kNdtRecord, s);
    const double l3 = ndt_cell_likelihood(m, meas + (j + 3) * kNdtRecord, s);
    acc += sum4(l0, l1, l2, l3);
  }
  for (; j < k; ++j) acc += ndt_cell_likelihood(m, meas + j * kNdtRecord, s);
  return acc;
}
template <class View>
__device__ __forceinline__ void reweight_ndt_lanes(const Particles& p, uint64_t n, const View& m, const double* __restrict__ meas, uint32_t k) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n) return;
  p.w[i] *= ndt_lane_sum(load_pose(p, i), m, meas, k);  // actions::reweight (actions/reweight.hpp:53-60)
}
__global__ __launch_bounds__(kBlock) void k_reweight_ndt(Particles p, uint64_t n, NdtMapView m, const double* __restrict__ meas, uint32_t k) {
  reweight_ndt_lanes(p, n, m, meas, k);
}
__global__ __launch_bounds__(kBlock) void k_reweight_ndt_hashed(Particles p, uint64_t n, NdtHashView m, const double* __restrict__ meas, uint32_t k) {
  reweight_ndt_lanes(p, n, m, meas, k);
}

// The same weights from a wave per particle (small sets: at 2000 particles a lane per particle is eight workgroups on 256 CUs, each lane
// walking K cells x up to 9 neighbours x one f64 exp in a row).  Lane l of pass q takes measurement cell 64 q + l, each lane loading
// its own record; the sum keeps k_reweight_ndt's association, so the weight is the same bits: a pass of 64 cells is sixteen aligned blocks
// of four, each block's (l0 + l1) + (l2 + l3) is formed across its four lanes by two quad permutations (a + b = b + a: lane 0 of the
// quad holds exactly sum4), and the quad sums are chained into the running sum in cell order through v_readlane; the last K mod 4 cells
// follow one by one.  Every lane carries the same running sum.  No workgroup memory, no atomics.
// (the body: block `block` of ONE set - blockIdx.x in k_reweight_ndt_wave, a member's local block in k_batch_reweight_ndt)
// (the sum itself, for the pose s: every lane of the wave returns it)
template <class View>
__device__ __forceinline__ double ndt_wave_sum(uint32_t lane, const Pose2& s, const View& m, const double* __restrict__ meas, uint32_t k) {
  double acc = 1.0;
  for (uint32_t base = 0; base < k; base += kWave) {
    const uint32_t j = base + lane;
    double l = 0.0;
    if (j < k) l = ndt_cell_likelihood(m, meas + static_cast<size_t>(j) * kNdtRecord, s);
    double quad = l + dpp_f64<0xB1>(l);  // quad_perm [1,0,3,2]: lanes 0 and 2 of a quad hold l0 + l1 and l2 + l3
    quad = quad + dpp_f64<0x4E>(quad);   // quad_perm [2,3,0,1]: lane 0 holds (l0 + l1) + (l2 + l3)
    const uint32_t left = k - base;      // cells from this pass on
    const uint32_t full = left >= kWave ? kWave / 4 : left / 4;
#pragma unroll
    for (uint32_t b = 0; b < kWave / 4; ++b)
      if (b < full) acc += readlane_f64(quad, 4 * b);
    if (left < kWave)
      for (uint32_t r = 4 * full; r < left; ++r) acc += readlane_f64(l, static_cast<int>(r));
  }
  return acc;
}
template <class View>
__device__ __forceinline__ void reweight_ndt_wave_block(uint32_t block, const Particles& p, uint64_t n, const View& m,
                                                        const double* __restrict__ meas, uint32_t k) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t i = static_cast<uint64_t>(block) * (kBlock / kWave) + (threadIdx.x >> 6);
  if (i >= n) return;  // (the whole wave)
  const double acc = ndt_wave_sum(lane, load_pose(p, i), m, meas, k);
  if (lane == 0) p.w[i] *= acc;  // actions::reweight (actions/reweight.hpp:53-60)
}
__global__ __launch_bounds__(kBlock) void k_reweight_ndt_wave(Particles p, uint64_t n, NdtMapView m, const double* __restrict__ meas, uint32_t k) {
  reweight_ndt_wave_block(blockIdx.x, p, n, m, meas, k);
}
__global__ __launch_bounds__(kBlock) void k_reweight_ndt_wave_hashed(Particles p, uint64_t n, NdtHashView m, const double* __restrict__ meas, uint32_t k) {
  reweight_ndt_wave_block(blockIdx.x, p, n, m, meas, k);
}
// The sensor model as a function (mcl_likelihoods, mcl_likelihoods_ndt_cells): out[i] = 1 + the sum for the caller's pose i - the factor the
// reweight kernels above multiply a particle at that pose by, from their own sums (ndt_lane_sum, ndt_wave_sum: the same bits from
// either).  A plain array of poses (cos, sin, x, y) in, a plain array out; nothing of a filter is read or written.
__device__ __forceinline__ Pose2 pose_at(const double4* __restrict__ poses, uint64_t i) {
  const double4 v = poses[i];
  return Pose2{Rot2{v.x, v.y}, v.z, v.w};
}
template <class View>
__global__ __launch_bounds__(kBlock) void k_likelihoods_ndt(const double4* __restrict__ poses, uint64_t n, View m, const double* __restrict__ meas,
                                                            uint32_t k, double* __restrict__ out) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n) return;
  out[i] = ndt_lane_sum(pose_at(poses, i), m, meas, k);
}
template <class View>
__global__ __launch_bounds__(kBlock) void k_likelihoods_ndt_wave(const double4* __restrict__ poses, uint64_t n, View m,
                                                                 const double* __restrict__ meas, uint32_t k, double* __restrict__ out) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * (kBlock / kWave) + (threadIdx.x >> 6);
  if (i >= n) return;  // (the whole wave)
  const double acc = ndt_wave_sum(lane, pose_at(poses, i), m, meas, k);
  if (lane == 0) out[i] = acc;
}
template <class View>
void launch_likelihoods_ndt_view(hipStream_t st, const double4* poses, uint64_t n, const View& m, const double* meas, uint32_t k, double* out) {
  if (n == 0) return;
  if (n <= kLikelihoodsWaveMax) {
    hipLaunchKernelGGL(k_likelihoods_ndt_wave<View>, dim3(batch_ndt_blocks(n, 1)), dim3(kBlock), 0, st, poses, n, m, meas, k, out);
    return;
  }
  for (uint64_t at = 0; at < n; at += kLikelihoodsLaneChunk) {  // (a grid dimension holds 2^31 - 1 blocks)
    const uint64_t count = std::min<uint64_t>(kLikelihoodsLaneChunk, n - at);
    hipLaunchKernelGGL(k_likelihoods_ndt<View>, dim3(blocks_for(count)), dim3(kBlock), 0, st, poses + at, count, m, meas, k, out + at);
  }
}

// The same over a fleet's NDT members (mcl_batch_update; the pattern is k_batch_reweight_beam, beam_kernels.hip): a workgroup finds its
// member over the first_ndt_block prefix - a member without a block (n = 0, no measurement cell, another family's member) is never found -
// and runs the body with its LOCAL block number on the member's own map and staged cells.
static_assert(kBatchNdtThreads == kBlock && kBatchNdtBlock == kBlock / kWave, "batch_host.h restates the wave-per-particle NDT kernel's launch geometry");
__global__ __launch_bounds__(kBlock) void k_batch_reweight_ndt(const BatchItem* __restrict__ items, uint32_t count) {
  const BatchItem& it = items[batch_member_of(count, blockIdx.x, [items](uint32_t m) { return items[m].first_ndt_block; })];
  reweight_ndt_wave_block(blockIdx.x - it.first_ndt_block, it.p, it.n, it.ndt, it.scan_dst, it.ndt_cells);
}

}  // namespace

void launch_reweight_ndt(hipStream_t st, Particles p, uint64_t n, const NdtMapView& m, const double* meas, uint32_t k) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_reweight_ndt, dim3(blocks_for(n)), dim3(kBlock), 0, st, p, n, m, meas, k);
}
void launch_reweight_ndt_wave(hipStream_t st, Particles p, uint64_t n, const NdtMapView& m, const double* meas, uint32_t k) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_reweight_ndt_wave, dim3(batch_ndt_blocks(n, 1)), dim3(kBlock), 0, st, p, n, m, meas, k);
}
void launch_reweight_ndt_hashed(hipStream_t st, Particles p, uint64_t n, const NdtHashView& m, const double* meas, uint32_t k) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_reweight_ndt_hashed, dim3(blocks_for(n)), dim3(kBlock), 0, st, p, n, m, meas, k);
}
void launch_reweight_ndt_wave_hashed(hipStream_t st, Particles p, uint64_t n, const NdtHashView& m, const double* meas, uint32_t k) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_reweight_ndt_wave_hashed, dim3(batch_ndt_blocks(n, 1)), dim3(kBlock), 0, st, p, n, m, meas, k);
}
void launch_likelihoods_ndt(hipStream_t st, const double4* poses, uint64_t n, const NdtMapView& m, const double* meas, uint32_t k, double* out) {
  launch_likelihoods_ndt_view(st, poses, n, m, meas, k, out);
}
void launch_likelihoods_ndt_hashed(hipStream_t st, const double4* poses, uint64_t n, const NdtHashView& m, const double* meas, uint32_t k, double* out) {
  launch_likelihoods_ndt_view(st, poses, n, m, meas, k, out);
}
void launch_batch_reweight_ndt(hipStream_t st, const BatchItem* d_items, uint32_t members, uint32_t blocks) {
  if (blocks == 0) return;
  hipLaunchKernelGGL(k_batch_reweight_ndt, dim3(blocks), dim3(kBlock), 0, st, d_items, members);
}

}  // namespace mcl
