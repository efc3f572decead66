// ndt_build_kernels.hip — the 2D NDT map built on gfx950 from a point cloud or an occupancy grid: detail::to_cells with fit_points
// (sensor/ndt_sensor_model.hpp:66-110) as context.hip's ndt_fit_cells restates it on the host, for 10^5 .. 10^7 points.
//
//   keys    : a point's cell key is (p / resolution) truncated toward zero; one pass finds the keys' box (k_ndt_key_box), a second
//             writes every point's key relative to the box's corner as one 64-bit word, x in the high half (k_ndt_sort_keys): the
//             order of those words is the host's order of (x, y) pairs.
//   grouping: a least-significant-digit radix sort of (word, point index) by 8-bit digits, over the bits the box needs only.
//             Every pass is STABLE (k_ndt_radix_scatter ranks with ballots, waves and workgroups chained in order), so inside a
//             cell the points stay in input order.
//   fit     : the first point of every run of 5 or more equal words starts a cell (k_ndt_mark_cells, an exclusive scan,
//             k_ndt_cell_starts); a lane per cell adds the run up in input order, exactly as the host loop does - count, mean, then
//             the sample covariance about that mean, diagonal clamped at 1e-5 - and writes the record, the key and the cell's
//             entry in the index grid (k_ndt_fit_cells).  The translation unit is built with -ffp-contract=off like the rest: no
//             product is fused into a sum, the records equal the host's bit for bit.
//   grid    : the centres of the occupied cells of an occupancy grid, row-major, through the grid's origin (k_ndt_grid_flags, the
//             scan, k_ndt_grid_points).
// f64 throughout; no kernel needs scratch memory.
#include <hip/hip_runtime.h>

#include "device_common.hpp"

namespace mcl {
namespace {

constexpr int kRadixBits = 8;
constexpr int kRadix = 1 << kRadixBits;
constexpr int kSortWaves = kBlock / 64;
constexpr int kSortRounds = kChunk / kBlock;  // a wave's share of a chunk: 512 consecutive elements, 64 at a time
static_assert(kRadix == kBlock, "a thread per digit");
constexpr uint32_t kMinPointsPerCell = 5;

// (p / resolution).cast<int>(): false where the point is not finite or a component does not fit (the cast is undefined there)
__device__ __forceinline__ bool point_key(const double2 p, double resolution, int32_t& kx, int32_t& ky) {
  const double qx = p.x / resolution, qy = p.y / resolution;
  if (!(fabs(qx) < 2147483647.0 && fabs(qy) < 2147483647.0)) return false;
  kx = static_cast<int32_t>(qx);
  ky = static_cast<int32_t>(qy);
  return true;
}

__device__ __forceinline__ int32_t wave_min_i32(int32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ int32_t wave_max_i32(int32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}

// box = {min x, max x, min y, max y, bad}: the keys' box (initialised to INT_MAX / INT_MIN / 0 by the caller), bad != 0 if a point
// has no key.  Minima and maxima: the result does not depend on the order of the atomics.
__global__ __launch_bounds__(kBlock) void k_ndt_key_box(const double2* __restrict__ pts, uint32_t n, double resolution, int32_t* __restrict__ box) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  int32_t kx = 0, ky = 0;
  const bool live = i < n;
  const bool good = live && point_key(pts[live ? i : 0], resolution, kx, ky);
  const int32_t x0 = wave_min_i32(good ? kx : INT_MAX), x1 = wave_max_i32(good ? kx : INT_MIN);
  const int32_t y0 = wave_min_i32(good ? ky : INT_MAX), y1 = wave_max_i32(good ? ky : INT_MIN);
  const bool bad = __builtin_amdgcn_ballot_w64(live && !good) != 0;
  if ((threadIdx.x & 63) == 0) {
    if (x0 <= x1) {
      atomicMin(&box[0], x0);
      atomicMax(&box[1], x1);
      atomicMin(&box[2], y0);
      atomicMax(&box[3], y1);
    }
    if (bad) atomicOr(&box[4], 1);
  }
}

// words[i] = (key x - x0) << 32 | (key y - y0): every point has a key inside the box (k_ndt_key_box reported none without)
__global__ __launch_bounds__(kBlock) void k_ndt_sort_keys(const double2* __restrict__ pts, uint32_t n, double resolution, int32_t x0, int32_t y0,
                                                          unsigned long long* __restrict__ words) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  int32_t kx = x0, ky = y0;
  (void)point_key(pts[i], resolution, kx, ky);
  const unsigned long long rx = static_cast<unsigned long long>(static_cast<long long>(kx) - x0);
  const unsigned long long ry = static_cast<unsigned long long>(static_cast<long long>(ky) - y0);
  words[i] = (rx << 32) | ry;
}

// ---- exclusive scan of uint32, in place: chunk sums, one workgroup over the chunk sums, the chunks ------------------------------
__global__ __launch_bounds__(kBlock) void k_ndt_scan_sums(const uint32_t* __restrict__ v, uint32_t n, uint32_t* __restrict__ chunk_sum) {
  __shared__ uint32_t s_wave[kBlock / 64];
  const uint32_t base = blockIdx.x * kChunk + threadIdx.x * (kChunk / kBlock);
  uint32_t local = 0;
#pragma unroll
  for (int k = 0; k < kChunk / kBlock; ++k) local += (base + k < n) ? v[base + k] : 0u;
  for (int o = 32; o > 0; o >>= 1) local += __shfl_down(local, o);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = local;
  __syncthreads();
  if (threadIdx.x == 0) chunk_sum[blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}
// An inclusive scan over the workgroup's kBlock values, one per thread; -> this thread's inclusive value.  s_wave: kBlock / 64 words.
__device__ __forceinline__ uint32_t block_inclusive_u32(uint32_t v, uint32_t* s_wave) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t up = __shfl_up(incl, o);
    if (lane >= static_cast<uint32_t>(o)) incl += up;
  }
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  for (uint32_t q = 0; q < wave; ++q) incl += s_wave[q];
  __syncthreads();
  return incl;
}
// chunk_sum[c] becomes the sum of the chunks before c; *total = the sum of all.  One workgroup, tiles of kBlock chunks with a carry.
__global__ __launch_bounds__(kBlock) void k_ndt_scan_chunks(uint32_t* __restrict__ chunk_sum, uint32_t count, uint32_t* __restrict__ total) {
  __shared__ uint32_t s_wave[kBlock / 64];
  __shared__ uint32_t s_carry;
  if (threadIdx.x == 0) s_carry = 0;
  __syncthreads();
  for (uint32_t start = 0; start < count; start += kBlock) {
    const uint32_t c = start + threadIdx.x;
    const uint32_t v = c < count ? chunk_sum[c] : 0u;
    const uint32_t incl = block_inclusive_u32(v, s_wave);
    const uint32_t carry = s_carry;
    if (c < count) chunk_sum[c] = carry + incl - v;
    __syncthreads();
    if (threadIdx.x == kBlock - 1) s_carry = carry + incl;
    __syncthreads();
  }
  if (threadIdx.x == 0) *total = s_carry;
}
__global__ __launch_bounds__(kBlock) void k_ndt_scan_apply(uint32_t* __restrict__ v, uint32_t n, const uint32_t* __restrict__ chunk_offset) {
  __shared__ uint32_t s_wave[kBlock / 64];
  const uint32_t base = blockIdx.x * kChunk + threadIdx.x * (kChunk / kBlock);
  uint32_t before[kChunk / kBlock];
  uint32_t run = 0;
#pragma unroll
  for (int k = 0; k < kChunk / kBlock; ++k) {
    before[k] = run;
    run += (base + k < n) ? v[base + k] : 0u;
  }
  const uint32_t prefix = chunk_offset[blockIdx.x] + block_inclusive_u32(run, s_wave) - run;
#pragma unroll
  for (int k = 0; k < kChunk / kBlock; ++k)
    if (base + k < n) v[base + k] = prefix + before[k];
}
void scan_u32(hipStream_t st, uint32_t* v, uint32_t n, uint32_t* chunk_tmp, uint32_t* total) {
  const uint32_t chunks = num_chunks(n);
  hipLaunchKernelGGL(k_ndt_scan_sums, dim3(chunks), dim3(kBlock), 0, st, v, n, chunk_tmp);
  hipLaunchKernelGGL(k_ndt_scan_chunks, dim3(1), dim3(kBlock), 0, st, chunk_tmp, chunks, total);
  hipLaunchKernelGGL(k_ndt_scan_apply, dim3(chunks), dim3(kBlock), 0, st, v, n, chunk_tmp);
}

// ---- one stable pass of the radix sort, by the digit at `shift` -------------------------------------------------------------------
// table[digit][chunk] = the chunk's count of that digit; its exclusive scan in that (digit-major) order is where the chunk's first
// element of the digit goes.
__global__ __launch_bounds__(kBlock) void k_ndt_radix_hist(const unsigned long long* __restrict__ words, uint32_t n, uint32_t shift,
                                                           uint32_t* __restrict__ table, uint32_t nblocks) {
  __shared__ uint32_t hist[kRadix];
  hist[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t base = blockIdx.x * kChunk;
#pragma unroll
  for (int k = 0; k < kChunk / kBlock; ++k) {
    const uint32_t e = base + k * kBlock + threadIdx.x;
    if (e < n) atomicAdd(&hist[static_cast<uint32_t>(words[e] >> shift) & (kRadix - 1)], 1u);
  }
  __syncthreads();
  table[static_cast<size_t>(threadIdx.x) * nblocks + blockIdx.x] = hist[threadIdx.x];
}
// The lanes of the wave that hold the same digit (an invalid lane: the invalid ones, which nobody uses): eight ballots.
__device__ __forceinline__ unsigned long long same_digit_lanes(uint32_t digit, bool valid) {
  unsigned long long same = __builtin_amdgcn_ballot_w64(valid);
  same = valid ? same : ~same;
#pragma unroll
  for (uint32_t bit = 0; bit < kRadixBits; ++bit) {
    const bool set = (digit >> bit) & 1u;
    const unsigned long long b = __builtin_amdgcn_ballot_w64(set);
    same &= set ? b : ~b;
  }
  return same;
}
// Every wave walks a contiguous quarter of the chunk 64 elements at a time: an element's rank among the chunk's elements of its digit
// = the wave's count of the digit so far (LDS) + the lanes below with the same digit; the waves' counts are then chained in wave
// order behind the chunk's place in the table.  idx_in == nullptr: the first pass (an element's index is its place).
__global__ __launch_bounds__(kBlock) void k_ndt_radix_scatter(const unsigned long long* __restrict__ words_in, const uint32_t* __restrict__ idx_in,
                                                              uint32_t n, uint32_t shift, const uint32_t* __restrict__ table, uint32_t nblocks,
                                                              unsigned long long* __restrict__ words_out, uint32_t* __restrict__ idx_out) {
  __shared__ uint32_t wave_count[kSortWaves][kRadix];  // counts, then first destinations
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < kSortWaves; ++q) wave_count[q][threadIdx.x] = 0;
  __syncthreads();
  volatile uint32_t* mine = wave_count[wave];
  const uint32_t base = blockIdx.x * kChunk + wave * (kChunk / kSortWaves);
  unsigned long long word[kSortRounds];
  uint32_t rank[kSortRounds];
#pragma unroll
  for (int k = 0; k < kSortRounds; ++k) {
    const uint32_t e = base + k * 64 + lane;
    const bool valid = e < n;
    word[k] = valid ? words_in[e] : 0ull;
    const uint32_t digit = static_cast<uint32_t>(word[k] >> shift) & (kRadix - 1);
    const unsigned long long same = same_digit_lanes(digit, valid);
    const uint32_t below = static_cast<uint32_t>(__popcll(same & ((1ull << lane) - 1ull)));
    const uint32_t before = valid ? mine[digit] : 0u;
    rank[k] = before + below;
    __builtin_amdgcn_wave_barrier();
    if (valid && below == 0) mine[digit] = before + static_cast<uint32_t>(__popcll(same));
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  {
    uint32_t run = table[static_cast<size_t>(threadIdx.x) * nblocks + blockIdx.x];
#pragma unroll
    for (int q = 0; q < kSortWaves; ++q) {
      const uint32_t c = wave_count[q][threadIdx.x];
      wave_count[q][threadIdx.x] = run;
      run += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kSortRounds; ++k) {
    const uint32_t e = base + k * 64 + lane;
    if (e < n) {
      const uint32_t to = wave_count[wave][static_cast<uint32_t>(word[k] >> shift) & (kRadix - 1)] + rank[k];
      words_out[to] = word[k];
      idx_out[to] = idx_in ? idx_in[e] : e;
    }
  }
}

// ---- cells ---------------------------------------------------------------------------------------------------------------------
// flags[t] = 1 where sorted position t is the first of a run of kMinPointsPerCell or more equal words (a cell the map keeps), else 0;
// kept_box = {min x, max x, min y, max y} of those cells' relative keys (initialised to UINT_MAX / 0 by the caller).
__global__ __launch_bounds__(kBlock) void k_ndt_mark_cells(const unsigned long long* __restrict__ words, uint32_t n, uint32_t* __restrict__ flags,
                                                           uint32_t* __restrict__ kept_box) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  bool kept = false;
  unsigned long long w = 0;
  if (t < n) {
    w = words[t];
    const bool head = t == 0 || words[t - 1] != w;
    const uint32_t last = t + (kMinPointsPerCell - 1);  // (n < 2^31: no wrap)
    kept = head && last < n && words[last] == w;
    flags[t] = kept ? 1u : 0u;
  }
  // (unsigned order through the signed wave reductions: the top bit flipped)
  const int32_t rx = static_cast<int32_t>(static_cast<uint32_t>(w >> 32) ^ 0x80000000u), ry = static_cast<int32_t>(static_cast<uint32_t>(w) ^ 0x80000000u);
  const int32_t x0 = wave_min_i32(kept ? rx : INT_MAX), x1 = wave_max_i32(kept ? rx : INT_MIN);
  const int32_t y0 = wave_min_i32(kept ? ry : INT_MAX), y1 = wave_max_i32(kept ? ry : INT_MIN);
  if ((threadIdx.x & 63) == 0 && x0 <= x1) {
    atomicMin(&kept_box[0], static_cast<uint32_t>(x0) ^ 0x80000000u);
    atomicMax(&kept_box[1], static_cast<uint32_t>(x1) ^ 0x80000000u);
    atomicMin(&kept_box[2], static_cast<uint32_t>(y0) ^ 0x80000000u);
    atomicMax(&kept_box[3], static_cast<uint32_t>(y1) ^ 0x80000000u);
  }
}
// offsets = the exclusive scan of the flags: a kept cell's first position t has offsets[t + 1] == offsets[t] + 1 (the last
// kMinPointsPerCell - 1 positions start no cell).  starts[cell] = t.
__global__ __launch_bounds__(kBlock) void k_ndt_cell_starts(const uint32_t* __restrict__ offsets, uint32_t n, uint32_t* __restrict__ starts) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t + 1 >= n) return;
  const uint32_t o = offsets[t];
  if (offsets[t + 1] != o) starts[o] = t;
}

// A lane per cell: fit_points over the cell's run, the points in input order (the sort is stable), as ndt_fit_cells adds them.
__global__ __launch_bounds__(kBlock) void k_ndt_fit_cells(const double2* __restrict__ pts, const unsigned long long* __restrict__ words,
                                                          const uint32_t* __restrict__ idx, uint32_t n, const uint32_t* __restrict__ starts,
                                                          uint32_t cells, NdtBuildLayout lay, double* __restrict__ records, int32_t* __restrict__ keys,
                                                          int32_t* __restrict__ grid) {
  const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
  if (c >= cells) return;
  const uint32_t first = starts[c];
  const unsigned long long w = words[first];
  uint32_t m = 0;
  double sx = 0.0, sy = 0.0;
  for (uint32_t t = first; t < n && words[t] == w; ++t, ++m) {
    const double2 p = pts[idx[t]];
    sx += p.x;
    sy += p.y;
  }
  const double mx = sx / static_cast<double>(m), my = sy / static_cast<double>(m);
  double cxx = 0.0, cxy = 0.0, cyy = 0.0;
  for (uint32_t t = first; t < first + m; ++t) {
    const double2 p = pts[idx[t]];
    const double dx = p.x - mx, dy = p.y - my;
    cxx += dx * dx;
    cxy += dx * dy;
    cyy += dy * dy;
  }
  const double denom = static_cast<double>(m - 1);  // sample covariance
  const double vxx = cxx / denom, vyy = cyy / denom;
  double2* rec = reinterpret_cast<double2*>(records + static_cast<size_t>(c) * kNdtRecord);
  rec[0] = double2{mx, my};
  rec[1] = double2{vxx < 1e-5 ? 1e-5 : vxx, cxy / denom};
  rec[2] = double2{vyy < 1e-5 ? 1e-5 : vyy, 0.0};
  const long long kx = lay.x0 + static_cast<long long>(w >> 32), ky = lay.y0 + static_cast<long long>(w & 0xFFFFFFFFull);
  keys[2 * c] = static_cast<int32_t>(kx);
  keys[2 * c + 1] = static_cast<int32_t>(ky);
  if (grid) grid[(ky - lay.grid_y0) * lay.gw + (kx - lay.grid_x0)] = static_cast<int32_t>(c);
}

// A lane per cell of the hashed layout (ndt_hash.h): the first empty slot from the key's home on is claimed by a compare-and-swap on its
// record word (the explicit empty marker), then takes the key.  The keys are distinct, so no lane ever needs to read another's key; a
// claimed slot stays claimed, so every slot between a key's home and its own is occupied - what ndt_hash_find relies on.  The walk is
// bounded by the capacity: with a load of at most 1/2 it ends long before, and a table that something else has filled loses the cell.
__global__ __launch_bounds__(kBlock) void k_ndt_hash_insert(const int32_t* __restrict__ keys, uint32_t cells, NdtSlot* __restrict__ slots,
                                                            uint32_t mask, uint32_t shift, uint32_t* __restrict__ longest) {
  const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
  if (c >= cells) return;
  const uint64_t key = ndt_pack_key(keys[2 * c], keys[2 * c + 1]);
  uint32_t at = ndt_hash_home(key, shift);
  for (uint32_t probe = 1;; ++probe, ++at) {
    NdtSlot* slot = slots + (at & mask);
    if (atomicCAS(&slot->record, kNdtNoRecord, static_cast<int32_t>(c)) == kNdtNoRecord) {
      slot->key = key;
      atomicMax(longest, probe);
      return;
    }
    if (probe > mask) return;  // (every slot seen)
  }
}

// ---- occupancy grid -> points ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_ndt_grid_flags(const int8_t* __restrict__ cells, uint32_t count, int8_t occupied, uint32_t* __restrict__ flags) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i < count) flags[i] = cells[i] == occupied ? 1u : 0u;
}
// The centre of occupied cell (xi, yi), origin * (resolution * (index + 0.5)), at the cell's rank among the occupied cells in row-major order.
__global__ __launch_bounds__(kBlock) void k_ndt_grid_points(const int8_t* __restrict__ cells, uint32_t W, uint32_t count, int8_t occupied,
                                                            const uint32_t* __restrict__ offsets, double resolution, Pose2 origin,
                                                            double2* __restrict__ pts) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= count || cells[i] != occupied) return;
  const uint32_t yi = i / W, xi = i - yi * W;
  const double lx = (static_cast<double>(xi) + 0.5) * resolution, ly = (static_cast<double>(yi) + 0.5) * resolution;
  double wx, wy;
  rot_apply(origin.r, lx, ly, wx, wy);
  pts[offsets[i]] = double2{wx + origin.x, wy + origin.y};
}

}  // namespace

void launch_ndt_key_box(hipStream_t st, const double* pts, uint32_t n, double resolution, int32_t* d_box) {
  hipLaunchKernelGGL(k_ndt_key_box, dim3(blocks_for(n)), dim3(kBlock), 0, st, reinterpret_cast<const double2*>(pts), n, resolution, d_box);
}

int launch_ndt_group_points(hipStream_t st, const double* pts, uint32_t n, double resolution, int32_t x0, int32_t y0, uint32_t bits_x,
                             uint32_t bits_y, const NdtBuildScratch& s) {
  hipLaunchKernelGGL(k_ndt_sort_keys, dim3(blocks_for(n)), dim3(kBlock), 0, st, reinterpret_cast<const double2*>(pts), n, resolution, x0, y0,
                     s.words[0]);
  const uint32_t nblocks = num_chunks(n);
  int from = 0;
  bool first = true;
  auto pass = [&](uint32_t shift) {
    hipLaunchKernelGGL(k_ndt_radix_hist, dim3(nblocks), dim3(kBlock), 0, st, s.words[from], n, shift, s.table, nblocks);
    scan_u32(st, s.table, static_cast<uint32_t>(kRadix) * nblocks, s.chunk_tmp, s.counters + kNdtCountScratch);
    hipLaunchKernelGGL(k_ndt_radix_scatter, dim3(nblocks), dim3(kBlock), 0, st, s.words[from], first ? nullptr : s.idx[from], n, shift, s.table,
                       nblocks, s.words[1 - from], s.idx[1 - from]);
    from = 1 - from;
    first = false;
  };
  for (uint32_t b = 0; b < bits_y; b += kRadixBits) pass(b);
  for (uint32_t b = 0; b < bits_x; b += kRadixBits) pass(32 + b);
  if (first) pass(0);  // (a single cell: the index list still has to be written)
  // the sorted lists are in words[from] / idx[from]
  hipLaunchKernelGGL(k_ndt_mark_cells, dim3(blocks_for(n)), dim3(kBlock), 0, st, s.words[from], n, s.flags, s.counters + kNdtCountKeptBox);
  scan_u32(st, s.flags, n, s.chunk_tmp, s.counters + kNdtCountCells);
  return from;
}
size_t ndt_radix_table_words(uint32_t n) { return static_cast<size_t>(kRadix) * num_chunks(n); }

void launch_ndt_fit_cells(hipStream_t st, const double* pts, uint32_t n, const NdtBuildScratch& s, int sorted, uint32_t cells,
                          const NdtBuildLayout& lay, double* records, int32_t* keys, int32_t* grid) {
  hipLaunchKernelGGL(k_ndt_cell_starts, dim3(blocks_for(n)), dim3(kBlock), 0, st, s.flags, n, s.starts);
  hipLaunchKernelGGL(k_ndt_fit_cells, dim3(blocks_for(cells)), dim3(kBlock), 0, st, reinterpret_cast<const double2*>(pts), s.words[sorted],
                     s.idx[sorted], n, s.starts, cells, lay, records, keys, grid);
}

void launch_ndt_hash_insert(hipStream_t st, const int32_t* keys, uint32_t cells, NdtSlot* slots, uint32_t mask, uint32_t shift, uint32_t* d_longest) {
  hipLaunchKernelGGL(k_ndt_hash_insert, dim3(blocks_for(cells)), dim3(kBlock), 0, st, keys, cells, slots, mask, shift, d_longest);
}

void launch_ndt_grid_offsets(hipStream_t st, const int8_t* cells, uint32_t count, int8_t occupied, uint32_t* offsets, uint32_t* chunk_tmp,
                             uint32_t* d_total) {
  hipLaunchKernelGGL(k_ndt_grid_flags, dim3(blocks_for(count)), dim3(kBlock), 0, st, cells, count, occupied, offsets);
  scan_u32(st, offsets, count, chunk_tmp, d_total);
}
void launch_ndt_grid_points(hipStream_t st, const int8_t* cells, uint32_t W, uint32_t H, int8_t occupied, const uint32_t* offsets,
                            double resolution, Pose2 origin, double* pts) {
  const uint32_t count = W * H;
  hipLaunchKernelGGL(k_ndt_grid_points, dim3(blocks_for(count)), dim3(kBlock), 0, st, cells, W, count, occupied, offsets, resolution, origin,
                     reinterpret_cast<double2*>(pts));
}

}  // namespace mcl
