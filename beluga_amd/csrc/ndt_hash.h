// ndt_hash.h — the hashed layout of an NDT map's cells (mcl_set_ndt_map_layout): an open-addressing table from a cell's key
// (int32 x, int32 y) to the number of its record, for maps whose keys' box is too large for the dense index grid (kernels.h NdtMapView).
// One piece of source for the host (ndt_host.cpp builds the table, the CPU tests probe it) and the kernels (ndt_kernels.hip), so plain
// C++: <cstdint> and MCL_HD.
//
//   slots    : 2^c of them, c = the smallest >= 1 with 2^c >= 2 n for n cells: the load is at most 1/2.  A slot holds the packed key
//              and the record number; record < 0 (kNdtNoRecord) marks an empty slot - every 64-bit word is some key, (-1, -1) included,
//              so the key word cannot say it.
//   key      : (uint32(x) << 32) | uint32(y).
//   hash     : home = (key * 0x9E3779B97F4A7C15) >> (64 - c): the Fibonacci multiply (2^64 / golden ratio, the multiplier of the
//              reference's spatial_hash.hpp), the top c bits kept.
//   probing  : linear, every index masked with 2^c - 1.  A key stored `d` slots behind its home has d occupied slots in front of it,
//              so a look-up ends at the key, at an empty slot, or after `longest_probe` slots - the most slots any stored key needed,
//              recorded by whoever built the table.  The bound is what ends the loop: a table that a bug has filled or whose slots
//              were overwritten gives "none" (a wrong weight) after longest_probe reads, whatever the slots hold.
//   neighbours: a centre key plus a kernel offset is formed in 64 bits; a neighbour key that does not fit an int32 is no key of any
//              map (mcl_set_ndt_map takes int32 keys) and is NOT probed: packing it would wrap it onto another cell's key.
#pragma once
#include <cstdint>

#include "se2.h"  // MCL_HD

namespace mcl {

constexpr uint64_t kNdtHashMultiplier = 0x9E3779B97F4A7C15ull;
constexpr int32_t kNdtNoRecord = -1;

struct alignas(16) NdtSlot {
  uint64_t key;
  int32_t record;  // kNdtNoRecord: empty
  int32_t unused;
};
struct NdtHashTable {
  const NdtSlot* slots;
  uint32_t mask;           // 2^c - 1
  uint32_t shift;          // 64 - c, 32 .. 63
  uint32_t longest_probe;  // slots read for the stored key that is farthest from its home, at least 1
};

// c for n cells (n < 2^31): 1 .. 32.
MCL_HD uint32_t ndt_hash_log2_capacity(uint64_t n) {
  uint32_t c = 1;
  while ((uint64_t{1} << c) < 2 * n) ++c;
  return c;
}
MCL_HD uint64_t ndt_pack_key(int32_t x, int32_t y) {
  return (static_cast<uint64_t>(static_cast<uint32_t>(x)) << 32) | static_cast<uint64_t>(static_cast<uint32_t>(y));
}
MCL_HD uint32_t ndt_hash_home(uint64_t key, uint32_t shift) { return static_cast<uint32_t>((key * kNdtHashMultiplier) >> shift); }

// The record number of `key`, kNdtNoRecord if the table does not hold it.
MCL_HD int32_t ndt_hash_find(const NdtHashTable& t, uint64_t key) {
  uint32_t at = ndt_hash_home(key, t.shift);
  for (uint32_t probe = 0; probe < t.longest_probe; ++probe, ++at) {
    const NdtSlot s = t.slots[at & t.mask];
    if (s.record < 0) return kNdtNoRecord;
    if (s.key == key) return s.record;
  }
  return kNdtNoRecord;
}
// ... of the neighbour (cx + dx, cy + dy) of a centre key; kNdtNoRecord, nothing read, where that is not an int32 key.
MCL_HD int32_t ndt_hash_find_neighbour(const NdtHashTable& t, int64_t cx, int64_t cy, int32_t dx, int32_t dy) {
  const int64_t x = cx + dx, y = cy + dy;
  if (x < INT32_MIN || x > INT32_MAX || y < INT32_MIN || y > INT32_MAX) return kNdtNoRecord;
  return ndt_hash_find(t, ndt_pack_key(static_cast<int32_t>(x), static_cast<int32_t>(y)));
}

}  // namespace mcl
