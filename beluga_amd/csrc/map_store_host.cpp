// map_store_host.cpp — see map_store_host.h.
#include "map_store_host.h"

#include <algorithm>

namespace mcl {

namespace {
bool likelihood_field_kind(int32_t kind) { return kind == MCL_SENSOR_LIKELIHOOD_FIELD || kind == MCL_SENSOR_LIKELIHOOD_FIELD_PROB; }
}  // namespace

const char* map_store_check_kind(int32_t sensor_kind) {
  if (sensor_kind == MCL_SENSOR_BEAM || likelihood_field_kind(sensor_kind)) return nullptr;
  return "mcl_shared_map_create: only the likelihood-field and beam models read an occupancy-grid map (NDT, landmark and bearing contexts have maps of their own)";
}

const char* map_store_mismatch(const MapStoreKey& store, int32_t device, int32_t sensor_kind, const mcl_lf_params& lf) {
  if (store.device != device) return "mcl_use_shared_map: the map is on another device than the context";
  if (sensor_kind == MCL_SENSOR_BEAM || store.sensor_kind == MCL_SENSOR_BEAM) {
    if (sensor_kind != store.sensor_kind) return "mcl_use_shared_map: a beam-model map serves beam-model contexts only, a likelihood-field map none of them";
    return nullptr;
  }
  if (sensor_kind != store.sensor_kind) return "mcl_use_shared_map: sensor_kind differs (likelihood field against likelihood field prob: their tables differ)";
  if (lf.max_obstacle_distance != store.lf.max_obstacle_distance) return "mcl_use_shared_map: lf.max_obstacle_distance differs from the map's";
  if (lf.max_laser_distance != store.lf.max_laser_distance) return "mcl_use_shared_map: lf.max_laser_distance differs from the map's";
  if (lf.z_hit != store.lf.z_hit) return "mcl_use_shared_map: lf.z_hit differs from the map's";
  if (lf.z_random != store.lf.z_random) return "mcl_use_shared_map: lf.z_random differs from the map's";
  if (lf.sigma_hit != store.lf.sigma_hit) return "mcl_use_shared_map: lf.sigma_hit differs from the map's";
  if (lf.model_unknown_space != store.lf.model_unknown_space) return "mcl_use_shared_map: lf.model_unknown_space differs from the map's";
  if (lf.only_obstacle_boundaries != store.lf.only_obstacle_boundaries) return "mcl_use_shared_map: lf.only_obstacle_boundaries differs from the map's";
  return nullptr;
}

MapTableLayout map_table_layout(uint32_t W, uint32_t H) {
  MapTableLayout t{};
  t.tiles_x = (static_cast<uint64_t>(W) + 7) / 8 + 2;
  t.tiles_y = (static_cast<uint64_t>(H) + 7) / 8 + 2;
  const uint64_t pal_base = ((static_cast<uint64_t>(H) + 2) * 4u + 7u) & ~7ull;
  t.palette_possible = t.tiles_x * t.tiles_y * 128 < (1ull << 31) && W < (1u << 26) && pal_base + 8 <= 65536;
  if (!t.palette_possible) return t;
  t.pal_base = static_cast<uint32_t>(pal_base);
  t.max_entries = static_cast<uint32_t>(std::min<uint64_t>(kMapMaxPalette, (65536 - pal_base) / 8));
  t.pal_idx_count = t.tiles_x * t.tiles_y * 64;
  t.pal_pitch = static_cast<uint32_t>(t.tiles_x * 128);
  t.pal_bytes = static_cast<uint32_t>(t.tiles_x * t.tiles_y * 128);
  t.far_row_bytes = static_cast<uint32_t>((t.tiles_x + 7) / 8);
  t.far_bytes = static_cast<uint32_t>((static_cast<uint64_t>(t.far_row_bytes) * t.tiles_y + 15) & ~15ull);
  t.far_possible = t.tiles_x * t.tiles_y < (1ull << 31) && t.far_bytes <= 48 * 1024 && t.far_row_bytes < (1u << 13);
  t.far_linear_bytes = static_cast<uint32_t>(((t.tiles_x * t.tiles_y + 7) / 8 + 15) & ~15ull);
  return t;
}

MapStoreBytes map_store_bytes(const MapStoreShape& s) {
  const uint64_t cells = static_cast<uint64_t>(s.W) * s.H;
  MapStoreBytes b{0, 0};
  b.device += cells;                                  // occupancy
  b.device += 4 * std::max<uint64_t>(s.n_free, 1);    // free-cell list
  if (s.sensor_kind == MCL_SENSOR_BEAM) {
    b.device += 4 * s.nonfree_words;
    return b;
  }
  b.device += 4 * cells;        // field
  b.device += 8 * (cells + 1);  // pz^3 table (+1 slot for out-of-grid beams)
  b.host += 4 * cells;          // the host copy of the field
  const MapTableLayout t = map_table_layout(s.W, s.H);
  if (s.pal_count && t.palette_possible) {
    b.device += (4 + 8) * static_cast<uint64_t>(s.pal_count);  // keys, values
    b.device += 2 * t.pal_idx_count;
    if (t.far_possible) {
      b.device += 4 * static_cast<uint64_t>(s.pal_count);  // votes
      b.device += t.far_bytes;
      if (s.far_tiles) b.device += t.far_linear_bytes;
    }
  }
  return b;
}

}  // namespace mcl
