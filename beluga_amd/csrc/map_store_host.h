// map_store_host.h — what a map store (map_store.h) decides and counts without touching device memory: which contexts may read a store,
// how the palette and far-tile tables of a W x H field are laid out, how many bytes a store holds, and a context's counted hold on a
// store.  context.hip calls them around its uploads and launches.  Plain C++17, no HIP.
#pragma once

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <memory>
#include <utility>

#include "beluga_mcl.h"

namespace mcl {

// ---- who may read a store ------------------------------------------------------------------------------------------------------------
// What a store was built for: everything of a config that its contents depend on.
struct MapStoreKey {
  int32_t device;
  int32_t sensor_kind;  // MCL_SENSOR_BEAM, MCL_SENSOR_LIKELIHOOD_FIELD or MCL_SENSOR_LIKELIHOOD_FIELD_PROB
  mcl_lf_params lf;     // (the likelihood-field kinds: the field, the pz^3 table and the palette are functions of all of it)
};
// mcl_shared_map_create: the sensor kinds with an occupancy-grid map.  nullptr: fine; otherwise what is wrong.
const char* map_store_check_kind(int32_t sensor_kind);
// mcl_use_shared_map: may a context of this device, kind and likelihood-field parameters read the store?  nullptr: yes; otherwise the
// mismatch.  The beam model compares the device and the family only; the likelihood-field models also the kind (the pz^3 table of
// LF-prob is another table) and every field of mcl_lf_params.
const char* map_store_mismatch(const MapStoreKey& store, int32_t device, int32_t sensor_kind, const mcl_lf_params& lf);

// ---- the tables over a W x H field -----------------------------------------------------------------------------------------------------
constexpr uint32_t kMapMaxPalette = 2048;  // (kernels.h kMaxPalette)
struct MapTableLayout {
  uint64_t tiles_x, tiles_y;    // 8 x 8-cell tiles, one border tile on every side
  uint32_t pal_base;            // bytes of the LF kernels' row-offset table, which comes first in LDS
  bool palette_possible;        // the tiled index table can be addressed with 32 bits and its entries fit behind pal_base
  uint32_t max_entries;         // of a palette (<= kMapMaxPalette)
  uint64_t pal_idx_count;       // uint16 entries of the tiled index table
  uint32_t pal_pitch, pal_bytes;
  uint32_t far_row_bytes, far_bytes;  // the far-tile bitmap by rows of tiles
  bool far_possible;                  // ... fits the kernels' LDS budget
  uint32_t far_linear_bytes;          // the same bits by the tiles' linear index
};
MapTableLayout map_table_layout(uint32_t W, uint32_t H);

// ---- bytes -----------------------------------------------------------------------------------------------------------------------------
// What the builder found of one map; nonfree_words: the beam model's packed occupancy (kernels.h nonfree_words), 0 otherwise.
struct MapStoreShape {
  int32_t sensor_kind;
  uint32_t W, H;
  uint64_t n_free;
  uint64_t nonfree_words;
  uint32_t pal_count;  // distinct values of the field incl. the unknown value, 0: no palette
  bool far_tiles;      // the far-tile vote passed
};
struct MapStoreBytes {
  uint64_t device, host;
};
// The bytes a store built from nothing holds for that map (a private store that took over larger buffers holds those).
MapStoreBytes map_store_bytes(const MapStoreShape& s);

// ---- a context's hold on a store -----------------------------------------------------------------------------------------------------
// Store: any type with a member `mutable std::atomic<uint32_t> users` - the contexts that read it through mcl_use_shared_map.  The
// hold never is empty: a context without a map holds `none`, a store of no cells.  A private store (own) is not counted.
template <class Store>
class MapHold {
 public:
  explicit MapHold(std::shared_ptr<const Store> none) : none_(none), store_(std::move(none)) {}
  MapHold(const MapHold&) = delete;
  MapHold& operator=(const MapHold&) = delete;
  ~MapHold() { drop(); }
  const Store* operator->() const { return store_.get(); }
  const Store& operator*() const { return *store_; }
  const std::shared_ptr<const Store>& ptr() const { return store_; }
  bool shared() const { return shared_; }
  // A private store, built for this context alone.
  void own(std::shared_ptr<const Store> s) {
    drop();
    store_ = std::move(s);
  }
  // A store that other contexts read as well.
  void attach(std::shared_ptr<const Store> s) {
    s->users.fetch_add(1, std::memory_order_relaxed);  // (before the old one goes: attaching the store already held keeps it alive)
    drop();
    store_ = std::move(s);
    shared_ = true;
  }
  // Back to no map.  The store dies here if this was its last reference.
  void drop() {
    if (shared_) store_->users.fetch_sub(1, std::memory_order_relaxed);
    shared_ = false;
    store_ = none_;
  }
  // A private store gives itself up for its buffers (nullptr: the hold is shared, or holds no map): the caller is its only owner.
  // (Every store is created as a plain object; only the views handed out are const.)
  std::shared_ptr<Store> take_private() {
    if (shared_ || store_ == none_ || store_.use_count() != 1) return nullptr;
    std::shared_ptr<Store> s = std::const_pointer_cast<Store>(store_);
    store_ = none_;
    return s;
  }

 private:
  std::shared_ptr<const Store> none_, store_;
  bool shared_{false};
};

}  // namespace mcl
