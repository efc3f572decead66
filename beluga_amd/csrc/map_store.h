// map_store.h — MapStore: everything that is held on behalf of one occupancy-grid map, on the host and on one device.  A context reads
// its map only through a store (mcl_ctx::map, a MapHold): a private one that mcl_set_map built for it, or one that
// mcl_shared_map_create built and any number of contexts read (mcl_use_shared_map).  A store does not change once its builder
// (context.hip build_map_store) has returned it; a new map, or a new field, is a new store.  What a context builds lazily or from
// parameters of its own - the beam range table, scratch, the planner's statistics - stays in the context.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <utility>
#include <vector>

#include "kernels.h"
#include "map_build.h"
#include "map_store_host.h"

namespace mcl {

template <class T>
struct DeviceBuffer {
  T* ptr{nullptr};
  size_t count{0};
  DeviceBuffer() = default;
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
  // (hipFree takes no stream: the owner sees to it that the device is bound and that nothing on it still reads the memory)
  ~DeviceBuffer() { release(); }
  hipError_t ensure(size_t n) {
    if (n <= count) return hipSuccess;
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    count = 0;
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&ptr), n * sizeof(T));
    if (e == hipSuccess) count = n;
    return e;
  }
  void release() {
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    count = 0;
  }
  // The other buffer's memory instead of this one's (a store built in the place of a private one takes its buffers over).
  void take(DeviceBuffer& other) {
    release();
    std::swap(ptr, other.ptr);
    std::swap(count, other.count);
  }
  uint64_t bytes() const { return static_cast<uint64_t>(count) * sizeof(T); }
};

// Pinned host memory, and - mapped - the address the device sees it at.
template <class T>
struct HostBuffer {
  T* host{nullptr};
  T* device{nullptr};
  size_t count{0};
  HostBuffer() = default;
  HostBuffer(const HostBuffer&) = delete;
  HostBuffer& operator=(const HostBuffer&) = delete;
  ~HostBuffer() { release(); }
  hipError_t ensure(size_t n, bool mapped) {
    if (n <= count) return hipSuccess;
    release();
    hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&host), n * sizeof(T), mapped ? hipHostMallocMapped : hipHostMallocDefault);
    if (e == hipSuccess && mapped) e = hipHostGetDevicePointer(reinterpret_cast<void**>(&device), host, 0);
    if (e == hipSuccess) count = n;
    return e;
  }
  void release() {
    if (host) (void)hipHostFree(host);
    host = device = nullptr;
    count = 0;
  }
};

// A pinned buffer the host fills and one stream reads behind the call that filled it, and what the next fill has to wait for:
// reserve() before every fill, used() right behind the copy or the launch that reads the memory, idle() where the stream has been synchronised.
template <class T>
struct StagedUpload {
  HostBuffer<T> buf;
  hipEvent_t event{nullptr};  // made by the first use that asks for one, destroyed with the owner
  bool in_flight{false}, event_valid{false};  // a use may still be reading buf; `event` stands behind it (otherwise only the stream's end does)
  ~StagedUpload() { if (event) (void)hipEventDestroy(event); }
  // Waits for the previous use - its event, or without one all that `stream` holds - and grows the buffer to n elements.
  hipError_t reserve(hipStream_t stream, size_t n, bool mapped) {
    if (in_flight)
      if (const hipError_t e = event_valid ? hipEventSynchronize(event) : hipStreamSynchronize(stream); e != hipSuccess) return e;
    in_flight = false;
    return buf.ensure(n, mapped);
  }
  // with_event: the caller may return before the stream is synchronised, so the next reserve() waits for this use alone.  Without
  // one nothing is recorded on the stream (the update cycle, which always ends in a synchronisation and idle()).
  hipError_t used(hipStream_t stream, bool with_event) {
    in_flight = true;
    event_valid = false;  // (a failure below leaves the next reserve() the stream to wait for)
    if (!with_event) return hipSuccess;
    hipError_t e = event ? hipSuccess : hipEventCreateWithFlags(&event, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(event, stream);
    event_valid = e == hipSuccess;
    return e;
  }
  void idle() { in_flight = false; }
};

struct MapStore {
  MapStoreKey key{0, MCL_SENSOR_LIKELIHOOD_FIELD, {}};
  struct Rebind {  // (see ~MapStore)
    int device{-1};
    ~Rebind() {
      if (device >= 0) (void)hipSetDevice(device);
    }
  } rebind;
  // geometry
  uint32_t W{0}, H{0};
  double resolution{0};
  Pose2 origin{}, origin_inverse{};
  OccupancyTraits traits{0, -1, 100};
  // occupancy and the free cells (every kind)
  DeviceBuffer<int8_t> d_cells;
  DeviceBuffer<uint32_t> d_free;
  uint64_t n_free{0};
  DeviceBuffer<uint32_t> d_nonfree_bits;  // beam model: 1 bit per cell and the coarse bitmaps (NonFreeBits)
  // the likelihood-field kinds
  std::vector<float> h_field;
  DeviceBuffer<float> d_field;
  DeviceBuffer<double> d_cube;  // pz^3 table of the field (+1 slot for out-of-grid beams)
  // palette form of the same table (FieldView::pal_*), built when the field has <= kMaxPalette distinct values
  DeviceBuffer<uint16_t> d_pal_idx;
  DeviceBuffer<double> d_pal_val;
  DeviceBuffer<uint32_t> d_pal_keys;
  uint32_t pal_count{0}, pal_pitch{0}, pal_base{0}, pal_bytes{0};
  DeviceBuffer<uint8_t> d_far_bits;   // FieldView::far_bits: tiles of d_pal_idx uniformly equal to the table's most common entry
  DeviceBuffer<uint32_t> d_far_votes;
  uint32_t far_row_bytes{0}, far_bytes{0}, far_entry{0};
  DeviceBuffer<uint8_t> d_far_linear;  // FieldView::far_linear: the same bits by the tiles' linear index
  uint32_t far_linear_bytes{0};
  uint64_t far_tiles{0};  // number of set bits' worth of tiles voted for far_entry (0 = no bitmap)
  // how the field came to be
  bool field_built_on_device{false};
  double field_build_ms{0.0};
  // contexts that read the store through mcl_use_shared_map (MapHold)
  mutable std::atomic<uint32_t> users{0};

  MapStore() = default;
  MapStore(const MapStore&) = delete;
  MapStore& operator=(const MapStore&) = delete;
  // Binds the store's device for the buffers' destructors, which run behind this body; `rebind`, declared in front of every buffer and
  // so destroyed behind them all, gives the caller its device back.
  ~MapStore() {
    if (!device_bytes()) return;
    int current = 0;
    if (hipGetDevice(&current) == hipSuccess && current != key.device) rebind.device = current;
    (void)hipSetDevice(key.device);
  }

  uint64_t device_bytes() const {
    return d_cells.bytes() + d_free.bytes() + d_nonfree_bits.bytes() + d_field.bytes() + d_cube.bytes() + d_pal_idx.bytes() + d_pal_val.bytes() +
           d_pal_keys.bytes() + d_far_bits.bytes() + d_far_votes.bytes() + d_far_linear.bytes();
  }
  uint64_t host_bytes() const { return static_cast<uint64_t>(h_field.size()) * sizeof(float); }
  // The buffers of a private store that nobody reads any more, to be filled again.
  void take_buffers(MapStore& old) {
    d_cells.take(old.d_cells);
    d_free.take(old.d_free);
    d_nonfree_bits.take(old.d_nonfree_bits);
    d_field.take(old.d_field);
    d_cube.take(old.d_cube);
    d_pal_idx.take(old.d_pal_idx);
    d_pal_val.take(old.d_pal_val);
    d_pal_keys.take(old.d_pal_keys);
    d_far_bits.take(old.d_far_bits);
    d_far_votes.take(old.d_far_votes);
    d_far_linear.take(old.d_far_linear);
    h_field.swap(old.h_field);
  }
};

}  // namespace mcl
