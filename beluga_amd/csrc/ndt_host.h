// ndt_host.h — the host passes of the 2D NDT sensor model: the fit of a scan's measurement cells (detail::to_cells), the cell record
// and the layout of a map given as cells (mcl_set_ndt_map).  Host only: beluga_mcl.h and the standard library, no HIP and no mcl_ctx, so
// that a plain C++ compiler can build and check it (like cluster_host.cpp and map_build.cpp).  The device side - the reweight kernel and
// the map built from points - is in ndt_kernels.hip and ndt_build_kernels.hip; context.hip uploads what these functions return.
// A function that can refuse its input returns the status and leaves the message in *error.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "beluga_mcl.h"
#include "ndt_hash.h"
#include "sensor_records.h"

namespace mcl {

// A cell record (kNdtRecord doubles: mean x, y, covariance xx, xy, yy, 0) from and to mean[2] and a row-major covariance[4].
inline void ndt_pack_record(const double* mean, const double* cov, double* rec) {
  rec[0] = mean[0], rec[1] = mean[1], rec[2] = cov[0], rec[3] = cov[1], rec[4] = cov[3], rec[5] = 0.0;
}
inline void ndt_unpack_record(const double* rec, double* mean, double* cov) {
  mean[0] = rec[0], mean[1] = rec[1], cov[0] = rec[2], cov[1] = rec[3], cov[2] = rec[3], cov[3] = rec[4];
}

// detail::to_cells (ndt_sensor_model.hpp:88-110) with fit_points (:66-80): one record per cell into `out` (cleared first), the cells in
// ascending key order (the reference's order is an unordered_map's: only the rounding of the weight's sum depends on it).  The group
// key is (p / resolution).cast<int>() - division and truncation toward zero, NOT the floor of cell_near.  Points that are not finite or
// whose key does not fit an int are dropped (the reference's cast is undefined there).
void ndt_fit_cells(const double* pts, uint64_t B, double resolution, std::vector<double>& out);

// The index grid of an NDT map over the keys' box [x0, x1] x [y0, y1] (kernels.h NdtMapView): the box with a border of 2 * reach.
struct NdtGridShape {
  int32_t reach;
  int64_t x0, y0, x1, y1;
  int64_t grid_x0, grid_y0;  // key of the grid's cell (0, 0)
  int64_t gw, gh;
  bool fits;  // within 2^26 cells
};
int32_t ndt_reach(const mcl_ndt_params& prm);  // the largest |component| of a kernel offset, at least 1
NdtGridShape ndt_grid_shape(int32_t reach, int64_t x0, int64_t x1, int64_t y0, int64_t y1);

// A map given as n cells - keys (x, y) (cell_near of the means: a floor), means[2], row-major covariances[4] - checked and laid out as
// NdtMapView wants it.  Everything mcl_set_ndt_map can refuse without its context is refused here, in its order and its words.
struct NdtMapLayout {
  mcl_ndt_params params;        // the caller's, the defaults where there were none
  NdtGridShape shape;
  std::vector<int32_t> grid;    // shape.gw x shape.gh, row-major: the number of the cell with that key, -1 where there is none
  std::vector<double> records;  // one per cell, in the caller's order
};
mcl_status ndt_layout_map(const int32_t* cells, const double* means, const double* covariances, uint64_t n, double resolution,
                          const mcl_ndt_params* params, NdtMapLayout* out, std::string* error);

// The layout mode of a context (mcl_set_ndt_map_layout) and what it makes of the next map: the hashed table (ndt_hash.h) instead of
// the index grid - always, or where the grid would not fit.
enum NdtLayoutMode : int32_t { kNdtLayoutDense = 0, kNdtLayoutAuto = 1, kNdtLayoutHashed = 2 };
inline bool ndt_layout_mode_valid(int32_t mode) { return mode >= kNdtLayoutDense && mode <= kNdtLayoutHashed; }
inline bool ndt_map_is_hashed(int32_t mode, bool grid_fits) { return mode == kNdtLayoutHashed || (mode == kNdtLayoutAuto && !grid_fits); }

// The same map laid out as NdtHashView wants it: ndt_layout_map's checks in its order and its words, except that no box is too large
// (shape.fits only reports what the dense layout would have said; shape's box and reach are what the kernels test first).
struct NdtHashLayout {
  mcl_ndt_params params;
  NdtGridShape shape;
  uint32_t log2_capacity;      // ndt_hash_log2_capacity(n)
  uint32_t longest_probe;      // the most slots any key needed, its own included
  std::vector<NdtSlot> slots;  // 2^log2_capacity
  std::vector<double> records;  // one per cell, in the caller's order
  NdtHashTable table() const { return NdtHashTable{slots.data(), static_cast<uint32_t>(slots.size() - 1), 64 - log2_capacity, longest_probe}; }
};
// Whether the dense index grid of these keys would fit (ndt_grid_shape of their box), asked BEFORE any layout so that mode 1 checks a
// map once: arguments that both layouts refuse anyway (no cells, too many, a bad number of offsets) count as fitting.
bool ndt_keys_fit_grid(const int32_t* cells, uint64_t n, const mcl_ndt_params* params);
mcl_status ndt_layout_map_hashed(const int32_t* cells, const double* means, const double* covariances, uint64_t n, double resolution,
                                 const mcl_ndt_params* params, NdtHashLayout* out, std::string* error);

}  // namespace mcl
