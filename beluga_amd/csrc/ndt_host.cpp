// ndt_host.cpp — see ndt_host.h.  Also the NDT entries of the C ABI that take no context.
#include "ndt_host.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>

namespace mcl {

#define NDT_REQUIRE(cond, msg) \
  do { if (!(cond)) { if (error) *error = (msg); return MCL_ERR_INVALID_ARGUMENT; } } while (0)

void ndt_fit_cells(const double* pts, uint64_t B, double resolution, std::vector<double>& out) {
  out.clear();
  std::vector<std::pair<std::pair<int32_t, int32_t>, uint64_t>> keyed;
  keyed.reserve(B);
  for (uint64_t i = 0; i < B; ++i) {
    const double qx = pts[2 * i] / resolution, qy = pts[2 * i + 1] / resolution;
    if (!(std::abs(qx) < 2147483647.0 && std::abs(qy) < 2147483647.0)) continue;
    keyed.push_back({{static_cast<int32_t>(qx), static_cast<int32_t>(qy)}, i});
  }
  std::sort(keyed.begin(), keyed.end());
  for (size_t a = 0; a < keyed.size();) {
    size_t b = a;
    while (b < keyed.size() && keyed[b].first == keyed[a].first) ++b;
    const size_t m = b - a;
    if (m >= 5) {  // kMinPointsPerCell
      double sx = 0.0, sy = 0.0;
      for (size_t t = a; t < b; ++t) {
        sx += pts[2 * keyed[t].second];
        sy += pts[2 * keyed[t].second + 1];
      }
      const double mx = sx / static_cast<double>(m), my = sy / static_cast<double>(m);
      double cxx = 0.0, cxy = 0.0, cyy = 0.0;
      for (size_t t = a; t < b; ++t) {
        const double dx = pts[2 * keyed[t].second] - mx, dy = pts[2 * keyed[t].second + 1] - my;
        cxx += dx * dx;
        cxy += dx * dy;
        cyy += dy * dy;
      }
      const double denom = static_cast<double>(m - 1);  // sample covariance
      const double mean[2] = {mx, my}, cov[4] = {std::max(cxx / denom, 1e-5), cxy / denom, cxy / denom, std::max(cyy / denom, 1e-5)};
      out.resize(out.size() + kNdtRecord);
      ndt_pack_record(mean, cov, out.data() + out.size() - kNdtRecord);
    }
    a = b;
  }
}

int32_t ndt_reach(const mcl_ndt_params& prm) {
  int32_t reach = 1;
  for (uint32_t k = 0; k < 2 * prm.num_offsets; ++k) reach = std::max(reach, std::abs(prm.offsets[k]));
  return reach;
}

NdtGridShape ndt_grid_shape(int32_t reach, int64_t x0, int64_t x1, int64_t y0, int64_t y1) {
  NdtGridShape g{reach, x0, y0, x1, y1, x0 - 2 * reach, y0 - 2 * reach, (x1 - x0 + 1) + 4 * reach, (y1 - y0 + 1) + 4 * reach, false};
  constexpr int64_t kMaxGridCells = int64_t{1} << 26;
  g.fits = !(g.gw > kMaxGridCells || g.gh > kMaxGridCells || g.gw * g.gh > kMaxGridCells);
  return g;
}

namespace {

// What both layouts check before the box matters: the arguments, the parameters into `prm`, every cell's values; the keys' box.
mcl_status ndt_check_map(const int32_t* cells, const double* means, const double* covariances, uint64_t n, double resolution,
                         const mcl_ndt_params* params, mcl_ndt_params& prm, NdtGridShape* shape, std::string* error) {
  NDT_REQUIRE(cells && means && covariances && n > 0, "mcl_set_ndt_map: null argument or no cells");
  NDT_REQUIRE(n < (1ull << 31), "mcl_set_ndt_map: too many cells");
  NDT_REQUIRE(std::isfinite(resolution) && resolution > 0.0, "mcl_set_ndt_map: resolution must be positive and finite");
  if (params) prm = *params;
  else mcl_default_ndt_params(&prm);
  NDT_REQUIRE(prm.num_offsets >= 1 && prm.num_offsets <= MCL_NDT_MAX_OFFSETS, "mcl_set_ndt_map: 1 .. 32 kernel offsets");
  NDT_REQUIRE(std::isfinite(prm.d1) && std::isfinite(prm.d2) && std::isfinite(prm.minimum_likelihood) && prm.minimum_likelihood >= 0.0,
              "mcl_set_ndt_map: d1, d2 must be finite and minimum_likelihood finite and >= 0");
  for (uint32_t k = 0; k < 2 * prm.num_offsets; ++k)
    NDT_REQUIRE(prm.offsets[k] >= -64 && prm.offsets[k] <= 64, "mcl_set_ndt_map: kernel offsets are limited to 64 cells");
  int64_t x0 = INT64_MAX, y0 = INT64_MAX, x1 = INT64_MIN, y1 = INT64_MIN;
  for (uint64_t i = 0; i < n; ++i) {
    x0 = std::min<int64_t>(x0, cells[2 * i]);
    x1 = std::max<int64_t>(x1, cells[2 * i]);
    y0 = std::min<int64_t>(y0, cells[2 * i + 1]);
    y1 = std::max<int64_t>(y1, cells[2 * i + 1]);
    const double* m = means + 2 * i;
    const double* c = covariances + 4 * i;
    NDT_REQUIRE(std::isfinite(m[0]) && std::isfinite(m[1]) && std::isfinite(c[0]) && std::isfinite(c[1]) && std::isfinite(c[2]) &&
                    std::isfinite(c[3]),
                "mcl_set_ndt_map: cell " + std::to_string(i) + " has a value that is not finite");
    NDT_REQUIRE(std::abs(c[1] - c[2]) <= 1e-12 * std::max(std::abs(c[1]), std::abs(c[2])),
                "mcl_set_ndt_map: the covariance of cell " + std::to_string(i) + " is not symmetric");
  }
  *shape = ndt_grid_shape(ndt_reach(prm), x0, x1, y0, y1);
  return MCL_OK;
}

}  // namespace

mcl_status ndt_layout_map(const int32_t* cells, const double* means, const double* covariances, uint64_t n, double resolution,
                          const mcl_ndt_params* params, NdtMapLayout* out, std::string* error) {
  if (const mcl_status s = ndt_check_map(cells, means, covariances, n, resolution, params, out->params, &out->shape, error)) return s;
  const NdtGridShape g = out->shape;
  if (!g.fits) {
    if (error)
      *error = "mcl_set_ndt_map: the bounding box of the keys exceeds 2^26 cells (" + std::to_string(g.gw) + " x " + std::to_string(g.gh) +
               " with its border)";
    return MCL_ERR_UNSUPPORTED;
  }
  out->grid.assign(static_cast<size_t>(g.gw * g.gh), -1);
  out->records.resize(static_cast<size_t>(n) * kNdtRecord);
  for (uint64_t i = 0; i < n; ++i) {
    const size_t at = static_cast<size_t>((cells[2 * i + 1] - g.grid_y0) * g.gw + (cells[2 * i] - g.grid_x0));
    NDT_REQUIRE(out->grid[at] < 0, "mcl_set_ndt_map: duplicate key (" + std::to_string(cells[2 * i]) + ", " + std::to_string(cells[2 * i + 1]) + ")");
    out->grid[at] = static_cast<int32_t>(i);
    ndt_pack_record(means + 2 * i, covariances + 4 * i, out->records.data() + i * kNdtRecord);
  }
  return MCL_OK;
}

bool ndt_keys_fit_grid(const int32_t* cells, uint64_t n, const mcl_ndt_params* params) {
  mcl_ndt_params prm;
  if (params) prm = *params;
  else mcl_default_ndt_params(&prm);
  if (!cells || n == 0 || n >= (1ull << 31) || prm.num_offsets < 1 || prm.num_offsets > MCL_NDT_MAX_OFFSETS) return true;
  int64_t x0 = INT64_MAX, y0 = INT64_MAX, x1 = INT64_MIN, y1 = INT64_MIN;
  for (uint64_t i = 0; i < n; ++i) {
    x0 = std::min<int64_t>(x0, cells[2 * i]);
    x1 = std::max<int64_t>(x1, cells[2 * i]);
    y0 = std::min<int64_t>(y0, cells[2 * i + 1]);
    y1 = std::max<int64_t>(y1, cells[2 * i + 1]);
  }
  // (an offset beyond 64 cells is refused later; here it only widens the border)
  return ndt_grid_shape(ndt_reach(prm), x0, x1, y0, y1).fits;
}

mcl_status ndt_layout_map_hashed(const int32_t* cells, const double* means, const double* covariances, uint64_t n, double resolution,
                                 const mcl_ndt_params* params, NdtHashLayout* out, std::string* error) {
  if (const mcl_status s = ndt_check_map(cells, means, covariances, n, resolution, params, out->params, &out->shape, error)) return s;
  out->log2_capacity = ndt_hash_log2_capacity(n);
  out->longest_probe = 1;
  out->slots.assign(size_t{1} << out->log2_capacity, NdtSlot{~uint64_t{0}, kNdtNoRecord, kNdtNoRecord});
  out->records.resize(static_cast<size_t>(n) * kNdtRecord);
  const uint32_t mask = static_cast<uint32_t>(out->slots.size() - 1), shift = 64 - out->log2_capacity;
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t key = ndt_pack_key(cells[2 * i], cells[2 * i + 1]);
    uint32_t at = ndt_hash_home(key, shift), probe = 1;
    for (; out->slots[at & mask].record >= 0; ++at, ++probe)  // (ends: the load is at most 1/2)
      NDT_REQUIRE(out->slots[at & mask].key != key,
                  "mcl_set_ndt_map: duplicate key (" + std::to_string(cells[2 * i]) + ", " + std::to_string(cells[2 * i + 1]) + ")");
    out->slots[at & mask] = NdtSlot{key, static_cast<int32_t>(i), 0};
    out->longest_probe = std::max(out->longest_probe, probe);
    ndt_pack_record(means + 2 * i, covariances + 4 * i, out->records.data() + i * kNdtRecord);
  }
  return MCL_OK;
}

}  // namespace mcl

extern "C" {

void mcl_default_ndt_params(mcl_ndt_params* params) {
  if (!params) return;
  std::memset(params, 0, sizeof(*params));
  params->minimum_likelihood = 0.0;  // NDTModelParam (ndt_sensor_model.hpp:153-166)
  params->d1 = 1.0;
  params->d2 = 1.0;
  static const int32_t kernel[9][2] = {{-1, -1}, {-1, 0}, {-1, 1}, {0, -1}, {0, 0}, {0, 1}, {1, -1}, {1, 0}, {1, 1}};  // :113-123
  params->num_offsets = 9;
  for (int k = 0; k < 9; ++k) {
    params->offsets[2 * k] = kernel[k][0];
    params->offsets[2 * k + 1] = kernel[k][1];
  }
}

mcl_status mcl_ndt_measurement_cells(const double* points_xy, uint64_t num_points, double resolution, double* means_out, double* covs_out,
                                     uint64_t* num_cells) {
  if (!num_cells || (num_points && !points_xy) || !(std::isfinite(resolution) && resolution > 0.0)) return MCL_ERR_INVALID_ARGUMENT;
  if (num_points >= 5 && (!means_out || !covs_out)) return MCL_ERR_INVALID_ARGUMENT;
  std::vector<double> recs;
  mcl::ndt_fit_cells(points_xy, num_points, resolution, recs);
  const uint64_t k = recs.size() / mcl::kNdtRecord;
  for (uint64_t j = 0; j < k; ++j) mcl::ndt_unpack_record(recs.data() + j * mcl::kNdtRecord, means_out + 2 * j, covs_out + 4 * j);
  *num_cells = k;
  return MCL_OK;
}

}  // extern "C"
