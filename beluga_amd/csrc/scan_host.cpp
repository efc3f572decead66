// scan_host.cpp — the entries of the C ABI (include/beluga_mcl.h) that turn a sensor message into the points of a scan and the estimate's
// sums into the estimate, and the rule about which points of a scan are staged (scan_host.h).  They take no context and use no device.  Host only: se2.h, beluga_mcl.h and the standard library, no HIP and
// no mcl_ctx, so that a plain C++ compiler can build and check it (like cluster_host.cpp and map_build.cpp).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>

#include "beluga_mcl.h"
#include "scan_host.h"
#include "se2.h"

using namespace mcl;

uint64_t mcl::scan_finite_points(const double* points_xy, uint64_t num_points, double* kept_xy, uint32_t* slots) {
  uint64_t kept = 0;
  for (uint64_t i = 0; i < num_points; ++i) {
    const double x = points_xy[2 * i], y = points_xy[2 * i + 1];
    if (!(std::isfinite(x) && std::isfinite(y))) continue;
    kept_xy[2 * kept] = x;
    kept_xy[2 * kept + 1] = y;
    if (slots) slots[kept] = static_cast<uint32_t>(i);
    ++kept;
  }
  return kept;
}

extern "C" {

mcl_status mcl_prepare_laser_scan(const mcl_laser_scan* scan, double* points_xy, uint64_t* num_points) {
  if (!scan || !num_points || (scan->num_ranges && (!scan->ranges || !points_xy))) return MCL_ERR_INVALID_ARGUMENT;
  const uint64_t n = scan->num_ranges, count = scan->max_beams;
  const double lo = std::max(static_cast<double>(scan->range_min), scan->min_range);  // laser_scan.hpp:61-62
  const double hi = std::min(static_cast<double>(scan->range_max), scan->max_range);
  const double qx = scan->origin_se3[0], qy = scan->origin_se3[1], qz = scan->origin_se3[2], qw = scan->origin_se3[3];
  const uint64_t taken = n == 0 ? 0 : std::min(n, count);  // take_evenly.hpp:47-57
  uint64_t m = 0;
  for (uint64_t k = 0; k < taken; ++k) {
    uint64_t i = k;  // take_evenly.hpp:126-148: ceil(k * (size - 1) / (count - 1))
    if (count <= n && k > 0) {
      if (count == 1) break;
      const int64_t a = static_cast<int64_t>(k) * (static_cast<int64_t>(n) - 1), b = static_cast<int64_t>(count) - 1;
      i = static_cast<uint64_t>(a / b + ((a % b == 0) ? 0 : 1));
    }
    if (i >= n) break;
    const double range = static_cast<double>(scan->ranges[i]);
    // float arithmetic first, then widened (laser_scan.hpp:73-77)
    const double theta = static_cast<double>(scan->angle_min + static_cast<float>(static_cast<int>(i)) * scan->angle_increment);
    if (std::isnan(range) || !(range >= lo) || !(range <= hi)) continue;  // sensor/data/laser_scan.hpp:79-83
    const double px = range * std::cos(theta), py = range * std::sin(theta), pz = 0.0;
    // origin * (x, y, 0): Sophus SO3 rotates with uv = 2 (q.vec x p); p + q.w uv + q.vec x uv, then adds the translation
    double ux = qy * pz - qz * py, uy = qz * px - qx * pz, uz = qx * py - qy * px;
    ux += ux;
    uy += uy;
    uz += uz;
    points_xy[2 * m] = (px + qw * ux + (qy * uz - qz * uy)) + scan->origin_se3[4];
    points_xy[2 * m + 1] = (py + qw * uy + (qz * ux - qx * uz)) + scan->origin_se3[5];
    ++m;
  }
  *num_points = m;
  return MCL_OK;
}

mcl_status mcl_project_point_cloud(const float* points_xyz, uint64_t num_points, const double origin_se3[7], double* points_xy) {
  if (!origin_se3 || (num_points && (!points_xyz || !points_xy))) return MCL_ERR_INVALID_ARGUMENT;
  const double qx = origin_se3[0], qy = origin_se3[1], qz = origin_se3[2], qw = origin_se3[3];
  for (uint64_t i = 0; i < num_points; ++i) {
    // beluga_ros/src/amcl.cpp:73-76: origin * p.cast<double>(), keep x and y.  Sophus SO3 rotates with
    // uv = 2 (q.vec x p); p + q.w uv + q.vec x uv, then adds the translation.
    const double px = static_cast<double>(points_xyz[3 * i]), py = static_cast<double>(points_xyz[3 * i + 1]),
                 pz = static_cast<double>(points_xyz[3 * i + 2]);
    double ux = qy * pz - qz * py, uy = qz * px - qx * pz, uz = qx * py - qy * px;
    ux += ux;
    uy += uy;
    uz += uz;
    points_xy[2 * i] = (px + qw * ux + (qy * uz - qz * uy)) + origin_se3[4];
    points_xy[2 * i + 1] = (py + qw * uy + (qz * ux - qx * uz)) + origin_se3[5];
  }
  return MCL_OK;
}

// algorithm/estimation.hpp:436-475 from the single-pass sufficient statistics.
mcl_status mcl_estimate_from_sums(const double sums[12], mcl_estimate* out) {
  if (!sums || !out) return MCL_ERR_INVALID_ARGUMENT;
  const double sw = sums[0], sw2 = sums[1];
  const double mc = sums[2] / sw, ms = sums[3] / sw;
  const double mdx = sums[4] / sw, mdy = sums[5] / sw;
  const double sq = sw2 / (sw * sw);  // sum of squared normalised weights
  const double corr = 1.0 - sq;       // estimation.hpp:270
  const double cxx = (sums[6] / sw - mdx * mdx) / corr;
  const double cxy = (sums[7] / sw - mdx * mdy) / corr;
  const double cyy = (sums[8] / sw - mdy * mdy) / corr;
  for (double& v : out->covariance) v = 0.0;
  out->covariance[0] = cxx;
  out->covariance[1] = cxy;
  out->covariance[3] = cxy;
  out->covariance[4] = cyy;
  out->pose[2] = sums[9] + mdx;
  out->pose[3] = sums[10] + mdy;
  const double norm = std::sqrt(mc * mc + ms * ms);
  if (norm < std::numeric_limits<double>::epsilon()) {  // estimation.hpp:460-466
    out->covariance[8] = std::numeric_limits<double>::infinity();
    const Rot2 zero = rot_exp(0.0);
    out->pose[0] = zero.c;
    out->pose[1] = zero.s;
  } else {
    out->covariance[8] = -2.0 * std::log(norm);
    const Rot2 r = rot_from_complex(mc, ms);
    out->pose[0] = r.c;
    out->pose[1] = r.s;
  }
  return MCL_OK;
}

}  // extern "C"
