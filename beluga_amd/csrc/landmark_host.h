// landmark_host.h — the host passes of the landmark and bearing sensor models: the map of mcl_set_landmark_map (parameters, the box,
// the landmarks grouped by category) and the detection records of a call.  Host only: beluga_mcl.h and the standard library, no HIP and
// no mcl_ctx, so that a plain C++ compiler can build and check it (like cluster_host.cpp and map_build.cpp).  The kernels that read
// these records are in landmark_kernels.hip; context.hip uploads what these functions return.
// Both functions return the status and leave the message of a refusal in *error.
#pragma once
#include <cstdint>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "beluga_mcl.h"
#include "sensor_records.h"

namespace mcl {

using LandmarkRanges = std::map<uint32_t, std::pair<uint32_t, uint32_t>>;  // category -> (first, count) in the grouped landmarks

// What mcl_set_landmark_map makes of its arguments on a context of sensor model `kind` (MCL_SENSOR_LANDMARK or MCL_SENSOR_BEARING;
// `params` is that model's struct, NULL for its defaults).  Everything the entry can refuse without its context is refused here, in its
// order and its words.
struct LandmarkMapLayout {
  double den_range{0.0}, den_bearing{0.0};  // (2. * sigma) * sigma
  double random_prob{0.0};
  double Rs[9]{};  // bearing model: sensor_pose_in_robot's rotation (row-major, Eigen's toRotationMatrix) and translation
  double ts[3]{};
  double lo[3], hi[3];           // the boundaries as given, or the landmarks' bounding box (LandmarkMap(landmarks), landmark_map.hpp:61-71)
  std::vector<double> landmarks;  // 4 doubles each (x, y, z, 0), grouped by category in ascending order, the map's order kept inside a
                                  // category (std::min_element returns the first of equal candidates)
  LandmarkRanges ranges;
};
mcl_status landmark_layout_map(int32_t kind, const double* positions_xyz, const uint32_t* categories, uint64_t n, const double boundaries[6],
                               const void* params, LandmarkMapLayout* out, std::string* error);

// The detection records of a call (kernels.h, kLandmarkRecord) into `out`: what does not depend on the particle - the norm, the
// normalized vector and the category's range ((0xFFFFFFFF, 0) for a category the map does not have) - is computed here, once.  The
// landmark model's records keep the caller's order; the bearing model's are sorted by category (stable), each with its place in the
// caller's order.  `ranges`: the map's, NULL where there is no map yet (MCL_ERR_NOT_READY, behind the checks of the arguments).  `who`
// is the entry the messages name.  `out` is written only when every check has passed.
mcl_status landmark_records(const char* who, int32_t kind, const double* xyz, const uint32_t* categories, uint64_t n,
                            const LandmarkRanges* ranges, std::vector<double>& out, std::string* error);

}  // namespace mcl
