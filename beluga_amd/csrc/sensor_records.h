// sensor_records.h — the sizes of the records that the host packs (ndt_host.cpp, landmark_host.cpp) and the kernels read
// (ndt_kernels.hip, ndt_build_kernels.hip, landmark_kernels.hip).  Their layouts are described in kernels.h.
#pragma once

namespace mcl {

constexpr int kNdtRecord = 6;        // doubles per NDT cell record: mean x, y, covariance xx, xy, yy, 0
constexpr int kLandmarkRecord = 10;  // doubles per detection record of the landmark and bearing models

}  // namespace mcl
