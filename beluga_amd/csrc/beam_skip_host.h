// beam_skip_host.h - the host side of beam skipping (mcl_set_beam_skip, DESIGN.md "Beam skipping") that touches no device memory: the
// parameter checks, the field value a cell must exceed for an end-point to agree with a pose, and the decision over the per-beam
// counts.  context.hip calls them around its count launch.  Plain C++17, no HIP.
#pragma once

#include <cstdint>

#include "beluga_mcl.h"

namespace mcl {

// nullptr: fine; otherwise what is wrong (enabled 0 / 1; distance positive and finite; both thresholds in [0, 1]).
const char* beam_skip_check_params(const mcl_beam_skip_params& p);

// What the field builder's last expression (map_build.cpp, likelihood_field_model_base.hpp:136-146,181-182) gives for a cell whose
// squared distance to the nearest obstacle is float(distance * distance).  Parameters only, never the map.
float beam_skip_level(const mcl_lf_params& lf, double distance);

// The decision over count[b], b < B, of n live particles: kept[b] = count[b] / n > threshold; if the skipped share of the scan reaches
// error_threshold the whole scan is used after all (used_all; kept[] still says what the vote was).  kept may be nullptr.
struct BeamSkipDecision {
  uint64_t skipped;
  bool used_all;
};
BeamSkipDecision beam_skip_decide(const uint32_t* counts, uint64_t B, uint64_t n, double threshold, double error_threshold, uint8_t* kept);

}  // namespace mcl
