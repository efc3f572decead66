// options_host.cpp — the table of the per-context switches (options_host.h).  Plain C++17, no HIP.
#include "options_host.h"

#include <cctype>
#include <cstdlib>
#include <cstring>
#include <string>

namespace mcl {

namespace {

enum class Rule : int {
  kFlag,       // 0 / 1
  kTristate,   // -1 / 0 / 1
  kClamp,      // [lo, hi]
  kLowBits,    // value & 3
  kLfVariant,  // 0, 1, 3 name their kernel family; everything else the default one
  kLfPatch,    // 0 .. 2, everything else 1
  kKeyBits     // 4 .. 6, everything else 0
};

struct Option {
  const char* name;
  int Tuning::*member;
  Rule rule;
  int64_t lo, hi;  // kClamp
};

constexpr Option kOptions[] = {
    {"lf_variant", &Tuning::lf_variant, Rule::kLfVariant, 0, 0},
    {"lf_fast", &Tuning::lf_fast, Rule::kTristate, 0, 0},
    {"lf_table", &Tuning::lf_table, Rule::kFlag, 0, 0},
    {"lf_patch", &Tuning::lf_patch, Rule::kLfPatch, 0, 0},
    {"lf_dispersed", &Tuning::lf_dispersed, Rule::kClamp, 0, 2},
    {"lf_far_tiles", &Tuning::lf_far_tiles, Rule::kClamp, 0, 2},
    {"key_layout", &Tuning::key_layout, Rule::kTristate, 0, 0},
    {"lf_loose_below", &Tuning::lf_loose_below, Rule::kClamp, 0, 257},
    {"lf_small_particles", &Tuning::lf_small_particles, Rule::kClamp, 0, INT32_MAX},
    {"device_policy", &Tuning::device_policy, Rule::kFlag, 0, 0},
    {"sort_min_particles", &Tuning::sort_min_particles, Rule::kClamp, 0, 1ll << 30},
    {"beam_sort_min_particles", &Tuning::beam_sort_min_particles, Rule::kClamp, 0, 1ll << 30},
    {"field_build", &Tuning::field_build, Rule::kFlag, 0, 0},
    {"key_curve", &Tuning::key_curve, Rule::kFlag, 0, 0},
    {"key_warp", &Tuning::key_warp, Rule::kFlag, 0, 0},
    {"key_bits_xy", &Tuning::key_bits_xy, Rule::kKeyBits, 0, 0},
    {"lf_margin", &Tuning::lf_margin, Rule::kFlag, 0, 0},
    {"lf_split", &Tuning::lf_split, Rule::kLowBits, 0, 0},  // 1: side by side only, 2: stacked only, 3: both
    {"lf_queue_grid", &Tuning::lf_queue_grid, Rule::kClamp, 0, 1 << 20},
    {"shard_pad_permille", &Tuning::shard_pad_permille, Rule::kClamp, 0, 8000},
    {"lf_queue", &Tuning::lf_queue, Rule::kFlag, 0, 0},
    {"lf_ends_first", &Tuning::lf_ends_first, Rule::kFlag, 0, 0},
    {"beam_free_ahead", &Tuning::beam_free_ahead, Rule::kFlag, 0, 0},
    {"beam_sectors", &Tuning::beam_sectors, Rule::kFlag, 0, 0},
    {"lf_weight_sums", &Tuning::lf_weight_sums, Rule::kFlag, 0, 0},
    {"beam_table", &Tuning::beam_table, Rule::kFlag, 0, 0},
    {"cycle_spin", &Tuning::cycle_spin, Rule::kTristate, 0, 0},
    {"scan_fused", &Tuning::scan_fused, Rule::kClamp, 0, 2},
    {"draw_fold", &Tuning::draw_fold, Rule::kClamp, 0, 2},
    {"lf_unit_weights", &Tuning::lf_unit_weights, Rule::kFlag, 0, 0},
    {"small_fused", &Tuning::small_fused, Rule::kFlag, 0, 0},
    {"norm_store", &Tuning::norm_store, Rule::kFlag, 0, 0},
    {"noise_ahead", &Tuning::noise_ahead, Rule::kClamp, 0, 2},
    {"order_ahead", &Tuning::order_ahead, Rule::kFlag, 0, 0},
    {"lf_far_beams_per_wave", &Tuning::lf_far_beams_per_wave, Rule::kClamp, 0, 4096},
    {"batch_cluster_fused", &Tuning::batch_cluster_fused, Rule::kFlag, 0, 0},
    {"batch_beam_fused", &Tuning::batch_beam_fused, Rule::kFlag, 0, 0},
    {"draw_key_hist", &Tuning::draw_key_hist, Rule::kFlag, 0, 0},
    {"rows_merged", &Tuning::rows_merged, Rule::kFlag, 0, 0},
};
constexpr size_t kOptionCount = sizeof(kOptions) / sizeof(kOptions[0]);
// Options added since the rows above were recorded.  tests/test_options_host_cpu.py pins those rows - the names tuning_names lists, one
// environment look-up each - against the record of what they stored before the table existed; a row here is read by set_tuning
// (mcl_set_option) alone: it is no part of that list and has no BELUGA_MCL_* variable.
constexpr Option kLaterOptions[] = {
    {"lf_pose_ahead", &Tuning::lf_pose_ahead, Rule::kFlag, 0, 0},
    {"search_chunk", &Tuning::search_chunk, Rule::kClamp, 64, 1ll << 22},
    {"cast_chunk", &Tuning::cast_chunk, Rule::kClamp, 64, 1ll << 28},
    {"range_table_launch", &Tuning::range_table_launch, Rule::kClamp, 256, 1ll << 30},
};

int normalised(const Option& o, int64_t value) {
  switch (o.rule) {
    case Rule::kFlag: return value ? 1 : 0;
    case Rule::kTristate: return value < 0 ? -1 : (value ? 1 : 0);
    case Rule::kClamp: return static_cast<int>(std::clamp<int64_t>(value, o.lo, o.hi));
    case Rule::kLowBits: return static_cast<int>(value & 3);
    case Rule::kLfVariant: return value == 0 ? kLfWavePerParticle : (value == 1 ? kLfLanePerParticle : (value == 3 ? kLfBeamLanes : kLfSortedLanes));
    case Rule::kLfPatch: return value < 0 || value > 2 ? 1 : static_cast<int>(value);
    case Rule::kKeyBits: return (value >= 4 && value <= 6) ? static_cast<int>(value) : 0;
  }
  return 0;
}

}  // namespace

const char* const* tuning_names(size_t* count) {
  static const char* names[kOptionCount];
  static const bool filled = [] {
    for (size_t i = 0; i < kOptionCount; ++i) names[i] = kOptions[i].name;
    return true;
  }();
  (void)filled;
  *count = kOptionCount;
  return names;
}

bool set_tuning(Tuning& t, const char* name, int64_t value) {
  for (const Option& o : kOptions) {
    if (std::strcmp(o.name, name) != 0) continue;
    t.*o.member = normalised(o, value);
    return true;
  }
  for (const Option& o : kLaterOptions) {
    if (std::strcmp(o.name, name) != 0) continue;
    t.*o.member = normalised(o, value);
    return true;
  }
  if (std::strcmp(name, "range_table_max_bytes") == 0) {  // (a byte count: the one value an int does not hold)
    t.range_table_max_bytes = std::clamp<int64_t>(value, 0, 1ll << 62);
    return true;
  }
  return false;
}

void tuning_from_environment(Tuning& t, const std::function<const char*(const char*)>& lookup) {
  for (const Option& o : kOptions) {
    std::string env = "BELUGA_MCL_";
    for (const char* c = o.name; *c; ++c) env += static_cast<char>(std::toupper(static_cast<unsigned char>(*c)));
    const char* v = lookup(env.c_str());
    if (!v) continue;
    const bool cube = std::strcmp(o.name, "lf_table") == 0 && std::strcmp(v, "cube") == 0;
    t.*o.member = normalised(o, cube ? 1 : std::atoi(v));
  }
}

}  // namespace mcl
