// options_host.h — the per-context switches (Tuning, cycle_types.h) by name: one table with a row per option - its name, its member and the
// rule that brings a caller's value into the member's range - that mcl_set_option and mcl_create's BELUGA_MCL_* defaults both read.
// Plain C++17, no HIP.
#pragma once

#include <cstddef>
#include <cstdint>
#include <functional>

#include "cycle_types.h"

namespace mcl {

// The option names, in the table's order (the recorded rows: an option added since - lf_pose_ahead - is set by name through set_tuning
// and is neither listed here nor read from the environment; options_host.cpp says why).
const char* const* tuning_names(size_t* count);

// The option `name` takes `value`, normalised by its rule; false (and nothing changes) for a name that is no option.
bool set_tuning(Tuning& t, const char* name, int64_t value);

// Every option whose variable BELUGA_MCL_<NAME IN UPPER CASE> is set (lookup: getenv-like, nullptr = unset) takes its value: atoi of the
// text, and for lf_table the spelling "cube" as 1.
void tuning_from_environment(Tuning& t, const std::function<const char*(const char*)>& lookup);

}  // namespace mcl
