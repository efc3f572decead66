// scan_host.h — the one rule about a scan's points that every call which stages them for a likelihood-field kernel shares (scan_host.cpp).
#pragma once
#include <cstdint>

namespace mcl {
// The points of a scan whose two coordinates are both finite, in the caller's order, into kept_xy (room for num_points points; not the
// scan's own memory); returns how many.  A point with a NaN or infinite coordinate has no cell for any pose and is left out; finite
// coordinates whose |x| + |y| overflows stay.  slots, if given: per kept point the caller's index of it.
uint64_t scan_finite_points(const double* points_xy, uint64_t num_points, double* kept_xy, uint32_t* slots = nullptr);
}  // namespace mcl
