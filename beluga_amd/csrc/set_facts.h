// What the host remembers about the live particle set between launches, and the only places where it changes.  Kernels are chosen
// from these facts, so a stale one is silently wrong weights, not an error: every write is one of the events below.  Plain C++17.
//
//   unit      every weight of the live set is exactly 1.0 (particle_traits.hpp:105): the LF patch and far-beams kernels skip the old weight
//   lf sums   workgroup sums of the new weights that the last LF launch left: the normalisation behind it builds its factor on them
//   divides   the last normalisation left the weights undivided: the CDF kernel behind it divides
//   order     the spatial order of the set as the propagation of (step, n, layout) will leave it, computed a cycle ahead; `accepted`
//             once this cycle's propagation found it usable: the reweight then skips the ordering passes
//   normals   the propagation normals of (step, seed) for the global indices [offset, offset + n), drawn a cycle ahead; they depend on
//             nothing else, so any set of that size at that step may use them
//   pivot     the point the estimate sums of the live set are taken about (dx = x - pivot): it has to lie within the set, or the
//             covariance loses (distance / spread)^2 of its digits.  Known from whoever installed the set (the mean it drew about, the
//             first state it copied) or from the set's last finite estimate; void once another set has replaced it
//   field poses  the buffer of field-frame poses (FieldPoseOut, kernels.h) holds world_to_field * pose of every particle of the live set,
//             for the map frame of generation G (the context counts the maps it has been given): the likelihood-field kernels load them
//             instead of forming the product (option lf_pose_ahead).  Void behind anything that writes poses without them
//
//   event                              unit            lf sums    divides    order       normals
//   set_changes                        .               void       .          void        .
//   pivot_given(x, y)                  .               .          .          .           .             (pivot: = (x, y) if finite)
//   estimate_reported(c, s, x, y)      .               .          .          .           .             (pivot: = (x, y) if finite, heading (c, s))
//   pivot_carried(dc, ds, tx, ty)      .               .          .          .           .             (pivot: moved by the control action if its heading is known)
//   set_replaced(unit[, keep_pivot])   = unit          void       .          void        .             (pivot: void unless kept)
//   set_resized(grew)                  false if grew   void       .          void        .
//   weights_rewrite_begins             false           .          .          .           .
//   weights_touched                    false           .          .          .           .
//   take_unit_weights                  read, false     .          .          .           .
//   lf_sums_left(count)                .               = count    .          .           .
//   lf_sums_dropped                    .               void       .          .           .
//   weights_left_undivided(yes)        .               .          = yes      .           .
//   take_cdf_divides                   .               .          read, no   .           .
//   resampled_set_committed            true            .          .          .           .
//   commit_rolled_back                 false           .          .          .           .
//   order_ahead_recorded(s, n, l)      .               .          .          = (s, n, l) .
//   take_order_ahead(s, n, l)          .               .          .          read, void  .
//   order_accepted(yes) / take_...     .               .          .          accepted    .
//   noise_ahead_recorded(s, n, o, sd)  .               .          .          .           = (s, n, o, sd)
//
//   event                              field poses
//   field_poses_written(G)             = G            (a propagation that stored them beside the poses; k_field_pose)
//   poses_moved                        void           (a propagation that stored none)
//   set_changes, set_replaced, set_resized, resampled_set_committed, commit_rolled_back
//                                      void           (an initialisation, mcl_set_particles, a loaded shard, a resampling or an exchange
//                                                      and its roll-back: none of their kernels writes the buffer)
//   field_poses_current(G)             read           (false for any other generation: mcl_set_map, the swap of a map built ahead,
//                                                      mcl_use_shared_map and mcl_set_likelihood_field each begin a new one)
//
// set_changes comes first in every entry point that replaces or resizes the set, ahead of its argument checks: a call that fails has
// still voided what described the old set.  A rewrite that begins and fails leaves unit false; one that succeeds ends in
// set_replaced(true).  lf_sums_dropped is both the normalisation consuming the sums and anything that makes them stale (a failed
// launch, a resampling that begins, the small tail).  `unit_weights()` is read by nothing but tests: the reweight takes it.
// set_replaced voids the pivot; the entry point gives the new one behind it (pivot_given, through install_set).  set_changes alone
// and set_resized keep it: a call that fails leaves the old set live, and a resized set still holds the particles the pivot lay among.  A resampling
// does not void it: the new set is drawn from the old one's particles.  An estimate that is not finite leaves the pivot as it was.
#pragma once

#include <cstdint>

namespace mcl {

class SetFacts {
 public:
  struct OrderTaken { bool recorded, matched; };

  bool unit_weights() const { return unit_; }
  uint32_t lf_sums() const { return lf_sums_; }
  uint64_t noise_ahead_count() const { return noise_n_; }
  // Do the normals drawn ahead serve the first n particles of a set at (step, seed, offset)?
  bool noise_ahead_serves(uint32_t step, uint64_t n, uint64_t seed, uint64_t offset) const {
    return noise_n_ >= n && noise_step_ == step && noise_seed_ == seed && noise_offset_ == offset;
  }

  bool field_poses_current(uint64_t generation) const { return field_poses_ && field_generation_ == generation; }

  bool pivot_known() const { return pivot_known_; }
  bool pivot_heading_known() const { return pivot_known_ && heading_known_; }
  const double* pivot() const { return pivot_; }  // (0, 0) while void

  void set_changes() { lf_sums_ = 0; order_recorded_ = false; field_poses_ = false; }
  void pivot_given(double x, double y) {
    if (!(x - x == 0.0 && y - y == 0.0)) return;  // (neither NaN nor infinite)
    pivot_known_ = true; heading_known_ = false; pivot_[0] = x; pivot_[1] = y;
  }
  // (c, s): the heading of the estimate, a unit complex number; one that is not finite leaves the position alone known
  void estimate_reported(double c, double s, double x, double y) {
    if (!(x - x == 0.0 && y - y == 0.0)) return;
    pivot_given(x, y);
    if (c - c == 0.0 && s - s == 0.0) { heading_known_ = true; heading_[0] = c; heading_[1] = s; }
  }
  // The control action (dc, ds, tx, ty) = previous^-1 * current, as the propagation applies it to every particle: the pivot goes where
  // a particle at the last estimate goes, noise apart.  Without a heading (a pivot that was given, not estimated) it stays.
  void pivot_carried(double dc, double ds, double tx, double ty) {
    if (!pivot_heading_known() || !(dc - dc == 0.0 && ds - ds == 0.0 && tx - tx == 0.0 && ty - ty == 0.0)) return;
    const double c = heading_[0], s = heading_[1];
    pivot_[0] += c * tx - s * ty;
    pivot_[1] += s * tx + c * ty;
    heading_[0] = c * dc - s * ds;
    heading_[1] = s * dc + c * ds;
  }
  // keep_pivot: a shard of a sharded filter - every rank sums about the same point and none knows the others' states, so the pivot
  // stays what the ranks' last collective estimate made it (finish_sums' second pass, context.hip, moves it into the set).
  void set_replaced(bool unit, bool keep_pivot = false) {
    set_changes(); unit_ = unit;
    if (!keep_pivot) { pivot_known_ = heading_known_ = false; pivot_[0] = pivot_[1] = 0.0; }
  }
  void set_resized(bool grew) { set_changes(); if (grew) unit_ = false; }  // (what lies beyond the old set is whatever was there)
  void weights_rewrite_begins() { unit_ = false; }
  void weights_touched() { unit_ = false; }
  bool take_unit_weights() { const bool was = unit_; unit_ = false; return was; }
  void lf_sums_left(uint32_t count) { lf_sums_ = count; }
  void lf_sums_dropped() { lf_sums_ = 0; }
  void weights_left_undivided(bool yes) { divides_ = yes; }
  bool take_cdf_divides() { const bool was = divides_; divides_ = false; return was; }
  void resampled_set_committed() { unit_ = true; field_poses_ = false; }  // (every output slot took a weight of 1.0)
  void commit_rolled_back() { unit_ = false; field_poses_ = false; }      // (the old set is live again: its weights are normalised)
  void field_poses_written(uint64_t generation) { field_poses_ = true; field_generation_ = generation; }
  void poses_moved() { field_poses_ = false; }
  void order_ahead_recorded(uint32_t step, uint64_t n, uint32_t layout) {
    order_recorded_ = true; order_step_ = step; order_n_ = n; order_layout_ = layout;
  }
  // Consumes the record: whether there was one, and whether it was computed for this (step, n, layout).
  OrderTaken take_order_ahead(uint32_t step, uint64_t n, uint32_t layout) {
    const bool recorded = order_recorded_;
    order_recorded_ = false;
    return OrderTaken{recorded, recorded && order_step_ == step && order_n_ == n && order_layout_ == layout};
  }
  void order_accepted(bool yes) { order_accepted_ = yes; }
  bool take_order_accepted() { const bool was = order_accepted_; order_accepted_ = false; return was; }
  void noise_ahead_recorded(uint32_t step, uint64_t n, uint64_t offset, uint64_t seed) {
    noise_step_ = step; noise_n_ = n; noise_offset_ = offset; noise_seed_ = seed;
  }

 private:
  bool unit_{false}, divides_{false}, order_recorded_{false}, order_accepted_{false};
  uint32_t lf_sums_{0}, order_step_{0}, order_layout_{0}, noise_step_{0};
  uint64_t order_n_{0}, noise_n_{0}, noise_offset_{0}, noise_seed_{0};
  bool field_poses_{false};
  uint64_t field_generation_{0};
  bool pivot_known_{false}, heading_known_{false};
  double pivot_[2]{0.0, 0.0}, heading_[2]{1.0, 0.0};
};

}  // namespace mcl
