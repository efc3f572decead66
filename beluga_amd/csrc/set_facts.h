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
//
//   event                              unit            lf sums    divides    order       normals
//   set_changes                        .               void       .          void        .
//   set_replaced(unit)                 = unit          void       .          void        .
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
// set_changes comes first in every entry point that replaces or resizes the set, ahead of its argument checks: a call that fails has
// still voided what described the old set.  A rewrite that begins and fails leaves unit false; one that succeeds ends in
// set_replaced(true).  lf_sums_dropped is both the normalisation consuming the sums and anything that makes them stale (a failed
// launch, a resampling that begins, the small tail).  `unit_weights()` is read by nothing but tests: the reweight takes it.
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

  void set_changes() { lf_sums_ = 0; order_recorded_ = false; }
  void set_replaced(bool unit) { set_changes(); unit_ = unit; }
  void set_resized(bool grew) { set_changes(); if (grew) unit_ = false; }  // (what lies beyond the old set is whatever was there)
  void weights_rewrite_begins() { unit_ = false; }
  void weights_touched() { unit_ = false; }
  bool take_unit_weights() { const bool was = unit_; unit_ = false; return was; }
  void lf_sums_left(uint32_t count) { lf_sums_ = count; }
  void lf_sums_dropped() { lf_sums_ = 0; }
  void weights_left_undivided(bool yes) { divides_ = yes; }
  bool take_cdf_divides() { const bool was = divides_; divides_ = false; return was; }
  void resampled_set_committed() { unit_ = true; }  // (every output slot took a weight of 1.0)
  void commit_rolled_back() { unit_ = false; }      // (the old set is live again: its weights are normalised)
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
};

}  // namespace mcl
