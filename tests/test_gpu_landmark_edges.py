"""What the landmark and bearing reweight kernels (beluga_amd/csrc/landmark_kernels.hip) are held to: every form - a lane per particle, a
wave per particle, a fleet's shared launch - on every case of every family of tests/landmark_families.py (near ties of the match under
three kinds of pose at two scales, baits at both ends of every category range, degenerate vectors, weights down to the denormals and
below, UTM-scale maps) against landmark_reference.weights_exact: the match by the reference's own f64 sequence, everything behind it in
60-digit arithmetic.  The lane forms meet every state of a case at their largest size (a case has at most 64 states), the wave forms by
walking the states with their sizes in turn.  Each launch is pinned by the counters landmark_lane_launches / landmark_wave_launches:
a silent re-route fails the test.  Slots past n keep their weights.

The tolerance, per family, relative: 4 MEASURED_F64_ERROR[family] + (k + 4) 2^-53 (and, for tiny_weights, (k + 2) denormal steps
absolute; beside it, every form and launch returns +0 wherever the exact weight is below 2^-1075).  MEASURED_F64_ERROR is the error of the f64 loop form (the kernels' operations in the kernels' order with libm's exp, atan2
and sqrt) against the exact value, measured on the CPU (test_landmark_reference_cpu.py) - what f64 costs on these inputs, range_error's
cancellation and the size of the exponents included.  The margin of 4: the device's exp, atan2 and sqrt and libm's each err by about
an ulp, of which the loop form's figure holds one sample.  (k + 4) 2^-53: the product of k terms and the prior weight.  Nothing here
was fitted to what a device returned.

Bit equality where the project claims it: wave = lane on every state, a fleet member = its lone twin.

What is not observable: in the bearing model equal dot products with the detection mean equal apertures, so WHICH of two tied landmarks
is matched never shows in a weight; the bearing cases are required to give the exact value, and there is no pick test for them.

The RULE families (overflowing and underflowing squares, poses that are not finite) are held to the f64 sequence itself, class by class
(NaN where it is NaN, no negative zero) and value by value within landmark_families.rule_bound.  No index leaves its buffer there, for
any pose: a record's range (first, count) comes from the host and does not depend on the particle; the lane kernels index first + t with
t < count only; the wave kernels take an index only from a lane that scanned (t < count) - pick_beats settles a lane without a candidate
before it looks at a value, and a record with count > 0 always has lane 0 of its group scanning - so a NaN or an infinity can change
WHICH index of the range is kept, never make one; the bearing kernels' slots are place (a permutation of 0 .. k-1) and the lane.
"""
import mpmath
import numpy as np
import pytest

import landmark_families as fam
import landmark_reference as ref
from beluga_amd.amcl import (Amcl, AmclBatch, AmclParams, BearingModelParam, DifferentialDriveModelParam, LandmarkMap, LandmarkModelParam,
                             se2_from_xytheta)

pytestmark = pytest.mark.gpu

MOTION = DifferentialDriveModelParam(0.1, 0.05, 0.1, 0.05)
COUNTERS = ("landmark_lane_launches", "landmark_wave_launches")
PAST = 8  # slots kept behind n
LANE_SIZES = {False: (1, 63, 64, 65, 255, 256, 257), True: (1, 63, 64, 65)}  # the landmark kernel's block is 256, the bearing kernel's one wave
WAVE_SIZES = (1, 3, 4, 5)
BELOW_DENORMALS = mpmath.mpf(2) ** -1075  # half the smallest denormal: an exact weight below it rounds to 0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    """Bit for bit; a NaN stands for any NaN (the payload is not part of the contract)."""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(bits(a[~nan]), bits(b[~nan]))


def sensor(case):
    if case.bearing:
        return BearingModelParam(case.params["sigma_bearing"], tuple(case.params["sensor_pose_in_robot"]))
    return LandmarkModelParam(case.params["sigma_range"], case.params["sigma_bearing"], case.params["random_prob"])


def launches(case, wave):
    """(n, first state) of every launch of a form on a case: the lane form at each of its sizes, the wave form's sizes walked over the
    case's states until every state has been through one of them."""
    if not wave:
        return [(n, 0) for n in LANE_SIZES[case.bearing]]
    out, first = [(n, 0) for n in WAVE_SIZES], 0
    while first < len(case.states):
        for n in WAVE_SIZES:
            out.append((n, first))
            first += n
    return out


def states_of(case, n, first):
    return (first + np.arange(n)) % len(case.states)


def run_forms(case):
    """{"lane" | "wave": {(n, first): weights}}: one filter, the switch off and on; checks the counters and the slots past n."""
    cap = max(LANE_SIZES[case.bearing]) + PAST
    f = Amcl(LandmarkMap((case.positions, case.categories)), MOTION, sensor(case), AmclParams(min_particles=cap, max_particles=cap), seed=11)
    out = {}
    for wave in (False, True):
        f.set_landmark_small_cycle(wave)
        moved = COUNTERS[int(wave)]
        out["wave" if wave else "lane"] = by_launch = {}
        for n, first in launches(case, wave):
            pick = (first + np.arange(cap)) % len(case.states)
            states, w0 = case.states[pick], case.w0[pick]
            f.set_particles(states, w0)
            f.set_num_particles(n)
            before = {c: f.counter(c) for c in COUNTERS}
            (f.reweight_bearings if case.bearing else f.reweight_landmarks)((case.det, case.dcat))
            delta = {c: f.counter(c) - before[c] for c in COUNTERS}
            assert delta == {c: int(c == moved) for c in COUNTERS}, (case.tag, wave, n, delta)
            f.set_num_particles(cap)
            got = f.particles()[1]
            assert np.array_equal(bits(got[n:]), bits(w0[n:])), "weights past n were written"
            by_launch[(n, first)] = got[:n]
    f.close()
    return out


def check_wave_is_lane(case, results):
    assert len(case.states) <= 64
    lane = results["lane"][(max(LANE_SIZES[case.bearing]), 0)]
    for (n, first), got in results["lane"].items():
        assert same_bits(got, lane[:n]), (case.tag, "lane", n)
    for (n, first), got in results["wave"].items():
        assert same_bits(got, lane[states_of(case, n, first)]), (case.tag, "wave", n, first)


_exact = {}


def exact(name, number, case):
    if (name, number) not in _exact:
        _exact[(name, number)] = case.exact()[0]
    return _exact[(name, number)]


@pytest.mark.parametrize("name", sorted(fam.FAMILIES))
def test_every_form_returns_the_exact_weights(name):
    zeros = 0
    for number, case in enumerate(fam.FAMILIES[name]()):
        want_all = exact(name, number, case)
        bound = 4 * fam.MEASURED_F64_ERROR[name] + (case.k + 4) * 2.0**-53
        results = run_forms(case)
        worst = 0.0
        for form, by_launch in results.items():
            for (n, first), got in by_launch.items():
                assert not np.isnan(got).any() and not np.signbit(got).any(), (case.tag, form, n, first)
                at = states_of(case, n, first)
                if name == "tiny_weights":  # an exact weight below half a denormal step is +0 (the sign is checked above), beside the tolerance
                    below = np.array([want_all[i] < BELOW_DENORMALS for i in at])
                    assert np.all(got[below] == 0.0), (case.tag, form, n, first, got[below].max())
                    zeros += int(below.sum())
                err = float(ref.excess_errors(got, [want_all[i] for i in at], case.absolute_steps()).max())
                worst = max(worst, err)
                assert err <= bound, (case.tag, form, n, first, err, bound)
        print("landmark_edges %s k=%d worst=%.3g (%.2f of the bound)" % (case.tag, case.k, worst, worst / bound))
        check_wave_is_lane(case, results)
    assert zeros > 0 or name != "tiny_weights"  # (weights below the denormals were met: test_landmark_reference_cpu.py counts them per case)


@pytest.mark.parametrize("name", sorted(fam.RULE_FAMILIES))
def test_rule_families_follow_the_f64_sequence(name):
    """Overflowing and underflowing squares, poses that are not finite: the class of every weight (NaN / finite) is the f64 sequence's, no
    weight is a negative zero, every finite weight stands within landmark_families.rule_bound of it, and every form returns the same."""
    for case in fam.RULE_FAMILIES[name]():
        want, _, exponents = case.loop()
        bound = fam.rule_bound(case, exponents)
        results = run_forms(case)
        check_wave_is_lane(case, results)
        worst = 0.0
        for form, by_launch in results.items():
            for (n, first), got in by_launch.items():
                at = states_of(case, n, first)
                w, b = want[at], bound[at]
                assert np.array_equal(np.isnan(got), np.isnan(w)), (case.tag, form, n, first)
                fin = ~np.isnan(w)
                assert np.all(np.isfinite(got[fin])) and not np.signbit(got[fin]).any(), (case.tag, form, n, first)
                assert np.array_equal(got[fin] == 0.0, w[fin] == 0.0)
                live = fin & (w != 0.0)
                share = np.max(np.abs(got[live] - w[live]) / w[live] / b[live], initial=0.0)
                worst = max(worst, float(share))
                assert share <= 1.0, (case.tag, form, n, first, share)
        print("landmark_edges %s k=%d worst %.2f of the bound" % (case.tag, case.k, worst))


def test_a_fleet_member_equals_its_lone_twin_and_the_exact_weights():
    """Three members on the fleet's shared launch (k_batch_reweight_landmarks): a landmark member, a bearing member and a landmark member
    without detections (it takes no block of the launch).  Each member's states, weights and estimate are its lone twin's bit for bit,
    the twins' own launches are the wave kernels', and the weights are the exact ones of the propagated states, normalised - within the
    reweight's tolerance plus the normalisation's (2 (n - 1) + 1) 2^-53.  No resampling in the cycle.

    The shared launch propagates before it reweights, so it meets none of the engineered (state, detection) pairs; what ties it to the
    edges is that its body IS the wave kernels' (reweight_landmarks_wave_block / reweight_bearings_wave_block), held on every pair
    above, and the bit equality with the twin here."""
    lcase, bcase = fam.far_maps()
    members = [(lcase, True), (bcase, True), (lcase, False)]
    params = AmclParams(min_particles=5, max_particles=5, resample_interval=1000)
    spec = lambda case, k: dict(grid=LandmarkMap((case.positions, case.categories)), motion=MOTION, sensor=sensor(case), params=params, seed=5 + k,
                                landmark_small_cycle=True)
    batch = AmclBatch([spec(case, k) for k, (case, _) in enumerate(members)])
    twins = [Amcl(**spec(case, k)) for k, (case, _) in enumerate(members)]
    for k, (case, _) in enumerate(members):
        for f in (batch.members[k], twins[k]):
            f.set_particles(case.states[3:8], case.w0[3:8])
    control = se2_from_xytheta(0.0, 0.0, 0.0)
    dets = [(case.det, case.dcat) if has else (np.zeros((0, 3)), np.zeros(0, dtype=np.uint32)) for case, has in members]
    before = [{c: t.counter(c) for c in COUNTERS} for t in twins]
    shared = batch.counter("landmark_launches")
    got = batch.update_detections([control] * 3, dets)
    assert batch.counter("landmark_launches") == shared + 1
    for k, (case, has) in enumerate(members):
        want = twins[k].update(control, dets[k])
        assert np.array_equal(got[k][0], want[0]) and np.array_equal(got[k][1], want[1], equal_nan=True)
        (ms, mw), (ts, tw) = batch.members[k].particles(), twins[k].particles()
        assert np.array_equal(bits(ms), bits(ts)) and np.array_equal(bits(mw), bits(tw))
        delta = {c: twins[k].counter(c) - before[k][c] for c in COUNTERS}
        assert delta == {"landmark_lane_launches": 0, "landmark_wave_launches": int(has)}, (k, delta)
        assert batch.members[k].counter("landmark_wave_launches") == int(has)
        det, dcat = dets[k]
        exact_w = ref.weights_exact(case.ref_map(), ts, det, dcat, case.w0[3:8], case.bearing, **case.params)[0]
        total = sum(exact_w)
        bound = 4 * fam.MEASURED_F64_ERROR["far_maps"] + ((len(det) + 4) + 2 * (len(tw) - 1) + 1) * 2.0**-53
        assert ref.excess_errors(tw, [w / total for w in exact_w]).max() <= bound, k
    batch.close()
    for t in twins:
        t.close()
