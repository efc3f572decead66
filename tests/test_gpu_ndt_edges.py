"""What the NDT reweight kernels' CELL CHOICE is held to: every form (lane per particle and wave per particle, dense and hashed layout, a
fleet's shared launch) on every family of tests/ndt_families.py - transformed means engineered onto cell edges under axis-aligned and
general rotations, centres around the centre box for every kernel reach, far poses, keys at the ends of int32, every count of
measurement cells the wave kernel distinguishes, condition numbers up to 1e12, singular sums - against ndt_reference.weights_exact: the
centre key by the reference's own f64 sequence, everything behind it in 60-digit arithmetic.  The maps are revealing
(ndt_reference.revealing_map): on the well-conditioned families a centre one cell off that finds other cells moves a likelihood by
more than 1e-3 of it (asserted case by case in test_ndt_reference_cpu.py), so the comparison decides the cell - but for the two `wide`
maps of far_poses and hashed_ends, whose covariances of 2^31 cells show WHETHER a cell was found (through a wrapped key, say), not
which.  The lone forms meet every state of every case: the lane forms at n = 65, the wave forms by walking the states with their
sizes in turn.  Each lone form is pinned by the counters ndt_lane_launches / ndt_wave_launches: a silent re-route fails the test.

The tolerance, per family, relative: 4 MEASURED_F64_ERROR[family] + (K + 4) 2^-53.  MEASURED_F64_ERROR is the error of the f64 loop form
(the kernel's operations in the kernel's order, with libm's exp) against the exact value, measured on the CPU
(test_ndt_reference_cpu.py) - what f64 arithmetic costs on these inputs, cancellation and conditioning included.  The margin of 4: the
device's exp and libm's each err by up to an ulp, which the exponent's size does not amplify but which the loop form's own figure holds
only one sample of, and the kernels add the K terms in blocks of four where the loop form adds them one by one.  (K + 4) 2^-53: any
association of K positive terms against the exact sum, the final 1 + sum, and the product with the prior weight (which is not 1).
Nothing here was fitted to what a device returned.

Bit equality where the project claims it: wave = lane, hashed = dense on every map both hold, a fleet member = its lone twin.  Slots
past n keep their weights.

Why no index or key these kernels form can leave its buffer, for ANY finite or non-finite pose (read off ndt_cell_likelihood,
csrc/ndt_kernels.hip; the poses beyond int32 of far_poses, up to 1e300, were added only after this was established): the centre is formed in
f64 - fx = floor(ux inv) - key_x0, no cast - and tested against the centre box (fx >= 0 && fx < box_w, the same in y; NaN and the
infinities fail the test) BEFORE anything becomes an integer.  Inside the box, dense: 0 <= fx < box_w <= 2^26, so the casts are exact and
the index (fy + reach) gw + fx + reach plus any offset's delta (|dy| <= reach rows, |dx| <= reach columns) lies inside the grid, whose
border is 2 reach.  Hashed: fx < box_w <= 2^32 + 2 * 64, cast to a 64-bit integer and added to a 64-bit first key; a neighbour key outside
int32 is not probed (ndt_hash_find_neighbour), any other is masked into the table, and the probe is bounded.  Outside the box no
look-up happens and the term is minimum_likelihood: that is the device's contract for poses whose keys the reference's int cast
leaves undefined; far_poses[not_finite] holds poses at +-inf and NaN to it.

singular: S' + S_map with det == 0 exactly, or rounding noise of either sign.  Read off the same function: inv_det = 1 / det is +-inf
or huge; with e == 0 or e along the wall the exponent is 0 * inf or inf - inf = NaN, and `likelihood > min ? likelihood : min` gives the
minimum (the one deliberate departure from the reference, whose std::max(NaN, min) returns the NaN); with e across the wall the exponent
is -inf for det >= 0 (the term is 0) and +huge for a tiny negative det (exp gives +inf, the weight is infinite).  No NaN reaches a
weight unless the prior weight is 0 and the sum infinite.  The device is held to exactly that rule (ndt_families.device_rule, the loop
form's f64 classes), every form to the same bits.
"""
import numpy as np
import pytest

import ndt_families as fam
import ndt_reference as ref
from beluga_amd.amcl import Amcl, AmclBatch, AmclParams, DifferentialDriveModelParam, NDTMap2d, NDTModelParam2d

pytestmark = pytest.mark.gpu

MOTION = DifferentialDriveModelParam(0.1, 0.05, 0.1, 0.05)
DENSE, HASHED = 0, 2
COUNTERS = ("ndt_lane_launches", "ndt_wave_launches")
PAST = 8  # slots kept behind n
# form -> (sizes, ndt_small_cycle, layout, the counter that moves)
FORMS = {"lane_dense": ((1, 63, 64, 65), False, DENSE, "ndt_lane_launches"), "wave_dense": ((1, 3, 4, 5), True, DENSE, "ndt_wave_launches"),
         "lane_hashed": ((1, 63, 64, 65), False, HASHED, "ndt_lane_launches"), "wave_hashed": ((1, 3, 4, 5), True, HASHED, "ndt_wave_launches")}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def ndt_map(case):
    return NDTMap2d(case.keys.astype(np.int32), case.means, case.covs, case.resolution)


def sensor(case):
    return NDTModelParam2d(case.minimum, case.d1, case.d2, case.kernel)


def launches(case, form):
    """(n, first state) of every launch of a form on a case.  The lane forms take every state at their largest size.  The wave forms'
    sizes are 1 to 5, so they walk the case's states, their sizes in turn, until every state has been through each of them - uy flips,
    placements at reach and reach + 1 and centres beyond int32 included, which five fixed states would miss."""
    sizes = FORMS[form][0]
    if not FORMS[form][1]:
        return [(n, 0) for n in sizes]
    out, first = [(n, 0) for n in sizes], 0
    while first < len(case.states):
        for n in sizes:
            out.append((n, first))
            first += n
    return out


def run_form(case, form):
    """{(n, first): weights of n particles - the case's states from `first` on, in turn, with their prior weights} under `form`; checks
    the counters and the slots past n."""
    sizes, small, layout, moved = FORMS[form]
    cap = max(sizes) + PAST
    f = Amcl(ndt_map(case), MOTION, sensor(case), AmclParams(min_particles=cap, max_particles=cap), seed=11, ndt_small_cycle=small,
             ndt_map_layout=layout)
    assert f.ndt_map_layout() == (layout, 1 if layout == HASHED else 0)
    out = {}
    for n, first in launches(case, form):
        pick = (first + np.arange(cap)) % len(case.states)
        states, w0 = case.states[pick], case.w0[pick]
        f.set_particles(states, w0)
        f.set_num_particles(n)
        before = {c: f.counter(c) for c in COUNTERS}
        f.reweight_ndt_cells(case.cell_means, case.cell_covs.reshape(-1, 4))
        delta = {c: f.counter(c) - before[c] for c in COUNTERS}
        assert delta == {c: int(c == moved and len(case.cell_means) > 0) for c in COUNTERS}, (case.tag, form, n, delta)
        f.set_num_particles(cap)
        got = f.particles()[1]
        assert np.array_equal(bits(got[n:]), bits(w0[n:])), "weights past n were written"
        out[(n, first)] = got[:n]
    f.close()
    return out


def states_of(case, n, first):
    return (first + np.arange(n)) % len(case.states)


def forms_of(case):
    return [form for form in FORMS if case.layout == "both" or FORMS[form][2] == HASHED]


_exact = {}


def exact(name, number, case):
    if (name, number) not in _exact:
        _exact[(name, number)] = case.exact()[0]
    return _exact[(name, number)]


def check_bits(case, results):
    """wave = lane, state by state over every wave launch (the lane form's 65 slots hold every state of a case: at most 64); hashed =
    dense on a map both hold."""
    assert len(case.states) <= 65
    for layout in ("dense", "hashed"):
        if "lane_" + layout in results:
            lane = results["lane_" + layout][(65, 0)]
            for (n, first), got in results["wave_" + layout].items():
                assert np.array_equal(bits(got), bits(lane[states_of(case, n, first)])), (case.tag, layout, n, first)
    if "lane_dense" in results:
        for kind in ("lane", "wave"):
            for at, got in results[kind + "_dense"].items():
                assert np.array_equal(bits(got), bits(results[kind + "_hashed"][at])), (case.tag, kind, at)


@pytest.mark.parametrize("name", fam.EXACT_FAMILIES)
def test_every_form_picks_the_reference_cell(name):
    for number, case in enumerate(fam.FAMILIES[name]()):
        want_all = exact(name, number, case)
        K = len(case.cell_means)
        bound = 4 * fam.MEASURED_F64_ERROR[name] + (K + 4) * 2.0**-53
        results = {}
        for form in forms_of(case):
            results[form] = run_form(case, form)
            for (n, first), got in results[form].items():
                want = want_all[states_of(case, n, first)]
                err = float(np.max(np.abs(got - want) / want))
                print("ndt_edges %s %s n=%d first=%d K=%d worst=%.3g (%.2f of the bound)" % (case.tag, form, n, first, K, err, err / bound))
                assert err <= bound, (case.tag, form, n, first, err, bound)
        check_bits(case, results)


def test_singular_sums_follow_the_written_rule():
    """NaN terms count as minimum_likelihood, an infinite term gives an infinite weight, every form returns the same bits; the finite
    weights agree with the loop form's (the same f64 operations in the same order, so the same exponent bits; exp within an ulp on
    either side) within (K + 12) 2^-53."""
    case = fam.singular()[0]
    want = fam.device_rule(case)
    assert np.isinf(want).any() and np.isfinite(want).any()
    K = len(case.cell_means)
    results = {form: run_form(case, form) for form in FORMS}
    check_bits(case, results)
    for form, by_n in results.items():
        for (n, first), got in by_n.items():
            w = want[states_of(case, n, first)]
            assert not np.isnan(got).any(), (form, n)
            assert np.array_equal(np.isinf(got), np.isinf(w)) and np.all(got[np.isinf(w)] > 0), (form, n)
            fin = np.isfinite(w)
            assert np.max(np.abs(got[fin] - w[fin]) / w[fin], initial=0.0) <= (K + 12) * 2.0**-53, (form, n)
    # the states whose every singular term is a NaN or 0: exactly the floor's share for those cells
    terms = fam.singular_terms(case)
    got = results["lane_dense"][(65, 0)][:2]
    held = np.where(np.isnan(terms[:2]), case.minimum, np.maximum(terms[:2], case.minimum))
    np.testing.assert_allclose(got, case.w0[:2] * (1.0 + held.sum(axis=1)), rtol=(K + 12) * 2.0**-53)


def cluster_scan(cells, resolution, seed):
    """Six points inside each of the base-frame cells `cells` (a measurement cell each: five points make one), in no cell order."""
    rng = np.random.Generator(np.random.PCG64(seed))
    pts = [(np.array(c) + rng.uniform(0.2, 0.8, (6, 2))) * resolution for c in cells]
    return np.concatenate(pts) if pts else np.zeros((0, 2))


def test_a_fleet_member_equals_its_lone_twin_and_the_exact_weights():
    """Three NDT members on the fleet's shared launch (k_batch_reweight_ndt), one of them with a scan that fits no measurement cell
    (K = 0: it takes no block of the launch and keeps its weights): each member's states, weights and estimate are its lone twin's bit
    for bit, the twins' own launches are the wave kernel's, and the weights are the exact ones of the propagated states, normalised -
    within the reweight's tolerance plus the normalisation's (2 (n - 1) + 1) 2^-53 (test_gpu_lf_edges.py).  No resampling in the cycle.

    What this does NOT do: a fleet takes scans, not measurement cells, and propagates before it reweights, so the shared launch meets
    none of the engineered (state, cell) pairs - its cells come out of the measurement fit and its poses out of the motion model, on
    one box_edges map - and it is not among the forms of the singular test.  What ties k_batch_reweight_ndt to the edges is that its
    body IS the wave kernel's (reweight_ndt_wave_block, one function), which the tests above hold on every pair, and the bit equality
    with the twin here, which shows that the member's record carries the same view and cells into it."""
    from beluga_amd.amcl import se2_from_xytheta
    case = fam.box_edges()[0]
    res = case.resolution
    params = AmclParams(min_particles=5, max_particles=5, resample_interval=1000)
    scans = [cluster_scan([(1, 0), (-2, 1), (0, -3)], res, 1), cluster_scan([], res, 2)[:0], cluster_scan([(2, 2), (-1, -1), (3, -2), (0, 1), (1, 1)], res, 3)]
    scans[1] = np.array([(0.1, 0.1), (0.2, 0.1), (0.3, 0.2), (0.1, 0.3)])  # four points: no cell
    specs = [dict(grid=ndt_map(case), motion=MOTION, sensor=sensor(case), params=params, seed=5 + k, options=None, ndt_small_cycle=True)
             for k in range(3)]
    batch = AmclBatch(specs)
    twins = [Amcl(ndt_map(case), MOTION, sensor(case), params, seed=5 + k, ndt_small_cycle=True) for k in range(3)]
    states, w0 = case.states[6:11], case.w0[6:11]
    for f in batch.members + twins:
        f.set_particles(states, w0)
    control = se2_from_xytheta(0.0, 0.0, 0.0)
    before = [{c: t.counter(c) for c in COUNTERS} for t in twins]
    launches = batch.ndt_counts()
    got = batch.update([control] * 3, scans)
    assert batch.ndt_counts() == (launches[0] + 1, launches[1] + 3)
    for k in range(3):
        want = twins[k].update(control, scans[k])
        assert np.array_equal(got[k][0], want[0]) and np.array_equal(got[k][1], want[1], equal_nan=True)
        (ms, mw), (ts, tw) = batch.members[k].particles(), twins[k].particles()
        assert np.array_equal(bits(ms), bits(ts)) and np.array_equal(bits(mw), bits(tw))
        delta = {c: twins[k].counter(c) - before[k][c] for c in COUNTERS}
        cell_means, cell_covs = ref.to_cells(scans[k], res)
        K = len(cell_means)
        assert K == (3, 0, 5)[k]
        assert delta == {"ndt_lane_launches": 0, "ndt_wave_launches": int(K > 0)}, (k, delta)
        exact_w = ref.weights_exact(case.ref_map(), ts, cell_means, cell_covs, w0, **case.model())[0]
        bound = 4 * fam.MEASURED_F64_ERROR["box_edges"] + ((K + 4) + 2 * (len(tw) - 1) + 1) * 2.0**-53
        assert np.max(np.abs(tw - exact_w / exact_w.sum()) / tw) <= bound, k
    batch.close()
    for t in twins:
        t.close()
