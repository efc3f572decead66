"""What the likelihood-field kernels' CELL DECISION is held to: every kernel form on every family of tests/lf_families.py (end-points
engineered onto cell boundaries, the fast path's trigger, the grid's borders, the 2^14-cell guard, tiny grids, every beam count, scan
points without a cell), against tests/lf_reference.py on a field where one wrong cell moves a weight by more than 1e-6
(lf_reference.revealing_field).  Each form is pinned by its launch counters: a silent re-route fails the test.

Held: weights within (B + 4) 2^-53 relative of lf_reference.weights - the terms are positive and identical on both sides, any association
of B of them errs by at most (B - 1) 2^-53 against the exact sum, plus the rounding of the reference's own sum, of the kernels' final
`1 + sum` and of the product with the prior weight (which is not 1).  The prob model: the suite's 1e-11 against weights_prob.  Bit
equality where the project claims it (patch = gather, far tiles = plain on the same field, fast = lf_fast 0, a batch member = its lone
twin).  Nothing is written past n.

Why no address these kernels form can leave its buffer, for ANY int cell and ANY finite pose (read off csrc/kernels.hip; the families
long_lever and no_cell were run only after this was established):
  * lf_beam (index order, k_reweight_lf_sorted<false>): the cell is range-checked (`inside`, unsigned compares) before it becomes an
    index; outside lanes read element 0.
  * k_reweight_lf_sorted<true>: lf_cube_fetch range-checks the cell and otherwise reads the table's extra "unknown" slot; the load is a
    buffer load with num_records = (cells + 1) * 8.
  * the palette kernels' exact path (issue / term / add_exact, the beams kernel, the far-beams fallback): clamp_cell = v_med3_i32(v, -1, W
    or H) for any int, so the LDS row index yc + 1 lies in [0, H + 1] - the row table has H + 2 words - and the byte offset is at most the
    table's last border tile; the load is a buffer load with num_records = pal_bytes (out of range returns 0, moves nothing).
  * the fast paths (issue_fast, far-beams issue, the patch kernel's gathered look-ups): v_med3_i32 of the biased high word against
    kFastBias - 1 and kFastBias + W / H, for any bit pattern (NaN and infinities included); then as above.  The far-tile bitmap is indexed by
    the clamped cell's tile (tiles of the bordered table: inside far_bytes / far_linear_bytes by construction of the bitmap).
  * the patch kernel's LDS look-ups (patch_address) are NOT clamped and NOT range-checked: inside the planner's bound they fall into the
    patch; outside it nothing in the code confines them.  What makes them harmless is a property of the HARDWARE, not an argument from
    the code: they are LDS reads, and on CDNA an LDS read beyond the workgroup's allocation returns 0 and faults nothing (the kernel's own
    comment relies on the same).  A wrong patch read can therefore give a wrong WEIGHT - which these tests would show - but no fault.  The
    producer's stores go to fixed places of the patch buffers.
  * scan points are read by beam index b < B (or padded with zeros in LDS); poses through perm[t < n].
Points without a cell never reach a kernel: the host takes NaN and infinite points out where the scan is staged and starts every
particle's sum at their count times the unknown-space term (FieldView::acc0).  FINITE points so large that |v| >= 2^31 are out of contract
(INTEGRATION.md): they are in the CPU reference's family, not in the device's.
"""
import numpy as np
import pytest

import lf_families as fam
import lf_reference as ref
from beluga_amd.amcl import (Amcl, AmclParams, DifferentialDriveModelParam, LikelihoodFieldModelParam, LikelihoodFieldProbModelParam,
                             OccupancyGrid)

pytestmark = pytest.mark.gpu

MOTION = DifferentialDriveModelParam(0.1, 0.05, 0.1, 0.05)
MAX_LASER = 100.0
LF = LikelihoodFieldModelParam(2.0, MAX_LASER, 0.5, 0.5, 0.2, True)
LF_PROB = LikelihoodFieldProbModelParam(2.0, MAX_LASER, 0.5, 0.5, 0.2, True)
ORDERED_N = 16_411  # 32 workgroups of 512 and 27 particles; the ordered kernels engage from 16 384 (lf_small_particles pinned)
COUNTERS = ("lf_beams_launches", "lf_fast_launches", "lf_patch_launches", "lf_queue_launches", "lf_far_launches", "lf_far_beams_launches")

# form -> (particle counts, options, the counters that must have moved by one; all others of COUNTERS must not have moved, field kind)
FORMS = {
    "beams": ((1, 63, 64, 65, 1025), {}, ("lf_beams_launches",), "palette"),                                  # k_reweight_lf_beams
    "beams_variant3": ((65,), {"lf_variant": 3}, ("lf_beams_launches",), "palette"),
    # five particles per wave (ceil(16 411 / 4096)): the launch a set reported as dispersed gets under lf_dispersed = 1 - that option
    # changes only how the planner arrives at it (after a probing patch launch), not the kernel or its arguments
    "beams_per_wave5": ((ORDERED_N,), {"lf_small_particles": 65_536}, ("lf_beams_launches",), "palette"),
    "index_order": ((1, 65, 1025), {"lf_table": 1}, (), "cube"),                                              # lf_beam, a lane per particle
    "index_order_variant0": ((65,), {"lf_variant": 0}, (), "palette"),
    "index_order_variant1": ((65,), {"lf_variant": 1}, (), "palette"),
    "sorted_cube": ((ORDERED_N,), {"lf_table": 1}, (), "cube"),                                              # k_reweight_lf_sorted<true>
    "palette_exact": ((ORDERED_N,), {"lf_fast": 0, "lf_patch": 0}, (), "palette"),                           # k_reweight_lf_palette<false>
    "palette_fast": ((ORDERED_N,), {"lf_patch": 0, "lf_far_tiles": 0, "lf_dispersed": 0}, ("lf_fast_launches",), "palette"),
    "palette_fast_key_layout1": ((ORDERED_N,), {"lf_patch": 0, "lf_far_tiles": 0, "lf_dispersed": 0, "key_layout": 1}, ("lf_fast_launches",),
                                 "palette"),
    "patch": ((ORDERED_N,), {"lf_patch": 2}, ("lf_fast_launches", "lf_patch_launches"), "palette"),           # k_reweight_lf_patch<false>
    # k_reweight_lf_patch<true>: 37 blocks of 448 particles on 8 resident workgroups that take them from a queue; one segment only,
    # i.e. fewer than 128 beams (MAX_POINTS)
    "patch_queue": ((ORDERED_N,), {"lf_patch": 2, "lf_queue": 1, "lf_queue_grid": 8},
                    ("lf_fast_launches", "lf_patch_launches", "lf_queue_launches"), "palette"),
    "palette_fast_far_field": ((ORDERED_N,), {"lf_patch": 0, "lf_far_tiles": 0, "lf_dispersed": 0}, ("lf_fast_launches",), "far"),
    "palette_far": ((ORDERED_N,), {"lf_patch": 0, "lf_far_tiles": 2, "lf_dispersed": 0}, ("lf_fast_launches", "lf_far_launches"), "far"),
    "far_beams": ((ORDERED_N,), {"lf_patch": 0, "lf_far_tiles": 2, "lf_dispersed": 2},
                  ("lf_fast_launches", "lf_far_launches", "lf_far_beams_launches"), "far"),                   # k_reweight_lf_far_beams<false>
    "far_beams_per_wave5": ((ORDERED_N,), {"lf_patch": 0, "lf_far_tiles": 2, "lf_dispersed": 2, "lf_far_beams_per_wave": 5},
                            ("lf_fast_launches", "lf_far_launches", "lf_far_beams_launches"), "far"),
}
PROB_FORMS = ("beams", "palette_exact", "palette_fast", "patch", "far_beams")
# patch = gather, fast = exact, either key layout; the far-tile gather = the plain one ON THE SAME FIELD; the far-beams kernel whatever a
# wave's share of poses (against the lane-per-particle kernels it differs in the rounding of the lane sums: no bit equality claimed)
BIT_EQUAL = (("patch", "palette_fast"), ("palette_fast", "palette_exact"), ("palette_fast_key_layout1", "palette_fast"),
             ("palette_far", "palette_fast_far_field"), ("far_beams_per_wave5", "far_beams"))
MAX_POINTS = {"patch_queue": 120}
# index_order*, sorted_cube and palette_exact move none of the library's counters: the library counts no launches of theirs, so these
# five are told apart from the counted forms but not from each other by the pin.  Their options leave launch_reweight_lf one way each.
# (The far-tile forms engage on the tiniest grids too: the table's border tiles of "unknown" cells are far tiles.)


def field_for(shape, kind):
    """The revealing field; kind "far": its right half flat (one value of its own), so that the far-tile bitmap has tiles to mark - the
    engineered end-points in the left half still show a wrong cell."""
    H, W = shape
    if kind != "far":
        return ref.revealing_field(H, W, kind)
    f = ref.revealing_field(H, W, "palette").copy()
    if W >= 32:
        f[:, W // 2:] = np.float32(0.71875)
    elif H >= 32:
        f[H // 2:, :] = np.float32(0.71875)
    return f


_filters = {}


def filter_for(case, n, prob):
    """One filter per (grid, capacity, model), kept for the module: options and the field are set per use."""
    key = (case["shape"], case["resolution"], tuple(case["origin"]), n, prob)
    if key not in _filters:
        H, W = case["shape"]
        grid = OccupancyGrid(cells=np.zeros((H, W), dtype=np.int8), resolution=case["resolution"], origin=case["origin"])
        f = Amcl(grid, MOTION, LF_PROB if prob else LF, AmclParams(min_particles=n + 64, max_particles=n + 64), seed=11)
        f.set_option("lf_small_particles", 16_384)
        _filters[key] = f
    return _filters[key]


@pytest.fixture(scope="module", autouse=True)
def _close_filters():
    yield
    for f in _filters.values():
        f.close()
    _filters.clear()


DEFAULTS = {"lf_variant": 2, "lf_table": 0, "lf_fast": 1, "lf_patch": 1, "lf_far_tiles": 1, "lf_dispersed": 2, "key_layout": 0,
            "lf_far_beams_per_wave": 0, "lf_small_particles": 16_384, "lf_queue": 1, "lf_queue_grid": 0}


def run_form(case, points, form, n, prob=False, expect=None):
    """Weights of n particles (the case's poses in turn, prior weights not 1) under `form`; checks the counters and the rows past n."""
    _, options, moved, kind = FORMS[form]
    m = len(case["states"])
    states = case["states"][np.arange(n + 64) % m]
    w0 = np.random.Generator(np.random.MT19937(3)).uniform(0.5, 1.5, n + 64)
    f = filter_for(case, n, prob)
    for name, value in {**DEFAULTS, **options}.items():
        f.set_option(name, value)
    f.set_likelihood_field(field_for(case["shape"], kind))
    f.set_particles(states, w0)
    f.set_num_particles(n)
    before = {c: f.counter(c) for c in COUNTERS}
    f.reweight(points)
    delta = {c: f.counter(c) - before[c] for c in COUNTERS}
    want_moved = set(moved if expect is None else expect)
    assert delta == {c: (1 if c in want_moved else 0) for c in COUNTERS}, (form, n, delta)
    f.set_num_particles(n + 64)
    got = f.particles()[1]
    assert np.array_equal(got[n:], w0[n:]), "weights past n were written"
    return got[:n], w0[:n]


_want = {}


def reference(case, points, kind, prob, tag):
    key = (tag, kind, prob)
    if key not in _want:
        fn = ref.weights_prob if prob else ref.weights
        _want[key] = fn(field_for(case["shape"], kind), case["resolution"], case["origin"], MAX_LASER, case["states"], points)
    return _want[key]


def expected_counters(form, points):
    """Where a form cannot engage, what runs instead: a scan of which no point is left (none given, or none with a cell) has no far-beams
    launch (launch_reweight_lf: B > 0) - the far-tile gather kernel takes it."""
    moved = set(FORMS[form][2])
    if int(np.isfinite(np.asarray(points, dtype=np.float64).reshape(-1, 2)).all(axis=1).sum()) == 0:
        moved -= {"lf_far_beams_launches"}
    return moved


def check(case, points, form, tag, prob=False, sizes=None, results=None):
    if form in MAX_POINTS and len(points) > MAX_POINTS[form]:
        points, tag = points[:MAX_POINTS[form]], "%s[:%d]" % (tag, MAX_POINTS[form])
    B = len(points)
    for n in sizes or FORMS[form][0]:
        got, w0 = run_form(case, points, form, n, prob, expect=expected_counters(form, points))
        want = reference(case, points, FORMS[form][3], prob, tag)[np.arange(n) % len(case["states"])] * w0
        err = np.max(np.abs(got - want) / want)
        bound = 1e-11 if prob else (B + 4) * 2.0 ** -53
        print("lf_edges %s %s n=%d B=%d prob=%d worst=%.3g (%.2f of the bound)" % (tag, form, n, B, prob, err, err / bound))
        assert err <= bound, (form, tag, n, err, bound)
        if results is not None:
            results[(form, n)] = got


# A table of 16 000 rows (long_lever along y) leaves no room in LDS for the patches or the far-tile bitmap next to the row offsets: the library
# sends such a map to the plain gather kernels, which the other forms cover - these forms skip that case.
LDS_HUNGRY = ("patch", "patch_queue", "palette_far", "far_beams", "far_beams_per_wave5")


def fits(case, form):
    return not (case["shape"][0] > 4096 and form in LDS_HUNGRY)


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", ["ulp_straddle", "trigger_ring", "long_lever", "borders", "small_grids", "no_cell"])
def test_every_form_picks_the_reference_cell(name, form):
    """no_cell: every form gives the written rule's weight (a point without a cell counts as unknown space)."""
    for k, case in enumerate(fam.FAMILIES[name]()):
        if fits(case, form):
            check(case, case["points"], form, "%s[%d]" % (name, k))


@pytest.mark.parametrize("form", PROB_FORMS)
@pytest.mark.parametrize("name", ["ulp_straddle", "borders", "no_cell"])
def test_prob_model_instances_pick_the_reference_cell(name, form):
    """(The first 100 points of a case: the product of more than ~150 unknown-space terms of 0.01 leaves the doubles' range.)"""
    for k, case in enumerate(fam.FAMILIES[name]()[:2]):
        check(case, case["points"][:100], form, "%s[%d][:100]" % (name, k), prob=True, sizes=FORMS[form][0][-1:])


@pytest.mark.parametrize("name", ["ulp_straddle", "trigger_ring", "long_lever", "borders"])
def test_forms_that_claim_the_same_bits_give_them(name):
    for k, case in enumerate(fam.FAMILIES[name]()):
        results = {}
        pairs = [(a, b) for a, b in BIT_EQUAL if fits(case, a) and fits(case, b)]
        for form in sorted({f for pair in pairs for f in pair}):
            check(case, case["points"], form, "%s[%d]" % (name, k), results=results)
        for a, b in pairs:
            assert np.array_equal(results[(a, ORDERED_N)], results[(b, ORDERED_N)]), (name, k, a, b)


@pytest.mark.parametrize("form", ["sorted_cube", "palette_exact", "palette_fast", "patch", "palette_far"])
def test_group_of_8_kernels_over_every_beam_count(form):
    """0 .. 41 beams: 0 to 5 groups of 8 (prologue only, odd and even exits of the pipelined loop) times tails of 0 to 7 (the block of four
    and the singles); then the segmented launches (lf_families.SEGMENT_COUNTS: short last segments)."""
    case = fam.beam_counts()[0]
    for B in fam.GROUP_OF_8_COUNTS + fam.SEGMENT_COUNTS:
        check(case, case["points"][:B], form, "beam_counts[%d]" % B)


@pytest.mark.parametrize("form", ["beams", "far_beams", "index_order"])
def test_lanes_over_beams_kernels_over_every_beam_count(form):
    case = fam.beam_counts()[0]
    for B in fam.LANE_COUNTS:
        check(case, case["points"][:B], form, "beam_counts[%d]" % B, sizes=FORMS[form][0][-1:])


def test_update_and_batch_update_take_a_scan_with_points_without_a_cell():
    """The same scan through mcl_update (the scan staged ahead and pulled by the propagation kernel) and through mcl_batch_update (the
    fleet's shared k_batch_reweight_lf_beams: FieldView::acc0 and the staged count travel in the member's record): a batch member
    equals its lone twin bit for bit, and a twin fed the scan with every point without a cell replaced by a finite point outside
    every grid - the same unknown-space terms, added inside the scan instead of in front of it - has the same states and estimate
    and weights within 2 (B + 4) 2^-53 (the two sums' roundings).  No resampling in the cycle: the weights are the reweight's, normalised."""
    from beluga_amd.amcl import AmclBatch, se2_from_xytheta
    case = fam.no_cell()[4]
    H, W = case["shape"]
    grid = OccupancyGrid(cells=np.zeros((H, W), dtype=np.int8), resolution=case["resolution"], origin=case["origin"])
    params = AmclParams(min_particles=600, max_particles=600, resample_interval=1000)
    bad = case["points"]
    far = np.where(np.isfinite(bad).all(axis=1)[:, None], bad, 1e6)
    assert (~np.isfinite(bad).all(axis=1)).sum() == 5
    batch = AmclBatch([dict(grid=grid, motion=MOTION, sensor=LF, params=params, seed=5 + k, options=None) for k in range(2)])
    twins = [Amcl(grid, MOTION, LF, params, seed=5 + k) for k in range(2)]
    others = [Amcl(grid, MOTION, LF, params, seed=5 + k) for k in range(2)]
    field = ref.revealing_field(H, W, "palette")
    mean = (case["origin"][2] + 3.0, case["origin"][3] + 4.0, 1.0)
    for f in batch.members + twins + others:
        f.set_likelihood_field(field)
        f.initialize(mean, np.diag([0.25, 0.25, 0.1]))
    control = se2_from_xytheta(0.0, 0.0, 0.0)
    got = batch.update([control, control], [bad, bad])
    assert batch.counter("members_fused") == 2
    B = len(bad)
    for k in range(2):
        want = twins[k].update(control, bad)
        alt = others[k].update(control, far)
        assert np.array_equal(got[k][0], want[0]) and np.array_equal(got[k][1], want[1])
        ms, mw = batch.members[k].particles()
        ts, tw = twins[k].particles()
        os_, ow = others[k].particles()
        assert np.array_equal(ms, ts) and np.array_equal(mw, tw)
        assert np.array_equal(ts, os_) and np.all(np.isfinite(tw))
        assert np.max(np.abs(tw - ow) / ow) <= 2 * (B + 4) * 2.0 ** -53
        np.testing.assert_allclose(want[0], alt[0], rtol=0, atol=1e-12)
        # and against the exact reference: the propagated states' weights, normalised
        exact = ref.weights(field, case["resolution"], case["origin"], MAX_LASER, ts, bad)
        # (B + 4) 2^-53 for the reweight as everywhere in this file, and for the normalisation: the device's sum of n = 600 positive
        # weights in some association and numpy's pairwise one, (n - 1) 2^-53 each against the exact sum, and the division
        bound = ((B + 4) + 2 * (len(tw) - 1) + 1) * 2.0 ** -53
        assert np.max(np.abs(tw - exact / exact.sum()) / tw) <= bound
    batch.close()
    for f in twins + others:
        f.close()
