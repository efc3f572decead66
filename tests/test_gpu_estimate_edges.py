"""The estimate kernels against the exact reference (tests/estimate_reference.py) on the families of tests/estimate_families.py:
  (a) the nine sums of k_estimate_partials / k_final_rows at every size of the launch geometry, about three pivots;
  (b) mcl_estimate_pose wherever the cloud sits: right after set_particles, after initialize at a far mean, with a pivot left over from
      a set somewhere else, and a second time on the same set;
  (c) the estimate update() returns on a grid at a far origin: the one-workgroup tail with and without resampling, the large path with
      the sums folded into the draw kernel and behind it;
  (d) estimate_clusters and cluster_based_estimate on blobs 100 m apart, on both cluster paths.
A figure is held to max(estimate_error_bound(n), 4 x the oracle's error on the same inputs) of its conditioned units
(estimate_families.limit); the bound is derived in estimate_reference.estimate_error_bound and is not fitted to the device."""
import numpy as np
import pytest

import estimate_families as fam
import estimate_reference as ref
from oracle import binding as orc

pytestmark = pytest.mark.gpu

SUMS_CASES = fam.sums_cases()
POSE_CASES = fam.pose_cases()
CAPACITY = fam.N_STRIDED


@pytest.fixture(scope="module")
def filt():
    """One filter for the module: set_particles replaces the set of any size up to its capacity."""
    from beluga_amd.amcl import Amcl, AmclParams, DifferentialDriveModelParam, LikelihoodFieldModelParam, OccupancyGrid, se2_from_xytheta
    grid = OccupancyGrid(np.zeros((64, 64), dtype=np.int8), 0.05, origin=se2_from_xytheta(0.0, 0.0, 0.0))
    f = Amcl(grid, DifferentialDriveModelParam(0.1, 0.05, 0.1, 0.05), LikelihoodFieldModelParam(2.0, 100.0, 0.5, 0.5, 0.2, True),
             AmclParams(min_particles=CAPACITY, max_particles=CAPACITY), seed=7)
    yield f
    f.close()


# ---- (a) the sums kernels alone ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SUMS_CASES, ids=[c[0] for c in SUMS_CASES])
def test_estimate_sums_against_the_exact_sums(filt, case):
    label, n, centre = case[0], case[1], case[2]
    s, w = fam.cloud(*case[1:])
    filt.set_particles(s, w)
    bound = ref.estimate_error_bound(n)
    for name, pivot in fam.sums_pivots(centre).items():
        got = filt.estimate_sums(pivot)
        again = filt.estimate_sums(pivot)
        assert got.tobytes() == again.tobytes(), f"{label}, pivot {name}: two calls differ"
        assert got[9] == pivot[0] and got[10] == pivot[1]
        e = ref.sum_errors(ref.sums(s, w, pivot), got[:9])
        print(f"{label}, pivot {name}: " + " ".join(f"{k} {v:.3g}" for k, v in zip(ref.SUM_NAMES, e)) + f" units (bound {bound})")
        assert e.max() <= bound, f"{label}, pivot {name}: {ref.SUM_NAMES[int(e.argmax())]} {e.max()} units > {bound}"


# ---- (b) mcl_estimate_pose wherever the cloud sits ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", POSE_CASES, ids=[c[0] for c in POSE_CASES])
def test_estimate_after_set_particles_and_again(filt, case):
    """The first estimate of a set, and a second one on the same set (its pivot: the first estimate)."""
    label, n = case[0], case[1]
    s, w = fam.cloud(*case[1:])
    r, oracle = fam.yardstick(case)
    filt.set_particles(s, w)
    fam.hold(label + " first", n, ref.errors(r, *filt.estimate()), oracle)
    fam.hold(label + " second", n, ref.errors(r, *filt.estimate()), oracle)


STALE_CASES = [c for c in POSE_CASES if c[2] != "origin"]


@pytest.mark.parametrize("case", STALE_CASES, ids=[c[0] for c in STALE_CASES])
def test_estimate_with_a_pivot_left_by_a_set_elsewhere(filt, case):
    """An estimate at one centre, then set_particles at another: the first estimate's pivot must not serve the second set."""
    label, n = case[0], case[1]
    elsewhere = "utm_west" if case[2] != "utm_west" else "utm"
    s0, w0 = fam.cloud(65, elsewhere, "s0.05", "gamma", "tight")
    filt.set_particles(s0, w0)
    filt.estimate()
    s, w = fam.cloud(*case[1:])
    r, oracle = fam.yardstick(case)
    filt.set_particles(s, w)
    fam.hold(label + " after a set at " + elsewhere, n, ref.errors(r, *filt.estimate()), oracle)


INIT_N = (65, 4097, 65_537)
INIT_MEANS = {"utm": (5e5, 4e6, 0.7), "utm_west": (-4e6, 5e5, -2.0), "near": (57.3, -41.2, 0.3)}
INIT_SIGMAS = (0.5, 0.05, 0.01)


@pytest.fixture(scope="module")
def init_filters():
    """One filter per size of INIT_N, built on first use."""
    from beluga_amd.amcl import Amcl, AmclParams, DifferentialDriveModelParam, LikelihoodFieldModelParam, OccupancyGrid, se2_from_xytheta
    made = {}

    def get(n):
        if n not in made:
            grid = OccupancyGrid(np.zeros((64, 64), dtype=np.int8), 0.05, origin=se2_from_xytheta(0.0, 0.0, 0.0))
            made[n] = Amcl(grid, DifferentialDriveModelParam(0.1, 0.05, 0.1, 0.05), LikelihoodFieldModelParam(2.0, 100.0, 0.5, 0.5, 0.2, True),
                           AmclParams(min_particles=n, max_particles=n), seed=11)
        return made[n]

    yield get
    for f in made.values():
        f.close()


@pytest.mark.parametrize("n", INIT_N)
@pytest.mark.parametrize("sigma", INIT_SIGMAS)
@pytest.mark.parametrize("where", list(INIT_MEANS))
def test_estimate_after_initialize_at_a_far_mean(init_filters, where, sigma, n):
    """initialize(mean, cov) draws the set on the device; the reference is taken over the particles read back.  Before it, an estimate
    of a set on the other side of the map leaves a stale pivot behind."""
    f = init_filters(n)
    other = INIT_MEANS["utm_west" if where != "utm_west" else "utm"]
    f.initialize(other, np.diag([0.01, 0.01, 0.01]))
    f.estimate()
    f.initialize(INIT_MEANS[where], np.diag([sigma ** 2, sigma ** 2, 0.01]))
    got = f.estimate()
    s, w = f.particles()
    assert len(w) == n
    r = ref.estimate(s, w)
    fam.hold(f"initialize {where} sigma {sigma} n {n}", n, ref.errors(r, *got), ref.errors(r, *orc.estimate(s, w)))


def test_a_second_pass_is_taken_exactly_where_the_pivot_lies_outside_the_set(filt):
    """mcl_get_counter("estimate_repivots").  A set installed about a point of itself takes no second pass; nor does a second
    estimate, the caller's own estimate_sums, or a shrunk set (set_num_particles keeps the pivot).  Of two blobs 100 m apart every
    cluster of the blob the pivot is not in takes one, and none takes two."""
    s, w = fam.cloud(4097, "utm", "s0.05", "gamma", "tight")
    before = filt.counter("estimate_repivots")
    filt.set_particles(s, w)
    filt.estimate()
    filt.estimate()
    filt.estimate_sums((0.0, 0.0))
    filt.set_num_particles(4000)
    filt.estimate()
    assert filt.counter("estimate_repivots") == before
    # two blobs 100 m apart: the overall pivot (the first weighted state, in one blob) is outside the other blob's clusters
    sb, wb, which = fam.blobs(20_001, "utm", 2)
    filt.set_particles(sb, wb)
    labels = filt.cluster_labels()
    before = filt.counter("estimate_repivots")
    total, found = filt.estimate_clusters()
    far = sum(1 for cid, *_ in found if int(which[labels == cid][0]) != int(which[0]))
    assert far >= 1
    taken = filt.counter("estimate_repivots") - before
    assert far <= taken <= len(found), (far, taken, len(found))  # every cluster of the other blob, once each; none twice


# ---- (c) the estimate that update() returns -------------------------------------------------------------------------------------------
FAR_ORIGIN = (5e5, 4e6)
UPDATE_PATHS = {  # n, resample_interval, options
    "small tail, resampling": (2000, 1, {}),
    "small tail, no resampling": (2000, 3, {}),
    "large path, sums folded into the draw": (20_001, 1, {"draw_fold": 1}),
    "large path, k_estimate_partials behind the draw": (20_001, 1, {"draw_fold": 0}),
}


@pytest.mark.parametrize("path", list(UPDATE_PATHS))
def test_update_returns_the_estimate_of_the_set_it_leaves_on_a_far_map(path):
    """A 128 x 128 grid whose origin is at (5e5, 4e6): the first update() after initialize and the one after it, each held to the exact
    reference over particles() read back behind it (the set and the weights the cycle leaves)."""
    from beluga_amd import synth
    from beluga_amd.amcl import Amcl, AmclParams, DifferentialDriveModelParam, LikelihoodFieldModelParam, OccupancyGrid, se2_from_xytheta
    n, interval, options = UPDATE_PATHS[path]
    cells = synth.make_rooms_map(128, 128, seed=5, n_rooms=4)
    grid = OccupancyGrid(cells, 0.05, origin=se2_from_xytheta(FAR_ORIGIN[0], FAR_ORIGIN[1], 0.0))
    truth = synth.find_free_pose(cells, 0.05, FAR_ORIGIN, seed=3, clearance_cells=6)
    angles = synth.lidar_angles(90, 270.0)
    f = Amcl(grid, DifferentialDriveModelParam(0.1, 0.05, 0.1, 0.05), LikelihoodFieldModelParam(2.0, 100.0, 0.5, 0.5, 0.2, True),
             AmclParams(min_particles=n, max_particles=n, resample_interval=interval), seed=42)
    try:
        for name, value in options.items():
            f.set_option(name, value)
        f.initialize(truth, np.diag([0.04, 0.04, 0.01]))
        pose, odom = truth, (0.0, 0.0, 0.0)
        tails = f.counter("small_tail_launches")
        for c in range(2):
            pose = synth.odometry_step(pose, 0.3, 0.05)
            odom = synth.odometry_step(odom, 0.3, 0.05)
            ranges = synth.cast_scan(cells, 0.05, FAR_ORIGIN, pose, angles, 8.0, 0.01, seed=c)
            got = f.update(se2_from_xytheta(*odom), synth.scan_points(ranges, angles))
            assert got is not None
            assert bool(f.last_info["resampled"]) == (interval == 1), path
            s, w = f.particles()
            r = ref.estimate(s, w)
            fam.hold(f"{path}, cycle {c}", len(w), ref.errors(r, *got), ref.errors(r, *orc.estimate(s, w)))
        assert (f.counter("small_tail_launches") - tails == 2) == (n <= 4096), path
        print(f"{path}: second passes {f.counter('estimate_repivots')}")
        assert f.counter("estimate_repivots") == 0, path  # (the set was installed about its mean and the pivot is carried with it)
    finally:
        f.close()


def test_a_batch_member_returns_the_estimate_of_the_set_it_leaves_on_a_far_map():
    """Two members of an AmclBatch on the far grid (k_batch_small_tail, finish_small_cycle per member): each member's estimate of each
    cycle against the exact reference over that member's particles() read back."""
    from beluga_amd import synth
    from beluga_amd.amcl import AmclBatch, AmclParams, DifferentialDriveModelParam, LikelihoodFieldModelParam, OccupancyGrid, se2_from_xytheta
    cells = synth.make_rooms_map(128, 128, seed=5, n_rooms=4)
    grid = OccupancyGrid(cells, 0.05, origin=se2_from_xytheta(FAR_ORIGIN[0], FAR_ORIGIN[1], 0.0))
    truth = synth.find_free_pose(cells, 0.05, FAR_ORIGIN, seed=3, clearance_cells=6)
    angles = synth.lidar_angles(90, 270.0)
    sizes = (2000, 1501)
    batch = AmclBatch([dict(grid=grid, motion=DifferentialDriveModelParam(0.1, 0.05, 0.1, 0.05),
                            sensor=LikelihoodFieldModelParam(2.0, 100.0, 0.5, 0.5, 0.2, True),
                            params=AmclParams(min_particles=n, max_particles=n), seed=40 + i) for i, n in enumerate(sizes)])
    try:
        for m in batch.members:
            m.initialize(truth, np.diag([0.04, 0.04, 0.01]))
        pose, odom = truth, (0.0, 0.0, 0.0)
        for c in range(2):
            pose = synth.odometry_step(pose, 0.3, 0.05)
            odom = synth.odometry_step(odom, 0.3, 0.05)
            pts = synth.scan_points(synth.cast_scan(cells, 0.05, FAR_ORIGIN, pose, angles, 8.0, 0.01, seed=c), angles)
            got = batch.update([se2_from_xytheta(*odom)] * 2, [pts, pts])
            for i, m in enumerate(batch.members):
                assert got[i] is not None
                s, w = m.particles()
                r = ref.estimate(s, w)
                fam.hold(f"batch member {i}, cycle {c}", len(w), ref.errors(r, *got[i]), ref.errors(r, *orc.estimate(s, w)))
        assert batch.counter("members_fused") == 4
    finally:
        batch.close()


# ---- (d) cluster estimates ---------------------------------------------------------------------------------------------------------------
BLOB_CASES = fam.blob_cases()


@pytest.mark.parametrize("case", BLOB_CASES, ids=[c[0] for c in BLOB_CASES])
def test_cluster_estimates_against_the_exact_reference_of_their_particles(filt, case):
    """estimate_clusters and cluster_based_estimate on blobs 100 m and more apart: every entry against the exact reference over the
    particles mcl_cluster_labels assigns to it, in that cluster's own units."""
    label, n, centre, k = case
    s, w, which = fam.blobs(n, centre, k)
    filt.set_particles(s, w)
    labels = filt.cluster_labels()
    total, found = filt.estimate_clusters()
    counts = np.bincount(labels)
    assert total == int((counts > 1).sum()) >= k and len(found) == min(total, 64), (total, len(found))
    assert len({int(which[labels == cid][0]) for cid, *_ in found}) == k  # (every blob is met; a blob may split into several clusters)
    for cid, count, weight, pose, cov in found:  # a cluster lies within one blob
        assert len(set(which[labels == cid].tolist())) == 1 and count == int((labels == cid).sum())
    fam.hold_clusters(label + " estimate_clusters", s, w, labels, [(cid, pose, cov) for cid, _, _, pose, cov in found], n)
    pose, cov = filt.cluster_based_estimate()
    fam.hold_clusters(label + " cluster_based_estimate", s, w, labels, [(found[0][0], pose, cov)], n)
