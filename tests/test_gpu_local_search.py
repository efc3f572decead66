"""mcl_local_search*: a lattice of offsets about each seed scored with the sensor model on the device, its best and its moments.

The expected values come in three steps: tests/local_search_reference.py enumerates the lattice's poses in numpy, mcl_likelihoods* - the
existing call - scores them, and the reference picks the best and forms exact sums.  The search promises those bits.
  1. candidates: the lattice as the device makes it equals the reference's poses bit for bit;
  2. best: offsets, score, seed_score, plateau and pose equal the reference exactly, on all six sensor models;
  3. ties: a plateau of equal scores gives the centre, plateau == L, the seed as the mean, the uniform lattice's covariance;
  4. sums: within L 2^-52 sum|term| of the exact sums, the same bits between calls and between chunk sizes;
  5. a scenario's provable properties; 6. the filter untouched; 7. refusals; 8. reuse; 9. relocalize(refine=...).
"""
import ctypes as C
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import local_search_reference as ref
from beluga_amd import capi, synth
from beluga_amd.amcl import (Amcl, AmclBatch, AmclParams, BeamModelParam, BearingModelParam, DifferentialDriveModelParam, LandmarkMap,
                             LandmarkMapBoundaries, LandmarkModelParam, LandmarkPositionDetection, LikelihoodFieldModelParam,
                             LikelihoodFieldProbModelParam, NDTModelParam2d, OccupancyGrid, SharedMap, load_ndt_map_npz, se2_from_xytheta)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MOTION = DifferentialDriveModelParam(0.1, 0.05, 0.1, 0.05)
LF = LikelihoodFieldModelParam(max_obstacle_distance=2.0, max_laser_distance=100.0, z_hit=0.5, z_random=0.5, sigma_hit=0.2, model_unknown_space=True)
LF_PROB = LikelihoodFieldProbModelParam(max_obstacle_distance=2.0, max_laser_distance=100.0, z_hit=0.5, z_random=0.5, sigma_hit=0.2,
                                        model_unknown_space=True)
LF_NEAR = LikelihoodFieldModelParam(max_obstacle_distance=0.5, max_laser_distance=100.0, z_hit=0.5, z_random=0.5, sigma_hit=0.2, model_unknown_space=True)
BEAM = BeamModelParam(0.5, 0.05, 0.05, 0.5, 0.2, 0.1, 60.0)
SMALL = AmclParams(max_particles=64)
COV = np.diag([0.25, 0.25, 0.04])
SHAPES = [(0, 0), (1, 1), (2, 3), (6, 8)]  # L = 1, 27, 175, 2873: one lane, below a wave, no multiple of 64, several strides of a workgroup
STEP_THETA = math.pi / 360


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def demo_grid():
    """The 64 x 48 map of tests/test_gpu_search_demo.py: a border, a wall along x at row 30 with a door, one along y at column 40."""
    W, H = 64, 48
    cells = np.zeros((H, W), dtype=np.int8)
    cells[0, :] = cells[-1, :] = cells[:, 0] = cells[:, -1] = 100
    cells[30, [x for x in range(W) if x < 12 or x > 18]] = 100
    cells[:30, 40] = 100
    return OccupancyGrid(cells=cells, resolution=0.1, origin=se2_from_xytheta(-1.0, -1.0, 0.0))


SCAN = np.array([[3.0, 0.0], [0.0, 2.0], [-1.0, 0.0], [0.0, -1.0], [3.0, 1.0], [3.0, -1.0], [1.0, 2.0], [-1.0, 1.0]])


def unnormalised(x, y, theta):
    """A pose whose rotation is not normalised to the last bit."""
    return np.array([math.cos(theta) * (1.0 + 2.0 ** -51), math.sin(theta) * (1.0 + 2.0 ** -51), x, y])


def seeds_of(n):
    """Seeds about cell (10, 10) of the demo map, the first with a rotation that is not normalised."""
    rng = np.random.default_rng(17)
    rows = [unnormalised(0.05 + 0.013, 0.05 - 0.021, 0.04)]
    for _ in range(n - 1):
        rows.append(se2_from_xytheta(0.05 + rng.uniform(-0.3, 0.3), 0.05 + rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2)))
    return np.array(rows)


def expected(f, seeds, measurement, Kx, Kt, step_xy, step_theta):
    """Per seed: the reference's poses, mcl_likelihoods*' scores of them, the reference's best and plateau."""
    out = []
    for seed in seeds:
        poses = ref.lattice_poses(seed, Kx, Kt, step_xy, step_theta)
        scores = f.likelihoods(poses, measurement)
        best, plateau = ref.best_of(scores, Kx, Kt)
        out.append((poses, scores, best, plateau))
    return out


def check_hits(hits, want, seeds, Kx, Kt, what):
    assert len(hits) == len(want)
    centre = ref.local_id(Kx, Kt, 0, 0, 0)
    for h, (poses, scores, best, plateau), seed in zip(hits, want, seeds):
        i, j, k = (int(v) for v in ref.offsets_of(Kx, Kt, best))
        assert (h.di, h.dj, h.dk) == (i, j, k), what
        assert h.plateau == plateau, what
        assert bits(h.score) == bits(scores[best]) and bits(h.seed_score) == bits(scores[centre]), what
        assert np.array_equal(bits(h.pose), bits(poses[best])), what
        assert h.score >= h.seed_score
        assert np.array_equal(bits(poses[centre]), bits(seed))


def check_sums(h, scores, Kx, Kt, what):
    """Each sum within L 2^-52 sum|term| of the exact sum of the same terms: the worst case of any summation order over L terms of one
    sign pattern each rounded once (L - 1 additions and one product, each within 2^-53 relative), so no measurement stands behind it."""
    exact, magnitude = ref.exact_sums(scores, Kx, Kt)
    L = len(scores)
    for n in range(10):
        error = abs(Fraction(float(h.sums[n])) - exact[n])
        print(f"{what} sum {n}: error {float(error):.3e} bound {float(L * Fraction(1, 2 ** 52) * magnitude[n]):.3e}")
        assert error <= L * Fraction(1, 2 ** 52) * magnitude[n], (what, n)


# ---- 1. candidates ------------------------------------------------------------------------------------------------------------------------
def test_candidates_equal_the_reference_bit_for_bit():
    grid = demo_grid()
    f = Amcl(grid, MOTION, LF, SMALL, seed=1, options={"search_chunk": 64})
    seed = unnormalised(0.063, 0.029, 0.7)
    for Kx, Kt in SHAPES:
        for step_xy in (None, 0.013):
            want = ref.lattice_poses(seed, Kx, Kt, 0.25 * grid.resolution if step_xy is None else step_xy, STEP_THETA)
            poses, total = f.local_search_candidates(seed, Kx, Kt, step_xy, STEP_THETA)
            assert total == len(want) == ref.candidates(Kx, Kt)
            assert np.array_equal(bits(poses), bits(want)), (Kx, Kt)
            assert np.array_equal(bits(poses[ref.local_id(Kx, Kt, 0, 0, 0)]), bits(seed))
            for first, count in ((0, 1), (total // 2, 70), (max(total - 3, 0), 10), (total, 4), (total + 5, 4)):
                window, again = f.local_search_candidates(seed, Kx, Kt, step_xy, STEP_THETA, first=first, count=count)
                assert again == total and np.array_equal(bits(window), bits(want[first:first + count])), (Kx, Kt, first)
    f.close()


# ---- 2. best ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sensor", [LF, LF_PROB, BEAM], ids=["lf", "lf_prob", "beam"])
def test_best_equals_the_reference_on_grid_models(sensor):
    grid = demo_grid()
    f = Amcl(grid, MOTION, sensor, SMALL, seed=1)
    step_xy = 0.25 * grid.resolution
    for n in (1, 5):
        seeds = seeds_of(n)
        for Kx, Kt in SHAPES:
            want = expected(f, seeds, SCAN, Kx, Kt, step_xy, STEP_THETA)
            hits = f.local_search(seeds, SCAN, Kx, Kt, None, STEP_THETA)
            check_hits(hits, want, seeds, Kx, Kt, (n, Kx, Kt))
            info = f.last_local_search_info
            assert info["candidates_per_seed"] == ref.candidates(Kx, Kt) and info["step_xy"] == step_xy
            assert (info["seeds_per_pass"], info["passes"]) == (ref.pass_plan(n, ref.candidates(Kx, Kt), 1 << 20)[0], 1) and info["launches"] == 3
            if (Kx, Kt) == (0, 0):  # the seed itself, with mcl_likelihoods' score of it
                for h, seed, score in zip(hits, seeds, f.likelihoods(seeds, SCAN)):
                    assert np.array_equal(bits(h.pose), bits(seed)) and bits(h.score) == bits(score) == bits(h.seed_score) and h.plateau == 1
    f.close()


def test_best_equals_the_reference_on_an_ndt_map():
    ndt_map = load_ndt_map_npz(os.path.join(HERE, "golden", "turtlebot3_world_ndt.npz"))
    f = Amcl(ndt_map, MOTION, NDTModelParam2d(), SMALL, seed=1)
    rng = np.random.default_rng(3)
    pts = np.column_stack([rng.uniform(-1.5, 1.5, 40), rng.uniform(-1.5, 1.5, 40)])
    step_xy = 0.25 * ndt_map.resolution
    for n in (1, 5):
        seeds = np.array([unnormalised(-0.5, 0.3, 0.2)] + [se2_from_xytheta(*rng.uniform(-1, 1, 3)) for _ in range(n - 1)])
        for Kx, Kt in SHAPES:
            want = expected(f, seeds, pts, Kx, Kt, step_xy, STEP_THETA)
            check_hits(f.local_search(seeds, pts, Kx, Kt, None, STEP_THETA), want, seeds, Kx, Kt, ("ndt", n, Kx, Kt))
            assert f.last_local_search_info["step_xy"] == step_xy
    f.close()


LANDMARKS = [LandmarkPositionDetection((1.0, 2.0, 0.5), 0), LandmarkPositionDetection((-2.0, 1.0, 1.0), 1), LandmarkPositionDetection((3.0, -2.0, 0.7), 0),
             LandmarkPositionDetection((-1.0, -3.0, 0.2), 2)]


@pytest.mark.parametrize("kind", ["landmark", "bearing"])
def test_best_equals_the_reference_on_landmark_maps(kind):
    box = LandmarkMapBoundaries((-6.0, -6.0, 0.0), (6.0, 6.0, 2.0))
    landmark_map = LandmarkMap(box, LANDMARKS)
    sensor = (LandmarkModelParam(sigma_range=0.2, sigma_bearing=0.1, random_prob=1e-3) if kind == "landmark" else
              BearingModelParam(sigma_bearing=0.1, sensor_pose_in_robot=(0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.5)))
    f = Amcl(landmark_map, MOTION, sensor, SMALL, seed=1)
    vectors = np.array([[0.9, 1.8, 0.5], [-2.1, 0.7, 1.0], [2.8, -2.2, 0.7]])
    if kind == "bearing":
        vectors = vectors - np.array([0.0, 0.0, 0.5])
        vectors = vectors / np.linalg.norm(vectors, axis=1)[:, None]
    detections = (vectors, np.array([0, 1, 0], dtype=np.uint32))
    rng = np.random.default_rng(8)
    for n in (1, 5):
        seeds = np.array([unnormalised(0.1, 0.15, 0.05)] + [se2_from_xytheta(*rng.uniform(-0.3, 0.3, 3)) for _ in range(n - 1)])
        for Kx, Kt in SHAPES:
            want = expected(f, seeds, detections, Kx, Kt, 0.02, STEP_THETA)
            check_hits(f.local_search(seeds, detections, Kx, Kt, 0.02, STEP_THETA), want, seeds, Kx, Kt, (kind, n, Kx, Kt))
    with pytest.raises(capi.MclError) as refused:  # no cell size stands behind step_xy None
        f.local_search(seeds, detections, 1, 1, None, STEP_THETA)
    assert refused.value.status == capi.MCL_ERR_INVALID_ARGUMENT
    f.close()


# ---- 3. ties -------------------------------------------------------------------------------------------------------------------------------
TIE_SEED = se2_from_xytheta(1.05, 0.55, 0.3)  # the centre of cell (20, 15): 1.5 m from the walls below and above, 2 m from those at its sides
TIE_SCAN = np.array([[0.3, 0.0], [0.0, 0.3], [-0.3, 0.0], [0.2, -0.2]])


# (tests/test_local_search_reference_cpu.py shows on the CPU, with tests/lf_reference.py, that this seed and scan give equal scores)
def test_a_plateau_gives_the_centre_and_the_uniform_covariance():
    grid = demo_grid()
    f = Amcl(grid, MOTION, LF_NEAR, SMALL, seed=1)
    step_xy = 0.25 * grid.resolution
    for Kx, Kt in SHAPES:
        L = ref.candidates(Kx, Kt)
        scores = f.likelihoods(ref.lattice_poses(TIE_SEED, Kx, Kt, step_xy, STEP_THETA), TIE_SCAN)
        assert np.all(bits(scores) == bits(scores[0]))
        h = f.local_search(TIE_SEED[None, :], TIE_SCAN, Kx, Kt, None, STEP_THETA)[0]
        assert (h.di, h.dj, h.dk) == (0, 0, 0) and h.plateau == L and bits(h.score) == bits(scores[0]) == bits(h.seed_score)
        assert np.array_equal(bits(h.pose), bits(TIE_SEED)) and h.moments_valid
        check_sums(h, scores, Kx, Kt, ("tie", Kx, Kt))
        # the mean is the seed and the covariance the uniform lattice's, as far as sums within the bound above and the finish's own
        # operations (ref.finish_bound) allow: the exact finish of the exact sums is (0, 0, 0) and K (K + 1) / 3 step^2 on the diagonal.
        exact, magnitude = ref.exact_sums(scores, Kx, Kt)
        sum_error = [L * Fraction(1, 2 ** 52) * m / exact[0] for m in magnitude]  # per sum, relative to S0
        steps = [Fraction(step_xy), Fraction(step_xy), Fraction(STEP_THETA)]
        extent = [Kx, Kx, Kt]
        for a, coordinate in ((0, 2), (1, 3)):
            assert abs(Fraction(float(h.mean_pose[coordinate])) - Fraction(float(TIE_SEED[coordinate]))) <= \
                steps[a] * sum_error[1 + a] * 2 + Fraction(1, 2 ** 52) * abs(Fraction(float(TIE_SEED[coordinate]))), (Kx, Kt, a)
        assert abs(math.remainder(math.atan2(h.mean_pose[1], h.mean_pose[0]) - 0.3, 2 * math.pi)) <= float(steps[2] * sum_error[3] * 2) + 1e-15
        want = [ref.uniform_covariance(Kx, step_xy), ref.uniform_covariance(Kx, step_xy), ref.uniform_covariance(Kt, STEP_THETA)]
        second = {pair: 4 + n for n, pair in enumerate(ref.SECOND)}
        for a in range(3):
            for b in range(3):
                # |d(S_ab / S0 - m_a m_b)| <= e_ab + |S_ab / S0| e_0 + the means' errors times the means' reach (at most the extent)
                slot = second[(min(a, b), max(a, b))]
                scale = steps[a] * steps[b]
                allowed = scale * (sum_error[slot] + extent[a] * extent[b] * sum_error[0] + extent[a] * sum_error[1 + b] + extent[b] * sum_error[1 + a]) * 2
                allowed += ref.finish_bound(h.sums, step_xy, STEP_THETA)[1][a][b]
                assert abs(Fraction(float(h.cov[a, b])) - (want[a] if a == b else 0)) <= allowed, (Kx, Kt, a, b)
    f.close()


# ---- 4. sums --------------------------------------------------------------------------------------------------------------------------------
def test_sums_within_the_bound_and_the_same_bits_between_calls_and_chunks():
    grid = demo_grid()
    f = Amcl(grid, MOTION, LF, SMALL, seed=1)
    step_xy = 0.25 * grid.resolution
    seeds = seeds_of(5)
    for Kx, Kt in SHAPES:
        L = ref.candidates(Kx, Kt)
        want = expected(f, seeds, SCAN, Kx, Kt, step_xy, STEP_THETA)
        f.set_option("search_chunk", 1 << 20)
        first = f.local_search(seeds, SCAN, Kx, Kt, None, STEP_THETA)
        again = f.local_search(seeds, SCAN, Kx, Kt, None, STEP_THETA)
        f.set_option("search_chunk", 64)
        chunked = f.local_search(seeds, SCAN, Kx, Kt, None, STEP_THETA)
        info = f.last_local_search_info
        per_pass = {1: 64, 27: 2, 175: 1, 2873: 1}[L]
        assert info["seeds_per_pass"] == per_pass and info["passes"] == -(-5 // per_pass) and info["launches"] == 3 * info["passes"]
        check_hits(chunked, want, seeds, Kx, Kt, ("chunk 64", Kx, Kt))
        for s, (a, b, c) in enumerate(zip(first, again, chunked)):
            assert np.array_equal(bits(a.sums), bits(b.sums)) and np.array_equal(bits(a.sums), bits(c.sums)), (Kx, Kt, s)
            assert np.array_equal(bits(a.cov), bits(c.cov)) and np.array_equal(bits(a.mean_pose), bits(c.mean_pose))
            if s < 2:
                check_sums(a, want[s][1], Kx, Kt, (Kx, Kt, s))
            # the finish is the host rule's on these sums
            mean, cov, valid = np.zeros(4), np.zeros(9), C.c_int32(0)
            p = capi.LocalSearchParams(Kx, Kt, step_xy, STEP_THETA)
            dp = lambda v: v.ctypes.data_as(capi.c_double_p)
            assert capi.load().mcl_local_search_finish(dp(a.sums), C.byref(p), dp(np.ascontiguousarray(seeds[s])), dp(mean), dp(cov), C.byref(valid)) == capi.MCL_OK
            assert valid.value == 1 and a.moments_valid and np.array_equal(bits(mean), bits(a.mean_pose)) and np.array_equal(bits(cov), bits(a.cov.reshape(-1)))
    f.close()


# ---- 5. the scenario ------------------------------------------------------------------------------------------------------------------------
def test_scenario_argmax_properties():
    """The scan is expected_scan at a true pose 0.03 m, -0.02 m and 2.3 degrees off the centre of cell (10, 10) at heading 0 (a candidate
    of global_search with stride 2 and 72 headings); the seed is the best hit of global_search.  Both assertions follow from the argmax.
    The distances to the truth before and after are printed, not asserted."""
    grid = demo_grid()
    f = Amcl(grid, MOTION, LF, SMALL, seed=1)
    truth = (0.05 + 0.03, 0.05 - 0.02, math.radians(2.3))
    angles = np.linspace(-math.pi, math.pi, 90, endpoint=False)
    ranges = f.expected_scan(truth, angles, max_range=8.0)
    pts = np.column_stack([ranges * np.cos(angles), ranges * np.sin(angles)])
    seed = f.global_search(pts)[0]
    h = f.local_search(seed.pose[None, :], pts)[0]
    assert h.score >= h.seed_score and bits(h.seed_score) == bits(f.likelihoods(seed.pose[None, :], pts)[0])
    step_xy, step_theta = f.last_local_search_info["step_xy"], f.last_local_search_info["step_theta"]
    seed_theta = math.atan2(seed.pose[1], seed.pose[0])
    nearest = [int(np.clip(round((truth[0] - seed.pose[2]) / step_xy), -4, 4)), int(np.clip(round((truth[1] - seed.pose[3]) / step_xy), -4, 4)),
               int(np.clip(round(math.remainder(truth[2] - seed_theta, 2 * math.pi) / step_theta), -5, 5))]
    poses = ref.lattice_poses(seed.pose, 4, 5, step_xy, step_theta)
    assert h.score >= f.likelihoods(poses[ref.local_id(4, 5, *nearest)][None, :], pts)[0]

    def distance(pose):
        return math.hypot(pose[2] - truth[0], pose[3] - truth[1]), abs(math.remainder(math.atan2(pose[1], pose[0]) - truth[2], 2 * math.pi))

    print("distance to the truth (m, rad): seed", distance(seed.pose), "best", distance(h.pose), "mean", distance(h.mean_pose))
    f.close()


# ---- 6. the filter is untouched ---------------------------------------------------------------------------------------------------------------
CYCLE_COUNTERS = ("lf_fast_launches", "lf_patch_launches", "lf_beams_launches", "lf_far_launches", "small_tail_launches", "field_pose_rebuilds",
                  "estimate_repivots", "noise_ahead_used", "order_ahead_used", "order_ahead_missed")
TWIN_PARAMS = AmclParams(min_particles=300, max_particles=1000, update_min_d=0.0, update_min_a=0.0, resample_interval=1)
START = (0.05, 0.05, 0.0)


def snapshot(f):
    s, w = f.particles()
    counters = {}
    for name in CYCLE_COUNTERS:
        try:
            counters[name] = f.counter(name)
        except capi.MclError:
            pass
    return bits(s).tobytes(), bits(w).tobytes(), f.last_info, counters


def run_twins(asked, twin, cycles=3):
    seeds = seeds_of(3)
    assert asked.local_search(seeds, SCAN, 2, 3)
    odom = (0.0, 0.0, 0.0)
    for c in range(cycles):
        odom = synth.odometry_step(odom, 0.05, 0.02)
        a, b = asked.update(se2_from_xytheta(*odom), SCAN), twin.update(se2_from_xytheta(*odom), SCAN)
        assert (a is None) == (b is None)
        if a is not None:
            assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1])), c
        assert snapshot(asked) == snapshot(twin), c
        assert asked.local_search(seeds, SCAN, 2, 3) and asked.local_search_candidates(seeds[0], 1, 1)[1] == 27
        assert snapshot(asked) == snapshot(twin), c


def test_untouched_own_map_and_shared_map():
    grid = demo_grid()
    pair = [Amcl(grid, MOTION, LF, TWIN_PARAMS, seed=42) for _ in range(2)]
    for f in pair:
        f.initialize(START, COV)
    run_twins(pair[0], pair[1])
    shared = SharedMap(grid, LF)
    on_shared = [Amcl(grid, MOTION, LF, TWIN_PARAMS, seed=42) for _ in range(2)]
    for f in on_shared:
        f.use_map(shared)
        f.initialize(START, COV)
    run_twins(on_shared[0], on_shared[1])
    a, b = on_shared[0].local_search(seeds_of(3), SCAN, 2, 3), pair[0].local_search(seeds_of(3), SCAN, 2, 3)
    assert all(np.array_equal(bits(x.sums), bits(y.sums)) and (x.di, x.dj, x.dk) == (y.di, y.dj, y.dk) for x, y in zip(a, b))
    for f in pair + on_shared:
        f.close()
    shared.close()


def test_untouched_member_of_a_batch():
    grid = demo_grid()
    specs = [dict(grid=grid, motion=MOTION, sensor=LF, params=TWIN_PARAMS, seed=20 + k) for k in range(3)]
    fleets = [AmclBatch(specs) for _ in range(2)]
    for fleet in fleets:
        for m in fleet.members:
            m.initialize(START, COV)
    asked = fleets[0].members[1]
    lone = Amcl(grid, MOTION, LF, SMALL, seed=1)
    seeds = seeds_of(3)
    odom = (0.0, 0.0, 0.0)
    for c in range(3):
        a, b = asked.local_search(seeds, SCAN, 2, 3), lone.local_search(seeds, SCAN, 2, 3)
        assert all(np.array_equal(bits(x.sums), bits(y.sums)) and np.array_equal(bits(x.pose), bits(y.pose)) for x, y in zip(a, b))
        odom = synth.odometry_step(odom, 0.05, 0.02)
        results = [fleet.update([se2_from_xytheta(*odom)] * 3, [SCAN] * 3) for fleet in fleets]
        for x, y in zip(*results):
            assert (x is None) == (y is None)
            if x is not None:
                assert np.array_equal(bits(x[0]), bits(y[0])) and np.array_equal(bits(x[1]), bits(y[1])), c
        for x, y in zip(fleets[0].members, fleets[1].members):
            assert snapshot(x) == snapshot(y), c
        assert fleets[0].last_infos == fleets[1].last_infos
    lone.close()
    for fleet in fleets:
        fleet.close()


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------------
SENTINEL = 0x5A


def raw_local(f, seeds, pts, params, n=None, hits=True, null_seeds=False, null_points=False, null_ctx=False):
    lib = capi.load()
    seeds = np.ascontiguousarray(seeds, dtype=np.float64)
    buf = (capi.LocalHit * 8)()
    C.memset(buf, SENTINEL, C.sizeof(buf))
    info = capi.LocalSearchInfo()
    C.memset(C.byref(info), SENTINEL, C.sizeof(info))
    p = np.ascontiguousarray(pts, dtype=np.float64)
    status = lib.mcl_local_search(None if null_ctx else f._ctx, None if null_seeds else seeds.ctypes.data_as(capi.c_double_p), len(seeds) if n is None else n,
                                  None if null_points else p.ctypes.data_as(capi.c_double_p), len(p), C.byref(params) if params is not None else None,
                                  buf if hits else None, C.byref(info))
    untouched = bytes(buf) == bytes([SENTINEL]) * C.sizeof(buf) and bytes(info) == bytes([SENTINEL]) * C.sizeof(info)
    return status, untouched


def test_refusals_leave_the_outputs_as_they_were():
    grid = demo_grid()
    P = capi.LocalSearchParams
    f = Amcl(grid, MOTION, LF, SMALL, seed=1)
    seeds = seeds_of(2)
    good = P(1, 1, 0.0, STEP_THETA)
    bad = [P(33, 1, 0.0, 0.01), P(1, 65, 0.0, 0.01), P(1, 1, -0.1, 0.01), P(1, 1, 0.1, 0.0), P(1, 1, 0.1, -0.01), P(1, 1, math.inf, 0.01),
           P(1, 1, 0.1, math.inf), P(1, 1, math.nan, 0.01), P(1, 1, 0.1, math.nan), P(1, 64, 0.1, math.pi / 64), P(1, 1, 0.1, math.pi)]
    for params in bad:
        assert raw_local(f, seeds, SCAN, params) == (capi.MCL_ERR_INVALID_ARGUMENT, True), (params.half_steps_xy, params.half_steps_theta, params.step_xy, params.step_theta)
    assert raw_local(f, seeds, SCAN, P(32, 64, 0.0, 0.04), n=0) == (capi.MCL_OK, True)  # the limits themselves pass; n == 0 does nothing
    assert raw_local(f, seeds, SCAN, good, hits=False) == (capi.MCL_ERR_INVALID_ARGUMENT, True)
    assert raw_local(f, seeds, SCAN, good, null_seeds=True) == (capi.MCL_ERR_INVALID_ARGUMENT, True)
    assert raw_local(f, seeds, SCAN, good, null_points=True) == (capi.MCL_ERR_INVALID_ARGUMENT, True)
    assert raw_local(f, seeds, SCAN, good, null_ctx=True) == (capi.MCL_ERR_INVALID_ARGUMENT, True)
    assert raw_local(f, seeds, SCAN, good, n=0, null_seeds=True, hits=False) == (capi.MCL_OK, True)
    for c in range(4):
        for value in (math.nan, math.inf, -math.inf):
            broken = seeds.copy()
            broken[1, c] = value
            assert raw_local(f, broken, SCAN, good) == (capi.MCL_ERR_INVALID_ARGUMENT, True), (c, value)
    assert raw_local(f, seeds, SCAN, good)[0] == capi.MCL_OK and raw_local(f, seeds, SCAN, None)[0] == capi.MCL_OK  # NULL: the defaults
    # the landmark entries on a grid context, and the candidates' entry
    lib = capi.load()
    hits = (capi.LocalHit * 2)()
    C.memset(hits, SENTINEL, C.sizeof(hits))
    xyz, cat = np.array([[1.0, 0.0, 0.0]]), np.array([0], dtype=np.uint32)
    for fn in (lib.mcl_local_search_landmarks, lib.mcl_local_search_bearings):
        assert fn(f._ctx, seeds.ctypes.data_as(capi.c_double_p), 2, xyz.ctypes.data_as(capi.c_double_p), cat.ctypes.data_as(capi.c_u32_p), 1, C.byref(good), hits,
                  None) == capi.MCL_ERR_UNSUPPORTED
    assert bytes(hits) == bytes([SENTINEL]) * C.sizeof(hits)
    total = C.c_uint64(77)
    poses = np.full((8, 4), 99.0)
    seed = np.ascontiguousarray(seeds[0])
    candidates = lambda ctx, s, params, out, tot: lib.mcl_local_search_candidates(ctx, s, params, 0, 8, out, tot)
    dp = lambda a: a.ctypes.data_as(capi.c_double_p)
    for params in bad:
        assert candidates(f._ctx, dp(seed), C.byref(params), dp(poses), C.byref(total)) == capi.MCL_ERR_INVALID_ARGUMENT
    assert candidates(f._ctx, None, C.byref(good), dp(poses), C.byref(total)) == capi.MCL_ERR_INVALID_ARGUMENT
    assert candidates(f._ctx, dp(seed), C.byref(good), None, C.byref(total)) == capi.MCL_ERR_INVALID_ARGUMENT
    assert candidates(f._ctx, dp(seed), C.byref(good), dp(poses), None) == capi.MCL_ERR_INVALID_ARGUMENT
    assert candidates(None, dp(seed), C.byref(good), dp(poses), C.byref(total)) == capi.MCL_ERR_INVALID_ARGUMENT
    assert candidates(f._ctx, dp(np.array([1.0, 0.0, math.nan, 0.0])), C.byref(good), dp(poses), C.byref(total)) == capi.MCL_ERR_INVALID_ARGUMENT
    assert total.value == 77 and np.all(poses == 99.0)
    f.close()
    # what mcl_likelihoods refuses of the measurement: more than 4096 points on a beam context
    f = Amcl(grid, MOTION, BEAM, SMALL, seed=1)
    assert raw_local(f, seeds, np.zeros((4097, 2)), good) == (capi.MCL_ERR_INVALID_ARGUMENT, True)
    f.close()
    # no map
    f = Amcl(None, MOTION, LF, SMALL, seed=1)
    assert raw_local(f, seeds, SCAN, good) == (capi.MCL_ERR_NOT_READY, True)
    assert candidates(f._ctx, dp(seed), C.byref(good), dp(poses), C.byref(total)) == capi.MCL_ERR_NOT_READY and total.value == 77
    f.close()
    # a landmark context: step_xy 0 has no cell size behind it, and mcl_local_search is not its entry
    box = LandmarkMapBoundaries((-6.0, -6.0, 0.0), (6.0, 6.0, 2.0))
    f = Amcl(LandmarkMap(box, LANDMARKS), MOTION, LandmarkModelParam(sigma_range=0.2, sigma_bearing=0.1, random_prob=1e-3), SMALL, seed=1)
    assert raw_local(f, seeds, SCAN, P(1, 1, 0.1, 0.01)) == (capi.MCL_ERR_UNSUPPORTED, True)
    C.memset(hits, SENTINEL, C.sizeof(hits))
    assert lib.mcl_local_search_landmarks(f._ctx, dp(seeds), 2, dp(xyz), cat.ctypes.data_as(capi.c_u32_p), 1, C.byref(good), hits, None) == capi.MCL_ERR_INVALID_ARGUMENT
    assert lib.mcl_local_search_bearings(f._ctx, dp(seeds), 2, dp(xyz), cat.ctypes.data_as(capi.c_u32_p), 1, C.byref(P(1, 1, 0.1, 0.01)), hits,
                                         None) == capi.MCL_ERR_UNSUPPORTED
    assert bytes(hits) == bytes([SENTINEL]) * C.sizeof(hits)
    assert candidates(f._ctx, dp(seed), C.byref(good), dp(poses), C.byref(total)) == capi.MCL_ERR_INVALID_ARGUMENT and total.value == 77
    assert lib.mcl_local_search_landmarks(f._ctx, dp(seeds), 2, dp(xyz), cat.ctypes.data_as(capi.c_u32_p), 1, C.byref(P(1, 1, 0.1, 0.01)), hits, None) == capi.MCL_OK
    f.close()


# ---- 8. reuse -----------------------------------------------------------------------------------------------------------------------------------
def test_buffers_grow_and_a_small_call_follows():
    grid = demo_grid()
    f = Amcl(grid, MOTION, LF, SMALL, seed=1)
    step_xy = 0.25 * grid.resolution
    for n, (Kx, Kt) in ((1, (1, 1)), (7, (6, 8)), (2, (0, 0)), (3, (2, 3))):
        seeds = seeds_of(n)
        want = expected(f, seeds, SCAN, Kx, Kt, step_xy, STEP_THETA)
        check_hits(f.local_search(seeds, SCAN, Kx, Kt, None, STEP_THETA), want, seeds, Kx, Kt, ("reuse", n, Kx, Kt))
        poses, total = f.local_search_candidates(seeds[-1], Kx, Kt, None, STEP_THETA)
        assert np.array_equal(bits(poses), bits(want[-1][0]))
    f.close()


# ---- 9. relocalize(refine=...) --------------------------------------------------------------------------------------------------------------------
RELOC_PARAMS = AmclParams(min_particles=300, max_particles=1500, update_min_d=0.0, update_min_a=0.0)


def test_relocalize_with_refinement_starts_at_the_best_mean_pose():
    grid = demo_grid()
    f = Amcl(grid, MOTION, LF, RELOC_PARAMS, seed=5)
    lone = Amcl(grid, MOTION, LF, SMALL, seed=1)
    coarse = lone.global_search(SCAN, headings=36, max_results=5)
    refined = lone.local_search(np.array([h.pose for h in coarse]), SCAN)
    order = sorted(range(len(refined)), key=lambda k: -refined[k].score)  # stable
    hits = f.relocalize(SCAN, refine={}, headings=36, max_results=5)
    assert len(hits) == len(coarse)
    for h, k in zip(hits, order):
        assert np.array_equal(bits(h.pose), bits(refined[k].pose)) and np.array_equal(bits(h.sums), bits(refined[k].sums)) and bits(h.score) == bits(refined[k].score)
    assert all(a.score >= b.score for a, b in zip(hits, hits[1:]))
    best = hits[0]
    assert best.moments_valid
    estimate = f.estimate()
    pose = estimate[0]
    step_xy, step_theta = f.last_local_search_info["step_xy"], f.last_local_search_info["step_theta"]
    assert abs(pose[2] - best.mean_pose[2]) <= 4 * step_xy and abs(pose[3] - best.mean_pose[3]) <= 4 * step_xy
    assert abs(math.remainder(math.atan2(pose[1], pose[0]) - math.atan2(best.mean_pose[1], best.mean_pose[0]), 2 * math.pi)) <= 5 * step_theta
    # the covariance handed to initialize is positive definite, also with no steps at all
    assert np.all(np.linalg.eigvalsh(best.cov + np.diag([step_xy ** 2 / 12, step_xy ** 2 / 12, step_theta ** 2 / 12])) > 0)
    g = Amcl(grid, MOTION, LF, RELOC_PARAMS, seed=5)
    assert g.relocalize(SCAN, refine=dict(half_steps_xy=0, half_steps_theta=0), headings=36, max_results=5)
    with pytest.raises(ValueError):
        g.relocalize(SCAN, headings=36)
    for x in (f, g, lone):
        x.close()


def test_relocalize_without_refinement_is_what_it_was():
    """refine=None: global_search, then initialize(best pose, covariance) - a twin does exactly that by hand."""
    grid = demo_grid()
    cov = np.diag([0.01, 0.01, 0.0025])
    a, b = (Amcl(grid, MOTION, LF, RELOC_PARAMS, seed=5) for _ in range(2))
    hits = a.relocalize(SCAN, cov, headings=36, max_results=5)
    want = b.global_search(SCAN, headings=36, max_results=5)
    b.initialize([want[0].pose[2], want[0].pose[3], math.atan2(want[0].pose[1], want[0].pose[0])], cov)
    assert [(h.id, h.score) for h in hits] == [(h.id, h.score) for h in want]
    assert snapshot(a) == snapshot(b)
    assert a.relocalize(SCAN, cov, refine=None, headings=36, max_results=5) and b.relocalize(SCAN, cov, headings=36, max_results=5)
    assert snapshot(a) == snapshot(b)
    ea, eb = a.update(se2_from_xytheta(0.0, 0.0, 0.0), SCAN), b.update(se2_from_xytheta(0.0, 0.0, 0.0), SCAN)
    assert np.array_equal(bits(ea[0]), bits(eb[0])) and np.array_equal(bits(ea[1]), bits(eb[1]))
    a.close()
    b.close()
