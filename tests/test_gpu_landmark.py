"""The landmark and bearing sensor models on the GPU (landmark_kernels.hip through the C ABI) against the numpy restatement of the
reference (tests/landmark_reference.py) and the CPU oracle's cycle stages.  Tolerances as in test_gpu_parity.py: weights relative
1e-12, resampling counts and KLD cut bit-exact, ancestors except at CDF-step ties, estimates 1e-9."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from beluga_amd import capi, synth
from beluga_amd.amcl import (Amcl, AmclParams, BearingModelParam, DifferentialDriveModelParam, LandmarkBearingDetection, LandmarkMap,
                             LandmarkMapBoundaries, LandmarkModelParam, LandmarkPositionDetection, LikelihoodFieldModelParam,
                             OccupancyGrid, make_laser_scan, se2_from_xytheta)
from oracle import binding as orc

import landmark_reference as ref
from test_landmark_cpu import BEARING, BEARING_CASES, BOX, IDENTITY, LANDMARK, LANDMARK_CASES, POSE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOTION = DifferentialDriveModelParam(0.1, 0.05, 0.1, 0.05)
MOTION_T = (0.1, 0.05, 0.1, 0.05)
HASH = (0.5, 0.5, math.radians(10))
TILTED = (0.1, -0.2, 0.3, math.sqrt(1.0 - 0.14), 0.2, -0.1, 0.8)  # a unit quaternion (x, y, z, w) and an offset
L_SENSOR = LandmarkModelParam(sigma_range=0.4, sigma_bearing=0.15, random_prob=1e-3)
B_SENSOR = BearingModelParam(sigma_bearing=0.5, sensor_pose_in_robot=TILTED)


def facade_map(entries, box=BOX):
    return LandmarkMap(LandmarkMapBoundaries(*box), [LandmarkPositionDetection(p, c) for p, c in entries])


def new_filter(lmap, n, sensor, **kw):
    seed = kw.pop("seed", 11)
    return Amcl(lmap, MOTION, sensor, AmclParams(min_particles=kw.pop("min_particles", n), max_particles=n, **kw), seed=seed)


def scene(n_landmarks=40, n_categories=5, extent=20.0, seed=1):
    """Landmarks scattered over a square of `extent` metres with heights up to 2 m; categories 0 .. n - 1, plus category 100 with a
    single landmark; two landmarks are duplicates of others; category 200 has no landmark."""
    rng = np.random.Generator(np.random.PCG64(seed))
    pos = np.column_stack([rng.uniform(-extent / 2, extent / 2, (n_landmarks, 2)), rng.uniform(0.0, 2.0, n_landmarks)])
    cat = rng.integers(0, n_categories, n_landmarks).astype(np.uint32)
    pos = np.concatenate([pos, pos[:2], [[1.5, -2.5, 1.0]]])
    cat = np.concatenate([cat, cat[:2], [100]]).astype(np.uint32)
    half = extent / 2 + 2.0
    return pos, cat, ((-half, -half, 0.0), (half, half, 2.0))


def detections(k, n_categories=5, seed=0, bearing=False, missing=None):
    """k detections over the scene's categories (several per category from k = 9 on), one of them of the single-landmark category 100
    from k = 3 on.  The category without landmarks, 200: in the landmark model's cases from k = 3 on (its term is random_prob); the
    bearing model's term for it is 0.0 and makes every weight 0, so there it is asked for by `missing` only - in a case of its own
    (test_bearing_detection_of_a_category_without_landmarks_zeroes_the_weight), never where weights are compared at 1e-12."""
    rng = np.random.Generator(np.random.PCG64(seed))
    d = np.column_stack([rng.uniform(-8.0, 8.0, (k, 2)), rng.uniform(-0.5, 1.5, k)])
    if bearing:
        d = d / np.linalg.norm(d, axis=1)[:, None] * rng.uniform(0.5, 2.0, k)[:, None]  # (bearings need not be unit vectors)
    cat = rng.integers(0, n_categories, k).astype(np.uint32)
    if k >= 3:
        cat[2] = 100
        if missing if missing is not None else not bearing:
            cat[1] = 200
    return d, cat


def restated(bearing, rmap, states, det, cat, sensor):
    if bearing:
        return ref.bearing_weights(rmap, states, det, cat, sensor.sigma_bearing, sensor.sensor_pose_in_robot)
    return ref.landmark_weights(rmap, states, det, cat, sensor.sigma_range, sensor.sigma_bearing, sensor.random_prob)


def device_weights(f, bearing, states, w0, det, cat):
    f.set_particles(states, w0)
    (f.reweight_bearings if bearing else f.reweight_landmarks)((det, cat))
    return f.particles()[1]


@pytest.mark.parametrize("name", sorted(LANDMARK_CASES))
def test_reference_landmark_cases_through_the_device_kernel(name):
    entries, dets, expected, tolerance, closed = LANDMARK_CASES[name]
    f = new_filter(facade_map([]), 1, LandmarkModelParam(**LANDMARK))  # (MapUpdate: an empty map first, then the case's)
    w = device_weights(f, False, POSE, np.ones(1), [d[0] for d in dets], [d[1] for d in dets])
    assert w[0] == pytest.approx(LANDMARK["random_prob"] ** len(dets), rel=1e-14)  # (no landmark of any category)
    f.update_map(facade_map(entries))
    w = device_weights(f, False, POSE, np.ones(1), [d[0] for d in dets], [d[1] for d in dets])
    assert abs(w[0] - expected) <= tolerance
    if closed is not None:
        assert w[0] == pytest.approx(closed, rel=1e-12)
    f.close()


@pytest.mark.parametrize("name", sorted(BEARING_CASES))
def test_reference_bearing_cases_through_the_device_kernel(name):
    entries, dets, expected, tolerance, closed = BEARING_CASES[name]
    f = new_filter(facade_map([]), 1, BearingModelParam(**BEARING))
    w = device_weights(f, True, POSE, np.ones(1), [d[0] for d in dets], [d[1] for d in dets])
    assert w[0] == 0.0
    f.update_map(facade_map(entries))
    w = device_weights(f, True, POSE, np.ones(1), [d[0] for d in dets], [d[1] for d in dets])
    assert abs(w[0] - expected) <= tolerance
    assert w[0] == pytest.approx(closed, rel=1e-12, abs=0.0)
    f.close()


def _compare(bearing, n, k, sample=None):
    pos, cat, box = scene()
    sensor = B_SENSOR if bearing else L_SENSOR
    rmap = ref.LandmarkMap(pos, cat, box)
    states = synth.normal_particles(n, (0.5, -0.5, 0.0), (6.0, 6.0, 3.0), seed=n + k)
    w0 = np.random.Generator(np.random.PCG64(n)).uniform(0.5, 2.0, n)
    det, dcat = detections(k, seed=k, bearing=bearing)
    f = new_filter(LandmarkMap(LandmarkMapBoundaries(*box), (pos, cat)), n, sensor)
    got = device_weights(f, bearing, states, w0, det, dcat)
    f.close()
    idx = np.arange(n) if sample is None else np.random.Generator(np.random.PCG64(9)).choice(n, sample, replace=False)
    want, gaps = restated(bearing, rmap, states[idx], det, dcat, sensor)
    # no particle is left out: on these inputs every match is clear of its runner-up
    assert gaps.size == 0 or gaps.min() > 1e-9, f"smallest best-to-second gap {gaps.min()}"
    # ... and the comparison is one of numbers that carry the model: no weight is zero or denormal (a product of k terms of at least
    # exp(-pi^2 / (2 sigma_bearing^2)) = 2.7e-9, or of at least random_prob = 1e-3), the bearing model's differ from particle to particle,
    # and a sizeable part of the landmark model's is not swamped by random_prob
    if k:
        assert np.all(want > 1e-200) and np.all(np.isfinite(want))
        if n >= 1000:
            if bearing:
                assert len(np.unique(want)) > 0.9 * len(want) and np.mean(want > 1e-6 ** k) > 0.5
            else:
                assert np.mean(want > 1.001 * sensor.random_prob ** k) > 0.01
        if k >= 9:  # (several detections of one category: the bearing kernel's runs)
            assert np.unique(dcat, return_counts=True)[1].max() >= 2
    np.testing.assert_allclose(got[idx], w0[idx] * want, rtol=1e-12)
    if k == 0:
        assert np.array_equal(got, w0)


@pytest.mark.parametrize("bearing", [False, True], ids=["landmark", "bearing"])
@pytest.mark.parametrize("n", [1, 63, 64, 1000, 100_000])
def test_reweight_matches_the_restatement(bearing, n):
    _compare(bearing, n, 16)


@pytest.mark.parametrize("bearing", [False, True], ids=["landmark", "bearing"])
@pytest.mark.parametrize("k", [0, 1, 3, 4, 5, 9])
def test_reweight_detection_counts_around_the_blocks_of_four(bearing, k):
    _compare(bearing, 1000, k)


@pytest.mark.parametrize("bearing", [False, True], ids=["landmark", "bearing"])
def test_reweight_1m_sampled_against_the_restatement(bearing):
    _compare(bearing, 1_000_000, 16, sample=20_000)


@pytest.mark.parametrize("k", [3, 16])
def test_bearing_detection_of_a_category_without_landmarks_zeroes_the_weight(k):
    pos, cat, box = scene()
    det, dcat = detections(k, seed=k, bearing=True, missing=True)
    assert 200 in dcat and 200 not in cat
    n = 1000
    states = synth.normal_particles(n, (0.5, -0.5, 0.0), (6.0, 6.0, 3.0), seed=k)
    f = new_filter(LandmarkMap(LandmarkMapBoundaries(*box), (pos, cat)), n, B_SENSOR)
    got = device_weights(f, True, states, np.full(n, 1.5), det, dcat)
    f.close()
    want, _ = restated(True, ref.LandmarkMap(pos, cat, box), states, det, dcat, B_SENSOR)
    assert np.all(want == 0.0) and np.all(got == 0.0)


def test_tied_candidates_pick_the_first_in_map_order_on_the_device():
    det, cat = [(1.0, 0.0, 0.0)], [7]
    sensor = LandmarkModelParam(sigma_range=0.5, sigma_bearing=0.25, random_prob=1e-4)
    out = []
    for entries in ([((3.0, 0.0, 0.0), 7), ((1.0, 2.0, 0.0), 7)], [((1.0, 2.0, 0.0), 7), ((3.0, 0.0, 0.0), 7)]):
        f = new_filter(facade_map(entries), 1, sensor)
        got = device_weights(f, False, IDENTITY, np.ones(1), det, cat)[0]
        f.close()
        want, gaps = ref.landmark_weights(ref.LandmarkMap([e[0] for e in entries], [7, 7], BOX), IDENTITY, det, cat, 0.5, 0.25, 1e-4)
        assert gaps[0, 0] == 0.0
        assert got == pytest.approx(want[0], rel=1e-12)
        out.append(got)
    assert out[0] == pytest.approx(math.exp(-4.0 / 0.5) + 1e-4, rel=1e-12) and out[0] != out[1]
    # the bearing model's tie: equal dot products are equal apertures, so the pick does not show in the value; it must still be finite
    b = facade_map([((2.0, 0.0, 0.0), 7), ((0.0, 0.0, 2.0), 7)])
    f = new_filter(b, 1, BearingModelParam(sigma_bearing=0.5))
    got = device_weights(f, True, IDENTITY, np.ones(1), [(1.0, 0.0, 1.0)], [7])[0]
    f.close()
    assert got == pytest.approx(math.exp(-(math.pi / 4) ** 2 / 0.5), rel=1e-12)


def _tie_flips(got, want, w, seed, step, rows):
    """Rows of `rows` where got and want differ by more than 1e-9, all explained by a CDF step within 1e-9 of the draw."""
    cdf = np.cumsum(w / w.sum())
    diff = [j for j in rows if np.any(np.abs(got[j] - want[j]) > 1e-9)]
    for j in diff:
        r = orc.draw(seed, step, 2, int(j))
        u = float((int(r[0]) << 32 | int(r[1])) >> 11) * 2.0 ** -53
        k = np.searchsorted(cdf, u, side="left")
        near = min(abs(cdf[min(k, len(cdf) - 1)] - u), abs(cdf[max(k - 1, 0)] - u))
        assert near < 1e-9, f"slot {j}: differs from the oracle's ancestor away from a CDF step (gap {near})"
    return len(diff)


def world_detections(pos, cat, pose, count, rng, noise, bearing, sensor_pose=None):
    """`count` landmarks seen from `pose` (x, y, theta): positions in the robot frame, or bearings in the (untilted) sensor frame."""
    pick = rng.choice(len(pos), count, replace=False)
    c, s = math.cos(pose[2]), math.sin(pose[2])
    v = pos[pick] - np.array([pose[0], pose[1], 0.0])
    local = np.column_stack([c * v[:, 0] + s * v[:, 1], c * v[:, 1] - s * v[:, 0], v[:, 2]])
    if bearing:
        local = local - np.asarray(sensor_pose[4:])
        local = local / np.linalg.norm(local, axis=1)[:, None]
    return local + rng.normal(0.0, noise, local.shape), cat[pick]


@pytest.mark.parametrize("bearing", [False, True], ids=["landmark", "bearing"])
@pytest.mark.parametrize("min_p,max_p", [(20_000, 20_000), (500, 50_000)], ids=["fixed", "kld"])
def test_update_cycle_matches_the_oracle_stages(bearing, min_p, max_p, cycles=6, seed=21):
    pos, cat, box = scene()
    sensor = BearingModelParam(0.1, (0.0, 0.0, 0.0, 1.0, 0.1, 0.0, 0.5)) if bearing else L_SENSOR
    rmap = ref.LandmarkMap(pos, cat, box)
    params = AmclParams(min_particles=min_p, max_particles=max_p, alpha_slow=0.0, alpha_fast=0.0)
    gpu = Amcl(LandmarkMap(LandmarkMapBoundaries(*box), (pos, cat)), MOTION, sensor, params, seed=seed)
    truth = (-0.5, 0.3, 0.2)
    cov = np.diag([0.09, 0.09, 0.04])
    gpu.initialize(truth, cov)
    states, w = orc.init_normal(max_p, truth, cov, seed)
    g0, _ = gpu.particles()
    np.testing.assert_allclose(g0, states, rtol=1e-12, atol=1e-12)
    states = g0.copy()
    odom, pose, prev = (0.0, 0.0, 0.0), truth, None
    rng = np.random.Generator(np.random.PCG64(4))
    for c in range(cycles):
        odom = synth.odometry_step(odom, 0.3, 0.05)
        pose = synth.odometry_step(pose, 0.3, 0.05)
        ctrl = se2_from_xytheta(*odom)
        det, dcat = world_detections(pos, cat, pose, 6, rng, 0.02, bearing, sensor.sensor_pose_in_robot if bearing else None)
        gpu.force_update()
        est = gpu.update(ctrl, (det, dcat))
        assert est is not None
        sampler = orc.diffdrive_sampler(ctrl, prev if prev is not None else ctrl, MOTION_T)
        prev = ctrl
        states = orc.propagate(states, sampler, seed, c + 1)
        w = orc.normalize(w * restated(bearing, rmap, states, det, dcat, sensor)[0])[0]
        want, anc = orc.resample(states, w, min_p, max_p, 0.05, 3.0, HASH, 0.0, seed, c + 1)
        got, gw = gpu.particles()
        assert len(got) == len(want), f"cycle {c}: particle counts differ"
        assert np.all(gw == 1.0)
        assert _tie_flips(got, want, w, seed, c + 1, range(len(got))) <= 3, f"cycle {c}"
        om, oc = orc.estimate(got, np.ones(len(got)))
        np.testing.assert_allclose(est[0], om, atol=1e-9)
        np.testing.assert_allclose(est[1], oc, rtol=1e-8, atol=1e-9)
        states, w = got, np.ones(len(got))
    gpu.close()


def test_update_cycle_with_injection_draws_from_the_box():
    """The recovery filters set apart: the injected slots are the oracle's, every injected state is the restated box draw, the other
    slots hold the oracle's ancestors."""
    pos, cat, box = scene()
    rmap = ref.LandmarkMap(pos, cat, box)
    n, seed = 20_000, 21
    a_slow, a_fast = 0.001, 0.1
    gpu = Amcl(LandmarkMap(LandmarkMapBoundaries(*box), (pos, cat)), MOTION, L_SENSOR,
               AmclParams(min_particles=n, max_particles=n, alpha_slow=a_slow, alpha_fast=a_fast), seed=seed)
    truth = (-0.5, 0.3, 0.2)
    gpu.initialize(truth, np.diag([0.09, 0.09, 0.04]))
    states, w = gpu.particles()
    slow, fast = 2.0 / n, 0.5 / n
    gpu.debug_set_recovery_filters(slow, fast)
    odom, pose, prev = (0.0, 0.0, 0.0), truth, None
    rng = np.random.Generator(np.random.PCG64(4))
    injected = 0
    for c in range(3):
        odom = synth.odometry_step(odom, 0.3, 0.05)
        pose = synth.odometry_step(pose, 0.3, 0.05)
        ctrl = se2_from_xytheta(*odom)
        det, dcat = world_detections(pos, cat, pose, 6, rng, 0.02, False)
        gpu.force_update()
        est = gpu.update(ctrl, (det, dcat))
        assert est is not None
        sampler = orc.diffdrive_sampler(ctrl, prev if prev is not None else ctrl, MOTION_T)
        prev = ctrl
        states = orc.propagate(states, sampler, seed, c + 1)
        w = orc.normalize(w * restated(False, rmap, states, det, dcat, L_SENSOR)[0])[0]
        avg = w.sum() / len(w)  # ThrunRecoveryProbabilityEstimator on the normalised weights
        slow = avg if slow == 0.0 else slow + a_slow * (avg - slow)
        fast = avg if fast == 0.0 else fast + a_fast * (avg - fast)
        p = min(max(1.0 - fast / slow, 0.0), 1.0) if slow != 0.0 else 0.0
        assert gpu.last_info["random_state_probability"] == pytest.approx(p, abs=1e-12), f"cycle {c}"
        p = gpu.last_info["random_state_probability"]
        if p > 0.0:
            slow = fast = 0.0
        want, anc = orc.resample(states, w, n, n, 0.05, 3.0, HASH, p, seed, c + 1, free_xy=np.zeros((1, 2)))
        got, gw = gpu.particles()
        assert len(got) == len(want) == n and np.all(gw == 1.0)
        inj = anc == -1
        injected += int(inj.sum())
        assert _tie_flips(got, want, w, seed, c + 1, np.flatnonzero(~inj)) <= 3, f"cycle {c}"
        if inj.any():
            slots = np.flatnonzero(inj)
            np.testing.assert_allclose(got[slots], ref.box_states(rmap, seed, c + 1, slots), rtol=1e-12, atol=1e-12)
        states, w = got, np.ones(n)
    assert injected > 1000
    gpu.close()


def test_initialize_from_map_is_the_box_generator_at_step_0():
    pos, cat, box = scene()
    rmap = ref.LandmarkMap(pos, cat, box)
    f = new_filter(LandmarkMap(LandmarkMapBoundaries(*box), (pos, cat)), 50_000, B_SENSOR, seed=5)
    f.initialize_from_map()
    got, w = f.particles()
    f.close()
    assert len(got) == 50_000 and np.all(w == 1.0)
    idx = np.concatenate([np.arange(200), np.random.Generator(np.random.PCG64(1)).choice(50_000, 1800, replace=False)])
    np.testing.assert_allclose(got[idx], ref.box_states(rmap, 5, 0, idx), rtol=1e-12, atol=1e-12)
    assert got[:, 2].min() >= box[0][0] and got[:, 2].max() <= box[1][0] and got[:, 3].min() >= box[0][1] and got[:, 3].max() <= box[1][1]
    assert abs(got[:, 2].mean()) < 0.3 and got[:, 2].std() == pytest.approx(24.0 / math.sqrt(12.0), rel=0.02)
    # the implicit boundaries: the landmarks' bounding box
    g = new_filter(LandmarkMap((pos, cat)), 1000, L_SENSOR, seed=5)
    g.initialize_from_map()
    s = g.particles()[0]
    g.close()
    np.testing.assert_allclose(s[:50], ref.box_states(ref.LandmarkMap(pos, cat), 5, 0, range(50)), rtol=1e-12, atol=1e-12)


def localisation_scene():
    rng = np.random.Generator(np.random.PCG64(12))
    pos = np.column_stack([rng.uniform(-10.0, 10.0, (40, 2)), rng.uniform(0.2, 2.0, 40)])
    cat = (np.arange(40) % 5).astype(np.uint32)
    return pos, cat, ((-12.0, -12.0, 0.0), (12.0, 12.0, 2.0))


LOCALISE = {False: LandmarkModelParam(sigma_range=0.3, sigma_bearing=0.15, random_prob=1e-3),
            True: BearingModelParam(sigma_bearing=0.08, sensor_pose_in_robot=(0.0, 0.0, 0.0, 1.0, 0.1, 0.0, 0.5))}


def localisation_run(bearing, update, cycles=30):
    """The true trajectory and the detections of the global localisation test; update(control, detections, categories) per cycle."""
    pos, cat, _ = localisation_scene()
    rng = np.random.Generator(np.random.PCG64(3))
    pose, odom = (2.0, -1.5, 0.7), (0.0, 0.0, 0.0)
    for _ in range(cycles):
        pose = synth.odometry_step(pose, 0.3, 0.08)
        odom = synth.odometry_step(odom, 0.3, 0.08)
        det, dcat = world_detections(pos, cat, pose, 12, rng, 0.01 if bearing else 0.03, bearing,
                                     LOCALISE[bearing].sensor_pose_in_robot if bearing else None)
        update(se2_from_xytheta(*odom), det, dcat)
    return pose


@pytest.mark.parametrize("bearing", [False, True], ids=["landmark", "bearing"])
def test_global_localisation_from_initialize_from_map(bearing):
    """40 landmarks in 5 categories over 20 m x 20 m, 12 noisy detections a cycle along a true trajectory; from a uniform start over
    the map's box the estimate is within 0.3 m and 0.2 rad of the truth after 30 cycles."""
    pos, cat, box = localisation_scene()
    f = Amcl(LandmarkMap(LandmarkMapBoundaries(*box), (pos, cat)), MOTION, LOCALISE[bearing],
             AmclParams(min_particles=2000, max_particles=200_000), seed=0xBE1A6A)
    f.initialize_from_map()
    est = []

    def update(ctrl, det, dcat):
        f.force_update()
        e = f.update(ctrl, (det, dcat))
        if e is not None:
            est[:] = [e]

    pose = localisation_run(bearing, update)
    f.close()
    ex, ey, et = est[0][0][2], est[0][0][3], math.atan2(est[0][0][1], est[0][0][0])
    d, a = math.hypot(ex - pose[0], ey - pose[1]), abs(math.remainder(et - pose[2], 2 * math.pi))
    assert d < 0.3 and a < 0.2, (d, a)


def test_error_codes():
    lib = capi.load()
    pos, cat, box = scene()
    dp, up = capi.c_double_p, capi.c_u32_p
    f = new_filter(LandmarkMap(LandmarkMapBoundaries(*box), (pos, cat)), 100, L_SENSOR)
    b = new_filter(LandmarkMap(LandmarkMapBoundaries(*box), (pos, cat)), 100, B_SENSOR)
    det = np.ones((65, 3))
    dcat = np.zeros(65, dtype=np.uint32)
    ctrl = se2_from_xytheta(0, 0, 0)
    est, info = capi.Estimate(), capi.UpdateInfo()
    args = (det.ctypes.data_as(dp), dcat.ctypes.data_as(up))
    U, I = capi.MCL_ERR_UNSUPPORTED, capi.MCL_ERR_INVALID_ARGUMENT
    # the other kind's entries, and the scan forms
    assert lib.mcl_reweight_bearings(f._ctx, *args, 1) == U and lib.mcl_reweight_landmarks(b._ctx, *args, 1) == U
    assert lib.mcl_update_bearings(f._ctx, ctrl.ctypes.data_as(dp), *args, 1, C.byref(est), C.byref(info)) == U
    assert lib.mcl_update_landmarks(b._ctx, ctrl.ctypes.data_as(dp), *args, 1, C.byref(est), C.byref(info)) == U
    for ctx in (f._ctx, b._ctx):
        assert lib.mcl_update(ctx, ctrl.ctypes.data_as(dp), det.ctypes.data_as(dp), 1, C.byref(est), C.byref(info)) == U
        assert lib.mcl_reweight(ctx, det.ctypes.data_as(dp), 1) == U
        assert lib.mcl_update_point_cloud(ctx, ctrl.ctypes.data_as(dp), np.zeros(3, dtype=np.float32).ctypes.data_as(capi.c_float_p), 1,
                                          np.array(ref.IDENTITY_SE3).ctypes.data_as(dp), C.byref(est), C.byref(info)) == U
        assert lib.mcl_comm_attach(ctx, 0, 1, None) == U
        assert lib.mcl_comm_attach_rccl(ctx, bytes(128), 0, 1) == U
        scan = make_laser_scan(np.ones(8, dtype=np.float32), 0.0, 0.1, 0.1, 10.0)
        assert lib.mcl_update_laser_scan(ctx, ctrl.ctypes.data_as(dp), C.byref(scan), C.byref(est), C.byref(info)) == U
        field = np.zeros(4, dtype=np.float32)
        assert lib.mcl_get_likelihood_field(ctx, field.ctypes.data_as(capi.c_float_p)) == U
        assert lib.mcl_set_likelihood_field(ctx, field.ctypes.data_as(capi.c_float_p)) == U
        assert lib.mcl_set_ndt_map(ctx, None, None, None, 0, 1.0, None) == U
    grid = OccupancyGrid(cells=np.zeros((8, 8), dtype=np.int8), resolution=0.1)
    for call in (lambda: f.update_map(grid), lambda: f.update_map_async(grid)):
        with pytest.raises(capi.MclError) as e:
            call()
        assert e.value.status == U
    with pytest.raises(RuntimeError):
        f.likelihood_field_origin()
    assert not f.has_likelihood_field()
    # the cap on the detections, values that are not finite
    assert lib.mcl_reweight_landmarks(f._ctx, *args, 65) == I and lib.mcl_reweight_landmarks(f._ctx, *args, 64) == capi.MCL_OK
    bad = det.copy()
    bad[0, 1] = np.nan
    assert lib.mcl_reweight_landmarks(f._ctx, bad.ctypes.data_as(dp), dcat.ctypes.data_as(up), 2) == I
    # bad maps and parameters
    inf_pos = pos.copy()
    inf_pos[3, 2] = np.inf
    for bad_map, sensor in [(LandmarkMap(LandmarkMapBoundaries((1.0, 0.0, 0.0), (0.0, 1.0, 0.0)), (pos, cat)), None),
                            (LandmarkMap(LandmarkMapBoundaries((0.0, 0.0, 0.0), (np.nan, 1.0, 0.0)), (pos, cat)), None),
                            (LandmarkMap(LandmarkMapBoundaries(*box), (inf_pos, cat)), None),
                            (LandmarkMap([]), None),
                            (LandmarkMap((pos, cat)), LandmarkModelParam(sigma_range=0.0)),
                            (LandmarkMap((pos, cat)), LandmarkModelParam(sigma_bearing=float("inf"))),
                            (LandmarkMap((pos, cat)), LandmarkModelParam(random_prob=float("nan")))]:
        if sensor is not None:
            f._landmark_params = sensor
        with pytest.raises(capi.MclError) as e:
            f.update_map(bad_map)
        assert e.value.status == I
    for sensor in [BearingModelParam(sigma_bearing=-1.0), BearingModelParam(1.0, (0.0, 0.0, 0.0, 1.1, 0.0, 0.0, 0.0)),
                   BearingModelParam(1.0, (0.0, 0.0, 0.0, 1.0, 0.0, np.nan, 0.0)), BearingModelParam(1.0, (0.0, 0.0, 0.0, 1.0 + 1e-8, 0.0, 0.0, 0.0))]:
        b._landmark_params = sensor
        with pytest.raises(capi.MclError) as e:
            b.update_map(LandmarkMap((pos, cat)))
        assert e.value.status == I
    b._landmark_params = BearingModelParam(1.0, (0.0, 0.0, 0.0, 1.0 + 1e-10, 0.0, 0.0, 0.0))  # (unit within 1e-9)
    b.update_map(LandmarkMap((pos, cat)))
    f.close()
    b.close()
    # a landmark context without a map; a landmark map on a likelihood-field context
    cfg = capi.Config()
    lib.mcl_default_config(cfg)
    cfg.sensor_kind = capi.MCL_SENSOR_LANDMARK
    cfg.amcl.min_particles = cfg.amcl.max_particles = 10
    ctx = capi._ctx()
    assert lib.mcl_create(C.byref(cfg), C.byref(ctx)) == capi.MCL_OK
    assert lib.mcl_reweight_landmarks(ctx, *args, 1) == capi.MCL_ERR_NOT_READY
    assert lib.mcl_initialize_from_map(ctx) == capi.MCL_ERR_NOT_READY
    lib.mcl_destroy(ctx)
    g = Amcl(grid, MOTION, LikelihoodFieldModelParam(), AmclParams(min_particles=10, max_particles=10))
    assert lib.mcl_set_landmark_map(g._ctx, pos.ctypes.data_as(dp), cat.ctypes.data_as(up), len(pos), None, None) == U
    assert lib.mcl_reweight_landmarks(g._ctx, *args, 1) == U
    g.close()


def test_update_map_replaces_the_map_between_updates():
    pos, cat, box = scene()
    f = new_filter(LandmarkMap(LandmarkMapBoundaries(*box), (pos, cat)), 1000, L_SENSOR)
    states = synth.normal_particles(1000, (0.0, 0.0, 0.0), (4.0, 4.0, 3.0), seed=3)
    det, dcat = detections(8, seed=2)
    a = device_weights(f, False, states, np.ones(1000), det, dcat)
    moved = pos + np.array([1.0, -1.0, 0.0])
    f.update_map(LandmarkMap(LandmarkMapBoundaries(*box), (moved, cat)))
    b = device_weights(f, False, states, np.ones(1000), det, dcat)
    f.close()
    want, _ = restated(False, ref.LandmarkMap(moved, cat, box), states, det, dcat, L_SENSOR)
    np.testing.assert_allclose(b, want, rtol=1e-12)
    assert not np.array_equal(a, b)


def test_cpp_landmark_demo_matches_the_python_facade(tmp_path):
    lib_dir = os.path.join(ROOT, "beluga_amd", "lib")
    exe = tmp_path / "landmark_demo"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "landmark_demo.cpp"), "-L", lib_dir, "-lbeluga_mcl", f"-Wl,-rpath,{lib_dir}",
                           "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    cpp = np.array([[float(v) for v in line.split()] for line in out.stdout.strip().splitlines()])
    # the demo's scene: 12 landmarks on a circle of 5 m at heights 0.5 / 1.0 / 1.5, categories 0 .. 3; the robot stands at the origin
    entries = [((5.0 * math.cos(k * math.pi / 6), 5.0 * math.sin(k * math.pi / 6), 0.5 * (1 + k % 3)), k % 4) for k in range(12)]
    lm = LandmarkMap(LandmarkMapBoundaries((-6.0, -6.0, 0.0), (6.0, 6.0, 2.0)), [LandmarkPositionDetection(p, c) for p, c in entries])
    rows = []
    for sensor, offset in ((LandmarkModelParam(0.2, 0.1, 1e-3), 0.0), (BearingModelParam(0.1, (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.5)), 0.5)):
        py = Amcl(lm, MOTION, sensor, AmclParams(min_particles=2000, max_particles=2000), seed=7)
        py.initialize((0.0, 0.0, 0.0), np.diag([0.04, 0.04, 0.01]))
        if offset == 0.0:
            dets = [LandmarkPositionDetection(p, c) for p, c in entries[::2]]
        else:
            dets = [LandmarkBearingDetection((p[0], p[1], p[2] - offset), c) for p, c in entries[::2]]
        for _ in range(4):
            py.force_update()
            e = py.update(se2_from_xytheta(0, 0, 0), dets)
            rows.append([e[0][2], e[0][3], math.atan2(e[0][1], e[0][0])])
        py.close()
    np.testing.assert_allclose(cpp, np.array(rows), rtol=0, atol=1e-12)
